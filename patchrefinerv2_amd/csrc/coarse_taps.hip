// The coarse half of a ``cat([fine, coarse_roi])`` 3x3 convolution, computed ONCE PER FRAME at coarse resolution.
//
//   GatedConvUnit.forward        estimator/models/blocks/bi_directional_fusion_model.py:70-73   fusion_conv(cat([out, c_feat]))
//   BiDirectionalFusion.forward  ...bi_directional_fusion_model.py:424-426                      fusion_layers_1(cat([c, f]))
//   coarse_postprocess_test      estimator/models/patchrefinerplus.py:263-283                   c_feat = roi_align(feat.repeat(K), boxes, (h, w), h / P)
//
// ``c_feat`` is a bilinear zoom (roi_align with one sample per bin) of a window of the per-frame pyramid level F, and it enters the
// conv with no activation in front.  The conv is linear, so its coarse half is
//     B(p) = sum_tap [p + d_tap inside the tile] * Bil(G_tap; s(p + d_tap)),      G_tap = W_coarse[:, :, tap] . F   (1x1 GEMM at coarse resolution)
// with s(.) roi_align's sample position and Bil its clamped bilinear sample.  The reference evaluates 9 * Cin * Cout MACs per OUTPUT
// pixel of every one of the frame's 81 tiles; here the MFMA work is 9 * Cin * Cout MACs per COARSE pixel per frame.
//
// Tiles of one frame share their size, so consecutive output pixels are ``b`` = 1 / split apart in coarse coordinates on either axis,
// and U(y, x) = sum_tap Bil(G_tap; y + dy b_h, x + dx b_w) -- the sum WITHOUT the border mask -- is piecewise bilinear with knots at
// {k - b, k, k + b}, k integer.  It is therefore fixed by its values on that knot grid (``V``: 3H x 3W knots, the size of G), and a
// tile's B is a 4-tap gather from V -- the cost of the roi_align it replaces -- minus, on the tile's border pixels only, the taps the
// conv's zero padding hides (3 per edge pixel, 5 per corner, sampled from G).  Exact algebra; fp32 rounding differs (1e-7 relative).
//
// BUILD NOTE: this file is compiled with packed fp32 math OFF (PRV2_NO_PACKED_FP32_BEGIN below: a function attribute, common.h).  With
// hipcc 7.2's v_pk_fma_f32 / v_pk_add_f32 code for tap_gather_kernel the border pixels of a tile came out wrong INTERMITTENTLY --
// always the low halves of the packed pairs (channels 4k and 4k + 2) of the last quarter-wave (lanes 48-63), values off by one tap
// term -- but only inside a frame with two tile streams and a third stream busy; never in isolation, and independent of every
// s_waitcnt / s_nop added around the loads and the store (tools/probes/taps_stage_checksums.py, profiles/r04_experiments.txt).
// Scalar v_fma_f32 code is bit-stable under the same load; the kernels are HBM-bound, the flag costs nothing measurable.
//
// Frames (FR = true, the *_frames entry points): G [B, H, W, ldg] -> V [B, 3H, 3W, ldv] with grid.z = frame, and the gather takes
// boxes (frame, x1, y1, x2, y2) and reads each tile's own frame's tables (frame index clamped to [0, B)).  The single-frame entry
// points are the FR = false instances of the same kernels.
#include <cstdlib>

#include "common.h"

PRV2_NO_PACKED_FP32_BEGIN  // (common.h)

#include "coarse_taps_walk.h"  // fma4, knot_cell, roi_axis and the gather's column walk (shared with the gate kernels' epilogue)

namespace prv2 {

// weights of the rows (k - 1, k, k + 1) for the position k + o * b, o in -2 .. 2, b <= 1/2 (clamped rows replicate: roi_align's
// ``x <= 0 -> 0`` / ``lo >= size - 1 -> lo = hi = size - 1`` rules)
__device__ __forceinline__ void offset_weights(int o, float b, float (&w)[3]) {
  const float t = (float)o * b;
  if (o < 0) { w[0] = -t; w[1] = 1.0f + t; w[2] = 0.f; }
  else { w[0] = 0.f; w[1] = 1.0f - t; w[2] = t; }
}

// V[3k + a][3m + c][ch] = sum_tap Bil(G_tap; k + (a - 1 + dy) b_h, m + (c - 1 + dx) b_w).
// G: [H, W, ldg], channel = tap * C + ch at ``g_off``; thread = (coarse pixel, 4 channels): per tap the 3 x 3 neighbourhood is
// loaded once (9 loads) and serves the 9 knots of the pixel.
template <bool FR = false>
__global__ void __launch_bounds__(256) tap_knots_kernel(const float* __restrict__ G, int H, int W, int C, int ldg, float bh, float bw,
                                                        float* __restrict__ V, int ldv) {
  if constexpr (FR) {
    G += (int64_t)blockIdx.z * H * W * ldg;
    V += (int64_t)blockIdx.z * 9 * H * W * ldv;
  }
  const unsigned cg = C / 4;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)W * cg) return;
  const int m = (int)(t / cg), ch = (int)(t - (unsigned)m * cg) * 4;
  const int k = blockIdx.y;
  const int rows[3] = {max(k - 1, 0), k, min(k + 1, H - 1)};
  const int cols[3] = {max(m - 1, 0), m, min(m + 1, W - 1)};
  float4 acc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[a][c] = zero4();
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int tap = ky * 3 + kx;
      float4 g[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) g[r][q] = *reinterpret_cast<const float4*>(G + ((int64_t)rows[r] * W + cols[q]) * ldg + tap * C + ch);
      // horizontal first: hz[r][c] = sum_q wx[c][q] g[r][q]
      float4 hz[3][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float wx[3];
        offset_weights(c - 1 + kx - 1, bw, wx);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          float4 s = zero4();
          fma4(s, wx[0], g[r][0]);
          fma4(s, wx[1], g[r][1]);
          fma4(s, wx[2], g[r][2]);
          hz[r][c] = s;
        }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float wy[3];
        offset_weights(a - 1 + ky - 1, bh, wy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          fma4(acc[a][c], wy[0], hz[0][c]);
          fma4(acc[a][c], wy[1], hz[1][c]);
          fma4(acc[a][c], wy[2], hz[2][c]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(V + ((int64_t)(3 * k + a) * (3 * W) + 3 * m + c) * ldv + ch) = acc[a][c];
}

// B[k, i, j, ch] = U(ys(i), xs(j)) - (taps hidden by the zero padding at the tile border).  Thread = (column j, 4 channels) x R
// output rows: coarse_taps_walk (coarse_taps_walk.h) with a sink that stores each row to HBM.
template <int R, bool NT = false, bool FR = false>
__global__ void __launch_bounds__(256) tap_gather_kernel(const float* __restrict__ V, const float* __restrict__ G, int H, int W, int C, int ldv,
                                                         int ldg, float kbh, float kbw, const float* __restrict__ boxes, float scale, int oh,
                                                         int ow, float* __restrict__ out, int ldo, int B = 1) {
  const unsigned cg = C / 4;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (unsigned)ow * cg) return;
  const int px = (int)(t / cg), ch = (int)(t - (unsigned)px * cg) * 4;
  const int py0 = blockIdx.y * R, k = blockIdx.z;
  TapTables tt = {V, G, H, W, C, ldv, ldg, kbh, kbw};
  const float* b = tap_tile_box(tt, boxes, k, FR ? B : 0);
  const int pxs[1] = {px};
  coarse_taps_walk<R, 1>(tt, b, scale, oh, ow, pxs, ch, py0, [&](int, int, int py, const float4& acc) {
    float4* dst = reinterpret_cast<float4*>(out + (((int64_t)k * oh + py) * ow + px) * ldo + ch);
    if constexpr (NT) {
      typedef float f32x4n __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(f32x4n{acc.x, acc.y, acc.z, acc.w}, reinterpret_cast<f32x4n*>(dst));
    } else {
      *dst = acc;
    }
  });
}

}  // namespace prv2

using namespace prv2;

static int tap_knots_impl(const char* name, const float* g, int32_t B, int32_t h, int32_t w, int32_t c, int32_t ldg, float knot_bh, float knot_bw,
                          float* v, int32_t ldv, void* stream) {
  PRV2_REQUIRE(g && v, "%s: null pointer", name);
  PRV2_REQUIRE(h > 0 && w > 0 && c > 0 && c % 4 == 0 && ldg >= 9 * c && ldg % 4 == 0 && ldv >= c && ldv % 4 == 0 && aligned16(g) && aligned16(v),
               "%s: c %% 4 == 0, ldg >= 9 c, 16-byte aligned rows (c=%d ldg=%d ldv=%d)", name, c, ldg, ldv);
  PRV2_REQUIRE(knot_bh > 0.f && knot_bh <= 0.5f && knot_bw > 0.f && knot_bw <= 0.5f,
               "%s: the knot offsets (tile size / frame size per axis) must be in (0, 1/2] (got %g, %g)", name, (double)knot_bh, (double)knot_bw);
  PRV2_REQUIRE(h <= 65535 && B <= 65535, "%s: grid too large", name);
  if (B == 0) {
    const dim3 grid((unsigned)cdiv((int64_t)w * (c / 4), 256), (unsigned)h);
    hipLaunchKernelGGL(tap_knots_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, h, w, c, ldg, knot_bh, knot_bw, v, ldv);
  } else {
    const dim3 grid((unsigned)cdiv((int64_t)w * (c / 4), 256), (unsigned)h, (unsigned)B);
    hipLaunchKernelGGL(tap_knots_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, h, w, c, ldg, knot_bh, knot_bw, v, ldv);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_coarse_tap_knots(const float* g, int32_t h, int32_t w, int32_t c, int32_t ldg, float knot_bh, float knot_bw, float* v,
                                     int32_t ldv, void* stream) {
  return tap_knots_impl("coarse_tap_knots", g, 0, h, w, c, ldg, knot_bh, knot_bw, v, ldv, stream);
}

extern "C" int prv2_coarse_tap_knots_frames(const float* g, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldg, float knot_bh, float knot_bw,
                                            float* v, int32_t ldv, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "coarse_tap_knots_frames: n_frames %d < 1", n_frames);
  return tap_knots_impl("coarse_tap_knots_frames", g, n_frames, h, w, c, ldg, knot_bh, knot_bw, v, ldv, stream);
}

static int tap_gather_impl(const char* name, const float* v, const float* g, int32_t B, int32_t h, int32_t w, int32_t c, int32_t ldv, int32_t ldg,
                           float knot_bh, float knot_bw, const float* boxes, int32_t k, float spatial_scale, int32_t oh, int32_t ow, float* out,
                           int32_t ldo, void* stream) {
  PRV2_REQUIRE(v && g && boxes && out, "%s: null pointer", name);
  PRV2_REQUIRE(h > 0 && w > 0 && k > 0 && oh > 0 && ow > 0 && c > 0 && c % 4 == 0 && ldg >= 9 * c && ldg % 4 == 0 && ldv >= c && ldv % 4 == 0 &&
                   ldo >= c && ldo % 4 == 0 && aligned16(g) && aligned16(v) && aligned16(out),
               "%s: c %% 4 == 0, ldg >= 9 c, 16-byte aligned rows (c=%d ldg=%d ldv=%d ldo=%d)", name, c, ldg, ldv, ldo);
  PRV2_REQUIRE(knot_bh > 0.f && knot_bh <= 0.5f && knot_bw > 0.f && knot_bw <= 0.5f,
               "%s: the knot offsets must be in (0, 1/2] (got %g, %g)", name, (double)knot_bh, (double)knot_bw);
  static const int variant = getenv("PRV2_TAPG") ? atoi(getenv("PRV2_TAPG")) : 0;  // A/B switch: bit 0 = 8 rows per thread, bit 1 = nontemporal stores
  const int R = (variant & 1) && oh >= 32 ? 8 : 4;
  PRV2_REQUIRE(cdiv(oh, 4) <= 65535 && k <= 65535, "%s: grid too large", name);
  const dim3 grid((unsigned)cdiv((int64_t)ow * (c / 4), 256), (unsigned)cdiv(oh, R), (unsigned)k);
#define PRV2_TG(R_, NT_, FR_) hipLaunchKernelGGL((tap_gather_kernel<R_, NT_, FR_>), grid, dim3(256), 0, (hipStream_t)stream, v, g, h, w, c, ldv, ldg, knot_bh, \
                                                 knot_bw, boxes, spatial_scale, oh, ow, out, ldo, B > 0 ? B : 1)
  if (B == 0) {
    if (R == 8) { if (variant & 2) PRV2_TG(8, true, false); else PRV2_TG(8, false, false); }
    else { if (variant & 2) PRV2_TG(4, true, false); else PRV2_TG(4, false, false); }
  } else {
    if (R == 8) { if (variant & 2) PRV2_TG(8, true, true); else PRV2_TG(8, false, true); }
    else { if (variant & 2) PRV2_TG(4, true, true); else PRV2_TG(4, false, true); }
  }
#undef PRV2_TG
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_coarse_tap_gather(const float* v, const float* g, int32_t h, int32_t w, int32_t c, int32_t ldv, int32_t ldg, float knot_bh,
                                      float knot_bw, const float* boxes, int32_t k, float spatial_scale, int32_t oh, int32_t ow, float* out,
                                      int32_t ldo, void* stream) {
  return tap_gather_impl("coarse_tap_gather", v, g, 0, h, w, c, ldv, ldg, knot_bh, knot_bw, boxes, k, spatial_scale, oh, ow, out, ldo, stream);
}

extern "C" int prv2_coarse_tap_gather_frames(const float* v, const float* g, int32_t n_frames, int32_t h, int32_t w, int32_t c, int32_t ldv, int32_t ldg,
                                             float knot_bh, float knot_bw, const float* boxes, int32_t k, float spatial_scale, int32_t oh, int32_t ow,
                                             float* out, int32_t ldo, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "coarse_tap_gather_frames: n_frames %d < 1", n_frames);
  return tap_gather_impl("coarse_tap_gather_frames", v, g, n_frames, h, w, c, ldv, ldg, knot_bh, knot_bw, boxes, k, spatial_scale, oh, ow, out, ldo,
                         stream);
}

PRV2_NO_PACKED_FP32_END
