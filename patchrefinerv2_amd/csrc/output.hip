// GPU output stage (include/prv2.h "Output stage"): the pixel bytes of every file the tester writes, produced where the maps
// already are.  Exact order statistics of a masked fp32 map (radix select), colour / 16-bit / gray PNG scanlines, the
// pseudo-label uncertainty and the bilinear resize of the coarse prediction.  Every entry point takes B >= 1 frames [n, h, w],
// enqueues a fixed number of launches and never synchronises with the host; results are bit-deterministic (integer atomics
// only: their sums do not depend on arrival order).
//
// Arithmetic contract (what makes the scanlines byte-identical to metrics.colorize / tester._emit / tester._write_pl):
//   - the file is built with -ffp-contract=off (Makefile CXXFLAGS): no FMA in any expression below;
//   - fp32 normalisation is written with __fsub_rn / __fdiv_rn / __fmul_rn (IEEE, round to nearest), the pseudo-label
//     uncertainty in float64 like tester.pseudo_label_uncertainty;
//   - the colour index follows matplotlib's Colormap.__call__: xa = x * N, xa == N -> N - 1, xa < 0 -> under, xa >= N -> over,
//     NaN -> bad, else truncation; the (N + 3) x 4 byte table is the caller's ((cmap._lut * 255).astype(uint8)).
#include <limits.h>

#include "common.h"
#include "rows.h"

namespace prv2 {
namespace {

constexpr int kMaxRanks = 8;     // order statistics per call
constexpr int kPasses = 4;       // radix select: 4 digits of 8 bits, most significant first
constexpr int kBins = 256;
constexpr int kSelBlocks = 256;  // histogram blocks per frame

// ---------------------------------------------------------------------------------------------------------------
// order statistics
// ---------------------------------------------------------------------------------------------------------------
// monotone key of np.sort's order: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN (every NaN, whatever its sign, sorts last)
__device__ __forceinline__ uint32_t key_of(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// per-frame selection state in the workspace
struct SelState {
  uint32_t hist[kPasses][kMaxRanks][kBins];  // pass 0 uses row 0 only (one histogram: every rank has the empty prefix)
  uint32_t prefix[kMaxRanks];                // digits chosen so far
  uint32_t k[kMaxRanks];                     // rank inside the prefix's bucket
  int32_t rep[kMaxRanks];                    // first rank with the same prefix: the one whose histogram is built
  uint32_t count;
};

struct SelArgs {
  const float* value;
  const uint8_t* mask;  // nullable: valid = mask != 0
  const float* gate;    // nullable: valid needs !(gate < gate_thr) as well (float64 comparison)
  double gate_thr;
  float invalid_val;    // without a mask: valid = value != invalid_val
  int64_t hw;
  int32_t n_ranks;
  int64_t ranks[kMaxRanks];  // >= 0: from the smallest; < 0: count + rank (-1 = the largest); clamped to [0, count - 1]
  int32_t levels;            // > 0: ranks[r] is a sparsification level k, the rank (count - floor(count k / levels)) - 1 of each frame's own count
  int32_t out_stride;        // floats between two frames' rows of ``out``
};

__device__ __forceinline__ bool sel_valid(const SelArgs& a, int64_t i, float v) {
  bool ok = a.mask ? a.mask[i] != 0 : v != a.invalid_val;
  if (a.gate) ok = ok && !((double)a.gate[i] < a.gate_thr);
  return ok;
}

template <int PASS>
__global__ void __launch_bounds__(256) sel_hist_kernel(SelArgs a, SelState* __restrict__ st) {
  constexpr int R = PASS == 0 ? 1 : kMaxRanks;
  constexpr int shift = 24 - 8 * PASS;
  __shared__ uint32_t h[R][kBins];
  __shared__ uint32_t s_prefix[kMaxRanks];
  __shared__ int32_t s_rep[kMaxRanks];
  const int f = blockIdx.y, tid = threadIdx.x;
  SelState* s = st + f;
  for (int r = 0; r < R; ++r) h[r][tid] = 0;
  if (PASS > 0 && tid < kMaxRanks) {
    s_prefix[tid] = tid < a.n_ranks ? s->prefix[tid] : 0;
    s_rep[tid] = tid < a.n_ranks ? s->rep[tid] : -1;
  }
  __syncthreads();
  const int64_t base = (int64_t)f * a.hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.hw; i += (int64_t)gridDim.x * 256) {
    const float v = a.value[base + i];
    if (!sel_valid(a, base + i, v)) continue;
    const uint32_t key = key_of(v);
    if (PASS == 0) {
      atomicAdd(&h[0][key >> 24], 1u);
    } else {
      const uint32_t hi = key >> (shift + 8), d = (key >> shift) & 0xFFu;
#pragma unroll
      for (int r = 0; r < kMaxRanks; ++r)
        if (s_rep[r] == r && hi == s_prefix[r]) atomicAdd(&h[r][d], 1u);
    }
  }
  __syncthreads();
  // block first, then at most one global atomic per bin (integer adds: the sum does not depend on arrival order)
  for (int r = 0; r < R; ++r) {
    const uint32_t c = h[r][tid];
    if (c) atomicAdd(&s->hist[PASS][r][tid], c);
  }
}

// one block per frame: pick each rank's bucket of this pass; the last pass writes the values
template <int PASS>
__global__ void __launch_bounds__(256) sel_scan_kernel(SelArgs a, SelState* __restrict__ st, int64_t* __restrict__ counts,
                                                       float* __restrict__ out) {
  __shared__ uint32_t h[kMaxRanks][kBins];
  const int f = blockIdx.x, tid = threadIdx.x;
  SelState* s = st + f;
  const int R = PASS == 0 ? 1 : a.n_ranks;
  for (int r = 0; r < R; ++r) h[r][tid] = s->hist[PASS][r][tid];
  __syncthreads();
  __shared__ uint32_t s_prefix[kMaxRanks];
  const int r = tid;  // lanes 0 .. n_ranks - 1 each follow one rank
  uint32_t prefix = 0, k = 0, count = 0;
  if (r < a.n_ranks || r == 0) {
    if (PASS == 0) {
      for (int b = 0; b < kBins; ++b) count += h[0][b];
      if (r == 0) {
        s->count = count;
        counts[f] = (int64_t)count;
      }
      int64_t want = a.ranks[r] < 0 ? (int64_t)count + a.ranks[r] : a.ranks[r];
      if (a.levels > 0) want = (int64_t)count - ((int64_t)count * a.ranks[r]) / a.levels - 1;
      if (want > (int64_t)count - 1) want = (int64_t)count - 1;
      if (want < 0) want = 0;
      k = (uint32_t)want;
    } else {
      count = s->count;
      prefix = s->prefix[r];
      k = s->k[r];
    }
  }
  if (r < a.n_ranks) {
    const uint32_t* hr = h[PASS == 0 ? 0 : s->rep[r]];
    uint32_t cum = 0;
    int b = 0;
    if (count > 0) {
      for (; b < kBins - 1; ++b) {
        if (k < cum + hr[b]) break;
        cum += hr[b];
      }
    }
    prefix = (prefix << 8) | (uint32_t)b;
    k -= cum;
    if (PASS == kPasses - 1) {
      out[(int64_t)f * a.out_stride + r] = count > 0 ? value_of(prefix) : __uint_as_float(0x7FC00000u);
    } else {
      s->prefix[r] = prefix;
      s->k[r] = k;
      s_prefix[r] = prefix;
    }
  }
  __syncthreads();
  if (PASS < kPasses - 1 && r < a.n_ranks) {
    int rep = r;
    for (int q = r - 1; q >= 0; --q)
      if (s_prefix[q] == prefix) rep = q;
    s->rep[r] = rep;
  }
}

__global__ void __launch_bounds__(256) sel_clear_kernel(SelState* __restrict__ st) {
  uint32_t* p = (uint32_t*)(st + blockIdx.y);
  constexpr int words = (int)(sizeof(SelState) / 4);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) p[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------------
// PNG scanlines (rows.h: rows_kernel and its launch): the per-pixel functions
// ---------------------------------------------------------------------------------------------------------------
// matplotlib's index rule on x already multiplied by N; T = float (fp32 maps) or double (the float64 uncertainty)
template <typename T>
__device__ __forceinline__ int color_index(T xa, int ncolors) {
  if (xa != xa) return ncolors + 2;  // bad
  if (xa == (T)ncolors) xa = (T)(ncolors - 1);
  if (xa < (T)0) return ncolors;     // under
  if (xa >= (T)ncolors) return ncolors + 1;  // over
  return (int)xa;
}

struct ColorOp {
  static constexpr int bpp = 3;
  static constexpr bool lut = true;
  const float* value;
  const uint8_t* invalid;  // nullable
  const float* norm;       // [n][2] vmin, vmax
  float invalid_val;
  uint32_t background;     // r | g << 8 | b << 16
  int32_t ncolors;
  __device__ __forceinline__ uint32_t pixel(int f, int64_t i, const uint32_t* table) const {
    const float v = value[i];
    if (invalid ? invalid[i] != 0 : v == invalid_val) return background;
    const float vmin = norm[2 * f], vmax = norm[2 * f + 1];
    const float x = vmin != vmax ? __fdiv_rn(__fsub_rn(v, vmin), __fsub_rn(vmax, vmin)) : __fmul_rn(v, 0.0f);
    return table[color_index<float>(__fmul_rn(x, (float)ncolors), ncolors)];
  }
};

struct Quant16Op {
  static constexpr int bpp = 2;
  static constexpr bool lut = false;
  const float* value;
  float scale;
  __device__ __forceinline__ uint32_t pixel(int, int64_t i, const uint32_t*) const {
    const float p = __fmul_rn(value[i], scale);
    // truncation inside [0, 65536); saturation outside, NaN -> 0 (numpy's cast is platform-defined there)
    const uint32_t u = !(p > 0.0f) ? 0u : p >= 65535.0f ? 65535u : (uint32_t)p;
    return (u >> 8) | ((u & 0xFFu) << 8);  // big-endian
  }
};

// tester.pseudo_label_uncertainty in float64: prm = [n][5] lo, hi (of the whole map), thr (count_thr * n_tiles), umin, umax (of u)
struct PlBase {
  const float* unc;
  const float* cnt;
  const double* prm;
  __device__ __forceinline__ double u(int f, int64_t i) const {
    const double lo = prm[5 * f], hi = prm[5 * f + 1], thr = prm[5 * f + 2];
    double r = hi > lo ? ((double)unc[i] - lo) / (hi - lo) : 0.0;
    if ((double)cnt[i] < thr) r = 1.0;
    return r;
  }
};
struct PlQuantOp : PlBase {
  static constexpr int bpp = 2;
  static constexpr bool lut = false;
  __device__ __forceinline__ uint32_t pixel(int f, int64_t i, const uint32_t*) const {
    const double q = floor(u(f, i) * 256.0);  // np.clip(np.floor(u * 256), 0, 65535).astype(uint16)
    const uint32_t v = !(q > 0.0) ? 0u : q >= 65535.0 ? 65535u : (uint32_t)q;
    return (v >> 8) | ((v & 0xFFu) << 8);
  }
};
struct PlColorOp : PlBase {
  static constexpr int bpp = 3;
  static constexpr bool lut = true;
  int32_t ncolors;
  __device__ __forceinline__ uint32_t pixel(int f, int64_t i, const uint32_t* table) const {
    const double umin = prm[5 * f + 3], umax = prm[5 * f + 4], v = u(f, i);
    const double x = umin != umax ? (v - umin) / (umax - umin) : v * 0.0;
    return table[color_index<double>(x * (double)ncolors, ncolors)];
  }
};

struct MaskOp {
  static constexpr int bpp = 1;
  static constexpr bool lut = false;
  const uint8_t* mask;
  __device__ __forceinline__ uint32_t pixel(int, int64_t i, const uint32_t*) const { return mask[i] ? 255u : 0u; }
};

// F.interpolate(mode='bilinear', align_corners=False) of [n, ph, pw] -> [n, oh, ow] (ATen area_pixel_compute_source_index /
// guard_index_and_lambda: src = scale (dst + 0.5) - 0.5 clamped at 0, scale = float(in) / out; identity when the sizes agree).
// The source coordinate and the two-tap sums are evaluated with the fused multiply-adds torch's vectorised CPU kernel contracts
// them to (src = fma(scale, dst + 0.5, -0.5); t = fma(w0, a, w1 * b), x first): the two-rounding form of src alone moves a
// weight by an ulp of the coordinate, 1e-4 of a depth step.
struct LinTap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ LinTap lin_tap(int dst, float scale, int n_in, int n_out) {
  LinTap t;
  if (n_in == n_out) {
    t.i0 = t.i1 = dst;
    t.l0 = 1.0f;
    t.l1 = 0.0f;
    return t;
  }
  float src = fmaf(scale, __fadd_rn((float)dst, 0.5f), -0.5f);
  if (src < 0.0f) src = 0.0f;
  int i0 = (int)floorf(src);
  if (i0 > n_in - 1) i0 = n_in - 1;
  float l1 = __fsub_rn(src, (float)i0);
  l1 = fminf(fmaxf(l1, 0.0f), 1.0f);
  t.i0 = i0;
  t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  t.l1 = l1;
  t.l0 = __fsub_rn(1.0f, l1);
  return t;
}

__global__ void __launch_bounds__(256) upsample_map_kernel(const float* __restrict__ x, int n, int ph, int pw, float* __restrict__ y, int oh,
                                                           int ow, float sh, float sw) {
  const int64_t total = (int64_t)n * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % ow);
    const int64_t t = i / ow;
    const int oy = (int)(t % oh), f = (int)(t / oh);
    const LinTap ty = lin_tap(oy, sh, ph, oh), tx = lin_tap(ox, sw, pw, ow);
    const float* p = x + (int64_t)f * ph * pw;
    const float a = p[(int64_t)ty.i0 * pw + tx.i0], b = p[(int64_t)ty.i0 * pw + tx.i1];
    const float c = p[(int64_t)ty.i1 * pw + tx.i0], d = p[(int64_t)ty.i1 * pw + tx.i1];
    const float top = fmaf(tx.l0, a, __fmul_rn(tx.l1, b));
    const float bot = fmaf(tx.l0, c, __fmul_rn(tx.l1, d));
    y[i] = fmaf(ty.l0, top, __fmul_rn(ty.l1, bot));
  }
}

static int check_lut(const char* name, const void* lut, int ncolors) {
  PRV2_REQUIRE(lut != nullptr, "%s: null pointer (lut)", name);
  PRV2_REQUIRE(((uintptr_t)lut & 3) == 0, "%s: the colour table must be 4-byte aligned", name);
  PRV2_REQUIRE(ncolors >= 1 && ncolors + 3 <= kMaxColors, "%s: %d colours out of range [1, %d]", name, ncolors, kMaxColors - 3);
  return 0;
}

// the launches of one selection: a clear, then per digit a histogram and a scan (a count-only call stops after the first pair: still a
// fixed launch count per argument set)
static void launch_select(const SelArgs& a, int n, int64_t* counts, float* out, void* workspace, hipStream_t s) {
  SelState* st = (SelState*)workspace;
  const int blocks = (int)(cdiv(a.hw, 256) < kSelBlocks ? cdiv(a.hw, 256) : kSelBlocks);
  const dim3 grid(blocks, n);
  hipLaunchKernelGGL(sel_clear_kernel, dim3(8, n), dim3(256), 0, s, st);
  hipLaunchKernelGGL(sel_hist_kernel<0>, grid, dim3(256), 0, s, a, st);
  hipLaunchKernelGGL(sel_scan_kernel<0>, dim3(n), dim3(256), 0, s, a, st, counts, out);
  if (a.n_ranks > 0) {
    hipLaunchKernelGGL(sel_hist_kernel<1>, grid, dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(sel_scan_kernel<1>, dim3(n), dim3(256), 0, s, a, st, counts, out);
    hipLaunchKernelGGL(sel_hist_kernel<2>, grid, dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(sel_scan_kernel<2>, dim3(n), dim3(256), 0, s, a, st, counts, out);
    hipLaunchKernelGGL(sel_hist_kernel<3>, grid, dim3(256), 0, s, a, st);
    hipLaunchKernelGGL(sel_scan_kernel<3>, dim3(n), dim3(256), 0, s, a, st, counts, out);
  }
}

}  // namespace

// The same selection for csrc/sparsify.hip (declared there): the ranks follow each frame's own count, rank r of a frame with ``count``
// valid pixels is the n_k-th smallest value, n_k = count - floor(count k / levels), k = k0 + r -- the threshold of sparsification level
// k.  ``mask`` is required; the arguments are the caller's to check (n frames of hw pixels, n_ranks in [1, 8], a workspace of
// prv2_output_workspace_bytes(n)).  out[f * out_stride + r]; counts as prv2_order_stats.
void order_stats_levels(const float* value, const uint8_t* mask, int n, int64_t hw, int levels, int k0, int n_ranks, int64_t* counts,
                        float* out, int out_stride, void* workspace, hipStream_t s) {
  SelArgs a{};
  a.value = value;
  a.mask = mask;
  a.hw = hw;
  a.n_ranks = n_ranks < kMaxRanks ? n_ranks : kMaxRanks;
  for (int r = 0; r < a.n_ranks; ++r) a.ranks[r] = k0 + r;
  a.levels = levels;
  a.out_stride = out_stride;
  launch_select(a, n, counts, out, workspace, s);
}

}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_output_workspace_bytes(int32_t n) {
  if (n < 1 || n > 65535) return -1;
  return (int64_t)n * (int64_t)sizeof(SelState);
}

extern "C" int64_t prv2_rows_bytes(int32_t h, int32_t w, int32_t bpp) {
  if (h < 1 || w < 1 || bpp < 1 || bpp > 4) return -1;
  return rows_bytes(h, w, bpp);
}

extern "C" int prv2_order_stats(const float* value, const uint8_t* mask, float invalid_val, const float* gate, double gate_thr, int32_t n,
                                int32_t h, int32_t w, const int64_t* ranks_host, int32_t n_ranks, int64_t* counts, float* out,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "order_stats";
  PRV2_REQUIRE(value && counts, "%s: null pointer", name);
  PRV2_REQUIRE(n_ranks >= 0 && n_ranks <= kMaxRanks, "%s: %d ranks out of range [0, %d]", name, n_ranks, kMaxRanks);
  PRV2_REQUIRE(n_ranks == 0 || (ranks_host && out), "%s: null pointer (ranks / out)", name);
  if (check_map(name, n, h, w)) return 1;
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  PRV2_REQUIRE(workspace_bytes >= prv2_output_workspace_bytes(n), "%s: workspace of %lld bytes < %lld (prv2_output_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)prv2_output_workspace_bytes(n));
  PRV2_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
  SelArgs a{};
  a.value = value;
  a.mask = mask;
  a.gate = gate;
  a.gate_thr = gate_thr;
  a.invalid_val = invalid_val;
  a.hw = (int64_t)h * w;
  a.n_ranks = n_ranks;
  for (int r = 0; r < n_ranks; ++r) a.ranks[r] = ranks_host[r];
  a.out_stride = n_ranks;
  launch_select(a, n, counts, out, workspace, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_colorize_rows(const float* value, const uint8_t* invalid_mask, float invalid_val, int32_t n, int32_t h, int32_t w,
                                  const float* norm, const uint8_t* lut, int32_t ncolors, uint32_t background_rgb, uint8_t* rows,
                                  int64_t rows_fstride, void* stream) {
  const char* name = "colorize_rows";
  PRV2_REQUIRE(value && norm, "%s: null pointer", name);
  if (check_map(name, n, h, w) || check_lut(name, lut, ncolors) || check_rows(name, rows, rows_fstride, n, h, w, 3)) return 1;
  ColorOp op{value, invalid_mask, norm, invalid_val, background_rgb & 0xFFFFFFu, ncolors};
  launch_rows(op, lut, ncolors + 3, n, h, w, rows, rows_fstride, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_quantize16_rows(const float* value, int32_t n, int32_t h, int32_t w, float scale, uint8_t* rows, int64_t rows_fstride,
                                    void* stream) {
  const char* name = "quantize16_rows";
  PRV2_REQUIRE(value != nullptr, "%s: null pointer", name);
  if (check_map(name, n, h, w) || check_rows(name, rows, rows_fstride, n, h, w, 2)) return 1;
  Quant16Op op{value, scale};
  launch_rows(op, nullptr, 0, n, h, w, rows, rows_fstride, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_pl_uncertainty_rows(const float* uncertainty, const float* count_map, int32_t n, int32_t h, int32_t w, const double* params,
                                        const uint8_t* lut, int32_t ncolors, uint8_t* rows16, int64_t rows16_fstride, uint8_t* rows_rgb,
                                        int64_t rows_rgb_fstride, void* stream) {
  const char* name = "pl_uncertainty_rows";
  PRV2_REQUIRE(uncertainty && count_map && params, "%s: null pointer", name);
  if (check_map(name, n, h, w) || check_lut(name, lut, ncolors) || check_rows(name, rows16, rows16_fstride, n, h, w, 2) ||
      check_rows(name, rows_rgb, rows_rgb_fstride, n, h, w, 3))
    return 1;
  PlQuantOp q;
  q.unc = uncertainty, q.cnt = count_map, q.prm = params;
  PlColorOp c;
  c.unc = uncertainty, c.cnt = count_map, c.prm = params, c.ncolors = ncolors;
  launch_rows(q, nullptr, 0, n, h, w, rows16, rows16_fstride, (hipStream_t)stream);
  launch_rows(c, lut, ncolors + 3, n, h, w, rows_rgb, rows_rgb_fstride, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_mask_rows(const uint8_t* mask, int32_t n, int32_t h, int32_t w, uint8_t* rows, int64_t rows_fstride, void* stream) {
  const char* name = "mask_rows";
  PRV2_REQUIRE(mask != nullptr, "%s: null pointer", name);
  if (check_map(name, n, h, w) || check_rows(name, rows, rows_fstride, n, h, w, 1)) return 1;
  MaskOp op{mask};
  launch_rows(op, nullptr, 0, n, h, w, rows, rows_fstride, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_upsample_bilinear_map(const float* x, int32_t n, int32_t ph, int32_t pw, float* y, int32_t oh, int32_t ow, void* stream) {
  const char* name = "upsample_bilinear_map";
  PRV2_REQUIRE(x && y, "%s: null pointer", name);
  if (check_map(name, n, ph, pw) || check_map(name, n, oh, ow)) return 1;
  const float sh = (float)ph / (float)oh, sw = (float)pw / (float)ow;
  const int64_t total = (int64_t)n * oh * ow;
  hipLaunchKernelGGL(upsample_map_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, x, n, ph, pw, y, oh, ow, sh, sw);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
