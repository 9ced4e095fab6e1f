// The column walk of the coarse-tap gather (coarse_taps.hip, head of that file for the algebra): thread = (NC pixel columns of one tile,
// 4 channels), R output rows walked downwards.  Shared by tap_gather_kernel, which stores the rows to HBM, and by the epilogue of the
// 256-column gate kernels (conv3x3_gate_epi.h), which adds them to the C tile in LDS -- one text, so that the two give the same bits.
//
// Every kernel that runs the walk must be compiled with packed fp32 math OFF (BUILD NOTE in coarse_taps.hip): what counts is the KERNEL's
// setting -- the function attribute of common.h (PRV2_NO_PACKED_FP32_BEGIN) does not survive inlining into a kernel that lacks it.
// coarse_taps.hip carries the attribute; conv3x3_gate.hip / conv3x3_f6.hip get the target feature for their whole device pass (Makefile
// NO_PK_FLAGS).  tests/test_isa_hazards.py and tests/test_taps_fold_host.py assert the ISA.
#pragma once
#include "common.h"

namespace prv2 {

__device__ __forceinline__ void fma4(float4& a, float w, const float4& v) {
  a.x = fmaf(w, v.x, a.x);
  a.y = fmaf(w, v.y, a.y);
  a.z = fmaf(w, v.z, a.z);
  a.w = fmaf(w, v.w, a.w);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// the cell of the knot grid {k - b, k, k + b} (index 3k, 3k + 1, 3k + 2; n coarse samples) that holds position v, and the weight of
// its upper knot.  Below the first / above the last knot U is constant (every shifted sample is clamped there).
struct KnotCell {
  int i0, i1;
  float t;
};
__device__ __forceinline__ KnotCell knot_cell(float v, int n, float b) {
  const float kf = floorf(v), f = v - kf;
  const int k = (int)kf;
  KnotCell c;
  if (f < b) { c.i0 = 3 * k + 1; c.t = f / b; }
  else if (f < 1.0f - b) { c.i0 = 3 * k + 2; c.t = (f - b) / (1.0f - 2.0f * b); }
  else { c.i0 = 3 * k + 3; c.t = (f - (1.0f - b)) / b; }
  c.i1 = c.i0 + 1;
  if (c.i0 < 0) { c.i0 = 0; c.i1 = 0; }
  if (c.i1 > 3 * n - 1) { c.i1 = 3 * n - 1; c.i0 = min(c.i0, 3 * n - 1); }
  return c;
}

// roi_align's clamped axis sample: (lo, hi, weight of hi)
__device__ __forceinline__ void roi_axis(float v, int n, int& lo, int& hi, float& l) {
  float vv = v <= 0.f ? 0.f : v;
  lo = (int)vv;
  if (lo >= n - 1) { hi = lo = n - 1; vv = (float)lo; } else hi = lo + 1;
  l = vv - (float)lo;
}

// the tables of one frame (V [3H, 3W, ldv] knots, G [H, W, ldg] tap-major) and the knot offsets they were built for
struct TapTables {
  const float* V;
  const float* G;
  int H, W, C, ldv, ldg;
  float kbh, kbw;
};

// tile k's box (x1, y1, x2, y2) out of ``boxes``; n_frames >= 1: rows (frame, x1, y1, x2, y2), and the tables move to the tile's own
// frame (index clamped to [0, n_frames))
__device__ __forceinline__ const float* tap_tile_box(TapTables& t, const float* boxes, int k, int n_frames) {
  if (n_frames < 1) return boxes + 4 * k;
  const float* b = boxes + 5 * k;
  const int64_t f = min(max((int)b[0], 0), n_frames - 1);
  t.G += f * t.H * t.W * t.ldg;
  t.V += f * 9 * t.H * t.W * t.ldv;
  return b + 1;
}

// B[i, j, ch .. ch + 3] = U(ys(i), xs(j)) - (taps hidden by the zero padding at the tile border) of the oh x ow tile with box ``b``,
// for the columns j = px[0 .. NC) and the rows i = py0 .. min(py0 + R, oh) - 1: ``sink(r, c, py, value)`` per row r and column c.
// The x-interpolated knot rows of the previous output row are kept (consecutive rows share one knot row); the columns of one thread
// share the rows' cells, so their knot loads are issued together.
template <int R, int NC, class Sink>
__device__ __forceinline__ void coarse_taps_walk(const TapTables& tt, const float* __restrict__ b, float scale, int oh, int ow, const int (&px)[NC],
                                                 int ch, int py0, Sink&& sink) {
  const float* __restrict__ const V = tt.V;
  const float* __restrict__ const G = tt.G;
  const int H = tt.H, W = tt.W, C = tt.C, ldv = tt.ldv, ldg = tt.ldg;
  const float kbh = tt.kbh, kbw = tt.kbw;
  // torchvision roi_align_forward_kernel_impl, aligned=True (as gather.hip::roi_align_kernel)
  const float rsw = b[0] * scale - 0.5f, rsh = b[1] * scale - 0.5f;
  const float rew = b[2] * scale - 0.5f, reh = b[3] * scale - 0.5f;
  const float bin_h = (reh - rsh) / (float)oh, bin_w = (rew - rsw) / (float)ow;
  const int W3 = 3 * W;
  float x[NC];
  KnotCell cx[NC];
  bool xedge[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    x[c] = rsw + (float)px[c] * bin_w + .5f * bin_w;
    cx[c] = knot_cell(x[c], W, kbw);
    xedge[c] = px[c] == 0 || px[c] == ow - 1;
  }
  int c0 = -1, c1 = -1;  // knot rows whose x-interpolated values are in registers
  float4 h0[NC], h1[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) h0[c] = h1[c] = zero4();
  auto hrow = [&](int i, float4 (&r)[NC]) {
    float4 a[NC], e[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      a[c] = *reinterpret_cast<const float4*>(V + ((int64_t)i * W3 + cx[c].i0) * ldv + ch);
      e[c] = *reinterpret_cast<const float4*>(V + ((int64_t)i * W3 + cx[c].i1) * ldv + ch);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      r[c] = zero4();
      fma4(r[c], 1.0f - cx[c].t, a[c]);
      fma4(r[c], cx[c].t, e[c]);
    }
  };
  auto copy = [](float4 (&d)[NC], const float4 (&s)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = s[c];
  };
  auto tap_sample = [&](int tap, float yy, float xx) {  // Bil(G_tap; yy, xx)
    int yl, yh, xl, xh;
    float ly, lx;
    roi_axis(yy, H, yl, yh, ly);
    roi_axis(xx, W, xl, xh, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* g = G + tap * C + ch;
    float4 r = zero4();
    const float4 a0 = *reinterpret_cast<const float4*>(g + ((int64_t)yl * W + xl) * ldg);
    const float4 a1 = *reinterpret_cast<const float4*>(g + ((int64_t)yl * W + xh) * ldg);
    const float4 a2 = *reinterpret_cast<const float4*>(g + ((int64_t)yh * W + xl) * ldg);
    const float4 a3 = *reinterpret_cast<const float4*>(g + ((int64_t)yh * W + xh) * ldg);
    fma4(r, hy * hx, a0);
    fma4(r, hy * lx, a1);
    fma4(r, ly * hx, a2);
    fma4(r, ly * lx, a3);
    return r;
  };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int py = py0 + r;
    if (py >= oh) break;
    const float y = rsh + (float)py * bin_h + .5f * bin_h;
    const KnotCell cy = knot_cell(y, H, kbh);
    float4 lo[NC], hi[NC];
    if (cy.i0 == c0) copy(lo, h0); else if (cy.i0 == c1) copy(lo, h1); else hrow(cy.i0, lo);
    if (cy.i1 == cy.i0) copy(hi, lo); else if (cy.i1 == c1) copy(hi, h1); else if (cy.i1 == c0) copy(hi, h0); else hrow(cy.i1, hi);
    c0 = cy.i0; copy(h0, lo); c1 = cy.i1; copy(h1, hi);
    const bool top = py == 0, bot = py == oh - 1;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float4 acc = zero4();
      fma4(acc, 1.0f - cy.t, lo[c]);
      fma4(acc, cy.t, hi[c]);
      if (top || bot || xedge[c]) {  // (uniform where a wave is one pixel column and one row per step: both callers)
        const bool left = px[c] == 0, right = px[c] == ow - 1;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const bool hidden = (ky == 0 && top) || (ky == 2 && bot) || (kx == 0 && left) || (kx == 2 && right);
            if (hidden) {
              const float4 s = tap_sample(ky * 3 + kx, y + (float)(ky - 1) * kbh, x[c] + (float)(kx - 1) * kbw);
              acc.x -= s.x; acc.y -= s.y; acc.z -= s.z; acc.w -= s.w;
            }
          }
      }
      sink(r, c, py, acc);
    }
  }
}

}  // namespace prv2
