// The per-pixel code the scoring kernels share (csrc/evalgt.hip depth_metrics_kernel, csrc/ssi_eval.hip): the four-pixel load, the
// in-kernel bilinear sample of a prediction of another resolution, the reference's cleaning of a prediction value and the error terms
// of compute_errors (estimator/utils/metric.py:11-50).  One definition, so the two kernels cannot drift apart; both files are built
// with -ffp-contract=off, the fused operations are spelled out.
#pragma once

#include "common.h"

namespace prv2 {
namespace {

constexpr int kErrTerms = 10;  // sums 0 .. 9 of prv2_depth_metrics

// four pixels x0 .. x0 + 3 of a row per thread (one 16-byte load when the rows are aligned), zero behind the row's end
__device__ __forceinline__ void load4(const float* __restrict__ row, int x0, int w, int vec, float* v) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(row + x0);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = x0 + k < w ? row[x0 + k] : 0.f;
  }
}

// F.interpolate(mode='bilinear', align_corners=False) at one output coordinate, as PyTorch's kernel computes it (its compiler
// contracts a * b + c, so the fused operations are spelled out here): the source coordinate fma(scale, dst + 0.5, -0.5) clamped at 0,
// the lower index, whether there is an upper one, and the weight lambda
__device__ __forceinline__ void bilinear_src(float scale, int dst, int n_in, int& i0, int& step, float& lam) {
  float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  s = s < 0.f ? 0.f : s;
  i0 = min((int)s, n_in - 1);  // (never beyond the map, whatever the rounding of scale)
  step = i0 < n_in - 1 ? 1 : 0;
  lam = s - (float)i0;
}

// the resized prediction at output column x of an output row whose two source rows are pr0 / pr1 with the weight ly
__device__ __forceinline__ float bilinear_at(const float* __restrict__ pr0, const float* __restrict__ pr1, float ly, float scw, int x, int pw) {
  int sx0, sxs;
  float lx;
  bilinear_src(scw, x, pw, sx0, sxs, lx);
  const float hy = 1.0f - ly, hx = 1.0f - lx;
  const float top = __builtin_fmaf(hx, pr0[sx0], lx * pr0[sx0 + sxs]);
  const float bot = __builtin_fmaf(hx, pr1[sx0], lx * pr1[sx0 + sxs]);
  return __builtin_fmaf(hy, top, ly * bot);
}

// compute_metrics' cleaning of a prediction value in the reference's order: NaN -> min, clamp, inf -> max (the clamp has done it)
__device__ __forceinline__ float clean_pred(float pk, float mn, float mx) {
  pk = pk != pk ? mn : pk;
  pk = pk < mn ? mn : pk;
  pk = pk > mx ? mx : pk;
  return pk;
}

// the terms 0 .. 9 of one valid pixel: float64 from the fp32 ground truth gk and the cleaned fp32 prediction pk
__device__ __forceinline__ void error_terms(float gk, float pk, double* t) {
  const double G = (double)gk, P = (double)pk;
  const double ratio = fmax(G / P, P / G);
  const double d = G - P, err = log(P) - log(G), d2 = d * d;
  t[0] = 1.0;
  t[1] = ratio < 1.25 ? 1.0 : 0.0;
  t[2] = ratio < 1.5625 ? 1.0 : 0.0;
  t[3] = ratio < 1.953125 ? 1.0 : 0.0;
  t[4] = fabs(d) / G;
  t[5] = d2;
  t[6] = fabs(log10(G) - log10(P));
  t[7] = err * err;
  t[8] = err;
  t[9] = d2 / G;
}

static inline bool aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace
}  // namespace prv2
