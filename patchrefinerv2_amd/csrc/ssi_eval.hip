// Scale-and-shift-invariant evaluation (include/prv2.h "Scale-and-shift-invariant evaluation"): compute_scale_and_shift
// (estimator/models/losses.py:523-544) and the three modes of ScaleAndShiftInvariantLoss (:600-700) as evaluation scores of B frames,
// beside the error sums of compute_errors on the aligned prediction.
//
//   ssi_pass_kernel<false>  the fit: the normal-equation sums of three 2 x 2 systems (the values, the vertical and the horizontal
//                           stride-2 differences) from one read of gt and pred
//   ssi_fit_final_kernel    the partials summed in block order, the three systems solved on the device (det <= 0: scale = shift = 0)
//   ssi_pass_kernel<true>   the scores: reads the six coefficients from device memory; SSI L1, the gradient-matching sums with and
//                           without the alignment, the gradient-space ('inverse') sums and the error sums of the aligned prediction
//   ssi_score_final_kernel  the partials summed in block order
//
// A block owns kRows rows x kCols columns of a frame, a thread one quad of columns (float4 loads when the rows are 16-byte aligned)
// which it walks down the rows, the last three rows of its quad in registers: the row two above comes from there, the two columns to
// the right of the quad from one more 8-byte load of a line the neighbouring thread has just fetched.  A vertical pair belongs to the
// block that owns its upper row, so a block reads two rows of the block below (from the cache, they are streamed there at the same
// time).  Every term is float64 from the fp32 values; a thread's sums stay in registers, a wave reduces by shuffles, the four waves
// through LDS in wave order, the partials are added in block order: no atomics, the same bits on every call and for a frame alone or
// in a batch (the grid of a frame does not depend on the frame count).
#include <limits.h>

#include "evalgt_terms.h"

namespace prv2 {
namespace {

constexpr int kRows = 8;      // rows a block owns
constexpr int kCols = 1024;   // columns a block owns: 256 threads x one quad
constexpr int kFit = 15;      // 3 systems x (a00, a01, a11, b0, b1)
constexpr int kScore = 7;     // l1, ssi_gm v / h, gm v / h, inverse v / h
constexpr int kPart = kScore + kErrTerms;  // the larger of the two passes' partial rows (the workspace's row length)
constexpr int K = PRV2_SSI_VALUES;
static_assert(kFit <= kPart && K == 7 + kFit + kScore + 12, "layout of prv2_ssi_metrics' out");

struct SsiArgs {
  const float* gt;
  const float* pred;
  int h, w, vec;
  float mn, mx;
  int y0, y1, x0, x1;
  int ph, pw;      // LOWRES: pred is [n, ph, pw]
  float sch, scw;  // LOWRES: ph / h and pw / w (fp32 divisions)
};

// a thread's quad of one row and the two columns to its right: values, and whether each pixel is in the mask
struct Row6 {
  float g[6], p[6];
  bool m[6];
};

template <bool LOWRES>
__device__ __forceinline__ void load_row(const SsiArgs& a, const float* __restrict__ gt, const float* __restrict__ pred, int y, int x0, Row6& r) {
  const int w = a.w;
  const float* __restrict__ grow = gt + (int64_t)y * w;
  load4(grow, x0, w, a.vec, r.g);
  if (a.vec) {
    float2 t = make_float2(0.f, 0.f);
    if (x0 + 4 < w) t = *reinterpret_cast<const float2*>(grow + x0 + 4);
    r.g[4] = t.x, r.g[5] = t.y;
  } else {
    for (int k = 4; k < 6; ++k) r.g[k] = x0 + k < w ? grow[x0 + k] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int x = x0 + k;
    r.m[k] = x >= a.x0 && x < a.x1 && r.g[k] > a.mn && r.g[k] < a.mx;  // (x1 <= w; a NaN gt is not valid)
  }
  if (LOWRES) {  // only where the mask needs it: a sparse ground truth samples a sparse set
    int sy0, sys;
    float ly;
    bilinear_src(a.sch, y, a.ph, sy0, sys, ly);
    const float* __restrict__ pr0 = pred + (int64_t)sy0 * a.pw;
    const float* __restrict__ pr1 = pr0 + (int64_t)sys * a.pw;
#pragma unroll
    for (int k = 0; k < 6; ++k) r.p[k] = r.m[k] ? bilinear_at(pr0, pr1, ly, a.scw, x0 + k, a.pw) : 0.f;
  } else {
    const float* __restrict__ prow = pred + (int64_t)y * w;
    load4(prow, x0, w, a.vec, r.p);
    if (a.vec) {
      float2 t = make_float2(0.f, 0.f);
      if (x0 + 4 < w) t = *reinterpret_cast<const float2*>(prow + x0 + 4);
      r.p[4] = t.x, r.p[5] = t.y;
    } else {
      for (int k = 4; k < 6; ++k) r.p[k] = x0 + k < w ? prow[x0 + k] : 0.f;
    }
  }
}

// one masked sample (P, G) into a system's five sums
__device__ __forceinline__ void fit_add(double* s, double P, double G) {
  s[0] += P * P;
  s[1] += P;
  s[2] += 1.0;
  s[3] += P * G;
  s[4] += G;
}

// SCORE == false: acc = the kFit normal-equation sums; SCORE == true: acc = kScore sums, then the kErrTerms error sums
template <bool SCORE, bool LOWRES>
__global__ void __launch_bounds__(256) ssi_pass_kernel(SsiArgs a, const double* __restrict__ coef, double* __restrict__ part) {
  constexpr int NV = SCORE ? kScore + kErrTerms : kFit;
  __shared__ double sh[4][NV];
  const int f = blockIdx.z, h = a.h, w = a.w;
  const float* __restrict__ gt = a.gt + (int64_t)f * h * w;
  const float* __restrict__ pred = a.pred + (LOWRES ? (int64_t)f * a.ph * a.pw : (int64_t)f * h * w);
  double acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.0;
  double s = 0.0, t = 0.0, sv = 0.0, tv = 0.0, shh = 0.0, th = 0.0;
  if (SCORE) {
    const double* c = coef + (int64_t)f * K;
    s = c[0], t = c[1], sv = c[2], tv = c[3], shh = c[4], th = c[5];
  }

  const int r0 = blockIdx.y * kRows;
  const int ya = max(r0, a.y0), yb = min(min(r0 + kRows, h), a.y1);  // the rows this block owns, inside the crop
  const int yend = min(yb + 2, a.y1);                                 // and the two below them that its vertical pairs end in
  const int x0 = blockIdx.x * kCols + (int)threadIdx.x * 4;
  if (ya < yb && x0 < w && x0 + 3 >= a.x0 && x0 < a.x1) {  // a quad outside the crop's columns starts no pair
    float g0[4], p0[4], g1[4], p1[4];                       // rows y - 2 and y - 1 of the quad
    bool m0[4] = {false, false, false, false}, m1[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < 4; ++k) g0[k] = p0[k] = g1[k] = p1[k] = 0.f;
    for (int y = ya; y < yend; ++y) {
      Row6 r;
      load_row<LOWRES>(a, gt, pred, y, x0, r);
      if (y < yb) {  // the row's own pixels and the horizontal pairs that start at them
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!r.m[k]) continue;
          const double P = (double)r.p[k], G = (double)r.g[k];
          const bool pair = r.m[k + 2];
          const double P2 = (double)r.p[k + 2], G2 = (double)r.g[k + 2];
          if (!SCORE) {
            fit_add(acc, P, G);
            if (pair) fit_add(acc + 10, P - P2, G - G2);
          } else {
            const double al = s * P + t;
            const double d = al - G;
            acc[0] += fabs(d);
            if (pair) {
              const double d2 = (s * P2 + t) - G2;
              acc[2] += fabs(d - d2);
              acc[4] += fabs((P - G) - (P2 - G2));
              acc[6] += fabs((shh * (P - P2) + th) - (G - G2));
            }
            double e[kErrTerms];
            error_terms(r.g[k], clean_pred((float)al, a.mn, a.mx), e);
#pragma unroll
            for (int j = 0; j < kErrTerms; ++j) acc[kScore + j] += e[j];
          }
        }
      }
      if (y - 2 >= ya) {  // the vertical pairs that start two rows up (a row this block owns) and end here
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(m0[k] && r.m[k])) continue;
          const double P = (double)p0[k], G = (double)g0[k], P2 = (double)r.p[k], G2 = (double)r.g[k];
          if (!SCORE) {
            fit_add(acc + 5, P - P2, G - G2);
          } else {
            acc[1] += fabs(((s * P + t) - G) - ((s * P2 + t) - G2));
            acc[3] += fabs((P - G) - (P2 - G2));
            acc[5] += fabs((sv * (P - P2) + tv) - (G - G2));
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g0[k] = g1[k], p0[k] = p1[k], m0[k] = m1[k];
        g1[k] = r.g[k], p1[k] = r.p[k], m1[k] = r.m[k];
      }
    }
  }
  // wave: shuffles (fixed tree); block: the four waves' sums through LDS, added in wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double v = acc[j];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (int64_t)gridDim.x * gridDim.y;
    part[((int64_t)f * nblk + blk) * kPart + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
  }
}

// out[f]: 0..5 scale / shift of the values, the vertical and the horizontal differences, 6 N, 7..21 the normal-equation sums
__global__ void __launch_bounds__(64) ssi_fit_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk) {
  __shared__ double sums[kFit];
  const int f = blockIdx.x, j = threadIdx.x;
  if (j < kFit) {
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += part[((int64_t)f * nblk + b) * kPart + j];
    sums[j] = v;
    out[(int64_t)f * K + 7 + j] = v;
  }
  __syncthreads();
  if (j < 3) {  // compute_scale_and_shift (losses.py:537-542), the operations in its order
    const double a00 = sums[5 * j], a01 = sums[5 * j + 1], a11 = sums[5 * j + 2], b0 = sums[5 * j + 3], b1 = sums[5 * j + 4];
    const double det = a00 * a11 - a01 * a01;
    double x0 = 0.0, x1 = 0.0;
    if (det > 0.0) {  // (false for a NaN too)
      x0 = (a11 * b0 - a01 * b1) / det;
      x1 = (-a01 * b0 + a00 * b1) / det;
    }
    out[(int64_t)f * K + 2 * j] = x0;
    out[(int64_t)f * K + 2 * j + 1] = x1;
    if (j == 0) out[(int64_t)f * K + 6] = a11;
  }
}

// out[f]: 22..28 the score sums, 29..38 the error sums of the aligned prediction, 39..40 zero (no boundary map: the layout of
// prv2_depth_metrics' twelve)
__global__ void __launch_bounds__(64) ssi_score_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk) {
  const int f = blockIdx.x, j = threadIdx.x;
  if (j < kPart) {
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += part[((int64_t)f * nblk + b) * kPart + j];
    out[(int64_t)f * K + 7 + kFit + j] = v;
  } else if (j < kPart + 2) {
    out[(int64_t)f * K + 7 + kFit + j] = 0.0;
  }
}

static inline int64_t ssi_blocks(int h, int w) { return cdiv(h, kRows) * cdiv(w, kCols); }

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_ssi_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || cdiv(h, kRows) > 65535) return -1;
  return (int64_t)n * ssi_blocks(h, w) * kPart * (int64_t)sizeof(double);
}

extern "C" int prv2_ssi_metrics(const float* gt, const float* pred, int32_t n, int32_t h, int32_t w, int32_t ph, int32_t pw, float min_depth,
                                float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, double* out, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const char* name = "ssi_metrics";
  PRV2_REQUIRE(gt && pred && out, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1 && cdiv(h, kRows) <= 65535, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE(ph >= 1 && pw >= 1, "%s: bad prediction shape %d x %d", name, ph, pw);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX, "%s: %d frames of %d x %d exceed 2^31 pixels", name, n, h, w);
  PRV2_REQUIRE((int64_t)n * ph * pw < (int64_t)INT_MAX, "%s: %d predictions of %d x %d exceed 2^31 pixels", name, n, ph, pw);
  PRV2_REQUIRE(y0 >= 0 && y0 <= y1 && y1 <= h && x0 >= 0 && x0 <= x1 && x1 <= w, "%s: crop rows [%d, %d) columns [%d, %d) outside %d x %d", name,
               y0, y1, x0, x1, h, w);
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 8) && aligned(out, 8), "%s: null or misaligned workspace / out", name);
  const int64_t need = prv2_ssi_metrics_workspace_bytes(n, h, w);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_ssi_metrics_workspace_bytes)", name, (long long)workspace_bytes,
               (long long)need);
  const bool lowres = ph != h || pw != w;
  SsiArgs a;
  a.gt = gt, a.pred = pred;
  a.h = h, a.w = w;
  a.vec = w % 4 == 0 && aligned(gt, 16) && (lowres || aligned(pred, 16));
  a.mn = min_depth, a.mx = max_depth;
  a.y0 = y0, a.y1 = y1, a.x0 = x0, a.x1 = x1;
  a.ph = ph, a.pw = pw;
  a.sch = (float)ph / (float)h, a.scw = (float)pw / (float)w;
  const int nblk = (int)ssi_blocks(h, w);
  double* part = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(w, kCols), (unsigned)cdiv(h, kRows), (unsigned)n), block(256);
  const double* coef = out;
  if (lowres)
    hipLaunchKernelGGL((ssi_pass_kernel<false, true>), grid, block, 0, s, a, coef, part);
  else
    hipLaunchKernelGGL((ssi_pass_kernel<false, false>), grid, block, 0, s, a, coef, part);
  hipLaunchKernelGGL(ssi_fit_final_kernel, dim3(n), dim3(64), 0, s, (const double*)part, out, nblk);
  if (lowres)
    hipLaunchKernelGGL((ssi_pass_kernel<true, true>), grid, block, 0, s, a, coef, part);
  else
    hipLaunchKernelGGL((ssi_pass_kernel<true, false>), grid, block, 0, s, a, coef, part);
  hipLaunchKernelGGL(ssi_score_final_kernel, dim3(n), dim3(64), 0, s, (const double*)part, out, nblk);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
