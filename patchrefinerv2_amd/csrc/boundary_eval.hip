// Scale-invariant boundary F1 evaluation (include/prv2.h "Boundary F1 evaluation"): the occluding-boundary counts behind the boundary
// F1 of Depth Pro (Bochkovskii et al., 2024) for B frames.  A pair of neighbouring valid pixels (a, b) is a boundary of a depth map at
// the ratio t when a > t * b (direction L / T: the left / top pixel is farther) or b > t * a (R / B); per ratio and direction the
// pairs flagged in the prediction and the ground truth (tp), in the prediction (np) and in the ground truth (ng) are counted.
//
//   boundary_pass_kernel   one read of gt and pred -> per block 2 + 12 T integer counts (n_h, n_v, then [T][L, T, R, B][tp, np, ng])
//   boundary_final_kernel  the per-block rows added in block order, written as float64
//
// The structure is csrc/ssi_eval.hip's: a block owns kRows rows x kCols columns of a frame, a thread one quad of columns which it
// walks down the rows with the previous row in registers; the one column to the right of the quad comes from one more load of a line
// the neighbouring thread has just fetched.  A vertical pair belongs to the block that owns its upper row.
//
// How the 12 T flags of a pair are counted: per-lane registers.  A thread starts at most 4 kRows horizontal and 4 kRows vertical pairs,
// so every count of a thread fits a byte: the four directions of one (ratio, tp / np / ng) share one 32-bit register, 3 T registers in
// all, and a pair adds its flags with three packed additions per ratio.  A pair that is no boundary at the smallest ratio in either
// map (nearly all of them, in a real depth map) is recognised by one test and skips the ratios; this needs no order among the
// thresholds (fl(t b) is monotone in t for b >= 0; with a negative min_depth the test is left out), unlike a classification by "how
// many ratios are exceeded".  The registers are unpacked once per block into an LDS table by integer additions (which commute: the
// order in which lanes arrive changes nothing), the block's row goes out as 64-bit integers with plain stores, no global atomics: the
// same bits on every call and for a frame alone or in a batch (the grid of a frame does not depend on the frame count).
#include <limits.h>
#include <math.h>

#include "evalgt_terms.h"

namespace prv2 {
namespace {

constexpr int kRows = 8;     // rows a block owns
constexpr int kCols = 1024;  // columns a block owns: 256 threads x one quad
constexpr int kMaxT = PRV2_BOUNDARY_MAX_THRESHOLDS;
constexpr int kPart = PRV2_BOUNDARY_VALUES(kMaxT);  // a block's row in the workspace (its length does not depend on T)
static_assert(4 * kRows < 256, "a thread's count of one direction must fit the byte it is packed into");
static_assert(kPart == 2 + 12 * kMaxT && kPart <= 256, "one thread per value in the final kernel");

struct BoundaryArgs {
  const float* gt;
  const float* pred;
  int h, w, vec;
  float mn, mx;
  int y0, y1, x0, x1;
  int ph, pw;      // LOWRES: pred is [n, ph, pw]
  float sch, scw;  // LOWRES: ph / h and pw / w (fp32 divisions)
  int nt;          // T
  int skip;        // min_depth >= 0: every compared value is >= 0, so fl(t b) is monotone in t and the test at tmin decides
  float tmin;      // the smallest threshold
  float t[kMaxT];
};

// a thread's quad of one row and the column to its right: ground truth, cleaned prediction, and whether each pixel is in the mask
struct Row5 {
  float g[5], p[5];
  bool m[5];
};

template <bool LOWRES>
__device__ __forceinline__ void load_row(const BoundaryArgs& a, const float* __restrict__ gt, const float* __restrict__ pred, int y, int x0,
                                         Row5& r) {
  const int w = a.w;
  const float* __restrict__ grow = gt + (int64_t)y * w;
  load4(grow, x0, w, a.vec, r.g);
  r.g[4] = x0 + 4 < w ? grow[x0 + 4] : 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int x = x0 + k;
    r.m[k] = x >= a.x0 && x < a.x1 && r.g[k] > a.mn && r.g[k] < a.mx;  // (x1 <= w; a NaN gt is not valid)
  }
  if (LOWRES) {  // sampled only where the mask needs it
    int sy0, sys;
    float ly;
    bilinear_src(a.sch, y, a.ph, sy0, sys, ly);
    const float* __restrict__ pr0 = pred + (int64_t)sy0 * a.pw;
    const float* __restrict__ pr1 = pr0 + (int64_t)sys * a.pw;
#pragma unroll
    for (int k = 0; k < 5; ++k) r.p[k] = r.m[k] ? clean_pred(bilinear_at(pr0, pr1, ly, a.scw, x0 + k, a.pw), a.mn, a.mx) : 0.f;
  } else {
    const float* __restrict__ prow = pred + (int64_t)y * w;
    load4(prow, x0, w, a.vec, r.p);
    r.p[4] = x0 + 4 < w ? prow[x0 + 4] : 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) r.p[k] = r.m[k] ? clean_pred(r.p[k], a.mn, a.mx) : 0.f;
  }
}

// one valid pair (a = left / top, b = right / bottom) of the ground truth (ga, gb) and the prediction (pa, pb): its flags at every
// ratio into the packed counters c[i] = {tp, np, ng}.  SH = 0: a horizontal pair (L in byte 0, R in byte 2); SH = 8: a vertical pair (T in
// byte 1, B in byte 3).  Compare after multiply, the product rounded to fp32 (the file is built with -ffp-contract=off).
template <int SH>
__device__ __forceinline__ void add_pair(const BoundaryArgs& a, float ga, float gb, float pa, float pb, uint32_t (&c)[kMaxT][3]) {
  const float tm = a.tmin;
  if (a.skip && !(ga > tm * gb || gb > tm * ga || pa > tm * pb || pb > tm * pa)) return;  // no boundary at the smallest ratio: none at any
#pragma unroll
  for (int i = 0; i < kMaxT; ++i) {
    if (i < a.nt) {
      const float t = a.t[i];
      const uint32_t ng = (ga > t * gb ? 1u : 0u) | (gb > t * ga ? 0x10000u : 0u);
      const uint32_t np = (pa > t * pb ? 1u : 0u) | (pb > t * pa ? 0x10000u : 0u);
      c[i][0] += (np & ng) << SH;
      c[i][1] += np << SH;
      c[i][2] += ng << SH;
    }
  }
}

template <bool LOWRES>
__global__ void __launch_bounds__(256) boundary_pass_kernel(BoundaryArgs a, long long* __restrict__ part) {
  __shared__ unsigned int tab[kPart];
  const int f = blockIdx.z, h = a.h, w = a.w;
  const float* __restrict__ gt = a.gt + (int64_t)f * h * w;
  const float* __restrict__ pred = a.pred + (LOWRES ? (int64_t)f * a.ph * a.pw : (int64_t)f * h * w);
  for (int j = threadIdx.x; j < kPart; j += 256) tab[j] = 0u;
  __syncthreads();

  uint32_t c[kMaxT][3];
#pragma unroll
  for (int i = 0; i < kMaxT; ++i) c[i][0] = c[i][1] = c[i][2] = 0u;
  uint32_t nh = 0u, nv = 0u;

  const int r0 = blockIdx.y * kRows;
  const int ya = max(r0, a.y0), yb = min(min(r0 + kRows, h), a.y1);  // the rows this block owns, inside the crop
  const int yend = min(yb + 1, a.y1);                                 // and the one below them that its vertical pairs end in
  const int x0 = blockIdx.x * kCols + (int)threadIdx.x * 4;
  if (ya < yb && x0 < w && x0 + 3 >= a.x0 && x0 < a.x1) {  // a quad outside the crop's columns starts no pair
    float g1[4], p1[4];                                     // row y - 1 of the quad
    bool m1[4] = {false, false, false, false};
#pragma unroll
    for (int k = 0; k < 4; ++k) g1[k] = p1[k] = 0.f;
    for (int y = ya; y < yend; ++y) {
      Row5 r;
      load_row<LOWRES>(a, gt, pred, y, x0, r);
      if (y < yb) {  // the horizontal pairs that start at the row's own pixels
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(r.m[k] && r.m[k + 1])) continue;
          ++nh;
          add_pair<0>(a, r.g[k], r.g[k + 1], r.p[k], r.p[k + 1], c);
        }
      }
      if (y > ya) {  // the vertical pairs that start one row up (a row this block owns) and end here
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!(m1[k] && r.m[k])) continue;
          ++nv;
          add_pair<8>(a, g1[k], r.g[k], p1[k], r.p[k], c);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) g1[k] = r.g[k], p1[k] = r.p[k], m1[k] = r.m[k];
    }
  }
  // the pair counts: a wave's sum by shuffles, one LDS addition per wave; the packed flags: one LDS addition per non-zero byte
  // (integer additions commute: the table does not depend on the order the lanes arrive in)
  for (int o = 32; o > 0; o >>= 1) {
    nh += __shfl_down(nh, o, 64);
    nv += __shfl_down(nv, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nh) atomicAdd(&tab[0], nh);
    if (nv) atomicAdd(&tab[1], nv);
  }
#pragma unroll
  for (int i = 0; i < kMaxT; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const uint32_t v = c[i][j];
      if (v == 0u) continue;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t b = (v >> (8 * d)) & 255u;
        if (b) atomicAdd(&tab[2 + (i * 4 + d) * 3 + j], b);
      }
    }
  }
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (int64_t)gridDim.x * gridDim.y;
  for (int j = threadIdx.x; j < kPart; j += 256) part[((int64_t)f * nblk + blk) * kPart + j] = (long long)tab[j];
}

// out[f][j], j < nv = 2 + 12 T: the blocks' rows added in block order (integers below 2^53: exact as float64)
__global__ void __launch_bounds__(256) boundary_final_kernel(const long long* __restrict__ part, double* __restrict__ out, int nblk, int nv) {
  const int f = blockIdx.x, j = threadIdx.x;
  if (j >= nv) return;
  long long v = 0;
  for (int b = 0; b < nblk; ++b) v += part[((int64_t)f * nblk + b) * kPart + j];
  out[(int64_t)f * nv + j] = (double)v;
}

static inline int64_t boundary_blocks(int h, int w) { return cdiv(h, kRows) * cdiv(w, kCols); }

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_boundary_f1_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || cdiv(h, kRows) > 65535) return -1;
  return (int64_t)n * boundary_blocks(h, w) * kPart * (int64_t)sizeof(long long);
}

extern "C" int prv2_boundary_f1(const float* gt, const float* pred, int32_t n, int32_t h, int32_t w, int32_t ph, int32_t pw, float min_depth,
                                float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, const float* thresholds, int32_t n_thresholds,
                                double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "boundary_f1";
  PRV2_REQUIRE(gt && pred && out && thresholds, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1 && cdiv(h, kRows) <= 65535, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE(ph >= 1 && pw >= 1, "%s: bad prediction shape %d x %d", name, ph, pw);
  PRV2_REQUIRE((int64_t)h * w < (int64_t)INT_MAX, "%s: a frame of %d x %d exceeds 2^31 pixels", name, h, w);
  PRV2_REQUIRE((int64_t)ph * pw < (int64_t)INT_MAX, "%s: a prediction of %d x %d exceeds 2^31 pixels", name, ph, pw);
  PRV2_REQUIRE(y0 >= 0 && y0 <= y1 && y1 <= h && x0 >= 0 && x0 <= x1 && x1 <= w, "%s: crop rows [%d, %d) columns [%d, %d) outside %d x %d", name,
               y0, y1, x0, x1, h, w);
  PRV2_REQUIRE(n_thresholds >= 1 && n_thresholds <= kMaxT, "%s: %d thresholds, not in [1, %d]", name, n_thresholds, kMaxT);
  BoundaryArgs a;
  a.nt = n_thresholds;
  a.tmin = thresholds[0];
  for (int i = 0; i < kMaxT; ++i) {
    a.t[i] = i < n_thresholds ? thresholds[i] : 0.f;
    if (i >= n_thresholds) continue;
    PRV2_REQUIRE(isfinite(a.t[i]) && a.t[i] > 1.0f, "%s: threshold %d = %g is not a finite ratio > 1", name, i, (double)a.t[i]);
    a.tmin = fminf(a.tmin, a.t[i]);
  }
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 8) && aligned(out, 8), "%s: null or misaligned workspace / out", name);
  const int64_t need = prv2_boundary_f1_workspace_bytes(n, h, w);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_boundary_f1_workspace_bytes)", name, (long long)workspace_bytes,
               (long long)need);
  const bool lowres = ph != h || pw != w;
  a.gt = gt, a.pred = pred;
  a.h = h, a.w = w;
  a.vec = w % 4 == 0 && aligned(gt, 16) && (lowres || aligned(pred, 16));
  a.mn = min_depth, a.mx = max_depth;
  a.skip = min_depth >= 0.f;
  a.y0 = y0, a.y1 = y1, a.x0 = x0, a.x1 = x1;
  a.ph = ph, a.pw = pw;
  a.sch = (float)ph / (float)h, a.scw = (float)pw / (float)w;
  const int nblk = (int)boundary_blocks(h, w);
  long long* part = (long long*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(w, kCols), (unsigned)cdiv(h, kRows), (unsigned)n), block(256);
  if (lowres)
    hipLaunchKernelGGL((boundary_pass_kernel<true>), grid, block, 0, s, a, part);
  else
    hipLaunchKernelGGL((boundary_pass_kernel<false>), grid, block, 0, s, a, part);
  hipLaunchKernelGGL(boundary_final_kernel, dim3(n), dim3(256), 0, s, (const long long*)part, out, nblk, PRV2_BOUNDARY_VALUES(n_thresholds));
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
