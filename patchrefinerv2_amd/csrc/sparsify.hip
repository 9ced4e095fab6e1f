// Sparsification scores of a per-pixel uncertainty (include/prv2.h "Sparsification"): the curves behind AUSE / AURG (Ilg et al. 2018,
// Poggi et al. 2020) of B frames.  Not in the reference: the definition is the header's, the oracle metrics.compute_uncertainty_metrics.
//
//   sparsify_terms_kernel   one pass over gt / pred / uncert / count: the three key maps (the uncertainty with the count override,
//                           e_rel, e_sq: correctly rounded fp32, no contraction) and the valid mask.  The maps ARE materialised
//                           (13 bytes per pixel in the workspace): the radix select reads a key map and a mask eight times per
//                           call, and the sums pass reads them once more instead of recomputing them.
//   order_stats_levels      csrc/output.hip's radix select (prv2_order_stats' kernels), at most 8 levels per call: 3 x ceil(L / 8)
//                           calls; the rank of level k follows each frame's own count on the device, so nothing is read back
//   sparsify_sums_kernel    one pass over the key maps: the 3 L thresholds in LDS, every valid pixel finds its bucket in each of the
//                           three orderings by bisection (bucket b: key in (t_{b+1}, t_b]) and adds its count and terms there
//   sparsify_final_kernel   the partials in block order, the suffix sums over the buckets (S_k = buckets k .. L - 1), n, the thresholds
//
// Fixed order everywhere: a wave gathers the lanes of one bucket at a time (the bucket of its first pending lane), reduces their
// terms by a shuffle tree and its lane 0 adds the sum to the wave's own LDS row -- as many rounds as the wave holds distinct buckets,
// no level is tested per pixel and no floating-point atomic exists; the four waves' rows are added in wave order, the blocks'
// partials in block order.  A frame's grid does not depend on the frame count: the same bits on every call, alone or in a batch.
#include <limits.h>
#include <math.h>

#include "evalgt_terms.h"

namespace prv2 {

// csrc/output.hip
void order_stats_levels(const float* value, const uint8_t* mask, int n, int64_t hw, int levels, int k0, int n_ranks, int64_t* counts,
                        float* out, int out_stride, void* workspace, hipStream_t s);

namespace {

constexpr int kMaxLevels = PRV2_SPARSIFY_MAX_LEVELS;
constexpr int kQ = 7;            // per bucket: count / sum e_rel / sum e_sq (uncertainty order), count / sum e_rel (e_rel order), count / sum e_sq (e_sq order)
constexpr int kPixPerBlock = 4096;
constexpr int kMaxBlocks = 1024;  // per frame; the rest is grid-strided
constexpr int kSelRanks = 8;     // prv2_order_stats' limit per call
static_assert(kMaxLevels == 64, "one LDS row of 64 buckets per quantity");

struct SpArgs {
  const float* gt;
  const float* pred;
  const float* uncert;
  const float* count;  // nullable
  double min_count;
  float mn, mx;
  int64_t hw;
  int levels;
  float* keys;    // [3][n][hw]
  uint8_t* mask;  // [n][hw]
  int64_t plane;  // n * hw
};

__global__ void __launch_bounds__(256) sparsify_terms_kernel(SpArgs a) {
  const int64_t base = (int64_t)blockIdx.y * a.hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.hw; i += (int64_t)gridDim.x * 256) {
    const float g = a.gt[base + i];
    const bool valid = g > a.mn && g < a.mx;  // (a NaN is not valid)
    float ku = 0.f, kr = 0.f, ks = 0.f;
    if (valid) {
      const float p = clean_pred(a.pred[base + i], a.mn, a.mx);
      const float d = __fsub_rn(g, p);
      kr = __fdiv_rn(fabsf(d), g);
      ks = __fmul_rn(d, d);
      ku = a.uncert[base + i];
      if (a.count && (double)a.count[base + i] < a.min_count) ku = INFINITY;
    }
    a.keys[base + i] = ku;
    a.keys[a.plane + base + i] = kr;
    a.keys[2 * a.plane + base + i] = ks;
    a.mask[base + i] = valid ? 1 : 0;
  }
}

// K <= t in np.sort's order (every NaN last)
__device__ __forceinline__ bool key_le(float K, float t) { return t != t || K <= t; }

// the largest k with K <= t[k]; t is non-increasing, and t[0] is the largest valid key
__device__ __forceinline__ int bucket_of(const float* t, int L, float K) {
  int lo = 0, hi = L - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (key_le(K, t[mid]))
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the wave's lanes with b >= 0 add (1, v0[, v1]) to rows q0, q0 + 1[, q0 + 2] of the wave's LDS block at column b: one bucket per
// round, a shuffle tree over its lanes (the others give 0), lane 0 writes.  The loop condition is wave-uniform.
template <int NV>
__device__ __forceinline__ void wave_bucket_add(double* acc, int q0, int b, double v0, double v1, int lane) {
  unsigned long long todo = __ballot(b >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int cur = __shfl(b, leader, 64);
    const bool mine = b == cur;
    const unsigned long long grp = __ballot(mine);
    double s0 = mine ? v0 : 0.0, s1 = mine ? v1 : 0.0;
    for (int o = 32; o > 0; o >>= 1) {
      s0 += __shfl_down(s0, o, 64);
      if (NV > 1) s1 += __shfl_down(s1, o, 64);
    }
    if (lane == 0) {
      acc[q0 * kMaxLevels + cur] += (double)__popcll(grp);
      acc[(q0 + 1) * kMaxLevels + cur] += s0;
      if (NV > 1) acc[(q0 + 2) * kMaxLevels + cur] += s1;
    }
    todo &= ~grp;
  }
}

// thr: [n][3][L]; part: [n][nblk][kQ][L]
__global__ void __launch_bounds__(256) sparsify_sums_kernel(SpArgs a, const float* __restrict__ thr, double* __restrict__ part) {
  __shared__ float t[3][kMaxLevels];
  __shared__ double acc[4][kQ * kMaxLevels];
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = a.levels;
  for (int j = tid; j < 3 * L; j += 256) t[j / L][j % L] = thr[(int64_t)f * 3 * L + j];
  for (int j = tid; j < 4 * kQ * kMaxLevels; j += 256) (&acc[0][0])[j] = 0.0;
  __syncthreads();
  const int64_t base = (int64_t)f * a.hw;
  double* mine = acc[wave];
  // (the bound is block-uniform: every lane of a wave takes part in every round's shuffles)
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < a.hw; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + tid;
    const bool valid = i < a.hw && a.mask[base + i] != 0;
    int bu = -1, br = -1, bs = -1;
    double er = 0.0, es = 0.0;
    if (valid) {
      const float kr = a.keys[a.plane + base + i], ks = a.keys[2 * a.plane + base + i];
      bu = bucket_of(t[0], L, a.keys[base + i]);
      br = bucket_of(t[1], L, kr);
      bs = bucket_of(t[2], L, ks);
      er = (double)kr, es = (double)ks;
    }
    wave_bucket_add<2>(mine, 0, bu, er, es, lane);
    wave_bucket_add<1>(mine, 3, br, er, 0.0, lane);
    wave_bucket_add<1>(mine, 5, bs, es, 0.0, lane);
  }
  __syncthreads();
  double* out = part + ((int64_t)f * gridDim.x + blockIdx.x) * kQ * L;
  for (int j = tid; j < kQ * L; j += 256) {
    const int c = (j / L) * kMaxLevels + j % L;
    out[j] = ((acc[0][c] + acc[1][c]) + acc[2][c]) + acc[3][c];
  }
}

// out[f]: 0 n; 1 .. 3 L the thresholds (uncertainty, e_rel, e_sq order); then kQ rows of L suffix sums
__global__ void __launch_bounds__(256) sparsify_final_kernel(const double* __restrict__ part, const float* __restrict__ thr,
                                                            const int64_t* __restrict__ counts, double* __restrict__ out, int nblk, int L) {
  __shared__ double tot[kQ * kMaxLevels];
  const int f = blockIdx.x, tid = threadIdx.x;
  double* o = out + (int64_t)f * PRV2_SPARSIFY_VALUES(L);
  for (int j = tid; j < kQ * L; j += 256) {
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += part[((int64_t)f * nblk + b) * kQ * L + j];
    tot[j] = v;
  }
  for (int j = tid; j < 3 * L; j += 256) o[1 + j] = (double)thr[(int64_t)f * 3 * L + j];
  if (tid == 0) o[0] = (double)counts[f];
  __syncthreads();
  if (tid < kQ) {
    double s = 0.0;
    for (int k = L - 1; k >= 0; --k) {
      s += tot[tid * L + k];
      o[1 + 3 * L + tid * L + k] = s;
    }
  }
}

static inline int sp_blocks(int64_t hw) { return (int)(cdiv(hw, kPixPerBlock) < kMaxBlocks ? cdiv(hw, kPixPerBlock) : kMaxBlocks); }

struct SpLayout {
  int64_t part, counts, sel, keys, thr, mask, total;
};
static SpLayout sp_layout(int n, int64_t hw, int L) {
  SpLayout l;
  int64_t o = 0;
  l.part = o, o += (int64_t)n * sp_blocks(hw) * kQ * L * (int64_t)sizeof(double);
  l.counts = o, o += (int64_t)n * 8;
  l.sel = o, o += roundup(prv2_output_workspace_bytes(n), 8);
  l.keys = o, o += 3 * (int64_t)n * hw * 4;
  l.thr = o, o += (int64_t)n * 3 * L * 4;
  l.mask = o, o += (int64_t)n * hw;
  l.total = roundup(o, 16);
  return l;
}

static bool sp_shape_ok(int n, int h, int w, int levels) {
  return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)n * h * w < (int64_t)INT_MAX / 4 && levels >= 1 && levels <= kMaxLevels;
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_sparsify_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t levels) {
  if (!sp_shape_ok(n, h, w, levels)) return -1;
  return sp_layout(n, (int64_t)h * w, levels).total;
}

extern "C" int prv2_sparsify(const float* gt, const float* pred, const float* uncert, const float* count, double min_count, int32_t n,
                             int32_t h, int32_t w, float min_depth, float max_depth, int32_t levels, double* out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  const char* name = "sparsify";
  PRV2_REQUIRE(gt && pred && uncert && out, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad frame shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX / 4, "%s: %d frames of %d x %d exceed 2^29 pixels", name, n, h, w);
  PRV2_REQUIRE(levels >= 1 && levels <= kMaxLevels, "%s: %d levels out of range [1, %d]", name, levels, kMaxLevels);
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 8) && aligned(out, 8), "%s: null or misaligned workspace / out", name);
  const int64_t hw = (int64_t)h * w;
  const SpLayout l = sp_layout(n, hw, levels);
  PRV2_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %lld bytes < %lld (prv2_sparsify_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)l.total);
  char* ws = (char*)workspace;
  double* part = (double*)(ws + l.part);
  int64_t* counts = (int64_t*)(ws + l.counts);
  float* thr = (float*)(ws + l.thr);
  SpArgs a;
  a.gt = gt, a.pred = pred, a.uncert = uncert, a.count = count;
  a.min_count = min_count;
  a.mn = min_depth, a.mx = max_depth;
  a.hw = hw;
  a.levels = levels;
  a.keys = (float*)(ws + l.keys);
  a.mask = (uint8_t*)(ws + l.mask);
  a.plane = (int64_t)n * hw;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = sp_blocks(hw);
  hipLaunchKernelGGL(sparsify_terms_kernel, dim3(flat_grid(hw, 256), n), dim3(256), 0, s, a);
  for (int o = 0; o < 3; ++o)
    for (int k0 = 0; k0 < levels; k0 += kSelRanks)
      order_stats_levels(a.keys + o * a.plane, a.mask, n, hw, levels, k0, levels - k0 < kSelRanks ? levels - k0 : kSelRanks, counts,
                         thr + o * levels + k0, 3 * levels, ws + l.sel, s);
  hipLaunchKernelGGL(sparsify_sums_kernel, dim3(nblk, n), dim3(256), 0, s, a, (const float*)thr, part);
  hipLaunchKernelGGL(sparsify_final_kernel, dim3(n), dim3(256), 0, s, (const double*)part, (const float*)thr, (const int64_t*)counts, out, nblk,
                     levels);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
