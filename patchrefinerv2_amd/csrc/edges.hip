// Edge-aware depth evaluation on the GPU (include/prv2.h "Edge-aware evaluation"): the depth preprocessing of extract_edges,
// a Canny detector bit-identical to metrics.canny (scipy.ndimage arithmetic), an exact Euclidean distance transform, k x k
// binary dilation and the boundary-metric statistics of compute_boundary_metrics.  Every entry point takes B >= 1 frames
// [n, h, w] and a caller workspace of prv2_edges_workspace_bytes(n, h, w) bytes; the launch count of each is fixed.
// prv2_seg_canny (one frame) is kornia's Canny on a colour segmentation map, in the same workspace and with the same hysteresis kernels.
//
// Arithmetic contract of the Canny stages (what makes them bit-identical to scipy on identical fp32 input):
//   - the file is built with -ffp-contract=off (Makefile CXXFLAGS): no FMA in any expression below;
//   - a correlate1d pass loads fp32, accumulates in double in scipy's order (centre tap first, then the symmetric pairs
//     (x[-j] +/- x[+j]) * w_j from the outermost pair inward) and rounds to fp32 once at the end of the pass;
//   - fp32 products / sums / quotients are written with __fmul_rn / __fadd_rn / __fdiv_rn (IEEE, round to nearest).
#include <limits.h>

#include "common.h"

namespace prv2 {
namespace {

constexpr int kMaxRadius = 15;   // Gaussian taps per side (sigma <= 3.6)
constexpr int kRedBlocks = 256;  // blocks per frame of the deterministic reductions (fixed: B frames == B single calls)
constexpr int kTile = 32;        // CCL tile (32 x 32 pixels, 256 threads x 4)
constexpr int kEdtMaxW = 5120;   // EDT row pass keeps a row of g (int32) and the envelope (2 x int16) in LDS
constexpr int kStats = 8;        // TP, FP, FN, TN, n_bde, n_gt, sum D_target (bde), sum D_pred (gt)

struct GaussW {
  double w[kMaxRadius + 1];  // centre first
  int r;
};

struct Layout {
  size_t t, sm, isob, jsob, mag, low, lab, root, strong, part, total;
};

static Layout layout(int n, int h, int w) {
  const size_t N = (size_t)n * h * w;
  Layout L{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  };
  L.t = take(N * 4);
  L.sm = take(N * 4);
  L.isob = take(N * 4);
  L.jsob = take(N * 4);
  L.mag = take(N * 4);
  L.low = take(N);
  L.lab = take(N * 4);
  L.root = take(N * 4);
  L.strong = take(N * 4);
  L.part = take((size_t)n * kRedBlocks * kStats * 8);
  L.total = off;
  return L;
}

template <typename T>
static T* at(void* ws, size_t off) {
  return (T*)((char*)ws + off);
}

PRV2_NO_PACKED_FP32_BEGIN

// ------------------------------------------------------------------------------------------------ block reductions (fixed order)
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : (a < b ? a : b); }
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : (a > b ? a : b); }

template <bool MAX>
__device__ float block_minmax(float v, float* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = MAX ? max_nan(sh[t], sh[t + s]) : min_nan(sh[t], sh[t + s]);
    __syncthreads();
  }
  v = sh[0];
  __syncthreads();
  return v;
}

// ------------------------------------------------------------------------------------------------ preprocessing (metric.py:184-198)
// mode 0 'none': log((d > 0) * clamp(d, eps)) / log(1.5f); 1 'log': (d > 0) * log(clamp(d, eps)); 2 'inv': (d > 0) / clamp(d, eps)
// (then the two passes below).  torch's clamp keeps NaN; bool * x promotes the bool to 0.f / 1.f.
__global__ void __launch_bounds__(256) pre_kernel(const float* __restrict__ d, float* __restrict__ out, int64_t hw, int mode,
                                                  float* __restrict__ part) {
  __shared__ float sh[256];
  const int f = blockIdx.y;
  const float eps = 1.1920928955078125e-07f;
  const float log15 = 0.405465096235275268554688f;  // torch.log(torch.tensor(1.5)) (float32)
  float mn = __int_as_float(0x7f800000);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = d[f * hw + i];
    const float m = v > 0.f ? 1.f : 0.f;
    const float c = v < eps ? eps : v;
    float o;
    if (mode == 1) o = __fmul_rn(m, (float)log((double)c));  // (log in double, rounded once: the correctly rounded fp32 log)
    else if (mode == 2) o = __fdiv_rn(m, c);
    else o = __fdiv_rn((float)log((double)__fmul_rn(m, c)), log15);
    out[f * hw + i] = o;
    mn = min_nan(mn, o);
  }
  if (mode == 2) {
    mn = block_minmax<false>(mn, sh);
    if (threadIdx.x == 0) part[f * kRedBlocks + blockIdx.x] = mn;
  }
}

// 'inv' pass 2: out -= min(frame) (every block reduces the kRedBlocks partials itself), partial max of the result
__global__ void __launch_bounds__(256) inv_shift_kernel(float* __restrict__ out, int64_t hw, const float* __restrict__ part_min,
                                                        float* __restrict__ part_max) {
  __shared__ float sh[256];
  const int f = blockIdx.y;
  const float mn = block_minmax<false>(part_min[f * kRedBlocks + threadIdx.x], sh);
  float mx = -__int_as_float(0x7f800000);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
    const float o = __fsub_rn(out[f * hw + i], mn);
    out[f * hw + i] = o;
    mx = max_nan(mx, o);
  }
  mx = block_minmax<true>(mx, sh);
  if (threadIdx.x == 0) part_max[f * kRedBlocks + blockIdx.x] = mx;
}

// 'inv' pass 3: out /= max(frame)
__global__ void __launch_bounds__(256) inv_scale_kernel(float* __restrict__ out, int64_t hw, const float* __restrict__ part_max) {
  __shared__ float sh[256];
  const int f = blockIdx.y;
  const float mx = block_minmax<true>(part_max[f * kRedBlocks + threadIdx.x], sh);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x)
    out[f * hw + i] = __fdiv_rn(out[f * hw + i], mx);
}

// ------------------------------------------------------------------------------------------------ Canny: Gaussian (mode='constant')
// pass 1, axis 0: t = fp32(correlate1d(img, w, axis=0))
__global__ void __launch_bounds__(256) gauss0_kernel(const float* __restrict__ img, float* __restrict__ t, int n, int h, int w, GaussW g) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const float* src = img + f * hw + x;
    double acc = (double)src[(int64_t)y * w] * g.w[0];
    for (int j = g.r; j >= 1; --j) {
      const double a = y - j >= 0 ? (double)src[(int64_t)(y - j) * w] : 0.0;
      const double b = y + j < h ? (double)src[(int64_t)(y + j) * w] : 0.0;
      acc = acc + (a + b) * g.w[j];
    }
    t[i] = (float)acc;
  }
}

// pass 2, axis 1, and the bleed correction: smoothed = fp32(correlate1d(t, w, axis=1)) / (gaussian_filter(ones) + eps_f32).
// gaussian_filter(ones) is computed here the way scipy computes it: b0(y) = fp32(axis-0 pass of a column of ones), then the
// axis-1 pass over a row that holds b0(y) inside the frame and 0 outside.
__global__ void __launch_bounds__(256) gauss1_kernel(const float* __restrict__ t, float* __restrict__ sm, int n, int h, int w, GaussW g) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const float* row = t + f * hw + (int64_t)y * w;
    double acc = (double)row[x] * g.w[0];
    double b0 = 1.0 * g.w[0];
    for (int j = g.r; j >= 1; --j) {
      const double a = x - j >= 0 ? (double)row[x - j] : 0.0;
      const double b = x + j < w ? (double)row[x + j] : 0.0;
      acc = acc + (a + b) * g.w[j];
      b0 = b0 + ((y - j >= 0 ? 1.0 : 0.0) + (y + j < h ? 1.0 : 0.0)) * g.w[j];
    }
    const double c0 = (double)(float)b0;
    double bl = c0 * g.w[0];
    for (int j = g.r; j >= 1; --j) bl = bl + ((x - j >= 0 ? c0 : 0.0) + (x + j < w ? c0 : 0.0)) * g.w[j];
    const float bleed = __fadd_rn((float)bl, 1.1920928955078125e-07f);
    sm[i] = __fdiv_rn((float)acc, bleed);
  }
}

// ------------------------------------------------------------------------------------------------ Canny: Sobel (mode='reflect')
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - i - 1 : i); }

// ndi.sobel(s, axis): correlate1d([-1, 0, 1], axis) -> fp32, then correlate1d([1, 2, 1], other axis) -> fp32.  The derivative pass
// is scipy's antisymmetric loop: acc = x0 * 0, acc += (x[-1] - x[+1]) * -1.  magnitude = fp32 sqrt of the fp32 i*i + j*j (the
// double sqrt of an fp32 value rounded to fp32 is the correctly rounded fp32 sqrt).
__device__ __forceinline__ float dpass(float c, float m, float p) {
  double acc = (double)c * 0.0;
  acc = acc + ((double)m - (double)p) * -1.0;
  return (float)acc;
}
__device__ __forceinline__ float spass(float c, float m, float p) {
  double acc = (double)c * 2.0;
  acc = acc + ((double)m + (double)p) * 1.0;
  return (float)acc;
}

__global__ void __launch_bounds__(256) sobel_kernel(const float* __restrict__ sm, float* __restrict__ isob, float* __restrict__ jsob,
                                                    float* __restrict__ mag, int n, int h, int w) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const float* s = sm + f * hw;
    auto S = [&](int yy, int xx) { return s[(int64_t)reflect(yy, h) * w + reflect(xx, w)]; };
    // isobel: derivative along axis 0 at columns x-1, x, x+1, then [1, 2, 1] along axis 1
    float a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      const int xx = reflect(x + k - 1, w);
      a[k] = dpass(S(y, xx), S(y - 1, xx), S(y + 1, xx));
      const int yy = reflect(y + k - 1, h);
      b[k] = dpass(S(yy, x), S(yy, x - 1), S(yy, x + 1));
    }
    const float iv = spass(a[1], a[0], a[2]);
    const float jv = spass(b[1], b[0], b[2]);
    isob[i] = iv;
    jsob[i] = jv;
    mag[i] = (float)sqrt((double)__fadd_rn(__fmul_rn(iv, iv), __fmul_rn(jv, jv)));
  }
}

// ------------------------------------------------------------------------------------------------ Canny: non-maximum suppression
// metrics.canny's four sectors with bilinear weights w = num / den; a pixel in several sectors keeps the LAST sector's verdict
// (local_max[pts] = ... overwrites); the border ring is false.  Output: low = local_max & (mag >= low).
__device__ __forceinline__ bool side(float c1, float c2, float wt, float m) {
  return __fadd_rn(__fmul_rn(c2, wt), __fmul_rn(c1, __fsub_rn(1.f, wt))) <= m;
}

__global__ void __launch_bounds__(256) nms_kernel(const float* __restrict__ isob, const float* __restrict__ jsob,
                                                  const float* __restrict__ mag, uint8_t* __restrict__ low, int n, int h, int w,
                                                  float lo) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    bool lm = false;
    const float m = mag[i];
    if (y > 0 && y < h - 1 && x > 0 && x < w - 1 && m >= lo) {
      const float* M = mag + f * hw;
      auto G = [&](int dy, int dx) { return M[(int64_t)(y + dy) * w + (x + dx)]; };
      const float iv = isob[i], jv = jsob[i], ai = fabsf(iv), aj = fabsf(jv);
      const bool same = (iv >= 0.f && jv >= 0.f) || (iv <= 0.f && jv <= 0.f);
      const bool opp = (iv <= 0.f && jv >= 0.f) || (iv >= 0.f && jv <= 0.f);
      if (same && ai >= aj) {  // 0 - 45
        const float wt = __fdiv_rn(aj, ai);
        lm = side(G(1, 0), G(1, 1), wt, m) && side(G(-1, 0), G(-1, -1), wt, m);
      }
      if (same && ai <= aj) {  // 45 - 90
        const float wt = __fdiv_rn(ai, aj);
        lm = side(G(0, 1), G(1, 1), wt, m) && side(G(0, -1), G(-1, -1), wt, m);
      }
      if (opp && ai <= aj) {  // 90 - 135
        const float wt = __fdiv_rn(ai, aj);
        lm = side(G(0, 1), G(-1, 1), wt, m) && side(G(0, -1), G(1, -1), wt, m);
      }
      if (opp && ai >= aj) {  // 135 - 180
        const float wt = __fdiv_rn(aj, ai);
        lm = side(G(-1, 0), G(-1, 1), wt, m) && side(G(1, 0), G(1, -1), wt, m);
      }
    }
    low[i] = (lm && m >= lo) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ hysteresis: 8-connected labelling
// Labels are batch-flat pixel indices (frame * h * w + y * w + x); a root is its own label and every link points to a smaller index.
// 1. ccl_local: union-find of each 32 x 32 tile in LDS; every low pixel gets its tile-local root; strong[] is cleared.
// 2. ccl_merge: the 8-neighbour pairs that cross a tile border are joined in the global forest.  lab[] is written by other
//    workgroups in this launch, so every access to it is an agent-scope atomic (no plain loads: gfx950's per-XCD L2s).
// 3. ccl_resolve: root[p] = find(p) (lab[] is read-only here); a pixel with mag >= high marks strong[root].
// 4. ccl_final: edges = low & strong[root].
__device__ __forceinline__ int lds_ld(int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ int lds_find(int* L, int x) {
  for (;;) {
    const int p = lds_ld(&L[x]);
    if (p == x) return x;
    x = p;
  }
}

__device__ void lds_union(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(256) ccl_local_kernel(const uint8_t* __restrict__ low, int32_t* __restrict__ lab,
                                                        int32_t* __restrict__ strong, int h, int w) {
  __shared__ int L[kTile * kTile];
  const int f = blockIdx.z, ty0 = blockIdx.y * kTile, tx0 = blockIdx.x * kTile;
  const int64_t base = (int64_t)f * h * w;
  bool on[4];
  for (int k = 0; k < 4; ++k) {
    const int li = threadIdx.x + 256 * k, gy = ty0 + (li >> 5), gx = tx0 + (li & 31);
    const bool in = gy < h && gx < w;
    on[k] = in && low[base + (int64_t)gy * w + gx];
    L[li] = on[k] ? li : -1;
    if (in) strong[base + (int64_t)gy * w + gx] = 0;
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    if (!on[k]) continue;
    const int li = threadIdx.x + 256 * k, ly = li >> 5, lx = li & 31;
    if (lx > 0 && L[li - 1] >= 0) lds_union(L, li, li - 1);
    if (ly > 0) {
      if (lx > 0 && L[li - 33] >= 0) lds_union(L, li, li - 33);
      if (L[li - 32] >= 0) lds_union(L, li, li - 32);
      if (lx < 31 && L[li - 31] >= 0) lds_union(L, li, li - 31);
    }
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    if (!on[k]) continue;
    const int li = threadIdx.x + 256 * k, r = lds_find(L, li);
    lab[base + (int64_t)(ty0 + (li >> 5)) * w + tx0 + (li & 31)] = (int32_t)(base + (int64_t)(ty0 + (r >> 5)) * w + tx0 + (r & 31));
  }
}

__device__ __forceinline__ int g_ld(int32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// find with path halving: lab[x] only ever decreases to an ancestor of x, so the forest stays a forest of the same sets
__device__ int g_find(int32_t* lab, int x) {
  for (;;) {
    const int p = g_ld(&lab[x]);
    if (p == x) return x;
    const int gp = g_ld(&lab[p]);
    if (gp != p) __hip_atomic_fetch_min(&lab[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
}

__device__ void g_union(int32_t* lab, int a, int b) {
  for (;;) {
    a = g_find(lab, a);
    b = g_find(lab, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(&lab[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(256) ccl_merge_kernel(const uint8_t* __restrict__ low, int32_t* lab, int n, int h, int w) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const bool left = x > 0 && (x % kTile) == 0, top = y > 0 && (y % kTile) == 0;
    if (!(left || top) || !low[i]) continue;
    const int64_t fb = f * hw;
    auto join = [&](int yy, int xx) {
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) return;
      const int64_t q = fb + (int64_t)yy * w + xx;
      if (low[q]) g_union(lab, (int)i, (int)q);
    };
    if (left) {
      join(y - 1, x - 1);
      join(y, x - 1);
      join(y + 1, x - 1);
    }
    if (top) {
      join(y - 1, x - 1);
      join(y - 1, x);
      join(y - 1, x + 1);
    }
  }
}

__global__ void __launch_bounds__(256) ccl_resolve_kernel(const uint8_t* __restrict__ low, const float* __restrict__ mag,
                                                          const int32_t* __restrict__ lab, int32_t* __restrict__ root, int32_t* strong,
                                                          int64_t total, float hi) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (!low[i]) continue;
    int x = lab[i];
    for (int p = lab[x]; p != x; p = lab[x]) x = p;
    root[i] = x;
    if (mag[i] >= hi) __hip_atomic_store(&strong[x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(256) ccl_final_kernel(const uint8_t* __restrict__ low, const int32_t* __restrict__ root,
                                                        const int32_t* __restrict__ strong, uint8_t* __restrict__ edges, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
  {
    uint8_t e = 0;
    if (low[i]) e = strong[root[i]] ? 1 : 0;  // root[] is written only for low pixels
    edges[i] = e;
  }
}

// ------------------------------------------------------------------------------------------------ exact Euclidean distance transform
// Meijster, Roerdink & Hesselink (2000).  Phase 1 (per column): g = distance along the column to the nearest set pixel, h + w
// when the column has none.  Phase 2 (per row, one workgroup): the lower envelope of the parabolas (x - i)^2 + g(i)^2 built by one
// lane in LDS with integer separators (int64), then every lane reads its pixel's parabola by binary search over the segment starts.
__global__ void __launch_bounds__(256) edt_cols_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ g, int n, int h, int w) {
  const int64_t total = (int64_t)n * w;
  const int inf = h + w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / w;
    const int x = (int)(i - f * w);
    const uint8_t* m = mask + f * h * (int64_t)w + x;
    int32_t* o = g + f * h * (int64_t)w + x;
    int d = inf;
    for (int y = 0; y < h; ++y) {
      d = m[(int64_t)y * w] ? 0 : (d == inf ? inf : d + 1);
      o[(int64_t)y * w] = d;
    }
    d = inf;
    for (int y = h - 1; y >= 0; --y) {
      d = m[(int64_t)y * w] ? 0 : (d == inf ? inf : d + 1);
      if (d < o[(int64_t)y * w]) o[(int64_t)y * w] = d;
    }
  }
}

// floor(a / b), b > 0, |a| < 2^31: the double quotient of two exact integers cannot round across an integer (the distance from a
// non-integer quotient to the next integer, >= 1 / b, is far above its rounding error), and it avoids 64-bit integer division
__device__ __forceinline__ int floordiv(int a, int b) { return (int)floor((double)a / (double)b); }

__global__ void __launch_bounds__(256) edt_rows_kernel(const int32_t* __restrict__ g, int32_t* __restrict__ d2, int h, int w) {
  extern __shared__ int32_t smem[];
  int32_t* G = smem;
  int16_t *S = (int16_t*)(smem + w), *T = S + w;  // (w <= 5120: column indices fit int16; 8 w bytes of LDS per row)
  __shared__ int qs;
  const int y = blockIdx.x, f = blockIdx.y;
  const int64_t row = ((int64_t)f * h + y) * w;
  for (int x = threadIdx.x; x < w; x += blockDim.x) G[x] = g[row + x];
  __syncthreads();
  if (threadIdx.x == 0) {
    auto F = [&](int64_t x, int i) { return (x - i) * (x - i) + (int64_t)G[i] * G[i]; };
    int q = 0;
    S[0] = 0;
    T[0] = 0;
    for (int u = 1; u < w; ++u) {
      while (q >= 0 && F(T[q], S[q]) > F(T[q], u)) --q;
      if (q < 0) {
        q = 0;
        S[0] = (int16_t)u;
      } else {
        const int i = S[q];
        const int wv = 1 + floordiv(u * u - i * i + G[u] * G[u] - G[i] * G[i], 2 * (u - i));  // int32: see the h + w bound
        if (wv < w) {
          ++q;
          S[q] = (int16_t)u;
          T[q] = (int16_t)wv;
        }
      }
    }
    qs = q;
  }
  __syncthreads();
  const int q = qs;
  const int64_t big = (int64_t)(h + w) * (h + w);
  for (int u = threadIdx.x; u < w; u += blockDim.x) {
    int lo = 0, hi = q;  // last segment with T <= u (T[0] == 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (T[mid] <= u) lo = mid;
      else hi = mid - 1;
    }
    const int i = S[lo];
    const int64_t v = (int64_t)(u - i) * (u - i) + (int64_t)G[i] * G[i];
    d2[row + u] = v >= big ? INT_MAX : (int32_t)v;
  }
}

// ------------------------------------------------------------------------------------------------ k x k binary dilation (zero padding)
__global__ void __launch_bounds__(256) dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n, int h, int w, int r) {
  const int64_t hw = (int64_t)h * w, total = hw * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const uint8_t* s = in + f * hw;
    uint8_t any = 0;
    for (int yy = max(y - r, 0); yy <= min(y + r, h - 1) && !any; ++yy)
      for (int xx = max(x - r, 0); xx <= min(x + r, w - 1); ++xx) any |= s[(int64_t)yy * w + xx];
    out[i] = any ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ boundary statistics
// One pass per frame: kRedBlocks blocks write per-block partials (fixed grid-stride and tree order), one final block per frame sums
// them in block order.  No float atomics: bit-identical run to run and for B frames against B single calls.
// A frame without a set pixel has d2 = INT_MAX; scipy's distance_transform_edt then returns the distance to (-1, 0) (its feature
// transform finds no background), and the statistics use that value, as the reference does.
__device__ __forceinline__ double edt_dist(int32_t d2, int y, int x) {
  if (d2 == INT_MAX) return sqrt((double)((int64_t)(y + 1) * (y + 1) + (int64_t)x * x));
  return sqrt((double)d2);
}

__global__ void __launch_bounds__(256) stats_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                    const uint8_t* __restrict__ valid, const int32_t* __restrict__ d2t,
                                                    const int32_t* __restrict__ d2p, const uint8_t* __restrict__ gte,
                                                    const uint8_t* __restrict__ pre, int h, int w, double th, double* __restrict__ part) {
  __shared__ double sh[kStats][256];
  const int f = blockIdx.y;
  const int64_t hw = (int64_t)h * w, fb = f * hw;
  double acc[kStats] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < hw; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = fb + p;
    if (!valid[i]) continue;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    const bool ge = gte[i], pe = pre[i];
    acc[0] += (pe && ge) ? 1.0 : 0.0;
    acc[1] += (pe && !ge) ? 1.0 : 0.0;
    acc[2] += (!pe && ge) ? 1.0 : 0.0;
    acc[3] += (!pe && !ge) ? 1.0 : 0.0;
    if (pred[i]) {
      const double dt = edt_dist(d2t[i], y, x);
      if (dt < th) {
        acc[4] += 1.0;
        acc[6] += dt;
      }
    }
    if (gt[i]) {
      acc[5] += 1.0;
      acc[7] += edt_dist(d2p[i], y, x);
    }
  }
  for (int k = 0; k < kStats; ++k) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int k = 0; k < kStats; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < kStats) part[((int64_t)f * kRedBlocks + blockIdx.x) * kStats + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void __launch_bounds__(64) stats_final_kernel(const double* __restrict__ part, double* __restrict__ stats) {
  const int f = blockIdx.x, k = threadIdx.x;
  if (k >= kStats) return;
  double s = 0.0;
  for (int b = 0; b < kRedBlocks; ++b) s += part[((int64_t)f * kRedBlocks + b) * kStats + k];
  stats[f * kStats + k] = s;
}

// ------------------------------------------------------------------------------------------------ kornia's Canny on a colour map
// kornia.filters.canny(seg)[1] > 0 with its defaults (cityscapes_dataset.py:333-334; include/prv2.h prv2_seg_canny states every
// step).  All fp32, every product / sum / difference its own IEEE operation in the order the header gives (-ffp-contract=off and the
// __f*_rn intrinsics): on an axis-aligned class boundary the two pixels beside the step have mathematically equal magnitudes, and the
// strict > of the non-maximum suppression is decided by the last bit.  A thread owns four pixels of a row: float4 / uchar4 accesses
// for them when the rows are 16-byte aligned, single loads for the taps beside them.
struct Gauss5 {
  float w[5];
};

// a border index: reflect without the edge pixel (-1 -> 1, n -> n - 2) or replicate, then clamped (a quad's tail lanes stay in bounds)
template <bool REFLECT>
__device__ __forceinline__ int bidx(int i, int n) {
  if (REFLECT) i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return min(max(i, 0), n - 1);
}

// v[j] = row[border(x0 - R + j)], j in [0, 4 + 2 R): the quad's own four values as one float4 when vec
template <int R, bool REFLECT>
__device__ __forceinline__ void load_span(const float* __restrict__ row, int x0, int w, int vec, float* v) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(row + x0);
    v[R] = t.x, v[R + 1] = t.y, v[R + 2] = t.z, v[R + 3] = t.w;
    for (int j = 0; j < R; ++j) v[j] = row[bidx<REFLECT>(x0 - R + j, w)], v[R + 4 + j] = row[bidx<REFLECT>(x0 + 4 + j, w)];
  } else {
    for (int j = 0; j < 4 + 2 * R; ++j) v[j] = row[bidx<REFLECT>(x0 - R + j, w)];
  }
}

__device__ __forceinline__ void store4(float* __restrict__ dst, int x0, int w, int vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(dst + x0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4 && x0 + k < w; ++k) dst[x0 + k] = v[k];
  }
}

__device__ __forceinline__ void store4(uint8_t* __restrict__ dst, int x0, int w, int vec, const uint8_t* v) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(dst + x0) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
  } else {
    for (int k = 0; k < 4 && x0 + k < w; ++k) dst[x0 + k] = v[k];
  }
}

// the five taps summed from -2 to +2
__device__ __forceinline__ float gauss5(const Gauss5& g, float a, float b, float c, float d, float e) {
  float acc = __fmul_rn(g.w[0], a);
  acc = __fadd_rn(acc, __fmul_rn(g.w[1], b));
  acc = __fadd_rn(acc, __fmul_rn(g.w[2], c));
  acc = __fadd_rn(acc, __fmul_rn(g.w[3], d));
  return __fadd_rn(acc, __fmul_rn(g.w[4], e));
}

// grey = (0.299 R + 0.587 G) + 0.114 B, then the horizontal pass (reflect border)
__global__ void __launch_bounds__(256) seg_grey_blur_kernel(const float* __restrict__ seg, float* __restrict__ t, int h, int w, Gauss5 g, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq, hw = (int64_t)h * w;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    const int64_t ro = (int64_t)y * w;
    float r[8], gr[8], b[8], v[8], o[4];
    load_span<2, true>(seg + ro, x0, w, vec, r);
    load_span<2, true>(seg + hw + ro, x0, w, vec, gr);
    load_span<2, true>(seg + 2 * hw + ro, x0, w, vec, b);
    for (int j = 0; j < 8; ++j) v[j] = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r[j]), __fmul_rn(0.587f, gr[j])), __fmul_rn(0.114f, b[j]));
    for (int k = 0; k < 4; ++k) o[k] = gauss5(g, v[k], v[k + 1], v[k + 2], v[k + 3], v[k + 4]);
    store4(t + ro, x0, w, vec, o);
  }
}

// the vertical pass (reflect border)
__global__ void __launch_bounds__(256) seg_vblur_kernel(const float* __restrict__ t, float* __restrict__ sm, int h, int w, Gauss5 g, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    float v[5][4], o[4];
    for (int j = 0; j < 5; ++j) load_span<0, true>(t + (int64_t)bidx<true>(y - 2 + j, h) * w, x0, w, vec, v[j]);
    for (int k = 0; k < 4; ++k) o[k] = gauss5(g, v[0][k], v[1][k], v[2][k], v[3][k], v[4][k]);
    store4(sm + (int64_t)y * w, x0, w, vec, o);
  }
}

// unnormalised Sobel (replicate border), mag = sqrt((gx gx + gy gy) + 1e-6) and the axis the suppression compares along:
// 0 horizontal (|gy| <= T |gx|, which takes gx = gy = 0), 1 vertical (|gx| <= T |gy|), 2 the (+1, +1) diagonal (same signs), 3 the (+1, -1) one
__global__ void __launch_bounds__(256) seg_sobel_kernel(const float* __restrict__ sm, float* __restrict__ mag, uint8_t* __restrict__ axis, int h,
                                                        int w, int vec) {
  const float T = 0.414213568f;  // float32(tan(pi / 8))
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    float u[6], c[6], d[6], m[4];
    uint8_t ax[4];
    load_span<1, false>(sm + (int64_t)bidx<false>(y - 1, h) * w, x0, w, vec, u);
    load_span<1, false>(sm + (int64_t)y * w, x0, w, vec, c);
    load_span<1, false>(sm + (int64_t)bidx<false>(y + 1, h) * w, x0, w, vec, d);
    for (int k = 0; k < 4; ++k) {  // the pixel is at span index k + 1
      const float gx = __fadd_rn(__fadd_rn(__fsub_rn(u[k + 2], u[k]), __fmul_rn(2.0f, __fsub_rn(c[k + 2], c[k]))), __fsub_rn(d[k + 2], d[k]));
      const float gy = __fadd_rn(__fadd_rn(__fsub_rn(d[k], u[k]), __fmul_rn(2.0f, __fsub_rn(d[k + 1], u[k + 1]))), __fsub_rn(d[k + 2], u[k + 2]));
      // (the double sqrt of an fp32 value rounded to fp32 is the correctly rounded fp32 sqrt, as in sobel_kernel; __fsqrt_rn is the
      //  native instruction here, one ulp off in places)
      m[k] = (float)sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), 1e-6f));
      const float a = fabsf(gx), b = fabsf(gy);
      ax[k] = b <= __fmul_rn(T, a) ? 0 : (a <= __fmul_rn(T, b) ? 1 : ((gx > 0.f) == (gy > 0.f) ? 2 : 3));
    }
    store4(mag + (int64_t)y * w, x0, w, vec, m);
    store4(axis + (int64_t)y * w, x0, w, vec, ax);
  }
}

// local maximum: min(mag - n1, mag - n2) > 0 with the two neighbours along the axis, 0 outside the frame.  weak = maximum and
// mag > lo; strongf = 1.f where maximum and mag > hi, else 0.f (what ccl_resolve_kernel thresholds at 0.5)
__global__ void __launch_bounds__(256) seg_nms_kernel(const float* __restrict__ mag, const uint8_t* __restrict__ axis, uint8_t* __restrict__ weak,
                                                      float* __restrict__ strongf, int h, int w, float lo, float hi, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    float m[4], s[4];
    uint8_t ax[4] = {0, 0, 0, 0}, wk[4];
    load_span<0, false>(mag + (int64_t)y * w, x0, w, vec, m);
    if (vec) {
      const uint32_t t = *reinterpret_cast<const uint32_t*>(axis + (int64_t)y * w + x0);
      for (int k = 0; k < 4; ++k) ax[k] = (uint8_t)(t >> (8 * k));
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) ax[k] = axis[(int64_t)y * w + x0 + k];
    }
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      const int dy = ax[k] == 0 ? 0 : (ax[k] == 3 ? -1 : 1), dx = ax[k] == 1 ? 0 : 1;  // the (+dx, +dy) neighbour and its opposite
      auto M = [&](int yy, int xx) { return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? mag[(int64_t)yy * w + xx] : 0.f; };
      const float n1 = M(y + dy, x + dx), n2 = M(y - dy, x - dx);
      const bool mx = x < w && fminf(__fsub_rn(m[k], n1), __fsub_rn(m[k], n2)) > 0.f;
      wk[k] = (mx && m[k] > lo) ? 1 : 0;
      s[k] = (mx && m[k] > hi) ? 1.f : 0.f;
    }
    store4(weak + (int64_t)y * w, x0, w, vec, wk);
    store4(strongf + (int64_t)y * w, x0, w, vec, s);
  }
}

PRV2_NO_PACKED_FP32_END

static int check_frames(const char* name, int n, int h, int w) {
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 3 && w >= 3, "%s: frames must be at least 3 x 3 (got %d x %d)", name, h, w);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX, "%s: %d frames of %d x %d exceed 2^31 pixels", name, n, h, w);
  return 0;
}

static int check_ws(const char* name, int n, int h, int w, const void* ws, int64_t bytes) {
  PRV2_REQUIRE(ws != nullptr, "%s: null workspace", name);
  const int64_t need = (int64_t)layout(n, h, w).total;
  PRV2_REQUIRE(bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_edges_workspace_bytes)", name, (long long)bytes, (long long)need);
  return 0;
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_edges_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < 1 || w < 1) return -1;
  return (int64_t)layout(n, h, w).total;
}

extern "C" int prv2_depth_preprocess(const float* depth, int32_t n, int32_t h, int32_t w, int32_t mode, float* out, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  const char* name = "depth_preprocess";
  PRV2_REQUIRE(depth && out, "%s: null pointer", name);
  PRV2_REQUIRE(mode == PRV2_EDGE_PRE_NONE || mode == PRV2_EDGE_PRE_LOG || mode == PRV2_EDGE_PRE_INV, "%s: bad mode %d", name, mode);
  if (check_frames(name, n, h, w) || check_ws(name, n, h, w, workspace, workspace_bytes)) return 1;
  const Layout L = layout(n, h, w);
  float* pmin = at<float>(workspace, L.part);
  float* pmax = pmin + (int64_t)n * kRedBlocks;
  const int64_t hw = (int64_t)h * w;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pre_kernel, dim3(kRedBlocks, n), dim3(256), 0, s, depth, out, hw, (int)mode, pmin);
  if (mode == PRV2_EDGE_PRE_INV) {
    hipLaunchKernelGGL(inv_shift_kernel, dim3(kRedBlocks, n), dim3(256), 0, s, out, hw, pmin, pmax);
    hipLaunchKernelGGL(inv_scale_kernel, dim3(kRedBlocks, n), dim3(256), 0, s, out, hw, pmax);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_canny(const float* image, int32_t n, int32_t h, int32_t w, const double* gauss_w_host, int32_t radius, float low_threshold,
                          float high_threshold, uint8_t* edges, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "canny";
  PRV2_REQUIRE(image && edges && gauss_w_host, "%s: null pointer", name);
  PRV2_REQUIRE(radius >= 0 && radius <= kMaxRadius, "%s: Gaussian radius %d out of range [0, %d]", name, radius, kMaxRadius);
  if (check_frames(name, n, h, w) || check_ws(name, n, h, w, workspace, workspace_bytes)) return 1;
  const Layout L = layout(n, h, w);
  GaussW g{};
  g.r = radius;
  for (int j = 0; j <= radius; ++j) g.w[j] = gauss_w_host[j];
  float *t = at<float>(workspace, L.t), *sm = at<float>(workspace, L.sm), *isob = at<float>(workspace, L.isob);
  float *jsob = at<float>(workspace, L.jsob), *mag = at<float>(workspace, L.mag);
  uint8_t* low = at<uint8_t>(workspace, L.low);
  int32_t *lab = at<int32_t>(workspace, L.lab), *root = at<int32_t>(workspace, L.root), *strong = at<int32_t>(workspace, L.strong);
  const int64_t total = (int64_t)n * h * w;
  const int grid = flat_grid(total, 256);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gauss0_kernel, dim3(grid), dim3(256), 0, s, image, t, n, h, w, g);
  hipLaunchKernelGGL(gauss1_kernel, dim3(grid), dim3(256), 0, s, t, sm, n, h, w, g);
  hipLaunchKernelGGL(sobel_kernel, dim3(grid), dim3(256), 0, s, sm, isob, jsob, mag, n, h, w);
  hipLaunchKernelGGL(nms_kernel, dim3(grid), dim3(256), 0, s, isob, jsob, mag, low, n, h, w, low_threshold);
  hipLaunchKernelGGL(ccl_local_kernel, dim3(cdiv(w, kTile), cdiv(h, kTile), n), dim3(256), 0, s, low, lab, strong, h, w);
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid), dim3(256), 0, s, low, lab, n, h, w);
  hipLaunchKernelGGL(ccl_resolve_kernel, dim3(grid), dim3(256), 0, s, low, mag, lab, root, strong, total, high_threshold);
  hipLaunchKernelGGL(ccl_final_kernel, dim3(grid), dim3(256), 0, s, low, root, strong, edges, total);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_seg_canny(const float* seg_chw, int32_t h, int32_t w, const float* gauss_w5_host, float low_threshold,
                              float high_threshold, uint8_t* edges, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "seg_canny";
  PRV2_REQUIRE(seg_chw && edges && gauss_w5_host, "%s: null pointer", name);
  PRV2_REQUIRE(h >= 1 && w >= 1 && (int64_t)3 * h * w < (int64_t)INT_MAX, "%s: bad shape 3 x %d x %d", name, h, w);
  if (check_frames(name, 1, h, w) || check_ws(name, 1, h, w, workspace, workspace_bytes)) return 1;  // (3 x 3: a reflect pad of 2)
  const Layout L = layout(1, h, w);
  Gauss5 g;
  for (int j = 0; j < 5; ++j) g.w[j] = gauss_w5_host[j];
  // the plain detector's buffers under other names: isob holds the axis bytes, jsob the strong pixels as 0.f / 1.f
  float *t = at<float>(workspace, L.t), *sm = at<float>(workspace, L.sm), *mag = at<float>(workspace, L.mag);
  float* strongf = at<float>(workspace, L.jsob);
  uint8_t *axis = at<uint8_t>(workspace, L.isob), *low = at<uint8_t>(workspace, L.low);
  int32_t *lab = at<int32_t>(workspace, L.lab), *root = at<int32_t>(workspace, L.root), *strong = at<int32_t>(workspace, L.strong);
  const int64_t total = (int64_t)h * w;
  const int vec = w % 4 == 0 && aligned16(seg_chw) && aligned16(workspace);
  const int qgrid = flat_grid((int64_t)h * cdiv(w, 4), 256), grid = flat_grid(total, 256);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(seg_grey_blur_kernel, dim3(qgrid), dim3(256), 0, s, seg_chw, t, (int)h, (int)w, g, vec);
  hipLaunchKernelGGL(seg_vblur_kernel, dim3(qgrid), dim3(256), 0, s, (const float*)t, sm, (int)h, (int)w, g, vec);
  hipLaunchKernelGGL(seg_sobel_kernel, dim3(qgrid), dim3(256), 0, s, (const float*)sm, mag, axis, (int)h, (int)w, vec);
  hipLaunchKernelGGL(seg_nms_kernel, dim3(qgrid), dim3(256), 0, s, (const float*)mag, (const uint8_t*)axis, low, strongf, (int)h, (int)w,
                     low_threshold, high_threshold, vec);
  hipLaunchKernelGGL(ccl_local_kernel, dim3(cdiv(w, kTile), cdiv(h, kTile), 1), dim3(256), 0, s, low, lab, strong, h, w);
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid), dim3(256), 0, s, low, lab, 1, h, w);
  hipLaunchKernelGGL(ccl_resolve_kernel, dim3(grid), dim3(256), 0, s, low, strongf, lab, root, strong, total, 0.5f);
  hipLaunchKernelGGL(ccl_final_kernel, dim3(grid), dim3(256), 0, s, low, root, strong, edges, total);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_edt_sq(const uint8_t* mask, int32_t n, int32_t h, int32_t w, int32_t* d2, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  const char* name = "edt_sq";
  PRV2_REQUIRE(mask && d2, "%s: null pointer", name);
  if (check_frames(name, n, h, w) || check_ws(name, n, h, w, workspace, workspace_bytes)) return 1;
  PRV2_REQUIRE(w <= kEdtMaxW, "%s: width %d > %d (the row pass keeps its row in LDS)", name, w, kEdtMaxW);
  PRV2_REQUIRE(h + w <= 32768, "%s: h + w = %d > 32768 (separators in int32)", name, h + w);
  int32_t* g = at<int32_t>(workspace, layout(n, h, w).lab);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(edt_cols_kernel, dim3(flat_grid((int64_t)n * w, 256)), dim3(256), 0, s, mask, g, n, h, w);
  hipLaunchKernelGGL(edt_rows_kernel, dim3(h, n), dim3(256), (size_t)8 * w, s, g, d2, h, w);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_binary_dilate(const uint8_t* mask, int32_t n, int32_t h, int32_t w, int32_t k, uint8_t* out, void* stream) {
  const char* name = "binary_dilate";
  PRV2_REQUIRE(mask && out, "%s: null pointer", name);
  PRV2_REQUIRE(k == 3 || k == 5 || k == 7, "%s: k = %d (3, 5 or 7)", name, k);
  if (check_frames(name, n, h, w)) return 1;
  const int64_t total = (int64_t)n * h * w;
  hipLaunchKernelGGL(dilate_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, mask, out, n, h, w, k / 2);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_boundary_stats(const uint8_t* gt_edges, const uint8_t* pred_edges, const uint8_t* valid, const int32_t* d2_target,
                                   const int32_t* d2_pred, const uint8_t* gt_ext, const uint8_t* pred_ext, int32_t n, int32_t h, int32_t w,
                                   double th_edges_acc, double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "boundary_stats";
  PRV2_REQUIRE(gt_edges && pred_edges && valid && d2_target && d2_pred && gt_ext && pred_ext && stats, "%s: null pointer", name);
  if (check_frames(name, n, h, w) || check_ws(name, n, h, w, workspace, workspace_bytes)) return 1;
  double* part = at<double>(workspace, layout(n, h, w).part);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(stats_kernel, dim3(kRedBlocks, n), dim3(256), 0, s, gt_edges, pred_edges, valid, d2_target, d2_pred, gt_ext, pred_ext,
                     h, w, th_edges_acc, part);
  hipLaunchKernelGGL(stats_final_kernel, dim3(n), dim3(64), 0, s, part, stats);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
