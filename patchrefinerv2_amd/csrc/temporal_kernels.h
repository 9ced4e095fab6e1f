// The kernels of the temporal stabiliser (temporal.hip has the description), shared with the motion-compensated step (motion.hip),
// which runs the same four launches on a warped state.  Everything sits in an unnamed namespace: each file gets its own copy.
#pragma once
#include <limits.h>
#include <math.h>

#include "evalgt_terms.h"

namespace prv2 {
namespace {

constexpr int kRows = 8;     // rows a block owns
constexpr int kCols = 1024;  // columns a block owns: 256 threads x one quad
constexpr int kPart = 6;     // int64 partials per block: n, n_gate, sum qx, sum qx^2, sum qx qy, sum qy (the apply pass uses two)
constexpr int K = PRV2_TEMPORAL_STATS;
static_assert(K == 12, "layout of prv2_temporal_step's stats rows");
constexpr float kQ = 256.0f;         // fixed point per metre
constexpr float kQCap = 262144.0f;   // 2^18
constexpr int kMaxPixels = 1 << 25;  // (2^18)^2 * 2^25 < 2^63

struct TemporalArgs {
  const float* x;        // the frame's map [h, w]
  const float* prev;     // the previous output [h, w] (not read without has_prev)
  const uint8_t* lprev;  // the previous luma [h, w]
  uint8_t* lcur;         // the frame's luma [h, w]: written by the fit pass, read by the apply pass
  const float* image;    // the frame's image [3, ih, iw]
  float* out;            // the frame's output [h, w]
  float* state;          // the state map, written as well by a call's last frame (else null)
  int h, w, ih, iw;
  int vec;       // w % 4 == 0 and every map 16-byte, every luma buffer 4-byte aligned
  int vimg;      // vec, and the image has the map's size and is 16-byte aligned: its quad is three 16-byte loads
  int has_prev;  // there is a previous output of this shape
  int tau;
};

__device__ __forceinline__ bool valid(float v) { return v > 0.0f && v < INFINITY; }  // finite and > 0 (false for a NaN)

// "Geometry export" byte: clamp(rint(v), 0, 255), ties to even, NaN -> 0
__device__ __forceinline__ int colour_byte(float v) {
  const float r = rintf(v);
  return !(r > 0.0f) ? 0 : r >= 255.0f ? 255 : (int)r;
}
__device__ __forceinline__ int luma_of(float r, float g, float b) {
  return (77 * colour_byte(__fmul_rn(r, 255.0f)) + 150 * colour_byte(__fmul_rn(g, 255.0f)) + 29 * colour_byte(__fmul_rn(b, 255.0f)) + 128) >> 8;
}

// the luma of the quad x0 .. x0 + 3 of row y (0 behind the row's end): the image sampled as prv2_pointcloud_pack samples it
__device__ __forceinline__ void luma4(const TemporalArgs& a, int y, int x0, int* L) {
  const int64_t plane = (int64_t)a.ih * a.iw;
  if (a.vimg) {
    const float* c = a.image + (int64_t)y * a.w + x0;
    const float4 r = *reinterpret_cast<const float4*>(c), g = *reinterpret_cast<const float4*>(c + plane),
                 b = *reinterpret_cast<const float4*>(c + 2 * plane);
    L[0] = luma_of(r.x, g.x, b.x), L[1] = luma_of(r.y, g.y, b.y), L[2] = luma_of(r.z, g.z, b.z), L[3] = luma_of(r.w, g.w, b.w);
  } else {
    const int sy = (int)(((int64_t)(2 * y + 1) * a.ih) / (2 * (int64_t)a.h));
    const float* row = a.image + (int64_t)sy * a.iw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      L[k] = 0;
      if (x < a.w) {
        const float* c = row + (int)(((int64_t)(2 * x + 1) * a.iw) / (2 * (int64_t)a.w));
        L[k] = luma_of(c[0], c[plane], c[2 * plane]);
      }
    }
  }
}

// four luma bytes of a row per thread (one 4-byte load when the rows are aligned), zero behind the row's end
__device__ __forceinline__ void load4_u8(const uint8_t* __restrict__ row, int x0, int w, int vec, int* v) {
  if (vec) {
    const uint32_t t = *reinterpret_cast<const uint32_t*>(row + x0);
    v[0] = t & 255, v[1] = (t >> 8) & 255, v[2] = (t >> 16) & 255, v[3] = t >> 24;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = x0 + k < w ? row[x0 + k] : 0;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ row, int x0, int w, int vec, const float* v) {
  if (vec) {
    *reinterpret_cast<float4*>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; ++k)
      if (x0 + k < w) row[x0 + k] = v[k];
  }
}

// the gate of a pixel: the luma moved by at most tau and both depths are valid
__device__ __forceinline__ bool gate(int L, int Lp, int tau, float x, float p) { return abs(L - Lp) <= tau && valid(x) && valid(p); }

// rint(65536 * min(1, |v - p| / p)) of a gated pixel (p valid); a NaN ratio counts as 1
__device__ __forceinline__ int64_t change_term(float v, float p) {
  const double P = (double)p;
  const double c = fabs((double)v - P) / P;
  return (int64_t)rint(65536.0 * (c < 1.0 ? c : 1.0));
}

// NV int64 sums of a block: shuffles inside a wave, the four waves through LDS -> part[block][0 .. NV)
template <int NV>
__device__ __forceinline__ void block_sums(long long* acc, long long (*sh)[NV], int64_t* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    long long v = acc[j];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int j = threadIdx.x;
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[blk * kPart + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
  }
}

__global__ void __launch_bounds__(256) temporal_fit_kernel(TemporalArgs a, int64_t* __restrict__ part) {
  __shared__ long long sh[4][kPart];
  long long acc[kPart];
#pragma unroll
  for (int j = 0; j < kPart; ++j) acc[j] = 0;
  const int w = a.w, r0 = blockIdx.y * kRows;
  const int x0 = blockIdx.x * kCols + (int)threadIdx.x * 4;
  if (x0 < w) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int y = r0 + r;
      if (y >= a.h) break;
      const int64_t o = (int64_t)y * w;
      int L[4];
      luma4(a, y, x0, L);
      if (a.vec) {
        *reinterpret_cast<uint32_t*>(a.lcur + o + x0) = (uint32_t)L[0] | (uint32_t)L[1] << 8 | (uint32_t)L[2] << 16 | (uint32_t)L[3] << 24;
      } else {
        for (int k = 0; k < 4; ++k)
          if (x0 + k < w) a.lcur[o + x0 + k] = (uint8_t)L[k];
      }
      if (!a.has_prev) continue;
      float xv[4], pv[4];
      int Lp[4];
      load4(a.x + o, x0, w, a.vec, xv);  // (zero behind the row's end: not valid)
      load4(a.prev + o, x0, w, a.vec, pv);
      load4_u8(a.lprev + o, x0, w, a.vec, Lp);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!gate(L[k], Lp[k], a.tau, xv[k], pv[k])) continue;
        acc[1] += 1;
        const float qx = rintf(__fmul_rn(xv[k], kQ)), qy = rintf(__fmul_rn(pv[k], kQ));
        const double P = (double)pv[k];
        if (qx >= 1.0f && qx < kQCap && qy >= 1.0f && qy < kQCap && fabs((double)xv[k] - P) <= 0.5 * P) {
          const long long ix = (long long)qx, iy = (long long)qy;
          acc[0] += 1, acc[2] += ix, acc[3] += ix * ix, acc[4] += ix * iy, acc[5] += iy;
        }
      }
    }
  }
  block_sums<kPart>(acc, sh, part);
}

// sums NV partial columns of nblk blocks into sums[0 .. NV) (LDS), every thread of the 256 takes every 256th block
template <int NV>
__device__ __forceinline__ void final_sums(const int64_t* __restrict__ part, int nblk, long long (*sh)[NV], long long* sums) {
  long long acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0;
  for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] += part[(int64_t)b * kPart + j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    long long v = acc[j];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV) sums[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
  __syncthreads();
}

// row: 0 reset, 1 n, 2 n_gate, 3 .. 6 the sums of qx, qx^2, qx qy, qy, 9 s, 10 b (float64 bits), 11 fitted
__global__ void __launch_bounds__(256) temporal_fit_final_kernel(const int64_t* __restrict__ part, int nblk, long long min_count, double anchor,
                                                                 int64_t* __restrict__ row) {
  __shared__ long long sh[4][kPart];
  __shared__ long long sums[kPart];
  final_sums<kPart>(part, nblk, sh, sums);
  if (threadIdx.x != 0) return;
  const long long n = sums[0];
  const bool reset = n < min_count;  // no previous output, or a scene cut
  double s = 1.0, b = 0.0;
  long long fitted = 0;
  if (!reset) {  // compute_scale_and_shift's normal equations (losses.py:537-542): the new frame is the prediction
    const double a00 = (double)sums[3], a01 = (double)sums[2], a11 = (double)n, b0 = (double)sums[4], b1 = (double)sums[5];
    const double det = __dadd_rn(__dmul_rn(a00, a11), -__dmul_rn(a01, a01));
    if (det > 0.0) {  // (false for a NaN too)
      const double sf = __dadd_rn(__dmul_rn(a11, b0), -__dmul_rn(a01, b1)) / det;
      const double bf = (__dadd_rn(__dmul_rn(a00, b1), -__dmul_rn(a01, b0)) / det) / 256.0;
      if (sf >= 0.5 && sf <= 2.0 && fabs(bf) < (double)INFINITY) {
        s = __dadd_rn(1.0, __dmul_rn(anchor, sf - 1.0));
        b = __dmul_rn(anchor, bf);
        fitted = 1;
      }
    }
  }
  row[0] = reset ? 1 : 0;
  row[1] = n, row[2] = sums[1], row[3] = sums[2], row[4] = sums[3], row[5] = sums[4], row[6] = sums[5];
  row[9] = __double_as_longlong(s), row[10] = __double_as_longlong(b), row[11] = fitted;
}

__global__ void __launch_bounds__(256) temporal_apply_kernel(TemporalArgs a, const int64_t* __restrict__ row, double alpha, double rho,
                                                             int64_t* __restrict__ part) {
  __shared__ long long sh[4][2];
  long long acc[2] = {0, 0};
  const bool reset = row[0] != 0;
  const double s = __longlong_as_double(row[9]), b = __longlong_as_double(row[10]);
  const int w = a.w, r0 = blockIdx.y * kRows;
  const int x0 = blockIdx.x * kCols + (int)threadIdx.x * 4;
  if (x0 < w) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int y = r0 + r;
      if (y >= a.h) break;
      const int64_t o = (int64_t)y * w;
      float xv[4], pv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4];
      int L[4] = {0, 0, 0, 0}, Lp[4] = {0, 0, 0, 0};
      load4(a.x + o, x0, w, a.vec, xv);
      if (a.has_prev) {
        load4(a.prev + o, x0, w, a.vec, pv);
        load4_u8(a.lcur + o, x0, w, a.vec, L);
        load4_u8(a.lprev + o, x0, w, a.vec, Lp);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x = xv[k], p = pv[k];
        const bool g = a.has_prev && gate(L[k], Lp[k], a.tau, x, p);
        float v = x;
        if (!reset) {
          if (valid(x)) {
            const float al = (float)__dadd_rn(__dmul_rn(s, (double)x), b);
            if (valid(al)) v = al;
          }
          if (g) {
            const double A = (double)v, P = (double)p;
            const double q = ((A - P) / (A < P ? A : P)) / rho;
            const double wt = alpha / __dadd_rn(1.0, __dmul_rn(q, q));
            v = (float)__dadd_rn(A, __dmul_rn(wt, P - A));
          }
        }
        ov[k] = v;
        if (g) acc[0] += change_term(x, p), acc[1] += change_term(v, p);
      }
      store4(a.out + o, x0, w, a.vec, ov);
      if (a.state) store4(a.state + o, x0, w, a.vec, ov);
    }
  }
  block_sums<2>(acc, sh, part);
}

// row: 7 change_before, 8 change_after (sums of 65536ths over the gated pixels)
__global__ void __launch_bounds__(256) temporal_sum_final_kernel(const int64_t* __restrict__ part, int nblk, int64_t* __restrict__ row) {
  __shared__ long long sh[4][2];
  __shared__ long long sums[2];
  final_sums<2>(part, nblk, sh, sums);
  if (threadIdx.x < 2) row[7 + threadIdx.x] = sums[threadIdx.x];
}

static inline int64_t temporal_blocks(int h, int w) { return cdiv(h, kRows) * cdiv(w, kCols); }

}  // namespace
}  // namespace prv2
