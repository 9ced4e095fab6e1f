// Motion-compensated temporal stabilisation (include/prv2.h "Temporal motion"): before a frame is aligned to and blended with the
// previous output, that output and its luma are moved by a field of block vectors, so that a pan no longer gates the frame out.  The
// field is an integer block-matching search of the frame's luma against the previous one: bytes and integer sums throughout, which is
// what makes the bits equal temporal.temporal_motion_host.  Per frame that has a state, in order on the stream:
//
//   motion_luma_kernel     the frame's luma from its image and its quarter map Q (4 x 4 means), one thread per quarter pixel
//   motion_quarter_kernel  QP, the quarter map of the previous luma (recomputed every frame: nothing is carried between calls but the
//                          state itself, so the grouping of a sequence into calls cannot show)
//   motion_coarse_kernel   a workgroup owns a tile of 2 x 2 blocks: its window of Q and the window of QP widened by R are staged in
//                          LDS (clamped on load), one wave per block, the lanes across the (2R + 1)^2 candidates, 16 packed-byte SADs
//                          each; the key (S, dy^2 + dx^2, dy, dx) packs into 64 bits and a wave-wide min is the specification's
//                          lexicographic rule
//   motion_refine_kernel   one wave per block: the 3 x 3 vector median, then the 22 x 22 window of P at 4 v^ in LDS (clamped on load)
//                          and the block of L beside it (zero outside the frame); 49 lanes take the 49 candidates, 64 masked packed
//                          SADs each; the key (T, ey^2 + ex^2, ey, ex) packs into 32 bits; T(0, 0) from the block's own pixels
//   motion_warp_kernel     the previous output and luma moved by their block's vector into the workspace (quiet NaN / 0 where the
//                          source leaves the frame)
//   motion_final_kernel    the blocks' records summed into the frame's motion stats row
//
// then the four launches of temporal.hip (temporal_kernels.h) on the warped state.  A frame without a state zeroes its motion row and
// vectors (motion_none_kernel) and runs those four launches as prv2_temporal_step does.  No atomics, nothing allocated or synchronised.
#include "temporal_kernels.h"

namespace prv2 {
namespace {

constexpr int KM = PRV2_TEMPORAL_MOTION_STATS;
static_assert(KM == 8, "layout of prv2_temporal_motion_step's motion stats rows");
constexpr int kB = 16;                // pixels a side of a block
constexpr int kMaxR = 16;             // the largest search range, quarter pixels
constexpr int kTile = 2;              // coarse search: blocks a side of a workgroup's tile, one wave per block
constexpr int kQW = 4 * kTile + 4;    // rows and columns of Q under a tile's windows (an apron of 2 each side)
constexpr int kPW = kQW + 2 * kMaxR;  // the same of QP at the largest range
constexpr int kPStride = 48;          // bytes of a staged row of QP: a multiple of 4, three dwords readable from the last window
constexpr int kWin = kB + 6;          // refinement: rows and columns of the window of P (e in [-3, 3])
constexpr int kWStride = 24;          // bytes of a staged row of it: five dwords readable from byte offset 4
static_assert(kTile * kTile == 4, "one wave of the 256 threads per block of the tile");
static_assert(kPStride >= kPW && ((4 * (kTile - 1) + 2 * kMaxR) / 4 + 3) * 4 <= kPStride && kWStride >= kWin, "staged rows");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// bytes sh / 8 .. sh / 8 + 3 of the eight bytes hi:lo (sh = 0, 8, 16 or 24)
__device__ __forceinline__ uint32_t bytes_at(uint32_t hi, uint32_t lo, int sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh); }

__global__ void __launch_bounds__(256) motion_luma_kernel(TemporalArgs a, uint8_t* __restrict__ Q, int hq, int wq) {
  const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= hq || j >= wq) return;
  const int x0 = 4 * j, last = a.w - 1 - x0;  // (x0 < w)
  int sum = 0;
  for (int r = 0; r < 4; ++r) {
    const int y = min(4 * i + r, a.h - 1);
    int L[4];
    luma4(a, y, x0, L);
    if (4 * i + r < a.h) {
      const int64_t o = (int64_t)y * a.w;
      if (a.vec) {
        *reinterpret_cast<uint32_t*>(a.lcur + o + x0) = (uint32_t)L[0] | (uint32_t)L[1] << 8 | (uint32_t)L[2] << 16 | (uint32_t)L[3] << 24;
      } else {
        for (int k = 0; k < 4; ++k)
          if (k <= last) a.lcur[o + x0 + k] = (uint8_t)L[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += k <= last ? L[k] : last == 0 ? L[0] : last == 1 ? L[1] : L[2];  // columns clamped to w - 1
  }
  Q[(int64_t)i * wq + j] = (uint8_t)((sum + 8) >> 4);
}

__global__ void __launch_bounds__(256) motion_quarter_kernel(const uint8_t* __restrict__ P, int h, int w, uint8_t* __restrict__ QP, int hq, int wq) {
  const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= hq || j >= wq) return;
  int sum = 0;
  for (int r = 0; r < 4; ++r) {
    const uint8_t* row = P + (int64_t)min(4 * i + r, h - 1) * w;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += row[min(4 * j + k, w - 1)];
  }
  QP[(int64_t)i * wq + j] = (uint8_t)((sum + 8) >> 4);
}

__global__ void __launch_bounds__(256) motion_coarse_kernel(const uint8_t* __restrict__ Q, const uint8_t* __restrict__ QP, int hq, int wq, int nby,
                                                            int nbx, int R, int16_t* __restrict__ coarse) {
  __shared__ uint32_t qs[kQW][kQW / 4];
  __shared__ uint32_t ps[kPW][kPStride / 4];
  const int by0 = blockIdx.y * kTile, bx0 = blockIdx.x * kTile;
  const int i0 = 4 * by0 - 2, j0 = 4 * bx0 - 2, pw = kQW + 2 * R;
  uint8_t* qb = reinterpret_cast<uint8_t*>(qs);
  uint8_t* pb = reinterpret_cast<uint8_t*>(ps);
  for (int t = threadIdx.x; t < kQW * kQW; t += 256) {
    const int r = t / kQW, c = t % kQW;
    qb[r * kQW + c] = Q[(int64_t)clampi(i0 + r, 0, hq - 1) * wq + clampi(j0 + c, 0, wq - 1)];
  }
  for (int t = threadIdx.x; t < pw * pw; t += 256) {  // the clamp comes after the displacement: row r is quarter row i0 - R + r
    const int r = t / pw, c = t % pw;
    pb[r * kPStride + c] = QP[(int64_t)clampi(i0 - R + r, 0, hq - 1) * wq + clampi(j0 - R + c, 0, wq - 1)];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ty = wave / kTile, tx = wave % kTile, by = by0 + ty, bx = bx0 + tx;
  if (by >= nby || bx >= nbx) return;  // (behind the only barrier)
  uint32_t q[8][2];  // the block's window of Q: rows 4 ty .. 4 ty + 7 and bytes 4 tx .. 4 tx + 7 of the tile's
#pragma unroll
  for (int r = 0; r < 8; ++r) q[r][0] = qs[4 * ty + r][tx], q[r][1] = qs[4 * ty + r][tx + 1];
  auto sad_at = [&](int dy, int dx) -> uint32_t {
    const int o = 4 * tx + dx + R, sh = 8 * (o & 3);
    const uint32_t* row = &ps[4 * ty + dy + R][o >> 2];
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r, row += kPStride / 4) {
      const uint32_t w0 = row[0], w1 = row[1], w2 = row[2];
      s = __builtin_amdgcn_sad_u8(q[r][0], bytes_at(w1, w0, sh), s);
      s = __builtin_amdgcn_sad_u8(q[r][1], bytes_at(w2, w1, sh), s);
    }
    return s;
  };
  const int n = 2 * R + 1;
  unsigned long long best = ~0ull;  // (S, dy^2 + dx^2, dy + 16, dx + 16) in 32 + 10 + 6 + 6 bits
  for (int k = lane; k < n * n; k += 64) {
    const int dy = k / n - R, dx = k % n - R;
    const unsigned long long key = (unsigned long long)sad_at(dy, dx) << 32 | (unsigned long long)((dy * dy + dx * dx) << 12 | (dy + 16) << 6 | (dx + 16));
    best = key < best ? key : best;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other < best ? other : best;
  }
  const uint32_t s0 = sad_at(0, 0);
  if (lane == 0) {
    const bool take = (uint32_t)(best >> 32) + 64u < s0;
    int16_t* v = coarse + ((int64_t)by * nbx + bx) * 2;
    v[0] = take ? (int16_t)((int)((best >> 6) & 63) - 16) : (int16_t)0;
    v[1] = take ? (int16_t)((int)(best & 63) - 16) : (int16_t)0;
  }
}

// the fifth smallest of nine
__device__ __forceinline__ int median9(const int* v) {
  int m = v[0];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
    if (rank == 4) m = v[i];
  }
  return m;
}

// info: per block my, mx, T(m) (T(0, 0) for a zeroed block), T(0, 0)
__global__ void __launch_bounds__(256) motion_refine_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ P, int h, int w, int nby, int nbx,
                                                            const int16_t* __restrict__ coarse, int16_t* __restrict__ vec, int32_t* __restrict__ info) {
  __shared__ uint32_t win[4][kWin][kWStride / 4];
  __shared__ uint32_t cur[4][kB][kB / 4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + wave;
  const bool live = blk < nby * nbx;
  const int by = live ? blk / nbx : 0, bx = live ? blk % nbx : 0, y0 = kB * by, x0 = kB * bx;
  int cy = 0, cx = 0;
  if (live) {
    int vy[9], vx[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int16_t* c = coarse + ((int64_t)clampi(by + k / 3 - 1, 0, nby - 1) * nbx + clampi(bx + k % 3 - 1, 0, nbx - 1)) * 2;
      vy[k] = c[0], vx[k] = c[1];
    }
    cy = 4 * median9(vy), cx = 4 * median9(vx);
    uint8_t* wb = reinterpret_cast<uint8_t*>(win[wave]);
    for (int t = lane; t < kWin * kWin; t += 64) {
      const int r = t / kWin, c = t % kWin;
      wb[r * kWStride + c] = P[(int64_t)clampi(y0 + cy - 3 + r, 0, h - 1) * w + clampi(x0 + cx - 3 + c, 0, w - 1)];
    }
    uint8_t* cb = reinterpret_cast<uint8_t*>(cur[wave]);
    for (int t = lane; t < kB * kB; t += 64) {
      const int y = y0 + (t >> 4), x = x0 + (t & 15);
      cb[t] = y < h && x < w ? L[(int64_t)y * w + x] : (uint8_t)0;
    }
  }
  __syncthreads();
  if (!live) return;
  const int rows = min(kB, h - y0), cols = min(kB, w - x0), npix = rows * cols;
  uint32_t t0;  // T(0, 0): a lane takes four pixels of the block itself (no index leaves the frame)
  {
    const int r = lane >> 2, c0 = 4 * (lane & 3);
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(cur[wave]);
    int s = 0;
    for (int k = 0; k < 4; ++k)
      if (r < rows && c0 + k < cols) s += abs((int)cb[r * kB + c0 + k] - (int)P[(int64_t)(y0 + r) * w + x0 + c0 + k]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    t0 = (uint32_t)s;
  }
  uint32_t mask[4];  // the block's columns inside the frame
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int in = clampi(cols - 4 * q, 0, 4);
    mask[q] = in == 4 ? 0xFFFFFFFFu : (1u << (8 * in)) - 1u;
  }
  const bool cand = lane < 49;
  const int ey = cand ? lane / 7 - 3 : 0, ex = cand ? lane % 7 - 3 : 0;
  const int o = ex + 3, sh = 8 * (o & 3);
  uint32_t T = 0;
  for (int r = 0; r < rows; ++r) {
    const uint32_t* row = &win[wave][r + ey + 3][o >> 2];
    const uint32_t* c = cur[wave][r];
    const uint32_t w0 = row[0], w1 = row[1], w2 = row[2], w3 = row[3], w4 = row[4];
    T = __builtin_amdgcn_sad_u8(c[0], bytes_at(w1, w0, sh) & mask[0], T);
    T = __builtin_amdgcn_sad_u8(c[1], bytes_at(w2, w1, sh) & mask[1], T);
    T = __builtin_amdgcn_sad_u8(c[2], bytes_at(w3, w2, sh) & mask[2], T);
    T = __builtin_amdgcn_sad_u8(c[3], bytes_at(w4, w3, sh) & mask[3], T);
  }
  uint32_t best = cand ? T << 11 | (uint32_t)((ey * ey + ex * ex) << 6 | (ey + 3) << 3 | (ex + 3)) : ~0u;  // T <= 65280: 27 bits
  for (int s = 32; s > 0; s >>= 1) {
    const uint32_t other = __shfl_xor(best, s, 64);
    best = other < best ? other : best;
  }
  if (lane == 0) {
    const uint32_t tw = best >> 11;
    const bool take = tw + (uint32_t)npix < t0;
    const int my = take ? cy + (int)((best >> 3) & 7) - 3 : 0, mx = take ? cx + (int)(best & 7) - 3 : 0;
    vec[(int64_t)blk * 2] = (int16_t)my, vec[(int64_t)blk * 2 + 1] = (int16_t)mx;
    int32_t* rec = info + (int64_t)blk * 4;
    rec[0] = my, rec[1] = mx, rec[2] = (int32_t)(take ? tw : t0), rec[3] = (int32_t)t0;
  }
}

// a block owns kRows rows x kCols columns and a thread a quad of columns, as in the stabiliser's passes; a quad lies in one 16 x 16 block
__global__ void __launch_bounds__(256) motion_warp_kernel(const float* __restrict__ prev, const uint8_t* __restrict__ P, const int16_t* __restrict__ vec,
                                                          int h, int w, int nbx, int vecw, float* __restrict__ yw, uint8_t* __restrict__ Pw) {
  const int x0 = blockIdx.x * kCols + (int)threadIdx.x * 4, r0 = blockIdx.y * kRows;
  if (x0 >= w) return;
  for (int r = 0; r < kRows; ++r) {
    const int y = r0 + r;
    if (y >= h) break;
    const int16_t* m = vec + ((int64_t)(y / kB) * nbx + x0 / kB) * 2;
    const int sy = y + m[0], sx0 = x0 + m[1];
    float v[4];
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int sx = sx0 + k;
      const bool ok = sy >= 0 && sy < h && sx >= 0 && sx < w && x0 + k < w;
      v[k] = ok ? prev[(int64_t)sy * w + sx] : __uint_as_float(0x7FC00000u);
      p[k] = ok ? P[(int64_t)sy * w + sx] : 0u;
    }
    const int64_t o = (int64_t)y * w;
    store4(yw + o, x0, w, vecw, v);
    if (vecw) {
      *reinterpret_cast<uint32_t*>(Pw + o + x0) = p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24;
    } else {
      for (int k = 0; k < 4; ++k)
        if (x0 + k < w) Pw[o + x0 + k] = (uint8_t)p[k];
    }
  }
}

// row: 0 blocks, 1 blocks with m != 0, 2 sum my, 3 sum mx, 4 sum |my| + |mx|, 5 max(|my|, |mx|), 6 sum T(m), 7 sum T(0, 0)
__global__ void __launch_bounds__(256) motion_final_kernel(const int32_t* __restrict__ info, int nb, int64_t* __restrict__ row) {
  __shared__ long long sh[4][7];
  long long acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nb; b += 256) {
    const int32_t* rec = info + (int64_t)b * 4;
    const int my = rec[0], mx = rec[1];
    const long long big = max(abs(my), abs(mx));
    acc[0] += (my | mx) != 0 ? 1 : 0, acc[1] += my, acc[2] += mx, acc[3] += abs(my) + abs(mx);
    acc[4] = big > acc[4] ? big : acc[4];
    acc[5] += rec[2], acc[6] += rec[3];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    long long v = acc[j];
    for (int o = 32; o > 0; o >>= 1) {
      const long long u = __shfl_down(v, o, 64);
      v = j == 4 ? (u > v ? u : v) : v + u;
    }
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int j = threadIdx.x;
    long long v = sh[0][j];
    for (int k = 1; k < 4; ++k) v = j == 4 ? (sh[k][j] > v ? sh[k][j] : v) : v + sh[k][j];
    row[1 + j] = v;
  }
  if (threadIdx.x == 7) row[0] = nb;
}

// a frame whose motion stage does not run (no state): its row and its vectors are zero
__global__ void __launch_bounds__(256) motion_none_kernel(int64_t* __restrict__ row, int16_t* __restrict__ vec, int nb) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < KM) row[t] = 0;
  if (vec != nullptr && t < 2 * nb) vec[t] = 0;
}

// the workspace: the stabiliser's partials, then the warped state, the quarter maps and the blocks' records, each 16-byte aligned
struct MotionLayout {
  int64_t part, yw, pw, q, qp, coarse, vec, info, total;
  int hq, wq, nby, nbx, nb;
};
static inline MotionLayout motion_layout(int h, int w) {
  MotionLayout m;
  m.hq = (int)cdiv(h, 4), m.wq = (int)cdiv(w, 4), m.nby = (int)cdiv(h, kB), m.nbx = (int)cdiv(w, kB), m.nb = m.nby * m.nbx;
  const int64_t hw = (int64_t)h * w, hwq = (int64_t)m.hq * m.wq;
  int64_t o = 0;
  auto take = [&o](int64_t bytes) { const int64_t at = o; o += roundup(bytes, 16); return at; };
  m.part = take(temporal_blocks(h, w) * kPart * (int64_t)sizeof(int64_t));
  m.yw = take(hw * 4), m.pw = take(hw), m.q = take(hwq), m.qp = take(hwq);
  m.coarse = take((int64_t)m.nb * 4), m.vec = take((int64_t)m.nb * 4), m.info = take((int64_t)m.nb * 16);
  m.total = o;
  return m;
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_temporal_motion_workspace_bytes(int32_t h, int32_t w) {
  if (h < 1 || w < 1 || (int64_t)h * w > kMaxPixels || cdiv(h, kRows) > 65535) return -1;
  return motion_layout(h, w).total;
}

extern "C" int prv2_temporal_motion_step(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, double alpha,
                                         int32_t tau, double rho, double anchor, int32_t motion_range, float* state_depth, uint8_t* luma0,
                                         uint8_t* luma1, int32_t state_present, float* out, int64_t* stats, int64_t* motion_stats, int16_t* vectors,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "temporal_motion_step";
  PRV2_REQUIRE(depth && image && state_depth && luma0 && luma1 && out && stats && motion_stats, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w <= kMaxPixels, "%s: a frame of %d x %d exceeds 2^25 pixels (the bound of the exact int64 sums)", name, h, w);
  PRV2_REQUIRE(cdiv(h, kRows) <= 65535, "%s: %d rows exceed the grid (%d)", name, h, 65535 * kRows);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX, "%s: %d frames of %d x %d exceed 2^31 pixels", name, n, h, w);
  PRV2_REQUIRE(ih >= 1 && iw >= 1 && (int64_t)n * 3 * ih * iw < (int64_t)INT_MAX, "%s: bad image shape %d x %d", name, ih, iw);
  PRV2_REQUIRE(alpha >= 0.0 && alpha < 1.0, "%s: alpha %g outside [0, 1)", name, alpha);
  PRV2_REQUIRE(tau >= 0 && tau <= 255, "%s: tau %d outside 0 .. 255", name, tau);
  PRV2_REQUIRE(rho > 0.0 && rho < (double)INFINITY, "%s: rho %g must be positive and finite", name, rho);
  PRV2_REQUIRE(anchor >= 0.0 && anchor <= 1.0, "%s: anchor %g outside [0, 1]", name, anchor);
  PRV2_REQUIRE(motion_range >= 1 && motion_range <= kMaxR, "%s: motion_range %d outside 1 .. %d", name, motion_range, kMaxR);
  PRV2_REQUIRE(state_present == 0 || state_present == 1, "%s: state_present %d: 0 or 1", name, state_present);
  PRV2_REQUIRE(luma0 != luma1, "%s: the two luma buffers must differ (the search reads the previous luma beside the new one)", name);
  PRV2_REQUIRE(out != depth && state_depth != depth, "%s: out and the state must not alias the input map", name);
  PRV2_REQUIRE(aligned(depth, 4) && aligned(image, 4) && aligned(state_depth, 4) && aligned(out, 4), "%s: misaligned fp32 pointer", name);
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 8) && aligned(stats, 8) && aligned(motion_stats, 8) && aligned(vectors, 2),
               "%s: null or misaligned workspace / stats / vectors", name);
  const MotionLayout m = motion_layout(h, w);
  PRV2_REQUIRE(workspace_bytes >= m.total, "%s: workspace of %lld bytes < %lld (prv2_temporal_motion_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)m.total);
  const int64_t hw = (int64_t)h * w;
  const int nblk = (int)temporal_blocks(h, w);
  const long long min_count = hw / 100 > 64 ? hw / 100 : 64;
  char* ws = (char*)workspace;
  int64_t* part = (int64_t*)(ws + m.part);
  float* yw = (float*)(ws + m.yw);
  uint8_t *pw = (uint8_t*)(ws + m.pw), *q = (uint8_t*)(ws + m.q), *qp = (uint8_t*)(ws + m.qp);
  int16_t* coarse = (int16_t*)(ws + m.coarse);
  int32_t* info = (int32_t*)(ws + m.info);
  uint8_t* luma[2] = {luma0, luma1};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(w, kCols), (unsigned)cdiv(h, kRows)), block(256);
  const dim3 qgrid((unsigned)cdiv(m.wq, 64), (unsigned)cdiv(m.hq, 4)), qblock(64, 4);
  TemporalArgs a;
  a.h = h, a.w = w, a.ih = ih, a.iw = iw, a.tau = tau;
  a.vec = w % 4 == 0 && aligned(depth, 16) && aligned(state_depth, 16) && aligned(out, 16) && aligned(luma0, 4) && aligned(luma1, 4) &&
          aligned(yw, 16) && aligned(pw, 4);
  a.vimg = a.vec && ih == h && iw == w && aligned(image, 16);
  const int vecw = w % 4 == 0 && aligned(yw, 16) && aligned(pw, 4);
  for (int f = 0; f < n; ++f) {  // a chain: frame f reads the output of frame f - 1
    a.x = depth + f * hw;
    a.image = image + (int64_t)f * 3 * ih * iw;
    a.has_prev = f == 0 ? state_present : 1;
    const float* prev = f == 0 ? state_depth : out + (f - 1) * hw;
    a.lcur = luma[(f + 1) & 1];
    a.out = out + f * hw;
    a.state = f == n - 1 && out + f * hw != state_depth ? state_depth : nullptr;
    int64_t* row = stats + (int64_t)f * K;
    int64_t* mrow = motion_stats + (int64_t)f * KM;
    int16_t* vec = vectors ? vectors + (int64_t)f * m.nb * 2 : (int16_t*)(ws + m.vec);
    if (a.has_prev) {
      const uint8_t* lprev = luma[f & 1];
      hipLaunchKernelGGL(motion_luma_kernel, qgrid, qblock, 0, s, a, q, m.hq, m.wq);
      hipLaunchKernelGGL(motion_quarter_kernel, qgrid, qblock, 0, s, lprev, h, w, qp, m.hq, m.wq);
      hipLaunchKernelGGL(motion_coarse_kernel, dim3((unsigned)cdiv(m.nbx, kTile), (unsigned)cdiv(m.nby, kTile)), block, 0, s, (const uint8_t*)q,
                         (const uint8_t*)qp, m.hq, m.wq, m.nby, m.nbx, motion_range, coarse);
      hipLaunchKernelGGL(motion_refine_kernel, dim3((unsigned)cdiv(m.nb, 4)), block, 0, s, (const uint8_t*)a.lcur, lprev, h, w, m.nby, m.nbx,
                         (const int16_t*)coarse, vec, info);
      hipLaunchKernelGGL(motion_warp_kernel, grid, block, 0, s, prev, lprev, (const int16_t*)vec, h, w, m.nbx, vecw, yw, pw);
      hipLaunchKernelGGL(motion_final_kernel, dim3(1), block, 0, s, (const int32_t*)info, m.nb, mrow);
      a.prev = yw, a.lprev = pw;
    } else {
      hipLaunchKernelGGL(motion_none_kernel, dim3((unsigned)cdiv(vectors ? 2 * m.nb > KM ? 2 * m.nb : KM : KM, 256)), block, 0, s, mrow,
                         vectors ? vec : (int16_t*)nullptr, m.nb);
      a.prev = prev, a.lprev = luma[f & 1];
    }
    hipLaunchKernelGGL(temporal_fit_kernel, grid, block, 0, s, a, part);
    hipLaunchKernelGGL(temporal_fit_final_kernel, dim3(1), block, 0, s, (const int64_t*)part, nblk, min_count, anchor, row);
    hipLaunchKernelGGL(temporal_apply_kernel, grid, block, 0, s, a, (const int64_t*)row, alpha, rho, part);
    hipLaunchKernelGGL(temporal_sum_final_kernel, dim3(1), block, 0, s, (const int64_t*)part, nblk, row);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
