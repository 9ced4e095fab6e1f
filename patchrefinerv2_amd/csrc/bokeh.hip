// Depth-of-field export (include/prv2.h "Depth-of-field export"): a frame re-rendered with a thin lens focused at one distance, from its
// metric depth map.  Every output pixel gathers the sources of a (2 R + 1)^2 window, R = ceil(max_radius), each weighted by how much of
// its own circle of confusion (or the output pixel's, when the source lies behind it with the larger circle) reaches the output pixel.
//
// Arithmetic contract (the numpy restatement is output.py: bokeh_render_host / bokeh_image_host; bit for bit):
//   - the file is built with -ffp-contract=off and every rounded fp32 operation is written with __f*_rn, in the order of the header's
//     table: per source iz = 1 / Z, r = min(Rm, k |iz - 1 / Zf|), m = max(r, 0.5), ia = 1 / (m m); per tap cov = clamp((me + 0.5) - dist,
//     0, 1), wgt = cov ie, sw += wgt, sc += wgt c (a multiply, then an add); at the end sc / sw.  The divisions are __fdiv_rn (v_rcp_f32 is
//     not correctly rounded), dist = the correctly rounded fp32 square root of dx dx + dy dy (sqrt_rn_int below), once per workgroup into an
//     LDS table (the square root of an integer below 2^24 rounds to the same fp32 value from float64, the host's route, as directly);
//   - the taps are summed in raster order of the window (dy outer, dx inner), the order the specification visits them in.
//   - A TAP OF WEIGHT 0 CHANGES NO BIT: wgt is never negative or NaN, x + 0 = x and x + 0 * c = x for every finite c (sc never is -0).
//     So host and kernel may both bound their loops by the largest m in reach: with s = fl(M + 0.5), M the largest m of the tile and
//     its halo of R, an offset with max(|dx|, |dy|) >= ceil(s) has dist >= s >= fl(me + 0.5), hence cov = 0.  This is what makes tiling
//     legal: a tile walks Rt = ceil(s) - 1 <= R instead of R (0 where everything in reach is in focus: a copy), sources off the frame
//     or outside the walked window are weight-0 taps, and skipping them equals adding them.
//
// Shape: a workgroup of 256 lanes owns a tile of 64 x 16 outputs: lane l of wave v owns column l of rows 4 v .. 4 v + 3 and keeps their
// four running sums in registers.  The source rows the tile reaches stream through LDS in bands of 16 rows x (64 + 2 Rt) columns, three
// 8-byte words per source ((zk, r), (ia, red), (green, blue): ds_read_b64, 64 consecutive lanes, conflict-free); one source read feeds
// the four outputs of the lane.  dist is the same for every lane at a tap: a lane holds column `lane` of the table's row |dy| and the
// tap takes it with v_readlane.  LDS: 3 x 16 x 128 x 8 = 48 KiB of band + 4.3 KiB of table (three workgroups per CU at any radius up
// to the cap, kBokehMaxRadius = 32, which only sets the band's pitch of 64 + 2 x 32 columns).
#include "scene.h"

namespace prv2 {
namespace {

constexpr int kBokehMaxRadius = 32;                  // the cap of ceil(max_radius): the band's pitch is kTW + 2 * kBokehMaxRadius
constexpr int kTW = 64, kTH = 16, kPix = 4;          // the tile; rows of a lane (kTH = 4 waves * kPix)
constexpr int kBand = 16;                            // source rows per band
constexpr int kPitch = kTW + 2 * kBokehMaxRadius;    // 128
constexpr int kDistPitch = kBokehMaxRadius + 1;      // 33

int g_tile_bound = 1;  // prv2_bokeh_tile_bound: 0 walks the full window in every tile (measurement only; same bits)

struct BokehArgs {
  const float* depth;  // [n, h, w]
  ImageSrc img;        // [n, 3, ih, iw]
  float k;             // fx * aperture * 0.5
  float focus;         // > 0: the focus distance; else the focus pixel's depth
  float rm;            // max_radius
  Camera cam;          // (the kernel reads its depth range; fx is in k)
  int32_t h, w;
  int32_t fy, fx;      // the focus pixel
  int32_t R;           // ceil(max_radius)
  int32_t bound;       // per-tile walk bound on
  float* out;          // float mode: [n, 3, h, w]
  uint8_t* rows;       // rows mode: scanlines of [h][1 + 3 w]
  int64_t rows_fstride;
  float* focus_out;    // [n]
};

PRV2_NO_PACKED_FP32_BEGIN

// The runtime headers' small helpers (__syncthreads, atomicMax, __float_as_int, make_float2) lack the attribute above and would be CALLED
// from a function that has it, not inlined (the Makefile's note on conv3x3_gate): these are their bodies, under the attribute.
struct alignas(8) Pair {
  float x, y;
};
__device__ __forceinline__ Pair pair(float x, float y) { return Pair{x, y}; }
__device__ __forceinline__ int f2i(float v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ float i2f(int v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the circle of confusion of a depth, in pixels.  flat: the focus pixel is invalid and every radius is 0
__device__ __forceinline__ float bokeh_radius(const BokehArgs& a, float z, float invf, bool flat) {
  if (flat) return 0.0f;
  const float iz = valid_z(a.cam, z) ? __fdiv_rn(1.0f, z) : 0.0f;
  return fminf(a.rm, __fmul_rn(a.k, fabsf(__fsub_rn(iz, invf))));  // (fminf: a NaN product gives Rm)
}

// float32(sqrt(n)) of an integer 0 <= n < 2^24, correctly rounded (__fsqrt_rn compiles to the bare v_sqrt_f32 here: 1 ulp).  The hardware's
// value is one step at most from the answer, and the answer is the float whose two rounding boundaries (25-bit numbers: their squares
// are exact in float64) enclose n.  No tie exists: sqrt(n) is an integer or irrational.
__device__ __forceinline__ float sqrt_rn_int(int n) {
  if (n == 0) return 0.0f;
  float y = __builtin_amdgcn_sqrtf((float)n);
  const float up = i2f(f2i(y) + 1), dn = i2f(f2i(y) - 1);
  const double hi = ((double)y + (double)up) * 0.5, lo = ((double)y + (double)dn) * 0.5;
  if (hi * hi < (double)n) y = up;
  if (lo * lo > (double)n) y = dn;
  return y;
}

__device__ __forceinline__ float finite_or_zero(float c) { return fabsf(c) < __builtin_inff() ? c : 0.0f; }

struct BokehPixel {
  float zk, r, h, ia;  // h = m + 0.5
  float sw, sc[3];
};

// one tap: source (zq, rq, hq, iq, colour c) at distance d of pixel p
__device__ __forceinline__ void bokeh_tap(BokehPixel& p, float zq, float rq, float hq, float iq, float c0, float c1, float c2, float d) {
  const bool own = zq <= p.zk || rq <= p.r;
  const float he = own ? hq : p.h, ie = own ? iq : p.ia;
  const float cov = fminf(fmaxf(__fsub_rn(he, d), 0.0f), 1.0f);
  const float wgt = __fmul_rn(cov, ie);
  p.sw = __fadd_rn(p.sw, wgt);
  p.sc[0] = __fadd_rn(p.sc[0], __fmul_rn(wgt, c0));
  p.sc[1] = __fadd_rn(p.sc[1], __fmul_rn(wgt, c1));
  p.sc[2] = __fadd_rn(p.sc[2], __fmul_rn(wgt, c2));
}

// ROWS: write the PNG scanlines, else the fp32 planes
template <bool ROWS>
__global__ void __launch_bounds__(256) bokeh_kernel(BokehArgs a) {
  __shared__ Pair s_zr[kBand * kPitch];  // (zk, r); r = -1 off the frame (the source's own disc, weight 0).  Later the scanline bytes
  __shared__ Pair s_ic[kBand * kPitch];  // (ia, red)
  __shared__ Pair s_gb[kBand * kPitch];  // (green, blue)
  __shared__ float s_dist[kDistPitch * kDistPitch];
  __shared__ int s_mmax;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f = blockIdx.z, tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, h = a.h, w = a.w, R = a.R;
  const float* d = a.depth + (int64_t)f * h * w;

  // the focus distance: given, or read from the map (no host synchronisation)
  float zf = a.focus;
  bool flat = false;
  if (!(zf > 0.0f)) {
    zf = d[(int64_t)a.fy * w + a.fx];
    flat = !valid_z(a.cam, zf);
  }
  const float invf = flat ? 0.0f : __fdiv_rn(1.0f, zf);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.focus_out[f] = flat ? __builtin_nanf("") : zf;

  if (tid == 0) s_mmax = f2i(0.5f);
  for (int i = tid; i < (R + 1) * (R + 1); i += 256) {
    const int dy = i / (R + 1), dx = i - dy * (R + 1);
    s_dist[dy * kDistPitch + dx] = sqrt_rn_int(dx * dx + dy * dy);
  }
  block_sync();

  // the largest radius of the tile and its halo of R
  int Rt = R;
  if (a.bound) {
    Rt = 0;
    if (!flat && R > 0) {
      const int y0 = max(ty0 - R, 0), y1 = min(ty0 + kTH + R, h), x0 = max(tx0 - R, 0), x1 = min(tx0 + kTW + R, w);
      const int nx = x1 - x0, cnt = (y1 - y0) * nx;
      float mx = 0.5f;
      for (int i = tid; i < cnt; i += 256) {
        const int yy = i / nx, xx = i - yy * nx;
        mx = fmaxf(mx, bokeh_radius(a, d[(int64_t)(y0 + yy) * w + x0 + xx], invf, false));
      }
      __hip_atomic_fetch_max(&s_mmax, f2i(mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (positive floats order as their bits)
      block_sync();
      const float s = __fadd_rn(i2f(s_mmax), 0.5f);
      Rt = min(R, (int)ceilf(s) - 1);
    }
  }
  Rt = __builtin_amdgcn_readfirstlane(Rt);

  // this lane's outputs
  const int px = tx0 + lane, py0 = ty0 + wave * kPix;
  BokehPixel p[kPix];
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int py = py0 + j;
    float z = __builtin_inff(), r = 0.0f;
    if (px < w && py < h) {
      z = d[(int64_t)py * w + px];
      r = bokeh_radius(a, z, invf, flat);
      z = valid_z(a.cam, z) ? z : __builtin_inff();
    }
    const float m = fmaxf(r, 0.5f);
    p[j].zk = z, p[j].r = r, p[j].h = __fadd_rn(m, 0.5f), p[j].ia = __fdiv_rn(1.0f, __fmul_rn(m, m));
    p[j].sw = p[j].sc[0] = p[j].sc[1] = p[j].sc[2] = 0.0f;
  }

  const float* img = a.img.frame(f);
  const int64_t plane = a.img.plane();
  const int ncols = kTW + 2 * Rt, sy_end = ty0 + kTH + Rt;  // source rows [ty0 - Rt, sy_end), columns [tx0 - Rt, tx0 - Rt + ncols)
  for (int sy0 = ty0 - Rt; sy0 < sy_end; sy0 += kBand) {
    block_sync();  // (the previous band is consumed)
    for (int i = tid; i < kBand * ncols; i += 256) {
      const int br = i / ncols, bc = i - br * ncols, sy = sy0 + br, sx = tx0 - Rt + bc;
      Pair zr = pair(__builtin_inff(), -1.0f), ic = pair(0.0f, 0.0f), gb = pair(0.0f, 0.0f);
      if (sy >= 0 && sy < h && sy < sy_end && sx >= 0 && sx < w) {
        const float z = d[(int64_t)sy * w + sx];
        const float r = bokeh_radius(a, z, invf, flat), m = fmaxf(r, 0.5f);
        const float* c = img + (int64_t)nearest(sy, h, a.img.ih) * a.img.iw + nearest(sx, w, a.img.iw);
        zr = pair(valid_z(a.cam, z) ? z : __builtin_inff(), r);
        ic = pair(__fdiv_rn(1.0f, __fmul_rn(m, m)), finite_or_zero(c[0]));
        gb = pair(finite_or_zero(c[plane]), finite_or_zero(c[2 * plane]));
      }
      s_zr[br * kPitch + bc] = zr, s_ic[br * kPitch + bc] = ic, s_gb[br * kPitch + bc] = gb;
    }
    block_sync();
    for (int br = 0; br < kBand; ++br) {
      const int dy0 = sy0 + br - py0;  // the row's offset from the lane's first output; from output j: dy0 - j
      if (dy0 < -Rt) continue;
      if (dy0 > Rt + kPix - 1) break;
      // column `lane` of the table's row |dy| of each output (lanes above Rt hold nothing that is read)
      int drow[kPix];
      bool on[kPix];
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        const int dy = dy0 - j;
        on[j] = dy >= -Rt && dy <= Rt;
        drow[j] = f2i(s_dist[(on[j] ? abs(dy) : 0) * kDistPitch + (lane <= Rt ? lane : 0)]);
      }
      const int base = br * kPitch + lane;
      if (on[0] && on[kPix - 1]) {  // (then every output takes the row)
        Pair zr_n = s_zr[base], ic_n = s_ic[base], gb_n = s_gb[base];
        for (int bc = 0; bc <= 2 * Rt; ++bc) {
          const Pair zr = zr_n, ic = ic_n, gb = gb_n;
          const int nxt = base + min(bc + 1, 2 * Rt);  // the next source's reads are in flight while this one's taps run
          zr_n = s_zr[nxt], ic_n = s_ic[nxt], gb_n = s_gb[nxt];
          const float hq = __fadd_rn(fmaxf(zr.y, 0.5f), 0.5f);
          const int adx = abs(bc - Rt);
#pragma unroll
          for (int j = 0; j < kPix; ++j)
            bokeh_tap(p[j], zr.x, zr.y, hq, ic.x, ic.y, gb.x, gb.y, i2f(__builtin_amdgcn_readlane(drow[j], adx)));
        }
      } else {
        for (int bc = 0; bc <= 2 * Rt; ++bc) {
          const Pair zr = s_zr[base + bc], ic = s_ic[base + bc], gb = s_gb[base + bc];
          const float hq = __fadd_rn(fmaxf(zr.y, 0.5f), 0.5f);
          const int adx = abs(bc - Rt);
#pragma unroll
          for (int j = 0; j < kPix; ++j)
            if (on[j]) bokeh_tap(p[j], zr.x, zr.y, hq, ic.x, ic.y, gb.x, gb.y, i2f(__builtin_amdgcn_readlane(drow[j], adx)));
        }
      }
    }
  }

  if (!ROWS) {
    if (px < w) {
      float* o = a.out + (int64_t)f * 3 * h * w + px;
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        if (py0 + j >= h) break;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[((int64_t)ch * h + py0 + j) * w] = __fdiv_rn(p[j].sc[ch], p[j].sw);
      }
    }
    return;
  }

  // the scanlines: a tile row is the bytes [c0, c1) of its scanline (the filter byte with the first tile, the zeros up to the next
  // multiple of 16 behind the frame's last byte with the last), assembled in 256 bytes of LDS at LDS offset == global address (mod 16)
  block_sync();  // (every read of the band is done)
  uint8_t* buf = (uint8_t*)s_zr;
  const int64_t rowb = 1 + 3 * (int64_t)w, total = rowb * h;
  const int c0 = tx0 == 0 ? 0 : 1 + 3 * tx0, xe = min(tx0 + kTW, w), c1 = 1 + 3 * xe;
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int py = py0 + j;
    if (py >= h) break;  // (the same for every lane of the wave)
    const int64_t o = py * rowb + c0;
    const int shift = (int)(o & 15);  // (the buffer and its frame stride are 16-byte aligned)
    const int tail = (py == h - 1 && xe == w) ? (int)((total + 15) / 16 * 16 - total) : 0;
    uint8_t* row = buf + (wave * kPix + j) * 256 + shift;
    if (tx0 == 0 && lane == 0) row[0] = 0;
    if (lane < tail) row[c1 - c0 + lane] = 0;
    if (px < w) {
      uint8_t* q = row + (1 + 3 * px - c0);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) q[ch] = (uint8_t)color_byte(__fmul_rn(__fdiv_rn(p[j].sc[ch], p[j].sw), 255.0f));
    }
  }
  block_sync();
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    const int py = py0 + j;
    if (py >= h) break;
    const int64_t o = py * rowb + c0;
    const int shift = (int)(o & 15);
    const int tail = (py == h - 1 && xe == w) ? (int)((total + 15) / 16 * 16 - total) : 0;
    store_ragged(a.rows + (int64_t)f * a.rows_fstride + o, (const uint4*)s_zr + (wave * kPix + j) * 16, shift, c1 - c0 + tail, lane);
  }
}

PRV2_NO_PACKED_FP32_END

static int check_bokeh(const char* name, const float* depth, const float* image, int n, int h, int w, int ih, int iw, float fx, float aperture,
                       float focus, float focus_u, float focus_v, float max_radius, float lo, float hi, const float* focus_out) {
  PRV2_REQUIRE(depth && focus_out, "%s: null pointer (depth, focus_out)", name);
  if (check_map(name, n, h, w) || check_image(name, image, n, ih, iw) || check_camera(name, fx, fx, 0.0f, 0.0f) || check_range(name, lo, hi, 0.0f)) return 1;
  PRV2_REQUIRE(aperture >= 0.0f && aperture < __builtin_inff(), "%s: aperture %g: finite and not below 0", name, (double)aperture);
  PRV2_REQUIRE(max_radius >= 0.0f && max_radius <= (float)kBokehMaxRadius, "%s: max_radius %g: in [0, %d] (prv2_bokeh_max_radius)", name,
               (double)max_radius, kBokehMaxRadius);
  PRV2_REQUIRE(!(focus > 0.0f) || focus < __builtin_inff(), "%s: focus %g: a finite distance (0, less or NaN: the focus point)", name, (double)focus);
  PRV2_REQUIRE(focus_u >= 0.0f && focus_u <= 1.0f && focus_v >= 0.0f && focus_v <= 1.0f, "%s: focus point (%g, %g) outside [0, 1]^2", name,
               (double)focus_u, (double)focus_v);
  return 0;
}

static BokehArgs bokeh_args(const float* depth, const float* image, int h, int w, int ih, int iw, float fx, float aperture, float focus, float focus_u,
                            float focus_v, float max_radius, float lo, float hi, float* focus_out) {
  BokehArgs a{};
  a.depth = depth, a.img = ImageSrc{image, ih, iw};
  a.k = fx * aperture * 0.5f;  // (fp32, one rounding per product: the host specification's k)
  a.focus = focus > 0.0f ? focus : 0.0f;
  a.rm = max_radius;
  a.cam = Camera{fx, fx, 0.0f, 0.0f, lo, hi};
  a.h = h, a.w = w;
  const int fy = (int)floor((double)focus_v * h), fxp = (int)floor((double)focus_u * w);
  a.fy = fy < h - 1 ? fy : h - 1, a.fx = fxp < w - 1 ? fxp : w - 1;
  a.R = (int)ceilf(max_radius);
  a.bound = g_tile_bound;
  a.focus_out = focus_out;
  return a;
}

template <bool ROWS>
static void launch_bokeh(const BokehArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL((bokeh_kernel<ROWS>), dim3((unsigned)cdiv(a.w, kTW), (unsigned)cdiv(a.h, kTH), n), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int32_t prv2_bokeh_max_radius(void) { return kBokehMaxRadius; }

extern "C" int32_t prv2_bokeh_tile_bound(int32_t on) {
  const int was = g_tile_bound;
  if (on >= 0) g_tile_bound = on ? 1 : 0;
  return was;
}

extern "C" int prv2_bokeh_render(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                                 float aperture, float focus, float focus_u, float focus_v, float max_radius, float lo, float hi, float* out,
                                 float* focus_out, void* stream) {
  const char* name = "bokeh_render";
  if (check_bokeh(name, depth, image, n, h, w, ih, iw, fx, aperture, focus, focus_u, focus_v, max_radius, lo, hi, focus_out)) return 1;
  PRV2_REQUIRE(out != nullptr, "%s: null pointer (out)", name);
  PRV2_REQUIRE(cdiv(h, kTH) <= 65535, "%s: %d rows exceed the launch grid", name, h);
  BokehArgs a = bokeh_args(depth, image, h, w, ih, iw, fx, aperture, focus, focus_u, focus_v, max_radius, lo, hi, focus_out);
  a.out = out;
  launch_bokeh<false>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_bokeh_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                               float aperture, float focus, float focus_u, float focus_v, float max_radius, float lo, float hi, uint8_t* rows,
                               int64_t rows_fstride, float* focus_out, void* stream) {
  const char* name = "bokeh_rows";
  if (check_bokeh(name, depth, image, n, h, w, ih, iw, fx, aperture, focus, focus_u, focus_v, max_radius, lo, hi, focus_out)) return 1;
  if (check_rows(name, rows, rows_fstride, n, h, w, 3)) return 1;
  PRV2_REQUIRE(cdiv(h, kTH) <= 65535, "%s: %d rows exceed the launch grid", name, h);
  BokehArgs a = bokeh_args(depth, image, h, w, ih, iw, fx, aperture, focus, focus_u, focus_v, max_radius, lo, hi, focus_out);
  a.rows = rows, a.rows_fstride = rows_fstride;
  launch_bokeh<true>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
