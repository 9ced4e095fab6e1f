// Stereo export (include/prv2.h "Stereo export"): a frame re-rendered from a second eye position a baseline to the right, from its
// metric depth map.  With a horizontal baseline every image row is an independent one-dimensional problem: scatter the row's pixels to
// their target columns with a depth test, fill the disocclusions from the farther side, gather the colours, write the PNG scanline.  One
// workgroup owns one row of one frame and keeps it in LDS from the first step to the last; the row is read once from memory and its
// scanline written once with the ragged 16-byte store of the cloud's records (rows.h).
//
// Arithmetic contract (the numpy restatement is output.py: stereo_source_host / stereo_image_host; byte for byte):
//   - the file is built with -ffp-contract=off; the two fp32 operations that are rounded are written with __f*_rn: s = k / Z - c with
//     k = fx * baseline and c = k / convergence computed once on the host, then tf = (float)x - rint(s); everything after is integer;
//   - t(x) = (int)clip(tf, -1, w), NaN -> -1; a valid pixel covers [t(x), e], e = max(t(x), t(x + 1) - 1) when x + 1 is in the frame,
//     valid and joined to x (not |Z - Zn| > thr * min(Z, Zn), or thr <= 0), else t(x); columns outside [0, w - 1] are dropped;
//   - depth test: the smallest Z wins a column, between equal Z the smaller x.  The key of a source pixel is (ordered bits of Z) << 32 | x
//     and the test is ONE 64-bit LDS integer min per covered column (ds_min_u64: no compare-and-swap loop in the generated code, and
//     no second pass or barrier as the two-pass 32-bit form needs).  A minimum does not depend on arrival order: same bytes every call;
//   - fill: a hole takes the source of the nearest shown column on its left or right: the right one when its winner has the larger Z,
//     else the left one; the one that exists at the frame's border; -1 in a row that shows nothing (row_fill.h, shared with view.hip).
#include "row_fill.h"

namespace prv2 {
namespace {

constexpr int kStereoMaxWidth = 8192;  // the widest row a workgroup keeps in LDS (8 bytes per column: 64 KiB of the CU's 160)

struct StereoArgs {
  const float* depth;  // [n, h, w]
  ImageSrc img;        // [n, 3, ih, iw] (rows mode)
  float k, c;          // fx * baseline, k / convergence
  Camera cam;          // (the kernel reads its depth range; fx is in k)
  float thr;
  int32_t h, w;
  int32_t layout;      // PRV2_STEREO_RIGHT / _SBS / _ANAGLYPH (rows mode)
  uint8_t* rows;       // rows mode: scanlines of [h][1 + 3 wout], wout = w or 2 w (sbs)
  int64_t rows_fstride;
  int32_t* src;        // source mode: [n, h, w] each
  int32_t* filled;
};

// the target column of source pixel x, in [-1, w]
__device__ __forceinline__ int stereo_target(const StereoArgs& a, int x, float z) {
  const float s = __fsub_rn(__fdiv_rn(a.k, z), a.c);
  const float tf = __fsub_rn((float)x, rintf(s));
  if (!(tf > -1.0f)) return -1;  // (NaN as well)
  return tf >= (float)a.w ? a.w : (int)tf;
}

// unsigned keys in the order of the floats (finite Z; -0 is keyed as +0: they are equal depths)
__device__ __forceinline__ uint32_t ordered_bits(float z) {
  const uint32_t b = __float_as_uint(z == 0.0f ? 0.0f : z);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

// CAP: columns of LDS (w <= CAP).  ROWS: write the scanline of the layout, else the int32 src / filled maps.
template <int CAP, bool ROWS>
__global__ void __launch_bounds__(256) stereo_kernel(StereoArgs a) {
  constexpr int PER = CAP / 256;  // columns of a lane: i * 256 + tid
  __shared__ uint4 key4[CAP / 2];  // the depth-test keys; later the scanline's bytes
  __shared__ int32_t seg_left[CAP / 64], seg_right[CAP / 64];  // per 64 columns: the last / first shown column, then their scans
  unsigned long long* key = (unsigned long long*)key4;
  const int tid = threadIdx.x, y = blockIdx.x, f = blockIdx.y, w = a.w;
  const float* d = a.depth + ((int64_t)f * a.h + y) * w;

#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (i * 256 + tid < w) key[i * 256 + tid] = kHole;
  __syncthreads();

  // scatter with the depth test
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int x = i * 256 + tid;
    if (x >= w) continue;
    const float z = d[x];
    if (!valid_z(a.cam, z)) continue;
    const int t = stereo_target(a, x, z);
    int e = t;
    if (x + 1 < w) {
      const float zn = d[x + 1];
      if (valid_z(a.cam, zn) && joined(a.thr, z, zn)) {
        const int tn = stereo_target(a, x + 1, zn) - 1;
        e = tn > t ? tn : t;
      }
    }
    const int q0 = t > 0 ? t : 0, q1 = e < w - 1 ? e : w - 1;
    const unsigned long long mine = (unsigned long long)ordered_bits(z) << 32 | (unsigned)x;
    for (int q = q0; q <= q1; ++q) atomicMin(&key[q], mine);
  }
  __syncthreads();

  int32_t shown[PER], fill[PER];  // a lane's columns: the winning source (-1: hole), and with the holes filled
  row_fill<CAP>(key, seg_left, seg_right, w, tid, shown, fill);

  if (!ROWS) {
    const int64_t o = ((int64_t)f * a.h + y) * w;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = i * 256 + tid;
      if (q < w) a.src[o + q] = shown[i], a.filled[o + q] = fill[i];
    }
    return;
  }

  // the scanline: filter byte 0, then wout RGB pixels, assembled in LDS over the keys at LDS offset == global address (mod 16)
  __syncthreads();  // (every read of the keys is done)
  uint8_t* buf = (uint8_t*)key4;
  const int wout = a.layout == PRV2_STEREO_SBS ? 2 * w : w;
  const int64_t rowb = 1 + 3 * (int64_t)wout, total = rowb * a.h;
  const int shift = (int)((y * rowb) & 15);  // (the buffer and its frame stride are 16-byte aligned)
  // the last row also writes the zeros up to the next multiple of 16 (a scanline buffer's tail)
  const int nb = (int)rowb + (y == a.h - 1 ? (int)((total + 15) / 16 * 16 - total) : 0);
  if (tid < 16) buf[shift + rowb + tid] = 0;
  if (tid == 0) buf[shift] = 0;
  const float* img = a.img.frame(f) + (int64_t)nearest(y, a.h, a.img.ih) * a.img.iw;
  const int64_t plane = a.img.plane();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int q = i * 256 + tid;
    if (q >= w) continue;
    uint32_t r = 0, g = 0, b = 0;
    if (fill[i] >= 0) {
      const float* c = img + nearest(fill[i], w, a.img.iw);
      if (a.layout != PRV2_STEREO_ANAGLYPH) r = color_byte(__fmul_rn(c[0], 255.0f));
      g = color_byte(__fmul_rn(c[plane], 255.0f));
      b = color_byte(__fmul_rn(c[2 * plane], 255.0f));
    }
    uint8_t* px = buf + shift + 1 + 3 * (a.layout == PRV2_STEREO_SBS ? w + q : q);
    if (a.layout != PRV2_STEREO_RIGHT) {  // the left eye: the image itself on the depth map's grid
      const float* c = img + nearest(q, w, a.img.iw);
      if (a.layout == PRV2_STEREO_ANAGLYPH) {
        r = color_byte(__fmul_rn(c[0], 255.0f));
      } else {
        uint8_t* left = buf + shift + 1 + 3 * q;
        left[0] = (uint8_t)color_byte(__fmul_rn(c[0], 255.0f));
        left[1] = (uint8_t)color_byte(__fmul_rn(c[plane], 255.0f));
        left[2] = (uint8_t)color_byte(__fmul_rn(c[2 * plane], 255.0f));
      }
    }
    px[0] = (uint8_t)r, px[1] = (uint8_t)g, px[2] = (uint8_t)b;
  }
  __syncthreads();
  store_ragged(a.rows + (int64_t)f * a.rows_fstride + y * rowb, key4, shift, nb, tid);
}

static int check_stereo(const char* name, const float* depth, int n, int h, int w, float fx, float baseline, float convergence, float lo, float hi,
                        float edge_thr) {
  PRV2_REQUIRE(depth != nullptr, "%s: null pointer (depth)", name);
  if (check_map(name, n, h, w) || check_row_width(name, w) || check_camera(name, fx, fx, 0.0f, 0.0f) || check_range(name, lo, hi, edge_thr)) return 1;
  PRV2_REQUIRE(fabsf(baseline) < __builtin_inff(), "%s: baseline %g: finite", name, (double)baseline);
  PRV2_REQUIRE(convergence == convergence && convergence != 0.0f, "%s: convergence %g: a distance other than 0 (inf: parallel axes)", name,
               (double)convergence);
  return 0;
}

static StereoArgs stereo_args(const float* depth, int h, int w, float fx, float baseline, float convergence, float lo, float hi, float thr) {
  StereoArgs a{};
  a.depth = depth;
  a.k = fx * baseline;  // (fp32, one rounding: the host specification's k)
  a.c = fabsf(convergence) == __builtin_inff() ? 0.0f : a.k / convergence;
  a.cam = Camera{fx, fx, 0.0f, 0.0f, lo, hi}, a.thr = thr;
  a.h = h, a.w = w;
  return a;
}

template <bool ROWS>
static void launch_stereo(const StereoArgs& a, int n, hipStream_t s) {
  if (a.w <= 4096)
    hipLaunchKernelGGL((stereo_kernel<4096, ROWS>), dim3((unsigned)a.h, n), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((stereo_kernel<kStereoMaxWidth, ROWS>), dim3((unsigned)a.h, n), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int32_t prv2_stereo_max_width(void) { return kStereoMaxWidth; }

extern "C" int prv2_stereo_source(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float baseline, float convergence, float lo, float hi,
                                  float edge_thr, int32_t* src, int32_t* filled, void* stream) {
  const char* name = "stereo_source";
  if (check_stereo(name, depth, n, h, w, fx, baseline, convergence, lo, hi, edge_thr)) return 1;
  PRV2_REQUIRE(src && filled, "%s: null pointer (src, filled)", name);
  StereoArgs a = stereo_args(depth, h, w, fx, baseline, convergence, lo, hi, edge_thr);
  a.src = src, a.filled = filled;
  launch_stereo<false>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_stereo_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                                float baseline, float convergence, float lo, float hi, float edge_thr, int32_t layout, uint8_t* rows,
                                int64_t rows_fstride, void* stream) {
  const char* name = "stereo_rows";
  if (check_stereo(name, depth, n, h, w, fx, baseline, convergence, lo, hi, edge_thr)) return 1;
  if (check_image(name, image, n, ih, iw)) return 1;
  PRV2_REQUIRE(layout == PRV2_STEREO_RIGHT || layout == PRV2_STEREO_SBS || layout == PRV2_STEREO_ANAGLYPH, "%s: layout %d", name, layout);
  if (check_rows(name, rows, rows_fstride, n, h, layout == PRV2_STEREO_SBS ? 2 * w : w, 3)) return 1;
  StereoArgs a = stereo_args(depth, h, w, fx, baseline, convergence, lo, hi, edge_thr);
  a.img = ImageSrc{image, ih, iw}, a.layout = layout, a.rows = rows, a.rows_fstride = rows_fstride;
  launch_stereo<true>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
