// Novel-view export (include/prv2.h "Novel-view export"): a frame re-rendered from a camera that has moved, from its metric depth map.
// The map's own mesh -- the cells of "Mesh export" at stride 1 -- is rasterised with a depth test by three kernels chained on the
// caller's stream:
//   clear    the key buffer (one 64-bit key per view pixel) to all ones, 16 bytes per store;
//   raster   one workgroup per (frame, view, 64 x 16 source tile).  It projects the tile's 65 x 17 vertices (one halo row and column:
//            a cell belongs to the tile of its corner a) once into LDS, 16 bytes each (ux, uy, 1 / Zc, Z): 17,680 bytes.  A lane then
//            owns four vertices: it offers each as a point, and walks the boxes of the two faces of the cell below and right of it with
//            incremental integer edge functions.  Every candidate is ONE global 64-bit integer minimum on the key of its view pixel.
//            A projected coordinate never addresses memory: an index comes from a box cut to the frame, or from a point checked
//            against it;
//   resolve  one workgroup per (frame, view, row), shaped like the stereo view's: the row's winners into LDS, the fill of its holes
//            (row_fill.h), then the src / filled / iz maps or the PNG scanline, stored once with the ragged 16-byte store.
// A minimum has no order: the same input gives the same bits on every call.
//
// Arithmetic contract (the numpy restatement is output.py: view_source_host / view_image_host; bit for bit): the file is built with
// -ffp-contract=off, the divisions are __fdiv_rn; after the fixed-point positions everything but the interpolation of 1 / Zc is
// integer.  A face that passes the cap spans fewer than 288 units of 1/16 pixel each way, so its area and edge functions fit int32
// (and 2^24: their conversion to float is exact); the cap is therefore tested before the area is formed.
#include "row_fill.h"

namespace prv2 {
namespace {

constexpr int kViewMaxFace = 16;  // pixel centres a face's box may span in x and in y
constexpr int kTileW = 64, kTileH = 16, kVertW = kTileW + 1, kVertH = kTileH + 1;
constexpr int kUnseen = INT_MIN;  // ux of a vertex that is not seen

struct ViewArgs {
  const float* depth;  // [n, h, w]
  ImageSrc img;        // [n, 3, ih, iw] (rows mode)
  const float* poses;  // [nv, 12]
  Camera cam;
  float thr;
  int32_t h, w, nv;
  unsigned long long* keys;  // [n, nv, h, w]
  int32_t* src;        // source mode: [n, nv, h, w] each
  int32_t* filled;
  float* iz;           // (may be null)
  uint8_t* rows;       // rows mode: scanlines of [h][1 + 3 w] per (frame, view)
  int64_t rows_vstride;
};

struct Vert {
  int32_t ux, uy;  // 1/16 pixel; ux == kUnseen: not seen
  float iz, z;     // 1 / Zc; Z, NaN: not valid
};

__device__ __forceinline__ unsigned long long view_key(float q, int source) {
  return (unsigned long long)(0xFFFFFFFFu - __float_as_uint(q)) << 32 | (unsigned)source;
}

__global__ void __launch_bounds__(256) view_clear(uint4* keys4, int64_t n16, unsigned long long* tail) {
  const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) keys4[i] = ones;
  if (tail != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *tail = kHole;  // (an odd count of keys)
}

// one face: its vertices in the candidate's order, their source pixels; keys: the view's [h, w]
__device__ __forceinline__ void view_face(unsigned long long* keys, int h, int w, const Vert& p0, const Vert& p1, const Vert& p2, int s0, int s1,
                                          int s2) {
  const int minx = min(min(p0.ux, p1.ux), p2.ux), maxx = max(max(p0.ux, p1.ux), p2.ux);
  const int miny = min(min(p0.uy, p1.uy), p2.uy), maxy = max(max(p0.uy, p1.uy), p2.uy);
  int bx0 = (minx + 7) >> 4, bx1 = (maxx - 8) >> 4, by0 = (miny + 7) >> 4, by1 = (maxy - 8) >> 4;  // ceil / floor of (u - 8) / 16
  if (bx1 - bx0 + 1 > kViewMaxFace || by1 - by0 + 1 > kViewMaxFace) return;
  const int area = (p1.ux - p0.ux) * (p2.uy - p0.uy) - (p1.uy - p0.uy) * (p2.ux - p0.ux);
  if (area == 0) return;
  bx0 = max(bx0, 0), bx1 = min(bx1, w - 1), by0 = max(by0, 0), by1 = min(by1, h - 1);
  if (bx0 > bx1 || by0 > by1) return;
  const int s = area > 0 ? 1 : -1;
  const float fa = (float)(area > 0 ? area : -area);
  const int cx = 16 * bx0 + 8, cy = 16 * by0 + 8;
  // w_k at the box's first centre, and its steps of one pixel in x and in y
  int r0 = s * ((p2.ux - p1.ux) * (cy - p1.uy) - (p2.uy - p1.uy) * (cx - p1.ux));
  int r1 = s * ((p0.ux - p2.ux) * (cy - p2.uy) - (p0.uy - p2.uy) * (cx - p2.ux));
  int r2 = s * ((p1.ux - p0.ux) * (cy - p0.uy) - (p1.uy - p0.uy) * (cx - p0.ux));
  const int dx0 = -16 * s * (p2.uy - p1.uy), dx1 = -16 * s * (p0.uy - p2.uy), dx2 = -16 * s * (p1.uy - p0.uy);
  const int dy0 = 16 * s * (p2.ux - p1.ux), dy1 = 16 * s * (p0.ux - p2.ux), dy2 = 16 * s * (p1.ux - p0.ux);
  for (int py = by0; py <= by1; ++py, r0 += dy0, r1 += dy1, r2 += dy2) {
    int w0 = r0, w1 = r1, w2 = r2;
    unsigned long long* row = keys + (int64_t)py * w;
    for (int px = bx0; px <= bx1; ++px, w0 += dx0, w1 += dx1, w2 += dx2) {
      if ((w0 | w1 | w2) < 0) continue;
      const float q = __fdiv_rn(((float)w0 * p0.iz + (float)w1 * p1.iz) + (float)w2 * p2.iz, fa);
      const int source = (w0 >= w1 && w0 >= w2) ? s0 : w1 >= w2 ? s1 : s2;
      atomicMin(&row[px], view_key(q, source));
    }
  }
}

__global__ void __launch_bounds__(256) view_raster(ViewArgs a) {
  __shared__ int4 vert4[kVertW * kVertH];
  Vert* vert = (Vert*)vert4;
  const int tid = threadIdx.x, h = a.h, w = a.w;
  const int tiles_x = (w + kTileW - 1) / kTileW;
  const int x0 = (int)(blockIdx.x % tiles_x) * kTileW, y0 = (int)(blockIdx.x / tiles_x) * kTileH, v = blockIdx.y, f = blockIdx.z;
  const float* d = a.depth + (int64_t)f * h * w;
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = a.poses[v * 12 + i];

  for (int i = tid; i < kVertW * kVertH; i += 256) {
    const int ly = i / kVertW, lx = i - ly * kVertW, x = x0 + lx, y = y0 + ly;
    Vert p;
    p.ux = kUnseen, p.uy = 0, p.iz = 0.0f, p.z = __builtin_nanf("");
    if (x < w && y < h) {
      const float z = d[(int64_t)y * w + x];
      if (valid_z(a.cam, z)) {
        p.z = z;
        const float X = cam_x(a.cam, x, z), Y = cam_y(a.cam, y, z);
        const float xc = ((m[0] * X + m[1] * Y) + m[2] * z) + m[3];
        const float yc = ((m[4] * X + m[5] * Y) + m[6] * z) + m[7];
        const float zc = ((m[8] * X + m[9] * Y) + m[10] * z) + m[11];
        const float iz = __fdiv_rn(1.0f, zc);
        const float fu = a.cam.fx * __fdiv_rn(xc, zc) + a.cam.cx, fv = a.cam.fy * __fdiv_rn(yc, zc) + a.cam.cy;
        if (fabsf(zc) < __builtin_inff() && zc > 0.0f && fabsf(iz) < __builtin_inff() && fabsf(fu) < 65536.0f && fabsf(fv) < 65536.0f) {
          p.ux = (int)rintf(fu * 16.0f), p.uy = (int)rintf(fv * 16.0f), p.iz = iz;
        }
      }
    }
    vert[i] = p;
  }
  __syncthreads();

  unsigned long long* keys = a.keys + ((int64_t)f * a.nv + v) * h * w;
  for (int i = tid; i < kTileW * kTileH; i += 256) {
    const int ly = i / kTileW, lx = i - ly * kTileW, x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) continue;
    const Vert A = vert[ly * kVertW + lx];
    const int ia = y * w + x;
    if (A.ux != kUnseen) {  // the point
      const int px = A.ux >> 4, py = A.uy >> 4;
      if (px >= 0 && px < w && py >= 0 && py < h) atomicMin(&keys[(int64_t)py * w + px], view_key(A.iz, ia));
    }
    if (x + 1 >= w || y + 1 >= h) continue;
    const Vert B = vert[ly * kVertW + lx + 1], C = vert[(ly + 1) * kVertW + lx], D = vert[(ly + 1) * kVertW + lx + 1];
    // the cell's faces (a corner is kept where its Z is valid), each drawn where its three vertices are seen
    const CellFaces cf = cell_rule(a.thr, A.z, B.z, C.z, D.z, A.z == A.z, B.z == B.z, C.z == C.z, D.z == D.z);
    const bool sa = A.ux != kUnseen, sb = B.ux != kUnseen, sc = C.ux != kUnseen, sd = D.ux != kUnseen;
    const int ib = ia + 1, ic = ia + w, id = ia + w + 1;
    if (cf.ad) {  // (a, c, d) then (a, d, b)
      if (cf.first && sa && sc && sd) view_face(keys, h, w, A, C, D, ia, ic, id);
      if (cf.second && sa && sd && sb) view_face(keys, h, w, A, D, B, ia, id, ib);
    } else {      // (a, c, b) then (b, c, d)
      if (cf.first && sa && sc && sb) view_face(keys, h, w, A, C, B, ia, ic, ib);
      if (cf.second && sb && sc && sd) view_face(keys, h, w, B, C, D, ib, ic, id);
    }
  }
}

// CAP: columns of LDS (w <= CAP).  ROWS: write the scanline, else the int32 src / filled maps and the fp32 iz map.
template <int CAP, bool ROWS>
__global__ void __launch_bounds__(256) view_resolve(ViewArgs a) {
  constexpr int PER = CAP / 256;  // columns of a lane: i * 256 + tid
  __shared__ uint4 key4[CAP / 2];  // the row's winners; later the scanline's bytes
  __shared__ int32_t seg_left[CAP / 64], seg_right[CAP / 64];
  unsigned long long* key = (unsigned long long*)key4;
  const int tid = threadIdx.x, y = blockIdx.x, v = blockIdx.y, f = blockIdx.z, w = a.w;
  const int64_t o = (((int64_t)f * a.nv + v) * a.h + y) * w;
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (i * 256 + tid < w) key[i * 256 + tid] = a.keys[o + i * 256 + tid];
  __syncthreads();

  int32_t shown[PER], fill[PER];  // a lane's columns: the winning source (-1: hole), and with the holes filled
  row_fill<CAP>(key, seg_left, seg_right, w, tid, shown, fill);

  if (!ROWS) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int q = i * 256 + tid;
      if (q >= w) continue;
      a.src[o + q] = shown[i], a.filled[o + q] = fill[i];
      if (a.iz != nullptr) a.iz[o + q] = shown[i] >= 0 ? __uint_as_float(0xFFFFFFFFu - (uint32_t)(key[q] >> 32)) : 0.0f;
    }
    return;
  }

  // the scanline: filter byte 0, then w RGB pixels, assembled in LDS over the keys at LDS offset == global address (mod 16)
  __syncthreads();  // (every read of the keys is done)
  uint8_t* buf = (uint8_t*)key4;
  const int64_t rowb = 1 + 3 * (int64_t)w, total = rowb * a.h;
  const int shift = (int)((y * rowb) & 15);  // (the buffer and its view stride are 16-byte aligned)
  // the last row also writes the zeros up to the next multiple of 16 (a scanline buffer's tail)
  const int nb = (int)rowb + (y == a.h - 1 ? (int)((total + 15) / 16 * 16 - total) : 0);
  if (tid < 16) buf[shift + rowb + tid] = 0;
  if (tid == 0) buf[shift] = 0;
  const float* img = a.img.frame(f);
  const int64_t plane = a.img.plane();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int q = i * 256 + tid;
    if (q >= w) continue;
    uint32_t r = 0, g = 0, b = 0;
    if (fill[i] >= 0) {
      const int sy = fill[i] / w, sx = fill[i] - sy * w;
      const float* c = img + (int64_t)nearest(sy, a.h, a.img.ih) * a.img.iw + nearest(sx, w, a.img.iw);
      r = color_byte(__fmul_rn(c[0], 255.0f));
      g = color_byte(__fmul_rn(c[plane], 255.0f));
      b = color_byte(__fmul_rn(c[2 * plane], 255.0f));
    }
    uint8_t* px = buf + shift + 1 + 3 * q;
    px[0] = (uint8_t)r, px[1] = (uint8_t)g, px[2] = (uint8_t)b;
  }
  __syncthreads();
  store_ragged(a.rows + ((int64_t)f * a.nv + v) * a.rows_vstride + y * rowb, key4, shift, nb, tid);
}

static int64_t view_pixels(int n, int nv, int h, int w) {  // -1: bad arguments
  if (n < 1 || n > 65535 || nv < 1 || nv > 65535 || h < 1 || w < 1) return -1;
  const int64_t per = (int64_t)h * w;
  if (per >= (int64_t)INT_MAX / 4 || (int64_t)n * nv >= (int64_t)INT_MAX / 4 || per * n * nv >= (int64_t)INT_MAX / 4) return -1;
  return per * n * nv;
}

static int check_view(const char* name, const float* depth, int n, int h, int w, float fx, float fy, float cx, float cy, const float* poses, int nv,
                      float lo, float hi, float edge_thr, const void* workspace, int64_t workspace_bytes) {
  PRV2_REQUIRE(depth != nullptr && poses != nullptr, "%s: null pointer (depth, poses)", name);
  if (check_map(name, n, h, w)) return 1;
  PRV2_REQUIRE(nv >= 1 && nv <= 65535, "%s: view count %d out of range [1, 65535]", name, nv);
  PRV2_REQUIRE(view_pixels(n, nv, h, w) > 0, "%s: %d frames x %d views of %d x %d exceed 2^29 pixels", name, n, nv, h, w);
  if (check_row_width(name, w) || check_camera(name, fx, fy, cx, cy) || check_range(name, lo, hi, edge_thr)) return 1;
  PRV2_REQUIRE(workspace != nullptr && aligned16(workspace), "%s: the workspace must be 16-byte aligned", name);
  PRV2_REQUIRE(workspace_bytes >= 8 * view_pixels(n, nv, h, w), "%s: workspace of %lld bytes, %lld needed (prv2_view_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)(8 * view_pixels(n, nv, h, w)));
  return 0;
}

static ViewArgs view_args(const float* depth, int h, int w, float fx, float fy, float cx, float cy, const float* poses, int nv, float lo, float hi,
                          float thr, void* workspace) {
  ViewArgs a{};
  a.depth = depth, a.poses = poses;
  a.cam = Camera{fx, fy, cx, cy, lo, hi}, a.thr = thr;
  a.h = h, a.w = w, a.nv = nv;
  a.keys = (unsigned long long*)workspace;
  return a;
}

int g_view_stages = 7;  // measurement only (prv2_view_stages): bit 0 clear, bit 1 raster, bit 2 resolve

template <bool ROWS>
static void launch_view(const ViewArgs& a, int n, hipStream_t s) {
  const int64_t count = (int64_t)n * a.nv * a.h * a.w;
  if (g_view_stages & 1)
    hipLaunchKernelGGL(view_clear, dim3((unsigned)flat_grid(count / 2 + 1, 256)), dim3(256), 0, s, (uint4*)a.keys, count / 2,
                     (count & 1) ? a.keys + count - 1 : nullptr);
  const unsigned tiles = (unsigned)(cdiv(a.w, kTileW) * cdiv(a.h, kTileH));
  if (g_view_stages & 2) hipLaunchKernelGGL(view_raster, dim3(tiles, (unsigned)a.nv, (unsigned)n), dim3(256), 0, s, a);
  if (!(g_view_stages & 4)) return;
  if (a.w <= 4096)
    hipLaunchKernelGGL((view_resolve<4096, ROWS>), dim3((unsigned)a.h, (unsigned)a.nv, (unsigned)n), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((view_resolve<8192, ROWS>), dim3((unsigned)a.h, (unsigned)a.nv, (unsigned)n), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int32_t prv2_view_max_face(void) { return kViewMaxFace; }

extern "C" int32_t prv2_view_stages(int32_t mask) {
  const int32_t before = g_view_stages;
  if (mask >= 0) g_view_stages = mask & 7;
  return before;
}

extern "C" int64_t prv2_view_workspace_bytes(int32_t n, int32_t nv, int32_t h, int32_t w) {
  const int64_t px = view_pixels(n, nv, h, w);
  return px < 0 ? -1 : 8 * px;
}

extern "C" int prv2_view_source(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, const float* poses,
                                int32_t nv, float lo, float hi, float edge_thr, int32_t* src, int32_t* filled, float* iz, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const char* name = "view_source";
  if (check_view(name, depth, n, h, w, fx, fy, cx, cy, poses, nv, lo, hi, edge_thr, workspace, workspace_bytes)) return 1;
  PRV2_REQUIRE(src && filled, "%s: null pointer (src, filled)", name);
  ViewArgs a = view_args(depth, h, w, fx, fy, cx, cy, poses, nv, lo, hi, edge_thr, workspace);
  a.src = src, a.filled = filled, a.iz = iz;
  launch_view<false>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_view_rows(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx, float fy,
                              float cx, float cy, const float* poses, int32_t nv, float lo, float hi, float edge_thr, uint8_t* rows,
                              int64_t rows_vstride, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "view_rows";
  if (check_view(name, depth, n, h, w, fx, fy, cx, cy, poses, nv, lo, hi, edge_thr, workspace, workspace_bytes)) return 1;
  if (check_image(name, image, n, ih, iw)) return 1;
  if (check_rows(name, rows, rows_vstride, n, h, w, 3)) return 1;
  ViewArgs a = view_args(depth, h, w, fx, fy, cx, cy, poses, nv, lo, hi, edge_thr, workspace);
  a.img = ImageSrc{image, ih, iw}, a.rows = rows, a.rows_vstride = rows_vstride;
  launch_view<true>(a, n, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
