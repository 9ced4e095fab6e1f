// Adaptive mesh export (include/prv2.h "Adaptive mesh export"; the numpy restatement is output.py: mesh_adaptive_host, equal in every
// byte): a right-triangulated irregular network over the depth map of B >= 1 frames [n, h, w] -- large triangles where the surface is
// flat, pixel-sized ones at its boundaries.  Fixed launch counts, no host synchronisation, no read-modify-write atomics: the same
// input gives the same bytes on every call.
//
// The rule (output.py states it in full).  The vertex grid is padded to whole blocks of B x B cells, B = 2^L: Hp = B ceil((h - 1) / B) + 1;
// a padded vertex is neither kept nor smooth.  Block (y0, x0) has the corners A = (y0, x0), B' = (y0, x0 + B), C = (y0 + B, x0),
// D = (y0 + B, x0 + B) and the root triangles (D, A, C), (A, D, B'); (a, b, c) has the hypotenuse a-b, the apex c, the midpoint
// m = (a + b) / 2 and the children (c, a, m), (b, c, m); after 2L bisections the legs are one pixel long.  A triangle above the finest
// is a face iff its midpoint is not ``required``, else it splits; a finest one is a face iff its corners are kept and its edges joined.
// required(m): m is not smooth, a hypotenuse end or an existing apex of m is not kept, an existing child vertex of m is required, or
// |Zm (Za + Zb) - (Za Zb) 2| > T Zm (Za + Zb) (fp32, one rounding per operation, -ffp-contract=off like pointcloud.hip).
//
// Kernels, per call of prv2_mesh_adaptive_count:
//   kept       every padded vertex: the cloud's keep predicate at stride 1 (cloud.h), and its vertex index cleared to -1
//   seed       every padded vertex: smooth, and what of ``required`` does not depend on other vertices' ``required``
//   propagate  2L - 1 passes, fine to coarse (centres at hh = 1; edge midpoints, then centres at hh = 2, 4, ... B / 2): a vertex whose
//              child vertex is required becomes required.  A pass writes one class of vertices and reads the class below it.
//   count      a lane per finest slot of every block (2 B^2 per block, blocks in row-major order): it walks from its root towards its
//              slot and stops at the first triangle that does not split; that leaf is a face of the lane whose slot is the leaf's first.
//              Counts the faces of every run of kRun slots and marks the three vertices of every face (plain stores of one value).
//   scan       cloud.h's, on the face counts -> M; then the marked vertices of every run of padded pixels are counted and scanned -> N
// and of prv2_mesh_adaptive_pack:
//   vertices   ranks the marked vertices of a run, replaces their marks by their ranks and stores their records (cloud.h's vertex_record)
//   faces      walks as ``count`` does and stores the face records with the vertices' ranks
#include "cloud.h"

namespace prv2 {
namespace {

struct AdaArgs {
  const float* depth;   // [n, h, w]
  uint8_t* kept;        // [n, Hp, Wp]
  uint8_t* req;         // [n, Hp, Wp]
  int32_t* index;       // [n, Hp, Wp]: -1, 0 once a face uses the vertex, then its rank among the frame's used vertices
  int32_t* face_runs;   // [n, nrun_f]
  int32_t* vert_runs;   // [n, nrun_v]
  Camera cam;           // (the keep predicate reads lo and hi alone; the vertex records read all of it)
  float thr, tol;
  int32_t h, w, hp, wp;
  int32_t lg;           // L = log2 B
  int32_t nbx;          // blocks per row of blocks
  int32_t nslot;        // finest slots per frame: 2 B^2 blocks
  int32_t nvert;        // hp * wp
  int32_t nrun_f, nrun_v;
};

__device__ __forceinline__ CloudArgs cloud_of(const AdaArgs& m) {
  CloudArgs a{};
  a.depth = m.depth, a.cam = m.cam, a.thr = m.thr, a.h = m.h, a.w = m.w, a.stride = 1;
  return a;
}

// kept[f][y][x] of every padded vertex; index[f][y][x] = -1
__global__ void __launch_bounds__(256) ada_kept_kernel(AdaArgs m) {
  const int f = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.nvert) return;
  const int y = v / m.wp, x = v - y * m.wp;
  bool k = false;
  if (y < m.h && x < m.w) {
    const float* d = m.depth + (int64_t)f * m.h * m.w;
    k = keep_pixel(cloud_of(m), d, y, x, d[(int64_t)y * m.w + x]);
  }
  m.kept[(int64_t)f * m.nvert + v] = (uint8_t)k;
  m.index[(int64_t)f * m.nvert + v] = -1;
}

// the geometric test of a midpoint between two hypotenuse ends: the along-ray relative error of the harmonic mean
__device__ __forceinline__ bool geo_fails(float tol, float zm, float za, float zb) {
  const float p = __fmul_rn(zm, __fadd_rn(za, zb)), q = __fmul_rn(__fmul_rn(za, zb), 2.0f);
  return fabsf(__fsub_rn(p, q)) > __fmul_rn(tol, p);
}

// req[f][y][x] of every padded vertex that is not a block corner, without the child vertices' share
__global__ void __launch_bounds__(256) ada_seed_kernel(AdaArgs m) {
  const int f = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= m.nvert) return;
  const int y = v / m.wp, x = v - y * m.wp, B = 1 << m.lg;
  const uint8_t* kept = m.kept + (int64_t)f * m.nvert;
  uint8_t* req = m.req + (int64_t)f * m.nvert;
  if (((y | x) & (B - 1)) == 0) {  // a block corner is nobody's midpoint
    req[v] = 0;
    return;
  }
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  bool smooth = y < m.h && x < m.w && kept[v];
  float z = 0.0f;
  if (smooth) {
    z = d[(int64_t)y * m.w + x];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if ((dy == 0 && dx == 0) || yy < 0 || yy >= m.h || xx < 0 || xx >= m.w) continue;
        smooth = smooth && kept[yy * m.wp + xx] && joined(m.thr, z, d[(int64_t)yy * m.w + xx]);
      }
  }
  bool r = !smooth;
  if (!r) {  // (m is kept and inside the frame; an end or an apex that is kept is inside it too)
    const int l = __ffs(y | x | B) - 1, hh = 1 << l;
    const bool oy = (y >> l) & 1, ox = (x >> l) & 1;
    int ay, ax, by, bx;  // the hypotenuse ends
    if (oy && ox) {
      const bool main = 2 * hh == B || (((y >> (l + 1)) ^ (x >> (l + 1))) & 1) == 0;
      ay = y - hh, by = y + hh;
      ax = main ? x - hh : x + hh, bx = main ? x + hh : x - hh;
      r = !kept[ay * m.wp + ax] || !kept[by * m.wp + bx] || !kept[ay * m.wp + bx] || !kept[by * m.wp + ax];
    } else {
      ay = oy ? y - hh : y, by = oy ? y + hh : y;
      ax = ox ? x - hh : x, bx = ox ? x + hh : x;
      r = !kept[ay * m.wp + ax] || !kept[by * m.wp + bx];
      const int py = oy ? y : y - hh, px = oy ? x - hh : x, qy = oy ? y : y + hh, qx = oy ? x + hh : x;  // the apexes
      if (py >= 0 && px >= 0) r = r || !kept[py * m.wp + px];
      if (qy < m.hp && qx < m.wp) r = r || !kept[qy * m.wp + qx];
    }
    if (!r) r = geo_fails(m.tol, z, d[(int64_t)ay * m.w + ax], d[(int64_t)by * m.w + bx]);
  }
  req[v] = (uint8_t)r;
}

// One pass of the propagation at half-size hh: ``centres`` != 0: the centres (child vertices: the axial neighbours at hh), else the edge
// midpoints (child vertices: the diagonal neighbours at hh / 2 that exist).  A lane per vertex of the class.
__global__ void __launch_bounds__(256) ada_propagate_kernel(AdaArgs m, int hh, int centres) {
  const int f = blockIdx.y;
  int t = blockIdx.x * 256 + threadIdx.x;
  uint8_t* req = m.req + (int64_t)f * m.nvert;
  const int ny = (m.hp - 1) / (2 * hh), nx = (m.wp - 1) / (2 * hh);  // 2hh-squares each way
  if (centres) {
    if (t >= ny * nx) return;
    const int i = t / nx, j = t - i * nx, y = hh * (2 * i + 1), x = hh * (2 * j + 1);
    if (req[(y - hh) * m.wp + x] | req[(y + hh) * m.wp + x] | req[y * m.wp + x - hh] | req[y * m.wp + x + hh]) req[y * m.wp + x] = 1;
    return;
  }
  int y, x;
  if (t < (ny + 1) * nx) {  // on the rows that are multiples of 2hh
    const int i = t / nx, j = t - i * nx;
    y = 2 * hh * i, x = hh * (2 * j + 1);
  } else {
    t -= (ny + 1) * nx;
    if (t >= ny * (nx + 1)) return;
    const int i = t / (nx + 1), j = t - i * (nx + 1);
    y = hh * (2 * i + 1), x = 2 * hh * j;
  }
  const int q = hh / 2;
  bool any = false;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int yy = y + ((s & 2) ? q : -q), xx = x + ((s & 1) ? q : -q);
    if (yy >= 0 && yy < m.hp && xx >= 0 && xx < m.wp) any = any || req[yy * m.wp + xx];
  }
  if (any) req[y * m.wp + x] = 1;
}

// The face of finest slot g of a frame, if it has one -> vtx: its corners a, b, c as padded vertex numbers.  The walk: the root of the
// slot's block half, then the child the slot lies in, until a midpoint is not required (a leaf: the lane's face iff the slot is the
// leaf's first) or the legs are one pixel long.
__device__ __forceinline__ bool slot_face(const AdaArgs& m, const float* __restrict__ d, const uint8_t* __restrict__ kept, const uint8_t* __restrict__ req,
                                          int g, int (&vtx)[3]) {
  const int L2 = 2 * m.lg, B = 1 << m.lg;
  const int blk = g >> (L2 + 1), s = g & ((2 << L2) - 1);
  const int y0 = (blk / m.nbx) * B, x0 = (blk % m.nbx) * B;
  const bool second = (s >> L2) & 1;  // (D, A, C), then (A, D, B')
  int ay = second ? y0 : y0 + B, ax = second ? x0 : x0 + B, by = second ? y0 + B : y0, bx = second ? x0 + B : x0;
  int cy = second ? y0 : y0 + B, cx = second ? x0 + B : x0;
  for (int k = 0; k < L2; ++k) {
    const int my = (ay + by) >> 1, mx = (ax + bx) >> 1;
    if (!req[my * m.wp + mx]) {
      if (s & ((1 << (L2 - k)) - 1)) return false;
      vtx[0] = ay * m.wp + ax, vtx[1] = by * m.wp + bx, vtx[2] = cy * m.wp + cx;
      return true;
    }
    if ((s >> (L2 - k - 1)) & 1) {  // (b, c, m)
      ay = by, ax = bx, by = cy, bx = cx;
    } else {  // (c, a, m)
      const int ty = ay, tx = ax;
      ay = cy, ax = cx, by = ty, bx = tx;
    }
    cy = my, cx = mx;
  }
  vtx[0] = ay * m.wp + ax, vtx[1] = by * m.wp + bx, vtx[2] = cy * m.wp + cx;
  if (!(kept[vtx[0]] && kept[vtx[1]] && kept[vtx[2]])) return false;  // (kept: inside the frame)
  const float za = d[(int64_t)ay * m.w + ax], zb = d[(int64_t)by * m.w + bx], zc = d[(int64_t)cy * m.w + cx];
  return joined(m.thr, za, zb) && joined(m.thr, zb, zc) && joined(m.thr, za, zc);
}

// One step of a block over its run of slots (or of padded pixels): lane t has the flag k.  ``below``: flags of lower lanes of this wave,
// ``total``: of the whole wave.
__device__ __forceinline__ void step_rank(bool k, int& below, int& total) {
  const unsigned long long b = __ballot(k);
  below = __popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull));
  total = __popcll(b);
}

// faces of every run of slots: face_runs[f][run]; index = 0 at the three vertices of every face
__global__ void __launch_bounds__(256) ada_count_kernel(AdaArgs m) {
  __shared__ int32_t seg[kSegs + 1];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  const uint8_t *kept = m.kept + (int64_t)f * m.nvert, *req = m.req + (int64_t)f * m.nvert;
  int32_t* index = m.index + (int64_t)f * m.nvert;
#pragma unroll 1
  for (int r = 0; r < kRounds; ++r) {
    const int g = blockIdx.x * kRun + r * 256 + tid;
    int vtx[3], below, total;
    const bool k = g < m.nslot && slot_face(m, d, kept, req, g, vtx);
    if (k) index[vtx[0]] = 0, index[vtx[1]] = 0, index[vtx[2]] = 0;
    step_rank(k, below, total);
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);
  if (tid == 0) m.face_runs[(int64_t)f * m.nrun_f + blockIdx.x] = seg[kSegs];
}

// used vertices of every run of padded pixels: vert_runs[f][run]
__global__ void __launch_bounds__(256) ada_vertex_count_kernel(AdaArgs m) {
  __shared__ int32_t seg[kSegs + 1];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int32_t* index = m.index + (int64_t)f * m.nvert;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int v = blockIdx.x * kRun + r * 256 + tid;
    int below, total;
    step_rank(v < m.nvert && index[v] >= 0, below, total);
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);
  if (tid == 0) m.vert_runs[(int64_t)f * m.nrun_v + blockIdx.x] = seg[kSegs];
}

// The vertex records of every run of padded pixels, as pointcloud.hip's cloud_pack_kernel makes the cloud's: ranked in pixel order, built
// in LDS at LDS offset == global address (mod 16), stored as the byte range [15 off, 15 (off + cnt)) of the frame's vertex buffer.  The
// mark of a used vertex becomes its rank in the frame.
__global__ void __launch_bounds__(256) ada_vertex_pack_kernel(AdaArgs m, ImageSrc src, uint8_t* __restrict__ out, int64_t out_fstride) {
  __shared__ uint4 buf4[(kRun * kRecord + 16 + 15) / 16];
  __shared__ int32_t seg[kSegs + 1];
  uint8_t* buf = (uint8_t*)buf4;
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  int32_t* index = m.index + (int64_t)f * m.nvert;
  int32_t rank[kRounds];  // rank inside the wave's segment, -1: not used
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int v = blockIdx.x * kRun + r * 256 + tid;
    int below, total;
    const bool k = v < m.nvert && index[v] >= 0;
    step_rank(k, below, total);
    rank[r] = k ? below : -1;
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);
  const int32_t cnt = seg[kSegs];
  if (cnt == 0) return;
  const int32_t off = m.vert_runs[(int64_t)f * m.nrun_v + blockIdx.x];
  uint8_t* dst = out + (int64_t)f * out_fstride + (int64_t)kRecord * off;
  const int shift = (int)((uintptr_t)dst & 15);
  const float* img = src.frame(f);
  const int64_t plane = src.plane();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (rank[r] < 0) continue;
    const int v = blockIdx.x * kRun + r * 256 + tid;
    const int y = v / m.wp, x = v - y * m.wp;  // (used: kept, so inside the frame)
    const int32_t local = seg[r * 4 + wave] + rank[r];
    index[v] = off + local;
    vertex_record(m.cam, src, img, plane, m.h, m.w, y, x, d[(int64_t)y * m.w + x], buf + shift + kRecord * local);
  }
  __syncthreads();
  store_ragged(dst, buf4, shift, kRecord * cnt, tid);
}

// The face records of every run of slots, ranked in slot order, stored as the byte range [13 off, 13 (off + cnt)) of the frame's face buffer.
__global__ void __launch_bounds__(256) ada_face_pack_kernel(AdaArgs m, uint8_t* __restrict__ out, int64_t out_fstride) {
  __shared__ uint4 buf4[(kRun * kFace + 16 + 15) / 16];
  __shared__ int32_t seg[kSegs + 1];
  uint8_t* buf = (uint8_t*)buf4;
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  const uint8_t *kept = m.kept + (int64_t)f * m.nvert, *req = m.req + (int64_t)f * m.nvert;
  const int32_t* index = m.index + (int64_t)f * m.nvert;
  int32_t tri[kRounds][3];
  int32_t rank[kRounds];  // rank inside the wave's segment, -1: no face
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int g = blockIdx.x * kRun + r * 256 + tid;
    int vtx[3] = {0, 0, 0}, below, total;
    const bool k = g < m.nslot && slot_face(m, d, kept, req, g, vtx);
    step_rank(k, below, total);
    rank[r] = k ? below : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) tri[r][c] = k ? index[vtx[c]] : 0;
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);
  const int32_t cnt = seg[kSegs];
  if (cnt == 0) return;
  uint8_t* dst = out + (int64_t)f * out_fstride + (int64_t)kFace * m.face_runs[(int64_t)f * m.nrun_f + blockIdx.x];
  const int shift = (int)((uintptr_t)dst & 15);
#pragma unroll
  for (int r = 0; r < kRounds; ++r)
    if (rank[r] >= 0) face_record(tri[r], buf + shift + kFace * (seg[r * 4 + wave] + rank[r]));
  __syncthreads();
  store_ragged(dst, buf4, shift, kFace * cnt, tid);
}

static bool block_ok(int block) { return block >= 2 && block <= 64 && (block & (block - 1)) == 0; }
static int64_t padded(int v, int block) { return (int64_t)block * cdiv((int64_t)v - 1, block) + 1; }

// the shape checks every entry point makes, and the workspace's layout: index int32 [n, Hp, Wp], the face runs int32 [n, nrun_f], the
// vertex runs int32 [n, nrun_v], kept uint8 [n, Hp, Wp], required uint8 [n, Hp, Wp]
static int ada_args(const char* name, const float* depth, int n, int h, int w, float lo, float hi, float edge_thr, float tolerance, int block,
                    const void* workspace, int64_t workspace_bytes, AdaArgs* out) {
  PRV2_REQUIRE(depth != nullptr, "%s: null pointer (depth)", name);
  if (check_map(name, n, h, w) || check_range(name, lo, hi, edge_thr)) return 1;
  PRV2_REQUIRE(tolerance >= 0.0f && tolerance < __builtin_inff(), "%s: tolerance %g: finite and >= 0", name, (double)tolerance);
  PRV2_REQUIRE(block_ok(block), "%s: block %d: a power of two in [2, 64]", name, block);
  const int64_t need = prv2_mesh_adaptive_workspace_bytes(n, h, w, block);
  PRV2_REQUIRE(need >= 0, "%s: %d frames of %d x %d padded to blocks of %d exceed 2^29 vertices", name, n, h, w, block);
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  PRV2_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_mesh_adaptive_workspace_bytes)", name, (long long)workspace_bytes,
               (long long)need);
  AdaArgs m{};
  m.depth = depth;
  m.cam = Camera{1.0f, 1.0f, 0.0f, 0.0f, lo, hi};
  m.thr = edge_thr, m.tol = tolerance;
  m.h = h, m.w = w;
  m.hp = h < 2 || w < 2 ? 0 : (int32_t)padded(h, block), m.wp = h < 2 || w < 2 ? 0 : (int32_t)padded(w, block);  // (no cell: no vertex, no face)
  m.lg = __builtin_ctz((unsigned)block);
  m.nbx = (m.wp - 1) / block;
  m.nvert = m.hp * m.wp;
  m.nslot = m.nvert ? 2 * (m.hp - 1) * (m.wp - 1) : 0;
  m.nrun_f = (int32_t)cdiv(m.nslot, kRun), m.nrun_v = (int32_t)cdiv(m.nvert, kRun);
  m.index = (int32_t*)workspace;
  m.face_runs = m.index + (int64_t)n * m.nvert;
  m.vert_runs = m.face_runs + (int64_t)n * m.nrun_f;
  m.kept = (uint8_t*)(m.vert_runs + (int64_t)n * m.nrun_v);
  m.req = m.kept + (int64_t)n * m.nvert;
  *out = m;
  return 0;
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_mesh_adaptive_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t block) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || !block_ok(block) || (int64_t)n * h * w >= (int64_t)INT_MAX / 4) return -1;
  if (h < 2 || w < 2) return 4;
  const int64_t nvert = padded(h, block) * padded(w, block), nslot = 2 * (padded(h, block) - 1) * (padded(w, block) - 1);
  if ((int64_t)n * nvert >= (int64_t)INT_MAX / 4) return -1;
  return roundup((int64_t)n * (4 * nvert + 4 * cdiv(nslot, kRun) + 4 * cdiv(nvert, kRun) + 2 * nvert), 4);
}

extern "C" int64_t prv2_mesh_adaptive_vertex_bound(int32_t h, int32_t w) {
  if (h < 1 || w < 1) return -1;
  return (int64_t)kRecord * h * w;
}

extern "C" int64_t prv2_mesh_adaptive_face_bound(int32_t h, int32_t w) {
  if (h < 1 || w < 1) return -1;
  return 2 * (int64_t)kFace * (h - 1) * (w - 1);
}

extern "C" int prv2_mesh_adaptive_count(const float* depth, int32_t n, int32_t h, int32_t w, float lo, float hi, float edge_thr, float tolerance,
                                        int32_t block, int64_t* vertex_counts, int64_t* face_counts, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  const char* name = "mesh_adaptive_count";
  PRV2_REQUIRE(vertex_counts != nullptr && face_counts != nullptr, "%s: null pointer (counts)", name);
  AdaArgs m;
  if (ada_args(name, depth, n, h, w, lo, hi, edge_thr, tolerance, block, workspace, workspace_bytes, &m)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (m.nvert > 0) {
    const dim3 per_vertex((unsigned)cdiv(m.nvert, 256), n);
    hipLaunchKernelGGL(ada_kept_kernel, per_vertex, dim3(256), 0, s, m);
    hipLaunchKernelGGL(ada_seed_kernel, per_vertex, dim3(256), 0, s, m);
    for (int l = 0; l < m.lg; ++l) {
      const int hh = 1 << l;
      const int64_t ny = (m.hp - 1) / (2 * hh), nx = (m.wp - 1) / (2 * hh);
      if (l > 0)  // (the edge midpoints at hh = 1 have no child vertices)
        hipLaunchKernelGGL(ada_propagate_kernel, dim3((unsigned)cdiv((ny + 1) * nx + ny * (nx + 1), 256), n), dim3(256), 0, s, m, hh, 0);
      hipLaunchKernelGGL(ada_propagate_kernel, dim3((unsigned)cdiv(ny * nx, 256), n), dim3(256), 0, s, m, hh, 1);
    }
    hipLaunchKernelGGL(ada_count_kernel, dim3((unsigned)m.nrun_f, n), dim3(256), 0, s, m);
    hipLaunchKernelGGL(ada_vertex_count_kernel, dim3((unsigned)m.nrun_v, n), dim3(256), 0, s, m);
  }
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(n), dim3(256), 0, s, m.face_runs, m.nrun_f, face_counts);  // (no runs: M = 0, N = 0)
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(n), dim3(256), 0, s, m.vert_runs, m.nrun_v, vertex_counts);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_mesh_adaptive_pack(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                                       float fy, float cx, float cy, float lo, float hi, float edge_thr, float tolerance, int32_t block,
                                       void* workspace, int64_t workspace_bytes, uint8_t* vertices, int64_t vertices_fstride, uint8_t* faces,
                                       int64_t faces_fstride, void* stream) {
  const char* name = "mesh_adaptive_pack";
  PRV2_REQUIRE(vertices != nullptr, "%s: null pointer (vertices)", name);
  if (check_image(name, image, n, ih, iw) || check_camera(name, fx, fy, cx, cy)) return 1;
  AdaArgs m;
  if (ada_args(name, depth, n, h, w, lo, hi, edge_thr, tolerance, block, workspace, workspace_bytes, &m)) return 1;
  PRV2_REQUIRE(faces != nullptr || prv2_mesh_adaptive_face_bound(h, w) == 0, "%s: null pointer (faces)", name);
  PRV2_REQUIRE(vertices_fstride >= prv2_mesh_adaptive_vertex_bound(h, w), "%s: frame stride %lld of the vertex buffer < %lld (prv2_mesh_adaptive_vertex_bound)",
               name, (long long)vertices_fstride, (long long)prv2_mesh_adaptive_vertex_bound(h, w));
  PRV2_REQUIRE(faces_fstride >= prv2_mesh_adaptive_face_bound(h, w), "%s: frame stride %lld of the face buffer < %lld (prv2_mesh_adaptive_face_bound)",
               name, (long long)faces_fstride, (long long)prv2_mesh_adaptive_face_bound(h, w));
  m.cam = Camera{fx, fy, cx, cy, lo, hi};
  hipStream_t s = (hipStream_t)stream;
  if (m.nvert > 0) {
    hipLaunchKernelGGL(ada_vertex_pack_kernel, dim3((unsigned)m.nrun_v, n), dim3(256), 0, s, m, ImageSrc{image, ih, iw}, vertices, vertices_fstride);
    hipLaunchKernelGGL(ada_face_pack_kernel, dim3((unsigned)m.nrun_f, n), dim3(256), 0, s, m, faces, faces_fstride);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
