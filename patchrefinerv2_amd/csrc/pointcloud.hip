// Geometry export (include/prv2.h "Geometry export"): a metric depth map turned into geometry where it already is.  The vertex records
// of a binary PLY point cloud (float x, y, z + uchar red, green, blue: 15 bytes, kept pixels in row-major order) and the PNG scanlines
// of a surface-normal map, of B >= 1 frames [n, h, w].  Fixed launch counts, no host synchronisation, no atomics: the same input gives
// the same bytes on every call.  All three kernels are streaming passes (one read of the depth map and, for the cloud, one nearest
// sample of the image per kept pixel).  The faces of a triangle mesh over the cloud's vertices (include/prv2.h "Mesh export") are made the
// same way from the grid's cells: an index map, a count and a pack pass.
//
// Arithmetic contract (the numpy float32 restatement is output.py: pointcloud_host / normal_map_host; bit for bit):
//   - the file is built with -ffp-contract=off; every fp32 operation is written with __f*_rn (IEEE, one rounding each, in the order
//     of the restatement); division and square root are the correctly rounded ones (sqrtf: HIP's __fsqrt_rn is the native,
//     1-ulp instruction);
//   - camera, valid, joined, the colour sample and its bytes, the faces of a cell: scene.h; Z = D[y, x];
//   - the run a block owns, the keep predicate, the bytes of a vertex and of a face record, the scans: cloud.h (shared with mesh_adaptive.hip);
//   - flying: a valid in-frame 4-neighbour Zn that is not joined to Z;
//   - kept: valid, not flying, y % stride == 0 and x % stride == 0.
#include "cloud.h"

namespace prv2 {
namespace {

// One step of a block over its run: lane t evaluates pixel p0 + t (p0 a multiple of 64 inside the frame's pixel range or behind it).
// Returns the pixel's keep flag; ``below``: kept pixels of lower lanes of this wave, ``total``: of the whole wave.
__device__ __forceinline__ bool step_keep(const CloudArgs& a, const float* __restrict__ d, int64_t p, int64_t hw, float& z, int& y, int& x,
                                          int& below, int& total) {
  bool k = false;
  z = 0.0f, y = 0, x = 0;
  if (p < hw) {
    y = (int)(p / a.w);
    x = (int)(p - (int64_t)y * a.w);
    z = d[p];
    k = keep_pixel(a, d, y, x, z);
  }
  const unsigned long long b = __ballot(k);
  const int lane = threadIdx.x & 63;
  below = __popcll(b & ((1ull << lane) - 1ull));
  total = __popcll(b);
  return k;
}

// kept pixels of every run: counts[f][blk]
__global__ void __launch_bounds__(256) cloud_count_kernel(CloudArgs a, int32_t* __restrict__ counts) {
  __shared__ int32_t seg[kSegs];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int64_t hw = (int64_t)a.h * a.w, p0 = (int64_t)blockIdx.x * kRun;
  const float* d = a.depth + (int64_t)f * hw;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    float z;
    int y, x, below, total;
    step_keep(a, d, p0 + r * 256 + tid, hw, z, y, x, below, total);
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t c = 0;
    for (int s = 0; s < kSegs; ++s) c += seg[s];
    counts[(int64_t)f * a.nblk + blockIdx.x] = c;
  }
}

// The records of every run.  The block ranks its kept pixels in pixel order (ballot + popcount inside a wave, the (step, wave) segment
// totals through LDS), builds the records in LDS and stores its byte range [15 off, 15 (off + cnt)) of the frame's vertex buffer.  That
// range starts and ends at any byte alignment and the dwords at its two ends may belong to the neighbouring runs as well: the LDS image
// is shifted so that LDS offset == global address (mod 16), the bytes up to the first and from the last 16-byte boundary are stored one
// by one and only the aligned interior with 16-byte stores.  Nothing outside the range is written (or read).
__global__ void __launch_bounds__(256) cloud_pack_kernel(CloudArgs a, ImageSrc src, const int32_t* __restrict__ offsets,
                                                         uint8_t* __restrict__ out, int64_t out_fstride) {
  __shared__ uint4 buf4[(kRun * kRecord + 16 + 15) / 16];
  __shared__ int32_t seg[kSegs + 1];
  uint8_t* buf = (uint8_t*)buf4;
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int64_t hw = (int64_t)a.h * a.w, p0 = (int64_t)blockIdx.x * kRun;
  const float* d = a.depth + (int64_t)f * hw;
  float z[kRounds];
  int32_t rank[kRounds];  // rank inside the wave's segment, -1: not kept
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    int y, x, below, total;
    const bool k = step_keep(a, d, p0 + r * 256 + tid, hw, z[r], y, x, below, total);
    rank[r] = k ? below : -1;
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);  // exclusive prefix of the segment totals; seg[kSegs] = the run's count
  const int32_t cnt = seg[kSegs];
  if (cnt == 0) return;
  uint8_t* dst = out + (int64_t)f * out_fstride + (int64_t)kRecord * offsets[(int64_t)f * a.nblk + blockIdx.x];
  const int shift = (int)((uintptr_t)dst & 15);
  const float* img = src.frame(f);
  const int64_t plane = src.plane();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if (rank[r] < 0) continue;
    const int64_t p = p0 + r * 256 + tid;
    const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
    vertex_record(a.cam, src, img, plane, a.h, a.w, y, x, z[r], buf + shift + kRecord * (seg[r * 4 + wave] + rank[r]));
  }
  __syncthreads();
  store_ragged(dst, buf4, shift, kRecord * cnt, tid);
}

// ---- triangle mesh (include/prv2.h "Mesh export"; the numpy restatement is output.py: mesh_faces_host) -------------------------------
// The vertices are the cloud's.  Grid node (gy, gx) is pixel (gy * stride, gx * stride); cell (gy, gx), gy + 1 < gh, gx + 1 < gw, has the
// corners a = (gy, gx), b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1) and emits up to two faces.  Cells are ranked like pixels:
// a block owns a run of kRun cells in row-major order, a lane has 0, 1 or 2 faces (two ballots).

struct MeshArgs {
  const float* depth;    // [n, h, w]
  const int32_t* index;  // [n, gh, gw]: the vertex of a node, -1: not kept
  float thr;             // an edge is joined unless |Zp - Zq| > thr * min(Zp, Zq) (<= 0: always joined)
  int32_t h, w, stride, gh, gw;
  int32_t ncell;         // (gh - 1) * (gw - 1)
  int32_t nrun;          // blocks (runs of cells) per frame
};

// index[f][gy][gx] of every node: the rank of its pixel among the frame's kept pixels (cloud_pack_kernel's order), -1 where not kept
__global__ void __launch_bounds__(256) mesh_index_kernel(CloudArgs a, const int32_t* __restrict__ offsets, int32_t* __restrict__ index, int32_t gh,
                                                         int32_t gw) {
  __shared__ int32_t seg[kSegs + 1];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int64_t hw = (int64_t)a.h * a.w, p0 = (int64_t)blockIdx.x * kRun;
  const float* d = a.depth + (int64_t)f * hw;
  int32_t rank[kRounds];  // rank inside the wave's segment, -1: not kept
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    float z;
    int y, x, below, total;
    const bool k = step_keep(a, d, p0 + r * 256 + tid, hw, z, y, x, below, total);
    rank[r] = k ? below : -1;
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);  // exclusive prefix of the segment totals
  const int32_t base = offsets[(int64_t)f * a.nblk + blockIdx.x];
  int32_t* idx = index + (int64_t)f * gh * gw;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t p = p0 + r * 256 + tid;
    if (p >= hw) continue;
    const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
    if (y % a.stride != 0 || x % a.stride != 0) continue;
    idx[(int64_t)(y / a.stride) * gw + x / a.stride] = rank[r] < 0 ? -1 : base + seg[r * 4 + wave] + rank[r];
  }
}

// the faces of cell c of a frame (idx, d: the frame's index map and depth) -> their number; tri: their vertices, first candidate first
// (scene.h cell_rule; a corner is kept where it has a vertex)
__device__ __forceinline__ int cell_faces(const MeshArgs& m, const float* __restrict__ d, const int32_t* __restrict__ idx, int c, int32_t (&tri)[6]) {
  const int gy = c / (m.gw - 1), gx = c - gy * (m.gw - 1);
  const int32_t* i0 = idx + (int64_t)gy * m.gw + gx;
  const int32_t ia = i0[0], ib = i0[1], ic = i0[m.gw], id = i0[m.gw + 1];
  if ((ia >= 0) + (ib >= 0) + (ic >= 0) + (id >= 0) < 3) return 0;  // (no face: the depths are not read)
  const int64_t down = (int64_t)m.stride * m.w;
  const float* z0 = d + gy * down + (int64_t)gx * m.stride;
  const CellFaces cf = cell_rule(m.thr, z0[0], z0[m.stride], z0[down], z0[down + m.stride], ia >= 0, ib >= 0, ic >= 0, id >= 0);
  const int32_t f0[3] = {ia, ic, cf.ad ? id : ib}, f1[3] = {cf.ad ? ia : ib, cf.ad ? id : ic, cf.ad ? ib : id};
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    tri[v] = cf.first ? f0[v] : f1[v];
    tri[3 + v] = f1[v];
  }
  return (int)cf.first + (int)cf.second;
}

// One step of a block over its run of cells: lane t evaluates cell c.  Returns the cell's faces; ``below``: faces of lower lanes of this
// wave, ``total``: of the whole wave.
__device__ __forceinline__ int step_faces(const MeshArgs& m, const float* __restrict__ d, const int32_t* __restrict__ idx, int64_t c,
                                          int32_t (&tri)[6], int& below, int& total) {
  const int k = c < m.ncell ? cell_faces(m, d, idx, (int)c, tri) : 0;
  const unsigned long long b1 = __ballot(k >= 1), b2 = __ballot(k >= 2), lower = (1ull << (threadIdx.x & 63)) - 1ull;
  below = __popcll(b1 & lower) + __popcll(b2 & lower);
  total = __popcll(b1) + __popcll(b2);
  return k;
}

// faces of every run of cells: counts[f][run]
__global__ void __launch_bounds__(256) mesh_count_kernel(MeshArgs m, int32_t* __restrict__ counts) {
  __shared__ int32_t seg[kSegs];
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * kRun;
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  const int32_t* idx = m.index + (int64_t)f * m.gh * m.gw;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    int32_t tri[6];
    int below, total;
    step_faces(m, d, idx, c0 + r * 256 + tid, tri, below, total);
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t c = 0;
    for (int s = 0; s < kSegs; ++s) c += seg[s];
    counts[(int64_t)f * m.nrun + blockIdx.x] = c;
  }
}

// The face records of every run of cells, as cloud_pack_kernel makes the vertex records: ranked in cell order, built in LDS at
// LDS offset == global address (mod 16), stored as the byte range [13 off, 13 (off + cnt)) of the frame's face buffer.  Byte offsets
// are int64: 13 * M passes 2^31 for the largest frames.
__global__ void __launch_bounds__(256) mesh_pack_kernel(MeshArgs m, const int32_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                        int64_t out_fstride) {
  __shared__ uint4 buf4[(kRun * 2 * kFace + 16 + 15) / 16];
  __shared__ int32_t seg[kSegs + 1];
  uint8_t* buf = (uint8_t*)buf4;
  const int tid = threadIdx.x, wave = tid >> 6, f = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * kRun;
  const float* d = m.depth + (int64_t)f * m.h * m.w;
  const int32_t* idx = m.index + (int64_t)f * m.gh * m.gw;
  int32_t tri[kRounds][6];
  int32_t faces[kRounds], rank[kRounds];  // the cell's faces and the rank of its first one inside the wave's segment
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    int total;
    faces[r] = step_faces(m, d, idx, c0 + r * 256 + tid, tri[r], rank[r], total);
    if ((tid & 63) == 0) seg[r * 4 + wave] = total;
  }
  scan_segments(seg, tid);  // exclusive prefix of the segment totals; seg[kSegs] = the run's count
  const int32_t cnt = seg[kSegs];
  if (cnt == 0) return;
  uint8_t* dst = out + (int64_t)f * out_fstride + (int64_t)kFace * offsets[(int64_t)f * m.nrun + blockIdx.x];
  const int shift = (int)((uintptr_t)dst & 15);
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= faces[r]) continue;
      face_record(tri[r] + 3 * j, buf + shift + kFace * (seg[r * 4 + wave] + rank[r] + j));
    }
  }
  __syncthreads();
  store_ragged(dst, buf4, shift, kFace * cnt, tid);
}

// the surface normal of a pixel as RGB scanline bytes; pixels without a normal are (0, 0, 0)
struct NormalOp {
  static constexpr int bpp = 3;
  static constexpr bool lut = false;
  const float* depth;
  Camera cam;
  int32_t h, w;
  __device__ __forceinline__ bool point(const float* d, int y, int x, float& px, float& py, float& pz) const {
    if (y < 0 || y >= h || x < 0 || x >= w) return false;
    pz = d[(int64_t)y * w + x];
    if (!valid_z(cam, pz)) return false;
    px = cam_x(cam, x, pz);
    py = cam_y(cam, y, pz);
    return true;
  }
  // central difference of two valid neighbours, else the one-sided difference with the valid one
  __device__ __forceinline__ bool diff(const float* d, int y, int x, int dy, int dx, float cx_, float cy_, float cz_, float& gx, float& gy,
                                       float& gz) const {
    float ax, ay, az, bx, by, bz;
    const bool fwd = point(d, y + dy, x + dx, ax, ay, az), bwd = point(d, y - dy, x - dx, bx, by, bz);
    if (!fwd && !bwd) return false;
    if (!fwd) ax = cx_, ay = cy_, az = cz_;
    if (!bwd) bx = cx_, by = cy_, bz = cz_;
    gx = __fsub_rn(ax, bx), gy = __fsub_rn(ay, by), gz = __fsub_rn(az, bz);
    return true;
  }
  __device__ __forceinline__ uint32_t pixel(int f, int64_t i, const uint32_t*) const {
    const int64_t hw = (int64_t)h * w, local = i - (int64_t)f * hw;
    const int y = (int)(local / w), x = (int)(local - (int64_t)y * w);
    const float* d = depth + (int64_t)f * hw;
    float X, Y, Z, ux, uy, uz, vx, vy, vz;
    if (!point(d, y, x, X, Y, Z)) return 0u;
    if (!diff(d, y, x, 0, 1, X, Y, Z, ux, uy, uz) || !diff(d, y, x, 1, 0, X, Y, Z, vx, vy, vz)) return 0u;
    float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
    float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
    float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
    if (!(len > 0.0f) || !(len < __builtin_inff())) return 0u;
    nx = __fdiv_rn(nx, len), ny = __fdiv_rn(ny, len), nz = __fdiv_rn(nz, len);
    const float inf = __builtin_inff();
    if (!(fabsf(nx) < inf && fabsf(ny) < inf && fabsf(nz) < inf)) return 0u;
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(nx, X), __fmul_rn(ny, Y)), __fmul_rn(nz, Z));
    if (dot > 0.0f) nx = -nx, ny = -ny, nz = -nz;
    const uint32_t r = color_byte(__fmul_rn(__fadd_rn(__fmul_rn(nx, 0.5f), 0.5f), 255.0f));
    const uint32_t g = color_byte(__fmul_rn(__fadd_rn(__fmul_rn(ny, 0.5f), 0.5f), 255.0f));
    const uint32_t b = color_byte(__fmul_rn(__fadd_rn(__fmul_rn(nz, 0.5f), 0.5f), 255.0f));
    return r | g << 8 | b << 16;
  }
};

static int64_t cloud_blocks(int h, int w) { return cdiv((int64_t)h * w, kRun); }

static int check_cloud(const char* name, const float* depth, int n, int h, int w, float fx, float fy, float cx, float cy, float lo, float hi,
                       float edge_thr, int stride, const void* workspace, int64_t workspace_bytes) {
  PRV2_REQUIRE(depth != nullptr, "%s: null pointer (depth)", name);
  if (check_map(name, n, h, w) || check_camera(name, fx, fy, cx, cy) || check_range(name, lo, hi, edge_thr)) return 1;
  PRV2_REQUIRE(stride >= 1, "%s: stride %d < 1", name, stride);
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  PRV2_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
  PRV2_REQUIRE(workspace_bytes >= prv2_pointcloud_workspace_bytes(n, h, w), "%s: workspace of %lld bytes < %lld (prv2_pointcloud_workspace_bytes)",
               name, (long long)workspace_bytes, (long long)prv2_pointcloud_workspace_bytes(n, h, w));
  return 0;
}

static CloudArgs cloud_args(const float* depth, int h, int w, float fx, float fy, float cx, float cy, float lo, float hi, float thr, int stride) {
  CloudArgs a{};
  a.depth = depth;
  a.cam = Camera{fx, fy, cx, cy, lo, hi};
  a.thr = thr;
  a.h = h, a.w = w, a.stride = stride;
  a.nblk = (int32_t)cloud_blocks(h, w);
  return a;
}

static int64_t mesh_cells(int h, int w, int stride) { return (cdiv(h, stride) - 1) * (cdiv(w, stride) - 1); }

static int check_mesh(const char* name, const float* depth, int n, int h, int w, int stride, const void* workspace, int64_t workspace_bytes) {
  PRV2_REQUIRE(depth != nullptr, "%s: null pointer (depth)", name);
  if (check_map(name, n, h, w)) return 1;
  PRV2_REQUIRE(stride >= 1, "%s: stride %d < 1", name, stride);
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  PRV2_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", name);
  PRV2_REQUIRE(workspace_bytes >= prv2_mesh_workspace_bytes(n, h, w, stride), "%s: workspace of %lld bytes < %lld (prv2_mesh_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)prv2_mesh_workspace_bytes(n, h, w, stride));
  return 0;
}

// the mesh workspace: the index map int32 [n, gh, gw], then the face counts / offsets of the runs of cells int32 [n, nrun]
static MeshArgs mesh_args(const float* depth, int n, int h, int w, float thr, int stride, void* workspace, int32_t** runs) {
  MeshArgs m{};
  m.depth = depth;
  m.index = (const int32_t*)workspace;
  m.thr = thr;
  m.h = h, m.w = w, m.stride = stride;
  m.gh = (int32_t)cdiv(h, stride), m.gw = (int32_t)cdiv(w, stride);
  m.ncell = (int32_t)mesh_cells(h, w, stride);
  m.nrun = (int32_t)cdiv(m.ncell, kRun);
  *runs = (int32_t*)workspace + (int64_t)n * m.gh * m.gw;
  return m;
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int64_t prv2_pointcloud_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || n > 65535 || h < 1 || w < 1 || (int64_t)n * h * w >= (int64_t)INT_MAX / 4) return -1;
  return (int64_t)n * cloud_blocks(h, w) * (int64_t)sizeof(int32_t);
}

extern "C" int64_t prv2_pointcloud_bound(int32_t h, int32_t w, int32_t stride) {
  if (h < 1 || w < 1 || stride < 1) return -1;
  return cdiv(h, stride) * cdiv(w, stride) * kRecord;
}

extern "C" int prv2_pointcloud_count(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, float lo, float hi,
                                     float edge_thr, int32_t stride, int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "pointcloud_count";
  PRV2_REQUIRE(counts != nullptr, "%s: null pointer (counts)", name);
  if (check_cloud(name, depth, n, h, w, fx, fy, cx, cy, lo, hi, edge_thr, stride, workspace, workspace_bytes)) return 1;
  const CloudArgs a = cloud_args(depth, h, w, fx, fy, cx, cy, lo, hi, edge_thr, stride);
  hipLaunchKernelGGL(cloud_count_kernel, dim3((unsigned)a.nblk, n), dim3(256), 0, (hipStream_t)stream, a, (int32_t*)workspace);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (int32_t*)workspace, a.nblk, counts);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_pointcloud_pack(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, float fx,
                                    float fy, float cx, float cy, float lo, float hi, float edge_thr, int32_t stride, const void* workspace,
                                    int64_t workspace_bytes, uint8_t* vertices, int64_t vertices_fstride, void* stream) {
  const char* name = "pointcloud_pack";
  PRV2_REQUIRE(vertices != nullptr, "%s: null pointer (vertices)", name);
  if (check_image(name, image, n, ih, iw) || check_cloud(name, depth, n, h, w, fx, fy, cx, cy, lo, hi, edge_thr, stride, workspace, workspace_bytes)) return 1;
  PRV2_REQUIRE(vertices_fstride >= prv2_pointcloud_bound(h, w, stride), "%s: frame stride %lld of the vertex buffer < %lld (prv2_pointcloud_bound)",
               name, (long long)vertices_fstride, (long long)prv2_pointcloud_bound(h, w, stride));
  const CloudArgs a = cloud_args(depth, h, w, fx, fy, cx, cy, lo, hi, edge_thr, stride);
  hipLaunchKernelGGL(cloud_pack_kernel, dim3((unsigned)a.nblk, n), dim3(256), 0, (hipStream_t)stream, a, ImageSrc{image, ih, iw},
                     (const int32_t*)workspace, vertices, vertices_fstride);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int64_t prv2_mesh_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t stride) {
  if (prv2_pointcloud_workspace_bytes(n, h, w) < 0 || stride < 1) return -1;
  return (int64_t)n * (cdiv(h, stride) * cdiv(w, stride) + cdiv(mesh_cells(h, w, stride), kRun)) * (int64_t)sizeof(int32_t);
}

extern "C" int64_t prv2_mesh_bound(int32_t h, int32_t w, int32_t stride) {
  if (h < 1 || w < 1 || stride < 1) return -1;
  return 2 * kFace * mesh_cells(h, w, stride);
}

extern "C" int prv2_mesh_index(const float* depth, int32_t n, int32_t h, int32_t w, float lo, float hi, float edge_thr, int32_t stride,
                               const void* cloud_workspace, int64_t cloud_workspace_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "mesh_index";
  if (check_mesh(name, depth, n, h, w, stride, workspace, workspace_bytes)) return 1;
  PRV2_REQUIRE(cloud_workspace != nullptr && ((uintptr_t)cloud_workspace & 3) == 0, "%s: the cloud's workspace: null or not 4-byte aligned", name);
  PRV2_REQUIRE(cloud_workspace_bytes >= prv2_pointcloud_workspace_bytes(n, h, w), "%s: cloud workspace of %lld bytes < %lld (prv2_pointcloud_workspace_bytes)",
               name, (long long)cloud_workspace_bytes, (long long)prv2_pointcloud_workspace_bytes(n, h, w));
  const CloudArgs a = cloud_args(depth, h, w, 1.0f, 1.0f, 0.0f, 0.0f, lo, hi, edge_thr, stride);  // (the keep predicate does not read the camera)
  hipLaunchKernelGGL(mesh_index_kernel, dim3((unsigned)a.nblk, n), dim3(256), 0, (hipStream_t)stream, a, (const int32_t*)cloud_workspace,
                     (int32_t*)workspace, (int32_t)cdiv(h, stride), (int32_t)cdiv(w, stride));
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_mesh_count(const float* depth, int32_t n, int32_t h, int32_t w, float edge_thr, int32_t stride, int64_t* counts, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  const char* name = "mesh_count";
  PRV2_REQUIRE(counts != nullptr, "%s: null pointer (counts)", name);
  if (check_mesh(name, depth, n, h, w, stride, workspace, workspace_bytes)) return 1;
  int32_t* runs;
  const MeshArgs m = mesh_args(depth, n, h, w, edge_thr, stride, workspace, &runs);
  if (m.nrun > 0) hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)m.nrun, n), dim3(256), 0, (hipStream_t)stream, m, runs);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, runs, m.nrun, counts);  // (no runs: M = 0)
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_mesh_pack(const float* depth, int32_t n, int32_t h, int32_t w, float edge_thr, int32_t stride, const void* workspace,
                              int64_t workspace_bytes, uint8_t* faces, int64_t faces_fstride, void* stream) {
  const char* name = "mesh_pack";
  if (check_mesh(name, depth, n, h, w, stride, workspace, workspace_bytes)) return 1;
  PRV2_REQUIRE(faces != nullptr || prv2_mesh_bound(h, w, stride) == 0, "%s: null pointer (faces)", name);
  PRV2_REQUIRE(faces_fstride >= prv2_mesh_bound(h, w, stride), "%s: frame stride %lld of the face buffer < %lld (prv2_mesh_bound)", name,
               (long long)faces_fstride, (long long)prv2_mesh_bound(h, w, stride));
  int32_t* runs;
  const MeshArgs m = mesh_args(depth, n, h, w, edge_thr, stride, (void*)workspace, &runs);
  if (m.nrun > 0)
    hipLaunchKernelGGL(mesh_pack_kernel, dim3((unsigned)m.nrun, n), dim3(256), 0, (hipStream_t)stream, m, (const int32_t*)runs, faces, faces_fstride);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_normal_rows(const float* depth, int32_t n, int32_t h, int32_t w, float fx, float fy, float cx, float cy, float lo, float hi,
                                uint8_t* rows, int64_t rows_fstride, void* stream) {
  const char* name = "normal_rows";
  PRV2_REQUIRE(depth != nullptr, "%s: null pointer (depth)", name);
  if (check_map(name, n, h, w) || check_camera(name, fx, fy, cx, cy) || check_range(name, lo, hi, 0.0f)) return 1;
  if (check_rows(name, rows, rows_fstride, n, h, w, 3)) return 1;
  NormalOp op{depth, Camera{fx, fy, cx, cy, lo, hi}, h, w};
  launch_rows(op, nullptr, 0, n, h, w, rows, rows_fstride, (hipStream_t)stream);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
