// What the record-packing exports share (csrc/pointcloud.hip: the point cloud and the grid mesh; csrc/mesh_adaptive.hip: the adaptive mesh),
// once each: the run a block owns, the keep predicate of a pixel, the bytes of a vertex and of a face record, and the one-block scan that
// turns the runs' counts into offsets.  The ragged store of a block's records is rows.h's store_ragged.
#pragma once
#include "scene.h"

namespace prv2 {
namespace {

constexpr int kRun = 2048;     // pixels of a frame one block owns: kRounds steps of 256 lanes, lane t of step r has pixel r * 256 + t of the run
constexpr int kRounds = kRun / 256;
constexpr int kSegs = kRounds * 4;  // (step, wave) segments of 64 consecutive pixels
constexpr int kRecord = 15;    // bytes of a vertex
constexpr int kFace = 13;      // bytes of a face record: uchar 3 + three int32

struct CloudArgs {
  const float* depth;  // [n, h, w]
  Camera cam;
  float thr;           // flying-pixel threshold (<= 0: off)
  int32_t h, w, stride;
  int32_t nblk;        // blocks (runs) per frame
};

__device__ __forceinline__ bool flying(const Camera& c, float thr, float z, float zn) { return valid_z(c, zn) && !joined(thr, z, zn); }

// the keep predicate of pixel (y, x) of frame ``d``; z = d[y * w + x]
__device__ __forceinline__ bool keep_pixel(const CloudArgs& a, const float* __restrict__ d, int y, int x, float z) {
  if (!valid_z(a.cam, z) || y % a.stride != 0 || x % a.stride != 0) return false;
  if (!(a.thr > 0.0f)) return true;
  const int64_t i = (int64_t)y * a.w + x;
  bool fly = false;
  if (x > 0) fly = fly || flying(a.cam, a.thr, z, d[i - 1]);
  if (x + 1 < a.w) fly = fly || flying(a.cam, a.thr, z, d[i + 1]);
  if (y > 0) fly = fly || flying(a.cam, a.thr, z, d[i - a.w]);
  if (y + 1 < a.h) fly = fly || flying(a.cam, a.thr, z, d[i + a.w]);
  return !fly;
}

// the 15 bytes of the vertex of pixel (y, x) of an h x w map with depth z: float x, y, z and the colour of the nearest sample of the
// frame's image ``img`` (``plane``: its channel stride)
__device__ __forceinline__ void vertex_record(const Camera& cam, const ImageSrc& src, const float* __restrict__ img, int64_t plane, int h, int w, int y,
                                              int x, float z, uint8_t* rec) {
  const float* c = img + (int64_t)nearest(y, h, src.ih) * src.iw + nearest(x, w, src.iw);
  const uint32_t w0 = __float_as_uint(cam_x(cam, x, z)), w1 = __float_as_uint(cam_y(cam, y, z)), w2 = __float_as_uint(z);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    rec[b] = (uint8_t)(w0 >> (8 * b));
    rec[4 + b] = (uint8_t)(w1 >> (8 * b));
    rec[8 + b] = (uint8_t)(w2 >> (8 * b));
  }
  rec[12] = (uint8_t)color_byte(__fmul_rn(c[0], 255.0f));
  rec[13] = (uint8_t)color_byte(__fmul_rn(c[plane], 255.0f));
  rec[14] = (uint8_t)color_byte(__fmul_rn(c[2 * plane], 255.0f));
}

// the 13 bytes of a face: the list length 3, then its three vertex indices, little-endian
__device__ __forceinline__ void face_record(const int32_t* tri, uint8_t* rec) {
  rec[0] = 3;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const uint32_t word = (uint32_t)tri[v];
#pragma unroll
    for (int b = 0; b < 4; ++b) rec[1 + 4 * v + b] = (uint8_t)(word >> (8 * b));
  }
}

// one block per frame: counts[f][0 .. nblk) -> their exclusive prefix sums in block order (in place), totals[f] = the frame's N
__global__ void __launch_bounds__(256) cloud_scan_kernel(int32_t* __restrict__ counts, int32_t nblk, int64_t* __restrict__ totals) {
  __shared__ int32_t part[256];
  const int tid = threadIdx.x, f = blockIdx.x;
  int32_t* c = counts + (int64_t)f * nblk;
  const int per = (nblk + 255) / 256;  // a lane's contiguous chunk
  const int i0 = tid * per < nblk ? tid * per : nblk, i1 = i0 + per < nblk ? i0 + per : nblk;
  int32_t sum = 0;
  for (int i = i0; i < i1; ++i) sum += c[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int t = 0; t < 256; ++t) {
      const int32_t v = part[t];
      part[t] = run;
      run += v;
    }
    totals[f] = (int64_t)run;
  }
  __syncthreads();
  int32_t run = part[tid];
  for (int i = i0; i < i1; ++i) {
    const int32_t v = c[i];
    c[i] = run;
    run += v;
  }
}

// A block's (step, wave) segment totals in ``seg`` -> their exclusive prefix sums; seg[kSegs] = the run's count.  Every lane of
// the block calls it; it holds the barrier before and the one after.
__device__ __forceinline__ void scan_segments(int32_t* seg, int tid) {
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int s = 0; s < kSegs; ++s) {
      const int32_t v = seg[s];
      seg[s] = run;
      run += v;
    }
    seg[kSegs] = run;
  }
  __syncthreads();
}

}  // namespace
}  // namespace prv2
