// PNG scanline buffers (include/prv2.h "Output stage"): the kernel that turns a per-pixel function into deflate-ready scanlines, its
// launch and the argument checks of the entry points that write them (csrc/output.hip, csrc/pointcloud.hip).
#pragma once
#include <limits.h>

#include "common.h"

namespace prv2 {
namespace {

constexpr int kChunk = 4096;     // scanline bytes per block: 256 lanes x one 16-byte store
constexpr int kMaxColors = 1024; // colour-table entries kept in LDS (N + 3)

// ---------------------------------------------------------------------------------------------------------------
// PNG scanlines: [h][1 + BPP w] bytes per frame, filter byte 0 first in every row.  A row is never 16-byte aligned, so the
// frame's rows are treated as one byte stream: a block assembles 4096 consecutive bytes of it in LDS (one pixel per lane and
// step, byte writes into LDS) and each lane stores 16 of them.  The stream's tail up to the next multiple of 16 is zero.
// ---------------------------------------------------------------------------------------------------------------
// Op: bpp (bytes per pixel), lut (does pixel() read the colour table), pixel(frame, linear index f * h * w + row * w + col, table) ->
// the pixel's bytes, first byte lowest.
template <class Op>
__global__ void __launch_bounds__(256) rows_kernel(Op op, const uint8_t* __restrict__ lut, int nlut, int h, int w, uint8_t* __restrict__ out,
                                                   int64_t out_fstride) {
  constexpr int BPP = Op::bpp;
  __shared__ uint4 buf4[kChunk / 16];
  __shared__ uint32_t table[Op::lut ? kMaxColors : 1];
  uint8_t* buf = (uint8_t*)buf4;
  const int tid = threadIdx.x, f = blockIdx.y;
  const int64_t rowb = 1 + (int64_t)BPP * w, total = rowb * h;
  const int64_t o0 = (int64_t)blockIdx.x * kChunk;
  const int64_t o1 = o0 + kChunk < total ? o0 + kChunk : total;  // real bytes of this chunk: [o0, o1)
  buf4[tid] = make_uint4(0, 0, 0, 0);
  if (Op::lut)
    for (int i = tid; i < nlut; i += 256) table[i] = ((const uint32_t*)lut)[i];
  __syncthreads();
  // items of a row: 0 = the filter byte, j >= 1 = pixel j - 1.  rel counts items from the start of the chunk's first row.
  const int64_t row0 = o0 / rowb;
  const int c0 = (int)(o0 - row0 * rowb), c1 = (int)(o1 - 1 - row0 * rowb);  // c1 < kChunk + rowb: may lie in a later row
  const int j0 = c0 == 0 ? 0 : (c0 - 1) / BPP + 1;
  const int rows_in = (int)(c1 / rowb), cl = (int)(c1 - rows_in * rowb);
  const int rel1 = rows_in * (w + 1) + (cl == 0 ? 0 : (cl - 1) / BPP + 1);
  const int64_t hw = (int64_t)h * w;
  for (int rel = j0 + tid; rel <= rel1; rel += 256) {
    const int dr = rel / (w + 1), j = rel - dr * (w + 1);
    if (j == 0) continue;
    const int64_t row = row0 + dr;
    const uint32_t px = op.pixel(f, (int64_t)f * hw + row * w + (j - 1), table);
    const int64_t off = row * rowb + 1 + (int64_t)BPP * (j - 1) - o0;  // may start before / end after the chunk
#pragma unroll
    for (int b = 0; b < BPP; ++b) {
      const int64_t o = off + b;
      if (o >= 0 && o < o1 - o0) buf[o] = (uint8_t)(px >> (8 * b));
    }
  }
  __syncthreads();
  const int64_t o = o0 + (int64_t)tid * 16;
  if (o < (total + 15) / 16 * 16) *(uint4*)(out + (int64_t)f * out_fstride + o) = buf4[tid];
}

// A block's store of the LDS image buf[shift + i] to dst[i], i in [0, nb), where shift = dst mod 16 (so dst - shift is 16-byte aligned):
// the bytes before the first and from the last 16-byte boundary one by one, the aligned interior as 16-byte words
__device__ __forceinline__ void store_ragged(uint8_t* __restrict__ dst, const uint4* buf4, int shift, int nb, int tid) {
  const uint8_t* buf = (const uint8_t*)buf4;
  const int head = (16 - shift) & 15;              // bytes before the first 16-byte boundary
  const int h_end = head < nb ? head : nb;
  const int wide = (nb - h_end) / 16;              // aligned 16-byte words of the interior
  const int t_beg = h_end + 16 * wide;
  if (tid < h_end) dst[tid] = buf[shift + tid];
  uint4* dst4 = (uint4*)(dst + h_end);
  const uint4* src4 = buf4 + (shift + h_end) / 16;
  for (int i = tid; i < wide; i += 256) dst4[i] = src4[i];
  if (tid < nb - t_beg) dst[t_beg + tid] = buf[shift + t_beg + tid];
}

static int check_map(const char* name, int n, int h, int w) {
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad frame shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX / 4, "%s: %d frames of %d x %d exceed 2^29 pixels", name, n, h, w);
  return 0;
}

static int64_t rows_bytes(int h, int w, int bpp) { return roundup((int64_t)h * (1 + (int64_t)bpp * w), 16); }

static int check_rows(const char* name, const void* rows, int64_t fstride, int n, int h, int w, int bpp) {
  PRV2_REQUIRE(rows != nullptr, "%s: null pointer (rows)", name);
  PRV2_REQUIRE(((uintptr_t)rows & 15) == 0, "%s: the scanline buffer must be 16-byte aligned", name);
  PRV2_REQUIRE(fstride % 16 == 0 && fstride >= rows_bytes(h, w, bpp), "%s: frame stride %lld of the scanline buffer: a multiple of 16, at least %lld (prv2_rows_bytes)",
               name, (long long)fstride, (long long)rows_bytes(h, w, bpp));
  return 0;
}

template <class Op>
static void launch_rows(const Op& op, const uint8_t* lut, int nlut, int n, int h, int w, uint8_t* rows, int64_t fstride, hipStream_t s) {
  const int64_t chunks = cdiv(rows_bytes(h, w, Op::bpp), kChunk);
  hipLaunchKernelGGL((rows_kernel<Op>), dim3((unsigned)chunks, n), dim3(256), 0, s, op, lut, nlut, h, w, rows, fstride);
}

}  // namespace
}  // namespace prv2
