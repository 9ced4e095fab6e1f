// What the re-rendered views share (csrc/stereo.hip, csrc/view.hip): a row of 64-bit depth-test keys in LDS -- the smallest key of a
// column wins, its high word orders the winners by distance (the larger, the farther), its low word is the winner's source -- and the
// fill of the row's holes from the farther side.  (The rules of the depth map and the colour image: scene.h.)
#pragma once
#include "scene.h"

namespace prv2 {
namespace {

constexpr unsigned long long kHole = ~0ull;

// The fill of a row of w <= CAP keys in LDS, by a block of 256 lanes; lane tid owns the columns i * 256 + tid.  Call it after the
// barrier that ends the writes of the keys.  shown: the winning source of a lane's columns (-1: hole); fill: the same, a hole taking
// the source of the nearest shown column on its left or right: the right one when its winner's high word is the larger (it is
// farther), else the left one; the one that exists at the row's border; -1 in a row that shows nothing.  The keys are only read:
// a barrier is due before they are overwritten.  seg_left, seg_right: CAP / 64 words of LDS each.
template <int CAP>
__device__ __forceinline__ void row_fill(const unsigned long long* key, int32_t* seg_left, int32_t* seg_right, int w, int tid,
                                         int32_t (&shown)[CAP / 256], int32_t (&fill)[CAP / 256]) {
  constexpr int PER = CAP / 256;
  const int lane = tid & 63, wave = tid >> 6;
  // the last and the first shown column of every 64-column segment (segment i * 4 + wave = columns of step i of this wave)
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (i * 256 >= w) break;  // (the same for every lane)
    const int q = i * 256 + tid;
    const unsigned long long b = __ballot(q < w && key[q] != kHole);
    if (lane == 0) {
      const int q64 = i * 256 + wave * 64;
      seg_left[i * 4 + wave] = b ? q64 + 63 - __clzll((long long)b) : -1;
      seg_right[i * 4 + wave] = b ? q64 + __ffsll((unsigned long long)b) - 1 : w;
    }
  }
  __syncthreads();
  const int nseg = (w + 255) / 256 * 4;
  if (tid == 0) {  // max-scan: the last shown column before each segment
    int run = -1;
    for (int s = 0; s < nseg; ++s) {
      const int v = seg_left[s];
      seg_left[s] = run;
      run = v > run ? v : run;
    }
  }
  if (tid == 64) {  // min-scan from the right: the first shown column behind each segment
    int run = w;
    for (int s = nseg - 1; s >= 0; --s) {
      const int v = seg_right[s];
      seg_right[s] = run;
      run = v < run ? v : run;
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < PER; ++i) {
    shown[i] = fill[i] = -1;
    if (i * 256 >= w) break;
    const int q = i * 256 + tid, q64 = i * 256 + wave * 64;
    const bool on = q < w && key[q] != kHole;
    const unsigned long long b = __ballot(on);
    if (q >= w) continue;
    if (on) {
      shown[i] = fill[i] = (int32_t)(uint32_t)key[q];
      continue;
    }
    const unsigned long long below = b & ((1ull << lane) - 1ull), above = b & ~((1ull << lane) - 1ull);  // (this lane's bit is clear)
    const int l = below ? q64 + 63 - __clzll((long long)below) : seg_left[i * 4 + wave];
    const int r = above ? q64 + __ffsll(above) - 1 : seg_right[i * 4 + wave];
    if (r < w) {
      const unsigned long long kr = key[r];
      fill[i] = (int32_t)(uint32_t)kr;
      if (l >= 0) {
        const unsigned long long kl = key[l];
        if (!((uint32_t)(kr >> 32) > (uint32_t)(kl >> 32))) fill[i] = (int32_t)(uint32_t)kl;
      }
    } else if (l >= 0) {
      fill[i] = (int32_t)(uint32_t)key[l];
    }
  }
}

}  // namespace
}  // namespace prv2
