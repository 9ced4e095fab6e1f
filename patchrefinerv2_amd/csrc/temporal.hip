// Temporal stabilisation of depth maps across video frames (include/prv2.h "Temporal stabilisation"): a frame's metric map is aligned
// to the previous OUTPUT by a gated least-squares scale and shift, then blended with it where the image has not changed.  Per frame,
// in order on the stream:
//
//   temporal_fit_kernel        the frame's luma from its image (stored: it is the next frame's state), the masks and the exact integer
//                              sums of the 2 x 2 normal equations as per-block int64 partials
//   temporal_fit_final_kernel  the partials summed; reset / identity / fit decided and the coefficients written to the frame's stats
//                              row in DEVICE memory (no host round trip between the passes)
//   temporal_apply_kernel      reads the coefficients from that row; writes the output map (and, for a call's last frame, the state)
//                              and the per-block change sums
//   temporal_sum_final_kernel  the change partials summed into the stats row
//
// A block owns kRows rows x kCols columns, a thread one quad of columns which it walks down the rows (16-byte accesses of the maps and
// 4-byte accesses of the luma when the rows are aligned, else element by element).  Every sum is an int64 of integers: exact, so the
// order of the additions cannot show; a wave reduces by shuffles, the four waves through LDS, the partials in a final block -- no
// atomics.  n frames of a call are a chain of these four launches; the grid of a frame does not depend on n.  Every float64 step is one
// IEEE operation (the file is built with -ffp-contract=off and the multiply-adds are spelled __dmul_rn / __dadd_rn), which is what makes
// the bits equal temporal.temporal_step_host.
#include "temporal_kernels.h"

using namespace prv2;

extern "C" int64_t prv2_temporal_workspace_bytes(int32_t h, int32_t w) {
  if (h < 1 || w < 1 || (int64_t)h * w > kMaxPixels || cdiv(h, kRows) > 65535) return -1;
  return temporal_blocks(h, w) * kPart * (int64_t)sizeof(int64_t);
}

extern "C" int prv2_temporal_step(const float* depth, const float* image, int32_t n, int32_t h, int32_t w, int32_t ih, int32_t iw, double alpha,
                                  int32_t tau, double rho, double anchor, float* state_depth, uint8_t* luma0, uint8_t* luma1,
                                  int32_t state_present, float* out, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "temporal_step";
  PRV2_REQUIRE(depth && image && state_depth && luma0 && luma1 && out && stats, "%s: null pointer", name);
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
  PRV2_REQUIRE(state_present == 0 || state_present == 1, "%s: state_present %d: 0 or 1", name, state_present);
  PRV2_REQUIRE(luma0 != luma1, "%s: the two luma buffers must differ (the apply pass reads the previous luma beside the new one)", name);
  PRV2_REQUIRE(out != depth && state_depth != depth, "%s: out and the state must not alias the input map", name);
  PRV2_REQUIRE(aligned(depth, 4) && aligned(image, 4) && aligned(state_depth, 4) && aligned(out, 4), "%s: misaligned fp32 pointer", name);
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 8) && aligned(stats, 8), "%s: null or misaligned workspace / stats", name);
  const int64_t need = prv2_temporal_workspace_bytes(h, w);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_temporal_workspace_bytes)", name, (long long)workspace_bytes,
               (long long)need);
  const int64_t hw = (int64_t)h * w;
  const int nblk = (int)temporal_blocks(h, w);
  const long long min_count = hw / 100 > 64 ? hw / 100 : 64;
  int64_t* part = (int64_t*)workspace;
  uint8_t* luma[2] = {luma0, luma1};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv(w, kCols), (unsigned)cdiv(h, kRows)), block(256);
  TemporalArgs a;
  a.h = h, a.w = w, a.ih = ih, a.iw = iw, a.tau = tau;
  a.vec = w % 4 == 0 && aligned(depth, 16) && aligned(state_depth, 16) && aligned(out, 16) && aligned(luma0, 4) && aligned(luma1, 4);
  a.vimg = a.vec && ih == h && iw == w && aligned(image, 16);
  for (int f = 0; f < n; ++f) {  // a chain: frame f reads the output of frame f - 1
    a.x = depth + f * hw;
    a.image = image + (int64_t)f * 3 * ih * iw;
    a.prev = f == 0 ? state_depth : out + (f - 1) * hw;
    a.has_prev = f == 0 ? state_present : 1;
    a.lprev = luma[f & 1], a.lcur = luma[(f + 1) & 1];
    a.out = out + f * hw;
    a.state = f == n - 1 && out + f * hw != state_depth ? state_depth : nullptr;
    int64_t* row = stats + (int64_t)f * K;
    hipLaunchKernelGGL(temporal_fit_kernel, grid, block, 0, s, a, part);
    hipLaunchKernelGGL(temporal_fit_final_kernel, dim3(1), block, 0, s, (const int64_t*)part, nblk, min_count, anchor, row);
    hipLaunchKernelGGL(temporal_apply_kernel, grid, block, 0, s, a, (const int64_t*)row, alpha, rho, part);
    hipLaunchKernelGGL(temporal_sum_final_kernel, dim3(1), block, 0, s, (const int64_t*)part, nblk, row);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
