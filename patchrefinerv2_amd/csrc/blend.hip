// Overlap blend: the reference's RunningAverageMap (estimator/models/utils.py:22-49) kept on
// the device.  The running mean is ORDER dependent and has a ct>0 predicate (pass-1 pixels with
// zero Gaussian weight keep their pasted value), so it cannot be a sum(w*p)/sum(w).  To stay
// order-exact AND parallel, each thread owns one map pixel and walks the tile list in order
// (gather form): K is small (<= a few dozen), the maps are HBM-resident, one read + one write
// of the touched pixels per call.
// Frames (the *_frames entry points): B maps [B, MH, MW], grid.y = frame; frame f's tiles / predictions start at f * tile_fs /
// f * pred_fs (a frame-major tile list: the pass's tiles of every frame in one launch, no copies).  The single-frame entry
// points are the FR = false instances of the same kernels.
// Overlap statistics (the *_stats entry points, STATS = true): two more maps per frame -- m2, the weighted sum of squared
// deviations of the tile predictions from the running mean (West's weighted update), and ntl, the number of tiles whose
// footprint covers the pixel.  paste: m2 = 0, ntl = 1; update, per covering tile: ntl += 1, and when ct > 0
// m2 += ct (p - a_old)(p - a_new) = (c ct / (c + ct)) (p - a_old)^2.  avg / cnt are computed by the same expressions as without
// statistics (bit-identical depth); m2 / ntl are read only for pixels a tile of the launch covers.  The STATS = false instances
// compile to the instructions they had before the flag (the two pointer arguments are unused there).
#include "common.h"

PRV2_NO_PACKED_FP32_BEGIN  // (common.h)

namespace prv2 {

template <bool PASTE, bool FR = false, bool STATS = false>
__global__ void __launch_bounds__(256) blend_kernel(float* __restrict__ avg, float* __restrict__ cnt, int MH, int MW,
                                                    const float* __restrict__ pred, int ph, int pw,
                                                    const float* __restrict__ mask, const int* __restrict__ tiles, int K,
                                                    int th, int tw, float sy, float sx, int y_lo, int x_lo, int bh,
                                                    int bw, int64_t pred_fs = 0, int tile_fs = 0, float* __restrict__ m2 = nullptr,
                                                    float* __restrict__ ntl = nullptr) {
  if constexpr (FR) {  // this block's frame: its map, its tiles, its predictions
    const int f = blockIdx.y;
    avg += (int64_t)f * MH * MW;
    cnt += (int64_t)f * MH * MW;
    pred += (int64_t)f * pred_fs;
    tiles += (int64_t)f * 2 * tile_fs;
    if constexpr (STATS) {
      m2 += (int64_t)f * MH * MW;
      ntl += (int64_t)f * MH * MW;
    }
  }
  // threads cover the bounding box [y_lo, y_lo+bh) x [x_lo, x_lo+bw) of all tiles
  int64_t total = (int64_t)bh * bw;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int x = x_lo + (int)(idx % bw);
    int y = y_lo + (int)(idx / bw);
    int64_t o = (int64_t)y * MW + x;
    float a = avg[o], c = cnt[o];
    bool touched = false;
    float s = 0.f, n = 0.f;  // (STATS) this pixel's m2 / ntl, loaded at the first tile that covers it
    bool covered = false;
    for (int k = 0; k < K; ++k) {
      int h0 = tiles[2 * k], w0 = tiles[2 * k + 1];
      int ty = y - h0, tx = x - w0;
      if (ty < 0 || ty >= th || tx < 0 || tx >= tw) continue;
      float ct = mask[(int64_t)ty * tw + tx];
      int py = (ph == th) ? ty : nearest_src(ty, sy, ph);
      int px = (pw == tw) ? tx : nearest_src(tx, sx, pw);
      float p = pred[((int64_t)k * ph + py) * pw + px];
      if (PASTE) {
        // count_map[tile] = blur_mask ; pred_depth[tile] = temp_depth   (baseline_pretrain.py:352-355)
        a = p;
        c = ct;
        touched = true;
        if constexpr (STATS) {
          s = 0.f;
          n = 1.f;
          covered = true;
        }
      } else {
        if constexpr (STATS) {
          if (!covered) {
            s = m2[o];
            n = ntl[o];
            covered = true;
          }
          n += 1.f;  // every covering tile counts, whatever its weight
        }
        if (ct > 0.f) {
          // avg = (p*ct + count*avg) / (count + ct) ; count += ct          (utils.py:31-36)
          float num = p * ct + c * a;
          float den = c + ct;
          // m2 += ct d (p - a_new) with d = p - a_old, written as its exact equal (c ct / (c + ct)) d^2: no cancellation in
          // p - a_new (a pixel of zero weight, c = 0, adds exactly nothing) and never negative
          if constexpr (STATS) s += (c * ct / den) * ((p - a) * (p - a));
          a = num / den;
          c = den;
          touched = true;
        }
      }
    }
    if (touched) {
      avg[o] = a;
      cnt[o] = c;
    }
    if constexpr (STATS) {
      if (covered) {
        m2[o] = s;
        ntl[o] = n;
      }
    }
  }
}

template <bool FR = false, bool STATS = false>
__global__ void __launch_bounds__(256) blend_resize_kernel(const float* __restrict__ avg, const float* __restrict__ cnt,
                                                           int H, int W, float* __restrict__ avg_o,
                                                           float* __restrict__ cnt_o, int oh, int ow, float ny, float nx,
                                                           float by, float bx, const float* __restrict__ m2 = nullptr,
                                                           const float* __restrict__ ntl = nullptr, float* __restrict__ m2_o = nullptr,
                                                           float* __restrict__ ntl_o = nullptr) {
  if constexpr (FR) {
    const int f = blockIdx.y;
    avg += (int64_t)f * H * W;
    cnt += (int64_t)f * H * W;
    avg_o += (int64_t)f * oh * ow;
    cnt_o += (int64_t)f * oh * ow;
    if constexpr (STATS) {
      m2 += (int64_t)f * H * W;
      ntl += (int64_t)f * H * W;
      m2_o += (int64_t)f * oh * ow;
      ntl_o += (int64_t)f * oh * ow;
    }
  }
  int64_t total = (int64_t)oh * ow;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int ox = (int)(idx % ow), oy = (int)(idx / ow);
    avg_o[idx] = avg[(int64_t)nearest_src(oy, ny, H) * W + nearest_src(ox, nx, W)];
    AxisTap ty = ac_tap(oy, by, H), tx = ac_tap(ox, bx, W);
    float v00 = cnt[(int64_t)ty.i0 * W + tx.i0], v01 = cnt[(int64_t)ty.i0 * W + tx.i1];
    float v10 = cnt[(int64_t)ty.i1 * W + tx.i0], v11 = cnt[(int64_t)ty.i1 * W + tx.i1];
    float c_o = ty.w0 * (tx.w0 * v00 + tx.w1 * v01) + ty.w1 * (tx.w0 * v10 + tx.w1 * v11);
    cnt_o[idx] = c_o;
    if constexpr (STATS) {
      // the nearest source pixel's variance m2 / cnt, rescaled to the resampled weight; the tile count is resampled nearest
      int64_t src = (int64_t)nearest_src(oy, ny, H) * W + nearest_src(ox, nx, W);
      float c_s = cnt[src];
      float var = c_s > 0.f ? m2[src] / c_s : 0.f;
      m2_o[idx] = var * c_o;
      ntl_o[idx] = ntl[src];
    }
  }
}

template <bool PASTE, bool STATS = false>
static int blend_launch(const char* name, float* avg, float* cnt, int MH, int MW, const float* pred, int ph, int pw,
                        const float* mask, const int* tiles, int K, int th, int tw, void* stream, int B = 0, int64_t pred_fs = 0,
                        int tile_fs = 0, float* m2 = nullptr, float* ntl = nullptr) {
  PRV2_REQUIRE(avg && cnt && pred && mask && tiles, "%s: null pointer", name);
  if constexpr (STATS) PRV2_REQUIRE(m2 && ntl, "%s: null pointer (m2 / ntiles)", name);
  PRV2_REQUIRE(K > 0 && th > 0 && tw > 0 && ph > 0 && pw > 0 && th <= MH && tw <= MW, "%s: bad geometry", name);
  // tile coordinates live on the device; cover the whole map (cheap: one pass over <= 33 MB maps)
  int64_t total = (int64_t)MH * MW;
  if (B == 0) {  // (the single-frame entry points)
    hipLaunchKernelGGL(blend_kernel<PASTE>, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, avg, cnt, MH, MW,
                       pred, ph, pw, mask, tiles, K, th, tw, (float)ph / (float)th, (float)pw / (float)tw, 0, 0, MH, MW, 0, 0, nullptr, nullptr);
  } else {
    PRV2_REQUIRE(B >= 1 && B <= 65535, "%s: frame count %d out of range [1, 65535]", name, B);
    // frames must not overlap: frame f's K predictions / tiles lie in [f * stride, f * stride + K)
    PRV2_REQUIRE(tile_fs >= K && pred_fs >= (int64_t)K * ph * pw, "%s: frame strides (tiles %d, predictions %lld) smaller than the pass (%d tiles)",
                 name, tile_fs, (long long)pred_fs, K);
    hipLaunchKernelGGL((blend_kernel<PASTE, true, STATS>), dim3(flat_grid(total, 256), B), dim3(256), 0, (hipStream_t)stream, avg, cnt, MH, MW,
                       pred, ph, pw, mask, tiles, K, th, tw, (float)ph / (float)th, (float)pw / (float)tw, 0, 0, MH, MW, pred_fs, tile_fs, m2, ntl);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace prv2

using namespace prv2;

extern "C" int prv2_blend_paste(float* avg, float* cnt, int32_t map_h, int32_t map_w, const float* pred, int32_t ph,
                                int32_t pw, const float* mask, const int32_t* tiles, int32_t k, int32_t th, int32_t tw,
                                void* stream) {
  return blend_launch<true>("blend_paste", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream);
}

extern "C" int prv2_blend_update(float* avg, float* cnt, int32_t map_h, int32_t map_w, const float* pred, int32_t ph,
                                 int32_t pw, const float* mask, const int32_t* tiles, int32_t k, int32_t th, int32_t tw,
                                 void* stream) {
  return blend_launch<false>("blend_update", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream);
}

extern "C" int prv2_blend_paste_frames(float* avg, float* cnt, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred, int32_t ph,
                                       int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride, int32_t k,
                                       int32_t th, int32_t tw, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "blend_paste_frames: n_frames %d < 1", n_frames);
  return blend_launch<true>("blend_paste_frames", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream, n_frames, pred_fstride,
                            tile_fstride);
}

extern "C" int prv2_blend_update_frames(float* avg, float* cnt, int32_t n_frames, int32_t map_h, int32_t map_w, const float* pred, int32_t ph,
                                        int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles, int32_t tile_fstride, int32_t k,
                                        int32_t th, int32_t tw, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "blend_update_frames: n_frames %d < 1", n_frames);
  return blend_launch<false>("blend_update_frames", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream, n_frames, pred_fstride,
                             tile_fstride);
}

static int blend_resize_launch(const char* name, const float* avg, const float* cnt, int B, int h, int w, float* avg_out, float* cnt_out, int oh,
                               int ow, void* stream, const float* m2 = nullptr, const float* ntl = nullptr, float* m2_out = nullptr,
                               float* ntl_out = nullptr) {
  PRV2_REQUIRE(avg && cnt && avg_out && cnt_out && h > 0 && w > 0 && oh > 0 && ow > 0, "%s: bad arguments", name);
  int64_t total = (int64_t)oh * ow;
  if (B == 0)
    hipLaunchKernelGGL(blend_resize_kernel, dim3(flat_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, avg, cnt, h, w,
                       avg_out, cnt_out, oh, ow, (float)h / (float)oh, (float)w / (float)ow, ac_scale(h, oh),
                       ac_scale(w, ow), nullptr, nullptr, nullptr, nullptr);
  else if (m2 == nullptr)
    hipLaunchKernelGGL(blend_resize_kernel<true>, dim3(flat_grid(total, 256), B), dim3(256), 0, (hipStream_t)stream, avg, cnt, h, w,
                       avg_out, cnt_out, oh, ow, (float)h / (float)oh, (float)w / (float)ow, ac_scale(h, oh),
                       ac_scale(w, ow), nullptr, nullptr, nullptr, nullptr);
  else
    hipLaunchKernelGGL((blend_resize_kernel<true, true>), dim3(flat_grid(total, 256), B), dim3(256), 0, (hipStream_t)stream, avg, cnt, h, w,
                       avg_out, cnt_out, oh, ow, (float)h / (float)oh, (float)w / (float)ow, ac_scale(h, oh),
                       ac_scale(w, ow), m2, ntl, m2_out, ntl_out);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_blend_resize(const float* avg, const float* cnt, int32_t h, int32_t w, float* avg_out,
                                 float* cnt_out, int32_t oh, int32_t ow, void* stream) {
  return blend_resize_launch("blend_resize", avg, cnt, 0, h, w, avg_out, cnt_out, oh, ow, stream);
}

extern "C" int prv2_blend_resize_frames(const float* avg, const float* cnt, int32_t n_frames, int32_t h, int32_t w, float* avg_out,
                                        float* cnt_out, int32_t oh, int32_t ow, void* stream) {
  PRV2_REQUIRE(n_frames >= 1 && n_frames <= 65535, "blend_resize_frames: frame count %d out of range [1, 65535]", n_frames);
  return blend_resize_launch("blend_resize_frames", avg, cnt, n_frames, h, w, avg_out, cnt_out, oh, ow, stream);
}

// ---- overlap statistics (the STATS = true instances; B >= 1 frames, frame strides as the *_frames entry points) ------------------
extern "C" int prv2_blend_paste_stats(float* avg, float* cnt, float* m2, float* ntiles, int32_t n_frames, int32_t map_h, int32_t map_w,
                                      const float* pred, int32_t ph, int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles,
                                      int32_t tile_fstride, int32_t k, int32_t th, int32_t tw, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "blend_paste_stats: n_frames %d < 1", n_frames);
  return blend_launch<true, true>("blend_paste_stats", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream, n_frames, pred_fstride,
                                  tile_fstride, m2, ntiles);
}

extern "C" int prv2_blend_update_stats(float* avg, float* cnt, float* m2, float* ntiles, int32_t n_frames, int32_t map_h, int32_t map_w,
                                       const float* pred, int32_t ph, int32_t pw, int64_t pred_fstride, const float* mask, const int32_t* tiles,
                                       int32_t tile_fstride, int32_t k, int32_t th, int32_t tw, void* stream) {
  PRV2_REQUIRE(n_frames >= 1, "blend_update_stats: n_frames %d < 1", n_frames);
  return blend_launch<false, true>("blend_update_stats", avg, cnt, map_h, map_w, pred, ph, pw, mask, tiles, k, th, tw, stream, n_frames, pred_fstride,
                                   tile_fstride, m2, ntiles);
}

extern "C" int prv2_blend_resize_stats(const float* avg, const float* cnt, const float* m2, const float* ntiles, int32_t n_frames, int32_t h, int32_t w,
                                       float* avg_out, float* cnt_out, float* m2_out, float* ntiles_out, int32_t oh, int32_t ow, void* stream) {
  PRV2_REQUIRE(n_frames >= 1 && n_frames <= 65535, "blend_resize_stats: n_frames %d out of range [1, 65535]", n_frames);
  PRV2_REQUIRE(m2 && ntiles && m2_out && ntiles_out, "blend_resize_stats: null pointer (m2 / ntiles)");
  return blend_resize_launch("blend_resize_stats", avg, cnt, n_frames, h, w, avg_out, cnt_out, oh, ow, stream, m2, ntiles, m2_out, ntiles_out);
}

PRV2_NO_PACKED_FP32_END
