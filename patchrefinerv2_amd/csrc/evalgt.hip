// Dataset evaluation with ground truth (include/prv2.h "Ground-truth evaluation"): the device half of UnrealStereo4kDataset
// (estimator/datasets/u4k_dataset.py:120-233) and the sums behind compute_metrics (estimator/utils/metric.py:11-149).
//
//   u8_image_kernel       raw BGR bytes [h, w, 3] -> CHW fp32 / 255                                (u4k_dataset.py:125-147)
//   disp_gt_kernel        disparity -> depth = factor / disp and the boundary map, one pass        (u4k_dataset.py:128-129,216)
//   gt_decode_kernel      the general dataset's ground truth (ETH3D / Middlebury PFM / Cityscapes PNG samples) -> depth and the
//                         boundary map, one pass                                                   (general_dataset.py:103-151)
//   cityscapes_gt_kernel  CityScapesDataset's ground truth: the same decode with the frame's own factor, the noisy bands, the sky class,
//                         the boundary map of the final depth and the float segmentation map, one pass  (cityscapes_dataset.py:153-174,300)
//   depth16_gt_kernel     KittiDataset's / ScanNetDataset's ground truth: the 16-bit samples of a depth PNG read through a window (the
//                         kb-crop) or Pillow's NEAREST resize, / 256 or / 1000, and the boundary map of the re-gridded map, one pass
//                                                                                        (kitti_dataset.py:123-142, scannet_dataset.py:112-132)
//   cityscapes_masks_kernel  the edge and flatten pixel sets of CityScapesDataset.get_metrics, one pass  (cityscapes_dataset.py:360-365)
//   depth_metrics_kernel  the twelve sums of compute_errors + soft_edge_error of B frames, for up to three pixel sets at once
//   metrics_final_kernel  the per-block partials of a frame summed in block order
//   image_grad_kernel / edge_dilate_kernel / edge_region_kernel   ETHDataset's edge area from the IMAGE gradient: Sobel magnitude summed
//                         over the channels and its maximum, threshold + 3 x 3 dilation at image size, the non-zero taps of the
//                         bilinear(align_corners=True) resize at ground-truth size                    (eth_dataset.py:261-272)
//
// The metrics kernel is one streaming read of gt / pred / boundary / region: a block owns a fixed run of rows, a thread four pixels
// of a row at a time (float4 / uchar4 loads when the rows are 16-byte aligned), the per-pixel terms are float64 from the float32
// values, each thread keeps its 12 x S accumulators in registers, a wave reduces by shuffles, the four waves through LDS, and every
// block stores its partial; the final kernel adds the partials in block order.  No floating-point atomics anywhere: the sums are the
// same bits on every call.  Only boundary pixels (sparse) look at the 3 x 3 neighbourhood of gt, straight from L2.
// The LOWRES instances sample a prediction of another resolution where the others load it (bilinear, align_corners=False, the
// operations of PyTorch's upsample_bilinear2d kernel): the resized map is never written.
#include <limits.h>

#include "evalgt_terms.h"

namespace prv2 {
namespace {

constexpr int kTerms = 12;        // sums per pixel set (include/prv2.h prv2_depth_metrics): kErrTerms error sums, then the boundary's two
constexpr int kMaxSets = 3;       // all / inside the region / outside it
constexpr int kMaxBlocks = 1024;  // row blocks per frame

static inline int rows_per_block(int h) { return (int)cdiv(h, kMaxBlocks); }
static inline int row_blocks(int h) { return (int)cdiv(h, rows_per_block(h)); }

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) u8_image_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t hw, int swap_rb,
                                                       int vec) {
  const int64_t quads = (hw + 3) / 4;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p0 = q * 4;
    if (vec) {  // hw % 4 == 0, src 4-byte and dst 16-byte aligned: 12 bytes in, one float4 per plane out
      const uint32_t* s = reinterpret_cast<const uint32_t*>(src + p0 * 3);
      const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
      uint8_t b[12];
      for (int k = 0; k < 4; ++k) {
        b[k] = (uint8_t)(w0 >> (8 * k));
        b[4 + k] = (uint8_t)(w1 >> (8 * k));
        b[8 + k] = (uint8_t)(w2 >> (8 * k));
      }
      for (int c = 0; c < 3; ++c) {
        const int sc = swap_rb ? 2 - c : c;
        float4 v;
        v.x = (float)b[sc] / 255.0f;  // IEEE division (hipcc's default): numpy's float32 / 255.0
        v.y = (float)b[3 + sc] / 255.0f;
        v.z = (float)b[6 + sc] / 255.0f;
        v.w = (float)b[9 + sc] / 255.0f;
        *reinterpret_cast<float4*>(dst + c * hw + p0) = v;
      }
    } else {
      for (int k = 0; k < 4 && p0 + k < hw; ++k)
        for (int c = 0; c < 3; ++c) dst[c * hw + p0 + k] = (float)src[(p0 + k) * 3 + (swap_rb ? 2 - c : c)] / 255.0f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// four pixels x0 .. x0 + 3 of row y per thread (load4, evalgt_terms.h); the neighbours above / below come as rows, left / right as single loads
__global__ void __launch_bounds__(256) disp_gt_kernel(const float* __restrict__ disp, float* __restrict__ depth, uint8_t* __restrict__ boundary,
                                                      int h, int w, float factor, float th, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    const float* row = disp + (int64_t)y * w;
    float c[4], up[4], dn[4];
    load4(row, x0, w, vec, c);
    if (y > 0) load4(row - w, x0, w, vec, up);
    if (y + 1 < h) load4(row + w, x0, w, vec, dn);
    const float left = x0 > 0 ? row[x0 - 1] : 0.f, right = x0 + 4 < w ? row[x0 + 4] : 0.f;
    float d[4];
    uint8_t e[4];
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      d[k] = factor / c[k];  // IEEE: disp == 0 -> inf, NaN stays
      bool b = false;        // |difference| > th; a comparison with NaN is false, a frame border has no neighbour
      if (y > 0) b |= fabsf(c[k] - up[k]) > th;
      if (y + 1 < h) b |= fabsf(dn[k] - c[k]) > th;
      if (x > 0) b |= fabsf(c[k] - (k ? c[k - 1] : left)) > th;
      if (x + 1 < w) b |= fabsf((k < 3 ? c[k + 1] : right) - c[k]) > th;
      e[k] = b ? 1 : 0;
    }
    const int64_t o = (int64_t)y * w + x0;
    if (vec) {
      *reinterpret_cast<float4*>(depth + o) = make_float4(d[0], d[1], d[2], d[3]);
      *reinterpret_cast<uint32_t*>(boundary + o) = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) {
        depth[o + k] = d[k];
        boundary[o + k] = e[k];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// gt_decode: the raw samples of four pixels as 32-bit words (a uint16 sample zero-extended), zero behind the row's end
template <int KIND>
__device__ __forceinline__ void load_raw4(const void* __restrict__ src, int64_t row, int x0, int w, int vec, int bswap, uint32_t* r) {
  if (KIND == PRV2_GT_CITYSCAPES) {
    const uint16_t* s = reinterpret_cast<const uint16_t*>(src) + row * w;
    if (vec) {
      const uint2 t = *reinterpret_cast<const uint2*>(s + x0);
      r[0] = t.x & 0xffffu, r[1] = t.x >> 16, r[2] = t.y & 0xffffu, r[3] = t.y >> 16;
    } else {
      for (int k = 0; k < 4; ++k) r[k] = x0 + k < w ? s[x0 + k] : 0u;
    }
    if (bswap)
      for (int k = 0; k < 4; ++k) r[k] = ((r[k] & 0xffu) << 8) | (r[k] >> 8);
  } else {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src) + row * w;
    if (vec) {
      const uint4 t = *reinterpret_cast<const uint4*>(s + x0);
      r[0] = t.x, r[1] = t.y, r[2] = t.z, r[3] = t.w;
    } else {
      for (int k = 0; k < 4; ++k) r[k] = x0 + k < w ? s[x0 + k] : 0u;
    }
    if (bswap)
      for (int k = 0; k < 4; ++k) r[k] = __builtin_bswap32(r[k]);
  }
}

template <int KIND>
__device__ __forceinline__ uint32_t load_raw1(const void* __restrict__ src, int64_t row, int x, int w, int bswap) {
  if (KIND == PRV2_GT_CITYSCAPES) {
    const uint32_t v = reinterpret_cast<const uint16_t*>(src)[row * w + x];
    return bswap ? ((v & 0xffu) << 8) | (v >> 8) : v;
  }
  const uint32_t v = reinterpret_cast<const uint32_t*>(src)[row * w + x];
  return bswap ? __builtin_bswap32(v) : v;
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one sample -> its depth and the value the reference takes its edges from (numpy's float32 operations in numpy's order)
template <int KIND>
__device__ __forceinline__ void gt_decode1(uint32_t raw, float factor, float doffs, float& depth, float& edge) {
  if (KIND == PRV2_GT_ETH3D) {  // np.nan_to_num(depth, posinf=0., neginf=0., nan=0.)
    const float v = __uint_as_float(raw);
    depth = edge = finite_f32(v) ? v : 0.f;
  } else if (KIND == PRV2_GT_MIDDLEBURY) {  // invalid = disp == inf; depth = factor / (disp + doffs) / 1000; both 0 where invalid
    const float v = __uint_as_float(raw);
    const bool inv = raw == 0x7f800000u;
    const float t = (factor / (v + doffs)) / 1000.0f;
    depth = inv ? 0.f : t;
    edge = inv ? 0.f : v;
  } else {  // img_d[img_d > 0] = (img_d[img_d > 0] - 1) / 256; depth = factor / img_d; nan_to_num
    const float f = (float)raw;
    const float t = raw > 0u ? (f - 1.0f) / 256.0f : f;
    const float q = factor / t;
    depth = edge = finite_f32(q) ? q : 0.f;
  }
}

template <int KIND>
__global__ void __launch_bounds__(256) gt_decode_kernel(const void* __restrict__ src, float* __restrict__ depth, uint8_t* __restrict__ boundary,
                                                        int h, int w, float factor, float doffs, float th, int flip, int bswap, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    // output row y is source row sy; the rows above / below it in the output are sy - sd / sy + sd
    const int64_t sy = flip ? h - 1 - y : y, sd = flip ? -1 : 1;
    uint32_t rc[4], ru[4], rd[4];
    float d[4], c[4], up[4], dn[4], left = 0.f, right = 0.f, unused;
    load_raw4<KIND>(src, sy, x0, w, vec, bswap, rc);
    for (int k = 0; k < 4; ++k) gt_decode1<KIND>(rc[k], factor, doffs, d[k], c[k]);
    if (y > 0) {
      load_raw4<KIND>(src, sy - sd, x0, w, vec, bswap, ru);
      for (int k = 0; k < 4; ++k) gt_decode1<KIND>(ru[k], factor, doffs, unused, up[k]);
    }
    if (y + 1 < h) {
      load_raw4<KIND>(src, sy + sd, x0, w, vec, bswap, rd);
      for (int k = 0; k < 4; ++k) gt_decode1<KIND>(rd[k], factor, doffs, unused, dn[k]);
    }
    if (x0 > 0) gt_decode1<KIND>(load_raw1<KIND>(src, sy, x0 - 1, w, bswap), factor, doffs, unused, left);
    if (x0 + 4 < w) gt_decode1<KIND>(load_raw1<KIND>(src, sy, x0 + 4, w, bswap), factor, doffs, unused, right);
    uint8_t e[4];
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      bool b = false;  // the rule of disp_gt_kernel
      if (y > 0) b |= fabsf(c[k] - up[k]) > th;
      if (y + 1 < h) b |= fabsf(dn[k] - c[k]) > th;
      if (x > 0) b |= fabsf(c[k] - (k ? c[k - 1] : left)) > th;
      if (x + 1 < w) b |= fabsf((k < 3 ? c[k + 1] : right) - c[k]) > th;
      e[k] = b ? 1 : 0;
    }
    const int64_t o = (int64_t)y * w + x0;
    if (vec) {
      *reinterpret_cast<float4*>(depth + o) = make_float4(d[0], d[1], d[2], d[3]);
      *reinterpret_cast<uint32_t*>(boundary + o) = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) {
        depth[o + k] = d[k];
        boundary[o + k] = e[k];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// CityScapesDataset's ground truth (cityscapes_dataset.py:153-174, :300): gt_decode1<PRV2_GT_CITYSCAPES>, then -1 in the noisy bands
// (the last ceil(h / 4) rows, the first w / 16 and the last ceil(w / 16) columns), then 0 where the colour segmentation map shows the
// sky class (R == 70 and G == 130); the boundary map is taken from THAT map, so every neighbour is decoded the same way.
struct CsBands {
  int y1, x0, x1;  // a pixel is in a band when y >= y1 or x < x0 or x >= x1
};

// the R and G bytes of four pixels of a [h, w, 3] byte map (the 12 bytes as three words when vec), zero behind the row's end
__device__ __forceinline__ void load_seg4(const uint8_t* __restrict__ seg, int64_t row, int x0, int w, int vec, uint8_t* b) {
  const uint8_t* s = seg + (row * w + x0) * 3;
  if (vec) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(s);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    for (int k = 0; k < 4; ++k) {
      b[k] = (uint8_t)(w0 >> (8 * k));
      b[4 + k] = (uint8_t)(w1 >> (8 * k));
      b[8 + k] = (uint8_t)(w2 >> (8 * k));
    }
  } else {
    for (int k = 0; k < 12; ++k) b[k] = x0 + k / 3 < w ? s[k] : 0;
  }
}

__device__ __forceinline__ float cs_value(uint32_t raw, float factor, bool band, bool sky) {
  float d, unused;
  gt_decode1<PRV2_GT_CITYSCAPES>(raw, factor, 0.f, d, unused);
  return sky ? 0.f : (band ? -1.0f : d);
}

// the final values of the four pixels x0 .. x0 + 3 of row y (b: the row's segmentation bytes, as load_seg4 leaves them)
template <bool SEG>
__device__ __forceinline__ void cs_row4(const uint16_t* __restrict__ disp, const uint8_t* __restrict__ seg, int y, int x0, int w, int vec,
                                        float factor, CsBands bd, float* v, uint8_t* b) {
  uint32_t r[4];
  load_raw4<PRV2_GT_CITYSCAPES>(disp, y, x0, w, vec, 0, r);
  if (SEG) load_seg4(seg, y, x0, w, vec, b);
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + k;
    v[k] = cs_value(r[k], factor, y >= bd.y1 || x < bd.x0 || x >= bd.x1, SEG && b[3 * k] == 70 && b[3 * k + 1] == 130);
  }
}

template <bool SEG>
__device__ __forceinline__ float cs_at(const uint16_t* __restrict__ disp, const uint8_t* __restrict__ seg, int y, int x, int w, float factor,
                                       CsBands bd) {
  const int64_t i = (int64_t)y * w + x;
  return cs_value(disp[i], factor, y >= bd.y1 || x < bd.x0 || x >= bd.x1, SEG && seg[i * 3] == 70 && seg[i * 3 + 1] == 130);
}

template <bool SEG>
__global__ void __launch_bounds__(256) cityscapes_gt_kernel(const uint16_t* __restrict__ disp, const uint8_t* __restrict__ seg,
                                                            float* __restrict__ depth, uint8_t* __restrict__ boundary,
                                                            float* __restrict__ seg_out, int h, int w, float factor, CsBands bd, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq, hw = (int64_t)h * w;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    float c[4], up[4], dn[4], left = 0.f, right = 0.f;
    uint8_t b[12], nb[12];
    cs_row4<SEG>(disp, seg, y, x0, w, vec, factor, bd, c, b);
    if (y > 0) cs_row4<SEG>(disp, seg, y - 1, x0, w, vec, factor, bd, up, nb);
    if (y + 1 < h) cs_row4<SEG>(disp, seg, y + 1, x0, w, vec, factor, bd, dn, nb);
    if (x0 > 0) left = cs_at<SEG>(disp, seg, y, x0 - 1, w, factor, bd);
    if (x0 + 4 < w) right = cs_at<SEG>(disp, seg, y, x0 + 4, w, factor, bd);
    uint8_t e[4];
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      bool t = false;  // the rule of disp_gt_kernel with th = 1
      if (y > 0) t |= fabsf(c[k] - up[k]) > 1.0f;
      if (y + 1 < h) t |= fabsf(dn[k] - c[k]) > 1.0f;
      if (x > 0) t |= fabsf(c[k] - (k ? c[k - 1] : left)) > 1.0f;
      if (x + 1 < w) t |= fabsf((k < 3 ? c[k + 1] : right) - c[k]) > 1.0f;
      e[k] = t ? 1 : 0;
    }
    const int64_t o = (int64_t)y * w + x0;
    if (vec) {
      *reinterpret_cast<float4*>(depth + o) = make_float4(c[0], c[1], c[2], c[3]);
      *reinterpret_cast<uint32_t*>(boundary + o) = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
      if (SEG)
        for (int ch = 0; ch < 3; ++ch)
          *reinterpret_cast<float4*>(seg_out + ch * hw + o) = make_float4((float)b[ch], (float)b[3 + ch], (float)b[6 + ch], (float)b[9 + ch]);
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) {
        depth[o + k] = c[k];
        boundary[o + k] = e[k];
        if (SEG)
          for (int ch = 0; ch < 3; ++ch) seg_out[ch * hw + o + k] = (float)b[3 * k + ch];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// KittiDataset's and ScanNetDataset's ground truth (kitti_dataset.py:123-131, :142, :203; scannet_dataset.py:112-118, :132, :188): the
// uint16 samples of a depth PNG, RE-GRIDDED as they are read -- output pixel (y, x) is source pixel (row(y), col(x)) -- then
// depth = float32(sample) / divisor and the boundary map of the OUTPUT map: a neighbour of an output pixel is the output's neighbour,
// mapped through the same rule.
//   window   row(y) = top + y, col(x) = left + x                 (Image.crop: KITTI's kb-crop)
//   NEAREST  row(y) = (int)((y + 0.5) * (sh / H)), likewise col  (Image.resize(NEAREST) of Pillow: ONE float64 product per index, the
//            scale a float64 division made on the host; accumulating the step instead picks other pixels)
struct D16Grid {
  int top, left;  // window
  double sy, sx;  // NEAREST: sh / H and sw / W
};

// the source index of output index i (the clamp never acts on an exact product; it keeps a rounded-up one inside the map)
__device__ __forceinline__ int d16_index(int i, double scale, int n) { return min((int)(((double)i + 0.5) * scale), n - 1); }

// the samples of the four output pixels x0 .. x0 + 3 of one output row (p: the source row, at the window's first column), zero behind
// the row's end.  svec (window only, W % 4 == 0): 2 = the four samples are 8-byte aligned, 1 = 4-byte aligned (an even left margin), 0 =
// neither (KITTI's margin of 13).  cx (NEAREST): the source columns of the output columns x0 - 1 .. x0 + 4.
template <bool NEAREST>
__device__ __forceinline__ void d16_row4(const uint16_t* __restrict__ p, int x0, int W, int svec, const int* cx, float divisor, float* v) {
  uint32_t r[4];
  if (NEAREST) {
    for (int k = 0; k < 4; ++k) r[k] = x0 + k < W ? p[cx[k + 1]] : 0u;
  } else if (svec == 2) {
    const uint2 t = *reinterpret_cast<const uint2*>(p + x0);
    r[0] = t.x & 0xffffu, r[1] = t.x >> 16, r[2] = t.y & 0xffffu, r[3] = t.y >> 16;
  } else if (svec == 1) {
    const uint32_t t0 = *reinterpret_cast<const uint32_t*>(p + x0), t1 = *reinterpret_cast<const uint32_t*>(p + x0 + 2);
    r[0] = t0 & 0xffffu, r[1] = t0 >> 16, r[2] = t1 & 0xffffu, r[3] = t1 >> 16;
  } else {
    for (int k = 0; k < 4; ++k) r[k] = x0 + k < W ? p[x0 + k] : 0u;
  }
  for (int k = 0; k < 4; ++k) v[k] = (float)r[k] / divisor;  // IEEE division: numpy's astype(float32) / 256.0
}

template <bool NEAREST>
__global__ void __launch_bounds__(256) depth16_gt_kernel(const uint16_t* __restrict__ src, float* __restrict__ depth,
                                                         uint8_t* __restrict__ boundary, int sh, int sw, int H, int W, D16Grid g,
                                                         float divisor, float th, int svec, int vec) {
  const int wq = (W + 3) / 4;
  const int64_t quads = (int64_t)H * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    int cx[6] = {0, 0, 0, 0, 0, 0};
    if (NEAREST)
      for (int j = 0; j < 6; ++j) {
        const int X = x0 - 1 + j;
        if (X >= 0 && X < W) cx[j] = d16_index(X, g.sx, sw);
      }
    // the source rows of output rows y - 1, y, y + 1 (at the window's first column)
    const uint16_t* pc = src + (NEAREST ? (int64_t)d16_index(y, g.sy, sh) * sw : (int64_t)(g.top + y) * sw + g.left);
    float c[4], up[4], dn[4], left = 0.f, right = 0.f;
    d16_row4<NEAREST>(pc, x0, W, svec, cx, divisor, c);
    if (y > 0) {
      const uint16_t* pu = src + (NEAREST ? (int64_t)d16_index(y - 1, g.sy, sh) * sw : (int64_t)(g.top + y - 1) * sw + g.left);
      d16_row4<NEAREST>(pu, x0, W, svec, cx, divisor, up);
    }
    if (y + 1 < H) {
      const uint16_t* pd = src + (NEAREST ? (int64_t)d16_index(y + 1, g.sy, sh) * sw : (int64_t)(g.top + y + 1) * sw + g.left);
      d16_row4<NEAREST>(pd, x0, W, svec, cx, divisor, dn);
    }
    if (x0 > 0) left = (float)pc[NEAREST ? cx[0] : x0 - 1] / divisor;
    if (x0 + 4 < W) right = (float)pc[NEAREST ? cx[5] : x0 + 4] / divisor;
    uint8_t e[4];
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      bool b = false;  // the rule of disp_gt_kernel
      if (y > 0) b |= fabsf(c[k] - up[k]) > th;
      if (y + 1 < H) b |= fabsf(dn[k] - c[k]) > th;
      if (x > 0) b |= fabsf(c[k] - (k ? c[k - 1] : left)) > th;
      if (x + 1 < W) b |= fabsf((k < 3 ? c[k + 1] : right) - c[k]) > th;
      e[k] = b ? 1 : 0;
    }
    const int64_t o = (int64_t)y * W + x0;
    if (vec) {
      *reinterpret_cast<float4*>(depth + o) = make_float4(c[0], c[1], c[2], c[3]);
      *reinterpret_cast<uint32_t*>(boundary + o) = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    } else {
      for (int k = 0; k < 4 && x0 + k < W; ++k) {
        depth[o + k] = c[k];
        boundary[o + k] = e[k];
      }
    }
  }
}

// CityScapesDataset.get_metrics' two pixel sets (cityscapes_dataset.py:360-365): edge = seg_edges and dilate7(gt_edges) (the 7 x 7 blur
// > 0: positive weights, the window clipped at the frame), flatten = not edge and not hr_region.  Segmentation edges are sparse: only
// their pixels look at the 7 x 7 window of gt_edges, straight from L2.
__global__ void __launch_bounds__(256) cityscapes_masks_kernel(const uint8_t* __restrict__ seg_edges, const uint8_t* __restrict__ gt_edges,
                                                               const uint8_t* __restrict__ region, uint8_t* __restrict__ edge,
                                                               uint8_t* __restrict__ flatten, int h, int w, int vec) {
  const int wq = (w + 3) / 4;
  const int64_t quads = (int64_t)h * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(q / wq), x0 = (int)(q - (int64_t)y * wq) * 4;
    const int64_t o = (int64_t)y * w + x0;
    uint8_t s[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0}, e[4], f[4];
    if (vec) {
      const uint32_t ts = *reinterpret_cast<const uint32_t*>(seg_edges + o), tr = *reinterpret_cast<const uint32_t*>(region + o);
      for (int k = 0; k < 4; ++k) s[k] = (uint8_t)(ts >> (8 * k)), r[k] = (uint8_t)(tr >> (8 * k));
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) s[k] = seg_edges[o + k], r[k] = region[o + k];
    }
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k;
      uint8_t any = 0;
      if (s[k] && x < w)
        for (int yy = max(y - 3, 0); yy <= min(y + 3, h - 1) && !any; ++yy)
          for (int xx = max(x - 3, 0); xx <= min(x + 3, w - 1); ++xx) any |= gt_edges[(int64_t)yy * w + xx];
      e[k] = any ? 1 : 0;
      f[k] = (!any && !r[k]) ? 1 : 0;
    }
    if (vec) {
      *reinterpret_cast<uint32_t*>(edge + o) = (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
      *reinterpret_cast<uint32_t*>(flatten + o) = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    } else {
      for (int k = 0; k < 4 && x0 + k < w; ++k) edge[o + k] = e[k], flatten[o + k] = f[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
struct MetricArgs {
  const float* gt;
  const float* pred;
  const uint8_t* boundary;  // may be null
  const uint8_t* region;    // may be null (then one set)
  int h, w, rows_per_block, vec;
  float mn, mx;
  int y0, y1, x0, x1;
  int ph, pw;        // LOWRES: pred is [n, ph, pw]
  float sch, scw;    // LOWRES: ph / h and pw / w (fp32 divisions)
};

// (bilinear_src / bilinear_at, clean_pred and error_terms: evalgt_terms.h, shared with csrc/ssi_eval.hip)

// NaN-propagating minimum (np.minimum / torch.minimum)
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (b < a ? b : a); }

// soft_edge_error(radius=1) at one pixel: min over the 3 x 3 shifts of gt (zero outside the frame) of |shift(gt) - pred|, fp32
__device__ __forceinline__ float soft_edge(const float* __restrict__ g, int h, int w, int y, int x, float p) {
  float best = 0.f;
  bool first = true;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      const float v = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? g[(int64_t)yy * w + xx] : 0.f;
      const float d = fabsf(v - p);
      best = first ? d : min_nan(best, d);
      first = false;
    }
  return best;
}

template <int S, bool LOWRES>
__global__ void __launch_bounds__(256) depth_metrics_kernel(MetricArgs a, double* __restrict__ part) {
  __shared__ double sh[4][S * kTerms];
  const int f = blockIdx.y, h = a.h, w = a.w;
  const int64_t fb = (int64_t)f * h * w;
  const float* __restrict__ gt = a.gt + fb;
  const float* __restrict__ pred = a.pred + (LOWRES ? (int64_t)f * a.ph * a.pw : fb);
  const uint8_t* __restrict__ bnd = a.boundary ? a.boundary + fb : nullptr;
  const uint8_t* __restrict__ reg = a.region ? a.region + fb : nullptr;
  double acc[S][kTerms];
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < kTerms; ++k) acc[s][k] = 0.0;

  const int r0 = blockIdx.x * a.rows_per_block;
  const int ya = max(r0, a.y0), yb = min(min(r0 + a.rows_per_block, h), a.y1);
  const int q0 = a.x0 / 4, q1 = (min(a.x1, w) + 3) / 4;  // the quads that touch the crop's columns
  for (int y = ya; y < yb; ++y) {
    const int64_t ro = (int64_t)y * w;
    int sy0 = 0, sys = 0;
    float ly = 0.f;
    if (LOWRES) bilinear_src(a.sch, y, a.ph, sy0, sys, ly);
    const float* __restrict__ pr0 = pred + (int64_t)sy0 * a.pw;  // LOWRES: the two source rows of output row y
    const float* __restrict__ pr1 = pr0 + (int64_t)sys * a.pw;
    for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
      const int x0 = q * 4;
      float g[4], p[4];
      uint8_t b[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
      load4(gt + ro, x0, w, a.vec, g);
      if (LOWRES) {
        for (int k = 0; k < 4; ++k) p[k] = x0 + k < w ? bilinear_at(pr0, pr1, ly, a.scw, x0 + k, a.pw) : 0.f;
      } else {
        load4(pred + ro, x0, w, a.vec, p);
      }
      if (a.vec) {
        if (bnd) {
          const uint32_t t = *reinterpret_cast<const uint32_t*>(bnd + ro + x0);
          for (int k = 0; k < 4; ++k) b[k] = (uint8_t)(t >> (8 * k));
        }
        if (S > 1) {
          const uint32_t t = *reinterpret_cast<const uint32_t*>(reg + ro + x0);
          for (int k = 0; k < 4; ++k) r[k] = (uint8_t)(t >> (8 * k));
        }
      } else {
        for (int k = 0; k < 4 && x0 + k < w; ++k) {
          if (bnd) b[k] = bnd[ro + x0 + k];
          if (S > 1) r[k] = reg[ro + x0 + k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        const float gk = g[k];
        if (!(x >= a.x0 && x < a.x1 && x < w && gk > a.mn && gk < a.mx)) continue;  // a NaN gt is not valid
        const float pk = clean_pred(p[k], a.mn, a.mx);
        double t[kTerms];
        error_terms(gk, pk, t);
        t[10] = 0.0;
        t[11] = 0.0;
        if (b[k]) {
          t[10] = 1.0;
          t[11] = (double)soft_edge(gt, h, w, y, x, pk);
        }
        // the set index never addresses the registers: adding 0.0 leaves a sum's bits alone
        const bool in = S > 1 && r[k] != 0;
#pragma unroll
        for (int j = 0; j < kTerms; ++j) {
          acc[0][j] += t[j];
          if (S > 1) {
            acc[1][j] += in ? t[j] : 0.0;
            acc[S - 1][j] += in ? 0.0 : t[j];
          }
        }
      }
    }
  }
  // wave: shuffles (fixed tree); block: the four waves' sums through LDS, added in wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int j = 0; j < kTerms; ++j) {
      double v = acc[s][j];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if (lane == 0) sh[wave][s * kTerms + j] = v;
    }
  __syncthreads();
  if (threadIdx.x < S * kTerms) {
    const int j = threadIdx.x;
    part[((int64_t)f * gridDim.x + blockIdx.x) * (S * kTerms) + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
  }
}

__global__ void __launch_bounds__(64) metrics_final_kernel(const double* __restrict__ part, double* __restrict__ sums, int nblk, int nval) {
  const int f = blockIdx.x, j = threadIdx.x;
  if (j >= nval) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[((int64_t)f * nblk + b) * nval + j];
  sums[(int64_t)f * nval + j] = s;
}

// ------------------------------------------------------------------------------------------------------------------
// ETHDataset.get_metrics' edge area (eth_dataset.py:261-272).  No float map of ground-truth size exists: the gradient and the byte
// map of the dilated threshold live at image size, the last kernel writes the region's bytes.
//
// kornia.filters.spatial_gradient (Sobel / 8, replicate padding) per channel, m_c = sqrt(gx^2 + gy^2) (a correctly rounded sqrt),
// g = (m_0 + m_1) + m_2; the frame's maximum through an integer atomicMax on the bits of the non-negative floats (order-independent)
__global__ void __launch_bounds__(256) image_grad_kernel(const float* __restrict__ img, int h, int w, float* __restrict__ grad,
                                                         uint32_t* __restrict__ max_bits) {
  __shared__ uint32_t sh[4];
  const int64_t hw = (int64_t)h * w;
  uint32_t best = 0u;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    const int ym = max(y - 1, 0), yp = min(y + 1, h - 1), xm = max(x - 1, 0), xp = min(x + 1, w - 1);
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* p = img + k * hw;
      const float* ru = p + (int64_t)ym * w;
      const float* rc = p + (int64_t)y * w;
      const float* rd = p + (int64_t)yp * w;
      const float gx = (((ru[xp] - ru[xm]) + 2.0f * (rc[xp] - rc[xm])) + (rd[xp] - rd[xm])) * 0.125f;
      const float gy = (((rd[xm] - ru[xm]) + 2.0f * (rd[x] - ru[x])) + (rd[xp] - ru[xp])) * 0.125f;
      const float m = __fsqrt_rn(gx * gx + gy * gy);
      g = k ? g + m : m;
    }
    grad[i] = g;
    best = max(best, __float_as_uint(g));
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_down((int)best, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(max_bits, max(max(sh[0], sh[1]), max(sh[2], sh[3])));
}

// edge = g >= frac * max(g) (fp32), then gaussian_blur2d(3 x 3, reflect) > 0: every weight is positive and reflect stays inside the
// window, so it is the 3 x 3 dilation with the window clipped at the frame.  A constant image has max(g) == 0: every pixel is set.
__global__ void __launch_bounds__(256) edge_dilate_kernel(const float* __restrict__ grad, int h, int w, const uint32_t* __restrict__ max_bits,
                                                          float frac, uint8_t* __restrict__ wide) {
  const float thr = __uint_as_float(*max_bits) * frac;
  const int64_t hw = (int64_t)h * w;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    bool any = false;
    for (int yy = max(y - 1, 0); yy <= min(y + 1, h - 1); ++yy)
      for (int xx = max(x - 1, 0); xx <= min(x + 1, w - 1); ++xx) any |= grad[(int64_t)yy * w + xx] >= thr;
    wide[i] = any ? 1 : 0;
  }
}

// F.interpolate(bilinear, align_corners=True) > 0 of a non-negative map: one of the up to four taps with a NON-ZERO weight is set.
// PyTorch's fp32 source coordinate (ac_tap): the lower tap's weight 1 - lambda1 is never zero, the upper one's is lambda1 -- an
// output that lands exactly on a source pixel does not see the next one.
__device__ __forceinline__ uint8_t edge_region_at(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, bool up, int X, float sx,
                                                  int w) {
  const AxisTap tx = ac_tap(X, sx, w);
  const bool right = tx.w1 > 0.f;
  const bool v = r0[tx.i0] || (right && r0[tx.i1]) || (up && (r1[tx.i0] || (right && r1[tx.i1])));
  return v ? 1 : 0;
}

__global__ void __launch_bounds__(256) edge_region_kernel(const uint8_t* __restrict__ wide, int h, int w, uint8_t* __restrict__ region, int H,
                                                          int W, float sy, float sx, int vec) {
  const int wq = (W + 3) / 4;
  const int64_t quads = (int64_t)H * wq;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int Y = (int)(q / wq), X0 = (int)(q - (int64_t)Y * wq) * 4;
    const AxisTap ty = ac_tap(Y, sy, h);
    const uint8_t* r0 = wide + (int64_t)ty.i0 * w;
    const uint8_t* r1 = wide + (int64_t)ty.i1 * w;
    const bool up = ty.w1 > 0.f;
    const int64_t o = (int64_t)Y * W + X0;
    if (vec) {  // W % 4 == 0 and region 4-byte aligned
      uint32_t v = 0u;
      for (int k = 0; k < 4; ++k) v |= (uint32_t)edge_region_at(r0, r1, up, X0 + k, sx, w) << (8 * k);
      *reinterpret_cast<uint32_t*>(region + o) = v;
    } else {
      for (int k = 0; k < 4 && X0 + k < W; ++k) region[o + k] = edge_region_at(r0, r1, up, X0 + k, sx, w);
    }
  }
}

}  // namespace
}  // namespace prv2

using namespace prv2;

extern "C" int prv2_u8_image(const uint8_t* src, int32_t h, int32_t w, int32_t swap_rb, float* dst, void* stream) {
  const char* name = "u8_image";
  PRV2_REQUIRE(src && dst, "%s: null pointer", name);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w * 3 < (int64_t)INT_MAX, "%s: %d x %d x 3 exceeds 2^31 bytes", name, h, w);
  const int64_t hw = (int64_t)h * w;
  const int vec = hw % 4 == 0 && aligned(src, 4) && aligned(dst, 16);
  hipLaunchKernelGGL(u8_image_kernel, dim3(flat_grid(cdiv(hw, 4), 256)), dim3(256), 0, (hipStream_t)stream, src, dst, hw, swap_rb ? 1 : 0, vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_disp_gt(const float* disp, int32_t h, int32_t w, float factor, float th, float* depth, uint8_t* boundary, void* stream) {
  const char* name = "disp_gt";
  PRV2_REQUIRE(disp && depth && boundary, "%s: null pointer", name);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w < (int64_t)INT_MAX, "%s: %d x %d exceeds 2^31 pixels", name, h, w);
  const int vec = w % 4 == 0 && aligned(disp, 16) && aligned(depth, 16) && aligned(boundary, 4);
  hipLaunchKernelGGL(disp_gt_kernel, dim3(flat_grid((int64_t)h * cdiv(w, 4), 256)), dim3(256), 0, (hipStream_t)stream, disp, depth, boundary,
                     (int)h, (int)w, factor, th, vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int64_t prv2_depth_metrics_workspace_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || n > 65535 || h < 1 || w < 1) return -1;
  return (int64_t)n * row_blocks(h) * kMaxSets * kTerms * (int64_t)sizeof(double);
}

// prv2_depth_metrics (ph == h, pw == w: the prediction is loaded) and prv2_depth_metrics_lowres (it is sampled)
static int depth_metrics_impl(const char* name, const float* gt, const float* pred, const uint8_t* boundary, const uint8_t* region, int32_t n,
                              int32_t h, int32_t w, int32_t ph, int32_t pw, float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0,
                              int32_t x1, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  PRV2_REQUIRE(gt && pred && sums, "%s: null pointer", name);
  PRV2_REQUIRE(n >= 1 && n <= 65535, "%s: frame count %d out of range [1, 65535]", name, n);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE(ph >= 1 && pw >= 1, "%s: bad prediction shape %d x %d", name, ph, pw);
  PRV2_REQUIRE((int64_t)n * h * w < (int64_t)INT_MAX, "%s: %d frames of %d x %d exceed 2^31 pixels", name, n, h, w);
  PRV2_REQUIRE((int64_t)n * ph * pw < (int64_t)INT_MAX, "%s: %d predictions of %d x %d exceed 2^31 pixels", name, n, ph, pw);
  PRV2_REQUIRE(y0 >= 0 && y0 <= y1 && y1 <= h && x0 >= 0 && x0 <= x1 && x1 <= w, "%s: crop rows [%d, %d) columns [%d, %d) outside %d x %d", name,
               y0, y1, x0, x1, h, w);
  PRV2_REQUIRE(workspace != nullptr, "%s: null workspace", name);
  const int64_t need = prv2_depth_metrics_workspace_bytes(n, h, w);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_depth_metrics_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)need);
  const bool lowres = ph != h || pw != w;
  MetricArgs a;
  a.gt = gt, a.pred = pred, a.boundary = boundary, a.region = region;
  a.h = h, a.w = w, a.rows_per_block = rows_per_block(h);
  a.vec = w % 4 == 0 && aligned(gt, 16) && (lowres || aligned(pred, 16)) && aligned(boundary, 4) && aligned(region, 4);
  a.mn = min_depth, a.mx = max_depth;
  a.y0 = y0, a.y1 = y1, a.x0 = x0, a.x1 = x1;
  a.ph = ph, a.pw = pw;
  a.sch = (float)ph / (float)h, a.scw = (float)pw / (float)w;
  const int nblk = row_blocks(h), sets = region ? kMaxSets : 1;
  double* part = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nblk, n), block(256);
  if (region && lowres)
    hipLaunchKernelGGL((depth_metrics_kernel<kMaxSets, true>), grid, block, 0, s, a, part);
  else if (region)
    hipLaunchKernelGGL((depth_metrics_kernel<kMaxSets, false>), grid, block, 0, s, a, part);
  else if (lowres)
    hipLaunchKernelGGL((depth_metrics_kernel<1, true>), grid, block, 0, s, a, part);
  else
    hipLaunchKernelGGL((depth_metrics_kernel<1, false>), grid, block, 0, s, a, part);
  hipLaunchKernelGGL(metrics_final_kernel, dim3(n), dim3(64), 0, s, part, sums, nblk, sets * kTerms);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_depth_metrics(const float* gt, const float* pred, const uint8_t* boundary, const uint8_t* region, int32_t n, int32_t h,
                                  int32_t w, float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0, int32_t x1, double* sums,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return depth_metrics_impl("depth_metrics", gt, pred, boundary, region, n, h, w, h, w, min_depth, max_depth, y0, y1, x0, x1, sums, workspace,
                            workspace_bytes, stream);
}

extern "C" int prv2_depth_metrics_lowres(const float* gt, const float* pred, const uint8_t* boundary, const uint8_t* region, int32_t n, int32_t h,
                                         int32_t w, int32_t ph, int32_t pw, float min_depth, float max_depth, int32_t y0, int32_t y1, int32_t x0,
                                         int32_t x1, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  return depth_metrics_impl("depth_metrics_lowres", gt, pred, boundary, region, n, h, w, ph, pw, min_depth, max_depth, y0, y1, x0, x1, sums,
                            workspace, workspace_bytes, stream);
}

extern "C" int prv2_gt_decode(const void* src, int32_t kind, int32_t h, int32_t w, float factor, float doffs, float th, int32_t flip,
                              int32_t byteswap, float* depth, uint8_t* boundary, void* stream) {
  const char* name = "gt_decode";
  PRV2_REQUIRE(src && depth && boundary, "%s: null pointer", name);
  PRV2_REQUIRE(kind == PRV2_GT_ETH3D || kind == PRV2_GT_MIDDLEBURY || kind == PRV2_GT_CITYSCAPES, "%s: unknown kind %d (enum prv2_gt_kind)", name,
               kind);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w < (int64_t)INT_MAX, "%s: %d x %d exceeds 2^31 pixels", name, h, w);
  const int vec = w % 4 == 0 && aligned(src, kind == PRV2_GT_CITYSCAPES ? 8 : 16) && aligned(depth, 16) && aligned(boundary, 4);
  const dim3 grid(flat_grid((int64_t)h * cdiv(w, 4), 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int fl = flip ? 1 : 0, bs = byteswap ? 1 : 0;
  if (kind == PRV2_GT_ETH3D)
    hipLaunchKernelGGL(gt_decode_kernel<PRV2_GT_ETH3D>, grid, block, 0, s, src, depth, boundary, (int)h, (int)w, factor, doffs, th, fl, bs, vec);
  else if (kind == PRV2_GT_MIDDLEBURY)
    hipLaunchKernelGGL(gt_decode_kernel<PRV2_GT_MIDDLEBURY>, grid, block, 0, s, src, depth, boundary, (int)h, (int)w, factor, doffs, th, fl, bs, vec);
  else
    hipLaunchKernelGGL(gt_decode_kernel<PRV2_GT_CITYSCAPES>, grid, block, 0, s, src, depth, boundary, (int)h, (int)w, factor, doffs, th, fl, bs, vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_cityscapes_gt(const uint16_t* disp, const uint8_t* seg_hwc, int32_t h, int32_t w, float factor, float* depth,
                                  uint8_t* boundary, float* seg_chw, void* stream) {
  const char* name = "cityscapes_gt";
  PRV2_REQUIRE(disp && depth && boundary, "%s: null pointer", name);
  PRV2_REQUIRE((seg_hwc == nullptr) == (seg_chw == nullptr), "%s: seg_hwc and seg_chw come together or not at all", name);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w * 3 < (int64_t)INT_MAX, "%s: %d x %d x 3 exceeds 2^31 bytes", name, h, w);
  // Python's -h // 4, w // 16 and -w // 16 (cityscapes_dataset.py:163-165)
  const CsBands bd{h - (int)cdiv(h, 4), w / 16, w - (int)cdiv(w, 16)};
  const int vec = w % 4 == 0 && aligned(disp, 8) && aligned(depth, 16) && aligned(boundary, 4) && aligned(seg_hwc, 4) && aligned(seg_chw, 16);
  const dim3 grid(flat_grid((int64_t)h * cdiv(w, 4), 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (seg_hwc)
    hipLaunchKernelGGL(cityscapes_gt_kernel<true>, grid, block, 0, s, disp, seg_hwc, depth, boundary, seg_chw, (int)h, (int)w, factor, bd, vec);
  else
    hipLaunchKernelGGL(cityscapes_gt_kernel<false>, grid, block, 0, s, disp, seg_hwc, depth, boundary, seg_chw, (int)h, (int)w, factor, bd, vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_depth16_gt(const uint16_t* src, int32_t sh, int32_t sw, int32_t grid, int32_t top, int32_t left, int32_t H, int32_t W,
                               float divisor, float th, float* depth, uint8_t* boundary, void* stream) {
  const char* name = "depth16_gt";
  PRV2_REQUIRE(src && depth && boundary, "%s: null pointer", name);
  PRV2_REQUIRE(sh >= 1 && sw >= 1, "%s: bad source shape %d x %d", name, sh, sw);
  PRV2_REQUIRE(H >= 1 && W >= 1, "%s: bad output shape %d x %d", name, H, W);
  PRV2_REQUIRE((int64_t)sh * sw < (int64_t)INT_MAX && (int64_t)H * W < (int64_t)INT_MAX, "%s: %d x %d -> %d x %d exceeds 2^31 pixels", name, sh,
               sw, H, W);
  PRV2_REQUIRE(grid == PRV2_GRID_WINDOW || grid == PRV2_GRID_NEAREST, "%s: unknown grid %d (enum prv2_depth16_grid)", name, grid);
  PRV2_REQUIRE(divisor > 0.f, "%s: divisor %g is not positive", name, (double)divisor);  // (a NaN fails too)
  if (grid == PRV2_GRID_WINDOW)
    PRV2_REQUIRE(top >= 0 && left >= 0 && (int64_t)top + H <= sh && (int64_t)left + W <= sw,
                 "%s: window of %d x %d at row %d, column %d lies outside the %d x %d source", name, H, W, top, left, sh, sw);
  else
    PRV2_REQUIRE(top == 0 && left == 0, "%s: the nearest grid takes no window offset (row %d, column %d)", name, top, left);
  const int vec = W % 4 == 0 && aligned(depth, 16) && aligned(boundary, 4);
  const dim3 grd(flat_grid((int64_t)H * cdiv(W, 4), 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  D16Grid g{top, left, (double)sh / (double)H, (double)sw / (double)W};
  if (grid == PRV2_GRID_NEAREST && (H != sh || W != sw)) {
    hipLaunchKernelGGL(depth16_gt_kernel<true>, grd, block, 0, s, src, depth, boundary, (int)sh, (int)sw, (int)H, (int)W, g, divisor, th, 0, vec);
  } else {  // (equal sizes: the nearest rule is the identity, the whole-map window)
    // the first sample of every window row is 8- / 4-byte aligned: four (two) samples per load; else one at a time
    const uintptr_t a0 = (uintptr_t)src + 2 * ((uintptr_t)top * sw + left), step = 2 * (uintptr_t)sw;
    const int svec = W % 4 ? 0 : (a0 % 8 == 0 && step % 8 == 0 ? 2 : (a0 % 4 == 0 && step % 4 == 0 ? 1 : 0));
    hipLaunchKernelGGL(depth16_gt_kernel<false>, grd, block, 0, s, src, depth, boundary, (int)sh, (int)sw, (int)H, (int)W, g, divisor, th, svec,
                       vec);
  }
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int prv2_cityscapes_masks(const uint8_t* seg_edges, const uint8_t* gt_edges, const uint8_t* hr_region, int32_t h, int32_t w,
                                     uint8_t* edge_mask, uint8_t* flatten, void* stream) {
  const char* name = "cityscapes_masks";
  PRV2_REQUIRE(seg_edges && gt_edges && hr_region && edge_mask && flatten, "%s: null pointer", name);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad shape %d x %d", name, h, w);
  PRV2_REQUIRE((int64_t)h * w < (int64_t)INT_MAX, "%s: %d x %d exceeds 2^31 pixels", name, h, w);
  const int vec = w % 4 == 0 && aligned(seg_edges, 4) && aligned(hr_region, 4) && aligned(edge_mask, 4) && aligned(flatten, 4);
  hipLaunchKernelGGL(cityscapes_masks_kernel, dim3(flat_grid((int64_t)h * cdiv(w, 4), 256)), dim3(256), 0, (hipStream_t)stream, seg_edges,
                     gt_edges, hr_region, edge_mask, flatten, (int)h, (int)w, vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}

// workspace of prv2_image_edge_region: the maximum's word (16 bytes), the gradient fp32 [h, w], the dilated threshold uint8 [h, w]
extern "C" int64_t prv2_image_edge_region_workspace_bytes(int32_t h, int32_t w) {
  if (h < 1 || w < 1 || (int64_t)3 * h * w >= (int64_t)INT_MAX) return -1;
  return 16 + roundup((int64_t)h * w * 4, 16) + roundup((int64_t)h * w, 16);
}

extern "C" int prv2_image_edge_region(const float* image_chw, int32_t h, int32_t w, float frac, uint8_t* region, int32_t H, int32_t W,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
  const char* name = "image_edge_region";
  PRV2_REQUIRE(image_chw && region, "%s: null pointer", name);
  PRV2_REQUIRE(h >= 1 && w >= 1, "%s: bad image shape %d x %d", name, h, w);
  PRV2_REQUIRE(H >= 1 && W >= 1, "%s: bad region shape %d x %d", name, H, W);
  PRV2_REQUIRE((int64_t)3 * h * w < (int64_t)INT_MAX && (int64_t)H * W < (int64_t)INT_MAX, "%s: 3 x %d x %d -> %d x %d exceeds 2^31 pixels", name,
               h, w, H, W);
  PRV2_REQUIRE(frac == frac, "%s: frac is NaN", name);
  PRV2_REQUIRE(workspace != nullptr && aligned(workspace, 16), "%s: null or misaligned workspace", name);
  const int64_t need = prv2_image_edge_region_workspace_bytes(h, w);
  PRV2_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld (prv2_image_edge_region_workspace_bytes)", name,
               (long long)workspace_bytes, (long long)need);
  const int64_t hw = (int64_t)h * w;
  uint32_t* max_bits = (uint32_t*)workspace;
  float* grad = (float*)((char*)workspace + 16);
  uint8_t* wide = (uint8_t*)grad + roundup(hw * 4, 16);
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(max_bits, 0, 16, s);
  PRV2_REQUIRE(e == hipSuccess, "%s: hipMemsetAsync failed: %s", name, hipGetErrorString(e));
  hipLaunchKernelGGL(image_grad_kernel, dim3(flat_grid(hw, 256)), dim3(256), 0, s, image_chw, (int)h, (int)w, grad, max_bits);
  hipLaunchKernelGGL(edge_dilate_kernel, dim3(flat_grid(hw, 256)), dim3(256), 0, s, (const float*)grad, (int)h, (int)w,
                     (const uint32_t*)max_bits, frac, wide);
  const int vec = W % 4 == 0 && aligned(region, 4);
  hipLaunchKernelGGL(edge_region_kernel, dim3(flat_grid((int64_t)H * cdiv(W, 4), 256)), dim3(256), 0, s, (const uint8_t*)wide, (int)h, (int)w,
                     region, (int)H, (int)W, ac_scale(h, H), ac_scale(w, W), vec);
  PRV2_LAUNCH_CHECK(name);
  return 0;
}
