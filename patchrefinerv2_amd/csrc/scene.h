// The rules every export computed from a depth map shares (csrc/pointcloud.hip, stereo.hip, bokeh.hip, view.hip), once each: which depth
// is valid, when two neighbouring depths are joined, how a pixel is back-projected, how the colour image is sampled, how a float
// becomes a byte, which faces a cell of the mesh has -- and the host checks of the camera, the depth range and the image that the
// entry points of these files make.  The numpy restatement of every rule is in output.py (_valid_depth, sample_indices, color_bytes,
// mesh_faces_host); the files that include this are built with -ffp-contract=off and every rounded fp32 operation is one IEEE operation.
#pragma once
#include "rows.h"

namespace prv2 {
namespace {

struct Camera {
  float fx, fy, cx, cy;  // in pixels of the depth map's grid
  float lo, hi;          // valid: lo < Z < hi
};

// valid: Z finite and lo < Z < hi
__device__ __forceinline__ bool valid_z(const Camera& c, float z) { return fabsf(z) < __builtin_inff() && z > c.lo && z < c.hi; }

// two valid depths are joined unless |Zp - Zq| > thr * min(Zp, Zq) (thr <= 0: always joined)
__device__ __forceinline__ bool joined(float thr, float zp, float zq) {
  return !(thr > 0.0f) || !(fabsf(__fsub_rn(zp, zq)) > __fmul_rn(thr, fminf(zp, zq)));
}

// back-projection: X = (((float)x + 0.5) - cx) * Z / fx, Y likewise with cy, fy
__device__ __forceinline__ float cam_x(const Camera& c, int x, float z) {
  return __fdiv_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)x, 0.5f), c.cx), z), c.fx);
}
__device__ __forceinline__ float cam_y(const Camera& c, int y, float z) {
  return __fdiv_rn(__fmul_rn(__fsub_rn(__fadd_rn((float)y, 0.5f), c.cy), z), c.fy);
}

// the nearest sample of an axis of n_in values for position i of n_out: floor((2 i + 1) n_in / (2 n_out)), which is i for equal sizes
__device__ __forceinline__ int nearest(int i, int n_out, int n_in) {
  return n_in == n_out ? i : (int)(((int64_t)(2 * i + 1) * n_in) / (2 * (int64_t)n_out));
}

// clamp(rint(v), 0, 255), ties to even, NaN -> 0
__device__ __forceinline__ uint32_t color_byte(float v) {
  const float r = rintf(v);
  return !(r > 0.0f) ? 0u : r >= 255.0f ? 255u : (uint32_t)r;
}

// the colour image of the frames, of any size: fp32 [n, 3, ih, iw] in [0, 1]
struct ImageSrc {
  const float* image;
  int32_t ih, iw;
  __device__ __forceinline__ int64_t plane() const { return (int64_t)ih * iw; }
  __device__ __forceinline__ const float* frame(int f) const { return image + (int64_t)f * 3 * ih * iw; }
};

// The faces of a cell of the mesh with the corners a = (y, x), b = (y, x + 1), c = (y + 1, x), d = (y + 1, x + 1): their depths (a
// corner's counts only where it is kept), whether each is kept, and the joined threshold.  Four corners kept: the diagonal a-d if
// |Za - Zd| <= |Zb - Zc|, else b-c; three: the diagonal whose ends are kept; fewer: no face.  a-d: (a, c, d) then (a, d, b); b-c:
// (a, c, b) then (b, c, d); a candidate needs its three corners kept and its three edges joined.
struct CellFaces {
  bool ad;             // the diagonal is a-d (else b-c)
  bool first, second;  // the candidates that exist
};
__device__ __forceinline__ CellFaces cell_rule(float thr, float za, float zb, float zc, float zd, bool ka, bool kb, bool kc, bool kd) {
  const bool ad = ka && kb && kc && kd ? fabsf(__fsub_rn(za, zd)) <= fabsf(__fsub_rn(zb, zc)) : (ka && kd);
  const bool ac = ka && kc && joined(thr, za, zc), cd = kc && kd && joined(thr, zc, zd);
  const bool ab = ka && kb && joined(thr, za, zb), bd = kb && kd && joined(thr, zb, zd);
  const bool dg = ad ? joined(thr, za, zd) : joined(thr, zb, zc);  // (both ends of the chosen diagonal are kept)
  return CellFaces{ad, dg && ac && (ad ? cd : ab), dg && bd && (ad ? ab : cd)};
}

// ---- the host checks of the C entry points ------------------------------------------------------------------------------------------
// (an export that uses fx alone passes it for fy as well, and 0 for the principal point)
static int check_camera(const char* name, float fx, float fy, float cx, float cy) {
  PRV2_REQUIRE(fx > 0.0f && fy > 0.0f && fx < __builtin_inff() && fy < __builtin_inff(), "%s: intrinsics: focal lengths %g, %g: finite and positive",
               name, (double)fx, (double)fy);
  PRV2_REQUIRE(fabsf(cx) < __builtin_inff() && fabsf(cy) < __builtin_inff(), "%s: intrinsics: principal point %g, %g: finite", name, (double)cx,
               (double)cy);
  return 0;
}

// (an export without a threshold passes 0)
static int check_range(const char* name, float lo, float hi, float edge_thr) {
  PRV2_REQUIRE(lo == lo && hi == hi && edge_thr == edge_thr, "%s: NaN in the depth range or edge_thr", name);
  return 0;
}

static int check_image(const char* name, const float* image, int n, int ih, int iw) {
  PRV2_REQUIRE(image != nullptr, "%s: null pointer (image)", name);
  PRV2_REQUIRE(ih >= 1 && iw >= 1 && (int64_t)n * 3 * ih * iw < (int64_t)INT_MAX, "%s: bad image shape %d x %d", name, ih, iw);
  return 0;
}

// the widest row a workgroup keeps in LDS (stereo.hip, view.hip)
static int check_row_width(const char* name, int w) {
  PRV2_REQUIRE(w <= prv2_stereo_max_width(), "%s: a row of %d columns is wider than the %d a workgroup keeps in LDS (prv2_stereo_max_width)", name, w,
               prv2_stereo_max_width());
  return 0;
}

}  // namespace
}  // namespace prv2
