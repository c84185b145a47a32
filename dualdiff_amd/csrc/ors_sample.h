// ORS ray sampling, the one statement of "sample s of a ray -> voxel -> class" (networks/occ3d_proj.py:90-108), shared by
// dd_ors_project_kernel (elementwise.hip: every sample's label) and dd_ors_first_hit_kernel (ors_render.hip: the first
// occupied one).  fp32 with the reference's operation order and NO fma contraction: the result is a voxel index, a
// last-bit difference could flip a class.
#pragma once
#include "dd_common.h"

constexpr int DD_ORS_NX = 200, DD_ORS_NY = 200, DD_ORS_NZ = 16;   // the Occ3D volume, x-major
constexpr int DD_ORS_FREE = 17;                                   // "not occupied", and every sample outside the volume

// voxel index of sample s of the ray o + t d, t = s * step; any component may be out of range
__device__ __forceinline__ void dd_ors_voxel(const float* __restrict__ o, const float* __restrict__ d, int s, float step,
                                             int& ix, int& iy, int& iz) {
  const float t = __fmul_rn((float)s, step);
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = __fdiv_rn(__fadd_rn(o[a], __fmul_rn(t, d[a])), 40.0f);
  const float gz = __fsub_rn(__fdiv_rn(__fmul_rn(g[2], 40.0f), 3.2f), 0.6875f);
  auto idx = [](float c, float size) -> int {       // grid_sample nearest, align_corners = False
    return (int)rintf(__fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(c, 1.0f), size), 1.0f), 2.0f));
  };
  ix = idx(g[0], (float)DD_ORS_NX);
  iy = idx(g[1], (float)DD_ORS_NY);
  iz = idx(gz, (float)DD_ORS_NZ);
}

// the class at a voxel index: 17 outside the volume (grid_sample's zero padding, occ3d_proj.py:105-106)
__device__ __forceinline__ int dd_ors_class_at(const uint8_t* __restrict__ occ, int ix, int iy, int iz) {
  int lab = DD_ORS_FREE;
  if (ix >= 0 && ix < DD_ORS_NX && iy >= 0 && iy < DD_ORS_NY && iz >= 0 && iz < DD_ORS_NZ)
    lab = occ[(ix * DD_ORS_NY + iy) * DD_ORS_NZ + iz];
  return lab;
}

__device__ __forceinline__ int dd_ors_label(const uint8_t* __restrict__ occ, const float* __restrict__ o,
                                            const float* __restrict__ d, int s, float step) {
  int ix, iy, iz;
  dd_ors_voxel(o, d, s, step, ix, iy, iz);
  return dd_ors_class_at(occ, ix, iy, iz);
}
