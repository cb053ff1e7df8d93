// tsdf.hip -- TSDF fusion: depth images of known cameras integrated into a truncated signed distance volume
// (nerf_hip_tsdf_integrate; the definition is rule T of include/nerf_hip.h).
//   k_tsdf_integrate   per voxel: its state read once, up to TSDF_VIEWS views projected and averaged in, the state written once
//
// One thread per voxel with z fastest: the two volume reads and the two writes of a wave are 256 consecutive bytes each.  The cameras
// (nine fp64 and three fp32 each) are part of the kernel's arguments; the view index is uniform, so they reach the wave as scalar loads
// and live in scalar registers -- nothing per lane but the voxel, its state and one projection.  The projection of every (voxel, view)
// pair is evaluated from the voxel's own coordinates: an incremental form along z would change the rounding the rule fixes.  The only
// data-dependent address is the gathered pixel; x and y are compared against the image in fp64 BEFORE they become integers, so the
// index (c * H + x) * W + y lies inside the caller's n * H * W < 2^31 images.  No atomics, no LDS, no barrier.
#include "scan.h"

namespace nerf {

// grid = ceil(npts / TSDF_WG)
__global__ __launch_bounds__(TSDF_WG) void k_tsdf_integrate(const TsdfArgs a) {
  const long long idx = (long long)blockIdx.x * TSDF_WG + threadIdx.x;
  if (idx >= a.npts) return;
  const int k = (int)(idx % a.nz);
  const int ij = (int)(idx / a.nz);
  const int j = ij % a.ny, i = ij / a.ny;
  // the lattice point: one fp32 product and one fp32 sum per coordinate (the density grid's rule), then widened
  const double px = (double)(a.lo[0] + (float)i * a.step[0]);
  const double py = (double)(a.lo[1] + (float)j * a.step[1]);
  const double pz = (double)(a.lo[2] + (float)k * a.step[2]);
  float T = a.tsdf[idx], Wt = a.weight[idx];
  const double hmax = (double)(a.H - 1), wmax = (double)(a.W - 1);
  const long long hw = (long long)a.H * a.W;
#pragma unroll 1
  for (int c = 0; c < a.nviews; ++c) {
    const TsdfCam& cam = a.cam[c];
    const double wx = px - (double)cam.o[0], wy = py - (double)cam.o[1], wz = pz - (double)cam.o[2];
    const double m0 = (cam.Q[0] * wx + cam.Q[1] * wy) + cam.Q[2] * wz;
    const double m1 = (cam.Q[3] * wx + cam.Q[4] * wy) + cam.Q[5] * wz;
    const double m2 = (cam.Q[6] * wx + cam.Q[7] * wy) + cam.Q[8] * wz;
    const double x = floor(m0 / m2 + 0.5), y = floor(m1 / m2 + 0.5);
    if (!(m2 > 0.0 && 0.0 <= x && x <= hmax && 0.0 <= y && y <= wmax)) continue;  // (false on NaN: not in view)
    const long long pix = (long long)c * hw + (long long)(int)x * a.W + (int)y;
    const bool fg = a.opacity == nullptr || a.opacity[pix] >= a.min_opacity;
    double val = 1.0;
    if (fg) {
      const float df = a.depth[pix];
      const double d = (double)df;
      const double r = sqrt((wx * wx + wy * wy) + wz * wz);
      const double sdf = d - r;
      if (!(__builtin_isfinite(df) && d > 0.0 && sdf >= -a.trunc)) continue;
      val = fmin(1.0, sdf / a.trunc);
    } else if (!a.carve) {
      continue;
    }
    const double w0 = (double)Wt, w1 = w0 + 1.0;
    T = (float)((((double)T * w0) + val) / w1);
    Wt = (float)w1;
  }
  a.tsdf[idx] = T;
  a.weight[idx] = Wt;
}

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st) {
  if (a.npts > 0 && a.nviews > 0) LAUNCH(k_tsdf_integrate, dim3(grid(a.npts, TSDF_WG)), dim3(TSDF_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
