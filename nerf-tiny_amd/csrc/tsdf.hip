// tsdf.hip -- TSDF fusion: depth images of known cameras integrated into a truncated signed distance volume
// (nerf_hip_tsdf_integrate; the definition is rule T of include/nerf_hip.h), the views' colours fused beside it
// and the colour volume sampled at arbitrary points (nerf_hip_tsdf_integrate_color / nerf_hip_tsdf_sample_color; section 3h-10; rules
// TC and S).
//   k_tsdf_integrate<COLOR>   per voxel: its state read once, up to TSDF_VIEWS views projected and averaged in, the state written once;
//                             with COLOR also the colour state (R, G, B, Wc), touched only by voxels inside some view's band
//   k_tsdf_sample_color       per point: the trilinear mean of the coloured corners of its cell
//
// One thread per voxel with z fastest: the two volume reads and the two writes of a wave are 256 consecutive bytes each.  The cameras
// (nine fp64 and three fp32 each) are part of the kernel's arguments; the view index is uniform, so they reach the wave as scalar loads
// and live in scalar registers -- nothing per lane but the voxel, its state and one projection.  The projection of every (voxel, view)
// pair is evaluated from the voxel's own coordinates: an incremental form along z would change the rounding the rule fixes.  The only
// data-dependent address is the gathered pixel; x and y are compared against the image in fp64 BEFORE they become integers, so the
// index (c * H + x) * W + y lies inside the caller's n * H * W < 2^31 images (and three times it, the colour's, inside 2^33: 64-bit).
// The colour state is one 16-byte vector per voxel (a wave's access is 1 KB contiguous), loaded at a voxel's first colour observation
// of the launch and stored only if it was loaded: most voxels lie outside every view's band and move nothing.
// No atomics, no LDS, no barrier.
#include "scan.h"

namespace nerf {

// grid = ceil(npts / TSDF_WG)
template <bool COLOR>
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
  float4 col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (COLOR) the colour state, once loaded
  bool have_col = false;
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
      if constexpr (COLOR) {
        if (sdf <= a.trunc) {  // within one truncation distance of this view's surface, on either side
          const float* __restrict__ px3 = a.rgb + pix * 3;
          const float cr = px3[0], cg = px3[1], cb = px3[2];
          if (__builtin_isfinite(cr) && __builtin_isfinite(cg) && __builtin_isfinite(cb)) {
            if (!have_col) {
              col = a.color[idx];
              have_col = true;
            }
            const double wc0 = (double)col.w, wc1 = wc0 + 1.0;
            col.x = (float)((((double)col.x * wc0) + (double)cr) / wc1);
            col.y = (float)((((double)col.y * wc0) + (double)cg) / wc1);
            col.z = (float)((((double)col.z * wc0) + (double)cb) / wc1);
            col.w = (float)wc1;
          }
        }
      }
    } else if (!a.carve) {
      continue;
    }
    const double w0 = (double)Wt, w1 = w0 + 1.0;
    T = (float)((((double)T * w0) + val) / w1);
    Wt = (float)w1;
  }
  a.tsdf[idx] = T;
  a.weight[idx] = Wt;
  if constexpr (COLOR) {
    if (have_col) a.color[idx] = col;
  }
}

// grid = ceil(M / TSDF_WG).  Rule S: per axis the cell and the fraction in fp64, clamped before they become integers; the eight corners
// in the order (di, dj, dk), dk fastest.
__global__ __launch_bounds__(TSDF_WG) void k_tsdf_sample_color(const TsdfSampleArgs a) {
  const long long m = (long long)blockIdx.x * TSDF_WG + threadIdx.x;
  if (m >= a.M) return;
  const float xf[3] = {a.points[m * 3 + 0], a.points[m * 3 + 1], a.points[m * 3 + 2]};
  const int dim[3] = {a.nx, a.ny, a.nz};
  double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
  if (__builtin_isfinite(xf[0]) && __builtin_isfinite(xf[1]) && __builtin_isfinite(xf[2])) {
    int i0[3], cnt[3];
    double f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (dim[d] == 1) {
        i0[d] = 0;
        f[d] = 0.0;
        cnt[d] = 1;  // the upper corner is not read
      } else {
        const double g = ((double)xf[d] - (double)a.lo[d]) / (double)a.step[d];
        const double ci = fmin(fmax(floor(g), 0.0), (double)(dim[d] - 2));  // (fmax / fmin drop a NaN: the cell is then 0)
        i0[d] = (int)ci;
        f[d] = fmin(fmax(g - ci, 0.0), 1.0);
        cnt[d] = 2;
      }
    }
    for (int di = 0; di < cnt[0]; ++di)
      for (int dj = 0; dj < cnt[1]; ++dj)
        for (int dk = 0; dk < cnt[2]; ++dk) {
          const long long p = ((long long)(i0[0] + di) * a.ny + (i0[1] + dj)) * a.nz + (i0[2] + dk);
          const float4 c = a.color[p];
          if (!(c.w > 0.0f)) continue;
          const double wx = di ? f[0] : 1.0 - f[0], wy = dj ? f[1] : 1.0 - f[1], wz = dk ? f[2] : 1.0 - f[2];
          const double w = (wx * wy) * wz;
          num[0] = num[0] + w * (double)c.x;
          num[1] = num[1] + w * (double)c.y;
          num[2] = num[2] + w * (double)c.z;
          den = den + w;
        }
  }
  const bool ok = den > 0.0;
  a.rgb[m * 3 + 0] = ok ? (float)(num[0] / den) : 0.0f;
  a.rgb[m * 3 + 1] = ok ? (float)(num[1] / den) : 0.0f;
  a.rgb[m * 3 + 2] = ok ? (float)(num[2] / den) : 0.0f;
  a.valid[m] = ok ? 1 : 0;
}

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st) {
  if (a.npts <= 0 || a.nviews <= 0) return hipSuccess;
  if (a.color) {
    LAUNCH(k_tsdf_integrate<true>, dim3(grid(a.npts, TSDF_WG)), dim3(TSDF_WG), 0, st, a);
  } else {
    LAUNCH(k_tsdf_integrate<false>, dim3(grid(a.npts, TSDF_WG)), dim3(TSDF_WG), 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_tsdf_sample_color(const TsdfSampleArgs& a, hipStream_t st) {
  if (a.M > 0) LAUNCH(k_tsdf_sample_color, dim3((unsigned)((a.M + TSDF_WG - 1) / TSDF_WG)), dim3(TSDF_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
