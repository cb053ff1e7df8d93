// ray_ops_bwd.hip -- backward of the per-ray stages for MI355X (gfx950); one 64-lane wave per ray.
//   k_merge_bwd    d C_fine -> sorted-channel gradients (composite backward with reverse wave scans) ->
//                  un-sort through each channel's OWN permutation (quirk Q1) -> d rgb, d sigma of the coarse
//                  and fine samples and d t_fine (through the sorted deltas).
//   k_coarse_bwd   d t_fine -> inverse-CDF resampling backward (nerf.py:225-261; u, the ray-0 spacing and
//                  t_coarse carry no gradient) -> d w_coarse; plus d C_coarse; -> composite backward with the
//                  constant coarse delta -> d sigma_coarse, d rgb_coarse.
//   k_merge_bwd_x / k_coarse_bwd_x   the same kernel templates over the upstreams in ONE extras record (kernels.h RayExtras): of each
//                  ray's depth and opacity maps (nerf_hip_backward_maps) and, with them, of its distortion loss
//                  (nerf_hip_backward_distortion; rule DL)
// Formulas: SURVEY.md 8a BWD (verified there against autograd in fp64).  These replace the autograd graph the
// reference builds for nerf.py:286-323 when loss.backward() runs (nerf.py:473).
#include "kernels.h"
#include "ray_parts_bwd.h"

namespace nerf {

// ---------------------------------------------------------------------------------------------
// k_merge_bwd: grid = B blocks of 64 threads; dynamic LDS = 4 * N floats
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_merge_bwd(const MergeBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm_f[];
  merge_bwd_ray(a, blockIdx.x, threadIdx.x, sm_f, [] { __syncthreads(); });
}

// k_merge_bwd_x: k_merge_bwd plus the upstreams of the extras record x.  <false>: the fine maps' (x.dmaps [B][4] columns 2, 3;
// nerf_hip_backward_maps), dynamic LDS = 5 * N floats; <true>: also the fine distortion loss's (x.ddist [B][2] column 1, rule DL of
// include/nerf_hip.h; nerf_hip_backward_distortion), dynamic LDS = 6 * N floats.  The record is a kernel argument of its own,
// not part of MergeBwdArgs: that struct rides inside BwdFuse, the bf16 chain kernels' argument.
template <bool DL>
__global__ __launch_bounds__(64) void k_merge_bwd_x(const MergeBwdArgs a, const RayExtras x) {
  extern __shared__ __attribute__((aligned(16))) float sm_f[];
  merge_bwd_ray<true, DL>(a, blockIdx.x, threadIdx.x, sm_f, [] { __syncthreads(); }, &x);
}

// ---------------------------------------------------------------------------------------------
// k_coarse_bwd: one wave per ray, 4 rays per 256-thread block
// ---------------------------------------------------------------------------------------------
// dynamic LDS: 4 waves x (5 * Nc floats) then 4 waves x (Nf uint16, padded to even)
__global__ __launch_bounds__(256) void k_coarse_bwd(const CoarseBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm_c[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ray_raw = blockIdx.x * 4 + wv;
  const bool live = ray_raw < a.B;
  const int ray = live ? ray_raw : a.B - 1;
  float* w = sm_c + (size_t)wv * 5 * a.Nc;
  uint16_t* ks = reinterpret_cast<uint16_t*>(sm_c + (size_t)4 * 5 * a.Nc) + (size_t)wv * ((a.Nf + 1) & ~1);
  coarse_bwd_ray(a, ray, live, lane, w, ks, [] { __syncthreads(); });
}

// k_coarse_bwd_x: k_coarse_bwd plus the upstreams of the extras record x (passed as for k_merge_bwd_x), the same LDS.  <false>: the
// coarse maps' (x.dmaps [B][4] columns 0, 1); <true>: also the coarse distortion loss's (x.ddist [B][2] column 0)
template <bool DL>
__global__ __launch_bounds__(256) void k_coarse_bwd_x(const CoarseBwdArgs a, const RayExtras x) {
  extern __shared__ __attribute__((aligned(16))) float sm_c[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ray_raw = blockIdx.x * 4 + wv;
  const bool live = ray_raw < a.B;
  const int ray = live ? ray_raw : a.B - 1;
  float* w = sm_c + (size_t)wv * 5 * a.Nc;
  uint16_t* ks = reinterpret_cast<uint16_t*>(sm_c + (size_t)4 * 5 * a.Nc) + (size_t)wv * ((a.Nf + 1) & ~1);
  coarse_bwd_ray<true, DL>(a, ray, live, lane, w, ks, [] { __syncthreads(); }, &x);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// merge_bwd_ray's arrays of N = Nc + Nf floats: 4 (plain), 5 with the maps' upstream (+ w_k), 6 with the distortion loss's too (+ g dL/dt_k).
// N <= 2048: at most 48 KiB, inside the 64 KiB a launch may ask for as it is -- no attribute to raise
constexpr int MERGE_BWD_ARRAYS = 4, MERGE_BWD_ARRAYS_MAPS = 5, MERGE_BWD_ARRAYS_DIST = 6;
static size_t merge_bwd_lds_bytes(int N, int arrays) { return (size_t)arrays * N * sizeof(float); }
hipError_t launch_merge_bwd(const MergeBwdArgs& a, hipStream_t st, const RayExtras* x) {
  const int N = a.Nc + a.Nf;
  if (x && x->ddist) hipLaunchKernelGGL(k_merge_bwd_x<true>, dim3(a.B), dim3(64), merge_bwd_lds_bytes(N, MERGE_BWD_ARRAYS_DIST), st, a, *x);
  else if (x && x->dmaps) hipLaunchKernelGGL(k_merge_bwd_x<false>, dim3(a.B), dim3(64), merge_bwd_lds_bytes(N, MERGE_BWD_ARRAYS_MAPS), st, a, *x);
  else hipLaunchKernelGGL(k_merge_bwd, dim3(a.B), dim3(64), merge_bwd_lds_bytes(N, MERGE_BWD_ARRAYS), st, a);
  return hipGetLastError();
}
// k_coarse_bwd / k_coarse_bwd_x: 4 waves x (5 * Nc floats), then 4 waves x (Nf uint16, padded to even) -- every form the same
static size_t coarse_bwd_lds_bytes(int Nc, int Nf) { return (size_t)4 * 5 * Nc * sizeof(float) + (size_t)4 * ((Nf + 1) & ~1) * sizeof(uint16_t); }
constexpr size_t COARSE_BWD_LDS_DEFAULT = 64 * 1024;
hipError_t launch_coarse_bwd(const CoarseBwdArgs& a, hipStream_t st, const RayExtras* x) {
  const size_t lds = coarse_bwd_lds_bytes(a.Nc, a.Nf);
  auto go = [&](auto kernel, const auto&... extras) { return launch_dyn_lds(kernel, dim3((a.B + 3) / 4), dim3(256), lds, COARSE_BWD_LDS_DEFAULT, st, a, extras...); };
  if (x && x->ddist) return go(k_coarse_bwd_x<true>, *x);
  if (x && x->dmaps) return go(k_coarse_bwd_x<false>, *x);
  return go(k_coarse_bwd);
}

}  // namespace nerf
