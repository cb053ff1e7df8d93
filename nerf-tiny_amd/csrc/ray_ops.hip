// ray_ops.hip -- the per-ray (HBM/latency-bound) stages of the hot path for MI355X (gfx950):
//   k_rays              pixel -> camera/world direction, coarse depths, per-ray direction-branch vector
//   k_dirs_dvec         the direction-branch vector of queried points (nerf_hip_query)
//   k_coarse            sigma -> weights (inclusive transmittance), C_coarse, inverse-CDF resampling
//   k_merge             merge coarse+fine, five independent channel sorts, composite -> C_fine
//   k_coarse_x / k_merge_x   the same kernel templates over the optional per-ray outputs of ONE extras record (kernels.h RayExtras):
//                       each ray's expected depth and opacity (nerf_hip_forward_maps), with them its quantile depths (rule QD,
//                       nerf_hip_forward_quantiles) or its distortion loss (rule DL, nerf_hip_forward_distortion_train)
//   k_ray_loss          sum-of-squares loss and its gradient
// One 64-lane wave owns one ray: the transmittance cumsum / CDF are wave scans (fp64 accumulator like
// ATen's CPU cumsum, rounded to fp32 per element), searchsorted is a per-lane binary search in LDS and
// the channel sorts are bitonic networks in LDS.  Built with -ffp-contract=off: the arithmetic order is
// the reference's (SURVEY.md 8a SPEC); fused multiply-adds appear only where written as fmaf.
#include "kernels.h"
#include "prep_parts.h"
#include "ray_parts.h"

namespace nerf {

// ---------------------------------------------------------------------------------------------
// k_rays: nerf.py:52-67 (pose split), 186-197 (pixel -> unit camera dir), 211 (world dir), 288 (coarse
// depths, numpy.linspace in fp32) and the gamma_d half of dir_info (nerf.py:118) which is constant per ray.
// grid = B blocks of 128 threads.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(128) void k_rays(const RaysArgs a) {
  __shared__ float gd[DIR_DIM];
  ray_block(a, blockIdx.x, threadIdx.x, gd);
}

// k_dirs_dvec: the same start vectors for the colour point queries (nerf_hip_query), one per point from dirs[n][3] as given (not
// renormalised).  grid = n blocks of 128 threads.
__global__ __launch_bounds__(128) void k_dirs_dvec(const float* dirs, const float* w_dir, const float* b_dir, const float* b_fold, float* dvec) {
  __shared__ float gd[DIR_DIM];
  const size_t i = blockIdx.x;
  dvec_block(dirs + i * 3, w_dir, b_dir, b_fold, threadIdx.x, gd, dvec + i * HALF);
}

// ---------------------------------------------------------------------------------------------
// k_coarse: get_density (nerf.py:263-272) with delta = (far-near)/Nc, color_cum (nerf.py:274-281, :320),
// resample (nerf.py:225-261).  One wave per ray, 4 rays per 256-thread block.
// ---------------------------------------------------------------------------------------------


__global__ __launch_bounds__(256) void k_coarse(const CoarseArgs a) {
  __shared__ float s_w[4][MAXN];
  __shared__ float s_cdf[4][MAXN];
  __shared__ float s_t[4][MAXN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  coarse_ray_stage(a, blockIdx.x * 4 + wv, lane, s_w[wv], s_cdf[wv], s_t[wv], [] { __syncthreads(); });
}

// k_coarse_x: k_coarse with the optional per-ray outputs of the extras record x (kernels.h RayExtras), one instantiation per set asked for:
//   <true>               each live ray's coarse depth and opacity to x.maps [B][4] columns 0, 1 (nerf_hip_forward_maps)
//   <true, true>         ... and its coarse quantile depths (rule QD of include/nerf_hip.h) to row 0 of x.qdepth [B][2][nq] (nerf_hip_forward_quantiles)
//   <true, false, true>  ... and its coarse distortion loss (rule DL) to column 0 of x.dist [B][2] (nerf_hip_forward_distortion_train)
// The record is a kernel argument of its own, not part of CoarseArgs: CoarseArgs rides inside FwdFuse, the bf16 training kernels' argument.
template <bool MAPS, bool QD = false, bool DL = false>
__global__ __launch_bounds__(256) void k_coarse_x(const CoarseArgs a, const RayExtras x) {
  __shared__ float s_w[4][MAXN];
  __shared__ float s_cdf[4][MAXN];
  __shared__ float s_t[4][MAXN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  coarse_ray_stage<MAPS, QD, DL>(a, blockIdx.x * 4 + wv, lane, s_w[wv], s_cdf[wv], s_t[wv], [] { __syncthreads(); }, &x);
}

// ---------------------------------------------------------------------------------------------
// k_merge: nerf.py:302-321. cat -> sort(dim=1) of a [B,N,5] bundle = five INDEPENDENT ascending channel
// sorts (quirk Q1), delta_i = t_{i+1} - t_i with the last = `last`, weights, C_fine.
// One wave (64-thread block) per ray; bitonic sort over P = next_pow2(N) slots per channel in LDS.
// Ties are broken by original index (a stable sort); indices are kept for the backward pass.
// ---------------------------------------------------------------------------------------------

template <bool WITH_IDX>  // WITH_IDX: carry the original index (stable order + permutation for backward)
__global__ __launch_bounds__(64) void k_merge(const MergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* val = reinterpret_cast<float*>(smem_raw);                      // [5][P]
  uint16_t* idx = reinterpret_cast<uint16_t*>(val + 5 * (size_t)a.P);  // [5][P]
  merge_ray_stage<WITH_IDX>(a, blockIdx.x, threadIdx.x, val, idx, [] { __syncthreads(); });
}

// k_merge_x: k_merge with the optional per-ray outputs of the extras record x (passed as for k_coarse_x).  The same LDS; both sort paths
// (registers at P = 256, LDS otherwise) and the joint mode end in the same merge_ray_composite.
//   <WITH_IDX, true>           each ray's fine depth and opacity to x.maps [B][4] columns 2, 3 (nerf_hip_forward_maps, nerf_hip_forward_maps_train)
//   <WITH_IDX, true, true>     ... and its fine quantile depths (rule QD) to row 1 of x.qdepth [B][2][nq] (nerf_hip_forward_quantiles)
//   <true, true, false, true>  ... and its fine distortion loss (rule DL) to column 1 of x.dist [B][2]: the training form, which sorts with
//                              slots (nerf_hip_forward_distortion_train)
template <bool WITH_IDX, bool MAPS, bool QD = false, bool DL = false>
__global__ __launch_bounds__(64) void k_merge_x(const MergeArgs a, const RayExtras x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* val = reinterpret_cast<float*>(smem_raw);                      // [5][P]
  uint16_t* idx = reinterpret_cast<uint16_t*>(val + 5 * (size_t)a.P);  // [5][P]
  merge_ray_stage<WITH_IDX, MAPS, QD, DL>(a, blockIdx.x, threadIdx.x, val, idx, [] { __syncthreads(); }, &x);
}

// ---------------------------------------------------------------------------------------------
// k_ray_loss: nerf.py:325-331 (sum, not mean) and d loss / dC.  Single 1024-thread block (B*3 elements).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_ray_loss(const float* Cc, const float* Cf, const float* Ct, int n, float* loss, float* dCc,
                                                   float* dCf) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) {
    float d1, d2, term;
    ray_loss_element(Cc[i], Cf[i], Ct[i], d1, d2, term);
    acc += term;
    if (dCc) dCc[i] = d1;
    if (dCf) dCf[i] = d2;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += red[i];
    loss[0] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_rays(const RaysArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_rays, dim3(a.B), dim3(128), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_dirs_dvec(const float* dirs, int n, const float* w_dir, const float* b_dir, const float* b_fold, float* dvec, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dirs_dvec, dim3(n), dim3(128), 0, st, dirs, w_dir, b_dir, b_fold, dvec);
  return hipGetLastError();
}
hipError_t launch_coarse(const CoarseArgs& a, hipStream_t st, const RayExtras* x) {
  const dim3 grid((a.B + 3) / 4), block(256);  // one wave per ray; the LDS is static
  if (!x || !x->maps) hipLaunchKernelGGL(k_coarse, grid, block, 0, st, a);
  else if (x->dist) hipLaunchKernelGGL((k_coarse_x<true, false, true>), grid, block, 0, st, a, *x);
  else if (x->qdepth) hipLaunchKernelGGL((k_coarse_x<true, true>), grid, block, 0, st, a, *x);
  else hipLaunchKernelGGL((k_coarse_x<true>), grid, block, 0, st, a, *x);
  return hipGetLastError();
}
// k_merge / k_merge_x: val [5][P] floats and idx [5][P] u16
static size_t merge_lds_bytes(int P) { return (size_t)5 * P * (sizeof(float) + sizeof(uint16_t)); }
constexpr size_t MERGE_LDS_DEFAULT = 48 * 1024;
hipError_t launch_merge(const MergeArgs& a, hipStream_t st, const RayExtras* x) {
  const size_t lds = merge_lds_bytes(a.P);
  const bool with_idx = a.perm || a.joint;  // (the joint-sort mode needs the depth channel's permutation, stored or not)
  auto go = [&](auto kernel, const auto&... extras) { return launch_dyn_lds(kernel, dim3(a.B), dim3(64), lds, MERGE_LDS_DEFAULT, st, a, extras...); };
  if (!x || !x->maps) return with_idx ? go(k_merge<true>) : go(k_merge<false>);
  if (x->dist) return go(k_merge_x<true, true, false, true>, *x);  // (a training call: a.perm set)
  if (x->qdepth) return with_idx ? go(k_merge_x<true, true, true>, *x) : go(k_merge_x<false, true, true>, *x);
  return with_idx ? go(k_merge_x<true, true>, *x) : go(k_merge_x<false, true>, *x);
}
hipError_t launch_ray_loss(const float* Cc, const float* Cf, const float* Ct, int B, float* loss, float* dCc, float* dCf, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_loss, dim3(1), dim3(1024), 0, st, Cc, Cf, Ct, B * 3, loss, dCc, dCf);
  return hipGetLastError();
}

}  // namespace nerf
