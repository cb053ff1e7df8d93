// ray_ops.hip -- the per-ray (HBM/latency-bound) stages of the hot path for MI355X (gfx950):
//   k_rays              pixel -> camera/world direction, coarse depths, per-ray direction-branch vector
//   k_dirs_dvec         the direction-branch vector of queried points (nerf_hip_query)
//   k_coarse            sigma -> weights (inclusive transmittance), C_coarse, inverse-CDF resampling
//   k_merge             merge coarse+fine, five independent channel sorts, composite -> C_fine
//   k_coarse_maps / k_merge_maps   the same, plus each ray's expected depth and opacity (nerf_hip_forward_maps)
//   k_coarse_qmaps / k_merge_qmaps the maps kernels, plus each ray's quantile depths (nerf_hip_forward_quantiles, rule QD)
//   k_coarse_dmaps / k_merge_dmaps the training maps kernels, plus each ray's distortion loss (nerf_hip_forward_distortion_train, rule DL)
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

// k_coarse_maps: k_coarse that also stores each live ray's coarse depth and opacity to maps [B][4] columns 0, 1 (nerf_hip_forward_maps).  The
// pointer is a kernel argument of its own, not a CoarseArgs field: CoarseArgs rides inside FwdFuse, the bf16 training kernels' argument.
__global__ __launch_bounds__(256) void k_coarse_maps(const CoarseArgs a, float* maps) {
  __shared__ float s_w[4][MAXN];
  __shared__ float s_cdf[4][MAXN];
  __shared__ float s_t[4][MAXN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  coarse_ray_stage<true>(a, blockIdx.x * 4 + wv, lane, s_w[wv], s_cdf[wv], s_t[wv], [] { __syncthreads(); }, maps);
}

// k_coarse_qmaps: k_coarse_maps that also stores each live ray's coarse quantile depths (rule QD of include/nerf_hip.h) to row 0 of
// qdepth [B][2][nq] (nerf_hip_forward_quantiles).  The quantiles and the pointer are kernel arguments of their own, for k_coarse_maps's reason.
__global__ __launch_bounds__(256) void k_coarse_qmaps(const CoarseArgs a, float* maps, const QuantArgs qa, float* qdepth) {
  __shared__ float s_w[4][MAXN];
  __shared__ float s_cdf[4][MAXN];
  __shared__ float s_t[4][MAXN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  coarse_ray_stage<true, true>(a, blockIdx.x * 4 + wv, lane, s_w[wv], s_cdf[wv], s_t[wv], [] { __syncthreads(); }, maps, &qa, qdepth);
}

// k_coarse_dmaps: k_coarse_maps that also stores each live ray's coarse distortion loss (rule DL of include/nerf_hip.h) to column 0 of
// dist [B][2] (nerf_hip_forward_distortion_train).  The pointer is a kernel argument of its own, for k_coarse_maps's reason.
__global__ __launch_bounds__(256) void k_coarse_dmaps(const CoarseArgs a, float* maps, float* dist) {
  __shared__ float s_w[4][MAXN];
  __shared__ float s_cdf[4][MAXN];
  __shared__ float s_t[4][MAXN];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  coarse_ray_stage<true, false, true>(a, blockIdx.x * 4 + wv, lane, s_w[wv], s_cdf[wv], s_t[wv], [] { __syncthreads(); }, maps, nullptr, nullptr, dist);
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

// k_merge_maps: k_merge that also stores each ray's fine depth and opacity to maps [B][4] columns 2, 3 (nerf_hip_forward_maps; pointer passed
// as for k_coarse_maps).  Both sort paths (registers at P = 256, LDS otherwise) end in the same merge_ray_composite.
template <bool WITH_IDX>
__global__ __launch_bounds__(64) void k_merge_maps(const MergeArgs a, float* maps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* val = reinterpret_cast<float*>(smem_raw);                      // [5][P]
  uint16_t* idx = reinterpret_cast<uint16_t*>(val + 5 * (size_t)a.P);  // [5][P]
  merge_ray_stage<WITH_IDX, true>(a, blockIdx.x, threadIdx.x, val, idx, [] { __syncthreads(); }, maps);
}

// k_merge_qmaps: k_merge_maps that also stores each ray's fine quantile depths (rule QD) to row 1 of qdepth [B][2][nq]
// (nerf_hip_forward_quantiles).  Both sort paths and the joint mode end in the same merge_ray_composite, as for k_merge_maps.
template <bool WITH_IDX>
__global__ __launch_bounds__(64) void k_merge_qmaps(const MergeArgs a, float* maps, const QuantArgs qa, float* qdepth) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* val = reinterpret_cast<float*>(smem_raw);                      // [5][P]
  uint16_t* idx = reinterpret_cast<uint16_t*>(val + 5 * (size_t)a.P);  // [5][P]
  merge_ray_stage<WITH_IDX, true, true>(a, blockIdx.x, threadIdx.x, val, idx, [] { __syncthreads(); }, maps, &qa, qdepth);
}

// k_merge_dmaps: the training k_merge_maps (sorts with slots) that also stores each ray's fine distortion loss (rule DL) to column 1 of
// da.dist [B][2] (nerf_hip_forward_distortion_train).  Same LDS; both sort paths and the joint mode end in the same merge_ray_composite.
__global__ __launch_bounds__(64) void k_merge_dmaps(const MergeArgs a, float* maps, const DistArgs da) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* val = reinterpret_cast<float*>(smem_raw);                      // [5][P]
  uint16_t* idx = reinterpret_cast<uint16_t*>(val + 5 * (size_t)a.P);  // [5][P]
  merge_ray_stage<true, true, false, true>(a, blockIdx.x, threadIdx.x, val, idx, [] { __syncthreads(); }, maps, nullptr, nullptr, &da);
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
hipError_t launch_coarse(const CoarseArgs& a, hipStream_t st, float* maps) {
  if (maps) hipLaunchKernelGGL(k_coarse_maps, dim3((a.B + 3) / 4), dim3(256), 0, st, a, maps);
  else hipLaunchKernelGGL(k_coarse, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}
size_t merge_lds_bytes(int P) { return (size_t)5 * P * (sizeof(float) + sizeof(uint16_t)); }
template <bool WITH_IDX>
hipError_t launch_merge_maps(const MergeArgs& a, float* maps, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_maps<WITH_IDX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(k_merge_maps<WITH_IDX>, dim3(a.B), dim3(64), lds, st, a, maps);
  return hipGetLastError();
}
hipError_t launch_merge(const MergeArgs& a, hipStream_t st, float* maps) {
  const size_t lds = merge_lds_bytes(a.P);
  if (maps) return (a.perm || a.joint) ? launch_merge_maps<true>(a, maps, lds, st) : launch_merge_maps<false>(a, maps, lds, st);
  if (a.perm || a.joint) {  // (the joint-sort mode needs the depth channel's permutation, stored or not)
    if (lds > 48 * 1024)
      if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    hipLaunchKernelGGL(k_merge<true>, dim3(a.B), dim3(64), lds, st, a);
  } else {
    if (lds > 48 * 1024)
      if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
    hipLaunchKernelGGL(k_merge<false>, dim3(a.B), dim3(64), lds, st, a);
  }
  return hipGetLastError();
}
hipError_t launch_coarse_quantiles(const CoarseArgs& a, float* maps, const QuantArgs& qa, float* qdepth, hipStream_t st) {
  hipLaunchKernelGGL(k_coarse_qmaps, dim3((a.B + 3) / 4), dim3(256), 0, st, a, maps, qa, qdepth);
  return hipGetLastError();
}
template <bool WITH_IDX>
hipError_t launch_merge_qmaps(const MergeArgs& a, float* maps, const QuantArgs& qa, float* qdepth, size_t lds, hipStream_t st) {
  if (lds > 48 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_qmaps<WITH_IDX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(k_merge_qmaps<WITH_IDX>, dim3(a.B), dim3(64), lds, st, a, maps, qa, qdepth);
  return hipGetLastError();
}
hipError_t launch_merge_quantiles(const MergeArgs& a, float* maps, const QuantArgs& qa, float* qdepth, hipStream_t st) {
  const size_t lds = merge_lds_bytes(a.P);
  return (a.perm || a.joint) ? launch_merge_qmaps<true>(a, maps, qa, qdepth, lds, st) : launch_merge_qmaps<false>(a, maps, qa, qdepth, lds, st);
}
hipError_t launch_coarse_dist(const CoarseArgs& a, float* maps, float* dist, hipStream_t st) {
  hipLaunchKernelGGL(k_coarse_dmaps, dim3((a.B + 3) / 4), dim3(256), 0, st, a, maps, dist);
  return hipGetLastError();
}
hipError_t launch_merge_dist(const MergeArgs& a, float* maps, const DistArgs& da, hipStream_t st) {
  const size_t lds = merge_lds_bytes(a.P);
  if (lds > 48 * 1024)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_merge_dmaps), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(k_merge_dmaps, dim3(a.B), dim3(64), lds, st, a, maps, da);
  return hipGetLastError();
}
hipError_t launch_ray_loss(const float* Cc, const float* Cf, const float* Ct, int B, float* loss, float* dCc, float* dCf, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_loss, dim3(1), dim3(1024), 0, st, Cc, Cf, Ct, B * 3, loss, dCc, dCf);
  return hipGetLastError();
}

}  // namespace nerf
