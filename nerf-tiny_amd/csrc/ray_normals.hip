// ray_normals.hip -- per-ray normal maps (nerf_hip_forward_normals, rule NM of include/nerf_hip.h):
//   k_sample_points      the world points of one chunk of a pass's samples, from the ray records and the pass's depths
//   k_normal_composite   N = sum_i w_i n_i per ray, n_i the field normal of the sigma gradient at sample i
// Between the two run the gradient query's own launches (launch_query_grad_fwd / launch_query_grad_bwd) over the chunk's points.
// MI355X / gfx950 only; built with -ffp-contract=off like every other unit: the points are the forward's, bit for bit.
#include "field_common.h"
#include "ray_dist.h"

namespace nerf {

// One thread per sample of `nrays` whole rays of N samples: points[m] = sample_point(ray m / N, t[m * t_stride]).  rayf and t start at the
// chunk's first ray; t_stride = 1 (t_c) or 5 (channel 0 of the sorted bundle).
__global__ __launch_bounds__(256) void k_sample_points(const float* __restrict__ rayf, const float* __restrict__ t, int t_stride, int nrays, int N,
                                                       float* __restrict__ points) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= nrays * N) return;
  const int ray = m / N;
  float p[3];
  sample_point(rayf + (size_t)ray * RAYF, t[(size_t)m * t_stride], p);
  points[(size_t)m * 3] = p[0];
  points[(size_t)m * 3 + 1] = p[1];
  points[(size_t)m * 3 + 2] = p[2];
}

// One wave per ray (four rays per workgroup, as k_coarse), samples strided over the lanes: the field normal in fp32, every operation rounded
// (mesh.hip's rule: -g / sqrt(g0^2 + g1^2 + g2^2), zero where the length is 0 or not finite), three fp64 partial sums per lane, a wave
// reduction, lane 0 stores out[ray * out_stride + 0..2].  A weight that is 0 or NaN adds nothing.  Rays behind the batch store nothing.
// No LDS, no atomics, no barrier.
__global__ __launch_bounds__(256) void k_normal_composite(const float* __restrict__ w, const float* __restrict__ g, int B, int N,
                                                          float* __restrict__ out, int out_stride) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= B) return;  // (wave-uniform)
  const float* wr = w + (size_t)ray * N;
  const float* gr = g + (size_t)ray * N * 3;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = lane; i < N; i += 64) {
    const float wi = wr[i];
    const float g0 = gr[3 * i], g1 = gr[3 * i + 1], g2 = gr[3 * i + 2];
    const float len = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
    const bool ok = isfinite(len) && len > 0.0f;
    const float n0 = ok ? -g0 / len : 0.0f, n1 = ok ? -g1 / len : 0.0f, n2 = ok ? -g2 / len : 0.0f;
    if (wi > 0.0f || wi < 0.0f) {  // (false on NaN)
      a0 += (double)wi * (double)n0;
      a1 += (double)wi * (double)n1;
      a2 += (double)wi * (double)n2;
    }
  }
  a0 = wave_sum_f64(a0);
  a1 = wave_sum_f64(a1);
  a2 = wave_sum_f64(a2);
  if (lane == 0) {
    float* o = out + (size_t)ray * out_stride;
    o[0] = (float)a0;
    o[1] = (float)a1;
    o[2] = (float)a2;
  }
}

hipError_t launch_sample_points(const float* rayf, const float* t, int t_stride, int nrays, int N, float* points, hipStream_t st) {
  hipLaunchKernelGGL(k_sample_points, dim3((nrays * N + 255) / 256), dim3(256), 0, st, rayf, t, t_stride, nrays, N, points);
  return hipGetLastError();
}

hipError_t launch_normal_composite(const float* w, const float* g, int B, int N, float* out, int out_stride, hipStream_t st) {
  hipLaunchKernelGGL(k_normal_composite, dim3((B + 3) / 4), dim3(256), 0, st, w, g, B, N, out, out_stride);
  return hipGetLastError();
}

}  // namespace nerf
