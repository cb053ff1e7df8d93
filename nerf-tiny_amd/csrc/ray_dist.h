// ray_dist.h -- rule DL (include/nerf_hip.h): the distortion loss of ONE pass of one ray and its gradients, as pieces for ONE 64-lane wave
// that the per-ray stages of ray_parts.h (forward) and ray_parts_bwd.h (backward) call from their own loops.  Everything here is fp64 on
// the fp32 weights and depths widened exactly; `scan` is the caller's inclusive fp64 wave scan.  No barrier, no LDS of its own.
#pragma once
#include "kernels.h"

namespace nerf {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
// r of rule DL
__device__ __forceinline__ double dist_ray_scale(float near, float far) { return 1.0 / ((double)far - (double)near); }
// ... of ray `ray` for the merge kernels, from the bounds the extras record carries for them (kernels.h RayExtras)
__device__ __forceinline__ float dist_near(const RayExtras& x, int ray) { return x.rayf ? x.rayf[(size_t)ray * RAYF + RF_NEAR] : x.near_far[2 * ray]; }
__device__ __forceinline__ float dist_far(const RayExtras& x, int ray) { return x.rayf ? x.rayf[(size_t)ray * RAYF + RF_FAR] : x.near_far[2 * ray + 1]; }
__device__ __forceinline__ double dist_ray_scale(const RayExtras& x, int ray) { return dist_ray_scale(dist_near(x, ray), dist_far(x, ray)); }

// The prefix form, chunk by chunk: step() takes lane l's sample of the chunk (w_i, t_i, t_{i+1}; has_next = i < N - 1; lanes behind the
// ray pass w = 0, t = 0) and leaves its m_i, d_i and the exclusive prefixes We_i, Se_i in index order.  Every lane of the wave calls it.
struct DistScan {
  double cw = 0.0, cs = 0.0;  // W and S of the chunks before this one
  double m, d, We, Se;
  template <class Scan>
  __device__ __forceinline__ void step(float wi, float ti, float tn, bool has_next, int lane, Scan&& scan) {
    const double t0 = (double)ti, t1 = (double)tn, w = (double)wi;
    m = has_next ? (t0 + t1) * 0.5 : t0;
    d = has_next ? t1 - t0 : 0.0;  // (the last interval is never extrapolated)
    const double iw = scan(w, lane) + cw, is = scan(w * m, lane) + cs;
    const double uw = __shfl_up(iw, 1), us = __shfl_up(is, 1);
    We = lane ? uw : cw;
    Se = lane ? us : cs;
    cw = __shfl(iw, 63);
    cs = __shfl(is, 63);
  }
  // this lane's summand of L / r
  __device__ __forceinline__ double summand(float wi) const {
    const double w = (double)wi;
    return 2.0 * w * (m * We - Se) + w * w * d / 3.0;
  }
};

// The backward's terms of one pass: w [N] (LDS, written by this wave and ordered before this call), t_at(i) = t_i, g = the ray's upstream
// dloss / dL.  A first sweep takes the totals W and S (per lane, then a butterfly), a second one re-forms the prefixes and hands
// emit(i, fp32(double(g) dL/dw_i), fp32(double(g) dL/dt_i)) to lane i % 64 for every i < N.
template <class TAt, class Scan, class Emit>
__device__ __forceinline__ void dist_grad_terms(const float* w, TAt&& t_at, int N, double r, float g, int lane, Scan&& scan, Emit&& emit) {
  double Wl = 0.0, Sl = 0.0;
  for (int i = lane; i < N; i += 64) {
    const double t0 = (double)t_at(i);
    const double m = (i + 1 < N) ? (t0 + (double)t_at(i + 1)) * 0.5 : t0;
    Wl += (double)w[i];
    Sl += (double)w[i] * m;
  }
  const double W = wave_sum_f64(Wl), S = wave_sum_f64(Sl);
  DistScan sc;
  double a_carry = 0.0, q_carry = 0.0;  // a_{i-1}, w_{i-1}^2 / 3 of the chunk before
  for (int base = 0; base < N; base += 64) {
    const int i = base + lane;
    const bool v = i < N, hn = i + 1 < N;
    const float wi = v ? w[i] : 0.f;
    const float ti = v ? t_at(i) : 0.f;
    const float tn = hn ? t_at(i + 1) : ti;
    sc.step(wi, ti, tn, hn, lane, scan);
    const double wd = (double)wi;
    const double P = sc.m * sc.We - sc.Se;
    const double R = (S - sc.Se - wd * sc.m) - sc.m * (W - sc.We - wd);
    const double dLdw = r * (2.0 * (P + R) + 2.0 * wd * sc.d / 3.0);
    const double a = 2.0 * wd * (sc.We - (W - sc.We - wd));
    const double q = wd * wd / 3.0;
    double ap = __shfl_up(a, 1), qp = __shfl_up(q, 1);
    if (lane == 0) { ap = a_carry; qp = q_carry; }
    a_carry = __shfl(a, 63);
    q_carry = __shfl(q, 63);
    const double dLdt = r * ((hn ? 0.5 * a - q : a) + (i >= 1 ? 0.5 * ap + qp : 0.0));
    if (v) emit(i, (float)((double)g * dLdw), (float)((double)g * dLdt));
  }
}

}  // namespace nerf
