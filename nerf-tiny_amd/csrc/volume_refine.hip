// volume_refine.hip -- coarse-to-fine fine-tuning of a baked SH radiance volume: a total-variation prior over the level's active list,
// the x2 refinement of the lattice and the pruning of thin density (nerf_hip_volume_member_mask, _tv_backward, _upsample, _prune;
// DESIGN.md section 3h-14; rules VM, VT, VX and VP of include/nerf_hip.h).
//   k_volume_member           per list entry: a 1 into the (zeroed) mask
//   k_volume_tv               per (member, word): rule VT, a gather
//   k_volume_upsample         per (new point, word): rule VX, a gather
//   k_volume_prune_sigma      per point: rule VP's threshold
//   k_volume_prune_coef       per (point, coefficient word): +0 where the point is not active in the pruned sigma
//
// WHY THE TV KERNEL GATHERS.  The term of member p along axis a, Q_a(p), goes with a minus into p's word and with a plus into the word
// of p + e_a.  A scatter would need atomics, or two passes.  Here the thread of (q, word) forms every term ITS word receives: its own
// three Q_a(q), and for each axis the Q_a(q - e_a) of the backward neighbour when that one is a member, which costs that neighbour's tau
// (three more differences) again.  The terms are integers, so the order in which the thread sums them plays no role, and the word is
// read and written by this thread alone (the list's indices are distinct): a plain read-modify-write, no atomic, no LDS, nothing that
// depends on the launch order.  A Q_a(p) is the same llrint of the same fp64 expression in both threads that form it, so what p loses
// p + e_a gains exactly: the sum over the lattice of one word type is 0.
// ADDRESSES.  A neighbour's value is read only after its coordinate was compared with the lattice's size; the member byte of a point
// is read before any value of it.  Rule VX reads corner i + 1 only where the new index 2 i + 1 <= 2 n - 2 is odd, i.e. i <= n - 2.
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

namespace {

// the values of one word over the lattice: x(p) = base[p * stride]
struct VolWord {
  const float* base;
  long long stride;
};

// rule VT at the member p = (i, j, k) with the linear index lin: Q_x, Q_y, Q_z of this word
__device__ inline void vol_tv_terms(const VolTvArgs& a, const VolWord& x, int i, int j, int k, long long lin, double w, long long (&Q)[3]) {
  const long long sy = a.nz, sx = (long long)a.ny * a.nz;
  const double x0 = (double)x.base[lin * x.stride];
  double d[3] = {0.0, 0.0, 0.0};
  if (i + 1 < a.nx && a.member[lin + sx] != 0) d[0] = (double)x.base[(lin + sx) * x.stride] - x0;
  if (j + 1 < a.ny && a.member[lin + sy] != 0) d[1] = (double)x.base[(lin + sy) * x.stride] - x0;
  if (k + 1 < a.nz && a.member[lin + 1] != 0) d[2] = (double)x.base[(lin + 1) * x.stride] - x0;
  const double tau = sqrt((((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) + a.eps);
#pragma unroll
  for (int c = 0; c < 3; ++c) Q[c] = vol_fix(w * (d[c] / tau));
}

}  // namespace

// grid = ceil(n / VOL_WG); the mask was zeroed on the stream before
__global__ __launch_bounds__(VOL_WG) void k_volume_member(const VolMemberArgs a) {
  const long long m = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (m >= a.n) return;
  const long long p = a.index[m];
  if (p < 0 || p >= a.npts) return;  // never used as an address
  a.member[p] = 1;
}

// grid = ceil(n (1 + 3 ncoef) / VOL_WG): one thread per (member, word), the word fastest (k_volume_adam's mapping)
__global__ __launch_bounds__(VOL_WG) void k_volume_tv(const VolTvArgs a) {
  const long long W = 1 + 3 * (long long)a.ncoef;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.n * W) return;
  const long long pt = t / W;
  const int wd = (int)(t - pt * W);
  const long long npts = (long long)a.nx * a.ny * a.nz;
  const long long q = a.index[pt];
  if (q < 0 || q >= npts) return;  // never used as an address
  if (a.member[q] == 0) return;    // not a member of this level: it receives nothing
  const double w = wd == 0 ? a.w_sigma : a.w_coef;
  if (!(w > 0.0)) return;          // every term of this word is 0
  const int k = (int)(q % a.nz);
  const long long ij = q / a.nz;
  const int j = (int)(ij % a.ny), i = (int)(ij / a.ny);
  const long long sy = a.nz, sx = (long long)a.ny * a.nz;
  VolWord x;
  x.base = wd == 0 ? a.sigma : a.coef + (wd - 1);
  x.stride = wd == 0 ? 1 : W - 1;

  long long Q[3];
  vol_tv_terms(a, x, i, j, k, q, w, Q);
  long long sum = -Q[0] - Q[1] - Q[2];
  if (i > 0 && a.member[q - sx] != 0) {
    vol_tv_terms(a, x, i - 1, j, k, q - sx, w, Q);
    sum += Q[0];
  }
  if (j > 0 && a.member[q - sy] != 0) {
    vol_tv_terms(a, x, i, j - 1, k, q - sy, w, Q);
    sum += Q[1];
  }
  if (k > 0 && a.member[q - 1] != 0) {
    vol_tv_terms(a, x, i, j, k - 1, q - 1, w, Q);
    sum += Q[2];
  }
  long long* ap = wd == 0 ? a.acc_sigma + q : a.acc_coef + q * (W - 1) + (wd - 1);
  if (sum != 0) *ap = (long long)((unsigned long long)*ap + (unsigned long long)sum);
}

// grid = ceil(npts2 (1 + 3 ncoef) / VOL_WG): one thread per (new point, word), the word fastest
__global__ __launch_bounds__(VOL_WG) void k_volume_upsample(const VolUpsampleArgs a) {
  const long long W = 1 + 3 * (long long)a.ncoef;
  const int mx = 2 * a.nx - 1, my = 2 * a.ny - 1, mz = 2 * a.nz - 1;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= (long long)mx * my * mz * W) return;
  const long long P = t / W;
  const int wd = (int)(t - P * W);
  const int K = (int)(P % mz);
  const long long IJ = P / mz;
  const int J = (int)(IJ % my), I = (int)(IJ / my);
  const bool ox = (I & 1) != 0, oy = (J & 1) != 0, oz = (K & 1) != 0;
  // the far corner of an even axis is the near one again: never read past the lattice, and not used
  const long long dx = ox ? (long long)a.ny * a.nz : 0, dy = oy ? a.nz : 0, dz = oz ? 1 : 0;
  const long long base = ((long long)(I >> 1) * a.ny + (J >> 1)) * a.nz + (K >> 1);
  const float* __restrict__ src = wd == 0 ? a.sigma : a.coef + (wd - 1);
  const long long stride = wd == 0 ? 1 : W - 1;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = src[(base + ((c >> 2) & 1) * dx + ((c >> 1) & 1) * dy + (c & 1) * dz) * stride];
  // z first, then y, then x; an even index takes the value as it is
  float cz[4], cy[2];
#pragma unroll
  for (int c = 0; c < 4; ++c) cz[c] = oz ? vol_lerp(v[2 * c], v[2 * c + 1], 0.5f) : v[2 * c];
#pragma unroll
  for (int c = 0; c < 2; ++c) cy[c] = oy ? vol_lerp(cz[2 * c], cz[2 * c + 1], 0.5f) : cz[2 * c];
  const float r = ox ? vol_lerp(cy[0], cy[1], 0.5f) : cy[0];
  if (wd == 0) {
    a.sigma2[P] = r;
  } else {
    a.coef2[P * (W - 1) + (wd - 1)] = r;
  }
}

// grid = ceil(npts / VOL_WG)
__global__ __launch_bounds__(VOL_WG) void k_volume_prune_sigma(const VolPruneArgs a) {
  const long long p = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (p >= (long long)a.nx * a.ny * a.nz) return;
  const float s = a.sigma[p];
  a.sigma[p] = s > a.threshold ? s : 0.0f;
}

// grid = ceil(npts 3 ncoef / VOL_WG): one thread per (point, coefficient word); sigma is the pruned one
__global__ __launch_bounds__(VOL_WG) void k_volume_prune_coef(const VolPruneArgs a) {
  const long long C = 3 * (long long)a.ncoef;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= (long long)a.nx * a.ny * a.nz * C) return;
  const long long p = t / C;
  const int k = (int)(p % a.nz);
  const long long ij = p / a.nz;
  const int j = (int)(ij % a.ny), i = (int)(ij / a.ny);
  const int i0 = max(i - 1, 0), i1 = min(i + 1, a.nx - 1), j0 = max(j - 1, 0), j1 = min(j + 1, a.ny - 1);
  const int k0 = max(k - 1, 0), k1 = min(k + 1, a.nz - 1);
  bool on = a.sigma[p] > 0.0f;
  for (int x = i0; x <= i1 && !on; ++x)
    for (int y = j0; y <= j1 && !on; ++y)
      for (int z = k0; z <= k1; ++z) on = on || a.sigma[((long long)x * a.ny + y) * a.nz + z] > 0.0f;
  if (!on) a.coef[t] = 0.0f;
}

hipError_t launch_volume_member_mask(const VolMemberArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.member, 0, (size_t)a.npts, st));
  if (a.n > 0) LAUNCH(k_volume_member, dim3(grid(a.n, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_tv_backward(const VolTvArgs& a, hipStream_t st) {
  if (a.n > 0) LAUNCH(k_volume_tv, dim3(grid(a.n * (1 + 3 * (long long)a.ncoef), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_upsample(const VolUpsampleArgs& a, hipStream_t st) {
  const long long npts2 = (2ll * a.nx - 1) * (2ll * a.ny - 1) * (2ll * a.nz - 1);
  LAUNCH(k_volume_upsample, dim3(grid(npts2 * (1 + 3 * (long long)a.ncoef), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_prune(const VolPruneArgs& a, hipStream_t st) {
  const long long npts = (long long)a.nx * a.ny * a.nz;
  LAUNCH(k_volume_prune_sigma, dim3(grid(npts, VOL_WG)), dim3(VOL_WG), 0, st, a);
  LAUNCH(k_volume_prune_coef, dim3(grid(npts * 3 * a.ncoef, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
