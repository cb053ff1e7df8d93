// volume_compact.hip -- compact SH radiance volumes: the rows of the ACTIVE lattice points (rule VA) behind an int32 slot lattice, the
// coefficients fp32 or fp16 (the nerf_hip_volume_compact_* calls; rule VC of include/nerf_hip.h).
//   k_volume_compact_slots          per row r: slot[index[r]] = r, into a lattice the launch sequence filled with -1
//   k_volume_compact_pack<T>        per (row, word): the dense lattice's words of index[r] gathered into rows; T = _Float16 rounds to
//                                   nearest even and writes the pad halves as +0.  A null index is the identity (rows -> rows)
//   k_volume_compact_unpack<T>      per (row, word): the inverse scatter into dense arrays the caller zeroed
//   k_volume_compact_sample<NC, T>  per point: rule VC-L
//   k_volume_compact_march<NC, T>   per ray: rule VC-R, one ray per lane
// The lookup helpers (volc_rows, volc_sigma, volc_row, volc_color) live in volume_parts.h beside rule VL's, which they reuse
// (vol_cell, vol_corners, vol_tri, vol_basis).
//
// THE MARCH is k_volume_march's loop, expression for expression, with the two array reads replaced: per sample the block byte, then
// the eight slots, then up to eight sigma words (one per corner whose slot lies in [0, n)), and the eight rows only when sigma_s > 0.
// One ray per lane, workgroups of one wave, no LDS, no atomics, no barrier.  NC and T are template parameters: the row loops unroll,
// nothing is indexed with a runtime value (no scratch).  An fp16 row is 4 / 12 / 28 halves and starts on an 8-byte boundary, so it is
// read as 1 / 3 / 7 eight-byte words and widened in registers; an fp32 row is read as the dense row is.  This file, volume.hip and
// volume_grad.hip now hold three copies of the loop; one body over a storage policy is a follow-up.
//
// EQUIVALENCE.  Claims: (A) for a compact volume C and U = unpack(C) -- the dense volume with C's rows at the points whose slot lies
// in [0, n), +0 everywhere else, fp16 rows widened -- VC-L on C equals VL on U and VC-R on C equals VR on U, bit for bit.  (B) for ANY
// dense volume V, garbage at its inactive points included (negative sigma, -0, NaN, non-zero coefficients), rgb, maps and both
// columns of steps of VC-R on pack(V) equal VR on V bit for bit.
//   (C1) THE SAME OPERANDS.  volc_rows turns a corner p into the row slot[p] if 0 <= slot[p] < n and into "none" otherwise; volc_sigma
//        and volc_row then hand vol_tri / the bracketed sums sigma_rows[slot[p]] and coef_rows[slot[p]][.] or the constant +0.  Those
//        are U's words at p by the definition of U; widening fp16 to fp32 is exact, so widening on load and widening in unpack give the
//        same fp32 word.  Everything downstream (vol_cell, vol_tri, vol_basis, the sums in vol_color's order, the clamp) is the very
//        code of rule VL applied to equal operands -- a +0 row goes through the same products, it is not short-cut.  Hence VC-L = VL(U).
//   (C2) THE SAME LOOP.  The march computes t_k, x, the cell, the block, the jump of (V4), alpha, w, C, D, A, T with k_volume_march's
//        expressions in its order; occ, lo, step, B and the rays are the same inputs.  By (C1) every s and rgb is the same word, so
//        every branch goes the same way and every accumulator holds the same bits: VC-R = VR(U), steps[1] included.  This is (A).
//   (C3) INACTIVE POINTS DO NOT MATTER.  Let V be any dense volume, C = pack(V), U = unpack(C): U is V with sigma +0 and a +0 row at
//        every inactive point.  An inactive point q has no positive sigma in its clipped 3 x 3 x 3 neighbourhood (rule VA), and every
//        corner of a cell that has q as a corner lies in that neighbourhood; so all eight corners of such a cell are not > 0 in V, and
//        still not > 0 in U (some replaced by +0).  By (V3) of volume.hip -- three levels of lerp over values that are not > 0 -- the
//        cell's sigma_s is not > 0 in V and in U: the sample contributes in neither, whatever q holds, NaN included.
//   (C4) CONTRIBUTING SAMPLES READ ONLY ACTIVE POINTS.  A sample with sigma_s > 0 (in V or in U) has a corner with sigma > 0, by the
//        contrapositive of (V3); that corner's sigma is the same in V and U (a positive point is active).  All eight corners of the
//        cell lie in that corner's neighbourhood, so all eight are active and carry V's own words in U: s and rgb are the same bits in
//        V and U.  With (C3): the two marches agree on WHICH samples contribute and on their values.
//   (C5) THE SAME SAMPLES ARE LOOKED AT.  occ is rule VO's of V's sigma, which depends only on the points with sigma > 0; those are
//        active and unchanged, so occ(V) = occ(U) and the jumps of (V4) fall alike: steps[1] agrees too.  VR(V) = VR(U) = VC-R(C): (B).
// For T = _Float16, (B) holds against V with every coefficient replaced by fp32(fp16(.)): pack rounds, nothing else differs.
// Every index that becomes an address is clamped (cell, block: vol_cell and the min below) or compared with its array's size first
// (index[r] against the lattice, slot[p] against n); row addresses are formed in 64 bits.
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

// grid = ceil(n / VOL_WG).  The indices of an active list are distinct: a slot belongs to one thread.
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_slots(const VolSlotsArgs a) {
  const long long r = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (r >= a.n) return;
  const long long idx = a.index[r];
  if (idx < 0 || idx >= a.npts) return;  // never used as an address
  a.slot[idx] = (int)r;
}

// the words of a stored row (pad halves included), and the stored form of an fp32 word
template <class T>
__device__ inline int volc_stride(int ncoef);
template <>
__device__ inline int volc_stride<float>(int ncoef) { return 3 * ncoef; }
template <>
__device__ inline int volc_stride<_Float16>(int ncoef) { return vol_half_stride(ncoef); }

// grid = ceil(n (1 + stride) / VOL_WG): word 0 of a row is its sigma, words 1 .. stride its coefficients and pad
template <class T>
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_pack(const VolPackArgs a) {
  const int S = volc_stride<T>(a.ncoef), nw = 3 * a.ncoef;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.n * (S + 1)) return;
  const long long r = t / (S + 1);
  const int w = (int)(t % (S + 1));
  const long long idx = a.index ? (long long)a.index[r] : r;
  const bool ok = idx >= 0 && idx < a.npts;  // an index outside the lattice gives a +0 row
  if (w == 0) {
    if (a.sigma_rows) a.sigma_rows[r] = ok ? a.sigma[idx] : 0.0f;
  } else if (a.coef_rows) {
    const float v = (ok && w - 1 < nw) ? a.coef[idx * nw + (w - 1)] : 0.0f;
    static_cast<T*>(a.coef_rows)[r * S + (w - 1)] = (T)v;  // fp16: round to nearest even, past 65504 to +-inf
  }
}

// grid = ceil(n (1 + 3 ncoef) / VOL_WG)
template <class T>
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_unpack(const VolPackArgs a) {
  const int S = volc_stride<T>(a.ncoef), nw = 3 * a.ncoef;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.n * (nw + 1)) return;
  const long long r = t / (nw + 1);
  const int w = (int)(t % (nw + 1));
  const long long idx = a.index ? (long long)a.index[r] : r;
  if (idx < 0 || idx >= a.npts) return;  // never used as an address
  if (w == 0) {
    if (a.sigma) a.sigma[idx] = a.sigma_rows[r];
  } else if (a.coef) {
    a.coef[idx * nw + (w - 1)] = (float)static_cast<const T*>(a.coef_rows)[r * S + (w - 1)];
  }
}

// grid = ceil(M / VOL_WG)
template <int NC, class T>
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_sample(const VolCompactSampleArgs a) {
  const long long m = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (m >= a.M) return;
  const float x[3] = {a.points[m * 3 + 0], a.points[m * 3 + 1], a.points[m * 3 + 2]};
  const float d[3] = {a.dirs[m * 3 + 0], a.dirs[m * 3 + 1], a.dirs[m * 3 + 2]};
  int ci[3];
  float f[3], s = 0.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
  if (vol_cell(a.g, x, ci, f)) {
    long long p[8];
    int row[8];
    vol_corners(a.g, ci, p);
    volc_rows(a.c, p, row);
    s = volc_sigma(a.c.sigma_rows, row, f);
    float Y[9];
    vol_basis(d, Y);
    volc_color<NC>(static_cast<const T*>(a.c.coef_rows), row, f, Y, rgb);
  }
  a.out_sigma[m] = s;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.out_rgb[m * 3 + c] = rgb[c];
}

// grid = ceil(N / VOL_MARCH_WG): one ray per lane.  k_volume_march's loop over the compact form.
template <int NC, class T>
__global__ __launch_bounds__(VOL_MARCH_WG) void k_volume_compact_march(const VolCompactRenderArgs ca) {
  const VolRenderArgs& a = ca.r;
  const T* __restrict__ rows = static_cast<const T*>(ca.c.coef_rows);
  const long long r = (long long)blockIdx.x * VOL_MARCH_WG + threadIdx.x;
  if (r >= a.N) return;
  const float o[3] = {a.origins[r * 3 + 0], a.origins[r * 3 + 1], a.origins[r * 3 + 2]};
  const float d[3] = {a.dirs[r * 3 + 0], a.dirs[r * 3 + 1], a.dirs[r * 3 + 2]};
  const float tmin = a.tmin[r], tmax = a.tmax[r];
  const int dim[3] = {a.g.nx, a.g.ny, a.g.nz}, nb[3] = {a.bx, a.by, a.bz};
  float C[3] = {0.0f, 0.0f, 0.0f}, D = 0.0f, A = 0.0f;
  int contributing = 0, evaluated = 0;
  bool hit = finite3(o) && finite3(d) && isfinite(tmin) && isfinite(tmax);
  float ta = tmin, tb = tmax;
  if (hit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float hi = a.g.lo[c] + (float)(dim[c] - 1) * a.g.step[c];
      if (d[c] == 0.0f) {
        hit = hit && a.g.lo[c] <= o[c] && o[c] <= hi;
      } else {
        const float t1 = (a.g.lo[c] - o[c]) / d[c], t2 = (hi - o[c]) / d[c];
        ta = fmaxf(ta, fminf(t1, t2));
        tb = fminf(tb, fmaxf(t1, t2));
      }
    }
  }
  hit = hit && ta < tb;
  if (hit) {
    const int K = (int)fminf(ceilf((tb - ta) / a.dt), (float)VOL_MAX_STEPS);
    float Y[9];
    vol_basis(d, Y);
    float T_ = 1.0f;
    int k = 0;
#pragma unroll 1
    while (k < K) {
      const float tk = ta + ((float)k + 0.5f) * a.dt;
      const float x[3] = {o[0] + tk * d[0], o[1] + tk * d[1], o[2] + tk * d[2]};
      int ci[3];
      float f[3];
      ++evaluated;
      int next = k + 1;
      if (vol_cell(a.g, x, ci, f)) {
        int b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = min(ci[c] / a.B, nb[c] - 1);  // (ci >= 0, so b lies in [0, nb))
        if (a.occ[((long long)b[0] * a.by + b[1]) * a.bz + b[2]] != 0) {
          long long p[8];
          int row[8];
          vol_corners(a.g, ci, p);
          volc_rows(ca.c, p, row);
          const float s = volc_sigma(ca.c.sigma_rows, row, f);
          if (s > 0.0f) {
            float rgb[3];
            volc_color<NC>(rows, row, f, Y, rgb);
            const float alpha = -expm1f(-(s * a.dt));
            const float w = T_ * alpha;
#pragma unroll
            for (int c = 0; c < 3; ++c) C[c] = C[c] + w * rgb[c];
            D = D + w * tk;
            A = A + w;
            T_ = T_ - w;
            ++contributing;
            if (T_ < a.t_stop) break;
          }
        } else {
          // (V4) the block's range of cells per axis, the exit planes' t (a guess), the candidate, its verification
          int c0[3], c1[3];
          float te = VOL_INF;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const long long up = ((long long)b[c] + 1) * a.B;
            c0[c] = b[c] * a.B;  // <= ci
            c1[c] = up < dim[c] - 1 ? (int)up : dim[c] - 1;
            if (d[c] > 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c1[c] * a.g.step[c]) - o[c]) / d[c]);
            if (d[c] < 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c0[c] * a.g.step[c]) - o[c]) / d[c]);
          }
          const float kf = fminf(floorf((te - ta) / a.dt - 0.5f), (float)(K - 1));  // (fminf drops a NaN)
          int ke = kf > (float)k ? (int)kf : k;
          for (int tries = 0; tries < 2 && ke > k; ++tries, --ke) {
            const float te2 = ta + ((float)ke + 0.5f) * a.dt;
            const float xe[3] = {o[0] + te2 * d[0], o[1] + te2 * d[1], o[2] + te2 * d[2]};
            int ce[3];
            float fe[3];
            if (vol_cell(a.g, xe, ce, fe) && c0[0] <= ce[0] && ce[0] < c1[0] && c0[1] <= ce[1] && ce[1] < c1[1] && c0[2] <= ce[2] &&
                ce[2] < c1[2]) {
              next = ke + 1;
              break;
            }
          }
        }
      }
      k = next;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a.rgb[r * 3 + c] = C[c] + (1.0f - A) * a.bg[c];
  a.maps[r * 2 + 0] = D;
  a.maps[r * 2 + 1] = A;
  a.steps[r * 2 + 0] = contributing;
  a.steps[r * 2 + 1] = evaluated;
}

hipError_t launch_volume_compact_slots(const VolSlotsArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.slot, 0xFF, (size_t)a.npts * 4, st));  // every slot -1
  if (a.n > 0) LAUNCH(k_volume_compact_slots, dim3(grid(a.n, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_compact_pack(const VolPackArgs& a, bool half, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const dim3 b(VOL_WG);
  if (half) {
    LAUNCH(k_volume_compact_pack<_Float16>, dim3(grid(a.n * (vol_half_stride(a.ncoef) + 1), VOL_WG)), b, 0, st, a);
  } else {
    LAUNCH(k_volume_compact_pack<float>, dim3(grid(a.n * (3 * a.ncoef + 1), VOL_WG)), b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_compact_unpack(const VolPackArgs& a, bool half, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  const dim3 g(grid(a.n * (3 * a.ncoef + 1), VOL_WG)), b(VOL_WG);
  if (half) {
    LAUNCH(k_volume_compact_unpack<_Float16>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_compact_unpack<float>, g, b, 0, st, a);
  }
  return hipSuccess;
}

namespace {

template <class T>
hipError_t sample_of(const VolCompactSampleArgs& a, int ncoef, hipStream_t st) {
  const dim3 g(grid(a.M, VOL_WG)), b(VOL_WG);
  if (ncoef == 1) {
    LAUNCH((k_volume_compact_sample<1, T>), g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH((k_volume_compact_sample<4, T>), g, b, 0, st, a);
  } else {
    LAUNCH((k_volume_compact_sample<9, T>), g, b, 0, st, a);
  }
  return hipSuccess;
}

template <class T>
hipError_t march_of(const VolCompactRenderArgs& a, int ncoef, hipStream_t st) {
  const dim3 g(grid(a.r.N, VOL_MARCH_WG)), b(VOL_MARCH_WG);
  if (ncoef == 1) {
    LAUNCH((k_volume_compact_march<1, T>), g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH((k_volume_compact_march<4, T>), g, b, 0, st, a);
  } else {
    LAUNCH((k_volume_compact_march<9, T>), g, b, 0, st, a);
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_volume_compact_sample(const VolCompactSampleArgs& a, int ncoef, bool half, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  return half ? sample_of<_Float16>(a, ncoef, st) : sample_of<float>(a, ncoef, st);
}

hipError_t launch_volume_compact_render(const VolCompactRenderArgs& a, int ncoef, bool half, hipStream_t st) {
  if (a.r.N <= 0) return hipSuccess;
  return half ? march_of<_Float16>(a, ncoef, st) : march_of<float>(a, ncoef, st);
}

}  // namespace nerf
