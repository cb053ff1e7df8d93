// volume.hip -- SH radiance volumes: the field baked onto a dense lattice (sigma plus a few real spherical-harmonic colour coefficients
// per lattice point) and a ray-marcher with trilinear lookups (the nerf_hip_volume_* calls; the definitions
// are rules VA, VS, VO, VL and VR of include/nerf_hip.h).
//   scan.h's compaction over ActiveFlag   the ACTIVE lattice points (a positive sigma in the clipped 3 x 3 x 3 neighbourhood), ascending
//   k_volume_points       per active index: its world point by the lattice rule
//   k_volume_sh           per active point: one quadrature direction's term added to its (degree + 1)^2 x 3 coefficients
//   k_volume_blocks       per lattice point with sigma > 0: a 1 into the (at most eight) blocks whose cells touch it -- plain byte
//                         stores of the same value, so the order plays no role and there is no atomic
//   k_volume_sample<NC>   per point: rule VL
//   k_volume_march<NC>    per ray: rule VR, one ray per lane
// The lookup helpers (rule VL's cell, corners and interpolation, rule VS's basis) live in volume_parts.h, shared with volume_grad.hip.
//
// THE MARCH.  Everything a ray needs lives in its lane: origin, direction, the nine basis values of its direction (computed once), the
// running (C, D, A, T) and two counters.  No LDS, no atomics, no barrier; the lanes of a wave are neighbouring pixels, so their
// corners mostly share cache lines.  A sample reads its block's byte first, then the eight sigma corners, and the eight coefficient
// rows (12 NC bytes each, contiguous) only when sigma_s > 0: empty space never touches the coefficient array.  NC is a template
// parameter so that the coefficient loops unroll and nothing is indexed dynamically (no scratch).
//
// SKIPPING EMPTY BLOCKS.  Claim: for every block edge B the march accumulates exactly the contributing samples of rule VR, in order,
// so rgb, maps and steps[0] do not depend on B; only steps[1] does.
//   (V1) MONOTONE.  For a fixed ray, k -> t_k = fl(t_a + fl(fl(k + 0.5) dt)) is non-decreasing in k (dt > 0, rounding is monotone).
//        Per axis a, t -> x_a(t) = fl(o_a + fl(t d_a)) is monotone in t (in the direction of the sign of d_a), and
//        x -> g_a(x) = fl(fl(x - lo_a) / step_a) and g -> cell_a(g) = min(max(floor(g), 0), n_a - 2) are non-decreasing.  So along the
//        samples k -> g_a and k -> cell_a are monotone on every axis.
//   (V2) BRACKET.  If samples k < k' are both INSIDE and their cells lie in the same block on all three axes, then for every j in
//        between g_a(j) lies between g_a(k) and g_a(k'), hence in [0, n_a - 1]: sample j is inside; and cell_a(j) lies between two
//        cells of the block's range [b B, min((b + 1) B, n_a - 1)), hence in it: sample j lies in the same block.
//   (V3) AN EMPTY BLOCK CONTRIBUTES NOTHING.  occ[b] = 0 means no lattice point touched by a cell of b has sigma > 0 (rule VO); the
//        eight corners of a sample's cell are such points.  lerp(a, b, f) = fl(a + fl(f fl(b - a))) with 0 <= f <= 1 (f = g - cell is
//        in [0, 1] for an inside sample) of two values that are not > 0 is not > 0: with a NaN operand it is NaN; for b >= a,
//        fl(b - a) <= -a because b - a <= -a and -a is a float, so fl(f fl(b - a)) <= -a and the sum is <= 0; for b < a the product
//        is <= 0 and the sum <= a <= 0.  Three levels of it give sigma_s not > 0: the sample does not contribute.
//   (V4) THE JUMP.  At a sample k that is inside and in a block with occ = 0 the march estimates the last sample k' before the ray
//        leaves the block from the block's exit planes, and VERIFIES, by computing sample k' (and, failing that, k' - 1) with the
//        very expressions of rule VL, that it is inside and in the same block on all three axes.  Only then it continues at k' + 1:
//        by (V2) and (V3) none of k .. k' contributes.  The estimate is a guess for speed; the verification is what the proof uses.
//        Otherwise it continues at k + 1.  Samples outside the lattice are stepped one at a time.
//   (V5) TERMINATION.  Every step advances k by at least 1 and K <= VOL_MAX_STEPS.
// T changes only at contributing samples, so the early end (T < t_stop) falls on the same sample for every B.
// Every index that becomes an address -- the cell, the block -- is clamped into its array first; indices read from memory (the
// active list) are checked against the lattice before use.
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

namespace {

// ---- rule VA ----

// is lattice point i ACTIVE?  (sigma is an input of both scan launches: nothing changes a flag between them)
struct ActiveFlag {
  const float* sigma;
  int nx, ny, nz;
  __device__ int operator()(long long i) const {
    const int k = (int)(i % nz);
    const long long ij = i / nz;
    const int j = (int)(ij % ny), ii = (int)(ij / ny);
    const int i0 = ii > 0 ? ii - 1 : 0, i1 = ii < nx - 1 ? ii + 1 : nx - 1;
    const int j0 = j > 0 ? j - 1 : 0, j1 = j < ny - 1 ? j + 1 : ny - 1;
    const int k0 = k > 0 ? k - 1 : 0, k1 = k < nz - 1 ? k + 1 : nz - 1;
    int any = 0;
    for (int a = i0; a <= i1; ++a)
      for (int b = j0; b <= j1; ++b)
        for (int c = k0; c <= k1; ++c) any |= sigma[((long long)a * ny + b) * nz + c] > 0.0f ? 1 : 0;
    return any;
  }
};

struct ActiveSink {
  int* index;
  long long max_n;
  __device__ void operator()(long long i, int fl, long long pos) const {
    if (fl && pos < max_n) index[pos] = (int)i;
  }
};

}  // namespace

// grid = ceil(n / VOL_WG)
__global__ __launch_bounds__(VOL_WG) void k_volume_points(const VolPointsArgs a) {
  const long long m = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (m >= a.n) return;
  const long long npts = (long long)a.g.nx * a.g.ny * a.g.nz;
  const long long idx = a.index[m];
  float p[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (idx >= 0 && idx < npts) {
    const int k = (int)(idx % a.g.nz);
    const long long ij = idx / a.g.nz;
    const int j = (int)(ij % a.g.ny), i = (int)(ij / a.g.ny);
    p[0] = a.g.lo[0] + (float)i * a.g.step[0];
    p[1] = a.g.lo[1] + (float)j * a.g.step[1];
    p[2] = a.g.lo[2] + (float)k * a.g.step[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a.points[m * 3 + c] = p[c];
}

// grid = ceil(n / VOL_WG).  The indices of a call are distinct: a point's coefficients belong to one thread.
__global__ __launch_bounds__(VOL_WG) void k_volume_sh(const VolShArgs a) {
  const long long m = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (m >= a.n) return;
  const long long idx = a.index[m];
  if (idx < 0 || idx >= a.npts) return;  // never used as an address
  const float rgb[3] = {a.rgb[m * 3 + 0], a.rgb[m * 3 + 1], a.rgb[m * 3 + 2]};
  float* __restrict__ q = a.coef + idx * ((long long)a.ncoef * 3);
  for (int c = 0; c < a.ncoef; ++c)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) q[c * 3 + ch] = q[c * 3 + ch] + a.b[c] * rgb[ch];
}

// grid = ceil(npts / VOL_WG).  occ was zeroed by the launch sequence; every store writes 1.
__global__ __launch_bounds__(VOL_WG) void k_volume_blocks(const VolBlocksArgs a) {
  const long long idx = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (idx >= (long long)a.nx * a.ny * a.nz) return;
  if (!(a.sigma[idx] > 0.0f)) return;
  const int k = (int)(idx % a.nz);
  const long long ij = idx / a.nz;
  const int j = (int)(ij % a.ny), i = (int)(ij / a.ny);
  // point i is touched by the cells i - 1 and i, clipped to [0, n - 2]
  const int p[3] = {i, j, k}, dim[3] = {a.nx, a.ny, a.nz}, nb[3] = {a.bx, a.by, a.bz};
  int b0[3], b1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int c0 = p[c] > 0 ? p[c] - 1 : 0, c1 = p[c] < dim[c] - 2 ? p[c] : dim[c] - 2;
    b0[c] = min(c0 / a.B, nb[c] - 1);
    b1[c] = min(c1 / a.B, nb[c] - 1);
  }
  for (int x = b0[0]; x <= b1[0]; ++x)
    for (int y = b0[1]; y <= b1[1]; ++y)
      for (int z = b0[2]; z <= b1[2]; ++z) a.occ[((long long)x * a.by + y) * a.bz + z] = 1;
}

// grid = ceil(M / VOL_WG)
template <int NC>
__global__ __launch_bounds__(VOL_WG) void k_volume_sample(const VolSampleArgs a) {
  const long long m = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (m >= a.M) return;
  const float x[3] = {a.points[m * 3 + 0], a.points[m * 3 + 1], a.points[m * 3 + 2]};
  const float d[3] = {a.dirs[m * 3 + 0], a.dirs[m * 3 + 1], a.dirs[m * 3 + 2]};
  int ci[3];
  float f[3], s = 0.0f, rgb[3] = {0.0f, 0.0f, 0.0f};
  if (vol_cell(a.g, x, ci, f)) {
    long long p[8];
    vol_corners(a.g, ci, p);
    s = vol_sigma(a.sigma, p, f);
    float Y[9];
    vol_basis(d, Y);
    vol_color<NC>(a.coef, p, f, Y, rgb);
  }
  a.out_sigma[m] = s;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.out_rgb[m * 3 + c] = rgb[c];
}

// grid = ceil(N / VOL_MARCH_WG): one ray per lane
template <int NC>
__global__ __launch_bounds__(VOL_MARCH_WG) void k_volume_march(const VolRenderArgs a) {
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
    float T = 1.0f;
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
          vol_corners(a.g, ci, p);
          const float s = vol_sigma(a.sigma, p, f);
          if (s > 0.0f) {
            float rgb[3];
            vol_color<NC>(a.coef, p, f, Y, rgb);
            const float alpha = -expm1f(-(s * a.dt));
            const float w = T * alpha;
#pragma unroll
            for (int c = 0; c < 3; ++c) C[c] = C[c] + w * rgb[c];
            D = D + w * tk;
            A = A + w;
            T = T - w;
            ++contributing;
            if (T < a.t_stop) break;
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

hipError_t launch_volume_active(const VolActiveArgs& a, bool emit, hipStream_t st) {
  const long long npts = (long long)a.nx * a.ny * a.nz;
  const ActiveFlag flag{a.sigma, a.nx, a.ny, a.nz};
  if (emit) return scan_place(flag, ActiveSink{a.index, a.max_n}, npts, a.tot, a.base, a.count, st);
  return scan_count(flag, npts, a.tot, a.base, a.count, st);
}

hipError_t launch_volume_points(const VolPointsArgs& a, hipStream_t st) {
  if (a.n > 0) LAUNCH(k_volume_points, dim3(grid(a.n, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_sh_accumulate(const VolShArgs& a, hipStream_t st) {
  if (a.n > 0) LAUNCH(k_volume_sh, dim3(grid(a.n, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_blocks(const VolBlocksArgs& a, hipStream_t st) {
  const long long npts = (long long)a.nx * a.ny * a.nz;
  TRY(hipMemsetAsync(a.occ, 0, (size_t)a.bx * a.by * a.bz, st));
  LAUNCH(k_volume_blocks, dim3(grid(npts, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_sample(const VolSampleArgs& a, int ncoef, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  const dim3 g(grid(a.M, VOL_WG)), b(VOL_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_sample<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_sample<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_sample<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_render(const VolRenderArgs& a, int ncoef, hipStream_t st) {
  if (a.N <= 0) return hipSuccess;
  const dim3 g(grid(a.N, VOL_MARCH_WG)), b(VOL_MARCH_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_march<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_march<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_march<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

}  // namespace nerf
