// volume_grad.hip -- fine-tuning a baked SH radiance volume: the backward pass of the march and an Adam step over the baked active list
// (nerf_hip_volume_render_backward, nerf_hip_volume_adam_step; rules VG and VU of include/nerf_hip.h).
//   k_volume_march_grad<NC>   per ray: rule VG, one ray per lane, the scatter by the whole wave
//   k_volume_adam             per (active point, word): rule VU
//
// THE BACKWARD MARCH recomputes the ray and takes nothing from a forward call.  vol_step is ONE iteration of k_volume_march's loop
// (volume.hip), empty-block jump included, so both passes below see exactly the contributing samples of rule VR with the forward's own
// fp32 (w, T, colour, t): volume.hip's proof (V1) .. (V5) holds word for word.
//   pass 1   every lane marches its ray and sums S = sum_i w_i v_i in fp64
//   pass 2   marches again with the running P_i; a contributing sample yields dL/dsigma_s and dL/dc[3], and the WAVE scatters them
// THE SCATTER.  A corner's coefficient row is 3 NC consecutive int64 words (216 bytes at degree 2).  One lane scattering its own sample
// would issue 27 x 8 atomics with 64 different rows per instruction, the slow shape of global atomics (measured for f32 adds; the
// 64-bit integer form is not measured).  So pass 2's loop is wave-uniform -- it runs while any lane still has samples, lanes past N and
// lanes whose ray has ended stay in it as helpers, nothing returns in front of a broadcast -- and after every lane has advanced its own
// k the wave walks the ballot of the lanes that hold a contributing sample.  That lane's cell base, f, direction, dL/dc and dL/dsigma_s
// are read into scalars (readlane: the source lane is wave-uniform), and lane l adds word l % (3 NC) of corner slot l / (3 NC): 2
// corners per instruction at degree 2 (54 lanes), 4 at degree 1 (48 lanes), all 8 at degree 0 (24 lanes).  Corners 2 p and 2 p + 1 are
// neighbours along z, so their rows are contiguous: 432 bytes per instruction at degree 2.  The eight sigma words ride in the next eight
// lanes of the first instruction.  A lane's (corner slot, m, ch) is fixed for the whole kernel: Y_m and the channel are selected with
// compares, no register array is indexed with a runtime value (no scratch).
// The sums are integers (llrint(x 2^40)), so the accumulators do not depend on the order of arrival.  Every address is built from a cell
// clamped into [0, n - 2] per axis: all eight corners lie in the lattice.
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

namespace {

static_assert(VOL_GRAD_SHIFT == NERF_HIP_VOLUME_GRAD_SHIFT, "the header states the accumulators' fixed point");

// vol_color before its clamp (the same expressions: the clamped colour is fminf(fmaxf(raw, 0), 1) of it, bit for bit)
template <int NC>
__device__ inline void vol_color_raw(const float* __restrict__ coef, const long long (&p)[8], const float (&f)[3], const float (&Y)[9],
                                     float (&raw)[3]) {
  float v[3][8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float* __restrict__ q = coef + p[c] * (NC * 3);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float s = Y[0] * q[ch];
#pragma unroll
      for (int m = 1; m < NC; ++m) s = s + Y[m] * q[m * 3 + ch];
      v[ch][c] = s;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) raw[ch] = vol_tri(v[ch], f);
}

struct VolRay {
  float o[3], d[3], ta;
  int K;  // 0 for a miss
  float Y[9];
};

// a contributing sample, as the forward computes it
struct VolHit {
  long long base;  // the linear index of the cell's corner (0, 0, 0)
  float f[3], tk, w, Tn, c[3];
  bool pass[3];    // the unclamped colour lies in [0, 1]
};

// one iteration of k_volume_march's loop at sample k: k moves on, T is updated; true when the sample contributes (h is then filled);
// done is set where the forward breaks (T < t_stop)
template <int NC>
__device__ inline bool vol_step(const VolRenderArgs& a, const VolRay& ry, int& k, float& T, bool& done, VolHit& h) {
  const int dim[3] = {a.g.nx, a.g.ny, a.g.nz}, nb[3] = {a.bx, a.by, a.bz};
  const float tk = ry.ta + ((float)k + 0.5f) * a.dt;
  const float x[3] = {ry.o[0] + tk * ry.d[0], ry.o[1] + tk * ry.d[1], ry.o[2] + tk * ry.d[2]};
  int ci[3];
  float f[3];
  int next = k + 1;
  bool contributes = false;
  if (vol_cell(a.g, x, ci, f)) {
    int b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = min(ci[c] / a.B, nb[c] - 1);  // (ci >= 0, so b lies in [0, nb))
    if (a.occ[((long long)b[0] * a.by + b[1]) * a.bz + b[2]] != 0) {
      long long p[8];
      vol_corners(a.g, ci, p);
      const float s = vol_sigma(a.sigma, p, f);
      if (s > 0.0f) {
        float raw[3];
        vol_color_raw<NC>(a.coef, p, f, ry.Y, raw);
        const float alpha = -expm1f(-(s * a.dt));
        const float w = T * alpha;
        T = T - w;
        h.base = p[0];
        h.tk = tk;
        h.w = w;
        h.Tn = T;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          h.f[c] = f[c];
          h.c[c] = fminf(fmaxf(raw[c], 0.0f), 1.0f);
          h.pass[c] = 0.0f <= raw[c] && raw[c] <= 1.0f;
        }
        contributes = true;
        if (T < a.t_stop) done = true;
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
        if (ry.d[c] > 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c1[c] * a.g.step[c]) - ry.o[c]) / ry.d[c]);
        if (ry.d[c] < 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c0[c] * a.g.step[c]) - ry.o[c]) / ry.d[c]);
      }
      const float kf = fminf(floorf((te - ry.ta) / a.dt - 0.5f), (float)(ry.K - 1));  // (fminf drops a NaN)
      int ke = kf > (float)k ? (int)kf : k;
      for (int tries = 0; tries < 2 && ke > k; ++tries, --ke) {
        const float te2 = ry.ta + ((float)ke + 0.5f) * a.dt;
        const float xe[3] = {ry.o[0] + te2 * ry.d[0], ry.o[1] + te2 * ry.d[1], ry.o[2] + te2 * ry.d[2]};
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
  return contributes;
}

// rule VG's v_i
__device__ inline double vol_v(const VolHit& h, const float (&g)[3], double gD, double gA1) {
  return ((((double)g[0] * (double)h.c[0] + (double)g[1] * (double)h.c[1]) + (double)g[2] * (double)h.c[2]) + gD * (double)h.tk) + gA1;
}

// a value of lane src (wave-uniform) in every lane
__device__ inline float lane_value(float x, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src)); }
__device__ inline double lane_value(double x, int src) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ inline long long lane_value(long long x, int src) {
  const unsigned long long u = (unsigned long long)x;
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

}  // namespace

// grid = ceil(N / VOL_MARCH_WG): one ray per lane, one wave per workgroup
template <int NC>
__global__ __launch_bounds__(VOL_MARCH_WG) void k_volume_march_grad(const VolGradArgs ga) {
  static_assert(VOL_MARCH_WG == 64, "the scatter walks one wave's ballot");
  constexpr int ROW = 3 * NC;                          // int64 words of a corner's coefficient row
  constexpr int CPI = NC == 9 ? 2 : (NC == 4 ? 4 : 8);  // corners per scatter instruction
  static_assert(CPI * ROW + 8 <= 64, "the coefficient lanes and the eight sigma lanes of one instruction");
  const VolRenderArgs& a = ga.r;
  const int lane = threadIdx.x;
  const long long r = (long long)blockIdx.x * VOL_MARCH_WG + lane;
  const int dim[3] = {a.g.nx, a.g.ny, a.g.nz};

  // ---- this lane's ray (a lane past N holds a miss) ----
  VolRay ry;
  float g[3] = {0.0f, 0.0f, 0.0f}, gm[2] = {0.0f, 0.0f};
  float tmin = 0.0f, tmax = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) ry.o[c] = ry.d[c] = 0.0f;
  bool hit = r < a.N;
  if (hit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ry.o[c] = a.origins[r * 3 + c];
      ry.d[c] = a.dirs[r * 3 + c];
      g[c] = ga.g_rgb[r * 3 + c];
    }
    tmin = a.tmin[r], tmax = a.tmax[r];
    if (ga.g_maps) gm[0] = ga.g_maps[r * 2 + 0], gm[1] = ga.g_maps[r * 2 + 1];
  }
  hit = hit && finite3(ry.o) && finite3(ry.d) && isfinite(tmin) && isfinite(tmax) && finite3(g) && isfinite(gm[0]) && isfinite(gm[1]);
  float ta = tmin, tb = tmax;
  if (hit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float hi = a.g.lo[c] + (float)(dim[c] - 1) * a.g.step[c];
      if (ry.d[c] == 0.0f) {
        hit = hit && a.g.lo[c] <= ry.o[c] && ry.o[c] <= hi;
      } else {
        const float t1 = (a.g.lo[c] - ry.o[c]) / ry.d[c], t2 = (hi - ry.o[c]) / ry.d[c];
        ta = fmaxf(ta, fminf(t1, t2));
        tb = fminf(tb, fmaxf(t1, t2));
      }
    }
  }
  hit = hit && ta < tb;
  ry.ta = ta;
  ry.K = hit ? (int)fminf(ceilf((tb - ta) / a.dt), (float)VOL_MAX_STEPS) : 0;
  vol_basis(ry.d, ry.Y);
  const double gD = (double)gm[0];
  const double gA1 = (double)gm[1] - (((double)g[0] * (double)a.bg[0] + (double)g[1] * (double)a.bg[1]) + (double)g[2] * (double)a.bg[2]);
  const double dt = (double)a.dt;

  // ---- pass 1: S ----
  double S = 0.0;
  {
    int k = 0;
    float T = 1.0f;
    bool done = false;
    VolHit h;
#pragma unroll 1
    while (k < ry.K && !done)
      if (vol_step<NC>(a, ry, k, T, done, h)) S = S + (double)h.w * vol_v(h, g, gD, gA1);
  }

  // ---- this lane's words in a scatter instruction ----
  const int slot = lane / ROW, word = lane - slot * ROW;  // corner slot (< CPI for a coefficient lane) and the word of its row
  const int wm = word / 3, wch = word - wm * 3;
  const bool coef_lane = lane < CPI * ROW;
  const int sc = lane - CPI * ROW;                         // the corner of a sigma lane
  const bool sigma_lane = sc >= 0 && sc < 8;
  const long long sy = a.g.nz, sx = (long long)a.g.ny * a.g.nz;

  // ---- pass 2: the march again, the wave scatters ----
  int k = 0;
  float T = 1.0f;
  bool done = false;
  double P = 0.0;
#pragma unroll 1
  while (true) {
    const bool active = k < ry.K && !done;
    if (__ballot(active) == 0ull) break;
    VolHit h;
    h.base = 0;
    h.tk = h.w = h.Tn = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) h.f[c] = h.c[c] = 0.0f, h.pass[c] = false;
    bool has = false;
    double ds = 0.0, dc0 = 0.0, dc1 = 0.0, dc2 = 0.0;
    if (active && vol_step<NC>(a, ry, k, T, done, h)) {
      has = true;
      const double v = vol_v(h, g, gD, gA1);
      P = P + (double)h.w * v;
      ds = dt * ((double)h.Tn * v - (S - P));
      dc0 = h.pass[0] ? (double)h.w * (double)g[0] : 0.0;
      dc1 = h.pass[1] ? (double)h.w * (double)g[1] : 0.0;
      dc2 = h.pass[2] ? (double)h.w * (double)g[2] : 0.0;
    }
    unsigned long long todo = __ballot(has);
    while (todo != 0ull) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const long long base = lane_value(h.base, src);
      const double fx = (double)lane_value(h.f[0], src), fy = (double)lane_value(h.f[1], src), fz = (double)lane_value(h.f[2], src);
      const float db[3] = {lane_value(ry.d[0], src), lane_value(ry.d[1], src), lane_value(ry.d[2], src)};
      const double e0 = lane_value(dc0, src), e1 = lane_value(dc1, src), e2 = lane_value(dc2, src), es = lane_value(ds, src);
      float Yb[9];
      vol_basis(db, Yb);
      float ymf = Yb[0];
#pragma unroll
      for (int m = 1; m < NC; ++m) ymf = wm == m ? Yb[m] : ymf;
      const double ym = (double)ymf;
      const double e = wch == 0 ? e0 : (wch == 1 ? e1 : e2);
#pragma unroll
      for (int it = 0; it < 8 / CPI; ++it) {
        // a coefficient lane's corner of this instruction; in the first one a sigma lane's own corner
        const int c = (it == 0 && sigma_lane) ? sc : it * CPI + slot;
        const double tw = (((c >> 2) & 1 ? fx : 1.0 - fx) * ((c >> 1) & 1 ? fy : 1.0 - fy)) * (c & 1 ? fz : 1.0 - fz);
        const long long p = base + ((c >> 2) & 1) * sx + ((c >> 1) & 1) * sy + (c & 1);
        if (coef_lane) {
          const long long q = vol_fix((tw * ym) * e);
          if (q != 0) agent_add(ga.acc_coef + p * ROW + word, q);
        } else if (it == 0 && sigma_lane) {
          const long long q = vol_fix(tw * es);
          if (q != 0) agent_add(ga.acc_sigma + p, q);
        }
      }
    }
  }
}

// grid = ceil(n (1 + 3 ncoef) / VOL_WG): one thread per (active point, word)
__global__ __launch_bounds__(VOL_WG) void k_volume_adam(const VolAdamArgs a) {
  const long long W = 1 + 3 * (long long)a.ncoef;
  const long long i = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (i >= a.n * W) return;
  const long long pt = i / W;
  const int wd = (int)(i - pt * W);
  const long long p = a.index[pt];
  if (p < 0 || p >= a.npts) return;  // never used as an address
  float* xp = wd == 0 ? a.sigma + p : a.coef + p * (W - 1) + (wd - 1);
  long long* ap = wd == 0 ? a.acc_sigma + p : a.acc_coef + p * (W - 1) + (wd - 1);
  const long long acc = *ap;
  *ap = 0;
  const float x = *xp;
  if (wd == 0 && !(x > 0.0f)) return;  // dead: x, m and v are left alone
  const double lr = wd == 0 ? a.lr_sigma : a.lr_coef;
  const double g = ((double)acc * (1.0 / (double)(1ll << VOL_GRAD_SHIFT))) * a.grad_scale;
  const float m1 = (float)(a.beta1 * (double)a.m[i] + (1.0 - a.beta1) * g);
  const float v1 = (float)(a.beta2 * (double)a.v[i] + (1.0 - a.beta2) * (g * g));
  float x1 = (float)((double)x - lr * (((double)m1 / a.c1) / (sqrt((double)v1 / a.c2) + a.eps)));
  if (wd == 0) x1 = fmaxf(x1, 0.0f);
  a.m[i] = m1;
  a.v[i] = v1;
  *xp = x1;
}

hipError_t launch_volume_render_backward(const VolGradArgs& a, int ncoef, hipStream_t st) {
  if (a.r.N <= 0) return hipSuccess;
  const dim3 g(grid(a.r.N, VOL_MARCH_WG)), b(VOL_MARCH_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_march_grad<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_march_grad<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_march_grad<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_adam_step(const VolAdamArgs& a, hipStream_t st) {
  if (a.n > 0) LAUNCH(k_volume_adam, dim3(grid(a.n * (1 + 3 * (long long)a.ncoef), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
