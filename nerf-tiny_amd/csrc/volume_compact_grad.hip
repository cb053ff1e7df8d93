// volume_compact_grad.hip -- fine-tuning a compact SH radiance volume: the backward pass of the compact march, an Adam step over the rows
// and the TV prior through the slot lattice (nerf_hip_volume_compact_render_backward, _adam_step, _tv_backward; DESIGN.md section 3h-16;
// rules VCG, VCU and VCT of include/nerf_hip.h).  The rows are fp32; the accumulators and the moments are one per row.
//   k_volume_compact_march_grad<NC>   per ray: rule VCG, one ray per lane, the scatter by the whole wave
//   k_volume_compact_adam             per (row, word): rule VCU
//   k_volume_compact_tv               per (row, word): rule VCT, a gather
//
// THE BACKWARD MARCH is k_volume_march_grad (volume_grad.hip) with volume_compact.hip's two array reads: volc_step is ONE iteration of
// k_volume_compact_march's loop, empty-block jump included, and the two passes, the fp64 brackets, the ballot walk and the lane layout
// (lane l adds word l % (3 NC) of the corner l / (3 NC) + CPI it; the eight sigma words ride in the next eight lanes of the first
// instruction) are the dense kernel's.  It differs in one thing: not a cell base but the EIGHT ROWS of the source lane's cell are
// broadcast (readlane: eight scalars), and a lane picks its corner's row with compares against its fixed corner -- no register array
// is indexed with a runtime value.  A row is the slot of the corner where that lies in [0, n) and -1 otherwise (volc_rows); a corner
// without a row receives nothing, and only a checked slot becomes an address, formed in 64 bits.
// CONTIGUITY (an observation, nothing depends on it).  Corners 2 p and 2 p + 1 are z-neighbours.  In an ascending active list with z
// fastest two active z-neighbours are consecutive entries, so their slots are r and r + 1: the two rows of one degree-2 instruction are
// again 432 contiguous bytes, as in the dense kernel.  That holds for packed volumes only; any slot lattice gives the same sums.
// This is the fourth copy of the march loop; one body over a storage policy stays the follow-up of DESIGN.md section 3h-15.  vol_v and
// lane_value are volume_grad.hip's, which keeps them in its own unnamed namespace.
//
// EQUIVALENCE.  Let C be a compact volume with fp32 rows whose slots in [0, n) are distinct, U = unpack(C), and index[r] the point
// whose slot is r (-1: none).  Claims: (A) after the same calls on zeroed accumulators, acc_*_rows[r] equals the dense accumulator word
// at index[r] bit for bit -- VCG on C against VG on U, VCT on C against VT on U with member_mask(index) --, and VCU leaves sigma_rows,
// coef_rows, m and v equal to VU's on U over index at those points.  (B) if C = pack(V) for ANY dense V, garbage at its inactive
// points included, VG on V adds nothing outside the list and agrees with VCG on C inside it.
//   (G1) THE SAME SAMPLES, THE SAME VALUES.  volc_step reads what k_volume_compact_march reads and computes t_k, the cell, the block,
//        the jump, sigma_s, alpha, w and T with its expressions; by (C1) and (C2) of volume_compact.hip those are the words of VR on U.
//        volc_color_raw is volc_color without the clamp, as vol_color_raw is vol_color without it: by (C1) the unclamped colour is U's,
//        so c_i, the pass flags, f and t_i are U's too.  Both passes of both kernels therefore see the same contributing samples with
//        the same fp32 values, and S, P_i, v_i, dL/dsigma_s and dL/dc -- fp64 in VG's brackets -- are the same bits.
//   (G2) THE SAME INTEGERS, ROW BY ROW.  For a contributing sample and a corner c at the point p_c both kernels form the same
//        q = vol_fix((tw_c Y_m) dL/dc) and vol_fix(tw_c dL/dsigma_s).  VG adds them to the words of p_c; VCG adds them to the words of
//        row slot[p_c] when that lies in [0, n) and drops them otherwise.  index[r] = p exactly when slot[p] = r, so row r receives
//        what the point index[r] receives, contribution for contribution; integer sums do not depend on the order.  (A) for VCG.
//   (G3) INSIDE THE LIST.  For C = pack(V): by (C3) and (C4) V and U = unpack(C) have the same contributing samples with the same
//        values, and all eight corners of a contributing sample's cell are active.  So VG on V adds only to points of the list, adds
//        there what VG on U adds, and by (G2) what VCG on C adds to their rows; no contribution is dropped.  This is (B).
//   (U1) THE UPDATE.  k_volume_compact_adam is k_volume_adam with the point p replaced by the row r: the word (r, wd) has the
//        parameter, the accumulator and the moments that VU's word (index[r], wd) has in U, and the expressions are the same.  By
//        (A) the accumulators agree at entry, so x', m' and v' agree, a dead sigma is left alone alike and the accumulator is zeroed.
//   (T1) THE PRIOR.  A point is a member iff its slot lies in [0, n), which is member_mask(index).  A row whose point[r] is outside
//        the lattice, not a member, or a member whose slot is not r is skipped; with point = index none of the rows is.  The thread
//        of (r, wd) at q = point[r] forms rule VT's terms with a neighbour's value read through that neighbour's slot, U's word
//        there: the same fp64 d_a, tau and Q_a as k_volume_tv's thread of (q, wd), summed as integers into the word of row r.  (A) for VCT.
// From integer sums: the compact accumulators are identical for the same call twice, for permuted rays, for a split batch and for
// every block edge.  Every index that becomes an address is clamped (cell, block) or compared with its array's size first (a slot
// against n, point[r] against the lattice, a neighbour's coordinate against the lattice before its slot is read).
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

namespace {

// volc_color before its clamp (the same expressions: the clamped colour is fminf(fmaxf(raw, 0), 1) of it, bit for bit)
template <int NC>
__device__ inline void volc_color_raw(const float* __restrict__ rows, const int (&r)[8], const float (&f)[3], const float (&Y)[9],
                                      float (&raw)[3]) {
  float v[3][8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float q[NC * 3];
    volc_row<NC>(rows, r[c], q);
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

struct VolcRay {
  float o[3], d[3], ta;
  int K;  // 0 for a miss
  float Y[9];
};

// a contributing sample, as the forward computes it
struct VolcHit {
  int row[8];  // the corners' rows, -1 where a corner has none
  float f[3], tk, w, Tn, c[3];
  bool pass[3];  // the unclamped colour lies in [0, 1]
};

// one iteration of k_volume_compact_march's loop at sample k: k moves on, T is updated; true when the sample contributes (h is then
// filled); done is set where the forward breaks (T < t_stop)
template <int NC>
__device__ inline bool volc_step(const VolCompactGradArgs& ca, const VolcRay& ry, int& k, float& T, bool& done, VolcHit& h) {
  const VolRenderArgs& a = ca.r;
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
      int row[8];
      vol_corners(a.g, ci, p);
      volc_rows(ca.c, p, row);
      const float s = volc_sigma(ca.c.sigma_rows, row, f);
      if (s > 0.0f) {
        float raw[3];
        volc_color_raw<NC>(static_cast<const float*>(ca.c.coef_rows), row, f, ry.Y, raw);
        const float alpha = -expm1f(-(s * a.dt));
        const float w = T * alpha;
        T = T - w;
        h.tk = tk;
        h.w = w;
        h.Tn = T;
#pragma unroll
        for (int c = 0; c < 8; ++c) h.row[c] = row[c];
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
__device__ inline double volc_v(const VolcHit& h, const float (&g)[3], double gD, double gA1) {
  return ((((double)g[0] * (double)h.c[0] + (double)g[1] * (double)h.c[1]) + (double)g[2] * (double)h.c[2]) + gD * (double)h.tk) + gA1;
}

// a value of lane src (wave-uniform) in every lane
__device__ inline int lane_value(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ inline float lane_value(float x, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src)); }
__device__ inline double lane_value(double x, int src) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the row of the member p, -1 where p is none: a slot is compared with n before anything is read through it
__device__ inline int volc_member(const VolCompact& c, long long p) {
  const int s = c.slot[p];
  return (s >= 0 && (long long)s < c.n) ? s : -1;
}

// the values of one word over the rows: x(r) = base[r * stride]
struct VolcWord {
  const float* base;
  long long stride;
};

// rule VT at the member (i, j, k) with the linear index lin and the row r: Q_x, Q_y, Q_z of this word
__device__ inline void volc_tv_terms(const VolCompactTvArgs& a, const VolcWord& x, int i, int j, int k, long long lin, int r, double w,
                                     long long (&Q)[3]) {
  const long long sy = a.nz, sx = (long long)a.ny * a.nz;
  const double x0 = (double)x.base[(long long)r * x.stride];
  double d[3] = {0.0, 0.0, 0.0};
  if (i + 1 < a.nx) {
    const int s = volc_member(a.c, lin + sx);
    if (s >= 0) d[0] = (double)x.base[(long long)s * x.stride] - x0;
  }
  if (j + 1 < a.ny) {
    const int s = volc_member(a.c, lin + sy);
    if (s >= 0) d[1] = (double)x.base[(long long)s * x.stride] - x0;
  }
  if (k + 1 < a.nz) {
    const int s = volc_member(a.c, lin + 1);
    if (s >= 0) d[2] = (double)x.base[(long long)s * x.stride] - x0;
  }
  const double tau = sqrt((((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) + a.eps);
#pragma unroll
  for (int c = 0; c < 3; ++c) Q[c] = vol_fix(w * (d[c] / tau));
}

}  // namespace

// grid = ceil(N / VOL_MARCH_WG): one ray per lane, one wave per workgroup
template <int NC>
__global__ __launch_bounds__(VOL_MARCH_WG) void k_volume_compact_march_grad(const VolCompactGradArgs ga) {
  static_assert(VOL_MARCH_WG == 64, "the scatter walks one wave's ballot");
  constexpr int ROW = 3 * NC;                          // int64 words of a row's coefficient accumulators
  constexpr int CPI = NC == 9 ? 2 : (NC == 4 ? 4 : 8);  // corners per scatter instruction
  static_assert(CPI * ROW + 8 <= 64, "the coefficient lanes and the eight sigma lanes of one instruction");
  const VolRenderArgs& a = ga.r;
  const int lane = threadIdx.x;
  const long long r = (long long)blockIdx.x * VOL_MARCH_WG + lane;
  const int dim[3] = {a.g.nx, a.g.ny, a.g.nz};

  // ---- this lane's ray (a lane past N holds a miss) ----
  VolcRay ry;
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
    VolcHit h;
#pragma unroll 1
    while (k < ry.K && !done)
      if (volc_step<NC>(ga, ry, k, T, done, h)) S = S + (double)h.w * volc_v(h, g, gD, gA1);
  }

  // ---- this lane's words in a scatter instruction ----
  const int slot = lane / ROW, word = lane - slot * ROW;  // corner slot (< CPI for a coefficient lane) and the word of its row
  const int wm = word / 3, wch = word - wm * 3;
  const bool coef_lane = lane < CPI * ROW;
  const int sc = lane - CPI * ROW;                         // the corner of a sigma lane
  const bool sigma_lane = sc >= 0 && sc < 8;

  // ---- pass 2: the march again, the wave scatters ----
  int k = 0;
  float T = 1.0f;
  bool done = false;
  double P = 0.0;
#pragma unroll 1
  while (true) {
    const bool active = k < ry.K && !done;
    if (__ballot(active) == 0ull) break;
    VolcHit h;
    h.tk = h.w = h.Tn = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) h.row[c] = -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) h.f[c] = h.c[c] = 0.0f, h.pass[c] = false;
    bool has = false;
    double ds = 0.0, dc0 = 0.0, dc1 = 0.0, dc2 = 0.0;
    if (active && volc_step<NC>(ga, ry, k, T, done, h)) {
      has = true;
      const double v = volc_v(h, g, gD, gA1);
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
      int rb[8];  // the source lane's eight rows: scalars
#pragma unroll
      for (int c = 0; c < 8; ++c) rb[c] = lane_value(h.row[c], src);
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
        int row = -1;  // the row of corner c: a lane that is neither kind (c >= 8) keeps none
#pragma unroll
        for (int j = 0; j < 8; ++j) row = c == j ? rb[j] : row;
        if (row >= 0) {
          if (coef_lane) {
            const long long q = vol_fix((tw * ym) * e);
            if (q != 0) agent_add(ga.acc_coef_rows + (long long)row * ROW + word, q);
          } else if (it == 0 && sigma_lane) {
            const long long q = vol_fix(tw * es);
            if (q != 0) agent_add(ga.acc_sigma_rows + row, q);
          }
        }
      }
    }
  }
}

// grid = ceil(n (1 + 3 ncoef) / VOL_WG): one thread per (row, word) -- k_volume_adam with the rows as the list
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_adam(const VolCompactAdamArgs a) {
  const long long W = 1 + 3 * (long long)a.ncoef;
  const long long i = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (i >= a.n * W) return;
  const long long r = i / W;
  const int wd = (int)(i - r * W);
  float* xp = wd == 0 ? a.sigma_rows + r : a.coef_rows + r * (W - 1) + (wd - 1);
  long long* ap = wd == 0 ? a.acc_sigma_rows + r : a.acc_coef_rows + r * (W - 1) + (wd - 1);
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

// grid = ceil(n (1 + 3 ncoef) / VOL_WG): one thread per (row, word), the word fastest -- k_volume_tv with the slot lattice as the
// membership test.  The word of row r is read and written by this thread alone: a plain read-modify-write.
__global__ __launch_bounds__(VOL_WG) void k_volume_compact_tv(const VolCompactTvArgs a) {
  const long long W = 1 + 3 * (long long)a.ncoef;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.c.n * W) return;
  const long long r = t / W;
  const int wd = (int)(t - r * W);
  const long long npts = (long long)a.nx * a.ny * a.nz;
  const long long q = a.point[r];
  if (q < 0 || q >= npts) return;       // a row without a point: never used as an address
  if (volc_member(a.c, q) != r) return;  // not a member, or not this row's point: the row receives nothing
  const double w = wd == 0 ? a.w_sigma : a.w_coef;
  if (!(w > 0.0)) return;               // every term of this word is 0
  const int k = (int)(q % a.nz);
  const long long ij = q / a.nz;
  const int j = (int)(ij % a.ny), i = (int)(ij / a.ny);
  const long long sy = a.nz, sx = (long long)a.ny * a.nz;
  VolcWord x;
  x.base = wd == 0 ? a.c.sigma_rows : static_cast<const float*>(a.c.coef_rows) + (wd - 1);
  x.stride = wd == 0 ? 1 : W - 1;

  long long Q[3];
  volc_tv_terms(a, x, i, j, k, q, (int)r, w, Q);
  long long sum = -Q[0] - Q[1] - Q[2];
  if (i > 0) {
    const int s = volc_member(a.c, q - sx);
    if (s >= 0) {
      volc_tv_terms(a, x, i - 1, j, k, q - sx, s, w, Q);
      sum += Q[0];
    }
  }
  if (j > 0) {
    const int s = volc_member(a.c, q - sy);
    if (s >= 0) {
      volc_tv_terms(a, x, i, j - 1, k, q - sy, s, w, Q);
      sum += Q[1];
    }
  }
  if (k > 0) {
    const int s = volc_member(a.c, q - 1);
    if (s >= 0) {
      volc_tv_terms(a, x, i, j, k - 1, q - 1, s, w, Q);
      sum += Q[2];
    }
  }
  long long* ap = wd == 0 ? a.acc_sigma_rows + r : a.acc_coef_rows + r * (W - 1) + (wd - 1);
  if (sum != 0) *ap = (long long)((unsigned long long)*ap + (unsigned long long)sum);
}

hipError_t launch_volume_compact_render_backward(const VolCompactGradArgs& a, int ncoef, hipStream_t st) {
  if (a.r.N <= 0 || a.c.n <= 0) return hipSuccess;  // without rows no sample contributes
  const dim3 g(grid(a.r.N, VOL_MARCH_WG)), b(VOL_MARCH_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_compact_march_grad<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_compact_march_grad<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_compact_march_grad<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_compact_adam_step(const VolCompactAdamArgs& a, hipStream_t st) {
  if (a.n > 0) LAUNCH(k_volume_compact_adam, dim3(grid(a.n * (1 + 3 * (long long)a.ncoef), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_compact_tv_backward(const VolCompactTvArgs& a, hipStream_t st) {
  if (a.c.n > 0) LAUNCH(k_volume_compact_tv, dim3(grid(a.c.n * (1 + 3 * (long long)a.ncoef), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
