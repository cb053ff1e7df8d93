// mesh_raycast.hip -- rays against an indexed triangle mesh over a uniform grid of triangles, the shadow rays of face visibility and
// the selection of faces (nerf_hip_mesh_raycast_grid_count / _grid_fill, nerf_hip_mesh_raycast, nerf_hip_mesh_face_rays,
// nerf_hip_mesh_select_faces_count / _emit; the definitions are in include/nerf_hip.h).
//   k_rc_count       per face: does it take part, is it INSIDE, the cells of its box; summed per wave, then three integer atomics
//   k_rc_cells       per INSIDE face: its box's cells counted by integer atomics (PLACE: the face entered through the cells' cursors)
//   scan.h's cells_to_start   per-cell counts -> start[cell], the exclusive scan; the counts are zeroed for the cursors
//   scan.h's compaction over OutsideFlag   the OUTSIDE faces, ascending, and their number
//   k_rc_cast        per ray: the OUTSIDE list in full, then the grid walk below
//   k_rc_face_rays   per face: centroid, facing and in-view tests, the shadow ray towards the camera
//   k_sel_mark + scan.h's compaction over UsedFlag / KeepFlag   the vertices of the kept faces, then the kept faces, in their order
//
// THE HIT RULE (R in include/nerf_hip.h) is Moeller-Trumbore in fp64 with one more condition: the computed point h = o + t d lies in
// the face's box widened by e = 2^-20 max |coordinate|.  It is no watertight test: a ray through a shared edge can miss both
// neighbours.  rc_hit is the rule; everything else here only decides WHICH faces it is asked about.
//
// THE GRID WALK.  Claim: for every grid (lo, cell, dims) the walk asks rc_hit about every face whose hit can be the ray's answer, so
// the result is the brute-force minimum over all faces with the lowest face index among ties.
//   (W1) MONOTONE.  For a fixed ray and axis k, t -> h_k(t) = fl(o_k + fl(t d_k)) is monotone in t (rounding is monotone; the direction
//        of the monotonicity is the sign of d_k), and x -> cellidx_k(x) = floor(fl(fl(x - lo_k) / cell)) is monotone non-decreasing.  So
//        c_k(t) = cellidx_k(h_k(t)) is monotone in t, and for t in [ta, tb] c_k(t) lies between c_k(ta) and c_k(tb).
//   (W2) A HIT IS IN ITS FACE'S BOX.  An accepted hit of face f at t has min_k - e <= h_k(t) <= max_k + e on every axis (R's last
//        condition), with h_k(t) the very number the walk computes -- the same expression on the same operands.  By (W1) c_k(t) lies in
//        [cellidx_k(min_k - e), cellidx_k(max_k + e)], the face's own index box.  An INSIDE face is entered in every cell of its box, so it
//        is entered in the cell (c_x(t), c_y(t), c_z(t)), and that cell is a cell of the grid.
//   (W3) INTERVALS.  The walk takes breakpoints t_0 <= t_1 <= ... <= t_n = thi (any non-decreasing numbers: only the speed depends on
//        them) and on [t_i, t_i+1] tests the entries of every grid cell of the per-axis box between c(t_i) and c(t_i+1).  By (W1) and (W2)
//        every accepted hit of an INSIDE face with t in that interval is among them.  The walk stops after an interval when
//        best < t_i+1 STRICTLY: every hit not yet met has t >= t_i+1 > best, so it can neither win nor tie.  It also stops when c_m(t_i+1)
//        on the major axis m lies beyond the grid in the direction of travel: by (W1) it stays beyond for every later t, and by (W2) no
//        INSIDE face is hit there.
//   (W4) THE START.  t_0 = tlo = max(tmin, -DBL_MAX) (a hit has a finite t: at t = +-inf a coordinate of h is not finite and fails R's last
//        condition), unless a later ts is VERIFIED, by computing it, to have c_m(ts) before the grid against the direction of travel;
//        then by (W1) every t < ts is before the grid as well and the walk starts at ts.  ts is the entry plane's t less a margin; the
//        margin is a guess for speed, the verification is what the proof uses.
//   (W5) OUTSIDE faces are tested by every ray in full, faces that take no part by none (R: they are never hit).
//   (W6) TERMINATION.  Each interval advances the plane index j by one along the major axis; once j has left [0, dims_m) the next
//        breakpoint is thi and the walk ends: at most dims_m + 2 intervals.
// A face may be tested more than once (it lies in several cells); the minimum with the lowest-index tie rule does not notice.  The
// order of the entries inside a cell depends on the interleaving of the cursor atomics; no output does.  There is no float atomic.
// Every index read from memory -- a face's corner, a cell's bounds, an entry, a skip -- is checked before it is used as an address,
// and every store is clamped to the caller's capacity.
#include "scan.h"

namespace nerf {

namespace {

constexpr double RC_INF = __builtin_huge_val();
constexpr double RC_MAX = 1.7976931348623157e308;   // DBL_MAX
constexpr double RC_EPS = 9.5367431640625e-07;      // 2^-20: the box margin of the hit rule
constexpr double RC_SKIP = 9.094947017729282e-13;   // 2^-40: the margin of (W4)'s guess (speed only)

// does face f take part (corners in range with finite coordinates; they need not be distinct)?  -> the coordinates in p[corner][axis]
__device__ inline bool rc_face(const float* verts, const int* faces, int V, long long f, float (&p)[3][3]) {
  return face_coords<false>(verts, faces, V, f, p);
}

// the face's box widened by e: mn[k] = min_k - e, mx[k] = max_k + e
__device__ inline void rc_bounds(const float (&p)[3][3], double (&mn)[3], double (&mx)[3]) {
  float big = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) big = fmaxf(big, fabsf(p[c][d]));
  const double e = RC_EPS * (double)big;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    mn[d] = (double)fminf(fminf(p[0][d], p[1][d]), p[2][d]) - e;
    mx[d] = (double)fmaxf(fmaxf(p[0][d], p[1][d]), p[2][d]) + e;
  }
}

struct RcBest {
  double t, u, v;
  int face, side;
};

// THE HIT RULE for one face that takes part, against the ray (o, d) and the window [tmin, tmax]; a hit updates best
__device__ inline void rc_hit(const float (&p)[3][3], int f, const double (&o)[3], const double (&d)[3], double tmin, double tmax, RcBest& best) {
  double A[3], e1[3], e2[3], s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    A[k] = (double)p[0][k];
    e1[k] = (double)p[1][k] - A[k];
    e2[k] = (double)p[2][k] - A[k];
    s[k] = o[k] - A[k];
  }
  const double P[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
  const double det = (e1[0] * P[0] + e1[1] * P[1]) + e1[2] * P[2];
  if (!(det != 0.0)) return;
  const double q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
  const double u = ((s[0] * P[0] + s[1] * P[1]) + s[2] * P[2]) / det;
  const double v = ((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]) / det;
  const double t = ((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2]) / det;
  if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0 && tmin <= t && t <= tmax)) return;
  double mn[3], mx[3];
  rc_bounds(p, mn, mx);
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double h = o[k] + t * d[k];
    in = in && mn[k] <= h && h <= mx[k];
  }
  if (!in) return;
  if (best.face < 0 || t < best.t || (t == best.t && f < best.face)) {
    best.t = t;
    best.u = u;
    best.v = v;
    best.face = f;
    best.side = det > 0.0 ? 1 : -1;
  }
}

__device__ inline double rc_cellidx(double x, float lo, float cell) { return floor((x - (double)lo) / (double)cell); }

// the index box of a face that takes part -> is it INSIDE?  (b0, b1: its cells, set only when it is)
__device__ inline bool rc_box(const RcGridArgs& g, const float (&p)[3][3], int (&b0)[3], int (&b1)[3]) {
  double mn[3], mx[3];
  rc_bounds(p, mn, mx);
  bool inside = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double lo = rc_cellidx(mn[d], g.lo[d], g.cell), hi = rc_cellidx(mx[d], g.lo[d], g.cell);
    const bool ok = lo >= 0.0 && hi <= (double)(g.dims[d] - 1) && lo <= hi;
    inside = inside && ok;
    b0[d] = ok ? (int)lo : 0;
    b1[d] = ok ? (int)hi : -1;
  }
  return inside;
}

__device__ inline double rc_sel(int m, double a0, double a1, double a2) { return m == 0 ? a0 : (m == 1 ? a1 : a2); }

}  // namespace

// ---- the grid ----

// grid = ceil(F / CC_WG), whole waves, one thread per face
__global__ __launch_bounds__(CC_WG) void k_rc_count(const RcGridArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  long long t[3] = {0, 0, 0};
  float p[3][3];
  if (f < a.F && rc_face(a.verts, a.faces, a.V, f, p)) {
    int b0[3], b1[3];
    t[0] = 1;
    if (rc_box(a, p, b0, b1)) t[1] = ((long long)(b1[0] - b0[0] + 1) * (b1[1] - b0[1] + 1)) * (b1[2] - b0[2] + 1);  // (<= ncell < 2^31)
    else t[2] = 1;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long s = wave_sum(t[k]);
    if ((threadIdx.x & 63) == 0 && s != 0) agent_add(&a.counts[k], s);
  }
}

// grid = ceil(F / CC_WG), one thread per face.  PLACE: which entry of a cell a face gets depends on the interleaving; the cell's set
// of entries does not.
template <bool PLACE>
__global__ __launch_bounds__(CC_WG) void k_rc_cells(const RcGridArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  float p[3][3];
  if (f >= a.F || !rc_face(a.verts, a.faces, a.V, f, p)) return;
  int b0[3], b1[3];
  if (!rc_box(a, p, b0, b1)) return;
  for (int x = b0[0]; x <= b1[0]; ++x)
    for (int y = b0[1]; y <= b1[1]; ++y)
      for (int z = b0[2]; z <= b1[2]; ++z) {
        const long long c = ((long long)x * a.dims[1] + y) * a.dims[2] + z;  // (inside the grid: rc_box)
        if (!PLACE) {
          agent_add(&a.cnt[c], 1);
        } else {
          const long long b = a.start[c], e = a.start[c + 1];
          const long long at = b + (long long)agent_add(&a.cnt[c], 1);
          if (b >= 0 && at >= b && at < e && e <= a.cap_entries) a.entries[at] = (int)f;
        }
      }
}

namespace {

// the flag and sink of the OUTSIDE list.  k_flag_place recomputes the flags: no launch between the count and the placement writes
// the vertices or the faces
struct OutsideFlag {
  RcGridArgs a;
  __device__ int operator()(long long f) const {
    float p[3][3];
    int b0[3], b1[3];
    return rc_face(a.verts, a.faces, a.V, f, p) && !rc_box(a, p, b0, b1);
  }
};
struct OutsideSink {
  int* outside;
  long long F;
  __device__ void operator()(long long f, int flag, long long pos) const {
    if (flag && pos < F) outside[pos] = (int)f;
  }
};

// the entries of one cell against the ray
__device__ inline void rc_cell(const RcCastArgs& a, long long c, int skip, const double (&o)[3], const double (&d)[3], RcBest& best) {
  long long b = a.g.start[c], e = a.g.start[c + 1];
  if (b < 0 || e < b || e > a.g.cap_entries) b = e = 0;
  for (long long k = b; k < e; ++k) {
    const int f = a.g.entries[k];
    float p[3][3];
    if ((unsigned)f >= (unsigned)a.g.F || f == skip || !rc_face(a.g.verts, a.g.faces, a.g.V, f, p)) continue;
    rc_hit(p, f, o, d, a.tmin, a.tmax, best);
  }
}

}  // namespace

// ---- the cast ----

// grid = ceil(min(N, cap_n) / CC_WG), one ray per lane.  ANY: the walk stops at the first hit and only `occluded` is stored.
template <bool ANY>
__global__ __launch_bounds__(CC_WG) void k_rc_cast(const RcCastArgs a) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (i >= a.N || i >= a.cap_n) return;
  const RcGridArgs& g = a.g;
  const float fo[3] = {a.orig[i * 3 + 0], a.orig[i * 3 + 1], a.orig[i * 3 + 2]};
  const float fd[3] = {a.dir[i * 3 + 0], a.dir[i * 3 + 1], a.dir[i * 3 + 2]};
  RcBest best = {RC_INF, 0.0, 0.0, -1, 0};
  const bool part = isfinite(fo[0]) && isfinite(fo[1]) && isfinite(fo[2]) && isfinite(fd[0]) && isfinite(fd[1]) && isfinite(fd[2]) &&
                    (fd[0] != 0.0f || fd[1] != 0.0f || fd[2] != 0.0f);
  const double tlo = fmax(a.tmin, -RC_MAX), thi = fmin(a.tmax, RC_MAX);  // (W4)
  if (part && tlo <= thi) {
    const double o[3] = {(double)fo[0], (double)fo[1], (double)fo[2]}, d[3] = {(double)fd[0], (double)fd[1], (double)fd[2]};
    const int skip = a.skip ? a.skip[i] : -1;
    // (W5) the OUTSIDE faces
    long long no = g.info[1];
    no = no < 0 ? 0 : (no > g.F ? g.F : no);
    for (long long k = 0; k < no && !(ANY && best.face >= 0); ++k) {
      const int f = g.outside[k];
      float p[3][3];
      if ((unsigned)f >= (unsigned)g.F || f == skip || !rc_face(g.verts, g.faces, g.V, f, p)) continue;
      rc_hit(p, f, o, d, a.tmin, a.tmax, best);
    }
    // the major axis: the largest |d_k|, the lowest axis among equals
    const double ad[3] = {fabs(d[0]), fabs(d[1]), fabs(d[2])};
    const int m = ad[0] >= ad[1] ? (ad[0] >= ad[2] ? 0 : 2) : (ad[1] >= ad[2] ? 1 : 2);
    const double om = rc_sel(m, o[0], o[1], o[2]), dm = rc_sel(m, d[0], d[1], d[2]);
    const double lom = rc_sel(m, (double)g.lo[0], (double)g.lo[1], (double)g.lo[2]), cell = (double)g.cell;
    const double nm = rc_sel(m, (double)g.dims[0], (double)g.dims[1], (double)g.dims[2]);
    const bool fwd = dm > 0.0;
    bool go = !(ANY && best.face >= 0);
    double tc = tlo;
    {  // (W4) skip what lies before the grid, when that can be verified
      const double plane = fwd ? lom : lom + nm * cell;
      const double te = (plane - om) / dm;
      const double ts = (te - ((fabs(om) + fabs(plane)) * RC_SKIP) / fabs(dm)) - fabs(te) * RC_SKIP;
      if (ts > tc) {
        const double cs = rc_cellidx(om + ts * dm, (float)lom, g.cell);
        if (fwd ? cs < 0.0 : cs > nm - 1.0) {
          if (ts >= thi) go = false;  // the whole window lies before the grid
          else tc = ts;
        }
      }
    }
    if (go) {
      double cc[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) cc[k] = rc_cellidx(o[k] + tc * d[k], g.lo[k], g.cell);
      const double cm = rc_sel(m, cc[0], cc[1], cc[2]);
      if (fwd ? cm > nm - 1.0 : cm < 0.0) go = false;  // (W3) already beyond the grid
      long long j = (long long)fmin(fmax(cm, 0.0), nm - 1.0);
      int q0[3] = {0, 0, 0}, q1[3] = {-1, -1, -1};  // the box of the interval before (empty)
      while (go) {
        double tn = thi;  // (W6)
        if (j >= 0 && (double)j <= nm - 1.0) {
          const double plane = lom + (double)(fwd ? j + 1 : j) * cell;
          tn = fmin(fmax((plane - om) / dm, tc), thi);
        }
        double cn[3];
        int x0[3], x1[3];
        bool any = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          cn[k] = rc_cellidx(o[k] + tn * d[k], g.lo[k], g.cell);
          const double lo = fmin(cc[k], cn[k]), hi = fmax(cc[k], cn[k]), top = (double)(g.dims[k] - 1);
          any = any && hi >= 0.0 && lo <= top;
          x0[k] = (int)fmin(fmax(lo, 0.0), top);
          x1[k] = (int)fmin(fmax(hi, 0.0), top);
        }
        if (any) {
          for (int x = x0[0]; x <= x1[0]; ++x)
            for (int y = x0[1]; y <= x1[1]; ++y)
              for (int z = x0[2]; z <= x1[2]; ++z) {
                if (x >= q0[0] && x <= q1[0] && y >= q0[1] && y <= q1[1] && z >= q0[2] && z <= q1[2]) continue;  // tested one interval ago
                rc_cell(a, ((long long)x * g.dims[1] + y) * g.dims[2] + z, skip, o, d, best);
              }
#pragma unroll
          for (int k = 0; k < 3; ++k) q0[k] = x0[k], q1[k] = x1[k];
        } else {
          q1[0] = -1;
        }
        const double cnm = rc_sel(m, cn[0], cn[1], cn[2]);
        if ((ANY && best.face >= 0) || best.t < tn || tn >= thi || (fwd ? cnm > nm - 1.0 : cnm < 0.0)) break;  // (W3)
        tc = tn;
#pragma unroll
        for (int k = 0; k < 3; ++k) cc[k] = cn[k];
        j += fwd ? 1 : -1;
      }
    }
  }
  if (ANY) {
    a.occluded[i] = best.face >= 0 ? 1 : 0;
  } else {
    a.t[i] = best.t;
    a.uv[i * 2 + 0] = best.u;
    a.uv[i * 2 + 1] = best.v;
    a.face[i] = best.face;
    a.side[i] = (signed char)best.side;
  }
}

// ---- face visibility: the shadow rays of one camera ----

// grid = ceil(min(F, cap_f) / CC_WG), one thread per face
__global__ __launch_bounds__(CC_WG) void k_rc_face_rays(const RcFaceRaysArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (f >= a.F || f >= a.cap_f) return;
  float p[3][3], og[3] = {0.0f, 0.0f, 0.0f}, dr[3] = {0.0f, 0.0f, 0.0f};
  bool valid = false;
  if (rc_face(a.verts, a.faces, a.V, f, p)) {
    double A[3], e1[3], e2[3], G[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      A[k] = (double)p[0][k];
      e1[k] = (double)p[1][k] - A[k];
      e2[k] = (double)p[2][k] - A[k];
      G[k] = ((A[k] + (double)p[1][k]) + (double)p[2][k]) / 3.0;
      w[k] = (double)a.cam[k] - G[k];
      og[k] = (float)G[k];
    }
    const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const bool facing = (N[0] * w[0] + N[1] * w[1]) + N[2] * w[2] > 0.0;
    const double na = -w[0], nb = -w[1], nc = -w[2];
    double mm[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) mm[r] = (a.Q[r * 3 + 0] * na + a.Q[r * 3 + 1] * nb) + a.Q[r * 3 + 2] * nc;
    const double x = mm[0] / mm[2], y = mm[1] / mm[2];
    const bool view = mm[2] > 0.0 && -0.5 <= x && x < (double)a.H - 0.5 && -0.5 <= y && y < (double)a.W - 0.5;
    valid = facing && view;
    if (valid)
#pragma unroll
      for (int k = 0; k < 3; ++k) dr[k] = (float)((double)a.cam[k] - (double)og[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.orig[f * 3 + k] = og[k];
    a.dir[f * 3 + k] = dr[k];
  }
  a.valid[f] = valid ? 1 : 0;
}

// ---- face selection ----

namespace {

// -> the kept face's corners in i[3]
__device__ inline bool sel_face_kept(const SelArgs& a, long long f, int (&i)[3]) {
  return a.keep[f] != 0 && face_corners<false>(a.faces, a.V, f, i);
}

// the flags of the two compactions (the sinks are mesh_parts.h's).  k_flag_place recomputes the flags: `used` is written by k_sel_mark
// alone, before both
struct UsedFlag {
  const int* used;
  __device__ int operator()(long long v) const { return used[v] != 0; }
};
struct KeepFlag {
  SelArgs a;
  __device__ int operator()(long long f) const {
    int i[3];
    return sel_face_kept(a, f, i);
  }
};

}  // namespace

// grid = ceil(F / CC_WG): used[v] = 1 for the corners of the kept faces (every writer stores the same 1)
__global__ __launch_bounds__(CC_WG) void k_sel_mark(const SelArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  int i[3];
  if (f >= a.F || !sel_face_kept(a, f, i)) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.used[i[d]] = 1;
}

// ---- launchers ----

hipError_t launch_rc_grid_count(const RcGridArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 3 * sizeof(long long), st));
  if (a.F > 0 && a.V > 0) LAUNCH(k_rc_count, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_rc_grid_fill(const RcGridArgs& a, hipStream_t st) {
  const bool faces = a.F > 0 && a.V > 0;
  TRY(hipMemsetAsync(a.cnt, 0, (size_t)a.ncell * sizeof(int), st));
  TRY(hipMemsetAsync(a.info, 0, 2 * sizeof(long long), st));
  if (faces) LAUNCH(k_rc_cells<false>, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  TRY(cells_to_start(a.cnt, a.ncell, a.cap_entries, a.tot, a.base, a.start, a.info, nullptr, st));
  if (faces) {
    LAUNCH(k_rc_cells<true>, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
    TRY(scan_place(OutsideFlag{a}, OutsideSink{a.outside, a.F}, a.F, a.tot, a.base, a.info + 1, st));
  }
  return hipSuccess;
}

hipError_t launch_rc_cast(const RcCastArgs& a, bool any_hit, hipStream_t st) {
  const long long n = a.N < a.cap_n ? a.N : a.cap_n;
  if (n <= 0) return hipSuccess;
  if (any_hit) LAUNCH(k_rc_cast<true>, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  else LAUNCH(k_rc_cast<false>, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_rc_face_rays(const RcFaceRaysArgs& a, hipStream_t st) {
  const long long n = a.F < a.cap_f ? a.F : a.cap_f;
  if (n > 0) LAUNCH(k_rc_face_rays, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

namespace {

hipError_t sel_mark(const SelArgs& a, hipStream_t st) {
  if (a.V > 0) TRY(hipMemsetAsync(a.used, 0, (size_t)a.V * sizeof(int), st));
  if (a.F > 0 && a.V > 0) LAUNCH(k_sel_mark, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace

hipError_t launch_sel_count(const SelArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 2 * sizeof(long long), st));
  TRY(sel_mark(a, st));
  if (a.V > 0) TRY(scan_count(UsedFlag{a.used}, a.V, a.tot, a.base, a.counts, st));
  if (a.F > 0 && a.V > 0) TRY(scan_count(KeepFlag{a}, a.F, a.tot, a.base, a.counts + 1, st));
  return hipSuccess;
}

hipError_t launch_sel_emit(const SelArgs& a, hipStream_t st) {
  TRY(sel_mark(a, st));
  if (a.V > 0)
    TRY(scan_place(UsedFlag{a.used}, SubVertSink{a.verts, a.normals, a.rgb, a.out_verts, a.out_normals, a.out_rgb, a.newidx, a.max_v},
                   a.V, a.tot, a.base, a.counts, st));
  if (a.F > 0 && a.V > 0)  // (after the vertices' placement: the faces read newidx across workgroups)
    TRY(scan_place(KeepFlag{a}, SubFaceSink{a.faces, a.newidx, a.out_faces, a.max_f}, a.F, a.tot, a.base, a.counts + 1, st));
  return hipSuccess;
}

}  // namespace nerf
