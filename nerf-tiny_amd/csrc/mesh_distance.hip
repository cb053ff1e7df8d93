// mesh_distance.hip -- geometry evaluation of indexed triangle meshes and point clouds: measures, area-weighted surface samples, exact
// nearest points over a uniform grid and distance statistics (nerf_hip_mesh_measure, nerf_hip_mesh_sample, nerf_hip_points_grid_build,
// nerf_hip_points_nearest, nerf_hip_distance_stats; the definitions are in include/nerf_hip.h).
//   k_md_measure     per face: area, six volumes and centroid moments as int64 fixed point, summed per wave, then five integer atomics
//   scan.h's value scan over FaceWeight   per face: cum[f] = the inclusive prefix of the integer weights, the grand total W into info
//   k_md_sample      per sample: stratum -> face by binary search in cum -> folded barycentrics -> point
//   k_pn_count       per point: its cell's count by an integer atomic (reference points and queries alike)
//   scan.h's cells_to_start   per-cell counts -> start[cell], the exclusive scan; the counts are zeroed for the cursors
//   k_pn_place       per point: its record (x, y, z, index) placed through its cell's cursor atomic
//   k_pn_fill        per query: idx = -1, dist2 = +inf
//   k_pn_query       per query: Chebyshev shells of cells around its own cell until the stopping rule holds
//   k_md_stats       per distance: counts and fixed-point sums, summed per wave, then integer atomics
//
// THE NEAREST-POINT SEARCH.  cell(p) along an axis is k(p) = floor(fl(fl(p - lo) / cell)) in fp64 on the fp32-widened operands, clamped
// to [0, dims - 1].  fl() is monotone, so k is monotone non-decreasing in p.  A query at true position q (any finite position, inside
// the box or far outside it) starts in c = its own clamped cell and after shell r has examined every point whose cell lies in the block
// [c - r, c + r], clipped to the grid.
//   (N1) THE BOUND.  A point p not yet examined has a cell outside the block along at least one axis d, and that cell is inside the
//        grid: so it lies beyond a face of the block that is NOT a face of the grid, either low (L = c_d - r >= 1 and k(p_d) < L)
//        or high (H = c_d + r + 1 <= dims_d - 1 and k(p_d) >= H; the clamp at dims_d - 1 only moves points to cells below H or keeps them
//        at or above it).  k(p_d) < L gives fl(fl(p_d - lo_d) / cell) < L, hence in real arithmetic p_d < lo_d + L cell (1 + 3 eps),
//        eps = 2^-53; k(p_d) >= H gives p_d >= lo_d + H cell (1 - 3 eps).  So |q_d - p_d| >= q_d - lo_d - L cell (1 + 3 eps), or
//        >= lo_d + H cell (1 - 3 eps) - q_d.  Neither inequality asks where q lies: a query outside the box has c_d clamped to 0 or
//        dims_d - 1, the face on its own side IS a face of the grid and is never used, and the gap to the face on the other side only
//        grows.  A gap that comes out <= 0 is taken as 0 and never stops the walk.
//   (N2) THE MARGIN.  The kernel computes A = fl(L cell), P = fl(lo_d + A), b = fl(q_d - P) (or fl(P - q_d)), S = |q_d| + |lo_d| + A and
//        g = b - 2^-45 S.  Every rounding above and the 3 eps L cell of (N1) are each at most eps (1 + eps)^3 S, fewer than 16 of them:
//        together below 2^-49 S, while the margin is 2^-45 S.  So g <= the real gap <= |q_d - p_d|, g is an fp64 number, and by
//        monotonicity the computed difference fl(q_d - p_d) is at least g in magnitude; the computed d2(q, p) = fl(fl(dx dx + dy dy) +
//        dz dz) >= fl(g g), sums of non-negative terms and fl being monotone.  The walk stops when best < fl(g g) for the smallest g over
//        the open faces: every unexamined point then has d2 > best STRICTLY, so it can neither win nor tie (ties go to the lowest
//        index, which needs every point at the minimum distance to have been examined).
//   (N3) TERMINATION.  r grows by one per shell; once c_d - r <= 0 and c_d + r >= dims_d - 1 on the three axes no face is open, the
//        block is the grid, and the walk ends: after at most max(dims) shells, with every point examined.  An empty grid (no finite
//        reference point) ends the same way with idx = -1, dist2 = +inf.
// The grid is an accelerator only: whatever lo, cell and dims the caller passes, the result is the brute-force minimum over the finite
// reference points with the lowest index among ties.  The order of the records inside a cell depends on the interleaving of the cursor
// atomics; no output does.  There is no float atomic.  Every index read from memory -- a face's corner, a cell's bounds, a record's
// query index -- is checked before it is used as an address, and every store is clamped to the caller's capacity.
#include "scan.h"

namespace nerf {

namespace {

constexpr double MD_ONE = 1099511627776.0;       // 2^40: fixed point of the measures
constexpr double MD_W_ONE = 549755813888.0;      // 2^39: fixed point of the sampling weight |N| (so that w_f IS the area term)
constexpr double MD_D_ONE = 1073741824.0;        // 2^30: fixed point of the distance statistics
constexpr double MD_MARGIN = 2.842170943040401e-14;  // 2^-45 (N2)
constexpr double MD_INF = __builtin_huge_val();

// does face f take part (three distinct corners with finite coordinates)?  -> the coordinates in p[corner][axis]
__device__ inline bool md_face(const MdMeshArgs& a, long long f, float (&p)[3][3]) { return face_coords<true>(a.verts, a.faces, a.V, f, p); }

// the clamped box coordinates of a participating face's corners (section 3h-6's uc)
__device__ inline void md_box(const MdMeshArgs& a, const float (&p)[3][3], double (&u)[3][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double x = ((double)p[c][d] - (double)a.lo[d]) / (double)a.scale;
      u[c][d] = fmin(fmax(x, -1.0), 2.0);
    }
}

// |N| of the face in box coordinates
__device__ inline double md_cross_len(const double (&u)[3][3]) {
  double e1[3], e2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e1[d] = u[1][d] - u[0][d];
    e2[d] = u[2][d] - u[0][d];
  }
  const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  return sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
}

// the sampling weight of face f: rint(|N| 2^39), 0 for a face that takes no part
__device__ inline long long md_weight(const MdMeshArgs& a, long long f) {
  float p[3][3];
  if (!md_face(a, f, p)) return 0;
  double u[3][3];
  md_box(a, p, u);
  return (long long)__builtin_rint(md_cross_len(u) * MD_W_ONE);
}

__device__ inline unsigned md_fin(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the uniform number of (seed, sample i, stream) in (0, 1)
__device__ inline double md_uniform(unsigned seed, unsigned i, unsigned stream) {
  const unsigned h = md_fin(md_fin(md_fin(seed + 0x9E3779B9u * (stream + 1u)) ^ i) + seed);
  return ((double)h + 0.5) / 4294967296.0;
}

// the clamped cell of a finite coordinate along one axis
__device__ inline int md_cell(float p, float lo, float cell, int dim) {
  const double t = floor(((double)p - (double)lo) / (double)cell);
  return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

__device__ inline int md_cell3(const MdGridArgs& a, const float (&p)[3], int (&c)[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) c[d] = md_cell(p[d], a.lo[d], a.cell, a.dims[d]);
  return (c[0] * a.dims[1] + c[1]) * a.dims[2] + c[2];  // (< ncell < 2^31)
}

}  // namespace

// ---- A. measures ----

// grid = ceil(F / CC_WG), whole waves, one thread per face
__global__ __launch_bounds__(CC_WG) void k_md_measure(const MdMeshArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  float p[3][3];
  long long t[6] = {0, 0, 0, 0, 0, 0};
  if (f < a.F && md_face(a, f, p)) {
    double u[3][3];
    md_box(a, p, u);
    const double len = md_cross_len(u);
    const double area = len * 0.5;
    const double X[3] = {u[1][1] * u[2][2] - u[1][2] * u[2][1], u[1][2] * u[2][0] - u[1][0] * u[2][2], u[1][0] * u[2][1] - u[1][1] * u[2][0]};
    const double six = (u[0][0] * X[0] + u[0][1] * X[1]) + u[0][2] * X[2];
    t[0] = (long long)__builtin_rint(area * MD_ONE);
    t[1] = (long long)__builtin_rint(six * MD_ONE);
#pragma unroll
    for (int d = 0; d < 3; ++d) t[2 + d] = (long long)__builtin_rint((area * (((u[0][d] + u[1][d]) + u[2][d]) / 3.0)) * MD_ONE);
    t[5] = 1;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const long long s = wave_sum(t[k]);
    if ((threadIdx.x & 63) == 0 && s != 0) agent_add(&a.out[k], s);
  }
}

// ---- B. surface samples ----

namespace {

// the value and sink of the weights' scan.  k_value_place recomputes the weights: nothing they depend on changes between the launches
struct FaceWeight {
  MdMeshArgs a;
  __device__ long long operator()(long long f) const { return md_weight(a, f); }
};
struct CumSink {  // the inclusive prefix
  long long* cum;
  __device__ void operator()(long long f, long long w, long long pre) const { cum[f] = pre + w; }
  __device__ void end(long long) const {}
};

}  // namespace

// grid = ceil(min(n, cap_n) / CC_WG), one thread per sample
__global__ __launch_bounds__(CC_WG) void k_md_sample(const MdMeshArgs a) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (i >= a.n || i >= a.cap_n) return;
  const long long W = a.F > 0 ? a.info[0] : 0;
  int face = -1;
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (W > 0) {
    const double r0 = md_uniform(a.seed, (unsigned)i, 0u);
    const double x = floor((((double)i + r0) / (double)a.n) * (double)W);
    long long t = x >= 9223372036854775808.0 ? W - 1 : (long long)x;
    t = t > W - 1 ? W - 1 : t;
    long long lo = 0, hi = (long long)a.F - 1;  // the first f with cum[f] > t, kept inside [0, F)
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (a.cum[mid] > t) hi = mid;
      else lo = mid + 1;
    }
    float p[3][3];
    if (md_face(a, lo, p)) {
      face = (int)lo;
      double r1 = md_uniform(a.seed, (unsigned)i, 1u), r2 = md_uniform(a.seed, (unsigned)i, 2u);
      if (r1 + r2 > 1.0) {
        r1 = 1.0 - r1;
        r2 = 1.0 - r2;
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double A = (double)p[0][d], B = (double)p[1][d], C = (double)p[2][d];
        out[d] = (float)((A + r1 * (B - A)) + r2 * (C - A));
      }
    }
  }
  a.face[i] = face;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.points[i * 3 + d] = out[d];
}

// ---- C. the grid: a counting sort of points by cell ----

// grid = ceil(n / CC_WG), one thread per point
__global__ __launch_bounds__(CC_WG) void k_pn_count(const MdGridArgs a, const float* __restrict__ pts, int n, int* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]};
  if (!finite3(p)) return;
  int c[3];
  agent_add(&cnt[md_cell3(a, p, c)], 1);
}

// grid = ceil(n / CC_WG), one thread per point.  Which record of its cell a point gets depends on the interleaving; the cell's set of
// records does not.
__global__ __launch_bounds__(CC_WG) void k_pn_place(const MdGridArgs a, const float* __restrict__ pts, int n, int* __restrict__ cursor,
                                                    const int* __restrict__ start, float4* __restrict__ rec) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2]};
  if (!finite3(p)) return;
  int c[3];
  const int cell = md_cell3(a, p, c);
  const long long b = start[cell], e = start[cell + 1];
  const long long at = b + (long long)agent_add(&cursor[cell], 1);
  if (b >= 0 && at >= b && at < e && e <= n) rec[at] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));
}

// grid = ceil(n / CC_WG)
__global__ __launch_bounds__(CC_WG) void k_pn_fill(int* __restrict__ idx, double* __restrict__ dist2, long long n) {
  const long long j = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (j >= n) return;
  idx[j] = -1;
  dist2[j] = MD_INF;
}

namespace {

// the points of the cells [ca, cb] (consecutive along z, so consecutive records) against the query
__device__ inline void md_scan_cells(const MdGridArgs& a, long long ca, long long cb, const double (&q)[3], double& best, int& bi) {
  long long b = a.start[ca], e = a.start[cb + 1];
  if (b < 0 || e < b || e > a.M) b = e = 0;
  for (long long k = b; k < e; ++k) {
    const float4 r = a.rec[k];
    const double dx = q[0] - (double)r.x, dy = q[1] - (double)r.y, dz = q[2] - (double)r.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const int i = __float_as_int(r.w);
    if (d2 < best || (d2 == best && i < bi)) {
      best = d2;
      bi = i;
    }
  }
}

// (N2): a lower bound, safe under rounding, on the distance from q to any point beyond the plane lo + n cell (low: below it)
__device__ inline double md_gap(double q, double lo, double cell, long long n, bool low) {
  const double A = (double)n * cell;
  const double P = lo + A;
  const double b = low ? q - P : P - q;
  const double S = (fabs(q) + fabs(lo)) + A;
  return b - MD_MARGIN * S;
}

}  // namespace

// grid = ceil(N / CC_WG), one thread per query: SORTED walks the queries' records in cell order and scatters each result to the
// query's own slot (k_pn_fill has given the queries that are not finite their answer); otherwise thread j takes query j.
template <bool SORTED>
__global__ __launch_bounds__(CC_WG) void k_pn_query(const MdGridArgs a) {
  const long long s = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (s >= a.N) return;
  float p[3];
  long long j = s;
  if (SORTED) {
    if (s >= a.scratch[0]) return;  // (the finite queries)
    const float4 r = a.qrec[s];
    p[0] = r.x, p[1] = r.y, p[2] = r.z;
    j = __float_as_int(r.w);
    if (j < 0 || j >= a.N || !finite3(p)) return;
  } else {
    p[0] = a.query[s * 3 + 0], p[1] = a.query[s * 3 + 1], p[2] = a.query[s * 3 + 2];
  }
  if (j >= a.cap_n) return;
  double best = MD_INF;
  int bi = -1;
  if (finite3(p)) {
    const double q[3] = {(double)p[0], (double)p[1], (double)p[2]};
    int c[3];
    (void)md_cell3(a, p, c);
    const long long dy = a.dims[1], dz = a.dims[2];
    for (long long r = 0;; ++r) {
      const long long x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < a.dims[0] - 1 ? c[0] + r : a.dims[0] - 1;
      const long long y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < dy - 1 ? c[1] + r : dy - 1;
      const long long z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < dz - 1 ? c[2] + r : dz - 1;
      for (long long x = x0; x <= x1; ++x) {
        const bool fx = x - c[0] == r || c[0] - x == r;
        for (long long y = y0; y <= y1; ++y) {
          const long long row = (x * dy + y) * dz;
          if (fx || y - c[1] == r || c[1] - y == r) {
            md_scan_cells(a, row + z0, row + z1, q, best, bi);  // a column of the shell's x / y faces
          } else {  // its z faces only (r > 0 here)
            if (c[2] - r >= 0) md_scan_cells(a, row + c[2] - r, row + c[2] - r, q, best, bi);
            if (c[2] + r <= dz - 1) md_scan_cells(a, row + c[2] + r, row + c[2] + r, q, best, bi);
          }
        }
      }
      bool open = false;
      double g = MD_INF;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const long long L = c[d] - r, H = c[d] + r + 1;
        if (L > 0) {
          open = true;
          g = fmin(g, md_gap(q[d], (double)a.lo[d], (double)a.cell, L, true));
        }
        if (H < a.dims[d]) {
          open = true;
          g = fmin(g, md_gap(q[d], (double)a.lo[d], (double)a.cell, H, false));
        }
      }
      if (!open) break;                  // (N3) the block is the grid
      if (g > 0.0 && best < g * g) break;  // (N1), (N2)
    }
  }
  a.idx[j] = bi;
  a.dist2[j] = best;
}

// ---- D. distance statistics ----

// grid = ceil(N / CC_WG), whole waves, one thread per distance
__global__ __launch_bounds__(CC_WG) void k_md_stats(const MdStatsArgs a) {
  const long long j = (long long)blockIdx.x * CC_WG + threadIdx.x;
  long long t[4 + MD_MAX_TAU] = {};
  if (j < a.N) {
    const double d2 = a.dist2[j];
    if (isfinite(d2) && d2 >= 0.0) {
      const double d = sqrt(d2) / a.unit, e = d2 / (a.unit * a.unit);
      t[0] = 1;
      t[1] = (long long)__builtin_rint(fmin(d, 8.0) * MD_D_ONE);
      t[2] = (long long)__builtin_rint(fmin(e, 64.0) * MD_D_ONE);
      t[3] = (d > 8.0 || e > 64.0) ? 1 : 0;
#pragma unroll
      for (int k = 0; k < MD_MAX_TAU; ++k) t[4 + k] = (k < a.K && d2 <= a.tau2[k]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 4 + MD_MAX_TAU; ++k) {
    const long long s = wave_sum(t[k]);
    if (k < 4 + a.K && (threadIdx.x & 63) == 0 && s != 0) agent_add(&a.out[k], s);
  }
}

// ---- launchers ----

hipError_t launch_md_measure(const MdMeshArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.out, 0, 8 * sizeof(long long), st));
  if (a.F > 0 && a.V > 0) LAUNCH(k_md_measure, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_md_sample(const MdMeshArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.info, 0, sizeof(long long), st));
  if (a.F > 0) TRY(scan_values<long long>(FaceWeight{a}, NoWatch{}, CumSink{a.cum}, a.F, NO_CAP, a.tot, a.base, a.info, st));
  const long long n = a.n < a.cap_n ? a.n : a.cap_n;
  if (n > 0) LAUNCH(k_md_sample, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

namespace {

// the counting sort of pts[n] by cell: cnt (zeroed here), start, rec; *total = the finite points, *most (may be null) the fullest cell
hipError_t md_sort(const MdGridArgs& a, const float* pts, int n, int* cnt, int* start, float4* rec, long long* total, long long* most,
                   hipStream_t st) {
  TRY(hipMemsetAsync(cnt, 0, (size_t)a.ncell * sizeof(int), st));
  if (n > 0) LAUNCH(k_pn_count, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a, pts, n, cnt);
  TRY(cells_to_start(cnt, a.ncell, n, a.tot, a.base, start, total, most, st));
  if (n > 0) LAUNCH(k_pn_place, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a, pts, n, cnt, start, rec);
  return hipSuccess;
}

}  // namespace

hipError_t launch_md_grid_build(const MdGridArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 2 * sizeof(long long), st));
  return md_sort(a, a.ref, a.M, a.cnt, a.start, a.rec, a.counts, a.counts + 1, st);
}

hipError_t launch_md_nearest(const MdGridArgs& a, bool sort_queries, hipStream_t st) {
  const long long n = a.N < a.cap_n ? a.N : a.cap_n;
  if (n <= 0) return hipSuccess;
  if (sort_queries) {
    LAUNCH(k_pn_fill, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a.idx, a.dist2, n);
    TRY(md_sort(a, a.query, a.N, a.qcnt, a.qstart, a.qrec, a.scratch, nullptr, st));
    LAUNCH(k_pn_query<true>, dim3(grid(a.N, CC_WG)), dim3(CC_WG), 0, st, a);
  } else {
    LAUNCH(k_pn_query<false>, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_md_stats(const MdStatsArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.out, 0, (size_t)(4 + a.K) * sizeof(long long), st));
  if (a.N > 0) LAUNCH(k_md_stats, dim3(grid(a.N, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
