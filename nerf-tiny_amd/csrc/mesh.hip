// mesh.hip -- marching cubes over a density grid (nerf_hip_mesh_count / nerf_hip_mesh_emit), and the same under a
// mask of valid lattice points (nerf_hip_mesh_count_masked / nerf_hip_mesh_emit_masked; section 3h-10, rule M of include/nerf_hip.h):
//   k_mesh_count   per lattice point: the 0-3 vertices it owns (edges to its +x / +y / +z neighbour whose ends differ in insideness)
//                  and the triangle count of the cell whose lowest corner it is; in-block exclusive vertex offsets, block totals
//   k_mesh_scan    one workgroup: 64-bit exclusive scans of the block totals (scan.h scan_totals over two channels), and the totals V, F
//   k_mesh_emit    vertices + normals of the owned edges at their offsets, faces at the block's face base + an in-block scan of the
//                  recomputed triangle counts; vertex ids of neighbouring owners from the stored offsets
// A workgroup takes MESH_PTS consecutive lattice points in MESH_ROUNDS rounds of MESH_WG (reads along z are coalesced).  The output
// order is fixed by the scans -- no atomics place anything -- and every store is clamped to the caller's capacities.  The scan is
// three kernels, never a single-pass look-back: no flag crosses workgroups (or XCDs) inside a launch.  The in-workgroup prefixes
// (wg_prefix<MESH_WG, 2> over the vertex counts, <MESH_WG, 3> over the triangle counts) and the scan of the totals are scan.h's.
// MASKED (template <bool MASKED> over count and emit): a cell is live iff its eight corners are valid, triangles come from live cells
// only and an edge carries a vertex only where one of the up to four cells around it is live.  The mask is read directly, and only
// where the unmasked rule finds something: 8 bytes for a mixed cell, up to 18 for a sign-changing edge -- no pre-pass, no extra
// workspace.  Normals read the grid as before, at invalid points too.  The unmasked instantiations never touch the mask.
// Built with -ffp-contract=off: every product and sum below is rounded on its own, as tests/mc_reference.py restates them.
#include "scan.h"

#define MC_TABLE_QUALIFIER static constexpr
#include "mc_tables.h"

namespace nerf {

namespace {

struct TriTable {
  signed char e[256][16];
};
struct TriCount {
  unsigned char n[256];
};
constexpr TriTable make_tri_table() {
  TriTable t{};
  for (int c = 0; c < 256; ++c)
    for (int i = 0; i < 16; ++i) t.e[c][i] = mc_tri_table[c][i];
  return t;
}
constexpr TriCount make_tri_count() {
  TriCount t{};
  for (int c = 0; c < 256; ++c) {
    int n = 0;
    while (n < 16 && mc_tri_table[c][n] >= 0) ++n;
    t.n[c] = (unsigned char)(n / 3);
  }
  return t;
}

}  // namespace

__constant__ TriTable c_mc_tri = make_tri_table();
__constant__ TriCount c_mc_ntri = make_tri_count();
// edge e (mc_tables.h) -> its lower endpoint's corner offset (bit 0 dx, bit 1 dy, bit 2 dz) and axis (0 x, 1 y, 2 z)
__constant__ unsigned char c_mc_edge_own[12] = {0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 3, 2};
__constant__ unsigned char c_mc_edge_axis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

namespace {

struct Point {
  int p, i, j, k;
};

__device__ inline Point decode(int p, int ny, int nz) {
  Point q;
  q.p = p;
  const unsigned nynz = (unsigned)ny * (unsigned)nz;
  q.i = (int)((unsigned)p / nynz);
  const unsigned rem = (unsigned)p - (unsigned)q.i * nynz;
  q.j = (int)(rem / (unsigned)nz);
  q.k = (int)(rem - (unsigned)q.j * (unsigned)nz);
  return q;
}

// rule M: the cell whose lowest corner is (i, j, k) exists and its eight corners are valid
__device__ inline bool cell_live(const unsigned char* __restrict__ v, int i, int j, int k, int nx, int ny, int nz) {
  if (i < 0 || j < 0 || k < 0 || i + 1 >= nx || j + 1 >= ny || k + 1 >= nz) return false;
  const int X = ny * nz, Y = nz, p = (i * ny + j) * nz + k;
  // (no short circuit: the eight byte loads are independent and go out together)
  return ((v[p] != 0) & (v[p + 1] != 0) & (v[p + Y] != 0) & (v[p + Y + 1] != 0) & (v[p + X] != 0) & (v[p + X + 1] != 0) & (v[p + X + Y] != 0) &
          (v[p + X + Y + 1] != 0)) != 0;
}

// rule M: one of the up to four cells that contain the edge from (i, j, k) to its +ax neighbour is live
__device__ inline bool edge_live(const unsigned char* __restrict__ v, int i, int j, int k, int ax, int nx, int ny, int nz) {
  const int u[3] = {ax == 0 ? 0 : 1, ax == 1 ? 0 : 1, ax == 2 ? 0 : 1};  // the cells step back along the two other axes
  bool live = false;
  for (int di = 0; di <= u[0]; ++di)
    for (int dj = 0; dj <= u[1]; ++dj)
      for (int dk = 0; dk <= u[2]; ++dk) live |= cell_live(v, i - di, j - dj, k - dk, nx, ny, nz);
  return live;
}

// bit a: the edge from q to its +a neighbour has a vertex (NaN counts as outside: a comparison with NaN is false)
template <bool MASKED>
__device__ inline unsigned edge_mask(const float* __restrict__ s, const unsigned char* __restrict__ valid, const Point& q, int nx, int ny,
                                     int nz, float level) {
  const int nynz = ny * nz;
  const bool in0 = s[q.p] > level;
  unsigned m = 0;
  if (q.i + 1 < nx && (s[q.p + nynz] > level) != in0) m |= 1u;
  if (q.j + 1 < ny && (s[q.p + nz] > level) != in0) m |= 2u;
  if (q.k + 1 < nz && (s[q.p + 1] > level) != in0) m |= 4u;
  if constexpr (MASKED) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
      if ((m & (1u << ax)) && !edge_live(valid, q.i, q.j, q.k, ax, nx, ny, nz)) m &= ~(1u << ax);
  }
  return m;
}

// table row of the cell whose lowest corner is q (bit c set: corner c outside), or -1 where q is on the grid's upper faces
__device__ inline int cube_row(const float* __restrict__ s, const Point& q, int nx, int ny, int nz, float level) {
  if (q.i + 1 >= nx || q.j + 1 >= ny || q.k + 1 >= nz) return -1;
  const int X = ny * nz, Y = nz, p = q.p;
  const int off[8] = {0, X, X + Y, Y, 1, X + 1, X + Y + 1, Y + 1};
  int c = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) c |= (s[p + off[b]] > level) ? 0 : (1 << b);
  return c;
}

// triangles of the cell whose lowest corner is q, from its table row c (MASKED: none where the cell is not live)
template <bool MASKED>
__device__ inline int cell_faces(const unsigned char* __restrict__ valid, const Point& q, int c, int nx, int ny, int nz) {
  if (!(c > 0 && c < 255)) return 0;
  if constexpr (MASKED) {
    if (!cell_live(valid, q.i, q.j, q.k, nx, ny, nz)) return 0;
  }
  return c_mc_ntri.n[c];
}

__device__ inline float lattice(float lo, int i, float step) { return lo + (float)i * step; }

// d sigma / d x_a at lattice point p (index ia of na >= 2 along a): central inside, one-sided at the grid's faces
__device__ inline float grad_axis(const float* __restrict__ s, int p, int ia, int na, int stride, float step) {
  if (ia == 0) return (s[p + stride] - s[p]) / step;
  if (ia == na - 1) return (s[p] - s[p - stride]) / step;
  return (s[p + stride] - s[p - stride]) / (2.0f * step);
}

}  // namespace

// grid = nb workgroups of MESH_WG
template <bool MASKED>
__global__ __launch_bounds__(MESH_WG) void k_mesh_count(const MeshArgs a) {
  __shared__ int part[MESH_WG / 64];
  const float* __restrict__ s = a.sigma;
  const long long N = (long long)a.nx * a.ny * a.nz;
  const long long base = (long long)blockIdx.x * MESH_PTS;
  int run_v = 0, run_f = 0;
  for (int r = 0; r < MESH_ROUNDS; ++r) {
    const long long pl = base + r * MESH_WG + threadIdx.x;
    unsigned mask = 0;
    int nf = 0;
    Point q{};
    if (pl < N) {
      q = decode((int)pl, a.ny, a.nz);
      mask = edge_mask<MASKED>(s, a.valid, q, a.nx, a.ny, a.nz, a.level);
      const int c = cube_row(s, q, a.nx, a.ny, a.nz, a.level);
      nf = cell_faces<MASKED>(a.valid, q, c, a.nx, a.ny, a.nz);
    }
    int tot_v, tot_f;
    const int pre_v = wg_prefix<MESH_WG, 2>(__popc(mask), part, tot_v);
    (void)wg_prefix<MESH_WG, 3>(nf, part, tot_f);
    if (mask) a.offs[q.p] = ((unsigned)(run_v + pre_v) << 3) | mask;  // read back only for owners of vertices
    run_v += tot_v;
    run_f += tot_f;
  }
  if (threadIdx.x == 0) {
    a.tv[blockIdx.x] = run_v;
    a.tf[blockIdx.x] = run_f;
  }
}

// one workgroup of 1024
__global__ __launch_bounds__(1024) void k_mesh_scan(const MeshArgs a, int nb) {
  long long n[2];  // V, F
  scan_totals(nb, n, Totals<int, long long>{a.tv, a.bv}, Totals<int, long long>{a.tf, a.bf});
  if (threadIdx.x == 1023) {
    a.bv[nb] = n[0];
    a.bf[nb] = n[1];
    a.counts[0] = n[0];
    a.counts[1] = n[1];
  }
}

// grid = nb workgroups of MESH_WG
template <bool MASKED>
__global__ __launch_bounds__(MESH_WG) void k_mesh_emit(const MeshArgs a) {
  __shared__ int part[MESH_WG / 64];
  const float* __restrict__ s = a.sigma;
  const unsigned* __restrict__ offs = a.offs;
  const long long vb = a.bv[blockIdx.x], fb = a.bf[blockIdx.x];
  if (a.bv[blockIdx.x + 1] == vb && a.bf[blockIdx.x + 1] == fb) return;  // (uniform) no vertex, no face: sigma is not read again
  const int nx = a.nx, ny = a.ny, nz = a.nz, nynz = ny * nz;
  const long long N = (long long)nx * ny * nz;
  const long long base = (long long)blockIdx.x * MESH_PTS;
  const int stride[3] = {nynz, nz, 1};
  const int dim[3] = {nx, ny, nz};
  int run_f = 0;
  for (int r = 0; r < MESH_ROUNDS; ++r) {
    const long long pl = base + r * MESH_WG + threadIdx.x;
    int c = -1, nf = 0;
    Point q{};
    if (pl < N) {
      q = decode((int)pl, ny, nz);
      const unsigned mask = edge_mask<MASKED>(s, a.valid, q, nx, ny, nz, a.level);
      if (mask) {
        const int idx[3] = {q.i, q.j, q.k};
        float pa[3], ga[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          pa[d] = lattice(a.lo[d], idx[d], a.step[d]);
          ga[d] = grad_axis(s, q.p, idx[d], dim[d], stride[d], a.step[d]);
        }
        long long v = vb + (long long)(offs[q.p] >> 3);
        const float s0 = s[q.p];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          if (!(mask & (1u << ax))) continue;
          const int pb = q.p + stride[ax];
          const float s1 = s[pb];
          float t = (a.level - s0) / (s1 - s0);
          if (!isfinite(t)) t = 0.5f;
          float x[3] = {pa[0], pa[1], pa[2]};
          const float pb_ax = lattice(a.lo[ax], idx[ax] + 1, a.step[ax]);
          x[ax] = pa[ax] + t * (pb_ax - pa[ax]);
          float g[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const float gb = grad_axis(s, pb, idx[d] + (d == ax ? 1 : 0), dim[d], stride[d], a.step[d]);
            g[d] = ga[d] + t * (gb - ga[d]);
          }
          const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
          const bool ok = isfinite(len) && len > 0.0f;
          if (v >= 0 && v < a.max_v) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              a.verts[v * 3 + d] = x[d];
              a.normals[v * 3 + d] = ok ? -g[d] / len : 0.0f;
            }
          }
          ++v;
        }
      }
      c = cube_row(s, q, nx, ny, nz, a.level);
      nf = cell_faces<MASKED>(a.valid, q, c, nx, ny, nz);
    }
    int tot_f;
    const int pre_f = wg_prefix<MESH_WG, 3>(nf, part, tot_f);
    if (nf) {
      long long f = fb + run_f + pre_f;
      for (int t = 0; t < nf; ++t, ++f) {
        int id[3];
#pragma unroll
        for (int e3 = 0; e3 < 3; ++e3) {
          const int e = c_mc_tri.e[c][3 * t + e3];
          const unsigned own = c_mc_edge_own[e], ax = c_mc_edge_axis[e];
          const int o = q.p + ((own & 1) ? nynz : 0) + ((own & 2) ? nz : 0) + ((own & 4) ? 1 : 0);
          const unsigned w = offs[o];
          id[e3] = (int)(a.bv[o / MESH_PTS] + (long long)(w >> 3) + __popc(w & ((1u << ax) - 1u)));
        }
        if (f >= 0 && f < a.max_f) {
          a.faces[f * 3 + 0] = id[0];
          a.faces[f * 3 + 1] = id[1];
          a.faces[f * 3 + 2] = id[2];
        }
      }
    }
    run_f += tot_f;
  }
}

hipError_t launch_mesh_count(const MeshArgs& a, hipStream_t st) {
  const int nb = mesh_blocks((long long)a.nx * a.ny * a.nz);
  if (a.valid) {
    LAUNCH(k_mesh_count<true>, dim3(nb), dim3(MESH_WG), 0, st, a);
  } else {
    LAUNCH(k_mesh_count<false>, dim3(nb), dim3(MESH_WG), 0, st, a);
  }
  LAUNCH(k_mesh_scan, dim3(1), dim3(1024), 0, st, a, nb);
  return hipSuccess;
}

hipError_t launch_mesh_emit(const MeshArgs& a, hipStream_t st) {
  const int nb = mesh_blocks((long long)a.nx * a.ny * a.nz);
  if (a.valid) {
    LAUNCH(k_mesh_emit<true>, dim3(nb), dim3(MESH_WG), 0, st, a);
  } else {
    LAUNCH(k_mesh_emit<false>, dim3(nb), dim3(MESH_WG), 0, st, a);
  }
  return hipSuccess;
}

}  // namespace nerf
