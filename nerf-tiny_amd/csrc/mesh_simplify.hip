// mesh_simplify.hip -- simplification of an indexed triangle mesh by uniform vertex clustering (nerf_hip_mesh_simplify_*; DESIGN.md
// section 3h-4; the definition is in include/nerf_hip.h).
//   k_ms_keys        per vertex: its cell of the cluster lattice into vcl[v] (-1: a coordinate is not finite), occ[cell] = 1
//   scan.h's k_flag_count / k_flag_scan / k_flag_place   the three-launch compaction over a 0/1 flag per item, instantiated here for
//                    the occupied cells (-> ascending cluster ids), the referenced clusters (-> output vertex ids) and the kept faces
//   k_ms_accum       per vertex: vcl[v] = its cluster id; member counts and fixed-point coordinate / normal sums by integer atomics,
//                    aggregated inside the wave first
//   k_ms_faces       per face: take part / degenerate; the canonical cluster triple goes into the face table
//   k_ms_mark        per face: kept iff its slot holds its own index; kept faces mark their three clusters
//   k_ms_verts       per referenced cluster: sums -> position and normal (fp64 as defined)
//
// THE FACE TABLE: open addressing over `slots` int32 words (a power of two > F), -1 = empty, otherwise a face index.  The key of a
// face is its cluster triple rotated so that the smallest id comes first; a slot's key is the key of the face it holds, recomputed
// from faces[] and vcl[], which no launch that touches the table writes.
//   (T1) A slot leaves -1 only by atomicCAS(slot, -1, f) and is never emptied.  Afterwards it changes only by atomicMin(slot, f) with
//        an f whose key equals the slot's: the key of a non-empty slot never changes, and its value only decreases.
//   (T2) Every face of key K walks the same probe sequence and stops at the first slot that is empty (it claims it) or holds K.  By
//        (T1) a slot that some face passed over (it held another key) holds that key for ever, and a slot claimed for K holds K for
//        ever: every face of K ends in the same slot, whatever the interleaving, and after the launch that slot holds the lowest
//        face index of K.  A face is kept iff its slot holds its own index (read by the NEXT launch).
//   (T3) Every access to the table inside k_ms_faces is an agent-scope atomic (CAS and min; the CAS's return is the only read), so
//        nothing is served from an L1 or from another XCD's L2.  Nothing waits for another workgroup: a probe ends after at most
//        `slots` steps.  There are at most F keys in more than F slots, so an empty slot always exists; a probe that found none all
//        the same sets NERF_HIP_SIMPLIFY_TABLE_FULL in counts[3] and the caller raises -- never a hang, never a silent drop.
// Which slot a key lands in depends on the interleaving; nothing that leaves this file does.  All sums are integer atomics (order
// free), nothing is placed by an atomic, and the plain stores that race (occ[c] = 1, ref[c] = 1) all store the same value.  Every
// index read from memory is checked before it is used as an address and every output store is clamped to max_v / max_f.
#include "scan.h"

namespace nerf {

namespace {

constexpr double MS_POS_ONE = 1048576.0;    // 2^20: fixed point of the lattice coordinates (uc <= 2048: a term is at most 2^31)
constexpr double MS_NRM_ONE = 268435456.0;  // 2^28: fixed point of the normals' components (clamped to [-2, 2]: at most 2^29)
constexpr long long MS_FLAG_TABLE_FULL = 1;

// -> the slot's value before: -1 when f was stored
__device__ inline int ms_atomic_claim(int* p, int f) {
  int expected = -1;
  __hip_atomic_compare_exchange_strong(p, &expected, f, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return expected;
}

// the clamped lattice coordinates uc[3] of vertex v and its cell (C order, z fastest); -1 when a coordinate is not finite
__device__ inline int ms_cell(const MsArgs& a, long long v, float (&uc)[3]) {
  bool ok = true;
  long long lin = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float p = a.verts[v * 3 + d];
    ok = ok && isfinite(p);
    const float u = (p - a.lo[d]) / a.cell[d];  // two fp32 roundings, IEEE division
    const float dm = (float)a.dims[d];
    uc[d] = fminf(fmaxf(u, 0.0f), dm);  // (a NaN u, of a vertex that is left out anyway, becomes 0)
    lin = lin * a.dims[d] + (int)fminf(floorf(uc[d]), dm - 1.0f);
  }
  return ok ? (int)lin : -1;
}

// 0: face f takes no part, 1: degenerate, 2: a candidate, with its cluster triple k rotated so that the smallest id is first
__device__ inline int ms_triple(const MsArgs& a, long long f, int (&k)[3]) {
  const int i0 = a.faces[f * 3 + 0], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
  const unsigned V = (unsigned)a.V;
  if ((unsigned)i0 >= V || (unsigned)i1 >= V || (unsigned)i2 >= V) return 0;  // never used as an address
  const int c0 = a.vcl[i0], c1 = a.vcl[i1], c2 = a.vcl[i2];
  if ((unsigned)c0 >= V || (unsigned)c1 >= V || (unsigned)c2 >= V) return 0;  // (-1: a vertex in no cluster)
  if (c0 == c1 || c1 == c2 || c0 == c2) return 1;
  if (c0 < c1 && c0 < c2) {
    k[0] = c0, k[1] = c1, k[2] = c2;
  } else if (c1 < c2) {
    k[0] = c1, k[1] = c2, k[2] = c0;
  } else {
    k[0] = c2, k[1] = c0, k[2] = c1;
  }
  return 2;
}

__device__ inline unsigned ms_hash(const int (&k)[3]) {
  unsigned h = (unsigned)k[0] * 0x9E3779B1u ^ (unsigned)k[1] * 0x85EBCA77u ^ (unsigned)k[2] * 0xC2B2AE3Du;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h;
}

}  // namespace

// ---- the flags and sinks of scan.h's compaction.  k_flag_place recomputes the flags: a sink changes its own item only, and never
// whether it is flagged ----

// a non-zero word is flagged; the sink leaves rank + 1 in its place (0 stays 0), so the flags read the same before and after
struct MsWordFlag {
  const int* w;
  __device__ int operator()(long long i) const { return w[i] != 0; }
};
struct MsWordSink {
  int* w;
  __device__ void operator()(long long i, int flag, long long pos) const {
    if (flag) w[i] = (int)pos + 1;
  }
};

struct MsFaceKeep {
  const int* fstate;
  __device__ int operator()(long long i) const { return fstate[i] == 1; }
};
struct MsFaceSink {  // the kept faces' corners: vertex -> cluster -> output vertex, every step checked
  const int *faces, *vcl, *ref;
  int* out_faces;
  int V;
  long long max_f;
  __device__ void operator()(long long i, int flag, long long pos) const {
    if (!flag || pos >= max_f) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int v = faces[i * 3 + d];
      int o = -1;
      if ((unsigned)v < (unsigned)V) {
        const int c = vcl[v];
        if ((unsigned)c < (unsigned)V) o = ref[c] - 1;
      }
      out_faces[pos * 3 + d] = o;
    }
  }
};

// ---- vertices -> cells -> clusters ----

// grid = ceil(V / CC_WG), one thread per vertex
__global__ __launch_bounds__(CC_WG) void k_ms_keys(const MsArgs a) {
  const long long v = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (v >= a.V) return;
  float uc[3];
  const int c = ms_cell(a, v, uc);
  a.vcl[v] = c;
  if (c >= 0 && c < a.ncell) a.occ[c] = 1;  // (every writer stores the same 1)
}

// grid = ceil(V / CC_WG), whole waves.  One atomic per sum per distinct cluster per wave-instruction: the wave peels off the cluster of
// its first remaining lane (marching-cubes vertices arrive in cell order, so a wave holds few), its lanes are counted by a ballot,
// their terms summed across the wave, and the leading lane issues the atomics.  NRM: the normals' sums as well.
template <bool NRM>
__global__ __launch_bounds__(CC_WG) void k_ms_accum(const MsArgs a) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  constexpr int NS = NRM ? 6 : 3;
  long long term[NS];
#pragma unroll
  for (int d = 0; d < NS; ++d) term[d] = 0;
  int id = -1;
  if (i < a.V) {
    float uc[3];
    (void)ms_cell(a, i, uc);
    const int c = a.vcl[i];  // k_ms_keys' cell
    if ((unsigned)c < (unsigned)a.ncell) id = a.occ[c] - 1;
    if ((unsigned)id >= (unsigned)a.V) id = -1;  // (never taken for an occupied cell: clusters are at most V)
    a.vcl[i] = id;
    if (id >= 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) term[d] = (long long)__builtin_rint((double)uc[d] * MS_POS_ONE);
      if (NRM) {
        const float nx = a.normals[i * 3 + 0], ny = a.normals[i * 3 + 1], nz = a.normals[i * 3 + 2];
        if (isfinite(nx) && isfinite(ny) && isfinite(nz)) {
          const float n3[3] = {nx, ny, nz};
#pragma unroll
          for (int d = 0; d < 3; ++d) term[3 + d] = (long long)__builtin_rint((double)fminf(fmaxf(n3[d], -2.0f), 2.0f) * MS_NRM_ONE);
        }
      }
    }
  }
  const bool act = id >= 0;
  unsigned long long todo = __ballot(act);
  while (todo) {  // (uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const int lc = __shfl(id, lead);
    const bool mine = act && id == lc;
    const unsigned long long grp = __ballot(mine);
    const int k = __popcll(grp);
    long long r[NS];
#pragma unroll
    for (int d = 0; d < NS; ++d) {
      r[d] = mine ? term[d] : 0;
      if (k > 1) r[d] = wave_sum(r[d]);  // (uniform)
    }
    if (lane == lead) {
      agent_add(&a.cnt[lc], k);
#pragma unroll
      for (int d = 0; d < 3; ++d) agent_add(&a.S[(long long)lc * 3 + d], r[d]);
      if (NRM) {
#pragma unroll
        for (int d = 0; d < 3; ++d) agent_add(&a.T[(long long)lc * 3 + d], r[3 + d]);
      }
    }
    todo &= ~grp;
  }
}

// ---- faces ----

// grid = ceil(F / CC_WG), whole waves, one thread per face: (T1)-(T3) above
__global__ __launch_bounds__(CC_WG) void k_ms_faces(const MsArgs a) {
  const long long fl = (long long)blockIdx.x * CC_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int k[3] = {0, 0, 0};
  const int code = fl < a.F ? ms_triple(a, fl, k) : 0;
  if (code == 2) {
    const int f = (int)fl;
    const long long mask = a.slots - 1;
    const long long h = ms_hash(k);
    int slot = -1;
    for (long long p = 0; p < a.slots; ++p) {
      const long long s = (h + p) & mask;
      const int g = ms_atomic_claim(&a.table[s], f);
      if (g == -1) {  // claimed
        slot = (int)s;
        break;
      }
      int kg[3];
      if ((unsigned)g < (unsigned)a.F && ms_triple(a, g, kg) == 2 && kg[0] == k[0] && kg[1] == k[1] && kg[2] == k[2]) {
        if (f < g) agent_atomic_min(&a.table[s], f);  // (the slot only decreases: nothing to do for f > g)
        slot = (int)s;
        break;
      }
    }
    if (slot < 0) __hip_atomic_fetch_or(&a.counts[3], MS_FLAG_TABLE_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.fstate[f] = slot;
  } else if (fl < a.F) {
    a.fstate[fl] = -1;
  }
  const unsigned long long deg = __ballot(code == 1);
  if (lane == 0 && deg) agent_add(&a.counts[4], (long long)__popcll(deg));
}

// grid = ceil(F / CC_WG), whole waves
__global__ __launch_bounds__(CC_WG) void k_ms_mark(const MsArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool dup = false;
  if (f < a.F) {
    const int s = a.fstate[f];
    bool kept = false;
    if (s >= 0 && s < a.slots) {
      kept = a.table[s] == (int)f;
      dup = !kept;
    }
    int k[3];
    if (kept && ms_triple(a, f, k) == 2) {
      a.ref[k[0]] = 1;  // (ms_triple checked the three ids; every writer stores the same 1)
      a.ref[k[1]] = 1;
      a.ref[k[2]] = 1;
    } else {
      kept = false;
    }
    a.fstate[f] = kept ? 1 : 0;
  }
  const unsigned long long m = __ballot(dup);
  if (lane == 0 && m) agent_add(&a.counts[5], (long long)__popcll(m));
}

// ---- output vertices ----

// grid = ceil(V / CC_WG), one thread per possible cluster: the referenced ones store their position (and normal) at their output id
__global__ __launch_bounds__(CC_WG) void k_ms_verts(const MsArgs a) {
  const long long c = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (c >= a.V) return;
  const long long o = (long long)a.ref[c] - 1;
  if (o < 0 || o >= a.max_v) return;
  const double n = (double)a.cnt[c];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double mean = (double)a.S[c * 3 + d] / (n * MS_POS_ONE);
    a.out_verts[o * 3 + d] = (float)((double)a.lo[d] + (double)a.cell[d] * mean);
  }
  if (a.out_normals) {
    const double tx = (double)a.T[c * 3 + 0], ty = (double)a.T[c * 3 + 1], tz = (double)a.T[c * 3 + 2];
    const double len = sqrt((tx * tx + ty * ty) + tz * tz);
    a.out_normals[o * 3 + 0] = len > 0.0 ? (float)(tx / len) : 0.0f;
    a.out_normals[o * 3 + 1] = len > 0.0 ? (float)(ty / len) : 0.0f;
    a.out_normals[o * 3 + 2] = len > 0.0 ? (float)(tz / len) : 0.0f;
  }
}

// ---- launchers ----

hipError_t launch_ms_count(const MsArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 6 * sizeof(long long), st));
  if (a.V == 0) return hipSuccess;  // no cluster, and no face takes part
  TRY(hipMemsetAsync(a.occ, 0, (size_t)a.ncell * sizeof(int), st));
  TRY(hipMemsetAsync(a.cnt, 0, (size_t)a.V * sizeof(int), st));
  TRY(hipMemsetAsync(a.S, 0, (size_t)a.V * 3 * sizeof(long long), st));
  TRY(hipMemsetAsync(a.T, 0, (size_t)a.V * 3 * sizeof(long long), st));
  TRY(hipMemsetAsync(a.ref, 0, (size_t)a.V * sizeof(int), st));
  LAUNCH(k_ms_keys, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a);
  TRY(scan_place(MsWordFlag{a.occ}, MsWordSink{a.occ}, a.ncell, a.tot, a.base, a.counts + 2, st));
  if (a.normals)
    LAUNCH(k_ms_accum<true>, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a);
  else
    LAUNCH(k_ms_accum<false>, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a);
  if (a.F == 0) return hipSuccess;
  TRY(hipMemsetAsync(a.table, 0xFF, (size_t)a.slots * sizeof(int), st));
  LAUNCH(k_ms_faces, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  LAUNCH(k_ms_mark, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  TRY(scan_place(MsWordFlag{a.ref}, MsWordSink{a.ref}, a.V, a.tot, a.base, a.counts + 0, st));
  // the kept faces are only counted here: the emit call places them
  return scan_count(MsFaceKeep{a.fstate}, a.F, a.tot, a.base, a.counts + 1, st);
}

hipError_t launch_ms_emit(const MsArgs& a, hipStream_t st) {
  if (a.V == 0 || a.F == 0) return hipSuccess;  // V' = F' = 0
  if (a.max_v > 0) LAUNCH(k_ms_verts, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a);
  if (a.max_f > 0)
    TRY(scan_place(MsFaceKeep{a.fstate}, MsFaceSink{a.faces, a.vcl, a.ref, a.out_faces, a.V, a.max_f}, a.F, a.tot, a.base, a.scratch,
                         st));
  return hipSuccess;
}

}  // namespace nerf
