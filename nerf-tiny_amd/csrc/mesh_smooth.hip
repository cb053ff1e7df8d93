// mesh_smooth.hip -- edge topology, Taubin smoothing steps and face-derived vertex normals of an indexed triangle mesh
// (nerf_hip_mesh_edges_*, nerf_hip_mesh_smooth_step, nerf_hip_mesh_vertex_normals; the definition is in
// include/nerf_hip.h).
//   k_me_insert      per face: take part?; its three undirected edges go into the edge table, count and tally by integer atomics
//   k_me_edges       per slot: the edge's class -> counts; degrees by integer atomics, vertex flags by fetch_or
//   scan.h's value scan over Degree   per vertex: off[v] = its row's start, the grand total (2 E) into off[V]; its sum pass (DegWatch)
//                    leaves the vertices in use and the largest degree in counts
//   k_me_fill        per slot: the edge's two directed entries, each placed through its row's cursor atomic
//   k_me_step        per vertex: one Jacobi step -- walks its row, sums the neighbours' fixed-point coordinates in int64 registers
//   k_me_nrm_accum   per face: rint(cross product * 2^40) added to its three vertices by int64 atomics
//   k_me_nrm_final   per vertex: sums -> unit normal (fp64 as defined)
//
// THE EDGE TABLE: open addressing over `slots` int64 words (a power of two >= 4 F, so more than the 3 F keys it can meet), -1 = empty,
// otherwise the key (min << 32) | max of an edge -- never -1, both halves being vertex indices in [0, V).  A slot IS its key:
//   (T1) A slot leaves -1 only by atomicCAS(slot, -1, key) and never changes again.
//   (T2) Every face of key K walks the same probe sequence and stops at the first slot whose CAS returns -1 (it has just stored K) or K.
//        By (T1) a slot passed over holds another key for ever and a slot that holds K holds it for ever: all faces of K end in the
//        same slot, whatever the interleaving, and K occupies exactly one slot.
//   (T3) Every access to the table, the counts and the tallies inside k_me_insert is an agent-scope atomic (the CAS's return is the
//        only read), so nothing is served from an L1 or from another XCD's L2.  Nothing waits for another workgroup: a probe ends after
//        at most `slots` steps.  At most 3 F keys meet at least 4 F slots, so an empty slot always exists; a probe that found none all
//        the same sets NERF_HIP_EDGES_TABLE_FULL in counts[6] and the caller raises -- never a hang, never a silent drop.
// Which slot a key lands in, and the order of the entries inside a row of the adjacency, depend on the interleaving; nothing that
// leaves this file does: every public output is a count, a flag, or a sum of integers (a step sums its row in int64, whatever its
// order; the normals' sums are int64 atomics).  There is no float atomic.  Every index read from memory -- a face's corner, a key's
// halves, a row's bounds, a row's entry -- is checked before it is used as an address.
#include "scan.h"

namespace nerf {

namespace {

constexpr double ME_POS_ONE = 1073741824.0;     // 2^30: fixed point of the box coordinates (clamped to [-1, 2]: |q| <= 2^31)
constexpr double ME_NRM_ONE = 1099511627776.0;  // 2^40: fixed point of a face's cross product (|N_k| <= 18: a term is below 2^45)
constexpr long long ME_FLAG_TABLE_FULL = 1;

// -> the slot's value before: -1 when key was stored
__device__ inline long long me_claim(long long* p, long long key) {
  long long expected = -1;
  __hip_atomic_compare_exchange_strong(p, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return expected;
}

__device__ inline unsigned long long me_hash(unsigned long long k) {
  k ^= k >> 30;
  k *= 0xBF58476D1CE4E5B9ull;
  k ^= k >> 27;
  k *= 0x94D049BB133111EBull;
  k ^= k >> 31;
  return k;
}

// one add per wave: the lanes whose flag is set, counted by a ballot
__device__ inline void me_count(bool flag, long long* counter) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) agent_add(counter, (long long)__popcll(m));
}

// does face f take part (three distinct corners in range)?  -> its corners in i[3]
__device__ inline bool me_face(const MeArgs& a, long long f, int (&i)[3]) { return face_corners<true>(a.faces, a.V, f, i); }

// the edge of slot s: false for an empty slot (or a word that is no key of this mesh)
__device__ inline bool me_slot_edge(const MeArgs& a, long long s, int& lo, int& hi) {
  const long long key = a.keys[s];
  if (key < 0) return false;
  lo = (int)(key >> 32);
  hi = (int)(key & 0xFFFFFFFFll);
  return (unsigned)lo < (unsigned)a.V && (unsigned)hi < (unsigned)a.V && lo < hi;
}

// the clamped box coordinate of p along axis d
__device__ inline double me_uc(const MeArgs& a, float p, int d) {
  const double u = ((double)p - (double)a.lo[d]) / (double)a.scale;
  return fmin(fmax(u, -1.0), 2.0);
}

// the value, watch and sink of the degrees' scan.  A degree is what k_me_edges left, kept inside [0, V]; k_value_place recomputes
// it: nothing writes the degrees after k_me_edges
struct Degree {
  const int* degree;
  long long V;
  __device__ long long operator()(long long v) const { return count_in(degree, v, V); }
};
struct DegWatch {  // counts[5] = the vertices of degree > 0, counts[7] = the largest degree
  long long* counts;
  WatchMax top;
  __device__ void operator()(long long d) {
    top(d);
    me_count(d > 0, &counts[5]);
  }
  __device__ void done() { top.done(); }
};
struct RowSink {  // off[V] (the grand total) is k_flag_scan's
  long long* off;
  __device__ void operator()(long long v, long long, long long pre) const { off[v] = pre; }
  __device__ void end(long long) const {}
};

}  // namespace

// ---- faces -> edges ----

// grid = ceil(F / CC_WG), whole waves, one thread per face: (T1)-(T3) above
__global__ __launch_bounds__(CC_WG) void k_me_insert(const MeArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  int i[3] = {0, 0, 0};
  const bool part = f < a.F && me_face(a, f, i);
  if (part) {
    const long long mask = a.slots - 1;
    bool full = false;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int p = i[e], q = i[(e + 1) % 3];  // the face runs the edge p -> q
      const int lo = p < q ? p : q, hi = p < q ? q : p;
      const long long key = ((long long)lo << 32) | (long long)hi;
      const long long h = (long long)(me_hash((unsigned long long)key) & (unsigned long long)mask);
      long long slot = -1;
      for (long long t = 0; t < a.slots; ++t) {
        const long long s = (h + t) & mask;
        const long long g = me_claim(&a.keys[s], key);
        if (g == -1 || g == key) {
          slot = s;
          break;
        }
      }
      if (slot < 0) {
        full = true;
      } else {
        agent_add(&a.cnt[slot], 1);
        agent_add(&a.tally[slot], p < q ? 1 : -1);
      }
    }
    if (full) __hip_atomic_fetch_or(&a.counts[6], ME_FLAG_TABLE_FULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  me_count(part, &a.counts[0]);
}

// grid = ceil(slots / CC_WG), whole waves, one thread per slot
__global__ __launch_bounds__(CC_WG) void k_me_edges(const MeArgs a) {
  const long long s = (long long)blockIdx.x * CC_WG + threadIdx.x;
  int lo = 0, hi = 0;
  const bool edge = s < a.slots && me_slot_edge(a, s, lo, hi);
  int c = 0, t = 0;
  if (edge) {
    c = a.cnt[s];
    t = a.tally[s];
    agent_add(&a.degree[lo], 1);
    agent_add(&a.degree[hi], 1);
    const int bits = (c == 1 ? 1 : 0) | (c > 2 ? 2 : 0);
    if (bits) {
      __hip_atomic_fetch_or(&a.vflags[lo], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_or(&a.vflags[hi], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  me_count(edge, &a.counts[1]);
  me_count(edge && c == 1, &a.counts[2]);
  me_count(edge && c > 2, &a.counts[3]);
  me_count(edge && c == 2 && t != 0, &a.counts[4]);
}

// ---- row offsets -> the adjacency ----

// grid = ceil(slots / CC_WG), one thread per slot.  Which entry of its row an edge gets depends on the interleaving; the row's set of
// entries does not.
__global__ __launch_bounds__(CC_WG) void k_me_fill(const MeArgs a) {
  const long long s = (long long)blockIdx.x * CC_WG + threadIdx.x;
  int lo = 0, hi = 0;
  if (s >= a.slots || !me_slot_edge(a, s, lo, hi)) return;
  const int end[2] = {lo, hi};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int v = end[e];
    const long long b = a.off[v], n = a.off[v + 1];
    const long long at = b + (long long)agent_add(&a.cursor[v], 1);
    if (b >= 0 && at >= b && at < n && n <= a.cap) a.adj[at] = end[1 - e];
  }
}

// ---- one smoothing step ----

// grid = ceil(V / CC_WG), one thread per vertex.  Reads verts only, writes out only: a Jacobi step.
__global__ __launch_bounds__(CC_WG) void k_me_step(const MeArgs a) {
  const long long v = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (v >= a.V || v >= a.max_v) return;
  const unsigned* in = reinterpret_cast<const unsigned*>(a.verts);
  const unsigned bits[3] = {in[v * 3 + 0], in[v * 3 + 1], in[v * 3 + 2]};
  const float p[3] = {__uint_as_float(bits[0]), __uint_as_float(bits[1]), __uint_as_float(bits[2])};
  long long S[3] = {0, 0, 0}, n = 0;
  const bool pinned = a.pin != nullptr && (a.pin[v] & 1) != 0;
  if (finite3(p) && !pinned) {
    long long b = a.off[v], e = a.off[v + 1];
    if (b < 0 || e < b || e > a.cap) b = e = 0;
    for (long long r = b; r < e; ++r) {
      const int j = a.adj[r];
      if ((unsigned)j >= (unsigned)a.V) continue;
      const float pj[3] = {a.verts[(long long)j * 3 + 0], a.verts[(long long)j * 3 + 1], a.verts[(long long)j * 3 + 2]};
      if (!finite3(pj)) continue;
      ++n;
#pragma unroll
      for (int d = 0; d < 3; ++d) S[d] += (long long)__builtin_rint(me_uc(a, pj[d], d) * ME_POS_ONE);
    }
  }
  unsigned* out = reinterpret_cast<unsigned*>(a.out);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    unsigned o = bits[d];  // a vertex that does not move keeps its bits
    if (n > 0) {
      const double mean = (double)a.lo[d] + (double)a.scale * ((double)S[d] / ((double)n * ME_POS_ONE));
      const double pd = (double)p[d];
      o = __float_as_uint((float)(pd + a.w * (mean - pd)));
    }
    out[v * 3 + d] = o;
  }
}

// ---- vertex normals from faces ----

// grid = ceil(F / CC_WG), one thread per face: nine int64 atomics
__global__ __launch_bounds__(CC_WG) void k_me_nrm_accum(const MeArgs a) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  int i[3];
  if (f >= a.F || !me_face(a, f, i)) return;
  double u[3][3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p[3] = {a.verts[(long long)i[c] * 3 + 0], a.verts[(long long)i[c] * 3 + 1], a.verts[(long long)i[c] * 3 + 2]};
    ok = ok && finite3(p);
#pragma unroll
    for (int d = 0; d < 3; ++d) u[c][d] = me_uc(a, p[d], d);
  }
  if (!ok) return;
  double e1[3], e2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e1[d] = u[1][d] - u[0][d];
    e2[d] = u[2][d] - u[0][d];
  }
  const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const long long term = (long long)__builtin_rint(N[d] * ME_NRM_ONE);
    if (term == 0) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) agent_add(&a.T[(long long)i[c] * 3 + d], term);
  }
}

// grid = ceil(V / CC_WG), one thread per vertex
__global__ __launch_bounds__(CC_WG) void k_me_nrm_final(const MeArgs a) {
  const long long v = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (v >= a.V || v >= a.max_v) return;
  const double tx = (double)a.T[v * 3 + 0], ty = (double)a.T[v * 3 + 1], tz = (double)a.T[v * 3 + 2];
  const double len = sqrt((tx * tx + ty * ty) + tz * tz);
  a.out[v * 3 + 0] = len > 0.0 ? (float)(tx / len) : 0.0f;
  a.out[v * 3 + 1] = len > 0.0 ? (float)(ty / len) : 0.0f;
  a.out[v * 3 + 2] = len > 0.0 ? (float)(tz / len) : 0.0f;
}

// ---- launchers ----

hipError_t launch_me_build(const MeArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 8 * sizeof(long long), st));
  TRY(hipMemsetAsync(a.off, 0, ((size_t)a.V + 1) * sizeof(long long), st));  // (V == 0 or F == 0: every row is empty)
  if (a.V == 0) return hipSuccess;  // no face takes part
  TRY(hipMemsetAsync(a.degree, 0, (size_t)a.V * sizeof(int), st));
  TRY(hipMemsetAsync(a.vflags, 0, (size_t)a.V * sizeof(int), st));
  if (a.F == 0) return hipSuccess;
  TRY(hipMemsetAsync(a.keys, 0xFF, (size_t)a.slots * sizeof(long long), st));
  TRY(hipMemsetAsync(a.cnt, 0, (size_t)a.slots * sizeof(int), st));
  TRY(hipMemsetAsync(a.tally, 0, (size_t)a.slots * sizeof(int), st));
  TRY(hipMemsetAsync(a.cursor, 0, (size_t)a.V * sizeof(int), st));
  LAUNCH(k_me_insert, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  LAUNCH(k_me_edges, dim3(grid(a.slots, CC_WG)), dim3(CC_WG), 0, st, a);
  TRY(scan_values<long long>(Degree{a.degree, a.V}, DegWatch{a.counts, {&a.counts[7]}}, RowSink{a.off}, a.V, NO_CAP, a.tot, a.base,
                             a.off + a.V, st));
  LAUNCH(k_me_fill, dim3(grid(a.slots, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_me_step(const MeArgs& a, hipStream_t st) {
  const long long n = a.V < a.max_v ? a.V : a.max_v;
  if (n > 0) LAUNCH(k_me_step, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_me_normals(const MeArgs& a, hipStream_t st) {
  const long long n = a.V < a.max_v ? a.V : a.max_v;
  if (n == 0) return hipSuccess;
  TRY(hipMemsetAsync(a.T, 0, (size_t)a.V * 3 * sizeof(long long), st));
  if (a.F > 0) LAUNCH(k_me_nrm_accum, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  LAUNCH(k_me_nrm_final, dim3(grid(n, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
