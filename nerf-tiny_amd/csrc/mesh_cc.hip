// mesh_cc.hip -- connected components of an indexed triangle mesh (nerf_hip_mesh_cc_*; the definition is in
// include/nerf_hip.h): labels, per-component counts and boxes, and the compaction that drops components.
//   k_cc_init        L[v] = v
//   k_cc_hook        per face: the three labels r_k = L[v_k], m = min r_k, atomicMin(&L[r_k], m) for every r_k != m; sets `changed`
//   k_cc_compress    per vertex: walks x = L[x] to the root, halving the path on the way, and leaves the root in L[v]
//   scan.h's k_flag_count / k_flag_scan / k_flag_place   the three-launch compaction over a 0/1 flag per item, instantiated here for
//                    the roots (-> ascending component ids), the kept vertices and the kept faces
//   k_cc_fill / k_cc_faces                vert_comp of the non-roots from their root's id; face_comp
//   k_cc_stats_*     counts and boxes by integer atomics, aggregated inside the wave first
// One round of the labelling is a hook launch and a compress launch; the host reads `changed` after each round and stops at the first
// round that lowered nothing (ops.mesh_components), as density_band drives its rounds.
//
// WHY THE ROUNDS ARE SAFE ON THIS MEMORY SYSTEM (per-XCD L2s that are not coherent inside a launch, L1s that are never refreshed):
//   (I1) L[x] <= x always, and every write to L after k_cc_init is an agent-scope atomicMin, so an entry only ever decreases.  (The
//        path halving uses atomicMin too, not a plain store: a plain store that lost a race against another lane's lower store would
//        RAISE the entry again, and one that landed after the owner's final store would leave the entry uncompressed.)
//   (I2) Every value ever stored in L[x] is x's parent, an older ancestor of x, or its root: a vertex of the same component.  A stale
//        read therefore only yields an older ancestor, never a wrong one.
//   (I3) By (I1) every walk strictly descends and ends after at most x steps, whatever mixture of old and new values it reads.  No
//        kernel waits for another workgroup inside a launch.
//   (I4) A launch boundary makes every earlier write visible.  The roots are fixed during a compress launch (hooks run in the other
//        launch), each owner's walk ends at its true root r, and atomicMin(&L[v], r) leaves L[v] == r because nothing stored there is
//        lower: every round starts fully compressed, so the r_k that k_cc_hook reads are roots.
//   (I5) A hook launch that lowered nothing wrote nothing, so it read one consistent image (I4): every face had three equal labels
//        (an r_k != m that atomicMin did not lower would have been lowered by another lane of the same launch, which then sets
//        `changed`).  Labels are equal only inside a component (I2), so the stopping test is exact.
// Skipping r_k == m keeps a giant component from hammering one address: once it has one root, its faces issue no atomic at all.
// Nothing is placed by atomics; the only atomics are integer min / max / add, whose results do not depend on arrival order.  Every
// index read from memory is checked before it is used as an address, so a wrong argument gives wrong output, never a wild access.
#include "scan.h"

namespace nerf {

namespace {

// the floats' order-preserving unsigned images (ray_parts.h sort_key: -0 keyed as +0); only finite values are keyed here
__device__ inline unsigned cc_key(float x) {
  unsigned b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float cc_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
constexpr unsigned CC_KEY_NONE_LO = 0xFFFFFFFFu, CC_KEY_NONE_HI = 0u;  // the identities of min / max: the image of no finite float

}  // namespace

// ---- labelling ----

// grid = ceil(V / CC_WG)
__global__ __launch_bounds__(CC_WG) void k_cc_init(int* __restrict__ L, int V) {
  const long long v = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (v < V) L[v] = (int)v;
}

// grid = ceil(F / CC_WG), one thread per face
__global__ __launch_bounds__(CC_WG) void k_cc_hook(const int* __restrict__ faces, int V, int F, int* L, int* changed) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (f >= F) return;
  int i[3];
  if (!face_corners<false>(faces, V, f, i)) return;  // takes no part
  const int a = i[0], b = i[1], c = i[2];
  const int ra = L[a], rb = L[b], rc = L[c];
  if ((unsigned)ra > (unsigned)a || (unsigned)rb > (unsigned)b || (unsigned)rc > (unsigned)c) return;  // (I1) holds: never taken
  const int m = min(ra, min(rb, rc));
  bool lowered = false;
  if (ra != m) lowered |= agent_atomic_min(&L[ra], m) > m;
  if (rb != m) lowered |= agent_atomic_min(&L[rb], m) > m;
  if (rc != m) lowered |= agent_atomic_min(&L[rc], m) > m;
  if (lowered) *changed = 1;
}

// grid = ceil(V / CC_WG), one thread per vertex
__global__ __launch_bounds__(CC_WG) void k_cc_compress(int* L, int V) {
  const long long vl = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (vl >= V) return;
  const int v = (int)vl;
  const int p0 = L[v];
  int x = v, p = p0;
  while ((unsigned)p < (unsigned)x) {  // (I3): p < x until the root, where p == x
    const int g = L[p];
    if ((unsigned)g >= (unsigned)p) {
      x = p;
      break;
    }
    agent_atomic_min(&L[x], g);  // halve: x's grandparent becomes its parent
    x = g;
    p = L[x];
  }
  if (x != p0) agent_atomic_min(&L[v], x);
}

// ---- the flags and sinks of scan.h's compaction ----

// the flags (is item i counted?) and sinks (item i, its flag, its rank among the flagged) of the three uses; the sinks of the kept
// vertices and faces are mesh_parts.h's.  k_flag_place recomputes the flags: no launch between the count and the placement writes what
// they read
struct RootFlag {  // v is a root
  const int* L;
  __device__ int operator()(long long i) const { return L[i] == (int)i; }
};
struct RootSink {  // roots take their ids
  int* vert_comp;
  __device__ void operator()(long long i, int flag, long long pos) const {
    if (flag) vert_comp[i] = (int)pos;
  }
};

struct VertKeep {
  const int* vert_comp;
  const unsigned char* keep;
  int C;
  __device__ int operator()(long long i) const {
    const int c = vert_comp[i];
    return (unsigned)c < (unsigned)C && keep[c] != 0;
  }
};
struct FaceKeep {
  const int *faces, *face_comp;
  const unsigned char* keep;
  int V, C;
  __device__ int operator()(long long i) const {
    const int c = face_comp[i];
    if ((unsigned)c >= (unsigned)C || keep[c] == 0) return 0;
    int k[3];
    return face_corners<false>(faces, V, i, k);
  }
};

// grid = ceil(V / CC_WG): the non-roots take their root's id.  Reads only roots' entries of vert_comp (written by the launch before) and
// writes only non-roots' entries.
__global__ __launch_bounds__(CC_WG) void k_cc_fill(const int* __restrict__ L, int V, int* vert_comp) {
  const long long v = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (v >= V) return;
  const int r = L[v];
  if ((unsigned)r < (unsigned)v) vert_comp[v] = vert_comp[r];
}

// grid = ceil(F / CC_WG)
__global__ __launch_bounds__(CC_WG) void k_cc_faces(const int* __restrict__ faces, int V, int F, const int* __restrict__ vert_comp,
                                                    int* __restrict__ face_comp) {
  const long long f = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (f >= F) return;
  int i[3];
  face_comp[f] = face_corners<false>(faces, V, f, i) ? vert_comp[i[0]] : -1;
}

// ---- per-component counts and boxes ----

namespace {

__device__ inline unsigned cc_wave_min(unsigned x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, d));
  return x;
}
__device__ inline unsigned cc_wave_max(unsigned x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, d));
  return x;
}

}  // namespace

// grid = ceil(max_c / CC_WG)
__global__ __launch_bounds__(CC_WG) void k_cc_stats_init(const CcStatsArgs a) {
  const long long c = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (c >= a.max_c) return;
  a.n_verts[c] = 0;
  a.n_faces[c] = 0;
  if (a.lo) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.lo[c * 3 + d] = CC_KEY_NONE_LO;
      a.hi[c * 3 + d] = CC_KEY_NONE_HI;
    }
  }
}

// grid = ceil(n / CC_WG), whole waves.  One atomic per distinct component per wave-instruction: the wave peels off the component of its
// first remaining lane (a wave of a cell-ordered mesh usually holds one), its lanes are counted by a ballot and, BOX, their keys reduced
// across the wave; the leading lane issues the atomics.  BOX = false counts faces, BOX = true counts vertices and bounds them.
template <bool BOX>
__global__ __launch_bounds__(CC_WG) void k_cc_stats(const CcStatsArgs a) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  const long long n = BOX ? a.V : a.F;
  const int lane = threadIdx.x & 63;
  int c = -1;
  if (i < n) c = BOX ? a.vert_comp[i] : a.face_comp[i];
  const bool act = (unsigned)c < (unsigned)a.max_c;  // behind the caller's capacity (and -1 = a face that takes no part)
  unsigned klo[3] = {CC_KEY_NONE_LO, CC_KEY_NONE_LO, CC_KEY_NONE_LO}, khi[3] = {CC_KEY_NONE_HI, CC_KEY_NONE_HI, CC_KEY_NONE_HI};
  if (BOX && a.lo && act) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = a.verts[i * 3 + d];
      if (isfinite(x)) klo[d] = khi[d] = cc_key(x);
    }
  }
  int* const cnt = BOX ? a.n_verts : a.n_faces;
  unsigned long long todo = __ballot(act);
  while (todo) {  // (uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const int lc = __shfl(c, lead);
    const bool mine = act && c == lc;
    const unsigned long long grp = __ballot(mine);
    const int k = __popcll(grp);
    if (lane == lead) atomicAdd(&cnt[lc], k);
    if (BOX && a.lo) {
      unsigned rlo[3], rhi[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        rlo[d] = mine ? klo[d] : CC_KEY_NONE_LO;
        rhi[d] = mine ? khi[d] : CC_KEY_NONE_HI;
        if (k > 1) {  // (uniform)
          rlo[d] = cc_wave_min(rlo[d]);
          rhi[d] = cc_wave_max(rhi[d]);
        }
      }
      if (lane == lead) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (rlo[d] != CC_KEY_NONE_LO) {
            atomicMin(&a.lo[(long long)lc * 3 + d], rlo[d]);
            atomicMax(&a.hi[(long long)lc * 3 + d], rhi[d]);
          }
        }
      }
    }
    todo &= ~grp;
  }
}

// grid = ceil(3 max_c / CC_WG): keys -> floats in place; a component without a finite coordinate keeps (+inf, -inf)
__global__ __launch_bounds__(CC_WG) void k_cc_stats_decode(const CcStatsArgs a) {
  const long long i = (long long)blockIdx.x * CC_WG + threadIdx.x;
  if (i >= a.max_c * 3) return;
  const unsigned l = a.lo[i], h = a.hi[i];
  a.lo[i] = __float_as_uint(l == CC_KEY_NONE_LO ? INFINITY : cc_unkey(l));
  a.hi[i] = __float_as_uint(h == CC_KEY_NONE_HI ? -INFINITY : cc_unkey(h));
}

// ---- launchers ----

hipError_t launch_cc_round(const CcArgs& a, bool first, hipStream_t st) {
  if (first && a.V > 0) LAUNCH(k_cc_init, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a.L, a.V);
  TRY(hipMemsetAsync(a.changed, 0, sizeof(int), st));
  if (a.V == 0 || a.F == 0) return hipSuccess;  // no face can hook anything
  LAUNCH(k_cc_hook, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a.faces, a.V, a.F, a.L, a.changed);
  LAUNCH(k_cc_compress, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a.L, a.V);
  return hipSuccess;
}

hipError_t launch_cc_ids(const CcArgs& a, hipStream_t st) {
  if (a.V == 0) {
    TRY(hipMemsetAsync(a.count, 0, sizeof(long long), st));
  } else {
    TRY(scan_place(RootFlag{a.L}, RootSink{a.vert_comp}, a.V, a.tot, a.base, a.count, st));
    LAUNCH(k_cc_fill, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a.L, a.V, a.vert_comp);
  }
  if (a.F > 0) LAUNCH(k_cc_faces, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a.faces, a.V, a.F, a.vert_comp, a.face_comp);
  return hipSuccess;
}

hipError_t launch_cc_stats(const CcStatsArgs& a, hipStream_t st) {
  if (a.max_c == 0) return hipSuccess;
  LAUNCH(k_cc_stats_init, dim3(grid(a.max_c, CC_WG)), dim3(CC_WG), 0, st, a);
  if (a.V > 0) LAUNCH(k_cc_stats<true>, dim3(grid(a.V, CC_WG)), dim3(CC_WG), 0, st, a);
  if (a.F > 0) LAUNCH(k_cc_stats<false>, dim3(grid(a.F, CC_WG)), dim3(CC_WG), 0, st, a);
  if (a.lo) LAUNCH(k_cc_stats_decode, dim3(grid(a.max_c * 3, CC_WG)), dim3(CC_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_cc_compact(const CcCompactArgs& a, hipStream_t st) {
  TRY(hipMemsetAsync(a.counts, 0, 2 * sizeof(long long), st));
  if (a.V > 0)
    TRY(scan_place(VertKeep{a.vert_comp, a.keep, a.C},
                   SubVertSink{a.verts, a.normals, a.rgb, a.out_verts, a.out_normals, a.out_rgb, a.newidx, a.max_v}, a.V, a.tot, a.base,
                   a.counts, st));
  if (a.F > 0 && a.V > 0)  // (after the vertices' placement: the faces read newidx across workgroups)
    TRY(scan_place(FaceKeep{a.faces, a.face_comp, a.keep, a.V, a.C}, SubFaceSink{a.faces, a.newidx, a.out_faces, a.max_f}, a.F, a.tot,
                   a.base, a.counts + 1, st));
  return hipSuccess;
}

}  // namespace nerf
