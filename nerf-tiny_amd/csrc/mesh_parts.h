// mesh_parts.h -- the device helpers the kernels of indexed meshes and point grids share (mesh_cc.hip, mesh_simplify.hip,
// mesh_smooth.hip, mesh_distance.hip, mesh_raycast.hip, and scan.h's value scan): integer atomics, wave
// reductions, the checks of what is read from memory before it is used, and the sinks that emit a sub-mesh.  No kernel and no launch
// lives here.  Everything has internal linkage: every includer gets its own copy.
#pragma once
#include "kernels.h"

namespace nerf {

namespace {

// ---- relaxed agent-scope integer atomics: counts and fixed-point sums, whose results do not depend on the arrival order ----
__device__ inline int agent_add(int* p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline long long agent_add(long long* p, long long v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline int agent_atomic_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- over the wave's 64 lanes, the result in every lane (integers: the order plays no role) ----
__device__ inline long long wave_sum(long long x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ inline int wave_max(int x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(x, d);
    x = o > x ? o : x;
  }
  return x;
}

__device__ inline bool finite3(const float (&p)[3]) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// a count that an earlier launch left in memory, as a scan takes it: kept inside [0, cap]
__device__ inline long long count_in(const int* cnt, long long i, long long cap) {
  const long long v = cnt[i];
  return v < 0 ? 0 : (v > cap ? cap : v);
}

// ---- a face's corners ----

// the corners of face f -> i[3]; false when one lies outside [0, V), or (DISTINCT) when two of them coincide
template <bool DISTINCT>
__device__ inline bool face_corners(const int* __restrict__ faces, int V, long long f, int (&i)[3]) {
  i[0] = faces[f * 3 + 0], i[1] = faces[f * 3 + 1], i[2] = faces[f * 3 + 2];
  if ((unsigned)i[0] >= (unsigned)V || (unsigned)i[1] >= (unsigned)V || (unsigned)i[2] >= (unsigned)V) return false;  // never used as an address
  return !DISTINCT || (i[0] != i[1] && i[1] != i[2] && i[0] != i[2]);
}

// the same -> the corners' coordinates p[corner][axis]; false as well when a coordinate is not finite
template <bool DISTINCT>
__device__ inline bool face_coords(const float* __restrict__ verts, const int* __restrict__ faces, int V, long long f, float (&p)[3][3]) {
  int i[3];
  if (!face_corners<DISTINCT>(faces, V, f, i)) return false;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int d = 0; d < 3; ++d) p[c][d] = verts[(long long)i[c] * 3 + d];
    ok = ok && finite3(p[c]);
  }
  return ok;
}

// ---- the sinks of scan.h's compaction that emit a sub-mesh: first the kept vertices, then the kept faces (in a later launch: the
// faces read newidx across workgroups).  Each includer brings its own keep flags. ----

// a kept vertex takes its rank as its new index (-1 for a dropped one) and, up to max_v, copies its attributes
struct SubVertSink {
  const float *verts, *normals, *rgb;  // normals / rgb (with their outputs) may be null
  float *out_verts, *out_normals, *out_rgb;
  int* newidx;
  long long max_v;
  __device__ void operator()(long long v, int flag, long long pos) const {
    newidx[v] = flag ? (int)pos : -1;
    if (!flag || pos >= max_v) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      out_verts[pos * 3 + d] = verts[v * 3 + d];
      if (normals) out_normals[pos * 3 + d] = normals[v * 3 + d];
      if (rgb) out_rgb[pos * 3 + d] = rgb[v * 3 + d];
    }
  }
};

// a kept face, up to max_f, is rewritten through newidx (the keep flag has checked its three indices)
struct SubFaceSink {
  const int *faces, *newidx;
  int* out_faces;
  long long max_f;
  __device__ void operator()(long long f, int flag, long long pos) const {
    if (!flag || pos >= max_f) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) out_faces[pos * 3 + d] = newidx[faces[f * 3 + d]];
  }
};

}  // namespace

}  // namespace nerf
