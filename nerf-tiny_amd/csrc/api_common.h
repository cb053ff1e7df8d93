// api_common.h -- what the host translation units of the extern "C" surface share (api.hip: render, training, profiling;
// api_geometry.hip: queries, grids, meshes, metrics; api_volume.hip: SH radiance volumes): the error text, the workspace carve-up and the argument checks.
#pragma once
#include "../../include/nerf_hip.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "kernels.h"

namespace nerf {

extern thread_local char g_err[512];  // nerf_hip_last_error's text (defined in api.hip): the last failing call on this thread

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(NERF_HIP_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

template <class T>
T* at(void* ws, size_t off) {
  return reinterpret_cast<T*>(static_cast<unsigned char*>(ws) + off);
}

// carves a workspace into regions of whole 256-byte units: take -> the region's offset, o = the bytes taken so far
struct Carve {
  size_t o = 0;
  size_t take(size_t bytes) {
    const size_t r = o;
    o += al(bytes);
    return r;
  }
};

inline int check_ws(const void* ws, size_t ws_bytes, size_t need) {
  if (!ws) return fail(NERF_HIP_ERR_ARG, "workspace is null");
  if (((uintptr_t)ws & 255) != 0) return fail(NERF_HIP_ERR_ARG, "workspace must be 256-byte aligned");
  if (ws_bytes < need) return fail(NERF_HIP_ERR_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need);
  return NERF_HIP_OK;
}

// a small device output (counts, count, changed): set, and aligned to its element
inline int check_out(const void* p, const char* name, unsigned align) {
  if (!p) return fail(NERF_HIP_ERR_ARG, "%s is null", name);
  if (((uintptr_t)p & (align - 1)) != 0) return fail(NERF_HIP_ERR_ARG, "%s must be %u-byte aligned", name, align);
  return NERF_HIP_OK;
}

inline int check_device() {
  static thread_local int checked_dev = -1;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev == checked_dev) return NERF_HIP_OK;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(NERF_HIP_ERR_ARCH, "device %d is %s; this library is built for gfx950 only", dev, prop.gcnArchName);
  checked_dev = dev;
  return NERF_HIP_OK;
}

inline int check_weights(const float* const* w) {
  if (!w) return fail(NERF_HIP_ERR_ARG, "weights24 is null");
  for (int i = 0; i < 24; ++i) {
    if (!w[i]) return fail(NERF_HIP_ERR_ARG, "weights24[%d] is null", i);
    if (((uintptr_t)w[i] & 15) != 0) return fail(NERF_HIP_ERR_ARG, "weights24[%d] is not 16-byte aligned", i);
  }
  return NERF_HIP_OK;
}

inline Weights24 as_w24(const float* const* w) {
  Weights24 r;
  for (int i = 0; i < 24; ++i) r.p[i] = w[i];
  return r;
}

inline int check_grid(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1) return fail(NERF_HIP_ERR_ARG, "grid %d x %d x %d: every dimension must be positive", nx, ny, nz);
  // the kernels index lattice points with 32-bit integers, as the forward does its samples
  if ((long long)nx * ny * nz >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "grid %d x %d x %d: a grid must stay below 2^31 points", nx, ny, nz);
  return NERF_HIP_OK;
}

inline int check_mesh_sizes(int64_t V, int64_t F) {
  if (V < 0 || F < 0) return fail(NERF_HIP_ERR_ARG, "V=%lld F=%lld: counts must be >= 0", (long long)V, (long long)F);
  // vertex indices are int32, and the kernels index faces with 32-bit integers as well
  if (V >= (1ll << 31) || F >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "V=%lld F=%lld: a mesh must stay below 2^31 vertices and faces", (long long)V, (long long)F);
  return NERF_HIP_OK;
}

// the pointers of a mesh that has vertices / faces
inline int check_mesh_ptrs(const float* verts, const int32_t* faces, int64_t V, int64_t F) {
  if (V > 0 && !verts) return fail(NERF_HIP_ERR_ARG, "verts is null");
  if (F > 0 && !faces) return fail(NERF_HIP_ERR_ARG, "faces is null");
  return NERF_HIP_OK;
}

// the rows the caller's outputs hold
inline int check_cap(const char* name, int64_t cap) {
  if (cap < 0) return fail(NERF_HIP_ERR_ARG, "%s=%lld: a capacity must be >= 0", name, (long long)cap);
  return NERF_HIP_OK;
}
inline int check_caps(int64_t max_v, int64_t max_f) {
  if (max_v < 0 || max_f < 0) return fail(NERF_HIP_ERR_ARG, "max_v=%lld max_f=%lld: capacities must be >= 0", (long long)max_v, (long long)max_f);
  return NERF_HIP_OK;
}

// three finite floats: name[c] as the caller calls them, noun = what they are
inline int check_finite3(const float* p3, const char* name, const char* noun) {
  for (int c = 0; c < 3; ++c)
    if (!isfinite(p3[c])) return fail(NERF_HIP_ERR_ARG, "%s[%d]=%g: %s must be finite", name, c, (double)p3[c], noun);
  return NERF_HIP_OK;
}

}  // namespace nerf
