// volume_parts.h -- the device helpers the SH radiance volume kernels share (volume.hip: the lookups and the march; volume_grad.hip:
// the march's backward pass; volume_refine.hip: the TV prior; volume_compact.hip and volume_compact_grad.hip: the same lookups through a slot lattice; volume_vq.hip: the importance march; DESIGN.md sections 3h-12 to 3h-17): rule VL's cell, corners and interpolation and rule VS's basis, in the
// fp32 order the rules of include/nerf_hip.h fix.  No kernel and no launch lives here.  Everything has internal linkage: every includer
// gets its own copy.
#pragma once
#include "../../include/nerf_hip.h"
#include "mesh_parts.h"

namespace nerf {

namespace {

constexpr float VOL_INF = __builtin_huge_valf();

__device__ inline float vol_lerp(float a, float b, float f) { return a + f * (b - a); }

// v[di * 4 + dj * 2 + dk]: z first, then y, then x
__device__ inline float vol_tri(const float (&v)[8], const float (&f)[3]) {
  const float c00 = vol_lerp(v[0], v[1], f[2]), c01 = vol_lerp(v[2], v[3], f[2]);
  const float c10 = vol_lerp(v[4], v[5], f[2]), c11 = vol_lerp(v[6], v[7], f[2]);
  return vol_lerp(vol_lerp(c00, c01, f[1]), vol_lerp(c10, c11, f[1]), f[0]);
}

// rule VS's basis at d, in fp32
__device__ inline void vol_basis(const float (&d)[3], float (&Y)[9]) {
  constexpr float C[5] = NERF_HIP_VOLUME_SH_C;  // the header's constants: one copy for the rule, the host tables and this kernel
  constexpr float C0 = C[0], C1 = C[1], C2 = C[2], C3 = C[3], C4 = C[4];
  const float x = d[0], y = d[1], z = d[2];
  Y[0] = C0;
  Y[1] = C1 * y;
  Y[2] = C1 * z;
  Y[3] = C1 * x;
  Y[4] = C2 * (x * y);
  Y[5] = C2 * (y * z);
  Y[6] = C3 * ((3.0f * (z * z)) - 1.0f);
  Y[7] = C2 * (x * z);
  Y[8] = C4 * ((x * x) - (y * y));
}

// rule VL's cell of the point x: is it INSIDE?  ci is clamped into [0, n - 2] whatever x is (a NaN gives 0)
__device__ inline bool vol_cell(const VolLattice& g, const float (&x)[3], int (&ci)[3], float (&f)[3]) {
  const int dim[3] = {g.nx, g.ny, g.nz};
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float gg = (x[a] - g.lo[a]) / g.step[a];
    in = in && 0.0f <= gg && gg <= (float)(dim[a] - 1);
    const float fi = fminf(fmaxf(floorf(gg), 0.0f), (float)(dim[a] - 2));
    ci[a] = (int)fi;
    f[a] = gg - fi;
  }
  return in;
}

// the linear indices of the cell's eight corners, di * 4 + dj * 2 + dk
__device__ inline void vol_corners(const VolLattice& g, const int (&ci)[3], long long (&p)[8]) {
  const long long sy = g.nz, sx = (long long)g.ny * g.nz;
  const long long base = (long long)ci[0] * sx + (long long)ci[1] * sy + ci[2];
#pragma unroll
  for (int c = 0; c < 8; ++c) p[c] = base + (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1);
}

__device__ inline float vol_sigma(const float* __restrict__ sigma, const long long (&p)[8], const float (&f)[3]) {
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = sigma[p[c]];
  return vol_tri(v, f);
}

template <int NC>
__device__ inline void vol_color(const float* __restrict__ coef, const long long (&p)[8], const float (&f)[3], const float (&Y)[9],
                                 float (&rgb)[3]) {
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
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = fminf(fmaxf(vol_tri(v[ch], f), 0.0f), 1.0f);
}

// rule VG's fixed point: llrint(x 2^40) of the product clamped to +-2^62; a NaN adds 0
__device__ inline long long vol_fix(double x) {
  double y = x * (double)(1ll << VOL_GRAD_SHIFT);
  y = fmin(fmax(y, -(double)(1ll << 62)), (double)(1ll << 62));
  return x == x ? llrint(y) : 0ll;
}

// ---- rule VC-L: rule VL's corners taken through the slot lattice (volume_compact.hip) ----

typedef _Float16 volc_half4 __attribute__((ext_vector_type(4)));  // one 8-byte word of an fp16 row

// the corners' rows: the slot where it lies in [0, n), -1 otherwise -- only a checked slot ever becomes an address
__device__ inline void volc_rows(const VolCompact& c, const long long (&p)[8], int (&r)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int s = c.slot[p[k]];
    r[k] = (s >= 0 && (long long)s < c.n) ? s : -1;
  }
}

// an inactive corner has sigma +0
__device__ inline float volc_sigma(const float* __restrict__ sigma_rows, const int (&r)[8], const float (&f)[3]) {
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = r[k] >= 0 ? sigma_rows[r[k]] : 0.0f;
  return vol_tri(v, f);
}

// row r's 3 NC words as fp32 (an fp16 row widened word by word: exact), all +0 for r < 0; the address is formed in 64 bits
template <int NC>
__device__ inline void volc_row(const float* __restrict__ rows, int r, float (&q)[NC * 3]) {
#pragma unroll
  for (int i = 0; i < NC * 3; ++i) q[i] = 0.0f;
  if (r >= 0) {
    const float* __restrict__ w = rows + (long long)r * (NC * 3);
#pragma unroll
    for (int i = 0; i < NC * 3; ++i) q[i] = w[i];
  }
}

template <int NC>
__device__ inline void volc_row(const _Float16* __restrict__ rows, int r, float (&q)[NC * 3]) {
  constexpr int S = vol_half_stride(NC);
#pragma unroll
  for (int i = 0; i < NC * 3; ++i) q[i] = 0.0f;
  if (r >= 0) {
    const volc_half4* __restrict__ w = reinterpret_cast<const volc_half4*>(rows + (long long)r * S);
#pragma unroll
    for (int i = 0; i < S / 4; ++i) {
      const volc_half4 h = w[i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i * 4 + j < NC * 3) q[i * 4 + j] = (float)h[j];
    }
  }
}

// vol_color over rows: the same bracketed sums
template <int NC, class T>
__device__ inline void volc_color(const T* __restrict__ rows, const int (&r)[8], const float (&f)[3], const float (&Y)[9], float (&rgb)[3]) {
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
  for (int ch = 0; ch < 3; ++ch) rgb[ch] = fminf(fmaxf(vol_tri(v[ch], f), 0.0f), 1.0f);
}

}  // namespace

}  // namespace nerf
