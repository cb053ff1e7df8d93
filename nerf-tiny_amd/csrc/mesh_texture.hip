// mesh_texture.hip -- texture atlases of indexed meshes (nerf_hip_mesh_atlas_texels, nerf_hip_mesh_texture_sample; DESIGN.md section
// 3h-11; the definitions are rules TA and TX of include/nerf_hip.h).
//   k_atlas_texels     per texel of a band of atlas rows: the face that owns it, its integer weights, and from them the surface point
//                      and the viewing direction a shader is asked for
//   k_texture_sample   per lookup (face, u, v): the bilinear mean of the four texels of the face's chart around the point
//
// The atlas is a pure function of (F, n): every face has the same right-isosceles chart in half a cell of c = n + 5 texels, so a texel
// finds its face with two integer divisions by c and one comparison, and a lookup finds its texels with one division by Sx -- no
// table in memory.  c, Sx, W and n travel in the kernel arguments.  One thread per texel with x fastest: a wave's mask store is 64
// consecutive bytes and its point and direction stores 768 consecutive bytes each; the data-dependent reads are the face's three
// indices and its corners' positions and normals, which the 1 + n .. texels of a chart row share.  The indices are range-checked before
// they address anything.  No atomics, no LDS, no barrier: every output is a pure function of the input.
#include "mesh_parts.h"
#include "scan.h"

namespace nerf {

namespace {

// rule TA's weights of the cell-local texel (i, j) of a LOWER chart, as integers over 2n
__device__ inline void atlas_weights(int i, int j, int n, int (&w)[3]) {
  int a = i - 1, b = j - 1;
  if (a >= 0 && b >= 0 && a + b <= n + 1) {  // support: exact, one texel past the hypotenuse on a + b == n + 1 (w0 = -1/n)
    w[0] = 2 * n - 2 * a - 2 * b, w[1] = 2 * a, w[2] = 2 * b;
    return;
  }
  a = a < 0 ? 0 : (a > n ? n : a);  // gutter: the nearest point of the chart
  b = b < 0 ? 0 : (b > n ? n : b);
  if (a + b > n) {
    w[1] = a - b + n, w[2] = b - a + n;
  } else {
    w[1] = 2 * a, w[2] = 2 * b;
  }
  w[0] = 2 * n - w[1] - w[2];
}

}  // namespace

// grid = ceil(T / TEX_WG), T = rows * W < 2^31
__global__ __launch_bounds__(TEX_WG) void k_atlas_texels(const AtlasTexelsArgs a) {
  const long long t = (long long)blockIdx.x * TEX_WG + threadIdx.x;
  if (t >= a.T) return;
  const int x = (int)(t % a.W), y = a.row0 + (int)(t / a.W);
  const int cx = x / a.c, cy = y / a.c;
  int i = x - cx * a.c, j = y - cy * a.c;
  const int upper = i + j >= a.c ? 1 : 0;
  if (upper) i = a.c - 1 - i, j = a.c - 1 - j;  // the point reflection: the rules below are the lower face's
  const long long f = 2 * ((long long)cy * a.Sx + cx) + upper;
  float p[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  unsigned char m = 0;
  int idx[3];
  if (f < a.F && face_corners<false>(a.faces, a.V, f, idx)) {
    m = 1;
    int w[3];
    atlas_weights(i, j, a.n, w);
    float nb[3];
    const int one = w[1] == 0 && w[2] == 0 ? 0 : (w[0] == 0 && w[2] == 0 ? 1 : (w[0] == 0 && w[1] == 0 ? 2 : -1));
    if (one >= 0) {  // the texel sits on a vertex: its position and its normal as they are
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        p[e] = a.verts[(long long)idx[one] * 3 + e];
        nb[e] = a.normals[(long long)idx[one] * 3 + e];
      }
      if (finite3(nb)) {
#pragma unroll
        for (int e = 0; e < 3; ++e) d[e] = -nb[e];
      }
    } else {
      const float den = (float)(2 * a.n);
      const float w0 = (float)w[0] / den, u = (float)w[1] / den, v = (float)w[2] / den;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        p[e] = w0 * a.verts[(long long)idx[0] * 3 + e] + (u * a.verts[(long long)idx[1] * 3 + e] + v * a.verts[(long long)idx[2] * 3 + e]);
        nb[e] = w0 * a.normals[(long long)idx[0] * 3 + e] + (u * a.normals[(long long)idx[1] * 3 + e] + v * a.normals[(long long)idx[2] * 3 + e]);
      }
      const float len = sqrtf((nb[0] * nb[0] + nb[1] * nb[1]) + nb[2] * nb[2]);
      if (isfinite(len) && len > 0.0f) {
#pragma unroll
        for (int e = 0; e < 3; ++e) d[e] = -(nb[e] / len);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    a.points[t * 3 + e] = p[e];
    a.dirs[t * 3 + e] = d[e];
  }
  a.mask[t] = m;
}

// grid = ceil(N / TEX_WG).  Rule TX: all arithmetic fp64, the four texels in the order (dj, di), di fastest, one rounding at the end.
__global__ __launch_bounds__(TEX_WG) void k_texture_sample(const TextureSampleArgs a) {
  const long long q = (long long)blockIdx.x * TEX_WG + threadIdx.x;
  if (q >= a.N) return;
  const int f = a.face[q];
  double u = a.uv[q * 2 + 0], v = a.uv[q * 2 + 1];
  const bool ok = f >= 0 && f < a.F && __builtin_isfinite(u) && __builtin_isfinite(v);
  double acc[3] = {0.0, 0.0, 0.0};
  if (ok) {
    u = fmin(fmax(u, 0.0), 1.0);
    v = fmin(fmax(v, 0.0), 1.0 - u);
    const double tx = 1.0 + u * (double)a.n, ty = 1.0 + v * (double)a.n;  // in texel centres: corner A is texel (1, 1)
    const double fi = fmin(floor(tx), (double)(a.c - 2)), fj = fmin(floor(ty), (double)(a.c - 2));
    const int i0 = (int)fi, j0 = (int)fj;
    const double fx = tx - fi, fy = ty - fj;
    const int k = f >> 1, upper = f & 1;
    const int bx = (k % a.Sx) * a.c, by = (k / a.Sx) * a.c;
#pragma unroll
    for (int dj = 0; dj < 2; ++dj)
#pragma unroll
      for (int di = 0; di < 2; ++di) {
        const double w = (di ? fx : 1.0 - fx) * (dj ? fy : 1.0 - fy);
        if (!(w != 0.0)) continue;  // a texel without weight is not read
        const int i = i0 + di, j = j0 + dj;  // <= c - 1
        const int X = bx + (upper ? a.c - 1 - i : i), Y = by + (upper ? a.c - 1 - j : j);
        const float* __restrict__ px = a.image + ((long long)Y * a.W + X) * 3;
        acc[0] = acc[0] + w * (double)px[0];
        acc[1] = acc[1] + w * (double)px[1];
        acc[2] = acc[2] + w * (double)px[2];
      }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) a.rgb[q * 3 + e] = ok ? (float)acc[e] : a.bg[e];
  a.valid[q] = ok ? 1 : 0;
}

hipError_t launch_atlas_texels(const AtlasTexelsArgs& a, hipStream_t st) {
  if (a.T > 0) LAUNCH(k_atlas_texels, dim3(grid(a.T, TEX_WG)), dim3(TEX_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_texture_sample(const TextureSampleArgs& a, hipStream_t st) {
  if (a.N > 0) LAUNCH(k_texture_sample, dim3(grid(a.N, TEX_WG)), dim3(TEX_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
