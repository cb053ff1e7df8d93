// metrics.hip -- per-view MSE and SSIM of rendered frames against ground truth (nerf_hip_image_metrics):
//   k_metrics_tile   one workgroup per (view, tile of MT_Y x MT_X valid SSIM outputs): the tile's (MT_Y + 10) x (MT_X + 10) x 3 input
//                    patch of both images into LDS once; per channel the horizontal 11-tap pass into five moment rows (mu_x, mu_y,
//                    E[x^2], E[y^2], E[xy]) in LDS, then the vertical pass and the SSIM map; the squared errors of the patch pixels the
//                    tile owns.  Writes the tile's two sums to part[] -- every slot, every call.
//   k_metrics_final  one workgroup per view: the tiles' sums in a fixed order, divided by the counts.
// Everything after the fp32 loads is fp64.  No atomics: the sums' order is fixed by the thread and tile layout, so repeated calls give
// the same bits whatever the workspace held before.
#include "kernels.h"

namespace nerf {

namespace {

constexpr int MT_R = MT_WIN - 1;
constexpr int MT_PW = MT_X + MT_R, MT_PH = MT_Y + MT_R;  // input patch (pixels)
constexpr int MT_VIEWS_PER_LAUNCH_BLOCKS = 1 << 22;     // keeps a launch's work-items below 2^32
constexpr double MT_C1 = 0.01 * 0.01, MT_C2 = 0.03 * 0.03;

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the wave's sum
}

__global__ __launch_bounds__(MT_WG) void k_metrics_tile(const MetricsArgs a, int v0) {
  __shared__ float sx[MT_PH * MT_PW * 3];
  __shared__ float sy[MT_PH * MT_PW * 3];
  __shared__ double hm[5][MT_PH * MT_X];
  __shared__ double red[2][MT_WG / 64];
  const int tid = threadIdx.x;
  const int v = v0 + (int)(blockIdx.x / (unsigned)a.tiles);
  const int t = (int)(blockIdx.x % (unsigned)a.tiles);
  const int r0 = (t / a.tiles_x) * MT_Y, c0 = (t % a.tiles_x) * MT_X;
  const int H = a.H, W = a.W, Ho = H - MT_R, Wo = W - MT_R;
  // the last tile of a row / column also owns the MT_R pixels behind the valid outputs, so every pixel is counted once
  const bool last_y = r0 + MT_Y >= Ho, last_x = c0 + MT_X >= Wo;
  const size_t base = (size_t)v * H * W * 3;
  const float* P = a.pred + base;
  const float* G = a.gt + base;

  double se = 0.0;
  for (int i = tid; i < MT_PH * MT_PW * 3; i += MT_WG) {
    const int r = i / (MT_PW * 3), k = i - r * (MT_PW * 3);
    const int gr = r0 + r, gk = c0 * 3 + k;
    float x = 0.0f, y = 0.0f;
    if (gr < H && gk < W * 3) {  // outside the image: zeros, read only by outputs that are not valid
      const size_t o = (size_t)gr * W * 3 + gk;
      x = P[o];
      y = G[o];
      if ((r < MT_Y || last_y) && (k < MT_X * 3 || last_x)) {
        const double d = (double)x - (double)y;
        se = fma(d, d, se);
      }
    }
    sx[i] = x;
    sy[i] = y;
  }
  __syncthreads();

  double acc = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int i = tid; i < MT_PH * MT_X; i += MT_WG) {  // horizontal pass: every patch row, the tile's MT_X output columns
      const int r = i / MT_X, j = i - r * MT_X;
      const float* px = sx + (r * MT_PW + j) * 3 + ch;
      const float* py = sy + (r * MT_PW + j) * 3 + ch;
      double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
      for (int k = 0; k < MT_WIN; ++k) {
        const double X = px[3 * k], Y = py[3 * k], w = a.g[k];  // products of two fp32 values are exact in fp64
        mx = fma(w, X, mx);
        my = fma(w, Y, my);
        xx = fma(w, X * X, xx);
        yy = fma(w, Y * Y, yy);
        xy = fma(w, X * Y, xy);
      }
      hm[0][i] = mx;
      hm[1][i] = my;
      hm[2][i] = xx;
      hm[3][i] = yy;
      hm[4][i] = xy;
    }
    __syncthreads();
    for (int i = tid; i < MT_Y * MT_X; i += MT_WG) {  // vertical pass and the SSIM map of the valid outputs
      const int r = i / MT_X, j = i - r * MT_X;
      if (r0 + r < Ho && c0 + j < Wo) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MT_WIN; ++k) {
          const double w = a.g[k];
#pragma unroll
          for (int q = 0; q < 5; ++q) m[q] = fma(w, hm[q][(r + k) * MT_X + j], m[q]);
        }
        const double mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
        double sxx = m[2] - mxx, syy = m[3] - myy, sxy = m[4] - mxy;
        sxx = sxx < 0.0 ? 0.0 : sxx;  // written as comparisons so that NaN passes through (fmax would drop it)
        syy = syy < 0.0 ? 0.0 : syy;
        const double lim = sqrt(sxx * syy), axy = fabs(sxy);
        const double mn = axy < lim ? axy : lim;
        sxy = sxy > 0.0 ? mn : (sxy < 0.0 ? -mn : sxy);
        const double num = (2.0 * mxy + MT_C1) * (2.0 * sxy + MT_C2);
        const double den = (mxx + myy + MT_C1) * (sxx + syy + MT_C2);
        acc += num / den;
      }
    }
    __syncthreads();  // (hm is rewritten by the next channel)
  }

  se = wave_sum_f64(se);
  acc = wave_sum_f64(acc);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = se;
    red[1][tid >> 6] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = red[0][0], s1 = red[1][0];
#pragma unroll
    for (int w = 1; w < MT_WG / 64; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
    }
    double* p = a.part + 2 * ((size_t)v * a.tiles + t);
    p[0] = s0;
    p[1] = s1;
  }
}

__global__ __launch_bounds__(MT_WG) void k_metrics_final(const MetricsArgs a, int v0) {
  __shared__ double red[2][MT_WG];
  const int tid = threadIdx.x;
  const int v = v0 + (int)blockIdx.x;
  const double* p = a.part + 2 * (size_t)v * a.tiles;
  double se = 0.0, ss = 0.0;
  for (int t = tid; t < a.tiles; t += MT_WG) {
    se += p[2 * t];
    ss += p[2 * t + 1];
  }
  red[0][tid] = se;
  red[1][tid] = ss;
  __syncthreads();
  for (int s = MT_WG / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.mse[v] = red[0][0] / ((double)a.H * a.W * 3.0);
    a.ssim[v] = red[1][0] / (3.0 * (double)(a.H - MT_R) * (double)(a.W - MT_R));
  }
}

}  // namespace

hipError_t launch_image_metrics(const MetricsArgs& a, hipStream_t st) {
  const int per = MT_VIEWS_PER_LAUNCH_BLOCKS / a.tiles > 0 ? MT_VIEWS_PER_LAUNCH_BLOCKS / a.tiles : 1;  // views per tile launch
  for (int v0 = 0; v0 < a.n; v0 += per) {
    const int nv = a.n - v0 < per ? a.n - v0 : per;
    hipLaunchKernelGGL(k_metrics_tile, dim3((unsigned)nv * (unsigned)a.tiles), dim3(MT_WG), 0, st, a, v0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.n - v0 <= per) break;
  }
  for (int v0 = 0; v0 < a.n; v0 += MT_VIEWS_PER_LAUNCH_BLOCKS) {
    const int nv = a.n - v0 < MT_VIEWS_PER_LAUNCH_BLOCKS ? a.n - v0 : MT_VIEWS_PER_LAUNCH_BLOCKS;
    hipLaunchKernelGGL(k_metrics_final, dim3(nv), dim3(MT_WG), 0, st, a, v0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.n - v0 <= MT_VIEWS_PER_LAUNCH_BLOCKS) break;
  }
  return hipSuccess;
}

}  // namespace nerf
