// volume_vq.hip -- vector-quantised compact SH radiance volumes: per-row importance, a k-means codebook over the coefficient rows, the
// decode back to fp16 rows (nerf_hip_volume_compact_importance and the nerf_hip_volume_vq_* calls; rules VI,
// VQ-A, VQ-U and VQ-D of include/nerf_hip.h).
//   k_volume_compact_importance  per ray: rule VC-R's march without a colour; each contributing sample adds its weight, split by the
//                                trilinear corner terms, to the int64 word of every corner that has a row (rule VI)
//   k_volume_vq_assign<NC>       per row: the nearest code under the fp32 running-sum distance, lowest index first (rule VQ-A)
//   k_volume_vq_accumulate       per (row, word): the weighted fixed-point sums S and N of rule VQ-U
//   k_volume_vq_update           per (code, word): c = (float)(S / N) where N > 0
//   k_volume_vq_decode           per (row, 8-byte word): the fp16 row of a coded / kept / pruned row (rule VQ-D)
//
// THE IMPORTANCE MARCH is ONE MORE COPY of k_volume_compact_march's loop (volume_compact.hip), expression for expression: the slab
// test, t_k = t_a + (k + 0.5) dt, the block byte, the jump of (V4) with its verification, alpha = -expm1f(-(s dt)), w = T alpha,
// T = T - w, the end at t_stop.  What is gone: the rows' colour (nothing reads a coefficient row, so there is no NC and no T
// template), C, D and A.  What is new: eight corner terms in fp64 and up to eight int64 atomics per contributing sample.  With
// volume.hip, volume_grad.hip, volume_compact.hip and volume_compact_grad.hip that makes five copies of the loop; one body over a
// storage policy and a per-sample hook is the follow-up DESIGN.md section 3h-15 names -- not done here, the existing marchers are
// untouched.  steps equals k_volume_compact_march's bit for bit: contributing / evaluated are counted at the same places and every
// branch sees the same fp32 words (sigma_s, T).
//   One ray per lane, workgroups of one wave, no LDS.  The scatter is per lane, NOT the wave scatter of volume_compact_grad.hip: that
//   one exists because a backward sample sends 8 x (3 NC + 1) = up to 224 words and a lane-per-word layout turns them into a few wide
//   instructions; here a sample sends 8 words, a lane-per-word layout would use 8 of 64 lanes per instruction, and the ballot loop,
//   the readlanes and the second pass would cost more than the eight atomics they replace.
//
// THE ASSIGN KERNEL.  One row per lane, its W = 3 NC words in registers (NC is a template parameter: the loops unroll, nothing is
// indexed with a runtime value, no scratch).  The code index j is uniform over the workgroup, so the codebook is staged through LDS
// in tiles of VQ_TILE = 128 codes by all 256 threads and every distance term reads ONE LDS address per wave (a broadcast: no bank
// conflict).  A code is stored at a stride of S = W rounded up to 4 words (4 / 12 / 28) so that its words can be read 16 bytes at a
// time; the tile is 128 x 28 x 4 = 14 KiB at degree 2.  Against the 160 KiB of a CU: eight workgroups of four waves -- the 32 waves a
// CU holds -- take 112 KiB, so LDS does not bound the occupancy; the registers (make asm) decide it.  A larger tile would save
// barriers (two per tile, against 128 x 81 VALU operations between them: under 1 %) and cost occupancy; a smaller one only adds
// barriers.  d_j is the fp32 running sum of t * t in the order w = 0 .. W - 1, each difference, product and sum rounded on its own
// (-ffp-contract=off), so it has one value whatever the machine does; the scan is strict and ascending, so the lowest index wins a tie
// and a NaN distance never wins.  |q|^2 - 2 q.c + |c|^2 through the MFMA units would be several times faster and is NOT built: its
// cancellation and its order of summation make the distances, hence ties and the assignment, depend on the tiling.
// K that is no multiple of the tile: the last tile stages and scans K - j0 codes.  m that is no multiple of the workgroup: the lanes
// past m stage and wait at the barriers with the others, load nothing and store nothing.
//
// Every index that becomes an address is compared with its array's size first: slot[p] against n (volc_rows), assign[r] against K,
// code[.] against K, a rank against its class's count; row and code addresses are formed in 64 bits.
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

// ---- rule VI ----

// grid = ceil(N / VOL_MARCH_WG): one ray per lane.  k_volume_compact_march's loop; the hook at a contributing sample is the scatter.
__global__ __launch_bounds__(VOL_MARCH_WG) void k_volume_compact_importance(const VolImportanceArgs ia) {
  const VolRenderArgs& a = ia.r;
  const long long r = (long long)blockIdx.x * VOL_MARCH_WG + threadIdx.x;
  if (r >= a.N) return;
  const float o[3] = {a.origins[r * 3 + 0], a.origins[r * 3 + 1], a.origins[r * 3 + 2]};
  const float d[3] = {a.dirs[r * 3 + 0], a.dirs[r * 3 + 1], a.dirs[r * 3 + 2]};
  const float tmin = a.tmin[r], tmax = a.tmax[r];
  const int dim[3] = {a.g.nx, a.g.ny, a.g.nz}, nb[3] = {a.bx, a.by, a.bz};
  int contributing = 0, evaluated = 0;
  bool hit = finite3(o) && finite3(d) && isfinite(tmin) && isfinite(tmax);
  float ta = tmin, tb = tmax;
  if (hit) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float hi = a.g.lo[c] + (float)(dim[c] - 1) * a.g.step[c];
      if (d[c] == 0.0f) {
        hit = hit && a.g.lo[c] <= o[c] && o[c] <= hi;
      } else {
        const float t1 = (a.g.lo[c] - o[c]) / d[c], t2 = (hi - o[c]) / d[c];
        ta = fmaxf(ta, fminf(t1, t2));
        tb = fminf(tb, fmaxf(t1, t2));
      }
    }
  }
  hit = hit && ta < tb;
  if (hit) {
    const int K = (int)fminf(ceilf((tb - ta) / a.dt), (float)VOL_MAX_STEPS);
    float T_ = 1.0f;
    int k = 0;
#pragma unroll 1
    while (k < K) {
      const float tk = ta + ((float)k + 0.5f) * a.dt;
      const float x[3] = {o[0] + tk * d[0], o[1] + tk * d[1], o[2] + tk * d[2]};
      int ci[3];
      float f[3];
      ++evaluated;
      int next = k + 1;
      if (vol_cell(a.g, x, ci, f)) {
        int b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = min(ci[c] / a.B, nb[c] - 1);  // (ci >= 0, so b lies in [0, nb))
        if (a.occ[((long long)b[0] * a.by + b[1]) * a.bz + b[2]] != 0) {
          long long p[8];
          int row[8];
          vol_corners(a.g, ci, p);
          volc_rows(ia.c, p, row);
          const float s = volc_sigma(ia.c.sigma_rows, row, f);
          if (s > 0.0f) {
            const float alpha = -expm1f(-(s * a.dt));
            const float w = T_ * alpha;
            // rule VI: rule VG's corner terms in fp64 from the fp32 fractions, times this sample's w
            const double fx = (double)f[0], fy = (double)f[1], fz = (double)f[2], wd = (double)w;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              if (row[c] >= 0) {  // a corner without a row receives nothing; only a checked slot is an address
                const double tw = (((c >> 2) & 1 ? fx : 1.0 - fx) * ((c >> 1) & 1 ? fy : 1.0 - fy)) * (c & 1 ? fz : 1.0 - fz);
                const long long q = vol_fix(tw * wd);
                if (q != 0) agent_add(ia.imp_rows + row[c], q);
              }
            }
            T_ = T_ - w;
            ++contributing;
            if (T_ < a.t_stop) break;
          }
        } else {
          // (V4) the block's range of cells per axis, the exit planes' t (a guess), the candidate, its verification
          int c0[3], c1[3];
          float te = VOL_INF;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const long long up = ((long long)b[c] + 1) * a.B;
            c0[c] = b[c] * a.B;  // <= ci
            c1[c] = up < dim[c] - 1 ? (int)up : dim[c] - 1;
            if (d[c] > 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c1[c] * a.g.step[c]) - o[c]) / d[c]);
            if (d[c] < 0.0f) te = fminf(te, ((a.g.lo[c] + (float)c0[c] * a.g.step[c]) - o[c]) / d[c]);
          }
          const float kf = fminf(floorf((te - ta) / a.dt - 0.5f), (float)(K - 1));  // (fminf drops a NaN)
          int ke = kf > (float)k ? (int)kf : k;
          for (int tries = 0; tries < 2 && ke > k; ++tries, --ke) {
            const float te2 = ta + ((float)ke + 0.5f) * a.dt;
            const float xe[3] = {o[0] + te2 * d[0], o[1] + te2 * d[1], o[2] + te2 * d[2]};
            int ce[3];
            float fe[3];
            if (vol_cell(a.g, xe, ce, fe) && c0[0] <= ce[0] && ce[0] < c1[0] && c0[1] <= ce[1] && ce[1] < c1[1] && c0[2] <= ce[2] &&
                ce[2] < c1[2]) {
              next = ke + 1;
              break;
            }
          }
        }
      }
      k = next;
    }
  }
  a.steps[r * 2 + 0] = contributing;
  a.steps[r * 2 + 1] = evaluated;
}

// ---- rule VQ-A ----

// grid = ceil(m / VQ_WG).  No thread leaves before the last barrier.
template <int NC>
__global__ __launch_bounds__(VQ_WG) void k_volume_vq_assign(const VqAssignArgs a) {
  constexpr int W = 3 * NC, S = (W + 3) & ~3;
  __shared__ __attribute__((aligned(16))) float tile[VQ_TILE * S];
  const long long r = (long long)blockIdx.x * VQ_WG + threadIdx.x;
  const bool live = r < a.m;
  float q[W];
#pragma unroll
  for (int w = 0; w < W; ++w) q[w] = live ? a.rows[r * W + w] : 0.0f;
  float best = VOL_INF;
  int code = 0;
#pragma unroll 1
  for (long long j0 = 0; j0 < a.K; j0 += VQ_TILE) {
    const int nj = (int)(a.K - j0 < VQ_TILE ? a.K - j0 : VQ_TILE);
    __syncthreads();  // the previous tile has been read by every wave
    for (int i = threadIdx.x; i < nj * W; i += VQ_WG) {
      const int j = i / W, w = i - j * W;
      tile[j * S + w] = a.codebook[j0 * W + i];  // (j0 + j) * W + w: the tile's codes are contiguous
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < nj; ++j) {
      const float* __restrict__ c = tile + j * S;
      float t = q[0] - c[0];
      float dsum = t * t;
#pragma unroll
      for (int w = 1; w < W; ++w) {
        t = q[w] - c[w];
        dsum = dsum + t * t;
      }
      if (dsum < best) {  // strict: the lowest index wins a tie; false for a NaN
        best = dsum;
        code = (int)(j0 + j);
      }
    }
  }
  if (live) {
    a.assign[r] = code;
    if (a.dist) a.dist[r] = best;
  }
}

// ---- rule VQ-U ----

// rule VQ-U's fixed point: llrint(x 2^20) of the product clamped to +-2^62; a NaN adds 0
__device__ inline long long vq_fix(double x) {
  double y = x * (double)(1ll << VQ_SHIFT);
  y = fmin(fmax(y, -(double)(1ll << 62)), (double)(1ll << 62));
  return x == x ? llrint(y) : 0ll;
}

// grid = ceil(m (W + 1) / VOL_WG): word W of a row is its count term
__global__ __launch_bounds__(VOL_WG) void k_volume_vq_accumulate(const VqAccumulateArgs a) {
  const long long W = a.words;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.m * (W + 1)) return;
  const long long r = t / (W + 1);
  const int w = (int)(t - r * (W + 1));
  const long long j = a.assign[r];
  if (j < 0 || j >= a.K) return;  // never used as an address
  const double u = (a.weight && a.imax > 0) ? (double)a.weight[r] / (double)a.imax : 1.0;
  if (w < W) {
    const long long v = vq_fix(u * (double)a.rows[r * W + w]);
    if (v != 0) agent_add(a.sum + j * W + w, v);
  } else {
    const long long v = vq_fix(u);
    if (v != 0) agent_add(a.cnt + j, v);
  }
}

// grid = ceil(K W / VOL_WG)
__global__ __launch_bounds__(VOL_WG) void k_volume_vq_update(const VqUpdateArgs a) {
  const long long W = a.words;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.K * W) return;
  const long long n = a.cnt[t / W];
  if (n > 0) a.codebook[t] = (float)((double)a.sum[t] / (double)n);  // an empty code keeps its words
}

// ---- rule VQ-D ----

// grid = ceil(n (S / 4) / VOL_WG): one 8-byte word of an fp16 row
__global__ __launch_bounds__(VOL_WG) void k_volume_vq_decode(const VqDecodeArgs a) {
  const long long Q = a.stride / 4;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.n * Q) return;
  const long long r = t / Q, w = t - r * Q;
  const int cls = a.cls[r];
  const long long k = a.rank[r];
  unsigned long long v = 0ull;  // four +0 halves: a pruned row, and whatever does not check out
  if (cls == 1) {
    if (k >= 0 && k < a.n_coded) {
      const long long j = a.code[k];
      if (j < a.K) v = a.codebook[j * Q + w];
    }
  } else if (cls == 2) {
    if (k >= 0 && k < a.n_kept) v = a.kept[k * Q + w];
  }
  a.out[t] = v;
}

hipError_t launch_volume_compact_importance(const VolImportanceArgs& a, hipStream_t st) {
  if (a.r.N <= 0) return hipSuccess;
  LAUNCH(k_volume_compact_importance, dim3(grid(a.r.N, VOL_MARCH_WG)), dim3(VOL_MARCH_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_vq_assign(const VqAssignArgs& a, int ncoef, hipStream_t st) {
  if (a.m <= 0) return hipSuccess;
  const dim3 g(grid(a.m, VQ_WG)), b(VQ_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_vq_assign<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_vq_assign<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_vq_assign<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_vq_accumulate(const VqAccumulateArgs& a, hipStream_t st) {
  if (a.m <= 0) return hipSuccess;
  LAUNCH(k_volume_vq_accumulate, dim3(grid(a.m * (a.words + 1), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_vq_update(const VqUpdateArgs& a, hipStream_t st) {
  if (a.K <= 0) return hipSuccess;
  LAUNCH(k_volume_vq_update, dim3(grid(a.K * a.words, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_vq_decode(const VqDecodeArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  LAUNCH(k_volume_vq_decode, dim3(grid(a.n * (a.stride / 4), VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
