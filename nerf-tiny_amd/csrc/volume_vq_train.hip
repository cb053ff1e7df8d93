// volume_vq_train.hip -- fine-tuning a vector-quantised SH radiance volume with its assignments frozen: the codebook, the kept rows and
// sigma (nerf_hip_volume_vq_expand, _grad_reduce, _adam_step; rules VQ-X, VQ-G and VQ-V of
// include/nerf_hip.h).  The march and its gradient are volume_compact.hip's and volume_compact_grad.hip's, untouched: they read the
// fp32 rows VQ-X writes and fill the per-row accumulators VQ-G reads.
//   k_volume_vq_expand      per (row, word): the fp32 word of a coded / kept / pruned row from the masters (rule VQ-X)
//   k_volume_vq_reduce<NC>  per chunk of member[]: the rows' int64 accumulator words summed into their codes', and zeroed (rule VQ-G)
//   k_volume_vq_adam        per word of (sigma, kept rows, codebook): rule VU's bracket (rule VQ-V)
//
// THE REDUCE.  The coded rows arrive grouped by code (member[], offset[]).  A workgroup takes VQT_CHUNK = 256 CONSECUTIVE ENTRIES OF
// member[] -- not one (code, chunk) pair: offset[] is device memory, so the host cannot size a grid by the codes' counts without a
// read-back, and a grid of K x (the largest count / chunk) would idle on every skewed codebook.  Cutting member[] itself needs
// ceil(n_coded / 256) workgroups whatever the counts are, launches nothing for an empty code, splits a large code over as many
// workgroups as it needs, and lets a workgroup that meets several small codes visit them in turn.  The first code of a chunk is found
// by a binary search in offset[] (17 uniform steps at K = 65536); the walk ends at the first code that starts past the chunk.
//   Inside a segment (one code's entries inside the chunk) thread t < L W owns word t % W and member lane t / W, L = floor(256 / W)
//   (85 / 21 / 9 lanes at degree 0 / 1 / 2: a fixed eight lanes would leave 40 of 256 threads idle at degree 2 and 232 at degree
//   0).  It walks the segment's members in steps of L with one private int64 sum; a row's 8 W bytes are read by W consecutive
//   threads, each word is zeroed by the thread that read it.  The L partial sums of a word meet in LDS (plain stores), and after ONE
//   barrier W threads add them up and issue one int64 global atomic each.  The LDS buffer alternates between two halves from segment
//   to segment, so the adders of segment s and the writers of segment s + 1 never share a half and the barrier of segment s + 1 orders
//   the adders of s before the writers of s + 2: one barrier per segment, not two.  Everything that steers the walk (the chunk, the
//   offsets, the segment) is uniform over the workgroup, so every thread reaches every barrier.
//   Integers only: the sums are two's-complement adds (formed unsigned: no signed overflow in C++), so acc_code holds the same bits
//   whatever the order of the members, the chunking or the arrival of the atomics.  No float atomic anywhere.
//   BOUNDS.  i lies in [max(a_j, start), min(b_j, end)) with a_j, b_j clamped to [0, n_coded] and end <= n_coded: member[i] is inside
//   the array whatever offset[] holds.  r = member[i] is compared with [0, n) before r W + w is formed (in 64 bits).  j < K.
//
// THE UPDATE restates k_volume_compact_adam's word bracket (volume_compact_grad.hip) expression for expression instead of sharing it
// as a device function: sharing would mean editing that file and trusting the inliner to leave its code object alone; the bracket is
// five lines and -ffp-contract=off gives both copies the same roundings (tests/test_gpu_volume_vq_train.py holds them together bit
// for bit through the identity cases).
#include "../../include/nerf_hip.h"
#include "scan.h"
#include "volume_parts.h"

namespace nerf {

// ---- rule VQ-X ----

// grid = ceil(n W / VOL_WG): one fp32 word of a row
__global__ __launch_bounds__(VOL_WG) void k_volume_vq_expand(const VqExpandArgs a) {
  const long long W = a.words;
  const long long t = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  if (t >= a.n * W) return;
  const long long r = t / W, w = t - r * W;
  const int cls = a.cls[r];
  const long long k = a.rank[r];
  float x = 0.0f;  // +0: a pruned row, and whatever does not check out
  bool zero = true;
  if (cls == 1) {
    if (k >= 0 && k < a.n_coded) {
      const long long j = a.code[k];
      if (j < a.K) {
        x = a.codebook32[j * W + w];
        zero = false;
      }
    }
  } else if (cls == 2) {
    if (k >= 0 && k < a.n_kept) {
      x = a.kept32[k * W + w];
      zero = false;
    }
  }
  a.out[t] = x;
  if (zero && a.acc_coef_rows) a.acc_coef_rows[t] = 0;  // nothing else consumes the accumulator words of such a row
}

// ---- rule VQ-G ----

__device__ inline long long vqt_clamp(long long x, long long lo, long long hi) { return x < lo ? lo : (x > hi ? hi : x); }

// grid = ceil(n_coded / VQT_CHUNK).  No thread leaves before the last barrier.
template <int NC>
__global__ __launch_bounds__(VQT_WG) void k_volume_vq_reduce(const VqReduceArgs a) {
  constexpr int W = 3 * NC, L = VQT_WG / W;
  __shared__ long long part[2][L * W];
  const int t = threadIdx.x;
  const int lane = t / W, w = t - lane * W;
  const bool active = t < L * W;
  const long long start = (long long)blockIdx.x * VQT_CHUNK;
  const long long end = start + VQT_CHUNK < a.n_coded ? start + VQT_CHUNK : a.n_coded;
  // the last code whose (clamped) first entry is <= start: the codes before it end at or before start, or are empty
  long long lo = 0, hi = a.K - 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (vqt_clamp(a.offset[mid], 0, a.n_coded) <= start) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  int buf = 0;
#pragma unroll 1
  for (long long j = lo; j < a.K; ++j) {
    const long long aj = vqt_clamp(a.offset[j], 0, a.n_coded);
    if (aj >= end) break;  // this code and (ascending offsets) every later one start past the chunk
    const long long bj = vqt_clamp(a.offset[j + 1], aj, a.n_coded);
    const long long s0 = aj > start ? aj : start, s1 = bj < end ? bj : end;
    if (s0 >= s1) continue;  // an empty code, or one that ended before the chunk
    unsigned long long sum = 0ull;
    if (active) {
#pragma unroll 4
      for (long long i = s0 + lane; i < s1; i += L) {
        const long long r = a.member[i];
        if (r >= 0 && r < a.n) {  // a member outside the rows is skipped: never an address
          long long* p = a.acc_coef_rows + r * W + w;
          sum += (unsigned long long)*p;
          *p = 0;
        }
      }
      part[buf][t] = (long long)sum;
    }
    __syncthreads();
    if (t < W) {
      const int nl = s1 - s0 < L ? (int)(s1 - s0) : L;  // the lanes past the segment hold 0
      unsigned long long s = 0ull;
      for (int l = 0; l < nl; ++l) s += (unsigned long long)part[buf][l * W + t];
      if (s != 0ull) agent_add(a.acc_code + j * W + t, (long long)s);
    }
    buf ^= 1;
  }
}

// ---- rule VQ-V ----

// grid = ceil((n + n_kept W + K W) / VOL_WG): one word of (sigma | kept rows | codebook), the moments in that order
__global__ __launch_bounds__(VOL_WG) void k_volume_vq_adam(const VqAdamArgs a) {
  const long long W = a.words;
  const long long i = (long long)blockIdx.x * VOL_WG + threadIdx.x;
  const long long nk = a.n_kept * W;
  if (i >= a.n + nk + a.K * W) return;
  float* xp;
  long long* ap;
  const bool sigma = i < a.n;
  if (sigma) {
    xp = a.sigma_rows + i;
    ap = a.acc_sigma_rows + i;
  } else if (i < a.n + nk) {
    const long long q = i - a.n, k = q / W, w = q - k * W;
    const long long r = a.kept_row[k];
    if (r < 0 || r >= a.n) return;  // never an address: the words of such a kept row are left alone
    xp = a.kept32 + q;
    ap = a.acc_coef_rows + r * W + w;
  } else {
    const long long q = i - a.n - nk;
    xp = a.codebook32 + q;
    ap = a.acc_code + q;
  }
  const long long acc = *ap;
  *ap = 0;
  const float x = *xp;
  if (sigma && !(x > 0.0f)) return;  // dead: x, m and v are left alone
  const double lr = sigma ? a.lr_sigma : a.lr_coef;
  const double g = ((double)acc * (1.0 / (double)(1ll << VOL_GRAD_SHIFT))) * a.grad_scale;
  const float m1 = (float)(a.beta1 * (double)a.m[i] + (1.0 - a.beta1) * g);
  const float v1 = (float)(a.beta2 * (double)a.v[i] + (1.0 - a.beta2) * (g * g));
  float x1 = (float)((double)x - lr * (((double)m1 / a.c1) / (sqrt((double)v1 / a.c2) + a.eps)));
  if (sigma) x1 = fmaxf(x1, 0.0f);
  a.m[i] = m1;
  a.v[i] = v1;
  *xp = x1;
}

hipError_t launch_volume_vq_expand(const VqExpandArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  LAUNCH(k_volume_vq_expand, dim3(grid(a.n * a.words, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_volume_vq_grad_reduce(const VqReduceArgs& a, int ncoef, hipStream_t st) {
  if (a.n_coded <= 0 || a.K <= 0) return hipSuccess;
  const dim3 g(grid(a.n_coded, VQT_CHUNK)), b(VQT_WG);
  if (ncoef == 1) {
    LAUNCH(k_volume_vq_reduce<1>, g, b, 0, st, a);
  } else if (ncoef == 4) {
    LAUNCH(k_volume_vq_reduce<4>, g, b, 0, st, a);
  } else {
    LAUNCH(k_volume_vq_reduce<9>, g, b, 0, st, a);
  }
  return hipSuccess;
}

hipError_t launch_volume_vq_adam_step(const VqAdamArgs& a, hipStream_t st) {
  const long long words = a.n + (a.n_kept + a.K) * a.words;
  if (words > 0) LAUNCH(k_volume_vq_adam, dim3(grid(words, VOL_WG)), dim3(VOL_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
