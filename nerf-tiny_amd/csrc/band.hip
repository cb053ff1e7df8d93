// band.hip -- the bookkeeping of the narrow-band density grid (nerf_hip_band_begin / nerf_hip_band_grow).
// The lattice is cut into blocks of r^3 points; the field itself is evaluated by k_field_fwd_reg's SRC_CORNERS / SRC_BLOCKS forms.
//   k_band_seed      per block: seed[b] = its 8 corner samples are not all of one class; active[b] = 0
//   k_band_fill      per lattice point: the value of its block's lowest point (which is a corner sample)
//   k_band_new       per block: new = not active and a seed in its 27-neighbourhood; in-workgroup exclusive offsets, workgroup totals
//   k_band_scan      one workgroup: exclusive scan of the workgroup totals (scan.h scan_totals: the new blocks with bases, the points
//                    as a totals-only channel); counts = {new blocks, the points they own}
//   k_band_list      list[base + offset] = b for the new blocks (ascending block order), active[b] = 1
//   k_band_reseed    one wave per block: seed[b] = active, an in-grid 26-neighbour is not, and b owns a corner of a mixed cell
// The list's order is fixed by the scans -- no atomic places anything -- and no kernel reads, across workgroups, what the same launch
// writes: new / list / reseed are separate launches (DESIGN.md section 3h gives the reason).  Inside means sigma > level, NaN outside.
#include "scan.h"

namespace nerf {

namespace {

struct Blk {
  int x, y, z;
};

__device__ inline Blk blk_decode(int b, int nby, int nbz) {
  const unsigned yz = (unsigned)nby * (unsigned)nbz;
  Blk q;
  q.x = (int)((unsigned)b / yz);
  const unsigned rem = (unsigned)b - (unsigned)q.x * yz;
  q.y = (int)(rem / (unsigned)nbz);
  q.z = (int)(rem - (unsigned)q.y * (unsigned)nbz);
  return q;
}

// corner plane c_a(b) = min(b r, n - 1)
__device__ inline int corner_at(int b, int r, int n) {
  const unsigned c = (unsigned)b * (unsigned)r;
  return c < (unsigned)(n - 1) ? (int)c : n - 1;
}

// points block b owns along an axis of n points
__device__ inline int owned_along(int b, int r, int n) {
  const long long lo = (long long)b * r, hi = lo + r;
  return (int)((hi < n ? hi : n) - lo);
}

__device__ inline bool cell_mixed(const float* __restrict__ s, size_t p, size_t X, size_t Y, float level) {
  int n = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) n += (s[p + ((c & 1) ? X : 0) + ((c & 2) ? Y : 0) + ((c & 4) ? 1 : 0)] > level) ? 1 : 0;
  return n != 0 && n != 8;
}

}  // namespace

// grid = ceil(nblk / BAND_WG) workgroups of BAND_WG
__global__ __launch_bounds__(BAND_WG) void k_band_seed(const BandArgs a) {
  const long long bl = (long long)blockIdx.x * BAND_WG + threadIdx.x;
  if (bl >= a.nblk) return;
  const int b = (int)bl;
  const Blk q = blk_decode(b, a.nby, a.nbz);
  const int cx[2] = {corner_at(q.x, a.r, a.nx), corner_at(q.x + 1, a.r, a.nx)};
  const int cy[2] = {corner_at(q.y, a.r, a.ny), corner_at(q.y + 1, a.r, a.ny)};
  const int cz[2] = {corner_at(q.z, a.r, a.nz), corner_at(q.z + 1, a.r, a.nz)};
  int n = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) n += (a.sigma[((size_t)cx[c & 1] * a.ny + cy[(c >> 1) & 1]) * a.nz + cz[c >> 2]] > a.level) ? 1 : 0;
  a.seed[b] = (n != 0 && n != 8) ? 1 : 0;
  a.active[b] = 0;
}

// grid = ceil(N / BAND_WG).  Only lowest points are read and only other points are written: no point is both in one launch.
__global__ __launch_bounds__(BAND_WG) void k_band_fill(const BandArgs a) {
  const long long pl = (long long)blockIdx.x * BAND_WG + threadIdx.x;
  if (pl >= (long long)a.nx * a.ny * a.nz) return;
  const unsigned p = (unsigned)pl, nynz = (unsigned)a.ny * (unsigned)a.nz, r = (unsigned)a.r;
  const unsigned i = p / nynz, rem = p - i * nynz;
  const unsigned j = rem / (unsigned)a.nz, k = rem - j * (unsigned)a.nz;
  const unsigned low = ((i / r) * r * (unsigned)a.ny + (j / r) * r) * (unsigned)a.nz + (k / r) * r;
  if (low != p) a.sigma[p] = a.sigma[low];
}

// grid = nwg = ceil(nblk / BAND_WG)
__global__ __launch_bounds__(BAND_WG) void k_band_new(const BandArgs a) {
  __shared__ int part[BAND_WG / 64];
  __shared__ long long ppart[BAND_WG / 64];
  const long long bl = (long long)blockIdx.x * BAND_WG + threadIdx.x;
  const int b = (int)bl;
  int flag = 0;
  long long pts = 0;
  if (bl < a.nblk && !a.active[b]) {
    const Blk q = blk_decode(b, a.nby, a.nbz);
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dz = -1; dz <= 1; ++dz) {
          const int x = q.x + dx, y = q.y + dy, z = q.z + dz;
          if (x < 0 || y < 0 || z < 0 || x >= a.nbx || y >= a.nby || z >= a.nbz) continue;
          flag |= a.seed[((size_t)x * a.nby + y) * a.nbz + z];
        }
    if (flag) pts = (long long)owned_along(q.x, a.r, a.nx) * owned_along(q.y, a.r, a.ny) * owned_along(q.z, a.r, a.nz);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) pts += __shfl_xor(pts, d);
  if (lane == 0) ppart[wave] = pts;  // (published by wg_prefix's first barrier)
  int total;
  const int pre = wg_prefix<BAND_WG, 1>(flag, part, total);
  long long ptot = 0;
#pragma unroll
  for (int w = 0; w < BAND_WG / 64; ++w) ptot += ppart[w];
  if (bl < a.nblk) a.offs[b] = ((unsigned)pre << 1) | (unsigned)flag;
  if (threadIdx.x == 0) {
    a.tn[blockIdx.x] = total;
    a.tp[blockIdx.x] = ptot;
  }
}

// one workgroup of 1024
__global__ __launch_bounds__(1024) void k_band_scan(const BandArgs a) {
  long long n[2];  // new blocks, the points they own (no bases: the total only)
  scan_totals(a.nwg, n, Totals<int, int>{a.tn, a.bn}, Totals<long long, long long>{a.tp, nullptr});
  if (threadIdx.x == 1023) {
    a.counts[0] = n[0];
    a.counts[1] = n[1];
  }
}

// grid = nwg
__global__ __launch_bounds__(BAND_WG) void k_band_list(const BandArgs a) {
  const long long bl = (long long)blockIdx.x * BAND_WG + threadIdx.x;
  if (bl >= a.nblk) return;
  const int b = (int)bl;
  const unsigned w = a.offs[b];
  if (w & 1u) {
    a.list[a.bn[blockIdx.x] + (int)(w >> 1)] = b;  // (at most nblk new blocks: the index stays inside list[nblk])
    a.active[b] = 1;
  }
}

// grid = nblk workgroups of ONE wave, one per block; reads active and sigma, writes seed
__global__ __launch_bounds__(64) void k_band_reseed(const BandArgs a) {
  const int b = blockIdx.x;
  if (!a.active[b]) return;  // (uniform; its seed is 0: a seed becomes active in the round it is dilated)
  const Blk q = blk_decode(b, a.nby, a.nbz);
  int open = 0;
  if (threadIdx.x < 27) {
    const int x = q.x + (int)threadIdx.x / 9 - 1, y = q.y + ((int)threadIdx.x / 3) % 3 - 1, z = q.z + (int)threadIdx.x % 3 - 1;
    if (x >= 0 && y >= 0 && z >= 0 && x < a.nbx && y < a.nby && z < a.nbz) open = !a.active[((size_t)x * a.nby + y) * a.nbz + z];
  }
  if (__ballot(open) == 0) {  // every in-grid neighbour is active: nothing to grow into
    if (threadIdx.x == 0) a.seed[b] = 0;
    return;
  }
  // the cells with a corner among the block's points: lowest corner from one below the block's first point to its last point
  const int n[3] = {a.nx, a.ny, a.nz}, bq[3] = {q.x, q.y, q.z};
  int c0[3], ext[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const long long first = (long long)bq[d] * a.r;
    const long long last = first + owned_along(bq[d], a.r, n[d]) - 1;
    c0[d] = (int)(first > 0 ? first - 1 : 0);
    const long long c1 = last < n[d] - 2 ? last : n[d] - 2;
    ext[d] = (int)(c1 - c0[d] + 1);
  }
  int found = 0;
  if (ext[0] > 0 && ext[1] > 0 && ext[2] > 0) {
    const int total = ext[0] * ext[1] * ext[2];
    const size_t X = (size_t)a.ny * a.nz, Y = (size_t)a.nz;
    for (int t0 = 0; t0 < total && !found; t0 += 64) {  // (found is uniform: the wave stops at the first round with a mixed cell)
      const int t = t0 + (int)threadIdx.x;
      int mine = 0;
      if (t < total) {
        const int k = t % ext[2], ij = t / ext[2];
        const int j = ij % ext[1], i = ij / ext[1];
        mine = cell_mixed(a.sigma, (size_t)(c0[0] + i) * X + (size_t)(c0[1] + j) * Y + (size_t)(c0[2] + k), X, Y, a.level) ? 1 : 0;
      }
      found = __ballot(mine) != 0;
    }
  }
  if (threadIdx.x == 0) a.seed[b] = found ? 1 : 0;
}

hipError_t launch_band_begin(const BandArgs& a, hipStream_t st) {
  const long long N = (long long)a.nx * a.ny * a.nz;
  LAUNCH(k_band_seed, dim3(a.nwg), dim3(BAND_WG), 0, st, a);
  LAUNCH(k_band_fill, dim3(grid(N, BAND_WG)), dim3(BAND_WG), 0, st, a);
  return hipSuccess;
}

hipError_t launch_band_reseed(const BandArgs& a, hipStream_t st) {
  LAUNCH(k_band_reseed, dim3(a.nblk), dim3(64), 0, st, a);
  return hipSuccess;
}

hipError_t launch_band_next(const BandArgs& a, hipStream_t st) {
  LAUNCH(k_band_new, dim3(a.nwg), dim3(BAND_WG), 0, st, a);
  LAUNCH(k_band_scan, dim3(1), dim3(1024), 0, st, a);
  LAUNCH(k_band_list, dim3(a.nwg), dim3(BAND_WG), 0, st, a);
  return hipSuccess;
}

}  // namespace nerf
