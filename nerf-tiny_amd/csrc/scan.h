// scan.h -- the scan and compaction scaffolding of the geometry kernels.  Included by the geometry translation
// units only -- the mesh_*.hip files, mesh.hip, band.hip, tsdf.hip, volume.hip and volume_grad.hip --, never by a render or training one.
//   lane_prefix / wg_prefix     exclusive prefix of a small per-lane count inside the wave / the workgroup, in item order
//   wg_prefix_sum               the same for a value of any size (weights, per-cell counts) across a workgroup of CC_WG
//   Totals / scan_totals        channels of workgroup totals -> exclusive bases and the grand totals, by ONE workgroup of 1024
//   k_flag_count / k_flag_scan / k_flag_place   compaction over a 0/1 flag per item in three launches: totals per workgroup of CC_PTS
//                               items, the scan of the totals, then the placement (scan_count: the first two, scan_place: all three)
//   k_value_sum / k_flag_scan / k_value_place   the same three launches over an integer value per item: every item's exclusive prefix
//                               (scan_values); cells_to_start: per-cell counts -> start[], the middle of a counting sort by cell
// The output order is fixed by the scans -- no atomic places anything -- and the scan is three kernels, never a single-pass look-back:
// no flag crosses workgroups (or XCDs) inside a launch.  Everything here has internal linkage: every includer gets its own copy.
#pragma once
#include "mesh_parts.h"

#define LAUNCH(...)                               \
  do {                                            \
    hipLaunchKernelGGL(__VA_ARGS__);              \
    const hipError_t e_ = hipGetLastError();      \
    if (e_ != hipSuccess) return e_;              \
  } while (0)
#define TRY(x)                                    \
  do {                                            \
    const hipError_t e_ = (x);                    \
    if (e_ != hipSuccess) return e_;              \
  } while (0)

namespace nerf {

namespace {

inline unsigned grid(long long n, int wg) { return (unsigned)((n + wg - 1) / wg); }

// lanes below this one whose bit is set in the ballot m
__device__ inline unsigned lane_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Exclusive prefix of a small per-lane count (bits 0 .. NBITS-1; NBITS = 1: a 0/1 flag) across the WG / 64 waves of the workgroup, in
// item order, plus the workgroup's total.  Uses part[0 .. WG / 64) of LDS; ends with a barrier so part can be reused.
template <int WG, int NBITS>
__device__ inline int wg_prefix(int v, int* part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int pre = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    const unsigned long long m = __ballot((v >> b) & 1);
    pre += (int)lane_prefix(m) << b;
    tot += __popcll(m) << b;
  }
  if (lane == 0) part[wave] = tot;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WG / 64; ++w) {
    const int t = part[w];
    before += (w < wave) ? t : 0;
    total += t;
  }
  __syncthreads();
  return before + pre;
}

// Exclusive prefix of v across a workgroup of CC_WG in thread order, plus the workgroup's total; part[CC_WG / 64] of LDS, ends with a
// barrier.
template <class T>
__device__ inline T wg_prefix_sum(T v, T* part, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) part[wave] = x;
  __syncthreads();
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < CC_WG / 64; ++w) {
    const T t = part[w];
    before += (w < wave) ? t : 0;
    total += t;
  }
  __syncthreads();
  return before + x - v;
}

// One channel of the scan of workgroup totals: tot [nb] -> base [nb], base[b] = the sum of tot[0 .. b) (base null: the grand total only)
template <class T, class B>
struct Totals {
  const T* tot;
  B* base;
  __device__ void store(int b, long long e) const {
    if (base) base[b] = (B)e;
  }
};

// The channels' totals scanned by one workgroup of 1024: thread t sums a contiguous run of per = ceil(nb / 1024) totals, the runs are
// joined by an LDS scan, and each thread stores its run's bases.  The channels go through every step together (one pass over the
// totals, one over LDS).  total[c] = channel c's grand total, in every thread; ends with a barrier.
template <class... C>
__device__ inline void scan_totals(int nb, long long (&total)[sizeof...(C)], const C&... ch) {
  constexpr int N = sizeof...(C);
  __shared__ long long s[N][1024];
  const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per;
  long long t[N] = {};
  for (int q = 0; q < per; ++q) {
    const int b = b0 + q;
    if (b < nb) {
      int c = 0;
      ((t[c++] += ch.tot[b]), ...);
    }
  }
#pragma unroll
  for (int c = 0; c < N; ++c) s[c][threadIdx.x] = t[c];
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
    long long x[N];
#pragma unroll
    for (int c = 0; c < N; ++c) x[c] = threadIdx.x >= d ? s[c][threadIdx.x - d] : 0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) s[c][threadIdx.x] += x[c];
    __syncthreads();
  }
  long long e[N];
#pragma unroll
  for (int c = 0; c < N; ++c) e[c] = s[c][threadIdx.x] - t[c];
  for (int q = 0; q < per; ++q) {
    const int b = b0 + q;
    if (b < nb) {
      int c = 0;
      ((ch.store(b, e[c]), e[c++] += ch.tot[b]), ...);
    }
  }
#pragma unroll
  for (int c = 0; c < N; ++c) total[c] = s[c][1023];
  __syncthreads();
}

// ---- compaction over a flag per item: Flag = is item i counted?, Sink = (item i, its flag, its rank among the flagged) ----

// grid = nb = cc_blocks(n)
template <class Flag>
__global__ __launch_bounds__(CC_WG) void k_flag_count(const Flag flag, long long n, int* __restrict__ tot) {
  __shared__ int part[CC_WG / 64];
  const long long base = (long long)blockIdx.x * CC_PTS;
  int run = 0;
  for (int r = 0; r < CC_ROUNDS; ++r) {
    const long long i = base + r * CC_WG + threadIdx.x;
    int total;
    (void)wg_prefix<CC_WG, 1>(i < n ? flag(i) : 0, part, total);
    run += total;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = run;
}

// one workgroup of 1024 (a template, so that only the includers that launch it carry it)
template <class T, class B>
__global__ __launch_bounds__(1024) void k_flag_scan(const T* __restrict__ tot, B* __restrict__ base, int nb, long long* count) {
  long long total[1];
  scan_totals(nb, total, Totals<T, B>{tot, base});
  if (threadIdx.x == 1023) *count = total[0];
}

// grid = nb.  The flags are recomputed, not stored: between the count launch and this one nothing may change whether an item is
// flagged (each includer says at its Flag / Sink structs why that holds).
template <class Flag, class Sink>
__global__ __launch_bounds__(CC_WG) void k_flag_place(const Flag flag, const Sink sink, long long n, const int* __restrict__ bases) {
  __shared__ int part[CC_WG / 64];
  const long long base = (long long)blockIdx.x * CC_PTS;
  long long run = bases[blockIdx.x];
  for (int r = 0; r < CC_ROUNDS; ++r) {
    const long long i = base + r * CC_WG + threadIdx.x;
    const int fl = i < n ? flag(i) : 0;
    int total;
    const int pre = wg_prefix<CC_WG, 1>(fl, part, total);
    if (i < n) sink(i, fl, run + pre);
    run += total;
  }
}

// tot, base: [cc_blocks(n)]; *count = the flagged items
template <class Flag>
hipError_t scan_count(const Flag& flag, long long n, int* tot, int* base, long long* count, hipStream_t st) {
  const int nb = cc_blocks(n);
  LAUNCH((k_flag_count<Flag>), dim3(nb), dim3(CC_WG), 0, st, flag, n, tot);
  LAUNCH((k_flag_scan<int, int>), dim3(1), dim3(1024), 0, st, tot, base, nb, count);  // (at most n < 2^31 items are flagged: int bases)
  return hipSuccess;
}

template <class Flag, class Sink>
hipError_t scan_place(const Flag& flag, const Sink& sink, long long n, int* tot, int* base, long long* count, hipStream_t st) {
  TRY(scan_count(flag, n, tot, base, count, st));
  LAUNCH((k_flag_place<Flag, Sink>), dim3(cc_blocks(n)), dim3(CC_WG), 0, st, flag, sink, n, base);
  return hipSuccess;
}

// ---- the scan of a value per item: Value = item i -> a non-negative integer, Watch = sees every value of the sum pass (all lanes
// reach it in every round, with 0 past the end), Sink = (item i, its value, the sum of the values before it) and end(the sum of all).
// The sums run in 64 bits inside a workgroup; the totals, the bases and what the sink sees are kept at or below cap (NO_CAP: none). ----

constexpr long long NO_CAP = 0x7FFFFFFFFFFFFFFFll;

struct NoWatch {
  __device__ void operator()(long long) {}
  __device__ void done() {}
};
// the largest value (below 2^31) into *most by an integer atomic; most may be null
struct WatchMax {
  long long* most;
  int top = 0;
  __device__ void operator()(long long v) { top = (int)v > top ? (int)v : top; }
  __device__ void done() {
    if (!most) return;
    top = wave_max(top);
    if ((threadIdx.x & 63) == 0 && top > 0) __hip_atomic_fetch_max(most, (long long)top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// grid = nb = cc_blocks(n)
template <class T, class Value, class Watch>
__global__ __launch_bounds__(CC_WG) void k_value_sum(const Value value, Watch watch, long long n, long long cap, T* __restrict__ tot) {
  __shared__ long long part[CC_WG / 64];
  const long long base = (long long)blockIdx.x * CC_PTS;
  long long run = 0;
  for (int r = 0; r < CC_ROUNDS; ++r) {
    const long long i = base + r * CC_WG + threadIdx.x;
    const long long v = i < n ? (long long)value(i) : 0;
    long long total;
    (void)wg_prefix_sum<long long>(v, part, total);
    run += total;
    watch(v);
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = (T)(run > cap ? cap : run);
  watch.done();
}

// grid = nb.  The values are recomputed, not stored: between the sum launch and this one nothing may change them (a sink may change
// its own item's once it has been read).
template <class T, class Value, class Sink>
__global__ __launch_bounds__(CC_WG) void k_value_place(const Value value, const Sink sink, long long n, long long cap, const T* __restrict__ bases) {
  __shared__ long long part[CC_WG / 64];
  const long long base = (long long)blockIdx.x * CC_PTS;
  long long run = bases[blockIdx.x];
  for (int r = 0; r < CC_ROUNDS; ++r) {
    const long long i = base + r * CC_WG + threadIdx.x;
    const long long v = i < n ? (long long)value(i) : 0;
    long long total;
    const long long pre = wg_prefix_sum<long long>(v, part, total);
    if (i < n) sink(i, v, run + pre > cap ? cap : run + pre);
    run += total;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) sink.end(run > cap ? cap : run);
}

// tot, base: [cc_blocks(n)] of T; *count = the sum of the workgroups' (capped) totals
template <class T, class Value, class Watch, class Sink>
hipError_t scan_values(const Value& value, const Watch& watch, const Sink& sink, long long n, long long cap, T* tot, T* base,
                       long long* count, hipStream_t st) {
  const int nb = cc_blocks(n);
  LAUNCH((k_value_sum<T, Value, Watch>), dim3(nb), dim3(CC_WG), 0, st, value, watch, n, cap, tot);
  LAUNCH((k_flag_scan<T, T>), dim3(1), dim3(1024), 0, st, tot, base, nb, count);
  LAUNCH((k_value_place<T, Value, Sink>), dim3(nb), dim3(CC_WG), 0, st, value, sink, n, cap, base);
  return hipSuccess;
}

// ---- the middle of a counting sort by cell: between the caller's count launch, which left cnt[c] items in cell c, and its place
// launch, which takes cnt as the cells' cursors ----

struct CellCount {
  const int* cnt;
  long long cap;
  __device__ long long operator()(long long c) const { return count_in(cnt, c, cap); }
};
struct CellStart {  // start[c] = the items of the cells before c, start[ncell] = all of them; the counts become the cursors (0)
  int *cnt, *start;
  long long ncell;
  __device__ void operator()(long long c, long long, long long pre) const {
    start[c] = (int)pre;
    cnt[c] = 0;
  }
  __device__ void end(long long all) const { start[ncell] = (int)all; }
};

// cnt [ncell] -> start [ncell + 1], every entry at most cap (< 2^31); *total = the items, *most (may be null) = the fullest cell's.
// (T = int; a template, as k_flag_scan is, so that only the includers that call it carry its kernels)
template <class T>
hipError_t cells_to_start(T* cnt, int ncell, long long cap, T* tot, T* base, T* start, long long* total, long long* most, hipStream_t st) {
  return scan_values<T>(CellCount{cnt, cap}, WatchMax{most}, CellStart{cnt, start, ncell}, ncell, cap, tot, base, total, st);
}

}  // namespace

}  // namespace nerf
