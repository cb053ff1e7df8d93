// dw_bf16.hip -- weight gradients of the bf16-MLP variant: dW[o][i] = sum over samples of G[s][o] * X[s][i] on
// v_mfma_f32_32x32x16_bf16 with the SAMPLE index as the MFMA k (MI355X / gfx950).
//
// G (pre-activation gradients, written by field_bwd_bf16.hip) and X (layer inputs, saved by field_fwd_bf16.hip) live in
// HBM in fragment layout: per wave block of 32 samples, 1-KiB pieces in which lane (sample j, half h) holds 8 features of
// its sample.  Both MFMA operands need the transpose (8 consecutive SAMPLES of one feature per lane), which gfx950's
// ds_read_b64_tr_b16 does on the way out of LDS:
//   * a workgroup (8 waves, one per 32 output rows o) walks its share of the wave blocks; block b's G and X pieces are
//     brought to a 4-slot LDS ring by direct-to-LDS loads three blocks ahead (one barrier per block);
//   * the LDS image is the fragment layout with the sample index XOR-swizzled per (piece parity, half) -- done on the
//     SOURCE address of the load, the LDS side of a direct load being lane-linear -- so that the 32 lanes of a half hit
//     64 different banks in every transposed read (unswizzled: 4-way conflicts);
//   * per block and wave: 2 k-steps x (1 A fragment + NIT B fragments), 2 transposed reads each, NIT (+1: bias
//     gradient = G^T . ones) MFMAs per k-step; accumulators (NIT x 16 fp32 registers) persist over the whole share;
//   * the per-workgroup partial sums go to a slab and are added up in workgroup order by k_dw_bf16_reduce_batch: the result
//     does not depend on timing.
// The kernel is HBM-bound by construction (1 KiB of operands per 128 kFLOP): it is paced by the ring, not by the MFMAs.
#include "bf16_stream.h"

#include <stdlib.h>
#include <string.h>

namespace nerf {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef s16x4 __attribute__((address_space(3)))* lds_s16x4_p;

constexpr int DWB_WGS = 256;

struct DwBfArgs {
  // ngemm same-shaped products share one launch: workgroup b works on product b % ngemm with the samples split over the
  // gridDim.x / ngemm workgroups of that product -- all CUs busy with 1/ngemm of the slabs per product
  const unsigned char* G[6];   // start of the gradient tensor (fragment layout), g_ks pieces per wave block
  const unsigned char* X1[6];  // input tensor(s): the i index runs over X1's x1_ks pieces, then X2's (2 * NIT - x1_ks)
  const unsigned char* X2;     // (single products only)
  int ngemm;
  const unsigned char* Z;   // HAS_Z: a second, 2-piece gradient tensor whose product with the X tiles z_tile0 .. z_tile0 + 7 is formed as well (X^T Z)
  int z_tile0;
  int g_ks, o_tiles;        // o_tiles = output row tiles (waves w >= o_tiles only help loading)
  int x1_ks;
  int wb_tot;
  float* slabs;             // [product][workgroup][o_tiles*32 (+32 with Z)][NIT*32 + 1]  (last column: sum of G over the samples)
  // split-fp32 train step (SPLIT instantiations): every operand is a (hi, mid) pair of bf16 tensors of the same layout; the mid part of a
  // gradient-type tensor (G, Z) lies gdelta bytes behind its hi part, the mid part of an input tensor (X1, X2) xdelta bytes
  long long gdelta, xdelta;
};

// LDS unit (16 bytes) of (piece ks, half h, sample s) inside a tensor block: the sample index is XOR-swizzled
__device__ __forceinline__ int dwb_unit(int ks, int h, int s) { return ks * 64 + h * 32 + (s ^ (4 * (2 * (ks & 1) + h))); }

// MFMA operand (A or B alike) of feature tile t, k-step kstep (samples 16 kstep .. +15) from a tensor block in LDS
__device__ __forceinline__ u32x4 dwb_operand(const unsigned char* blk, int t, int kstep, int lane) {
  const int grp = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, hh = lane >> 5;
  const int ks = 2 * t + (grp & 1), h = p & 1, e = p >> 1;
  const int s0 = 16 * kstep + 8 * hh + q;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(blk + dwb_unit(ks, h, s0) * 16 + e * 8));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)(blk + dwb_unit(ks, h, s0 + 4) * 16 + e * 8));
  u32x4 r;
  r[0] = __builtin_bit_cast(uint2, lo).x;
  r[1] = __builtin_bit_cast(uint2, lo).y;
  r[2] = __builtin_bit_cast(uint2, hi).x;
  r[3] = __builtin_bit_cast(uint2, hi).y;
  return r;
}

template <int NIT, bool HAS_Z, bool SPLIT = false>
struct DwbGeom {
  static constexpr int XKS = 2 * NIT;
  static constexpr int PIECES = 16 + XKS + (HAS_Z ? 2 : 0);   // slot layout: G at piece 0, X at 16, Z at 16 + XKS; SPLIT: the mid parts behind, same order
  static constexpr int SLOT_PIECES = (SPLIT ? 2 : 1) * PIECES;
  static constexpr int SLOT_BYTES = SLOT_PIECES * BF_FRAG_BYTES;
  // ring slots: three blocks in flight are enough where a block is 32+ KiB; the products with small blocks (layer 0: 20 KiB, colour head:
  // 10 KiB used) were paced by the per-block latency (3.4-3.8 TB/s, profiles/r03_train_bf16_pmc.json): they get as many slots as fit.
  // SPLIT (two-part operands: twice the bytes per block): what fits 160 KiB, at most four -- two for the 256 x 256 products (64 KiB per block:
  // one being multiplied, one in flight)
  static constexpr int NSLOT_FIT = (160 * 1024) / SLOT_BYTES;
  static constexpr int NSLOT = SPLIT ? (NSLOT_FIT > 4 ? 4 : NSLOT_FIT) : (PIECES <= 20 ? 7 : (PIECES <= 26 ? 6 : 4));
  static constexpr int LDS_BYTES = NSLOT * SLOT_BYTES;
  static constexpr int NPW = (SLOT_PIECES + 7) / 8;           // loads per wave and block
  static_assert(NSLOT >= 2 && LDS_BYTES <= 160 * 1024, "LDS");
};

// The body of one workgroup: product `gi` of the argument block, workgroup `wg` of the `nwg` that share that product's samples; its
// partial sums go to slab_base + wg * rows * ld.
template <int NIT, bool HAS_Z, bool SPLIT = false>
__device__ __forceinline__ void dw_bf16_body(const DwBfArgs& a, unsigned char* lds, const int gi, const int wg, const int nwg, float* slab_base) {
  using Geo = DwbGeom<NIT, HAS_Z, SPLIT>;
  constexpr int XKS = Geo::XKS, NSLOT = Geo::NSLOT, NPW = Geo::NPW;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned lds_base = (unsigned)(uintptr_t)(lptr_t)lds;
  const unsigned char* const gG = a.G[gi];
  const unsigned char* const gX1 = a.X1[gi];
  const int per = (a.wb_tot + nwg - 1) / nwg;
  const int b_lo = wg * per, b_hi = min(a.wb_tot, b_lo + per);
  const int nb = b_hi - b_lo;
  const int gks = a.g_ks, x1 = a.x1_ks, total = gks + XKS + (HAS_Z ? 2 : 0);
  const bool worker = wv < a.o_tiles, zworker = HAS_Z && a.z_tile0 + wv < NIT;
  const int zt = a.z_tile0 + wv;  // the X tile this wave multiplies with Z

  f32x16 acc[NIT], accb, accz;
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NIT; ++i) acc[i] = zero;
  accb = zero;
  accz = zero;
  const u32x4 ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};  // bf16 1.0 pairs

  // pieces of a block are dealt round-robin to the waves; every wave issues the same NUMBER of loads per block (the
  // counted wait needs that): a wave whose turn falls beyond the last piece loads the last piece again.
  // Swizzle on the source side: LDS lane L of a piece holds sample (L & 31) ^ swz of half L >> 5.
  auto dma_block = [&](int b, int slot) {
    const int wb = b_lo + (b < nb ? b : nb - 1);
#pragma unroll
    for (int k = 0; k < NPW; ++k) {
      int pc = wv + 8 * k;
      constexpr int SETS = SPLIT ? 2 : 1;
      pc = pc < SETS * total ? pc : SETS * total - 1;
      const bool mid = SPLIT && pc >= total;  // SPLIT: pieces [total, 2 total) are the mid parts, slot pieces Geo::PIECES ..
      if (mid) pc -= total;
      const long long gd = mid ? a.gdelta : 0, xd = mid ? a.xdelta : 0;
      const unsigned char* src;
      int ks, dst;
      if (pc < gks) {
        ks = pc; dst = ks;
        src = gG + gd + ((size_t)wb * gks + ks) * BF_FRAG_BYTES;
      } else if (pc < gks + XKS) {
        const int x = pc - gks;
        ks = x; dst = 16 + x;  // parity of the slot piece = parity of x (x1_ks is even)
        src = (x < x1 ? gX1 + ((size_t)wb * x1 + x) * BF_FRAG_BYTES : a.X2 + ((size_t)wb * (XKS - x1) + (x - x1)) * BF_FRAG_BYTES) + xd;
      } else {
        ks = pc - gks - XKS; dst = 16 + XKS + ks;
        src = a.Z + gd + ((size_t)wb * 2 + ks) * BF_FRAG_BYTES;
      }
      if (mid) dst += Geo::PIECES;
      const int h = lane >> 5, s = (lane & 31) ^ (4 * (2 * (ks & 1) + h));
      glds16(src + (h * 32 + s) * 16, lds_base + slot * Geo::SLOT_BYTES + dst * BF_FRAG_BYTES);  // (the non-temporal form measured the same)
    }
  };
  if (nb > 0) {
#pragma unroll
    for (int b = 0; b < NSLOT - 1; ++b) dma_block(b, b);
    for (int b = 0; b < nb; ++b) {
      wait_vmcnt<(NSLOT - 2) * NPW>();  // my pieces of block b are in LDS ...
      __builtin_amdgcn_s_barrier();     // ... and everybody's; everybody is done with block b - 1
      asm volatile("" ::: "memory");
      dma_block(b + NSLOT - 1, (b + NSLOT - 1) % NSLOT);  // into the slot of block b - 1
      const unsigned char* gb = lds + (b % NSLOT) * Geo::SLOT_BYTES;
      const unsigned char* xb = gb + 16 * BF_FRAG_BYTES;
      constexpr int MID = Geo::PIECES * BF_FRAG_BYTES;  // SPLIT: the mid parts of the block sit this far behind their hi parts
      if (worker) {
#pragma unroll
        for (int kstep = 0; kstep < 2; ++kstep) {
          const u32x4 A = dwb_operand(gb, wv, kstep, lane);
          if constexpr (SPLIT) {  // G^T X = G_hi^T X_hi + G_hi^T X_mid + G_mid^T X_hi (+ O(2^-16)), the small products first; column sums of G_hi + G_mid
            const u32x4 Am = dwb_operand(gb + MID, wv, kstep, lane);
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
              const u32x4 Bh = dwb_operand(xb, i, kstep, lane);
              acc[i] = bf_mfma(Am, Bh, acc[i]);
              acc[i] = bf_mfma(A, dwb_operand(xb + MID, i, kstep, lane), acc[i]);
              acc[i] = bf_mfma(A, Bh, acc[i]);
            }
            accb = bf_mfma(Am, ones, accb);
            accb = bf_mfma(A, ones, accb);
          } else {
#pragma unroll
            for (int i = 0; i < NIT; ++i) acc[i] = bf_mfma(A, dwb_operand(xb, i, kstep, lane), acc[i]);
            accb = bf_mfma(A, ones, accb);
          }
        }
      }
      if (zworker) {  // rows = this wave's X tile, columns = Z features: (X^T Z) tile
        const unsigned char* zb = xb + XKS * BF_FRAG_BYTES;
#pragma unroll
        for (int kstep = 0; kstep < 2; ++kstep) {
          const u32x4 Xh = dwb_operand(xb, zt, kstep, lane), Zh = dwb_operand(zb, 0, kstep, lane);
          if constexpr (SPLIT) {
            accz = bf_mfma(dwb_operand(xb + MID, zt, kstep, lane), Zh, accz);
            accz = bf_mfma(Xh, dwb_operand(zb + MID, 0, kstep, lane), accz);
          }
          accz = bf_mfma(Xh, Zh, accz);
        }
      }
    }
    wait_vmcnt<0>();  // nothing may still be writing this workgroup's LDS when it ends
  }
  // accumulator layout: lane l holds column l & 31 and rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)
  const int NI = NIT * 32, ld = NI + 1;
  const int rows = a.o_tiles * 32 + (HAS_Z ? 32 : 0);
  float* slab = slab_base + (size_t)wg * rows * ld;
  const int n = lane & 31, hh = lane >> 5;
  if (worker) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * hh;
#pragma unroll
      for (int i = 0; i < NIT; ++i) slab[(size_t)o * ld + 32 * i + n] = acc[i][r];
      if (n == 0) slab[(size_t)o * ld + NI] = accb[r];
    }
  }
  if (zworker) {  // slab row o_tiles*32 + z, column i
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 * zt + (r & 3) + 8 * (r >> 2) + 4 * hh;
      slab[(size_t)(a.o_tiles * 32 + n) * ld + i] = accz[r];
    }
  }
}

template <int NIT, bool HAS_Z, bool SPLIT = false>
__global__ __launch_bounds__(BF_WG, 1) void k_dw_bf16(const DwBfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int gi = blockIdx.x % a.ngemm, wg = blockIdx.x / a.ngemm, nwg = gridDim.x / a.ngemm;
  const int rows = a.o_tiles * 32 + (HAS_Z ? 32 : 0);
  dw_bf16_body<NIT, HAS_Z, SPLIT>(a, lds, gi, wg, nwg, a.slabs + (size_t)gi * nwg * rows * (NIT * 32 + 1));
}

// ---- SMALL batches: every product of the step (or of its early / late part) in ONE launch -------------------------------------------
// A launch per product hands each of them ALL workgroups and so a slab per workgroup: 219 MB of partial sums written and read back per
// step whatever the batch -- a third of the phase at 512 rays (0.31 ms against 0.17 for an eighth of the 4096-ray phase) -- behind five
// launch boundaries and with 12-block streams whose ring never fills.  Here the workgroups of ONE launch are dealt out over the
// products in proportion to their bytes per wave block: as many CUs busy, streams of 100+ blocks, a quarter of the slabs.  Products of
// different shapes run different instantiations of the same body behind a block-uniform switch.
struct DwBfMulti {
  static constexpr int MAXP = 12;
  DwBfArgs a[MAXP];     // per product (ngemm = 1, product index 0); a[i].slabs = its slab base
  int kind[MAXP];       // instantiation: 2 * NIT + HAS_Z
  int wg0[MAXP + 1];    // first workgroup of product i (wg0[n] = grid size)
  int n;
};

template <bool SPLIT>
__global__ __launch_bounds__(BF_WG, 1) void k_dw_bf16_multi(const DwBfMulti m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int i = 0;
#pragma unroll 1
  while (i + 1 < m.n && (int)blockIdx.x >= m.wg0[i + 1]) ++i;
  i = __builtin_amdgcn_readfirstlane(i);
  const DwBfArgs& a = m.a[i];
  const int wg = blockIdx.x - m.wg0[i], nwg = m.wg0[i + 1] - m.wg0[i];
  switch (m.kind[i]) {
    case 2 * 10 + 0: dw_bf16_body<10, false, SPLIT>(a, lds, 0, wg, nwg, a.slabs); break;
    case 2 * 9 + 1: dw_bf16_body<9, true, SPLIT>(a, lds, 0, wg, nwg, a.slabs); break;
    case 2 * 8 + 0: dw_bf16_body<8, false, SPLIT>(a, lds, 0, wg, nwg, a.slabs); break;
    case 2 * 4 + 0: dw_bf16_body<4, false, SPLIT>(a, lds, 0, wg, nwg, a.slabs); break;
    case 2 * 2 + 0: dw_bf16_body<2, false, SPLIT>(a, lds, 0, wg, nwg, a.slabs); break;
    default: break;
  }
}

// dW[o][col0 + i - i_first] = sum over slabs of row o_first + o, column i; db[o] likewise from the last slab column
struct DwBfReduceArgs {
  const float* slabs;
  int nslab, rows, ni;          // slab = [rows][ni + 1]
  int o_first, o_count, i_first, i_count;   // slab columns [i_first, i_first + i_count) -> dW columns col0 ..
  float* dW; int ldw, col0;
  float* db;                    // or null
};
struct DwBfReduceBatch { DwBfReduceArgs r[16]; int n; };

// 64 output elements per block; the slabs are split over 4 thread groups whose partial sums are added in a fixed order.
// ONE launch for all slab sums of a step: blockIdx.y = descriptor (the thirteen per-product launches cost 90 us per step in launch
// gaps and tiny grids -- a quarter of the weight-gradient phase of a 512-ray step)
__global__ __launch_bounds__(256) void k_dw_bf16_reduce_batch(const DwBfReduceBatch b) {
  __shared__ float part[4][64];
  const DwBfReduceArgs& a = b.r[blockIdx.y];
  const int ld = a.ni + 1;
  if ((int)blockIdx.x * 64 >= a.o_count * ld) return;  // (block-uniform)
  const int e = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + e;
  const bool in_range = idx < a.o_count * ld;
  const int o = in_range ? idx / ld : 0, i = in_range ? idx - o * ld : 0;
  const bool wanted = in_range && ((i < a.ni && i >= a.i_first && i < a.i_first + a.i_count && a.dW != nullptr) || (i == a.ni && a.db != nullptr));
  float s = 0.f;
  if (wanted) {
    const float* p = a.slabs + (size_t)(a.o_first + o) * ld + i;
    const size_t stride = (size_t)a.rows * ld;
    const int per = (a.nslab + 3) / 4, k0 = grp * per, k1 = min(a.nslab, k0 + per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = k0;
    for (; k + 3 < k1; k += 4) {
      s0 += p[(size_t)k * stride];
      s1 += p[(size_t)(k + 1) * stride];
      s2 += p[(size_t)(k + 2) * stride];
      s3 += p[(size_t)(k + 3) * stride];
    }
    for (; k < k1; ++k) s0 += p[(size_t)k * stride];
    s = (s0 + s1) + (s2 + s3);
  }
  part[grp][e] = s;
  __syncthreads();
  if (grp == 0 && wanted) {
    const float t = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    if (i == a.ni)
      a.db[o] = t;
    else
      a.dW[(size_t)o * a.ldw + a.col0 + (i - a.i_first)] = t;
  }
}

// ---- host side: the products of a step as ONE table; launches, reduce descriptors and the slab space all come from it -------------
// One output of a product: slab rows [o_first, o_first + o_count), columns [i_first, i_first + i_count) -> tensor `dst` [o][col0 + i] of
// row length ldw, and the last slab column (the sums of G) -> tensor `bias`.  Tensors: 0..23 = the gradient tensors, DWB_MBUF = the
// folded product's M, -1 = none.  (o_count = 0: no such output.)
constexpr int DWB_MBUF = 24;
struct DwbOut { int o_first, o_count, i_first, i_count, dst, ldw, col0, bias; };
struct DwbProd {
  int g, g_ks;                 // gradient tensor (BG_*) and its pieces per wave block
  int x1, x1_ks, x2, x2_ks;    // input tensors (BS_*): the i index runs over X1's pieces, then X2's (x2 = -1: none)
  bool z;                      // BG_Z rides along: X^T Z in 32 extra slab rows (the sigma head, on the product whose X2 is h7)
  int pct;                     // cost of a KiB of this product in a multi launch, in per cent of a 256 x 256 product's (see DwbPhase::multi)
  bool early;                  // its outputs are tensors of point_layer[0..7]: final before the early event
  DwbOut out[3];
  constexpr int nit() const { return (x1_ks + x2_ks) / 2; }
  constexpr int kind() const { return 2 * nit() + (z ? 1 : 0); }          // DwBfMulti::kind
  constexpr int kib() const { return g_ks + x1_ks + x2_ks + (z ? 2 : 0); }  // read per wave block
  constexpr int o_tiles() const { return (g_ks + 1) / 2; }
  constexpr int z_tile0() const { return z ? x1_ks / 2 : 0; }             // Z multiplies the X2 tiles
  constexpr int rows() const { return o_tiles() * 32 + (z ? 32 : 0); }
  constexpr int ni() const { return nit() * 32; }
  constexpr size_t slab_floats() const { return (size_t)rows() * (ni() + 1); }  // per workgroup
};
constexpr DwbProd dwb_prod(int g, int x1, int x2, bool z, int pct, bool early, DwbOut o0, DwbOut o1 = {}, DwbOut o2 = {}) {
  return DwbProd{g, bg_ks(g), x1, bs_ks(x1), x2, x2 < 0 ? 0 : bs_ks(x2), z, pct, early, {o0, o1, o2}};
}
constexpr DwbProd dwb_layer(int l) {  // a 256 x 256 layer on the previous layer's output
  return dwb_prod(BG_L0 + l, BS_H0 + l - 1, -1, false, 100, true, {0, WIDTH, 0, WIDTH, 2 * l, WIDTH, 0, 2 * l + 1});
}
// The costs: a product's small blocks are paced by the ring's per-block latency, so its KiB weigh more than those of the 256 x 256 products
// (profiles/r03_train_bf16_pmc.json: those stream at 5.8 TB/s, layer 4 5.4, the folded product 4.3, the colour head 3.8, layer 0 3.4).
enum { DWP_L0, DWP_L1, DWP_L2, DWP_L3, DWP_L5, DWP_L6, DWP_L7, DWP_L4, DWP_FOLD, DWP_COL, DWP_N };
constexpr DwbProd kDwbProds[DWP_N] = {
    dwb_prod(BG_L0, BS_GP, -1, false, 170, true, {0, WIDTH, 0, POINT_DIM, W_L0, POINT_DIM, 0, B_L0}),  // layer 0: X = gamma_p
    dwb_layer(1), dwb_layer(2), dwb_layer(3), dwb_layer(5), dwb_layer(6), dwb_layer(7),
    // layer 4: one pass over dpre4 for both column groups of the [256][316] matrix, X = [h3 | gamma_p]
    dwb_prod(BG_L0 + 4, BS_H0 + 3, BS_GP, false, 107, true, {0, WIDTH, 0, WIDTH + POINT_DIM, 8, WIDTH + POINT_DIM, 0, 9}),
    // point_info folded into dir_info (bf16_common.h): ONE product dpre_dir^T [gamma_d | h7] -- columns 0..23 are dir_info's direction
    // columns, columns 32.. are M = dpre_dir^T h7 (-> k_fold_grads) -- and in the same pass over h7 the sigma head: row 3 of h7^T (dz, dspre)
    dwb_prod(BG_D, BS_GD, BS_H0 + 7, true, 135, false, {0, HALF, 0, DIR_DIM, W_DIR, WIDTH + DIR_DIM, 0, B_DIR},
             {0, HALF, 32, WIDTH, DWB_MBUF, WIDTH, 0, -1}, {HALF + 3, 1, 32, WIDTH, W_SIGMA, WIDTH, 0, -1}),
    // colour head = rows 0..2 of the (dz, dspre) tile against c; row 3 of its column sums = the sigma bias gradient
    dwb_prod(BG_Z, BS_C, -1, false, 150, false, {0, 3, 0, HALF, W_COLOR, HALF, 0, B_COLOR}, {3, 1, 0, 0, -1, 0, 0, B_SIGMA}),
};

// The three launch structures, each a list of table rows and the launcher it goes through (DwbPhase below):
//  * SMALL batches: every product in one multi launch; with an early event the early ones in one and the rest in another;
//  * LARGE batches: the six 256 x 256 products as a group (42 workgroups each: a sixth of the slab traffic), then the products with small
//    blocks in one multi launch, where their streams overlap (weight-gradient phase against a launch each: 2,048 rays 0.767 -> 0.707 ms,
//    4,096 rays 1.375 -> 1.36; layer 4 in a launch of its own: +-0);
//  * LARGE batches with an early event (it needs layer 0 in front of the event and the folded product and the colour head behind it): a
//    launch per product around the group -- DWP_L0, kDwbGroup, DWP_L4, <event>, DWP_FOLD, DWP_COL.
constexpr int kDwbSmall[DWP_N] = {DWP_L0, DWP_L1, DWP_L2, DWP_L3, DWP_L5, DWP_L6, DWP_L7, DWP_L4, DWP_FOLD, DWP_COL};
constexpr int DWB_SMALL_EARLY = 8;  // the early products of kDwbSmall come first
constexpr int DWB_NGROUP = 6, DWB_GROUP_WGS = DWB_WGS / DWB_NGROUP;
constexpr int kDwbGroup[DWB_NGROUP] = {DWP_L1, DWP_L2, DWP_L3, DWP_L5, DWP_L6, DWP_L7};
constexpr int kDwbLargeRest[4] = {DWP_L4, DWP_L0, DWP_FOLD, DWP_COL};

// the instantiated forms (NIT, HAS_Z); k_dw_bf16_multi's switch lists the same five
#define DWB_FORMS(F) F(10, false) F(9, true) F(8, false) F(4, false) F(2, false)
constexpr bool dwb_table_ok() {
  int nout = 0;
  for (int i = 0; i < DWP_N; ++i) {
    const DwbProd& p = kDwbProds[i];
    bool form = false;
#define DWB_IS(NIT, Z) form = form || (p.nit() == NIT && p.z == Z);
    DWB_FORMS(DWB_IS)
#undef DWB_IS
    if (!form || (p.x1_ks + p.x2_ks) % 2 || p.x1_ks % 2) return false;  // (the parity of a slot piece = the parity of its X piece)
    if (p.early != (i < DWB_SMALL_EARLY) || kDwbSmall[i] != i) return false;
    for (const DwbOut& o : p.out) nout += o.o_count > 0;
  }
  const DwbProd& g0 = kDwbProds[kDwbGroup[0]];
  for (int k : kDwbGroup) {  // a group is one DwBfArgs in front of the event: same shape, no X2, no Z, early
    const DwbProd& p = kDwbProds[k];
    if (p.kind() != g0.kind() || p.g_ks != g0.g_ks || p.x2_ks || p.z || !p.early) return false;
  }
  return nout <= (int)(sizeof(DwBfReduceBatch::r) / sizeof(DwBfReduceArgs));  // all slab sums of a step fit ONE reduce launch
}
static_assert(dwb_table_ok(), "a product of a shape that is not instantiated, an early product behind a late one, or too many outputs");

// Slab space: every product of a step keeps its own slabs (ONE reduce launch at the end).  The worst case is the launch per product: all
// DWB_WGS workgroups each, DWB_GROUP_WGS for the grouped ones.
constexpr bool dwb_grouped(int i) {
  for (int k : kDwbGroup)
    if (k == i) return true;
  return false;
}
constexpr size_t dwb_slab_floats(const int* prods, int n) {
  size_t f = 0;
  for (int i = 0; i < n; ++i) f += (dwb_grouped(prods[i]) ? DWB_GROUP_WGS : DWB_WGS) * kDwbProds[prods[i]].slab_floats();
  return f;
}
constexpr size_t dwb_most_slab_floats(const int* prods, int n) {
  size_t f = 0;
  for (int i = 0; i < n; ++i) f = kDwbProds[prods[i]].slab_floats() > f ? kDwbProds[prods[i]].slab_floats() : f;
  return f;
}
constexpr size_t DWB_SLAB_FLOATS = dwb_slab_floats(kDwbSmall, DWP_N);
static_assert(DWB_SLAB_FLOATS == 54770688, "the slab region is part of the workspace layout");
// (the large-batch structure without an event: the group, then a multi launch of at most DWB_WGS workgroups; a multi launch checks its own plan too)
static_assert(dwb_slab_floats(kDwbGroup, DWB_NGROUP) + DWB_WGS * dwb_most_slab_floats(kDwbLargeRest, 4) <= DWB_SLAB_FLOATS, "slab space");
size_t dw_bf16_slab_floats() { return DWB_SLAB_FLOATS; }

template <int NIT, bool HAS_Z, bool SPLIT>
static hipError_t dwb_launch_as(const DwBfArgs& a, int wgs, hipStream_t st) {
  static std::atomic<unsigned long long> opted{0};
  using Geo = DwbGeom<NIT, HAS_Z, SPLIT>;
  if (hipError_t e = ensure_dynamic_lds(opted, {reinterpret_cast<const void*>(&k_dw_bf16<NIT, HAS_Z, SPLIT>)}, Geo::LDS_BYTES)) return e;
  hipLaunchKernelGGL((k_dw_bf16<NIT, HAS_Z, SPLIT>), dim3(wgs), dim3(BF_WG), Geo::LDS_BYTES, st, a);
  return hipGetLastError();
}
// k_dw_bf16 of the form `kind` (a.gdelta / a.xdelta != 0: the two-part form of the split-fp32 train step)
static hipError_t dwb_launch(int kind, const DwBfArgs& a, int wgs, hipStream_t st) {
  const bool split = a.gdelta || a.xdelta;
  switch (kind) {
#define DWB_CASE(NIT, Z) \
  case 2 * NIT + (Z ? 1 : 0): return split ? dwb_launch_as<NIT, Z, true>(a, wgs, st) : dwb_launch_as<NIT, Z, false>(a, wgs, st);
    DWB_FORMS(DWB_CASE)
#undef DWB_CASE
    default: return hipErrorInvalidValue;
  }
}

// All products in one or two multi launches up to this many wave blocks -- where the per-product launches' slabs (219 MB per step whatever
// the batch) and launch boundaries weigh (a rank's share of a strong-scaling step, the reference's 400-ray batch) -- and the large-batch
// structures beyond.  NERF_DW_BF16_MULTI=0 / 1 overrides the choice (A/B measurements only).
constexpr int DW_BF16_MULTI_MAX_WB = 5120;  // 853 rays x (64 + 128); measured: 400 rays -25 %, 512 -18 %, 1024 +-0, 2048 +10 %, 4096 +30 %
static bool dw_bf16_multi(int wb_tot) {
  static const int forced = [] { const char* e = getenv("NERF_DW_BF16_MULTI"); return e ? atoi(e) : -1; }();
  return forced >= 0 ? forced != 0 : wb_tot <= DW_BF16_MULTI_MAX_WB;
}

// One weight-gradient phase being enqueued: the launchers carve each product's slabs from `slab` in launch order and note its slab sums
// in `rb`, which reduce() sends off in ONE launch.
struct DwbPhase {
  const unsigned char *bs, *bg;
  int wb_tot;
  float* const* dw;
  float* mbuf;
  float* slab;              // the next free slab
  const float* slab_limit;  // one past the slab space
  DwBfSplit sp;
  hipStream_t st;
  DwBfReduceBatch rb;

  float* dst(int t) const { return t < 0 ? nullptr : t == DWB_MBUF ? mbuf : dw[t]; }
  // product p joins the argument block `a` (zeroed, then the same-shaped products of a group one after the other), its slabs at `slabs`
  void add(DwBfArgs& a, const DwbProd& p, float* slabs) const {
    const int k = a.ngemm++;
    a.G[k] = bg + (size_t)wb_tot * bg_cum(p.g) * BF_FRAG_BYTES;
    a.X1[k] = bs + (size_t)wb_tot * bs_cum(p.x1) * BF_FRAG_BYTES;
    if (k) return;
    a.X2 = p.x2 < 0 ? a.X1[0] : bs + (size_t)wb_tot * bs_cum(p.x2) * BF_FRAG_BYTES;
    a.Z = p.z ? bg + (size_t)wb_tot * bg_cum(BG_Z) * BF_FRAG_BYTES : nullptr;
    a.z_tile0 = p.z_tile0(); a.g_ks = p.g_ks; a.o_tiles = p.o_tiles(); a.x1_ks = p.x1_ks; a.wb_tot = wb_tot; a.slabs = slabs;
    a.gdelta = sp.gdelta; a.xdelta = sp.xdelta;
  }
  void sums(const DwbProd& p, const float* slabs, int nslab) {
    for (const DwbOut& o : p.out) {
      if (o.o_count == 0) continue;
      DwBfReduceArgs& r = rb.r[rb.n++];
      r.slabs = slabs; r.nslab = nslab; r.rows = p.rows(); r.ni = p.ni();
      r.o_first = o.o_first; r.o_count = o.o_count; r.i_first = o.i_first; r.i_count = o.i_count;
      r.dW = dst(o.dst); r.ldw = o.ldw; r.col0 = o.col0; r.db = dst(o.bias);
    }
  }
  // one pass over the samples for ONE product on all workgroups: slabs <- G^T [X1 | X2]  (+ [X1 | X2]^T Z in 32 extra slab rows)
  hipError_t each(int prod) {
    const DwbProd& p = kDwbProds[prod];
    DwBfArgs a;
    memset(&a, 0, sizeof(a));
    add(a, p, slab);
    const int wgs = wb_tot < DWB_WGS ? wb_tot : DWB_WGS;
    sums(p, slab, wgs);
    slab += wgs * p.slab_floats();
    return dwb_launch(p.kind(), a, wgs, st);
  }
  // the products of kDwbGroup in one launch (workgroup b works on product b % 6), one after the other in the slab space
  hipError_t group() {
    DwBfArgs a;
    memset(&a, 0, sizeof(a));
    const int nwg = wb_tot < DWB_GROUP_WGS ? wb_tot : DWB_GROUP_WGS;
    for (int k = 0; k < DWB_NGROUP; ++k) {
      const DwbProd& p = kDwbProds[kDwbGroup[k]];
      add(a, p, slab);
      sums(p, slab + k * nwg * p.slab_floats(), nwg);
    }
    slab += DWB_NGROUP * nwg * kDwbProds[kDwbGroup[0]].slab_floats();
    return dwb_launch(kDwbProds[kDwbGroup[0]].kind(), a, nwg * DWB_NGROUP, st);
  }
  // n products of any shape in ONE launch of (at most) DWB_WGS workgroups, dealt out in proportion to the products' costs (largest
  // remainder, at least one each, never more than wave blocks): as many CUs busy as with a launch each, streams of 100+ blocks, a quarter
  // of the slabs.  Nothing is enqueued when the plan's slabs would run past the slab space.
  hipError_t multi(const int* prods, int n) {
    static_assert(DWP_N <= DwBfMulti::MAXP, "products of a multi launch");
    DwBfMulti m;
    memset(&m, 0, sizeof(m));
    m.n = n;
    int pieces[DwBfMulti::MAXP], total = 0;
    for (int i = 0; i < n; ++i) {
      pieces[i] = kDwbProds[prods[i]].kib() * kDwbProds[prods[i]].pct;
      total += pieces[i];
    }
    const int budget = DWB_WGS;
    int nwg[DwBfMulti::MAXP], used = 0;
    for (int i = 0; i < n; ++i) {
      nwg[i] = (int)((long long)budget * pieces[i] / total);
      if (nwg[i] < 1) nwg[i] = 1;
      if (nwg[i] > wb_tot) nwg[i] = wb_tot;
      used += nwg[i];
    }
    // hand the remaining workgroups to the products with the most bytes per workgroup (fixed order: deterministic slabs)
    while (used < budget) {
      int best = -1;
      double worst = 0.0;
      for (int i = 0; i < n; ++i) {
        const double load = (double)pieces[i] / nwg[i];
        if (nwg[i] < wb_tot && load > worst) { worst = load; best = i; }
      }
      if (best < 0) break;
      ++nwg[best]; ++used;
    }
    while (used > budget) {  // (only when n > budget or the minimum of one each overshoots: not with 12 products)
      int best = -1;
      double least = 1e30;
      for (int i = 0; i < n; ++i) {
        const double load = (double)pieces[i] / nwg[i];
        if (nwg[i] > 1 && load < least) { least = load; best = i; }
      }
      if (best < 0) break;
      --nwg[best]; --used;
    }
    float* end = slab;
    for (int i = 0; i < n; ++i) {
      const DwbProd& p = kDwbProds[prods[i]];
      add(m.a[i], p, end);
      m.kind[i] = p.kind();
      m.wg0[i + 1] = m.wg0[i] + nwg[i];
      end += nwg[i] * p.slab_floats();
    }
    if (end > slab_limit) return hipErrorOutOfMemory;
    for (int i = 0; i < n; ++i) sums(kDwbProds[prods[i]], m.a[i].slabs, nwg[i]);
    slab = end;
    // (bf16 operands: every form fits 144 KiB; two-part operands: the whole LDS, which DwbGeom holds every form to)
    constexpr int lds_bytes = 144 * 1024, lds_split = 160 * 1024;
#define DWB_FITS(NIT, Z) static_assert(DwbGeom<NIT, Z>::LDS_BYTES <= lds_bytes && DwbGeom<NIT, Z, true>::LDS_BYTES <= lds_split, "LDS of the multi launch");
    DWB_FORMS(DWB_FITS)
#undef DWB_FITS
    static std::atomic<unsigned long long> opted{0}, opted_split{0};
    if (sp.gdelta || sp.xdelta) {
      if (hipError_t e = ensure_dynamic_lds(opted_split, {reinterpret_cast<const void*>(&k_dw_bf16_multi<true>)}, lds_split)) return e;
      hipLaunchKernelGGL(k_dw_bf16_multi<true>, dim3(m.wg0[n]), dim3(BF_WG), lds_split, st, m);
      return hipGetLastError();
    }
    if (hipError_t e = ensure_dynamic_lds(opted, {reinterpret_cast<const void*>(&k_dw_bf16_multi<false>)}, lds_bytes)) return e;
    hipLaunchKernelGGL(k_dw_bf16_multi<false>, dim3(m.wg0[n]), dim3(BF_WG), lds_bytes, st, m);
    return hipGetLastError();
  }
  // the slab sums noted so far, in ONE launch
  hipError_t reduce() {
    int most = 1;
    for (int k = 0; k < rb.n; ++k) {
      const int blocks = (rb.r[k].o_count * (rb.r[k].ni + 1) + 63) / 64;
      most = blocks > most ? blocks : most;
    }
    hipLaunchKernelGGL(k_dw_bf16_reduce_batch, dim3(most, rb.n), dim3(256), 0, st, rb);
    rb.n = 0;
    return hipGetLastError();
  }
  // point_layer[0..7] are complete: their sums go out now, the rest of the products follow the event
  hipError_t early_done(hipEvent_t ev) {
    if (hipError_t e = reduce()) return e;
    return hipEventRecord(ev, st);
  }
};

#define DWB_TRY(expr) do { if (hipError_t e_ = (expr)) return e_; } while (0)
hipError_t launch_dw_bf16_phase(const unsigned char* bs, const unsigned char* bg, int wb_tot, float* const* dw, float* mbuf, float* slabs,
                                size_t slab_floats, const Weights24& w, void* early_event, DwBfSplit sp, hipStream_t st) {
  if (wb_tot < 1) return hipErrorInvalidValue;
  DwbPhase ph = {bs, bg, wb_tot, dw, mbuf, slabs, slabs + slab_floats, sp, st, {}};
  const hipEvent_t ev = static_cast<hipEvent_t>(early_event);
  if (dw_bf16_multi(wb_tot)) {
    const int first = ev ? DWB_SMALL_EARLY : DWP_N;
    DWB_TRY(ph.multi(kDwbSmall, first));
    if (ev) {
      DWB_TRY(ph.early_done(ev));
      DWB_TRY(ph.multi(kDwbSmall + first, DWP_N - first));
    }
  } else if (!ev) {
    DWB_TRY(ph.group());
    DWB_TRY(ph.multi(kDwbLargeRest, 4));
  } else {
    DWB_TRY(ph.each(DWP_L0));
    DWB_TRY(ph.group());
    DWB_TRY(ph.each(DWP_L4));
    DWB_TRY(ph.early_done(ev));
    DWB_TRY(ph.each(DWP_FOLD));
    DWB_TRY(ph.each(DWP_COL));
  }
  DWB_TRY(ph.reduce());
  return launch_fold_grads(fold_grad_args(w, dw, mbuf), st);
}
#undef DWB_TRY

}  // namespace nerf
