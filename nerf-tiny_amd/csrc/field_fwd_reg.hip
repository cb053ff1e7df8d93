// field_fwd_reg.hip -- inference forward of the field query with REGISTER-RESIDENT activations (MI355X / gfx950).
//
// Same arithmetic as k_field_fwd (field_fwd.hip) and the same packed weight image, but no activations in LDS and no barriers
// (the forms that save no activation rows send their lazy ReLU through 8 KiB of wave-private LDS: ReluLds below):
//   * one 64-lane wave owns 32 samples and computes ALL 256 features of every layer for them:
//     D[feature][sample] = W . act  with v_mfma_f32_32x32x2_f32, 8 feature tiles x 16 accumulator VGPRs;
//   * in the 32x32 accumulator layout lane (j, h) holds features 32t + 8g + 4h + r of sample j.  The MFMA sums over
//     its two lane halves, and WHICH k each half supplies is free as long as A and B agree -- so the post-ReLU
//     accumulator registers of layer L are used, as they stand, as the B operand of layer L+1
//     (k-step (t, 4g + r): half h supplies k = 32t + 8g + 4h + r), and the A fragment that goes with it is the
//     4 consecutive weights W[i][32t + 8g + 4h .. +3] -- exactly the float4 the packed image already stores;
//   * nothing is shared between waves, so nothing synchronises: a wave streams 8,192 MFMAs per tile (the saving forward 8,256) with a
//     2-stage register pipeline of A fragments (8 x 16-byte loads per k-block, L2/L1 resident, requested one
//     k-block = 32 MFMAs = 2048 cycles ahead, also across layer boundaries);
//   * biases are the start value of the accumulators: 16-byte loads straight into the accumulator registers, requested behind MFMAs
//     of the layer in front (reg_layer's NEXT_BIAS; the saving forward: one extra MFMA per tile, A = bias, B = 1 on lane half 0);
//     the sigma and colour heads are VALU dot products over the registers the wave already holds.
// One wave per SIMD (about 400 VGPRs).  Used when nothing has to be saved for backward, and for the point queries (k_field_fwd_reg's
// SRC / RGB template arguments below) -- with GSAVE, the forward of a gradient query (nerf_hip_query_grad).
#include "field_common.h"
#include <type_traits>

namespace nerf {

constexpr int RM = 32;  // samples per wave

// f(integral_constant<int, I>) for I = I0 .. I1 - 1
template <int I0, int I1, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    static_for<I0 + 1, I1>(f);
  }
}

template <int NFT>
struct WStage {
  float4 w[NFT];
};

template <int KB, int NFT>
__device__ __forceinline__ void stage_load(const float4* __restrict__ seg_lane, int kb, WStage<NFT>& s) {
#pragma unroll
  for (int f = 0; f < NFT; ++f) s.w[f] = seg_lane[(size_t)(f * KB + kb) * 64];
}

// ReLU as ONE instruction: for every non-NaN float max(x, 0) = the float whose bits are max(int bits, 0) (negative floats and
// -0 are negative integers).  fmaxf costs two (hipcc canonicalises its operand first), and next to fp32 MFMAs every VALU
// instruction is matrix time lost (the fp32 MFMA runs on the SIMD's fp32 lanes).
__device__ __forceinline__ float relu1(float x) { return __int_as_float(max(__float_as_int(x), 0)); }

__device__ __forceinline__ float f4c(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// The lazy ReLU of the instantiations that save no activation rows, through LDS instead of the VALU: next to fp32 MFMAs a
// v_accvgpr_read + v_max_i32 pair per value is matrix time lost, a DS instruction behind an MFMA is not (scripts/micro/mfma_f32_bank.hip,
// profiles/fwd_f32_relu_paths_micro.txt: ONE DS instruction per MFMA costs nothing, bursts of them do).  A tile of 16 accumulator
// registers makes the round trip in 24 DS instructions, group g of 4 registers in 6: ds_write_b128 straight from the accumulator
// registers, 4 x ds_max_i32 with 0 (integer max = relu1, -0 -> +0 included), ds_read_b128 into the B-operand registers.  The DS
// instructions of a wave execute in order, so the three need no barrier in a 64-thread workgroup, and the compiler counts lgkmcnt.
// Layout: 2 slots (tile t in slot t & 1) x 4 groups x 64 lanes x 16 bytes = 8 KiB.  The b128 forms are conflict-free with lanes 16 bytes
// apart; a b32 instruction serves 32 lanes per pass from 32 banks, so the c-th ds_max of lane l takes dword (c + l / 8) & 3 of the
// lane's 16 bytes: lanes 8 apart hit different banks, all 32 lanes of a pass distinct ones.
typedef int lds_i32 __attribute__((address_space(3), may_alias));
typedef int i32x4v __attribute__((ext_vector_type(4), may_alias));
typedef __attribute__((address_space(3))) i32x4v lds_i32x4;
constexpr int RELU_LDS_DWORDS = 2 * 4 * 64 * 4;
// behind the slots (inference forms with colour): W_color as it lies in memory, [3][128] floats, then b_color[3] at dword 3 * HALF.  The colour
// head runs behind the last MFMA with nothing to hide a global load behind; its operands are requested in the prologue, parked here, and
// come back as ds_read_b128 (every lane of a half reads the same 16 bytes: a broadcast, no bank conflict).
constexpr int COL_LDS_DWORDS = 3 * HALF + 4;
struct ReluLds {
  lds_i32* w;     // this lane's 16 bytes of slot 0, group 0
  lds_i32* m[4];  // the dword of them that this lane's c-th ds_max takes
};
__device__ __forceinline__ ReluLds relu_lds(lds_i32* base, int lane) {
  ReluLds L;
  L.w = base + 4 * lane;
#pragma unroll
  for (int c = 0; c < 4; ++c) L.m[c] = base + 4 * lane + ((c + (lane >> 3)) & 3);
  return L;
}
__device__ __forceinline__ float4 lds_ld4(const lds_i32* p) {  // ds_read_b128
  const i32x4v v = *reinterpret_cast<const lds_i32x4*>(p);
  return make_float4(__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]));
}
// DS instruction i (0..23) of the round trip of accumulator tile src through slot `slot`; the reads (i = 6g + 5) land in dst[4g .. 4g+3]
template <typename DST>
__device__ __forceinline__ void relu_lds_op(const ReluLds& L, const f32x16& src, DST& dst, int dst0, int slot, int i) {
  const int g = i / 6, j = i - 6 * g, off = (slot * 4 + g) * 256;
  if (j == 0) {
    const i32x4v v = {__float_as_int(src[4 * g]), __float_as_int(src[4 * g + 1]), __float_as_int(src[4 * g + 2]), __float_as_int(src[4 * g + 3])};
    *reinterpret_cast<lds_i32x4*>(L.w + off) = v;
  } else if (j < 5) {
    __hip_atomic_fetch_max(L.m[j - 1] + off, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
    const i32x4v v = *reinterpret_cast<lds_i32x4*>(L.w + off);
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[dst0 + c] = __int_as_float(v[c]);
  }
}

// acc[f] (+)= sum_k W[f-tile][k] * act(prev)[k]   over KB k-blocks of 8.
// prev = KB/4 register tiles in accumulator layout; RELU_IN: they are the previous layer's raw accumulators and the
// ReLU is applied lazily, one tile at a time, two k-blocks before the tile is first used -- VALU work in the shadow of
// the MFMA stream instead of a serial epilogue between layers.
// Two fragment stages: the A fragments of k-block kb+1 (or k-block 0 of the NEXT segment: NKB k-blocks, NNFT tiles) are
// requested at the top of k-block kb, i.e. 32 MFMAs = 2048 cycles before their first use; the scheduling barrier keeps
// the compiler from sinking the requests towards their uses.  st0 holds k-block 0 on entry and the next segment's
// k-block 0 on exit.  bv (8 bias rows of this lane) != nullptr: one extra MFMA per tile starts the accumulator
// at the bias (A = bias on every lane, B = 1 on lane half 0, C = 0).
// Training (SAVE = 1): the CONSUMER layer writes its activated input tiles to the row-major save buffer (lane (j, h) owns
// the 16-byte groups 32t + 8g + 4h of row j) and, for ReLU inputs, the u16 mask words in the tile kernels' layout.
// Gradient queries (SAVE = 2, the compact save): a ReLU-input layer writes only its mask words, the layer-0 input (gamma_p) only its rows
// -- the activation rows feed weight gradients alone, and a point gradient needs none.
struct SaveIn {
  float* rows;      // &save[tensor][this lane's row][4h]   (null = nothing to save); lanes past the end of the pass own a dump
                    // row behind the tensor (kernels.h: MSrows), so no store carries a predicate
  uint16_t* mask;   // &masks[layer][tile64][st][h*32 + j] (null = no masks); entry (f, wv) at + (f*2)*256 + wv*64
};

// LDS_RELU (never with SAVE = 1): a ReLU-input layer takes its input tiles through the LDS round trip above, ONE DS instruction behind
// each MFMA: tile t >= 1 behind the MFMAs of the second half of tile t - 1 (NFT = 8; from its second k-block on with NFT = 4), where the
// VALU form stood.  Tile 0 has no such lead -- it is complete 7 MFMAs before the producing layer ends -- so the PRODUCER (NEXT_RELU) sends
// group 0 of its accumulator tile 0 behind its last MFMAs and hands the registers over in `head`; the consumer sends groups 1..3
// behind the first 18 MFMAs of its first k-block (behind its bias MFMAs first, where it has them), each group well ahead of the
// k-block that reads it.
//
// NEXT_BIAS (never with SAVE = 1): the bias of the layer BEHIND this one enters as the start value of that layer's accumulators -- 16-byte
// loads that land in the accumulator registers, with no MFMA and no VALU, as the folded layer's dvec always did -- instead of one
// MFMA per tile (A = bias, B = 1, C = 0: 64 MFMA issue slots per layer that computed nothing).  This layer requests them, ONE load behind
// an MFMA: nb = that layer's bias + 4h (register 4g + r of tile t holds feature 32t + 8g + 4h + r), nacc = its accumulator tiles.  With
// NEXT_BIAS = 1 those are THIS layer's input tiles (the two sets ping-pong), and tile t may be overwritten once its last reader has gone:
// tile 0 in k-block 1, tile t >= 1 in k-block 4(t - 1) + 3, one k-block behind the ds_write / mask word that reads it last.  NEXT_BIAS = 2
// (layer 0, whose input is gamma_p): the tiles are free, tile t goes in k-block t.  The consuming layer then runs with bv = nullptr and
// ZERO_INIT = false.  (0 + b * 1 = b for every b but -0, which the MFMA form turned into +0; every such pre-activation goes through the
// integer ReLU, which gives +0 for both, and the mask words read `> 0`.)
__device__ __forceinline__ void bias_group(const float* b4h, int t, int g, f32x16& acc) {
  const float4 q = *reinterpret_cast<const float4*>(b4h + 32 * t + 8 * g);
  acc[4 * g + 0] = q.x;
  acc[4 * g + 1] = q.y;
  acc[4 * g + 2] = q.z;
  acc[4 * g + 3] = q.w;
}

template <int KB, int NFT, int NKB, int NNFT, bool ZERO_INIT, bool RELU_IN, int SAVE = 0, bool LDS_RELU = false, bool NEXT_RELU = false, int NEXT_BIAS = 0>
__device__ __forceinline__ void reg_layer(const int seg, const int next_seg /* float4 offsets into the packed image; < 0: none */, int lane,
                                          const f32x16* prev, f32x16* acc, WStage<8>& st0, const float* bv,
                                          const SaveIn sv, const RegBuf& rb, const ReluLds& rl, f32x4v& head,
                                          const float* nb = nullptr, f32x16* nacc = nullptr) {
  static_assert(!(LDS_RELU || NEXT_RELU || NEXT_BIAS) || SAVE != 1, "the saving forward keeps the VALU ReLU and the bias MFMAs");
  static_assert(NEXT_BIAS == 0 || ((LDS_RELU && RELU_IN) || NEXT_RELU), "the bias loads live in the stream with compile-time k-blocks");
  static_assert(NEXT_BIAS != 1 || (KB == 32 && RELU_IN), "NEXT_BIAS = 1 overwrites the 8 input tiles of a 256-wide ReLU layer");
  static_assert(NEXT_BIAS != 2 || KB == 8, "NEXT_BIAS = 2: one tile per k-block of layer 0");
  constexpr int KT = KB / 4;
  constexpr bool LR = LDS_RELU && RELU_IN;
  WStage<8> st1;
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (bv != nullptr) {  // accumulators start at the bias (same rounding order as ATen's addmm and as k_field_fwd)
    const float one_h0 = (lane < 32) ? 1.0f : 0.0f;
#pragma unroll
    for (int f = 0; f < NFT; ++f) acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[f], one_h0, zero, 0, 0, 0);
  }
  f32x16 tin[2];
  if constexpr (LR) {
#pragma unroll
    for (int c = 0; c < 4; ++c) tin[0][c] = head[c];
    if (bv != nullptr) {  // one behind each bias MFMA
#pragma unroll
      for (int i = 6; i < 14; ++i) relu_lds_op(rl, prev[0], tin[0], 4 * (i / 6), 0, i);
#pragma unroll
      for (int i = 6; i < 14; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x080, 1, 0);
      }
    }
  }
  [[maybe_unused]] const int lr0 = (bv != nullptr) ? 14 : 6;  // first DS instruction of tile 0 that goes behind the MFMAs of k-block 0
  auto mask_word = [&](int t) {  // gradient queries: the mask word comes from the raw accumulators, as in the VALU form
    unsigned bits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) bits |= (prev[t][r] > 0.f) ? (1u << r) : 0u;
    sv.mask[((t & 1) * 2) * 256 + (t >> 1) * 64] = (uint16_t)bits;
  };
  auto activate = [&](int t) {
    if constexpr (LR) {
      if (SAVE != 0) mask_word(t);
      return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tin[t & 1][r] = RELU_IN ? (SAVE == 1 ? fmaxf(prev[t][r], 0.f) : relu1(prev[t][r])) : prev[t][r];  // (the training variant's register allocation falls apart with the integer form)
    // pin the activated tile to this program point; without it the compiler hoists every tile's ReLU to the top of the
    // layer and spills ~370 registers
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(tin[t & 1][r]));
    if (SAVE == 1 || (SAVE == 2 && !RELU_IN)) {  // compile-time: such a layer always has rows, a SAVE && RELU_IN layer always has masks
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store_row4(sv.rows + 32 * t + 8 * g, make_float4(tin[t & 1][4 * g], tin[t & 1][4 * g + 1], tin[t & 1][4 * g + 2], tin[t & 1][4 * g + 3]));
    }
    if (SAVE != 0 && RELU_IN) {
      unsigned bits = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) bits |= (prev[t][r] > 0.f) ? (1u << r) : 0u;
      sv.mask[((t & 1) * 2) * 256 + (t >> 1) * 64] = (uint16_t)bits;  // feature tile t = (wave t>>1, f = t&1)
    }
  };
  activate(0);
  if constexpr (!(LR || NEXT_RELU)) {  // the VALU form, as it always was (the saving forward's register allocation hangs on this very text)
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    WStage<8>& ld = (kb & 1) ? st0 : st1;
    const WStage<8>& cur = (kb & 1) ? st1 : st0;
    if (kb + 1 < KB) {
#pragma unroll
      for (int f = 0; f < NFT; ++f) ld.w[f] = reg_ldw(rb, seg + (f * KB + kb + 1) * 64);
    } else if (next_seg >= 0) {
#pragma unroll
      for (int f = 0; f < NNFT; ++f) ld.w[f] = reg_ldw(rb, next_seg + (f * NKB) * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    if ((kb & 3) == 2 && (kb >> 2) + 1 < KT) activate((kb >> 2) + 1);  // next input tile, behind this k-block's MFMAs
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float b = tin[(kb >> 2) & 1][4 * (kb & 3) + s];
#pragma unroll
      for (int f = 0; f < NFT; ++f) {
        if (ZERO_INIT && bv == nullptr && kb == 0 && s == 0)
          acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(cur.w[f], s), b, zero, 0, 0, 0);
        else
          acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(cur.w[f], s), b, acc[f], 0, 0, 0);
      }
    }
  }
  } else {
  // The same stream with the DS instructions of the round trips behind its MFMAs.  The k-block is a compile-time constant here
  // (static_for): as a loop counter it leaves the DS schedule to the unroller, whose size limit the undecided body then exceeds.
  // DS instruction numbers that follow MFMA (k4, s, f) of tile kt: i0 of input tile 0, i1 of input tile kt + 1, i2 of output tile 0.
  auto ds0 = [&](int kt, int k4, int s, int f) { const int i = lr0 + (k4 * 4 + s) * NFT + f; return (LR && kt == 0 && i < 24) ? i : -1; };
  auto ds1 = [&](int kt, int k4, int s, int f) { const int i = (k4 * 4 + s) * NFT + f - (NFT == 8 ? 64 : 16); return (LR && kt + 1 < KT && i >= 0 && i < 24) ? i : -1; };
  auto ds2 = [&](int kt, int k4, int s, int f) { return (NEXT_RELU && kt == KT - 1 && k4 == 3 && s == 3 && f < 6) ? f : -1; };
  // the tile of the next layer's accumulators whose bias group f is requested behind MFMA (s = 0, f < 4) of k-block kb; -1: none
  auto nbt = [&](int kb, int s, int f) {
    if (NEXT_BIAS == 0 || s != 0 || f >= 4) return -1;
    if (NEXT_BIAS == 2) return kb;
    return kb == 1 ? 0 : (((kb & 3) == 3 && (kb >> 2) + 1 < KT) ? (kb >> 2) + 1 : -1);
  };
  static_for<0, KB>([&](auto kbc) __attribute__((always_inline)) {
    constexpr int kb = decltype(kbc)::value, kt = kb >> 2, k4 = kb & 3;
    WStage<8>& ld = (kb & 1) ? st0 : st1;
    const WStage<8>& cur = (kb & 1) ? st1 : st0;
    if (kb + 1 < KB) {
#pragma unroll
      for (int f = 0; f < NFT; ++f) ld.w[f] = reg_ldw(rb, seg + (f * KB + kb + 1) * 64);
    } else if (next_seg >= 0) {
#pragma unroll
      for (int f = 0; f < NNFT; ++f) ld.w[f] = reg_ldw(rb, next_seg + (f * NKB) * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (k4 == 2 && kt + 1 < KT) activate(kt + 1);  // (gradient queries: the mask word of the next input tile)
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float b = tin[kt & 1][4 * k4 + s];
#pragma unroll
      for (int f = 0; f < NFT; ++f) {
        if (ZERO_INIT && bv == nullptr && kb == 0 && s == 0)
          acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(cur.w[f], s), b, zero, 0, 0, 0);
        else
          acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4c(cur.w[f], s), b, acc[f], 0, 0, 0);
        const int i0 = ds0(kt, k4, s, f), i1 = ds1(kt, k4, s, f), i2 = ds2(kt, k4, s, f);
        if constexpr (LR) {
          if (i0 >= 0) relu_lds_op(rl, prev[0], tin[0], 4 * (i0 / 6), 0, i0);
          if (i1 >= 0) relu_lds_op(rl, prev[kt + 1], tin[(kt + 1) & 1], 4 * (i1 / 6), (kt + 1) & 1, i1);
        }
        if constexpr (NEXT_RELU) {
          if (i2 >= 0) relu_lds_op(rl, acc[0], head, 0, 0, i2);
        }
        if constexpr (NEXT_BIAS != 0) {
          const int tb = nbt(kb, s, f);
          if (tb >= 0) bias_group(nb, tb, f, nacc[tb]);
          any |= tb >= 0;
        }
        any |= i0 >= 0 || i1 >= 0 || i2 >= 0;
      }
    }
    // the order above is the order wanted: left alone the scheduler gathers each tile's DS instructions into bursts, and a burst holds
    // the wave's (in-order) issue until the LDS queue has drained -- the MFMAs behind it wait
    if (any) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int f = 0; f < NFT; ++f) {
          const int n = (ds0(kt, k4, s, f) >= 0) + (ds1(kt, k4, s, f) >= 0) + (ds2(kt, k4, s, f) >= 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (n == 1) __builtin_amdgcn_sched_group_barrier(0x080, 1, 0);
          if (n == 2) __builtin_amdgcn_sched_group_barrier(0x080, 2, 0);
          if (nbt(kb, s, f) >= 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
    }
  });
  }
  if (KB & 1) st0 = st1;  // (all segments have an even number of k-blocks: the next k-block 0 already sits in st0)
}

// bias rows of this lane (requested before the layer's k loop, consumed after it)
template <int NFT>
__device__ __forceinline__ void bias_load(const float* __restrict__ bias, int lane, float (&bv)[8]) {
#pragma unroll
  for (int f = 0; f < NFT; ++f) bv[f] = bias[f * 32 + (lane & 31)];
}

#ifdef NERF_STAMPS  // diagnostic build only (make stamps): cycle sums per phase, see scripts/phase_stamps.py
#define RSTAMP(slot)                                            \
  do {                                                          \
    __builtin_amdgcn_sched_barrier(0);                          \
    const unsigned long long t_ = __builtin_readcyclecounter(); \
    __builtin_amdgcn_sched_barrier(0);                          \
    tsum[slot] += t_ - tlast;                                   \
    tlast = t_;                                                 \
  } while (0)
#else
#define RSTAMP(slot) do { } while (0)
#endif

// Where a wave's 32 samples come from.  SRC_RAYS: a ray record and a depth per sample (sample_point; the forward passes, q unused).
// SRC_POINTS / SRC_LATTICE: the point queries (nerf_hip_query / nerf_hip_density_grid) -- sample m IS point m (no ray record, one
// dvec row per point): p = q.points[m], or the lattice point q.lo + (i, j, k) * q.step of m = (i * ny + j) * nz + k.
// RGB = false: sigma only -- the folded point_info / dir_info layer (512 of the 8,256 MFMAs per tile) and the colour head are skipped.
// The query forms are template arguments of THIS kernel rather than a shared inline body: moving the body into a function changes the
// register allocation of the forward instantiations, and these must stay instruction for instruction what they were.
// GSAVE (gradient queries, SRC_POINTS only; nerf_hip_query_grad): the compact save that k_field_bwd_reg's query form reads -- the ReLU
// masks of h0..h7, spre, gamma_p rows and (RGB) the c rows, laid out as kernels.h QGRAD_* describes; no activation rows.
// SRC_CORNERS / SRC_BLOCKS (sigma only; the narrow-band grid, nerf_hip_band_begin / nerf_hip_band_grow): sample m maps by integer
// arithmetic to a lattice index (kernels.h QuerySrc) -- the strided, clamped corner lattice, or a listed block's local point -- and from
// there to p exactly as SRC_LATTICE does; sigma goes to the dense grid at the point's own linear index, so the bits are density_grid's.
// Points of a ragged last block past the grid are computed on the clamped index and not stored.
enum { SRC_RAYS = 0, SRC_POINTS = 1, SRC_LATTICE = 2, SRC_CORNERS = 3, SRC_BLOCKS = 4 };

template <bool SAVE, bool DEBUG, int SRC = SRC_RAYS, bool RGB = true, bool GSAVE = false>
__global__ __launch_bounds__(64, 1) void k_field_fwd_reg(const FieldArgs a, const QuerySrc q) {
#ifdef NERF_STAMPS
  unsigned long long tsum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tlast = __builtin_readcyclecounter();
#endif
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * RM;
  const int m = m0 + j;
  const bool valid = m < a.M;
  const int mc = valid ? m : a.M - 1;
  const int ray = (SRC == SRC_RAYS) ? mc / a.N : mc;  // (the row of dvec)
  const float* rf = (SRC == SRC_RAYS) ? a.rayf + (size_t)ray * RAYF : nullptr;
  const float4* wp = a.wp;
  const RegBuf rb = reg_buf(a.wp, threadIdx.x);  // (64-thread workgroups: threadIdx.x is the lane)

  // first fragments of layer 0 are requested before anything else
  WStage<8> st0;
  stage_load<8, 8>(wp + seg_off4(SEG_L0) + lane, 0, st0);
  // the inference forms take the lazy ReLU through LDS (reg_layer) and keep the colour head's operands there; the saving forward allocates none
  constexpr bool LR = !SAVE;
  constexpr bool COL_LDS = LR && RGB;
  [[maybe_unused]] float4 cw0, cw1;  // W_color: 96 float4, lane l brings l and (l < 32) 64 + l; b_color: lanes 0..2
  [[maybe_unused]] float cb;
  if constexpr (COL_LDS) {
    const float4* wc4 = reinterpret_cast<const float4*>(a.w.p[W_COLOR]);
    cw0 = wc4[lane];
    cw1 = wc4[64 + j];
    cb = a.w.p[B_COLOR][lane < 3 ? lane : 2];
  }

  // ---- sample point and its encoding, straight into B-operand registers:
  // gp[t][4g + s] = gamma_p[k], k = 32t + 8g + 4h + s  (4 consecutive k = two (sin, cos) pairs)
  float p[3];
  [[maybe_unused]] bool band_keep = false;  // SRC_CORNERS / SRC_BLOCKS: this lane's point is stored, at band_at of the dense grid
  [[maybe_unused]] size_t band_at = 0;
  if constexpr (SRC == SRC_RAYS) {
    sample_point(rf, a.t[mc], p);
  } else if constexpr (SRC == SRC_POINTS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = q.points[(size_t)mc * 3 + c];
  } else if constexpr (SRC == SRC_LATTICE) {  // C order, z fastest; product and sum rounded separately (-ffp-contract=off): p is lo + (float)i * step bit for bit
    const int iz = mc % q.nz, ixy = mc / q.nz;
    const int iy = ixy % q.ny, ix = ixy / q.ny;
    p[0] = q.lo[0] + (float)ix * q.step[0];
    p[1] = q.lo[1] + (float)iy * q.step[1];
    p[2] = q.lo[2] + (float)iz * q.step[2];
  } else {
    static_assert(!RGB && !SAVE && !GSAVE && !DEBUG, "the band forms are sigma-only inference");
    const unsigned n[3] = {(unsigned)q.nx, (unsigned)q.ny, (unsigned)q.nz};
    unsigned idx[3];
    band_keep = valid;
    if constexpr (SRC == SRC_CORNERS) {
      const unsigned uz = (unsigned)mc % (unsigned)q.ext[2], uxy = (unsigned)mc / (unsigned)q.ext[2];
      idx[0] = uxy / (unsigned)q.ext[1] * (unsigned)q.r;
      idx[1] = uxy % (unsigned)q.ext[1] * (unsigned)q.r;
      idx[2] = uz * (unsigned)q.r;
    } else {
      const unsigned vol = (unsigned)(q.ext[0] * q.ext[1] * q.ext[2]);
      const unsigned e = (unsigned)mc / vol, l = (unsigned)mc - e * vol;
      band_keep = band_keep && (long long)q.e0 + e < *q.nlist;
      const unsigned b = band_keep ? (unsigned)q.list[(size_t)q.e0 + e] : 0u;
      const unsigned lz = l % (unsigned)q.ext[2], lxy = l / (unsigned)q.ext[2];
      const unsigned bz = b % (unsigned)q.nbz, bxy = b / (unsigned)q.nbz;
      idx[0] = bxy / (unsigned)q.nby * (unsigned)q.r + lxy / (unsigned)q.ext[1];
      idx[1] = bxy % (unsigned)q.nby * (unsigned)q.r + lxy % (unsigned)q.ext[1];
      idx[2] = bz * (unsigned)q.r + lz;
      band_keep = band_keep && idx[0] < n[0] && idx[1] < n[1] && idx[2] < n[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) idx[c] = idx[c] < n[c] ? idx[c] : n[c] - 1u;
    band_at = ((size_t)idx[0] * n[1] + idx[1]) * n[2] + idx[2];
    p[0] = q.lo[0] + (float)(int)idx[0] * q.step[0];
    p[1] = q.lo[1] + (float)(int)idx[1] * q.step[1];
    p[2] = q.lo[2] + (float)(int)idx[2] * q.step[2];
  }
  if (DEBUG && a.pts_dbg && valid && h == 0) {
    a.pts_dbg[(size_t)m * 3 + 0] = p[0];
    a.pts_dbg[(size_t)m * 3 + 1] = p[1];
    a.pts_dbg[(size_t)m * 3 + 2] = p[2];
  }
  // The pair index 4 g8 + 2 h + e depends on the lane half, so with the frequency table indexed by it every pair paid a dependent
  // global load (s_getpc + global_load_dword + s_waitcnt vmcnt(0): 16 exposed round trips per tile, each also waiting for the layer-0
  // fragments above) inside an exec-mask region of its own.  For fixed (g8, e) both candidates are compile-time values: frequency and
  // coordinate are selected on h from literals / registers, the zero padding (pairs 30, 31 = lane half 1 of g8 = 7) is a select too.
  // No memory, no branch: the encode is one block of VALU work in front of layer 0's first k-step, waiting for nothing but the sample point.
  f32x16 gp[2];
  static_for<0, 16>([&](auto ic) __attribute__((always_inline)) {
    constexpr int g8 = decltype(ic)::value >> 1, e = decltype(ic)::value & 1;
    constexpr int pa = 4 * g8 + e, pb = pa + 2;  // (sin, cos) pair index on lane half 0 / 1: k = 2 pi
    constexpr bool pad = pb >= 30;               // (lane half 1 computes half 0's pair and drops it)
    constexpr int ca = pa / 10, la = pa - 10 * ca, cb = pad ? ca : pb / 10, lb = pad ? la : pb - 10 * cb;
    static_assert(pa < 30, "lane half 0 never pads");
    constexpr uint32_t fa = kFreqPointLit[la], fb = kFreqPointLit[lb];
    const float x = (ca == cb) ? p[ca] : (h ? p[cb] : p[ca]);
    const float f = (la == lb) ? __uint_as_float(fa) : (h ? __uint_as_float(fb) : __uint_as_float(fa));
    float sv, cv;
    sincos_phase(x * f, sv, cv);
    if (pad) {
      sv = h ? 0.f : sv;
      cv = h ? 0.f : cv;
    }
    gp[g8 >> 2][4 * (g8 & 3) + 2 * e] = sv;
    gp[g8 >> 2][4 * (g8 & 3) + 2 * e + 1] = cv;
  });
  if (DEBUG && a.gp_dbg && valid) {
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 8 * g8 + 4 * h + s;
        if (k < POINT_DIM) a.gp_dbg[(size_t)m * POINT_DIM + k] = gp[g8 >> 2][4 * (g8 & 3) + s];
      }
  }

  // training: where this lane's rows / mask words go (rows of the coarse pass first, then the fine pass)
  const size_t MS = (size_t)a.MSrows * WIDTH;
  const long long rrow = valid ? (long long)(a.row0 + m) : a.Mtot + j;  // lanes past the end: dump row
  float* const srow = SAVE ? a.save + (size_t)rrow * WIDTH + 4 * h : nullptr;
  uint16_t* const mrow = (SAVE || GSAVE) ? a.masks + ((size_t)(a.tile0 + (m0 >> 6)) * 4 + ((m0 >> 5) & 1)) * 256 + h * 32 + j : nullptr;
  const size_t MKS = (size_t)a.tiles_tot * 4 * 256;
  auto sv_rows = [&](int tensor) { return SaveIn{SAVE ? srow + (size_t)tensor * MS : nullptr, nullptr}; };
  auto sv_relu = [&](int layer) { return SaveIn{SAVE ? srow + (size_t)layer * MS : nullptr, SAVE ? mrow + (size_t)layer * MKS : nullptr}; };
  // gradient queries: gamma_p rows of QGRAD_GP floats, then (RGB) c rows of QGRAD_C floats, MSrows rows each
  float* const gprow = GSAVE ? a.save + (size_t)rrow * QGRAD_GP + 4 * h : nullptr;
  float* const crow = GSAVE ? a.save + (size_t)a.MSrows * QGRAD_GP + (size_t)rrow * QGRAD_C + 4 * h : nullptr;
  constexpr int SV = SAVE ? 1 : (GSAVE ? 2 : 0);
  auto sv_in = [&](int layer) { return GSAVE ? SaveIn{nullptr, mrow + (size_t)layer * MKS} : sv_relu(layer); };

  ReluLds rl{};
  [[maybe_unused]] lds_i32* col = nullptr;
  if constexpr (LR) {
    __shared__ int relu_slots[RELU_LDS_DWORDS + (COL_LDS ? COL_LDS_DWORDS : 0)];
    rl = relu_lds((lds_i32*)relu_slots, lane);
    if constexpr (COL_LDS) {  // (a one-wave workgroup: its DS instructions execute in order, the reads at the end need no barrier)
      col = (lds_i32*)relu_slots + RELU_LDS_DWORDS;
      const i32x4v v0 = {__float_as_int(cw0.x), __float_as_int(cw0.y), __float_as_int(cw0.z), __float_as_int(cw0.w)};
      const i32x4v v1 = {__float_as_int(cw1.x), __float_as_int(cw1.y), __float_as_int(cw1.z), __float_as_int(cw1.w)};
      *reinterpret_cast<lds_i32x4*>(col + 4 * lane) = v0;
      *reinterpret_cast<lds_i32x4*>(col + 4 * (64 + j)) = v1;  // (both halves write the same 16 bytes)
      col[3 * HALF + (lane < 3 ? lane : 2)] = __float_as_int(cb);
    }
  }
  f32x4v head = {0.f, 0.f, 0.f, 0.f};  // group 0 of the next layer's input tile 0, activated (LR only)
  RSTAMP(0);  // prologue: ray / depth loads, sample point, positional encoding
  // two accumulator sets ping-pong: a layer reads the previous layer's raw accumulators (ReLU applied lazily)
  f32x16 A[8], B[8];
  constexpr int L256 = 8 * 32 * 64;  // float4 per 256x256 segment
  constexpr int sL1 = seg_off4(SEG_L1);
  constexpr int sL5 = seg_off4(SEG_L5);
  float bv[8];
  // The inference forms start every layer's accumulators at its bias with loads (reg_layer's NEXT_BIAS: requested by the layer in front,
  // layer 0's own right here); the saving forward keeps one bias MFMA per tile.  bl(i): the bias rows of weights24[i] for this lane half
  constexpr bool BL = LR;
  constexpr int NB1 = BL ? 1 : 0;
  auto bl = [&](int i) { return BL ? a.w.p[i] + 4 * h : nullptr; };
  auto bias_mfma = [&](int i) -> const float* {
    if constexpr (BL) return nullptr;
    bias_load<8>(a.w.p[i], lane, bv);
    return bv;
  };
  if constexpr (BL) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) bias_group(bl(B_L0), t, g, A[t]);
  }

  // ---- layer 0: gamma_p 60(64) -> 256
  reg_layer<8, 8, 32, 8, !BL, false, SV, LR, LR, BL ? 2 : 0>(seg_off4(SEG_L0), sL1, lane, gp, A, st0, bias_mfma(B_L0), GSAVE ? SaveIn{gprow, nullptr} : sv_rows(S_GP), rb, rl, head, bl(3), B);
  RSTAMP(1);  // layer 0 (256 MFMAs; the saving forward: 264)
  // ---- layers 1..3 (the segment after L3 is L4A: same shape)
  reg_layer<32, 8, 32, 8, !BL, true, SV, LR, LR, NB1>(sL1, sL1 + L256, lane, A, B, st0, bias_mfma(3), sv_in(0), rb, rl, head, bl(5), A);
  reg_layer<32, 8, 32, 8, !BL, true, SV, LR, LR, NB1>(sL1 + L256, sL1 + 2 * L256, lane, B, A, st0, bias_mfma(5), sv_in(1), rb, rl, head, bl(7), B);
  reg_layer<32, 8, 32, 8, !BL, true, SV, LR, LR, NB1>(sL1 + 2 * L256, seg_off4(SEG_L4A), lane, A, B, st0, bias_mfma(7), sv_in(2), rb, rl, head, bl(9), A);
  RSTAMP(2);  // layers 1..3 (3,072 MFMAs; the saving forward: 3,096)
  // ---- layer 4: cat(h3, gamma_p), hidden first (nerf.py:109); its first part requests layer 5's bias
  reg_layer<32, 8, 8, 8, !BL, true, SV, LR, false, NB1>(seg_off4(SEG_L4A), seg_off4(SEG_L4B), lane, B, A, st0, bias_mfma(9), sv_in(3), rb, rl, head, bl(11), B);
  reg_layer<8, 8, 32, 8, false, false, 0, LR, LR>(seg_off4(SEG_L4B), sL5, lane, gp, A, st0, nullptr, SaveIn{nullptr, nullptr}, rb, rl, head);
  RSTAMP(3);  // layer 4 (1,280 MFMAs; the saving forward: 1,288)
  // ---- layers 5..7 (the segment after L7 is the folded point_info / dir_info layer: 4 tiles)
  reg_layer<32, 8, 32, 8, !BL, true, SV, LR, LR, NB1>(sL5, sL5 + L256, lane, A, B, st0, bias_mfma(11), sv_in(4), rb, rl, head, bl(13), A);
  reg_layer<32, 8, 32, 8, !BL, true, SV, LR, LR, NB1>(sL5 + L256, sL5 + 2 * L256, lane, B, A, st0, bias_mfma(13), sv_in(5), rb, rl, head, bl(15), B);
  reg_layer<32, 8, 32, 4, !BL, true, SV, LR, false>(sL5 + 2 * L256, RGB ? seg_off4(SEG_FOLD) : -1, lane, A, B, st0, bias_mfma(15), sv_in(6), rb, rl, head);
  RSTAMP(4);  // layers 5..7 (3,072 MFMAs; the saving forward: 3,096)
  // ---- sigma head on h7 = relu(B) (VALU): sigma = |w_sigma . h7 + b|  (nerf.py:94, 115)
  {
    const float* ws = a.w.p[W_SIGMA] + 4 * h;
    float s = 0.f;
    // weights one tile ahead of their use, in explicit groups: under the register pressure of the training variant the
    // compiler otherwise issues the 32 loads one at a time, each followed by a full wait
    float4 wq[2][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) wq[0][g] = *reinterpret_cast<const float4*>(ws + 8 * g);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (t + 1 < 8) {
#pragma unroll
        for (int g = 0; g < 4; ++g) wq[(t + 1) & 1][g] = *reinterpret_cast<const float4*>(ws + 32 * (t + 1) + 8 * g);
      }
      if (SAVE) __builtin_amdgcn_sched_barrier(0);
      if (GSAVE) {  // the mask of h7, here in both forms (the fold layer, which stores it in training, does not run without colour)
        unsigned bits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) bits |= (B[t][r] > 0.f) ? (1u << r) : 0u;
        mrow[7 * MKS + ((t & 1) * 2) * 256 + (t >> 1) * 64] = (uint16_t)bits;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 q = wq[t & 1][g];
        s = __builtin_fmaf(relu1(B[t][4 * g + 0]), q.x, s);
        s = __builtin_fmaf(relu1(B[t][4 * g + 1]), q.y, s);
        s = __builtin_fmaf(relu1(B[t][4 * g + 2]), q.z, s);
        s = __builtin_fmaf(relu1(B[t][4 * g + 3]), q.w, s);
      }
      if (SAVE) __builtin_amdgcn_sched_barrier(0);
    }
    s += __shfl_xor(s, 32);
    if constexpr (SRC == SRC_CORNERS || SRC == SRC_BLOCKS) {
      if (band_keep && h == 0) a.sigma[band_at] = fabsf(s + a.w.p[B_SIGMA][0]);
    } else if (valid && h == 0) {
      const float pre = s + a.w.p[B_SIGMA][0];
      a.sigma[m] = fabsf(pre);
      if (SAVE || GSAVE) a.spre[a.row0 + m] = pre;
    }
  }
  RSTAMP(5);  // sigma head
  if constexpr (!RGB) return;
  // ---- point_info (256 -> 256, no activation) and dir_info's feature columns as ONE 128 x 256 layer on h7 (common.h SEG_FOLD):
  // c = relu(W_fold h7 + dvec), dvec (per ray) = b_dir + W_dir[:, :24] gamma_d + W_dir[:, 24:] b_pi = the accumulator start
  {
    const float* dv = a.dvec + (size_t)ray * HALF + 4 * h;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 q = *reinterpret_cast<const float4*>(dv + 32 * f + 8 * g);
        A[f][4 * g + 0] = q.x;
        A[f][4 * g + 1] = q.y;
        A[f][4 * g + 2] = q.z;
        A[f][4 * g + 3] = q.w;
      }
  }
  // (the VALU ReLU in every form: the sigma head above has just activated all of h7 for its own use and the compiler shares those
  // registers with this layer, so its input costs nothing more; sent through LDS as well, this layer measured 750 cycles per tile slower)
  reg_layer<32, 4, 32, 4, false, true, SAVE, false, false>(seg_off4(SEG_FOLD), -1, lane, B, A, st0, nullptr, GSAVE ? SaveIn{nullptr, nullptr} : sv_relu(7), rb, rl, head);
  RSTAMP(6);  // point_info + dir_info folded (512 MFMAs)
  // ---- colour head (VALU): rgb = sigmoid(W_c relu(.) + b)  (nerf.py:99, 119)
  {
    const float* wc = a.w.p[W_COLOR] + 4 * h;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 q0, q1, q2;
        if constexpr (COL_LDS) {
          q0 = lds_ld4(col + 4 * h + 32 * t + 8 * g);
          q1 = lds_ld4(col + 4 * h + HALF + 32 * t + 8 * g);
          q2 = lds_ld4(col + 4 * h + 2 * HALF + 32 * t + 8 * g);
        } else {
          q0 = *reinterpret_cast<const float4*>(wc + 32 * t + 8 * g);
          q1 = *reinterpret_cast<const float4*>(wc + HALF + 32 * t + 8 * g);
          q2 = *reinterpret_cast<const float4*>(wc + 2 * HALF + 32 * t + 8 * g);
        }
        const float c0 = relu1(A[t][4 * g + 0]), c1 = relu1(A[t][4 * g + 1]);
        const float c2 = relu1(A[t][4 * g + 2]), c3 = relu1(A[t][4 * g + 3]);
        if (SAVE) store_row4(srow + S_C * MS + 32 * t + 8 * g, make_float4(c0, c1, c2, c3));
        if (GSAVE) store_row4(crow + 32 * t + 8 * g, make_float4(c0, c1, c2, c3));
        z0 = __builtin_fmaf(c3, q0.w, __builtin_fmaf(c2, q0.z, __builtin_fmaf(c1, q0.y, __builtin_fmaf(c0, q0.x, z0))));
        z1 = __builtin_fmaf(c3, q1.w, __builtin_fmaf(c2, q1.z, __builtin_fmaf(c1, q1.y, __builtin_fmaf(c0, q1.x, z1))));
        z2 = __builtin_fmaf(c3, q2.w, __builtin_fmaf(c2, q2.z, __builtin_fmaf(c1, q2.y, __builtin_fmaf(c0, q2.x, z2))));
      }
    z0 += __shfl_xor(z0, 32);
    z1 += __shfl_xor(z1, 32);
    z2 += __shfl_xor(z2, 32);
    float bc[3];
    if constexpr (COL_LDS) {  // every lane, one address: no load inside the branch
      const float4 b = lds_ld4(col + 3 * HALF);
      bc[0] = b.x, bc[1] = b.y, bc[2] = b.z;
    }
    if (valid && h == 0) {
      if constexpr (!COL_LDS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) bc[c] = a.w.p[B_COLOR][c];
      }
      a.rgb[(size_t)m * 3 + 0] = 1.0f / (1.0f + expf(-(z0 + bc[0])));
      a.rgb[(size_t)m * 3 + 1] = 1.0f / (1.0f + expf(-(z1 + bc[1])));
      a.rgb[(size_t)m * 3 + 2] = 1.0f / (1.0f + expf(-(z2 + bc[2])));
    }
  }
#ifdef NERF_STAMPS
  RSTAMP(7);  // colour head + stores
  if (a.stamps && lane == 0) {
    for (int i = 0; i < 8; ++i) atomicAdd(a.stamps + i, tsum[i]);
    atomicAdd(a.stamps + 31, 1ull);
  }
#endif
}

hipError_t launch_field_fwd_reg(const FieldArgs& a, bool save, hipStream_t st) {
  const int tiles = (a.M + RM - 1) / RM;
  if (save)
    hipLaunchKernelGGL((k_field_fwd_reg<true, false>), dim3(tiles), dim3(64), 0, st, a, QuerySrc{});
  else if (a.pts_dbg || a.gp_dbg)
    hipLaunchKernelGGL((k_field_fwd_reg<false, true>), dim3(tiles), dim3(64), 0, st, a, QuerySrc{});
  else
    hipLaunchKernelGGL((k_field_fwd_reg<false, false>), dim3(tiles), dim3(64), 0, st, a, QuerySrc{});
  return hipGetLastError();
}

hipError_t launch_query_grad_fwd(const FieldArgs& a, const QuerySrc& q, bool rgb, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)(((long long)a.M + RM - 1) / RM);
  if (rgb)
    hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_POINTS, true, true>), dim3(tiles), dim3(64), 0, st, a, q);
  else
    hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_POINTS, false, true>), dim3(tiles), dim3(64), 0, st, a, q);
  return hipGetLastError();
}

hipError_t launch_query_reg(const FieldArgs& a, const QuerySrc& q, bool rgb, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  const unsigned tiles = (unsigned)(((long long)a.M + RM - 1) / RM);
  if (q.points == nullptr)
    hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_LATTICE, false>), dim3(tiles), dim3(64), 0, st, a, q);
  else if (rgb)
    hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_POINTS, true>), dim3(tiles), dim3(64), 0, st, a, q);
  else
    hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_POINTS, false>), dim3(tiles), dim3(64), 0, st, a, q);
  return hipGetLastError();
}

hipError_t launch_band_corners(const FieldArgs& a, const QuerySrc& q, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_CORNERS, false>), dim3((unsigned)(((long long)a.M + RM - 1) / RM)), dim3(64), 0, st, a, q);
  return hipGetLastError();
}

hipError_t launch_band_blocks(const FieldArgs& a, const QuerySrc& q, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_field_fwd_reg<false, false, SRC_BLOCKS, false>), dim3((unsigned)(((long long)a.M + RM - 1) / RM)), dim3(64), 0, st, a, q);
  return hipGetLastError();
}

}  // namespace nerf
