// bf16_split.h -- the two-part (hi + mid) form of the bf16 stream machinery, shared by the split-fp32 forward (field_fwd_split.hip) and
// backward chain (field_bwd_split.hip): every fp32 operand x = hi + mid + (rest), hi = bf16(x), mid = bf16(x - hi); the stream
// interleaves the two parts of every fragment of a bf16 stream of bf16_common.h (fragment 2 s = hi, 2 s + 1 = mid of step s), and a
// k-step is three MFMAs.  MI355X / gfx950 only.
#pragma once
#include "bf16_stream.h"
#include "bf16_weights.h"

namespace nerf {

// two fp32 values -> their hi parts (packed bf16 pair) and mid parts
struct HiMid { unsigned hi, mid; };
__device__ __forceinline__ HiMid split2(float x0, float x1) {
  HiMid r;
  r.hi = pack2(x0, x1);
  const float h0 = __uint_as_float(r.hi << 16), h1 = __uint_as_float(r.hi & 0xffff0000u);
  r.mid = pack2(x0 - h0, x1 - h1);
  return r;
}

struct EpiTmp { float x0, x1; unsigned hi; };  // state of one register pair between the three phases of its conversion
// a ReLU'd value is >= +0: alive (its ReLU passes the gradient) <=> its bit pattern is >= 1; bit 15 - r of a tile's mask word = register r
__device__ __forceinline__ unsigned alive_pair(float x0, float x1, int r) {
  return ((unsigned)min(__float_as_int(x0), 1) << (15 - r)) | ((unsigned)min(__float_as_int(x1), 1) << (14 - r));
}

// Segment ROW of the bf16 stream S::SEGS, in two parts: NFT output tiles x (KSA + KSB) k-steps starting at STEP S0 (fragments 2 S0 ..);
// inputs inA (k-steps 0..KSA-1) then inB, each as hi / mid parts.  Per step three MFMAs, the small products first.  Accumulator hand-over
// as in bf_segment (BT0 < 0: no biases, the accumulators start at zero), except that the epilogue of the finished tile is SPREAD: with
// one wave per SIMD nothing else fills the matrix pipe while this wave converts, so the 8 register pairs of a tile (epi(f, part, phase,
// acc, tmp): ~13 vector instructions each) go one per k-step behind k-steps 2 .. 9 of the next tile -- about four vector instructions
// per MFMA, which the 32-cycle MFMA hides -- instead of ~110 in one lump.  Segments shorter than ten k-steps keep the lump.
// (bf16_stream.h bf_burst_kstep is this rule for the store schedule.)
template <class S, int ROW, class Epi, class PrevEpi>
__device__ __forceinline__ void sp_segment(const BfCtx& c, u32x4 (&fr)[S::D], f32x16 (&acc)[2], const u32x4* inA_hi, const u32x4* inA_mid,
                                           const u32x4* inB_hi, const u32x4* inB_mid, Epi&& epi, PrevEpi&& prev_epi) {
  constexpr BfSeg G = S::SEGS[ROW];
  constexpr int S0 = G.s0, NFT = G.nft, KSA = G.ksa, KSB = G.ksb, BT0 = G.bt0, KS = KSA + KSB;
  constexpr int P0 = bf_seg_p0(S::SEGS, ROW), NEXT_BT = bf_seg_next_bt(S::SEGS, S::NSEG, ROW);
  constexpr int LAST = bf_burst_kstep(2, KS);  // k-step behind which the finished accumulator is free again
  constexpr bool SPREAD = LAST != BF_EPI_POS;
  static_assert(KS > LAST, "segment too short for the deferred epilogue");
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  EpiTmp tmp = {0.f, 0.f, 0u};
  static_for<NFT * KS>([&](auto I) {
    constexpr int f = I / KS, ks = I % KS, i0 = 2 * (S0 + I), i1 = i0 + 1;
    constexpr int cur = (P0 + f) & 1, oth = (P0 + f + 1) & 1;
    constexpr bool EPI = SPREAD && ks >= BF_EPI_POS && ks <= LAST;
    auto phase = [&](auto PH) {  // one third of the conversion of register pair ks - BF_EPI_POS of the finished tile, behind ONE MFMA
      if constexpr (EPI) {
        if constexpr (f == 0)
          prev_epi(ks - BF_EPI_POS, (int)PH, acc[oth], tmp);
        else
          epi(f - 1, ks - BF_EPI_POS, (int)PH, acc[oth], tmp);
      }
    };
    if constexpr (i0 % BF_CHUNK == BF_SYNC_POS) bf_sync<S, i0 / BF_CHUNK>(c);
    const u32x4 a_hi = fr[i0 % S::D];
    if constexpr (i0 + S::D < S::NFRAG) fr[i0 % S::D] = bf_frag<S>(c, i0 + S::D);
    const u32x4 a_mid = fr[i1 % S::D];
    if constexpr (i1 + S::D < S::NFRAG) fr[i1 % S::D] = bf_frag<S>(c, i1 + S::D);
    const u32x4& b_hi = ks < KSA ? inA_hi[ks < KSA ? ks : 0] : inB_hi[ks < KSA ? 0 : ks - KSA];
    const u32x4& b_mid = ks < KSA ? inA_mid[ks < KSA ? ks : 0] : inB_mid[ks < KSA ? 0 : ks - KSA];
    // program order = issue order for one wave per SIMD: every MFMA is followed by its share of vector work, and the fences keep
    // the compiler from collecting that work into lumps the matrix pipe would have to wait for
    acc[cur] = bf_mfma(a_mid, b_hi, acc[cur]);
    phase(std::integral_constant<int, 0>{});
    if constexpr (EPI) __builtin_amdgcn_sched_barrier(0);
    acc[cur] = bf_mfma(a_hi, b_mid, acc[cur]);
    phase(std::integral_constant<int, 1>{});
    if constexpr (EPI) __builtin_amdgcn_sched_barrier(0);
    acc[cur] = bf_mfma(a_hi, b_hi, acc[cur]);
    phase(std::integral_constant<int, 2>{});
    if constexpr (EPI) __builtin_amdgcn_sched_barrier(0);
    if constexpr (!SPREAD && ks == BF_EPI_POS) {
      static_for<8>([&](auto P) {
        static_for<3>([&](auto PH) {
          if constexpr (f == 0)
            prev_epi((int)P, (int)PH, acc[oth], tmp);
          else
            epi(f - 1, (int)P, (int)PH, acc[oth], tmp);
        });
      });
    }
    if constexpr (ks == LAST) {
      if constexpr (f + 1 < NFT)
        acc[oth] = BT0 >= 0 ? bf_bias_tile(c, BT0 + f + 1) : zero;
      else if constexpr (NEXT_BT >= 0)
        acc[oth] = bf_bias_tile(c, NEXT_BT);
      else
        acc[oth] = zero;
    }
  });
}

// one lane's hi and mid 16 bytes of fragment pair `frag` of a two-part weight image (bf16_weights.h frag_lane)
struct FragHiMid { u32x4 hi, mid; };
template <int ROWS, WeightFn W>
__device__ __forceinline__ FragHiMid frag_lane_split(const Weights24& w, const float* __restrict__ fold, int frag, int lane) {
  FragHiMid v;
  frag_lane<ROWS, W>(w, fold, frag, lane, [&](int q, float x0, float x1) {
    const HiMid e = split2(x0, x1);
    v.hi[q] = e.hi;
    v.mid[q] = e.mid;
  });
  return v;
}

}  // namespace nerf
