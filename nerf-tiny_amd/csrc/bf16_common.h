// bf16_common.h -- layout of the bf16 weight STREAM used by the bf16-MLP variant of the field query (cfg3 of
// BASELINE.json: "bf16 MLP / fp32 composite").  MI355X / gfx950 only.
//
// Arithmetic of the variant (restated by tests/test_gpu_bf16.py's torch emulation): every linear layer of the field
// MLP (nerf.py:78-99) multiplies bf16-rounded weights with bf16-rounded inputs, accumulates in fp32 starting from the
// fp32 bias, and hands its (ReLU'd) output to the next layer rounded to bf16 (round-to-nearest-even).  The positional
// encodings are computed in fp32 exactly as in the fp32 path and rounded to bf16 once.  sigma = |.| and the colour sigmoid are
// fp32 on the fp32 accumulators; everything outside the MLP (rays, depths, compositing, resampling, sort) stays fp32.
//
// The image holds one v_mfma_f32_32x32x16_bf16 A fragment (32 output features x 16 inputs, 8 bf16 = 16 bytes per lane,
// 1 KiB per wave) per MFMA, in the exact order a wave consumes them: layer by layer, output tile by output tile,
// k-step by k-step.  Lane (i, h) of fragment (f, ks) holds W[32f + i][k] for the 8 inputs
//     k = 16ks + 4h + {0,1,2,3} and 16ks + 8 + 4h + {0,1,2,3}
// which is where the 32x32 fp32 accumulator layout leaves them: lane (sample j, half h) of an accumulator tile holds
// features 8g + 4h + r of sample j (register 4g + r), so registers 0..7 / 8..15 of tile t, converted pairwise to bf16,
// ARE the B operands of k-steps 2t / 2t + 1 of the next layer -- no shuffle, no LDS round trip for activations.
// In front of the fragments sits one 16-KiB block with the fp32 biases per output tile.
#pragma once
#include "common.h"

namespace nerf {

constexpr int BF_FRAG_BYTES = 1024;
constexpr int BF_CHUNK = 16;              // fragments per LDS ring slot (16 KiB)
constexpr int BF_BIAS_BYTES = 16384;      // bias block (70 tiles x 32 floats used)

// ---- ONE description per stream: a row per segment.  Everything else that restates a stream's shape -- the BFS_* / BBS_* offsets below, the
// accumulator parity and the next bias tile of every segment call, the store schedules behind the counted waits (bf16_stream.h
// bf_store_table), the tiles-by-k-steps arithmetic of the packers (bf16_weights.h) -- is computed from these rows.
struct BfSeg {
  int s0;        // first fragment
  int nft;       // output tiles (32 features each)
  int ksa, ksb;  // k-steps (16 inputs each) of input A, then of input B
  int bt0;       // first bias tile in the bias block, or -1: the accumulators start at zero
  int pieces;    // 1-KiB pieces of the segment's output that a training kernel stores behind its last tile (0: none)
};
constexpr int bf_seg_ks(const BfSeg& g) { return g.ksa + g.ksb; }
constexpr int bf_seg_end(const BfSeg& g) { return g.s0 + g.nft * bf_seg_ks(g); }
// tile f of a segment runs in accumulator (P0 + f) & 1: the two accumulators alternate along the whole stream
constexpr int bf_seg_p0(const BfSeg* t, int row) {
  int n = 0;
  for (int i = 0; i < row; ++i) n += t[i].nft;
  return n & 1;
}
constexpr int bf_seg_next_bt(const BfSeg* t, int rows, int row) { return row + 1 < rows ? t[row + 1].bt0 : -1; }
// the segments tile [0, nfrag) exactly
constexpr bool bf_segs_tile(const BfSeg* t, int rows, int nfrag) {
  int at = 0;
  for (int i = 0; i < rows; ++i) {
    if (t[i].s0 != at) return false;
    at = bf_seg_end(t[i]);
  }
  return at == nfrag;
}

// forward stream.  point_info (no activation, nerf.py:117) is folded into dir_info's feature columns (common.h SEG_FOLD): W_fold =
// W_dir[:, 24:] W_pi is formed in fp32 (k_fold_weights) and rounded to bf16 ONCE; the sigma head is a tile of its own on h7.
enum { FSEG_L0, FSEG_L1, FSEG_L2, FSEG_L3, FSEG_L4, FSEG_L5, FSEG_L6, FSEG_L7, FSEG_SIG, FSEG_DIR, FSEG_COL, FSEG_N };
constexpr BfSeg kFwdSegs[FSEG_N] = {
    {0, 8, 4, 0, 0, 16},       // L0: gamma_p (60 -> 64)
    {32, 8, 16, 0, 8, 16},     // L1
    {160, 8, 16, 0, 16, 16},   // L2
    {288, 8, 16, 0, 24, 16},   // L3
    {416, 8, 16, 4, 32, 16},   // L4: 16 hidden + 4 gamma_p   (nerf.py:109: hidden first)
    {576, 8, 16, 0, 40, 16},   // L5
    {704, 8, 16, 0, 48, 16},   // L6
    {832, 8, 16, 0, 56, 16},   // L7
    {960, 1, 16, 0, 64, 0},    // SIG: row 0 = sigma_layer (on h7)
    {976, 4, 2, 16, 65, 8},    // DIR: 2 gamma_d (24 -> 32) + 16 h7 through W_fold   (nerf.py:117: direction first); bias b_dir + W_dir[:, 24:] b_pi
    {1048, 1, 8, 0, 69, 0}};   // COL: rows 0..2 = color_layer
constexpr int BFS_L0 = kFwdSegs[FSEG_L0].s0, BFS_L1 = kFwdSegs[FSEG_L1].s0, BFS_L4 = kFwdSegs[FSEG_L4].s0, BFS_L5 = kFwdSegs[FSEG_L5].s0;
constexpr int BFS_SIG = kFwdSegs[FSEG_SIG].s0, BFS_DIR = kFwdSegs[FSEG_DIR].s0, BFS_COL = kFwdSegs[FSEG_COL].s0;
constexpr int BF_NFRAG = bf_seg_end(kFwdSegs[FSEG_N - 1]);  // 1056
static_assert(bf_segs_tile(kFwdSegs, FSEG_N, BF_NFRAG), "the forward segments tile the stream");
constexpr int BF_NCHUNK = BF_NFRAG / BF_CHUNK;  // 66
static_assert(BF_NCHUNK * BF_CHUNK == BF_NFRAG, "stream must be whole chunks");
constexpr size_t BF_IMAGE_BYTES = (size_t)BF_BIAS_BYTES + (size_t)BF_NFRAG * BF_FRAG_BYTES;

// ---- backward (dX chain) stream: transposed weights, consumed from the colour head back to layer 0.  One image serves both passes: the
// coarse pass stops after L1T.
enum { BSEG_COLT, BSEG_FOLDT, BSEG_L7T, BSEG_L6T, BSEG_L5T, BSEG_L4T, BSEG_L3T, BSEG_L2T, BSEG_L1T, BSEG_G0T, BSEG_N };
constexpr BfSeg kBwdSegs[BSEG_N] = {
    {0, 4, 4, 0, -1, 8},        // COLT: d c = W_color^T dz (only k-step 0, inputs 0..2 = dz, is non-zero)
    {16, 8, 8, 1, -1, 16},      // FOLDT: d h7 = 8 k-steps W_fold^T dpre_dir + 1 k-step w_sigma (input slot 3 = dspre)
    {88, 8, 16, 0, -1, 16},     // L7T
    {216, 8, 16, 0, -1, 16},    // L6T
    {344, 8, 16, 0, -1, 16},    // L5T
    {472, 8, 16, 0, -1, 16},    // L4T (hidden columns)
    {600, 8, 16, 0, -1, 16},    // L3T
    {728, 8, 16, 0, -1, 16},    // L2T
    {856, 8, 16, 0, -1, 16},    // L1T
    {984, 2, 16, 16, -1, 0}};   // G0T, fine pass only: d gamma_p = 16 k-steps of W_0^T (input dpre0) + 16 of W_4[:, 256:]^T (input dpre4, re-read)
constexpr int BBS_COLT = kBwdSegs[BSEG_COLT].s0, BBS_FOLDT = kBwdSegs[BSEG_FOLDT].s0, BBS_L7T = kBwdSegs[BSEG_L7T].s0;
constexpr int BBS_L4T = kBwdSegs[BSEG_L4T].s0, BBS_L3T = kBwdSegs[BSEG_L3T].s0, BBS_G0T = kBwdSegs[BSEG_G0T].s0;
constexpr int BBC_NFRAG = BBS_G0T, BBF_NFRAG = bf_seg_end(kBwdSegs[BSEG_G0T]);  // 984, 1048
static_assert(bf_segs_tile(kBwdSegs, BSEG_G0T, BBC_NFRAG) && bf_segs_tile(kBwdSegs, BSEG_N, BBF_NFRAG), "the backward segments tile both streams");
constexpr int BBC_NCHUNK = (BBC_NFRAG + BF_CHUNK - 1) / BF_CHUNK, BBF_NCHUNK = (BBF_NFRAG + BF_CHUNK - 1) / BF_CHUNK;
constexpr size_t BB_IMAGE_BYTES = (size_t)BF_BIAS_BYTES + (size_t)BBF_NCHUNK * BF_CHUNK * BF_FRAG_BYTES;

// ---- training buffers in FRAGMENT layout: per wave block (32 consecutive samples of a pass) and tensor, ks pieces of
// 1 KiB = what the wave's 64 lanes hold as one packed B operand (lane (j, h): sample j, features 16ks + 4h + {0..3, 8..11}).
// Tensor-major: tensor t starts at wb_tot * 1024 * cum_ks(t); piece (wb, ks) of it at ((wb * ks_t) + ks) * 1024.
// saved by the forward (point_info's output is not: folded, no weight gradient needs it):
constexpr int BS_GP = 0, BS_H0 = 1, BS_C = 9, BS_GD = 10, NBS = 11;
__host__ __device__ constexpr int bs_ks(int t) { return t == BS_GP ? 4 : t < BS_C ? 16 : t == BS_C ? 8 : 2; }
__host__ __device__ constexpr int bs_cum(int t) { int o = 0; for (int i = 0; i < t; ++i) o += bs_ks(i); return o; }
constexpr int BS_TOTAL_KS = bs_cum(NBS);  // 142 KiB per wave block
// written by the backward chain (pre-activation gradients = A operands of the dW GEMMs):
constexpr int BG_L0 = 0, BG_D = 8, BG_Z = 9, NBG = 10;  // BG_Z: features 0..2 = dz (colour), 3 = dspre (sigma)
__host__ __device__ constexpr int bg_ks(int t) { return t < BG_D ? 16 : t == BG_D ? 8 : 2; }  // BG_Z: 2nd piece = zeros
__host__ __device__ constexpr int bg_cum(int t) { int o = 0; for (int i = 0; i < t; ++i) o += bg_ks(i); return o; }
constexpr int BG_TOTAL_KS = bg_cum(NBG);  // 138
// ReLU "alive" masks: u16 [9 layers: h0..h7, c][wb_tot][64 lanes][8 tiles], bit 15-r = accumulator register r > 0
constexpr int BM_LAYERS = 9;

// bias tiles (32 floats each) in the bias block
constexpr int BFB_L0 = kFwdSegs[FSEG_L0].bt0, BFB_SIGMA = kFwdSegs[FSEG_SIG].bt0, BFB_DIR = kFwdSegs[FSEG_DIR].bt0, BFB_COL = kFwdSegs[FSEG_COL].bt0;
constexpr int BF_NBIAS_TILES = BFB_COL + kFwdSegs[FSEG_COL].nft;  // 70

}  // namespace nerf
