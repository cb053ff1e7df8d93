// kernels.h -- kernel argument blocks and launchers shared by the .hip translation units and api.cpp.
#pragma once
#include "common.h"

#include <atomic>
#include <initializer_list>

namespace nerf {

// More than 64 KiB of dynamic LDS needs an opt-in per kernel -- and per DEVICE: the attribute belongs to the function's
// code object on the current device, so a process that moves to a second GPU must set it again.  `mask` = one bit per
// device ordinal already done (a static at the call site); ordinals >= 64 simply set it on every launch.
inline hipError_t ensure_dynamic_lds(std::atomic<unsigned long long>& mask, std::initializer_list<const void*> kernels, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 64 && ((mask.load(std::memory_order_relaxed) >> dev) & 1ull)) return hipSuccess;
  for (const void* k : kernels) {
    e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
  }
  if (dev < 64) mask.fetch_or(1ull << dev, std::memory_order_relaxed);
  return hipSuccess;
}

constexpr int LDA = 260;  // floats per LDS activation row of the field kernels
constexpr int FIELD_LDS_FLOATS = TM * LDA + 4 * TM * 3;

struct FieldArgs {
  const float4* wp;        // packed weights (PACKED_FWD_F4 float4)
  const unsigned char* wbf;  // bf16 weight stream (bf16_common.h), bf16-MLP variant only
  unsigned char* bsave;      // bf16 training: saved layer inputs in fragment layout (bf16_common.h); split-fp32 training: their hi parts
  unsigned char* bsave2;     // split-fp32 training: the mid parts, same layout
  uint16_t* bmask;           // bf16 training: ReLU alive masks
  int wb0, wb_tot;           // first wave block of this pass, wave blocks of both passes
  Weights24 w;             // raw parameter pointers (biases, sigma / colour heads)
  const float* rayf;       // [B][RAYF]
  const float* dvec;       // [B][128]  b_dir + W_dir[:, :24] * gamma_dir(ray)
  const float* t;          // [M] depths
  float* rgb;              // [M][3]
  float* sigma;            // [M]
  float* pts_dbg;          // [M][3] or null
  float* gp_dbg;           // [M][60] or null
  // ---- training only (SAVE): rows of the coarse pass come first, then the fine pass, in every buffer
  float* save;             // [NSAVE][Mtot][256]: h0..h7, c (128 used), gamma_p (64 used)
  uint16_t* masks;         // [8][tiles_tot][4][256]: ReLU masks of h0..h7 in accumulator layout
  float* spre;             // [Mtot] sigma pre-activation
  int row0;                // first row of this pass in the combined buffers
  int tile0;               // first tile of this pass in the mask buffer
  int tiles_tot;
  long long Mtot;
  long long MSrows;        // rows per saved tensor = Mtot + DUMP_ROWS: lanes past the end of a pass store to their own dump row
  int N;                   // samples per ray
  int M;                   // samples of this pass (B*N)
  unsigned long long* stamps;  // diagnostic build (-DNERF_STAMPS) only: [8] cycle sums per phase
};

// Point queries (nerf_hip_query / nerf_hip_density_grid; k_field_fwd_reg's SRC_POINTS / SRC_LATTICE forms): sample m of the launch is
// point m.  The FieldArgs of such a launch use wp, w, dvec ([M][128], one row per point; colour queries only), rgb, sigma and M.
struct QuerySrc {
  const float* points;     // [M][3] world points, or null: the lattice below
  float lo[3], step[3];    // lattice point (i, j, k) = lo + (i, j, k) * step, each coordinate one product and one sum
  int ny, nz;              // lattice: m = (i * ny + j) * nz + k (C order, z fastest)
  // ---- narrow-band forms (SRC_CORNERS / SRC_BLOCKS, nerf_hip_band_*): the samples are points of the nx x ny x nz lattice above, cut into
  // blocks of r^3 points, and sigma is stored at the point's own lattice index (a.sigma is the dense grid)
  const int* list;         // SRC_BLOCKS: ascending block ids, block = (bx * nby + by) * nbz + bz; this launch starts at entry e0
  const long long* nlist;  // SRC_BLOCKS: the list's length (device); entries past it are computed on block 0 and not stored
  int e0;
  int nx, r;
  int ext[3];              // SRC_CORNERS: corner planes per axis, plane u at min(u * r, n - 1), sample m = (ux * ext[1] + uy) * ext[2] + uz
                           // SRC_BLOCKS: points per block and axis = min(r, n), sample m = (entry * ext[0] * ext[1] * ext[2]) + local index
  int nby, nbz;            // SRC_BLOCKS: blocks along y and z
};
// Colour queries run in chunks of this many points: the dvec rows of one chunk live in the workspace (independent of M), and a chunk is
// 8 waves for every SIMD of the chip (256 CUs x 4 SIMDs x 32 points x 8) at the kernel's one wave per SIMD.
constexpr int QUERY_CHUNK = 256 * 4 * 32 * 8;
// Gradient queries (nerf_hip_query_grad): the compact save-carrying forward (k_field_fwd_reg<..., SRC_POINTS, RGB, GSAVE = true>) and the
// query form of the dX chain (k_field_bwd_reg<true, true, RGB>) run chunk by chunk, 4 rounds of one wave per SIMD (256 CUs x 4 SIMDs x
// 32 points x 4).  The FieldArgs / FieldBwdArgs of such a launch use, besides the query fields: save = [MSrows][QGRAD_GP] gamma_p rows,
// then (RGB) [MSrows][QGRAD_C] c rows; masks = [8][tiles_tot][4][256] ReLU masks of h0..h7 (the training layout); spre [MSrows];
// row0 = tile0 = 0, Mtot = the chunk's points, MSrows = QGRAD_CHUNK + DUMP_ROWS.  The chain's upstream is dsig ([M], null = ones) and,
// RGB, drgb [M][3] with the forward's rgb; its output dt is dpoints [M][3] (stored, not added).  G is null: no G / dz / dspre row is written.
constexpr int QGRAD_CHUNK = 256 * 4 * 32 * 4;
constexpr int QGRAD_GP = 64, QGRAD_C = 128;  // floats per saved gamma_p row (60 used) / c row

// saved by the forward: h0..h7, c, gamma_p (feat = point_info's output is not saved: with point_info folded into dir_info no weight
// gradient needs it, see common.h SEG_FOLD)
constexpr int S_H0 = 0, S_C = 8, S_GP = 9, NSAVE = 10;
// gradient buffers written by the backward chain: dpre of layers 0..7 and of dir_info
constexpr int G_L0 = 0, G_D = 8, NGRAD = 9;

struct RaysArgs {
  const int64_t* row;
  const int64_t* col;
  const float* pb;  // [B][17]
  float K[9];
  int B, Nc;
  float* rayf;       // [B][RAYF] or null
  float* dvec;       // [B][128] or null (needs w_dir / b_dir)
  const float* w_dir;  // [128][280]
  const float* b_dir;  // [128]
  const float* b_fold; // [128] W_dir[:, 24:] b_pi (k_fold_weights), added to dvec; or null
  float* t_c;        // [B][Nc] or null
  float* d_cam;      // [B][3] or null
  float* d_wrd;      // [B][3] or null
  unsigned* status;  // the workspace's status words [0, STATUS_STICKY_WORD) are zeroed here (first kernel of a forward), or null
};

struct CoarseArgs {
  const float* t_c;     // [B][Nc]
  const float* sigma;   // [B][Nc]
  const float* rgb;     // [B][Nc][3]
  const float* rayf;    // [B][RAYF] or null (then near_far is used)
  const float* near_far;  // [B][2] or null
  int B, Nc, Nf;
  int delta0_mode;      // 0: from rayf[0] (this batch's ray 0); 1: delta0 given
  float delta0;
  int ray0_override;    // delta0_mode 0 only: 1 = use near0/far0 below instead of rayf[0]
  float near0, far0;
  float* w_c;           // [B][Nc]
  float* C_coarse;      // [B][3]
  float* t_f;           // [B][Nf]
  uint32_t* status;
  uint32_t* sticky;     // or null: a second word that gets the same bits and that no kernel ever clears (nerf_hip_read_status_sticky)
};

struct MergeArgs {
  const float *t_c, *t_f, *sig_c, *sig_f, *rgb_c, *rgb_f;
  int B, Nc, Nf, P;
  float last;
  float* bundle;   // [B][N][5] or null
  float* w;        // [B][N] or null
  uint16_t* perm;  // [B][5][N] or null: sorted position -> original index (coarse first, then fine)
  float* C_fine;   // [B][3]
  int joint;       // NERF_HIP_CORRECTED: ONE stable sort by depth whose permutation moves all five channels (rgb and sigma stay with their
                   // sample) instead of the reference's five independent channel sorts (quirk Q1); perm then holds that permutation five times
};

// SMALL bf16 training batches (Nc = 64, Nf = 128): the per-ray stages ride in the field kernels instead of launches of their own --
// k_coarse / k_merge as EPILOGUES of the coarse / fine forward pass, k_merge_bwd / k_coarse_bwd as PROLOGUES of the fine / coarse chain
// (a workgroup's samples are whole rays: 128 samples = 2 coarse rays or 1 fine ray, 256 = 4 or 2); mode 0 = none
struct FwdFuse {
  int mode;      // 1: coarse composite + resampling behind the coarse pass, 2: merge + sorts + composite behind the fine pass
  CoarseArgs c;
  MergeArgs m;
  // mode 2 inside nerf_hip_train_step: ray_loss's per-element work rides along too (nerf.py:325-331) -- d loss / d C and the summands of the
  // loss, element by element as k_ray_loss forms them; the SUM is taken by the first block of the fine chain launch (BwdFuse), in
  // k_ray_loss's order.  C_true null: no loss here
  const float* C_true;    // [B][3]
  const float* C_coarse;  // [B][3] (written by the coarse pass's epilogue, an earlier launch)
  float *dC_c, *dC_f;     // [B][3]
  float* loss_terms;      // [B][3]
};
hipError_t launch_pack_weights(const Weights24& w, float* fold, float4* out, int nseg, hipStream_t st);  // fold: FOLD_FLOATS scratch (launch_fold_weights runs first)
hipError_t launch_fold_weights(const Weights24& w, float* fold, hipStream_t st);  // fold: FOLD_FLOATS (b_fold, then W_fold): bf16-MLP variant
hipError_t launch_field_fwd(const FieldArgs& a, bool save, hipStream_t st);
hipError_t launch_field_fwd_reg(const FieldArgs& a, bool save, hipStream_t st);
hipError_t launch_query_reg(const FieldArgs& a, const QuerySrc& q, bool rgb, hipStream_t st);  // rgb: colour and sigma (q.points, a.dvec set), else sigma
hipError_t launch_query_grad_fwd(const FieldArgs& a, const QuerySrc& q, bool rgb, hipStream_t st);  // launch_query_reg + the compact save (QGRAD_*)
// dir_info start vectors of n points from their directions: dvec[i][128] as k_rays forms them from a ray's world direction (ray_ops.hip)
hipError_t launch_dirs_dvec(const float* dirs, int n, const float* w_dir, const float* b_dir, const float* b_fold, float* dvec, hipStream_t st);
hipError_t launch_field_fwd_bf16(const FieldArgs& a, bool save, hipStream_t st, const FwdFuse* fuse = nullptr);
// the bf16 packers read the fp32 fold (launch_fold_weights, same stream, before them)
hipError_t launch_pack_weights_bf16(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
hipError_t launch_pack_bias_block_bf16(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
hipError_t launch_field_fwd_bf16x(const FieldArgs& a, hipStream_t st);  // inference, 16x16x32 MFMA form
// small batches, Nc = 64 / Nf = 128: the whole inference forward of a ray PAIR per workgroup in one launch (field_fwd_bf16x.hip)
struct PairArgs {
  const unsigned char* wbf;   // 16x16x32 weight image
  RaysArgs rays;              // row, col, pb, K (Nc = 64): the ray records are made in the kernel; rays.rayf / rays.t_c (may be null) get copies
  int B;
  unsigned gen;               // this call's generation (24 bits, never 0): stamps the status flags (common.h STATUS_*)
  int ray0_override;          // quirk Q6: 1 = near0 / far0 below are the batch's GLOBAL ray 0's, 0 = this call's ray 0
  float near0, far0;
  float last;                 // nerf.py:286
  float* C_coarse;            // [B][3]
  float* C_fine;              // [B][3]
  uint32_t* status;           // the workspace's status words (word 0 of the region)
  uint32_t* sticky;
  float *sig_c, *rgb_c, *w_c, *t_f, *sig_f, *rgb_f;  // the workspace's per-sample buffers (written for introspection; may be null)
};
hipError_t launch_render_pair_bf16x(const PairArgs& a, hipStream_t st);
hipError_t launch_pack_weights_bf16x(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
// split-fp32 inference (field_fwd_split.hip): fp32 operands as two bf16 parts, three bf16 MFMAs per product
size_t split_image_bytes();
// split-fp32 training (field_bwd_split.hip): the transposed image of the backward chain, hi and mid fragment of every step interleaved
size_t split_bwd_image_bytes();
hipError_t launch_pack_weights_split_bwd(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
hipError_t launch_pack_weights_split(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
hipError_t launch_field_fwd_split(const FieldArgs& a, bool save, hipStream_t st);  // save: + hi / mid fragment-layout saves, masks, spre (FieldArgs bsave / bsave2 / bmask)
hipError_t launch_rays(const RaysArgs& a, hipStream_t st);
// bf16 paths: fold + packed image(s) + ray records in ONE launch (prep_bf16.hip).  img_fwd: forward image (fwd_form 0: 32x32x16 stream,
// 1: 16x16x32) or null = weights unchanged; img_bwd: transposed image of the backward chain or null; ready: PREP_READY_WORDS u32 words of the
// workspace that no other kernel writes; token: unique per call; sticky: the sticky status word (timeout report) or null
constexpr int PREP_READY_WORDS = 256;
hipError_t launch_prep_bf16(const Weights24& w, float* fold, unsigned char* img_fwd, int fwd_form, unsigned char* img_bwd,
                            unsigned* ready, unsigned token, unsigned* sticky, const RaysArgs& rays, hipStream_t st);
// The optional per-ray outputs of one call of the per-ray stages, and in the backward their upstreams: ONE record from the C entry
// (api.hip) down to the device functions (ray_parts.h, ray_parts_bwd.h).  A null pointer = not asked for; which fields a kernel reads
// is fixed by the flags of its instantiation (MAPS, QD, DL), never tested at run time.
// It travels as a kernel argument of its own, not as fields of CoarseArgs / MergeArgs / MergeBwdArgs / CoarseBwdArgs: those structs ride
// inside FwdFuse / BwdFuse / PairArgs, the arguments of the bf16 training and pair kernels, whose layouts it must not touch.
constexpr int MAX_QUANTILES = 4;  // = NERF_HIP_MAX_QUANTILES
struct QuantArgs {
  float q[MAX_QUANTILES];
  int nq;
};
struct RayExtras {
  // MAPS (nerf_hip_forward_maps, nerf_hip_forward_maps_train): each ray's (D_c, A_c) by the coarse kernel, (D_f, A_f) by the merge kernel
  float* maps;            // [B][4]
  // QD (nerf_hip_forward_quantiles, with maps): each ray's quantile depths (rule QD of include/nerf_hip.h), row 0 by the coarse kernel,
  // row 1 by the merge kernel.  The quantiles themselves travel here too
  QuantArgs qa;
  float* qdepth;          // [B][2][qa.nq]
  // DL (nerf_hip_forward_distortion_train, with maps): each ray's distortion loss (rule DL), column 0 by the coarse kernel, column 1 by the
  // merge kernel.  The merge kernels have no ray records of their own: near / far come from rayf (the workspace's records) or near_far
  // (stage entries)
  float* dist;            // [B][2]
  const float* rayf;      // [B][RAYF] or null
  const float* near_far;  // [B][2], used when rayf is null
  // backward (nerf_hip_backward_maps, nerf_hip_backward_distortion): the upstreams (gD_c, gA_c, gD_f, gA_f) of the maps and (gL_c, gL_f) of
  // the distortion losses
  const float* dmaps;     // [B][4]; DL: or null = zeros (the distortion stage entries may come without it)
  const float* ddist;     // [B][2]
};
// (launchers of the per-ray stages) the launch of a kernel with `lds` bytes of dynamic LDS: above `limit`, what a launch may ask for as it is, the kernel's attribute is raised first
template <class... KArgs, class... Args>
inline hipError_t launch_dyn_lds(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, size_t limit, hipStream_t st, const Args&... args) {
  if (lds > limit)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}
// x == null or no pointer of it set: k_coarse / k_merge.  Otherwise the instantiation of k_coarse_x / k_merge_x for what x asks for: maps,
// maps + quantiles (qdepth set) or maps + distortion (dist set; the merge kernel then sorts with slots: a training call, a.perm set)
hipError_t launch_coarse(const CoarseArgs& a, hipStream_t st, const RayExtras* x = nullptr);
hipError_t launch_merge(const MergeArgs& a, hipStream_t st, const RayExtras* x = nullptr);
// nerf_hip_forward_normals (ray_normals.hip; rule NM of include/nerf_hip.h): the world points of nrays whole rays of N samples each (rayf and
// t start at the first of them; t_stride 1 = t_c, 5 = channel 0 of the sorted bundle), and the per-ray composite of the field normals of
// g [B][N][3] with the weights w [B][N] -> out[b * out_stride + 0..2]
hipError_t launch_sample_points(const float* rayf, const float* t, int t_stride, int nrays, int N, float* points, hipStream_t st);
hipError_t launch_normal_composite(const float* w, const float* g, int B, int N, float* out, int out_stride, hipStream_t st);
hipError_t launch_ray_loss(const float* Cc,const float* Cf, const float* Ct, int B, float* loss, float* dCc, float* dCf, hipStream_t st);

}  // namespace nerf

// ================================================================================================
// backward
// ================================================================================================
namespace nerf {

struct FieldBwdArgs {
  const float4* wp;        // packed weights incl. transposed segments
  Weights24 w;
  const float* rayf;       // [B][RAYF]
  const float* t;          // [M] depths of this pass
  const float* rgb;        // [M][3] forward output of this pass
  const float* drgb;       // [M][3] upstream gradient
  const float* dsig;       // [M]    upstream gradient
  const float* save;       // [NSAVE][Mtot][256]
  const uint16_t* masks;   // [8][tiles_tot][4][256]
  const float* spre;       // [Mtot]
  float* G;                // [NGRAD][Mtot][256] pre-activation gradients (inputs of the dW GEMMs)
  float* dz;               // [Mtot][4] colour-head pre-sigmoid gradient
  float* dspre;            // [Mtot]    sigma-head pre-abs gradient
  float* dt;               // [M] fine pass only: in = d loss/d t from the merge, out += direction . d loss/d point
  // bf16-MLP variant (field_bwd_bf16.hip): transposed stream of this pass, ReLU masks, gradient buffer (fragment layout)
  const unsigned char* wbf;
  const uint16_t* bmask;
  unsigned char* bG;
  unsigned char* bG2;      // split-fp32 training (field_bwd_split.hip): the gradients' mid parts (bG holds the hi parts), same layout
  int wb0, wb_tot;
  int row0, tile0, tiles_tot;
  long long Mtot;
  long long MSrows;        // rows per tensor of save / G = Mtot + DUMP_ROWS (see FieldArgs)
  int N, M;
  unsigned long long* stamps;  // diagnostic build only: cycle sums per phase (workspace dbg words [32, 64))
};

// One weight-gradient product dW = G^T X of the fp32 train step (dw_f32.hip).
struct DwItem {
  const float* G;          // [Mtot][256] pre-activation gradients, columns [0, nout)   (thin: the [Mtot][4] buffer dz_r, dz_g, dz_b, dsigma_pre)
  const float* X;          // [Mtot][256] layer inputs, columns [0, nin)                 (thin: c, 128 columns)
  const float* sig;        // has_sig: dsigma_pre, one float per row with a stride of 4 (column 3 of the [Mtot][4] buffer)
  int nout, nin;           // 256 / 128 output columns, 256 / 64 (padded) input columns
  int nin_real;            // input columns that exist in dW (60 of 64 for gamma_p)
  float* dW; int ldw, col0;  // destination [nout][ldw], columns col0 .. col0 + nin_real      (thin: dW_color[3][128])
  float* db;               // [nout] bias gradient = column sums of G, or null                 (thin: db_color[3])
  float* dW2;              // has_sig: dw_sigma[nin] = sum_m sig[m] * X[m][:]
  float* db2;              // thin only: db_sigma[1]
  int thin;                // 1: the colour head (and both heads' bias gradients) as one thin product
  int has_sig;             // 1: the sigma head rides on this product (X = h7): dW2 from the waves that hold X's columns
  float* raysum;           // dir_info product, rows aligned to rays (dw_ray_duty_ok): the column-sum waves also write the per-ray sums of G,
                           // [2][rays][128] (coarse rows, fine rows) -- the scratch of the gamma_d columns' kernels; else null
  int ray_nc, ray_nf;      // samples per ray of the coarse / fine pass
  int rows_c;              // rows of the coarse pass (= rays * ray_nc), the fine pass's rows follow
  int wg0, nwg;            // workgroups [wg0, wg0 + nwg) of the launch work on this product, each on 1/nwg of the rows
  long long slab_off;      // floats: this product's slabs inside DwBatch::slabs
  unsigned long long* stamps;  // diagnostic build only: per-wave (start, end, xcc, hw id) records
};
constexpr int DW_WGS = 256;  // workgroups of the launch: one per CU, dealt out over the products
constexpr int DW_MAX_ITEMS = 13;
// The seven 256 x 256 products share ONE launch (dw_f32.hip: k_dw4_group), DW_GROUP_WGS workgroups each.
constexpr int DW_GROUP_WGS = 36;
struct DwBatch {
  DwItem item[DW_MAX_ITEMS];
  int n;
  int grouped;             // > 0: items [0, grouped) are 256 x 256 products of equal nwg that share ONE launch (k_dw4_group)
  const float* slabs;
};

// gradients of point_info and of dir_info's feature columns from the folded product (dw_f32.hip: k_fold_grads)
struct FoldGradArgs {
  const float* M;        // [128][256] sum_m dpre_dir[m] (x) h7[m]
  const float* db_dir;   // [128] (final)
  const float* w_dir;    // [128][280]
  const float* w_pi;     // [256][256]
  const float* b_pi;     // [256]
  float* dW_pi;          // [256][256]
  float* db_pi;          // [256]
  float* dW_dir;         // [128][280], columns 24.. written
};
hipError_t launch_fold_grads(const FoldGradArgs& a, hipStream_t st);
// (w: the step's weights, dw: its 24 gradient tensors -- dw[B_DIR] final, mbuf: the folded product's sums)
inline FoldGradArgs fold_grad_args(const Weights24& w, float* const* dw, const float* mbuf) {
  FoldGradArgs a;
  a.M = mbuf; a.db_dir = dw[B_DIR]; a.w_dir = w.p[W_DIR]; a.w_pi = w.p[W_PI]; a.b_pi = w.p[B_PI];
  a.dW_pi = dw[W_PI]; a.db_pi = dw[B_PI]; a.dW_dir = dw[W_DIR];
  return a;
}

struct MergeBwdArgs {
  const float* dC_f;       // [B][3]
  const float* bundle;     // [B][N][5] sorted channels
  const uint16_t* perm;    // [B][5][N]
  int B, Nc, Nf;
  float last;
  float *drgb_c, *dsig_c;  // [B][Nc][3], [B][Nc]   (written: contribution through the merged composite)
  float *drgb_f, *dsig_f, *dt_f;  // [B][Nf][3], [B][Nf], [B][Nf]
};

struct CoarseBwdArgs {
  const float* dC_c;       // [B][3]
  const float* dt_f;       // [B][Nf] total d loss / d t_fine
  const float *t_c, *sigma, *rgb;  // coarse forward values
  const float* rayf;       // [B][RAYF] or null (then near_far is used)
  const float* near_far;   // [B][2] or null
  int B, Nc, Nf;
  int delta0_mode; float delta0;   // as CoarseArgs
  int ray0_override; float near0, far0;
  float *drgb_c, *dsig_c;  // in: merge contribution, out: total
};

struct BwdFuse {
  int mode;      // 1: merged-composite backward in front of the fine chain, 2: resampling + coarse-composite backward in front of the coarse chain
  MergeBwdArgs m;
  CoarseBwdArgs c;
  const float* loss_terms;  // mode 1, or null: block 0 adds up the 3 B summands of the loss in k_ray_loss's order
  float* loss;              // [1]
};

struct SmallGradArgs {
  const float* save;       // saves base
  const float* G;          // grads base
  const float* dz;         // [Mtot][4]
  const float* dspre;      // [Mtot]
  const float* rayf;
  long long Mtot;
  long long MSrows;        // rows per tensor of save / G (Mtot + DUMP_ROWS)
  int B, Nc, Nf;
  float *dW_color, *db_color, *dw_sigma, *db_sigma, *dW_dir;  // destinations (dW_dir: [128][280], cols 0..23 written)
  float* sbuf;             // [2][B][128] scratch: per-ray sums of dpre_dir over the coarse / the fine rows
  int sums_done;           // 1: sbuf was written by the dir_info product (DwItem::raysum); 0: k_dir_ray_sums does it
  float* gdbuf;            // [B][24]  scratch: gamma_dir per ray
};

hipError_t launch_field_bwd(const FieldBwdArgs& a, bool fine, hipStream_t st);
hipError_t launch_field_bwd_split(const FieldBwdArgs& a, bool fine, hipStream_t st);  // split-fp32 training chain (field_bwd_split.hip)
hipError_t launch_field_bwd_reg(const FieldBwdArgs& a, bool fine, hipStream_t st);
hipError_t launch_query_grad_bwd(const FieldBwdArgs& a, bool rgb, hipStream_t st);  // the query form of the chain: a.dt = dpoints [M][3] (QGRAD_*)
hipError_t launch_field_bwd_bf16(const FieldBwdArgs& a, bool fine, hipStream_t st, const BwdFuse* fuse = nullptr);
hipError_t launch_pack_weights_bf16_bwd(const Weights24& w, const float* fold, unsigned char* img, hipStream_t st);
// bf16 / split-fp32 weight-gradient phase (dw_bf16.hip): every product of a step over the fragment-layout buffers `bs` (layer inputs) and `bg`
// (pre-activation gradients) of wb_tot wave blocks, their slab sums into the 24 gradient tensors `dw` and the folded product's M (`mbuf`),
// then k_fold_grads on the weights `w`.  `slabs`: dw_bf16_slab_floats() floats of partial sums.  early_event (or null) is recorded as soon
// as the tensors of point_layer[0..7] (dw[0..15]) are final.
size_t dw_bf16_slab_floats();
// split-fp32 train step: every operand tensor is a (hi, mid) pair of the same layout -- the mid part of a gradient-type tensor (G, Z) lies
// gdelta bytes behind its hi part, the mid part of an input tensor xdelta bytes; {0, 0} = plain bf16 operands
struct DwBfSplit { long long gdelta = 0, xdelta = 0; };
hipError_t launch_dw_bf16_phase(const unsigned char* bs, const unsigned char* bg, int wb_tot, float* const* dw, float* mbuf, float* slabs,
                                size_t slab_floats, const Weights24& w, void* early_event, DwBfSplit sp, hipStream_t st);
hipError_t launch_dw(const DwBatch& b, long long Mtot, float* slabs, hipStream_t st, int first = 0, int count = -1);  // products [first, first + count) -> their slabs
hipError_t launch_dw_reduce(const DwBatch& b, hipStream_t st, int first = 0, int count = -1);  // the slabs of items [first, first + count) -> gradients, ONE launch
size_t dw_item_slab_floats(const DwItem& p);
bool dw_ray_duty_ok(const DwItem& p, long long Mtot, int B, int Nc, int Nf);  // may the product of G_dir carry the per-ray sums?
hipError_t launch_small_grads(const SmallGradArgs& a, float* scratch, hipStream_t st);  // scratch: >= 128 * 128 * 24 floats (the slab buffer, after the reduce)
// x == null or no upstream of it set: k_merge_bwd / k_coarse_bwd.  Otherwise k_merge_bwd_x / k_coarse_bwd_x with the maps' upstream
// (dmaps) or, ddist set, with the distortion losses' upstream too (ray_ops_bwd.hip)
hipError_t launch_merge_bwd(const MergeBwdArgs& a, hipStream_t st, const RayExtras* x = nullptr);
hipError_t launch_coarse_bwd(const CoarseBwdArgs& a, hipStream_t st, const RayExtras* x = nullptr);

struct AdamArgs {
  float* param[24];
  const float* grad[24];
  int numel[24];
  int offset[24];          // start of tensor t inside the flat moment buffers
  float* m;                // exp_avg, flat [593,924]
  float* v;                // exp_avg_sq
  float step_size;         // lr / (1 - beta1^t)
  float bias2_sqrt;        // sqrt(1 - beta2^t)
  float one_minus_beta1, beta2, one_minus_beta2, eps;
};

struct GatherArgs {
  const long long* index;  // [B] flat pixel indices
  const float* pixels;     // [n_pic*H*W][3]
  const float* poses;      // [n_pic][17] f32
  int B, H, W;
  long long *row, *col, *pic;  // [B] i64 (the dtypes the reference's collate produces)
  float* pix_val;          // [B][3]
  float* poses_bound;      // [B][17] f32
};

hipError_t launch_adam(const AdamArgs& a, hipStream_t st);
hipError_t launch_gather_rays(const GatherArgs& a, hipStream_t st);

// ---- marching cubes over a density grid (mesh.hip; nerf_hip_mesh_count / nerf_hip_mesh_emit and their _masked forms, DESIGN.md
// sections 3h and 3h-10) ----
constexpr int MESH_WG = 256;                   // threads per workgroup
constexpr int MESH_ROUNDS = 16;                // rounds of MESH_WG consecutive lattice points per workgroup
constexpr int MESH_PTS = MESH_WG * MESH_ROUNDS;  // lattice points per workgroup (the scan's block)

struct MeshArgs {
  const float* sigma;      // [nx][ny][nz], z fastest
  const unsigned char* valid;  // [nx][ny][nz] or null: rule M's mask (the MASKED instantiations; null selects the unmasked ones)
  int nx, ny, nz;          // every dimension >= 2, nx * ny * nz < 2^31
  float level;
  float lo[3], step[3];    // emit only
  unsigned* offs;          // [N]: (in-block exclusive vertex offset << 3) | owned-edge mask, written only where the mask is non-zero
  int *tv, *tf;            // [nb] per-block vertex / face totals
  long long *bv, *bf;      // [nb + 1] exclusive scans of tv / tf; [nb] = the totals
  long long* counts;       // [2] = V, F (count only)
  float *verts, *normals;  // [max_v][3] (emit only)
  int* faces;              // [max_f][3]
  long long max_v, max_f;
};

inline int mesh_blocks(long long n_points) { return (int)((n_points + MESH_PTS - 1) / MESH_PTS); }
hipError_t launch_mesh_count(const MeshArgs& a, hipStream_t st);  // count + in-block vertex scan, then the scan of the block totals
hipError_t launch_mesh_emit(const MeshArgs& a, hipStream_t st);

// ---- connected components of an indexed mesh (mesh_cc.hip; nerf_hip_mesh_cc_*) ----
constexpr int CC_WG = 256;                     // threads per workgroup
constexpr int CC_ROUNDS = 8;                   // rounds of CC_WG consecutive items per workgroup of the scans
constexpr int CC_PTS = CC_WG * CC_ROUNDS;      // items per workgroup (the scan's block)
constexpr int CC_MAX_ROUNDS = 64;              // labelling rounds before the call gives up (NERF_HIP_ERR_CONVERGE)

inline int cc_blocks(long long n) { return (int)((n + CC_PTS - 1) / CC_PTS); }

struct CcArgs {
  const int* faces;        // [F][3]
  int V, F;
  int* L;                  // [V] labels: L[x] <= x, a vertex of x's component (workspace)
  int* changed;            // [1] round only: 1 when the round's hooks lowered a label
  int *tot, *base;         // [cc_blocks(V)] ids only: roots per workgroup and their exclusive scan (workspace)
  int *vert_comp, *face_comp;  // [V], [F] ids only
  long long* count;        // [1] ids only: C
};

struct CcStatsArgs {
  const int *vert_comp, *face_comp;  // [V], [F]
  const float* verts;      // [V][3] or null (with lo / hi)
  long long V, F, max_c;   // ids >= max_c (and < 0) are left out
  int *n_verts, *n_faces;  // [max_c]
  unsigned *lo, *hi;       // [max_c][3] or null: keys while the atomics run, decoded to floats in place by the last launch
};

struct CcCompactArgs {
  const float *verts, *normals, *rgb;  // [V][3]; normals / rgb (with their outputs) may be null
  const int* faces;        // [F][3]
  int V, F, C;
  const int *vert_comp, *face_comp;
  const unsigned char* keep;  // [C]
  int* newidx;             // [V] rank of a kept vertex among the kept, -1 for a dropped one (workspace, in L's place)
  int *tot, *base;         // [cc_blocks(max(V, F))] (workspace)
  float *out_verts, *out_normals, *out_rgb;  // [max_v][3]
  int* out_faces;          // [max_f][3]
  long long max_v, max_f;
  long long* counts;       // [2] = V', F'
};

hipError_t launch_cc_round(const CcArgs& a, bool first, hipStream_t st);  // (first: L[v] = v,) changed = 0, hook, compress
hipError_t launch_cc_ids(const CcArgs& a, hipStream_t st);                // roots -> ascending ids (scan), vert_comp, face_comp, count
hipError_t launch_cc_stats(const CcStatsArgs& a, hipStream_t st);
hipError_t launch_cc_compact(const CcCompactArgs& a, hipStream_t st);     // the kept vertices' scan and placement, then the kept faces'

// ---- simplification of an indexed mesh by uniform vertex clustering (mesh_simplify.hip; nerf_hip_mesh_simplify_*, DESIGN.md
// section 3h-4).  The kernels use the component calls' workgroup shape (CC_WG, CC_PTS). ----
constexpr long long MS_MAX_SLOTS = 1ll << 31;  // the face table's slots are indexed by int32

// slots of the face table: the power of two that is at least 2 F (at least 2), capped at MS_MAX_SLOTS -- above F = 2^30 the table is
// between F and 2 F slots, still more than the keys it can hold
inline long long ms_table_slots(long long F) {
  long long s = 2;
  while (s < 2 * F && s < MS_MAX_SLOTS) s <<= 1;
  return s;
}

struct MsArgs {
  const float *verts, *normals;  // [V][3]; normals may be null (count only)
  const int* faces;        // [F][3]
  int V, F;
  float lo[3], cell[3];    // the cluster lattice
  int dims[3];
  long long ncell;         // dims[0] * dims[1] * dims[2] < 2^31
  long long slots;         // ms_table_slots(F)
  // workspace
  int* occ;                // [ncell] 1 where a vertex lies in the cell; after the scan the cell's cluster id + 1 (0: empty)
  int* vcl;                // [V] the vertex's cell, then (k_ms_accum) its cluster id; -1 for a vertex in no cluster
  int* cnt;                // [V] members of a cluster (clusters are at most V)
  long long *S, *T;        // [V][3] fixed-point sums of the members' lattice coordinates / normals
  int* ref;                // [V] 1 where a kept face uses the cluster; after the scan its output vertex id + 1 (0: dropped)
  int* fstate;             // [F] the face's table slot or -1 (k_ms_faces), then 1 for a kept face and 0 for any other (k_ms_mark)
  int* table;              // [slots] face indices, -1 for an empty slot
  int *tot, *base;         // [cc_blocks(max(ncell, V, F))]
  long long* scratch;      // [1] emit's throw-away total
  long long* counts;       // [6] = V', F', occupied clusters, flags, degenerate faces, duplicate faces (count only)
  float *out_verts, *out_normals;  // [max_v][3] (emit only; out_normals may be null)
  int* out_faces;          // [max_f][3]
  long long max_v, max_f;
};

hipError_t launch_ms_count(const MsArgs& a, hipStream_t st);  // everything up to counts
hipError_t launch_ms_emit(const MsArgs& a, hipStream_t st);   // positions / normals of the referenced clusters, the kept faces

// ---- edge topology, smoothing steps and face normals of an indexed mesh (mesh_smooth.hip; nerf_hip_mesh_edges_*,
// nerf_hip_mesh_smooth_step, nerf_hip_mesh_vertex_normals).  The component calls' workgroup shape. ----

// slots of the edge table: the power of two that is at least 4 F (at least 4) -- strictly more than the 3 F keys F faces can bring
inline long long me_table_slots(long long F) {
  long long s = 4;
  while (s < 4 * F) s <<= 1;
  return s;
}

struct MeArgs {
  const int* faces;        // [F][3] (build, normals)
  int V, F;
  long long slots;         // me_table_slots(F)
  long long cap;           // 6 F: the adjacency's entries (two per edge, at most 3 F edges)
  // workspace
  long long* keys;         // [slots] (min << 32) | max, -1 for an empty slot
  int *cnt, *tally;        // [slots] faces of the edge; those that run it min -> max less those that run it max -> min
  long long* off;          // [V + 1] row offsets into adj: the exclusive scan of the degrees
  int* cursor;             // [V] entries of the row placed so far (fill only)
  int* adj;                // [cap] the neighbours, row by row; the order inside a row is not defined
  long long *tot, *base;   // [cc_blocks(V)] degree sums per workgroup and their exclusive scan
  long long* T;            // [V][3] fixed-point sums of the incident faces' cross products (normals only)
  // build
  int *degree, *vflags;    // [V] outputs
  long long* counts;       // [8] = faces that take part, E, boundary, non-manifold, inconsistent edges, used vertices, flags, largest degree
  // step / normals
  const float* verts;      // [V][3]
  float* out;              // [max_v][3] the step's positions / the normals
  long long max_v;
  float lo[3], scale;      // the box
  double w;                // step only
  const int* pin;          // [V] step only: a vertex whose bit 0 is set stays (null: none is pinned)
};

hipError_t launch_me_build(const MeArgs& a, hipStream_t st);    // table, counts, degrees, flags, offsets, adjacency
hipError_t launch_me_step(const MeArgs& a, hipStream_t st);     // one Jacobi step verts -> out
hipError_t launch_me_normals(const MeArgs& a, hipStream_t st);  // T = 0, the faces' terms, the unit normals

// ---- geometry evaluation: measures, surface samples, exact nearest points, distance statistics (mesh_distance.hip;
// nerf_hip_mesh_measure, nerf_hip_mesh_sample, nerf_hip_points_*, nerf_hip_distance_stats).  The component
// calls' workgroup shape. ----
constexpr int MD_MAX_TAU = 8;  // thresholds of one statistics call

struct MdMeshArgs {
  const float* verts;      // [V][3]
  const int* faces;        // [F][3]
  int V, F;
  float lo[3], scale;      // the box (measure and the sampling weights)
  long long* out;          // measure: [8] = area, six volumes, three centroid moments (2^-40 box units), faces that take part, 0, 0
  // sampling
  long long n, cap_n;      // samples, and the rows the outputs hold
  unsigned seed;
  long long* cum;          // [F] inclusive prefix of the weights (workspace)
  long long *tot, *base;   // [cc_blocks(F)] weight sums per workgroup and their exclusive scan (workspace)
  long long* info;         // [1] = W
  float* points;           // [cap_n][3]
  int* face;               // [cap_n]
};

hipError_t launch_md_measure(const MdMeshArgs& a, hipStream_t st);
hipError_t launch_md_sample(const MdMeshArgs& a, hipStream_t st);

struct MdGridArgs {
  float lo[3], cell;       // the grid: corner and the one cell size
  int dims[3];
  int ncell;               // dims[0] * dims[1] * dims[2] < 2^31
  const float* ref;        // [M][3]
  const float* query;      // [N][3]
  int M, N;
  // workspace: the reference points' grid, then the queries' order
  int *cnt, *start;        // [ncell] points per cell (then the placement's cursors); [ncell + 1] a cell's first record
  float4* rec;             // [M] (x, y, z, original index), cell by cell
  int *qcnt, *qstart;      // the same for the queries
  float4* qrec;            // [N]
  int *tot, *base;         // [cc_blocks(ncell)] counts per workgroup of cells and their exclusive scan
  long long* scratch;      // [1] the queries' total (workspace)
  long long* counts;       // build: [2] = finite reference points, the fullest cell's points
  // query
  int* idx;                // [cap_n]
  double* dist2;           // [cap_n]
  long long cap_n;
};

hipError_t launch_md_grid_build(const MdGridArgs& a, hipStream_t st);
hipError_t launch_md_nearest(const MdGridArgs& a, bool sort_queries, hipStream_t st);

struct MdStatsArgs {
  const double* dist2;     // [N]
  long long N;
  double unit;
  int K;
  double tau2[MD_MAX_TAU]; // tau_k * tau_k
  long long* out;          // [4 + K]
};

hipError_t launch_md_stats(const MdStatsArgs& a, hipStream_t st);

// ---- ray casting against an indexed mesh, face visibility and face selection (mesh_raycast.hip; nerf_hip_mesh_raycast*,
// nerf_hip_mesh_face_rays, nerf_hip_mesh_select_faces_*).  The component calls' workgroup shape. ----
struct RcGridArgs {
  const float* verts;      // [V][3]
  const int* faces;        // [F][3]
  int V, F;
  float lo[3], cell;       // the grid: corner and the one cell size
  int dims[3];
  int ncell;               // dims[0] * dims[1] * dims[2] < 2^31
  long long cap_entries;   // the entries the workspace holds (< 2^31)
  // workspace
  int *cnt, *start;        // [ncell] entries per cell (then the placement's cursors); [ncell + 1] a cell's first entry
  int* entries;            // [cap_entries] face indices, cell by cell; the order inside a cell is not defined
  int* outside;            // [F] the OUTSIDE faces, ascending
  int *tot, *base;         // [cc_blocks(max(ncell, F))]
  long long* info;         // [2] = the entries the scan counted, the OUTSIDE faces
  long long* counts;       // count only: [3] = faces that take part, entries E, OUTSIDE faces
};

struct RcCastArgs {
  RcGridArgs g;
  const float *orig, *dir; // [N][3]
  const int* skip;         // [N] or null: the face ray i ignores
  long long N, cap_n;
  double tmin, tmax;
  double *t, *uv;          // [cap_n], [cap_n][2] (closest hit)
  int* face;               // [cap_n]
  signed char* side;       // [cap_n]
  unsigned char* occluded; // [cap_n] (any hit)
};

struct RcFaceRaysArgs {
  const float* verts;
  const int* faces;
  int V, F;
  float cam[3];
  double Q[9];             // row-major
  int H, W;
  float *orig, *dir;       // [cap_f][3]
  unsigned char* valid;    // [cap_f]
  long long cap_f;
};

struct SelArgs {
  const float *verts, *normals, *rgb;  // [V][3]; normals / rgb (with their outputs) may be null (emit)
  const int* faces;        // [F][3]
  const unsigned char* keep;  // [F]
  int V, F;
  int *used, *newidx;      // [V] 1 where a kept face uses the vertex; its rank among those, -1 for any other (workspace)
  int *tot, *base;         // [cc_blocks(max(V, F))] (workspace)
  long long* counts;       // count: [2] = V', F'; emit: the workspace's throw-away totals
  float *out_verts, *out_normals, *out_rgb;  // [max_v][3]
  int* out_faces;          // [max_f][3]
  long long max_v, max_f;
};

hipError_t launch_rc_grid_count(const RcGridArgs& a, hipStream_t st);
hipError_t launch_rc_grid_fill(const RcGridArgs& a, hipStream_t st);
hipError_t launch_rc_cast(const RcCastArgs& a, bool any_hit, hipStream_t st);
hipError_t launch_rc_face_rays(const RcFaceRaysArgs& a, hipStream_t st);
hipError_t launch_sel_count(const SelArgs& a, hipStream_t st);
hipError_t launch_sel_emit(const SelArgs& a, hipStream_t st);

// ---- TSDF fusion of depth images (tsdf.hip; nerf_hip_tsdf_integrate; rule T of include/nerf_hip.h), of the
// views' colours beside it and the colour volume sampled at points (nerf_hip_tsdf_integrate_color / nerf_hip_tsdf_sample_color, section
// 3h-10; rules TC and S) ----
constexpr int TSDF_VIEWS = 32;                 // views per launch (NERF_HIP_TSDF_VIEWS_PER_LAUNCH)
constexpr int TSDF_WG = 256;

struct TsdfCam {
  double Q[9];             // row-major: world direction -> homogeneous pixel coordinates
  float o[3];              // the camera's position
  float pad;
};

struct TsdfArgs {
  float *tsdf, *weight;    // [nx][ny][nz], z fastest
  float4* color;           // [nx][ny][nz] of (R, G, B, Wc), or null: rule TC's state (the COLOR instantiation; null selects the plain one)
  const float* rgb;        // [nviews][H][W][3]: the FIRST view of this launch onwards (COLOR only)
  int ny, nz;
  int npts;                // nx * ny * nz < 2^31
  float lo[3], step[3];
  const float* depth;      // [nviews][H][W]: the FIRST view of this launch onwards
  const float* opacity;    // the same, or null
  int nviews;              // 1 .. TSDF_VIEWS
  int H, W;
  int carve;
  float min_opacity;
  double trunc;
  TsdfCam cam[TSDF_VIEWS]; // by value: uniform reads of the kernel arguments, no buffer to fill and keep alive
};
static_assert(sizeof(TsdfArgs) <= 4096, "a kernel's arguments may take 4 KB");

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t st);

struct TsdfSampleArgs {
  const float* points;     // [M][3]
  const float4* color;     // [nx][ny][nz] of (R, G, B, Wc)
  int nx, ny, nz;
  float lo[3], step[3];
  float* rgb;              // [M][3]
  unsigned char* valid;    // [M]
  long long M;
};

hipError_t launch_tsdf_sample_color(const TsdfSampleArgs& a, hipStream_t st);

// ---- SH radiance volumes (volume.hip; the nerf_hip_volume_* calls; rules VA, VS, VO, VL and VR of
// include/nerf_hip.h).  The lattice: nx, ny, nz >= 2, npts = nx * ny * nz < 2^31 ----
constexpr int VOL_WG = 256;                    // the one-thread-per-item kernels
constexpr int VOL_MARCH_WG = 64;               // k_volume_march: one wave per workgroup, so a workgroup retires with its slowest ray
constexpr int VOL_MAX_STEPS = 65536;           // NERF_HIP_VOLUME_MAX_STEPS

struct VolLattice {
  int nx, ny, nz;
  float lo[3], step[3];
};

struct VolActiveArgs {
  const float* sigma;      // [nx][ny][nz]
  int nx, ny, nz;
  int *tot, *base;         // [cc_blocks(npts)] (workspace)
  long long* count;        // [1]: the caller's count, or the workspace's throw-away one (emit)
  int* index;              // [max_n] (emit)
  long long max_n;
};

struct VolPointsArgs {
  const int* index;        // [n]
  long long n;
  VolLattice g;
  float* points;           // [n][3]
};

struct VolShArgs {
  float* coef;             // [npts][ncoef][3]
  long long npts;
  int ncoef;
  const int* index;        // [n]
  long long n;
  const float* rgb;        // [n][3]
  float b[9];              // b_km of this call's direction
};

struct VolBlocksArgs {
  const float* sigma;
  int nx, ny, nz;
  int B;
  int bx, by, bz;
  unsigned char* occ;      // [bx][by][bz], zeroed by the launch sequence
};

struct VolSampleArgs {
  const float *sigma, *coef;
  VolLattice g;
  const float *points, *dirs;  // [M][3]
  long long M;
  float *out_sigma, *out_rgb;  // [M], [M][3]
};

struct VolRenderArgs {
  const float *sigma, *coef;
  const unsigned char* occ;
  VolLattice g;
  int B, bx, by, bz;
  const float *origins, *dirs, *tmin, *tmax;  // [N][3], [N][3], [N], [N]
  long long N;
  float dt, t_stop, bg[3];
  float *rgb, *maps;       // [N][3], [N][2]
  int* steps;              // [N][2]
};

hipError_t launch_volume_active(const VolActiveArgs& a, bool emit, hipStream_t st);
hipError_t launch_volume_points(const VolPointsArgs& a, hipStream_t st);
hipError_t launch_volume_sh_accumulate(const VolShArgs& a, hipStream_t st);
hipError_t launch_volume_blocks(const VolBlocksArgs& a, hipStream_t st);
hipError_t launch_volume_sample(const VolSampleArgs& a, int ncoef, hipStream_t st);
hipError_t launch_volume_render(const VolRenderArgs& a, int ncoef, hipStream_t st);

// ---- fine-tuning a baked volume (volume_grad.hip; nerf_hip_volume_render_backward, nerf_hip_volume_adam_step, DESIGN.md section
// 3h-13; rules VG and VU of include/nerf_hip.h) ----
constexpr int VOL_GRAD_SHIFT = 40;             // NERF_HIP_VOLUME_GRAD_SHIFT

struct VolGradArgs {
  VolRenderArgs r;         // the forward's arguments; its outputs (rgb, maps, steps) are not used
  const float *g_rgb, *g_maps;      // [N][3], [N][2] or null
  long long *acc_sigma, *acc_coef;  // [npts], [npts][ncoef][3]: fixed-point sums, 2^-40 units
};

struct VolAdamArgs {
  float *sigma, *coef;     // [npts], [npts][ncoef][3]
  long long npts;
  int ncoef;
  const int* index;        // [n]: the active list of the volume as baked
  long long n;
  long long *acc_sigma, *acc_coef;
  float *m, *v;            // [n][1 + 3 ncoef]
  double grad_scale, lr_sigma, lr_coef, beta1, beta2, eps;
  double c1, c2;           // 1 - beta1^step, 1 - beta2^step
};

hipError_t launch_volume_render_backward(const VolGradArgs& a, int ncoef, hipStream_t st);
hipError_t launch_volume_adam_step(const VolAdamArgs& a, hipStream_t st);

// ---- coarse-to-fine fine-tuning (volume_refine.hip; nerf_hip_volume_member_mask, _tv_backward, _upsample, _prune, DESIGN.md section
// 3h-14; rules VM, VT, VX and VP of include/nerf_hip.h) ----
struct VolMemberArgs {
  const int* index;        // [n]
  long long n, npts;
  unsigned char* member;   // [npts]
};

struct VolTvArgs {
  const float *sigma, *coef;        // [npts], [npts][ncoef][3]
  int nx, ny, nz, ncoef;
  const int* index;                 // [n]: distinct
  long long n;
  const unsigned char* member;      // [npts]: rule VM's mask of the level's whole list
  double w_sigma, w_coef, eps;
  long long *acc_sigma, *acc_coef;  // rule VG's accumulators
};

struct VolUpsampleArgs {
  const float *sigma, *coef;  // the coarse lattice nx x ny x nz
  int nx, ny, nz, ncoef;
  float *sigma2, *coef2;      // the lattice (2 nx - 1) x (2 ny - 1) x (2 nz - 1)
};

struct VolPruneArgs {
  float *sigma, *coef;
  int nx, ny, nz, ncoef;
  float threshold;
};

hipError_t launch_volume_member_mask(const VolMemberArgs& a, hipStream_t st);
hipError_t launch_volume_tv_backward(const VolTvArgs& a, hipStream_t st);
hipError_t launch_volume_upsample(const VolUpsampleArgs& a, hipStream_t st);
hipError_t launch_volume_prune(const VolPruneArgs& a, hipStream_t st);

// ---- compact volumes (volume_compact.hip; the nerf_hip_volume_compact_* calls; rule VC of
// include/nerf_hip.h): the rows of the active points behind an int32 slot lattice, fp32 or fp16 coefficients ----
// halves of an fp16 coefficient row: 3 ncoef rounded up to a multiple of 4 (4 / 12 / 28), so a row is whole 8-byte words
constexpr int vol_half_stride(int ncoef) { return (3 * ncoef + 3) & ~3; }

struct VolCompact {
  const int* slot;          // [nx][ny][nz]: the row of the point, or anything outside [0, n) where there is none
  const float* sigma_rows;  // [n]
  const void* coef_rows;    // [n][3 ncoef] fp32, or [n][vol_half_stride(ncoef)] fp16 (8-byte aligned)
  long long n;
};

struct VolSlotsArgs {
  const int* index;        // [n]
  long long n, npts;
  int* slot;               // [npts], filled with -1 by the launch sequence
};

// pack gathers dense -> rows, unpack scatters rows -> dense (zeroed by the caller); a null sigma pair / coef pair is left out
struct VolPackArgs {
  float *sigma, *coef;     // [npts], [npts][ncoef][3] (pack reads them, unpack writes them)
  long long npts;
  int ncoef;
  const int* index;        // [n], or null: row r is point r
  long long n;
  float* sigma_rows;       // [n]
  void* coef_rows;         // [n][stride]
};

struct VolCompactSampleArgs {
  VolCompact c;
  VolLattice g;
  const float *points, *dirs;  // [M][3]
  long long M;
  float *out_sigma, *out_rgb;  // [M], [M][3]
};

struct VolCompactRenderArgs {
  VolCompact c;
  VolRenderArgs r;         // the dense march's arguments; its sigma and coef are not used
};

hipError_t launch_volume_compact_slots(const VolSlotsArgs& a, hipStream_t st);
hipError_t launch_volume_compact_pack(const VolPackArgs& a, bool half, hipStream_t st);
hipError_t launch_volume_compact_unpack(const VolPackArgs& a, bool half, hipStream_t st);
hipError_t launch_volume_compact_sample(const VolCompactSampleArgs& a, int ncoef, bool half, hipStream_t st);
hipError_t launch_volume_compact_render(const VolCompactRenderArgs& a, int ncoef, bool half, hipStream_t st);

// ---- fine-tuning a compact volume (volume_compact_grad.hip; nerf_hip_volume_compact_render_backward, _adam_step, _tv_backward,
// DESIGN.md section 3h-16; rules VCG, VCU and VCT of include/nerf_hip.h): rules VG, VU and VT over fp32 rows, the accumulators and the
// moments one per row ----
struct VolCompactGradArgs {
  VolCompact c;            // fp32 rows
  VolRenderArgs r;         // the dense march's arguments; its sigma, coef and outputs are not used
  const float *g_rgb, *g_maps;                // [N][3], [N][2] or null
  long long *acc_sigma_rows, *acc_coef_rows;  // [n], [n][3 ncoef]: fixed-point sums, 2^-40 units
};

struct VolCompactAdamArgs {
  float *sigma_rows, *coef_rows;  // [n], [n][3 ncoef]
  int ncoef;
  long long n;
  long long *acc_sigma_rows, *acc_coef_rows;
  float *m, *v;            // [n][1 + 3 ncoef]
  double grad_scale, lr_sigma, lr_coef, beta1, beta2, eps;
  double c1, c2;           // 1 - beta1^step, 1 - beta2^step
};

struct VolCompactTvArgs {
  VolCompact c;            // fp32 rows; a point is a member iff its slot lies in [0, n)
  const int* point;        // [n]: the lattice point of each row, -1: none
  int nx, ny, nz, ncoef;
  double w_sigma, w_coef, eps;
  long long *acc_sigma_rows, *acc_coef_rows;
};

hipError_t launch_volume_compact_render_backward(const VolCompactGradArgs& a, int ncoef, hipStream_t st);
hipError_t launch_volume_compact_adam_step(const VolCompactAdamArgs& a, hipStream_t st);
hipError_t launch_volume_compact_tv_backward(const VolCompactTvArgs& a, hipStream_t st);

// ---- vector-quantised compact volumes (volume_vq.hip; nerf_hip_volume_compact_importance and the nerf_hip_volume_vq_* calls,
// DESIGN.md section 3h-17; rules VI, VQ-A, VQ-U and VQ-D of include/nerf_hip.h) ----
constexpr int VQ_WG = 256;                     // k_volume_vq_assign: one row per lane
constexpr int VQ_TILE = 128;                   // codes per LDS tile: 128 x 28 x 4 = 14 KiB at degree 2
constexpr int VQ_SHIFT = 20;                   // NERF_HIP_VOLUME_VQ_SHIFT
constexpr int VQ_MAX_CODES = 65536;            // NERF_HIP_VOLUME_VQ_MAX_CODES: a code is a uint16

struct VolImportanceArgs {
  VolCompact c;            // coef_rows is not read
  VolRenderArgs r;         // the dense march's arguments; of its outputs only steps is written
  long long* imp_rows;     // [n]: fixed-point sums, 2^-40 units
};

struct VqAssignArgs {
  const float* rows;       // [m][3 ncoef]
  long long m;
  const float* codebook;   // [K][3 ncoef]
  long long K;
  int* assign;             // [m]
  float* dist;             // [m] or null
};

struct VqAccumulateArgs {
  const float* rows;       // [m][words]
  long long m;
  int words;               // 3 ncoef
  const long long* weight; // [m] or null: u = 1
  long long imax;          // <= 0: u = 1
  const int* assign;       // [m]
  long long K;
  long long *sum, *cnt;    // [K][words], [K]: fixed-point sums, 2^-20 units
};

struct VqUpdateArgs {
  float* codebook;         // [K][words]
  long long K;
  int words;
  const long long *sum, *cnt;
};

struct VqDecodeArgs {
  const unsigned char* cls;          // [n]: 0 pruned, 1 coded, 2 kept
  const int* rank;                   // [n]: the row's rank within its class
  long long n;
  const unsigned short* code;        // [n_coded]
  long long n_coded;
  const unsigned long long* kept;    // [n_kept][stride / 4]: fp16 rows as 8-byte words
  long long n_kept;
  const unsigned long long* codebook;  // [K][stride / 4]
  long long K;
  int stride;                        // vol_half_stride(ncoef)
  unsigned long long* out;           // [n][stride / 4]
};

hipError_t launch_volume_compact_importance(const VolImportanceArgs& a, hipStream_t st);
hipError_t launch_volume_vq_assign(const VqAssignArgs& a, int ncoef, hipStream_t st);
hipError_t launch_volume_vq_accumulate(const VqAccumulateArgs& a, hipStream_t st);
hipError_t launch_volume_vq_update(const VqUpdateArgs& a, hipStream_t st);
hipError_t launch_volume_vq_decode(const VqDecodeArgs& a, hipStream_t st);

// ---- fine-tuning a vector-quantised volume (volume_vq_train.hip; nerf_hip_volume_vq_expand, _grad_reduce, _adam_step, DESIGN.md
// section 3h-18; rules VQ-X, VQ-G and VQ-V of include/nerf_hip.h) ----
constexpr int VQT_WG = 256;                    // k_volume_vq_reduce: floor(256 / W) member lanes of W words each
constexpr int VQT_CHUNK = 256;                 // NERF_HIP_VOLUME_VQ_REDUCE_CHUNK: consecutive entries of member[] per workgroup

struct VqExpandArgs {
  const unsigned char* cls;          // [n]
  const int* rank;                   // [n]
  long long n;
  const unsigned short* code;        // [n_coded]
  long long n_coded;
  const float* kept32;               // [n_kept][words]
  long long n_kept;
  const float* codebook32;           // [K][words]
  long long K;
  int words;                         // 3 ncoef
  float* out;                        // [n][words]
  long long* acc_coef_rows;          // [n][words] or null: zeroed where a row receives +0
};

struct VqReduceArgs {
  long long* acc_coef_rows;          // [n][3 ncoef]: read and zeroed at the members
  long long n;
  const int* offset;                 // [K + 1]: clamped by the kernel
  const int* member;                 // [n_coded]: rows, grouped by code
  long long n_coded, K;
  long long* acc_code;               // [K][3 ncoef]
};

struct VqAdamArgs {
  float* sigma_rows;                 // [n]
  long long n;
  float* kept32;                     // [n_kept][words]
  const int* kept_row;               // [n_kept]
  long long n_kept;
  float* codebook32;                 // [K][words]
  long long K;
  int words;
  long long *acc_sigma_rows, *acc_coef_rows, *acc_code;
  float *m, *v;                      // [n + n_kept words + K words]
  double grad_scale, lr_sigma, lr_coef, beta1, beta2, eps;
  double c1, c2;                     // 1 - beta1^step, 1 - beta2^step
};

hipError_t launch_volume_vq_expand(const VqExpandArgs& a, hipStream_t st);
hipError_t launch_volume_vq_grad_reduce(const VqReduceArgs& a, int ncoef, hipStream_t st);
hipError_t launch_volume_vq_adam_step(const VqAdamArgs& a, hipStream_t st);

// ---- texture atlases of indexed meshes (mesh_texture.hip; nerf_hip_mesh_atlas_texels, nerf_hip_mesh_texture_sample, DESIGN.md section
// 3h-11; rules TA and TX of include/nerf_hip.h).  The atlas of (F, n): cells of c = n + 5 texels, Sx per row, W = Sx * c wide ----
constexpr int TEX_WG = 256;

struct AtlasTexelsArgs {
  const float *verts, *normals;  // [V][3]
  const int* faces;        // [F][3]
  int V, F;
  int n, c, Sx, W;         // chart edge, cell edge, cells per atlas row, atlas width
  int row0;                // the band's first atlas row
  long long T;             // rows * W < 2^31: the band's texels
  float *points, *dirs;    // [T][3]
  unsigned char* mask;     // [T]
};

struct TextureSampleArgs {
  const float* image;      // [H][W][3]
  int F, n, c, Sx, W;
  const int* face;         // [N]
  const double* uv;        // [N][2]
  long long N;
  float bg[3];
  float* rgb;              // [N][3]
  unsigned char* valid;    // [N]
};

hipError_t launch_atlas_texels(const AtlasTexelsArgs& a, hipStream_t st);
hipError_t launch_texture_sample(const TextureSampleArgs& a, hipStream_t st);

// ---- narrow-band density grid (band.hip + k_field_fwd_reg's SRC_CORNERS / SRC_BLOCKS forms; nerf_hip_band_*) ----
constexpr int BAND_WG = 256;                   // blocks per workgroup of the per-block kernels (the scan's unit)

struct BandArgs {
  float* sigma;            // [nx][ny][nz], z fastest: the dense grid
  int nx, ny, nz;
  int r;                   // block size, 2 <= r <= max(nx, ny, nz)
  int nbx, nby, nbz, nblk; // blocks per axis = ceil(n / r), and their product
  int nwg;                 // ceil(nblk / BAND_WG)
  float level;
  unsigned char *active, *seed;  // [nblk] the sets A and S
  unsigned* offs;          // [nblk] (exclusive offset among the workgroup's new blocks << 1) | new
  int* list;               // [nblk] the new blocks, ascending
  int* tn;                 // [nwg] new blocks per workgroup
  long long* tp;           // [nwg] lattice points they own
  int* bn;                 // [nwg] exclusive scan of tn
  long long* counts;       // [2] = new blocks, the points they own
};

hipError_t launch_band_corners(const FieldArgs& a, const QuerySrc& q, hipStream_t st);  // a.M = ext[0] * ext[1] * ext[2]
hipError_t launch_band_blocks(const FieldArgs& a, const QuerySrc& q, hipStream_t st);   // a.M = entries * ext[0] * ext[1] * ext[2]
hipError_t launch_band_begin(const BandArgs& a, hipStream_t st);   // seeds from the corner samples (A = empty), then the fill
hipError_t launch_band_reseed(const BandArgs& a, hipStream_t st);  // S from A and the grid as it stands
hipError_t launch_band_next(const BandArgs& a, hipStream_t st);    // new = dilate(S) - A -> list, counts; A |= new

// ---- image metrics (metrics.hip): per-view MSE and SSIM of pred vs gt [n][H][W][3] fp32, fp64 arithmetic
constexpr int MT_WIN = 11;                   // SSIM's Gaussian window (taps); valid filtering drops MT_WIN - 1 rows / columns
constexpr int MT_X = 32, MT_Y = 16;          // valid SSIM outputs per workgroup (columns x rows)
constexpr int MT_WG = 256;

inline int metrics_tiles_x(int W) { return (W - MT_WIN + MT_X) / MT_X; }  // ceil((W - 10) / MT_X)
inline int metrics_tiles_y(int H) { return (H - MT_WIN + MT_Y) / MT_Y; }

struct MetricsArgs {
  const float *pred, *gt;  // [n][H][W][3]
  int n, H, W;             // H, W >= MT_WIN, H * W * 3 < 2^31
  int tiles_x, tiles;      // workgroups per view: tiles_x * tiles_y
  double* part;            // [n * tiles][2]: (sum of squared errors over the tile's own pixels, sum of the tile's SSIM map)
  double *mse, *ssim;      // [n]
  double g[MT_WIN];        // the normalised window
};

hipError_t launch_image_metrics(const MetricsArgs& a, hipStream_t st);  // per-tile partial sums, then a fixed-order pass per view

}  // namespace nerf
