/*
 * nerf_hip.h -- C ABI of libnerf_hip.so, the MI355X (gfx950) volume-rendering hot path.
 *
 * The reference (D-Hank/NeRF-tiny) has no FFI: its boundary for this path is the Python
 * method surface of NeRFModel (nerf.py:170 ctor, nerf.py:333-348 forward, nerf.py:325-331
 * ray_loss, autograd backward at nerf.py:473).  Each entry point below replaces the cited
 * span of nerf.py; INTEGRATION.md shows the ctypes stub a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / HIP C++ types.  `stream` is a hipStream_t passed
 *     as void* (NULL = default stream).  Every call only ENQUEUES work on `stream`; no call
 *     synchronises with the host except nerf_hip_read_status() / nerf_hip_read_status_sticky().
 *   - ownership: the caller allocates every buffer (device unless marked HOST) including the
 *     workspace; the library allocates nothing persistent and frees nothing.
 *   - errors: 0 = NERF_HIP_OK, negative = error; nerf_hip_last_error() gives the text
 *     (thread-local).  The library never aborts the process.
 *   - threading: re-entrant per (device, stream); calls sharing a workspace must be ordered
 *     on one stream.
 *   - stream capture: NOT replay-safe.  Every nerf_hip_forward / nerf_hip_train_step bakes a per-call token into
 *     kernel arguments (the in-launch hand-off of the bf16-MLP preparation, the generation stamp of the status word);
 *     a captured graph replayed later would present last replay's token.  Enqueue the calls afresh.
 *   - workspace: the caller zeroes its first 256 bytes (the status region) ONCE after allocating it; the library
 *     never clears words 32..63 of that region on its own (sticky flags, nerf_hip_read_status_sticky).
 *   - all floating point data is IEEE fp32 ("f32"), row-major.
 *
 * Weight order (`weights24`, HOST array of 24 DEVICE pointers) = NeRFModel.network.parameters()
 * order, nn.Linear layout [out, in] (nerf.py:85-99):
 *    0..15  point_layer[i].0.{weight,bias}  i = 0..7   W0[256,60] W1-3[256,256] W4[256,316] W5-7[256,256]
 *   16,17   sigma_layer.0.{weight[1,256],bias[1]}
 *   18,19   point_info.{weight[256,256],bias[256]}
 *   20,21   dir_info.0.{weight[128,280],bias[128]}
 *   22,23   color_layer.0.{weight[3,128],bias[3]}
 */
#ifndef NERF_HIP_H
#define NERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_HIP_ABI_VERSION 7 /* 2: NERF_HIP_BF16_MLP, nerf_hip_field_bf16; 3: nerf_hip_backward_overlap, NERF_HIP_SPLIT_MLP;
                                  4: nerf_hip_read_status_sticky; 5: nerf_hip_train_step; 6: NERF_HIP_CORRECTED;
                                  7: nerf_hip_query_ws_bytes, nerf_hip_query, nerf_hip_density_grid; later additions under 7:
                                     nerf_hip_mesh_ws_bytes, nerf_hip_mesh_count, nerf_hip_mesh_emit; nerf_hip_forward_maps;
                                     nerf_hip_query_grad_ws_bytes, nerf_hip_query_grad; nerf_hip_metrics_ws_bytes,
                                     nerf_hip_image_metrics; nerf_hip_forward_maps_train, nerf_hip_backward_maps;
                                     nerf_hip_band_ws_bytes, nerf_hip_band_begin, nerf_hip_band_grow; nerf_hip_mesh_cc_ws_bytes,
                                     nerf_hip_mesh_cc_round, nerf_hip_mesh_cc_ids, nerf_hip_mesh_cc_stats, nerf_hip_mesh_cc_compact
                                     (with NERF_HIP_ERR_CONVERGE); nerf_hip_mesh_simplify_ws_bytes, nerf_hip_mesh_simplify_count,
                                     nerf_hip_mesh_simplify_emit (with NERF_HIP_SIMPLIFY_TABLE_FULL); nerf_hip_mesh_edges_ws_bytes,
                                     nerf_hip_mesh_edges_build (with NERF_HIP_EDGES_TABLE_FULL), nerf_hip_mesh_smooth_step,
                                     nerf_hip_mesh_vertex_normals; nerf_hip_mesh_measure, nerf_hip_mesh_sample_ws_bytes,
                                     nerf_hip_mesh_sample, nerf_hip_points_nearest_ws_bytes, nerf_hip_points_grid_build,
                                     nerf_hip_points_nearest, nerf_hip_distance_stats; the nerf_hip_mesh_raycast* calls,
                                     nerf_hip_mesh_face_rays, nerf_hip_mesh_select_faces_*; nerf_hip_tsdf_integrate;
                                     nerf_hip_tsdf_integrate_color, nerf_hip_tsdf_sample_color, nerf_hip_mesh_count_masked,
                                     nerf_hip_mesh_emit_masked; nerf_hip_coarse_composite_maps,
                                     nerf_hip_coarse_composite_backward_maps, nerf_hip_merge_composite_train,
                                     nerf_hip_merge_composite_backward; nerf_hip_forward_quantiles,
                                     nerf_hip_coarse_composite_quantiles, nerf_hip_merge_composite_quantiles
                                     (with NERF_HIP_MAX_QUANTILES); nerf_hip_forward_distortion_train,
                                     nerf_hip_backward_distortion, nerf_hip_coarse_composite_distortion,
                                     nerf_hip_merge_composite_distortion, nerf_hip_coarse_composite_backward_distortion,
                                     nerf_hip_merge_composite_backward_distortion; nerf_hip_mesh_atlas_dims,
                                     nerf_hip_mesh_atlas_texels, nerf_hip_mesh_texture_sample; nerf_hip_normals_ws_bytes,
                                     nerf_hip_normals_ws_offset, nerf_hip_forward_normals, nerf_hip_normal_composite;
                                     the nerf_hip_volume_* calls (with NERF_HIP_VOLUME_MAX_STEPS);
                                     nerf_hip_volume_render_backward, nerf_hip_volume_adam_step
                                     (with NERF_HIP_VOLUME_GRAD_SHIFT); nerf_hip_volume_member_mask,
                                     nerf_hip_volume_tv_backward, nerf_hip_volume_upsample, nerf_hip_volume_prune;
                                     the nerf_hip_volume_compact_* calls; nerf_hip_volume_compact_importance and the
                                     nerf_hip_volume_vq_* calls (with NERF_HIP_VOLUME_VQ_SHIFT, NERF_HIP_VOLUME_VQ_MAX_CODES) */

enum {
  NERF_HIP_OK = 0,
  NERF_HIP_ERR_ARG = -1,       /* bad shape / null pointer / unsupported size        */
  NERF_HIP_ERR_WORKSPACE = -2, /* workspace too small for (B, Nc, Nf, flags)          */
  NERF_HIP_ERR_DEVICE = -3,    /* a HIP runtime call failed (text in last_error)      */
  NERF_HIP_ERR_ARCH = -4,      /* device is not gfx950                                */
  NERF_HIP_ERR_CONVERGE = -5   /* nerf_hip_mesh_cc_round: no fixed point within its cap of rounds */
};

/* flags */
enum {
  NERF_HIP_SAVE_FOR_BACKWARD = 1 << 0, /* forward keeps activations in the workspace for nerf_hip_backward */
  NERF_HIP_FORCE_TILE_KERNEL = 1 << 1, /* inference: use the LDS-tile field kernel instead of the register-resident one
                                          (same results up to summation order; for A/B measurements and tests).  With
                                          NERF_HIP_BF16_MLP: inference on the 32x32x16 kernel that training uses instead of the
                                          16x16x32 one (bit-identical to the forward half of a training call) */
  NERF_HIP_BF16_MLP = 1 << 2,          /* BASELINE.json cfg3 "bf16 MLP / fp32 composite": the 12 linear layers of the field MLP
                                          run on bf16 MFMA (bf16-rounded weights and layer inputs, fp32 accumulation and
                                          biases); rays, encodings, compositing, resampling and sort stay fp32.  NOT within
                                          1e-4 of the fp32 reference (about 1e-2); off by default */
  NERF_HIP_WEIGHTS_UNCHANGED = 1 << 3, /* nerf_hip_forward only: the caller guarantees that weights24 hold the same values as in the
                                          previous nerf_hip_forward call on this workspace with the same other flags, so the
                                          packed weight image in the workspace is reused instead of rebuilt (rendering loops) */
  NERF_HIP_SPLIT_MLP = 1 << 4,         /* OPT-IN split-fp32 arithmetic: the linear layers run on bf16 MFMA with every fp32 operand split into two
                                          bf16 parts (hi + mid, 16 significant bits) and three MFMAs per product, fp32 accumulation.
                                          Without NERF_HIP_SAVE_FOR_BACKWARD (inference): within the same 1e-4 bar as the exact-fp32 default
                                          (measured 3e-6 / 2e-5 against the reference's outputs), 3x its rate.  WITH it (the split-fp32 TRAIN
                                          step; pass the flag to nerf_hip_backward / nerf_hip_train_step as well): forward, dX chain and
                                          weight-gradient products in that arithmetic, 2.1x the exact step's rate, loss to 1e-5, gradients inside
                                          the bands the exact path is held to.  Off by default: the default keeps exact k-ordered fp32 fma
                                          chains.  Ignored with NERF_HIP_BF16_MLP */
  NERF_HIP_CORRECTED = 1 << 5,         /* OPTIONAL EXTRA, off by default, NOT the reference's results (SURVEY.md 8a "Q": reproduce the quirks by
                                          default, offer a flagged corrected mode): (Q1) the merged samples are sorted ONCE, by depth, stably, and
                                          rgb / sigma move with their sample, instead of nerf.py:307-308's five independent channel sorts; (Q9) t_fine
                                          is treated as detached: no gradient flows through the fine depths (neither through the sample positions
                                          nor through the merged deltas) into the coarse pass, instead of nerf.py:259's attached t_fine.  Every other
                                          quirk (Q2-Q8, Q10-Q12) stays.  Pass the same flag to forward and backward.  Parity of this mode is
                                          UNPINNED (the reference has no such mode): it is tested against the oracle's restatement of the same
                                          two changes only */
};

/* status word bits (nerf_hip_read_status) */
enum {
  NERF_HIP_STATUS_RESAMPLE_INDEX = 1 << 0, /* the condition on which nerf.py:251-253 calls exit(0) (quirk Q7) */
  NERF_HIP_STATUS_PREP_TIMEOUT = 1 << 1,   /* bf16-MLP calls only: a block of the one-launch preparation gave up waiting for the weight fold
                                              of the SAME launch (bounded wait; relies on in-order workgroup dispatch, which gfx950 provides but
                                              HIP does not promise -- NERF_PREP_BF16=0 in the environment selects separate launches instead).
                                              The packed weight image of that call is then POISONED with NaN: its C_coarse / C_fine / loss /
                                              gradients are NaN, never plausible wrong numbers.  Reported by nerf_hip_read_status for that call
                                              and for every later call that reuses the image (NERF_HIP_WEIGHTS_UNCHANGED), and in the sticky
                                              word.  Never seen outside the fault-injection test. */
};

/* Limits of this build: 2 <= B, 2 <= Nc <= 1024, 1 <= Nf <= 1024, Nc + Nf <= 2048. */

int nerf_hip_abi_version(void);
const char* nerf_hip_last_error(void);

/* Bytes of device workspace nerf_hip_forward / nerf_hip_backward need for these sizes. */
int nerf_hip_ws_bytes(int B, int Nc, int Nf, int flags, size_t* bytes);

/* Byte offset of a named intermediate inside the workspace (introspection for tests / debugging):
 * "t_c" "sig_c" "rgb_c" "w_c" "t_f" "sig_f" "rgb_f", and with NERF_HIP_SAVE_FOR_BACKWARD also "bundle" "w_m" "perm"
 * "save" "G" "dz" "dspre" "drgb_c" "dsig_c" "drgb_f" "dsig_f" "dt_f" (gradient buffers are valid after backward).
 * "save" and "G" are [tensor][B*(Nc+Nf) + 64][256] f32: 64 dump rows follow the real rows of every tensor; "dz" is
 * [B*(Nc+Nf)][4] = (dz_r, dz_g, dz_b, dsigma_pre).  "sbuf" [B][128] = per-ray sums of the dir_info pre-activation gradient,
 * "gdbuf" [B][24] = the direction encodings (both valid after a fp32 backward).  "dbg": 16384 u64 words written only by
 * diagnostic builds (make stamps). */
int nerf_hip_ws_offset(int B, int Nc, int Nf, int flags, const char* name, size_t* offset);

/*
 * Whole forward: replaces NeRFModel.forward -> render_rays (nerf.py:333-348, 286-323).
 *   row, col        [B] i64   pixel coordinates; x <- row, y <- col (nerf.py:186-188)
 *   poses_bound     [B,17] f32  rows as loader.py:33: 3x5 [R|o|hwf] then near, far (already cast, nerf.py:338)
 *   K_inv9          HOST [9] f32, the matrix passed to forward (already transposed, nerf.py:433)
 *   ray0_near_far   HOST [2] f32 or NULL.  The slope of the inverse CDF uses the coarse spacing of
 *                   RAY 0 OF THE BATCH for every ray (nerf.py:233); a caller that shards one batch
 *                   over several GPUs passes the global ray 0's (near, far) here; NULL = this call's ray 0.
 *   last_delta      nerf.py:286 `last` (1e-4)
 *   C_coarse,C_fine [B,3] f32 out
 *   ws              workspace of >= nerf_hip_ws_bytes(B,Nc,Nf,flags) bytes, 256-byte aligned
 */
int nerf_hip_forward(const float* const* weights24, const int64_t* row, const int64_t* col,
                     const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                     int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine,
                     void* ws, size_t ws_bytes, int flags, void* stream);

/*
 * nerf_hip_forward plus each ray's expected depth and accumulated opacity (INFERENCE only).
 *   maps            [B,4] f32 out, device: (D_c, A_c, D_f, A_f) per ray, where
 *                     D_c = sum_i w_c,i t_c,i   A_c = sum_i w_c,i   over the Nc coarse samples, with the weights of C_coarse;
 *                     D_f = sum_i w_i t_s,i     A_f = sum_i w_i     over the Nc + Nf merged, sorted samples, with the weights of C_fine.
 *                   t_s is the SORTED depth channel: without NERF_HIP_CORRECTED the five channels are sorted independently (as the
 *                   reference does), so D_f is what compositing t like a colour channel gives; with NERF_HIP_CORRECTED (one joint sort)
 *                   it is the physical expected depth.  Sums in fp32 per lane, then a wave reduction: deterministic, no atomics.
 *                   Disparity is not formed: a caller derives it from D and A.
 * Every other argument, the workspace (size and layout: nerf_hip_ws_bytes, NERF_HIP_WEIGHTS_UNCHANGED reuse) and C_coarse / C_fine / the
 * status word are exactly nerf_hip_forward's, bit for bit, in every inference mode.  NERF_HIP_SAVE_FOR_BACKWARD or a null maps ->
 * NERF_HIP_ERR_ARG before any device work.  (Small bf16-MLP batches run the separate launches instead of the one-launch ray-pair kernel.)
 */
int nerf_hip_forward_maps(const float* const* weights24, const int64_t* row, const int64_t* col,
                          const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                          int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine, float* maps,
                          void* ws, size_t ws_bytes, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Quantile depths: where along the ray the weight sits, beside the maps' mean D / A.
 *
 * QD. THE QUANTILE RULE, for one pass of one ray: samples t_0 .. t_{N-1} in the order the composite visits them, with the composite's own
 *    fp32 weights w_i.  Coarse pass: t_c with w_c.  Fine pass: the SORTED depth channel t_s with the w of C_fine -- without
 *    NERF_HIP_CORRECTED it inherits quirk Q1 exactly as D_f does (the five channels are sorted independently), with NERF_HIP_CORRECTED it
 *    is physical.  All arithmetic is fp64 on the fp32 inputs widened exactly; every operation is rounded on its own; every comparison is
 *    false on NaN.
 *       W_i   = the inclusive prefix sum of w, formed as the kernels form the cdf: inside each chunk of 64 samples (the last one padded
 *               with zeros) the Hillis-Steele steps d = 1, 2, 4, .. 32 (v_l += v_{l-d} for l >= d, all l at once), then + carry, the
 *               carry being element 63 of the chunk before (0 for the first).  This order is part of the rule.
 *       W     = W_{N-1};   theta = double(q) * W                           for a quantile q (fp32, 0 < q < 1)
 *       k     = the first i with W_i >= theta;   E = W_{k-1} (0 for k = 0)
 *       f     = (theta - E) / double(w_k);  f = f > 0 ? f : 0;  f = f < 1 ? f : 1
 *       t_nxt = t_{k+1} if k + 1 < N, else t_k                             (the last sample is never extrapolated: last_delta may be 1e10)
 *       Q(q)  = fp32(double(t_k) + f * (double(t_nxt) - double(t_k)))
 *    If no such k exists (W is NaN, or no W_i reaches theta), or w_k is not > 0 (W = 0: k = 0 with w_0 = 0), Q(q) = t_{N-1}: the pass's
 *    opacity A already tells the caller that the ray hit nothing.
 *    Q(q) is the q-quantile of the ray's normalised hit distribution -- the distribution whose mean is D / A --, linearly interpolated
 *    inside the sample interval.  Q(0.5) is the median depth.  Not differentiable; inference only.
 *
 * nerf_hip_forward_quantiles: the arguments of nerf_hip_forward_maps, then
 *   q       HOST [nq] f32: the quantiles, each strictly inside (0, 1); they travel in the kernels' arguments
 *   nq      1 .. NERF_HIP_MAX_QUANTILES
 *   qdepth  [B,2,nq] f32 out, device: row 0 = Q_c(q_j) of the coarse pass, row 1 = Q_f(q_j) of the fine pass
 * It runs in every inference mode nerf_hip_forward_maps runs in; C_coarse, C_fine, maps, the status word and the workspace are that
 * call's, bit for bit (k_coarse_qmaps / k_merge_qmaps: the maps kernels with one more loop per ray; small bf16-MLP batches take the
 * separate launches, as a maps call does).  NERF_HIP_ERR_ARG before any device work: nq < 1 or nq > NERF_HIP_MAX_QUANTILES, a NULL q or
 * qdepth, a q that is NaN or not strictly inside (0, 1), a NULL maps, NERF_HIP_SAVE_FOR_BACKWARD.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_MAX_QUANTILES 4

int nerf_hip_forward_quantiles(const float* const* weights24, const int64_t* row, const int64_t* col,
                               const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                               int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine, float* maps,
                               void* ws, size_t ws_bytes, int flags, void* stream,
                               const float* q /* HOST [nq] */, int nq, float* qdepth /* device [B][2][nq]: row 0 coarse, row 1 fine */);

/*
 * nerf_hip_forward_maps for TRAINING (the maps are differentiable through nerf_hip_backward_maps).  The arguments of
 * nerf_hip_forward_maps; NERF_HIP_SAVE_FOR_BACKWARD is required (without it, or with a null maps: NERF_HIP_ERR_ARG before any device
 * work).  Every training mode (exact fp32, NERF_HIP_FORCE_TILE_KERNEL, split-fp32, bf16 MLP, NERF_HIP_CORRECTED); C_coarse, C_fine, the
 * status word and the workspace's saves are those of nerf_hip_forward with the same flags.  The per-ray stages always run as separate
 * launches: at the small bf16-MLP sizes where nerf_hip_forward fuses them into the field launches, this call does not.
 */
int nerf_hip_forward_maps_train(const float* const* weights24, const int64_t* row, const int64_t* col,
                                const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                                int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine, float* maps,
                                void* ws, size_t ws_bytes, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Distortion loss: a trainable measure of how far a ray's weight is spread, the regulariser of
 * mip-NeRF 360 against floaters.  Beside rule QD, which shows the same spread at inference time.
 *
 * DL. THE DISTORTION RULE, for one pass of one ray: samples t_0 .. t_{N-1} in the order the composite visits them (non-decreasing), with
 *    the composite's own fp32 weights w_i.  Coarse pass: t_c with w_c.  Fine pass: the SORTED depth channel t_s with the w of C_fine --
 *    without NERF_HIP_CORRECTED it inherits quirk Q1 exactly as D_f and the quantiles do.  All arithmetic is fp64 on the fp32 inputs
 *    widened exactly.
 *       m_i = (t_i + t_{i+1}) / 2   for i < N-1        m_{N-1} = t_{N-1}
 *       d_i = t_{i+1} - t_i         for i < N-1        d_{N-1} = 0       (the last interval is never extrapolated: last_delta may be 1e10)
 *       r   = 1 / (far - near)      of the ray         (far > near is the caller's guarantee, as everywhere)
 *       We_i = sum_{j<i} w_j        Se_i = sum_{j<i} w_j m_j             (exclusive prefixes, index order)
 *       W = sum w                   S = sum w m
 *       P_i = m_i We_i - Se_i
 *       R_i = (S - Se_i - w_i m_i) - m_i (W - We_i - w_i)
 *       L   = r [ 2 sum_i w_i P_i + 1/3 sum_i w_i^2 d_i ]                stored as fp32
 *    L = r (sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i) because m is non-decreasing; at ties the sign of m_i - m_j is that of
 *    i - j, which fixes the subgradient.  L is dimensionless (depths in units of the ray's [near, far]).  Its gradients, also fp64:
 *       dL/dw_i = r [ 2 (P_i + R_i) + 2/3 w_i d_i ]
 *       a_i     = 2 w_i (We_i - (W - We_i - w_i))                        (= d/dm_i of the double sum)
 *       dL/dt_k = r [ (k < N-1 ? a_k / 2 - w_k^2 / 3 : a_k) + (k >= 1 ? a_{k-1} / 2 + w_{k-1}^2 / 3 : 0) ]
 *    With the upstream g = d loss / dL of the ray and pass, the backward adds fp32(double(g) dL/dw_k) to d w_k and fp32(double(g) dL/dt_k)
 *    to d t_s,k, each as a separate fp32 addition behind the maps terms of nerf_hip_backward_maps.  The depth gradient takes the route of
 *    the maps' gD_f w_k: through the t channel's own permutation to d t_fine; a coarse origin drops it; NERF_HIP_CORRECTED drops it with
 *    the rest; t_c carries no gradient, so the coarse pass contributes through d w_c,i alone.
 *    (The kernels take W and S per lane and then across the wave, and the prefixes by wave scans: fp64 sums whose order differs from the
 *    index order by rounding in the 16th digit, far below the one fp32 rounding of each result.)
 *
 * nerf_hip_forward_distortion_train: the arguments of nerf_hip_forward_maps_train, then
 *   dist    [B,2] f32 out, device: (L_c, L_f) per ray
 * NERF_HIP_SAVE_FOR_BACKWARD, maps and dist are required (else NERF_HIP_ERR_ARG before any device work).  Every training mode; C_coarse,
 * C_fine, maps, the status word and the workspace's saves are nerf_hip_forward_maps_train's, bit for bit (k_coarse_dmaps / k_merge_dmaps:
 * the training maps kernels with one more accumulation in the composite loop).  The workspace is that call's: nothing per sample is saved.
 *
 * nerf_hip_backward_distortion: the arguments of nerf_hip_backward_maps, then
 *   ddist   [B,2] f32, device, not NULL: g = (d loss / dL_c, d loss / dL_f) per ray
 * Valid after any training forward on the workspace (near and far come from the ray records every forward keeps).  With ddist = 0 every
 * gradient equals nerf_hip_backward_maps's.  The per-ray stages run as separate launches (k_merge_bwd_dist / k_coarse_bwd_dist), which
 * recompute W, S and the prefixes from the weights they recompute anyway.  Null dmaps or ddist -> NERF_HIP_ERR_ARG before any device work.
 * ------------------------------------------------------------------------------------------- */
int nerf_hip_forward_distortion_train(const float* const* weights24, const int64_t* row, const int64_t* col,
                                      const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                                      int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine, float* maps,
                                      void* ws, size_t ws_bytes, int flags, void* stream, float* dist /* device [B][2] */);
int nerf_hip_backward_distortion(const float* const* weights24, const float* dC_coarse, const float* dC_fine, const float* dmaps,
                                 const float* ray0_near_far, int B, int Nc, int Nf, float last_delta,
                                 float* const* dweights24, void* ws, size_t ws_bytes, int flags, void* stream,
                                 void* early_event, const float* ddist /* device [B][2] */);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Per-ray normal maps: the field's normals composited with the ray's own weights, beside the
 * maps' D / A and rule QD's quantile depths.
 *
 * NM. THE NORMAL RULE, for one pass of one ray: samples t_0 .. t_{N-1} in the order the composite visits them, with the composite's own
 *    fp32 weights w_i.  Coarse pass: t_c with w_c, N = Nc.  Fine pass: the SORTED depth channel t_s (channel 0 of the sorted bundle) with
 *    the w of C_fine, N = Nc + Nf -- without NERF_HIP_CORRECTED it inherits quirk Q1 exactly as D_f and the quantiles do, with
 *    NERF_HIP_CORRECTED it is physical.
 *       p_i = the world point of the ray at depth t_i as the forward forms it: v = d_cam * t_i, p = ((R0 v0 + R1 v1) + R2 v2) + o, every
 *             product and sum rounded separately -- the forward's own points, bit for bit
 *       g_i = what nerf_hip_query_grad(points = p_i, dirs = NULL, dsigma = NULL) stores in dpoints, bit for bit: the exact-fp32 gradient
 *             of sigma under the train step's convention, whatever NERF_HIP_BF16_MLP / NERF_HIP_SPLIT_MLP say (only the w_i come from
 *             the mode's own forward)
 *       n_i = the field normal of g_i, the marching-cubes kernel's rule, in fp32 with every operation rounded:
 *             len = sqrt((g0 g0 + g1 g1) + g2 g2);  n_i = -g_i / len,  or (0, 0, 0) where len is 0 or not finite
 *       N_c = fp32( sum_i double(w_i) * double(n_i,c) )    for c = 0 .. 2; a sample whose w_i is 0 or NaN adds nothing (w_i > 0 or
 *             w_i < 0 is required, and comparisons are false on NaN)
 *    The sum is fp64, deterministic and free of atomics (per-lane partial sums, then a wave reduction, as the colour sums); its ORDER is not
 *    part of the rule: a reordering moves an fp64 sum of at most 2,048 terms of magnitude <= |w_i| by less than 2048 * 2^-53 * sum |w_i|.
 *    N is in the world frame and NOT normalised: |N| <= A, and |N| / A says how far the normals along the ray agree.  Not differentiable;
 *    inference only.
 *
 * nerf_hip_normals_ws_bytes / nerf_hip_normals_ws_offset: the SIDE workspace of nerf_hip_forward_normals for these sizes, and the byte
 * offset of a named buffer inside it (introspection for tests): "bundle" [B,Nc+Nf,5] and "w_m" [B,Nc+Nf] of the fine pass (24 bytes per
 * merged sample: the only part that grows with B), then a sigma-only gradient query's workspace ("packed" "fold" "save" "masks" "spre") and
 * "sigma" "points" [.,3] "grad" [.,3] of ONE chunk of samples.  A chunk is floor(131072 / N) whole rays of the pass (N = Nc or Nc + Nf);
 * after a call, "points" and "grad" hold the last chunk of the last pass that ran (coarse first, then fine).  The main workspace
 * (nerf_hip_ws_bytes, nerf_hip_ws_offset) is unchanged by this feature.  Sizes as nerf_hip_ws_bytes checks them.
 *
 * nerf_hip_forward_normals: the arguments of nerf_hip_forward_maps, then
 *   passes     bit 0 = the coarse pass, bit 1 = the fine pass: 1, 2 or 3
 *   normals    [B,2,3] f32 out, device: row 0 = N of the coarse pass, row 1 = N of the fine pass; a row that is not asked for is untouched
 *   nws        side workspace of >= nerf_hip_normals_ws_bytes(B,Nc,Nf) bytes, 256-byte aligned
 * It runs in every inference mode nerf_hip_forward_maps runs in; C_coarse, C_fine, maps, the status word and the main workspace are that
 * call's, bit for bit (the same launches: the merge kernel also stores its sorted bundle and weights, to nws).  Behind them, per requested
 * pass and chunk: k_sample_points, the two launches of the gradient query, k_normal_composite; the gradient query's weight image is packed
 * once per call.  Enqueue-only on the caller's stream.  NERF_HIP_ERR_ARG before any device work: NERF_HIP_SAVE_FOR_BACKWARD, passes
 * outside 1..3, a NULL maps, normals or nws, nws too small or not 256-byte aligned; and whatever nerf_hip_forward_maps refuses.
 *
 * nerf_hip_normal_composite: the stage entry, the k_normal_composite launch on its own.  w [B,N], g [B,N,3] (sigma gradients), device;
 * out[b * out_stride + c] receives N_c of ray b (out_stride >= 3; nothing else is written).  1 <= N <= 2048.  B = 0 succeeds and launches
 * nothing.
 * ------------------------------------------------------------------------------------------- */
int nerf_hip_normals_ws_bytes(int B, int Nc, int Nf, size_t* bytes);
int nerf_hip_normals_ws_offset(int B, int Nc, int Nf, const char* name, size_t* offset);
int nerf_hip_forward_normals(const float* const* weights24, const int64_t* row, const int64_t* col,
                             const float* poses_bound, const float* K_inv9, const float* ray0_near_far,
                             int B, int Nc, int Nf, float last_delta, float* C_coarse, float* C_fine, float* maps,
                             void* ws, size_t ws_bytes, int flags, void* stream,
                             int passes, float* normals /* device [B][2][3] */, void* nws, size_t nws_bytes);
int nerf_hip_normal_composite(const float* w, const float* g, int B, int N, float* out, int out_stride, void* stream);

/*
 * Backward of nerf_hip_forward (autograd through nerf.py:286-323, called at nerf.py:473).
 * Needs the workspace of a forward run with NERF_HIP_SAVE_FOR_BACKWARD and the same sizes/inputs.
 *   dC_coarse, dC_fine [B,3] f32   upstream gradients
 *   ray0_near_far      as in nerf_hip_forward (must match the forward call)
 *   dweights24         HOST array of 24 DEVICE pointers, same shapes as weights24 (16-byte aligned);
 *                      OVERWRITTEN with the gradients of this batch (sum over rays, no averaging)
 */
int nerf_hip_backward(const float* const* weights24, const float* dC_coarse, const float* dC_fine,
                      const float* ray0_near_far, int B, int Nc, int Nf, float last_delta,
                      float* const* dweights24, void* ws, size_t ws_bytes, int flags, void* stream);

/*
 * nerf_hip_backward for a data-parallel trainer that overlaps its gradient all-reduce with the rest of the backward pass
 * (the collective sits where the reference has loss.backward(); optimizer.step(), nerf.py:473-474): the gradients of
 * point_layer[0..7] (tensors 0..15 of dweights24: 491,520 of the 593,924 parameters) are FINAL at the point where
 * `early_event` (a hipEvent_t created by the caller) is recorded on `stream`; the remaining weight-gradient products (sigma
 * head, point_info, dir_info, colour head: tensors 16..23) follow it.  A caller puts the all-reduce of tensors 0..15 on another
 * stream behind that event and the all-reduce of tensors 16..23 behind the call.  early_event == NULL: nerf_hip_backward.
 */
int nerf_hip_backward_overlap(const float* const* weights24, const float* dC_coarse, const float* dC_fine,
                              const float* ray0_near_far, int B, int Nc, int Nf, float last_delta,
                              float* const* dweights24, void* ws, size_t ws_bytes, int flags, void* stream,
                              void* early_event);

/*
 * nerf_hip_backward_overlap with the upstream gradient of the maps as well.
 *   dmaps   [B,4] f32, device, not NULL: g = (gD_c, gA_c, gD_f, gA_f) per ray, the gradient of the loss with respect to
 *           (D_c, A_c, D_f, A_f) of nerf_hip_forward_maps.  Its terms, added behind the colour terms as separate additions:
 *             d w_c,i += gD_c t_c,i + gA_c        (every coarse sample i; t_c carries no gradient)
 *             d w_k   += gD_f t_s,k + gA_f        (sorted position k of the merged samples)
 *             d t_s,k += gD_f w_k                 (through the t channel's own permutation to d t_fine; a coarse origin drops it;
 *                                                  NERF_HIP_CORRECTED detaches t_fine and drops it with the rest)
 *           With dmaps = 0 every gradient equals nerf_hip_backward's bit for bit.
 * Valid after either training forward (nerf_hip_forward or nerf_hip_forward_maps_train with NERF_HIP_SAVE_FOR_BACKWARD) on the
 * workspace.  The per-ray stages always run as separate launches (never fused into the bf16-MLP chain launches).  Null dmaps ->
 * NERF_HIP_ERR_ARG before any device work.
 */
int nerf_hip_backward_maps(const float* const* weights24, const float* dC_coarse, const float* dC_fine, const float* dmaps,
                           const float* ray0_near_far, int B, int Nc, int Nf, float last_delta,
                           float* const* dweights24, void* ws, size_t ws_bytes, int flags, void* stream,
                           void* early_event);

/*
 * One train step's device work in ONE call: nerf_hip_forward (with NERF_HIP_SAVE_FOR_BACKWARD), nerf_hip_ray_loss and
 * nerf_hip_backward_overlap enqueued back to back -- the three calls the reference's loop makes at nerf.py:470-473
 * (`model(...)`, `ray_loss`, `loss.backward()`), without the caller's interpreter between them (at a 400 / 512-ray batch the gaps
 * between three separate calls are 3 % of the step).  Same kernels, same results as the three calls.
 *   C_true            [B,3] f32   the batch's pixel colours
 *   C_coarse, C_fine  [B,3] f32 out (may not be NULL)
 *   loss              [1] f32 out
 *   dweights24, early_event   as in nerf_hip_backward_overlap
 *   flags             NERF_HIP_SAVE_FOR_BACKWARD is implied; ws sized for the flags INCLUDING it
 */
int nerf_hip_train_step(const float* const* weights24, const int64_t* row, const int64_t* col, const float* poses_bound,
                        const float* K_inv9, const float* ray0_near_far, const float* C_true, int B, int Nc, int Nf, float last_delta,
                        float* C_coarse, float* C_fine, float* loss, float* const* dweights24, void* ws, size_t ws_bytes, int flags,
                        void* stream, void* early_event);

/* ray_loss (nerf.py:325-331) and its gradient: loss[1] = sum (C_c-C*)^2 + sum (C_f-C*)^2,
 * dC_c = 2 (C_c - C*), dC_f = 2 (C_f - C*).  dC_* may be NULL. */
int nerf_hip_ray_loss(const float* C_coarse, const float* C_fine, const float* C_true, int B,
                      float* loss, float* dC_coarse, float* dC_fine, void* stream);

/* Copies the status word of the last forward on this workspace to the host (synchronises `stream`). */
int nerf_hip_read_status(const void* ws, size_t ws_bytes, uint32_t* status, void* stream);

/* The STICKY status word: every forward ORs the bits of its status word into it as well and no library call clears it, so a train loop
 * that looks at the status only every k-th iteration (one host sync) still sees a condition any iteration in between met -- the reference
 * checks its resampling indices in EVERY forward (nerf.py:251-253).  The caller zeroes the first 256 bytes of a fresh workspace once
 * (the library allocates nothing and cannot know a fresh workspace from a used one); clear != 0 resets the word after reading it.
 * Synchronises `stream`. */
int nerf_hip_read_status_sticky(void* ws, size_t ws_bytes, uint32_t* status, int clear, void* stream);

/*
 * Optional per-kernel timing with HIP events recorded on the caller's stream around every kernel the
 * library launches (used by bench.py for the roofline figure; off by default).  ONE session per process:
 * begin() creates 2*max_launches events; end() waits for them, adds each launch's elapsed ms to
 * ms_sum[kernel id] / count[kernel id] (arrays of n_kernels) and destroys the events.  While a session is open,
 * forward/backward calls from any thread or stream are recorded (slots are handed out under a mutex); begin() and
 * end() themselves must be called from one thread, and end() only after every call of the session has returned.
 */
enum {
  NERF_HIP_K_PACK = 0, NERF_HIP_K_RAYS = 1, NERF_HIP_K_FIELD_COARSE = 2, NERF_HIP_K_COARSE = 3,
  NERF_HIP_K_FIELD_FINE = 4, NERF_HIP_K_MERGE = 5,
  NERF_HIP_K_BWD_MERGE = 6, NERF_HIP_K_BWD_FIELD_FINE = 7, NERF_HIP_K_BWD_COARSE = 8,
  NERF_HIP_K_BWD_FIELD_COARSE = 9, NERF_HIP_K_BWD_DW = 10,
  NERF_HIP_K_RENDER_PAIR = 11, /* small bf16-MLP inference batches: both field passes and both composites of a ray pair in ONE launch */
  NERF_HIP_K_COUNT = 12
};
int nerf_hip_profile_begin(int max_launches);
int nerf_hip_profile_end(double* ms_sum, int* count, int n_kernels);

/* ---------------------------------------------------------------------------------------------
 * Rows f1/f2 of the scope table: what the caller does around the hot path once the renderer is fast.
 * ------------------------------------------------------------------------------------------- */

/* Fused Adam update of all 24 parameter tensors in one launch: torch.optim.Adam semantics as constructed at
 * nerf.py:425 (no weight decay, no amsgrad).  exp_avg / exp_avg_sq: flat [593,924] f32 moment buffers in
 * parameters() order (caller allocated, zero before step 1).  step = 1, 2, ...; lr = this step's learning rate
 * (the LambdaLR of nerf.py:426 is evaluated by the caller). */
int nerf_hip_adam_step(float* const* params24, const float* const* grads24, float* exp_avg, float* exp_avg_sq,
                       int step, float lr, float beta1, float beta2, float eps, void* stream);

/* GPU-resident replacement of NeRFDataset.__getitem__ + DataLoader collation (loader.py:119-133): for B flat pixel
 * indices into pixels[n_pic*H*W][3] (loader.py:88) and poses17[n_pic][17] (f32) writes row, col, pic [B] i64,
 * pix_val [B,3] and poses_bound [B,17] f32 -- the tuple nerf.py:458 iterates over, already on the device. */
int nerf_hip_gather_rays(const int64_t* index, const float* pixels, const float* poses17, int B, int H, int W,
                         int64_t* row, int64_t* col, int64_t* pic, float* pix_val, float* poses_bound, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The trained field at explicit points: density grids (occupancy, marching cubes, empty-space culling) and colour probes.
 * Same register-resident exact-fp32 kernel as the forward's field passes, fed with points instead of ray samples: results are
 * bit-identical to the forward's at the same point and direction.  The model's flags do not apply (no bf16 / split-fp32 variant).
 * Enqueue-only; each call packs its own weight image into `ws` (a query workspace, never a forward's).  Accurate for |p_c| <= 320:
 * the encoding's phase reduction holds its error below 1e-10 rad up to 2^20 rad, and the largest point frequency is 1024 pi.
 * Beyond that nothing is checked or refused, and the results are not those of sinf / cosf: sin and cos of a phase stay within 2^-23 of
 * the true values below 2^29 rad (|p_c| < 1.6e5), then the error doubles with every doubling of the phase (4e-5 at 2^39 rad, 4e-2 at
 * 2^49) while the values stay inside [-1, 1]; from 2^54 rad (|p_c| >= 5.6e12) they leave [-1, 1] and grow without bound (1e2 at 2^55
 * rad, 1e12 at 2^59; the first +-inf / NaN at 2^70 rad, nothing finite left by 2^90 rad), and so do the outputs.  Callers keep their points inside the domain.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) for the two calls below: packed weight image, fold and, with_rgb != 0, the direction
 * vectors of one chunk of points.  Independent of M and of the grid size. */
int nerf_hip_query_ws_bytes(int with_rgb, size_t* bytes);

/* Network + Encoder (nerf.py:101-124, 135-167) at explicit points: sigma[M] from points[M,3] (world frame).
 * dirs[M,3] (unit, world frame, NOT renormalised, as Encoder consumes them) and rgb[M,3] are both NULL (sigma only, 7,744 of the
 * 8,256 MFMAs of a sample) or both set (colour too; ws sized with with_rgb = 1).  M == 0 succeeds and launches nothing;
 * M < 0 is refused. */
int nerf_hip_query(const float* const* weights24, const float* points, const float* dirs, int M,
                   float* rgb, float* sigma, void* ws, size_t ws_bytes, void* stream);

/* sigma at the lattice points lo + (i, j, k) * step (HOST lo3 / step3; each coordinate lo_c + (float)i_c * step_c with the
 * product and the sum rounded separately), written C-order [nx][ny][nz] (z fastest).  Every dimension >= 1 and
 * nx * ny * nz < 2^31.  No points buffer is formed: a 512^3 grid needs only its 512 MiB of sigma. */
int nerf_hip_density_grid(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz,
                          float* sigma, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Point gradients of the field: the query above plus the exact-fp32 chain back to the points, for analytic
 * surface normals and autograd through a field query.  Gradient with respect to the points only; the weights are constants here.
 * Gradient convention (the train step's): the encoding's phase is phi = fp32(x_c * f_l), sin and cos are evaluated at that rounded
 * phase, and d(sin phi, cos phi)/d x_c is taken as f_l * (cos phi, -sin phi) -- the rounding of the product is not differentiated.
 * d|s|/ds = sign(s) with sign(0) = 0 at the sigma head, d relu = [pre > 0], as the train step has them.
 * Two kernels per chunk of 131,072 points (4 rounds of one wave per SIMD): the query forward with a compact save (ReLU masks of the 8
 * hidden layers, the sigma pre-activation, gamma_p and, with colour, the dir_info output c: 516 / 1,028 bytes per point) and the dX
 * chain of the train step reading it.  Workspace: 72.8 MB sigma only, 207.0 MB with colour, independent of M.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of nerf_hip_query_grad: packed weight image with the transposed segments, fold, one chunk's
 * save and (with_rgb != 0) its direction vectors.  Independent of M. */
int nerf_hip_query_grad_ws_bytes(int with_rgb, size_t* bytes);

/* sigma[M] (and rgb[M,3]) exactly as nerf_hip_query computes them at the same points, bit for bit, and the vector-Jacobian product
 * dpoints[m] = dsigma[m] * d sigma_m / d p_m + sum_c drgb[m][c] * d rgb_m[c] / d p_m  (STORED, [M,3]).
 * dsigma [M] or NULL (= every entry 1: dpoints is then the gradient of sigma).  dirs and rgb are both NULL (sigma only) or both set
 * (ws sized with with_rgb = 1); drgb [M,3] only with dirs, and may be NULL there (no colour term: the sigma-only chain runs).
 * Refused before any device work: M < 0, drgb without dirs, dirs without rgb or rgb without dirs, and with M > 0 a NULL points / sigma /
 * dpoints or a workspace that is NULL, too small or not 256-byte aligned.  M == 0 succeeds and launches nothing.  Enqueue-only. */
int nerf_hip_query_grad(const float* const* weights24, const float* points, const float* dirs, int M,
                        const float* dsigma, const float* drgb, float* rgb, float* sigma, float* dpoints,
                        void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image metrics of rendered frames: per view the MSE and the SSIM of pred against gt, both
 * [n][H][W][3] fp32, row-major (the layout of NeRFRunner.display()), device-resident.  Data range 1, no clipping.
 *   MSE_v  = sum over the H * W * 3 values of (pred - gt)^2 / (H * W * 3);  PSNR = -10 log10(MSE) is the caller's (+inf at 0).
 *   SSIM_v (Wang et al. 2004 as mip-NeRF's compute_ssim reports it), per channel c of x = pred, y = gt:
 *     g[k] = exp(-((k - 5) / 1.5)^2 / 2) / sum_j exp(-((j - 5) / 1.5)^2 / 2),  k = 0..10  (sigma 1.5, sum 1)
 *     f(z)[i][j] = sum_a g[a] sum_b g[b] z[i + a][j + b]  (horizontal pass first, then vertical; VALID: 0 <= i < H - 10,
 *                  0 <= j < W - 10, no padding)
 *     mu_x = f(x), mu_y = f(y), s_xx = max(f(x^2) - mu_x^2, 0), s_yy = max(f(y^2) - mu_y^2, 0),
 *     s_xy = sign(t) min(sqrt(s_xx s_yy), |t|) with t = f(xy) - mu_x mu_y,   C1 = 0.01^2, C2 = 0.03^2
 *     map = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2))
 *   SSIM_v = the mean of map over the 3 channels and the (H - 10) x (W - 10) valid pixels.
 * Every product, filter tap and sum runs in fp64.  No atomics: the per-tile partial sums go to `ws` and a fixed-order pass reduces
 * them, so repeated calls are bit-identical whatever `ws` held.  NaN / inf in a view's inputs reaches that view's results (the clamps
 * let NaN through).  One workgroup per (view, tile of 16 x 32 outputs) and one per view.  Enqueue-only.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of nerf_hip_image_metrics for n views of H x W: 16 bytes per (view, tile). */
int nerf_hip_metrics_ws_bytes(int n, int H, int W, size_t* bytes);

/* mse[n], ssim[n] (fp64, device) as defined above.  Refused before any device work: n < 0, H < 11 or W < 11 (the window),
 * H * W * 3 >= 2^31, and with n > 0 a NULL pred / gt / mse / ssim, or a workspace that is NULL, not 256-byte aligned or smaller
 * than nerf_hip_metrics_ws_bytes(n, H, W).  n == 0 succeeds and launches nothing. */
int nerf_hip_image_metrics(const float* pred, const float* gt, int n, int H, int W, double* mse, double* ssim,
                           void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Marching cubes over a density grid: an indexed triangle mesh of the isosurface sigma == level.
 * sigma is C-order fp32 [nx][ny][nz] (z fastest, as nerf_hip_density_grid writes it); lattice point (i, j, k) sits at
 * lo + (i, j, k) * step (each coordinate one fp32 product and one fp32 sum).  Inside means sigma > level; NaN is outside.
 * - A vertex on every lattice edge (to the +x, +y or +z neighbour) whose ends differ in insideness, at p_a + t * (p_b - p_a) with
 *   t = (level - s_a) / (s_b - s_a) (0.5 where that is not finite), ordered by the edge's lower endpoint's linear index
 *   (i * ny + j) * nz + k, then by axis x < y < z.  Its normal is -g / |g| ((0, 0, 0) where |g| is 0 or not finite), g the sigma
 *   gradient (central differences, one-sided at the grid's faces) interpolated with the same t.
 * - Faces (three int32 vertex indices) from the classic table (csrc/mc_tables.h), ordered by cell linear index (C order over the
 *   (nx-1)(ny-1)(nz-1) cells), then by the table's order; counter-clockwise seen from outside (cross(v1 - v0, v2 - v0) points toward
 *   decreasing sigma).
 * - Any dimension < 2: no cells, the empty mesh.  Every dimension >= 1, nx * ny * nz < 2^31, level finite; emit also needs every
 *   step > 0 (and finite) along a dimension of more than one point.
 * Enqueue-only: neither call synchronises with the host.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of a mesh over an nx x ny x nz grid: 4 bytes per lattice point and 24 per 4096 points. */
int nerf_hip_mesh_ws_bytes(int nx, int ny, int nz, size_t* bytes);

/* Counts the mesh: writes counts[0] = V and counts[1] = F (DEVICE int64[2]) and leaves the vertex offsets in ws for the emit. */
int nerf_hip_mesh_count(const float* sigma, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes, int64_t* counts,
                        void* stream);

/* Writes verts[V][3], normals[V][3] (fp32) and faces[F][3] (int32).  Must follow a nerf_hip_mesh_count on the same workspace, grid and
 * level (stream order).  max_v / max_f are the caller's capacities in rows: the kernels clamp every store to them, so a wrong capacity
 * or a mismatched count/emit pair gives wrong or partial output, never a write outside the buffers.  Face indices are int32: a mesh
 * with V >= 2^31 cannot be indexed (the caller refuses it after the count).  lo3 / step3 are HOST arrays. */
int nerf_hip_mesh_emit(const float* sigma, int nx, int ny, int nz, const float* lo3, const float* step3, float level, const void* ws,
                       size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t max_v, int64_t max_f, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Masked marching cubes: the two calls above with one more input, valid[nx][ny][nz] (uint8,
 * C order as sigma; non-zero = valid) -- e.g. the lattice points a TSDF fusion observed.
 *
 * M. THE MASK RULE.  A cell is LIVE iff all eight of its corners are valid.  Triangles come from live cells only; a cell's table row is
 *    computed from sigma > level at its eight corners exactly as above, whatever the mask says.  A lattice edge carries a vertex iff its
 *    ends differ in insideness (as above) AND at least one of the up to four cells that contain the edge is live.  Every sign-changing
 *    edge of a cell is used by one of that cell's triangles, so no vertex is unreferenced.
 *    Vertices and faces keep the order above (by the edge's lower endpoint, then axis; by cell, then the table's order).  The masked
 *    mesh is therefore the unmasked mesh of the same grid with the faces of the cells that are not live removed and the surviving
 *    vertices and faces renumbered in their order: what nerf_hip_mesh_select_faces_* produce from the unmasked mesh and the keep flags
 *    "this face's cell is live", bit for bit in verts, normals and faces.
 *    Normals stay the grid's central differences interpolated along the edge.  They read sigma at invalid points too -- the caller's
 *    fill value enters them near the mask's edge -- and are bit-identical to the unmasked normals of the same vertices.
 *
 * The workspace, its size (nerf_hip_mesh_ws_bytes), the capacities' clamping and every refusal are those of the unmasked calls; a NULL
 * valid is refused as well.  The mask is read directly: no pre-pass.  An all-valid mask gives the unmasked mesh.
 * ------------------------------------------------------------------------------------------- */
int nerf_hip_mesh_count_masked(const float* sigma, const uint8_t* valid, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes,
                               int64_t* counts, void* stream);

/* Must follow a nerf_hip_mesh_count_masked on the same workspace, grid, mask and level. */
int nerf_hip_mesh_emit_masked(const float* sigma, const uint8_t* valid, int nx, int ny, int nz, const float* lo3, const float* step3,
                              float level, const void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t max_v,
                              int64_t max_f, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Narrow-band density grid: the dense grid of nerf_hip_density_grid with the field evaluated only in a band
 * of blocks around the level set; everywhere else the array holds a fill value of the right class.  For marching cubes at the same
 * level: a surface crosses O(n^2) of the n^3 cells.  Lattice, point positions and the inside rule (sigma > level, NaN outside) are
 * nerf_hip_density_grid's and the mesh calls'; every evaluated value is nerf_hip_density_grid's, bit for bit.
 *   Blocks: per axis a, nb_a = ceil(n_a / block); block b owns the points [b * block, min((b + 1) * block, n_a)) and has its corner
 *   planes at the point indices min(b * block, n_a - 1) and min((b + 1) * block, n_a - 1).  A cell or a block is MIXED when its 8
 *   corners are not all of one class.
 *   begin: (1) the field at the corner lattice, each point once, stored at its own position; (2) seeds S = the blocks whose 8 corner
 *   samples are mixed, active set A = empty; (3) every lattice point takes the value of its block's lowest point; then the first list.
 *   grow (one round): the field at every point owned by the listed blocks; S = the blocks of A with an in-grid 26-neighbour outside A
 *   that own a corner point of a mixed cell of the array as it now stands; then the next list.
 *   The list: new = (S grown by one block in the 26-neighbourhood, clipped to the grid) minus A, in ascending block order
 *   (bx * nb_y + by) * nb_z + bz; A |= new; counts[0] = the list's length, counts[1] = the lattice points those blocks own.
 * The caller reads counts after begin and after every grow (one 16-byte read; this is the only synchronisation), and calls grow with
 * n_blocks = counts[0] until that is 0.  At that point every mixed cell of sigma has its 8 corners and their +-1 neighbours exact (this
 * needs block >= 2), so marching cubes over it gives the dense grid's mesh restricted to the cells the band reached -- vertices, faces
 * and normals bit for bit the dense mesh whenever every connected piece of the surface is mixed in some block's corner samples or is
 * connected to a piece that is.
 * WHAT IT CANNOT SEE: a piece of the surface that fits between the corner samples -- an island smaller than a block, a whole object
 * inside one block -- is never found and is missing from the mesh, silently.  Lower `block` where that matters; the dense calls stay.
 * Exact fp32 (the point queries' kernel in two more index forms).  Enqueue-only.  Refused before any device work: a dimension < 1,
 * nx * ny * nz >= 2^31, block < 2, more than 2^25 blocks, a level that is not finite, a NULL sigma / lo3 / step3 / counts / weights, a
 * workspace that is NULL, not 256-byte aligned or too small, counts not 8-byte aligned, n_blocks < 0 or above the number of blocks.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of the two calls below: nerf_hip_query_ws_bytes(0) plus 10 bytes per block and 16 per 256
 * blocks.  Nothing per lattice point. */
int nerf_hip_band_ws_bytes(int nx, int ny, int nz, int block, size_t* bytes);

/* Packs the weights, then steps (1)-(3) and the first list.  sigma [nx][ny][nz] (device) is written everywhere; counts is DEVICE
 * int64[2]; lo3 / step3 are HOST arrays as for nerf_hip_density_grid. */
int nerf_hip_band_begin(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, int block,
                        float level, float* sigma, void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* One round on the same arguments, workspace and weights as the begin before it (stream order; the packed image is reused): evaluates
 * the n_blocks listed blocks -- n_blocks as read from counts[0]; the kernel also bounds itself by the device's count, so a wrong value
 * leaves blocks unevaluated, never a write outside sigma -- then re-derives S and leaves the next list and its counts. */
int nerf_hip_band_grow(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, int block,
                       float level, int64_t n_blocks, float* sigma, void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components of an indexed triangle mesh: labels, per-component counts and boxes, and the
 * compaction that drops components -- the floaters of a density field's isosurface.  Any indexed mesh, not only marching cubes':
 * faces[F][3] int32 over V vertices, V, F < 2^31.
 * - Two vertices are connected when some face contains both (two triangles that share one vertex are one component); a vertex in no
 *   face is a component of its own with 0 faces.
 * - A face with an index outside [0, V) takes no part: it connects nothing, its face_comp is -1, no count includes it, the compaction
 *   drops it, and its indices are never used as addresses.
 * - Component ids are 0 .. C-1 in ascending order of the component's smallest vertex index.  vert_comp[V] is each vertex's id,
 *   face_comp[F] the id of the face's first vertex.
 * - n_verts[C], n_faces[C] (int32): the component's vertices and (participating) faces.  bbox_lo[C][3], bbox_hi[C][3] (fp32): per
 *   coordinate the minimum and maximum over the component's vertices; a coordinate that is not finite is ignored, -0 counts as +0, and
 *   a component without a finite value along a coordinate has (+inf, -inf) there.
 * Every output is a function of the input alone: integer atomics only (min, max, add -- the boxes go through the floats'
 * order-preserving unsigned images), nothing is placed by an atomic, identical bits from run to run.
 *
 * Labelling: min-label hooking in rounds that the HOST drives, as it drives nerf_hip_band_grow.  L[v] = v; a round is (hook) per
 * face, the labels r_k = L[v_k] of its vertices, m = min r_k, atomicMin(&L[r_k], m) for every r_k != m, and a device word `changed`
 * set when any of these lowered a label; then (compress) per vertex, L[v] = the root of v.  The caller reads `changed` (4 bytes: the
 * only synchronisation) after each round and stops at the first round that left it 0: then L is the smallest vertex index of each
 * component.  round = 0, 1, 2, ... in order; round >= 64 is refused with NERF_HIP_ERR_CONVERGE and enqueues nothing (a strip of 65,536
 * vertices in random order needs 11), so a caller's loop always ends, and a labelling that did not converge has no result.
 * Then nerf_hip_mesh_cc_ids (ids by a scan over the roots), nerf_hip_mesh_cc_stats, and nerf_hip_mesh_cc_compact as often as wanted.
 * All calls are enqueue-only on the caller's stream and check every argument on the host before anything is enqueued: V or F outside
 * [0, 2^31), a NULL array that the sizes need, a workspace that is NULL, not 256-byte aligned or too small, count(s) not 8-byte
 * aligned.  Indices read from device arrays (faces, vert_comp, face_comp) are range-checked by the kernels before use and every store is
 * clamped to the caller's capacities: wrong arguments give wrong output, never an access outside the buffers.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of the calls below: 4 bytes per vertex, and 8 per 2048 vertices or faces, whichever are more. */
int nerf_hip_mesh_cc_ws_bytes(int64_t V, int64_t F, size_t* bytes);

/* One labelling round (round 0 also initialises the labels in ws).  changed: DEVICE int32[1], cleared and then set by this round. */
int nerf_hip_mesh_cc_round(const int32_t* faces, int64_t V, int64_t F, int round, void* ws, size_t ws_bytes, int32_t* changed,
                           void* stream);

/* After the round that changed nothing, on the same workspace: vert_comp[V], face_comp[F] (int32) and count[0] = C (DEVICE int64[1]). */
int nerf_hip_mesh_cc_ids(const int32_t* faces, int64_t V, int64_t F, void* ws, size_t ws_bytes, int32_t* vert_comp, int32_t* face_comp,
                         int64_t* count, void* stream);

/* n_verts[max_c], n_faces[max_c] and, with bbox_lo / bbox_hi (both or neither; they need verts[V][3]), the boxes [max_c][3].  max_c is
 * the caller's capacity in components (C, read from count): ids outside [0, max_c) are left out, rows from C on are empty (0, 0, +inf,
 * -inf).  Needs no workspace. */
int nerf_hip_mesh_cc_stats(const float* verts, const int32_t* vert_comp, const int32_t* face_comp, int64_t V, int64_t F, int32_t* n_verts,
                           int32_t* n_faces, float* bbox_lo, float* bbox_hi, int64_t max_c, void* stream);

/* Drops the components c with keep[c] == 0 (keep: DEVICE uint8[C]).  Kept vertices go to out_verts (and normals / rgb [V][3], each may be
 * NULL with its output, to out_normals / out_rgb) at their rank among the kept vertices; kept faces (those that take part and whose
 * component is kept) go to out_faces with their indices renumbered; both keep their order.  counts (DEVICE int64[2]) = V', F'.  max_v /
 * max_f are the outputs' capacities in rows: every store is clamped to them.  The workspace's labels are overwritten. */
int nerf_hip_mesh_cc_compact(const float* verts, const float* normals, const float* rgb, const int32_t* faces, int64_t V, int64_t F,
                             const int32_t* vert_comp, const int32_t* face_comp, const uint8_t* keep, int64_t C, void* ws,
                             size_t ws_bytes, float* out_verts, float* out_normals, float* out_rgb, int32_t* out_faces, int64_t max_v,
                             int64_t max_f, int64_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Simplification of an indexed triangle mesh by uniform vertex clustering (Rossignac-Borrel).  Any indexed
 * mesh: verts[V][3] fp32, optional normals[V][3] fp32, faces[F][3] int32, V, F < 2^31; and a cluster lattice lo[3], cell[3] (fp32,
 * lo finite, each cell > 0 and finite), dims[3] (each in 1 .. 2048, product < 2^31).  Every output is a pure function of the input:
 * identical bits from run to run, no float atomic anywhere.
 * 1. Cell of a vertex.  Per axis u = fp32(fp32(p - lo) / cell) (two fp32 roundings, IEEE division), uc = clamp(u, 0, dims) and
 *    i = min(floor(uc), dims - 1); the linear cell index is in C order, z fastest (the grids' order).  A vertex with a coordinate that
 *    is not finite belongs to no cluster.  Vertices outside the lattice are pulled to its faces by the clamp (their uc as well, so
 *    they pull their cluster's position to the face): this is not an error.
 * 2. Clusters are the occupied cells.
 * 3. Faces.  A face takes no part if it has an index outside [0, V) (never used as an address) or a vertex in no cluster.  A face is
 *    degenerate if two of its vertices share a cell.  Among the remaining faces two are duplicates when their cell triples are equal up
 *    to rotation (the same orientation), and the one with the lowest input index is kept.  The triple in REVERSED orientation is a
 *    different face and both are kept: a thin sheet that collapsed, seen from its two sides.  Kept faces keep their input order and
 *    their own corner order.
 * 4. Vertices out are the clusters that at least one kept face uses, in ascending cell index.  Other clusters are dropped: an island
 *    inside one cell leaves nothing.
 * 5. Position of a cluster.  Per axis S = the sum over its members of rint(double(uc) * 2^20) as int64 (exact, order free; a term is
 *    at most 2^31, so it cannot overflow), n = the member count, and the coordinate is
 *    fp32(double(lo) + double(cell) * (double(S) / (double(n) * 2^20))), every fp64 operation rounded separately.
 * 6. Normal of a cluster (only with normals).  Per axis T = the sum of rint(double(clamp(nrm, -2, 2)) * 2^28) as int64 over the members
 *    whose normal has three finite components (any other member adds nothing); the component is fp32(T / sqrt((Tx Tx + Ty Ty) + Tz Tz))
 *    in fp64, products and sums rounded separately in that order, and (0, 0, 0) where the length is 0.
 * 7. Colours are not carried: the field is there to be asked at the new vertices.
 * 8. counts (DEVICE int64[6]) = V', F', the number of occupied clusters, a flags word (NERF_HIP_SIMPLIFY_TABLE_FULL), the number of
 *    degenerate faces, the number of duplicate faces dropped.
 * Two calls in the shape of nerf_hip_mesh_count / nerf_hip_mesh_emit: count does everything up to counts, the caller reads them (the
 * only synchronisation) and sizes the outputs, emit fills them; emit may be repeated.  Both are enqueue-only on the caller's stream and
 * check every argument on the host before anything is enqueued (NERF_HIP_ERR_ARG: sizes, NULL arrays, a lattice outside the limits
 * above, workspace NULL or not 256-byte aligned, counts not 8-byte aligned; NERF_HIP_ERR_WORKSPACE: workspace too small).  Indices read
 * from device arrays are range-checked by the kernels before use and every store is clamped to max_v / max_f.
 * Duplicates are found through an open-addressing table of face indices (a power of two of at least 2 F slots; above F = 2^30 it is
 * capped at 2^31 slots, still more than F).  A face's probe is bounded by the table size; a probe that found no slot -- which more
 * slots than faces rule out -- sets NERF_HIP_SIMPLIFY_TABLE_FULL in counts[3], and the result must then be discarded.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_SIMPLIFY_TABLE_FULL 1

/* Bytes of workspace (256-byte aligned) of the two calls below: 4 per cell of the cluster lattice; 60 per vertex; per face 4 and 4 per
 * slot of the face table (8 to 16 per face); and 8 per 2048 cells, vertices or faces, whichever are most. */
int nerf_hip_mesh_simplify_ws_bytes(int64_t V, int64_t F, const int* dims3, size_t* bytes);

/* Everything up to counts (DEVICE int64[6], see 8.).  lo3, cell3, dims3: HOST arrays.  normals may be NULL. */
int nerf_hip_mesh_simplify_count(const float* verts, const float* normals, const int32_t* faces, int64_t V, int64_t F, const float* lo3,
                                 const float* cell3, const int* dims3, void* ws, size_t ws_bytes, int64_t* counts, void* stream);

/* After the count call, with the same faces, sizes, lattice and workspace: out_verts[max_v][3], out_normals[max_v][3] (NULL: none; only
 * meaningful when the count call had normals) and out_faces[max_f][3]; max_v / max_f are the capacities in rows. */
int nerf_hip_mesh_simplify_emit(const int32_t* faces, int64_t V, int64_t F, const float* lo3, const float* cell3, const int* dims3, void* ws,
                                size_t ws_bytes, float* out_verts, float* out_normals, int32_t* out_faces, int64_t max_v, int64_t max_f,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Edge topology, smoothing steps and face-derived vertex normals of an indexed triangle mesh.  Any indexed
 * mesh: verts[V][3] fp32, faces[F][3] int32, V, F < 2^31.  Every output is a pure function of the input: identical bits from run to
 * run, no float atomic anywhere.
 *
 * A. EDGES AND TOPOLOGY (nerf_hip_mesh_edges_build).  Coordinates play no role.
 * 1. A face TAKES PART iff its three indices lie in [0, V) (others are never used as an address) and are pairwise different.
 * 2. The EDGES are the unordered pairs {a, b} that occur as (i0, i1), (i1, i2) or (i2, i0) of a face that takes part.  count(e) = the
 *    number of participating faces that contain e; tally(e) = (those that run it from its smaller index to its larger) - (those that
 *    run it from its larger to its smaller).
 * 3. A BOUNDARY edge has count == 1, a NON-MANIFOLD edge count > 2, an INCONSISTENT edge count == 2 and tally != 0 (its two faces
 *    run it in the same direction: they are oriented against each other).
 * 4. degree[V] int32 = the number of edges at the vertex (its distinct neighbours); vert_flags[V] int32: bit 0 = the vertex is on a
 *    boundary edge, bit 1 = on a non-manifold edge.
 * 5. counts (DEVICE int64[8]) = the faces that take part, E (the edges), the boundary edges, the non-manifold edges, the
 *    inconsistent edges, the vertices with degree > 0, a flags word (NERF_HIP_EDGES_TABLE_FULL), the largest degree.  From them
 *    euler = used vertices - E + participating faces, and a mesh is CLOSED iff it has a participating face and no boundary,
 *    non-manifold or inconsistent edge.
 * 6. The build call also leaves the NEIGHBOURS of every vertex (the other ends of its edges) in the workspace, for the step call; the
 *    order in which a row lists them is not defined and nothing depends on it.
 * The edges are found through an open-addressing table of int64 keys (a power of two of at least 4 F slots, at least 4).  A probe is
 * bounded by the table size; a probe that found no slot -- which more slots than the 3 F possible keys rule out -- sets
 * NERF_HIP_EDGES_TABLE_FULL in counts[6], and every result of the call must then be discarded.
 *
 * B. THE BOX AND THE FIXED-POINT COORDINATE (steps and normals).  A box is lo[3] (fp32, finite) and ONE scale (fp32, > 0, finite;
 * one scalar on purpose: an anisotropic scale would turn normals).  Per axis, for a finite coordinate p:
 *    uc = clamp((double(p) - double(lo)) / double(scale), -1, 2)      (fp64; the difference and the quotient rounded separately)
 *    q  = rint(uc * 2^30) as int64                                     (round half to even; |q| <= 2^31)
 * A vertex outside [lo - scale, lo + 2 scale] is pulled in by the clamp wherever it acts as a NEIGHBOUR or a CORNER: documented
 * behaviour, as in the simplification, not an error.  The callers' default box (mesh.smooth_box in the Python package): lo = the
 * per-axis minimum over the vertices whose three coordinates are finite; with hi their per-axis maximum and
 * ext = the largest of fp32(hi - lo) over the axes, scale = the smallest power of two >= ext (2^127 where ext is not finite or
 * above 2^127; 1 where ext is not > 0); a mesh without a finite vertex gets lo = 0 and scale = 1.  A caller that gives lo but no scale gets the same rule
 * with ITS lo: ext = the largest of fp32(hi - given lo), hi still the finite vertices' maximum (and lo stays as given, scale = 1,
 * without a finite vertex); a caller that gives scale but no lo gets lo = the minimum and that scale.
 *
 * C. A SMOOTHING STEP with weight w (a finite double) maps verts_in to verts_out, two buffers that do not overlap (a Jacobi step: it
 * reads only its input).
 * 1. A vertex MOVES iff its three coordinates are finite, it has at least one neighbour (A.6) whose three coordinates are finite,
 *    and it is not pinned: it is pinned iff vert_flags is given and bit 0 of its entry is set.
 * 2. For a moving vertex, per axis: S = the sum of q_j over its distinct neighbours j with three finite coordinates (int64, exact,
 *    order free: fewer than 2^31 terms of at most 2^31), n their number,
 *       m   = double(lo) + double(scale) * (double(S) / (double(n) * 2^30))
 *       out = fp32(double(p) + w * (m - double(p)))
 *    in fp64 with every product, quotient, sum and difference rounded on its own, evaluated as bracketed (no fused multiply-add).
 * 3. Any other vertex is copied bit for bit.
 * A Taubin iteration is a step with w = lambda > 0 followed by a step with w = mu < -lambda; plain Laplacian smoothing is the first
 * alone.
 *
 * D. VERTEX NORMALS FROM FACES (nerf_hip_mesh_vertex_normals).
 * 1. A face CONTRIBUTES iff it takes part (A.1) and its three vertices have three finite coordinates each.
 * 2. With u_a, u_b, u_c the clamped box coordinates uc (B; fp64, NOT the rounded q) of its corners i0, i1, i2:
 *    e1 = u_b - u_a, e2 = u_c - u_a, N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), every difference and product
 *    rounded on its own.  |N_k| <= 18.  The face's term is rint(N_k * 2^40) as int64 per component (below 2^45).
 * 3. T_v = the sum of the terms of the contributing faces that have v as a corner: area-weighted, no square root per face.  T_v is
 *    exact while it fits int64, which covers every vertex with fewer than 2^17 incident faces whatever their size (2^17 * 18 * 2^40
 *    < 2^63) and far more in practice; past that it wraps in two's complement.
 * 4. normal = fp32(T / sqrt((Tx Tx + Ty Ty) + Tz Tz)) in fp64, products and sums rounded separately in that order, and (0, 0, 0)
 *    where the length is 0.  Faces are counter-clockwise seen from outside, so the normal points outward.
 *
 * All three calls are enqueue-only on the caller's stream and check every argument on the host before anything is enqueued
 * (NERF_HIP_ERR_ARG: sizes, NULL arrays, lo / scale / w outside the limits above, overlapping step buffers, workspace NULL or not
 * 256-byte aligned, counts not 8-byte aligned; NERF_HIP_ERR_WORKSPACE: workspace too small).  Indices read from device arrays are
 * range-checked by the kernels before use and every store is clamped to max_v.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_EDGES_TABLE_FULL 1

/* Bytes of workspace (256-byte aligned) shared by the three calls below: 16 per slot of the edge table (key 8, count 4, tally 4; the
 * power of two >= 4 F slots, so 64 to 128 per face); 24 per face (the 6 F neighbour entries); 36 per vertex (row offset 8, cursor 4,
 * the normals' sums 24); and 16 per 2048 vertices (the scan). */
int nerf_hip_mesh_edges_ws_bytes(int64_t V, int64_t F, size_t* bytes);

/* A: degree[V], vert_flags[V] (DEVICE int32), counts (DEVICE int64[8]) and, in the workspace, the neighbours. */
int nerf_hip_mesh_edges_build(const int32_t* faces, int64_t V, int64_t F, void* ws, size_t ws_bytes, int32_t* degree, int32_t* vert_flags,
                              int64_t* counts, void* stream);

/* C: one step verts_in[V][3] -> verts_out[max_v][3] (rows from max_v on are not stored) over the neighbours a build call with the same
 * V, F and workspace left.  lo3: a HOST array.  vert_flags: the build call's (DEVICE int32[V]) to pin the boundary, or NULL to pin
 * nothing.  The workspace is only read. */
int nerf_hip_mesh_smooth_step(const float* verts_in, float* verts_out, int64_t V, int64_t F, const float* lo3, float scale, double w,
                              const int32_t* vert_flags, const void* ws, size_t ws_bytes, int64_t max_v, void* stream);

/* D: normals[max_v][3].  Needs no build call and leaves a build call's neighbours intact (it uses the workspace's sums only). */
int nerf_hip_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, void* ws,
                                 size_t ws_bytes, float* normals, int64_t max_v, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Geometry evaluation: measures of a mesh, area-weighted surface samples, exact nearest points between two clouds
 * and distance statistics.  Any indexed mesh (verts[V][3] fp32, faces[F][3] int32, V, F < 2^31), any clouds of
 * fewer than 2^31 points.  Every output is a pure function of the input: identical bits from run to run, no float atomic anywhere;
 * every product, quotient, sum and difference below is fp64 (unless marked fp32), rounded on its own and evaluated as bracketed.
 *
 * A. MEASURES (nerf_hip_mesh_measure) over a box lo[3] / scale (section B of the block above: one scale, fp32).
 * 1. A face TAKES PART iff its three indices lie in [0, V) (others are never used as an address), are pairwise different, and its
 *    three corners have three finite coordinates each.  u_a, u_b, u_c = the clamped box coordinates uc (fp64) of corners i0, i1, i2.
 * 2. e1 = u_b - u_a, e2 = u_c - u_a, N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), len = sqrt((Nx Nx + Ny Ny) + Nz Nz),
 *    area = len * 0.5.  X = (u_by u_cz - u_bz u_cy, u_bz u_cx - u_bx u_cz, u_bx u_cy - u_by u_cx), six = (u_ax Xx + u_ay Xy) + u_az Xz:
 *    six times the signed volume of the tetrahedron (box origin, a, b, c).  m_d = area * (((u_ad + u_bd) + u_cd) / 3.0) per axis d.
 * 3. The face's five terms are rint(area * 2^40), rint(six * 2^40) and rint(m_d * 2^40) as int64 (round half to even).  The sixth of
 *    the volume is left to the reader of the sums (one division instead of one rounding per face: a mesh whose box coordinates are
 *    small integers, a unit cube in its default box, has an exact volume whatever its triangulation).
 * 4. out (DEVICE int64[8]) = the sum of the area terms, of the six-volume terms, of the three moment terms, the number of faces that
 *    take part, 0, 0.  In box units: area = out[0] / 2^40, volume = out[1] / (6 * 2^40) (meaningful for a closed, consistently
 *    oriented mesh; positive for outward faces), area-weighted centroid = out[2 + d] / out[0]; in the mesh's units area * scale^2,
 *    volume * scale^3, lo + scale * centroid.
 * 5. THE BOUND.  With |uc| <= 2: |N_k| <= 18, area < 16, |six| <= 48, |m_d| < 32, so a term is below 2^46 and the sums are exact while
 *    F < 2^17, whatever the mesh and the box.  Inside its default box (mesh.smooth_box: uc in [0, 1]) a face has area < 1, |six| <= 2
 *    and |m_d| <= area, so every sum of a mesh of fewer than 2^22 faces is exact; a larger mesh keeps exact sums while its total area
 *    stays below 2^23 box faces and the absolute sum of its six-volumes below 2^23 (6 at most for a simple closed surface): any
 *    surface that does not fold millions of times across its box.  The 2^40 is the normals' (section 3h-6): a face of a 4096^3
 *    lattice still has 16 bits of area.  Past the bound the sums wrap in two's complement, as section 3h-6's normal sums do.
 *
 * B. SURFACE SAMPLES (nerf_hip_mesh_sample): n points distributed by area, a pure function of (verts, faces, n, seed, box).
 * 1. The WEIGHT of a face is w_f = rint(len * 2^39) as int64 with len of A.2 -- the area term of A.3, bit for bit -- and 0 for a face
 *    that takes no part.  cum[f] = w_0 + ... + w_f (int64), W = cum[F - 1] (0 for F == 0) = out[0] of A.  info (DEVICE int64[1]) = W.
 * 2. h(seed, i, s) for the uint32 seed, the sample i and the stream s in {0, 1, 2}, all arithmetic modulo 2^32:
 *       fin(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *       h = fin(fin(fin(seed + 0x9E3779B9 * (s + 1)) ^ i) + seed)           r_s = (double(h) + 0.5) / 2^32   in (0, 1)
 * 3. Sample i (stratified: one sample per stratum of W / n):  t = (int64) floor(((double(i) + r_0) / double(n)) * double(W)), at most
 *    W - 1;  f = the first face with cum[f] > t (a face of weight 0 is never chosen);  (r_1, r_2) folded: if r_1 + r_2 > 1.0 then
 *    r_1 = 1.0 - r_1 and r_2 = 1.0 - r_2;  per axis, on the ORIGINAL coordinates A, B, C of corners i0, i1, i2 widened to fp64:
 *       point = fp32((A + r_1 * (B - A)) + r_2 * (C - A))
 *    points[i] = point, face[i] = f.  Where W <= 0 (no area, or sums past A.5's bound), or the chosen face takes no part (possible
 *    only past that bound), face[i] = -1 and points[i] = 0.  Rows from cap_n on are not stored.
 *
 * C. NEAREST POINTS (nerf_hip_points_grid_build, nerf_hip_points_nearest): ref[M][3], query[N][3] fp32.
 * 1. d2(q, p) = (dx dx + dy dy) + dz dz with dx = double(q_x) - double(p_x) and so on.  dist2[j] (fp64) = the minimum of d2(query_j, p)
 *    over the reference points p with three finite coordinates; idx[j] (int32) = the LOWEST index that attains it.  A query with a
 *    coordinate that is not finite, and any query when no reference point is finite, gets idx = -1 and dist2 = +inf.  That is the
 *    brute-force result, bit for bit.
 * 2. THE GRID is an accelerator and never changes an output: lo[3] (fp32, finite), ONE cell size (fp32, > 0, finite) and dims[3]
 *    (>= 1 each, product < 2^31), any values.  A point's cell along an axis is floor((double(p) - double(lo)) / double(cell)) clamped to
 *    [0, dims - 1]; queries use the same function, so they may lie anywhere.  The callers' sizing rule (mesh.nearest_grid in the Python
 *    package, from one min / max read): over the finite reference points, their number m, lo = the per-axis minimum, ext =
 *    double(hi) - double(lo) per axis; no finite point or no ext > 0: cell = 1, dims = (1, 1, 1); otherwise with k = the axes of
 *    ext > 0, cell = fp32((the product of those ext / m) ^ (1 / k)) kept inside [2^-126, 2^127], doubled until dims_d =
 *    floor(ext_d / cell) + 1 (1 on an axis of zero extent) have a product <= 2 m + 8 (one cell if 2^127 is reached first):
 *    cells <= 2 M + 8, below 2^31.
 * 3. The build call sorts the reference points by cell (counts by integer atomics, an exclusive scan, placement through per-cell
 *    cursor atomics) into 16-byte records (x, y, z, index) in the workspace; counts (DEVICE int64[2]) = the finite reference points,
 *    the points of the fullest cell.  The order of the records inside a cell is not defined and nothing depends on it.
 * 4. The query call walks, per query, the Chebyshev shells r = 0, 1, 2, ... of cells around the query's own (clamped) cell and stops
 *    after shell r when best < g * g, g = the smallest over the faces of the block [c - r, c + r] that are not faces of the grid of
 *    (the distance from the query to the face's plane lo + n * cell) - 2^-45 * (|q| + |lo| + n * cell); or when the block covers the
 *    grid.  The proof that this is the brute-force result is at the top of csrc/mesh_distance.hip.  sort_queries != 0 processes the
 *    queries in their own cell order (the same counting sort) and scatters each result to the query's slot; the results are the same.
 *    The query call leaves the build call's records intact: one build serves any number of query calls with the same M, grid and
 *    workspace (N may differ as long as the workspace holds nerf_hip_points_nearest_ws_bytes(M, N, dims)).
 *
 * D. DISTANCE STATISTICS (nerf_hip_distance_stats): dist2[N] fp64, a unit (fp64, > 0, finite, its square as well) and K <= 8
 * thresholds tau_k (fp64, finite, >= 0; HOST array).  A distance COUNTS iff it is finite and >= 0.  out (DEVICE int64[4 + K]) =
 *    the distances that count;  the sum of rint(min(sqrt(d2) / unit, 8) * 2^30);  the sum of rint(min(d2 / (unit * unit), 64) * 2^30);
 *    those with sqrt(d2) / unit > 8 or d2 / (unit * unit) > 64 (CLAMPED: reported, never hidden);  per k those with d2 <= tau_k * tau_k.
 * A term is at most 2^36: the sums are exact for N < 2^27 whatever the distances, and for every N < 2^31 when nothing is clamped
 * and sqrt(d2) <= 2 unit.
 *
 * All calls are enqueue-only on the caller's stream and check every argument on the host before anything is enqueued
 * (NERF_HIP_ERR_ARG: sizes, NULL arrays, lo / scale / cell / unit / thresholds outside the limits above, workspace NULL or not
 * 256-byte aligned, int64 / fp64 outputs not 8-byte aligned; NERF_HIP_ERR_WORKSPACE: workspace too small).  Indices read from device
 * arrays are range-checked by the kernels before use and every store is clamped to cap_n.
 * ------------------------------------------------------------------------------------------- */

/* A: out (DEVICE int64[8]).  lo3: a HOST array. */
int nerf_hip_mesh_measure(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, int64_t* out,
                          void* stream);

/* Bytes of workspace (256-byte aligned) of the sampling call: 8 per face (cum) and 16 per 2048 faces (the scan). */
int nerf_hip_mesh_sample_ws_bytes(int64_t F, size_t* bytes);

/* B: points[cap_n][3] fp32, face[cap_n] int32, info (DEVICE int64[1]) = W.  n < 2^31. */
int nerf_hip_mesh_sample(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, int64_t n,
                         uint32_t seed, void* ws, size_t ws_bytes, float* points, int32_t* face, int64_t cap_n, int64_t* info,
                         void* stream);

/* Bytes of workspace (256-byte aligned) of the two calls below: the reference grid -- 8 per cell (count / cursor, start), 16 per
 * reference point (its record), 8 per 2048 cells (the scan) -- then the queries' order: 8 more per cell, 16 per query, 8 for their
 * total.  The build call needs only the first part: nerf_hip_points_nearest_ws_bytes(M, 0, dims). */
int nerf_hip_points_nearest_ws_bytes(int64_t M, int64_t N, const int* dims3, size_t* bytes);

/* C.3: the reference grid into the workspace, counts (DEVICE int64[2]).  lo3, dims3: HOST arrays. */
int nerf_hip_points_grid_build(const float* ref, int64_t M, const float* lo3, float cell, const int* dims3, void* ws, size_t ws_bytes,
                               int64_t* counts, void* stream);

/* C.4: idx[cap_n] int32, dist2[cap_n] fp64 for query[N][3] against the grid a build call with the same M, lo3, cell, dims3 and
 * workspace left. */
int nerf_hip_points_nearest(const float* query, int64_t M, int64_t N, const float* lo3, float cell, const int* dims3, void* ws,
                            size_t ws_bytes, int sort_queries, int32_t* idx, double* dist2, int64_t cap_n, void* stream);

/* D: out (DEVICE int64[4 + K]).  tau: a HOST array of K doubles. */
int nerf_hip_distance_stats(const double* dist2, int64_t N, double unit, const double* tau, int K, int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Rays against a mesh: closest hit and occlusion over a uniform grid of triangles, the visibility of faces from a
 * camera and the selection of faces.  Any indexed mesh (verts[V][3] fp32, faces[F][3] int32, V, F < 2^31),
 * fewer than 2^31 rays.  All arithmetic below is fp64 on the fp32 inputs widened exactly; every product, quotient, sum and difference
 * is rounded on its own and evaluated as bracketed; (a x b) = (ay bz - az by, az bx - ax bz, ax by - ay bx).  There is no float atomic:
 * every output is a pure function of the input, identical bits from run to run.  Every comparison is false on NaN.
 *
 * R. THE HIT RULE, a function of one ray and one face only.
 * 1. A face TAKES PART iff its three indices lie in [0, V) (others are never used as an address) and its nine coordinates are finite
 *    (the indices may repeat: such a face has det == 0 and is never hit).  A ray TAKES PART iff its origin o and direction d (fp32,
 *    d not normalised: t is in units of d) are six finite numbers and d != 0.
 * 2. With the corners A, B, C of indices i0, i1, i2 (Moeller-Trumbore):
 *       e1 = B - A,  e2 = C - A,  p = d x e2,  det = (e1x px + e1y py) + e1z pz,  s = o - A,  q = s x e1
 *       u = ((sx px + sy py) + sz pz) / det,   v = ((dx qx + dy qy) + dz qz) / det,   t = ((e2x qx + e2y qy) + e2z qz) / det
 *       h_k = o_k + t * d_k per axis k,        e = 2^-20 * the largest |coordinate| of the face's nine
 *    The ray HITS the face iff det != 0, u >= 0, v >= 0, u + v <= 1, tmin <= t <= tmax and on every axis
 *    min(A_k, B_k, C_k) - e <= h_k <= max(A_k, B_k, C_k) + e: a hit whose computed point is not on its triangle is no hit.  (That last
 *    condition is what lets a grid reproduce brute force exactly; it changed no answer on the test meshes.)
 * 3. A ray's answer is the hit with the smallest t, among equal t the LOWEST face index.  skip[N] (int32, may be NULL): ray i ignores
 *    face skip[i].  Outputs: t[N] fp64, uv[N][2] fp64 = (u, v), face[N] int32, side[N] int8 = +1 for det > 0 (the ray meets the
 *    counter-clockwise side), -1 for det < 0.  No hit, or a ray that takes no part: t = +inf, uv = 0, face = -1, side = 0.
 * 4. any_hit != 0: the only output is occluded[N] uint8 = (face >= 0 of the closest-hit call); the walk stops at the first hit.
 * 5. This is NOT a watertight test: u, v of two faces that share an edge are rounded independently, so a ray through the edge can
 *    in principle miss both.
 *
 * G. THE TRIANGLE GRID is an accelerator and never changes an output: lo[3] (fp32, finite), ONE cell size (fp32, > 0, finite) and
 *    dims[3] (>= 1 each, product < 2^31), any values.  cellidx_k(x) = floor((x - double(lo_k)) / double(cell)), not clamped.  The
 *    index box of a face that takes part is [cellidx_k(min_k - e), cellidx_k(max_k + e)] per axis with min, max and e of R.2.  A face
 *    whose box lies in [0, dims_k - 1] on every axis is INSIDE and is entered in every cell of its box; any other goes to the OUTSIDE
 *    list, which every ray tests in full; a face that takes no part is entered nowhere.  nerf_hip_mesh_raycast_grid_count returns
 *    counts (DEVICE int64[3]) = the faces that take part, the entries E (the sum of the INSIDE faces' box volumes), the OUTSIDE faces;
 *    the host reads E (it must be < 2^31) and sizes the workspace; nerf_hip_mesh_raycast_grid_fill counts the cells' entries by integer
 *    atomics, scans them and places the entries through per-cell cursor atomics.  The order of the entries inside a cell is not defined
 *    and nothing depends on it.  Nothing is stored past cap_entries (a cap below E leaves a grid that misses faces).  The callers'
 *    sizing rule (mesh.raycast_grid in the Python package): C.2's rule of the block above over the finite vertices' box grown by 2^-19
 *    of its largest |coordinate| on every side (more than e: no face with finite corners is OUTSIDE), with m = F, the cell doubled
 *    while E > 4 F + 64.  The cast call walks the ray through the cells in intervals of t; the proof that the result is the
 *    brute-force answer over all faces for every grid is at the top of csrc/mesh_raycast.hip.
 *
 * V. FACE VISIBILITY FROM A CAMERA (nerf_hip_mesh_face_rays): one shadow ray per face.  cam_o[3] (HOST fp32) is the camera's position
 *    and Q (HOST fp64 3x3, row-major) maps a world direction to homogeneous pixel coordinates: with the ray rule of nerf_hip_rays,
 *    p_j = (x K[j] + y K[3 + j]) + K[6 + j] and the world direction R p, Q = inverse(R K^T), formed by the caller.  Per face that takes
 *    part: G = ((A + B) + C) / 3.0, N = e1 x e2, w = double(cam_o) - G; FACING iff (Nx wx + Ny wy) + Nz wz > 0; m = Q (-w) row by row as
 *    (Q_i0 a + Q_i1 b) + Q_i2 c; IN VIEW iff m_2 > 0, -0.5 <= m_0 / m_2 < H - 0.5 and -0.5 <= m_1 / m_2 < W - 0.5 (x is the row: quirk
 *    Q2).  Outputs: orig[F][3] = fp32(G), valid[F] uint8 = facing and in view, dir[F][3] = fp32(double(cam_o) - double(orig)) for a valid
 *    face and 0 for any other; a face that takes no part gets orig = 0 as well.  The caller then casts (orig, dir) in any-hit mode
 *    with skip = the face itself over [tmin, 1]: the face is seen from this camera iff valid and not occluded.  tmin keeps the
 *    segment off the surface it starts on; the package's default 1e-4 of the segment is a choice, not a measurement.
 *
 * S. FACE SELECTION (nerf_hip_mesh_select_faces_count / _emit) with keep[F] uint8: a face is kept iff keep[f] != 0 and its three
 *    indices lie in [0, V); a vertex is kept iff a kept face uses it.  Both keep their order, the faces are renumbered, normals and
 *    rgb are carried where given.  The count call returns counts (DEVICE int64[2]) = V', F'; the emit call stores nothing past max_v /
 *    max_f rows.
 *
 * All calls are enqueue-only on the caller's stream and check every argument on the host before anything is enqueued
 * (NERF_HIP_ERR_ARG: sizes, NULL arrays, lo / cell / dims / cam_o / Q outside the limits above, tmin or tmax NaN, workspace NULL or not
 * 256-byte aligned, int64 / fp64 outputs not 8-byte aligned; NERF_HIP_ERR_WORKSPACE: workspace too small).  Indices read from device
 * arrays are range-checked by the kernels before use and every store is clamped to its capacity.
 * ------------------------------------------------------------------------------------------- */

/* Bytes of workspace (256-byte aligned) of the fill and cast calls: 8 per cell, 4 per entry, 4 per face (the OUTSIDE list), 8 per 2048
 * cells or faces (the scans), 16 more. */
int nerf_hip_mesh_raycast_ws_bytes(int64_t F, int64_t cap_entries, const int* dims3, size_t* bytes);

/* G: counts (DEVICE int64[3]).  lo3, dims3: HOST arrays.  Needs no workspace. */
int nerf_hip_mesh_raycast_grid_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell,
                                     const int* dims3, int64_t* counts, void* stream);

/* G: the grid into the workspace. */
int nerf_hip_mesh_raycast_grid_fill(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell,
                                    const int* dims3, int64_t cap_entries, void* ws, size_t ws_bytes, void* stream);

/* R: origins, dirs [N][3] fp32 against the grid a fill call with the same mesh, lo3, cell, dims3, cap_entries and workspace left.
 * any_hit == 0: t[cap_n], uv[cap_n][2], face[cap_n], side[cap_n] (occluded may be NULL); otherwise occluded[cap_n] (the others may be
 * NULL).  tmin, tmax: fp64, infinite ends allowed. */
int nerf_hip_mesh_raycast(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell, const int* dims3,
                          int64_t cap_entries, const void* ws, size_t ws_bytes, const float* origins, const float* dirs,
                          const int32_t* skip, int64_t N, double tmin, double tmax, int any_hit, double* t, double* uv, int32_t* face,
                          int8_t* side, uint8_t* occluded, int64_t cap_n, void* stream);

/* V: orig[cap_f][3], dir[cap_f][3] fp32, valid[cap_f] uint8.  cam_o3: HOST fp32[3]; Q9: HOST fp64[9]. */
int nerf_hip_mesh_face_rays(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* cam_o3, const double* Q9, int H,
                            int W, float* orig, float* dir, uint8_t* valid, int64_t cap_f, void* stream);

/* Bytes of workspace (256-byte aligned) of the two selection calls: 8 per vertex, 8 per 2048 vertices or faces, 16 more. */
int nerf_hip_mesh_select_faces_ws_bytes(int64_t V, int64_t F, size_t* bytes);

/* S: counts (DEVICE int64[2]) = V', F'. */
int nerf_hip_mesh_select_faces_count(const int32_t* faces, int64_t V, int64_t F, const uint8_t* keep, void* ws, size_t ws_bytes,
                                     int64_t* counts, void* stream);

/* S: out_verts / out_normals / out_rgb [max_v][3] (the latter two only where normals / rgb are given), out_faces[max_f][3].  Needs no
 * count call before it. */
int nerf_hip_mesh_select_faces_emit(const float* verts, const float* normals, const float* rgb, const int32_t* faces, int64_t V, int64_t F,
                                    const uint8_t* keep, void* ws, size_t ws_bytes, float* out_verts, float* out_normals, float* out_rgb,
                                    int32_t* out_faces, int64_t max_v, int64_t max_f, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 addition.  TSDF fusion: depth images of known cameras integrated into a truncated signed distance volume (DESIGN.md section
 * 3h-9).  tsdf and weight are fp32 volumes [nx][ny][nz] (C order, z fastest) on the lattice of nerf_hip_density_grid: point (i, j, k) is
 * lo + (i, j, k) * step, each coordinate one fp32 product and one fp32 sum.  The caller owns both volumes and zeroes them before the
 * first call; later calls continue the same fusion.  depth[n][H][W] (fp32) is the distance along the UNIT ray of pixel (row x, column
 * y) of view c; opacity[n][H][W] (fp32) may be NULL.  cam_o (HOST fp32 [n][3]) are the cameras' positions and Q (HOST fp64 [n][9],
 * row-major) their maps from a world direction to homogeneous pixel coordinates, Q = inverse(R K^T) as in rule V above.
 *
 * T. THE FUSION RULE.  All arithmetic is fp64 on the fp32 inputs widened exactly; every operation is rounded on its own and evaluated
 *    as bracketed (rule R's convention); every comparison is false on NaN.  Per voxel p, with state (T, Wt) = (tsdf, weight) at p, and
 *    per view c IN VIEW ORDER:
 *       w   = double(p) - double(cam_o_c)                                  per axis
 *       m_i = (Q_i0 wx + Q_i1 wy) + Q_i2 wz                                i = 0, 1, 2
 *       x   = floor(m_0 / m_2 + 0.5),   y = floor(m_1 / m_2 + 0.5)         (x is the row: quirk Q2)
 *       IN VIEW iff m_2 > 0, 0 <= x <= H - 1 and 0 <= y <= W - 1           (compared in fp64, before any conversion to an integer)
 *       r   = sqrt((wx wx + wy wy) + wz wz)
 *       d   = depth[c][x][y],   a = opacity[c][x][y]
 *       FOREGROUND iff opacity is NULL or a >= min_opacity
 *    A voxel that is not in view is not observed.  A FOREGROUND pixel observes the voxel iff d is finite, d > 0 and
 *    sdf = d - r >= -trunc; the observation is val = min(1.0, sdf / trunc).  With NERF_HIP_TSDF_CARVE a pixel that is in view and NOT
 *    foreground observes the voxel with val = 1.0 (the ray saw nothing: everything along it is empty); without the flag such a pixel
 *    observes nothing.  An observation updates
 *       T'  = fp32(((double(T) * double(Wt)) + val) / (double(Wt) + 1.0)),   Wt' = fp32(double(Wt) + 1.0)
 *    The state is rounded to fp32 after every view, so the result does not depend on how the views are grouped into launches or calls.
 *    T > 0 in front of the observed surface, T < 0 behind it (down to one truncation distance); Wt = the number of observations.
 *
 * One thread per voxel, z fastest; each launch reads and writes every voxel once and runs NERF_HIP_TSDF_VIEWS_PER_LAUNCH views, whose
 * cameras travel in the kernel arguments.  No atomics: every output is a pure function of the input.  Enqueue-only; every argument is
 * checked on the host before anything is enqueued (NERF_HIP_ERR_ARG): a dimension < 1, nx * ny * nz >= 2^31, n < 0, H < 1, W < 1,
 * n * H * W >= 2^31, a NULL tsdf / weight / lo3 / step3 and, with n > 0, a NULL depth / cam_o / Q, a lo, step, cam_o or Q that is not
 * finite, trunc not finite or not > 0, min_opacity NaN, a flag bit other than NERF_HIP_TSDF_CARVE.  n == 0 succeeds and launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_TSDF_CARVE 1
#define NERF_HIP_TSDF_VIEWS_PER_LAUNCH 32 /* 88 bytes of camera each: 2.8 KB of the 4 KB a kernel's arguments may take */

int nerf_hip_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* lo3, const float* step3,
                            const float* depth, const float* opacity, int n, int H, int W,
                            const float* cam_o /* HOST [n][3] */, const double* Q /* HOST [n][9] */,
                            double trunc, float min_opacity, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Colour fusion: the colours the views show, fused beside the distances, and read back at
 * arbitrary points.  The new state is a colour volume color[nx][ny][nz][4] (fp32; (R, G, B, Wc) per lattice point, z fastest, 16-byte
 * aligned), owned and zeroed by the caller like tsdf and weight.  rgb[n][H][W][3] (fp32) is the colour view c shows at pixel (x, y).
 *
 * TC. THE COLOUR RULE.  Per voxel and view, in view order, with rule T's quantities: the geometry update is rule T unchanged -- tsdf and
 *    weight leave nerf_hip_tsdf_integrate_color with the bits nerf_hip_tsdf_integrate gives them.  The view makes a COLOUR OBSERVATION
 *    of the voxel iff the voxel is in view, the pixel is FOREGROUND, it observes the voxel by rule T's foreground branch (d finite,
 *    d > 0, sdf >= -trunc), sdf <= trunc (fp64, false on NaN), and the pixel's three colour channels are finite.  So the voxel lies within
 *    one truncation distance of that view's surface, on either side; carving observations and observations far in front of the surface
 *    carry no colour, and a pixel whose colour is not finite still makes its geometry observation.  A colour observation updates, in
 *    fp64 on the fp32 state (C_ch, Wc) and the fp32 pixel colour c_ch, per channel
 *       C_ch' = fp32(((double(C_ch) * double(Wc)) + double(c_ch)) / (double(Wc) + 1.0)),   then   Wc' = fp32(double(Wc) + 1.0)
 *    (the three channels use the old Wc).  The state is rounded after every view, so the result does not depend on how the views are
 *    grouped into launches or calls.  Wc = the number of colour observations; a voxel with Wc == 0 has no colour.
 *    A voxel that receives no colour observation in a launch neither loads nor stores its colour state.
 *
 * Refusals: everything nerf_hip_tsdf_integrate refuses, a NULL or misaligned color and, with n > 0, a NULL rgb.  n == 0 succeeds and
 * launches nothing.
 * ------------------------------------------------------------------------------------------- */
int nerf_hip_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* lo3, const float* step3,
                                  const float* depth, const float* opacity, const float* rgb, int n, int H, int W,
                                  const float* cam_o /* HOST [n][3] */, const double* Q /* HOST [n][9] */,
                                  double trunc, float min_opacity, int flags, void* stream);

/* S. THE SAMPLING RULE.  points[M][3] (fp32) -> rgb[M][3] (fp32), valid[M] (uint8, 0 / 1): the colour volume interpolated trilinearly
 *    over the corners that have a colour.  Per point and axis a, in fp64 on the fp32 inputs:
 *       g = (x_a - lo_a) / step_a,   i = min(max(floor(g), 0), n_a - 2),   f = min(max(g - i, 0), 1)
 *    (clamped in fp64 before i becomes an integer: a point outside the box takes the colour of the box's nearest face); along an axis
 *    with n_a == 1, i = 0, f = 0 and the upper corner is not read.  The corners (i + di, j + dj, k + dk) of the cell are visited in the
 *    order (di, dj, dk), dk fastest; a corner with Wc > 0 (false on NaN) adds
 *       w = (wx * wy) * wz   to den   and   w * double(C_ch)   to num_ch,      w_a = f_a at the upper corner, 1.0 - f_a at the lower,
 *    every product and sum rounded on its own, the sums in that order from 0.0; a corner without a colour adds nothing.
 *    valid = den > 0 and rgb_ch = fp32(num_ch / den); an invalid point gets rgb = 0, as does a point with a coordinate that is not finite.
 * One thread per point; the only data-dependent addresses are the eight corners.  Refused: a dimension < 1, nx * ny * nz >= 2^31, M < 0
 * or >= 2^31, a NULL or misaligned color, a NULL lo3 / step3, a lo that is not finite, a step that is not finite and > 0 along a
 * dimension of more than one point and, with M > 0, a NULL points / rgb / valid.  M == 0 succeeds and launches nothing.  lo3 / step3
 * are HOST arrays.  Enqueue-only. */
int nerf_hip_tsdf_sample_color(const float* color, int nx, int ny, int nz, const float* lo3, const float* step3, const float* points,
                               int64_t M, float* rgb, uint8_t* valid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Texture atlases of indexed meshes: a parameterisation that is a pure function of the
 * face count, the surface point and viewing direction of every texel (the caller shades them: a field query, a colour volume), and
 * bilinear lookups by (face, u, v) -- what nerf_hip_mesh_raycast returns.  verts, normals [V][3] fp32, faces [F][3] int32.
 *
 * TA. THE ATLAS RULE.  Every face gets the same right-isosceles chart.  n (an int >= 2) is the chart edge in texels, c = n + 5 the cell
 *    edge, K = ceil(F / 2) the number of cells.  Sx is the smallest integer with Sx * Sx >= K (integer arithmetic), Sy = ceil(K / Sx);
 *    the atlas is W = Sx * c texels wide and H = Sy * c high, an image [H][W] with row y and column x; F = 0 gives Sx = Sy = W = H = 0.
 *    Face f lives in cell k = f >> 1 at (cx, cy) = (k % Sx, k / Sx).  Of the cell-local texel (i, j), 0 <= i, j < c (i along x), the
 *    even (LOWER) face owns i + j <= c - 1 and the odd (UPPER) face i + j >= c; the upper face is addressed through the point
 *    reflection (i, j) -> (c - 1 - i, c - 1 - j), after which everything below is the lower face's.  A texel whose face index is >= F
 *    (the last upper half of an odd F, the unused cells of the last row) is UNOWNED: mask 0, point 0, dir 0.
 *    Chart corners, in cell-local texel coordinates with texel (i, j)'s centre at (i + 0.5, j + 0.5): A = (1.5, 1.5),
 *    B = (1.5 + n, 1.5), C = (1.5, 1.5 + n) -- on texel centres; an upper face's are c - these.  The UV table: uv[f][corner] =
 *    (fp32(cx * c + x) / fp32(W), fp32(cy * c + y) / fp32(H)), one fp32 division each (the half-integers are exact in fp32 below
 *    2^23), y pointing DOWN (a file format with v pointing up stores 1 - y).
 *    Weights of a lower texel, with a = i - 1, b = j - 1, as integers over 2n:
 *       SUPPORT  a >= 0, b >= 0, a + b <= n + 1:   (w0, u, v) * 2n = (2n - 2a - 2b, 2a, 2b).  On a + b = n + 1 this extrapolates one
 *                texel past the hypotenuse (w0 = -1/n), on purpose: with it a bilinear lookup inside the chart returns a colour that is
 *                linear over the face exactly; clamping there instead is wrong by 0.1 .. 0.25 of the colour range at the hypotenuse.
 *       GUTTER   every other owned texel: a and b are clamped to [0, n]; then, if a + b > n, the point is projected onto the
 *                hypotenuse: (u, v) * 2n = (a - b + n, b - a + n); otherwise (u, v) * 2n = (2a, 2b).  w0 * 2n = 2n - u * 2n - v * 2n.
 *    Each weight is one fp32 division fp32(integer) / fp32(2n).  With the face's corners (A3, B3, C3) = verts[faces[f]] and their
 *    normals, per axis in fp32, every product and sum rounded on its own:
 *       p  = w0 * A3 + (u * B3 + v * C3),      nb = w0 * nA + (u * nB + v * nC)
 *       L  = sqrt((nb_x * nb_x + nb_y * nb_y) + nb_z * nb_z),      dir = -(nb / L) where L is finite and > 0, else (0, 0, 0)
 *    (the normalisation of the marching-cubes normals).  A texel ON A VERTEX -- two of the three integer weights are 0, the third is
 *    then 2n: the corner texels and the gutter texels clamped onto them -- takes that vertex's position and normal as they are:
 *    p = the vertex, dir = -normal (0 where a component of the normal is not finite).  Normalising a unit fp32 vector again can move
 *    it by an ulp; taken as it is, the corner texel is shaded with exactly the point and direction of the mesh's own vertex colour.
 *    An owned texel has mask 1 -- unless its face has an index outside [0, V): mask 0, point 0, dir 0.
 *    Two properties follow (tests/test_mesh_texture_cpu.py holds them): every texel a bilinear lookup inside a face's chart touches with
 *    non-zero weight is owned by that face, and a colour linear over the face comes back from the lookup exactly.
 *    Uniform charts: a sliver gets as many texels as a large face; charts sized by area are not built.
 *
 * TX. THE LOOKUP RULE.  face[N] int32, uv[N][2] fp64, image[H][W][3] fp32 over the atlas of (F, n) -> rgb[N][3] fp32, valid[N] uint8.
 *    face < 0, face >= F, or u or v not finite: rgb = background, valid = 0.  Otherwise valid = 1 and, in fp64 with every operation
 *    rounded on its own:  u = min(max(u, 0), 1),  v = min(max(v, 0), 1 - u);  tx = 1 + u * n,  ty = 1 + v * n  (the point
 *    A + u (n, 0) + v (0, n) in units of texel centres);  i0 = min(floor(tx), c - 2), fx = tx - i0, and j0, fy alike.  The four texels
 *    (i0 + di, j0 + dj) of the lower chart -- reflected for an upper face, then moved to the face's cell -- are visited in the order
 *    (dj, di), di fastest; one with weight w = wx * wy != 0 (wx = fx at di = 1, 1 - fx at di = 0) adds w * double(texel_ch) to a sum
 *    that starts at 0.0; one with weight 0 is not read.  rgb_ch = fp32(sum).  At a chart corner the result is the corner texel's bits.
 *
 * Refused (NERF_HIP_ERR_ARG): n < 2, F < 0 or V < 0, 3 F >= 2^31, W * H >= 2^31 (or W or H alone), row0 < 0, rows < 0,
 * row0 + rows > H, N < 0 or >= 2^31, a NULL out5, a NULL faces with F > 0, a NULL verts / normals with V > 0 and, where there is
 * something to write or read, a NULL points / dirs / mask, image / face / uv / background3 / rgb / valid; a uv that is not 8-byte
 * aligned.  Empty calls succeed and launch nothing.  Enqueue-only; background3 and out5 are HOST arrays.
 * ------------------------------------------------------------------------------------------- */

/* TA's sizes, on the host: out5 = c, Sx, Sy, W, H. */
int nerf_hip_mesh_atlas_dims(int64_t F, int n, int* out5);

/* TA: the texels of the atlas rows [row0, row0 + rows), T = rows * W of them in row-major order: points[T][3], dirs[T][3] fp32,
 * mask[T] uint8. */
int nerf_hip_mesh_atlas_texels(const float* verts, const float* normals, const int32_t* faces, int64_t V, int64_t F, int n, int row0,
                               int rows, float* points, float* dirs, uint8_t* mask, void* stream);

/* TX: image is the [H][W][3] atlas of (F, n). */
int nerf_hip_mesh_texture_sample(const float* image, int64_t F, int n, const int32_t* face, const double* uv, int64_t N,
                                 const float* background3, float* rgb, uint8_t* valid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage entry points (same kernels as nerf_hip_forward; exposed so each row of the hot-path
 * table can be parity-checked on its own).
 * ------------------------------------------------------------------------------------------- */

/* Ray generation (nerf.py:52-67, 186-197, 211, 288): per ray d_cam[B,3], d_wrd[B,3], t_coarse[B,Nc]. */
int nerf_hip_rays(const int64_t* row, const int64_t* col, const float* poses_bound, const float* K_inv9,
                  int B, int Nc, float* d_cam, float* d_wrd, float* t_coarse, void* stream);

/* The field query below with the bf16 MLP of NERF_HIP_BF16_MLP (no debug outputs).
 * ws: >= nerf_hip_ws_bytes(B, N, N, NERF_HIP_BF16_MLP). */
int nerf_hip_field_bf16(const float* const* weights24, const int64_t* row, const int64_t* col,
                        const float* poses_bound, const float* K_inv9, const float* t, int B, int N,
                        float* rgb, float* sigma, void* ws, size_t ws_bytes, void* stream);

/* Field query (nerf.py:200-219 + Encoder 135-167 + Network 101-124) at depths t[B,N]:
 * rgb[B,N,3], sigma[B,N]; optional debug outputs pts[B,N,3], gamma_p[B,N,60] (may be NULL).
 * ws: >= nerf_hip_ws_bytes(B, N, N, 0). */
int nerf_hip_field(const float* const* weights24, const int64_t* row, const int64_t* col,
                   const float* poses_bound, const float* K_inv9, const float* t, int B, int N,
                   float* rgb, float* sigma, float* pts, float* gamma_p,
                   void* ws, size_t ws_bytes, void* stream);

/* Coarse weights, colour and inverse-CDF resampling (nerf.py:263-281, 293-295, 225-261, 320):
 * in t_c, sigma_c [B,Nc], rgb_c [B,Nc,3], near_far [B,2]; out w_c [B,Nc], C_coarse [B,3], t_f [B,Nf],
 * status[1] u32 (OR-ed).  delta0 = coarse spacing used in the slope (HOST value). */
int nerf_hip_coarse_composite(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                              float delta0, int B, int Nc, int Nf, float* w_c, float* C_coarse, float* t_f,
                              uint32_t* status, void* stream);

/* Backward of nerf_hip_coarse_composite (autograd through nerf.py:225-281): given dC_coarse[B,3] and the TOTAL
 * d loss/d t_f [B,Nf], ADDS the gradients through C_coarse and through the inverse-CDF resampling to
 * dsig_c[B,Nc] and drgb_c[B,Nc,3] (which already hold the contribution of the merged composite). */
int nerf_hip_coarse_composite_backward(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                       float delta0, int B, int Nc, int Nf, const float* dC_coarse, const float* dt_f,
                                       float* dsig_c, float* drgb_c, void* stream);

/* Merge + per-channel sort + composite (nerf.py:302-321): in t_c/t_f, sigma_c/sigma_f, rgb_c/rgb_f;
 * out sorted bundle[B,Nc+Nf,5] (t,r,g,b,sigma; may be NULL), w[B,Nc+Nf] (may be NULL), C_fine[B,3]. */
int nerf_hip_merge_composite(const float* t_c, const float* t_f, const float* sigma_c, const float* sigma_f,
                             const float* rgb_c, const float* rgb_f, int B, int Nc, int Nf, float last_delta,
                             float* bundle, float* w, float* C_fine, void* stream);

/* nerf_hip_coarse_composite that also stores each ray's coarse depth and opacity (D_c = sum_i w_i t_c,i, A_c = sum_i w_i) to
 * columns 0, 1 of maps [B,4] (required; columns 2, 3 untouched): the k_coarse_maps launch of nerf_hip_forward_maps. */
int nerf_hip_coarse_composite_maps(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                   float delta0, int B, int Nc, int Nf, float* w_c, float* C_coarse, float* t_f,
                                   uint32_t* status, float* maps, void* stream);

/* nerf_hip_coarse_composite_backward with the optional upstream gradient of the maps: dmaps [B,4] (columns 0, 1 = d loss/d D_c,
 * d loss/d A_c are read; may be NULL, then this is nerf_hip_coarse_composite_backward).  ADDS to dsig_c / drgb_c like it. */
int nerf_hip_coarse_composite_backward_maps(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                            float delta0, int B, int Nc, int Nf, const float* dC_coarse, const float* dt_f,
                                            const float* dmaps, float* dsig_c, float* drgb_c, void* stream);

/* The TRAINING form of nerf_hip_merge_composite, as nerf_hip_forward launches it with NERF_HIP_SAVE_FOR_BACKWARD: the five channel
 * sorts carry each value's original slot (0..Nc-1 coarse, Nc..Nc+Nf-1 fine), which makes them stable, and
 * perm [B,5,Nc+Nf] u16 (required) receives, per channel (0 = t, 1..3 = rgb, 4 = sigma), sorted position -> original slot.
 * The order is torch.sort's: -0 == +0, every NaN last.  joint != 0 (NERF_HIP_CORRECTED): ONE stable sort by depth moves all five
 * channels; perm then holds that permutation five times.  maps [B,4] (may be NULL): columns 2, 3 receive the fine depth and opacity
 * D_f = sum_k w_k t_s,k, A_f = sum_k w_k over the sorted channels.  bundle and w may be NULL.  Nc >= 1, Nf >= 1, Nc + Nf <= 2048. */
int nerf_hip_merge_composite_train(const float* t_c, const float* t_f, const float* sigma_c, const float* sigma_f,
                                   const float* rgb_c, const float* rgb_f, int B, int Nc, int Nf, float last_delta,
                                   float* bundle, float* w, float* C_fine, uint16_t* perm, int joint, float* maps, void* stream);

/* The stage entries of nerf_hip_forward_quantiles (rule QD above; q / nq / qdepth [B,2,nq] and their refusals as there, maps required).
 * nerf_hip_coarse_composite_quantiles: the arguments of nerf_hip_coarse_composite_maps, then q, nq, qdepth -- the k_coarse_qmaps launch;
 * every output it shares with nerf_hip_coarse_composite_maps has that call's bits, and row 0 of qdepth is written (row 1 untouched).  With
 * delta0 given, Nc = 1 is accepted here (a one-sample ray: Q = t_0).
 * nerf_hip_merge_composite_quantiles: the arguments of nerf_hip_merge_composite_train, then q, nq, qdepth -- the k_merge_qmaps launch;
 * shared outputs as that call's, row 1 of qdepth written (row 0 untouched).  perm may be NULL when joint == 0: the values-only sort of
 * inference (the same bundle, weights, colour and maps). */
int nerf_hip_coarse_composite_quantiles(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                        float delta0, int B, int Nc, int Nf, float* w_c, float* C_coarse, float* t_f,
                                        uint32_t* status, float* maps, void* stream, const float* q, int nq, float* qdepth);
int nerf_hip_merge_composite_quantiles(const float* t_c, const float* t_f, const float* sigma_c, const float* sigma_f,
                                       const float* rgb_c, const float* rgb_f, int B, int Nc, int Nf, float last_delta,
                                       float* bundle, float* w, float* C_fine, uint16_t* perm, int joint, float* maps, void* stream,
                                       const float* q, int nq, float* qdepth);

/* Backward of the merged composite and the channel sorts (autograd through nerf.py:302-321): in the sorted bundle [B,Nc+Nf,5] and
 * perm [B,5,Nc+Nf] of nerf_hip_merge_composite_train, dC_fine [B,3] and the optional dmaps [B,4] (columns 2, 3 = d loss/d D_f,
 * d loss/d A_f are read; may be NULL).  WRITES every element of dsig_c [B,Nc], dsig_f [B,Nf], drgb_c [B,Nc,3], drgb_f [B,Nf,3]
 * (un-sorted through each channel's own permutation) and dt_f [B,Nf] (through the sorted deltas; t_coarse carries no gradient).
 * perm must hold a permutation of 0..Nc+Nf-1 per channel: a repeated slot leaves another unwritten.  Sizes as the forward's. */
int nerf_hip_merge_composite_backward(const float* bundle, const uint16_t* perm, const float* dC_fine, const float* dmaps,
                                      int B, int Nc, int Nf, float last_delta, float* dsig_c, float* dsig_f, float* drgb_c,
                                      float* drgb_f, float* dt_f, void* stream);

/* The stage entries of nerf_hip_forward_distortion_train / nerf_hip_backward_distortion (rule DL above); near_far [B,2] = each ray's
 * (near, far), dist / ddist [B,2] = (L_c, L_f) / their upstream, all device and required.
 * nerf_hip_coarse_composite_distortion: the arguments of nerf_hip_coarse_composite_maps, then dist -- the k_coarse_dmaps launch; every
 * shared output has that call's bits, column 0 of dist is written (column 1 untouched).
 * nerf_hip_merge_composite_distortion: the arguments of nerf_hip_merge_composite_train (maps required here), then near_far, dist -- the
 * k_merge_dmaps launch; shared outputs as that call's, column 1 of dist written (column 0 untouched).
 * nerf_hip_coarse_composite_backward_distortion: the arguments of nerf_hip_coarse_composite_backward_maps, then ddist (column 0 is
 * read).  ADDS to dsig_c / drgb_c like the call it extends; with ddist = 0 it adds that call's values.
 * nerf_hip_merge_composite_backward_distortion: the arguments of nerf_hip_merge_composite_backward, then near_far, ddist (column 1 is
 * read).  WRITES every element like the call it extends; with ddist = 0 its values. */
int nerf_hip_coarse_composite_distortion(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                         float delta0, int B, int Nc, int Nf, float* w_c, float* C_coarse, float* t_f,
                                         uint32_t* status, float* maps, void* stream, float* dist);
int nerf_hip_merge_composite_distortion(const float* t_c, const float* t_f, const float* sigma_c, const float* sigma_f,
                                        const float* rgb_c, const float* rgb_f, int B, int Nc, int Nf, float last_delta,
                                        float* bundle, float* w, float* C_fine, uint16_t* perm, int joint, float* maps, void* stream,
                                        const float* near_far, float* dist);
int nerf_hip_coarse_composite_backward_distortion(const float* t_c, const float* sigma_c, const float* rgb_c, const float* near_far,
                                                  float delta0, int B, int Nc, int Nf, const float* dC_coarse, const float* dt_f,
                                                  const float* dmaps, float* dsig_c, float* drgb_c, void* stream, const float* ddist);
int nerf_hip_merge_composite_backward_distortion(const float* bundle, const uint16_t* perm, const float* dC_fine, const float* dmaps,
                                                 int B, int Nc, int Nf, float last_delta, float* dsig_c, float* dsig_f, float* drgb_c,
                                                 float* drgb_f, float* dt_f, void* stream, const float* near_far, const float* ddist);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  SH radiance volumes: the field baked onto a dense lattice -- sigma and a few real
 * spherical-harmonic colour coefficients per lattice point -- and a ray-marcher with trilinear lookups that renders from it without
 * the network.  An approximate product of its own: nothing of nerf_hip_forward / nerf_hip_query changes.
 *
 * The lattice is nerf_hip_density_grid's: nx, ny, nz >= 2 points (at least one cell per axis), nx * ny * nz < 2^31, point (i, j, k) at
 * lo + (i, j, k) * step, each coordinate one fp32 product and one fp32 sum, linear index (i * ny + j) * nz + k.  Arrays:
 *    sigma [nx][ny][nz]            fp32
 *    coef  [nx][ny][nz][ncoef][3]  fp32, ncoef = (degree + 1)^2 with degree in {0, 1, 2}: a corner is one contiguous 12 ncoef bytes
 *    occ   [bx][by][bz]            uint8, b_a = ceil((n_a - 1) / B) blocks of B cells per axis
 * sigma and coef are separate arrays: empty space touches only occ and sigma.  All arithmetic is fp32, every product, sum and division
 * rounded on its own, evaluated as bracketed; every comparison is false on NaN.
 *
 * VA. ACTIVE POINTS.  A lattice point is ACTIVE iff some point of its 3 x 3 x 3 neighbourhood, clipped to the lattice, has sigma > 0:
 *    exactly the points that are a corner of a cell with a positive corner, i.e. the points whose coefficients a lookup with
 *    sigma_s > 0 can read.  nerf_hip_volume_active_count / _emit give their number and their linear indices ASCENDING, through a scan
 *    -- no atomic places anything.  nerf_hip_volume_points writes the world point of each index of a list (any chunk of it) by the
 *    lattice rule above; an index outside [0, nx ny nz) gives the point (NaN, NaN, NaN).
 *
 * VS. SH PROJECTION.  The basis is the 9 real spherical harmonics of degree <= 2 in the order (l, m) ascending, m = -l .. l, without
 *    the Condon-Shortley sign: for d = (x, y, z)
 *       Y_0 = C0             Y_1 = C1 y           Y_2 = C1 z                       Y_3 = C1 x          Y_4 = C2 (x y)
 *       Y_5 = C2 (y z)       Y_6 = C3 ((3 (z z)) - 1)                              Y_7 = C2 (x z)      Y_8 = C4 ((x x) - (y y))
 *    with C0 .. C4 = fp32(sqrt(1 / 4 pi)), fp32(sqrt(3 / 4 pi)), fp32(sqrt(15 / 4 pi)), fp32(sqrt(5 / 16 pi)), fp32(sqrt(15 / 16 pi))
 *    = 0.282094806, 0.488602519, 1.09254849, 0.31539157, 0.546274245 (NERF_HIP_VOLUME_SH_C).  The quadrature is the 12 vertices of the
 *    icosahedron, all weights w = 4 pi / 12: with phi = (1 + sqrt 5) / 2, vertex 4 c + 2 s1 + s2 (c = 0, 1, 2; s1, s2 = 0 for +, 1
 *    for -) has component c equal to 0, component (c + 1) % 3 equal to +-1 (s1) and component (c + 2) % 3 equal to +-phi (s2), divided
 *    by sqrt(1 + phi^2) in fp64 and rounded to fp32: NERF_HIP_VOLUME_DIRS below.  They form a spherical 5-design, so the products of
 *    two basis functions are integrated exactly: sum_k w Y_i(d_k) Y_j(d_k) = delta_ij (1.5e-7 with these fp32 directions).
 *    The bake: for k = 0 .. 11 IN ORDER, rgb_k = nerf_hip_query(the active points, dirs = d_k), and nerf_hip_volume_sh_accumulate(k)
 *       coef[p][m][ch] = coef[p][m][ch] + b_km * rgb_k[p][ch]          m < ncoef
 *    b_km = fp32(w Y_m(d_k)) with Y_m evaluated in fp64 with the unrounded constants at the fp32 direction widened; zero entries are
 *    +0 (NERF_HIP_VOLUME_SH_B, which nerf_hip_volume_sh_table returns beside the directions).  The caller zeroes coef before k = 0;
 *    inactive points keep 0.  The first (degree + 1)^2 coefficients do not depend on the degree: a lower-degree bake is the leading
 *    slab of the degree-2 bake, bit for bit.  An index outside the lattice is skipped.
 *
 * VO. BLOCK OCCUPANCY.  Block b of edge B (an int >= 1) covers the cells [b B, min((b + 1) B, n - 1)) per axis; occ[b] = 1 iff some
 *    lattice point touched by one of its cells -- the points b B .. min((b + 1) B, n - 1) per axis, both ends included -- has
 *    sigma > 0, else 0.  B >= every n - 1 gives one block.
 *
 * VL. LOOKUP at the point x along the direction d.  Per axis a
 *       g = (x - lo) / step          INSIDE iff 0 <= g and g <= n - 1 (on every axis; false on NaN, so a point that is not finite is outside)
 *       i = min(max(floor(g), 0), n - 2)          f = g - i
 *    An outside point has sigma_s = 0 and rgb = 0.  Otherwise, with v[di][dj][dk] the value at corner (i + di, j + dj, k + dk) and
 *    lerp(a, b, f) = a + (f * (b - a)), the z axis is interpolated first, then y, then x:
 *       c[di][dj] = lerp(v[di][dj][0], v[di][dj][1], fz),   c[di] = lerp(c[di][0], c[di][1], fy),   value = lerp(c[0], c[1], fx)
 *    sigma_s is that value of sigma.  The colour: each corner's channel value is s = Y_0(d) coef[corner][0][ch], then
 *    s = s + (Y_m(d) coef[corner][m][ch]) for m = 1 .. ncoef - 1, with Y_m(d) as in VS in fp32 and d AS GIVEN (not renormalised);
 *    the eight values are interpolated like sigma and the result is clamped, rgb = fmin(fmax(value, 0), 1) (a NaN becomes 0).
 *
 * VR. THE MARCH.  Per ray (o, d), window [tmin, tmax] and step dt > 0.  A ray whose o, d, tmin or tmax is not finite MISSES.  Else
 *    t_a = tmin, t_b = tmax and per axis, with the box [lo, hi], hi = lo + (n - 1) * step (the last lattice point):
 *       d == 0:  the ray misses unless lo <= o and o <= hi; nothing else is computed (no 0 * inf)
 *       else     t1 = (lo - o) / d, t2 = (hi - o) / d, t_a = fmax(t_a, fmin(t1, t2)), t_b = fmin(t_b, fmax(t1, t2))
 *    (x, y, z in turn).  !(t_a < t_b) is a miss.  K = min(ceil((t_b - t_a) / dt), NERF_HIP_VOLUME_MAX_STEPS), compared in fp32
 *    before it becomes an integer.  Sample k = 0 .. K - 1 sits at t_k = t_a + ((float(k) + 0.5) * dt), its point is o + (t_k * d) per
 *    axis, and VL gives (sigma_s, rgb) there along d.  A sample CONTRIBUTES iff sigma_s > 0.  From T = 1, C = D = A = 0:
 *       alpha = -expm1f(-(sigma_s * dt))        (the accurate library function)
 *       w = T * alpha,   C_ch = C_ch + (w * rgb_ch),   D = D + (w * t_k),   A = A + w,   T = T - w
 *    and after the update of a contributing sample the march ends when T < t_stop (t_stop in [0, 1); 0 never ends early).
 *       rgb_ch = C_ch + ((1 - A) * background_ch),   maps = (D, A),   steps = (contributing samples, evaluated samples)  int32
 *    d is the renderer's unit d_wrd, so D is on the depth scale of nerf_hip_forward_maps.  A miss gives the background, zero maps and
 *    zero steps.
 *    EMPTY BLOCKS.  The marcher may pass over samples that lie in a block with occ = 0 (csrc/volume.hip proves that none of them can
 *    contribute): rgb, maps and steps[0] do not depend on B, bit for bit; only steps[1], the samples it looked at, does.
 *
 * One thread per item everywhere; the march is one ray per lane, no LDS, no atomics.  The data-dependent addresses are the eight
 * corners and the block byte, each built from indices clamped into their arrays.  All calls are enqueue-only on the caller's stream
 * and check every argument on the host first (NERF_HIP_ERR_ARG): a dimension < 2, nx * ny * nz >= 2^31, degree outside {0, 1, 2},
 * block < 1, a lo that is not finite, a step that is not finite and > 0, dt not finite and > 0, t_stop outside [0, 1), a background
 * that is not finite, k outside [0, 12), a negative count or one >= 2^31, a NULL pointer or one that is not aligned to its element.
 * A count of 0 succeeds and launches nothing (its per-item pointers may then be NULL).  lo3 / step3 / background3 are HOST arrays.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_VOLUME_MAX_STEPS 65536 /* the cap on K: the march is bounded whatever the inputs; (k + 0.5) stays exact in fp32 */
#define NERF_HIP_VOLUME_NDIRS 12
#define NERF_HIP_VOLUME_SH_C {0.282094806f, 0.488602519f, 1.09254849f, 0.31539157f, 0.546274245f}
#define NERF_HIP_VOLUME_DIRS {                                                                      \
    0.0f, 0.525731087f, 0.850650787f,    0.0f, 0.525731087f, -0.850650787f,                         \
    0.0f, -0.525731087f, 0.850650787f,   0.0f, -0.525731087f, -0.850650787f,                        \
    0.850650787f, 0.0f, 0.525731087f,    -0.850650787f, 0.0f, 0.525731087f,                         \
    0.850650787f, 0.0f, -0.525731087f,   -0.850650787f, 0.0f, -0.525731087f,                        \
    0.525731087f, 0.850650787f, 0.0f,    0.525731087f, -0.850650787f, 0.0f,                         \
    -0.525731087f, 0.850650787f, 0.0f,   -0.525731087f, -0.850650787f, 0.0f}
#define NERF_HIP_VOLUME_SH_B {                                                                                                    \
    0.295408964f, 0.268997341f, 0.435246825f, 0.0f, 0.0f, 0.511663318f, 0.386695325f, 0.0f, -0.15811266f,                          \
    0.295408964f, 0.268997341f, -0.435246825f, 0.0f, 0.0f, -0.511663318f, 0.386695325f, 0.0f, -0.15811266f,                        \
    0.295408964f, -0.268997341f, 0.435246825f, 0.0f, 0.0f, -0.511663318f, 0.386695325f, 0.0f, -0.15811266f,                        \
    0.295408964f, -0.268997341f, -0.435246825f, 0.0f, 0.0f, 0.511663318f, 0.386695325f, 0.0f, -0.15811266f,                        \
    0.295408964f, 0.0f, 0.268997341f, 0.435246825f, 0.0f, 0.0f, -0.0564181209f, 0.511663318f, 0.413944334f,                        \
    0.295408964f, 0.0f, 0.268997341f, -0.435246825f, 0.0f, 0.0f, -0.0564181209f, -0.511663318f, 0.413944334f,                      \
    0.295408964f, 0.0f, -0.268997341f, 0.435246825f, 0.0f, 0.0f, -0.0564181209f, -0.511663318f, 0.413944334f,                      \
    0.295408964f, 0.0f, -0.268997341f, -0.435246825f, 0.0f, 0.0f, -0.0564181209f, 0.511663318f, 0.413944334f,                      \
    0.295408964f, 0.435246825f, 0.0f, 0.268997341f, 0.511663318f, 0.0f, -0.330277264f, 0.0f, -0.255831659f,                        \
    0.295408964f, -0.435246825f, 0.0f, 0.268997341f, -0.511663318f, 0.0f, -0.330277264f, 0.0f, -0.255831659f,                      \
    0.295408964f, 0.435246825f, 0.0f, -0.268997341f, -0.511663318f, 0.0f, -0.330277264f, 0.0f, -0.255831659f,                      \
    0.295408964f, -0.435246825f, 0.0f, -0.268997341f, 0.511663318f, 0.0f, -0.330277264f, 0.0f, -0.255831659f}

/* dirs36 [12][3] and b108 [12][9]: the two tables above (HOST arrays; either may be NULL).  Host only. */
int nerf_hip_volume_sh_table(float* dirs36, float* b108);

/* Bytes of workspace (256-byte aligned) of nerf_hip_volume_active_count / _emit: 8 bytes per 2048 lattice points and one count. */
int nerf_hip_volume_ws_bytes(int nx, int ny, int nz, size_t* bytes);

/* VA: count[0] (int64, device, 8-byte aligned) = the active points of sigma. */
int nerf_hip_volume_active_count(const float* sigma, int nx, int ny, int nz, void* ws, size_t ws_bytes, int64_t* count, void* stream);

/* VA: index[0 .. min(count, max_n)) = the active points' linear indices, ascending.  Needs no count call before it. */
int nerf_hip_volume_active_emit(const float* sigma, int nx, int ny, int nz, void* ws, size_t ws_bytes, int32_t* index, int64_t max_n,
                                void* stream);

/* VA: points[n][3] = the lattice points of index[0 .. n). */
int nerf_hip_volume_points(const int32_t* index, int64_t n, int nx, int ny, int nz, const float* lo3, const float* step3, float* points,
                           void* stream);

/* VS: direction k's term added to the coefficients of the points index[0 .. n); rgb[n][3] is nerf_hip_query's at those points along
 * d_k.  The indices of one call must be distinct (an active list's are): every point is updated by one thread. */
int nerf_hip_volume_sh_accumulate(float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n, const float* rgb, int k,
                                  void* stream);

/* VO: occ[bx][by][bz] of sigma for blocks of edge `block`; every byte is written. */
int nerf_hip_volume_blocks(const float* sigma, int nx, int ny, int nz, int block, uint8_t* occ, void* stream);

/* VL: out_sigma[M], out_rgb[M][3] at points[M][3] along dirs[M][3]. */
int nerf_hip_volume_sample(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const float* lo3, const float* step3,
                           const float* points, const float* dirs, int64_t M, float* out_sigma, float* out_rgb, void* stream);

/* VR: origins, dirs [N][3], tmin, tmax [N] (device) -> rgb[N][3], maps[N][2] fp32, steps[N][2] int32.  occ is VO's for `block`. */
int nerf_hip_volume_render(const float* sigma, const float* coef, const uint8_t* occ, int nx, int ny, int nz, int degree, int block,
                           const float* lo3, const float* step3, const float* origins, const float* dirs, const float* tmin,
                           const float* tmax, int64_t N, float dt, float t_stop, const float* background3, float* rgb, float* maps,
                           int32_t* steps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Fine-tuning a baked volume: the gradient of the march with respect to sigma and the
 * coefficients, accumulated exactly, and an Adam step over the baked active list.  Nothing of the calls above changes.
 *
 * VG. THE GRADIENT OF THE MARCH.  For one ray take i = 1 .. n over the contributing samples of rule VR, in order.  The early end at
 *    T < t_stop is a constant: no gradient flows through the decision.  Sample i has alpha_i, w_i, T_(i+1) (T after sample i), c_i (the
 *    clamped colour) and t_i, all the forward's own fp32 values.  Upstream: g_rgb[3] and g_maps = (gD, gA), (0, 0) when NULL.  From
 *    here on everything is fp64 (the fp32 values widened), evaluated as bracketed:
 *       gA' = gA - (((g_rgb[0] bg[0]) + (g_rgb[1] bg[1])) + (g_rgb[2] bg[2]))
 *       v_i = ((((g_rgb[0] c_i[0]) + (g_rgb[1] c_i[1])) + (g_rgb[2] c_i[2])) + (gD t_i)) + gA'
 *       P_i = P_(i-1) + (w_i v_i)   (P_0 = 0),    S = P_n
 *       dL/dsigma_s,i = dt (((T_(i+1)) v_i) - (S - P_i))                 (no division: alpha -> 1 is harmless)
 *       dL/dc_i[ch]   = w_i g_rgb[ch] where the UNCLAMPED colour of rule VL lies in [0, 1], both ends included (what a clamp
 *                       passes); 0 elsewhere (a NaN included)
 *    Corner c = (di, dj, dk) of the sample's cell has the weight tw_c = (wx wy) wz with w_a = f_a for d_a = 1 and 1 - f_a for d_a = 0,
 *    f the fp32 f of rule VL widened.  It receives
 *       (tw_c) (dL/dsigma_s,i)                   into its sigma word
 *       ((tw_c) (Y_m(d))) (dL/dc_i[ch])          into its coefficient word (m, ch), Y_m(d) rule VL's fp32 value widened
 *    Each contribution x is added as llrint(y), y = x 2^40 (NERF_HIP_VOLUME_GRAD_SHIFT) clamped to [-2^62, 2^62] (a NaN adds 0), into
 *    two int64 arrays with the shapes of sigma and coef: the conversion is never undefined, the sums are integers, and the result
 *    does not depend on the order in which the contributions arrive -- bit for bit whatever the launch, the batch split, the ray
 *    order or the block edge.  A contribution that rounds to 0 may be left out.  Misses add nothing; a ray whose upstream values
 *    (g_rgb, and g_maps when given) are not all finite adds nothing.
 *    OVERFLOW PRECONDITION.  Between two reads of a word the sum of |x| it receives stays below 2^22 (then |sum| < 2^62 < 2^63).
 *    Every |tw Y_m| < 1.1 and |dL/dc| <= |g|, so with |g| <= 2 that is about two million full-magnitude contributions to one word.
 *
 * VU. THE UPDATE over index[n], the ascending active list (rule VA) of the volume AS BAKED, one thread per (active point, word);
 *    a point's words are its sigma and its 3 ncoef coefficients, m and v are [n][1 + 3 ncoef] fp32 in that order.  Per word, with acc
 *    its accumulator, lr = lr_sigma or lr_coef, everything fp64 as bracketed and rounded to fp32 ONCE where fp32() says so:
 *       g  = (double(acc) 2^-40) grad_scale
 *       m' = fp32((beta1 m) + ((1 - beta1) g)),    v' = fp32((beta2 v) + ((1 - beta2) (g g)))
 *       x' = fp32(x - (lr ((m' / c1) / (sqrt(v' / c2) + eps))))         c1 = 1 - beta1^step,  c2 = 1 - beta2^step
 *    beta^step is formed on the host in fp64 by squaring: p = 1, b = beta, e = step; while e > 0: (e odd: p = p b), b = b b, e = e / 2.
 *    The accumulator word is zeroed whatever happens: no memset is needed between steps.  An index outside the lattice is skipped.
 *    FROZEN SUPPORT (the rule's invariant).  A sigma word is updated only while sigma > 0 at entry and is then clamped,
 *    sigma' = fmax(x', 0); a point that is not > 0 is DEAD: its x, m and v are left alone (its coefficient words are updated like any
 *    other).  The positive set can therefore only shrink: every corner a contributing sample reads stays inside the baked active
 *    list, the baked occ stays a valid superset of rule VO's, and accumulators outside the list stay zero.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_VOLUME_GRAD_SHIFT 40

/* VG over the rays of nerf_hip_volume_render (its arguments, no outputs): g_rgb[N][3], g_maps[N][2] or NULL (device, fp32) ->
 * contributions ADDED IN PLACE to acc_sigma [nx][ny][nz] and acc_coef [nx][ny][nz][ncoef][3] (device, int64, 8-byte aligned).  The
 * kernel recomputes the march; nothing is taken from a forward call. */
int nerf_hip_volume_render_backward(const float* sigma, const float* coef, const uint8_t* occ, int nx, int ny, int nz, int degree,
                                    int block, const float* lo3, const float* step3, const float* origins, const float* dirs,
                                    const float* tmin, const float* tmax, int64_t N, float dt, float t_stop, const float* background3,
                                    const float* g_rgb, const float* g_maps, int64_t* acc_sigma, int64_t* acc_coef, void* stream);

/* VU.  step >= 1; grad_scale, the rates, beta1, beta2 in [0, 1) and eps >= 0 finite.  n = 0 succeeds and launches nothing. */
int nerf_hip_volume_adam_step(float* sigma, float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                              int64_t* acc_sigma, int64_t* acc_coef, float* m, float* v, double grad_scale, int64_t step,
                              double lr_sigma, double lr_coef, double beta1, double beta2, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Coarse-to-fine fine-tuning: a total-variation prior over a level's active list, added to
 * rule VG's accumulators; the x2 refinement of the lattice; pruning.  Nothing of the calls above changes.  A refined or pruned volume
 * is fine-tuned with a NEW active list and new moments, so rule VU's frozen-support invariant holds level by level.
 *
 * VM. MEMBER MASK.  member[nx][ny][nz] uint8: 1 at the lattice points of index[n], 0 elsewhere.  Every byte is written; an index outside
 *    the lattice is skipped.  The mask is the membership test of the active list AS BAKED FOR THIS LEVEL, not a test of the current
 *    sigma: the positive set shrinks while training (rule VU), the list does not.
 *
 * VT. TOTAL VARIATION OVER THE MEMBERS, added to rule VG's accumulators.  A WORD is sigma or one coefficient (m, ch).  Everything is
 *    fp64 on the fp32 values widened, evaluated as bracketed.  For a member p, a word x and an axis a, with e_a the axis' unit step:
 *       d_a(p) = x(p + e_a) - x(p)    if p + e_a lies inside the lattice AND is a member,    else 0
 *       tau(p) = sqrt((((d_x d_x) + (d_y d_y)) + (d_z d_z)) + eps)
 *       Q_a(p) = llrint(y),  y = (w (d_a(p) / tau(p))) 2^40 clamped to [-2^62, 2^62]    (a NaN gives 0; rule VG's fixed point)
 *    with w = w_sigma for the sigma word and w_coef for a coefficient word.  The accumulator word of p receives -Q_a(p) and the one of
 *    p + e_a receives +Q_a(p), as INTEGER adds: the gradient of w sum_(p member) tau(p), one word's terms summed.  A difference whose
 *    far end is outside the lattice or not a member is the CONSTANT 0, so
 *       - a point that is not a member receives nothing: rule VU's "accumulators outside the list stay zero" survives;
 *       - the loss is a function of the members' values alone;
 *       - the integers one call adds to the words of one type (sigma, or one (m, ch)) sum to exactly 0 over the lattice.
 *    One thread per (entry of index[n], word) GATHERS: its own three Q_a(q), and Q_a(q - e_a) for every axis on which q - e_a lies inside
 *    the lattice and is a member (that point's tau is recomputed); then one plain read-modify-write of its own accumulator word.  No
 *    atomic, no LDS, no dependence on the launch order.  The indices of one call must be distinct (an active list's are); index[n]
 *    may be any chunk of the level's list, member is the mask of the WHOLE list; an entry that is outside the lattice or not a member is
 *    skipped.  A dead sigma word (sigma not > 0) receives its terms like any other; rule VU ignores and zeroes them.
 *    OVERFLOW PRECONDITION.  |d_a / tau| <= 1, so a word receives at most six terms of magnitude <= w <= 2^16 per call: within rule VG's.
 *
 * VX. x2 REFINEMENT.  The new lattice has 2 n - 1 points per axis over the same box: lo' = lo, step' = step * 0.5f (exact).  Per axis
 *       U(v)[2 i]     = v[i]                                  (taken as it is: no arithmetic, the bits are kept)
 *       U(v)[2 i + 1] = v[i] + (0.5f * (v[i + 1] - v[i]))     (rule VL's lerp at f = 0.5, fp32)
 *    applied along z first, then y, then x, to sigma and to every coefficient word.  One thread per (new point, word) gathers the at
 *    most eight coarse values and interpolates only along the axes whose new index is odd: bit for bit the three separable passes.
 *    sigma' >= 0 wherever sigma >= 0; rule VA's active set of sigma' is the refined support and contains every coarse active point's
 *    image.  A fine point between a coarse active point and an inactive one can lie outside it and still hold half a coefficient: no
 *    contributing sample reads it, and rule VP at threshold 0 clears it.  (2 nx - 1)(2 ny - 1)(2 nz - 1) >= 2^31 is refused.
 *
 * VP. PRUNE, in place, two stream-ordered kernels.  First, pointwise,
 *       sigma'(p) = sigma(p)  if sigma(p) > threshold (false on NaN),    +0 otherwise
 *    then every coefficient word of a point that is not active (rule VA) in sigma' becomes +0; the others keep their bits.
 *    threshold is finite and >= 0; threshold = 0 clears only stale coefficients (and a NaN or negative sigma).
 *
 * All four are enqueue-only and check every argument on the host first (NERF_HIP_ERR_ARG), as the calls above: the lattice, the degree,
 * a negative count or one >= 2^31, eps not finite or not > 0, a weight that is not finite, < 0 or > 2^16, a threshold that is not
 * finite or < 0, a NULL pointer or one that is not aligned to its element.  n = 0, or both weights 0, succeeds and launches no kernel
 * of rule VT.  Data-dependent addresses are built only from indices already compared with the size of their array.
 * ------------------------------------------------------------------------------------------- */

/* VM: member[nx][ny][nz] (device, uint8) of index[0 .. n). */
int nerf_hip_volume_member_mask(const int32_t* index, int64_t n, int nx, int ny, int nz, uint8_t* member, void* stream);

/* VT over index[0 .. n) with the mask of the whole list: the terms are ADDED IN PLACE to rule VG's accumulators. */
int nerf_hip_volume_tv_backward(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                                const uint8_t* member, double w_sigma, double w_coef, double eps, int64_t* acc_sigma, int64_t* acc_coef,
                                void* stream);

/* VX: sigma2 [2 nx - 1][2 ny - 1][2 nz - 1], coef2 [..][ncoef][3] (device; they do not overlap the inputs). */
int nerf_hip_volume_upsample(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, float* sigma2, float* coef2,
                             void* stream);

/* VP, in place. */
int nerf_hip_volume_prune(float* sigma, float* coef, int nx, int ny, int nz, int degree, float threshold, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Compact volumes: the deployment form of a volume.  Only the rows of the ACTIVE lattice
 * points (rule VA) are stored, behind an int32 slot lattice; the coefficients are fp32 or fp16.  Nothing of the calls above changes.
 *
 * VC. THE COMPACT FORM of a dense volume (sigma, coef) on the lattice nx x ny x nz whose ascending active list (rule VA) is index[n],
 *    ncoef = (degree + 1)^2:
 *       slot[nx][ny][nz]  int32: r at the lattice point index[r], -1 everywhere else -- a slot is the point's rank in rule VA's list;
 *       sigma_rows[n]     fp32:  sigma_rows[r] = sigma[index[r]], bit for bit;
 *       coef_rows[n][S]   half = 0: fp32, S = 3 ncoef, the dense row's words in the dense order (m-major, channel fastest);
 *                         half = 1: fp16, S = 3 ncoef rounded up to a multiple of 4 (4 / 12 / 28 for degree 0 / 1 / 2); every half is
 *                         the round-to-nearest-even fp16 of the fp32 word (a finite value past 65504 becomes +-inf, a NaN stays a
 *                         NaN), the pad halves are +0; every row starts on an 8-byte boundary and is read in 8-byte words;
 *       occ, lo, step, block, degree as in the dense form; occ is rule VO's occupancy of the dense sigma.
 *    PACK gathers the rows of index[n] from dense arrays (one thread per row word; an index outside the lattice gives a +0 row); with
 *    index = NULL the rows are the lattice's points in order (n = nx ny nz): the conversion of fp32 rows to fp16 rows.  UNPACK
 *    scatters rows to the points index[n] of dense arrays THE CALLER HAS ZEROED, fp16 widened (exact); an index outside the lattice
 *    is skipped.  SLOTS fills the lattice with -1 and stores r at index[r] (distinct indices; one outside the lattice is skipped).
 *
 *    VC-L. LOOKUP: rule VL with each corner's values taken through its slot.  A corner with slot < 0 or slot >= n has sigma +0 and
 *    an all-zero coefficient row -- a slot outside [0, n) is never turned into an address; any other corner has sigma_rows[slot] and
 *    the row coef_rows[slot], an fp16 row widened to fp32 word by word.  Everything after that is rule VL's fp32 arithmetic in rule
 *    VL's order (a zero row goes through the same products and sums).
 *    VC-R. MARCH: rule VR over VC-L, the passing over of empty blocks included.
 *
 *    EQUIVALENCE (proved in csrc/volume_compact.hip).  With U the dense volume that holds a compact volume's rows at the points whose
 *    slot lies in [0, n) and +0 elsewhere, VC-L equals VL on U and VC-R equals VR on U, bit for bit.  For ANY dense volume V -- garbage
 *    at its inactive points included: negative sigma, -0, NaN, non-zero coefficients -- rgb, maps and both columns of steps of VC-R on
 *    the fp32 pack of V equal rule VR on V bit for bit, and those of the fp16 pack equal rule VR on V with every coefficient replaced
 *    by fp32(fp16(.)).
 *
 * All five are enqueue-only and check every argument on the host first (NERF_HIP_ERR_ARG) as the calls above do, and in addition
 * half outside {0, 1}, n outside [0, nx ny nz], and fp16 coef_rows that are not 8-byte aligned.  n = 0 is legal: the row pointers may
 * then be NULL, every corner is inactive, sample gives zeros and render the background with zero maps.
 * ------------------------------------------------------------------------------------------- */

/* VC's slot[nx][ny][nz] (device, int32) of the active list index[0 .. n). */
int nerf_hip_volume_compact_slots(const int32_t* index, int64_t n, int nx, int ny, int nz, int32_t* slot, void* stream);

/* VC's PACK: dense (sigma, coef) -> sigma_rows[n], coef_rows[n][S] (device).  index may be NULL (the identity; then n = nx ny nz);
 * sigma and sigma_rows may both be NULL to convert the coefficients only. */
int nerf_hip_volume_compact_pack(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                                 int half, float* sigma_rows, void* coef_rows, void* stream);

/* VC's UNPACK into dense arrays the caller has zeroed.  coef_rows and coef may both be NULL to scatter sigma only. */
int nerf_hip_volume_compact_unpack(const float* sigma_rows, const void* coef_rows, int half, const int32_t* index, int64_t n, int nx, int ny,
                                   int nz, int degree, float* sigma, float* coef, void* stream);

/* VC-L at points[M][3] along dirs[M][3] -> out_sigma[M], out_rgb[M][3] (device, fp32), as nerf_hip_volume_sample. */
int nerf_hip_volume_compact_sample(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n, int half, int nx, int ny,
                                   int nz, int degree, const float* lo3, const float* step3, const float* points, const float* dirs,
                                   int64_t M, float* out_sigma, float* out_rgb, void* stream);

/* VC-R over N rays -> rgb[N][3], maps[N][2], steps[N][2], as nerf_hip_volume_render. */
int nerf_hip_volume_compact_render(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n, int half,
                                   const uint8_t* occ, int nx, int ny, int nz, int degree, int block, const float* lo3, const float* step3,
                                   const float* origins, const float* dirs, const float* tmin, const float* tmax, int64_t N, float dt,
                                   float t_stop, const float* background3, float* rgb, float* maps, int32_t* steps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Fine-tuning a compact volume: rules VG, VU and VT over the rows of a compact volume
 * whose coefficients are fp32 (half = 0).  The accumulators and the moments are kept PER ROW:
 *       acc_sigma_rows[n], acc_coef_rows[n][3 ncoef]   int64, 8-byte aligned, rule VG's fixed point (units of 2^-40);
 *       m, v [n][1 + 3 ncoef]                          fp32, a row's sigma word first, then its coefficient words.
 * Nothing of the calls above changes; the dense training calls keep taking the dense form only.
 *
 * VCG. THE GRADIENT OF THE COMPACT MARCH: rule VG over rule VC-R's march.  The contributing samples, alpha_i, w_i, T_(i+1), c_i, the
 *    unclamped colour and t_i are rule VC-R's own fp32 values; the fp64 brackets, the shift, the clamp to [-2^62, 2^62], misses and
 *    upstream values that are not finite adding nothing, and the overflow precondition are rule VG's, verbatim.  A corner of a
 *    contributing sample's cell whose slot r lies in [0, n) adds its contributions into the words of row r; a corner whose slot lies
 *    outside [0, n) receives nothing, and its slot is never turned into an address.
 *
 * VCU. THE UPDATE OVER ROWS: rule VU with the rows as the list, one thread per (row, word) -- no index list.  The word (r, 0) is
 *    sigma_rows[r], the word (r, 1 + j) is coef_rows[r][j]; the brackets, beta^step by squaring on the host, the FROZEN SUPPORT (a row
 *    whose sigma is not > 0 at entry is dead: its sigma word and that word's m and v are left alone) and the accumulator word being
 *    zeroed whatever happens are rule VU's.
 *
 * VCT. TOTAL VARIATION OVER ROWS: rule VT with the slot lattice as the membership test -- a lattice point is a member iff its slot lies
 *    in [0, n).  point[n] (int32) is the lattice point of each row; a row r whose point is -1, outside the lattice, not a member, or a
 *    member whose slot is not r is skipped (a point list that disagrees with the slots adds nothing for that row).
 *    One thread per (row, word) gathers its own three Q_a(q) and the up to three Q_a(q - e_a), a neighbour's value read
 *    through that neighbour's slot (compared with n first), then does one plain read-modify-write of its own accumulator word.
 *
 * EQUIVALENCE (proved in csrc/volume_compact_grad.hip).  Let the slots in [0, n) be distinct, U be the dense volume that holds the
 *    rows at the points with such a slot and +0 elsewhere, and index[r] the point whose slot is r.  After the same calls on zeroed
 *    accumulators, acc_*_rows[r] equals the dense accumulator word at index[r] bit for bit -- VCG against rule VG on U, VCT against
 *    rule VT on U with rule VM's mask of index -- and VCU leaves sigma_rows, coef_rows, m and v equal to rule VU's on U over index at
 *    those points.  If the compact volume is rule VC's PACK of ANY dense volume V (garbage at its inactive points included), rule VG
 *    on V adds nothing outside the active list and agrees with VCG inside it.  The sums are integers: the accumulators hold the same
 *    bits for the same call twice, for permuted rays, for a split batch and for every block edge.
 *
 * All three are enqueue-only and check every argument on the host first (NERF_HIP_ERR_ARG) as the calls above do: the lattice, the
 * degree, n outside [0, nx ny nz] (VCU: < 0 or >= 2^31), a NULL pointer or one that is not aligned to its element (the accumulators: 8
 * bytes), and the scalars as rules VG, VU and VT state them.  n = 0 succeeds and launches nothing (the row pointers may then be NULL),
 * as does N = 0 for VCG and both weights 0 for VCT.  Data-dependent addresses are built only from values already compared with the
 * size of their array.
 * ------------------------------------------------------------------------------------------- */

/* VCG over the rays of nerf_hip_volume_compact_render (its arguments without half -- the rows are fp32 -- and without outputs):
 * g_rgb[N][3], g_maps[N][2] or NULL (device, fp32) -> contributions ADDED IN PLACE to acc_sigma_rows[n] and acc_coef_rows[n][3 ncoef]. */
int nerf_hip_volume_compact_render_backward(const int32_t* slot, const float* sigma_rows, const float* coef_rows, int64_t n,
                                            const uint8_t* occ, int nx, int ny, int nz, int degree, int block, const float* lo3,
                                            const float* step3, const float* origins, const float* dirs, const float* tmin,
                                            const float* tmax, int64_t N, float dt, float t_stop, const float* background3,
                                            const float* g_rgb, const float* g_maps, int64_t* acc_sigma_rows, int64_t* acc_coef_rows,
                                            void* stream);

/* VCU.  The scalars are nerf_hip_volume_adam_step's. */
int nerf_hip_volume_compact_adam_step(float* sigma_rows, float* coef_rows, int64_t n, int degree, int64_t* acc_sigma_rows,
                                      int64_t* acc_coef_rows, float* m, float* v, double grad_scale, int64_t step, double lr_sigma,
                                      double lr_coef, double beta1, double beta2, double eps, void* stream);

/* VCT: the terms are ADDED IN PLACE to the rows' accumulators.  The weights lie in [0, 2^16], eps is finite and > 0. */
int nerf_hip_volume_compact_tv_backward(const int32_t* slot, const float* sigma_rows, const float* coef_rows, const int32_t* point,
                                        int64_t n, int nx, int ny, int nz, int degree, double w_sigma, double w_coef, double eps,
                                        int64_t* acc_sigma_rows, int64_t* acc_coef_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Vector-quantised compact volumes: a per-row importance from training rays, a k-means
 * codebook over the coefficient rows, and the decode of (class, code) back to rule VC's fp16 rows.  Nothing of the calls above
 * changes; the marchers keep reading rows -- the quantised form is a FILE form, decoded once after loading.
 *
 * VI. IMPORTANCE.  Rule VC-R's march, unchanged: the slab test, the samples t_k = t_a + (k + 0.5) dt, the passing over of empty
 *    blocks with its verification, alpha = -expm1f(-(sigma_s dt)), w = T alpha, T = T - w, the end once T < t_stop.  No coefficient
 *    row is read (the call takes none).  At each contributing sample, with (f_x, f_y, f_z) the cell's fp32 fractions and w the
 *    sample's fp32 weight (BEFORE T is updated), every corner c = di 4 + dj 2 + dk whose slot r lies in [0, n) receives
 *       imp_rows[r] += llrint( clamp( (((wx wy) wz) (double)w) 2^40, +-2^62 ) )
 *    where wx = f_x if di else 1 - f_x (likewise wy, wz), formed in fp64 from the fp32 fractions exactly as rule VG forms its corner
 *    terms; the units (NERF_HIP_VOLUME_GRAD_SHIFT) and the clamp are rule VG's.  The additions are int64 atomics: the sums hold the
 *    same bits whatever the order of the rays, the split of a batch or the block edge.  A corner whose slot lies outside [0, n)
 *    receives nothing and its slot is never turned into an address.  imp_rows belongs to the caller and is ADDED to.  steps[N][2]
 *    equals nerf_hip_volume_compact_render's bit for bit.  A row's sum stays below 2^62 for fewer than 2^22 contributing samples
 *    per row and call sequence at full weight; the caller's precondition, as rule VG's.
 *
 * VQ-A. ASSIGN.  rows[m][W] and codebook[K][W] are fp32, W = 3 ncoef, 1 <= K <= NERF_HIP_VOLUME_VQ_MAX_CODES.  For row q and code j
 *       d_j = (..((t_0 t_0) + t_1 t_1) + ..) + t_(W-1) t_(W-1),      t_w = q_w - c_jw
 *    in fp32, every difference, product and sum rounded on its own, in the order w = 0 .. W - 1.  assign[r] is the result of scanning
 *    j = 0 .. K - 1 with  "if (d_j < best) best = d_j, code = j"  from best = +inf, code = 0: the lowest index wins a tie, a NaN d_j
 *    never wins, and code 0 is the answer when nothing wins.  dist[r] (optional) is the final best (+inf when nothing won).
 *
 * VQ-U. UPDATE.  weight[m] is int64 with 0 <= weight[r] <= imax (rule VI's sums of the coded rows and their maximum);
 *    u_r = (double)weight[r] / (double)imax, and u_r = 1 when weight is NULL or imax = 0.  ACCUMULATE adds, for every row r whose
 *    assign[r] = j lies in [0, K) (any other value is skipped and never becomes an address),
 *       sum[j][w] += llrint( clamp( (u_r (double)q_rw) 2^20, +-2^62 ) )   (a NaN product adds 0),      cnt[j] += llrint(u_r 2^20)
 *    with int64 atomics (NERF_HIP_VOLUME_VQ_SHIFT = 20): the sums do not depend on the order of the rows.  THE BOUND: with
 *    |q_rw| <= 2^10, u_r <= 1 and m < 2^31 a sum stays below 2^10 2^20 2^31 = 2^61 < 2^62 and a count below 2^51; rows with a larger or
 *    non-finite word are the caller's to keep out (volume.vq_classes keeps them verbatim).  UPDATE then sets, per code and word,
 *       c_jw = (float)((double)sum[j][w] / (double)cnt[j])     where cnt[j] > 0;
 *    a code with cnt[j] <= 0 keeps its words.  The caller zeroes sum and cnt between iterations.
 *
 * VQ-D. DECODE.  cls[n] (uint8: 0 pruned, 1 coded, 2 kept), rank[n] (int32: the row's rank among the rows of its class, in row order),
 *    code[n_coded] (uint16), kept[n_kept][S] and codebook[K][S] (fp16, S = rule VC's fp16 stride, pads +0) -> coef_rows[n][S] fp16:
 *    a coded row r copies the S halves of codebook[code[rank[r]]], a kept row those of kept[rank[r]], a pruned row is +0 -- as is any
 *    row whose class is none of the three, whose rank lies outside its class, or whose code is >= K.  One thread per 8-byte word.
 *
 * All five are enqueue-only and check every argument on the host first (NERF_HIP_ERR_ARG) as the calls above do: the lattice, the
 * degree, a count < 0 or >= 2^31, K outside [1, 65536] (decode: [0, 65536], and > 0 with coded rows), imax < 0,
 * n_coded + n_kept > n, a NULL pointer or one that is not aligned to its element (int64: 8; fp16 rows: 8).  N = 0, m = 0 and n = 0
 * succeed and launch nothing.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_VOLUME_VQ_SHIFT 20
#define NERF_HIP_VOLUME_VQ_MAX_CODES 65536

/* VI over the rays of nerf_hip_volume_compact_render (its arguments without coef_rows, half, degree, background and the float
 * outputs): contributions ADDED IN PLACE to imp_rows[n] (device, int64, units of 2^-40); steps[N][2] as render's. */
int nerf_hip_volume_compact_importance(const int32_t* slot, const float* sigma_rows, int64_t n, const uint8_t* occ, int nx, int ny, int nz,
                                       int block, const float* lo3, const float* step3, const float* origins, const float* dirs,
                                       const float* tmin, const float* tmax, int64_t N, float dt, float t_stop, int64_t* imp_rows,
                                       int32_t* steps, void* stream);

/* VQ-A: assign[m] (device, int32) and, unless NULL, dist[m] (fp32). */
int nerf_hip_volume_vq_assign(const float* rows, int64_t m, const float* codebook, int64_t K, int degree, int32_t* assign, float* dist,
                              void* stream);

/* VQ-U's ACCUMULATE into sum[K][W] and cnt[K] (device, int64, zeroed by the caller); weight may be NULL. */
int nerf_hip_volume_vq_accumulate(const float* rows, int64_t m, int degree, const int64_t* weight, int64_t imax, const int32_t* assign,
                                  int64_t K, int64_t* sum, int64_t* cnt, void* stream);

/* VQ-U's UPDATE of codebook[K][W] in place. */
int nerf_hip_volume_vq_update(float* codebook, int64_t K, int degree, const int64_t* sum, const int64_t* cnt, void* stream);

/* VQ-D -> coef_rows[n][S] (device, fp16, 8-byte aligned). */
int nerf_hip_volume_vq_decode(const uint8_t* cls, const int32_t* rank, int64_t n, const uint16_t* code, int64_t n_coded, const void* kept,
                              int64_t n_kept, const void* codebook, int64_t K, int degree, void* coef_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ABI 7 additions.  Fine-tuning a vector-quantised volume: VQRF's fourth step -- the codebook, the kept rows
 * and sigma trained jointly against the training rays with the assignments FROZEN.  Nothing of the calls above changes: the march
 * and its gradient stay rules VC-R and VCG over fp32 rows; what is new is the way from the trainable state to those rows (VQ-X), the
 * way from the rows' accumulators to the codes' (VQ-G) and an update over three kinds of parameter (VQ-V).  Throughout W = 3 ncoef and
 *       sigma_rows[n]            fp32, trained;
 *       kept32[n_kept][W]        fp32 masters of the kept rows, trained;
 *       codebook32[K][W]         fp32 masters of the codebook, trained;
 *       cls[n], rank[n], code[n_coded]   frozen, as in rule VQ-D.
 *
 * VQ-X. EXPAND: rule VQ-D in fp32 and without pads.  coef_rows[n][W] fp32: a coded row r receives the W words of
 *    codebook32[code[rank[r]]], a kept row those of kept32[rank[r]], a pruned row +0 -- as does any row whose class is none of the
 *    three, whose rank lies outside its class, or whose code is >= K.  No index becomes an address before it has been compared with
 *    the size of its array.  One thread per (row, word).  These rows are what nerf_hip_volume_compact_render and
 *    nerf_hip_volume_compact_render_backward read.  A row that receives +0 still has a slot, so rule VCG adds to its accumulator words
 *    whenever it is a corner of a contributing cell, and nothing below consumes them: with acc_coef_rows not NULL, EXPAND also sets the
 *    W accumulator words of every row that receives +0 to 0 (the words of the other rows are not touched).
 *
 * VQ-G. REDUCE: from the rows' accumulators to the codes'.  The coded rows are given GROUPED BY CODE: member[n_coded] (int32 row
 *    numbers) and offset[K + 1] (int32, ascending, offset[0] = 0, offset[K] = n_coded): the members of code j are
 *    member[offset[j] .. offset[j + 1]).  The caller builds both once -- the codes are frozen.  Then, for every code j and word w,
 *       acc_code[j][w] += sum over the members r of code j of acc_coef_rows[r][w]
 *    in plain int64 adds (two's complement: the sum of the members' words, whatever the order), and every word that was read is set
 *    to 0.  The result does not depend on the order of the members within a code, on the launch shape or on where a large code is
 *    split.  A member outside [0, n) is skipped and never becomes an address.  The members must be distinct (a row has one code); a
 *    row listed twice is read and cleared by two threads in no order.  offset is DEVICE memory: the host cannot see it and refuses
 *    only what it can (below); the kernel clamps -- code j covers [a_j, b_j) with a_j = min(max(offset[j], 0), n_coded) and
 *    b_j = min(max(offset[j + 1], a_j), n_coded), so whatever offset holds no address leaves member[0 .. n_coded).
 *    OVERFLOW PRECONDITION, as rule VG's: between two updates the sum, over the members of one code, of the |x| their words (m, ch)
 *    received stays below 2^22; then |acc_code| < 2^62 < 2^63.  WHY IT HOLDS FOR ANY GROUPING.  One ray, one word (m, ch): sample i
 *    sends ((tw_c Y_m) (w_i g_ch)) to corner c (rule VG).  A cell's corner terms tw_c are >= 0 and sum to 1; the weights w_i are >= 0
 *    and sum to the ray's opacity, at most 1 (rule VR: w = T alpha, T = T - w from T = 1); |tw Y_m| < 1.1 (rule VG).  So the |x| one
 *    ray sends to ALL rows together, for one word, sum to less than 1.1 |g_ch|.  With |g_rgb| <= 2 -- the gradient 2 (rgb - target) of
 *    a squared error between colours in [0, 1] -- a batch of at most 2^20 rays sends less than 2.2 2^20 < 2^22 to all rows, hence to
 *    the members of any one code, and to any one row (rule VG's own precondition).  The rounding of each contribution to a multiple of
 *    2^-40 adds at most 2^-41 per contribution: with fewer than 2^31 contributions, below 2^-10.
 *
 * VQ-V. UPDATE: rule VU's word bracket, verbatim -- g = (double(acc) 2^-40) grad_scale, m' and v' each rounded to fp32 once,
 *    x' = fp32(x - (lr ((m' / c1) / (sqrt(v' / c2) + eps)))), beta^step by squaring on the host, the accumulator word zeroed whatever
 *    happens -- over three groups of words in one launch, one thread per word:
 *       (a) the sigma word of every row r: x = sigma_rows[r], acc = acc_sigma_rows[r], lr = lr_sigma, with rule VCU's FROZEN SUPPORT (a
 *           row whose sigma is not > 0 at entry is dead: x, m and v are left alone; otherwise sigma' = fmax(x', 0));
 *       (b) the W words of every kept row k: x = kept32[k][w], acc = acc_coef_rows[kept_row[k]][w], lr = lr_coef; kept_row[n_kept]
 *           (int32) is the row of kept row k; a kept_row outside [0, n) never becomes an address and its words are left alone;
 *       (c) the K W words of the codebook: x = codebook32[j][w], acc = acc_code[j][w], lr = lr_coef.
 *    m, v [n + n_kept W + K W] fp32 hold the moments in that order: 8 bytes of moments per coded row, where rule VCU holds 8 (1 + W).
 *    The accumulator words of a pruned row's coefficients belong to none of the groups: rule VQ-X clears them.
 *
 * ONE STEP is: rule VC-R's render of the rows, rule VCG with 2 (rgb - target), VQ-G, VQ-V with grad_scale = 1 / (3 N), VQ-X.  With
 * every code holding one row, or every row kept, it equals rule VCU's step on the same rows bit for bit.
 *
 * All three are enqueue-only and check every argument on the host first (NERF_HIP_ERR_ARG) as the calls above do: the degree, a
 * count < 0 or >= 2^31, K outside [0, 65536] (and > 0 with coded rows), n_coded + n_kept > n, the scalars as rule VU states them, a
 * NULL pointer or one that is not aligned to its element (int64: 8).  Zero counts succeed and launch nothing.
 * ------------------------------------------------------------------------------------------- */
#define NERF_HIP_VOLUME_VQ_REDUCE_CHUNK 256

/* VQ-X -> coef_rows[n][3 ncoef] (device, fp32); acc_coef_rows[n][3 ncoef] (int64) or NULL. */
int nerf_hip_volume_vq_expand(const uint8_t* cls, const int32_t* rank, int64_t n, const uint16_t* code, int64_t n_coded, const float* kept32,
                              int64_t n_kept, const float* codebook32, int64_t K, int degree, float* coef_rows, int64_t* acc_coef_rows,
                              void* stream);

/* VQ-G: acc_coef_rows[n][3 ncoef] -> ADDED to acc_code[K][3 ncoef] (device, int64), the words read are zeroed.  The members are walked
 * in chunks of NERF_HIP_VOLUME_VQ_REDUCE_CHUNK consecutive entries of member[], one workgroup each. */
int nerf_hip_volume_vq_grad_reduce(int64_t* acc_coef_rows, int64_t n, int degree, const int32_t* offset, const int32_t* member,
                                   int64_t n_coded, int64_t K, int64_t* acc_code, void* stream);

/* VQ-V.  The scalars are nerf_hip_volume_adam_step's. */
int nerf_hip_volume_vq_adam_step(float* sigma_rows, int64_t n, float* kept32, const int32_t* kept_row, int64_t n_kept, float* codebook32,
                                 int64_t K, int degree, int64_t* acc_sigma_rows, int64_t* acc_coef_rows, int64_t* acc_code, float* m,
                                 float* v, double grad_scale, int64_t step, double lr_sigma, double lr_coef, double beta1, double beta2,
                                 double eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_HIP_H */
