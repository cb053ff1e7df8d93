"""The operands of the weight-gradient products, read back from a train step's workspace, and a float64 reference of the 24
gradients the kernels form from them (tests/test_gpu_weight_gradients.py).

After a backward the workspace still holds exactly what the products read: ``save`` / ``G`` / ``dz`` (fp32 train step), the
fragment-layout ``bsave`` / ``bG`` (bf16 MLP) and also their mid parts ``bsave2`` / ``bG2`` (split-fp32 train step).  Evaluating
the products in float64 from those operands leaves only the kernels' fp32 accumulation order as a source of difference, whatever
the upstream gradient's conditioning.

Operands are dicts of name -> tuple of parts, each part a [real rows, features] tensor on the device (one part: fp32 and bf16;
two parts (hi, mid): split).  Rows are the real samples of the coarse pass, then those of the fine pass.
  gp  gamma_p (60)   h0..h7 (256)   c (128)   gd  gamma_d (24, per sample)
  g0..g7  pre-activation gradients of point_layer[0..7] (256)   gdir  of dir_info (128)   dz  colour head (3)   dspre  sigma head (1)
"""
import torch

# ---- constants of the kernels ----------------------------------------------------------------------------------------
FRAG_BYTES = 1024        # csrc/bf16_common.h:23  BF_FRAG_BYTES
WAVE_ROWS = 32           # csrc/bf16_common.h:54  a wave block = 32 consecutive samples of a pass
# csrc/bf16_common.h:58-59  saved layer inputs: BS_GP = 0, BS_H0 = 1, BS_C = 9, BS_GD = 10; bs_ks(t) pieces of 16 features each
BS_GP, BS_H0, BS_C, BS_GD = 0, 1, 9, 10
BS_KS = [4] + [16] * 8 + [8, 2]
# csrc/bf16_common.h:63-64  pre-activation gradients: BG_L0 = 0, BG_D = 8, BG_Z = 9 (features 0..2 = dz, 3 = dspre); bg_ks(t)
BG_L0, BG_D, BG_Z = 0, 8, 9
BG_KS = [16] * 8 + [8, 2]
DUMP_ROWS = 64           # csrc/common.h:24  rows behind every tensor of save / G
S_H0, S_C, S_GP = 0, 8, 9  # csrc/kernels.h:60  save tensors (NSAVE = 10)
G_D = 8                  # csrc/kernels.h:62  G tensors: dpre0..7, dpre_dir (NGRAD = 9)
NSAVE, NGRAD = 10, 9
WIDTH, HALF, POINT_DIM, DIR_DIM = 256, 128, 60, 24  # csrc/common.h:10-15
# csrc/common.h:68  dweights24 indices
W_SIGMA, B_SIGMA, W_PI, B_PI, W_DIR, B_DIR, W_COLOR, B_COLOR = 16, 17, 18, 19, 20, 21, 22, 23


def wave_blocks(B, N):
    """csrc/api.hip:56: wave blocks of one pass of the bf16 kernels -- whole 256-sample workgroups."""
    return ((B * N + 255) // 256) * 8


def pass_rows(B, Nc, Nf):
    """(wb_c, wb_tot, [(first, count)] of the real rows of the coarse and the fine pass inside the wave blocks)."""
    wb_c = wave_blocks(B, Nc)
    return wb_c, wb_c + wave_blocks(B, Nf), [(0, B * Nc), (wb_c * WAVE_ROWS, B * Nf)]


def decode(buf, wb_tot, ks_list, tensor):
    """Fragment layout -> [wb_tot * 32 samples, 16 * ks features] bf16, on buf's device.  Tensor t starts at
    wb_tot * 1024 * cum_ks(t); piece (wb, ks) of it at (wb * ks_t + ks) * 1024; lane (j, h) = 16-byte unit h * 32 + j of the piece
    holds sample wb * 32 + j, slot s (of 8) = feature 16 ks + 4 h + (s & 3) + 8 (s >> 2)  (csrc/bf16_common.h:54-56, dw_bf16.hip dma_block)."""
    ks_t = ks_list[tensor]
    start = wb_tot * FRAG_BYTES * sum(ks_list[:tensor])
    raw = buf[start:start + wb_tot * ks_t * FRAG_BYTES].view(torch.bfloat16).view(wb_tot, ks_t, 2, WAVE_ROWS, 2, 4)  # wb, ks, h, j, q, r
    # feature = 16 ks + 8 q + 4 h + r
    return raw.permute(0, 3, 1, 4, 2, 5).reshape(wb_tot * WAVE_ROWS, ks_t * 16)


def _real(t, ranges):
    return torch.cat([t[a:a + n] for a, n in ranges])


def _fragment_parts(ws, B, Nc, Nf, flags, names):
    from nerf_tiny_amd import _abi

    _, wb_tot, ranges = pass_rows(B, Nc, Nf)
    out = []
    for sname, gname in names:
        bs = _abi.ws_view(ws, B, Nc, Nf, flags, sname, (wb_tot * sum(BS_KS) * FRAG_BYTES,), torch.uint8)
        bg = _abi.ws_view(ws, B, Nc, Nf, flags, gname, (wb_tot * sum(BG_KS) * FRAG_BYTES,), torch.uint8)
        x = lambda t, n: _real(decode(bs, wb_tot, BS_KS, t), ranges)[:, :n]
        g = lambda t, n: _real(decode(bg, wb_tot, BG_KS, t), ranges)[:, :n]
        p = {"gp": x(BS_GP, POINT_DIM), "c": x(BS_C, HALF), "gd": x(BS_GD, DIR_DIM), "gdir": g(BG_D, HALF)}
        for l in range(8):
            p[f"h{l}"] = x(BS_H0 + l, WIDTH)
            p[f"g{l}"] = g(BG_L0 + l, WIDTH)
        z = g(BG_Z, 4)
        p["dz"], p["dspre"] = z[:, :3], z[:, 3:4]
        out.append(p)
    return {k: tuple(p[k] for p in out) for k in out[0]}


def read_operands(ws, B, Nc, Nf, flags):
    """The products' operands after a backward with these flags (csrc/api.hip layout(): which buffers exist)."""
    from nerf_tiny_amd import _abi

    if flags & _abi.BF16_MLP:
        return _fragment_parts(ws, B, Nc, Nf, flags, [("bsave", "bG")])
    if flags & _abi.SPLIT_MLP:
        return _fragment_parts(ws, B, Nc, Nf, flags, [("bsave", "bG"), ("bsave2", "bG2")])
    Mtot = B * (Nc + Nf)
    MS = Mtot + DUMP_ROWS
    view = lambda name, shape: _abi.ws_view(ws, B, Nc, Nf, flags, name, shape)
    save, G, dz = view("save", (NSAVE, MS, WIDTH)), view("G", (NGRAD, MS, WIDTH)), view("dz", (Mtot, 4))
    # gamma_d is stored once per ray (gdbuf); the reference repeats it for every sample of the ray, coarse rows then fine rows
    gdbuf = view("gdbuf", (B, DIR_DIM))
    ray = torch.cat((torch.arange(B * Nc, device=ws.device) // Nc, torch.arange(B * Nf, device=ws.device) // Nf))
    p = {"gp": save[S_GP, :Mtot, :POINT_DIM], "c": save[S_C, :Mtot, :HALF], "gd": gdbuf[ray], "gdir": G[G_D, :Mtot, :HALF],
         "dz": dz[:, :3], "dspre": dz[:, 3:4]}
    for l in range(8):
        p[f"h{l}"] = save[S_H0 + l, :Mtot]
        p[f"g{l}"] = G[l, :Mtot]
    return {k: (v,) for k, v in p.items()}


def rows(ops, a, b):
    """The operands of rows [a, b) only."""
    return {k: tuple(t[a:b] for t in v) for k, v in ops.items()}


def _prod(G, X):
    """(sum_s G[s]^T X[s], the same on absolute values) in float64.  Split operands: hi.hi + hi.mid + mid.hi -- the three products
    dw_bf16.hip forms (the mid.mid term is not part of the kernels' arithmetic); otherwise the one product."""
    terms = [(0, 0)] if len(G) == 1 else [(1, 0), (0, 1), (0, 0)]
    v = m = 0
    for i, j in terms:
        g, x = G[i].double(), X[j].double()
        v = v + g.T @ x
        m = m + g.abs().T @ x.abs()
    return v, m


def _colsum(G):
    """Column sums of G in float64, with the magnitude.  Split: of hi AND mid (dw_bf16.hip accumulates G_mid . 1 and G_hi . 1)."""
    v = sum(t.double().sum(0) for t in G)
    m = sum(t.double().abs().sum(0) for t in G)
    return v, m


def dw_reference(ops, weights):
    """float64 (value, magnitude) of each of the 24 gradient tensors (include/nerf_hip.h weight order) from the products' operands.
    `weights`: the model's fp32 parameters, for the fold of point_info into dir_info.  The magnitude is the same formula on absolute
    values (|G|^T |X|, |W|^T |M| through the fold): the scale against which a summation-order difference is measured."""
    cat = lambda a, b: tuple(torch.cat((x, y), 1) for x, y in zip(a, b))
    out = [None] * 24
    for l in range(8):
        X = ops["gp"] if l == 0 else cat(ops["h3"], ops["gp"]) if l == 4 else ops[f"h{l - 1}"]  # nerf.py:109: hidden first
        out[2 * l] = _prod(ops[f"g{l}"], X)
        out[2 * l + 1] = _colsum(ops[f"g{l}"])
    out[W_SIGMA] = _prod(ops["dspre"], ops["h7"])
    sb, sbm = _colsum(ops["dspre"])
    out[B_SIGMA] = (sb.reshape(1), sbm.reshape(1))
    # point_info folded into dir_info (csrc/dw_f32.hip:670-674, k_fold_grads): M = dpre_dir^T h7, db_dir = column sums of dpre_dir,
    # dW_pi = W_dir[:, 24:]^T M, db_pi = W_dir[:, 24:]^T db_dir, dW_dir[:, 24:] = M W_pi^T + db_dir (x) b_pi
    M, Mm = _prod(ops["gdir"], ops["h7"])
    db, dbm = _colsum(ops["gdir"])
    Wd, Wpi, bpi = (weights[i].double() for i in (W_DIR, W_PI, B_PI))
    Wf = Wd[:, DIR_DIM:]
    out[W_PI] = (Wf.T @ M, Wf.abs().T @ Mm)
    out[B_PI] = (Wf.T @ db, Wf.abs().T @ dbm)
    D, Dm = _prod(ops["gdir"], ops["gd"])  # direction columns: nerf.py:117, direction first
    out[W_DIR] = (torch.cat((D, M @ Wpi.T + torch.outer(db, bpi)), 1), torch.cat((Dm, Mm @ Wpi.abs().T + torch.outer(dbm, bpi.abs())), 1))
    out[B_DIR] = (db, dbm)
    out[W_COLOR] = _prod(ops["dz"], ops["c"])
    out[B_COLOR] = _colsum(ops["dz"])
    return out


def dw_statistic(got, ref, mag):
    """||got - ref|| / ||mag||: does not grow where the sum cancels (bias gradients, the scalar sigma bias)."""
    return float((got.double().reshape(ref.shape) - ref).norm() / mag.norm().clamp_min(1e-300))
