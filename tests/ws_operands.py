"""The operands of the weight-gradient products, read back from a train step's workspace, and a float64 reference of the 24
gradients the kernels form from them (tests/test_gpu_weight_gradients.py); the operands of every forward layer and every layer of
the dX chain, and float64 references of each layer from its own saved operands (tests/test_gpu_layers.py).

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
    """csrc/api.hip wave_blocks(): wave blocks of one pass of the bf16 kernels -- whole 256-sample workgroups."""
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


# ---- the forward and the dX chain: readers -------------------------------------------------------------------------------------
TM = 64                  # csrc/common.h:16  samples per tile of the fp32 field kernels (the fp32 mask image)
BM_LAYERS = 9            # csrc/bf16_common.h:68  bmask layers: h0..h7, c
NOT_ROWS = {"fold", "b_fold"}  # per-call operands (no rows): rows() passes them through


def relu_mask_image(hidden, tiles):
    """ReLU masks in the fp32 field kernels' accumulator layout: [8][tiles][4][256] int16, bit r of entry
    (f*2+st, tid = wv*64 + h*32 + j) <-> feature wv*64 + f*32 + 8(r>>2) + 4h + (r&3) of sample st*32 + j."""
    f, st, wv, h, j, r = torch.meshgrid(torch.arange(2), torch.arange(2), torch.arange(4), torch.arange(2), torch.arange(32),
                                        torch.arange(16), indexing="ij")
    feat = wv * 64 + f * 32 + 8 * (r >> 2) + 4 * h + (r & 3)
    samp = st * 32 + j
    out = []
    for H in hidden:  # [M, 256]
        M = H.shape[0]
        Hp = torch.zeros(tiles * 64, 256, dtype=torch.bool)
        Hp[:M] = H > 0
        Hp = Hp.view(tiles, 64, 256)
        bits = Hp[:, samp, feat].to(torch.int32)  # [tiles, f, st, wv, h, j, r]
        word = (bits << torch.arange(16, dtype=torch.int32)).sum(-1)
        word = word - 65536 * (word >= 32768).to(torch.int32)
        out.append(word.reshape(tiles, 4, 256).to(torch.int16))
    return torch.stack(out)  # [8, tiles, 4, 256]


def decode_relu_masks(img):
    """The inverse of relu_mask_image: [L][tiles][4][256] int16 -> [L, tiles * 64 samples, 256 features] bool, on img's device."""
    L, tiles = img.shape[:2]
    r = torch.arange(16, device=img.device, dtype=torch.int32)
    bits = (img.to(torch.int32).view(L, tiles, 2, 2, 4, 2, 32, 1) >> r) & 1  # L, tile, f, st, wv, h, j, r
    bits = bits.view(L, tiles, 2, 2, 4, 2, 32, 4, 4)                          # r = 4 rq + rr
    # sample st*32 + j, feature wv*64 + f*32 + 8 rq + 4h + rr
    return bits.permute(0, 1, 3, 6, 4, 2, 7, 5, 8).reshape(L, tiles * 64, WIDTH).bool()


def decode_bmask(words, wb_tot):
    """bf16 / split `bmask`: u16 [9 layers: h0..h7, c][wb_tot][64 lanes][8 tiles], bit 15 - r = accumulator register r of tile f; lane
    h * 32 + j holds sample wb * 32 + j, register r = feature 32 f + 8 (r >> 2) + 4 h + (r & 3) (csrc/bf16_common.h:67, the map of
    decode).  -> [9, wb_tot * 32, 256] bool (the c layer's features 128..255 are the zero words of tiles 4..7)."""
    r = torch.arange(16, device=words.device, dtype=torch.int32)
    bits = (words.to(torch.int32).view(BM_LAYERS, wb_tot, 2, WAVE_ROWS, 8, 1) >> (15 - r)) & 1  # l, wb, h, j, f, r
    bits = bits.view(BM_LAYERS, wb_tot, 2, WAVE_ROWS, 8, 4, 4)                                 # r = 4 rq + rr
    return bits.permute(0, 1, 3, 4, 5, 2, 6).reshape(BM_LAYERS, wb_tot * WAVE_ROWS, WIDTH).bool()


def read_layer_operands(ws, B, Nc, Nf, flags):
    """read_operands plus what the forward and the chain read and write besides the products' operands:
      m0..m7, mc  ReLU masks of h0..h7 and c (bool; fp32: c's mask is c > 0, as field_bwd_reg.hip forms it from the saved c)
      spre  sigma pre-activation   sig, rgb  per-sample outputs   drgb, dsig  their upstream gradients
      start  fp32: dir_info's per-ray start vector (dvec) of every row
      fold, b_fold  bf16 / split: the fp32 W_fold [128][256] and b_fold [128] of the workspace (no rows)
    Every per-row entry is a tuple of parts like read_operands' (one part except the split's layer inputs and gradients)."""
    from nerf_tiny_amd import _abi

    ops = read_operands(ws, B, Nc, Nf, flags)
    dev = ws.device
    view = lambda name, shape, dt=None: _abi.ws_view(ws, B, Nc, Nf, flags, name, shape, dt)
    cat = lambda a, b: torch.cat((a, b))
    ops["spre"] = (view("spre", (B * (Nc + Nf),)),)
    ops["sig"] = (cat(view("sig_c", (B * Nc,)), view("sig_f", (B * Nf,))),)
    ops["rgb"] = (cat(view("rgb_c", (B * Nc, 3)), view("rgb_f", (B * Nf, 3))),)
    ops["drgb"] = (cat(view("drgb_c", (B * Nc, 3)), view("drgb_f", (B * Nf, 3))),)
    ops["dsig"] = (cat(view("dsig_c", (B * Nc,)), view("dsig_f", (B * Nf,))),)
    if flags & (_abi.BF16_MLP | _abi.SPLIT_MLP):
        _, wb_tot, ranges = pass_rows(B, Nc, Nf)
        m = decode_bmask(view("bmask", (BM_LAYERS * wb_tot * 64 * 8,), torch.int16), wb_tot)
        for l in range(8):
            ops[f"m{l}"] = (_real(m[l], ranges),)
        ops["mc"] = (_real(m[8], ranges)[:, :HALF],)
        fold = view("fold", (HALF + HALF * WIDTH,))
        ops["b_fold"], ops["fold"] = (fold[:HALF],), (fold[HALF:].view(HALF, WIDTH),)
        return ops
    tiles_c, tiles_f = -(-B * Nc // TM), -(-B * Nf // TM)
    m = decode_relu_masks(view("masks", (8, tiles_c + tiles_f, 4, 256), torch.int16))
    for l in range(8):
        ops[f"m{l}"] = (cat(m[l, :B * Nc], m[l, tiles_c * TM:tiles_c * TM + B * Nf]),)
    ops["mc"] = (ops["c"][0] > 0,)
    ray = torch.cat((torch.arange(B * Nc, device=dev) // Nc, torch.arange(B * Nf, device=dev) // Nf))
    ops["start"] = (view("dvec", (B, HALF))[ray],)
    return ops


def rows(ops, a, b):
    """The operands of rows [a, b) only."""
    return {k: v if k in NOT_ROWS else tuple(t[a:b] for t in v) for k, v in ops.items()}


# ---- bf16 rounding, exactly ----------------------------------------------------------------------------------------------------
BF16_EMIN = -133  # exponent of the smallest bf16 subnormal


def pow2(q):
    """2^q as float64, exactly, for integer tensors q in [-1022, 1023] (torch.ldexp forms 2^q with pow, which need not be exact on the
    device)."""
    return ((q.to(torch.int64) + 1023) << 52).view(torch.float64)


def _bf16_exponent(x):
    """Exponent q of the bf16 unit in the last place at |x| (8 significant bits; subnormals share 2^-133)."""
    _, e = torch.frexp(x)
    return torch.clamp(e.to(torch.int64) - 8, min=BF16_EMIN)


def rne_bf16(x):
    """float64 -> the nearest bf16 value, ties to even (torch.round rounds half to even), as float64.  Exact: no detour through fp32
    (.to(torch.bfloat16) of a float64 may round twice), and the scalings are exact powers of two.  Beyond the bf16 range nothing is checked: the operands here are far inside."""
    q = _bf16_exponent(x)
    return torch.round(x * pow2(-q)) * pow2(q)


def trunc_bf16(x):
    """float64 -> bf16 by truncation toward zero (the teeth of the RNE interval test)."""
    q = _bf16_exponent(x)
    return torch.trunc(x * pow2(-q)) * pow2(q)


def ulp_bf16(x):
    """The bf16 spacing at |x| (upward from |x|)."""
    return pow2(_bf16_exponent(x))


def split_bf16(w):
    """fp32 values (as float64) -> (hi, mid) = (RNE(w), RNE(w - hi)): the split-fp32 parts (w - hi is exact in fp32)."""
    hi = rne_bf16(w)
    return hi, rne_bf16(w - hi)


# ---- the forward and the dX chain: float64 references --------------------------------------------------------------------------
SPLIT_TERMS = ((0, 0), (0, 1), (1, 0))  # (operand part, weight part): hi.hi + hi.mid + mid.hi (mid.mid is not in the kernels' arithmetic)


def _mv(X, Wp, Wmag=None, terms=SPLIT_TERMS, transpose=True):
    """sum over terms of X[i] W[j]^T (transpose=False: X[i] W[j]) in float64, and the same on absolute values (Wmag: the magnitude
    matrix of a weight whose value is not a plain product -- the fp32 fold)."""
    terms = [(0, 0)] if len(X) == 1 else terms
    v = m = 0
    for i, j in terms:
        x, w = X[i].double(), Wp[j]
        wm = Wmag if Wmag is not None else w.abs()
        if transpose:
            w, wm = w.T, wm.T
        v = v + x @ w
        m = m + x.abs() @ wm
    return v, m


def reference_weights(ops, weights, mode):
    """The weight operands the kernels multiplied by, float64, as tuples of parts, and the float64 biases.
      fp32   the parameters; W_fold = W_dir[:, 24:] W_pi in float64 (the fp32 packer folds straight into `packed`), magnitude
             |W_dir[:, 24:]| |W_pi|; the start of dir_info = the workspace's dvec (no W_dir[:, :24] term)
      bf16   RNE-bf16 of the parameters and of the device's fp32 W_fold (oracle.mlp_bf16 is the spec); the start = b_dir + b_fold
             plus W_dir[:, :24] gamma_d
      split  (hi, mid) of the same fp32 values"""
    parts = (lambda w: (w.double(),)) if mode == "fp32" else (lambda w: (rne_bf16(w.double()),)) if mode == "bf16" else \
        (lambda w: split_bf16(w.double()))
    out = {"W": [parts(weights[2 * l]) for l in range(8)], "b": [weights[2 * l + 1].double() for l in range(8)],
           "w_sigma": parts(weights[W_SIGMA]), "b_sigma": weights[B_SIGMA].double(),
           "W_color": parts(weights[W_COLOR]), "b_color": weights[B_COLOR].double()}
    Wd = weights[W_DIR].double()
    if mode == "fp32":
        Wpi = weights[W_PI].double()
        out["W_fold"], out["W_fold_mag"] = (Wd[:, DIR_DIM:] @ Wpi,), Wd[:, DIR_DIM:].abs() @ Wpi.abs()
    else:
        out["W_fold"], out["W_fold_mag"] = parts(ops["fold"][0]), None
        out["W_dir_gd"] = parts(weights[W_DIR][:, :DIR_DIM])
        out["b_dir"] = weights[B_DIR].double() + ops["b_fold"][0].double()
    return out


def iter_layer_reference(ops, weights, mode, terms=SPLIT_TERMS):
    """Each forward layer in float64 from the device's own saved input of that layer: yields (name, (value, magnitude, pre-activation)).
      h0..h7  relu(W_l x + b_l), x = gamma_p, h_{l-1}, or cat(h3, gamma_p) (hidden first) for layer 4
      spre    w_sigma . h7 + b_sigma          sigma  |spre|
      c       relu(W_fold h7 + start)         rgb    sigmoid(W_c c + b_c)  (magnitude and pre-activation: of W_c c + b_c)
    mode: "fp32", "bf16" or "split" (reference_weights).  Magnitude = the same formula on absolute values, |W| |x| + |b|."""
    R = reference_weights(ops, weights, mode)
    cat = lambda a, b: tuple(torch.cat((x, y), 1) for x, y in zip(a, b))
    for l in range(8):
        X = ops["gp"] if l == 0 else cat(ops["h3"], ops["gp"]) if l == 4 else ops[f"h{l - 1}"]
        v, m = _mv(X, R["W"][l], terms=terms)
        v, m = v + R["b"][l], m + R["b"][l].abs()
        yield f"h{l}", (v.clamp_min(0), m, v)
        del v, m
    v, m = _mv(ops["h7"], R["w_sigma"], terms=terms)
    v, m = v[:, 0] + R["b_sigma"], m[:, 0] + R["b_sigma"].abs()
    yield "spre", (v, m, v)
    yield "sigma", (v.abs(), m, v)
    v, m = _mv(ops["h7"], R["W_fold"], R["W_fold_mag"], terms=terms)
    if mode == "fp32":
        s = ops["start"][0].double()
        v, m = v + s, m + s.abs()
    else:
        vd, md = _mv(ops["gd"], R["W_dir_gd"], terms=terms)
        v, m = v + vd + R["b_dir"], m + md + R["b_dir"].abs()
    yield "c", (v.clamp_min(0), m, v)
    v, m = _mv(ops["c"], R["W_color"], terms=terms)
    v, m = v + R["b_color"], m + R["b_color"].abs()
    yield "rgb", (torch.sigmoid(v), m, v)


def layer_reference(ops, weights, mode):
    """{name: (value, magnitude, pre-activation)} of iter_layer_reference (all at once: small batches and CPU checks)."""
    return dict(iter_layer_reference(ops, weights, mode))


def upstream_reference(ops):
    """The chain's first step, in the kernels' fp32 arithmetic (field_bwd_reg.hip:233, -ffp-contract=off): dz = drgb * ((1 - o) * o),
    o the saved per-sample rgb, and dspre = dsig * sign(spre), sign(0) = 0.  fp32 tensors."""
    o, up = ops["rgb"][0], ops["drgb"][0]
    return up * ((1 - o) * o), ops["dsig"][0] * torch.sign(ops["spre"][0])


def iter_chain_reference(ops, weights, mode, terms=SPLIT_TERMS):
    """Each layer of the dX chain in float64 from the device's own next-layer operand: yields (name, (value, magnitude)).
      gdir  [c > 0] (W_c^T dz)          g7  mask7 (W_fold^T gdir + w_sigma dspre)
      g_l   mask_l (W_{l+1}^T g_{l+1}), the first 256 columns of W4 for g3
    The masks are the device's (checked against the forward's pre-activations separately)."""
    R = reference_weights(ops, weights, mode)
    v, m = _mv(ops["dz"], R["W_color"], terms=terms, transpose=False)
    mk = ops["mc"][0]
    yield "gdir", (v * mk, m * mk)
    v, m = _mv(ops["gdir"], R["W_fold"], R["W_fold_mag"], terms=terms, transpose=False)
    vs, ms = _mv(ops["dspre"], R["w_sigma"], terms=terms, transpose=False)
    mk = ops["m7"][0]
    yield "g7", ((v + vs) * mk, (m + ms) * mk)
    for l in range(6, -1, -1):
        W = tuple(w[:, :WIDTH] for w in R["W"][l + 1])
        v, m = _mv(ops[f"g{l + 1}"], W, terms=terms, transpose=False)
        mk = ops[f"m{l}"][0]
        yield f"g{l}", (v * mk, m * mk)
        del v, m


def chain_reference(ops, weights, mode):
    """{name: (value, magnitude)} of iter_chain_reference."""
    return dict(iter_chain_reference(ops, weights, mode))
