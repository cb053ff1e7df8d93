"""GPU: vector-quantised compact SH radiance volumes (csrc/volume_vq.hip; rules VI, VQ-A, VQ-U and VQ-D of include/nerf_hip.h) -- the
importance sums against the march's own steps, against themselves under every reordering, against the restatement bit for bit where
alpha is the device's own (the slab) and within the DERIVED budget elsewhere; assign, accumulate, update and k-means against the numpy
restatements bit for bit; quantize / dequantize against convert and the restatement; the file round trip; refusals; the runner."""
import os

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_grad_reference as GR
import volume_reference as R
import volume_vq_reference as Q

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))   # 27 / 130 / 324 rows
ROWS = (27, 130, 324)
BLOCKS = (1, 2, 4, 8, 1 << 30)                   # the last: one block
NRAYS = 300
DT = Q.DT
TILE = 128                                       # VQ_TILE of csrc/kernels.h
_cache = {}


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)


def bits(a):
    a = host(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def scene(shape):
    if shape not in _cache:
        _cache[shape] = Q.scene(shape, nrays=NRAYS)
    return _cache[shape]


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def compact(pkg, dev, s, block=2, degree=2, dtype="fp32"):
    sg = on(dev, s["sigma"])                                                       # the garbage is there
    dv = pkg.volume.Volume(sg, on(dev, s["coef"][..., :(degree + 1) ** 2, :]), pkg.volume.blocks(sg, block), s["lo"], s["step"],
                           min(block, pkg.volume.ONE_BLOCK), degree)
    return pkg.volume.pack(dv, dtype)


def rays_on(dev, s, sel=slice(None)):
    return tuple(on(dev, s[k][sel]) for k in ("o", "d", "tmin", "tmax"))


def imp_of(pkg, dev, s, cv, sel=slice(None), acc=None, t_stop=0.3):
    return pkg.volume.importance(cv, *rays_on(dev, s, sel), acc=acc, dt=DT, t_stop=t_stop)


# ---- rule VI ----

@pytest.mark.parametrize("shape", LATTICES)
def test_importance_steps_and_order(pkg, dev, shape):
    s = scene(shape)
    cv = compact(pkg, dev, s)
    n = ROWS[LATTICES.index(shape)]
    assert cv.sigma.shape[0] == n == s["n"]
    for t_stop in (0.0, 0.3):
        acc, steps = imp_of(pkg, dev, s, cv, t_stop=t_stop)
        assert acc.dtype == torch.int64 and acc.shape == (n,) and steps.dtype == torch.int32
        assert same(steps, pkg.volume.render(cv, *rays_on(dev, s), dt=DT, t_stop=t_stop)[2])
        assert int((acc > 0).sum()) > n // 3 and int(acc.min()) >= 0 and int(steps[:, 0].sum()) > NRAYS
    base, steps = imp_of(pkg, dev, s, cv)
    assert same(imp_of(pkg, dev, s, cv)[0], base)                                  # the same call twice
    perm = np.random.default_rng(1).permutation(NRAYS)
    got, psteps = imp_of(pkg, dev, s, cv, sel=perm)
    assert same(got, base) and same(psteps, steps[on(dev, perm)])                  # the rays permuted
    two, _ = imp_of(pkg, dev, s, cv, sel=slice(0, 130))
    assert not same(two, base)
    again, _ = imp_of(pkg, dev, s, cv, sel=slice(130, NRAYS), acc=two)             # two half batches into one buffer
    assert again is two and same(two, base)
    for B in BLOCKS:                                                               # every block edge, both row dtypes, every degree
        for degree, dtype in ((2, "fp32"), (2, "fp16"), (0, "fp16"), (1, "fp32")):
            if B != 2 and degree != 2:
                continue
            c2 = compact(pkg, dev, s, B, degree, dtype)
            a2, s2 = imp_of(pkg, dev, s, c2)
            assert same(a2, base) and same(s2[:, 0], steps[:, 0]), (B, degree, dtype)
    none, zsteps = imp_of(pkg, dev, s, cv, sel=slice(0, 0))                        # no rays
    assert not none.any() and zsteps.shape == (0, 2)


def test_importance_slab_is_bit_exact(pkg, dev):
    """constant sigma: every contributing sample has the same alpha.  The device's own alpha is the opacity of a one-sample ray
    (A = 0 + 1 * alpha, exact); the restatement's fp32 recurrence on THAT alpha and its fp64 corner terms must give the device's
    sums bit for bit."""
    sigma, coef, lo, step, o, d, tmin, tmax, dt, K, sigma0, c = R.slab_case()
    sg = on(dev, sigma)
    cv = pkg.volume.pack(pkg.volume.Volume(sg, on(dev, coef), pkg.volume.blocks(sg, 2), lo, step, 2, 0))
    n = int(cv.sigma.shape[0])
    assert n == sigma.size                                                         # every point is active: slot = the point
    one = pkg.volume.render(cv, on(dev, o[:1]), on(dev, d[:1]), on(dev, tmin[:1]), on(dev, (tmin[:1] + dt).astype(F)), dt=dt, t_stop=0.0)
    assert host(one[2]).tolist() == [[1, 1]]
    alpha = F(host(one[1])[0, 1])
    assert 0 < alpha < 1 and abs(float(alpha) - (-np.expm1(-float(sigma0) * float(dt)))) < 8 * R.U
    acc, steps = pkg.volume.importance(cv, on(dev, o), on(dev, d), on(dev, tmin), on(dev, tmax), dt=dt, t_stop=0.0)
    assert np.array_equal(host(steps)[:, 0], K) and np.array_equal(host(steps)[:, 1], K)
    G = GR.geometry(sigma, coef, lo, step, o, d, tmin, tmax, dt)
    idx = GR.pad(G, np.full(G.tk.shape, sigma0, F))
    valid = idx >= 0
    assert np.array_equal(valid.sum(1), K)
    w = np.zeros(idx.shape, F)
    for r in range(len(K)):
        w[r, :K[r]] = Q.recurrence32(alpha, int(K[r]))
    want = Q.importance_fixed(G, idx, valid, w, np.arange(n, dtype=np.int32).reshape(sigma.shape), n)
    assert same(acc, want) and (want > 0).sum() >= 12                                 # (axis-parallel rays: few rows, all of them checked)
    # the rows hold the rays' whole opacity, to the fixed point: sum_r imp_r = sum_rays A
    assert abs(float(want.sum()) * 2.0 ** -40 - float(w.sum(dtype=np.float64))) < 8 * K.sum() * 2.0 ** -41


@pytest.mark.parametrize("t_stop", (0.0, 0.3))
@pytest.mark.parametrize("shape", LATTICES)
def test_importance_budget(pkg, dev, shape, t_stop):
    """every row against the fp64 restatement within the budget DERIVED in tests/volume_vq_reference.py (the fp32 alpha, w, T are the
    only inexact inputs, plus half a unit per llrint); the rays are truncated where the device's own march ended"""
    s = scene(shape)
    cv = compact(pkg, dev, s)
    acc, steps = imp_of(pkg, dev, s, cv, t_stop=t_stop)
    with np.errstate(all="ignore"):
        ref = Q.importance_reference(s["G"], s["sig"], s["slot"], s["n"], limit=host(steps)[:, 0])
    assert np.array_equal(ref["valid"].sum(1), host(steps)[:, 0])
    ratio = Q.importance_ratio(host(acc), ref)
    print(f"VI {shape} t_stop {t_stop}: worst |device - fp64| / budget = {ratio:.4f} over {int((ref['budget'] > 0).sum())} rows")
    assert ratio <= 1.0, ratio
    if t_stop == 0.0:                                                              # the planted mistakes are far outside it
        idx, valid = ref["idx"], ref["valid"]
        with np.errstate(all="ignore"):
            w, Tb, wa, _ = Q.forward32_all(s["G"], s["sig"], idx, 0.0)
        for mutate in ("T", "no_wz", "w_after"):
            assert Q.importance_ratio(Q.importance_fixed(s["G"], idx, valid, w, s["slot"], s["n"], mutate=mutate, T_before=Tb, w_after=wa), ref) > 100


def test_importance_corner_without_a_row(pkg, dev):
    """a corner whose slot lies outside [0, n) receives nothing and nothing is read through it: its sigma word is made a NaN"""
    s = scene((9, 8, 7))
    cv = compact(pkg, dev, s)
    n = s["n"]
    base, steps = imp_of(pkg, dev, s, cv)
    r = int(np.flatnonzero((host(base) != 0) & ~(s["sigma_rows"] > 0))[0])         # it contributes only as a neighbour: its sigma is +0
    assert s["sigma_rows"][r] == 0
    keep = torch.arange(n, device=dev) != r
    for bad_slot in (-1, n, -2, 2**31 - 1):
        slot = cv.slot.clone()
        slot.view(-1)[int(s["index"][r])] = bad_slot
        sig = cv.sigma.clone()
        sig[r] = float("nan")
        got, gsteps = imp_of(pkg, dev, s, cv._replace(slot=slot, sigma=sig))
        assert got[r] == 0 and same(got[keep], base[keep]) and same(gsteps, steps), bad_slot
    # no rows at all
    nothing = np.zeros((9, 8, 7), F)
    nothing[1, 1, 1], nothing[0, 0, 0] = np.nan, -1.0
    c0 = compact(pkg, dev, {**s, "sigma": nothing})
    a0, s0 = imp_of(pkg, dev, s, c0)
    assert a0.shape == (0,) and not s0[:, 0].any() and s0[:, 1].any()


# ---- rule VQ-A ----

def codebook_for(rng, rows, K):
    """K codes around the rows, with duplicated codes and a NaN code where there is room"""
    c = (rows[rng.integers(0, rows.shape[0], K)] + rng.normal(0, 0.05, (K, rows.shape[1]))).astype(F)
    if K >= 37:
        c[30], c[11] = c[4], c[4]                   # duplicates: the lowest index wins
        c[0, 1] = np.nan                            # a NaN code never wins
    return c


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_assign(pkg, dev, degree):
    W = 3 * (degree + 1) ** 2
    rng = np.random.default_rng(degree)
    for shape in ((17, 9, 12), (5, 4, 3)):                                         # m = 324: two workgroups, the second partial; m = 27
        rows = np.ascontiguousarray(scene(shape)["words"][:, :W])
        for K in (1, 2, 37, TILE - 1, TILE + 1):
            c = codebook_for(rng, rows, K)
            if K >= 37:
                rows = rows.copy()
                rows[5] = c[4]                                                     # a row that IS the duplicated code
            want_code, want_dist = Q.assign(rows, c)
            code, dist = pkg.ops.volume_vq_assign(on(dev, rows), on(dev, c), with_dist=True)
            assert same(code, want_code) and same(dist, want_dist), (shape, K)
            assert same(pkg.ops.volume_vq_assign(on(dev, rows), on(dev, c)), want_code)
            if K >= 37:
                assert want_code[5] == 4 and want_dist[5] == 0 and (want_code != 0).all() and len(np.unique(want_code)) > 10
    nan = np.full((1, W), np.nan, F)                                               # nothing wins: code 0, distance +inf
    code, dist = pkg.ops.volume_vq_assign(on(dev, rows), on(dev, nan), with_dist=True)
    assert not code.any() and bool(torch.isinf(dist).all())
    code = pkg.ops.volume_vq_assign(on(dev, rows[:0]), on(dev, c))
    assert code.shape == (0,)


# ---- rule VQ-U ----

@pytest.mark.parametrize("degree", (0, 1, 2))
def test_accumulate_and_update(pkg, dev, degree):
    W = 3 * (degree + 1) ** 2
    s = scene((17, 9, 12))
    rng = np.random.default_rng(10 + degree)
    rows = np.ascontiguousarray(s["words"][:, :W])
    m, K = rows.shape[0], 37
    c = codebook_for(rng, rows, K)
    code, _ = Q.assign(rows, c)
    code[code == 7] = 8                                                            # code 7 stays empty
    assert (code == 8).any()
    imp = host(imp_of(pkg, dev, s, compact(pkg, dev, s))[0])
    assert (imp == 0).any() and (imp > 1 << 30).any()
    perm = rng.permutation(m)
    for weight in (imp, None, np.zeros(m, np.int64)):
        imax = 0 if weight is None else int(weight.max())
        wS, wN = Q.accumulate(rows, weight, code, K)
        S, N = pkg.ops.volume_vq_accumulate(on(dev, rows), None if weight is None else on(dev, weight), imax, on(dev, code), K)
        assert same(S, wS) and same(N, wN) and N[7] == 0 and not S[7].any() and bool((N > 0).sum() > 10)
        book = on(dev, c)
        assert pkg.ops.volume_vq_update(book, S, N) is book
        assert same(book, Q.update(c, wS, wN)) and same(book[7], c[7]) and not same(book[8], c[8])
        Sp, Np = pkg.ops.volume_vq_accumulate(on(dev, rows[perm]), None if weight is None else on(dev, weight[perm]), imax,
                                              on(dev, code[perm]), K)               # the rows permuted, the assignment along
        assert same(Sp, S) and same(Np, N)
    bad = code.copy()
    bad[3], bad[4] = -1, K                                                         # outside [0, K): skipped, never an address
    S, N = pkg.ops.volume_vq_accumulate(on(dev, rows), on(dev, imp), int(imp.max()), on(dev, bad), K)
    wS, wN = Q.accumulate(rows, imp, bad, K)
    assert same(S, wS) and same(N, wN)


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_kmeans(pkg, dev, degree):
    W = 3 * (degree + 1) ** 2
    s = scene((17, 9, 12))
    rows = np.ascontiguousarray(s["words"][:, :W])
    imp = host(imp_of(pkg, dev, s, compact(pkg, dev, s))[0])
    for weight, K in ((imp, 16), (None, 16), (imp, TILE + 1), (imp, 1000)):
        want_c, want_code, trail = Q.kmeans(rows, weight, K, 3)
        book, code = pkg.volume.kmeans(on(dev, rows), None if weight is None else on(dev, weight), K, 3)
        assert book.shape == (min(K, 324), W) and same(book, want_c) and same(code, want_code), K
        if K == 16:
            assert not same(trail[0], trail[3]) and len(np.unique(want_code)) > 8
    book, code = pkg.volume.kmeans(on(dev, rows), on(dev, imp), 324, 0)            # K' = m, no iteration: every row is its own code
    assert same(book[code.long()], rows)


# ---- quantize / dequantize, the file ----

def same_compact(a, b):
    return (same(a.slot, b.slot) and same(a.sigma, b.sigma) and same(a.coef, b.coef) and same(a.occ, b.occ) and a.block == b.block
            and a.degree == b.degree and tuple(a.shape) == tuple(b.shape) and same(a.lo, b.lo) and same(a.step, b.step))


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_identity_quantization_is_convert(pkg, dev, shape, degree):
    s = scene(shape)
    for dtype in ("fp32", "fp16"):
        cv = compact(pkg, dev, s, 2, degree, dtype)
        imp, _ = imp_of(pkg, dev, s, cv)
        m = s["n"]
        for K in (m, 65536):
            vq = pkg.volume.quantize(cv, imp, K=K, iters=0)
            assert isinstance(vq, pkg.volume.VQVolume) and vq.codebook.shape == (m, X.row_width(degree, True)) and bool((vq.cls == 1).all())
            assert vq.code.dtype == torch.uint16 and vq.kept.shape[0] == 0 and same(vq.point, s["index"].astype(np.int32))
            dq = pkg.volume.dequantize(vq)
            want = pkg.volume.convert(cv, "fp16")
            assert same_compact(dq, want)
            r1, r2 = (pkg.volume.render(v, *rays_on(dev, s), dt=DT, t_stop=0.3, background=(0.25, 0.5, 1.0)) for v in (dq, want))
            assert all(same(a, b) for a, b in zip(r1, r2)) and bool(r1[2][:, 0].any())


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_quantize_with_classes(pkg, dev, degree, tmp_path):
    s = scene((17, 9, 12))
    W = 3 * (degree + 1) ** 2
    cv = compact(pkg, dev, s, 2, degree, "fp16" if degree == 1 else "fp32")
    rows32 = host(cv.coef)[:, :W].astype(F)
    imp, _ = imp_of(pkg, dev, s, cv)
    vq = pkg.volume.quantize(cv, imp, K=8, iters=2, prune_share=0.05, keep_share=0.3)
    want = Q.quantize(host(cv.sigma), rows32, host(imp), 8, 2, 0.05, 0.3)
    cls = want["cls"]
    counts = [int((cls == k).sum()) for k in (0, 1, 2)]
    assert min(counts) >= 5 and sum(counts) == 324
    assert same(vq.cls, cls) and same(vq.code, want["code"]) and same(vq.kept, want["kept"]) and same(vq.codebook, want["codebook"])
    assert same(vq.sigma, want["sigma"]) and vq.codebook.shape[0] == 8
    dq = pkg.volume.dequantize(vq)
    S = X.row_width(degree, True)
    assert same(dq.coef, Q.decode(cls, want["code"], want["kept"], want["codebook"])) and dq.coef.shape == (324, S)
    pruned, kept = on(dev, cls == 0), on(dev, cls == 2)
    assert not bits(dq.coef[pruned]).any() and not bits(dq.sigma[pruned]).any()    # +0 words, sigma +0
    assert same(dq.coef[kept], X.rows(rows32[cls == 2], True)) and same(dq.sigma[~pruned], cv.sigma[~pruned])
    assert same(dq.slot, cv.slot) and same(dq.occ, pkg.volume.with_block(dq, 2).occ)
    # nbytes from the class counts: point, sigma, cls per row; a code per coded row; a row per kept row and per code
    assert pkg.volume.nbytes(vq) == 324 * (4 + 4 + 1) + counts[1] * 2 + counts[2] * S * 2 + 8 * S * 2
    # the file: every array bit for bit; a dense and a compact file still load as what they are
    path = str(tmp_path / "vq.npz")
    pkg.volume.save(path, vq)
    back = pkg.volume.load(path, dev)
    assert isinstance(back, pkg.volume.VQVolume) and all(same(a, b) for a, b in zip(back[:8], vq[:8]))
    assert back[8:] == vq[8:] and back.point.dtype == torch.int32 and back.point.device.type == "cuda"
    with np.load(path) as z:
        assert sorted(z.files) == ["block", "cls", "code", "codebook", "degree", "kept", "lo", "mask", "shape", "sigma_rows", "step"]
        assert z["mask"].dtype == np.uint8 and z["mask"].size == (17 * 9 * 12 + 7) // 8
    assert same_compact(pkg.volume.dequantize(back), dq)
    pkg.volume.save(str(tmp_path / "c.npz"), cv)
    pkg.volume.save(str(tmp_path / "d.npz"), pkg.volume.unpack(cv))
    assert same_compact(pkg.volume.load(str(tmp_path / "c.npz"), dev), cv)
    dense = pkg.volume.load(str(tmp_path / "d.npz"), dev)
    assert isinstance(dense, pkg.volume.Volume) and same(dense.sigma, pkg.volume.unpack(cv).sigma)
    assert os.path.getsize(path) < os.path.getsize(str(tmp_path / "c.npz"))


def test_importance_views_and_refusals(pkg, dev):
    s = scene((9, 8, 7))
    cv = compact(pkg, dev, s)
    V = pkg.volume
    P = np.zeros((3, 3, 5), F)                                                     # the cameras of test_gpu_volume.py::test_render_views
    P[:, :, :3] = np.eye(3)
    P[:, :, 3] = [[0.5, 0.3, -3.0], [0.4, 0.2, -3.5], [0.45, 0.35, -2.5]]
    pb = torch.from_numpy(np.concatenate([P.reshape(3, 15), np.asarray([[1.0, 6.0], [2.0, 7.0], [0.5, 6.0]], F)], axis=1))
    K_inv = torch.tensor([[0.0, 0.02, 0.0], [0.02, 0.0, 0.0], [-0.12, -0.1, 1.0]])
    acc, steps = V.importance_views(cv, pb, K_inv, 12, 12)
    assert steps.shape == (3, 12, 12, 2) and same(steps, V.render_views(cv, pb, K_inv, 12, 12)[2]) and bool(acc.any())
    one = None
    for v in range(3):
        one, _ = V.importance_views(cv, pb[v:v + 1], K_inv, 12, 12, acc=one)
    assert same(one, acc) and same(V.importance_views(cv, pb, K_inv, 12, 12, views_per_call=2)[0], acc)
    imp, _ = imp_of(pkg, dev, s, cv)
    rays = rays_on(dev, s)
    with pytest.raises(TypeError, match="CompactVolume"):
        V.importance(V.unpack(cv), *rays)
    with pytest.raises(TypeError, match="CompactVolume"):
        V.quantize(V.unpack(cv), imp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.importance(cv, rays[0].cpu(), *rays[1:])
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.quantize(cv, imp.cpu())
    for K in (0, 65537, -1, 2.5):
        with pytest.raises(ValueError, match="65536"):
            V.quantize(cv, imp, K=K)
        with pytest.raises(ValueError, match="65536"):
            V.kmeans(cv.coef, imp, K, 1)
    with pytest.raises(ValueError):
        V.quantize(cv, imp[:-1])
    with pytest.raises(ValueError):
        V.quantize(cv, imp, prune_share=1.5)
    vq = V.quantize(cv, imp, K=4, iters=1)
    for call in (lambda: V.render(vq, *rays), lambda: V.sample(vq, rays[0], rays[1]), lambda: V.render_views(vq, pb, K_inv, 4, 4),
                 lambda: V.CompactFinetuner(vq), lambda: V.Finetuner(vq), lambda: V.importance(vq, *rays)):
        with pytest.raises(TypeError, match="dequantize"):
            call()
    L = pkg._abi.lib()
    assert L.nerf_hip_volume_vq_assign(cv.coef.data_ptr(), 4, cv.coef.data_ptr(), 0, 2, cv.slot.data_ptr(), None, None) == -1
    assert L.nerf_hip_volume_vq_assign(cv.coef.data_ptr(), 4, cv.coef.data_ptr(), 65537, 2, cv.slot.data_ptr(), None, None) == -1
    assert L.nerf_hip_volume_vq_assign(cv.coef.data_ptr(), 4, cv.coef.data_ptr(), 2, 3, cv.slot.data_ptr(), None, None) == -1
    assert L.nerf_hip_volume_vq_update(cv.coef.data_ptr(), 2, 2, imp.data_ptr() + 4, imp.data_ptr(), None) == -1


def test_runner(pkg, dev, tmp_path, capsys):
    """--volume 16 --volume-compact fp16 --volume-vq 32 --volume-vq-prune 0.01 --volume-preview train, as main.py passes them"""
    tmp = str(tmp_path)
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/rs/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=1, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=1)
    with pytest.raises(ValueError, match="compact"):
        run.bake_volume(16, save=False, vq=32)
    with pytest.raises(ValueError, match="65536"):
        run.bake_volume(16, save=False, compact="fp16", vq=0)
    capsys.readouterr()
    vol = run.bake_volume(16, compact="fp16", save=True, preview="train", vq=32, vq_iters=2, vq_prune=0.01, vq_keep=0.1)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VOLUME]")]
    assert len(lines) == 3 and " vq 32 codes, 2 iterations over 2 train views" in lines[2]
    assert "[PSNR] compact" in lines[2] and "dequantized" in lines[2] and "[SSIM] compact" in lines[2]
    assert isinstance(vol, pkg.volume.CompactVolume) and vol.coef.dtype == torch.float16
    info = run.last_volume_vq
    path = f"{tmp}/rs/{run.start_time}_{run.last_iter}_volume16_c16_vq32.npz"
    assert info["path"] == path and os.path.exists(path) and os.path.exists(path.replace("_vq32", ""))
    vq = pkg.volume.load(path, dev)
    n = int(vol.sigma.shape[0])
    assert isinstance(vq, pkg.volume.VQVolume) and vq.shape == (16, 16, 16) and vq.cls.shape == (n,) and n > 32
    assert info["pruned"] + info["coded"] + info["kept"] == n and info["K"] == 32 == vq.codebook.shape[0]
    assert info["nbytes"] == pkg.volume.nbytes(vq) < info["compact_nbytes"]
    dq = pkg.volume.dequantize(vq)
    assert same(dq.slot, vol.slot) and dq.coef.shape == vol.coef.shape and np.isfinite(info["psnr_vq"]) and np.isfinite(info["psnr_compact"])
