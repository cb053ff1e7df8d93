"""GPU: fine-tuning vector-quantised SH radiance volumes (csrc/volume_vq_train.hip; rules VQ-X, VQ-G and VQ-V of include/nerf_hip.h) --
expand, reduce and update against the numpy restatements bit for bit (the reduce also against Python integer sums, under every
permutation of the members), the tuner against CompactFinetuner where the two must agree, one whole step against the restatement fed
the device's own accumulators, the invariants over five steps, volume(), the file round trip, refusals, learning and the runner."""
import os

import numpy as np
import pytest
import torch

import volume_grad_reference as GR
import volume_vq_reference as Q
import volume_vq_train_reference as TR

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))   # 27 / 130 / 324 rows
ROWS = (27, 130, 324)
NRAYS = 300
DT = Q.DT
BG = (0.25, 0.5, 1.0)
C = TR.CHUNK                                     # VQT_CHUNK of csrc/kernels.h
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
        s = Q.scene(shape, nrays=NRAYS)
        s["target"] = np.random.default_rng(5).uniform(0.0, 1.0, (NRAYS, 3)).astype(F)
        _cache[shape] = s
    return _cache[shape]


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def compact(pkg, dev, s, block=2, degree=2, dtype="fp32"):
    sg = on(dev, s["sigma"])
    dv = pkg.volume.Volume(sg, on(dev, s["coef"][..., :(degree + 1) ** 2, :]), pkg.volume.blocks(sg, block), s["lo"], s["step"],
                           min(block, pkg.volume.ONE_BLOCK), degree)
    return pkg.volume.pack(dv, dtype)


def rays_on(dev, s, sel=slice(None)):
    return tuple(on(dev, s[k][sel]) for k in ("o", "d", "tmin", "tmax"))


def quantized(pkg, dev, shape, degree=2, **kw):
    """the scene's compact volume and its VQVolume for quantize's keywords"""
    s = scene(shape)
    cv = compact(pkg, dev, s, 2, degree)
    imp, _ = pkg.volume.importance(cv, *rays_on(dev, s), dt=DT, t_stop=0.3)
    return s, cv, pkg.volume.quantize(cv, imp, **kw)


# ---- rule VQ-X ----

@pytest.mark.parametrize("degree", (0, 1, 2))
def test_expand(pkg, dev, degree):
    rng = np.random.default_rng(degree)
    n, K = 700, 37                                                                 # 700 x 27 words: several workgroups, the last partial
    cls, rank, code, kept32, book32 = TR.random_classes(rng, n, K, degree)
    W = kept32.shape[1]
    acc = rng.integers(1, 2 ** 40, (n, W)).astype(np.int64)
    want_acc = acc.copy()
    want = TR.expand(cls, rank, code, kept32, book32, want_acc)
    d_acc = on(dev, acc)
    args = (on(dev, cls), on(dev, rank), on(dev, code), on(dev, kept32), on(dev, book32), degree)
    got = pkg.ops.volume_vq_expand(*args, acc_coef_rows=d_acc)
    assert same(got, want) and same(d_acc, want_acc) and got.shape == (n, W)
    zero = ~bits(want).any(1)                                                      # bad classes, ranks and codes give +0
    assert zero.sum() == (cls == 0).sum() + 6 and not want_acc[zero].any() and want_acc[~zero].all()
    out = torch.full((n, W), 7.0, device=dev)                                      # into given rows, the accumulators left alone
    assert pkg.ops.volume_vq_expand(*args, out=out) is out and same(out, want)
    none = pkg.ops.volume_vq_expand(args[0][:0], args[1][:0], args[2][:0], args[3][:0], args[4][:0], degree)
    assert none.shape == (0, W)


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_expand_is_decode_in_fp32(pkg, dev, degree):
    """rule VQ-D: convert() of the fp32 expansion of the fp16-exact masters equals dequantize's rows; the working volume is dequantize's"""
    _, cv, vq = quantized(pkg, dev, (17, 9, 12), degree, K=37, iters=2, prune_share=0.05, keep_share=0.3)
    assert min(int((vq.cls == k).sum()) for k in (0, 1, 2)) >= 5
    tuner = pkg.volume.VQFinetuner(vq)
    dq = pkg.volume.dequantize(vq)
    half = pkg.volume.convert(tuner.cvol, "fp16")
    assert tuner.cvol.coef.dtype == torch.float32 and tuner.cvol.coef.shape == (324, 3 * (degree + 1) ** 2)
    assert same(half.coef, dq.coef) and same(half.slot, dq.slot) and same(half.sigma, dq.sigma) and same(half.occ, dq.occ)
    assert same(tuner.codebook32, host(vq.codebook)[:, :tuner.codebook32.shape[1]].astype(F))


# ---- rule VQ-G ----

@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("degree", (0, 1, 2))
def test_reduce(pkg, dev, degree, big):
    """synthetic accumulators, no lattice: codes with 0, 1, C - 1, C, C + 1 and 2 C + 3 members and an empty code between full ones"""
    W = 3 * (degree + 1) ** 2
    rng = np.random.default_rng(10 + degree)
    counts = [0, 1, C - 1, 0, C, C + 1, 2 * C + 3, 0]
    K, n_coded = len(counts), sum(counts)
    n = n_coded + 40                                                               # 40 rows of other classes: kept, pruned
    member = rng.permutation(n)[:n_coded].astype(np.int32)
    offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    lim = 2 ** 61 // (2 * C + 3) if big else 2 ** 44
    acc = rng.integers(-lim, lim, (n, W)).astype(np.int64)
    start = rng.integers(-2 ** 40, 2 ** 40, (K, W)).astype(np.int64)
    want = [[int(start[j, w]) + sum(int(acc[r, w]) for r in member[offset[j]:offset[j + 1]]) for w in range(W)] for j in range(K)]
    want = np.asarray(want, np.int64)
    consumed = np.zeros(n, bool)
    consumed[member] = True

    def run(mem, off=offset):
        rows, codes = on(dev, acc), on(dev, start)
        assert pkg.ops.volume_vq_grad_reduce(rows, on(dev, off), on(dev, mem), codes) is codes
        return host(rows), host(codes)

    rows, codes = run(member)
    assert same(codes, want) and (not big or np.abs(want).max() > 2 ** 55)
    assert not rows[consumed].any() and same(rows[~consumed], acc[~consumed])      # consumed words zero, every other row untouched
    for seed in range(3):                                                          # members permuted within their codes
        perm, prng = member.copy(), np.random.default_rng(seed)
        for j in range(K):
            perm[offset[j]:offset[j + 1]] = prng.permutation(perm[offset[j]:offset[j + 1]])
        prows, pcodes = run(perm)
        assert same(pcodes, want) and same(prows, rows), seed
    bad = member.copy()                                                            # a member outside [0, n) is skipped
    bad[[1, C + 5, n_coded - 1]] = (-1, n, 2 ** 31 - 1)
    brows, bcodes = run(bad)
    w_rows, w_codes = acc.copy(), start.copy()
    TR.reduce(w_rows, offset, bad, w_codes)
    assert same(bcodes, w_codes) and same(brows, w_rows) and same(brows[member[1]], acc[member[1]])
    wild = offset.copy()                                                           # offsets past the members are clamped to them
    wild[-2:] = 2 ** 31 - 1
    wrows, wcodes = run(member, wild)
    assert same(wcodes, want) and same(wrows, rows)
    empty = on(dev, start)                                                         # no coded rows: nothing is launched
    pkg.ops.volume_vq_grad_reduce(on(dev, acc), on(dev, np.zeros(K + 1, np.int32)), on(dev, member[:0]), empty)
    assert same(empty, start)


def test_reduce_one_code_on_a_lattice(pkg, dev):
    """K = 1 at 324 rows: every row in one code, across the chunk edge; the accumulators are the device's own"""
    s, cv, vq = quantized(pkg, dev, (17, 9, 12), 2, K=1, iters=1)
    assert bool((vq.cls == 1).all()) and vq.codebook.shape[0] == 1 and 324 > C
    tuner = pkg.volume.VQFinetuner(vq)
    assert tuner.offset.tolist() == [0, 324] and same(tuner.member, np.arange(324, dtype=np.int32))
    g = on(dev, np.random.default_rng(7).normal(0.0, 1.0, (NRAYS, 3)).astype(F))
    pkg.volume.compact_render_backward(tuner.cvol, tuner.grad, *rays_on(dev, s), g, dt=DT, t_stop=0.3, background=BG)
    rows = host(tuner.grad.acc_coef).copy()
    assert np.count_nonzero(rows) > 324
    pkg.ops.volume_vq_grad_reduce(tuner.grad.acc_coef, tuner.offset, tuner.member, tuner.acc_code)
    assert same(tuner.acc_code, rows.sum(0, keepdims=True)) and not tuner.grad.acc_coef.any() and tuner.grad.acc_sigma.any()


# ---- rule VQ-V ----

@pytest.mark.parametrize("degree", (0, 1, 2))
def test_update(pkg, dev, degree):
    rng = np.random.default_rng(20 + degree)
    n, K = 300, 37
    cls, rank, code, kept32, book32 = TR.random_classes(rng, n, K, degree, bad=False)
    W, n_kept = kept32.shape[1], kept32.shape[0]
    kept_row = np.flatnonzero(cls == 2).astype(np.int32)
    kept_row[2] = n                                                                # outside the rows: its words are left alone
    sigma = rng.uniform(0.2, 3.0, n).astype(F)
    sigma[::7] = 0                                                                 # dead rows
    words = n + (n_kept + K) * W
    H = dict(s=sigma.copy(), k=kept32.copy(), b=book32.copy(), m=np.zeros(words, F), v=np.zeros(words, F))
    D = {k: on(dev, x) for k, x in H.items()}
    d_kept_row = on(dev, kept_row)
    owned = np.zeros(n, bool)
    owned[kept_row[kept_row < n]] = True
    for step in (1, 2, 3):                                                         # one step, then three: every step is compared
        aS, aR, aC = (rng.integers(-2 ** 44, 2 ** 44, sh).astype(np.int64) for sh in ((n,), (n, W), (K, W)))
        dS, dR, dC = on(dev, aS), on(dev, aR), on(dev, aC)
        TR.update(H["s"], H["k"], kept_row, H["b"], aS, aR, aC, H["m"], H["v"], 1.0 / 900, step, 2.0, 0.05)
        pkg.ops.volume_vq_adam_step(D["s"], D["k"], d_kept_row, D["b"], degree, dS, dR, dC, D["m"], D["v"], 1.0 / 900, step, 2.0, 0.05)
        assert all(same(D[k], H[k]) for k in H), step
        assert not dS.any() and not dC.any() and not dR[on(dev, owned)].any() and same(dR, aR)     # every accumulator read is zero
    assert not D["s"][::7].any() and not D["m"][:n][::7].any() and not D["v"][:n][::7].any()    # a dead row: sigma, m, v left alone
    assert bool((D["s"] > 0).any()) and bool((D["s"][1::7] == 0).any())                         # a live sigma reached 0 at this rate
    assert same(D["k"][2], kept32[2]) and not D["m"][n + 2 * W:n + 3 * W].any()


# ---- the tuner against CompactFinetuner, where the two must agree ----

def steps_of(tuner, rays, target, k=3):
    return [tuner.step(*rays, target, background=BG, dt=DT, t_stop=0.0) for _ in range(k)]


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("case", ("one row per code", "every row kept"))
def test_identity_with_the_compact_tuner(pkg, dev, case, degree):
    kw = dict(K=65536, iters=0) if case == "one row per code" else dict(K=4, iters=1, keep_share=1)
    s, cv, vq = quantized(pkg, dev, (9, 8, 7), degree, **kw)
    n = 130
    if case == "one row per code":
        assert bool((vq.cls == 1).all()) and sorted(host(vq.code).tolist()) == list(range(n))    # the codes are a permutation
    else:
        assert bool((vq.cls == 2).all()) and vq.codebook.shape[0] == 0 and vq.kept.shape[0] == n
    rays, target = rays_on(dev, s), on(dev, s["target"])
    lrs = dict(lr_sigma=2.0, lr_coef=0.02)                                         # a rate at which sigmas reach 0
    vt, ct = pkg.volume.VQFinetuner(vq, **lrs), pkg.volume.CompactFinetuner(pkg.volume.dequantize(vq), **lrs)
    la, lb = steps_of(vt, rays, target), steps_of(ct, rays, target)
    assert all(same(a, b) for a, b in zip(la, lb)) and la[0].dim() == 0 and float(la[0]) > 0
    assert same(vt.cvol.sigma, ct.cvol.sigma) and same(vt.cvol.coef, ct.cvol.coef) and vt.steps == 3
    masters = vt.codebook32[vq.code.long()] if case == "one row per code" else vt.kept32
    assert same(masters, ct.cvol.coef) and not same(ct.cvol.coef, pkg.volume.convert(cv, "fp32").coef)
    print(f"{case}, degree {degree}: {int(((vt.cvol.sigma == 0) & (vq.sigma > 0)).sum())} sigmas reached 0 in three steps")
    assert not vt.grad.acc_sigma.any() and not vt.grad.acc_coef.any() and not vt.acc_code.any()


# ---- the general case ----

def general(pkg, dev, degree=2):
    s, cv, vq = quantized(pkg, dev, (17, 9, 12), degree, K=37, iters=2, prune_share=0.05, keep_share=0.3)
    assert min(int((vq.cls == k).sum()) for k in (0, 1, 2)) >= 5 and vq.codebook.shape[0] == 37
    return s, vq


def manual_step(pkg, dev, s, t, parts, lr=(0.5, 0.02)):
    """VQFinetuner.step at the ops level, the batch given as the ray selections ``parts`` into the accumulators before ONE update"""
    rgb = pkg.volume.render(t.cvol, *rays_on(dev, s), dt=DT, t_stop=0.0, background=BG)[0]
    g = host(2.0 * (rgb - on(dev, s["target"])))
    for sel in parts:
        pkg.volume.compact_render_backward(t.cvol, t.grad, *rays_on(dev, s, sel), on(dev, g[sel]), dt=DT, t_stop=0.0, background=BG)
    before = (host(t.grad.acc_sigma).copy(), host(t.grad.acc_coef).copy())
    pkg.ops.volume_vq_grad_reduce(t.grad.acc_coef, t.offset, t.member, t.acc_code)
    t.steps += 1
    pkg.ops.volume_vq_adam_step(t.cvol.sigma, t.kept32, t.kept_row, t.codebook32, t.cvol.degree, t.grad.acc_sigma, t.grad.acc_coef, t.acc_code,
                                t.m, t.v, 1.0 / (3 * NRAYS), t.steps, lr[0], lr[1])
    pkg.ops.volume_vq_expand(t.cls, t.rank, t.code, t.kept32, t.codebook32, t.cvol.degree, out=t.cvol.coef, acc_coef_rows=t.grad.acc_coef)
    return before


def state_equal(t, st):
    return (same(t.cvol.sigma, st.c.sigma) and same(t.cvol.coef, st.c.coef) and same(t.kept32, st.kept32) and same(t.codebook32, st.codebook32)
            and same(t.m, st.m) and same(t.v, st.v))


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_one_step_against_the_restatement(pkg, dev, degree):
    """the house rule, against its own operands: the restated reduce, update and expand are fed the accumulators the device's own
    compact_render_backward filled for the working volume; two steps, so the second starts from updated masters and moments"""
    s, vq = general(pkg, dev, degree)
    t = pkg.volume.VQFinetuner(vq)
    st = TR.State((17, 9, 12), s["index"], host(vq.sigma), host(vq.cls), host(vq.code), host(vq.kept), host(vq.codebook), degree)
    assert same(t.offset, st.offset) and same(t.member, st.member) and same(t.kept_row, st.kept_row) and same(t.rank, st.rank)
    assert state_equal(t, st)
    for step in (1, 2):
        aS, aR = manual_step(pkg, dev, s, t, [slice(None)])
        assert np.count_nonzero(aR) > 324 and aR[host(vq.cls) == 0].any()          # a pruned row does receive, as a corner
        st.acc_sigma[...], st.acc_rows[...] = aS, aR
        st.apply(1.0 / (3 * NRAYS), 0.5, 0.02)
        assert state_equal(t, st), step
        assert not t.grad.acc_sigma.any() and not t.grad.acc_coef.any() and not t.acc_code.any()


def test_five_steps_keep_the_sharing_and_do_not_depend_on_the_order(pkg, dev):
    s, vq = general(pkg, dev)
    perm = np.random.default_rng(1).permutation(NRAYS)
    whole, permuted, halves = (pkg.volume.VQFinetuner(vq) for _ in range(3))
    coded, pruned = vq.cls == 1, vq.cls == 0
    start = whole.codebook32.clone()
    for step in range(5):
        manual_step(pkg, dev, s, whole, [slice(None)])
        manual_step(pkg, dev, s, permuted, [perm])
        manual_step(pkg, dev, s, halves, [slice(0, 130), slice(130, NRAYS)])
        for t in (permuted, halves):                                               # the same bits for permuted rays and a split batch
            assert all(same(getattr(t, k), getattr(whole, k)) for k in ("kept32", "codebook32", "m", "v")), step
            assert same(t.cvol.sigma, whole.cvol.sigma) and same(t.cvol.coef, whole.cvol.coef), step
        assert same(whole.cvol.coef[coded], whole.codebook32[vq.code.long()])      # rows that share a code stay bit-equal
        assert not bits(whole.cvol.coef[pruned]).any() and not bits(whole.cvol.sigma[pruned]).any()   # pruned rows stay +0
        assert not whole.grad.acc_coef.any() and not whole.grad.acc_sigma.any() and not whole.acc_code.any()
    assert not same(whole.codebook32, start) and len(np.unique(bits(whole.cvol.coef[coded]), axis=0)) <= 37
    # the class itself takes the same steps
    a, b = pkg.volume.VQFinetuner(vq, lr_sigma=0.5, lr_coef=0.02), pkg.volume.VQFinetuner(vq)
    rays, target = rays_on(dev, s), on(dev, s["target"])
    for _ in range(5):
        loss = a.step(*rays, target, background=BG, dt=DT, t_stop=0.0)
        manual_step(pkg, dev, s, b, [slice(None)])
    assert same(a.codebook32, b.codebook32) and same(a.cvol.sigma, b.cvol.sigma) and same(a.m, b.m) and loss.dim() == 0


# ---- volume(), the file ----

def test_volume_and_file(pkg, dev, tmp_path):
    s, vq = general(pkg, dev)
    V_ = pkg.volume
    t = V_.VQFinetuner(vq, lr_sigma=0.5, lr_coef=0.02)
    rays, target = rays_on(dev, s), on(dev, s["target"])
    steps_of(t, rays, target)
    out = t.volume()
    assert isinstance(out, V_.VQVolume) and same(out.point, vq.point) and same(out.cls, vq.cls) and same(out.code, vq.code)
    assert same(out.sigma, t.cvol.sigma) and out.sigma.data_ptr() != t.cvol.sigma.data_ptr() and out[8:] == vq[8:]
    assert same(out.lo, vq.lo) and same(out.step, vq.step)
    assert same(out.codebook, V_._rows_to_half(t.codebook32, 2)) and same(out.kept, V_._rows_to_half(t.kept32, 2))
    assert not same(out.codebook, vq.codebook) and not same(out.kept, vq.kept) and not same(out.sigma, vq.sigma)
    assert V_.nbytes(out) == V_.nbytes(vq)                                         # the small file stays as small
    path = str(tmp_path / "tuned.npz")
    V_.save(path, out)
    back = V_.load(path, dev)
    assert isinstance(back, V_.VQVolume) and all(same(a, b) for a, b in zip(back[:8], out[:8])) and back[8:] == out[8:]
    # dequantize(volume()) renders, and equals a render of the tuner's working rows rounded to fp16
    kw = dict(dt=DT, t_stop=0.3, background=BG)
    r1, r2 = V_.render(V_.dequantize(back), *rays, **kw), V_.render(V_.convert(t.cvol, "fp16"), *rays, **kw)
    assert all(same(a, b) for a, b in zip(r1, r2)) and bool(r1[2][:, 0].any())
    # a tuner on the result starts from the rounded masters
    again = V_.VQFinetuner(out)
    assert same(again.codebook32, host(out.codebook)[:, :27].astype(F)) and again.steps == 0


# ---- refusals ----

def test_refusals(pkg, dev):
    s, vq = general(pkg, dev)
    V_ = pkg.volume
    cv = V_.dequantize(vq)
    rays, target = rays_on(dev, s), on(dev, s["target"])
    for bad in (cv, V_.unpack(cv), None):
        with pytest.raises(TypeError, match="VQVolume"):
            V_.VQFinetuner(bad)
        with pytest.raises(TypeError, match="VQVolume"):
            V_.finetune_vq(bad, None, None, 1)
    cpu = vq._replace(**{k: getattr(vq, k).cpu() for k in ("point", "sigma", "cls", "code", "kept", "codebook")})
    with pytest.raises(RuntimeError, match="no CPU path"):
        V_.VQFinetuner(cpu)
    t = V_.VQFinetuner(vq)
    with pytest.raises(RuntimeError, match="no CPU path"):
        t.step(rays[0].cpu(), *rays[1:], target)
    big = torch.zeros(2 ** 20 + 1, 3, device=dev)
    with pytest.raises(ValueError, match="2\\^20"):
        t.step(big, big, 0.0, 1.0, big)
    with pytest.raises(ValueError, match="2\\^20"):
        V_.finetune_vq(vq, None, None, 1, batch=2 ** 20 + 1)
    assert t.steps == 0 and not t.grad.acc_coef.any()
    for call in (lambda: V_.CompactFinetuner(vq), lambda: V_.Finetuner(vq), lambda: V_.finetune_compact(vq, None, None, 1),
                 lambda: V_.compact_grad_buffers(vq), lambda: V_.render(vq, *rays)):
        with pytest.raises(TypeError, match="VQFinetuner"):
            call()
    # the ops layer: dtypes, shapes, devices
    O = pkg.ops
    with pytest.raises(ValueError):
        O.volume_vq_expand(t.cls, t.rank.long(), t.code, t.kept32, t.codebook32, 2)
    with pytest.raises(ValueError):
        O.volume_vq_expand(t.cls, t.rank, t.code, t.kept32[:, :12].contiguous(), t.codebook32, 2)
    with pytest.raises(ValueError):
        O.volume_vq_grad_reduce(t.grad.acc_coef, t.offset[:-1].contiguous(), t.member, t.acc_code)
    with pytest.raises(ValueError):
        O.volume_vq_grad_reduce(t.grad.acc_coef, t.offset.long(), t.member, t.acc_code)
    with pytest.raises(ValueError):
        O.volume_vq_adam_step(t.cvol.sigma, t.kept32, t.kept_row, t.codebook32, 2, t.grad.acc_sigma, t.grad.acc_coef, t.acc_code, t.m[:-1].contiguous(),
                              t.v, 1.0, 1, 0.1, 0.01)
    with pytest.raises(pkg._abi.NerfHipError):
        O.volume_vq_adam_step(t.cvol.sigma, t.kept32, t.kept_row, t.codebook32, 2, t.grad.acc_sigma, t.grad.acc_coef, t.acc_code, t.m, t.v, 1.0, 0,
                              0.1, 0.01)
    # the C entries, with device pointers
    L, P = pkg._abi.lib(), lambda x: x.data_ptr()
    n, n_coded, n_kept, K = 324, int(t.code.shape[0]), int(t.kept32.shape[0]), 37
    ok = lambda **kw: L.nerf_hip_volume_vq_grad_reduce(P(t.grad.acc_coef), kw.get("n", n), kw.get("degree", 2), P(t.offset), P(t.member),
                                                       kw.get("n_coded", n_coded), kw.get("K", K), kw.get("acc_code", P(t.acc_code)), None)
    assert ok() == 0
    for kw in (dict(n=-1), dict(degree=3), dict(n_coded=n + 1), dict(K=0), dict(K=65537), dict(acc_code=P(t.acc_code) + 4), dict(acc_code=None)):
        assert ok(**kw) == -1 and L.nerf_hip_last_error(), kw
    ex = lambda **kw: L.nerf_hip_volume_vq_expand(P(t.cls), P(t.rank), n, P(t.code), kw.get("n_coded", n_coded), P(t.kept32),
                                                  kw.get("n_kept", n_kept), P(t.codebook32), kw.get("K", K), 2, kw.get("out", P(t.cvol.coef)),
                                                  None, None)
    assert ex() == 0
    for kw in (dict(n_coded=n), dict(n_kept=-1), dict(K=0), dict(out=None), dict(out=P(t.cvol.coef) + 2)):
        assert ex(**kw) == -1 and L.nerf_hip_last_error(), kw
    torch.cuda.synchronize()


# ---- learning ----

def test_learning(pkg, dev):
    """tests/test_volume_vq_train_cpu.py::test_learning's seeded case on the device: the teacher of the dense learning case quantised at
    K = 2 by the restatement, LEARN_STEPS steps at the default rates; the final loss must be below LEARN_MARGIN x the first -- the margin
    chosen there, on the restatement alone (observed there: x 0.466)."""
    case = TR.learning_case()
    q = case["q"]
    vq = pkg.volume.VQVolume(on(dev, case["index"].astype(np.int32)), on(dev, q["sigma"]), on(dev, q["cls"]), on(dev, q["code"]),
                             on(dev, q["kept"]), on(dev, q["codebook"]), case["lo"], case["step"], 2, 2, GR.LEARN_SHAPE)
    t = pkg.volume.VQFinetuner(vq)
    rays = tuple(on(dev, case[k]) for k in ("o", "d", "tmin", "tmax"))
    target = on(dev, case["target"])
    kw = dict(background=GR.LEARN_BG, dt=GR.LEARN_DT, t_stop=0.0)
    losses = [float(x) for x in torch.stack([t.step(*rays, target, **kw) for _ in range(TR.LEARN_STEPS)]).cpu()]
    rgb = pkg.volume.render(t.cvol, *rays, **kw)[0]
    losses.append(float(((rgb - target) ** 2).mean()))
    print(f"device VQ fine-tuning: loss {losses[0]:.4e} -> {losses[-1]:.4e} (x {losses[-1] / losses[0]:.3f}) over {TR.LEARN_STEPS} steps")
    assert losses[-1] < TR.LEARN_MARGIN * losses[0]
    assert len(np.unique(bits(t.cvol.coef), axis=0)) == 2                          # the sharing is intact: two distinct rows


# ---- the runner ----

def test_runner(pkg, dev, tmp_path, capsys):
    """--volume 16 --volume-compact fp16 --volume-vq 16 --volume-vq-finetune 4 --volume-preview train, as main.py passes them"""
    tmp = str(tmp_path)
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/rs/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=1, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=1)
    with pytest.raises(ValueError, match="vq_finetune"):
        run.bake_volume(16, save=False, compact="fp16", vq_finetune=4)
    capsys.readouterr()
    vol = run.bake_volume(16, compact="fp16", save=True, preview="train", vq=16, vq_iters=2, vq_keep=0.1, vq_finetune=4, vq_finetune_batch=128)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VOLUME]")]
    assert len(lines) == 3 and " vq 16 codes, 2 iterations over 2 train views" in lines[2]
    assert "vq finetune 4 steps of 128 train rays: batch loss" in lines[2] and "[PSNR] tuned" in lines[2] and "[SSIM] tuned" in lines[2]
    assert isinstance(vol, pkg.volume.CompactVolume)
    info = run.last_volume_vq
    path = f"{tmp}/rs/{run.start_time}_{run.last_iter}_volume16_c16_vq16.npz"
    assert info["path"] == path and info["finetune_path"] == path[:-4] + "_ft4.npz" and os.path.exists(path) and os.path.exists(info["finetune_path"])
    assert info["finetune_iters"] == 4 and info["first_loss"] > 0 and info["last_loss"] > 0 and info["finetune_seconds"] > 0
    assert np.isfinite(info["psnr_vq_ft"]) and np.isfinite(info["ssim_vq_ft"]) and np.isfinite(info["psnr_vq"])
    raw, tuned = pkg.volume.load(path, dev), pkg.volume.load(info["finetune_path"], dev)
    assert isinstance(tuned, pkg.volume.VQVolume) and same(tuned.cls, raw.cls) and same(tuned.code, raw.code) and same(tuned.point, raw.point)
    assert not same(tuned.codebook, raw.codebook) and pkg.volume.nbytes(tuned) == pkg.volume.nbytes(raw) == info["nbytes"]
    assert os.path.getsize(info["finetune_path"]) < 1.05 * os.path.getsize(path)
