"""No GPU: the restatements of rules VI, VQ-A, VQ-U, VQ-D, of volume.vq_classes and of the k-means init
(tests/volume_vq_reference.py), each vectorised form against its scalar-loops form; volume.vq_classes itself (exact integer plumbing,
it runs on CPU tensors) on hand-made importances; the identity codebook; the k-means objective on the seeded scene; the planted
mistakes of rule VI against the derived budget; and what the package and the C entries refuse without a device."""
import os
import re

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_grad_reference as GR
import volume_vq_reference as Q

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def scene(shape, nrays=60):
    if (shape, nrays) not in _cache:
        s = Q.scene(shape, nrays=nrays)
        idx = GR.pad(s["G"], s["sig"])
        with np.errstate(all="ignore"):
            w, Tb, wa, valid = Q.forward32_all(s["G"], s["sig"], idx, 0.0)
        s.update(idx=idx, w=w, Tb=Tb, wa=wa, valid=valid, imp=Q.importance_fixed(s["G"], idx, valid, w, s["slot"], s["n"]))
        _cache[(shape, nrays)] = s
    return _cache[(shape, nrays)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- rule VI ----

@pytest.mark.parametrize("shape", ((5, 4, 3), (9, 8, 7)))
def test_importance_vectorised_equals_loops(shape):
    s = scene(shape)
    G, idx, valid = s["G"], s["idx"], s["valid"]
    j = idx[valid]
    loops = Q.importance_loops(G.f[j], G.ci[j], s["w"][valid], s["slot"], s["n"])
    assert s["imp"].dtype == np.int64 and np.array_equal(s["imp"], np.asarray(loops, np.int64))
    assert (s["imp"] > 0).sum() > s["n"] // 3
    # a corner without a row receives nothing, the other rows are untouched
    r = int(np.argmax(s["imp"]))
    for bad in (-1, s["n"], -7):
        slot = s["slot"].copy()
        slot.reshape(-1)[s["index"][r]] = bad
        less = Q.importance_fixed(G, idx, valid, s["w"], slot, s["n"])
        keep = np.arange(s["n"]) != r
        assert less[r] == 0 and np.array_equal(less[keep], s["imp"][keep])


@pytest.mark.parametrize("t_stop", (0.0, 0.3))
def test_importance_budget_and_planted_mistakes(t_stop):
    s = scene((9, 8, 7), nrays=120)
    G, slot, n = s["G"], s["slot"], s["n"]
    with np.errstate(all="ignore"):
        ref = Q.importance_reference(G, s["sig"], slot, n, t_stop=t_stop)
        idx, valid = ref["idx"], ref["valid"]
        w, Tb, wa, valid32 = Q.forward32_all(G, s["sig"], idx, t_stop)
    assert np.array_equal(valid, valid32)           # the fp32 recurrence ends every ray where the fp64 one does, on this scene
    assert (ref["budget"] > 0).sum() > n // 3 and ref["budget"].max() < 1e-3
    good = Q.importance_ratio(Q.importance_fixed(G, idx, valid, w, slot, n), ref)
    assert good <= 1.0, good
    for mutate in ("T", "no_wz", "w_after"):
        bad = Q.importance_ratio(Q.importance_fixed(G, idx, valid, w, slot, n, mutate=mutate, T_before=Tb, w_after=wa), ref)
        assert bad > 100.0, (mutate, bad)


# ---- the classes ----

def test_classes_hand_made():
    imp = np.asarray([0, 5, 5, 0, 10, 20, 40, 0], np.int64)       # total 80; the order: rows 0, 3, 7 (0), 1, 2 (5), 4, 5, 6
    # prune 0.25 -> threshold 20: the running sums 0, 0, 0, 5, 10, 20, 40, 80 -> rows 0, 3, 7, 1, 2, 4 are pruned
    assert list(Q.classes(imp, 0.25)) == [0, 0, 0, 0, 0, 1, 1, 0]
    # keep 0.5 -> threshold 40: from the top 40, 60 -> row 6 alone is kept; None prunes nothing, not even the zeros
    assert list(Q.classes(imp, None, 0.5)) == [1, 1, 1, 1, 1, 1, 2, 1]
    # prune 0 prunes exactly the rows of importance 0; keep 0.75 -> threshold 60: rows 6 and 5
    assert list(Q.classes(imp, 0, 0.75)) == [0, 1, 1, 0, 1, 2, 2, 0]
    # a tie at the threshold: prune 1/16 -> threshold 5: only the LOWER row of the two fives goes
    assert list(Q.classes(imp, 0.0625)) == [0, 0, 1, 0, 1, 1, 1, 0]
    # a share that floating point would get wrong: total 10^17 + 1, share 1/3 -> the integer floor, exactly
    big = np.asarray([33333333333333333, 1, 66666666666666667], np.int64)
    assert list(Q.classes(big, 1 / 3)) == [1, 0, 1] and list(Q.classes(big, 0.34)) == [0, 0, 1]
    # rows: a NaN word, an inf word and a word above 1024 are kept whatever the importance, 1024 itself is not
    rows = np.zeros((8, 3), F)
    rows[0, 1], rows[3, 2], rows[7, 0], rows[1, 0] = np.nan, np.inf, -1024.5, 1024.0
    assert list(Q.classes(imp, 0.25, 0.0, rows)) == [2, 0, 0, 2, 0, 1, 1, 2]
    # all zero: every running sum meets both thresholds; pruning wins where it is asked for
    zero = np.zeros(4, np.int64)
    assert list(Q.classes(zero)) == [2] * 4 and list(Q.classes(zero, 0.5)) == [0] * 4
    assert Q.classes(np.zeros(0, np.int64), 0.5).shape == (0,)


def test_classes_vectorised_equals_loops_and_package(pkg):
    rng = np.random.default_rng(3)
    for trial in range(12):
        n = int(rng.integers(1, 60))
        imp = (rng.integers(0, 6, n) * rng.integers(0, 1 << 40, n)).astype(np.int64)     # zeros and ties included
        imp[rng.integers(0, n, n // 3)] = imp[0]
        rows = rng.normal(0, 400, (n, 12)).astype(F)
        rows[rng.integers(0, n), 3] = np.nan
        for prune, keep in ((None, 0.0), (0.25, 0.0), (0.001, 0.5), (0.5, 0.5), (0, 1), (1, 0.25)):
            for r in (None, rows):
                want = Q.classes_loops(imp, prune, keep, r)
                assert np.array_equal(Q.classes(imp, prune, keep, r), want), (trial, prune, keep)
                got = pkg.volume.vq_classes(torch.from_numpy(imp), prune, keep, None if r is None else torch.from_numpy(r))
                assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (trial, prune, keep)
    with pytest.raises(ValueError):
        pkg.volume.vq_classes(torch.zeros(3, dtype=torch.int64), 1.5)
    with pytest.raises(ValueError):
        pkg.volume.vq_classes(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        pkg.volume.vq_classes(torch.tensor([1, -1], dtype=torch.int64))


# ---- VQ-A, VQ-U, the init, VQ-D ----

@pytest.mark.parametrize("W", (3, 12, 27))
def test_assign_vectorised_equals_loops(W):
    rng = np.random.default_rng(W)
    q = rng.normal(0, 1, (23, W)).astype(F)
    c = rng.normal(0, 1, (9, W)).astype(F)
    c[5] = c[2]                                   # duplicated codes: the lowest index wins
    q[4] = c[2]
    c[0, 1] = np.nan                              # a NaN code never wins
    q[7, 0] = np.inf                              # every distance +inf (or NaN): nothing wins, code 0
    q[8, 2] = np.nan
    code, dist = Q.assign(q, c)
    code2, dist2 = Q.assign_loops(q, c)
    assert np.array_equal(code, code2) and same(dist, dist2)
    assert code[4] == 2 and dist[4] == 0 and (code != 0).sum() >= 20 and (code != 5).all()
    assert code[7] == 0 and code[8] == 0 and np.isinf(dist[7]) and np.isinf(dist[8])
    one, d1 = Q.assign(q, c[:1])                  # a single NaN code
    assert (one == 0).all() and np.isinf(d1).all()


def test_update_vectorised_equals_loops():
    rng = np.random.default_rng(5)
    q = rng.normal(0, 30, (40, 12)).astype(F)
    weight = (rng.integers(0, 3, 40) * rng.integers(1, 1 << 45, 40)).astype(np.int64)
    code = rng.integers(0, 7, 40).astype(np.int32)
    code[code == 3] = 4                           # code 3 stays empty
    code[5], code[6] = -1, 7                      # outside [0, K): skipped
    c = rng.normal(0, 1, (7, 12)).astype(F)
    for wgt in (weight, None, np.zeros(40, np.int64)):
        S, N = Q.accumulate(q, wgt, code, 7)
        S2, N2 = Q.accumulate_loops(q, wgt, code, 7)
        assert np.array_equal(S, S2) and np.array_equal(N, N2) and N[3] == 0 and not S[3].any()
        new = Q.update(c, S, N)
        assert same(new, Q.update_loops(c, S, N)) and same(new[3], c[3]) and not same(new[4], c[4])
    S1, N1 = Q.accumulate(q, None, code, 7)       # unit weights: N counts the rows in units of 2^20
    assert np.array_equal(N1, np.bincount(code[(code >= 0) & (code < 7)], minlength=7) << 20)
    perm = rng.permutation(40)                    # integer sums: the order of the rows plays no role
    Sp, Np = Q.accumulate(q[perm], weight[perm], code[perm], 7)
    S, N = Q.accumulate(q, weight, code, 7)
    assert np.array_equal(S, Sp) and np.array_equal(N, Np)


def test_init_and_decode_vectorised_equal_loops():
    rng = np.random.default_rng(9)
    q = rng.normal(0, 1, (31, 3)).astype(F)
    weight = rng.integers(0, 4, 31).astype(np.int64)              # many ties
    for K in (1, 2, 7, 31, 64):
        for wgt in (weight, None):
            assert same(Q.init(q, wgt, K), Q.init_loops(q, wgt, K))
    top = np.lexsort((np.arange(31), -weight))
    assert same(Q.init(q, weight, 31), q[top]) and same(Q.init(q, weight, 1), q[top[:1]])
    cls = rng.integers(0, 3, 31).astype(np.uint8)
    kept = X.rows(rng.normal(0, 1, (int((cls == 2).sum()), 3)).astype(F), True)
    book = X.rows(rng.normal(0, 1, (5, 3)).astype(F), True)
    code = rng.integers(0, 5, int((cls == 1).sum())).astype(np.uint16)
    out = Q.decode(cls, code, kept, book)
    assert same(out, Q.decode_loops(cls, code, kept, book)) and out.shape == (31, 4) and not bits(out[cls == 0]).any()


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_identity_codebook_decodes_to_the_fp16_rounding(degree):
    s = scene((9, 8, 7))
    nc = (degree + 1) ** 2
    words = np.ascontiguousarray(s["words"][:, :3 * nc])
    m = words.shape[0]
    for K in (m, m + 5, 65536):
        z = Q.quantize(s["sigma_rows"], words, s["imp"], K, 0)
        assert (z["cls"] == 1).all() and z["codebook"].shape == (m, X.row_width(degree, True)) and z["kept"].shape[0] == 0
        assert same(Q.decode(z["cls"], z["code"], z["kept"], z["codebook"]), X.rows(words, True))
        assert same(z["sigma"], s["sigma_rows"])
    # with classes: pruned rows decode to +0 with sigma +0, kept rows to their own rounding
    z = Q.quantize(s["sigma_rows"], words, s["imp"], 8, 2, prune_share=0.05, keep_share=0.3)
    out = Q.decode(z["cls"], z["code"], z["kept"], z["codebook"])
    assert min((z["cls"] == k).sum() for k in (0, 1, 2)) >= 5 and z["codebook"].shape[0] == 8
    assert not bits(out[z["cls"] == 0]).any() and not bits(z["sigma"][z["cls"] == 0]).any()
    assert same(out[z["cls"] == 2], X.rows(words[z["cls"] == 2], True)) and same(z["sigma"][z["cls"] != 0], s["sigma_rows"][z["cls"] != 0])


def test_kmeans_lowers_the_weighted_objective():
    """the condition of the seeded scene: lattice (9, 8, 7), make_volume(seed = 11), the importance of 60 make_rays rays as weights,
    K = 16 -- eight iterations bring the weighted fp64 objective below the initial codebook's"""
    s = scene((9, 8, 7))
    used = s["imp"] > 0
    rows, weight = s["words"][used], s["imp"][used]
    assert rows.shape[0] > 40
    c, code, trail = Q.kmeans(rows, weight, 16, 8)
    obj = [Q.objective(rows, weight, t) for t in trail]
    assert obj[8] < 0.8 * obj[0], obj
    assert code.min() >= 0 and code.max() < 16 and len(np.unique(code)) > 8
    c2, code2, _ = Q.kmeans(rows, weight, 16, 8)
    assert same(c, c2) and np.array_equal(code, code2)


# ---- what is refused without a device; the surface ----

def test_surface_and_refusals(pkg):
    hdr = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    for name in ("nerf_hip_volume_compact_importance", "nerf_hip_volume_vq_assign", "nerf_hip_volume_vq_accumulate",
                 "nerf_hip_volume_vq_update", "nerf_hip_volume_vq_decode"):
        assert re.search(r"\bint\s+" + name + r"\(", hdr) and name in pkg._abi.EXPORTS
    assert re.search(r"#define\s+NERF_HIP_VOLUME_VQ_SHIFT\s+20\b", hdr) and re.search(r"#define\s+NERF_HIP_VOLUME_VQ_MAX_CODES\s+65536\b", hdr)
    assert "volume_vq.hip" in open(os.path.join(ROOT, "nerf-tiny_amd", "csrc", "Makefile")).read()
    V = pkg.volume
    lo, step = np.zeros(3, F), np.ones(3, F)
    cpu = V.CompactVolume(torch.full((2, 2, 2), -1, dtype=torch.int32), torch.zeros(0), torch.zeros(0, 3), torch.zeros(1, 1, 1, dtype=torch.uint8),
                          lo, step, 1, 0, (2, 2, 2))
    rays = torch.zeros(1, 3), torch.ones(1, 3), 0.0, 1.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.importance(cpu, *rays)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.quantize(cpu, torch.zeros(0, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.kmeans(torch.zeros(4, 3), None, 2, 1)
    dense = V.Volume(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2, 1, 3), torch.zeros(1, 1, 1, dtype=torch.uint8), lo, step, 1, 0)
    with pytest.raises(TypeError, match="CompactVolume"):
        V.importance(dense, *rays)
    with pytest.raises(TypeError, match="CompactVolume"):
        V.quantize(dense, torch.zeros(8, dtype=torch.int64))
    vq = V.VQVolume(torch.zeros(0, dtype=torch.int32), torch.zeros(0), torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint16),
                    torch.zeros(0, 4, dtype=torch.float16), torch.zeros(0, 4, dtype=torch.float16), lo, step, 1, 0, (2, 2, 2))
    for call in (lambda: V.render(vq, *rays), lambda: V.sample(vq, rays[0], rays[1]), lambda: V.with_block(vq, 2), lambda: V.pack(vq),
                 lambda: V.render_views(vq, torch.zeros(1, 17), torch.eye(3), 2, 2), lambda: V.Finetuner(vq), lambda: V.CompactFinetuner(vq),
                 lambda: V.compact_grad_buffers(vq), lambda: V.importance(vq, *rays)):
        with pytest.raises(TypeError, match="dequantize"):
            call()
    assert V.nbytes(vq) == 0 and V.default_dt(vq) == 0.5
    with pytest.raises(TypeError):
        V.dequantize(cpu)
