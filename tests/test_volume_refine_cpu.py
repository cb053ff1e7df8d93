"""No GPU: the restatements of rules VM, VT, VX and VP (tests/volume_refine_reference.py) against torch.autograd in fp64, against the
coarse lookups within the bound derived in that module, with planted mistakes that have to leave each band, and the level-by-level
learning condition on the restatement alone."""
import os
import re

import numpy as np
import pytest
import torch

import volume_grad_reference as V
import volume_reference as R
import volume_refine_reference as X

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = [(5, 4, 3), (9, 8, 7)]
QUANT_BAND = 6 * 2.0 ** -41     # six contributions per word, each rounded to a multiple of 2^-40


def random_members(shape, seed, nc=9):
    rng = np.random.default_rng(seed)
    sigma = rng.uniform(0.0, 4.0, shape).astype(F)
    coef = rng.normal(0.0, 1.0, shape + (nc, 3)).astype(F)
    member = (rng.uniform(size=shape) < 0.7).astype(np.uint8)
    member[0, 0, 0] = member[-1, -1, -1] = 1            # members on the lattice's corners: their far ends are outside
    return sigma, coef, member


def autograd_tv(sigma, coef, member, w_sigma, w_coef, eps):
    """d / d words of the stated loss in fp64 -> [nx, ny, nz, W]"""
    Xw = torch.tensor(X.words(sigma, coef).astype(np.float64), requires_grad=True)
    mem = torch.tensor(member.astype(bool))
    ss = torch.zeros_like(Xw)
    for a in range(3):
        near, far = X._axis_slices(a)
        d = torch.zeros_like(Xw)
        ok = (mem[near] & mem[far])[..., None]
        d[near] = torch.where(ok, Xw[far] - Xw[near], torch.zeros_like(Xw[near]))
        ss = ss + d * d
    tau = torch.sqrt(ss + eps) * mem[..., None]
    loss = w_sigma * tau[..., 0].sum() + w_coef * tau[..., 1:].sum()
    loss.backward()
    return Xw.grad.numpy(), float(loss.detach())


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("w", [(1.0, 0.5), (3.0, 40.0)])
def test_vt_against_autograd(shape, w):
    sigma, coef, member = random_members(shape, seed=sum(shape))
    eps = 1e-9
    want, loss = autograd_tv(sigma, coef, member, w[0], w[1], eps)
    assert abs(X.tv_loss(sigma, coef, member, w[0], w[1], eps) - loss) <= 1e-12 * abs(loss)
    total = X.tv_totals(sigma, coef, member, w[0], w[1], eps)
    assert total.shape[-1] == 28
    wvec = np.concatenate([[w[0]], np.full(27, w[1])])
    err = np.abs(total.astype(np.float64) * 2.0 ** -X.SHIFT - want)
    band = QUANT_BAND * np.maximum(1.0, wvec)
    print("VT vs autograd: worst error / band", float((err / band).max()), "worst error", float(err.max()))
    assert (err <= band).all()
    assert not total[member == 0].any()                              # non-members receive nothing
    assert not total.reshape(-1, 28).sum(0).any()                    # per word type the integers sum to exactly 0
    # vt adds the rows of the list, and only those
    index = np.flatnonzero(member.reshape(-1))
    aS, aC = np.full(shape, 5, np.int64), np.full(shape + (9, 3), -7, np.int64)
    X.vt(sigma, coef, index[::2], member, w[0], w[1], eps, aS, aC)
    got = X.words(aS, aC).reshape(-1, 28)
    base = X.words(np.full(shape, 5, np.int64), np.full(shape + (9, 3), -7, np.int64)).reshape(-1, 28)
    rows = np.zeros(got.shape[0], bool)
    rows[index[::2]] = True
    assert np.array_equal(got[rows], (base + total.reshape(-1, 28))[rows]) and np.array_equal(got[~rows], base[~rows])


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("mutate", ["no_far_member", "no_backward", "eps_outside"])
def test_vt_planted_mistakes_leave_the_band(shape, mutate):
    """eps = 1e-3 here: at 1e-9 an eps outside the root moves the gradient by about 1e-9 only"""
    sigma, coef, member = random_members(shape, seed=1 + sum(shape))
    w, eps = (1.0, 0.5), 1e-3
    want, _ = autograd_tv(sigma, coef, member, w[0], w[1], eps)
    good = np.abs(X.tv_totals(sigma, coef, member, w[0], w[1], eps).astype(np.float64) * 2.0 ** -X.SHIFT - want).max()
    bad = np.abs(X.tv_totals(sigma, coef, member, w[0], w[1], eps, mutate=mutate).astype(np.float64) * 2.0 ** -X.SHIFT - want).max()
    assert good <= QUANT_BAND and bad > 1000 * QUANT_BAND, (good, bad)


def test_vm():
    m = X.member_mask([0, 59, 7, -1, 60, 2**31 - 1], (5, 4, 3))
    assert m.dtype == np.uint8 and m.shape == (5, 4, 3) and np.array_equal(np.flatnonzero(m.reshape(-1)), [0, 7, 59])


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_vx_shape_and_support(shape, degree):
    sigma, coef, lo, step = R.make_volume(shape, seed=11, degree=degree)
    keep = np.zeros(int(np.prod(shape)), bool)
    keep[R.active(sigma)] = True
    coef = (coef * keep.reshape(shape)[..., None, None]).astype(F)      # rule VS: inactive points keep 0
    s2, c2 = X.vx(sigma, coef)
    assert s2.shape == X.up_shape(shape) and c2.shape == X.up_shape(shape) + coef.shape[3:] and s2.dtype == F and c2.dtype == F
    assert (s2 >= 0).all()
    assert np.array_equal(s2[::2, ::2, ::2].view(np.uint32), sigma.view(np.uint32))
    assert np.array_equal(c2[::2, ::2, ::2].view(np.uint32), coef.view(np.uint32))
    act2 = np.zeros(s2.size, bool)
    act2[R.active(s2)] = True
    act2 = act2.reshape(s2.shape)
    assert act2[::2, ::2, ::2][keep.reshape(shape)].all()              # the refined points of the coarse support
    # (a fine point between an active coarse point with sigma 0 and an inactive one is NOT active, yet holds half a coefficient: the
    # refined coefficients outside the refined support are not all 0; nothing reads them, and rule VP at threshold 0 clears them)
    s3, c3 = X.vp(s2, c2, 0.0)
    assert np.array_equal(s3.view(np.uint32), s2.view(np.uint32)) and not c3[~act2].any()
    assert np.array_equal(c3[act2].view(np.uint32), c2[act2].view(np.uint32))
    assert np.array_equal(X.half_step(step) * F(2), step)


def quarter_points(lo, step, shape):
    """every quarter-step point of the box, both ends included, in fp32"""
    ax = [(lo[a] + (np.arange(4 * (shape[a] - 1) + 1).astype(F) * F(0.25)) * step[a]).astype(F) for a in range(3)]
    ax[0][-1], ax[1][-1], ax[2][-1] = [F(lo[a] + F(shape[a] - 1) * step[a]) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def test_vx_lookups_dyadic_bit_for_bit():
    shape = (5, 4, 3)
    lo, step = np.asarray([-1.0, -0.75, -0.5], F), np.asarray([0.5, 0.5, 0.5], F)
    rng = np.random.default_rng(3)
    sigma = (rng.integers(0, 24, shape) / 4.0).astype(F)
    coef = (rng.integers(-8, 9, shape + (1, 3)) / 4.0).astype(F)
    s2, c2 = X.vx(sigma, coef)
    x = quarter_points(lo, step, shape)
    d = np.broadcast_to(np.asarray([0.0, 0.0, 1.0], F), x.shape)
    a, _ = R.lookup(sigma, coef, lo, step, x, d)
    b, _ = R.lookup(s2, c2, lo, X.half_step(step), x, d)
    assert (a > 0).any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("degree", [0, 2])
def test_vx_lookups_within_the_derived_bound(shape, degree):
    sigma, coef, lo, step = R.make_volume(shape, seed=11, degree=degree)
    x = quarter_points(lo, step, shape)
    rng = np.random.default_rng(5)
    d = rng.normal(size=x.shape)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    bs, bc = X.lookup_bounds(sigma, coef, d)
    a_s, a_c = R.lookup(sigma, coef, lo, step, x, d)
    for f, inside in ((0.5, True), (0.25, False)):
        s2, c2 = X.vx(sigma, coef, f=f)
        b_s, b_c = R.lookup(s2, c2, lo, X.half_step(step), x, d)
        es = np.abs(a_s.astype(np.float64) - b_s)
        ec = np.abs(a_c.astype(np.float64) - b_c).max(1)
        print(f"f={f}: sigma worst / bound {es.max() / bs:.3g}, colour worst / bound {(ec / bc).max():.3g}")
        if inside:
            assert (es <= bs).all() and (ec <= bc).all()
        else:                                   # the planted mistake leaves the bound by a large factor
            assert es.max() > 1000 * bs and (ec / bc).max() > 1000


def test_vp():
    shape = (9, 8, 7)
    sigma, coef, lo, step = R.make_volume(shape, seed=11)
    act = np.zeros(sigma.size, bool)
    act[R.active(sigma)] = True
    clean = (coef * act.reshape(shape)[..., None, None]).astype(F)
    clean[clean == 0] = 0                                                    # -0 -> +0
    s0, c0 = X.vp(sigma, clean, 0.0)
    assert np.array_equal(s0.view(np.uint32), sigma.view(np.uint32)) and np.array_equal(c0.view(np.uint32), clean.view(np.uint32))
    # stale coefficients of dead points are cleared, a NaN sigma becomes 0
    s1, c1 = X.vp(sigma, coef, 0.0)
    assert np.array_equal(c1.view(np.uint32), clean.view(np.uint32)) and (coef[~act.reshape(shape)] != 0).any()
    sn = sigma.copy()
    sn[4, 4, 3] = np.nan
    assert X.vp(sn, coef, 0.0)[0][4, 4, 3] == 0 and not np.isnan(X.vp(sn, coef, 1.0)[0]).any()
    # a threshold: the march of the pruned volume is the march of the same sigma with junk in the cleared words
    s2, c2 = X.vp(sigma, coef, 3.0)
    assert 0 < (s2 > 0).sum() < (sigma > 0).sum() and (s2[s2 > 0] > 3.0).all()
    dead = np.ones(s2.size, bool)
    dead[R.active(s2)] = False
    assert not c2.reshape(-1, 27)[dead].any()
    junk = c2.copy().reshape(-1, 27)
    junk[dead] = np.random.default_rng(1).normal(0, 50, (int(dead.sum()), 27)).astype(F)
    junk[np.flatnonzero(dead)[0]] = np.nan
    junk = junk.reshape(c2.shape)
    o, d, tmin, tmax = R.make_rays(40, 5, lo, step, shape)
    occ = R.blocks(s2, 2)
    A = R.march(s2, c2, occ, 2, lo, step, o, d, tmin, tmax, F(0.04), bg=(0.25, 0.5, 1.0))
    B = R.march(s2, junk, occ, 2, lo, step, o, d, tmin, tmax, F(0.04), bg=(0.25, 0.5, 1.0))
    assert (A[2][:, 0] > 0).any()
    for a, b in zip(A[:3], B[:3]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)


@pytest.fixture(scope="module")
def case():
    return V.learning_case()


@pytest.mark.parametrize("tv", [0.0, 1e-3])
def test_learning_condition_on_the_reference(case, tv):
    """25 full-batch steps at the default rates, the lattice doubled after step 12"""
    out = X.learn_levels(case, upsample_at=(12,), tv=(tv, tv))
    losses = out["losses"]
    (before, after), = out["switches"]
    print(f"tv={tv}: first {losses[0]:.6e} final {losses[-1]:.6e} ratio {losses[-1] / losses[0]:.4f}; switch {before:.8e} -> {after:.8e}")
    assert losses.size == V.LEARN_STEPS + 1 and out["sigma"].shape == (17, 15, 13)
    assert losses[-1] <= 0.25 * losses[0]
    assert abs(after - before) <= 1e-4 * before
    # the frozen support, level by level: every positive sigma of a level's end lies in the level's own list
    for L, end in zip(out["levels"], (None, out["sigma"])):
        if end is not None:
            assert np.isin(np.flatnonzero(end.reshape(-1) > 0), L["index"]).all()


def test_header_has_the_rules_and_abi_stays_7():
    hdr = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define NERF_HIP_ABI_VERSION 7\b", hdr)
    for rule in ("VM. MEMBER MASK", "VT. TOTAL VARIATION", "VX. x2 REFINEMENT", "VP. PRUNE"):
        assert rule in hdr, rule
    for name in ("nerf_hip_volume_member_mask", "nerf_hip_volume_tv_backward", "nerf_hip_volume_upsample", "nerf_hip_volume_prune"):
        assert re.search(r"\b" + name + r"\(", hdr), name
