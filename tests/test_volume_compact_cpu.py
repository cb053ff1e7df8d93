"""No GPU: rule VC's restatement (tests/volume_compact_reference.py) -- the premise of the device tests (garbage at the inactive points
of a dense volume does not reach the march), the round trips, the slots, the lookup through slots against rule VL on the unpacked
volume, the derived bound on what fp16 rows move in the image -- and what the package refuses without a device."""
import os
import re

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_reference as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))
NRAYS = 120
DT = F(0.04)
BG = (0.25, 0.5, 1.0)
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def scene(shape):
    """make_volume with garbage sigma at its inactive points, the rays, and the marches of the garbage volume, of unpack(pack(.)) for
    both element types (computed once, never changed)"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        garbage, inactive = X.with_garbage(sigma, coef)
        occ = R.blocks(garbage, 2)
        rays = (o, d, tmin, tmax)
        m = lambda s, c: R.march(s, c, occ, 2, lo, step, o, d, tmin, tmax, DT, 0.0, BG)
        c32, c16 = X.pack(garbage, coef, False), X.pack(garbage, coef, True)
        _cache[shape] = dict(sigma=sigma, garbage=garbage, inactive=inactive, coef=coef, lo=lo, step=step, rays=rays, occ=occ, c32=c32, c16=c16,
                             m_garbage=m(garbage, coef), m32=m(*X.unpack(c32)), m16=m(*X.unpack(c16)))
    return _cache[shape]


@pytest.mark.parametrize("shape", LATTICES)
def test_garbage_at_inactive_points_does_not_reach_the_march(shape):
    s = scene(shape)
    assert s["inactive"].any() and np.isnan(s["garbage"]).any() and (s["garbage"] < 0).any() and (s["coef"][s["inactive"]] != 0).any()
    assert np.array_equal(R.blocks(s["garbage"], 2), R.blocks(s["sigma"], 2))          # occ depends only on the positive points
    a, b = s["m_garbage"], s["m32"]
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(a[2], b[2])                                                  # both columns of steps
    contributing, n_active = int(a[2][:, 0].sum()), int(s["c32"].sigma.shape[0])
    print(f"{shape}: {contributing} contributing samples, {n_active} of {s['sigma'].size} points active")
    assert contributing > 2000 and 0 < n_active < s["sigma"].size


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("degree", (0, 1, 2))
def test_round_trips_and_slots(shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    index = R.active(s["garbage"])
    for half in (False, True):
        c = X.pack(s["garbage"], coef, half)
        assert c.slot.dtype == np.int32 and c.sigma.dtype == F and c.coef.dtype == (np.float16 if half else F)
        assert c.coef.shape == (len(index), X.row_width(degree, half)) and X.row_width(degree, True) == (4, 12, 28)[degree]
        # the slots: -1, or the rank in lattice order
        flat = c.slot.reshape(-1)
        assert np.array_equal(np.flatnonzero(flat >= 0), index) and np.array_equal(flat[flat >= 0], np.arange(len(index)))
        assert (flat[flat < 0] == -1).all()
        if half:
            assert not bits(c.coef[:, 3 * nc:]).any()                                  # the pad halves are +0
        # pack(unpack(c)) == c
        u_sigma, u_coef = X.unpack(c)
        c2 = X.pack(u_sigma, u_coef, half)
        # (unpack writes +0 at the inactive points, so the active list of the result can only lose points whose whole
        # neighbourhood is not positive -- none: the positive points are kept)
        assert np.array_equal(c2.slot, c.slot) and np.array_equal(bits(c2.sigma), bits(c.sigma)) and np.array_equal(bits(c2.coef), bits(c.coef))
        if not half:
            z_sigma, z_coef = X.zeroed(s["garbage"], coef, s["inactive"])
            assert np.array_equal(bits(u_sigma), bits(z_sigma)) and np.array_equal(bits(u_coef), bits(z_coef))


sample_points = X.sample_points


@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("half", (False, True))
def test_lookup_through_slots_is_rule_vl_on_unpack(shape, half):
    s = scene(shape)
    x, d = sample_points(shape, s["lo"], s["step"])
    for degree in (0, 1, 2):
        c = X.pack(s["garbage"], np.ascontiguousarray(s["coef"][..., :(degree + 1) ** 2, :]), half)
        got = X.lookup(c, s["lo"], s["step"], x, d)
        want = R.lookup(*X.unpack(c), s["lo"], s["step"], x, d)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        assert (want[0] > 0).sum() > 20 and ((want[1] > 0) & (want[1] < 1)).any()
    # slots outside [0, n) are inactive corners
    c = X.pack(s["garbage"], s["coef"], half)
    n = c.sigma.shape[0]
    bad = c.slot.copy().reshape(-1)
    pts = np.flatnonzero(bad >= 0)[[1, -2]]
    bad[pts] = (n, -2)
    cb = c._replace(slot=bad.reshape(shape))
    us, uc = X.unpack(c)
    us.reshape(-1)[pts] = 0
    uc.reshape(-1, 27)[pts] = 0
    got, want = X.lookup(cb, s["lo"], s["step"], x, d), R.lookup(us, uc, s["lo"], s["step"], x, d)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(bits(X.unpack(cb)[0]), bits(us))


@pytest.mark.parametrize("shape", LATTICES)
def test_fp16_moves_the_image_by_no_more_than_rounding_allows(shape):
    """Per ray |rgb16 - rgb32| <= 2^-11 M + 2 bound(n) (1 + max |bg|).  The weights w_k are the same bits in both marches (sigma is not
    rounded), they sum to at most 1, the clamp and the trilinear mean do not expand, and a corner's colour sum_m Y_m c_m moves by at most
    sum_m |Y_m| |c_m| 2^-11 when every c_m is rounded to fp16's 11 significant bits: 2^-11 M with M the largest such sum over the corners
    the ray's contributing samples read.  Each march is within bound(n) (1 + max |bg|) of its own exact composite.  (A coefficient below
    2^-14 rounds to a subnormal half with an absolute error of 2^-25 instead; the fp32 roundings of the colour sums are of the same
    order.  Neither is in the issue's formula; both are far below its slack here: printed.)"""
    s = scene(shape)
    a, b = s["m32"], s["m16"]
    assert np.array_equal(a[2], b[2]) and np.array_equal(bits(a[1]), bits(b[1]))       # the same samples, the same weights: D and A too
    coef = s["coef"]
    worst, worst_ratio, changed = 0.0, 0.0, 0
    for r, (smp, used) in enumerate(a[3]):
        if smp is None or not used:
            assert np.array_equal(bits(a[0][r]), bits(b[0][r]))
            continue
        Y = np.abs(R.basis32(smp["d"][None])[0].astype(np.float64))
        ci = smp["ci"][used]
        M = 0.0
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    cc = np.abs(coef[ci[:, 0] + di, ci[:, 1] + dj, ci[:, 2] + dk].astype(np.float64))      # [n, 9, 3]
                    M = max(M, float((Y[None, :, None] * cc).sum(1).max()))
        lim = 2.0 ** -11 * M + 2 * R.bound(len(used)) * (1 + max(abs(x) for x in BG))
        e = float(np.abs(a[0][r].astype(np.float64) - b[0][r]).max())
        worst, worst_ratio = max(worst, e), max(worst_ratio, e / lim)
        changed += e > 0
        assert e <= lim, (r, e, lim)
    c32, c16 = s["c32"], s["c16"]
    moved = float((c16.coef[:, :27].astype(F) != c32.coef).mean())
    print(f"{shape}: fp16 moves rgb by at most {worst:.3e} (worst error / bound {worst_ratio:.3f}); {moved:.3f} of the coefficients change")
    assert changed > 10 and moved > 0.9


def test_fp16_rounding_of_the_restatement():
    """ties to even, subnormals, the largest half, past it, signed zeros"""
    v = np.asarray([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 3e-6, 65504.0, -65504.0, 65519.0, 65520.0,
                    1e6, -1e6, 0.0, -0.0, np.inf, np.nan], F)
    got = X.rows(v[None, :], True)[0]
    want = np.asarray([1.0, 1.0 + 2.0 ** -9, 2.0 ** -24, 0.0, 2.0 ** -23, 0.0, 65504.0, -65504.0, 65504.0, np.inf, np.inf, -np.inf,
                       0.0, -0.0, np.inf, np.nan], np.float64)
    want[5] = np.round(3e-6 / 2.0 ** -24) * 2.0 ** -24          # a subnormal half: a multiple of 2^-24 (50.3 -> 50)
    ok = ~np.isnan(want)
    assert np.array_equal(got.astype(np.float64)[ok], want[ok]) and np.isnan(got[~ok]).all()
    assert np.signbit(got[13]) and not np.signbit(got[12])


def compact_on_cpu(pkg, degree=2, half=True):
    n = 5
    return pkg.volume.CompactVolume(torch.full((5, 4, 3), -1, dtype=torch.int32), torch.zeros(n), torch.zeros(n, X.row_width(degree, half),
                                    dtype=torch.float16 if half else torch.float32), torch.zeros(2, 2, 1, dtype=torch.uint8),
                                    np.zeros(3, F), np.ones(3, F), 2, degree, (5, 4, 3))


def test_training_calls_refuse_a_compact_volume(pkg):
    V = pkg.volume
    c = compact_on_cpu(pkg)
    z = torch.zeros(4, 3)
    calls = [lambda: V.grad_buffers(c), lambda: V.render_backward(c, None, z, z, 0.0, 1.0, z), lambda: V.render_train(c, z, z, 0.0, 1.0),
             lambda: V.Finetuner(c), lambda: V.finetune(c, None, None, 1), lambda: V.upsample(c), lambda: V.prune(c, 0.0),
             lambda: V.tv_backward(c, None, None, None, 1.0, 1.0), lambda: V.pack(c)]
    for call in calls:
        with pytest.raises(TypeError, match="unpack"):
            call()
    with pytest.raises(TypeError):
        V.unpack(V.Volume(torch.zeros(5, 4, 3), torch.zeros(5, 4, 3, 9, 3), torch.zeros(2, 2, 1, dtype=torch.uint8), np.zeros(3, F), np.ones(3, F),
                          2, 2))
    # no CPU path, and the arguments that need no device
    for call in (lambda: V.render(c, z, z, 0.0, 1.0), lambda: V.sample(c, z, z), lambda: V.unpack(c), lambda: V.with_block(c, 4)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        V.pack(V.Volume(torch.zeros(5, 4, 3), torch.zeros(5, 4, 3, 9, 3), None, None, None, 2, 2), dtype="fp8")
    assert V.nbytes(c) == 60 * 4 + 5 * 4 + 5 * 28 * 2 + 4


def test_c_entries_refuse_bad_arguments_without_a_device(pkg):
    """everything here is refused on the host before any device call; the pointers are never read"""
    L, f3 = pkg._abi.lib(), pkg._abi.f32_array
    p = 1 << 20                     # a non-null, 8-byte aligned stand-in
    lo, step, bg = f3([0.0] * 3), f3([1.0] * 3), f3([0.0] * 3)
    ERR = -1

    def render(n=5, half=1, rows=p, nx=5, slot=p):
        return L.nerf_hip_volume_compact_render(slot, p, rows, n, half, p, nx, 4, 3, 2, 2, lo, step, p, p, p, p, 4, 0.1, 0.0, bg, p, p, p, None)

    def sample(n=5, half=1, rows=p, nx=5, slot=p):
        return L.nerf_hip_volume_compact_sample(slot, p, rows, n, half, nx, 4, 3, 2, lo, step, p, p, 4, p, p, None)

    for call in (render, sample):
        for kw in (dict(half=2), dict(half=-1), dict(n=61), dict(n=-1), dict(rows=p + 4), dict(rows=p + 2, half=0), dict(nx=1), dict(slot=None),
                   dict(rows=None), dict(slot=p + 2)):
            assert call(**kw) == ERR and L.nerf_hip_last_error(), kw
    assert L.nerf_hip_volume_compact_slots(p, 61, 5, 4, 3, p, None) == ERR
    assert L.nerf_hip_volume_compact_slots(p, -1, 5, 4, 3, p, None) == ERR
    assert L.nerf_hip_volume_compact_slots(None, 5, 5, 4, 3, p, None) == ERR
    assert L.nerf_hip_volume_compact_slots(p, 5, 5, 4, 3, None, None) == ERR
    assert L.nerf_hip_volume_compact_slots(p, 5, 5, 1, 3, p, None) == ERR
    pack = lambda sigma=p, coef=p, degree=2, index=p, n=5, half=1, srows=p, crows=p: L.nerf_hip_volume_compact_pack(
        sigma, coef, 5, 4, 3, degree, index, n, half, srows, crows, None)
    for kw in (dict(half=2), dict(n=61), dict(n=-1), dict(degree=3), dict(crows=p + 4), dict(index=None, n=5), dict(sigma=None), dict(srows=None),
               dict(coef=None), dict(crows=None), dict(index=p + 2)):
        assert pack(**kw) == ERR and L.nerf_hip_last_error(), kw
    unpack = lambda srows=p, crows=p, half=1, index=p, n=5, degree=2, sigma=p, coef=p: L.nerf_hip_volume_compact_unpack(
        srows, crows, half, index, n, 5, 4, 3, degree, sigma, coef, None)
    for kw in (dict(half=2), dict(n=61), dict(degree=-1), dict(crows=p + 4), dict(coef=None), dict(crows=None), dict(sigma=None), dict(srows=None),
               dict(index=None)):
        assert unpack(**kw) == ERR and L.nerf_hip_last_error(), kw


def test_driver_option_header_and_abi():
    import importlib

    ap = importlib.import_module("nerf_tiny_amd.main").build_parser()
    a = ap.parse_args(["--volume", "24", "--volume-compact", "fp16", "--volume-preview"])
    assert (a.volume, a.volume_compact, a.volume_preview) == (24, "fp16", "test")
    assert ap.parse_args(["--volume", "24"]).volume_compact is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--volume", "8", "--volume-compact", "int8"])
    hdr = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define NERF_HIP_ABI_VERSION 7\b", hdr)
    for text in ("VC. THE COMPACT FORM", "VC-L. LOOKUP", "VC-R. MARCH"):
        assert text in hdr, text
    for name in ("slots", "pack", "unpack", "sample", "render"):
        assert re.search(r"\bnerf_hip_volume_compact_" + name + r"\(", hdr), name
