"""CPU: the restatements of tests/field_ends_reference.py -- the accuracy of sincos_phase over its documented domain and what it does
beyond it, bit equality with the oracle's fp32 stages, the inputs' coverage classes, and the teeth of the output-end bar.

Figures of these tests (printed by each):
  sincos_phase against float64 sin / cos of the same fp32 phase, bar 2^-23 absolute:
    1,048,576 random phases, log-uniform in [2^-30, 2^20), both signs      9.17e-8  (0.77 x 2^-23)
    76,480 fp32 neighbours of 19,120 multiples n pi/2 up to 2^20 rad        5.87e-8  (0.49 x 2^-23)
    +-0 and subnormals: exact, signs included (sin x = x, cos x = 1)
  beyond the domain (a fixed grid of 8,192 phases and the neighbours of 1,024 multiples of pi/2 per binade, both signs):
    the 2^-23 bar holds below 2^29 rad (|p_c| < 1.6e5 at the largest frequency; worst 9.7e-8 on the grid, 1.03e-7 on 4 M random phases of
    [2^28, 2^29)); [2^29, 2^30) reaches it (1.11e-7, random 1.17e-7); [2^30, 2^31) exceeds it (1.29e-7) and from there the error doubles
    per binade (pi/2 as a float64 is 6.1e-17 off, times n): 4.3e-5 at 2^39, 4.4e-2 at 2^49, 0.69 at 2^53
    outputs stay inside [-1, 1] below 2^54 rad; from 2^54 rad (|p_c| >= 5.6e12) double(phase) * 2/pi is past 2^53, n is no longer the
    nearest integer, the reduced argument grows with the spacing of n and the polynomials return 1.23 in [2^54, 2^55), 1.9e2, 7.5e4, ...
    1.6e12 at 2^59; the first +-inf / NaN in [2^70, 2^71) (the z^4 term of the cosine polynomial overflows fp32 once r reaches 2^18: 0.7 % of
    the grid there, 21 % at 2^71, 53 % at 2^72) and no finite pair by 2^90 -- unbounded values, not the bounded wrong ones sinf would give

sin(-0): the polynomial path alone gives +0 for -0 -- n = rint(-0 * 2/pi) = -0, fma(+0, pi/2, -0) = (+0) + (-0) = +0 under
round-to-nearest, and fmaf(ps z, r, r) adds zeros of opposite sign once more -- so sincos_phase ends with sn = (ph == 0) ? ph : sn, and
test_sin_of_zero_keeps_its_sign holds it to libm's sin(+-0) = +-0.
"""
import numpy as np
import pytest
import torch

import field_ends_reference as F
import ws_operands as W
from test_gpu_layers import E_BF16, E_FP32

BAR = 2.0 ** -23


def _err(ph):
    with np.errstate(all="ignore"):
        s, c = F.sincos_phase(ph)
    x = ph.astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.maximum(np.abs(s.astype(np.float64) - np.sin(x)), np.abs(c.astype(np.float64) - np.cos(x)))
        big = np.maximum(np.abs(s.astype(np.float64)), np.abs(c.astype(np.float64)))
    return np.where(np.isnan(e), np.inf, e), np.where(np.isnan(big), np.inf, big)


def _neighbours(n):
    """The fp32 values on either side of n * pi/2 (n float64 integers)."""
    x = n * F.PI_OVER_2
    with np.errstate(over="ignore"):
        lo = x.astype(np.float32)
        lo = np.where(lo.astype(np.float64) > x, np.nextafter(lo, np.float32(-np.inf)), lo).astype(np.float32)
        hi = np.nextafter(lo, np.float32(np.inf))
    out = np.concatenate((lo, hi))
    return out[np.isfinite(out)]


def test_reduction_is_formed_exactly():
    """The vectorised fma of reduce_phase against rational arithmetic, inside and far outside the domain."""
    rng = np.random.default_rng(0)
    xs = np.concatenate((2.0 ** (50 * rng.random(2000) - 30) * np.where(rng.random(2000) < 0.5, -1, 1), 2.0 ** (20 + 107 * rng.random(2000)),
                         _neighbours(np.rint(2.0 ** (19 * rng.random(500))))[:1000])).astype(np.float32)
    n, r = F.reduce_phase(xs)
    for i, x in enumerate(xs):
        assert F.reduce_phase_exact(x) == (n[i], r[i]), (float(x), n[i], r[i])


def test_constants_are_the_headers_literals():
    src = open(F.os.path.join(F.CSRC, "field_common.h")).read()
    body = src[src.index("void sincos_phase("):src.index("// gamma_p of this thread's sample")]
    for lit in ("0.63661977236758134308", "1.57079632679489661923", "-1.9515295891e-4f", "8.3321608736e-3f", "-1.6666654611e-1f",
                "2.443315711809948e-5f", "-1.388731625493765e-3f", "4.166664568298827e-2f", "-0.5f", "1.0f"):
        assert lit in body, lit


def test_sincos_phase_is_within_one_ulp_over_its_domain():
    """DESIGN.md "Queries", include/nerf_hip.h: <= 1 ulp for |phase| < 2^20.  2^-23 absolute = one ulp of a value in [0.5, 1)."""
    rng = np.random.default_rng(1)
    N = 1 << 20
    ph = (2.0 ** (50 * rng.random(N) - 30) * np.where(rng.random(N) < 0.5, -1.0, 1.0)).astype(np.float32)
    ph = ph[np.abs(ph) < 2.0 ** 20]
    assert ph.size >= 10 ** 6 and float(np.abs(ph).min()) < 2.0 ** -29 and float(np.abs(ph).max()) > 2.0 ** 19.9
    e_rand = float(_err(ph)[0].max())
    nmax = 2.0 ** 20 * F.TWO_OVER_PI
    n = np.unique(np.rint(2.0 ** np.linspace(0, np.log2(nmax), 40000)))
    adv = _neighbours(np.concatenate((n, -n)))
    adv = adv[np.abs(adv) < 2.0 ** 20]
    assert n.size >= 10 ** 4
    _, r = F.reduce_phase(adv)
    e_adv = float(_err(adv)[0].max())
    sub = np.array([0.0, 1e-45, -1e-45, 1e-42, -1e-39, 1.1754942e-38, -1.1754942e-38], dtype=np.float32)
    s, c = F.sincos_phase(sub)
    print(f"\nsincos_phase: random {ph.size} phases {e_rand:.3g} ({e_rand / BAR:.2f} x 2^-23); adversarial {adv.size} neighbours of "
          f"{n.size} multiples of pi/2 (closest {float(np.abs(r).min()):.2g} rad) {e_adv:.3g} ({e_adv / BAR:.2f} x 2^-23)")
    assert e_rand <= BAR and e_adv <= BAR
    assert np.array_equal(s.view(np.uint32), sub.view(np.uint32)) and bool((c == 1).all())  # sin x = x, cos x = 1, subnormals kept
    s0, c0 = F.sincos_phase(np.array([-0.0], dtype=np.float32))
    assert float(s0[0]) == 0.0 and float(c0[0]) == 1.0


def test_sin_of_zero_keeps_its_sign():
    """sin(+-0) = +-0 bit for bit, as libm's (the final select of sincos_phase; without it the reduction's fma gives +0 for -0)."""
    z = np.array([0.0, -0.0], dtype=np.float32)
    s, _ = F.sincos_phase(z)
    assert [f"{b:08x}" for b in s.view(np.uint32)] == [f"{b:08x}" for b in z.view(np.uint32)]


# ---- beyond the domain ----------------------------------------------------------------------------------------------------------------
HOLDS_BELOW = 29      # the 2^-23 bar holds with margin (<= 0.9 x) below 2^29 rad; [2^29, 2^30) reaches it (0.93 x on the grid, 0.98 x on
#                       4 M random phases); [2^30, 2^31) is the first binade that exceeds it
LEAVES_UNIT_AT = 54   # every grid output is inside [-1, 1] below 2^54 rad; some output in [2^54, 2^55) is not
NONFINITE_AT = 70     # every grid output is finite below 2^70 rad; some sin or cos in [2^70, 2^71) is +-inf or NaN
NONE_FINITE_BY = 90   # from 2^90 rad no grid phase has a finite (sin, cos) pair


def _binade_grid(k, m=8192, multiples=1024):
    g = 2.0 ** k * (1.0 + np.arange(m) / m)
    n = np.unique(np.rint(2.0 ** k * F.TWO_OVER_PI * (1.0 + np.arange(multiples) / multiples)))
    nb = _neighbours(n).astype(np.float64)
    nb = nb[(nb >= 2.0 ** k) & (nb < 2.0 ** (k + 1))]
    g = np.concatenate((g, nb))
    return np.concatenate((g, -g)).astype(np.float32)


def test_beyond_the_domain_the_error_grows_and_then_the_outputs_leave_the_unit_interval():
    """What the code does for |phase| >= 2^20 (callers of nerf_hip_query / nerf_hip_query_grad / the density grid supply the points):
    pinned from the restatement on a fixed grid per binade.  include/nerf_hip.h and DESIGN.md "Queries" say the same."""
    err, big, finite = {}, {}, {}
    for k in range(20, 110):
        e, b = _err(_binade_grid(k))
        err[k], big[k], finite[k] = float(e.max()), float(b.max()), float(np.isfinite(b).mean())
    holds = next(k for k in range(20, 110) if err[k] > BAR)
    leaves = next(k for k in range(20, 110) if big[k] > 1.0)
    nonfinite = next(k for k in range(20, 110) if finite[k] < 1.0)
    none_finite = next(k for k in range(20, 110) if all(finite[j] == 0.0 for j in range(k, 110)))
    print("\nsincos_phase beyond 2^20 rad, worst error per binade: " + ", ".join(f"2^{k} {err[k]:.3g}" for k in (20, 28, 29, 30, 39, 49, 53)) +
          f"; largest |output|: " + ", ".join(f"2^{k} {big[k]:.4g}" for k in (53, 54, 55, 56, 59)) + f"; first non-finite output in 2^{nonfinite} (finite share "
          + ", ".join(f"2^{k} {finite[k]:.4f}" for k in (70, 71, 72, 80)) + f"), none finite from 2^{none_finite}")
    assert holds == HOLDS_BELOW + 1 and leaves == LEAVES_UNIT_AT and nonfinite == NONFINITE_AT, (holds, leaves, nonfinite)
    assert none_finite <= NONE_FINITE_BY, none_finite
    assert all(err[k] <= 0.9 * BAR for k in range(20, HOLDS_BELOW)), err
    assert all(big[k] <= 1.0 for k in range(20, LEAVES_UNIT_AT)) and all(big[k] > 1.0 for k in range(LEAVES_UNIT_AT, 110))
    assert 2e-5 < err[39] < 1e-4 and 2e-2 < err[49] < 1e-1 and big[59] > 1e11  # 4e-5 near 1e12 rad, 4e-2 near 1e15, outputs of 1e12 near 1e18
    for name in ("include/nerf_hip.h", "DESIGN.md"):
        text = open(F.os.path.join(F.ROOT, name)).read()
        for k in (HOLDS_BELOW, LEAVES_UNIT_AT, NONFINITE_AT, NONE_FINITE_BY):
            assert f"2^{k} rad" in text, (name, k)


# ---- the restatements against the oracle's fp32 stages ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,B,Nc,Nf", [("lego", 48, 64, 128), ("fern", 40, 24, 40), ("fern", 7, 5, 3)])
def test_restatements_equal_the_oracles_fp32_stages(oracle, fixture, B, Nc, Nf):
    """Rays, depths and points bit for bit (the oracle is torch fp32, one rounding per operation: the same arithmetic); the encodings to
    the 2e-6 the oracle documents for torch's fp32 sin / cos across hosts (tests/test_oracle_golden.py).  Pins the restatement."""
    row, col, pb, K, _ = (oracle.lego_inputs if fixture == "lego" else oracle.fern_inputs)(B, seed=5)
    st = {}
    with torch.no_grad():
        oracle.render(oracle.make_weights(6, sharp=True), row, col, pb, K, Nc, Nf, stages=st, check=False)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    eq = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), b.contiguous().numpy().view(np.uint32))
    assert eq(rf[:, F.RF_R:F.RF_R + 9], st["R"].reshape(B, 9)) and eq(rf[:, F.RF_O:F.RF_O + 3], st["o"])
    assert eq(rf[:, F.RF_DCAM:F.RF_DCAM + 3], st["d_cam"]) and eq(rf[:, F.RF_DWRD:F.RF_DWRD + 3], st["d_wrd"])
    assert eq(rf[:, F.RF_NEAR], st["near"]) and eq(rf[:, F.RF_FAR], st["far"])
    assert eq(rf[:, F.RF_DELTA], (st["far"] - st["near"]) / Nc)
    t_c = F.coarse_depth(rf, Nc)
    assert eq(t_c, st["t_c"])
    assert eq(F.sample_point(rf, t_c), st["pts_c"]) and eq(F.sample_point(rf, st["t_f"].numpy()), st["pts_f"])
    f_p, f_d = oracle.frequencies()
    assert eq(F.FREQ_POINT, f_p) and eq(F.FREQ_DIR, f_d)
    worst = 0.0
    for t, pts in ((t_c, st["pts_c"]), (st["t_f"].numpy(), st["pts_f"])):
        gp = F.gamma_p(rf, t)
        assert not gp[:, 60:].any()
        worst = max(worst, float(np.abs(gp[:, :60].astype(np.float64) - oracle.encode(pts, f_p).reshape(-1, 60).double().numpy()).max()))
    gd = F.gamma_d(rf[:, F.RF_DWRD:F.RF_DWRD + 3], "phase")
    worst_d = float(np.abs(gd.astype(np.float64) - st["gd"].double().numpy()).max())
    lib = F.gamma_d(rf[:, F.RF_DWRD:F.RF_DWRD + 3], "libm")
    assert float(np.abs(gd.astype(np.float64) - lib).max()) <= BAR
    print(f"\n{fixture} {B}x({Nc}+{Nf}): restated encodings against the oracle's torch fp32: gamma_p {worst:.3g}, gamma_d {worst_d:.3g}")
    assert worst < 2e-6 and worst_d < 2e-6


# ---- the inputs of the GPU test: coverage, checked here on the coarse samples ---------------------------------------------------------------
SIZES = [(2, 2, 1), (7, 5, 3), (50, 24, 40), (130, 31, 65), (3, 1024, 1024)]


SMALL_CASE_FLOORS = {(2, 2, 1): (0, 3), (7, 5, 3): (29, 9), (3, 1024, 1024): (22, 40)}  # (pairs, near_multiple) of the coarse samples


def coverage_wanted(B, Nc, Nf):
    """What a case of this size can hold (tests/test_gpu_field_ends.py asserts the same on all of its rows).  A case always has a
    coordinate in (300, 320] and an exact zero, by construction of two translations.  All four quadrants of both signs for every one of
    the 30 pairs are 8 classes per pair, and 64 phases of |n| > 2^18 within 2^-10 rad of a multiple of pi/2 come from choosing
    translations (a random phase is that close with probability 1.2e-3): both need rays to choose from -- 6 or 56 samples cannot hold 8
    classes per pair, and the nine translations of 3 rays give neither both signs of a slowly moving coordinate at the lowest frequency
    (22 pairs) nor 64 close phases (40).  Asserted in full from 50 rays; the smaller cases are held to the counts their coarse samples
    have (SMALL_CASE_FLOORS: the fine samples can only add to them), so that the inputs cannot degrade unnoticed."""
    if B >= 50:
        return {"big": 1, "zero": 1, "pairs": 30, "near_multiple": 64}
    pairs, near = SMALL_CASE_FLOORS[(B, Nc, Nf)]
    return {"big": 1, "zero": 1, "pairs": pairs, "near_multiple": near}


@pytest.mark.parametrize("B,Nc,Nf", SIZES)
def test_the_inputs_cover_their_phase_classes(oracle, B, Nc, Nf):
    row, col, pb, K, _ = F.field_ends_inputs(oracle, B, Nc)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    cov = F.coverage(F.sample_point(rf, F.coarse_depth(rf, Nc)))
    print(f"\n{B}x({Nc}+{Nf}) coarse samples: {cov}")
    assert cov["max_abs"] <= 320.0
    for k, v in coverage_wanted(B, Nc, Nf).items():
        assert cov[k] >= v, (k, cov)


def test_the_cases_together_hold_every_class(oracle):
    tot = {"near_multiple": 0, "big": 0, "zero": 0}
    for B, Nc, Nf in SIZES:
        row, col, pb, K, _ = F.field_ends_inputs(oracle, B, Nc)
        rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
        cov = F.coverage(F.sample_point(rf, F.coarse_depth(rf, Nc)))
        for k in tot:
            tot[k] += cov[k]
    assert tot["near_multiple"] >= 64 and tot["big"] > 0 and tot["zero"] > 0, tot


# ---- teeth of the output-end bar -----------------------------------------------------------------------------------------------------------
def _teeth_case(oracle, mode):
    B, Nc, Nf = 50, 24, 40
    row, col, pb, K, _ = F.field_ends_inputs(oracle, B, Nc)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    gen = torch.Generator().manual_seed(3)
    u = torch.rand(B, Nf, generator=gen).sort(dim=1)[0].numpy()
    t_f = (rf[:, F.RF_NEAR, None] + u * (rf[:, F.RF_FAR, None] - rf[:, F.RF_NEAR, None])).astype(np.float32)
    weights = list(oracle.make_weights(6, sharp=True).values())
    g = [torch.randn(B * Nf, W.WIDTH, generator=gen) * (torch.rand(B * Nf, W.WIDTH, generator=gen) < 0.5) for _ in range(2)]  # half masked
    parts = (lambda x: (x,)) if mode == "fp32" else (lambda x: (W.rne_bf16(x.double()),)) if mode == "bf16" else \
        (lambda x: W.split_bf16(x.double()))
    Wd, Wpi = weights[W.W_DIR], weights[W.W_PI]
    ops = {"fold": (Wd[:, W.DIR_DIM:] @ Wpi,), "b_fold": (Wd[:, W.DIR_DIM:] @ weights[W.B_PI],)}
    R = W.reference_weights(ops, weights, mode)
    return parts(g[0]), parts(g[1]), R, rf, t_f


@pytest.mark.parametrize("mode", ["fp32", "bf16", "split"])
def test_teeth_every_mutation_breaks_the_bar_on_a_quarter_of_the_elements(oracle, mode):
    """Each mutation of the restated dt_field against the unmutated one under the bar of tests/test_gpu_field_ends.py; the gamma_p
    mutations also against the forward end's bit equality (share of rows with a differing bit)."""
    g0, g4, R, rf, t_f = _teeth_case(oracle, mode)
    E = E_FP32 if mode == "fp32" else E_BF16
    ref, mag = F.dt_field(g0, g4, R, rf, t_f)
    bar = F.dt_bar(mag, ref, E)
    assert float(((F.dt_field(g0, g4, R, rf, t_f)[0] - ref).abs() / bar).max()) == 0.0  # the unmutated restatement: ratio 0
    vac = float((bar > 0.5 * ref.abs()).double().mean())
    out = []
    gp = F.gamma_p(rf, t_f)
    for mut in F.MUTATIONS:
        share = float(((F.dt_field(g0, g4, R, rf, t_f, mutate=mut)[0] - ref).abs() > bar).double().mean())
        msg = f"{mut} {100 * share:.1f} %"
        if mut in ("frequency_off", "lane_half", "coordinate_off"):
            rows = float((F.gamma_p(rf, t_f, mutate=mut) != gp).any(axis=1).mean())
            msg += f" (gamma_p rows {100 * rows:.1f} %)"
            assert rows >= 0.25, (mut, rows)
        out.append(msg)
        assert share >= 0.25, (mut, share)
    print(f"\n{mode}: elements outside the bar per mutation: " + ", ".join(out) + f"; bar above half the reference on {100 * vac:.2f} %")
    assert vac < 0.10
