"""CPU restatements of the two ends of the field that the layer suites take as given (tests/test_field_ends_cpu.py,
tests/test_gpu_field_ends.py).

Input end: what turns (row, col, pose, K^-1) into the first layer's operands -- the ray record and the coarse depths
(csrc/prep_parts.h ray_record, coarse_depth), the sample point and the fp32 sin / cos of a phase (csrc/field_common.h sample_point,
sincos_phase) and the encodings built from them.  Every fp32 product, sum and quotient is evaluated in float64 and rounded to fp32 on its
own (exact for fp32 operands: 53 >= 2 * 24 + 2 bits); an fmaf is one rounding of the exact a * b + c (round-to-odd in float64, then to
fp32); the float64 fma of the argument reduction is formed exactly (an error-free product, an exact difference) and rounded once.  The
library is built with -ffp-contract=off and writes its fmas out, so these restatements are meant to equal the device bit for bit.

Output end: d gamma_p -> d point -> d t of the fine pass (field_bwd.hip, field_bwd_reg.hip, field_bwd_bf16.hip, field_bwd_split.hip) in
float64 with its magnitude, from the device's own g0 / g4 and the weights the kernels multiplied by (ws_operands.reference_weights).

The frequencies are read from the bit patterns of csrc/common.h (NERF_FREQ_POINT_BITS, kFreqDirBits), never recomputed; the constants
of sincos_phase are the literals of field_common.h:199-215, each converted to the nearest fp32 / float64 as the compiler converts them.
"""
import os
import re
from fractions import Fraction

import numpy as np
import torch

import ws_operands as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf-tiny_amd", "csrc")

# common.h RF_*: the ray record
RF_R, RF_O, RF_DCAM, RF_DWRD, RF_NEAR, RF_FAR, RF_STEP, RF_DELTA, RAYF = 0, 9, 12, 15, 18, 19, 20, 21, 24
L_POINT, L_DIR = 10, 4
GP_COLS = 64  # the saved gamma_p row: 60 encodings, columns 60..63 zero

MUTATIONS = ("cos_negated", "sin_cos_swapped", "skip_dropped", "frequency_off", "lane_half", "coordinate_off")


def _freq_bits():
    src = open(os.path.join(CSRC, "common.h")).read()
    point = re.search(r"#define NERF_FREQ_POINT_BITS (.*)", src).group(1)
    dirs = re.search(r"kFreqDirBits\[4\] = \{(.*?)\}", src).group(1)
    conv = lambda s: np.array([int(x.strip().rstrip("u"), 16) for x in s.split(",")], dtype=np.uint32).view(np.float32)
    fp, fd = conv(point), conv(dirs)
    assert fp.shape == (L_POINT,) and fd.shape == (L_DIR,)
    return fp, fd


FREQ_POINT, FREQ_DIR = _freq_bits()  # fp32


def f32_literal(text):
    """The fp32 value of a decimal literal with an f suffix: the nearest fp32 to the decimal, ties to even (one rounding, not two)."""
    q = Fraction(text)
    c = np.float32(float(q))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(v.view(np.uint32)) & 1))


# field_common.h:201-210
TWO_OVER_PI = float("0.63661977236758134308")
PI_OVER_2 = float("1.57079632679489661923")
S1, S2, S3 = (float(f32_literal(s)) for s in ("-1.9515295891e-4", "8.3321608736e-3", "-1.6666654611e-1"))
C1, C2, C3 = (float(f32_literal(s)) for s in ("2.443315711809948e-5", "-1.388731625493765e-3", "4.166664568298827e-2"))


# ---- fp32 arithmetic in float64 ---------------------------------------------------------------------------------------------------
def _r(x):
    """float64 -> the nearest fp32, as float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _fmaf(a, b, c):
    """fmaf(a, b, c) of fp32 values held in float64: ONE rounding of the exact a * b + c.  a * b is exact in float64; the sum is taken
    with its exact error (TwoSum) and rounded to odd, which makes the final rounding to fp32 that of the exact value."""
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s) & np.isfinite(e)
        fix = fin & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return _r(s)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker, with Veltkamp's split), float64."""
    with np.errstate(all="ignore"):
        p = a * b
        sp = 134217729.0  # 2^27 + 1
        t = sp * a
        ah = t - (t - a)
        al = a - ah
        t = sp * b
        bh = t - (t - b)
        bl = b - bh
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        return p, e


def reduce_phase(ph32):
    """(n, r): n = rint(double(ph) * 2/pi) as float64 and r = fp32(fma(-n, pi/2, ph)) as float64 (field_common.h:200-202).  The fma:
    n * pi/2 = p + e exactly; ph - p is exact (both lie on the grid of ulp(p) and the difference is smaller than p: Sterbenz for
    |n| >= 2, the grid for |n| = 1, p = 0 for n = 0), so (ph - p) - e rounds the exact value once."""
    x = np.asarray(ph32, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        n = np.rint(x * TWO_OVER_PI)
        p, e = _two_prod(n, PI_OVER_2)
        r = (x - p) - e
    return n, _r(r)


def reduce_phase_exact(ph32):
    """reduce_phase by rational arithmetic, one scalar at a time (the check of the vectorised form)."""
    x = float(np.float32(ph32))
    n = float(np.rint(np.float64(x) * TWO_OVER_PI))
    q = Fraction(x) - Fraction(n) * Fraction(PI_OVER_2)
    r64 = q.numerator / q.denominator  # int / int: correctly rounded
    return n, float(np.float32(r64))


def quadrant(n):
    """(long long)n & 3 (field_common.h:203).  Past +-2^63 the conversion is not defined by the language; held at the nearest end here
    -- sin / cos are far outside [-1, 1] long before (test_field_ends_cpu.py)."""
    with np.errstate(invalid="ignore"):
        nn = np.clip(np.nan_to_num(n, nan=0.0), -9.2233720368547748e18, 9.2233720368547748e18)
    return nn.astype(np.int64) & 3


def sincos_phase(ph32):
    """field_common.h sincos_phase, bit for bit: fp32 arrays (sin, cos) of the fp32 phases."""
    ph32 = np.asarray(ph32, dtype=np.float32)
    n, r = reduce_phase(ph32)
    q = quadrant(n)
    with np.errstate(all="ignore"):
        z = _r(r * r)
        ps = _fmaf(z, S1, S2)
        ps = _fmaf(z, ps, S3)
        ps = _fmaf(_r(ps * z), r, r)
        pc = _fmaf(z, C1, C2)
        pc = _fmaf(z, pc, C3)
        pc = _fmaf(_r(pc * z), z, _fmaf(z, -0.5, 1.0))
    odd = (q & 1) != 0
    a = np.where(odd, pc, ps)
    b = np.where(odd, ps, pc)
    sn = np.where((q & 2) != 0, -a, a)
    cs = np.where(((q + 1) & 2) != 0, -b, b)
    sn = np.where(ph32 == 0, ph32.astype(np.float64), sn)  # sn = (ph == 0.f) ? ph : sn: sin(-0) = -0
    return sn.astype(np.float32), cs.astype(np.float32)


# ---- rays, depths, points (prep_parts.h:58-92, field_common.h:189-193) ------------------------------------------------------------
def _np32(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32)


def ray_record(row, col, pb, K_inv, Nc):
    """prep_parts.h ray_record -> rayf [B, 24] fp32 (columns 22, 23 zero).  row, col: integers; pb [B, 17] fp32 (the pose rows after
    the cast); K_inv [3, 3] fp32, read row-major as the kernel's K[9]."""
    pb = _np32(pb).astype(np.float64)
    K = _np32(K_inv).reshape(9).astype(np.float64)
    as_f32 = lambda v: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.int64).astype(np.float32)
    x, y = as_f32(row).astype(np.float64), as_f32(col).astype(np.float64)
    p = [_r(_r(_r(x * K[j]) + _r(y * K[3 + j])) + K[6 + j]) for j in range(3)]
    ss = _fmaf(p[2], p[2], _fmaf(p[1], p[1], _r(p[0] * p[0])))
    nrm = np.maximum(_r(np.sqrt(ss)), float(np.float32(1e-12)))
    d = [_r(p[j] / nrm) for j in range(3)]
    rec = np.zeros((pb.shape[0], RAYF), dtype=np.float64)
    for c in range(3):
        rec[:, RF_R + 3 * c:RF_R + 3 * c + 3] = pb[:, 5 * c:5 * c + 3]
        rec[:, RF_O + c] = pb[:, 5 * c + 3]
        rec[:, RF_DCAM + c] = d[c]
        rec[:, RF_DWRD + c] = _r(_r(_r(pb[:, 5 * c] * d[0]) + _r(pb[:, 5 * c + 1] * d[1])) + _r(pb[:, 5 * c + 2] * d[2]))
    near, far = pb[:, 15], pb[:, 16]
    rec[:, RF_NEAR], rec[:, RF_FAR] = near, far
    span = _r(far - near)
    rec[:, RF_STEP] = _r(span / float(np.float32(Nc - 1)))
    rec[:, RF_DELTA] = _r(span / float(np.float32(Nc)))
    return rec.astype(np.float32)


def coarse_depth(rayf, Nc):
    """prep_parts.h coarse_depth -> t_c [B, Nc] fp32: (float)i * step + near, two roundings; the end point is far itself."""
    rf = _np32(rayf).astype(np.float64)
    i = np.arange(Nc, dtype=np.float32).astype(np.float64)
    t = _r(_r(i[None, :] * rf[:, RF_STEP, None]) + rf[:, RF_NEAR, None])
    t[:, Nc - 1] = rf[:, RF_FAR]
    return t.astype(np.float32)


def sample_point(rayf, t):
    """field_common.h sample_point -> p [B, N, 3] fp32 from rayf [B, 24] and the depths t [B, N]."""
    rf = _np32(rayf).astype(np.float64)[:, None, :]
    t = _np32(t).astype(np.float64)
    v = [_r(rf[..., RF_DCAM + k] * t) for k in range(3)]
    p = [_r(_r(_r(_r(rf[..., RF_R + 3 * c] * v[0]) + _r(rf[..., RF_R + 3 * c + 1] * v[1])) + _r(rf[..., RF_R + 3 * c + 2] * v[2]))
            + rf[..., RF_O + c]) for c in range(3)]
    return np.stack(p, axis=-1).astype(np.float32)


def point_phases(p, mutate=None):
    """fp32(p_c * f_l) -> [..., 3, 10] fp32 (one rounding: the encode sites multiply in fp32)."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    f = FREQ_POINT.astype(np.float64)
    if mutate == "coordinate_off":
        p = np.roll(p, -1, axis=-1)          # coordinate c reads p[(c + 1) % 3]
    ph = _r(p[..., :, None] * f)
    if mutate == "frequency_off":            # pair (c, l) = (1, 6) takes f_7
        ph[..., 1, 6] = _r(p[..., 1] * f[7])
    return ph.astype(np.float32)


def _encode_points(p, mutate=None):
    """(sin, cos) [rows, 30] each, pair pi = 10 c + l."""
    ph = point_phases(p, mutate).reshape(-1, 3 * L_POINT)
    sn, cs = sincos_phase(ph)
    if mutate == "lane_half":                # pairs pi and pi + 2 exchanged where pi & 2 == 0 (the other lane half's pair)
        idx = np.arange(3 * L_POINT)
        sw = np.where((idx ^ 2) < 3 * L_POINT, idx ^ 2, idx)  # (28, 29 have no partner: 30, 31 are the padding)
        sn, cs = sn[:, sw], cs[:, sw]
    return sn, cs


def gamma_p(rayf, t, mutate=None):
    """The saved gamma_p rows [B * N, 64] fp32: column 20 c + 2 l + s = (sin, cos)[s](fp32(p_c * f_l)), columns 60..63 zero
    (field_common.h encode_point_to_lds, field_fwd_reg.hip:426-443, bf16_stream.h encode_pair: all three through sincos_phase)."""
    sn, cs = _encode_points(sample_point(rayf, t).reshape(-1, 3), mutate)
    out = np.zeros((sn.shape[0], GP_COLS), dtype=np.float32)
    out[:, 0:2 * 3 * L_POINT:2] = sn
    out[:, 1:2 * 3 * L_POINT:2] = cs
    return out


def dir_phases(d_wrd):
    """fp32(d_wrd_c * f_l) -> [B, 3, 4] fp32."""
    d = np.asarray(d_wrd, dtype=np.float32).astype(np.float64)
    return _r(d[..., :, None] * FREQ_DIR.astype(np.float64)).astype(np.float32)


def gamma_d(d_wrd, site):
    """gamma_d [B, 24]: column 8 c + 2 l + s = (sin, cos)[s](fp32(d_wrd_c * f_l)).  Two sites compute it, read from the code:
      "libm"   sinf / cosf of the device library -- dvec_block (prep_parts.h:99-104: the start vector dvec of fp32 and fp32_tile) and
               k_dir_prep (field_bwd.hip:268-276: gdbuf, the weight-gradient operand of fp32 and fp32_tile).  Not restated bit for bit:
               returned as float64 sin / cos of the fp32 phase, to be compared at the library's documented ulp bound.
      "phase"  encode_dir_pair -> sincos_phase (field_fwd_bf16.hip:88, field_fwd_split.hip:87: the saved gamma_d of bf16_mlp and
               split_train, then rounded to bf16 / split into hi and mid).  fp32, bit for bit."""
    ph = dir_phases(d_wrd).reshape(-1, 3 * L_DIR)
    if site == "libm":
        sn, cs = np.sin(ph.astype(np.float64)), np.cos(ph.astype(np.float64))
        out = np.zeros((ph.shape[0], 2 * 3 * L_DIR), dtype=np.float64)
    else:
        assert site == "phase", site
        sn, cs = sincos_phase(ph)
        out = np.zeros((ph.shape[0], 2 * 3 * L_DIR), dtype=np.float32)
    out[:, 0::2] = sn
    out[:, 1::2] = cs
    return out


# ---- the output end ------------------------------------------------------------------------------------------------------------------
def dt_field(g0, g4, R, rayf, t, mutate=None):
    """The field's own part of d loss / d t_fine, float64, and its magnitude: ([rows], [rows]) on g0's device.
      d gamma_p = W_0^T g0 + W_4[:, 256:]^T g4                              mag_gamma = |W|^T |g|
      dp_c = sum_l f_l (cos phi . d gamma_sin - sin phi . d gamma_cos)       dt = sum_c d_wrd_c dp_c
      mag_dt = sum_c |d_wrd_c| sum_l f_l (|cos phi| mag_gamma,sin + |sin phi| mag_gamma,cos)
    g0, g4: tuples of parts [rows, 256] (ws_operands.read_operands); R: ws_operands.reference_weights of the mode (split: hi.hi + hi.mid
    + mid.hi); rayf [B, 24], t [B, N] the device's own.  phi is the rounded fp32 phase and sin / cos at phi are the restated fp32 values
    (the gradient is straight-through on the rounded phase)."""
    dev = g0[0].device
    W0 = R["W"][0]
    W4 = tuple(w[:, W.WIDTH:] for w in R["W"][4])
    v, m = W._mv(g0, W0, transpose=False)
    if mutate != "skip_dropped":
        v4, m4 = W._mv(g4, W4, transpose=False)
        v, m = v + v4, m + m4
    p = sample_point(rayf, t).reshape(-1, 3)
    sn, cs = _encode_points(p, mutate if mutate in ("frequency_off", "lane_half", "coordinate_off") else None)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double().to(dev)
    sn, cs = to(sn), to(cs)                                   # [rows, 30]
    f = to(FREQ_POINT).repeat(3)                               # f_l of pair 10 c + l
    if mutate == "frequency_off":
        f[1 * L_POINT + 6] = float(FREQ_POINT[7])
    dgs, dgc, ms, mc = v[:, 0:60:2], v[:, 1:60:2], m[:, 0:60:2], m[:, 1:60:2]
    if mutate == "sin_cos_swapped":
        sn, cs = cs, sn
    term = f * ((-cs if mutate == "cos_negated" else cs) * dgs - sn * dgc)
    tmag = f * (cs.abs() * ms + sn.abs() * mc)
    B, N = t.shape
    dw = to(_np32(rayf)[:, RF_DWRD:RF_DWRD + 3]).repeat_interleave(N, dim=0)  # [rows, 3]
    dp = term.view(-1, 3, L_POINT).sum(2)
    dpm = tmag.view(-1, 3, L_POINT).sum(2)
    return (dw * dp).sum(1), (dw.abs() * dpm).sum(1)


def dt_bar(mag_dt, dt_f, E, stages=1):
    """The bar of an element of the fine pass's dt_f: (s E + 2^-20) mag_dt + 2^-24 |dt_f| -- s accumulations of the mode's E behind
    d gamma_p; 2^-20 for the fp32 tail (ten levels of multiply / multiply-subtract / add per coordinate, one cross-half add and a
    three-term fma: <= 16 roundings of 2^-24 on mag_dt); 2^-24 |dt_f| for the single accumulate onto the merge's dt."""
    return (stages * E + 2.0 ** -20) * mag_dt + 2.0 ** -24 * dt_f.abs()


# ---- the test's inputs: a pose row per ray whose translation is chosen, so that the phases cover their classes --------------------------
BIG, ZERO, LOG, ORIG = range(4)
KINDS = (BIG, BIG, ZERO, LOG, ORIG)  # of translation component 3 b + c, cyclically
NEAR_MULTIPLE = 2.0 ** -10           # rad
LARGE_N = 2.0 ** 18


def field_ends_inputs(oracle, B, Nc, seed=9, candidates=256):
    """fern_inputs (lego_inputs at Nc = 64) with every ray's pose translation replaced: (row, col, pb [B, 17] float64 holding fp32 values,
    K_inv, C_true).  Component c of ray b is, by kind KINDS[(3 b + c) % 5]:
      BIG   sign (-1)^(b + c), chosen among `candidates` seeded values that put the ray's middle coarse sample at |p_c| in [290, 310] (so
            every sample of the ray stays inside the documented |p_c| <= 320) as the one with most coarse phases of |n| > 2^18 within
            2^-10 rad of a multiple of pi/2 -- the deepest cancellation of the argument reduction
      ZERO  the negative of the partial sum of coarse sample min(b, Nc - 1), so that this sample's coordinate is exactly 0
      LOG   sign (-1)^b, magnitude log-uniform in [2^-4, 2^8]
      ORIG  the fixture's own
    Deterministic.  The coverage these give is asserted by the tests that use them (coverage())."""
    row, col, pb, K, Ct = oracle.lego_inputs(B, seed=seed) if Nc == 64 else oracle.fern_inputs(B, seed=seed)
    pb = pb.to(torch.float32).numpy().copy()
    rng = np.random.default_rng([seed, B, Nc])
    rf = ray_record(row, col, pb, K, Nc)
    t_c = coarse_depth(rf, Nc)
    zero_o = rf.copy()
    zero_o[:, RF_O:RF_O + 3] = 0
    part = sample_point(zero_o, t_c).astype(np.float64)  # p - o: the sum ahead of the translation (adding 0 changes nothing)
    mid = Nc // 2
    f89 = FREQ_POINT[8:10].astype(np.float64)
    for b in range(B):
        for c in range(3):
            kind = KINDS[(3 * b + c) % len(KINDS)]
            if kind == BIG:
                sgn = -1.0 if (b + c) & 1 else 1.0
                o = (sgn * rng.uniform(290.0, 310.0, size=candidates) - part[b, mid, c]).astype(np.float32)
                p = _r(part[b, None, :, c] + o[:, None].astype(np.float64))                       # [candidates, Nc]
                ph = _r(p[:, :, None] * f89).astype(np.float32)                                       # levels 8, 9
                n, r = reduce_phase(ph)
                hits = ((np.abs(n) > LARGE_N) & (np.abs(r) < NEAR_MULTIPLE)).sum(axis=(1, 2))
                pb[b, 5 * c + 3] = o[int(hits.argmax())]
            elif kind == ZERO:
                pb[b, 5 * c + 3] = np.float32(-part[b, min(b, Nc - 1), c])
            elif kind == LOG:
                pb[b, 5 * c + 3] = np.float32((-1.0 if b & 1 else 1.0) * 2.0 ** rng.uniform(-4.0, 8.0))
    return row, col, torch.from_numpy(pb.astype(np.float64)), K, Ct


def coverage(p):
    """The classes of the phases of the points p [rows, 3] fp32:
      pairs         of the 30 (c, l) pairs, how many see all four quadrants of both signs of the phase
      near_multiple phases with |n| > 2^18 within 2^-10 rad of a multiple of pi/2
      big           coordinates with |p_c| in (300, 320]
      zero          coordinates that are exactly +-0
      max_abs       the largest |p_c|"""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    ph = point_phases(p).reshape(-1, 3 * L_POINT)
    n, r = reduce_phase(ph)
    q = quadrant(n)
    cls = q + 4 * (ph < 0)  # the quadrant is taken mod 4 of n: a negative phase has negative n
    seen = np.stack([((cls == k) & (ph != 0)).any(axis=0) for k in range(8)])
    a = np.abs(p)
    return {"pairs": int(seen.all(axis=0).sum()),
            "near_multiple": int(((np.abs(n) > LARGE_N) & (np.abs(r) < NEAR_MULTIPLE)).sum()),
            "big": int(((a > 300) & (a <= 320)).sum()), "zero": int((p == 0).sum()), "max_abs": float(a.max())}
