"""numpy restatement of rule VC of include/nerf_hip.h -- compact volumes: the rows of the active lattice points behind an int32 slot
lattice, fp32 or fp16 coefficients --, beside tests/volume_reference.py, whose rules VA and VL it reuses.  Shared by
tests/test_volume_compact_cpu.py and tests/test_gpu_volume_compact.py.

pack / unpack are bit-exact restatements (numpy's astype(float16) rounds to nearest even, past 65504 to +-inf, as the rule says);
``lookup`` is rule VC-L: rule VL with every corner's words taken through its slot.
"""
from typing import NamedTuple

import numpy as np

import volume_reference as R

F = np.float32
H = np.float16


class Compact(NamedTuple):
    slot: np.ndarray      # [nx, ny, nz] int32
    sigma: np.ndarray     # [n] fp32
    coef: np.ndarray      # [n, S] fp32 or fp16
    degree: int


def row_width(degree, half):
    w = 3 * (degree + 1) ** 2
    return (w + 3) // 4 * 4 if half else w


def slots(index, shape):
    s = np.full(int(np.prod(shape)), -1, np.int32)
    s[np.asarray(index, np.int64)] = np.arange(len(index), dtype=np.int32)
    return s.reshape(shape)


def rows(coef_words, half):
    """coef_words [n, 3 ncoef] fp32 -> the stored rows: the same words, or their fp16 roundings with +0 pad halves"""
    coef_words = np.asarray(coef_words, F)
    if not half:
        return coef_words.copy()
    n, w = coef_words.shape
    out = np.zeros((n, (w + 3) // 4 * 4), H)
    with np.errstate(over="ignore"):
        out[:, :w] = coef_words.astype(H)
    return out


def pack(sigma, coef, half):
    """dense (sigma [nx, ny, nz], coef [nx, ny, nz, ncoef, 3]) -> Compact over rule VA's active list"""
    shape = sigma.shape
    nc = coef.shape[3]
    index = R.active(sigma)
    return Compact(slots(index, shape), np.asarray(sigma, F).reshape(-1)[index].copy(),
                   rows(np.asarray(coef, F).reshape(-1, nc * 3)[index], half), {1: 0, 4: 1, 9: 2}[nc])


def unpack(c):
    """-> dense (sigma, coef) fp32: the rows at the points whose slot lies in [0, n), +0 elsewhere"""
    shape = c.slot.shape
    nc = (c.degree + 1) ** 2
    n = c.sigma.shape[0]
    flat = c.slot.reshape(-1)
    pts = np.flatnonzero((flat >= 0) & (flat < n))
    sigma = np.zeros(flat.size, F)
    coef = np.zeros((flat.size, nc * 3), F)
    sigma[pts] = c.sigma[flat[pts]]
    coef[pts] = c.coef[flat[pts], :nc * 3].astype(F)
    return sigma.reshape(shape), coef.reshape(*shape, nc, 3)


def lookup(c, lo, step, x, d):
    """Rule VC-L at points x [M, 3] along d [M, 3] -> (sigma_s [M], rgb [M, 3]) fp32: rule VL's arithmetic (volume_reference's _tri and
    its bracketed sums) over corner values fetched through the slots, one corner at a time."""
    x = np.asarray(x, F).reshape(-1, 3)
    d = np.asarray(d, F).reshape(-1, 3)
    shape = c.slot.shape
    nc = (c.degree + 1) ** 2
    n = c.sigma.shape[0]
    inside, ci, f = R.cells(x, lo, step, shape)
    M = x.shape[0]
    sv = np.zeros((M, 2, 2, 2), F)
    cv = np.zeros((M, 2, 2, 2, nc, 3), F)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                s = c.slot[ci[:, 0] + di, ci[:, 1] + dj, ci[:, 2] + dk]
                ok = (s >= 0) & (s < n)
                r = np.where(ok, s, 0)
                if n:
                    sv[:, di, dj, dk] = np.where(ok, c.sigma[r], F(0))
                    cv[:, di, dj, dk] = np.where(ok[:, None, None], c.coef[r, :nc * 3].astype(F).reshape(M, nc, 3), F(0))
    sig = R._tri(sv, f)
    Y = R.basis32(d)[:, :nc]
    with np.errstate(all="ignore"):
        val = (Y[:, None, None, None, 0, None] * cv[..., 0, :]).astype(F)
        for m in range(1, nc):
            val = (val + (Y[:, None, None, None, m, None] * cv[..., m, :]).astype(F)).astype(F)
        rgb = np.fmin(np.fmax(R._tri(val, f), F(0)), F(1)).astype(F)
    return np.where(inside, sig, F(0)).astype(F), np.where(inside[:, None], rgb, F(0)).astype(F)


GARBAGE = np.asarray([-3.0, -0.0, np.nan, -1e-3], F)


def with_garbage(sigma, coef, seed=1):
    """sigma with the INACTIVE points overwritten by draws from {-3, -0, NaN, -1e-3}; the coefficients (random everywhere) are left.
    -> (sigma', the inactive mask [nx, ny, nz])"""
    act = np.zeros(sigma.size, bool)
    act[R.active(sigma)] = True
    inactive = ~act.reshape(sigma.shape)
    rng = np.random.default_rng(seed)
    out = sigma.copy()
    out[inactive] = GARBAGE[rng.integers(0, 4, int(inactive.sum()))]
    return out, inactive


def zeroed(sigma, coef, inactive):
    """the volume with +0 at the inactive points"""
    s, c = sigma.copy(), coef.copy()
    s[inactive] = 0
    c[inactive] = 0
    return s, c


def sample_points(shape, lo, step, seed=3):
    """test_gpu_volume.py::test_sample's point classes: inside, lattice points, faces, one ulp outside, far outside, non-finite"""
    rng = np.random.default_rng(seed)
    hi = (lo + (np.asarray(shape) - 1).astype(F) * step).astype(F)
    inside = (lo + rng.uniform(0, 1, (120, 3)) * (hi - lo)).astype(F)
    lattice = R.lattice_points(np.arange(int(np.prod(shape)))[::3], shape, lo, step)
    faces = inside[:24].copy()
    ax, low = np.arange(24) % 3, np.arange(24) % 2 == 0
    faces[np.arange(24), ax] = np.where(low, lo[ax], hi[ax])
    outside = (inside[:30] + np.asarray([2.5, 0, 0], F) * rng.choice([-1, 1], (30, 1))).astype(F)
    beyond = faces.copy()
    beyond[np.arange(24), ax] = np.nextafter(beyond[np.arange(24), ax], np.where(low, -np.inf, np.inf).astype(F))
    weird = np.asarray([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], F)
    x = np.concatenate([inside, lattice, faces, outside, beyond, weird]).astype(F)
    d = rng.normal(size=x.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[5] *= 1.7
    return x, d.astype(F)
