"""The narrow-band density grid of nerf_hip_band_begin / nerf_hip_band_grow (include/nerf_hip.h) restated in
vectorised numpy.  The exact field values are copied from a given dense grid, so `band(dense, level, r)` is what the device must return
when its field launches write density_grid's bits.  Used by tests/test_mesh_band_cpu.py and tests/test_gpu_mesh_band.py."""
import numpy as np


def corner_indices(n, r):
    """The unique corner planes min(b * r, n - 1), b = 0 .. ceil(n / r), of an axis of n points."""
    nb = -(-n // r)
    return np.unique(np.minimum(np.arange(nb + 1) * r, n - 1))


def _mixed(inside):
    """[a, b, c] classes -> [a-1, b-1, c-1]: the 8 corners of a cell are not all of one class (an axis of one point has no cells)."""
    a, b, c = (max(n - 1, 0) for n in inside.shape)
    cnt = np.zeros((a, b, c), np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += inside[dx:dx + a, dy:dy + b, dz:dz + c]
    return (cnt > 0) & (cnt < 8)


def _dilate(m):
    """m grown by one block in the 26-neighbourhood, clipped to the grid."""
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    a, b, c = m.shape
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= p[dx:dx + a, dy:dy + b, dz:dz + c]
    return out


def _erode_in_grid(m):
    """Blocks whose in-grid 26-neighbours (and they themselves) are all in m."""
    return ~_dilate(~m)


def _expand(blocks, shape, r):
    """Per-block flags -> per-point flags of the points the blocks own."""
    out = blocks
    for a in range(3):
        out = np.repeat(out, r, axis=a)
    return out[:shape[0], :shape[1], :shape[2]]


def band(dense, level, r):
    """-> (array, info).  array: the dense-shaped fp32 grid after corner pass, fill and the grow rounds; info: rounds, blocks_active,
    blocks_total, points_evaluated, points_total, and `trace` = [(new blocks, next seeds)] per round."""
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    r = int(r)
    if r < 2:
        raise ValueError("block >= 2")
    level = np.float32(level)
    shape = dense.shape
    nb = tuple(-(-n // r) for n in shape)
    cidx = [corner_indices(n, r) for n in shape]
    # 1. corner pass (their own positions; the fill below overwrites the clamped last planes again) and 3. seeds from these samples
    cpos = [np.minimum(np.arange(k + 1) * r, n - 1) for k, n in zip(nb, shape)]
    with np.errstate(invalid="ignore"):
        cin = dense[np.ix_(*cpos)] > level  # [nbx + 1, nby + 1, nbz + 1], NaN outside
    cnt = np.zeros(nb, np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += cin[dx:dx + nb[0], dy:dy + nb[1], dz:dz + nb[2]]
    S = (cnt > 0) & (cnt < 8)
    evaluated = int(np.prod([c.size for c in cidx]))
    # 2. fill: every point takes its block's lowest point
    low = [(np.arange(n) // r) * r for n in shape]
    out = dense[np.ix_(*low)].copy()
    A = np.zeros(nb, bool)
    trace = []
    rounds = 0
    while S.any():
        new = _dilate(S) & ~A
        A |= new
        pts = _expand(new, shape, r)
        out[pts] = dense[pts]
        evaluated += int(pts.sum())
        with np.errstate(invalid="ignore"):
            mixed = _mixed(out > level)
        # points that are a corner of a mixed cell
        touched = np.zeros(shape, bool)
        a, b, c = mixed.shape
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    touched[dx:dx + a, dy:dy + b, dz:dz + c] |= mixed
        own_touch = np.zeros(nb, bool)
        ti, tj, tk = np.nonzero(touched)
        own_touch[ti // r, tj // r, tk // r] = True
        S = A & ~_erode_in_grid(A) & own_touch
        rounds += 1
        trace.append((int(new.sum()), int(S.sum())))
    info = dict(rounds=rounds, blocks_active=int(A.sum()), blocks_total=int(np.prod(nb)), points_evaluated=evaluated,
                points_total=int(np.prod(shape)), trace=trace)
    return out, info


# ---- the test field: sigma = 100 max(0, cos(pi x) + cos(pi y) + cos(pi z) - thr), one closed blob on [-1, 1]^3 ----
BOX_LO, BOX_HI, LEVEL = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 30.0
# (shape, block, thr) -> dense V, F and the rounds as (new blocks, next seeds), computed on the CPU from the analytic fp32 field
CASES = [
    ((49, 49, 49), 4, 1.5, 3150, 6296, [(696, 16), (16, 0)]),
    ((50, 41, 45), 4, 1.5, 2734, 5464, [(548, 26), (52, 0)]),
    ((64, 70, 61), 5, 2.0, 3028, 6052, [(406, 18), (40, 0)]),
    ((33, 33, 33), 2, 2.4, 294, 584, [(312, 33), (57, 0)]),
    ((65, 65, 65), 8, 2.2, 2094, 4184, [(160, 6), (12, 0)]),
    ((129, 129, 129), 8, 2.2, 8382, 16760, [(432, 0)]),
    ((257, 129, 65), 4, 1.5, 26486, 52968, [(5008, 334), (362, 0)]),  # 36,465 blocks: a block scan over many workgroups
]


def blob_weights(oracle, thr):
    """The hand-built MLP of the blob: make_weights(5, False) with the density branch replaced (the colour layers keep their weights)."""
    import torch

    w = oracle.make_weights(5, False)
    for i in range(8):
        w[f"network.point_layer.{i}.0.weight"] = torch.zeros_like(w[f"network.point_layer.{i}.0.weight"])
        w[f"network.point_layer.{i}.0.bias"] = torch.zeros_like(w[f"network.point_layer.{i}.0.bias"])
    w["network.sigma_layer.0.weight"] = torch.zeros_like(w["network.sigma_layer.0.weight"])
    w["network.sigma_layer.0.bias"] = torch.zeros_like(w["network.sigma_layer.0.bias"])
    for c in range(3):
        w["network.point_layer.0.0.weight"][0, 20 * c + 1] = 1.0  # cos(f_0 x_c), f_0 = fp32 pi
    w["network.point_layer.0.0.bias"][0] = 3.0
    for i in range(1, 7):
        w[f"network.point_layer.{i}.0.weight"][0, 0] = 1.0
    w["network.point_layer.7.0.weight"][0, 0] = 100.0
    w["network.point_layer.7.0.bias"][0] = -100.0 * (3.0 + thr)
    w["network.sigma_layer.0.weight"][0, 0] = 1.0
    return w


def blob_points(shape):
    """The lattice axes of density_grid over the box: lo + i * step, one fp32 product and one fp32 sum."""
    lo, hi = np.float32(BOX_LO), np.float32(BOX_HI)
    step = [(hi[c] - lo[c]) / np.float32(max(n - 1, 1)) if n > 1 else np.float32(0) for c, n in enumerate(shape)]
    return [lo[c] + np.arange(n, dtype=np.float32) * np.float32(step[c]) for c, n in enumerate(shape)], np.float32(step)


def blob_analytic(shape, thr):
    axes, _ = blob_points(shape)
    c = [np.cos(np.float32(np.pi) * a, dtype=np.float32) for a in axes]
    s = c[0][:, None, None] + c[1][None, :, None] + c[2][None, None, :]
    return (np.float32(100) * np.maximum(np.float32(0), s - np.float32(thr))).astype(np.float32)
