"""CPU: rule QD (the per-ray quantile depths of include/nerf_hip.h) through its numpy restatement (tests/quantile_reference.py), the
depth-image rule of NeRFModel.fuse_depth(depth_stat=, max_spread=) and the refusals the library makes before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import quantile_reference as QR

F32 = np.float32
QS = (0.25, 0.5, 0.75)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _exact_rays(B, N, seed):
    """weights that are multiples of 2^-20 (and sum far below 2^33): every prefix sum is exact in fp64 whatever its order"""
    rng = np.random.default_rng(seed)
    w = (rng.integers(0, 1 << 12, size=(B, N)) * rng.integers(0, 2, size=(B, N))).astype(np.float64) * 2.0 ** -20
    t = np.sort(rng.uniform(2.0, 6.0, size=(B, N)), axis=1)
    return w.astype(F32), t.astype(F32)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 192, 340])
def test_restatement_equals_the_sequential_definition_on_exact_weights(N):
    w, t = _exact_rays(5, N, N)
    q = np.array([0.1, 0.25, 0.5, 0.9], F32)
    Wi = QR.prefix_sums(w)
    assert np.array_equal(Wi, np.cumsum(w.astype(np.float64), axis=1))  # exact sums: the scan order cannot matter
    got = QR.quantile_depths(w, t, q)
    want = np.array([[QR.definition(w[b], t[b], qq) for qq in q] for b in range(w.shape[0])], F32)
    assert _bits(got, want)


def test_scan_order_is_the_hillis_steele_order_not_the_sequential_one():
    """on ordinary fp32 weights the two orders round differently somewhere: the restatement must carry the kernels' order"""
    rng = np.random.default_rng(0)
    w = rng.uniform(0, 1, size=(8, 200)).astype(F32)
    Wi = QR.prefix_sums(w)
    seq = np.cumsum(w.astype(np.float64), axis=1)
    assert np.allclose(Wi, seq, rtol=1e-14, atol=0)
    # lane 3 of a chunk holds (w0 + w1) + (w2 + w3), not ((w0 + w1) + w2) + w3
    d = w.astype(np.float64)
    assert np.array_equal(Wi[:, 3], (d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3]))
    assert np.array_equal(Wi[:, 64], d[:, 64] + Wi[:, 63])  # element 0 of the second chunk: its own weight + the carry


def test_monotone_in_q():
    rng = np.random.default_rng(1)
    for N in (5, 64, 130):
        w = (rng.uniform(0, 1, size=(16, N)) * (rng.uniform(size=(16, N)) < 0.4)).astype(F32)
        t = np.sort(rng.uniform(2, 6, size=(16, N)), axis=1).astype(F32)
        q = np.sort(rng.uniform(0.01, 0.99, size=4)).astype(F32)
        Q = QR.quantile_depths(w, t, q)
        assert (np.diff(Q, axis=1) >= 0).all()
        assert (Q >= t[:, :1]).all() and (Q <= t[:, -1:]).all()


def test_scaling_the_weights_by_a_power_of_two_changes_nothing():
    rng = np.random.default_rng(2)
    w = rng.uniform(0, 1, size=(8, 150)).astype(F32)
    t = np.sort(rng.uniform(2, 6, size=(8, 150)), axis=1).astype(F32)
    Q = QR.quantile_depths(w, t, QS)
    for s in (2.0 ** -7, 2.0 ** 5):
        assert _bits(QR.quantile_depths((w * F32(s)).astype(F32), t, QS), Q)


def test_fallbacks_give_the_last_sample():
    t = np.linspace(2, 6, 70, dtype=F32)[None]
    zero = np.zeros((1, 70), F32)
    assert (QR.quantile_depths(zero, t, QS) == t[0, -1]).all()
    nan = np.full((1, 70), 0.01, F32)
    nan[0, 30] = np.nan
    assert (QR.quantile_depths(nan, t, QS) == t[0, -1]).all()  # W is NaN: no comparison holds
    assert (QR.quantile_depths(np.array([[0.7]], F32), np.array([[3.5]], F32), QS) == F32(3.5)).all()  # N = 1: t_next = t_0
    assert (QR.quantile_depths(np.array([[0.0]], F32), np.array([[3.5]], F32), QS) == F32(3.5)).all()


def test_all_weight_in_the_first_or_the_last_sample():
    t = np.linspace(2, 6, 70, dtype=F32)[None]
    w = np.zeros((1, 70), F32)
    w[0, 0] = 0.8
    Q = QR.quantile_depths(w, t, QS)  # f = q: a q-fraction into the first interval
    want = [F32(np.float64(t[0, 0]) + np.float64(F32(q)) * (np.float64(t[0, 1]) - np.float64(t[0, 0]))) for q in QS]
    assert _bits(Q[0], np.array(want, F32))
    w = np.zeros((1, 70), F32)
    w[0, 69] = 0.8
    assert (QR.quantile_depths(w, t, QS) == t[0, 69]).all()  # the last sample is never extrapolated


def test_hit_in_element_0_of_the_second_chunk_takes_the_carry():
    t = np.linspace(2, 6, 100, dtype=F32)[None]
    w = np.zeros((1, 100), F32)
    w[0, 10], w[0, 64] = 0.25, 0.75  # W_63 = 0.25 = the carry; theta(0.5) = 0.5 lies in sample 64
    Q = QR.quantile_depths(w, t, [0.5])
    f = (0.5 - 0.25) / 0.75
    assert Q[0, 0] == F32(np.float64(t[0, 64]) + f * (np.float64(t[0, 65]) - np.float64(t[0, 64])))
    assert Q[0, 0] == QR.definition(w[0], t[0], 0.5)


def test_a_zero_weight_plateau_in_front_of_the_hit():
    t = np.linspace(2, 6, 40, dtype=F32)[None]
    w = np.zeros((1, 40), F32)
    w[0, 5], w[0, 20] = 0.5, 0.5  # W_i = 0.5 on samples 5 .. 19; theta(0.75) is first reached in sample 20
    Q = QR.quantile_depths(w, t, [0.5, 0.75])
    assert Q[0, 0] == t[0, 6]  # W_5 = theta exactly: f = 1, the far end of sample 5's interval -- not somewhere on the plateau
    assert Q[0, 1] == F32(np.float64(t[0, 20]) + 0.5 * (np.float64(t[0, 21]) - np.float64(t[0, 20])))


@pytest.mark.parametrize("a,front", [(0.3, False), (0.7, True)])
def test_two_layer_ray_the_median_stays_on_a_layer_the_mean_does_not(a, front):
    """a front layer with the share a of the hit distribution at t_a, the rest on a layer at t_b (QR.two_layer_s)"""
    N, ia, ib = 64, 12, 40
    t = np.linspace(2, 6, N, dtype=F32)
    delta = float(t[1] - t[0])
    s = np.zeros(N)
    s[ia], s[ib] = QR.two_layer_s(a)
    w = QR.weights_inclusive(s).astype(F32)
    assert abs(float(w[ia]) / float(w.sum(dtype=np.float64)) - a) < 1e-6 and np.count_nonzero(w) == 2
    med = float(QR.quantile_depths(w[None], t[None], [0.5])[0, 0])
    mean = float((w.astype(np.float64) * t).sum() / w.astype(np.float64).sum())
    ta, tb = float(t[ia]), float(t[ib])
    assert abs(med - (ta if front else tb)) <= delta, (med, ta, tb)
    assert ta < mean < tb and min(mean - ta, tb - mean) > 2 * delta  # the mean lies on neither layer


def test_depth_image_rule(pkg):
    rng = np.random.default_rng(3)
    n = 200
    a = rng.uniform(0, 1, n).astype(F32)
    a[:3] = (0.5, np.nextafter(F32(0.5), F32(0)), np.nan)
    mean = rng.uniform(2, 6, n).astype(F32)
    Q3 = np.sort(rng.uniform(2, 6, (n, 3)), axis=1).astype(F32)
    Q3[5] = (3.0, 3.1, 3.2)
    f = pkg.nerf.tsdf_depth_image
    for stat in ("mean", "median"):
        for spread in (None, 0.0, 0.5, 10.0):
            want, wrej = QR.depth_image(mean, a, Q3, stat, 0.5, spread)
            got, rej = f(mean, a, Q3, stat, 0.5, spread)
            assert _bits(got, want) and np.array_equal(rej, wrej)
            tg, tr = f(torch.from_numpy(mean), torch.from_numpy(a), torch.from_numpy(Q3), stat, 0.5, spread)
            assert _bits(tg.numpy(), want) and np.array_equal(tr.numpy(), wrej)
            fg = a >= 0.5
            assert np.isinf(got[~fg]).all() and (got[~fg] > 0).all() and not rej[~fg].any()
            assert np.isnan(got[rej]).all() and np.isfinite(got[fg & ~rej]).all()
    assert QR.depth_image(mean, a, Q3, "median", 0.5, 0.0)[1].sum() == (a >= 0.5).sum()  # every foreground pixel has spread > 0 here
    assert not QR.depth_image(mean, a, Q3, "median", 0.5, 10.0)[1].any()
    with pytest.raises(ValueError):
        f(mean, a, Q3, "mode", 0.5, None)


def test_render_refuses_quantiles_without_maps_or_outside_the_unit_interval(pkg):
    chk = pkg.nerf._check_quantiles
    assert chk(None, False) is None and chk((0.25, 0.5), True) == (0.25, 0.5)
    for bad, maps in (((0.5,), False), ((), True), ((0.1, 0.2, 0.3, 0.4, 0.5), True), ((0.0,), True), ((1.0,), True), ((float("nan"),), True)):
        with pytest.raises(ValueError):
            chk(bad, maps)


def test_the_library_refuses_bad_quantiles_before_any_device_work(pkg):
    """pointers that are never dereferenced: every refusal comes from the host-side checks"""
    _abi = pkg._abi
    L = _abi.lib()
    p = ctypes.c_void_p(256)
    ok_q = _abi.f32_array([0.5])
    ERR = -1

    def coarse(q, nq, qdepth, maps=p):
        return L.nerf_hip_coarse_composite_quantiles(p, p, p, p, 0.1, 4, 8, 8, p, p, p, p, maps, None, q, nq, qdepth)

    def merge(q, nq, qdepth, maps=p):
        return L.nerf_hip_merge_composite_quantiles(p, p, p, p, p, p, 4, 8, 8, 1e-4, p, p, p, None, 0, maps, None, q, nq, qdepth)

    def forward(q, nq, qdepth, maps=p, flags=0):
        return L.nerf_hip_forward_quantiles(p, p, p, p, p, None, 4, 8, 8, 1e-4, p, p, maps, p, 1 << 30, flags, None, q, nq, qdepth)

    for call in (coarse, merge, forward):
        assert call(ok_q, 0, p) == ERR and call(ok_q, 5, p) == ERR and call(ok_q, -1, p) == ERR
        assert call(None, 1, p) == ERR and call(ok_q, 1, None) == ERR
        assert call(ok_q, 1, p, maps=None) == ERR
        for bad in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
            assert call(_abi.f32_array([0.5, bad]), 2, p) == ERR, bad
        assert L.nerf_hip_last_error()
    assert forward(ok_q, 1, p, flags=_abi.SAVE_FOR_BACKWARD) == ERR
    assert _abi.MAX_QUANTILES == 4
