"""CPU: rule NM (the per-ray normal composite of include/nerf_hip.h) through its numpy restatement (tests/normal_reference.py),
nerf.unit_normals, render's normals keyword and the refusals the library makes before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import normal_reference as NR

F32 = np.float32


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _exact_rays(B, N, seed):
    """weights that are multiples of 2^-20 and axis-aligned gradients (normals (+-1, 0, 0) and so on): every product and sum is exact"""
    rng = np.random.default_rng(seed)
    w = (rng.integers(0, 1 << 12, size=(B, N)) * rng.integers(0, 2, size=(B, N))).astype(np.float64) * 2.0 ** -20
    g = np.zeros((B, N, 3), F32)
    ax = rng.integers(0, 3, size=(B, N))
    mag = rng.uniform(0.1, 50.0, size=(B, N)) * rng.choice([-1.0, 1.0], size=(B, N))
    np.put_along_axis(g, ax[..., None], mag[..., None].astype(F32), axis=2)
    return w.astype(F32), g


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 192, 340])
def test_restatement_equals_the_sequential_definition_on_exact_operands(N):
    w, g = _exact_rays(5, N, N)
    n = NR.field_normals(g)
    assert set(np.unique(n)) <= {-1.0, 0.0, 1.0} and (np.abs(n).sum(-1) == 1).all()
    S = NR.composite64(w, g)
    want = np.stack([NR.sequential(w[b], g[b]) for b in range(w.shape[0])])
    assert np.array_equal(S, want)
    assert _bits(NR.composite(w, g), want.astype(F32))


def test_zero_infinite_and_nan_gradients_give_a_zero_normal():
    g = np.array([[0, 0, 0], [np.inf, 1, 2], [1, -np.inf, 0], [np.nan, 1, 1], [1, 1, np.nan], [3e38, 3e38, 0], [0, -0.0, 0]], F32)
    assert (NR.field_normals(g) == 0).all() and not np.isnan(NR.field_normals(g)).any()
    n = NR.field_normals(np.array([[3, 0, -4]], F32))
    assert _bits(n, np.array([[F32(-3) / F32(5), -0.0, F32(4) / F32(5)]], F32))
    w = np.full((1, 7), 0.5, F32)
    assert (NR.composite(w, g[None]) == 0).all()


def test_zero_and_nan_weights_add_nothing():
    rng = np.random.default_rng(0)
    w = rng.uniform(0, 1, size=(4, 100)).astype(F32)
    g = rng.normal(size=(4, 100, 3)).astype(F32)
    base = NR.composite64(w[:, :60], g[:, :60])
    w2 = w.copy()
    w2[:, 60:80] = 0.0
    w2[:, 80:] = np.nan
    S = NR.composite64(w2, g)
    assert np.isfinite(S).all() and np.array_equal(S, base)
    assert np.array_equal(NR.bound(w2, S), NR.bound(w[:, :60], base))
    g2 = g.copy()
    g2[:, 60:] = np.nan  # (and a NaN gradient under a NaN weight)
    assert np.array_equal(NR.composite64(w2, g2), base)


def test_length_is_bounded_by_the_opacity():
    rng = np.random.default_rng(1)
    for N in (3, 64, 192, 2048):
        w = (rng.uniform(0, 1, size=(16, N)) * (rng.uniform(size=(16, N)) < 0.5)).astype(F32)
        g = (rng.normal(size=(16, N, 3)) * 10.0 ** rng.uniform(-3, 3, size=(16, N, 1))).astype(F32)
        S = NR.composite64(w, g)
        A = w.astype(np.float64).sum(axis=1)
        assert (np.sqrt((S * S).sum(-1)) <= A * (1 + 1e-6)).all()
        aligned = np.broadcast_to(np.array([1.0, -2.0, 2.0], F32), g.shape)  # every normal the same: |N| = A up to the normals' rounding
        S = NR.composite64(w, aligned)
        assert np.allclose(np.sqrt((S * S).sum(-1)), A, rtol=1e-6, atol=0)


def test_scaling_the_gradients_by_a_power_of_two_changes_nothing():
    rng = np.random.default_rng(2)
    w = rng.uniform(0, 1, size=(8, 150)).astype(F32)
    g = rng.normal(size=(8, 150, 3)).astype(F32)
    N = NR.composite(w, g)
    for s in (2.0 ** -9, 2.0 ** 7):
        assert _bits(NR.field_normals((g * F32(s)).astype(F32)), NR.field_normals(g))
        assert _bits(NR.composite(w, (g * F32(s)).astype(F32)), N)


def test_opposite_normals_of_equal_weight_cancel_exactly():
    rng = np.random.default_rng(3)
    g = rng.normal(size=(6, 40, 3)).astype(F32)
    w = rng.uniform(0, 1, size=(6, 40)).astype(F32)
    g2 = np.concatenate((g, -g), axis=1)
    w2 = np.concatenate((w, w), axis=1)
    # pair by pair (sample i and its mirror behind each other): every partial sum returns to exactly 0
    order = np.stack((np.arange(40), np.arange(40) + 40), axis=1).reshape(-1)
    for b in range(6):
        assert (NR.sequential(w2[b, order], g2[b, order]) == 0).all()
    assert (NR.composite(w2[:, order[:2]], g2[:, order[:2]]) == 0).all()
    S = NR.composite64(w2, g2)  # any other order: inside the reordering bound of 0
    assert (np.abs(S) <= 1e-12 * w2.astype(np.float64).sum(axis=1)[:, None]).all()


def test_unit_normals(pkg):
    f = pkg.nerf.unit_normals
    Nrm = np.array([[0.3, 0.0, -0.4], [0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [0.1, 0.1, 0.1], [np.nan, 0.0, 0.0], [0.0, 2e-3, 0.0]], F32)
    A = np.array([0.9, 0.9, 0.5, 0.49, 0.9, np.nan], F32)
    got = f(Nrm, A)
    assert got.dtype == F32 and got.shape == Nrm.shape
    assert np.allclose(got[0], [0.6, 0.0, -0.8], rtol=1e-6) and _bits(got[2], np.array([1.0, 0.0, 0.0], F32))
    assert (got[[1, 3, 4, 5]] == 0).all() and not np.isnan(got).any()
    assert (f(Nrm, A, min_opacity=0.0)[3] > 0.5).all()  # below the default bar only
    t = f(torch.from_numpy(Nrm), torch.from_numpy(A))
    assert _bits(t.numpy(), got)
    img = f(np.broadcast_to(Nrm[0], (4, 5, 3)), np.full((4, 5), 0.9, F32))
    assert img.shape == (4, 5, 3) and np.allclose(np.sqrt((img * img).sum(-1)), 1.0, rtol=1e-6)


def test_render_refuses_normals_without_maps_or_of_an_unknown_kind(pkg):
    chk = pkg.nerf._check_normals
    assert chk(False, False) == 0 and chk(None, True) == 0
    assert chk(True, True) == 2 and chk("fine", True) == 2 and chk("coarse", True) == 1 and chk("both", True) == 3
    for bad, maps in ((True, False), ("fine", False), ("all", True), (3, True), ("", True)):
        with pytest.raises(ValueError):
            chk(bad, maps)
    C, M, Q, Nrm = (torch.zeros(2, k) for k in (3, 4, 2, 6))
    res = pkg.nerf._render_result
    assert res(C, C, M, None, Nrm)[-1] is Nrm and len(res(C, C, M, None, Nrm)) == 4
    assert res(C, C, M, Q, Nrm)[3] is Q and res(C, C, M, Q, Nrm)[4] is Nrm
    assert len(res(C, C, M, Q)) == 4 and len(res(C, C, M, None)) == 3 and len(res(C, C, None, None)) == 2


def test_cli_and_display_take_the_normal_map_switch(pkg):
    import importlib
    import inspect

    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    assert ap.parse_args(["--normal-map"]).normal_map is True and ap.parse_args([]).normal_map is False
    assert inspect.signature(pkg.NeRFRunner.display).parameters["normals"].default is False
    assert inspect.signature(pkg.NeRFModel.render).parameters["normals"].default is False
    par = importlib.import_module("nerf_tiny_amd.parallel")
    assert inspect.signature(par.render_rows_sharded).parameters["normals"].default is False


def test_the_library_refuses_bad_normal_calls_before_any_device_work(pkg):
    """pointers that are never dereferenced: every refusal comes from the host-side checks"""
    _abi = pkg._abi
    L = _abi.lib()
    p = ctypes.c_void_p(256)
    ERR = -1
    need = _abi.normals_ws_bytes(4, 8, 8)

    def forward(passes=2, normals=p, nws=p, nws_bytes=need, maps=p, flags=0, B=4, Nc=8, Nf=8):
        return L.nerf_hip_forward_normals(p, p, p, p, p, None, B, Nc, Nf, 1e-4, p, p, maps, p, 1 << 30, flags, None, passes, normals, nws,
                                          nws_bytes)

    for passes in (0, 4, -1, 7):
        assert forward(passes=passes) == ERR
    assert forward(normals=None) == ERR and forward(nws=None) == ERR and forward(maps=None) == ERR
    assert forward(nws_bytes=need - 1) == ERR and forward(nws_bytes=0) == ERR
    assert forward(nws=ctypes.c_void_p(384)) == ERR  # not 256-byte aligned
    assert forward(flags=_abi.SAVE_FOR_BACKWARD) == ERR
    assert forward(B=1) == ERR and forward(Nc=1) == ERR and forward(Nf=0) == ERR and forward(Nc=1025) == ERR  # what the maps call refuses
    assert L.nerf_hip_last_error()

    def stage(w=p, g=p, B=4, N=8, out=p, stride=3):
        return L.nerf_hip_normal_composite(w, g, B, N, out, stride, None)

    assert stage(N=0) == ERR and stage(N=2049) == ERR and stage(B=-1) == ERR and stage(stride=2) == ERR
    assert stage(w=None) == ERR and stage(g=None) == ERR and stage(out=None) == ERR
    assert stage(B=0) == 0 and stage(B=0, w=None, g=None, out=None) == 0  # nothing to launch

    n = ctypes.c_size_t(0)
    assert L.nerf_hip_normals_ws_bytes(4, 8, 8, None) == ERR and L.nerf_hip_normals_ws_bytes(1, 8, 8, ctypes.byref(n)) == ERR
    assert L.nerf_hip_normals_ws_offset(4, 8, 8, b"nothing", ctypes.byref(n)) == ERR
    assert L.nerf_hip_normals_ws_offset(4, 8, 8, None, ctypes.byref(n)) == ERR and L.nerf_hip_normals_ws_offset(4, 8, 8, b"grad", None) == ERR


def test_side_workspace_layout(pkg):
    _abi = pkg._abi
    L = _abi.lib()

    def off(B, Nc, Nf, name):
        n = ctypes.c_size_t(0)
        _abi.check(L.nerf_hip_normals_ws_offset(B, Nc, Nf, name.encode(), ctypes.byref(n)))
        return n.value

    names = ("bundle", "w_m", "packed", "fold", "save", "masks", "spre", "sigma", "points", "grad")
    for B, Nc, Nf in ((2, 8, 8), (7, 65, 63), (700, 64, 128), (16384, 64, 128)):
        o = [off(B, Nc, Nf, nm) for nm in names]
        assert o[0] == 0 and all(x % 256 == 0 for x in o) and o == sorted(o) and len(set(o)) == len(o)
        total = _abi.normals_ws_bytes(B, Nc, Nf)
        chunk = 131072
        assert o[1] - o[0] >= B * (Nc + Nf) * 20 and o[2] - o[1] >= B * (Nc + Nf) * 4
        assert o[9] - o[8] >= chunk * 12 and total - o[9] >= chunk * 12 and total - o[9] < chunk * 12 + 256
    # the part that grows with B: 24 bytes per merged sample
    d = _abi.normals_ws_bytes(16384, 64, 128) - _abi.normals_ws_bytes(8192, 64, 128)
    assert d == 8192 * 192 * 24


def test_the_main_workspace_is_the_parents(pkg):
    """the inference layouts of the main workspace still hold no bundle and no merged weights (test_bf16_layout_cpu holds the recorded
    sizes and offsets): the side workspace took nothing from and added nothing to the main one"""
    _abi = pkg._abi
    for flags in (0, _abi.BF16_MLP, _abi.SPLIT_MLP):
        n = ctypes.c_size_t(0)
        for name in (b"bundle", b"w_m"):
            assert _abi.lib().nerf_hip_ws_offset(64, 64, 128, flags, name, ctypes.byref(n)) == -1  # not part of an inference layout
