"""GPU: rays against a mesh on the device (nerf_hip_mesh_raycast*, nerf_hip_mesh_face_rays, nerf_hip_mesh_select_faces_*;
mesh.build_raycast / raycast / camera_rays / render_depth / visibility / filter_faces; extract_mesh(visible=)) against the numpy
restatement in tests/raycast_reference.py.  Everything is exact equality: t and uv as bits, faces, sides, flags and counts as
integers."""
import functools
import glob

import numpy as np
import pytest
import torch

import raycast_reference as R
import simplify_meshes as M

pytestmark = pytest.mark.gpu
F32 = np.float32

TRIANGLE = (np.array([[0.5, 0.25, 0.0], [3.0, 0.5, 1.0], [1.0, 2.5, -1.0]], F32), np.array([[0, 1, 2]], np.int32))
MESHES = {
    "blobs": lambda: M.blobs()[:2],
    "random": lambda: M.random_mesh()[:2],
    "fan": lambda: M.fan()[:2],
    "bad_input": lambda: M.bad_input()[:2],
    "triangle": lambda: TRIANGLE,
}
INSIDE = {"blobs": M.BALLS[0][0]}  # the centre of the first ball: every ray from it meets a face from behind


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the inputs are read-only)


def _mesh(pkg, dev, v, f, n=None, c=None):
    return pkg.mesh.Mesh(_t(np.asarray(v, F32), dev), _t(np.asarray(f, np.int32), dev), None if n is None else _t(n, dev),
                         None if c is None else _t(c, dev))


def _bytes(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    """four outputs of a closest-hit cast, bit for bit (t and uv as fp64 bits)"""
    assert len(got) == len(want) == 4
    for g, w, dt in zip(got, want, (torch.float64, torch.float64, torch.int32, torch.int8)):
        assert g.dtype == dt and tuple(g.shape) == tuple(w.shape)
        if not np.array_equal(_bytes(g), _bytes(w)):
            return False
    return True


def look_at(cam, target, near=1.0, far=60.0):
    """a pose row [17]: the camera at cam looking at target (the third column of R is the viewing direction of K_INV's rays)"""
    cam, target = np.asarray(cam, np.float64), np.asarray(target, np.float64)
    fwd = (target - cam) / np.linalg.norm(target - cam)
    right = np.cross(fwd, [0.0, 0.3, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    P = np.zeros((3, 5))
    P[:, 0], P[:, 1], P[:, 2], P[:, 3] = right, up, fwd, cam
    return np.concatenate((P.reshape(-1), [near, far])).astype(F32)


def k_inv(H, W, s):
    """pixel (x, y) -> p = (s (x - H / 2), s (y - W / 2), 1)"""
    return np.array([[s, 0, 0], [0, s, 0], [-s * H / 2, -s * W / 2, 1]], F32)


def _box(v):
    return R._box(v)


def _cameras(v, n=4, dist=2.2):
    lo, hi = _box(v)
    c, r = (lo + hi).astype(np.float64) / 2, float(np.linalg.norm(hi - lo)) / 2 + 1e-3
    dirs = np.array([[1, 0.2, 0.3], [-0.6, 1, 0.1], [0.1, -0.7, 1], [-0.5, -0.6, -0.8], [0.9, 0.8, -0.4], [-1, 0.1, 0.5]], np.float64)[:n]
    return np.stack([look_at(c + d / np.linalg.norm(d) * r * dist, c) for d in dirs])


@functools.lru_cache(maxsize=None)
def _cpu_rays(name):
    """every ray set that needs no device, concatenated -> (o, d, the slices by name)"""
    v, f = MESHES[name]()
    sets = {"lattice": R.lattice_rays(v, step=2.5 if name in ("random", "bad_input") else 1.5)}
    lo, hi = _box(v)
    sets["inside"] = R.random_rays(v, 100, 2, inside=INSIDE.get(name, (lo + hi) / 2))
    o, d = R.random_rays(v, 120, 3)
    sets["scaled"] = (np.concatenate((o[:60], o[60:])), np.concatenate((d[:60] * F32(1e-3), d[60:] * F32(1e6))))
    sets["planes"] = R.plane_rays(R.raycast_grid(v, f), n=4)
    sets["planes"] = (sets["planes"][0][::2], sets["planes"][1][::2])
    far = (o[:60].astype(np.float64) - d[:60].astype(np.float64) * 3000.0).astype(F32)
    sets["far"] = (np.concatenate((far, (o[60:].astype(np.float64) * 1e4).astype(F32))), np.concatenate((d[:60], -o[60:])))
    sets["bad"] = R.bad_rays()
    cut, at = {}, 0
    for k, (oo, dd) in sets.items():
        cut[k] = slice(at, at + len(oo))
        at += len(oo)
    return np.concatenate([s[0] for s in sets.values()]), np.concatenate([s[1] for s in sets.values()]), cut


@functools.lru_cache(maxsize=None)
def _want(name):
    v, f = MESHES[name]()
    o, d, _ = _cpu_rays(name)
    return R.cast(v, f, o, d)


# ---- (1) closest hit ----

@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "triangle"])
def test_closest_hit(pkg, dev, name):
    v, f = MESHES[name]()
    h = pkg.mesh.build_raycast(_mesh(pkg, dev, v, f))
    o, d, cut = _cpu_rays(name)
    want = _want(name)
    got = pkg.mesh.raycast(h, _t(o, dev), _t(d, dev))
    assert _same(got, want)
    t, uv, face, side = want
    hit = face >= 0
    print(f"{name}: F {len(f)}, grid {h.dims} cell {float(h.cell):.4g} E {h.entries} OUTSIDE {h.outside}; {len(o)} rays, {int(hit.sum())} hit")
    assert h.taking_part == int(R.face_part(v, f).sum()) and [h.taking_part, h.entries, h.outside] == R.grid_counts(v, f, h.lo, h.cell, h.dims)
    assert (face[cut["bad"]][[1, 2, 3, 4, 5, 6]] == -1).all() and np.isinf(t[cut["bad"]][[1, 2, 3, 4, 5, 6]]).all()
    assert (side[~hit] == 0).all() and not uv[~hit].any() and np.isinf(t[~hit]).all() and (np.abs(side[hit]) == 1).all()
    if name in ("blobs", "random"):
        # rays down the axes through lattice points run along shared edges and vertices: the lowest face index wins
        lat = cut["lattice"]
        ties = 0
        for i in np.flatnonzero(hit[lat])[:150]:
            tt = R.cast(v, f, o[lat][i:i + 1], d[lat][i:i + 1], skip=face[lat][i:i + 1])[0][0]
            ties += int(tt == t[lat][i])
        print(f"{name}: {int(hit[lat].sum())} of {lat.stop - lat.start} lattice rays hit, {ties} of the first 150 tie between faces")
        assert ties >= 30 and hit[lat].sum() >= 50
    if name == "blobs":
        ins = cut["inside"]
        assert hit[ins].all() and (side[ins] == -1).all() and (side[cut["far"]][hit[cut["far"]]] == 1).all() and hit[cut["far"]].sum() > 20
        sc = cut["scaled"]
        assert hit[sc].sum() > 30 and t[sc][:60][hit[sc][:60]].min() > 100 and t[sc][60:][hit[sc][60:]].max() < 1e-5
    # windows that cut off the first hit, and skip, on every fifth ray
    sub = slice(None, None, 5)
    first = face[sub].copy()
    tf = t[sub][first >= 0]
    tmid = float(np.median(tf)) if len(tf) else 1.0
    for kw in (dict(tmin=tmid), dict(tmax=tmid), dict(tmin=tmid * 0.5, tmax=tmid * 1.5), dict(tmin=-np.inf, tmax=np.inf), dict(skip=first),
               dict(tmin=2.0, tmax=1.0)):
        w = R.cast(v, f, o[sub], d[sub], **kw)
        kg = {k: (_t(x.astype(np.int32), dev) if k == "skip" else x) for k, x in kw.items()}
        assert _same(pkg.mesh.raycast(h, _t(o[sub], dev), _t(d[sub], dev), **kg), w), kw
        occ = pkg.mesh.raycast(h, _t(o[sub], dev), _t(d[sub], dev), any_hit=True, **kg)
        assert occ.dtype == torch.uint8 and np.array_equal(occ.cpu().numpy(), (w[2] >= 0).astype(np.uint8)), kw
    if hit.any():
        assert not np.array_equal(R.cast(v, f, o[sub], d[sub], skip=first)[2][first >= 0], first[first >= 0])
    occ = pkg.mesh.raycast(h, _t(o, dev), _t(d, dev), any_hit=True)
    assert np.array_equal(occ.cpu().numpy(), hit.astype(np.uint8))


@pytest.mark.parametrize("name", ["blobs", "bad_input"])
def test_camera_rays_and_depth_images(pkg, dev, name):
    v, f = MESHES[name]()
    h = pkg.mesh.build_raycast(_mesh(pkg, dev, v, f))
    H, W = 20, 23
    poses, K = _cameras(v, 2), k_inv(H, W, 0.03)
    o, d = pkg.mesh.camera_rays(_t(poses, dev), torch.from_numpy(K), H, W)
    assert tuple(o.shape) == (2 * H * W, 3) == tuple(d.shape) and o.dtype == torch.float32 == d.dtype
    on, dn = o.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(on.reshape(2, H * W, 3), np.broadcast_to(poses[:, None, :15].reshape(2, 1, 3, 5)[..., 3], (2, H * W, 3)))
    assert np.abs(np.linalg.norm(dn.astype(np.float64), axis=1) - 1).max() < 1e-6  # d_wrd: unit directions, so t is a depth
    # pixel (x, y) of camera c: along R (s (x - H / 2), s (y - W / 2), 1)
    x, y, c = 7, 19, 1
    p = np.array([0.03 * (x - H / 2), 0.03 * (y - W / 2), 1.0])
    want_d = poses[c][:15].reshape(3, 5)[:, :3].astype(np.float64) @ (p / np.linalg.norm(p))
    assert np.abs(dn[(c * H + x) * W + y] - want_d).max() < 1e-6
    want = R.cast(v, f, on, dn)
    assert _same(pkg.mesh.raycast(h, o, d), want) and (want[2] >= 0).sum() > 50
    t, face, uv = pkg.mesh.render_depth(h, _t(poses, dev), torch.from_numpy(K), H, W)
    assert tuple(t.shape) == (2, H, W) == tuple(face.shape) and tuple(uv.shape) == (2, H, W, 2)
    assert np.array_equal(_bytes(t.reshape(-1)), _bytes(want[0])) and np.array_equal(face.reshape(-1).cpu().numpy(), want[2])
    assert np.array_equal(_bytes(uv.reshape(-1, 2)), _bytes(want[1]))


def test_empty_meshes_and_no_rays(pkg, dev):
    o, d = R.random_rays(np.array([[0, 0, 0], [4, 4, 4]], F32), 70, 1)
    for v, f in ((np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), (TRIANGLE[0], np.zeros((0, 3), np.int32)),
                 (np.full((4, 3), np.nan, F32), np.array([[0, 1, 2], [1, 2, 3]], np.int32))):
        h = pkg.mesh.build_raycast(_mesh(pkg, dev, v, f))
        assert (h.taking_part, h.entries, h.outside) == (0, 0, 0) and h.dims == (1, 1, 1)
        assert _same(pkg.mesh.raycast(h, _t(o, dev), _t(d, dev)), R.cast(v, f, o, d))
        assert not pkg.mesh.raycast(h, _t(o, dev), _t(d, dev), any_hit=True).any()
    h = pkg.mesh.build_raycast(_mesh(pkg, dev, *TRIANGLE))
    none = torch.zeros(0, 3, device=dev)
    got = pkg.mesh.raycast(h, none, none)
    assert [tuple(g.shape) for g in got] == [(0,), (0, 2), (0,), (0,)] and tuple(pkg.mesh.raycast(h, none, none, any_hit=True).shape) == (0,)
    with pytest.raises(ValueError, match="NaN"):
        pkg.mesh.raycast(h, none, none, tmin=float("nan"))


# ---- (2) the grid never changes an output ----

@pytest.mark.parametrize("name", ["blobs", "random", "bad_input"])
def test_grid_independence(pkg, dev, name):
    v, f = MESHES[name]()
    m = _mesh(pkg, dev, v, f)
    o, d, _ = _cpu_rays(name)
    o, d = o[::2], d[::2]
    want = tuple(a[::2] for a in _want(name))
    to, td = _t(o, dev), _t(d, dev)
    default = pkg.mesh.raycast_grid(m.verts, m.faces)
    lo, hi = _box(v)
    used = v[np.unique(f[((f >= 0) & (f < len(v))).all(1)])]
    mid = np.median(used[np.isfinite(used).all(1), 0])
    grids = {"default": None, "one cell": (lo, 1.0, (1, 1, 1)), "flat": (lo - F32(0.5), 5.0, (37, 1, 5)), "tiny cells": (lo + F32(2.0), 0.2, (64, 64, 64)),
             "regular": (lo - F32(0.01), 1.4, (17, 17, 17)), "shifted": (np.array([mid, lo[1] - 0.01, lo[2] - 0.01], F32), 1.4, (17, 17, 17))}
    ref = R.raycast_grid(v, f)
    assert np.array_equal(default[0], ref[0]) and default[1] == ref[1] and tuple(default[2]) == tuple(ref[2])
    first = None
    for gname, grid in grids.items():
        h = pkg.mesh.build_raycast(m, grid)
        counts = R.grid_counts(v, f, h.lo, h.cell, h.dims)
        print(f"{name} / {gname}: dims {h.dims} cell {float(h.cell):.4g}: takes part {h.taking_part} E {h.entries} OUTSIDE {h.outside}")
        assert [h.taking_part, h.entries, h.outside] == counts, gname
        got = pkg.mesh.raycast(h, to, td)
        assert _same(got, want), gname
        if first is None:
            first = got
        assert all(np.array_equal(_bytes(a), _bytes(b)) for a, b in zip(got, first)), gname
        assert np.array_equal(pkg.mesh.raycast(h, to, td, any_hit=True).cpu().numpy(), (want[2] >= 0).astype(np.uint8)), gname
        if gname == "one cell":
            assert h.entries == 0 and h.outside == h.taking_part  # brute force through the same kernel
        if gname == "shifted":
            assert 0.2 * h.taking_part < h.outside < 0.9 * h.taking_part
        if gname in ("regular", "tiny cells") and name != "bad_input":
            assert h.entries > h.taking_part - h.outside > 0


@pytest.mark.parametrize("dims", [(23, 1, 89), (16, 8, 16), (3, 683, 1)])
def test_grids_at_the_scan_edges(pkg, dev, dims):
    """Grids of 2047, 2048 and 2049 cells -- one workgroup of the cell scan less one, exactly one, one more -- under the random mesh
    stretched to fill the grid, and one triangle beside it: entries from the first cell to the last, one face OUTSIDE."""
    assert int(np.prod(dims)) in (2047, 2048, 2049)
    v, f = MESHES["random"]()
    lo, hi = _box(v)
    v = ((v - lo) / (hi - lo) * (np.asarray(dims, F32) - F32(0.04)) + F32(0.02)).astype(F32)
    v, f = np.concatenate((v, np.array([[-3, -3, -3], [-2, -3, -3], [-3, -2, -3]], F32))), np.concatenate((f, [[len(v), len(v) + 1, len(v) + 2]])).astype(np.int32)
    m = _mesh(pkg, dev, v, f)
    h = pkg.mesh.build_raycast(m, (np.zeros(3, F32), 1.0, dims))
    counts = R.grid_counts(v, f, h.lo, h.cell, h.dims)
    assert tuple(h.dims) == dims and [h.taking_part, h.entries, h.outside] == counts and h.outside == 1 and h.entries > h.taking_part
    part, inside, b0, b1 = R.grid_boxes(v, f, h.lo, h.cell, h.dims)
    cell_of = lambda b: int(((b[0] * dims[1] + b[1]) * dims[2] + b[2]))
    firsts, lasts = [cell_of(b) for b in b0[inside]], [cell_of(b) for b in b1[inside]]
    assert min(firsts) == 0 and max(lasts) == int(np.prod(dims)) - 1  # the first and the last cell hold entries
    o, d = R.random_rays(v, 200, 5)
    want = R.cast(v, f, o, d)
    assert _same(pkg.mesh.raycast(h, _t(o, dev), _t(d, dev)), want) and (want[2] >= 0).sum() > 20
    assert np.array_equal(pkg.mesh.raycast(h, _t(o, dev), _t(d, dev), any_hit=True).cpu().numpy(), (want[2] >= 0).astype(np.uint8))


# ---- (3) visibility and face selection ----

def test_visibility_on_nested_balls(pkg, dev):
    v, f, inner = R.nested_blobs()
    m = _mesh(pkg, dev, v, f)
    H, W = 48, 48
    poses, K = _cameras(v, 4), k_inv(H, W, 0.035)
    cams = [R.camera_q(p, K) for p in poses]
    want_seen, want_counts, want_valid = R.visibility(v, f, cams, H, W)
    for c, (Q, cam) in enumerate(cams):
        Qp, camp = pkg.mesh.camera_q(poses[c], K)
        assert np.array_equal(Q, Qp) and np.array_equal(cam, camp)
        orig, dirs, valid = pkg.ops.mesh_face_rays(m.verts, m.faces, cam.tolist(), Q.reshape(-1).tolist(), H, W)
        wo, wd, wv = R.face_rays(v, f, cam, Q, H, W)
        assert valid.dtype == torch.uint8 and np.array_equal(valid.cpu().numpy(), wv) and np.array_equal(wv, want_valid[c])
        assert np.array_equal(_bytes(orig), _bytes(wo)) and np.array_equal(_bytes(dirs), _bytes(wd))
    seen, counts = pkg.mesh.visibility(m, _t(poses, dev), torch.from_numpy(K), H, W)
    print(f"nested: F {len(f)} ({int(inner.sum())} inner), valid per camera {want_valid.sum(1).tolist()}, seen per camera {want_counts}, "
          f"seen {int(want_seen.sum())}, outer faces seen {int(want_seen[~inner].sum())} of {int((~inner).sum())}")
    assert seen.dtype == torch.bool and np.array_equal(seen.cpu().numpy(), want_seen) and counts == want_counts
    assert inner.sum() > 300 and not want_seen[inner].any()  # every face of the inner copy is hidden
    assert want_seen[~inner].sum() > 0.5 * (~inner).sum() and want_valid[:, inner].any() and min(want_counts) > 100
    # a smaller tmin and a window that excludes everything
    s2, c2 = pkg.mesh.visibility(m, _t(poses[:2], dev), torch.from_numpy(K), H, W, tmin=1e-2)
    w2 = R.visibility(v, f, cams[:2], H, W, tmin=1e-2)
    assert np.array_equal(s2.cpu().numpy(), w2[0]) and c2 == w2[1]


def test_filter_faces(pkg, dev):
    v, f, n = M.bad_input()[:3]  # (faces with indices -1, V and 2^31 - 1 among them)
    rng = np.random.default_rng(6)
    rgb = rng.random((len(v), 3), dtype=F32)
    bad = ~((f >= 0) & (f < len(v))).all(1)
    for keep in ((rng.random(len(f)) < 0.4) | bad, np.ones(len(f), bool), np.zeros(len(f), bool), bad):
        for nn, cc in ((n, rgb), (None, None), (n, None)):
            got = pkg.mesh.filter_faces(_mesh(pkg, dev, v, f, nn, cc), _t(keep, dev))
            want = R.select_faces(v, f, keep, nn, cc)
            for g, w in zip(got, want):
                assert (g is None) == (w is None)
                if w is not None:
                    assert tuple(g.shape) == tuple(w.shape) and np.array_equal(_bytes(g), _bytes(w))
    assert bad.sum() == 60 and len(R.select_faces(v, f, bad)[1]) == 0 and len(R.select_faces(v, f, np.ones(len(f), bool))[1]) == len(f) - 60
    v2, f2, inner = R.nested_blobs()
    got = pkg.mesh.filter_faces(_mesh(pkg, dev, v2, f2), _t(~inner, dev))
    assert np.array_equal(_bytes(got.verts), _bytes(M.blobs()[0])) and np.array_equal(got.faces.cpu().numpy(), M.blobs()[1])
    e = pkg.mesh.filter_faces(_mesh(pkg, dev, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), torch.zeros(0, dtype=torch.bool, device=dev))
    assert tuple(e.verts.shape) == (0, 3) and tuple(e.faces.shape) == (0, 3)
    with pytest.raises(ValueError, match="one entry per face"):
        pkg.mesh.filter_faces(_mesh(pkg, dev, v, f), torch.ones(5, device=dev))


# ---- (4) determinism ----

def test_two_runs_give_identical_bytes(pkg, dev):
    v, f, inner = R.nested_blobs()
    m = _mesh(pkg, dev, v, f)
    o, d, _ = _cpu_rays("blobs")
    poses, K = _cameras(v, 3), k_inv(32, 32, 0.05)
    runs = []
    for _ in range(2):
        h = pkg.mesh.build_raycast(m)
        t, uv, face, side = pkg.mesh.raycast(h, _t(o, dev), _t(d, dev))
        seen, counts = pkg.mesh.visibility(m, _t(poses, dev), torch.from_numpy(K), 32, 32)
        kept = pkg.mesh.filter_faces(m, seen)
        runs.append((t.view(torch.int64), uv.view(torch.int64), face, side, seen, counts, kept.verts.view(torch.int32), kept.faces,
                     (h.entries, h.outside, h.dims)))
    for x, y in zip(*runs):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


# ---- (5) guard regions behind every output and the workspace ----

GUARD = 4096


def test_outputs_stay_inside_their_capacities(pkg, dev):
    v, f = MESHES["bad_input"]()
    m = _mesh(pkg, dev, v, f)
    o, d, _ = _cpu_rays("bad_input")
    o, d = o[::3], d[::3]
    want = tuple(a[::3] for a in _want("bad_input"))
    N, V, F = len(o), len(v), len(f)
    to, td = _t(o, dev), _t(d, dev)
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    lo, cell, dims = (np.asarray([0.0, 0.0, 0.0], F32), 1.25, (13, 13, 13))
    lo3, dims3 = pkg._abi.f32_array(lo.tolist()), pkg._abi.i32_array(dims)
    counts = torch.full((3 + 8,), -5, dtype=torch.int64, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_raycast_grid_count(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, cell, dims3, counts.data_ptr(), st))
    assert counts[:3].tolist() == R.grid_counts(v, f, lo, cell, dims) and (counts[3:] == -5).all()
    E = int(counts[1])
    nws = pkg._abi.mesh_raycast_ws_bytes(F, E, dims)
    ws = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_raycast_grid_fill(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, cell, dims3, E, ws.data_ptr(), nws, st))
    for cap in (N, N // 2, 0, N - 1, N + 100):
        k = min(cap, N)
        t = torch.full((cap + GUARD,), 7.25, dtype=torch.float64, device=dev)
        uv = torch.full((cap + GUARD, 2), 7.25, dtype=torch.float64, device=dev)
        face = torch.full((cap + GUARD,), -9, dtype=torch.int32, device=dev)
        side = torch.full((cap + GUARD,), 77, dtype=torch.int8, device=dev)
        occ = torch.full((cap + GUARD,), 99, dtype=torch.uint8, device=dev)
        for any_hit in (0, 1):
            pkg._abi.check(L.nerf_hip_mesh_raycast(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, cell, dims3, E, ws.data_ptr(), nws, to.data_ptr(),
                                                   td.data_ptr(), None, N, 0.0, float("inf"), any_hit, t.data_ptr(), uv.data_ptr(), face.data_ptr(),
                                                   side.data_ptr(), occ.data_ptr(), cap, st))
        torch.cuda.synchronize()
        assert (t[k:] == 7.25).all() and (uv[k:] == 7.25).all() and (face[k:] == -9).all() and (side[k:] == 77).all() and (occ[k:] == 99).all()
        assert _same((t[:k], uv[:k], face[:k], side[:k]), tuple(a[:k] for a in want))
        assert np.array_equal(occ[:k].cpu().numpy(), (want[2][:k] >= 0).astype(np.uint8))
    assert (ws[nws:] == 0x5A).all()
    # the shadow rays and the selection
    Q, cam = R.camera_q(_cameras(v, 1)[0], k_inv(32, 32, 0.05))
    wo, wd, wv = R.face_rays(v, f, cam, Q, 32, 32)
    import ctypes

    q9 = (ctypes.c_double * 9)(*Q.reshape(-1).tolist())
    for cap in (F, F // 3, 0):
        orig = torch.full((cap + GUARD, 3), 7.25, device=dev)
        dirs = torch.full((cap + GUARD, 3), 7.25, device=dev)
        valid = torch.full((cap + GUARD,), 99, dtype=torch.uint8, device=dev)
        pkg._abi.check(L.nerf_hip_mesh_face_rays(m.verts.data_ptr(), m.faces.data_ptr(), V, F, pkg._abi.f32_array(cam.tolist()), q9, 32, 32,
                                                 orig.data_ptr(), dirs.data_ptr(), valid.data_ptr(), cap, st))
        torch.cuda.synchronize()
        assert (orig[cap:] == 7.25).all() and (dirs[cap:] == 7.25).all() and (valid[cap:] == 99).all()
        assert np.array_equal(_bytes(orig[:cap]), _bytes(wo[:cap])) and np.array_equal(_bytes(dirs[:cap]), _bytes(wd[:cap]))
        assert np.array_equal(valid[:cap].cpu().numpy(), wv[:cap])
    keep = np.random.default_rng(8).random(F) < 0.5
    wv2, wf2, _, _ = R.select_faces(v, f, keep)
    tk = _t(keep.astype(np.uint8), dev)
    nsel = pkg._abi.mesh_select_faces_ws_bytes(V, F)
    ws2 = torch.full((nsel + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    c2 = torch.full((2 + 8,), -5, dtype=torch.int64, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_select_faces_count(m.faces.data_ptr(), V, F, tk.data_ptr(), ws2.data_ptr(), nsel, c2.data_ptr(), st))
    assert c2[:2].tolist() == [len(wv2), len(wf2)] and (c2[2:] == -5).all()
    for mv, mf in ((len(wv2), len(wf2)), (len(wv2) // 2, len(wf2) // 3), (0, 0)):
        ov = torch.full((mv + GUARD, 3), 7.25, device=dev)
        of = torch.full((mf + GUARD, 3), -9, dtype=torch.int32, device=dev)
        pkg._abi.check(L.nerf_hip_mesh_select_faces_emit(m.verts.data_ptr(), None, None, m.faces.data_ptr(), V, F, tk.data_ptr(), ws2.data_ptr(), nsel,
                                                         ov.data_ptr(), None, None, of.data_ptr(), mv, mf, st))
        torch.cuda.synchronize()
        assert (ov[mv:] == 7.25).all() and (of[mf:] == -9).all() and (ws2[nsel:] == 0x5A).all()
        assert np.array_equal(_bytes(ov[:mv]), _bytes(wv2[:mv])) and np.array_equal(of[:mf].cpu().numpy(), wf2[:mf])
    assert np.array_equal(_bytes(m.verts), _bytes(v)) and np.array_equal(m.faces.cpu().numpy(), f)  # the inputs are unchanged


# ---- (6) refusals on the host: nothing is enqueued ----

def test_host_refusals_enqueue_nothing(pkg, dev):
    import ctypes

    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F, N, E = 64, 32, 48, 100
    dims = (3, 2, 2)
    verts = torch.zeros(V, 3, device=dev)
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    rays = torch.zeros(N, 3, device=dev)
    keep = torch.ones(F, dtype=torch.uint8, device=dev)
    need, need_s = pkg._abi.mesh_raycast_ws_bytes(F, E, dims), pkg._abi.mesh_select_faces_ws_bytes(V, F)
    ws = torch.full((max(need, need_s),), 0x5A, dtype=torch.uint8, device=dev)
    out8 = torch.full((16,), -5, dtype=torch.int64, device=dev)
    ot = torch.full((N,), 2.5, dtype=torch.float64, device=dev)
    ouv = torch.full((N, 2), 2.5, dtype=torch.float64, device=dev)
    oface = torch.full((N,), -9, dtype=torch.int32, device=dev)
    oside = torch.full((N,), 77, dtype=torch.int8, device=dev)
    oocc = torch.full((N,), 99, dtype=torch.uint8, device=dev)
    ov = torch.full((V, 3), 2.5, device=dev)
    of = torch.full((F, 3), -9, dtype=torch.int32, device=dev)
    f3, i3 = pkg._abi.f32_array, pkg._abi.i32_array
    q9 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    nan, inf = float("nan"), float("inf")

    def count(v=V, f=F, lo=(0, 0, 0), cell=0.5, d=dims, vp=verts.data_ptr(), fp=faces.data_ptr(), cp=out8.data_ptr()):
        return L.nerf_hip_mesh_raycast_grid_count(vp, fp, v, f, f3(lo), cell, i3(d), cp, st)

    def fill(v=V, f=F, lo=(0, 0, 0), cell=0.5, d=dims, e=E, vp=verts.data_ptr(), fp=faces.data_ptr(), w=ws.data_ptr(), nbytes=need):
        return L.nerf_hip_mesh_raycast_grid_fill(vp, fp, v, f, f3(lo), cell, i3(d), e, w, nbytes, st)

    def cast(v=V, f=F, lo=(0, 0, 0), cell=0.5, d=dims, e=E, vp=verts.data_ptr(), fp=faces.data_ptr(), w=ws.data_ptr(), nbytes=need, n=N,
             op=rays.data_ptr(), dp=rays.data_ptr(), tmin=0.0, tmax=inf, any_hit=0, tp=ot.data_ptr(), up=ouv.data_ptr(), ip=oface.data_ptr(),
             sp=oside.data_ptr(), cp=oocc.data_ptr(), cap=N):
        return L.nerf_hip_mesh_raycast(vp, fp, v, f, f3(lo), cell, i3(d), e, w, nbytes, op, dp, None, n, tmin, tmax, any_hit, tp, up, ip, sp, cp, cap, st)

    def frays(v=V, f=F, cam=(0, 0, 0), q=q9, H=8, W=8, vp=verts.data_ptr(), fp=faces.data_ptr(), op=ov.data_ptr(), dp=ov.data_ptr(),
              mp=oocc.data_ptr(), cap=F):
        return L.nerf_hip_mesh_face_rays(vp, fp, v, f, f3(cam), q, H, W, op, dp, mp, cap, st)

    def scount(v=V, f=F, fp=faces.data_ptr(), kp=keep.data_ptr(), w=ws.data_ptr(), nbytes=need_s, cp=out8.data_ptr()):
        return L.nerf_hip_mesh_select_faces_count(fp, v, f, kp, w, nbytes, cp, st)

    def semit(v=V, f=F, vp=verts.data_ptr(), fp=faces.data_ptr(), kp=keep.data_ptr(), w=ws.data_ptr(), nbytes=need_s, ovp=ov.data_ptr(),
              ofp=of.data_ptr(), mv=V, mf=F):
        return L.nerf_hip_mesh_select_faces_emit(vp, None, None, fp, v, f, kp, w, nbytes, ovp, None, None, ofp, mv, mf, st)

    for call in (count, fill, cast, frays):
        assert call(v=-1) == -1 and call(f=1 << 31) == -1 and call(vp=None) == -1 and call(fp=None) == -1
    for call in (count, fill, cast):
        assert call(lo=(0, nan, 0)) == -1 and call(lo=(inf, 0, 0)) == -1
        for cell in (0.0, -0.5, nan, inf):
            assert call(cell=cell) == -1
        assert call(d=(0, 1, 1)) == -1 and call(d=(1, -2, 1)) == -1 and call(d=(2048, 2048, 512)) == -1
    assert count(cp=None) == -1 and count(cp=out8.data_ptr() + 4) == -1
    for call, nb in ((fill, need), (cast, need), (scount, need_s), (semit, need_s)):
        assert call(w=None) == -1 and call(w=ws.data_ptr() + 4) == -1 and call(nbytes=nb - 1) == -2  # one byte short
    for call in (fill, cast):
        assert call(e=-1) == -1 and call(e=1 << 31) == -1
    assert cast(n=-1) == -1 and cast(n=1 << 31) == -1 and cast(cap=-1) == -1 and cast(op=None) == -1 and cast(dp=None) == -1
    assert cast(tmin=nan) == -1 and cast(tmax=nan) == -1 and cast(tp=None) == -1 and cast(up=None) == -1 and cast(ip=None) == -1 and cast(sp=None) == -1
    assert cast(tp=ot.data_ptr() + 4) == -1 and cast(any_hit=1, cp=None) == -1
    assert frays(cam=(0, nan, 0)) == -1 and frays(q=(ctypes.c_double * 9)(1, 0, 0, 0, inf, 0, 0, 0, 1)) == -1 and frays(q=None) == -1
    assert frays(H=0) == -1 and frays(W=-1) == -1 and frays(cap=-1) == -1 and frays(op=None) == -1 and frays(mp=None) == -1
    for call in (scount, semit):
        assert call(v=-1) == -1 and call(f=1 << 31) == -1 and call(fp=None) == -1 and call(kp=None) == -1
    assert scount(cp=None) == -1 and scount(cp=out8.data_ptr() + 4) == -1
    assert semit(vp=None) == -1 and semit(mv=-1) == -1 and semit(mf=-1) == -1 and semit(ovp=None) == -1 and semit(ofp=None) == -1
    torch.cuda.synchronize()
    untouched = lambda: ((out8 == -5).all() and (ws == 0x5A).all() and (ot == 2.5).all() and (ouv == 2.5).all() and (oface == -9).all()
                         and (oside == 77).all() and (oocc == 99).all() and (ov == 2.5).all() and (of == -9).all())
    assert untouched()
    # and the good calls go through: every face is the point 0 three times -- it takes part, is INSIDE one cell and is never hit
    assert count() == 0 and fill() == 0 and cast() == 0 and cast(any_hit=1) == 0
    torch.cuda.synchronize()
    assert out8[:3].tolist() == [F, F, 0] and (out8[3:] == -5).all()
    assert torch.isinf(ot).all() and not ouv.any() and (oface == -1).all() and (oside == 0).all() and (oocc == 0).all()
    assert scount() == 0 and semit() == 0 and frays() == 0
    torch.cuda.synchronize()
    assert out8[:2].tolist() == [1, F] and not ov[:F].any() and (ov[F:] == 2.5).all() and not of.any() and (oocc == 0).all()


# ---- (7) inside extract_mesh ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


LO, HI, RES = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), 24


def test_extract_mesh_visible(pkg, dev, model):
    level = float(model.density_grid(LO, HI, RES).median())
    kw = dict(normals="grid", color=True, min_faces=8)
    base = model.extract_mesh(LO, HI, RES, level, **kw)
    again = model.extract_mesh(LO, HI, RES, level, **kw)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base, again))  # unchanged without the argument
    H, W = 32, 32
    c = (np.asarray(LO) + np.asarray(HI)) / 2
    poses = np.stack([look_at(c + 4.0 * np.asarray(d) / np.linalg.norm(d), c) for d in ([1, 0.2, 0.3], [-0.6, 1, 0.1], [0.1, -0.7, 1])])
    K = torch.from_numpy(k_inv(H, W, 0.03))
    tp = _t(poses, dev)
    got = model.extract_mesh(LO, HI, RES, level, visible=(tp, K, H, W), **kw)
    # by hand: the same mesh before normals and colours, its visibility, the faces kept, then the colours at the kept vertices
    plain = model.extract_mesh(LO, HI, RES, level, normals="grid", color=False, min_faces=8)
    seen, counts = pkg.mesh.visibility(plain, tp, K, H, W)
    kept = pkg.mesh.filter_faces(plain, seen)
    rgb = model.query(kept.verts, -kept.normals)[0]
    print(f"extract_mesh(visible=): {int(seen.sum())} of {len(seen)} faces seen (per camera {counts}), V {len(plain.verts)} -> {len(kept.verts)}")
    assert 0 < int(seen.sum()) < len(seen) and len(kept.faces) == int(seen.sum()) and torch.equal(model.last_visibility[0], seen)
    for a, b in zip(got, (kept.verts, kept.faces, kept.normals, rgb)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # with the later stages: they see the filtered mesh
    sm = model.extract_mesh(LO, HI, RES, level, visible=(tp, K, H, W), smooth=2, simplify=2, normals="grid", color=False, min_faces=8)
    by_hand, _ = pkg.mesh.smooth(pkg.mesh.Mesh(kept.verts, kept.faces, None, None), 2, lo=np.asarray(LO, F32),
                                 scale=pkg.nerf.smooth_scale_of_grid(np.asarray(LO, F32), np.asarray(HI, F32)))
    assert len(sm.faces) < len(kept.faces) and len(by_hand.verts) == len(kept.verts)


def test_runner_visible_from(pkg, dev, tmp_path, capsys):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    level = float(np.median(run.density_grid(24, save=False)))
    plain = run.extract_mesh(24, level, save=True)
    files = glob.glob(rs + "*_mesh24.ply")
    assert len(files) == 1 and "[VISIBLE]" not in capsys.readouterr().out
    before = open(files[0], "rb").read()
    got = run.extract_mesh(24, level, save=True, visible_from="train")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH]") and "[VISIBLE]" in ln]
    assert len(line) == 1 and glob.glob(rs + "*_mesh24.ply") == files  # the same file name
    seen, per_cam = run.model.last_visibility
    assert f"{int(seen.sum())} / {len(plain.faces)} faces seen from the 3 train cameras" in line[0] and len(per_cam) == 3
    assert len(got.faces) == int(seen.sum()) <= len(plain.faces)
    m = pkg.mesh.Mesh(torch.from_numpy(plain.verts).to(dev), torch.from_numpy(plain.faces).to(dev), None, None)
    want, _ = pkg.mesh.visibility(m, run.train_rays.poses, run.K_inv, 24, 24)
    assert torch.equal(want, seen)
    again = run.extract_mesh(24, level, save=True)
    assert open(files[0], "rb").read() == before and np.array_equal(again.faces, plain.faces)
    with pytest.raises(ValueError, match="visible_from"):
        run.extract_mesh(24, level, save=False, visible_from="all")
