"""GPU: texture atlases on the device (nerf_hip_mesh_atlas_texels / nerf_hip_mesh_texture_sample; mesh.atlas_texels / bake_texture /
sample_texture / render_texture / write_obj; NeRFModel.bake_texture / extract_mesh(texture=) / extract_mesh_tsdf(texture=);
NeRFRunner.extract_mesh(texture=)) against the numpy restatement of rules TA and TX in tests/texture_reference.py.  Points,
directions, images and colours are compared as bits."""
import ctypes
import glob

import numpy as np
import pytest
import torch

import texture_reference as R
import tsdf_color_reference as RC
import tsdf_reference as RT

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: some inputs are read-only)


def _same(got, want):
    """a device tensor and a numpy array of the same dtype, bit for bit"""
    want = np.ascontiguousarray(want)
    g = got.cpu().contiguous().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes()


def _u8(t):
    return t.to(torch.uint8) if t.dtype == torch.bool else t


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _mesh(pkg, dev, verts, normals, faces, rgb=None):
    return pkg.mesh.Mesh(_t(verts, dev), _t(faces, dev), _t(normals, dev), rgb)


# ---- (1) rule TA bit for bit: one partial workgroup, and many ----

@pytest.mark.parametrize("F,n,size", [(5, 2, 14), (200, 8, 130)])
def test_atlas_texels_bit_identical(pkg, dev, F, n, size):
    verts, normals, faces = R.random_mesh(F, 40, seed=F)
    assert R.dims(F, n)[3:] == (size, size)
    want = R.texels(verts, normals, faces, n)
    m = _mesh(pkg, dev, verts, normals, faces)
    got = pkg.mesh.atlas_texels(m, n)
    assert got[2].dtype == torch.bool and all(_same(_u8(g), w) for g, w in zip(got, want))
    owner, wts, _ = R.owner(F, n)
    lost = (owner >= 0) & (want[2] == 0)  # owned texels of the face with an index out of range
    print(f"F={F} n={n}: {int(want[2].sum())} of {size * size} texels with a face, {int((owner < 0).sum())} unowned, {int(lost.sum())} of bad faces, "
          f"{int(np.isnan(want[0]).any(-1).sum())} points with NaN, {int(((want[2] == 1) & ~want[1].any(-1)).sum())} owned without a direction")
    assert bool((owner < 0).any()) == (F == 5) and lost.any() and np.isnan(want[0]).any() and ((want[2] == 1) & ~want[1].any(-1)).any()
    assert not want[0][want[2] == 0].any() and not want[1][want[2] == 0].any()
    # a band is the slice of the whole; a second run gives the same bytes
    for row0, rows in [(0, 1), (3, 5), (size - 2, 2), (size, 0), (4, 0)]:
        band = pkg.mesh.atlas_texels(m, n, row0, rows)
        assert all(tuple(b.shape)[:2] == (rows, size) and _same(_u8(b), w[row0:row0 + rows]) for b, w in zip(band, want))
    again = pkg.mesh.atlas_texels(m, n)
    assert all(_same(_u8(a), w) for a, w in zip(again, want))
    with pytest.raises(ValueError):
        pkg.mesh.atlas_texels(m, n, size - 1, 2)
    with pytest.raises(ValueError):
        pkg.mesh.atlas_texels(m._replace(normals=None), n)


def test_empty_mesh(pkg, dev):
    m = pkg.mesh.Mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), torch.zeros(0, 3, device=dev), None)
    p, d, k = pkg.mesh.atlas_texels(m, 4)
    assert tuple(p.shape) == (0, 0, 3) and tuple(d.shape) == (0, 0, 3) and tuple(k.shape) == (0, 0)
    tex = pkg.mesh.bake_texture(m, 4, lambda p, d: p)
    assert tuple(tex.image.shape) == (0, 0, 3) and tex.faces == 0 and tuple(tex.uv.shape) == (0, 3, 2)
    rgb, valid = pkg.mesh.sample_texture(tex, _t(np.array([0, -1], np.int32), dev), torch.zeros(2, 2, dtype=torch.float64, device=dev), (1.0, 2.0, 3.0))
    assert not valid.any() and rgb.tolist() == [[1.0, 2.0, 3.0]] * 2
    # faces over no vertices: every index is out of range
    m = pkg.mesh.Mesh(torch.zeros(0, 3, device=dev), torch.zeros(3, 3, dtype=torch.int32, device=dev), torch.zeros(0, 3, device=dev), None)
    p, d, k = pkg.mesh.atlas_texels(m, 2)
    assert tuple(k.shape) == (7, 14) and not k.any() and not p.any() and not d.any()


# ---- (2) rule TX bit for bit ----

@pytest.mark.parametrize("F,n", [(5, 2), (200, 8), (51, 3)])
def test_sample_texture_bit_identical(pkg, dev, F, n):
    c, Sx, Sy, W, H = R.dims(F, n)
    rng = np.random.default_rng(F * 31 + n)
    image = rng.uniform(-1.0, 2.0, (H, W, 3)).astype(F32)
    bary = R.barycentrics(300, seed=n)
    outside = rng.uniform(-0.5, 1.5, (40, 2))  # clamped into the triangle
    bad_uv = np.array([[np.nan, 0.2], [0.2, np.inf], [-np.inf, np.nan]])
    uv = np.concatenate((bary, outside, bad_uv, bary[:4]))
    face = rng.integers(0, F, len(uv)).astype(np.int32)
    face[:9] = np.arange(9) % F
    face[-4:] = (-1, F, F + 7, -2 ** 31)
    face[9:13] = F - 1  # the last face: a lower one of an odd F
    bg = (0.25, -1.0, 7.5)
    want = R.sample(image, F, n, face, uv, bg)
    tex = pkg.mesh.Texture(_t(image, dev), None, n, F, None)
    rgb, valid = pkg.mesh.sample_texture(tex, _t(face, dev), _t(uv, dev), bg)
    assert valid.dtype == torch.bool and _same(rgb, want[0]) and _same(valid.to(torch.uint8), want[1])
    assert want[1].sum() == len(uv) - 7 and (want[0][want[1] == 0] == np.asarray(bg, F32)).all()
    # at a corner the lookup is the corner texel
    for f in sorted({0, 1 % F, F - 1}):
        got, ok = pkg.mesh.sample_texture(tex, _t(np.full(3, f, np.int32), dev), _t(np.array([[0, 0], [1, 0], [0, 1]], np.float64), dev))
        px = np.rint(R.uv_table(F, n)[f].astype(np.float64) * (W, H) - 0.5).astype(int)
        assert bool(ok.all()) and _same(got, image[px[:, 1], px[:, 0]])
    none = pkg.mesh.sample_texture(tex, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 2, dtype=torch.float64, device=dev))
    assert tuple(none[0].shape) == (0, 3) and tuple(none[1].shape) == (0,)
    again = pkg.mesh.sample_texture(tex, _t(face, dev), _t(uv, dev), bg)
    assert _eq(again[0], rgb) and torch.equal(again[1], valid)
    with pytest.raises(ValueError):
        pkg.mesh.sample_texture(tex._replace(faces=F + 2 * Sx), _t(face, dev), _t(uv, dev))  # an image of another atlas


def test_uv_table_on_the_device(pkg, dev):
    for F, n in [(5, 2), (200, 8)]:
        assert _same(pkg.mesh.atlas_uv(F, n, dev), R.uv_table(F, n))


# ---- (3) the textured mesh seen from a camera ----

def test_render_texture_on_a_tetrahedron(pkg, dev):
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    normals = (verts / np.sqrt(F32(3))).astype(F32)
    m = _mesh(pkg, dev, verts, normals, faces)
    F, n = 4, 3
    c, Sx, Sy, W, H = R.dims(F, n)
    image = np.random.default_rng(8).random((H, W, 3)).astype(F32)
    tex = pkg.mesh.Texture(_t(image, dev), None, n, F, pkg.mesh.atlas_uv(F, n, dev))
    h = pkg.mesh.build_raycast(m)
    pose = _t(RT.look_at((3.0, 0.4, 0.8), (0.0, 0.0, 0.0))[None], dev)
    K = torch.from_numpy(RT.k_inv(8, 12, 0.12))
    bg = (0.5, 0.25, 0.125)
    rgb, hit = pkg.mesh.render_texture(h, tex, pose, K, 8, 12, bg)
    t, face, uv = pkg.mesh.render_depth(h, pose, K, 8, 12)
    want, ok = pkg.mesh.sample_texture(tex, face.reshape(-1), uv.reshape(-1, 2), bg)
    assert tuple(rgb.shape) == (1, 8, 12, 3) and tuple(hit.shape) == (1, 8, 12) and hit.dtype == torch.bool
    assert _eq(rgb.reshape(-1, 3), want) and torch.equal(hit.reshape(-1), ok) and torch.equal(hit, face >= 0) and torch.equal(hit, torch.isfinite(t))
    print(f"tetrahedron: {int(hit.sum())} of 96 pixels hit, faces {sorted(set(face[hit].tolist()))}")
    assert 0 < int(hit.sum()) < 96 and len(set(face[hit].tolist())) >= 2
    assert (rgb[~hit] == torch.tensor(bg, device=dev)).all()
    ref = R.sample(image, F, n, face.cpu().numpy().reshape(-1), uv.cpu().numpy().reshape(-1, 2), bg)
    assert _same(rgb.reshape(-1, 3), ref[0])


# ---- (4) baking with a model ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


LO, HI, SHAPE = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), (9, 7, 11)


@pytest.fixture(scope="module")
def baked(pkg, dev, model):
    """(level, the mesh of extract_mesh, chart, the restatement's texels, the whole-atlas bake)"""
    level = float(model.density_grid(LO, HI, SHAPE).median())
    m = model.extract_mesh(LO, HI, SHAPE, level)
    n = 3
    want = R.texels(m.verts.cpu().numpy(), m.normals.cpu().numpy(), m.faces.cpu().numpy(), n)
    tex = model.bake_texture(m, n, rows_per_call=R.dims(len(m.faces), n)[4])
    return level, m, n, want, tex


def test_bake_texture_is_the_field_at_the_texels(pkg, dev, model, baked):
    level, m, n, (P, D, M), tex = baked
    F = len(m.faces)
    c, Sx, Sy, W, H = R.dims(F, n)
    print(f"bake: V {len(m.verts)} F {F}, atlas {W} x {H}, chart {n}, {int(M.sum())} owned texels")
    assert F > 8 and tex.chart == n and tex.faces == F and tuple(tex.image.shape) == (H, W, 3) and tex.image.dtype == torch.float32
    assert _same(tex.mask.to(torch.uint8), M) and _same(tex.uv, R.uv_table(F, n))
    field = model.query(_t(P.reshape(-1, 3), dev), _t(D.reshape(-1, 3), dev))[0].view(H, W, 3)
    assert _eq(tex.image, torch.where(tex.mask[..., None], field, torch.zeros_like(field)))
    assert not tex.image[~tex.mask].any() and bool((~tex.mask).any())
    for per in (1, 3, None):
        other = model.bake_texture(m, n, rows_per_call=per)
        assert _eq(other.image, tex.image) and torch.equal(other.mask, tex.mask) and _eq(other.uv, tex.uv)
    with pytest.raises(ValueError):
        model.bake_texture(m, n, rows_per_call=0)


def test_corner_texels_are_the_vertex_colours(pkg, dev, model, baked):
    level, m, n, _, tex = baked
    F = len(m.faces)
    c, Sx, Sy, W, H = R.dims(F, n)
    px = np.rint(R.uv_table(F, n).astype(np.float64) * (W, H) - 0.5).astype(np.int64)  # [F, 3, (x, y)]
    texel = tex.image[_t(px[..., 1], dev), _t(px[..., 0], dev)]  # [F, 3, 3]
    vert = m.rgb[m.faces.long()]
    differ = int((texel.view(torch.int32) != vert.view(torch.int32)).any(-1).sum())
    print(f"corner texels: {differ} of {3 * F} differ from their vertex colour")
    assert _eq(texel, vert)
    # and a lookup at the corner returns them
    f = torch.arange(F, dtype=torch.int32, device=dev).repeat_interleave(3)
    uv = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], dtype=torch.float64, device=dev).repeat(F, 1)
    got, ok = pkg.mesh.sample_texture(tex, f, uv)
    assert bool(ok.all()) and _eq(got.view(F, 3, 3), vert)


def test_extract_mesh_texture(pkg, dev, model, baked):
    level, m, n, _, tex = baked
    F = len(m.faces)
    S = R.dims(F, n)[1] * (n + 5) + 2  # the largest chart under S is n
    assert pkg.mesh.atlas_chart(F, S) == n
    model.last_texture = None
    got = model.extract_mesh(LO, HI, SHAPE, level, texture=S)
    assert all(_eq(a, b) for a, b in zip(got, m))  # the same four arrays
    lt = model.last_texture
    assert lt.chart == n and lt.faces == F and _eq(lt.image, tex.image) and torch.equal(lt.mask, tex.mask) and _eq(lt.uv, tex.uv)
    plain = model.extract_mesh(LO, HI, SHAPE, level, simplify=2, normals="field")
    simple = model.extract_mesh(LO, HI, SHAPE, level, simplify=2, normals="field", texture=S)
    F2 = len(plain.faces)
    lt = model.last_texture
    print(f"simplify=2: F {F} -> {F2}, chart {n} -> {lt.chart}")
    assert 0 < F2 < F and all(_eq(a, b) for a, b in zip(simple, plain))
    assert lt.faces == F2 and lt.chart == pkg.mesh.atlas_chart(F2, S) and tuple(lt.image.shape[:2]) == R.dims(F2, lt.chart)[:2:-1]
    assert _eq(lt.image, model.bake_texture(plain, lt.chart).image)
    with pytest.raises(ValueError, match="color"):
        model.extract_mesh(LO, HI, SHAPE, level, color=False, texture=S)
    with pytest.raises(ValueError):
        model.extract_mesh(LO, HI, SHAPE, level, texture=8)  # no chart fits


def test_fused_texture_on_the_sphere(pkg, dev, model):
    s = RT.sphere_scene()
    T, Wt = pkg.mesh.tsdf_volume(s["shape"], dev)
    C = pkg.mesh.tsdf_color_volume(s["shape"], dev)
    pkg.mesh.tsdf_integrate(T, Wt, s["lo"], s["step"], _t(s["depth"], dev), np.ascontiguousarray(s["poses"]), np.array(s["K"]), opacity=_t(s["opacity"], dev),
                            trunc=s["trunc"], rgb=_t(RC.sphere_rgb(), dev), color=C)
    lo32, hi32 = np.full(3, -1.0, F32), np.full(3, 1.0, F32)
    assert pkg.nerf.grid_step(lo32, hi32, s["shape"]).tobytes() == s["step"].tobytes()
    v, f, nrm = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt, "solid"), 0.0, lo32, s["step"])
    S = pkg.mesh.atlas_dims(len(f), 2)[3]  # the smallest atlas: chart 2
    plain = model._mesh_stages(v, f, nrm, lo32, hi32, s["shape"], True, "grid", None, None, None, None, None, fused=C)
    got = model._mesh_stages(v, f, nrm, lo32, hi32, s["shape"], True, "grid", None, None, None, None, None, fused=C, texture=S)
    assert all(_eq(a, b) for a, b in zip(got, plain))
    tex = model.last_texture
    n = pkg.mesh.atlas_chart(len(f), S)
    p, d, k = pkg.mesh.atlas_texels(got, n)
    rgb, ok = pkg.mesh.tsdf_sample_color(C, lo32, s["step"], p.view(-1, 3))
    ok = ok.view(k.shape) & k
    print(f"sphere: F {len(f)}, atlas {tuple(tex.image.shape[:2])}, chart {n}, {int(ok.sum())} of {int(k.sum())} owned texels with a fused colour")
    assert tex.chart == n and tex.faces == len(f) and int(ok.sum()) > 0 and torch.equal(tex.mask, k)
    assert _eq(tex.image[ok], rgb.view(*k.shape, 3)[ok])
    rest = k & ~ok  # the field where the volume has no colour
    if bool(rest.any()):
        assert _eq(tex.image[rest], model.query(p[rest], d[rest])[0])


# ---- (5) refusals on the host: nothing is enqueued ----

def test_host_refusals_enqueue_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F, n, N = 16, 5, 2, 8
    c, Sx, Sy, W, H = R.dims(F, n)
    verts = torch.zeros(V, 3, device=dev)
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    points = torch.full((H * W, 3), 2.5, device=dev)
    dirs = torch.full((H * W, 3), 2.5, device=dev)
    mask = torch.full((H * W,), 99, dtype=torch.uint8, device=dev)
    image = torch.zeros(H, W, 3, device=dev)
    face = torch.zeros(N, dtype=torch.int32, device=dev)
    uv = torch.zeros(N + 1, 2, dtype=torch.float64, device=dev)
    rgb = torch.full((N, 3), 2.5, device=dev)
    valid = torch.full((N,), 99, dtype=torch.uint8, device=dev)
    bg3 = pkg._abi.f32_array((0, 0, 0))
    out5 = (ctypes.c_int * 5)(*([-7] * 5))

    def texels(v=V, f=F, n=n, row0=0, rows=H, vp=verts.data_ptr(), np_=verts.data_ptr(), fp=faces.data_ptr(), pp=points.data_ptr(),
               dp=dirs.data_ptr(), mp=mask.data_ptr()):
        return L.nerf_hip_mesh_atlas_texels(vp, np_, fp, v, f, n, row0, rows, pp, dp, mp, st)

    def sample(f=F, n=n, N=N, ip=image.data_ptr(), fp=face.data_ptr(), up=uv.data_ptr(), bp=bg3, rp=rgb.data_ptr(), vp=valid.data_ptr()):
        return L.nerf_hip_mesh_texture_sample(ip, f, n, fp, up, N, bp, rp, vp, st)

    for bad in (dict(n=1), dict(n=0), dict(n=-4), dict(f=-1), dict(f=715_827_883), dict(f=200_000_000), dict(n=2 ** 31 - 6)):
        assert texels(**bad) == -1 and sample(**bad) == -1
        assert L.nerf_hip_mesh_atlas_dims(bad.get("f", F), bad.get("n", n), out5) == -1
    assert L.nerf_hip_mesh_atlas_dims(F, n, None) == -1 and list(out5) == [-7] * 5
    assert texels(v=-1) == -1 and texels(v=1 << 31) == -1 and texels(vp=None) == -1 and texels(np_=None) == -1 and texels(fp=None) == -1
    assert texels(row0=-1) == -1 and texels(rows=-1) == -1 and texels(row0=1) == -1 and texels(row0=H, rows=1) == -1 and texels(rows=H + 1) == -1
    assert texels(row0=2 ** 31 - 1, rows=2 ** 31 - 1) == -1
    assert texels(pp=None) == -1 and texels(dp=None) == -1 and texels(mp=None) == -1
    assert sample(N=-1) == -1 and sample(N=1 << 31) == -1 and sample(ip=None) == -1 and sample(fp=None) == -1 and sample(up=None) == -1
    assert sample(up=uv.data_ptr() + 4) == -1 and sample(bp=None) == -1 and sample(rp=None) == -1 and sample(vp=None) == -1
    assert b"null" in L.nerf_hip_last_error()
    torch.cuda.synchronize()
    assert (points == 2.5).all() and (dirs == 2.5).all() and (mask == 99).all() and (rgb == 2.5).all() and (valid == 99).all()
    # empty calls succeed without pointers, and the good calls go through
    assert texels(rows=0, pp=None, dp=None, mp=None) == 0 and texels(row0=H, rows=0) == 0 and sample(N=0, fp=None, up=None, rp=None, vp=None) == 0
    assert texels(v=0, f=0, vp=None, np_=None, fp=None, rows=0, pp=None, dp=None, mp=None) == 0
    assert L.nerf_hip_mesh_atlas_dims(F, n, out5) == 0 and tuple(out5) == (c, Sx, Sy, W, H)
    assert texels() == 0 and sample() == 0
    torch.cuda.synchronize()
    owner = torch.from_numpy(R.owner(F, n)[0].reshape(-1) >= 0)
    assert torch.equal(mask.cpu() != 0, owner) and not points.any() and not dirs.any()  # every face is vertex 0 three times, at 0 with normal 0
    assert bool((valid == 1).all()) and not rgb.any()
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.atlas_texels(pkg.mesh.Mesh(verts.cpu(), faces.cpu(), verts.cpu(), None), n)


# ---- (6) the runner writes the OBJ beside the PLY ----

def test_runner_texture(pkg, dev, tmp_path, capsys):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    level = float(np.median(run.density_grid(12, save=False)))
    plain = run.extract_mesh(12, level, save=True, simplify=2)
    files = glob.glob(rs + "*_mesh12.ply")
    assert len(files) == 1 and "[TEXTURE]" not in capsys.readouterr().out and not glob.glob(rs + "*.obj")
    before = open(files[0], "rb").read()
    got = run.extract_mesh(12, level, save=True, simplify=2, texture=128)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH]") and "[TEXTURE]" in ln]
    tex = run.model.last_texture
    assert len(line) == 1 and f"{tex.image.shape[1]} x {tex.image.shape[0]}, chart {tex.chart}, {len(plain.faces)} faces" in line[0]
    assert all(np.array_equal(a, b) for a, b in zip(got, plain)) and open(files[0], "rb").read() == before
    stem = files[0][:-4]
    obj = open(stem + ".obj").read().splitlines()
    assert sum(ln.startswith("vt ") for ln in obj) == 3 * len(plain.faces) and sum(ln.startswith("f ") for ln in obj) == len(plain.faces)
    assert open(stem + ".mtl").read().split()[-1] == stem.split("/")[-1] + ".png" and open(stem + ".png", "rb").read()[:4] == b"\x89PNG"
