"""GPU: the field at explicit points (NeRFModel.query / density_grid, nerf_hip_query / nerf_hip_density_grid) against the CPU oracle,
bit for bit against the ray path's field kernel, and through the driver's .npz export."""
import glob

import numpy as np
import pytest
import torch

from conftest import golden_inputs, load_golden, max_rel

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _model(pkg, oracle, dev, seed, sharp):
    w = oracle.make_weights(seed, sharp)
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(w)
    return m.to(dev), w


def _unit_dirs(gen, M):
    d = torch.randn(M, 3, generator=gen)
    return d / d.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("M", [1, 31, 33, 4097, 100003])
def test_query_against_oracle(oracle, pkg, dev, sharp, M):
    m, w = _model(pkg, oracle, dev, 11, sharp)
    gen = torch.Generator().manual_seed(M)
    pts = (torch.rand(M, 3, generator=gen) * 8.0 - 4.0).float()
    dirs = _unit_dirs(gen, M)
    rgb, sig = m.query(pts.to(dev), dirs.to(dev))
    _, sig_only = m.query(pts.to(dev))
    fp, fd = oracle.frequencies()
    with torch.no_grad():
        orgb, osig = oracle.mlp(w, oracle.encode(pts, fp), oracle.encode(dirs, fd))
    assert rgb.shape == (M, 3) and sig.shape == (M,)
    assert max_rel(sig, osig) < TOL
    assert max_rel(rgb, orgb) < TOL
    assert torch.equal(sig_only, sig)  # the sigma-only form stops after the same sigma head


@pytest.mark.parametrize("name", ["cfg1_lego_crop32", "cfg4_fern_rand512"])
def test_query_is_bit_identical_to_the_ray_path(oracle, pkg, dev, name):
    """The production inference field kernel (ops.field without debug outputs) at the ray samples == query() at the same points with
    the rays' world directions: same encoding, same MLP, same dir_info start vectors, same bits."""
    g = load_golden(name)
    row, col, pb, K, _ = golden_inputs(g)
    B, N = min(row.shape[0], 256), int(g["Nc"])
    row, col, pb = row[:B], col[:B], pb[:B]
    m, w = _model(pkg, oracle, dev, int(g["seed"]), bool(g["sharp"]))
    pd = [p.detach() for p in m.network.parameters()]
    R, o, near, far = oracle.poses_extract(pb)
    t = oracle.coarse_depths(near, far, N)
    rgb_f, sig_f = pkg.ops.field(pd, row.to(dev), col.to(dev), pb.float().to(dev), K, t.to(dev))
    pts = oracle.sample_points(R, o, oracle.camera_dirs(row, col, K), t).reshape(-1, 3)
    _, d_wrd, _ = pkg.ops.rays(row.to(dev), col.to(dev), pb.float().to(dev), K, N)
    dirs = d_wrd[:, None, :].expand(B, N, 3).reshape(-1, 3)
    rgb_q, sig_q = m.query(pts.to(dev), dirs)
    assert torch.equal(rgb_q, rgb_f.reshape(-1, 3))
    assert torch.equal(sig_q, sig_f.reshape(-1))
    _, sig_s = m.query(pts.to(dev))
    assert torch.equal(sig_s, sig_f.reshape(-1))


@pytest.mark.parametrize("sharp", [False, True])
def test_density_grid_is_the_lattice_query(oracle, pkg, dev, sharp):
    m, w = _model(pkg, oracle, dev, 5, sharp)
    shape = (37, 20, 45)
    lo, hi = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35)
    grid = m.density_grid(lo, hi, shape)
    assert grid.shape == shape and grid.dtype == torch.float32
    lo32 = torch.tensor(lo, dtype=torch.float32)
    step = (torch.tensor(hi, dtype=torch.float32) - lo32) / torch.tensor([n - 1 for n in shape], dtype=torch.float32)
    axes = [lo32[c] + torch.arange(shape[c], dtype=torch.float32) * step[c] for c in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    _, sig = m.query(pts.to(dev))
    assert torch.equal(grid.reshape(-1), sig)
    fp, fd = oracle.frequencies()
    with torch.no_grad():
        _, osig = oracle.mlp(w, oracle.encode(pts, fp), torch.zeros(pts.shape[0], 24))
    assert max_rel(grid.reshape(-1), osig) < TOL


def test_density_grid_slabs(oracle, pkg, dev):
    """A 128^3 grid == its x-slabs computed as grids of their own (a lattice whose points are exact in fp32: lo + i * step is the
    same number whichever slab it is formed in)."""
    m, _ = _model(pkg, oracle, dev, 2, True)
    n, lo, step = 128, -2.0, 1.0 / 32.0
    hi = lo + (n - 1) * step
    full = m.density_grid((lo,) * 3, (hi,) * 3, n)
    parts = []
    for x0, x1 in ((0, 1), (1, 40), (40, 97), (97, 128)):
        parts.append(pkg.ops.density_grid([p.detach() for p in m.network.parameters()], [lo + x0 * step, lo, lo], [step] * 3,
                                          (x1 - x0, n, n)))
    assert torch.equal(torch.cat(parts, dim=0), full)


def test_query_model_surface(oracle, pkg, dev):
    m, _ = _model(pkg, oracle, dev, 3, True)
    before = [p.detach().clone() for p in m.network.parameters()]
    gen = torch.Generator().manual_seed(0)
    pts, dirs = (torch.rand(1000, 3, generator=gen) * 4 - 2).to(dev), _unit_dirs(gen, 1000).to(dev)
    with torch.enable_grad():
        rgb, sig = m.query(pts, dirs)
        grid = m.density_grid((-1, -1, -1), (1, 1, 1), 9)
    assert not rgb.requires_grad and not sig.requires_grad and not grid.requires_grad
    assert all(torch.equal(a, b) for a, b in zip(before, m.network.parameters()))
    # queries are exact fp32 whatever the model's inference flags say
    m.bf16_mlp = True
    rgb_b, sig_b = m.query(pts, dirs)
    grid_b = m.density_grid((-1, -1, -1), (1, 1, 1), 9)
    m.bf16_mlp, m.split_mlp = False, True
    rgb_s, sig_s = m.query(pts, dirs)
    m.split_mlp = False
    assert torch.equal(rgb_b, rgb) and torch.equal(sig_b, sig) and torch.equal(grid_b, grid)
    assert torch.equal(rgb_s, rgb) and torch.equal(sig_s, sig)
    # empty queries
    r0, s0 = m.query(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev))
    assert r0.shape == (0, 3) and s0.shape == (0,)
    r0, s0 = m.query(torch.empty(0, 3, device=dev))
    assert r0 is None and s0.shape == (0,)
    # the query workspaces do not travel into a pickle
    assert m.__getstate__()["_qws"] == {}


def test_runner_exports_a_density_grid(pkg, dev, tmp_path):
    scene = pkg.data.synthetic_scene(n_pic=4, H=32, W=32, seed=1)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=6, batch_ray=256, learning=3e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1000, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1000)
    run = pkg.NeRFRunner(continue_=False, **kw)
    assert run.trainer("train") == 5
    sig = run.density_grid(32, save=True)
    files = glob.glob(rs + "*_5_sigma32.npz")
    assert len(files) == 1
    z = np.load(files[0])
    assert z["sigma"].shape == (32, 32, 32) and z["sigma"].dtype == np.float32
    assert np.isfinite(z["sigma"]).all() and (z["sigma"] >= 0).all()
    assert np.array_equal(z["sigma"], sig)
    assert np.array_equal(z["lo"], np.float32([-1.5] * 3)) and np.array_equal(z["hi"], np.float32([1.5] * 3))
    assert np.array_equal(z["step"], np.float32([3.0 / 31] * 3)) and int(z["iter"]) == 5
