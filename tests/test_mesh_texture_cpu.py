"""CPU: rule TA / TX of include/nerf_hip.h on the numpy restatement tests/texture_reference.py -- no bleeding between faces (P1) and
linear colours exactly back from a bilinear lookup (P2) --, the atlas's sizes in the package, the restatement and the library, the
new symbols of the C ABI, and the OBJ / MTL / PNG writer read back (no device)."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import texture_reference as R
from conftest import ROOT

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24  # half an ulp of fp32, relative: the error of one rounding


def _faces_under_test(F):
    return sorted(set(range(F)) if F <= 5 else {0, 1, 2, 3, F // 2, F // 2 + 1, F - 2, F - 1})


# ---- (1) P1 and P2 ----

@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("F", [1, 4, 5, 51, 200])
def test_no_bleeding_and_linear_colours_come_back(F, n):
    """Per face a colour that is linear over it, written into the atlas with rule TA's fp32 weights and operation order; every texel no
    face owns is NaN.  P1: every texel a lookup reads (weight != 0) belongs to the lookup's face.  P2: the lookup returns the linear
    colour.  The bound counts roundings, each at most EPS of the rounded quantity, with M the largest |corner colour| of the face and
    |w0| + |u| + |v| <= 1 + 2 / n <= 2 on the support: the three weights (2 EPS M together), the three products (2 EPS M), the inner sum
    (|u| + |v| <= 1.5: 1.5 EPS M), the outer sum (2 EPS M) -- 7.5 EPS M per texel, kept by the lookup's convex fp64 weights --, the final
    rounding of the lookup to fp32 (EPS M: the result lies inside the corners' range), and for the lookup's and the expectation's own
    fp64 operations 64 roundings of 2^-53 M.  9 EPS M covers them and the second-order terms."""
    rng = np.random.default_rng(1000 * F + n)
    c, Sx, Sy, W, H = R.dims(F, n)
    face, wts, support = R.owner(F, n)
    corner = (rng.uniform(-1.0, 1.0, (F, 3, 3)) * rng.choice([1.0, 100.0, 1e-3], (F, 1, 1))).astype(F32)  # [face, corner, channel]
    image = np.full((H, W, 3), np.nan, F32)
    den = F32(2 * n)
    for y, x in zip(*np.nonzero(face >= 0)):
        w0, u, v = (F32(k) / den for k in wts[y, x])
        cA, cB, cC = corner[face[y, x]]
        image[y, x] = w0 * cA + (u * cB + v * cC)
    owned = int((face >= 0).sum())
    assert owned == (F // 2) * c * c + (F % 2) * (c * (c + 1) // 2)  # a lower face owns the diagonal as well
    bary = R.barycentrics(64, seed=F + n)
    assert (bary.sum(1) <= 1.0).all()
    worst = 0.0
    for f in _faces_under_test(F):
        touched = []
        got, valid = R.sample(image, F, n, np.full(len(bary), f), bary, touched=touched)
        assert valid.all()
        bleed = [t for t in touched if face[t[1], t[2]] != f]
        assert not bleed, f"face {f}: {len(bleed)} texels of other faces read, first {bleed[0]}"
        assert all(w > 0 for _, _, _, w in touched)
        cA, cB, cC = corner[f].astype(F64)
        u, v = bary[:, :1], bary[:, 1:]
        want = ((1.0 - u) - v) * cA + (u * cB + v * cC)
        M = float(np.abs(corner[f]).max())
        err = float(np.abs(got.astype(F64) - want).max())
        worst = max(worst, err / M)
        assert err <= 9 * EPS * M, f"face {f}: error {err:.3e} = {err / (EPS * M):.2f} EPS M"
        # at the corners the lookup is the corner texel, bit for bit
        k, up = f >> 1, f & 1
        for q, (i, j) in enumerate([(1, 1), (1 + n, 1), (1, 1 + n)]):
            X, Y = (k % Sx) * c + (c - 1 - i if up else i), (k // Sx) * c + (c - 1 - j if up else j)
            assert got[q].tobytes() == image[Y, X].tobytes() == corner[f, q].tobytes()
    print(f"F={F} n={n}: atlas {W} x {H}, {owned} owned texels ({int(support.sum())} support), worst error {worst / EPS:.2f} EPS M")


def test_lookup_edges():
    F, n = 5, 3
    c, Sx, Sy, W, H = R.dims(F, n)
    image = np.random.default_rng(2).random((H, W, 3)).astype(F32)
    face = np.array([-1, F, 0, 0, 0, 4, 4, 2], np.int64)
    uv = np.array([[0.2, 0.2], [0.2, 0.2], [np.nan, 0.1], [0.1, np.inf], [-3.0, 0.5], [2.0, 2.0], [0.75, 0.75], [0.25, 0.5]])
    got, valid = R.sample(image, F, n, face, uv, background=(0.25, 0.5, 0.75))
    assert valid.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert (got[:4] == np.array([0.25, 0.5, 0.75], F32)).all()
    # clamped into the triangle: (-3, .5) -> (0, .5); (2, 2) -> (1, 0); (.75, .75) -> (.75, .25)
    want, _ = R.sample(image, F, n, face[4:7], np.array([[0.0, 0.5], [1.0, 0.0], [0.75, 0.25]]))
    assert got[4:7].tobytes() == want.tobytes()


# ---- (2) the atlas's sizes ----

@pytest.mark.parametrize("K", [1, 4, 5, 9, 10])
def test_atlas_dims_at_perfect_squares_and_their_neighbours(pkg, K):
    for F in (2 * K - 1, 2 * K):
        for n in (2, 3, 16):
            c, Sx, Sy, W, H = d = pkg.mesh.atlas_dims(F, n)
            assert d == R.dims(F, n) == pkg._abi.mesh_atlas_dims(F, n)
            assert c == n + 5 and Sx * Sx >= K > (Sx - 1) * (Sx - 1) and Sx * Sy >= K > Sx * (Sy - 1) and (W, H) == (Sx * c, Sy * c)
    assert pkg.mesh.atlas_dims(2 * K, 2)[1:3] == {1: (1, 1), 4: (2, 2), 5: (3, 2), 9: (3, 3), 10: (4, 3)}[K]


def test_atlas_dims_empty_and_refusals(pkg):
    assert pkg.mesh.atlas_dims(0, 2) == (7, 0, 0, 0, 0) == R.dims(0, 2) == pkg._abi.mesh_atlas_dims(0, 2)
    big = 20_000_000  # K = 10^7, Sx = 3163: 22141 x 22134 texels at n = 2
    assert pkg.mesh.atlas_dims(big, 2) == R.dims(big, 2) == pkg._abi.mesh_atlas_dims(big, 2)
    bad = [(1, 1), (1, 0), (1, -3), (-1, 2), (715_827_883, 2),  # n < 2; F < 0; 3 F = 2^31 + 1
           (200_000_000, 2),   # 70000 x 70000 texels
           (big, 10), (2, 2 ** 31 - 6), (2, 46_336)]  # (2, 46336): one cell of 46341^2 >= 2^31 texels
    for F, n in bad:
        with pytest.raises(ValueError):
            pkg.mesh.atlas_dims(F, n)
        with pytest.raises(pkg._abi.NerfHipError):
            pkg._abi.mesh_atlas_dims(F, n)
    assert pkg.mesh.atlas_dims(2, 46_335)[3] == 46_340  # 46340^2 < 2^31
    assert pkg._abi.lib().nerf_hip_mesh_atlas_dims(4, 2, None) == -1  # NERF_HIP_ERR_ARG
    with pytest.raises(ValueError):
        pkg.mesh.atlas_dims(2.5, 2)


def test_atlas_chart(pkg):
    for F, size in [(1, 7), (2, 64), (5, 512), (51, 512), (200, 130), (9000, 2048), (150_000, 4096)]:
        n = pkg.mesh.atlas_chart(F, size)
        Sx = pkg.mesh.atlas_dims(F, n)[1]
        assert n >= 2 and Sx * (n + 5) <= size < Sx * (n + 6)
    assert pkg.mesh.atlas_chart(200, 130) == 8 and pkg.mesh.atlas_dims(200, 8)[3:] == (130, 130)
    assert pkg.mesh.atlas_chart(5, 14) == 2 and pkg.mesh.atlas_dims(5, 2)[3:] == (14, 14)
    for F, size in [(1, 6), (200, 69), (0, 512), (150_000, 1024)]:
        with pytest.raises(ValueError):
            pkg.mesh.atlas_chart(F, size)


def test_uv_table_matches_the_restatement(pkg):
    for F, n in [(1, 2), (5, 2), (51, 3), (200, 8)]:
        got = pkg.mesh.atlas_uv(F, n, "cpu")
        want = R.uv_table(F, n)
        assert got.dtype == torch.float32 and got.numpy().tobytes() == want.tobytes()
        c, Sx, Sy, W, H = R.dims(F, n)
        px = want.astype(F64) * (W, H)  # the corners sit on texel centres of texels the face owns
        face, _, _ = R.owner(F, n)
        for f in range(F):
            for q in range(3):
                x, y = px[f, q]
                assert abs(x - 0.5 - round(x - 0.5)) < 1e-4 and face[int(y), int(x)] == f
    assert tuple(pkg.mesh.atlas_uv(0, 2, "cpu").shape) == (0, 3, 2)


# ---- (3) the C ABI ----

def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    src = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define NERF_HIP_ABI_VERSION 7\b", src) and pkg._abi.NERF_HIP_ABI_VERSION == 7
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    for name in ("nerf_hip_mesh_atlas_dims", "nerf_hip_mesh_atlas_texels", "nerf_hip_mesh_texture_sample"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in pkg._abi.EXPORTS and hasattr(lib, name), name
    assert pkg._abi.lib().nerf_hip_abi_version() == 7


def test_no_cpu_path(pkg):
    v = torch.zeros(3, 3)
    m = pkg.mesh.Mesh(v, torch.tensor([[0, 1, 2]], dtype=torch.int32), v, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.atlas_texels(m, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.bake_texture(m, 2, lambda p, d: p)
    tex = pkg.mesh.Texture(torch.zeros(7, 7, 3), torch.zeros(7, 7, dtype=torch.bool), 2, 1, pkg.mesh.atlas_uv(1, 2, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.sample_texture(tex, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.float64))


# ---- (4) the OBJ / MTL / PNG writer, read back ----

def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)  # 8-bit RGB, not interlaced
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(H, 1 + 3 * W)
    assert not raw[:, 0].any()  # filter 0 on every row
    return raw[:, 1:].reshape(H, W, 3)


def test_write_obj_round_trip(pkg, tmp_path):
    F, n = 2, 2
    c, Sx, Sy, W, H = R.dims(F, n)
    rng = np.random.default_rng(4)
    verts = np.array([[0, 0, 0], [1, 0, 0.125], [0, 1, -2.5], [1.1, 0.9, 1e-3]], F32)
    normals = np.array([[0, 0, 1], [0, 0.6, 0.8], [1, 0, 0], [0, -1, 0]], F32)
    faces = np.array([[0, 1, 2], [3, 2, 1]], np.int32)
    image = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(F32)
    image[0, 0] = (-0.5, 1.5, 0.5)  # clipped below and above; 127.5 is a tie: rint rounds to even
    image[0, 1] = (1.0, 0.0, 0.25)
    tex = pkg.mesh.Texture(torch.from_numpy(image), torch.ones(H, W, dtype=torch.bool), n, F, torch.from_numpy(R.uv_table(F, n)))
    m = pkg.mesh.Mesh(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(normals), None)
    paths = pkg.mesh.write_obj(str(tmp_path / "out.obj"), m, tex)
    assert [os.path.basename(p) for p in paths] == ["out.obj", "out.mtl", "out.png"] and all(os.path.exists(p) for p in paths)
    lines = open(paths[0]).read().splitlines()
    rows = lambda key: [ln.split()[1:] for ln in lines if ln.split()[0] == key]
    assert rows("mtllib") == [["out.mtl"]] and rows("usemtl") == [["out"]]
    assert lines.index("usemtl out") < min(i for i, ln in enumerate(lines) if ln.startswith("f "))
    v = np.array(rows("v"), F64).astype(F32)
    vn = np.array(rows("vn"), F64).astype(F32)
    vt = np.array(rows("vt"), F64).astype(F32)
    assert v.tobytes() == verts.tobytes() and vn.tobytes() == normals.tobytes()  # the decimal text reads back to the same fp32
    uv = R.uv_table(F, n).reshape(-1, 2)
    assert vt.shape == (3 * F, 2) and vt[:, 0].tobytes() == uv[:, 0].tobytes() and vt[:, 1].tobytes() == (F32(1.0) - uv[:, 1]).tobytes()
    f = [[tuple(int(x) for x in corner.split("/")) for corner in row] for row in rows("f")]
    assert len(f) == F
    for k, row in enumerate(f):  # 1-based: position / texture / normal
        assert [a for a, _, _ in row] == (faces[k] + 1).tolist() == [c_ for _, _, c_ in row]
        assert [t for _, t, _ in row] == [3 * k + 1, 3 * k + 2, 3 * k + 3]
    mtl = open(paths[1]).read().split()
    assert mtl[mtl.index("newmtl") + 1] == "out" and mtl[mtl.index("map_Kd") + 1] == "out.png"
    px = _read_png(paths[2])
    want = np.clip(np.rint(image.astype(F64) * 255.0), 0, 255).astype(np.uint8)
    assert px.shape == (H, W, 3) and px.tobytes() == want.tobytes()
    assert px[0, 0].tolist() == [0, 255, 128] and px[0, 1].tolist() == [255, 0, 64] and px.min() == 0 and px.max() == 255
    # without normals: f a/ta; a texture of another face count is refused
    pkg.mesh.write_obj(str(tmp_path / "plain.obj"), m._replace(normals=None), tex)
    plain = open(tmp_path / "plain.obj").read().splitlines()
    assert not any(ln.startswith("vn ") for ln in plain) and "f 1/1 2/2 3/3" in plain
    with pytest.raises(ValueError):
        pkg.mesh.write_obj(str(tmp_path / "bad.obj"), m._replace(faces=torch.from_numpy(faces[:1])), tex)
