"""Triangle meshes of the field's isosurfaces (not in the reference): marching cubes over a device density grid (HIP kernels,
csrc/mesh.hip) and a binary PLY writer.  NeRFModel.extract_mesh / NeRFRunner.extract_mesh build on these."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


class Mesh(NamedTuple):
    verts: object    # [V, 3] fp32 world coordinates
    faces: object    # [F, 3] int32 vertex indices, counter-clockwise seen from outside
    normals: object  # [V, 3] fp32 unit outward normals (-grad sigma / |grad sigma|; 0 where the gradient vanishes)
    rgb: object      # [V, 3] fp32 colours, or None


def marching_cubes(sigma, level, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), ws=None):
    """The isosurface sigma == level of a DEVICE grid sigma[nx, ny, nz] (C order, z fastest; e.g. model.density_grid, or the ``sigma``
    of an exported .npz moved to the device).  Lattice point (i, j, k) sits at lo + (i, j, k) * step, each coordinate one fp32 product
    and one fp32 sum (the density grid's rule: pass the .npz's ``lo`` and ``step``).  Inside is sigma > level.  Returns
    (verts [V, 3] fp32, faces [F, 3] int32, normals [V, 3] fp32) on sigma's device; the exact vertex, face and normal rules are in
    include/nerf_hip.h.  A CPU tensor raises: there is no CPU path."""
    from . import ops

    sigma = torch.as_tensor(sigma)
    if sigma.device.type != "cuda":
        raise RuntimeError("marching_cubes runs only on a ROCm device (MI355X): sigma.to('cuda'); there is no CPU path")
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    step32 = np.asarray(step, dtype=np.float32).reshape(3)
    return ops.marching_cubes(sigma, lo32.tolist(), step32.tolist(), float(np.float32(level)), ws=ws)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, verts, faces, normals=None, rgb=None):
    """Binary little-endian PLY 1.0: vertex properties ``x y z`` (float), then ``nx ny nz`` (float) with normals and ``red green
    blue`` (uchar, clip(rint(rgb * 255), 0, 255)) with rgb; faces as ``list uchar int vertex_indices``.  Tensors or arrays."""
    v = _np(verts).astype("<f4").reshape(-1, 3)
    f = _np(faces).astype("<i4").reshape(-1, 3)
    cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    parts = [v]
    if normals is not None:
        cols += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
        parts.append(_np(normals).astype("<f4").reshape(-1, 3))
    if rgb is not None:
        cols += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
        parts.append(np.clip(np.rint(_np(rgb).astype(np.float64).reshape(-1, 3) * 255.0), 0, 255).astype("u1"))
    for p in parts:
        if len(p) != len(v):
            raise ValueError(f"per-vertex arrays of {len(p)} and {len(v)} rows")
    vrec = np.empty(len(v), dtype=np.dtype(cols))
    c = 0
    for p in parts:
        for k in range(3):
            vrec[cols[c][0]] = p[:, k]
            c += 1
    frec = np.empty(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"] = 3
    frec["i"] = f
    header = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", *props, f"element face {len(f)}",
                        "property list uchar int vertex_indices", "end_header"]) + "\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
