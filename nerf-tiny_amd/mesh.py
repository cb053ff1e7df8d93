"""Triangle meshes of the field's isosurfaces (not in the reference): marching cubes over a device density grid (HIP kernels,
csrc/mesh.hip), connected components on the device -- label, measure and drop the floaters (csrc/mesh_cc.hip,
DESIGN.md section 3h-3) --, simplification by uniform vertex clustering on the device (csrc/mesh_simplify.hip)
and a binary PLY writer.  NeRFModel.extract_mesh / NeRFRunner.extract_mesh build on these."""
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


class Components(NamedTuple):
    vert_comp: object  # [V] int32 component id of each vertex; ids 0 .. C-1 ascend with the component's smallest vertex index
    face_comp: object  # [F] int32 id of the face's first vertex; -1 for a face with an index outside [0, V)
    n_verts: object    # [C] int32
    n_faces: object    # [C] int32
    bbox_lo: object    # [C, 3] fp32 minimum of the component's finite vertex coordinates (+inf where it has none), or None
    bbox_hi: object    # [C, 3] fp32 maximum (-inf where it has none), or None
    rounds: object = None  # labelling rounds the device took, the last one changing nothing


def components(faces, num_verts, verts=None):
    """Connected components of an indexed triangle mesh on the DEVICE: faces [F, 3] int32 over num_verts vertices (any indexed mesh,
    not only marching_cubes').  Two vertices are connected when some face contains both, so two triangles that share one vertex are
    one component; a vertex in no face is a component of its own with 0 faces; a face with an index outside [0, num_verts) takes no
    part (face_comp -1).  Returns Components of device tensors, the boxes only with verts [V, 3]; the exact rules are in
    include/nerf_hip.h and every output is a pure function of the input (identical bits from run to run).  A CPU tensor raises: there
    is no CPU path."""
    from . import ops

    faces = torch.as_tensor(faces)
    if faces.device.type != "cuda":
        raise RuntimeError("components runs only on a ROCm device (MI355X): faces.to('cuda'); there is no CPU path")
    return Components(*ops.mesh_components(faces, num_verts, verts))


def select_components(comps, min_faces=1, keep_largest=None):
    """A keep mask [C] bool over comps (a Components): n_faces >= min_faces, and with keep_largest=k also among the k components with
    the most faces (ties go to the lower id).  Bookkeeping on the [C] arrays in torch; build a mask of your own from comps.bbox_lo /
    bbox_hi / n_verts where these rules do not fit (e.g. keep what intersects a box)."""
    n = torch.as_tensor(comps.n_faces)
    keep = n >= int(min_faces)
    if keep_largest is not None:
        k = int(keep_largest)
        if k < 0:
            raise ValueError(f"keep_largest={k} < 0")
        order = torch.sort(n, descending=True, stable=True).indices  # (stable: equal counts stay in id order)
        top = torch.zeros_like(keep)
        top[order[:k]] = True
        keep = keep & top
    return keep


def filter_components(m, comps, keep):
    """The Mesh m without the components whose keep[c] is False (device compaction): kept vertices -- with their normals and rgb where m
    has them -- and kept faces stay in their order, face indices are renumbered, faces that take no part (face_comp -1) are dropped."""
    from . import ops

    keep = torch.as_tensor(keep).to(comps.n_faces.device) != 0
    if tuple(keep.shape) != tuple(comps.n_faces.shape):
        raise ValueError(f"keep {tuple(keep.shape)}: one entry per component, [{len(comps.n_faces)}]")
    V1 = int(comps.n_verts[keep].sum())  # (one read; the device writes the same counts)
    F1 = int(comps.n_faces[keep].sum())
    v, f, n, c, _ = ops.mesh_compact(m.verts, m.faces, m.normals, m.rgb, comps.vert_comp, comps.face_comp, keep, V1, F1)
    return Mesh(v, f, n, c)


SIMPLIFY_MAX_DIM = 2048  # cells per axis of a cluster lattice (include/nerf_hip.h)


def simplify_lattice(verts, cell, lo=None):
    """The default cluster lattice of simplify(): (lo [3] fp32, cell [3] fp32, dims [3] int) as numpy arrays.  Over the vertices whose
    three coordinates are finite, lo = the per-axis minimum (unless lo is given) and, with hi the per-axis maximum,
    dims = clamp(floor(fp32(fp32(hi - lo) / cell)) + 1, 1, 2048) -- the cell rule of include/nerf_hip.h applied to hi, so every finite
    vertex lies in the cell of its own coordinates unless an axis needs more than 2048 cells (the clamp then pulls the rest into the
    last one).  A mesh without a finite vertex gets lo = 0 (unless given) and dims = 1."""
    cell32 = np.broadcast_to(np.asarray(cell, dtype=np.float32), (3,)).copy()
    v = torch.as_tensor(verts).to(torch.float32).reshape(-1, 3)
    ok = torch.isfinite(v).all(1, keepdim=True)
    if not bool(ok.any()):
        return (np.zeros(3, np.float32) if lo is None else np.asarray(lo, np.float32).reshape(3)), cell32, np.ones(3, np.int64)
    inf = torch.full_like(v, float("inf"))
    if lo is None:
        lo = torch.where(ok, v, inf).amin(0).cpu().numpy()
    lo = np.asarray(lo, np.float32).reshape(3)
    hi = torch.where(ok, v, -inf).amax(0).cpu().numpy()
    with np.errstate(all="ignore"):
        u = ((hi - lo).astype(np.float32) / cell32).astype(np.float32)
        dims = np.clip(np.floor(u.astype(np.float64)) + 1, 1, SIMPLIFY_MAX_DIM)
    return lo, cell32, np.where(np.isnan(dims), 1, dims).astype(np.int64)


def simplify(m, cell, lo=None, dims=None):
    """The Mesh m simplified on the DEVICE by uniform vertex clustering (Rossignac-Borrel): the vertices in one cell of a regular
    lattice merge into one vertex at their mean, faces that lose a corner this way or repeat an earlier face go.  Any indexed mesh.
    cell: the cell size, a float or three (> 0); lo: the lattice's corner (three floats), dims: its cells per axis (three ints in
    1 .. 2048, product < 2^31) -- by default simplify_lattice(m.verts, cell, lo), which covers the finite vertices; vertices outside a
    given lattice are pulled to its faces.  Returns (Mesh, info): verts, faces, normals (the members' normals summed and normalised;
    None when m has none) and rgb=None -- colours are not carried, query the field at the new vertices --; info = dict(verts_in,
    faces_in, verts_out, faces_out, clusters, degenerate_faces, duplicate_faces, lo, cell, dims).  A face whose three corners fall into
    the same three cells in the OPPOSITE orientation of an earlier one is kept: a collapsed thin sheet seen from both sides.  The
    exact rules are in include/nerf_hip.h; every output is a pure function of the input (identical bits from run to run).  A CPU
    tensor raises: there is no CPU path."""
    from . import ops

    verts, faces = torch.as_tensor(m.verts), torch.as_tensor(m.faces)
    if verts.device.type != "cuda":
        raise RuntimeError("simplify runs only on a ROCm device (MI355X): move the mesh to 'cuda'; there is no CPU path")
    cell32 = np.broadcast_to(np.asarray(cell, dtype=np.float32), (3,)).copy()
    if lo is None or dims is None:
        dlo, _, ddims = simplify_lattice(verts, cell32, lo)
        lo = dlo
        dims = ddims if dims is None else dims
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    dims3 = [int(d) for d in np.asarray(dims).reshape(3)]
    v, f, n, info = ops.mesh_simplify(verts, faces, m.normals, lo32.tolist(), cell32.tolist(), dims3)
    info.update(lo=lo32, cell=cell32, dims=tuple(dims3))
    return Mesh(v, f, n, None), info


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
