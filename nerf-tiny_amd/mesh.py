"""Triangle meshes of the field's isosurfaces (not in the reference): marching cubes over a device density grid (HIP kernels,
csrc/mesh.hip), connected components on the device -- label, measure and drop the floaters (csrc/mesh_cc.hip,
DESIGN.md section 3h-3) --, simplification by uniform vertex clustering on the device (csrc/mesh_simplify.hip),
edge topology, Taubin smoothing and face-derived vertex normals on the device (csrc/mesh_smooth.hip), geometry
evaluation on the device -- measures, area-weighted surface samples, exact nearest points, Chamfer distance and F-scores
(csrc/mesh_distance.hip) --, rays against a mesh on the device -- closest hits, occlusion, depth images, the
faces no camera sees (csrc/mesh_raycast.hip) --, TSDF fusion of depth images into a signed distance volume on the
device (csrc/tsdf.hip), with the views' colours fused beside it and marching cubes under a mask of observed
points, texture atlases -- a per-face parameterisation, the texels' surface points and viewing directions on
the device, a baker, bilinear lookups by (face, u, v) and the textured mesh seen from a camera (csrc/mesh_texture.hip, DESIGN.md section
3h-11) --, a PLY writer and reader and an OBJ / MTL / PNG writer.  NeRFModel.extract_mesh / NeRFRunner.extract_mesh
build on these."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


class Mesh(NamedTuple):
    verts: object    # [V, 3] fp32 world coordinates
    faces: object    # [F, 3] int32 vertex indices, counter-clockwise seen from outside
    normals: object  # [V, 3] fp32 unit outward normals (-grad sigma / |grad sigma|; 0 where the gradient vanishes)
    rgb: object      # [V, 3] fp32 colours, or None


def marching_cubes(sigma, level, lo=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), ws=None, valid=None):
    """The isosurface sigma == level of a DEVICE grid sigma[nx, ny, nz] (C order, z fastest; e.g. model.density_grid, or the ``sigma``
    of an exported .npz moved to the device).  Lattice point (i, j, k) sits at lo + (i, j, k) * step, each coordinate one fp32 product
    and one fp32 sum (the density grid's rule: pass the .npz's ``lo`` and ``step``).  Inside is sigma > level.  Returns
    (verts [V, 3] fp32, faces [F, 3] int32, normals [V, 3] fp32) on sigma's device; the exact vertex, face and normal rules are in
    include/nerf_hip.h.  valid=None: every lattice point counts.  valid = a bool or uint8 DEVICE tensor of sigma's shape: masked
    marching cubes (rule M of include/nerf_hip.h) -- triangles only from the cells whose eight corners are valid, a vertex only on an
    edge of such a cell; the result is, bit for bit, filter_faces of the unmasked mesh with the faces of the other cells dropped.  The
    normals still read sigma at invalid points: fill them with a value of the class you want there.  A CPU tensor raises: there is no
    CPU path."""
    from . import ops

    sigma = torch.as_tensor(sigma)
    if sigma.device.type != "cuda" or (valid is not None and torch.as_tensor(valid).device.type != "cuda"):
        raise RuntimeError("marching_cubes runs only on a ROCm device (MI355X): sigma.to('cuda'); there is no CPU path")
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    step32 = np.asarray(step, dtype=np.float32).reshape(3)
    if valid is None:
        return ops.marching_cubes(sigma, lo32.tolist(), step32.tolist(), float(np.float32(level)), ws=ws)
    return ops.marching_cubes(sigma, lo32.tolist(), step32.tolist(), float(np.float32(level)), ws=ws, valid=torch.as_tensor(valid))


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


class Topology(NamedTuple):
    degree: object              # [V] int32 distinct neighbours of each vertex (device)
    vert_flags: object          # [V] int32: bit 0 = on a boundary edge, bit 1 = on a non-manifold edge (device)
    faces: int                  # faces that take part: three different indices in [0, V)
    edges: int                  # E: the unique undirected edges of those faces
    boundary_edges: int         # edges in one face
    nonmanifold_edges: int      # edges in more than two faces
    inconsistent_edges: int     # edges whose two faces run them in the same direction
    used_verts: int             # vertices with degree > 0
    max_degree: int
    euler: int                  # used_verts - edges + faces
    closed: bool                # faces > 0 and no boundary, non-manifold or inconsistent edge

    def summary(self) -> str:
        return (f"E {self.edges}, boundary {self.boundary_edges}, non-manifold {self.nonmanifold_edges}, inconsistent "
                f"{self.inconsistent_edges}, closed {self.closed}, euler {self.euler}")


def _topology(degree, flags, c):
    closed = c["faces"] > 0 and c["boundary_edges"] == 0 and c["nonmanifold_edges"] == 0 and c["inconsistent_edges"] == 0
    return Topology(degree, flags, c["faces"], c["edges"], c["boundary_edges"], c["nonmanifold_edges"], c["inconsistent_edges"],
                    c["used_verts"], c["max_degree"], c["used_verts"] - c["edges"] + c["faces"], closed)


def topology(faces, num_verts):
    """The edge topology of an indexed triangle mesh on the DEVICE: faces [F, 3] int32 over num_verts vertices (any indexed mesh).  A
    face takes part iff its three indices lie in [0, num_verts) and differ; the edges are the unordered index pairs of those faces.
    Returns a Topology: the per-vertex degree and flags as device tensors, the counts as Python ints (one host read) and euler /
    closed derived from them.  The exact rules are in include/nerf_hip.h; every output is a pure function of the input.  A CPU tensor
    raises: there is no CPU path."""
    from . import ops

    faces = torch.as_tensor(faces)
    if faces.device.type != "cuda":
        raise RuntimeError("topology runs only on a ROCm device (MI355X): faces.to('cuda'); there is no CPU path")
    degree, flags, counts, _ = ops.mesh_edges(faces, num_verts)
    return _topology(degree, flags, ops.mesh_edge_counts(counts.cpu().tolist(), int(num_verts), int(faces.shape[0])))


def pow2_at_least(ext) -> np.float32:
    """The scale rule of the smoothing box: the smallest power of two >= ext as fp32; 2^127 where ext is not finite or lies above
    2^127 (the box coordinates reach 2, so it still holds ext), 1 where ext is not > 0."""
    ext = np.float32(ext)
    if not ext > 0:
        return np.float32(1.0)
    if not np.isfinite(ext):
        return np.float32(2.0 ** 127)
    m, e = np.frexp(ext)  # ext = m * 2^e, m in [0.5, 1)
    return ext if m == 0.5 else np.float32(np.ldexp(np.float64(1.0), min(int(e), 127)))


def smooth_box(verts, lo=None, scale=None):
    """The default box of smooth() / vertex_normals(): (lo [3] fp32 numpy, scale fp32).  Over the vertices whose three coordinates
    are finite, lo = the per-axis minimum (unless given) and scale = pow2_at_least(the largest of fp32(hi - lo) over the axes) with hi
    the per-axis maximum (unless given).  A mesh without a finite vertex gets lo = 0 and scale = 1 (unless given)."""
    given = lo is not None and scale is not None
    v = torch.as_tensor(verts).to(torch.float32).reshape(-1, 3)
    ok = None if given else torch.isfinite(v).all(1, keepdim=True)
    if given or not bool(ok.any()):
        lo = np.zeros(3, np.float32) if lo is None else np.asarray(lo, np.float32).reshape(3)
        return lo, np.float32(1.0 if scale is None else scale)
    inf = torch.full_like(v, float("inf"))
    ext = torch.stack((torch.where(ok, v, inf).amin(0), torch.where(ok, v, -inf).amax(0))).cpu().numpy()  # (one host read)
    lo = ext[0] if lo is None else np.asarray(lo, np.float32).reshape(3)
    if scale is None:
        with np.errstate(all="ignore"):
            scale = pow2_at_least((ext[1] - lo).astype(np.float32).max())
    return lo.astype(np.float32), np.float32(scale)


def _check_box(lo, scale):
    if not np.isfinite(lo).all():
        raise ValueError(f"lo={lo!r}: the box's corner must be finite")
    if not np.isfinite(scale) or not scale > 0:
        raise ValueError(f"scale={scale!r}: must be finite and > 0")


def vertex_normals(verts, faces, lo=None, scale=None):
    """Unit vertex normals computed from the faces on the DEVICE: the area-weighted sum of the incident faces' cross products, in
    fixed point over the box lo / scale (by default smooth_box(verts)), normalised in fp64; (0, 0, 0) for a vertex without a
    contributing face.  Faces are counter-clockwise seen from outside, so the normals point outward.  verts [V, 3] fp32, faces [F, 3]
    int32 (any indexed mesh) -> [V, 3] fp32.  The exact rules are in include/nerf_hip.h; identical bits from run to run.  A CPU tensor
    raises: there is no CPU path."""
    from . import ops

    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    if verts.device.type != "cuda":
        raise RuntimeError("vertex_normals runs only on a ROCm device (MI355X): move the mesh to 'cuda'; there is no CPU path")
    lo, scale = smooth_box(verts, lo, scale)
    _check_box(lo, scale)
    return ops.mesh_vertex_normals(verts, faces, lo.tolist(), float(scale))


def smooth(m, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, lo=None, scale=None, normals=True):
    """The Mesh m with its vertex positions smoothed on the DEVICE by ``iterations`` Taubin iterations: a Jacobi step that moves every
    vertex by lam towards the mean of its distinct neighbours, then one by mu (< -lam: it undoes the shrinkage of the first); mu=None
    runs the lam steps alone (plain Laplacian smoothing, which shrinks).  The neighbours come from the mesh's unique edges, built once;
    the means are exact fixed-point sums over the box lo / scale (by default smooth_box(m.verts)), so the result is a pure function of
    the input -- identical bits from run to run.  fix_boundary: vertices on a boundary edge stay where they are (otherwise every
    opening shrinks).  Vertices with a coordinate that is not finite, or without a finite neighbour, stay as well.  Any indexed
    mesh.  Returns (Mesh, info): verts, the input's faces tensor, normals = vertex_normals of the result over the same box, rgb=None --
    colours are not carried, query the field at the new vertices --; info = dict(faces, edges, boundary_edges, nonmanifold_edges,
    inconsistent_edges, used_verts, max_degree, euler, closed, pinned, steps, lo, scale).  normals=False skips the normal pass (a
    memset, nine int64 atomics per face and a pass over the vertices) and returns normals=None, for a caller that makes its own.
    One host read of the counts.  The exact
    rules are in include/nerf_hip.h.  A CPU tensor raises: there is no CPU path."""
    from . import ops

    verts, faces = torch.as_tensor(m.verts), torch.as_tensor(m.faces)
    if verts.device.type != "cuda":
        raise RuntimeError("smooth runs only on a ROCm device (MI355X): move the mesh to 'cuda'; there is no CPU path")
    if int(iterations) != iterations or int(iterations) < 0:
        raise ValueError(f"iterations={iterations!r}: an int >= 0")
    if not np.isfinite(lam) or (mu is not None and not np.isfinite(mu)):
        raise ValueError(f"lam={lam!r} mu={mu!r}: finite weights (mu=None: no second step)")
    lo, scale = smooth_box(verts, lo, scale)
    _check_box(lo, scale)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    degree, flags, counts, ws = ops.mesh_edges(faces, V)
    pinned = (flags & 1).sum().reshape(1) if fix_boundary else torch.zeros(1, dtype=torch.int64, device=counts.device)
    host = torch.cat((counts, pinned)).cpu().tolist()  # (the one read)
    topo = _topology(degree, flags, ops.mesh_edge_counts(host[:8], V, F))
    cur = verts.to(torch.float32).contiguous()
    weights = ([float(lam)] if mu is None else [float(lam), float(mu)]) * int(iterations)
    if weights:
        bufs = [torch.empty_like(cur), torch.empty_like(cur) if len(weights) > 1 else None]
        for i, w in enumerate(weights):
            cur = ops.mesh_smooth_step(cur, bufs[i & 1], F, lo.tolist(), float(scale), w, flags if fix_boundary else None, ws)
    nrm = ops.mesh_vertex_normals(cur, faces, lo.tolist(), float(scale), ws=ws) if normals else None
    info = {k: getattr(topo, k) for k in Topology._fields[2:]}
    info.update(pinned=int(host[8]), steps=len(weights), lo=lo, scale=np.float32(scale))
    return Mesh(cur, m.faces, nrm, None), info


class Measure(NamedTuple):
    area: float        # surface area, in the mesh's units squared
    volume: float      # signed enclosed volume (meaningful for a closed, consistently oriented mesh; > 0 for outward faces)
    centroid: object   # [3] fp64 area-weighted centroid of the surface (NaN without area)
    faces: int         # faces that take part: three different indices in [0, V), finite corners
    raw: tuple         # the device's int64 sums: area, six volumes, three moments (2^-40 box units), faces, 0, 0


MEASURE_ONE = float(2 ** 40)


def measure_from_raw(raw, lo, scale):
    """The host's reading of nerf_hip_mesh_measure's eight int64s over the box lo / scale -> Measure."""
    raw = tuple(int(x) for x in raw)
    lo64, sc = np.asarray(lo, np.float32).reshape(3).astype(np.float64), float(np.float32(scale))
    with np.errstate(all="ignore"):
        cen = lo64 + sc * (np.array(raw[2:5], np.float64) / np.float64(raw[0])) if raw[0] else np.full(3, np.nan)
    return Measure(raw[0] / MEASURE_ONE * sc * sc, raw[1] / (6.0 * MEASURE_ONE) * sc * sc * sc, cen, raw[5], raw)


def _on_device(t, what):
    t = torch.as_tensor(t)
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on a ROCm device (MI355X): move the input to 'cuda'; there is no CPU path")
    return t


def measure(m, lo=None, scale=None):
    """Area, enclosed volume and area-weighted centroid of the Mesh m (any indexed mesh) on the DEVICE: per face the fp64 terms over
    the box lo / scale (by default smooth_box(m.verts)) rounded to int64 fixed point and summed by integer atomics, so the result is a
    pure function of the input.  Returns a Measure (one host read).  The exact rules are in include/nerf_hip.h.  A CPU tensor raises:
    there is no CPU path."""
    from . import ops

    verts, faces = _on_device(m.verts, "measure"), torch.as_tensor(m.faces)
    lo, scale = smooth_box(verts, lo, scale)
    _check_box(lo, scale)
    return measure_from_raw(ops.mesh_measure(verts, faces, lo.tolist(), float(scale)).cpu().tolist(), lo, scale)


def sample_surface(m, n, seed=0, lo=None, scale=None):
    """n points on the surface of the Mesh m distributed by area, on the DEVICE: stratified over the integer prefix of the faces'
    areas, the face by binary search, folded barycentrics from a counter-based hash of (seed, sample, stream) -- a pure function of
    (verts, faces, n, seed, box), no generator state.  seed: an int in [0, 2^32).  The box lo / scale (by default smooth_box(m.verts))
    only fixes the weights' fixed point.  Returns (points [n, 3] fp32, face [n] int32) on the device; a mesh without area raises
    ValueError (one host read of the total weight).  The exact rules are in include/nerf_hip.h.  A CPU tensor raises: there is no CPU
    path."""
    from . import ops

    verts, faces = _on_device(m.verts, "sample_surface"), torch.as_tensor(m.faces)
    if int(n) != n or int(n) < 0 or int(n) >= 2 ** 31:
        raise ValueError(f"n={n!r}: an int in [0, 2^31)")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"seed={seed!r}: an int in [0, 2^32)")
    lo, scale = smooth_box(verts, lo, scale)
    _check_box(lo, scale)
    points, face, info = ops.mesh_sample(verts, faces, int(n), int(seed), lo.tolist(), float(scale))
    W = int(info.cpu())
    if W <= 0:
        raise ValueError(f"sample_surface: the mesh has no area to sample (V={int(verts.shape[0])} F={int(faces.shape[0])}, total weight {W})")
    return points, face


def _cloud_box(p):
    """-> (lo [3], hi [3] fp32 numpy over the finite rows, their number): one host read"""
    v = torch.as_tensor(p).to(torch.float32).reshape(-1, 3)
    if v.shape[0] == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32), 0
    ok = torch.isfinite(v).all(1, keepdim=True)
    inf = torch.full_like(v, float("inf"))
    host = torch.cat((torch.where(ok, v, inf).amin(0).double(), torch.where(ok, v, -inf).amax(0).double(), ok.sum().double().reshape(1)))
    host = host.cpu().numpy()
    m = int(host[6])
    if m == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32), 0
    return host[0:3].astype(np.float32), host[3:6].astype(np.float32), m


def grid_rule(lo, hi, m):
    """The sizing rule of nearest()'s grid (include/nerf_hip.h): (lo [3] fp32, cell fp32, dims (3 ints)) from the finite reference
    points' box lo / hi and their number m: about one point per cell, at most 2 m + 8 cells, one cell along an axis of zero extent."""
    lo = np.asarray(lo, np.float32).reshape(3)
    ext = np.asarray(hi, np.float32).reshape(3).astype(np.float64) - lo.astype(np.float64)
    pos = ext > 0
    if m <= 0 or not pos.any():
        return lo, np.float32(1.0), (1, 1, 1)
    with np.errstate(all="ignore"):
        cell = np.float32((np.prod(ext[pos]) / m) ** (1.0 / int(pos.sum())))
    top = np.float32(2.0 ** 127)
    if not cell >= np.float32(2.0 ** -126):
        cell = np.float32(2.0 ** -126)
    cell = min(cell, top)
    while True:
        dims = tuple(int(np.floor(e / np.float64(cell))) + 1 if e > 0 else 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= 2 * m + 8:
            return lo, np.float32(cell), dims
        if cell >= top:
            return lo, np.float32(cell), (1, 1, 1)
        cell = np.float32(cell * np.float32(2.0))


def nearest_grid(ref):
    """grid_rule over the finite rows of ref [M, 3] (one host read of their minimum, maximum and number) -> (lo, cell, dims)."""
    return grid_rule(*_cloud_box(ref))


def nearest(ref, query, grid=None, sort_queries=False):
    """The exact nearest reference point of every query on the DEVICE: ref [M, 3], query [N, 3] fp32 -> (idx [N] int32, dist2 [N] fp64),
    dist2 the fp64 squared distance to the nearest ref row with three finite coordinates and idx the LOWEST index that attains it;
    idx -1 and dist2 +inf for a query that is not finite, and for every query when no ref row is finite.  That is the brute-force
    result bit for bit; a uniform grid over ref (grid = (lo, cell, dims), by default nearest_grid(ref)) only accelerates it, and
    sort_queries (process the queries in cell order, scatter the results back; off by default: measured no faster, DESIGN.md
    section 3h-7) changes the speed alone.  The exact rules are in
    include/nerf_hip.h.  CPU tensors raise: there is no CPU path."""
    from . import ops

    ref, query = _on_device(ref, "nearest"), _on_device(query, "nearest")
    lo, cell, dims = nearest_grid(ref) if grid is None else grid
    lo = np.asarray(lo, np.float32).reshape(3)
    ws, _ = ops.points_grid(ref, lo.tolist(), float(cell), dims, n_query=int(query.shape[0]))
    return ops.points_nearest(query, int(ref.shape[0]), lo.tolist(), float(cell), dims, ws, sort_queries=sort_queries)


DIST_ONE = float(2 ** 30)


def stats_from_raw(raw, unit, n):
    """The host's reading of nerf_hip_distance_stats' int64s for n distances in units of `unit` -> dict(mean, rms, count, total,
    clamped, within [K])."""
    raw = [int(x) for x in raw]
    c = raw[0]
    mean = raw[1] / (c * DIST_ONE) * unit if c else float("nan")
    rms = float(np.sqrt(raw[2] / (c * DIST_ONE))) * unit if c else float("nan")
    return dict(mean=mean, rms=rms, count=c, total=int(n), clamped=raw[3], within=raw[4:])


def chamfer(a, b, thresholds=(), unit=None):
    """Chamfer distance and F-scores between two point clouds a [Na, 3] and b [Nb, 3] on the DEVICE: nearest() both ways, then the
    distances' statistics as exact integer sums (nerf_hip_distance_stats), so the result is a pure function of the input.  unit: the
    fixed point's unit, by default pow2_at_least(the two clouds' joint extent) -- then no distance reaches the clamp at 8 units; a
    non-zero ``clamped`` count in the result says the means are lower bounds.  thresholds: up to 8 distances tau.  Returns a dict:
    a_to_b / b_to_a = dict(mean, rms, count, total, clamped, within) (count: the finite distances among total), chamfer = the mean of
    the two means, thresholds, and per threshold precision (the share of a within tau of b), recall (of b within tau of a) and fscore
    (their harmonic mean), clamped, unit.  a is the cloud under test, b the ground truth.  CPU tensors raise: there is no CPU path."""
    from . import ops

    a, b = _on_device(a, "chamfer"), _on_device(b, "chamfer")
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > 8 or any(not np.isfinite(t) or t < 0 for t in thresholds):
        raise ValueError(f"thresholds={thresholds!r}: at most 8 finite distances >= 0")
    box_a, box_b = _cloud_box(a), _cloud_box(b)
    if unit is None:
        both = [bx for bx in (box_a, box_b) if bx[2] > 0]
        ext = 1.0
        if both:
            with np.errstate(all="ignore"):
                ext = (np.max([bx[1] for bx in both], axis=0) - np.min([bx[0] for bx in both], axis=0)).astype(np.float32).max()
        unit = float(pow2_at_least(ext))
    unit = float(unit)
    if not np.isfinite(unit) or not unit > 0 or not np.isfinite(unit * unit) or not unit * unit > 0:
        raise ValueError(f"unit={unit!r}: must be finite and > 0, its square as well")
    _, d_ab = nearest(b, a, grid=grid_rule(*box_b))
    _, d_ba = nearest(a, b, grid=grid_rule(*box_a))
    raw = torch.cat((ops.distance_stats(d_ab, unit, thresholds), ops.distance_stats(d_ba, unit, thresholds))).cpu().tolist()  # (one read)
    k = 4 + len(thresholds)
    ab, ba = stats_from_raw(raw[:k], unit, d_ab.shape[0]), stats_from_raw(raw[k:], unit, d_ba.shape[0])
    frac = lambda s: [w / s["total"] if s["total"] else float("nan") for w in s["within"]]
    prec, rec = frac(ab), frac(ba)
    fs = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)]
    return dict(a_to_b=ab, b_to_a=ba, chamfer=0.5 * (ab["mean"] + ba["mean"]), thresholds=list(thresholds), precision=prec, recall=rec,
                fscore=fs, clamped=ab["clamped"] + ba["clamped"], unit=unit)


def compare(m_a, m_b, n=200_000, seed=0, thresholds=()):
    """The geometric distance between two meshes on the DEVICE: n area-weighted samples of each (sample_surface with seeds seed and
    seed + 1), chamfer(samples of m_a, samples of m_b, thresholds) and both meshes' measure() as measure_a / measure_b.  m_a is the
    mesh under test (precision), m_b the ground truth (recall).  A mesh without area raises ValueError."""
    pa, _ = sample_surface(m_a, n, seed)
    pb, _ = sample_surface(m_b, n, (int(seed) + 1) & 0xFFFFFFFF)
    out = chamfer(pa, pb, thresholds)
    out.update(samples=int(n), seed=int(seed), measure_a=measure(m_a), measure_b=measure(m_b))
    return out


class Raycaster(NamedTuple):
    verts: object    # [V, 3] fp32 (device): the mesh the grid was built over
    faces: object    # [F, 3] int32
    lo: object       # [3] fp32 numpy: the grid's corner
    cell: object     # fp32: its one cell size
    dims: tuple      # (3 ints): its cells per axis
    entries: int     # E: the (face, cell) pairs of the INSIDE faces
    taking_part: int  # faces with indices in range and finite corners
    outside: int     # faces that reach out of the grid: every ray tests them in full
    ws: object       # the device workspace that holds the grid


def raycast_grid(verts, faces, count=None):
    """The sizing rule of build_raycast()'s triangle grid -> (lo [3] fp32, cell fp32, dims (3 ints)): grid_rule over the finite vertices'
    box, grown by 2^-19 of its largest |coordinate| on every side, with m = F (about one cell per face), the cell doubled while the
    entries E -- the sum over the faces of the cells their boxes touch -- exceed 4 F + 64.  With this box no face with finite
    corners is OUTSIDE (the growth covers the 2^-20 by which the hit rule widens a face's box).  count(lo, cell, dims) -> E; by default the device's count
    call (nerf_hip_mesh_raycast_grid_count: one 24-byte read per attempt), for which CPU tensors raise."""
    from . import ops

    verts, faces = torch.as_tensor(verts), torch.as_tensor(faces)
    if count is None:
        _on_device(verts, "raycast_grid")
        count = lambda lo, cell, dims: int(ops.mesh_raycast_count(verts, faces, lo.tolist(), float(cell), dims).cpu()[1])
    blo, bhi, n = _cloud_box(verts)
    F = int(faces.shape[0])
    # the box grows by 2^-19 of its largest |coordinate| on every side: more than the 2^-20 by which the hit rule widens a face's box
    pad = np.float32(2.0 ** -19) * np.float32(max(np.abs(blo).max(), np.abs(bhi).max()))
    blo, bhi = (blo - pad).astype(np.float32), (bhi + pad).astype(np.float32)
    lo, cell, dims = grid_rule(blo, bhi, F if n > 0 else 0)
    ext = bhi.astype(np.float64) - blo.astype(np.float64)
    top = np.float32(2.0 ** 127)
    while F > 0 and n > 0 and cell < top and count(lo, cell, dims) > 4 * F + 64:
        cell = np.float32(cell * np.float32(2.0))
        dims = tuple(int(np.floor(e / np.float64(cell))) + 1 if e > 0 else 1 for e in ext)
    return lo, np.float32(cell), dims


def build_raycast(m, grid=None):
    """A Raycaster over the Mesh m (any indexed mesh) on the DEVICE: the faces entered in the cells of a uniform grid, grid = (lo, cell,
    dims) or by default raycast_grid(m.verts, m.faces).  The grid is an accelerator only: raycast() gives the brute-force answer over
    all faces for every grid (include/nerf_hip.h, rule G; the proof is at the top of csrc/mesh_raycast.hip).  One host read of the
    grid's sizes.  The mesh must not change while the Raycaster is used.  A CPU tensor raises: there is no CPU path."""
    from . import ops

    verts, faces = _on_device(m.verts, "build_raycast"), torch.as_tensor(m.faces)
    verts = verts.to(torch.float32).contiguous()
    faces = faces.contiguous()
    lo, cell, dims = raycast_grid(verts, faces) if grid is None else grid
    lo = np.asarray(lo, np.float32).reshape(3)
    dims = tuple(int(d) for d in dims)
    part, E, out = (int(x) for x in ops.mesh_raycast_count(verts, faces, lo.tolist(), float(cell), dims).cpu())
    if E >= 2 ** 31:
        raise ValueError(f"build_raycast: the grid {dims} of cell {float(cell)!r} has {E} entries, at most 2^31 - 1 (use larger cells)")
    ws = ops.mesh_raycast_fill(verts, faces, lo.tolist(), float(cell), dims, E)
    return Raycaster(verts, faces, lo, np.float32(cell), dims, E, part, out, ws)


def raycast(handle, origins, dirs, tmin=0.0, tmax=float("inf"), skip=None, any_hit=False):
    """Casts rays against a Raycaster's mesh on the DEVICE: origins, dirs [N, 3] fp32 (dirs need not be normalised: t is in units of
    dirs) -> (t [N] fp64, uv [N, 2] fp64, face [N] int32, side [N] int8): the closest hit with tmin <= t <= tmax, the lowest face
    index among equal t; its barycentrics (the point is (1 - u - v) A + u B + v C); side +1 where the ray meets the counter-clockwise
    (outer) side, -1 the other.  No hit, or a ray with a component that is not finite or dirs == 0: t = +inf, uv = 0, face = -1,
    side = 0.  skip: int32 [N], ray i ignores face skip[i].  any_hit=True -> occluded [N] uint8 alone (= face >= 0; the walk stops
    at the first hit).  The hit rule is Moeller-Trumbore in fp64 (include/nerf_hip.h, rule R), not a watertight test; every output
    is a pure function of the input.  CPU tensors raise: there is no CPU path."""
    from . import ops

    origins, dirs = _on_device(origins, "raycast"), _on_device(dirs, "raycast")
    if np.isnan(tmin) or np.isnan(tmax):
        raise ValueError(f"tmin={tmin!r} tmax={tmax!r}: the window's ends may be infinite, not NaN")
    h = handle
    return ops.mesh_raycast(h.verts, h.faces, h.lo.tolist(), float(h.cell), h.dims, h.entries, h.ws, origins, dirs, tmin, tmax,
                            None if skip is None else torch.as_tensor(skip).to(h.faces.device), any_hit)


def camera_q(pose17, K_inv):
    """-> (Q [3, 3] fp64 numpy, cam_o [3] fp32 numpy) of one camera: with the project's ray rule (pixel (x, y), x the row: p_j =
    (x K[j] + y K[3 + j]) + K[6 + j] over the nine entries K of K_inv, world direction R p), Q = inverse(R K^T) maps a world direction to
    homogeneous pixel coordinates; cam_o is the pose's translation."""
    pb = np.asarray(torch.as_tensor(pose17).detach().cpu().numpy(), np.float32).reshape(17)
    K = np.asarray(torch.as_tensor(K_inv).detach().cpu().numpy(), np.float32).reshape(3, 3).astype(np.float64)
    P = pb[:15].reshape(3, 5)
    return np.linalg.inv(P[:, :3].astype(np.float64) @ K.T), P[:, 3].copy()


def camera_rays(poses_bound17, K_inv, H, W, device=None):
    """The rays of every pixel of the cameras poses_bound17 [n, 17] (or [17]) through the project's own ray kernel (ops.rays) ->
    (origins [n * H * W, 3], dirs [n * H * W, 3] fp32 on the device), pixel (row x, column y) of camera c at index (c * H + x) * W + y:
    the origin is the pose's translation and the direction the unit d_wrd the renderer marches along, so t of raycast() is on the
    scale of render(maps=True)'s depth."""
    from . import ops

    pb = torch.as_tensor(poses_bound17)
    dev = torch.device(device) if device is not None else (pb.device if pb.device.type == "cuda" else torch.device("cuda"))
    pb = pb.to(dev, torch.float32).reshape(-1, 17)
    n, H, W = int(pb.shape[0]), int(H), int(W)
    if n * H * W == 0:
        return torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev)
    row = torch.arange(H, device=dev).repeat_interleave(W).repeat(n)
    col = torch.arange(W, device=dev).repeat(n * H)
    per = pb.repeat_interleave(H * W, dim=0).contiguous()
    _, d_wrd, _ = ops.rays(row, col, per, torch.as_tensor(K_inv), 2)
    return per.view(-1, 17)[:, :15].reshape(-1, 3, 5)[:, :, 3].contiguous(), d_wrd


def render_depth(handle, poses_bound17, K_inv, H, W):
    """The mesh seen from the cameras poses_bound17 [n, 17]: raycast(handle, *camera_rays(...)) as images -> (t [n, H, W] fp64 -- +inf
    where the pixel's ray meets no face --, face [n, H, W] int32, uv [n, H, W, 2] fp64): the mesh's depth along the rays whose expected
    depth render(maps=True) gives."""
    o, d = camera_rays(poses_bound17, K_inv, H, W, device=handle.faces.device)
    t, uv, face, _ = raycast(handle, o, d)
    n = o.shape[0] // max(int(H) * int(W), 1)
    return t.view(n, H, W), face.view(n, H, W), uv.view(n, H, W, 2)


def visibility(m, poses_bound, K_inv, H, W, tmin=1e-4):
    """Which faces of the Mesh m does some camera see?  On the DEVICE, per camera of poses_bound [n, 17] with the H x W image of K_inv:
    a face is VALID iff it takes part, faces the camera (its counter-clockwise side) and its centroid projects into the image; a
    valid face is SEEN iff the segment from its centroid to the camera, over t in [tmin, 1] of the segment, meets no other face (an
    any-hit cast with the face itself skipped).  tmin keeps the segment off the surface it starts on: the default 1e-4 of the segment
    is a choice, not a measurement.  One shadow ray per face and camera -- the centroid stands for the face; pixel-ray visibility is
    not built.  Returns (seen [F] bool on the device, per-camera counts of seen faces as a list of ints: one host read).  The exact
    rules are in include/nerf_hip.h (rules V and R).  A CPU tensor raises: there is no CPU path."""
    from . import ops

    verts, faces = _on_device(m.verts, "visibility"), torch.as_tensor(m.faces)
    pb = torch.as_tensor(poses_bound).detach().cpu().reshape(-1, 17)
    h = build_raycast(Mesh(verts, faces, None, None))
    F = int(faces.shape[0])
    own = torch.arange(F, dtype=torch.int32, device=h.faces.device)
    seen = torch.zeros(F, dtype=torch.bool, device=h.faces.device)
    counts = []
    for c in range(pb.shape[0]):
        Q, cam = camera_q(pb[c], K_inv)
        orig, dirs, valid = ops.mesh_face_rays(h.verts, h.faces, cam.tolist(), Q.reshape(-1).tolist(), H, W)
        vis = (valid != 0) & (raycast(h, orig, dirs, tmin, 1.0, skip=own, any_hit=True) == 0)
        seen |= vis
        counts.append(vis.sum())
    counts = torch.stack(counts).cpu().tolist() if counts else []
    return seen, counts


def filter_faces(m, keep):
    """The Mesh m restricted to the faces with keep[f] true (device compaction): kept faces and the vertices they use -- with their
    normals and rgb where m has them -- stay in their order, face indices are renumbered, faces with an index outside [0, V) go.
    One host read of the new sizes.  A CPU tensor raises: there is no CPU path."""
    from . import ops

    verts = _on_device(m.verts, "filter_faces")
    keep = torch.as_tensor(keep).to(verts.device) != 0
    return Mesh(*ops.mesh_select_faces(verts, torch.as_tensor(m.faces), m.normals, m.rgb, keep))


def tsdf_volume(shape, device):
    """A zeroed TSDF state (T, Wt): two fp32 [nx, ny, nz] volumes on ``device`` -- the truncated signed distance, in units of the
    truncation distance, and the number of observations of every lattice point -- for tsdf_integrate."""
    from .nerf import grid_shape

    shape = grid_shape(shape)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("tsdf_volume: the volumes live on a ROCm device (MI355X); there is no CPU path")
    return torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.float32, device=dev)


def tsdf_color_volume(shape, device):
    """A zeroed colour state C beside tsdf_volume's (T, Wt): fp32 [nx, ny, nz, 4] on ``device`` -- per lattice point the mean colour
    (R, G, B) of its colour observations and their number Wc -- for tsdf_integrate(rgb=, color=) and tsdf_sample_color."""
    from .nerf import grid_shape

    shape = grid_shape(shape)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("tsdf_color_volume: the volume lives on a ROCm device (MI355X); there is no CPU path")
    return torch.zeros(shape + (4,), dtype=torch.float32, device=dev)


def tsdf_trunc(step):
    """The default truncation distance of a lattice of fp32 ``step`` [3]: 4 x its largest step (a choice, not a measurement)."""
    return 4.0 * float(np.asarray(step, dtype=np.float32).reshape(3).max())


def tsdf_integrate(T, Wt, lo, step, depth, poses_bound17, K_inv, opacity=None, trunc=None, min_opacity=0.5, carve=True, rgb=None, color=None):
    """Integrates depth images into the TSDF state (T, Wt) IN PLACE on the DEVICE and returns it.  T, Wt: tsdf_volume's pair over the
    lattice lo + (i, j, k) * step (the density grid's: pass its lo and fp32 step).  depth [n, H, W] fp32: per pixel (row x, column y) of
    camera c the distance to the surface along the UNIT ray the renderer marches along -- render(maps=True)'s D / A, raycast()'s t over
    camera_rays(); +inf, NaN or <= 0: the pixel saw no surface.  poses_bound17 [n, 17] and K_inv: the cameras, as everywhere (camera_q
    forms each view's Q and position).  opacity [n, H, W] or None: a pixel with opacity < min_opacity is background; with carve it
    then marks every lattice point along its ray as empty, without carve it says nothing.  trunc: the truncation distance in world
    units, by default tsdf_trunc(step).  Every lattice point within trunc behind a view's surface, or in front of it, averages
    min(1, (depth - distance to the camera) / trunc) into T and counts 1 into Wt; the exact rule is T of include/nerf_hip.h and the
    result does not depend on how the views are split over calls.
    rgb / color: both None (nothing more happens), or rgb [n, H, W, 3] fp32 -- the colour each view shows at each pixel -- and color,
    tsdf_color_volume's C over the same lattice: the colours are fused IN PLACE beside the same geometry update (rule TC of
    include/nerf_hip.h) and (T, Wt, C) is returned.  A view gives a lattice point its pixel's colour only where the point lies within
    trunc of that view's surface, on either side; carved space and space far in front of the surface get none, nor does a pixel whose
    colour is not finite.  C[..., :3] is the mean of those colours and C[..., 3] their number.  CPU tensors raise: there is no CPU
    path."""
    from . import ops

    if (rgb is None) != (color is None):
        raise ValueError("tsdf_integrate: rgb and color are both given or both None")
    T, Wt = _on_device(T, "tsdf_integrate"), _on_device(Wt, "tsdf_integrate")
    depth = torch.as_tensor(depth)
    if depth.dim() != 3:
        raise ValueError(f"depth {tuple(depth.shape)}: [n, H, W]")
    pb = poses_bound17 if torch.is_tensor(poses_bound17) else torch.from_numpy(np.array(poses_bound17))  # (np.array: a writable copy)
    pb = pb.detach().cpu().reshape(-1, 17)
    if pb.shape[0] != depth.shape[0]:
        raise ValueError(f"{pb.shape[0]} poses for {depth.shape[0]} depth images")
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    step32 = np.asarray(step, dtype=np.float32).reshape(3)
    cams = [camera_q(pb[c], K_inv) for c in range(pb.shape[0])]
    args = (T, Wt, lo32.tolist(), step32.tolist(), depth, opacity, [cam.tolist() for _, cam in cams], [Q.reshape(-1).tolist() for Q, _ in cams],
            tsdf_trunc(step32) if trunc is None else float(trunc), min_opacity, carve)
    if color is None:
        ops.tsdf_integrate(*args)
        return T, Wt
    color = _on_device(color, "tsdf_integrate")
    ops.tsdf_integrate(*args, rgb=_on_device(rgb, "tsdf_integrate"), color=color)
    return T, Wt, color


def tsdf_sample_color(C, lo, step, points):
    """The fused colours at arbitrary points, on the DEVICE: C = tsdf_color_volume's state over the lattice lo + (i, j, k) * step,
    points [M, 3] -> (rgb [M, 3] fp32, valid [M] bool).  Trilinear interpolation over the corners of the point's cell that have a colour
    (Wc > 0), renormalised by their weights; valid is False, and rgb 0, where none of the eight has one or a coordinate is not finite.
    A point outside the lattice takes the colour at the box's nearest face.  The exact rule is S of include/nerf_hip.h.  CPU tensors
    raise: there is no CPU path."""
    from . import ops

    C, points = _on_device(C, "tsdf_sample_color"), _on_device(points, "tsdf_sample_color")
    lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
    step32 = np.asarray(step, dtype=np.float32).reshape(3)
    rgb, valid = ops.tsdf_sample_color(C, lo32.tolist(), step32.tolist(), points)
    return rgb, valid != 0


def tsdf_grid(T, Wt, unseen="solid"):
    """The array marching_cubes(..., level=0.0) takes from a TSDF state: -T where Wt > 0 (marching cubes' inside is value > level, so
    the negation keeps inside = behind the surface and the grid normals pointing outward); where no view observed the point, +1 for
    unseen="solid" (unseen space is inside: the mesh closes behind what the cameras saw) or -1 for unseen="empty"."""
    if unseen not in ("solid", "empty"):
        raise ValueError(f"unseen={unseen!r}: 'solid' or 'empty'")
    T = torch.as_tensor(T)
    return torch.where(torch.as_tensor(Wt) > 0, -T, torch.full_like(T, 1.0 if unseen == "solid" else -1.0))


class Texture(NamedTuple):
    image: object    # [H, W, 3] fp32 (device): the baked atlas, row y from the top; 0 where mask is False
    mask: object     # [H, W] bool: the texels some face owns
    chart: int       # n: the chart edge in texels
    faces: int       # F: the face count the atlas was laid out for
    uv: object       # [F, 3, 2] fp32 (device): per face and corner (x / W, y / H), y pointing down


ATLAS_PAD = 5  # a cell is chart + 5 texels wide (rule TA of include/nerf_hip.h)


def atlas_dims(F, chart):
    """The sizes of rule TA's atlas (include/nerf_hip.h) for F faces with charts of ``chart`` texels -> (c, Sx, Sy, W, H) as ints: the
    cell edge c = chart + 5, the cells per row and column, and the W x H texels.  Two faces share a cell, the cells fill the rows of
    the smallest square that holds them; F = 0 gives a 0 x 0 atlas.  Integer arithmetic only.  ValueError for chart < 2, F < 0,
    3 F >= 2^31 or W * H >= 2^31 (what nerf_hip_mesh_atlas_dims refuses)."""
    import math

    if int(F) != F or int(chart) != chart:
        raise ValueError(f"F={F!r} chart={chart!r}: two ints")
    F, n = int(F), int(chart)
    if n < 2:
        raise ValueError(f"chart={n}: a chart has at least 2 texels along its edge")
    if F < 0 or 3 * F >= 2 ** 31:
        raise ValueError(f"F={F}: 0 <= 3 F < 2^31")
    c, K = n + ATLAS_PAD, (F + 1) // 2
    Sx = math.isqrt(K)
    Sx += Sx * Sx < K
    Sy = -(-K // Sx) if Sx else 0
    if Sx * c * Sy * c >= 2 ** 31:
        raise ValueError(f"F={F} chart={n}: the atlas of {Sx * c} x {Sy * c} texels must stay below 2^31 texels")
    return c, Sx, Sy, Sx * c, Sy * c


def atlas_chart(F, size):
    """The largest chart n >= 2 whose atlas for F faces is at most ``size`` texels wide (and so at most as high): Sx * (n + 5) <= size.
    ValueError where even n = 2 does not fit, or F = 0."""
    Sx = atlas_dims(F, 2)[1]
    n = int(size) // Sx - ATLAS_PAD if Sx else 0
    if n < 2:
        raise ValueError(f"size={size!r}: the atlas of F={int(F)} faces needs at least {Sx * (2 + ATLAS_PAD)} texels along its edge (and F > 0)")
    atlas_dims(F, n)
    return n


def atlas_uv(F, chart, device):
    """Rule TA's UV table [F, 3, 2] fp32 on ``device``: per face and corner (x / W, y / H) of the chart's corners A, B, C in the atlas,
    y pointing down -- the half-integer texel coordinates as fp32, one correctly rounded division each (formed in fp64 from the two
    fp32 operands, which rounds to the same fp32)."""
    c, Sx, _, W, H = atlas_dims(F, chart)
    n = int(chart)
    f = torch.arange(int(F), device=device)
    k = f >> 1
    upper = (f & 1).view(-1, 1).double()
    local = torch.tensor([[1.5, 1.5], [1.5 + n, 1.5], [1.5, 1.5 + n]], dtype=torch.float64, device=device)  # A, B, C of a lower chart
    x = local[:, 0].view(1, 3) * (1 - 2 * upper) + upper * c + ((k % max(Sx, 1)) * c).view(-1, 1).double()  # (an upper chart's are c - these)
    y = local[:, 1].view(1, 3) * (1 - 2 * upper) + upper * c + ((k // max(Sx, 1)) * c).view(-1, 1).double()
    size = torch.tensor([max(W, 1), max(H, 1)], dtype=torch.float32, device=device).double()
    return (torch.stack((x, y), dim=2).float().double() / size).float()


def atlas_texels(m, chart, row0=0, rows=None):
    """The surface point and the viewing direction of every texel of the rows [row0, row0 + rows) (default: to the last row) of the
    Mesh m's atlas with charts of ``chart`` texels, on the DEVICE -> (points [rows, W, 3], dirs [rows, W, 3] fp32, mask [rows, W]
    bool).  A texel's point is the barycentric blend of its face's corners and its direction the negated, normalised blend of their
    normals (m.normals is required): what extract_mesh asks the field for at a vertex, at every texel.  mask is False, and both are
    0, for the texels no face owns and for faces with an index outside [0, V).  The exact rule is TA of include/nerf_hip.h; identical
    bits from run to run.  A CPU tensor raises: there is no CPU path."""
    from . import ops

    verts, faces = _on_device(m.verts, "atlas_texels"), torch.as_tensor(m.faces)
    if m.normals is None:
        raise ValueError("atlas_texels: the mesh needs vertex normals (the texels' viewing directions)")
    _, _, _, W, H = atlas_dims(faces.shape[0], chart)
    rows = H - int(row0) if rows is None else int(rows)
    if int(row0) < 0 or rows < 0 or int(row0) + rows > H:
        raise ValueError(f"row0={row0!r} rows={rows!r}: a band of the atlas's {H} rows")
    p, d, k = ops.mesh_atlas_texels(verts, torch.as_tensor(m.normals), faces, int(chart), int(row0), rows)
    return p.view(rows, W, 3), d.view(rows, W, 3), k.view(rows, W) != 0


def bake_texture(m, chart, shade, rows_per_call=None):
    """Bakes a texture atlas for the Mesh m on the DEVICE: shade(points [T, 3], dirs [T, 3]) -> rgb [T, 3] is called on the texels of
    atlas_texels(m, chart), a band of rows_per_call atlas rows at a time (default: about 2^20 texels), so no more than one band's
    points and directions exist at once; the result does not depend on rows_per_call.  Returns a Texture: the image (0 where no face
    owns the texel), the mask, the chart, the face count and the UV table.  Every face gets the same chart -- a sliver as many texels as
    a large face; simplify the mesh first (simplify= of extract_mesh) to make the faces more uniform.  shade sees the unowned
    texels too (point 0, direction 0); their result is dropped."""
    verts, faces = _on_device(m.verts, "bake_texture"), torch.as_tensor(m.faces)
    F = int(faces.shape[0])
    _, _, _, W, H = atlas_dims(F, chart)
    per = max(1, (1 << 20) // max(W, 1)) if rows_per_call is None else int(rows_per_call)
    if per < 1:
        raise ValueError(f"rows_per_call={rows_per_call!r}: None or an int >= 1")
    image = torch.zeros(H, W, 3, device=verts.device)
    mask = torch.zeros(H, W, dtype=torch.bool, device=verts.device)
    for r0 in range(0, H, per):
        r = min(per, H - r0)
        p, d, k = atlas_texels(m, chart, r0, r)
        rgb = torch.as_tensor(shade(p.view(-1, 3), d.view(-1, 3))).view(r, W, 3)
        image[r0:r0 + r] = torch.where(k[..., None], rgb, torch.zeros_like(rgb))
        mask[r0:r0 + r] = k
    return Texture(image, mask, int(chart), F, atlas_uv(F, chart, verts.device))


def sample_texture(tex, face, uv, background=(0.0, 0.0, 0.0)):
    """The Texture tex looked up at (face [N] int32, uv [N, 2] fp64) -- raycast()'s face and barycentrics: the point is
    (1 - u - v) A + u B + v C -- on the DEVICE -> (rgb [N, 3] fp32, valid [N] bool): bilinear over the four texels of the face's chart
    around the point, in fp64, (u, v) clamped into the triangle; ``background`` and valid False for face < 0, face >= tex.faces or a
    uv that is not finite.  A lookup touches only texels its own face owns, and at a corner returns the corner texel's bits.  The
    exact rule is TX of include/nerf_hip.h.  CPU tensors raise: there is no CPU path."""
    from . import ops

    image, face = _on_device(tex.image, "sample_texture"), _on_device(face, "sample_texture")
    rgb, valid = ops.mesh_texture_sample(image, tex.faces, tex.chart, face.reshape(-1), torch.as_tensor(uv).reshape(-1, 2), background)
    return rgb, valid != 0


def render_texture(handle, tex, poses_bound17, K_inv, H, W, background=(0.0, 0.0, 0.0)):
    """The textured mesh seen from the cameras poses_bound17 [n, 17] along the renderer's own rays: camera_rays -> raycast(handle) ->
    sample_texture(tex) -> (rgb [n, H, W, 3] fp32, hit [n, H, W] bool), ``background`` where a pixel's ray meets no face.  handle: a
    build_raycast of the mesh tex was baked for.  The images feed metrics.image_metrics as they are."""
    _, face, uv = render_depth(handle, poses_bound17, K_inv, H, W)
    rgb, valid = sample_texture(tex, face.reshape(-1), uv.reshape(-1, 2), background)
    return rgb.view(*face.shape, 3), valid.view(face.shape)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def png_bytes(rgb8):
    """An 8-bit RGB PNG of rgb8 [H, W, 3] uint8, top row first: one IDAT chunk, filter 0 on every row, the standard library's zlib."""
    import struct
    import zlib

    img = np.ascontiguousarray(rgb8, dtype=np.uint8)
    H, W = img.shape[:2]
    raw = np.concatenate((np.zeros((H, 1), np.uint8), img.reshape(H, W * 3)), axis=1).tobytes()
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6))
            + chunk(b"IEND", b""))


def write_obj(path, m, tex):
    """The Mesh m with the Texture tex as a Wavefront OBJ: ``path`` (.obj) with ``v`` / ``vn`` / ``vt`` lines -- 3 F ``vt`` entries, face f's
    corners at 3 f + 1 .. 3 f + 3, as (x, 1 - y): OBJ's v points up --, ``f a/ta/na`` faces (1-based), ``mtllib`` / ``usemtl``; beside it
    <stem>.mtl with ``map_Kd <stem>.png`` and <stem>.png, the atlas as 8-bit RGB (clip(rint(x * 255), 0, 255) as in write_ply, top row
    first; png_bytes).  Floats are written with 9 significant digits, which reads back to the same fp32.  An empty atlas (F = 0) is
    written as a 1 x 1 black image.  Returns the three paths."""
    import os

    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    v = _np(m.verts).astype(np.float32).reshape(-1, 3)
    f = _np(m.faces).astype(np.int64).reshape(-1, 3)
    vn = None if m.normals is None else _np(m.normals).astype(np.float32).reshape(-1, 3)
    uv = _np(tex.uv).astype(np.float32).reshape(-1, 2)
    if len(uv) != 3 * len(f) or tex.faces != len(f):
        raise ValueError(f"the texture was laid out for {tex.faces} faces, the mesh has {len(f)}")
    img = np.clip(np.rint(_np(tex.image).astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    if img.size == 0:
        img = np.zeros((1, 1, 3), np.uint8)
    g = lambda x: np.format_float_positional(x, precision=9, unique=True, trim="0") if np.isfinite(x) else repr(float(x))
    lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
    lines += [f"v {g(p[0])} {g(p[1])} {g(p[2])}" for p in v]
    if vn is not None:
        lines += [f"vn {g(p[0])} {g(p[1])} {g(p[2])}" for p in vn]
    lines += [f"vt {g(t[0])} {g(np.float32(1.0) - t[1])}" for t in uv]
    for k, (a, b, c) in enumerate(f + 1):
        t = 3 * k + 1
        lines.append(f"f {a}/{t}/{a} {b}/{t + 1}/{b} {c}/{t + 2}/{c}" if vn is not None else f"f {a}/{t} {b}/{t + 1} {c}/{t + 2}")
    with open(stem + ".obj", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w") as fh:
        fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    with open(stem + ".png", "wb") as fh:
        fh.write(png_bytes(img))
    return stem + ".obj", stem + ".mtl", stem + ".png"


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


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """Reads a triangle mesh from a PLY 1.0 file, ASCII or binary little-endian: what write_ply writes, and any file whose ``vertex``
    element carries scalar properties with ``x y z`` among them (others are skipped by their declared sizes) followed by a ``face``
    element of one list property of 3 indices each.  Returns (verts [V, 3] fp32, faces [F, 3] int32, normals [V, 3] fp32 or None --
    ``nx ny nz`` --, rgb [V, 3] uint8 or None -- uchar ``red green blue``, as stored: divide by 255 for floats) as numpy arrays.
    Anything else raises ValueError naming the offending header line; faces that are not triangles are refused, not triangulated."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    nl = data.find(b"\n", end) if end >= 0 else -1
    if not data.startswith(b"ply") or nl < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header' header)")
    try:
        lines = [ln.strip() for ln in data[:nl].decode("ascii").splitlines()]
    except UnicodeDecodeError:
        raise ValueError(f"{path}: the PLY header is not ASCII") from None
    body = data[nl + 1:]
    if lines[0] != "ply" or lines[-1] != "end_header":
        raise ValueError(f"{path}: unsupported PLY header line {lines[0] if lines[0] != 'ply' else lines[-1]!r}")
    fmt, elems = None, []  # elems: [name, count, properties]
    for ln in lines[1:-1]:
        tok = ln.split()
        bad = ValueError(f"{path}: unsupported PLY header line {ln!r}")
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if fmt is not None or len(tok) != 3 or tok[1] not in ("ascii", "binary_little_endian") or tok[2] != "1.0":
                raise bad
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit() or len(elems) >= 2 or tok[1] != ("vertex", "face")[len(elems)]:
                raise bad
            elems.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elems:
                raise bad
            if len(tok) == 3 and tok[1] in _PLY_TYPES and elems[-1][0] == "vertex":
                elems[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            elif (len(tok) == 5 and tok[1] == "list" and elems[-1][0] == "face" and not elems[-1][2] and tok[2] in _PLY_TYPES
                  and tok[3] in _PLY_TYPES and _PLY_TYPES[tok[2]][0] in "iu" and _PLY_TYPES[tok[3]][0] in "iu"):
                elems[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                raise bad
        else:
            raise bad
    if fmt is None:
        raise ValueError(f"{path}: the PLY header has no 'format' line")
    if len(elems) != 2 or not elems[1][2]:
        raise ValueError(f"{path}: the PLY header needs 'element vertex' and 'element face' with one list property")
    (_, V, vprops), (_, F, (flist,)) = elems
    names = [p[0] for p in vprops]
    if len(set(names)) != len(names) or any(k not in names for k in "xyz"):
        raise ValueError(f"{path}: the vertex element needs properties x, y and z, once each (it has {names})")
    if fmt == "ascii":
        tok = body.split()
        need = V * len(vprops)
        if len(tok) < need:
            raise ValueError(f"{path}: {len(tok)} values, the {V} vertices need {need}")
        try:
            table = np.array([float(t) for t in tok[:need]], dtype=np.float64).reshape(V, len(vprops))
            rest = np.array([int(t) for t in tok[need:]], dtype=np.int64)
        except ValueError:
            raise ValueError(f"{path}: a value of the body is not a number") from None
        vcol = {k: table[:, i].astype(t) for i, (k, t) in enumerate(vprops)}
        whole = min(len(rest) // 4, F)
        rows = rest[:whole * 4].reshape(whole, 4)
        counts, index = rows[:, 0], rows[:, 1:]
    else:
        vdt = np.dtype([(k, "<" + t) for k, t in vprops])
        fdt = np.dtype([("n", "<" + flist[1]), ("i", "<" + flist[2], (3,))])
        if len(body) < V * vdt.itemsize:
            raise ValueError(f"{path}: {len(body)} bytes, the {V} vertices need {V * vdt.itemsize}")
        vrec = np.frombuffer(body, dtype=vdt, count=V)
        vcol = {k: vrec[k] for k in names}
        fbody = body[V * vdt.itemsize:]
        whole = min(F, len(fbody) // fdt.itemsize)
        frec = np.frombuffer(fbody, dtype=fdt, count=whole)
        counts, index = frec["n"].astype(np.int64), frec["i"].astype(np.int64)
    if (counts != 3).any():  # (the first such face is where it says: every face before it had 3 indices)
        k = int(np.argmax(counts != 3))
        raise ValueError(f"{path}: face {k} has {int(counts[k])} indices: only triangles are supported")
    if whole < F:
        raise ValueError(f"{path}: the face list ends after {whole} of {F} triangles")
    if F and (index.min() < -2 ** 31 or index.max() >= 2 ** 31):
        raise ValueError(f"{path}: a face index does not fit int32")
    types = dict(vprops)
    col3 = lambda keys, dt: np.stack([vcol[k].astype(dt) for k in keys], axis=1).reshape(V, 3)
    verts = col3("xyz", np.float32)
    normals = col3(("nx", "ny", "nz"), np.float32) if all(k in vcol for k in ("nx", "ny", "nz")) else None
    rgb = col3(("red", "green", "blue"), np.uint8) if all(types.get(k) == "u1" for k in ("red", "green", "blue")) else None
    return verts, np.ascontiguousarray(index, dtype=np.int32).reshape(F, 3), normals, rgb
