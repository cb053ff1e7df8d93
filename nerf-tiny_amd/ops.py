"""Stage-level calls into libnerf_hip.so (one per row of the hot-path table), used by the parity tests."""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _k9(K_inv):
    return _abi.f32_array(K_inv.detach().to("cpu", torch.float32).reshape(-1).tolist())


def rays(row, col, poses_bound_f32, K_inv, Nc):
    """-> d_cam[B,3], d_wrd[B,3], t_coarse[B,Nc]"""
    B, dev = row.shape[0], row.device
    d_cam = torch.empty(B, 3, device=dev)
    d_wrd = torch.empty(B, 3, device=dev)
    t_c = torch.empty(B, Nc, device=dev)
    _abi.check(_abi.lib().nerf_hip_rays(row.data_ptr(), col.data_ptr(), poses_bound_f32.data_ptr(), _k9(K_inv), B, Nc,
                                        d_cam.data_ptr(), d_wrd.data_ptr(), t_c.data_ptr(), _stream(row)))
    return d_cam, d_wrd, t_c


def field(params, row, col, poses_bound_f32, K_inv, t, debug=False):
    """-> rgb[B,N,3], sigma[B,N] (+ pts[B,N,3], gamma_p[B,N,60] if debug)"""
    B, N = t.shape
    dev = t.device
    rgb = torch.empty(B, N, 3, device=dev)
    sigma = torch.empty(B, N, device=dev)
    pts = torch.empty(B, N, 3, device=dev) if debug else None
    gp = torch.empty(B, N, 60, device=dev) if debug else None
    n = _abi.ws_bytes(max(B, 2), max(N, 2), max(N, 2), 0)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_field(_abi.ptr_array(params), row.data_ptr(), col.data_ptr(), poses_bound_f32.data_ptr(),
                                         _k9(K_inv), t.contiguous().data_ptr(), B, N, rgb.data_ptr(), sigma.data_ptr(),
                                         pts.data_ptr() if debug else None, gp.data_ptr() if debug else None,
                                         ws.data_ptr(), ws.numel(), _stream(t)))
    return (rgb, sigma, pts, gp) if debug else (rgb, sigma)


def field_bf16(params, row, col, poses_bound_f32, K_inv, t):
    """field() with the bf16 MLP (NERF_HIP_BF16_MLP) -> rgb[B,N,3], sigma[B,N]"""
    B, N = t.shape
    dev = t.device
    rgb = torch.empty(B, N, 3, device=dev)
    sigma = torch.empty(B, N, device=dev)
    n = _abi.ws_bytes(max(B, 2), max(N, 2), max(N, 2), _abi.BF16_MLP)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_field_bf16(_abi.ptr_array(params), row.data_ptr(), col.data_ptr(), poses_bound_f32.data_ptr(),
                                              _k9(K_inv), t.contiguous().data_ptr(), B, N, rgb.data_ptr(), sigma.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream(t)))
    return rgb, sigma


def query(params, points, dirs=None, ws=None):
    """The field at explicit points (nerf_hip_query, exact fp32): points[M,3] (and unit world dirs[M,3]) on the device ->
    (rgb[M,3] or None, sigma[M]).  ws: a uint8 device buffer of >= _abi.query_ws_bytes(dirs is not None) bytes (allocated here if None)."""
    M, dev = points.shape[0], points.device
    with_rgb = dirs is not None
    points = points.to(torch.float32).contiguous()
    dirs = dirs.to(dev, torch.float32).contiguous() if with_rgb else None
    if with_rgb and dirs.shape != points.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and points {tuple(points.shape)} differ")
    sigma = torch.empty(M, device=dev)
    rgb = torch.empty(M, 3, device=dev) if with_rgb else None
    if ws is None:
        ws = torch.empty(_abi.query_ws_bytes(with_rgb), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_query(_abi.ptr_array(params), points.data_ptr(), dirs.data_ptr() if with_rgb else None, M,
                                         rgb.data_ptr() if with_rgb else None, sigma.data_ptr(), ws.data_ptr(), ws.numel(), _stream(points)))
    return rgb, sigma


def query_grad(params, points, dirs=None, dsigma=None, drgb=None, ws=None):
    """The field and its vector-Jacobian product with respect to the points (nerf_hip_query_grad, exact fp32): points[M,3] (and unit
    world dirs[M,3]) on the device; upstream dsigma[M] (None = ones: the gradient of sigma) and, only with dirs, drgb[M,3] (None = no
    colour term) -> (rgb[M,3] or None, sigma[M], dpoints[M,3]).  rgb and sigma are query()'s bits.  ws: a uint8 device buffer of
    >= _abi.query_grad_ws_bytes(dirs is not None) bytes (allocated here if None)."""
    M, dev = points.shape[0], points.device
    with_rgb = dirs is not None
    if drgb is not None and not with_rgb:
        raise ValueError("drgb needs dirs: without them no colour is computed")
    points = points.to(torch.float32).contiguous()
    dirs = dirs.to(dev, torch.float32).contiguous() if with_rgb else None
    if with_rgb and dirs.shape != points.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and points {tuple(points.shape)} differ")
    if dsigma is not None:
        dsigma = dsigma.to(dev, torch.float32).reshape(-1).contiguous()
        if dsigma.shape[0] != M:
            raise ValueError(f"dsigma has {dsigma.shape[0]} entries for {M} points")
    if drgb is not None:
        drgb = drgb.to(dev, torch.float32).contiguous()
        if drgb.shape != points.shape:
            raise ValueError(f"drgb {tuple(drgb.shape)} and points {tuple(points.shape)} differ")
    sigma = torch.empty(M, device=dev)
    rgb = torch.empty(M, 3, device=dev) if with_rgb else None
    dpoints = torch.empty(M, 3, device=dev)
    if ws is None:
        ws = torch.empty(_abi.query_grad_ws_bytes(with_rgb), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _abi.check(_abi.lib().nerf_hip_query_grad(_abi.ptr_array(params), points.data_ptr(), ptr(dirs), M, ptr(dsigma), ptr(drgb), ptr(rgb),
                                              sigma.data_ptr(), dpoints.data_ptr(), ws.data_ptr(), ws.numel(), _stream(points)))
    return rgb, sigma, dpoints


def density_grid(params, lo, step, shape, ws=None):
    """sigma at lo + (i, j, k) * step (nerf_hip_density_grid, exact fp32): lo / step three host floats, shape (nx, ny, nz) ->
    sigma[nx, ny, nz] on the parameters' device.  ws as in query() (sigma only)."""
    nx, ny, nz = (int(n) for n in shape)
    dev = params[0].device
    sigma = torch.empty(max(nx, 0), max(ny, 0), max(nz, 0), device=dev)
    if ws is None:
        ws = torch.empty(_abi.query_ws_bytes(False), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_density_grid(_abi.ptr_array(params), _abi.f32_array(lo), _abi.f32_array(step), nx, ny, nz,
                                                sigma.data_ptr(), ws.data_ptr(), ws.numel(), _stream(sigma)))
    return sigma


def density_band(params, lo, step, shape, level, block=8, ws=None, sigma=None, counts=None):
    """density_grid() with the field evaluated only in a band of ``block``^3-point blocks around the level set sigma == level
    (nerf_hip_band_begin, then nerf_hip_band_grow until the surface no longer leaves the band; include/nerf_hip.h states the rounds and
    what the band cannot see).  -> (sigma[nx, ny, nz], info): every evaluated value is density_grid's bits, the rest a fill value of
    the right class; info = dict(rounds, blocks_active, blocks_total, points_evaluated, points_total).  One 16-byte read of the device
    counts after the begin and after every round (each synchronises with the stream).  ws: a uint8 device buffer of
    >= _abi.band_ws_bytes(nx, ny, nz, block) bytes; sigma / counts: caller-owned outputs (fp32 [nx, ny, nz] contiguous / int64 [2]);
    each is allocated here if None."""
    nx, ny, nz = (int(n) for n in shape)
    block = int(block)
    dev = params[0].device
    L = _abi.lib()
    if ws is None:
        ws = torch.empty(_abi.band_ws_bytes(nx, ny, nz, block), dtype=torch.uint8, device=dev)
    if sigma is None:
        sigma = torch.empty(max(nx, 0), max(ny, 0), max(nz, 0), device=dev)
    if counts is None:
        counts = torch.empty(2, dtype=torch.int64, device=dev)
    st = _stream(sigma)
    head = (_abi.ptr_array(params), _abi.f32_array(lo), _abi.f32_array(step), nx, ny, nz, block, float(level))
    tail = (sigma.data_ptr(), ws.data_ptr(), ws.numel(), counts.data_ptr(), st)
    _abi.check(L.nerf_hip_band_begin(*head, *tail))
    r = min(block, max(nx, ny, nz, 2))
    corner_planes = lambda n: (n - 1 + r - 1) // r + 1
    info = dict(rounds=0, blocks_active=0, blocks_total=-(-nx // r) * -(-ny // r) * -(-nz // r),
                points_evaluated=corner_planes(nx) * corner_planes(ny) * corner_planes(nz), points_total=nx * ny * nz)
    while True:
        n_new, n_pts = (int(n) for n in counts.cpu())
        if n_new == 0:
            return sigma, info
        _abi.check(L.nerf_hip_band_grow(*head, n_new, *tail))
        info["rounds"] += 1
        info["blocks_active"] += n_new
        info["points_evaluated"] += n_pts


def marching_cubes(sigma, lo, step, level, ws=None, valid=None):
    """Isosurface sigma == level of a device grid sigma[nx, ny, nz] (nerf_hip_mesh_count + nerf_hip_mesh_emit): lo / step three host
    floats (lattice point (i, j, k) at lo + (i, j, k) * step) -> (verts[V, 3] fp32, faces[F, 3] int32, normals[V, 3] fp32) on sigma's
    device.  One count call, one 16-byte read of the counts (this synchronises with the stream), then the emit into buffers sized from
    them.  ws: a uint8 device buffer of >= _abi.mesh_ws_bytes(nx, ny, nz) bytes (allocated here if None).  valid: None, or a bool /
    uint8 device tensor of sigma's shape -- the masked calls (nerf_hip_mesh_count_masked + nerf_hip_mesh_emit_masked; rule M of
    include/nerf_hip.h): triangles only from cells whose eight corners are valid."""
    if sigma.dim() != 3:
        raise ValueError(f"sigma {tuple(sigma.shape)}: a [nx, ny, nz] grid")
    nx, ny, nz = (int(n) for n in sigma.shape)
    dev = sigma.device
    sigma = sigma.to(torch.float32).contiguous()
    if valid is not None:
        if valid.shape != sigma.shape or valid.device != dev or valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"valid {tuple(valid.shape)} {valid.dtype} on {valid.device}: a bool or uint8 tensor of sigma's shape {tuple(sigma.shape)} on {dev}")
        valid = valid.to(torch.uint8).contiguous()
    if ws is None:
        ws = torch.empty(_abi.mesh_ws_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    L, st = _abi.lib(), _stream(sigma)
    if valid is None:
        _abi.check(L.nerf_hip_mesh_count(sigma.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), ws.numel(), counts.data_ptr(), st))
    else:
        _abi.check(L.nerf_hip_mesh_count_masked(sigma.data_ptr(), valid.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), ws.numel(),
                                                counts.data_ptr(), st))
    V, F = (int(n) for n in counts.cpu())
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"the mesh has {V} vertices and {F} faces: int32 face indices hold fewer than 2^31 of either "
                         "(raise the level or lower the resolution)")
    verts = torch.empty(V, 3, device=dev)
    normals = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V == 0:
        return verts, faces, normals
    tail = (nx, ny, nz, _abi.f32_array(lo), _abi.f32_array(step), float(level), ws.data_ptr(), ws.numel(), verts.data_ptr(), normals.data_ptr(),
            faces.data_ptr(), V, F, st)
    if valid is None:
        _abi.check(L.nerf_hip_mesh_emit(sigma.data_ptr(), *tail))
    else:
        _abi.check(L.nerf_hip_mesh_emit_masked(sigma.data_ptr(), valid.data_ptr(), *tail))
    return verts, faces, normals


def _cc_faces(faces, num_verts):
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"faces {tuple(faces.shape)} {faces.dtype}: an int32 [F, 3] tensor")
    V = int(num_verts)
    if V < 0:
        raise ValueError(f"num_verts={V} < 0")
    return faces.contiguous(), V, int(faces.shape[0])


def mesh_components(faces, num_verts, verts=None, ws=None):
    """Connected components of the indexed mesh faces[F, 3] (int32, device) over num_verts vertices (nerf_hip_mesh_cc_round until a
    round changes nothing, then nerf_hip_mesh_cc_ids and nerf_hip_mesh_cc_stats; the definition is in include/nerf_hip.h) ->
    (vert_comp[V] int32, face_comp[F] int32, n_verts[C] int32, n_faces[C] int32, bbox_lo[C, 3], bbox_hi[C, 3] fp32 -- both None without
    verts[V, 3] --, rounds).  One 4-byte read of the device's `changed` word per round and one 8-byte read of C (each synchronises with
    the stream).  A labelling that does not converge within the library's cap of rounds raises NerfHipError: there is no partial
    result.  ws: a uint8 device buffer of >= _abi.mesh_cc_ws_bytes(V, F) bytes (allocated here if None)."""
    faces, V, F = _cc_faces(faces, num_verts)
    dev = faces.device
    if verts is not None:
        if tuple(verts.shape) != (V, 3) or verts.device != dev:
            raise ValueError(f"verts {tuple(verts.shape)} on {verts.device}: a [{V}, 3] tensor on {dev}")
        verts = verts.to(torch.float32).contiguous()
    if ws is None:
        ws = torch.empty(max(_abi.mesh_cc_ws_bytes(V, F), 1), dtype=torch.uint8, device=dev)
    L, st = _abi.lib(), _stream(faces)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    rounds = 0
    while True:  # (the library refuses the round past its cap: the loop ends)
        _abi.check(L.nerf_hip_mesh_cc_round(faces.data_ptr(), V, F, rounds, ws.data_ptr(), ws.numel(), changed.data_ptr(), st))
        rounds += 1
        if int(changed.cpu()) == 0:
            break
    vert_comp = torch.empty(V, dtype=torch.int32, device=dev)
    face_comp = torch.empty(F, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _abi.check(L.nerf_hip_mesh_cc_ids(faces.data_ptr(), V, F, ws.data_ptr(), ws.numel(), vert_comp.data_ptr(), face_comp.data_ptr(),
                                      count.data_ptr(), st))
    C_ = int(count.cpu())
    n_verts = torch.empty(C_, dtype=torch.int32, device=dev)
    n_faces = torch.empty(C_, dtype=torch.int32, device=dev)
    lo = hi = None
    if verts is not None:
        lo, hi = torch.empty(C_, 3, device=dev), torch.empty(C_, 3, device=dev)
    _abi.check(L.nerf_hip_mesh_cc_stats(verts.data_ptr() if verts is not None else None, vert_comp.data_ptr(), face_comp.data_ptr(), V, F,
                                        n_verts.data_ptr(), n_faces.data_ptr(), lo.data_ptr() if lo is not None else None,
                                        hi.data_ptr() if hi is not None else None, C_, st))
    return vert_comp, face_comp, n_verts, n_faces, lo, hi, rounds


def mesh_compact(verts, faces, normals, rgb, vert_comp, face_comp, keep, max_v, max_f, ws=None):
    """Drops the components c with keep[c] == 0 (nerf_hip_mesh_cc_compact): -> (verts[max_v, 3], faces[max_f, 3], normals, rgb -- None
    where the input is None --, counts int64[2] = (V', F') on the device).  max_v / max_f: the outputs' rows (the kept components'
    n_verts / n_faces sums); nothing is stored past them.  keep: a bool or uint8 [C] device tensor."""
    faces, V, F = _cc_faces(faces, verts.shape[0])
    dev = faces.device
    f32 = lambda a: None if a is None else a.to(torch.float32).contiguous()
    verts, normals, rgb = f32(verts), f32(normals), f32(rgb)
    for a in (verts, normals, rgb):
        if a is not None and (tuple(a.shape) != (V, 3) or a.device != dev):
            raise ValueError(f"a per-vertex array {tuple(a.shape)} on {a.device}: [{V}, 3] on {dev}")
    if tuple(vert_comp.shape) != (V,) or tuple(face_comp.shape) != (F,) or vert_comp.dtype != torch.int32 or face_comp.dtype != torch.int32:
        raise ValueError(f"vert_comp {tuple(vert_comp.shape)} / face_comp {tuple(face_comp.shape)}: int32 [{V}] / [{F}]")
    keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
    if ws is None:
        ws = torch.empty(max(_abi.mesh_cc_ws_bytes(V, F), 1), dtype=torch.uint8, device=dev)
    max_v, max_f = int(max_v), int(max_f)
    out = lambda a: None if a is None else torch.empty(max_v, 3, device=dev)
    ov, on, oc = out(verts), out(normals), out(rgb)
    of = torch.empty(max_f, 3, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    ptr = lambda a: None if a is None else a.data_ptr()
    _abi.check(_abi.lib().nerf_hip_mesh_cc_compact(ptr(verts), ptr(normals), ptr(rgb), faces.data_ptr(), V, F, vert_comp.contiguous().data_ptr(),
                                                   face_comp.contiguous().data_ptr(), keep.data_ptr(), keep.numel(), ws.data_ptr(), ws.numel(),
                                                   ptr(ov), ptr(on), ptr(oc), of.data_ptr(), max_v, max_f, counts.data_ptr(), _stream(faces)))
    return ov, of, on, oc, counts


def mesh_simplify(verts, faces, normals, lo, cell, dims, ws=None, counts=None):
    """Uniform vertex clustering of the indexed mesh (verts[V, 3] fp32, faces[F, 3] int32, normals[V, 3] fp32 or None; device) over the
    cluster lattice lo / cell (three host floats each) / dims (three host ints): nerf_hip_mesh_simplify_count, one 48-byte read of the
    device counts (this synchronises with the stream), then nerf_hip_mesh_simplify_emit into buffers sized from them; the definition
    is in include/nerf_hip.h.  -> (verts[V', 3], faces[F', 3] int32, normals[V', 3] or None, info) with info = dict(verts_in, faces_in,
    verts_out, faces_out, clusters, degenerate_faces, duplicate_faces).  A face table that reports itself full raises NerfHipError:
    there is no partial result.  ws: a uint8 device buffer of >= _abi.mesh_simplify_ws_bytes(V, F, dims) bytes; counts: an int64 [6]
    device tensor; each is allocated here if None."""
    faces, V, F = _cc_faces(faces, verts.shape[0])
    dev = faces.device
    f32 = lambda a: None if a is None else a.to(torch.float32).contiguous()
    verts, normals = f32(verts), f32(normals)
    for a in (verts, normals):
        if a is not None and (tuple(a.shape) != (V, 3) or a.device != dev):
            raise ValueError(f"a per-vertex array {tuple(a.shape)} on {a.device}: [{V}, 3] on {dev}")
    lo3, cell3, dims3 = _abi.f32_array(lo), _abi.f32_array(cell), _abi.i32_array(dims)
    if len(lo3) != 3 or len(cell3) != 3 or len(dims3) != 3:
        raise ValueError("lo, cell and dims have three entries each")
    if ws is None:
        ws = torch.empty(max(_abi.mesh_simplify_ws_bytes(V, F, dims), 1), dtype=torch.uint8, device=dev)
    if counts is None:
        counts = torch.empty(6, dtype=torch.int64, device=dev)
    L, st = _abi.lib(), _stream(faces)
    ptr = lambda a: None if a is None else a.data_ptr()
    _abi.check(L.nerf_hip_mesh_simplify_count(ptr(verts), ptr(normals), faces.data_ptr(), V, F, lo3, cell3, dims3, ws.data_ptr(), ws.numel(),
                                              counts.data_ptr(), st))
    V1, F1, clusters, flags, n_deg, n_dup = (int(n) for n in counts.cpu())
    if flags & _abi.SIMPLIFY_TABLE_FULL:
        raise _abi.NerfHipError(f"mesh_simplify: the face table reported itself full (V={V} F={F}); no result")
    ov = torch.empty(V1, 3, device=dev)
    on = torch.empty(V1, 3, device=dev) if normals is not None else None
    of = torch.empty(F1, 3, dtype=torch.int32, device=dev)
    _abi.check(L.nerf_hip_mesh_simplify_emit(faces.data_ptr(), V, F, lo3, cell3, dims3, ws.data_ptr(), ws.numel(), ptr(ov), ptr(on),
                                             of.data_ptr(), V1, F1, st))
    info = dict(verts_in=V, faces_in=F, verts_out=V1, faces_out=F1, clusters=clusters, degenerate_faces=n_deg, duplicate_faces=n_dup)
    return ov, of, on, info


def _box(lo, scale):
    lo3 = _abi.f32_array(lo)
    if len(lo3) != 3:
        raise ValueError("lo has three entries")
    return lo3, float(scale)


def mesh_edges(faces, num_verts, ws=None, counts=None):
    """The unique undirected edges of the indexed mesh faces[F, 3] (int32, device) over num_verts vertices (nerf_hip_mesh_edges_build;
    the definition is in include/nerf_hip.h) -> (degree[V] int32, vert_flags[V] int32, counts int64[8] ON THE DEVICE, ws).  Enqueue
    only: the caller reads counts (and raises on EDGES_TABLE_FULL in counts[6]).  The workspace then holds every vertex's neighbours
    for mesh_smooth_step.  ws: a uint8 device buffer of >= _abi.mesh_edges_ws_bytes(V, F) bytes; counts: an int64 [8] device tensor;
    each is allocated here if None."""
    faces, V, F = _cc_faces(faces, num_verts)
    dev = faces.device
    if ws is None:
        ws = torch.empty(_abi.mesh_edges_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    if counts is None:
        counts = torch.empty(8, dtype=torch.int64, device=dev)
    degree = torch.empty(V, dtype=torch.int32, device=dev)
    flags = torch.empty(V, dtype=torch.int32, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_edges_build(faces.data_ptr(), V, F, ws.data_ptr(), ws.numel(), degree.data_ptr(), flags.data_ptr(),
                                                    counts.data_ptr(), _stream(faces)))
    return degree, flags, counts, ws


EDGE_COUNT_NAMES = ("faces", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "used_verts", "flags", "max_degree")


def mesh_edge_counts(counts, V, F):
    """The host's reading of mesh_edges' counts (eight ints, already on the host) -> a dict by EDGE_COUNT_NAMES without the flags word;
    a table that reported itself full raises NerfHipError: there is no partial result."""
    c = dict(zip(EDGE_COUNT_NAMES, (int(n) for n in counts)))
    if c.pop("flags") & _abi.EDGES_TABLE_FULL:
        raise _abi.NerfHipError(f"mesh_edges: the edge table reported itself full (V={V} F={F}); no result")
    return c


def mesh_smooth_step(verts_in, verts_out, num_faces, lo, scale, w, vert_flags, ws):
    """One smoothing step with weight w (nerf_hip_mesh_smooth_step): verts_in[V, 3] -> verts_out[V, 3], two contiguous fp32 device
    tensors that do not overlap, over the neighbours mesh_edges left in ws.  vert_flags: mesh_edges' flags to pin the boundary, or
    None.  Enqueue only."""
    V = int(verts_in.shape[0])
    for a in (verts_in, verts_out):
        if tuple(a.shape) != (V, 3) or a.dtype != torch.float32 or not a.is_contiguous() or a.device != ws.device:
            raise ValueError(f"a position array {tuple(a.shape)} {a.dtype} on {a.device}: contiguous fp32 [{V}, 3] on {ws.device}")
    if vert_flags is not None and (tuple(vert_flags.shape) != (V,) or vert_flags.dtype != torch.int32 or not vert_flags.is_contiguous()
                                   or vert_flags.device != ws.device):
        raise ValueError(f"vert_flags {tuple(vert_flags.shape)} {vert_flags.dtype} on {vert_flags.device}: contiguous int32 [{V}] on {ws.device}")
    lo3, scale = _box(lo, scale)
    _abi.check(_abi.lib().nerf_hip_mesh_smooth_step(verts_in.data_ptr(), verts_out.data_ptr(), V, int(num_faces), lo3, scale, float(w),
                                                    vert_flags.data_ptr() if vert_flags is not None else None, ws.data_ptr(), ws.numel(), V,
                                                    _stream(verts_in)))
    return verts_out


def mesh_vertex_normals(verts, faces, lo, scale, ws=None):
    """Area-weighted vertex normals from the faces (nerf_hip_mesh_vertex_normals; the definition is in include/nerf_hip.h): verts[V, 3]
    fp32, faces[F, 3] int32 (device), the box lo (three host floats) / scale -> normals[V, 3] fp32.  Enqueue only.  ws: as mesh_edges
    (whose neighbours it leaves intact)."""
    faces, V, F = _cc_faces(faces, verts.shape[0])
    dev = faces.device
    verts = verts.to(torch.float32).contiguous()
    if tuple(verts.shape) != (V, 3) or verts.device != dev:
        raise ValueError(f"verts {tuple(verts.shape)} on {verts.device}: [{V}, 3] on {dev}")
    if ws is None:
        ws = torch.empty(_abi.mesh_edges_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    lo3, scale = _box(lo, scale)
    normals = torch.empty(V, 3, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_vertex_normals(verts.data_ptr(), faces.data_ptr(), V, F, lo3, scale, ws.data_ptr(), ws.numel(),
                                                       normals.data_ptr(), V, _stream(faces)))
    return normals


def _md_mesh(verts, faces):
    faces, V, F = _cc_faces(faces, verts.shape[0])
    verts = verts.to(torch.float32).contiguous()
    if tuple(verts.shape) != (V, 3) or verts.device != faces.device:
        raise ValueError(f"verts {tuple(verts.shape)} on {verts.device}: [{V}, 3] on {faces.device}")
    return verts, faces, V, F


def mesh_measure(verts, faces, lo, scale):
    """The measures of an indexed mesh over the box lo / scale (nerf_hip_mesh_measure; the definition is in include/nerf_hip.h) ->
    int64[8] ON THE DEVICE: the fixed-point sums of the area, the six-volumes and the three centroid moments, the faces that take
    part, 0, 0.  Enqueue only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    lo3, scale = _box(lo, scale)
    out = torch.empty(8, dtype=torch.int64, device=faces.device)
    _abi.check(_abi.lib().nerf_hip_mesh_measure(verts.data_ptr(), faces.data_ptr(), V, F, lo3, scale, out.data_ptr(), _stream(faces)))
    return out


def mesh_sample(verts, faces, n, seed, lo, scale, ws=None):
    """n area-weighted surface samples of an indexed mesh (nerf_hip_mesh_sample; the definition is in include/nerf_hip.h) ->
    (points[n, 3] fp32, face[n] int32, info int64[1] = the total weight W ON THE DEVICE).  Enqueue only: the caller reads info (W <= 0:
    a mesh without area, every face id is -1).  ws: a uint8 device buffer of >= _abi.mesh_sample_ws_bytes(F) bytes."""
    verts, faces, V, F = _md_mesh(verts, faces)
    dev = faces.device
    n = int(n)
    if n < 0:
        raise ValueError(f"n={n} < 0")
    lo3, scale = _box(lo, scale)
    if ws is None:
        ws = torch.empty(max(_abi.mesh_sample_ws_bytes(F), 256), dtype=torch.uint8, device=dev)
    points = torch.empty(n, 3, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.empty(1, dtype=torch.int64, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_sample(verts.data_ptr(), faces.data_ptr(), V, F, lo3, scale, n, int(seed) & 0xFFFFFFFF, ws.data_ptr(),
                                               ws.numel(), points.data_ptr(), face.data_ptr(), n, info.data_ptr(), _stream(faces)))
    return points, face, info


def _md_points(p, name):
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} {tuple(p.shape)}: a [n, 3] tensor")
    return p.to(torch.float32).contiguous()


def points_grid(ref, lo, cell, dims, n_query=0, ws=None):
    """Sorts the reference points ref[M, 3] (fp32, device) by cell of the grid lo (three host floats) / cell (one float) / dims (three
    host ints) (nerf_hip_points_grid_build) -> (ws, counts int64[2] ON THE DEVICE = the finite points, the fullest cell's points).  ws
    is sized for queries of up to n_query points: a uint8 device buffer of >= _abi.points_nearest_ws_bytes(M, n_query, dims) bytes."""
    ref = _md_points(ref, "ref")
    M = int(ref.shape[0])
    lo3, dims3 = _abi.f32_array(lo), _abi.i32_array(dims)
    if len(lo3) != 3 or len(dims3) != 3:
        raise ValueError("lo and dims have three entries each")
    if ws is None:
        ws = torch.empty(_abi.points_nearest_ws_bytes(M, n_query, dims), dtype=torch.uint8, device=ref.device)
    counts = torch.empty(2, dtype=torch.int64, device=ref.device)
    _abi.check(_abi.lib().nerf_hip_points_grid_build(ref.data_ptr(), M, lo3, float(cell), dims3, ws.data_ptr(), ws.numel(), counts.data_ptr(),
                                                     _stream(ref)))
    return ws, counts


def points_nearest(query, num_ref, lo, cell, dims, ws, sort_queries=False):
    """The nearest reference point of every query[N, 3] (fp32, device) over the grid points_grid left in ws (nerf_hip_points_nearest; the
    definition is in include/nerf_hip.h) -> (idx[N] int32, dist2[N] fp64).  Enqueue only."""
    query = _md_points(query, "query")
    N = int(query.shape[0])
    if query.device != ws.device:
        raise ValueError(f"query on {query.device}: the grid is on {ws.device}")
    idx = torch.empty(N, dtype=torch.int32, device=query.device)
    dist2 = torch.empty(N, dtype=torch.float64, device=query.device)
    _abi.check(_abi.lib().nerf_hip_points_nearest(query.data_ptr(), int(num_ref), N, _abi.f32_array(lo), float(cell), _abi.i32_array(dims),
                                                  ws.data_ptr(), ws.numel(), 1 if sort_queries else 0, idx.data_ptr(), dist2.data_ptr(), N,
                                                  _stream(query)))
    return idx, dist2


def _rc_grid(lo, dims):
    lo3, dims3 = _abi.f32_array(lo), _abi.i32_array(dims)
    if len(lo3) != 3 or len(dims3) != 3:
        raise ValueError("lo and dims have three entries each")
    return lo3, dims3


def mesh_raycast_count(verts, faces, lo, cell, dims, counts=None):
    """The sizes of the triangle grid lo (three host floats) / cell (one float) / dims (three host ints) over an indexed mesh
    (nerf_hip_mesh_raycast_grid_count; the definition is in include/nerf_hip.h) -> counts int64[3] ON THE DEVICE = the faces that take
    part, the entries E, the OUTSIDE faces.  Enqueue only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    lo3, dims3 = _rc_grid(lo, dims)
    if counts is None:
        counts = torch.empty(3, dtype=torch.int64, device=faces.device)
    _abi.check(_abi.lib().nerf_hip_mesh_raycast_grid_count(verts.data_ptr(), faces.data_ptr(), V, F, lo3, float(cell), dims3, counts.data_ptr(),
                                                           _stream(faces)))
    return counts


def mesh_raycast_fill(verts, faces, lo, cell, dims, cap_entries, ws=None):
    """Enters the faces in the cells of the triangle grid (nerf_hip_mesh_raycast_grid_fill) -> ws, a uint8 device buffer of >=
    _abi.mesh_raycast_ws_bytes(F, cap_entries, dims) bytes (allocated here if None).  cap_entries: E of mesh_raycast_count.  Enqueue
    only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    lo3, dims3 = _rc_grid(lo, dims)
    if ws is None:
        ws = torch.empty(_abi.mesh_raycast_ws_bytes(F, cap_entries, dims), dtype=torch.uint8, device=faces.device)
    _abi.check(_abi.lib().nerf_hip_mesh_raycast_grid_fill(verts.data_ptr(), faces.data_ptr(), V, F, lo3, float(cell), dims3, int(cap_entries),
                                                          ws.data_ptr(), ws.numel(), _stream(faces)))
    return ws


def mesh_raycast(verts, faces, lo, cell, dims, cap_entries, ws, origins, dirs, tmin=0.0, tmax=float("inf"), skip=None, any_hit=False):
    """Casts the rays origins[N, 3] / dirs[N, 3] (fp32, device) against the mesh over the grid mesh_raycast_fill left in ws
    (nerf_hip_mesh_raycast; the definition is in include/nerf_hip.h) -> (t[N] fp64, uv[N, 2] fp64, face[N] int32, side[N] int8), or
    occluded[N] uint8 with any_hit.  skip: int32 [N] or None.  Enqueue only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    origins, dirs = _md_points(origins, "origins"), _md_points(dirs, "dirs")
    N, dev = int(origins.shape[0]), faces.device
    if tuple(dirs.shape) != (N, 3) or origins.device != dev or dirs.device != dev or ws.device != dev:
        raise ValueError(f"origins {tuple(origins.shape)} on {origins.device}, dirs {tuple(dirs.shape)} on {dirs.device}: [N, 3] each on {dev}")
    if skip is not None:
        if tuple(skip.shape) != (N,) or skip.device != dev:
            raise ValueError(f"skip {tuple(skip.shape)} on {skip.device}: [{N}] on {dev}")
        skip = skip.to(torch.int32).contiguous()
    lo3, dims3 = _rc_grid(lo, dims)
    ptr = lambda a: None if a is None else a.data_ptr()
    t = uv = face = side = occ = None
    if any_hit:
        occ = torch.empty(N, dtype=torch.uint8, device=dev)
    else:
        t = torch.empty(N, dtype=torch.float64, device=dev)
        uv = torch.empty(N, 2, dtype=torch.float64, device=dev)
        face = torch.empty(N, dtype=torch.int32, device=dev)
        side = torch.empty(N, dtype=torch.int8, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_raycast(verts.data_ptr(), faces.data_ptr(), V, F, lo3, float(cell), dims3, int(cap_entries), ws.data_ptr(),
                                                ws.numel(), origins.data_ptr(), dirs.data_ptr(), ptr(skip), N, float(tmin), float(tmax),
                                                1 if any_hit else 0, ptr(t), ptr(uv), ptr(face), ptr(side), ptr(occ), N, _stream(faces)))
    return occ if any_hit else (t, uv, face, side)


def mesh_face_rays(verts, faces, cam_o, Q, H, W):
    """One shadow ray per face towards the camera at cam_o (three host floats) with Q (nine host doubles, row-major)
    (nerf_hip_mesh_face_rays; the definition is in include/nerf_hip.h) -> (orig[F, 3], dir[F, 3] fp32, valid[F] uint8).  Enqueue only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    dev = faces.device
    cam3 = _abi.f32_array(cam_o)
    q9 = (C.c_double * 9)(*[float(x) for x in Q])
    if len(cam3) != 3:
        raise ValueError("cam_o has three entries")
    orig = torch.empty(F, 3, device=dev)
    dirs = torch.empty(F, 3, device=dev)
    valid = torch.empty(F, dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_face_rays(verts.data_ptr(), faces.data_ptr(), V, F, cam3, q9, int(H), int(W), orig.data_ptr(),
                                                  dirs.data_ptr(), valid.data_ptr(), F, _stream(faces)))
    return orig, dirs, valid


def mesh_select_faces(verts, faces, normals, rgb, keep, ws=None):
    """The faces with keep[f] != 0 and the vertices they use (nerf_hip_mesh_select_faces_count, one 16-byte read of the device counts --
    this synchronises with the stream --, then nerf_hip_mesh_select_faces_emit) -> (verts[V', 3], faces[F', 3] int32, normals, rgb --
    None where the input is None).  keep: a bool or uint8 [F] device tensor."""
    faces, V, F = _cc_faces(faces, verts.shape[0])
    dev = faces.device
    f32 = lambda a: None if a is None else a.to(torch.float32).contiguous()
    verts, normals, rgb = f32(verts), f32(normals), f32(rgb)
    for a in (verts, normals, rgb):
        if a is not None and (tuple(a.shape) != (V, 3) or a.device != dev):
            raise ValueError(f"a per-vertex array {tuple(a.shape)} on {a.device}: [{V}, 3] on {dev}")
    if tuple(keep.shape) != (F,):
        raise ValueError(f"keep {tuple(keep.shape)}: one entry per face, [{F}]")
    keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
    if ws is None:
        ws = torch.empty(_abi.mesh_select_faces_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    L, st = _abi.lib(), _stream(faces)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _abi.check(L.nerf_hip_mesh_select_faces_count(faces.data_ptr(), V, F, keep.data_ptr(), ws.data_ptr(), ws.numel(), counts.data_ptr(), st))
    V1, F1 = (int(n) for n in counts.cpu())
    out = lambda a: None if a is None else torch.empty(V1, 3, device=dev)
    ov, on, oc = out(verts), out(normals), out(rgb)
    of = torch.empty(F1, 3, dtype=torch.int32, device=dev)
    ptr = lambda a: None if a is None else a.data_ptr()
    _abi.check(L.nerf_hip_mesh_select_faces_emit(ptr(verts), ptr(normals), ptr(rgb), faces.data_ptr(), V, F, keep.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), ptr(ov), ptr(on), ptr(oc), of.data_ptr(), V1, F1, st))
    return ov, of, on, oc


def tsdf_integrate(tsdf, weight, lo, step, depth, opacity, cam_o, Q, trunc, min_opacity=0.5, carve=True, rgb=None, color=None):
    """Integrates the depth images depth[n, H, W] (fp32, device; opacity the same or None) of the cameras cam_o (n x 3 host floats) / Q
    (n x 9 host doubles, row-major) into the volumes tsdf / weight [nx, ny, nz] IN PLACE (nerf_hip_tsdf_integrate; rule T of
    include/nerf_hip.h): contiguous fp32 device tensors on the lattice lo + (i, j, k) * step (three host floats each).  rgb / color:
    both None, or the views' colour images [n, H, W, 3] and the colour volume [nx, ny, nz, 4] -- then nerf_hip_tsdf_integrate_color
    (rule TC) fuses the colours beside the same geometry update and (tsdf, weight, color) is returned.  Enqueue only."""
    if tsdf.dim() != 3 or tsdf.shape != weight.shape:
        raise ValueError(f"tsdf {tuple(tsdf.shape)} weight {tuple(weight.shape)}: two [nx, ny, nz] volumes")
    if (rgb is None) != (color is None):
        raise ValueError("rgb and color: both or neither")
    vols = (("tsdf", tsdf), ("weight", weight)) + ((("color", color),) if color is not None else ())
    for name, t in vols:
        if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous fp32 device tensor (it is updated in place)")
    if color is not None and tuple(color.shape) != tuple(tsdf.shape) + (4,):
        raise ValueError(f"color {tuple(color.shape)}: the volumes' shape {tuple(tsdf.shape)} and 4 channels (R, G, B, Wc)")
    if depth.dim() != 3:
        raise ValueError(f"depth {tuple(depth.shape)}: [n, H, W]")
    dev = tsdf.device
    depth = depth.to(dev, torch.float32).contiguous()
    n, H, W = (int(x) for x in depth.shape)
    if opacity is not None:
        opacity = opacity.to(dev, torch.float32).contiguous()
        if opacity.shape != depth.shape:
            raise ValueError(f"opacity {tuple(opacity.shape)}: the depth's shape {tuple(depth.shape)}")
    cam = [float(x) for row in cam_o for x in row]
    q = [float(x) for row in Q for x in row]
    if len(cam) != 3 * n or len(q) != 9 * n:
        raise ValueError(f"cam_o / Q: three and nine entries for each of the {n} views")
    nx, ny, nz = (int(x) for x in tsdf.shape)
    grid = (nx, ny, nz, _abi.f32_array(lo), _abi.f32_array(step))
    op = opacity.data_ptr() if opacity is not None else None
    tail = (n, H, W, _abi.f32_array(cam), (C.c_double * len(q))(*q), float(trunc), float(min_opacity), _abi.TSDF_CARVE if carve else 0,
            _stream(tsdf))
    if color is None:
        _abi.check(_abi.lib().nerf_hip_tsdf_integrate(tsdf.data_ptr(), weight.data_ptr(), *grid, depth.data_ptr(), op, *tail))
        return tsdf, weight
    rgb = rgb.to(dev, torch.float32).contiguous()
    if tuple(rgb.shape) != (n, H, W, 3):
        raise ValueError(f"rgb {tuple(rgb.shape)}: a colour per pixel of the depth images, [{n}, {H}, {W}, 3]")
    _abi.check(_abi.lib().nerf_hip_tsdf_integrate_color(tsdf.data_ptr(), weight.data_ptr(), color.data_ptr(), *grid, depth.data_ptr(), op,
                                                        rgb.data_ptr(), *tail))
    return tsdf, weight, color


def tsdf_sample_color(color, lo, step, points):
    """The colour volume color[nx, ny, nz, 4] (fp32 (R, G, B, Wc), device, contiguous) on the lattice lo + (i, j, k) * step sampled at
    points[M, 3] (nerf_hip_tsdf_sample_color; rule S of include/nerf_hip.h) -> (rgb[M, 3] fp32, valid[M] uint8).  Enqueue only."""
    if color.dim() != 4 or color.shape[3] != 4 or color.device.type != "cuda" or color.dtype != torch.float32 or not color.is_contiguous():
        raise ValueError(f"color {tuple(color.shape)} {color.dtype}: a contiguous fp32 [nx, ny, nz, 4] device tensor")
    dev = color.device
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points {tuple(points.shape)}: [M, 3]")
    points = points.to(dev, torch.float32).contiguous()
    M = int(points.shape[0])
    rgb = torch.empty(M, 3, device=dev)
    valid = torch.empty(M, dtype=torch.uint8, device=dev)
    nx, ny, nz = (int(x) for x in color.shape[:3])
    _abi.check(_abi.lib().nerf_hip_tsdf_sample_color(color.data_ptr(), nx, ny, nz, _abi.f32_array(lo), _abi.f32_array(step), points.data_ptr(),
                                                     M, rgb.data_ptr(), valid.data_ptr(), _stream(color)))
    return rgb, valid


def mesh_atlas_texels(verts, normals, faces, n, row0, rows):
    """The texels of the rows [row0, row0 + rows) of the atlas of faces[F, 3] with charts of n texels (nerf_hip_mesh_atlas_texels; rule
    TA of include/nerf_hip.h), T = rows * W of them in row-major order -> (points[T, 3], dirs[T, 3] fp32, mask[T] uint8).  verts,
    normals [V, 3] fp32 on faces' device.  Enqueue only."""
    verts, faces, V, F = _md_mesh(verts, faces)
    normals = normals.to(torch.float32).contiguous()
    if tuple(normals.shape) != (V, 3) or normals.device != faces.device:
        raise ValueError(f"normals {tuple(normals.shape)} on {normals.device}: [{V}, 3] on {faces.device}")
    dev = faces.device
    W = _abi.mesh_atlas_dims(F, n)[3]
    T = max(int(rows), 0) * W
    points = torch.empty(T, 3, device=dev)
    dirs = torch.empty(T, 3, device=dev)
    mask = torch.empty(T, dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_atlas_texels(verts.data_ptr(), normals.data_ptr(), faces.data_ptr(), V, F, int(n), int(row0), int(rows),
                                                     points.data_ptr(), dirs.data_ptr(), mask.data_ptr(), _stream(faces)))
    return points, dirs, mask


def mesh_texture_sample(image, F, n, face, uv, background=(0.0, 0.0, 0.0)):
    """Bilinear lookups in the atlas image[H, W, 3] (fp32, device, contiguous) of F faces with charts of n texels at face[N] (int32),
    uv[N, 2] (fp64) (nerf_hip_mesh_texture_sample; rule TX of include/nerf_hip.h) -> (rgb[N, 3] fp32, valid[N] uint8); background
    (three host floats) where a lookup is not valid.  Enqueue only."""
    _, _, _, W, H = _abi.mesh_atlas_dims(F, n)
    if image.device.type != "cuda" or image.dtype != torch.float32 or not image.is_contiguous() or tuple(image.shape) != (H, W, 3):
        raise ValueError(f"image {tuple(image.shape)} {image.dtype}: a contiguous fp32 [{H}, {W}, 3] device tensor, the atlas of F={F} n={n}")
    dev = image.device
    if face.dim() != 1 or tuple(uv.shape) != (face.shape[0], 2):
        raise ValueError(f"face {tuple(face.shape)} uv {tuple(uv.shape)}: [N] and [N, 2]")
    face = face.to(dev, torch.int32).contiguous()
    uv = uv.to(dev, torch.float64).contiguous()
    N = int(face.shape[0])
    bg = _abi.f32_array(background)
    if len(bg) != 3:
        raise ValueError("background has three entries")
    rgb = torch.empty(N, 3, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_mesh_texture_sample(image.data_ptr(), int(F), int(n), face.data_ptr(), uv.data_ptr(), N, bg, rgb.data_ptr(),
                                                       valid.data_ptr(), _stream(image)))
    return rgb, valid


def distance_stats(dist2, unit, thresholds=()):
    """The statistics of squared distances dist2[N] (fp64, device) in units of `unit` (nerf_hip_distance_stats; the definition is in
    include/nerf_hip.h) -> int64[4 + K] ON THE DEVICE: the finite count, the fixed-point sums of d / unit and d2 / unit^2, the clamped,
    and per threshold the distances <= it.  Enqueue only."""
    if dist2.dim() != 1 or dist2.dtype != torch.float64:
        raise ValueError(f"dist2 {tuple(dist2.shape)} {dist2.dtype}: an fp64 [N] tensor")
    dist2 = dist2.contiguous()
    tau = (C.c_double * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    out = torch.empty(4 + len(thresholds), dtype=torch.int64, device=dist2.device)
    _abi.check(_abi.lib().nerf_hip_distance_stats(dist2.data_ptr(), int(dist2.shape[0]), float(unit), tau, len(thresholds), out.data_ptr(),
                                                  _stream(dist2)))
    return out


def image_metrics(pred, gt, ws=None):
    """Per-view MSE and SSIM (nerf_hip_image_metrics, fp64 arithmetic; definition in include/nerf_hip.h): pred, gt [n, H, W, 3] device
    tensors of the same shape and device (cast to contiguous fp32 here) -> (mse[n], ssim[n]) fp64 on that device.  ws: a uint8 device
    buffer of >= _abi.metrics_ws_bytes(n, H, W) bytes (allocated here if None)."""
    if pred.dim() != 4 or pred.shape[-1] != 3 or tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)}: two [n, H, W, 3] tensors of the same shape")
    if pred.device != gt.device or pred.device.type != "cuda":
        raise ValueError(f"pred on {pred.device}, gt on {gt.device}: both on one ROCm device (there is no CPU path)")
    n, H, W, _ = (int(d) for d in pred.shape)
    dev = pred.device
    pred = pred.to(torch.float32).contiguous()
    gt = gt.to(torch.float32).contiguous()
    mse = torch.empty(n, dtype=torch.float64, device=dev)
    ssim = torch.empty(n, dtype=torch.float64, device=dev)
    if ws is None:
        ws = torch.empty(max(_abi.metrics_ws_bytes(n, H, W), 1), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().nerf_hip_image_metrics(pred.data_ptr(), gt.data_ptr(), n, H, W, mse.data_ptr(), ssim.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), _stream(pred)))
    return mse, ssim


# ---- the per-ray stages on their own (the stage entries of include/nerf_hip.h).  Four helpers, one per stage, allocate the outputs, fill
# the optional ones with their initial values and make the library call; the public functions below say which entry and which optional
# outputs they stand for.  The optional outputs are those of the library's extras record: maps, quantile depths, distortion loss ----
_NAN = float("nan")


def _near_far(near, far, dev):
    return torch.stack((near, far), dim=1).contiguous().to(dev)


def _ptr(t):
    return None if t is None else t.contiguous().data_ptr()


def _coarse_stage(entry, t_c, sigma_c, rgb_c, near, far, delta0, Nf, rays=None, maps=False, tail=(), who="coarse_composite"):
    """One forward coarse stage call `entry` of the first `rays` rays (default: all) -> w_c, C_coarse, t_f, status(int), maps[B,4] or None
    (NaN where the kernel does not write); tail: the entry's arguments behind the stream"""
    B, Nc = t_c.shape
    rays = B if rays is None else int(rays)
    if not 1 <= rays <= B:
        raise ValueError(f"{who}: 1 <= rays <= B")
    dev = t_c.device
    nf = _near_far(near, far, dev)
    w_c = torch.empty(B, Nc, device=dev)
    C_c = torch.empty(B, 3, device=dev)
    t_f = torch.empty(B, Nf, device=dev)
    M = torch.full((B, 4), _NAN, device=dev) if maps else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = [_ptr(t_c), _ptr(sigma_c), _ptr(rgb_c), nf.data_ptr(), float(delta0), rays, Nc, Nf, w_c.data_ptr(), C_c.data_ptr(), t_f.data_ptr(),
            status.data_ptr()]
    _abi.check(getattr(_abi.lib(), entry)(*args, *([M.data_ptr()] if maps else []), _stream(t_c), *tail))
    return w_c, C_c, t_f, int(status.item()), M


def _merge_stage(entry, t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last, train=None, tail=()):
    """One forward merge stage call `entry` -> bundle, w, C_fine, perm, maps.  train: None for the inference entry, else (perm, joint, maps)
    -- whether the call gets perm[B,5,N] int16 (starting at -1) and maps[B,4] (starting at NaN), which come back as None otherwise"""
    B, Nc = t_c.shape
    Nf = t_f.shape[1]
    dev = t_c.device
    bundle = torch.empty(B, Nc + Nf, 5, device=dev)
    w = torch.empty(B, Nc + Nf, device=dev)
    C_f = torch.empty(B, 3, device=dev)
    pm = M = None
    mid = []
    if train is not None:
        perm, joint, maps = train
        pm = torch.full((B, 5, Nc + Nf), -1, dtype=torch.int16, device=dev) if perm else None
        M = torch.full((B, 4), _NAN, device=dev) if maps else None
        mid = [_ptr(pm), int(bool(joint)), _ptr(M)]
    _abi.check(getattr(_abi.lib(), entry)(_ptr(t_c), _ptr(t_f), _ptr(sigma_c), _ptr(sigma_f), _ptr(rgb_c), _ptr(rgb_f), B, Nc, Nf, float(last),
                                          bundle.data_ptr(), w.data_ptr(), C_f.data_ptr(), *mid, _stream(t_c), *tail))
    return bundle, w, C_f, pm, M


def _coarse_stage_backward(entry, t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb, rays=None, mid=(), tail=(), who=""):
    """One backward coarse stage call `entry` of the first `rays` rays (default: all), which ADDS to dsig[B,Nc], drgb[B,Nc,3] in place;
    mid: the entry's arguments between dt_f and dsig (dmaps), tail: those behind the stream (ddist)"""
    B, Nc = t_c.shape
    Nf = dt_f.shape[1]
    rays = B if rays is None else int(rays)
    if not (1 <= rays <= B and dsig.shape == (B, Nc) and drgb.shape == (B, Nc, 3) and dsig.is_contiguous() and drgb.is_contiguous()):
        raise ValueError(f"{who}: contiguous dsig [B,Nc] / drgb [B,Nc,3] and 1 <= rays <= B")
    nf = _near_far(near, far, t_c.device)
    _abi.check(getattr(_abi.lib(), entry)(_ptr(t_c), _ptr(sigma_c), _ptr(rgb_c), nf.data_ptr(), float(delta0), rays, Nc, Nf, _ptr(dC_c), _ptr(dt_f),
                                          *mid, dsig.data_ptr(), drgb.data_ptr(), _stream(t_c), *tail))
    return dsig, drgb


def _merge_stage_backward(entry, bundle, perm, dC_f, Nc, last, dmaps, tail=(), who="merge_composite_backward"):
    """One backward merge stage call `entry` -> dsig_c, dsig_f, drgb_c, drgb_f, dt_f; the outputs start as NaN: the kernel writes every
    element.  tail: the entry's arguments behind the stream"""
    B, N, _ = bundle.shape
    Nf = N - Nc
    dev = bundle.device
    if perm.dtype != torch.int16 or perm.shape != (B, 5, N):
        raise ValueError(f"{who}: perm is int16 [B,5,N]")
    nan = lambda *s: torch.full(s, _NAN, device=dev)
    dsig_c, dsig_f, drgb_c, drgb_f, dt_f = nan(B, Nc), nan(B, Nf), nan(B, Nc, 3), nan(B, Nf, 3), nan(B, Nf)
    _abi.check(getattr(_abi.lib(), entry)(_ptr(bundle), _ptr(perm), _ptr(dC_f), _ptr(dmaps), B, Nc, Nf, float(last), dsig_c.data_ptr(),
                                          dsig_f.data_ptr(), drgb_c.data_ptr(), drgb_f.data_ptr(), dt_f.data_ptr(), _stream(bundle), *tail))
    return dsig_c, dsig_f, drgb_c, drgb_f, dt_f


def coarse_composite(t_c, sigma_c, rgb_c, near, far, delta0, Nf):
    """-> w_c[B,Nc], C_coarse[B,3], t_f[B,Nf], status(int)"""
    return _coarse_stage("nerf_hip_coarse_composite", t_c, sigma_c, rgb_c, near, far, delta0, Nf)[:4]


def merge_composite(t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last=1e-4):
    """-> bundle[B,N,5], w[B,N], C_fine[B,3]"""
    return _merge_stage("nerf_hip_merge_composite", t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last)[:3]


def coarse_composite_backward(t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f):
    """-> dsig_c[B,Nc], drgb_c[B,Nc,3] (contributions through C_coarse and the resampled depths)"""
    B, Nc = t_c.shape
    dsig = torch.zeros(B, Nc, device=t_c.device)
    drgb = torch.zeros(B, Nc, 3, device=t_c.device)
    return _coarse_stage_backward("nerf_hip_coarse_composite_backward", t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb,
                                  who="coarse_composite_backward")


def coarse_composite_maps(t_c, sigma_c, rgb_c, near, far, delta0, Nf):
    """coarse_composite through k_coarse_x<maps> -> w_c, C_coarse, t_f, status(int), maps[B,4] (columns 0, 1 written; 2, 3 left NaN)"""
    return _coarse_stage("nerf_hip_coarse_composite_maps", t_c, sigma_c, rgb_c, near, far, delta0, Nf, maps=True)


def coarse_composite_backward_add(t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb, dmaps=None, rays=None):
    """ADDS the coarse stage's gradients of the first `rays` rays (default: all) to dsig[B,Nc], drgb[B,Nc,3] in place; dmaps[B,4]: the
    optional upstream of the coarse maps (k_coarse_bwd_x)"""
    return _coarse_stage_backward("nerf_hip_coarse_composite_backward_maps", t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb,
                                  rays=rays, mid=(_ptr(dmaps),), who="coarse_composite_backward_add")


def merge_composite_train(t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last=1e-4, joint=False, maps=False):
    """the training form of merge_composite (k_merge<true>) -> bundle[B,N,5], w[B,N], C_fine[B,3], perm[B,5,N] int16 (sorted position ->
    original slot per channel), maps[B,4] (columns 2, 3 written; 0, 1 left NaN) or None"""
    return _merge_stage("nerf_hip_merge_composite_train", t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last, train=(True, joint, maps))


def merge_composite_backward(bundle, perm, dC_f, Nc, last=1e-4, dmaps=None):
    """backward of merge_composite_train -> dsig_c[B,Nc], dsig_f[B,Nf], drgb_c[B,Nc,3], drgb_f[B,Nf,3], dt_f[B,Nf]; the outputs start as NaN:
    the kernel writes every element"""
    return _merge_stage_backward("nerf_hip_merge_composite_backward", bundle, perm, dC_f, Nc, last, dmaps)


def coarse_composite_quantiles(t_c, sigma_c, rgb_c, near, far, delta0, Nf, q, sentinel=float("nan"), rays=None):
    """coarse_composite_maps through k_coarse_x<maps, quantiles> (nerf_hip_coarse_composite_quantiles) -> w_c, C_coarse, t_f, status(int),
    maps[B,4], qdepth[B,2,nq]: row 0 = the coarse quantile depths of q (rule QD of include/nerf_hip.h), row 1 left at `sentinel`.  rays: a
    call of the first `rays` rays only (default: all) -- the outputs keep their B rows, and those behind the call their initial values"""
    Q = torch.full((t_c.shape[0], 2, len(q)), sentinel, device=t_c.device)
    return _coarse_stage("nerf_hip_coarse_composite_quantiles", t_c, sigma_c, rgb_c, near, far, delta0, Nf, rays=rays, maps=True,
                         tail=(_abi.f32_array(q), len(q), Q.data_ptr()), who="coarse_composite_quantiles") + (Q,)


def merge_composite_quantiles(t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, q, last=1e-4, joint=False, perm=True, sentinel=float("nan")):
    """merge_composite_train(maps=True) through k_merge_x<maps, quantiles> (nerf_hip_merge_composite_quantiles) -> bundle, w, C_fine, perm
    (None with perm=False: the values-only sort, joint=False only), maps[B,4], qdepth[B,2,nq]: row 1 = the fine quantile depths of q (rule
    QD), row 0 left at `sentinel`"""
    Q = torch.full((t_c.shape[0], 2, len(q)), sentinel, device=t_c.device)
    return _merge_stage("nerf_hip_merge_composite_quantiles", t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last, train=(perm, joint, True),
                        tail=(_abi.f32_array(q), len(q), Q.data_ptr())) + (Q,)


def coarse_composite_distortion(t_c, sigma_c, rgb_c, near, far, delta0, Nf, sentinel=float("nan"), rays=None):
    """coarse_composite_maps through k_coarse_x<maps, distortion> (nerf_hip_coarse_composite_distortion) -> w_c, C_coarse, t_f, status(int),
    maps[B,4], dist[B,2]: column 0 = the coarse distortion loss L_c (rule DL of include/nerf_hip.h), column 1 left at `sentinel`.  rays: a
    call of the first `rays` rays only (default: all) -- the outputs keep their B rows, and those behind the call their initial values"""
    dist = torch.full((t_c.shape[0], 2), sentinel, device=t_c.device)
    return _coarse_stage("nerf_hip_coarse_composite_distortion", t_c, sigma_c, rgb_c, near, far, delta0, Nf, rays=rays, maps=True,
                         tail=(dist.data_ptr(),), who="coarse_composite_distortion") + (dist,)


def merge_composite_distortion(t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, near, far, last=1e-4, joint=False, sentinel=float("nan")):
    """merge_composite_train(maps=True) through k_merge_x<maps, distortion> (nerf_hip_merge_composite_distortion) -> bundle, w, C_fine, perm,
    maps[B,4], dist[B,2]: column 1 = the fine distortion loss L_f (rule DL), column 0 left at `sentinel`"""
    nf = _near_far(near, far, t_c.device)
    dist = torch.full((t_c.shape[0], 2), sentinel, device=t_c.device)
    return _merge_stage("nerf_hip_merge_composite_distortion", t_c, t_f, sigma_c, sigma_f, rgb_c, rgb_f, last, train=(True, joint, True),
                        tail=(nf.data_ptr(), dist.data_ptr())) + (dist,)


def coarse_composite_backward_distortion_add(t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb, ddist, dmaps=None, rays=None):
    """coarse_composite_backward_add through k_coarse_bwd_x<distortion> (nerf_hip_coarse_composite_backward_distortion): ADDS the coarse
    stage's gradients, the upstream ddist[B,2] (column 0) of the coarse distortion loss included, to dsig[B,Nc], drgb[B,Nc,3] in place"""
    return _coarse_stage_backward("nerf_hip_coarse_composite_backward_distortion", t_c, sigma_c, rgb_c, near, far, delta0, dC_c, dt_f, dsig, drgb,
                                  rays=rays, mid=(_ptr(dmaps),), tail=(_ptr(ddist),), who="coarse_composite_backward_distortion_add")


def merge_composite_backward_distortion(bundle, perm, dC_f, Nc, near, far, ddist, last=1e-4, dmaps=None):
    """merge_composite_backward through k_merge_bwd_x<distortion> (nerf_hip_merge_composite_backward_distortion), with the upstream
    ddist[B,2] (column 1) of the fine distortion loss -> dsig_c, dsig_f, drgb_c, drgb_f, dt_f; the outputs start as NaN: the kernel writes
    every element"""
    nf = _near_far(near, far, bundle.device)
    return _merge_stage_backward("nerf_hip_merge_composite_backward_distortion", bundle, perm, dC_f, Nc, last, dmaps,
                                 tail=(nf.data_ptr(), _ptr(ddist)), who="merge_composite_backward_distortion")


def normal_composite(w, g, out=None, out_stride=3, rays=None, sentinel=float("nan")):
    """The k_normal_composite launch on its own (nerf_hip_normal_composite, rule NM of include/nerf_hip.h): weights w[B,N] and sigma
    gradients g[B,N,3] on the device -> out[B, out_stride] whose columns 0..2 are N = sum_i w_i n_i per ray and whose other columns keep
    `sentinel`.  rays: a call of the first `rays` rays only (default: all) -- the rows behind the call keep `sentinel` too."""
    B, N = w.shape
    rays = B if rays is None else int(rays)
    dev = w.device
    if out is None:
        out = torch.full((B, int(out_stride)), sentinel, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().nerf_hip_normal_composite(w.contiguous().data_ptr(), g.contiguous().data_ptr(), rays, N, out.data_ptr(),
                                                    int(out_stride), _stream(w)))
    return out


def forward_normals(params, row, col, poses_bound_f32, K_inv, Nc, Nf, flags=0, passes=2, ray0=None, last=1e-4, ws=None, nws=None,
                    sentinel=float("nan")):
    """One nerf_hip_forward_normals call: the maps call plus each ray's composited field normals (rule NM of include/nerf_hip.h).
    passes: bit 0 = coarse, bit 1 = fine.  -> (C_coarse[B,3], C_fine[B,3], maps[B,4], normals[B,2,3], ws, nws): row 0 / 1 of normals = the
    coarse / fine pass's N, a row not asked for keeps `sentinel`; ws / nws = the main and the side workspace the call ran on (uint8 device
    buffers of >= _abi.ws_bytes(B, Nc, Nf, flags) / _abi.normals_ws_bytes(B, Nc, Nf) bytes, allocated here if None).  ray0: the (near, far)
    of the batch's global ray 0 (two host floats) or None."""
    B, dev = row.shape[0], row.device
    if ws is None:
        ws = torch.zeros(_abi.ws_bytes(B, Nc, Nf, flags), dtype=torch.uint8, device=dev)
    if nws is None:
        nws = torch.empty(_abi.normals_ws_bytes(B, Nc, Nf), dtype=torch.uint8, device=dev)
    C_c = torch.empty(B, 3, dtype=torch.float32, device=dev)
    C_f = torch.empty(B, 3, dtype=torch.float32, device=dev)
    maps = torch.empty(B, 4, dtype=torch.float32, device=dev)
    nrm = torch.full((B, 2, 3), sentinel, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().nerf_hip_forward_normals(_abi.ptr_array(params), row.data_ptr(), col.data_ptr(), poses_bound_f32.data_ptr(),
                                                   _k9(K_inv), None if ray0 is None else _abi.f32_array(ray0), B, Nc, Nf, float(last),
                                                   C_c.data_ptr(), C_f.data_ptr(), maps.data_ptr(), ws.data_ptr(), ws.numel(), int(flags),
                                                   _stream(row), int(passes), nrm.data_ptr(), nws.data_ptr(), nws.numel()))
    return C_c, C_f, maps, nrm, ws, nws


def _vol_f32(t, what, shape=None):
    if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous fp32 device tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} {tuple(t.shape)}: {tuple(shape)}")
    return t


def _vol_index(index, dev):
    index = index.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    return index, int(index.shape[0])


def volume_active(sigma, ws=None):
    """The ACTIVE lattice points of sigma[nx, ny, nz] (rule VA of include/nerf_hip.h: a positive sigma in the clipped 3 x 3 x 3
    neighbourhood) -> their linear indices, int32, ascending (nerf_hip_volume_active_count, one 8-byte read of the device count -- this
    synchronises with the stream --, then nerf_hip_volume_active_emit)."""
    sigma = _vol_f32(sigma, "sigma")
    if sigma.dim() != 3:
        raise ValueError(f"sigma {tuple(sigma.shape)}: [nx, ny, nz]")
    nx, ny, nz = (int(n) for n in sigma.shape)
    dev = sigma.device
    if ws is None:
        ws = torch.empty(_abi.volume_ws_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    L, st = _abi.lib(), _stream(sigma)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _abi.check(L.nerf_hip_volume_active_count(sigma.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(), count.data_ptr(), st))
    n = int(count.cpu())
    index = torch.empty(n, dtype=torch.int32, device=dev)
    _abi.check(L.nerf_hip_volume_active_emit(sigma.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(), index.data_ptr() if n else None, n, st))
    return index


def volume_points(index, shape, lo, step):
    """The lattice points lo + (i, j, k) * step of the linear indices index[n] (int32, device) of a lattice of ``shape``
    (nerf_hip_volume_points) -> points[n, 3] fp32.  Enqueue only."""
    if index.device.type != "cuda":
        raise ValueError("index: a device tensor")
    index, n = _vol_index(index, index.device)
    nx, ny, nz = (int(x) for x in shape)
    points = torch.empty(n, 3, device=index.device)
    _abi.check(_abi.lib().nerf_hip_volume_points(index.data_ptr() if n else None, n, nx, ny, nz, _abi.f32_array(lo), _abi.f32_array(step),
                                                 points.data_ptr() if n else None, _stream(index)))
    return points


def volume_sh_accumulate(coef, index, rgb, k):
    """Quadrature direction k's term of rule VS added IN PLACE to the coefficients coef[nx, ny, nz, ncoef, 3] of the points index[n]:
    rgb[n, 3] is query()'s colour at those points along direction k (nerf_hip_volume_sh_accumulate).  Enqueue only."""
    coef = _vol_f32(coef, "coef")
    if coef.dim() != 5 or coef.shape[4] != 3 or int(coef.shape[3]) not in (1, 4, 9):
        raise ValueError(f"coef {tuple(coef.shape)}: [nx, ny, nz, (degree + 1)^2, 3]")
    index, n = _vol_index(index, coef.device)
    rgb = _vol_f32(rgb.to(coef.device, torch.float32).contiguous(), "rgb", (n, 3))
    nx, ny, nz, nc = (int(x) for x in coef.shape[:4])
    _abi.check(_abi.lib().nerf_hip_volume_sh_accumulate(coef.data_ptr(), nx, ny, nz, {1: 0, 4: 1, 9: 2}[nc], index.data_ptr() if n else None, n,
                                                        rgb.data_ptr() if n else None, int(k), _stream(coef)))
    return coef


def volume_block_dims(shape, block):
    """Blocks per axis of rule VO: ceil((n - 1) / block)."""
    return tuple((int(n) - 1 + int(block) - 1) // int(block) for n in shape)


def volume_blocks(sigma, block):
    """Rule VO's block occupancy of sigma[nx, ny, nz] for blocks of ``block`` cells per axis (nerf_hip_volume_blocks) ->
    occ[bx, by, bz] uint8.  Enqueue only."""
    sigma = _vol_f32(sigma, "sigma")
    if sigma.dim() != 3:
        raise ValueError(f"sigma {tuple(sigma.shape)}: [nx, ny, nz]")
    if int(block) != block or int(block) < 1:
        raise ValueError(f"block={block!r}: an int >= 1")
    block = min(int(block), 2**31 - 1)
    nx, ny, nz = (int(n) for n in sigma.shape)
    occ = torch.empty(volume_block_dims((max(nx, 2), max(ny, 2), max(nz, 2)), block), dtype=torch.uint8, device=sigma.device)
    _abi.check(_abi.lib().nerf_hip_volume_blocks(sigma.data_ptr(), nx, ny, nz, block, occ.data_ptr(), _stream(sigma)))
    return occ


def _vol_arrays(sigma, coef):
    sigma = _vol_f32(sigma, "sigma")
    if sigma.dim() != 3:
        raise ValueError(f"sigma {tuple(sigma.shape)}: [nx, ny, nz]")
    coef = _vol_f32(coef, "coef")
    if coef.dim() != 5 or tuple(coef.shape[:3]) != tuple(sigma.shape) or coef.shape[4] != 3 or int(coef.shape[3]) not in (1, 4, 9):
        raise ValueError(f"coef {tuple(coef.shape)}: sigma's shape {tuple(sigma.shape)}, then [(degree + 1)^2, 3]")
    if coef.device != sigma.device:
        raise ValueError("sigma and coef live on different devices")
    return sigma, coef, tuple(int(n) for n in sigma.shape), {1: 0, 4: 1, 9: 2}[int(coef.shape[3])]


def volume_sample(sigma, coef, lo, step, points, dirs):
    """Rule VL: the volume (sigma[nx, ny, nz], coef[nx, ny, nz, ncoef, 3]) on the lattice lo + (i, j, k) * step looked up at points[M, 3]
    along dirs[M, 3] (nerf_hip_volume_sample) -> (sigma[M], rgb[M, 3]) fp32; a point outside the lattice gives zeros.  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    dev = sigma.device
    points = points.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    if dirs.shape != points.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and points {tuple(points.shape)} differ")
    M = int(points.shape[0])
    out_s = torch.empty(M, device=dev)
    out_c = torch.empty(M, 3, device=dev)
    ptr = lambda t: t.data_ptr() if M else None
    _abi.check(_abi.lib().nerf_hip_volume_sample(sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree, _abi.f32_array(lo), _abi.f32_array(step),
                                                 ptr(points), ptr(dirs), M, ptr(out_s), ptr(out_c), _stream(sigma)))
    return out_s, out_c


def volume_render(sigma, coef, occ, block, lo, step, origins, dirs, tmin, tmax, dt, t_stop=0.0, background=(0.0, 0.0, 0.0)):
    """Rule VR: the rays (origins[N, 3], dirs[N, 3], windows tmin[N] .. tmax[N]) marched through the volume in steps of dt
    (nerf_hip_volume_render); occ is volume_blocks(sigma, block) -> (rgb[N, 3], maps[N, 2] = (D, A) fp32, steps[N, 2] int32 =
    (contributing, evaluated)).  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    dev = sigma.device
    block = min(int(block), 2**31 - 1)
    if occ.device != dev or occ.dtype != torch.uint8 or not occ.is_contiguous() or (
            block >= 1 and tuple(occ.shape) != volume_block_dims((nx, ny, nz), block)):
        raise ValueError(f"occ {tuple(occ.shape)} {occ.dtype}: the contiguous uint8 block occupancy of sigma for block={block}")
    origins = origins.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    N = int(origins.shape[0])
    if dirs.shape != origins.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and origins {tuple(origins.shape)} differ")
    win = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev).expand(N).contiguous() if torch.as_tensor(t).dim() == 0 else \
        torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    tmin, tmax = win(tmin), win(tmax)
    if tmin.shape[0] != N or tmax.shape[0] != N:
        raise ValueError(f"tmin / tmax: a scalar or one entry per ray ({N})")
    rgb = torch.empty(N, 3, device=dev)
    maps = torch.empty(N, 2, device=dev)
    steps = torch.empty(N, 2, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if N else None
    _abi.check(_abi.lib().nerf_hip_volume_render(sigma.data_ptr(), coef.data_ptr(), occ.data_ptr(), nx, ny, nz, degree, block,
                                                 _abi.f32_array(lo), _abi.f32_array(step), ptr(origins), ptr(dirs), ptr(tmin), ptr(tmax), N,
                                                 float(dt), float(t_stop), _abi.f32_array(background), ptr(rgb), ptr(maps), ptr(steps),
                                                 _stream(sigma)))
    return rgb, maps, steps


def _vol_acc(t, what, shape):
    if t.device.type != "cuda" or t.dtype != torch.int64 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: a contiguous int64 device tensor of shape {tuple(shape)}")
    return t


def volume_render_backward(sigma, coef, occ, block, lo, step, origins, dirs, tmin, tmax, dt, t_stop, background, g_rgb, g_maps, acc_sigma,
                           acc_coef):
    """Rule VG: the gradient of volume_render's march for the upstream g_rgb[N, 3] and g_maps[N, 2] (or None), ADDED IN PLACE to the int64
    fixed-point accumulators acc_sigma (sigma's shape) and acc_coef (coef's shape), in units of 2^-40
    (nerf_hip_volume_render_backward).  The kernel recomputes the march.  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    dev = sigma.device
    block = min(int(block), 2**31 - 1)
    if occ.device != dev or occ.dtype != torch.uint8 or not occ.is_contiguous() or (
            block >= 1 and tuple(occ.shape) != volume_block_dims((nx, ny, nz), block)):
        raise ValueError(f"occ {tuple(occ.shape)} {occ.dtype}: the contiguous uint8 block occupancy of sigma for block={block}")
    acc_sigma = _vol_acc(acc_sigma, "acc_sigma", sigma.shape)
    acc_coef = _vol_acc(acc_coef, "acc_coef", coef.shape)
    origins = origins.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    N = int(origins.shape[0])
    if dirs.shape != origins.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and origins {tuple(origins.shape)} differ")
    win = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev).expand(N).contiguous() if torch.as_tensor(t).dim() == 0 else \
        torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    tmin, tmax = win(tmin), win(tmax)
    if tmin.shape[0] != N or tmax.shape[0] != N:
        raise ValueError(f"tmin / tmax: a scalar or one entry per ray ({N})")
    g_rgb = _vol_f32(g_rgb.detach().to(dev, torch.float32).contiguous(), "g_rgb", (N, 3))
    if g_maps is not None:
        g_maps = _vol_f32(g_maps.detach().to(dev, torch.float32).contiguous(), "g_maps", (N, 2))
    ptr = lambda t: t.data_ptr() if N else None
    _abi.check(_abi.lib().nerf_hip_volume_render_backward(sigma.data_ptr(), coef.data_ptr(), occ.data_ptr(), nx, ny, nz, degree, block,
                                                          _abi.f32_array(lo), _abi.f32_array(step), ptr(origins), ptr(dirs), ptr(tmin),
                                                          ptr(tmax), N, float(dt), float(t_stop), _abi.f32_array(background), ptr(g_rgb),
                                                          ptr(g_maps) if g_maps is not None else None, acc_sigma.data_ptr(),
                                                          acc_coef.data_ptr(), _stream(sigma)))


def volume_adam_step(sigma, coef, index, acc_sigma, acc_coef, m, v, grad_scale, step, lr_sigma, lr_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    """Rule VU: one Adam step IN PLACE over the words of the points index[n] (int32, device: the ascending active list of the volume as
    baked) from the fixed-point accumulators, which are zeroed; m, v [n, 1 + 3 ncoef] fp32 are the moments (nerf_hip_volume_adam_step).
    A sigma that is not > 0 stays as it is, with its moments.  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    dev = sigma.device
    if not torch.is_tensor(index) or index.device.type != "cuda":
        raise ValueError("index: a device tensor")
    index, n = _vol_index(index, dev)
    acc_sigma = _vol_acc(acc_sigma, "acc_sigma", sigma.shape)
    acc_coef = _vol_acc(acc_coef, "acc_coef", coef.shape)
    words = 1 + 3 * int(coef.shape[3])
    m = _vol_f32(m, "m", (n, words))
    v = _vol_f32(v, "v", (n, words))
    ptr = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_adam_step(sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree, ptr(index), n, acc_sigma.data_ptr(),
                                                    acc_coef.data_ptr(), ptr(m), ptr(v), float(grad_scale), int(step), float(lr_sigma),
                                                    float(lr_coef), float(beta1), float(beta2), float(eps), _stream(sigma)))


def volume_member_mask(index, shape):
    """Rule VM: member[nx, ny, nz] uint8, 1 at the lattice points of index[n] (int32, device) and 0 elsewhere
    (nerf_hip_volume_member_mask).  Enqueue only."""
    if not torch.is_tensor(index) or index.device.type != "cuda":
        raise ValueError("index: a device tensor")
    index, n = _vol_index(index, index.device)
    nx, ny, nz = (int(x) for x in shape)
    member = torch.empty(nx, ny, nz, dtype=torch.uint8, device=index.device)
    _abi.check(_abi.lib().nerf_hip_volume_member_mask(index.data_ptr() if n else None, n, nx, ny, nz, member.data_ptr(), _stream(index)))
    return member


def volume_tv_backward(sigma, coef, index, member, w_sigma, w_coef, eps, acc_sigma, acc_coef):
    """Rule VT: the gradient of w_sigma sum_p tau_sigma(p) + w_coef sum_p sum_words tau(p) over the members, ADDED IN PLACE to rule VG's
    int64 accumulators for the words of the points index[n] (int32, device, distinct: the level's active list or a chunk of it); member
    is volume_member_mask of the WHOLE list (nerf_hip_volume_tv_backward).  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    dev = sigma.device
    if not torch.is_tensor(index) or index.device.type != "cuda":
        raise ValueError("index: a device tensor")
    index, n = _vol_index(index, dev)
    if member.device != dev or member.dtype != torch.uint8 or not member.is_contiguous() or tuple(member.shape) != (nx, ny, nz):
        raise ValueError(f"member {tuple(member.shape)} {member.dtype}: the contiguous uint8 mask of sigma's shape {(nx, ny, nz)}")
    acc_sigma = _vol_acc(acc_sigma, "acc_sigma", sigma.shape)
    acc_coef = _vol_acc(acc_coef, "acc_coef", coef.shape)
    _abi.check(_abi.lib().nerf_hip_volume_tv_backward(sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree, index.data_ptr() if n else None, n,
                                                      member.data_ptr(), float(w_sigma), float(w_coef), float(eps), acc_sigma.data_ptr(),
                                                      acc_coef.data_ptr(), _stream(sigma)))


def volume_upsample(sigma, coef):
    """Rule VX: the volume on the lattice of 2 n - 1 points per axis (nerf_hip_volume_upsample) -> (sigma2, coef2), new tensors.
    Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    shape2 = (2 * nx - 1, 2 * ny - 1, 2 * nz - 1)
    if shape2[0] * shape2[1] * shape2[2] >= 2**31:
        raise ValueError(f"volume {(nx, ny, nz)}: the refined lattice {shape2} must stay below 2^31 points")
    sigma2 = torch.empty(shape2, device=sigma.device)
    coef2 = torch.empty(shape2 + tuple(coef.shape[3:]), device=sigma.device)
    _abi.check(_abi.lib().nerf_hip_volume_upsample(sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree, sigma2.data_ptr(), coef2.data_ptr(),
                                                   _stream(sigma)))
    return sigma2, coef2


def volume_prune(sigma, coef, threshold):
    """Rule VP IN PLACE: sigma not > threshold becomes +0, then the coefficients of the points that are not active (rule VA) in the
    result become +0 (nerf_hip_volume_prune).  Enqueue only."""
    sigma, coef, (nx, ny, nz), degree = _vol_arrays(sigma, coef)
    _abi.check(_abi.lib().nerf_hip_volume_prune(sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree, float(threshold), _stream(sigma)))
    return sigma, coef


def volume_row_width(degree, half):
    """Rule VC: the words of a stored coefficient row -- 3 (degree + 1)^2 fp32 words, or that many halves rounded up to a multiple of 4."""
    w = 3 * (int(degree) + 1) ** 2
    return (w + 3) & ~3 if half else w


def _vol_compact(slot, sigma_rows, coef_rows, degree):
    """The arrays of a compact volume, checked -> ((nx, ny, nz), n, half)."""
    if slot.device.type != "cuda" or slot.dtype != torch.int32 or not slot.is_contiguous() or slot.dim() != 3:
        raise ValueError(f"slot {tuple(slot.shape)} {slot.dtype}: a contiguous int32 device tensor [nx, ny, nz]")
    if degree not in (0, 1, 2):
        raise ValueError(f"degree={degree!r}: 0, 1 or 2")
    sigma_rows = _vol_f32(sigma_rows, "sigma rows")
    n = int(sigma_rows.shape[0])
    if coef_rows.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"coefficient rows {coef_rows.dtype}: fp32 or fp16")
    half = coef_rows.dtype == torch.float16
    if (coef_rows.device != slot.device or sigma_rows.device != slot.device or not coef_rows.is_contiguous() or sigma_rows.dim() != 1
            or tuple(coef_rows.shape) != (n, volume_row_width(degree, half))):
        raise ValueError(f"rows {tuple(sigma_rows.shape)} / {tuple(coef_rows.shape)}: [n] and [n, {volume_row_width(degree, half)}] on the slots' device")
    return tuple(int(x) for x in slot.shape), n, int(half)


def volume_compact_slots(index, shape):
    """Rule VC's slot lattice of the active list index[n] (int32, ascending, device) of a lattice of ``shape``
    (nerf_hip_volume_compact_slots) -> slot[nx, ny, nz] int32: the row of the point, -1 where there is none.  Enqueue only."""
    if index.device.type != "cuda":
        raise ValueError("index: a device tensor")
    index, n = _vol_index(index, index.device)
    nx, ny, nz = (int(x) for x in shape)
    slot = torch.empty(nx, ny, nz, dtype=torch.int32, device=index.device)
    _abi.check(_abi.lib().nerf_hip_volume_compact_slots(index.data_ptr() if n else None, n, nx, ny, nz, slot.data_ptr(), _stream(index)))
    return slot


def volume_compact_pack(sigma, coef, index, half):
    """Rule VC's PACK (nerf_hip_volume_compact_pack): the rows of the points index[n] of the dense coef[nx, ny, nz, ncoef, 3] and, unless
    ``sigma`` is None, sigma[nx, ny, nz] -> (sigma_rows [n] fp32 or None, coef_rows [n, S] fp32 or, with ``half``, fp16 with the pad
    halves +0).  index = None: every lattice point in order -- the conversion of fp32 rows seen as a lattice to fp16.  Enqueue only."""
    coef = _vol_f32(coef, "coef")
    if coef.dim() != 5 or coef.shape[4] != 3 or int(coef.shape[3]) not in (1, 4, 9):
        raise ValueError(f"coef {tuple(coef.shape)}: [nx, ny, nz, (degree + 1)^2, 3]")
    nx, ny, nz, nc = (int(x) for x in coef.shape[:4])
    degree = {1: 0, 4: 1, 9: 2}[nc]
    dev = coef.device
    if sigma is not None:
        sigma = _vol_f32(sigma, "sigma", (nx, ny, nz))
    if index is None:
        n = nx * ny * nz
    else:
        index, n = _vol_index(index, dev)
    sigma_rows = None if sigma is None else torch.empty(n, device=dev)
    coef_rows = torch.empty(n, volume_row_width(degree, half), dtype=torch.float16 if half else torch.float32, device=dev)
    ptr = lambda t: t.data_ptr() if (t is not None and n) else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_pack(None if sigma is None else sigma.data_ptr(), coef.data_ptr(), nx, ny, nz, degree,
                                                       ptr(index), n, int(bool(half)), None if sigma is None else ptr(sigma_rows),
                                                       ptr(coef_rows), _stream(coef)))
    return sigma_rows, coef_rows


def volume_compact_unpack(sigma_rows, coef_rows, index, shape, degree):
    """Rule VC's UNPACK (nerf_hip_volume_compact_unpack): the rows scattered to the points index[n] of zeroed dense arrays, fp16 widened
    -> (sigma [nx, ny, nz], coef [nx, ny, nz, ncoef, 3]) fp32; coef_rows = None: (sigma, None).  Enqueue only."""
    sigma_rows = _vol_f32(sigma_rows, "sigma rows")
    dev = sigma_rows.device
    index, n = _vol_index(index, dev)
    nx, ny, nz = (int(x) for x in shape)
    nc = (int(degree) + 1) ** 2
    half = coef_rows is not None and coef_rows.dtype == torch.float16
    if sigma_rows.dim() != 1 or int(sigma_rows.shape[0]) != n:
        raise ValueError(f"sigma rows {tuple(sigma_rows.shape)}: one per index ({n})")
    if coef_rows is not None and (coef_rows.device != dev or coef_rows.dtype not in (torch.float32, torch.float16) or not coef_rows.is_contiguous()
                                  or tuple(coef_rows.shape) != (n, volume_row_width(degree, half))):
        raise ValueError(f"coefficient rows {tuple(coef_rows.shape)} {coef_rows.dtype}: contiguous fp32 / fp16 [{n}, {volume_row_width(degree, half)}]")
    sigma = torch.zeros(nx, ny, nz, device=dev)
    coef = None if coef_rows is None else torch.zeros(nx, ny, nz, nc, 3, device=dev)
    ptr = lambda t: t.data_ptr() if (t is not None and n) else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_unpack(ptr(sigma_rows), ptr(coef_rows), int(half), ptr(index), n, nx, ny, nz, int(degree),
                                                         sigma.data_ptr(), None if coef is None else coef.data_ptr(), _stream(sigma_rows)))
    return sigma, coef


def volume_compact_sample(slot, sigma_rows, coef_rows, degree, lo, step, points, dirs):
    """Rule VC-L: volume_sample over the compact form (nerf_hip_volume_compact_sample) -> (sigma[M], rgb[M, 3]) fp32.  Enqueue only."""
    (nx, ny, nz), n, half = _vol_compact(slot, sigma_rows, coef_rows, degree)
    dev = slot.device
    points = points.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    if dirs.shape != points.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and points {tuple(points.shape)} differ")
    M = int(points.shape[0])
    out_s = torch.empty(M, device=dev)
    out_c = torch.empty(M, 3, device=dev)
    ptr = lambda t: t.data_ptr() if M else None
    row = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_sample(slot.data_ptr(), row(sigma_rows), row(coef_rows), n, half, nx, ny, nz, int(degree),
                                                         _abi.f32_array(lo), _abi.f32_array(step), ptr(points), ptr(dirs), M, ptr(out_s),
                                                         ptr(out_c), _stream(slot)))
    return out_s, out_c


def volume_compact_render(slot, sigma_rows, coef_rows, degree, occ, block, lo, step, origins, dirs, tmin, tmax, dt, t_stop=0.0,
                          background=(0.0, 0.0, 0.0)):
    """Rule VC-R: volume_render over the compact form (nerf_hip_volume_compact_render) -> (rgb[N, 3], maps[N, 2] fp32, steps[N, 2]
    int32).  Enqueue only."""
    (nx, ny, nz), n, half = _vol_compact(slot, sigma_rows, coef_rows, degree)
    dev = slot.device
    block = min(int(block), 2**31 - 1)
    if occ.device != dev or occ.dtype != torch.uint8 or not occ.is_contiguous() or (
            block >= 1 and tuple(occ.shape) != volume_block_dims((nx, ny, nz), block)):
        raise ValueError(f"occ {tuple(occ.shape)} {occ.dtype}: the contiguous uint8 block occupancy of sigma for block={block}")
    origins = origins.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    N = int(origins.shape[0])
    if dirs.shape != origins.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and origins {tuple(origins.shape)} differ")
    win = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev).expand(N).contiguous() if torch.as_tensor(t).dim() == 0 else \
        torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    tmin, tmax = win(tmin), win(tmax)
    if tmin.shape[0] != N or tmax.shape[0] != N:
        raise ValueError(f"tmin / tmax: a scalar or one entry per ray ({N})")
    rgb = torch.empty(N, 3, device=dev)
    maps = torch.empty(N, 2, device=dev)
    steps = torch.empty(N, 2, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if N else None
    row = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_render(slot.data_ptr(), row(sigma_rows), row(coef_rows), n, half, occ.data_ptr(), nx, ny, nz,
                                                         int(degree), block, _abi.f32_array(lo), _abi.f32_array(step), ptr(origins),
                                                         ptr(dirs), ptr(tmin), ptr(tmax), N, float(dt), float(t_stop),
                                                         _abi.f32_array(background), ptr(rgb), ptr(maps), ptr(steps), _stream(slot)))
    return rgb, maps, steps


def _vol_compact_train(slot, sigma_rows, coef_rows, degree, acc_sigma_rows, acc_coef_rows):
    """The arrays of a compact volume under training: fp32 rows and one int64 accumulator word per row word -> ((nx, ny, nz), n)."""
    shape, n, half = _vol_compact(slot, sigma_rows, coef_rows, degree)
    if half:
        raise ValueError("coefficient rows torch.float16: a compact volume is trained on fp32 rows")
    _vol_acc(acc_sigma_rows, "acc_sigma rows", (n,))
    _vol_acc(acc_coef_rows, "acc_coef rows", (n, volume_row_width(degree, False)))
    if acc_sigma_rows.device != slot.device or acc_coef_rows.device != slot.device:
        raise ValueError("the accumulators and the slots live on different devices")
    return shape, n


def volume_compact_render_backward(slot, sigma_rows, coef_rows, degree, occ, block, lo, step, origins, dirs, tmin, tmax, dt, t_stop,
                                   background, g_rgb, g_maps, acc_sigma_rows, acc_coef_rows):
    """Rule VCG: volume_render_backward over the compact form with fp32 rows, ADDED IN PLACE to the per-row int64 accumulators
    acc_sigma_rows [n] and acc_coef_rows [n, 3 ncoef] (nerf_hip_volume_compact_render_backward).  Enqueue only."""
    (nx, ny, nz), n = _vol_compact_train(slot, sigma_rows, coef_rows, degree, acc_sigma_rows, acc_coef_rows)
    dev = slot.device
    block = min(int(block), 2**31 - 1)
    if occ.device != dev or occ.dtype != torch.uint8 or not occ.is_contiguous() or (
            block >= 1 and tuple(occ.shape) != volume_block_dims((nx, ny, nz), block)):
        raise ValueError(f"occ {tuple(occ.shape)} {occ.dtype}: the contiguous uint8 block occupancy of sigma for block={block}")
    origins = origins.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    N = int(origins.shape[0])
    if dirs.shape != origins.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and origins {tuple(origins.shape)} differ")
    win = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev).expand(N).contiguous() if torch.as_tensor(t).dim() == 0 else \
        torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    tmin, tmax = win(tmin), win(tmax)
    if tmin.shape[0] != N or tmax.shape[0] != N:
        raise ValueError(f"tmin / tmax: a scalar or one entry per ray ({N})")
    g_rgb = _vol_f32(g_rgb.detach().to(dev, torch.float32).contiguous(), "g_rgb", (N, 3))
    if g_maps is not None:
        g_maps = _vol_f32(g_maps.detach().to(dev, torch.float32).contiguous(), "g_maps", (N, 2))
    ptr = lambda t: t.data_ptr() if N else None
    row = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_render_backward(
        slot.data_ptr(), row(sigma_rows), row(coef_rows), n, occ.data_ptr(), nx, ny, nz, int(degree), block, _abi.f32_array(lo),
        _abi.f32_array(step), ptr(origins), ptr(dirs), ptr(tmin), ptr(tmax), N, float(dt), float(t_stop), _abi.f32_array(background), ptr(g_rgb),
        ptr(g_maps) if g_maps is not None else None, row(acc_sigma_rows), row(acc_coef_rows), _stream(slot)))


def volume_compact_adam_step(sigma_rows, coef_rows, degree, acc_sigma_rows, acc_coef_rows, m, v, grad_scale, step, lr_sigma, lr_coef,
                             beta1=0.9, beta2=0.999, eps=1e-8):
    """Rule VCU: one Adam step IN PLACE over the words of the fp32 rows from their fixed-point accumulators, which are zeroed; m, v
    [n, 1 + 3 ncoef] fp32 are the moments (nerf_hip_volume_compact_adam_step).  A row whose sigma is not > 0 keeps it, with its
    moments.  Enqueue only."""
    if degree not in (0, 1, 2):
        raise ValueError(f"degree={degree!r}: 0, 1 or 2")
    sigma_rows = _vol_f32(sigma_rows, "sigma rows")
    if sigma_rows.dim() != 1:
        raise ValueError(f"sigma rows {tuple(sigma_rows.shape)}: [n]")
    n, width = int(sigma_rows.shape[0]), volume_row_width(degree, False)
    coef_rows = _vol_f32(coef_rows, "coefficient rows", (n, width))
    _vol_acc(acc_sigma_rows, "acc_sigma rows", (n,))
    _vol_acc(acc_coef_rows, "acc_coef rows", (n, width))
    m = _vol_f32(m, "m", (n, 1 + width))
    v = _vol_f32(v, "v", (n, 1 + width))
    ptr = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_adam_step(ptr(sigma_rows), ptr(coef_rows), n, int(degree), ptr(acc_sigma_rows),
                                                            ptr(acc_coef_rows), ptr(m), ptr(v), float(grad_scale), int(step), float(lr_sigma),
                                                            float(lr_coef), float(beta1), float(beta2), float(eps), _stream(sigma_rows)))


def volume_compact_tv_backward(slot, sigma_rows, coef_rows, degree, point, w_sigma, w_coef, eps, acc_sigma_rows, acc_coef_rows):
    """Rule VCT: volume_tv_backward over the compact form with fp32 rows -- the members are the points whose slot lies in [0, n), point[n]
    (int32, device) is the lattice point of each row --, ADDED IN PLACE to the per-row accumulators
    (nerf_hip_volume_compact_tv_backward).  Enqueue only."""
    (nx, ny, nz), n = _vol_compact_train(slot, sigma_rows, coef_rows, degree, acc_sigma_rows, acc_coef_rows)
    if not torch.is_tensor(point) or point.device.type != "cuda":
        raise ValueError("point: a device tensor")
    point, npoint = _vol_index(point, slot.device)
    if npoint != n:
        raise ValueError(f"point {npoint}: one lattice point per row ({n})")
    row = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_tv_backward(slot.data_ptr(), row(sigma_rows), row(coef_rows), row(point), n, nx, ny, nz,
                                                              int(degree), float(w_sigma), float(w_coef), float(eps), row(acc_sigma_rows),
                                                              row(acc_coef_rows), _stream(slot)))


VQ_MAX_CODES = 65536   # NERF_HIP_VOLUME_VQ_MAX_CODES: a code is a uint16
VQ_SHIFT = 20          # NERF_HIP_VOLUME_VQ_SHIFT


def volume_compact_importance(slot, sigma_rows, occ, block, lo, step, origins, dirs, tmin, tmax, dt, t_stop, imp_rows):
    """Rule VI: volume_compact_render's march without a colour; every contributing sample's weight, split by the trilinear corner terms,
    ADDED IN PLACE to the int64 fixed-point words imp_rows [n] (units of 2^-40) of the corners that have a row
    (nerf_hip_volume_compact_importance) -> steps[N, 2] int32, volume_compact_render's own.  Enqueue only."""
    if slot.device.type != "cuda" or slot.dtype != torch.int32 or not slot.is_contiguous() or slot.dim() != 3:
        raise ValueError(f"slot {tuple(slot.shape)} {slot.dtype}: a contiguous int32 device tensor [nx, ny, nz]")
    dev = slot.device
    sigma_rows = _vol_f32(sigma_rows, "sigma rows")
    if sigma_rows.dim() != 1 or sigma_rows.device != dev:
        raise ValueError(f"sigma rows {tuple(sigma_rows.shape)}: [n] on the slots' device")
    n = int(sigma_rows.shape[0])
    _vol_acc(imp_rows, "imp rows", (n,))
    if imp_rows.device != dev:
        raise ValueError("the importance words and the slots live on different devices")
    nx, ny, nz = (int(x) for x in slot.shape)
    block = min(int(block), 2**31 - 1)
    if occ.device != dev or occ.dtype != torch.uint8 or not occ.is_contiguous() or (
            block >= 1 and tuple(occ.shape) != volume_block_dims((nx, ny, nz), block)):
        raise ValueError(f"occ {tuple(occ.shape)} {occ.dtype}: the contiguous uint8 block occupancy of sigma for block={block}")
    origins = origins.to(dev, torch.float32).reshape(-1, 3).contiguous()
    dirs = dirs.to(dev, torch.float32).reshape(-1, 3).contiguous()
    N = int(origins.shape[0])
    if dirs.shape != origins.shape:
        raise ValueError(f"dirs {tuple(dirs.shape)} and origins {tuple(origins.shape)} differ")
    win = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev).expand(N).contiguous() if torch.as_tensor(t).dim() == 0 else \
        torch.as_tensor(t).to(dev, torch.float32).reshape(-1).contiguous()
    tmin, tmax = win(tmin), win(tmax)
    if tmin.shape[0] != N or tmax.shape[0] != N:
        raise ValueError(f"tmin / tmax: a scalar or one entry per ray ({N})")
    steps = torch.empty(N, 2, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if N else None
    row = lambda t: t.data_ptr() if n else None
    _abi.check(_abi.lib().nerf_hip_volume_compact_importance(slot.data_ptr(), row(sigma_rows), n, occ.data_ptr(), nx, ny, nz, block,
                                                             _abi.f32_array(lo), _abi.f32_array(step), ptr(origins), ptr(dirs), ptr(tmin),
                                                             ptr(tmax), N, float(dt), float(t_stop), row(imp_rows), ptr(steps),
                                                             _stream(slot)))
    return steps


def _vq_rows(rows, what="rows"):
    """fp32 rows [m, W], W in (3, 12, 27) -> (m, degree)"""
    rows = _vol_f32(rows, what)
    if rows.dim() != 2 or int(rows.shape[1]) not in (3, 12, 27):
        raise ValueError(f"{what} {tuple(rows.shape)}: [m, 3 (degree + 1)^2]")
    return int(rows.shape[0]), {3: 0, 12: 1, 27: 2}[int(rows.shape[1])]


def _vq_codebook(codebook, degree, dev):
    K, d2 = _vq_rows(codebook, "codebook")
    if d2 != degree or codebook.device != dev:
        raise ValueError(f"codebook {tuple(codebook.shape)}: [K, {3 * (degree + 1) ** 2}] on the rows' device")
    if not 1 <= K <= VQ_MAX_CODES:
        raise ValueError(f"K={K}: a codebook has 1 .. {VQ_MAX_CODES} codes")
    return K


def volume_vq_assign(rows, codebook, with_dist=False):
    """Rule VQ-A: the nearest code of every fp32 row [m, W] in the fp32 codebook [K, W] under the fp32 running-sum distance, the lowest
    index on a tie (nerf_hip_volume_vq_assign) -> assign [m] int32, or (assign, dist [m] fp32).  Enqueue only."""
    m, degree = _vq_rows(rows)
    K = _vq_codebook(codebook, degree, rows.device)
    assign = torch.empty(m, dtype=torch.int32, device=rows.device)
    dist = torch.empty(m, device=rows.device) if with_dist else None
    ptr = lambda t: t.data_ptr() if (t is not None and m) else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_assign(ptr(rows), m, codebook.data_ptr(), K, degree, ptr(assign), ptr(dist), _stream(rows)))
    return (assign, dist) if with_dist else assign


def volume_vq_accumulate(rows, weight, imax, assign, K, sums=None, counts=None):
    """Rule VQ-U's ACCUMULATE: the weighted fixed-point sums of the rows of every code, ADDED to sums [K, W] and counts [K] (int64,
    units of 2^-20; zeroed buffers are made when None).  weight [m] int64 in [0, imax] or None (u = 1)
    (nerf_hip_volume_vq_accumulate) -> (sums, counts).  Enqueue only."""
    m, degree = _vq_rows(rows)
    dev, W = rows.device, int(rows.shape[1])
    K = int(K)
    if not 1 <= K <= VQ_MAX_CODES:
        raise ValueError(f"K={K}: a codebook has 1 .. {VQ_MAX_CODES} codes")
    if weight is not None:
        _vol_acc(weight, "weight", (m,))
    if assign.device != dev or assign.dtype != torch.int32 or not assign.is_contiguous() or tuple(assign.shape) != (m,):
        raise ValueError(f"assign: a contiguous int32 device tensor [{m}]")
    sums = torch.zeros(K, W, dtype=torch.int64, device=dev) if sums is None else _vol_acc(sums, "sums", (K, W))
    counts = torch.zeros(K, dtype=torch.int64, device=dev) if counts is None else _vol_acc(counts, "counts", (K,))
    ptr = lambda t: t.data_ptr() if (t is not None and m) else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_accumulate(ptr(rows), m, degree, ptr(weight), int(imax), ptr(assign), K, sums.data_ptr(),
                                                        counts.data_ptr(), _stream(rows)))
    return sums, counts


def volume_vq_update(codebook, sums, counts):
    """Rule VQ-U's UPDATE, IN PLACE: every word of a code with a positive count becomes (float)(sum / count); an empty code keeps its
    words (nerf_hip_volume_vq_update).  Enqueue only."""
    K, degree = _vq_rows(codebook, "codebook")
    K = _vq_codebook(codebook, degree, codebook.device)
    _vol_acc(sums, "sums", (K, int(codebook.shape[1])))
    _vol_acc(counts, "counts", (K,))
    _abi.check(_abi.lib().nerf_hip_volume_vq_update(codebook.data_ptr(), K, degree, sums.data_ptr(), counts.data_ptr(), _stream(codebook)))
    return codebook


def volume_vq_decode(cls, rank, code, kept, codebook, degree):
    """Rule VQ-D: cls [n] uint8 (0 pruned, 1 coded, 2 kept), rank [n] int32 (the rank within the class), code [n_coded] uint16, kept
    [n_kept, S] and codebook [K, S] fp16 -> the fp16 rows [n, S] of rule VC (nerf_hip_volume_vq_decode).  Enqueue only."""
    if degree not in (0, 1, 2):
        raise ValueError(f"degree={degree!r}: 0, 1 or 2")
    S = volume_row_width(degree, True)
    dev = cls.device
    if dev.type != "cuda" or cls.dtype != torch.uint8 or cls.dim() != 1 or not cls.is_contiguous():
        raise ValueError("cls: a contiguous uint8 device tensor [n]")
    n = int(cls.shape[0])
    if rank.device != dev or rank.dtype != torch.int32 or tuple(rank.shape) != (n,) or not rank.is_contiguous():
        raise ValueError(f"rank: a contiguous int32 device tensor [{n}]")
    if code.device != dev or code.dtype != torch.uint16 or code.dim() != 1 or not code.is_contiguous():
        raise ValueError("code: a contiguous uint16 device tensor [n_coded]")
    for t, what in ((kept, "kept"), (codebook, "codebook")):
        if t.device != dev or t.dtype != torch.float16 or t.dim() != 2 or int(t.shape[1]) != S or not t.is_contiguous():
            raise ValueError(f"{what} {tuple(t.shape)} {t.dtype}: a contiguous fp16 device tensor [., {S}]")
    n_coded, n_kept, K = int(code.shape[0]), int(kept.shape[0]), int(codebook.shape[0])
    if K > VQ_MAX_CODES:
        raise ValueError(f"K={K}: a codebook has at most {VQ_MAX_CODES} codes")
    out = torch.empty(n, S, dtype=torch.float16, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_decode(ptr(cls), ptr(rank), n, ptr(code), n_coded, ptr(kept), n_kept, ptr(codebook), K, int(degree),
                                                    ptr(out), _stream(cls)))
    return out


VQ_REDUCE_CHUNK = 256  # NERF_HIP_VOLUME_VQ_REDUCE_CHUNK: entries of member[] per workgroup of volume_vq_grad_reduce
VQ_MAX_RAYS = 2**20    # rule VQ-G's overflow precondition: rays per update


def _vq_classes(cls, rank, code):
    """cls [n] uint8, rank [n] int32, code [n_coded] uint16, contiguous on one device -> (n, n_coded)"""
    dev = cls.device
    if dev.type != "cuda" or cls.dtype != torch.uint8 or cls.dim() != 1 or not cls.is_contiguous():
        raise ValueError("cls: a contiguous uint8 device tensor [n]")
    n = int(cls.shape[0])
    if rank.device != dev or rank.dtype != torch.int32 or tuple(rank.shape) != (n,) or not rank.is_contiguous():
        raise ValueError(f"rank: a contiguous int32 device tensor [{n}]")
    if code.device != dev or code.dtype != torch.uint16 or code.dim() != 1 or not code.is_contiguous():
        raise ValueError("code: a contiguous uint16 device tensor [n_coded]")
    return n, int(code.shape[0])


def _vq_masters(kept32, codebook32, degree, dev):
    """the fp32 masters [n_kept, W] and [K, W] -> (n_kept, K)"""
    W = volume_row_width(degree, False)
    for t, what in ((kept32, "kept32"), (codebook32, "codebook32")):
        _vol_f32(t, what)
        if t.device != dev or t.dim() != 2 or int(t.shape[1]) != W:
            raise ValueError(f"{what} {tuple(t.shape)}: [., {W}] on the rows' device")
    K = int(codebook32.shape[0])
    if K > VQ_MAX_CODES:
        raise ValueError(f"K={K}: a codebook has at most {VQ_MAX_CODES} codes")
    return int(kept32.shape[0]), K


def volume_vq_expand(cls, rank, code, kept32, codebook32, degree, out=None, acc_coef_rows=None):
    """Rule VQ-X: rule VQ-D in fp32 and without pads -- the fp32 rows [n, 3 ncoef] of the classes (cls, rank, code) from the fp32
    masters kept32 [n_kept, W] and codebook32 [K, W]; whatever does not check out gives +0.  ``out``: the rows to overwrite (made when
    None).  ``acc_coef_rows`` [n, W] int64 or None: the accumulator words of every row that receives +0 are zeroed
    (nerf_hip_volume_vq_expand).  Enqueue only.  -> out"""
    if degree not in (0, 1, 2):
        raise ValueError(f"degree={degree!r}: 0, 1 or 2")
    n, n_coded = _vq_classes(cls, rank, code)
    dev, W = cls.device, volume_row_width(degree, False)
    n_kept, K = _vq_masters(kept32, codebook32, degree, dev)
    out = torch.empty(n, W, device=dev) if out is None else _vol_f32(out, "coefficient rows", (n, W))
    if acc_coef_rows is not None:
        _vol_acc(acc_coef_rows, "acc_coef rows", (n, W))
    ptr = lambda t: t.data_ptr() if (t is not None and t.numel()) else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_expand(ptr(cls), ptr(rank), n, ptr(code), n_coded, ptr(kept32), n_kept, ptr(codebook32), K,
                                                    int(degree), ptr(out), ptr(acc_coef_rows), _stream(cls)))
    return out


def volume_vq_grad_reduce(acc_coef_rows, offset, member, acc_code):
    """Rule VQ-G: the rows' int64 accumulator words acc_coef_rows [n, W] summed into their codes' acc_code [K, W] (ADDED IN PLACE) and
    zeroed; the coded rows are given grouped by code, member [n_coded] int32 with offset [K + 1] int32 (device).  Integer adds: the same
    bits whatever the order of the members or the launch (nerf_hip_volume_vq_grad_reduce).  Enqueue only.  -> acc_code"""
    if acc_coef_rows.dim() != 2 or int(acc_coef_rows.shape[1]) not in (3, 12, 27):
        raise ValueError(f"acc_coef rows {tuple(acc_coef_rows.shape)}: [n, 3 (degree + 1)^2]")
    n, W = (int(x) for x in acc_coef_rows.shape)
    _vol_acc(acc_coef_rows, "acc_coef rows", (n, W))
    dev = acc_coef_rows.device
    if acc_code.dim() != 2:
        raise ValueError(f"acc_code {tuple(acc_code.shape)}: [K, {W}]")
    K = int(acc_code.shape[0])
    _vol_acc(acc_code, "acc_code", (K, W))
    if K > VQ_MAX_CODES:
        raise ValueError(f"K={K}: a codebook has at most {VQ_MAX_CODES} codes")
    for t, what, shape in ((offset, "offset", (K + 1,)), (member, "member", None)):
        if t.device != dev or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or (shape and tuple(t.shape) != shape):
            raise ValueError(f"{what}: a contiguous int32 tensor {list(shape) if shape else '[n_coded]'} on the accumulators' device")
    n_coded = int(member.shape[0])
    if acc_code.device != dev:
        raise ValueError("acc_code and the rows' accumulators live on different devices")
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_grad_reduce(ptr(acc_coef_rows), n, {3: 0, 12: 1, 27: 2}[W], ptr(offset), ptr(member), n_coded, K,
                                                         ptr(acc_code), _stream(acc_coef_rows)))
    return acc_code


def volume_vq_adam_step(sigma_rows, kept32, kept_row, codebook32, degree, acc_sigma_rows, acc_coef_rows, acc_code, m, v, grad_scale, step,
                        lr_sigma, lr_coef, beta1=0.9, beta2=0.999, eps=1e-8):
    """Rule VQ-V: one Adam step IN PLACE over the sigma word of every row (frozen support, lr_sigma), the words of the kept rows'
    masters kept32 [n_kept, W] (their accumulators are those of the rows kept_row [n_kept] int32) and the words of codebook32 [K, W]
    (accumulators acc_code [K, W]); every accumulator word read is zeroed; m, v [n + n_kept W + K W] fp32 hold the moments in that
    order (nerf_hip_volume_vq_adam_step).  Enqueue only."""
    if degree not in (0, 1, 2):
        raise ValueError(f"degree={degree!r}: 0, 1 or 2")
    sigma_rows = _vol_f32(sigma_rows, "sigma rows")
    if sigma_rows.dim() != 1:
        raise ValueError(f"sigma rows {tuple(sigma_rows.shape)}: [n]")
    n, W, dev = int(sigma_rows.shape[0]), volume_row_width(degree, False), sigma_rows.device
    n_kept, K = _vq_masters(kept32, codebook32, degree, dev)
    if kept_row.device != dev or kept_row.dtype != torch.int32 or tuple(kept_row.shape) != (n_kept,) or not kept_row.is_contiguous():
        raise ValueError(f"kept_row: a contiguous int32 device tensor [{n_kept}]")
    _vol_acc(acc_sigma_rows, "acc_sigma rows", (n,))
    _vol_acc(acc_coef_rows, "acc_coef rows", (n, W))
    _vol_acc(acc_code, "acc_code", (K, W))
    words = n + (n_kept + K) * W
    m = _vol_f32(m, "m", (words,))
    v = _vol_f32(v, "v", (words,))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _abi.check(_abi.lib().nerf_hip_volume_vq_adam_step(ptr(sigma_rows), n, ptr(kept32), ptr(kept_row), n_kept, ptr(codebook32), K, int(degree),
                                                       ptr(acc_sigma_rows), ptr(acc_coef_rows), ptr(acc_code), ptr(m), ptr(v),
                                                       float(grad_scale), int(step), float(lr_sigma), float(lr_coef), float(beta1),
                                                       float(beta2), float(eps), _stream(sigma_rows)))
