// api_geometry.hip -- the geometry part of the extern "C" surface of libnerf_hip.so (include/nerf_hip.h): point and gradient queries,
// density grids, marching cubes, the narrow band, mesh components, mesh simplification, mesh edges / smoothing / normals, mesh
// measures / samples / nearest points / distance statistics, ray casting / face visibility / face selection, TSDF fusion and image metrics.  Host code only, as api.hip: argument checks,
// workspace carve-up and kernel sequencing on the caller's stream.  No allocation, no host sync.
#include <math.h>

#include "api_common.h"

using namespace nerf;

namespace {

// Workspace of the point queries: the packed weight image, the fold, and (colour queries) the dvec rows of ONE chunk of QUERY_CHUNK points.
// Nothing in it depends on the number of points or the grid size.
struct QueryLayout {
  size_t packed, fold, dvec, total;
};
QueryLayout query_layout(bool rgb) {
  QueryLayout L;
  Carve c;
  L.packed = c.take((size_t)PACKED_ALL_F4 * 16);  // (the extent the register kernels' buffer resource declares: reg_buf)
  L.fold = c.take((size_t)FOLD_FLOATS * 4);
  L.dvec = rgb ? c.take((size_t)QUERY_CHUNK * HALF * 4) : 0;
  L.total = c.o;
  return L;
}

}  // namespace

extern "C" {

int nerf_hip_query_ws_bytes(int with_rgb, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  *bytes = query_layout(with_rgb != 0).total;
  return NERF_HIP_OK;
}

int nerf_hip_query(const float* const* weights24, const float* points, const float* dirs, int M, float* rgb, float* sigma, void* ws,
                   size_t ws_bytes, void* stream) {
  if (M < 0) return fail(NERF_HIP_ERR_ARG, "M=%d < 0", M);
  if ((dirs == nullptr) != (rgb == nullptr)) return fail(NERF_HIP_ERR_ARG, "dirs and rgb must both be null (sigma only) or both be set");
  const bool with_rgb = dirs != nullptr;
  if (M == 0) return NERF_HIP_OK;
  if (int rc = check_weights(weights24)) return rc;
  if (!points || !sigma) return fail(NERF_HIP_ERR_ARG, "null argument");
  const QueryLayout L = query_layout(with_rgb);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Weights24 w = as_w24(weights24);
  HIP_TRY(launch_pack_weights(w, at<float>(ws, L.fold), at<float4>(ws, L.packed), NSEG_FWD, st));
  FieldArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.wp = at<float4>(ws, L.packed);
  fa.w = w;
  QuerySrc q;
  memset(&q, 0, sizeof(q));
  if (!with_rgb) {
    fa.sigma = sigma;
    fa.M = M;
    q.points = points;
    HIP_TRY(launch_query_reg(fa, q, false, st));
    return NERF_HIP_OK;
  }
  // colour: chunk by chunk through the workspace's dvec rows (stream order: a chunk's rows are consumed before the next chunk writes them)
  fa.dvec = at<float>(ws, L.dvec);
  for (int off = 0; off < M; off += QUERY_CHUNK) {
    const int n = (M - off < QUERY_CHUNK) ? M - off : QUERY_CHUNK;
    HIP_TRY(launch_dirs_dvec(dirs + (size_t)off * 3, n, w.p[W_DIR], w.p[B_DIR], at<float>(ws, L.fold), at<float>(ws, L.dvec), st));
    fa.rgb = rgb + (size_t)off * 3;
    fa.sigma = sigma + off;
    fa.M = n;
    q.points = points + (size_t)off * 3;
    HIP_TRY(launch_query_reg(fa, q, true, st));
    if (M - off <= QUERY_CHUNK) break;  // (off + QUERY_CHUNK could pass INT_MAX)
  }
  return NERF_HIP_OK;
}

int nerf_hip_density_grid(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, float* sigma,
                          void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_grid(nx, ny, nz)) return rc;
  if (int rc = check_weights(weights24)) return rc;
  if (!lo3 || !step3 || !sigma) return fail(NERF_HIP_ERR_ARG, "null argument");
  const QueryLayout L = query_layout(false);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Weights24 w = as_w24(weights24);
  HIP_TRY(launch_pack_weights(w, at<float>(ws, L.fold), at<float4>(ws, L.packed), NSEG_FWD, st));
  FieldArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.wp = at<float4>(ws, L.packed);
  fa.w = w;
  fa.sigma = sigma;
  fa.M = nx * ny * nz;
  QuerySrc q;
  memset(&q, 0, sizeof(q));
  for (int c = 0; c < 3; ++c) {
    q.lo[c] = lo3[c];
    q.step[c] = step3[c];
  }
  q.ny = ny;
  q.nz = nz;
  HIP_TRY(launch_query_reg(fa, q, false, st));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the gradient queries: the packed weight image WITH the transposed segments (the chain reads them), the fold, and for ONE
// chunk of QGRAD_CHUNK points the compact save (kernels.h QGRAD_*) and, colour queries, the dvec rows.  Independent of M.
struct QGradLayout {
  size_t packed, fold, dvec, save, masks, spre, total;
};
QGradLayout qgrad_layout(bool rgb) {
  QGradLayout L;
  Carve c;
  const size_t rows = (size_t)QGRAD_CHUNK + DUMP_ROWS;
  L.packed = c.take((size_t)PACKED_ALL_F4 * 16);
  L.fold = c.take((size_t)FOLD_FLOATS * 4);
  L.dvec = rgb ? c.take((size_t)QGRAD_CHUNK * HALF * 4) : 0;
  L.save = c.take(rows * (QGRAD_GP + (rgb ? QGRAD_C : 0)) * 4);
  L.masks = c.take((size_t)8 * (QGRAD_CHUNK / 64) * 4 * 256 * 2);
  L.spre = c.take(rows * 4);
  L.total = c.o;
  return L;
}

}  // namespace

extern "C" {

int nerf_hip_query_grad_ws_bytes(int with_rgb, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  *bytes = qgrad_layout(with_rgb != 0).total;
  return NERF_HIP_OK;
}

int nerf_hip_query_grad(const float* const* weights24, const float* points, const float* dirs, int M, const float* dsigma, const float* drgb,
                        float* rgb, float* sigma, float* dpoints, void* ws, size_t ws_bytes, void* stream) {
  if (M < 0) return fail(NERF_HIP_ERR_ARG, "M=%d < 0", M);
  if (drgb && !dirs) return fail(NERF_HIP_ERR_ARG, "drgb needs dirs: without them no colour is computed");
  if ((dirs == nullptr) != (rgb == nullptr)) return fail(NERF_HIP_ERR_ARG, "dirs and rgb must both be null (sigma only) or both be set");
  const bool with_rgb = dirs != nullptr;
  if (M == 0) return NERF_HIP_OK;  // (empty buffers may have null pointers, as for nerf_hip_query)
  if (!points || !sigma || !dpoints) return fail(NERF_HIP_ERR_ARG, "null argument (points, sigma and dpoints are required)");
  if (int rc = check_weights(weights24)) return rc;
  const QGradLayout L = qgrad_layout(with_rgb);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Weights24 w = as_w24(weights24);
  HIP_TRY(launch_pack_weights(w, at<float>(ws, L.fold), at<float4>(ws, L.packed), NSEG, st));
  FieldArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.wp = at<float4>(ws, L.packed);
  fa.w = w;
  fa.dvec = with_rgb ? at<float>(ws, L.dvec) : nullptr;
  fa.save = at<float>(ws, L.save);
  fa.masks = at<uint16_t>(ws, L.masks);
  fa.spre = at<float>(ws, L.spre);
  fa.tiles_tot = QGRAD_CHUNK / 64;
  fa.MSrows = (long long)QGRAD_CHUNK + DUMP_ROWS;
  FieldBwdArgs fb;
  memset(&fb, 0, sizeof(fb));  // G = null: the chain writes no gradient rows
  fb.wp = fa.wp;
  fb.w = w;
  fb.save = fa.save;
  fb.masks = fa.masks;
  fb.spre = fa.spre;
  fb.tiles_tot = fa.tiles_tot;
  fb.MSrows = fa.MSrows;
  QuerySrc q;
  memset(&q, 0, sizeof(q));
  // chunk by chunk through the workspace (stream order: the chain has read a chunk's save before the next forward overwrites it)
  for (int off = 0; off < M; off += QGRAD_CHUNK) {
    const int n = (M - off < QGRAD_CHUNK) ? M - off : QGRAD_CHUNK;
    if (with_rgb) HIP_TRY(launch_dirs_dvec(dirs + (size_t)off * 3, n, w.p[W_DIR], w.p[B_DIR], at<float>(ws, L.fold), at<float>(ws, L.dvec), st));
    fa.rgb = with_rgb ? rgb + (size_t)off * 3 : nullptr;
    fa.sigma = sigma + off;
    fa.M = n;
    fa.Mtot = n;
    q.points = points + (size_t)off * 3;
    HIP_TRY(launch_query_grad_fwd(fa, q, with_rgb, st));
    fb.rgb = fa.rgb;
    fb.drgb = drgb ? drgb + (size_t)off * 3 : nullptr;
    fb.dsig = dsigma ? dsigma + off : nullptr;
    fb.dt = dpoints + (size_t)off * 3;
    fb.M = n;
    fb.Mtot = n;
    HIP_TRY(launch_query_grad_bwd(fb, drgb != nullptr, st));  // no drgb: the colour branch adds nothing, the sigma-only chain runs
    if (M - off <= QGRAD_CHUNK) break;  // (off + QGRAD_CHUNK could pass INT_MAX)
  }
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the mesh calls: per lattice point its in-block vertex offset and owned-edge mask, then per workgroup of MESH_PTS points
// its vertex / face totals and their 64-bit exclusive scans.
struct MeshLayout {
  size_t offs, tv, tf, bv, bf, total;
  int nb;
};
MeshLayout mesh_layout(int nx, int ny, int nz) {
  MeshLayout L;
  const long long n = (long long)nx * ny * nz;
  L.nb = mesh_blocks(n);
  Carve c;
  L.offs = c.take((size_t)n * 4);
  L.tv = c.take((size_t)L.nb * 4);
  L.tf = c.take((size_t)L.nb * 4);
  L.bv = c.take((size_t)(L.nb + 1) * 8);
  L.bf = c.take((size_t)(L.nb + 1) * 8);
  L.total = c.o;
  return L;
}

int check_mesh_call(const float* sigma, int nx, int ny, int nz, float level, const void* ws, size_t ws_bytes, MeshLayout* L) {
  if (int rc = check_grid(nx, ny, nz)) return rc;
  if (!isfinite(level)) return fail(NERF_HIP_ERR_ARG, "level %g is not finite", (double)level);
  if (!sigma) return fail(NERF_HIP_ERR_ARG, "sigma is null");
  *L = mesh_layout(nx, ny, nz);
  return check_ws(ws, ws_bytes, L->total);
}

MeshArgs mesh_args(const float* sigma, int nx, int ny, int nz, float level, const void* ws, const MeshLayout& L) {
  MeshArgs a;
  memset(&a, 0, sizeof(a));
  void* w = const_cast<void*>(ws);
  a.sigma = sigma;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.level = level;
  a.offs = at<unsigned>(w, L.offs);
  a.tv = at<int>(w, L.tv);
  a.tf = at<int>(w, L.tf);
  a.bv = at<long long>(w, L.bv);
  a.bf = at<long long>(w, L.bf);
  return a;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_ws_bytes(int nx, int ny, int nz, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_grid(nx, ny, nz)) return rc;
  *bytes = mesh_layout(nx, ny, nz).total;
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// nerf_hip_mesh_count and its masked form (valid non-null; masked: a null valid is refused)
int mesh_count(const float* sigma, const uint8_t* valid, bool masked, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes,
               int64_t* counts, void* stream) {
  MeshLayout L;
  if (int rc = check_mesh_call(sigma, nx, ny, nz, level, ws, ws_bytes, &L)) return rc;
  if (masked && !valid) return fail(NERF_HIP_ERR_ARG, "valid is null");
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (nx < 2 || ny < 2 || nz < 2) {  // no cells: the empty mesh
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    return NERF_HIP_OK;
  }
  MeshArgs a = mesh_args(sigma, nx, ny, nz, level, ws, L);
  a.valid = valid;
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_mesh_count(a, st));
  return NERF_HIP_OK;
}

// nerf_hip_mesh_emit and its masked form
int mesh_emit(const float* sigma, const uint8_t* valid, bool masked, int nx, int ny, int nz, const float* lo3, const float* step3, float level,
              const void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t max_v, int64_t max_f, void* stream) {
  MeshLayout L;
  if (int rc = check_mesh_call(sigma, nx, ny, nz, level, ws, ws_bytes, &L)) return rc;
  if (masked && !valid) return fail(NERF_HIP_ERR_ARG, "valid is null");
  if (!lo3 || !step3) return fail(NERF_HIP_ERR_ARG, "lo3 / step3 is null");
  const int dims[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) {
    // a step <= 0 would mirror the lattice and silently flip the winding
    if (dims[c] > 1 && !(step3[c] > 0.0f && isfinite(step3[c])))
      return fail(NERF_HIP_ERR_ARG, "step[%d] = %g: must be positive and finite along a dimension of more than one point", c, (double)step3[c]);
  }
  if (int rc = check_caps(max_v, max_f)) return rc;
  if (max_v > 0 && (!verts || !normals)) return fail(NERF_HIP_ERR_ARG, "verts / normals is null");
  if (max_f > 0 && !faces) return fail(NERF_HIP_ERR_ARG, "faces is null");
  if (int rc = check_device()) return rc;
  if (nx < 2 || ny < 2 || nz < 2 || (max_v == 0 && max_f == 0)) return NERF_HIP_OK;  // nothing to write
  MeshArgs a = mesh_args(sigma, nx, ny, nz, level, ws, L);
  a.valid = valid;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.step[c] = step3[c];
  }
  a.verts = verts;
  a.normals = normals;
  a.faces = faces;
  a.max_v = max_v;
  a.max_f = max_f;
  HIP_TRY(launch_mesh_emit(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_count(const float* sigma, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes, int64_t* counts, void* stream) {
  return mesh_count(sigma, nullptr, false, nx, ny, nz, level, ws, ws_bytes, counts, stream);
}

int nerf_hip_mesh_emit(const float* sigma, int nx, int ny, int nz, const float* lo3, const float* step3, float level, const void* ws,
                       size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t max_v, int64_t max_f, void* stream) {
  return mesh_emit(sigma, nullptr, false, nx, ny, nz, lo3, step3, level, ws, ws_bytes, verts, normals, faces, max_v, max_f, stream);
}

int nerf_hip_mesh_count_masked(const float* sigma, const uint8_t* valid, int nx, int ny, int nz, float level, void* ws, size_t ws_bytes,
                               int64_t* counts, void* stream) {
  return mesh_count(sigma, valid, true, nx, ny, nz, level, ws, ws_bytes, counts, stream);
}

int nerf_hip_mesh_emit_masked(const float* sigma, const uint8_t* valid, int nx, int ny, int nz, const float* lo3, const float* step3,
                              float level, const void* ws, size_t ws_bytes, float* verts, float* normals, int32_t* faces, int64_t max_v,
                              int64_t max_f, void* stream) {
  return mesh_emit(sigma, valid, true, nx, ny, nz, lo3, step3, level, ws, ws_bytes, verts, normals, faces, max_v, max_f, stream);
}

}  // extern "C"

namespace {

// Workspace of the narrow-band grid: the point queries' packed weight image and fold, then per block of r^3 lattice points 10 bytes
// (the sets A and S, the new-block offsets, the list) and per BAND_WG blocks 16 more.  Nothing per lattice point.
struct BandLayout {
  size_t packed, fold, active, seed, offs, list, tn, tp, bn, total;
  int r, nb[3], nblk, nwg;
};
constexpr int BAND_MAX_BLOCKS = 1 << 25;  // (one wave per block in k_band_reseed: the launch stays below 2^32 threads)

int band_layout(int nx, int ny, int nz, int block, BandLayout* L) {
  if (int rc = check_grid(nx, ny, nz)) return rc;
  if (block < 2) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least 2 points along every axis", block);
  const int nmax = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  L->r = block < nmax ? block : (nmax > 2 ? nmax : 2);  // (any block >= the grid is one block per axis)
  const int n[3] = {nx, ny, nz};
  long long nblk = 1;
  for (int c = 0; c < 3; ++c) {
    L->nb[c] = (n[c] + L->r - 1) / L->r;
    nblk *= L->nb[c];
  }
  if (nblk > BAND_MAX_BLOCKS)
    return fail(NERF_HIP_ERR_ARG, "grid %d x %d x %d in blocks of %d: %lld blocks, at most %d (raise block)", nx, ny, nz, block, nblk, BAND_MAX_BLOCKS);
  L->nblk = (int)nblk;
  L->nwg = (L->nblk + BAND_WG - 1) / BAND_WG;
  const QueryLayout Q = query_layout(false);
  Carve c{Q.total};
  L->packed = Q.packed;
  L->fold = Q.fold;
  L->active = c.take((size_t)L->nblk);
  L->seed = c.take((size_t)L->nblk);
  L->offs = c.take((size_t)L->nblk * 4);
  L->list = c.take((size_t)L->nblk * 4);
  L->tn = c.take((size_t)L->nwg * 4);
  L->tp = c.take((size_t)L->nwg * 8);
  L->bn = c.take((size_t)L->nwg * 4);
  L->total = c.o;
  return NERF_HIP_OK;
}

// the checks of both band calls, in the mesh calls' order: grid, block, level, pointers, workspace, counts
int check_band_call(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, int block, float level,
                    const float* sigma, const void* ws, size_t ws_bytes, const int64_t* counts, BandLayout* L) {
  if (int rc = band_layout(nx, ny, nz, block, L)) return rc;
  if (!isfinite(level)) return fail(NERF_HIP_ERR_ARG, "level %g is not finite", (double)level);
  if (!sigma) return fail(NERF_HIP_ERR_ARG, "sigma is null");
  if (!lo3 || !step3) return fail(NERF_HIP_ERR_ARG, "lo3 / step3 is null");
  if (int rc = check_ws(ws, ws_bytes, L->total)) return rc;
  if (int rc = check_out(counts, "counts", 8)) return rc;
  return check_weights(weights24);
}

BandArgs band_args(float* sigma, int nx, int ny, int nz, float level, void* ws, const BandLayout& L, int64_t* counts) {
  BandArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.r = L.r;
  a.nbx = L.nb[0];
  a.nby = L.nb[1];
  a.nbz = L.nb[2];
  a.nblk = L.nblk;
  a.nwg = L.nwg;
  a.level = level;
  a.active = at<unsigned char>(ws, L.active);
  a.seed = at<unsigned char>(ws, L.seed);
  a.offs = at<unsigned>(ws, L.offs);
  a.list = at<int>(ws, L.list);
  a.tn = at<int>(ws, L.tn);
  a.tp = at<long long>(ws, L.tp);
  a.bn = at<int>(ws, L.bn);
  a.counts = reinterpret_cast<long long*>(counts);
  return a;
}

void band_field_args(const Weights24& w, const float* lo3, const float* step3, int nx, int ny, int nz, float* sigma, void* ws,
                     const BandLayout& L, FieldArgs* fa, QuerySrc* q) {
  memset(fa, 0, sizeof(*fa));
  fa->wp = at<float4>(ws, L.packed);
  fa->w = w;
  fa->sigma = sigma;
  memset(q, 0, sizeof(*q));
  for (int c = 0; c < 3; ++c) {
    q->lo[c] = lo3[c];
    q->step[c] = step3[c];
  }
  q->nx = nx;
  q->ny = ny;
  q->nz = nz;
  q->r = L.r;
  q->nby = L.nb[1];
  q->nbz = L.nb[2];
}

}  // namespace

extern "C" {

int nerf_hip_band_ws_bytes(int nx, int ny, int nz, int block, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  BandLayout L;
  if (int rc = band_layout(nx, ny, nz, block, &L)) return rc;
  *bytes = L.total;
  return NERF_HIP_OK;
}

int nerf_hip_band_begin(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, int block, float level,
                        float* sigma, void* ws, size_t ws_bytes, int64_t* counts, void* stream) {
  BandLayout L;
  if (int rc = check_band_call(weights24, lo3, step3, nx, ny, nz, block, level, sigma, ws, ws_bytes, counts, &L)) return rc;
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Weights24 w = as_w24(weights24);
  HIP_TRY(launch_pack_weights(w, at<float>(ws, L.fold), at<float4>(ws, L.packed), NSEG_FWD, st));
  FieldArgs fa;
  QuerySrc q;
  band_field_args(w, lo3, step3, nx, ny, nz, sigma, ws, L, &fa, &q);
  const int n[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c) q.ext[c] = (n[c] - 1 + L.r - 1) / L.r + 1;  // the unique planes min(u r, n - 1)
  fa.M = q.ext[0] * q.ext[1] * q.ext[2];  // (<= nx ny nz)
  HIP_TRY(launch_band_corners(fa, q, st));
  const BandArgs a = band_args(sigma, nx, ny, nz, level, ws, L, counts);
  HIP_TRY(launch_band_begin(a, st));
  HIP_TRY(launch_band_next(a, st));
  return NERF_HIP_OK;
}

int nerf_hip_band_grow(const float* const* weights24, const float* lo3, const float* step3, int nx, int ny, int nz, int block, float level,
                       int64_t n_blocks, float* sigma, void* ws, size_t ws_bytes, int64_t* counts, void* stream) {
  BandLayout L;
  if (int rc = check_band_call(weights24, lo3, step3, nx, ny, nz, block, level, sigma, ws, ws_bytes, counts, &L)) return rc;
  if (n_blocks < 0 || n_blocks > L.nblk) return fail(NERF_HIP_ERR_ARG, "n_blocks=%lld: the grid has %d blocks", (long long)n_blocks, L.nblk);
  if (int rc = check_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BandArgs a = band_args(sigma, nx, ny, nz, level, ws, L, counts);
  FieldArgs fa;
  QuerySrc q;
  band_field_args(as_w24(weights24), lo3, step3, nx, ny, nz, sigma, ws, L, &fa, &q);
  const int n[3] = {nx, ny, nz};
  long long vol = 1;
  for (int c = 0; c < 3; ++c) {
    q.ext[c] = n[c] < L.r ? n[c] : L.r;
    vol *= q.ext[c];  // (<= nx ny nz)
  }
  q.list = a.list;
  q.nlist = a.counts;
  // the listed blocks, in launches of fewer than 2^31 samples (the counts are read by these launches and rewritten only after them)
  const long long per = ((1ll << 31) - 64) / vol;
  for (long long e0 = 0; e0 < n_blocks; e0 += per) {
    const long long ne = n_blocks - e0 < per ? n_blocks - e0 : per;
    q.e0 = (int)e0;
    fa.M = (int)(ne * vol);
    HIP_TRY(launch_band_blocks(fa, q, st));
  }
  HIP_TRY(launch_band_reseed(a, st));
  HIP_TRY(launch_band_next(a, st));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the component calls: 4 bytes per vertex (the labels L; the compaction keeps its new vertex indices there) and 8 bytes
// per CC_PTS vertices or faces, whichever are more (a workgroup's total and its exclusive scan).
struct CcLayout {
  size_t L, tot, base, total;
};
CcLayout cc_layout(long long V, long long F) {
  CcLayout L;
  const int nb = cc_blocks(V > F ? V : F);
  Carve c;
  L.L = c.take((size_t)V * 4);
  L.tot = c.take((size_t)nb * 4);
  L.base = c.take((size_t)nb * 4);
  L.total = c.o;
  return L;
}

int check_cc_ws(int64_t V, int64_t F, const void* ws, size_t ws_bytes, CcLayout* L) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  *L = cc_layout(V, F);
  return check_ws(ws, ws_bytes, L->total);
}

}  // namespace

extern "C" {

int nerf_hip_mesh_cc_ws_bytes(int64_t V, int64_t F, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(V, F)) return rc;
  *bytes = cc_layout(V, F).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_cc_round(const int32_t* faces, int64_t V, int64_t F, int round, void* ws, size_t ws_bytes, int32_t* changed, void* stream) {
  CcLayout L;
  if (int rc = check_cc_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (F > 0 && !faces) return fail(NERF_HIP_ERR_ARG, "faces is null");
  if (int rc = check_out(changed, "changed", 4)) return rc;
  if (round < 0) return fail(NERF_HIP_ERR_ARG, "round=%d < 0", round);
  if (round >= CC_MAX_ROUNDS)
    return fail(NERF_HIP_ERR_CONVERGE, "the component labelling did not converge in %d rounds (V=%lld F=%lld); no result", CC_MAX_ROUNDS,
                (long long)V, (long long)F);
  if (int rc = check_device()) return rc;
  CcArgs a;
  memset(&a, 0, sizeof(a));
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  a.L = at<int>(ws, L.L);
  a.changed = changed;
  HIP_TRY(launch_cc_round(a, round == 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_cc_ids(const int32_t* faces, int64_t V, int64_t F, void* ws, size_t ws_bytes, int32_t* vert_comp, int32_t* face_comp,
                         int64_t* count, void* stream) {
  CcLayout L;
  if (int rc = check_cc_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (F > 0 && (!faces || !face_comp)) return fail(NERF_HIP_ERR_ARG, "faces / face_comp is null");
  if (V > 0 && !vert_comp) return fail(NERF_HIP_ERR_ARG, "vert_comp is null");
  if (int rc = check_out(count, "count", 8)) return rc;
  if (int rc = check_device()) return rc;
  CcArgs a;
  memset(&a, 0, sizeof(a));
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  a.L = at<int>(ws, L.L);
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  a.vert_comp = vert_comp;
  a.face_comp = face_comp;
  a.count = reinterpret_cast<long long*>(count);
  HIP_TRY(launch_cc_ids(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_cc_stats(const float* verts, const int32_t* vert_comp, const int32_t* face_comp, int64_t V, int64_t F, int32_t* n_verts,
                           int32_t* n_faces, float* bbox_lo, float* bbox_hi, int64_t max_c, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (max_c < 0 || max_c >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "max_c=%lld: a capacity in [0, 2^31)", (long long)max_c);
  if (V > 0 && !vert_comp) return fail(NERF_HIP_ERR_ARG, "vert_comp is null");
  if (F > 0 && !face_comp) return fail(NERF_HIP_ERR_ARG, "face_comp is null");
  if (max_c > 0 && (!n_verts || !n_faces)) return fail(NERF_HIP_ERR_ARG, "n_verts / n_faces is null");
  if ((bbox_lo == nullptr) != (bbox_hi == nullptr)) return fail(NERF_HIP_ERR_ARG, "bbox_lo and bbox_hi come together");
  if (bbox_lo && V > 0 && !verts) return fail(NERF_HIP_ERR_ARG, "boxes need verts");
  if (int rc = check_device()) return rc;
  CcStatsArgs a;
  memset(&a, 0, sizeof(a));
  a.vert_comp = vert_comp;
  a.face_comp = face_comp;
  a.verts = verts;
  a.V = V;
  a.F = F;
  a.max_c = max_c;
  a.n_verts = n_verts;
  a.n_faces = n_faces;
  a.lo = reinterpret_cast<unsigned*>(bbox_lo);
  a.hi = reinterpret_cast<unsigned*>(bbox_hi);
  HIP_TRY(launch_cc_stats(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_cc_compact(const float* verts, const float* normals, const float* rgb, const int32_t* faces, int64_t V, int64_t F,
                             const int32_t* vert_comp, const int32_t* face_comp, const uint8_t* keep, int64_t C, void* ws, size_t ws_bytes,
                             float* out_verts, float* out_normals, float* out_rgb, int32_t* out_faces, int64_t max_v, int64_t max_f,
                             int64_t* counts, void* stream) {
  CcLayout L;
  if (int rc = check_cc_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (C < 0 || C > V) return fail(NERF_HIP_ERR_ARG, "C=%lld: a mesh of %lld vertices has at most as many components", (long long)C, (long long)V);
  if (int rc = check_caps(max_v, max_f)) return rc;
  if (V > 0 && (!verts || !vert_comp)) return fail(NERF_HIP_ERR_ARG, "verts / vert_comp is null");
  if (F > 0 && (!faces || !face_comp)) return fail(NERF_HIP_ERR_ARG, "faces / face_comp is null");
  if (C > 0 && !keep) return fail(NERF_HIP_ERR_ARG, "keep is null");
  if (max_v > 0 && (!out_verts || (normals && !out_normals) || (rgb && !out_rgb))) return fail(NERF_HIP_ERR_ARG, "an output of max_v rows is null");
  if (max_f > 0 && !out_faces) return fail(NERF_HIP_ERR_ARG, "out_faces is null");
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  CcCompactArgs a;
  memset(&a, 0, sizeof(a));
  a.verts = verts;
  a.normals = normals;
  a.rgb = rgb;
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  a.C = (int)C;
  a.vert_comp = vert_comp;
  a.face_comp = face_comp;
  a.keep = keep;
  a.newidx = at<int>(ws, L.L);
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  a.out_verts = out_verts;
  a.out_normals = out_normals;
  a.out_rgb = out_rgb;
  a.out_faces = out_faces;
  a.max_v = max_v;
  a.max_f = max_f;
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_cc_compact(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the simplification calls.  Per cell of the cluster lattice 4 bytes (occupancy, then cluster ids); per vertex 60: its
// cell / cluster (4), and per possible cluster -- there are at most V -- the member count (4), the coordinate and normal sums (24
// each) and the referenced mark / output id (4); per face 4 (state) and the face table's 4 bytes per slot (the power of two >= 2 F:
// 8 to 16 bytes per face); and 8 bytes per CC_PTS cells, vertices or faces, whichever are most (the scans).
struct MsLayout {
  size_t occ, vcl, cnt, S, T, ref, fstate, table, tot, base, scratch, total;
  long long ncell, slots;
};
MsLayout ms_layout(long long V, long long F, const int* dims3) {
  MsLayout L;
  L.ncell = (long long)dims3[0] * dims3[1] * dims3[2];
  L.slots = ms_table_slots(F);
  long long most = L.ncell > V ? L.ncell : V;
  most = most > F ? most : F;
  const int nb = cc_blocks(most);
  Carve c;
  L.occ = c.take((size_t)L.ncell * 4);
  L.vcl = c.take((size_t)V * 4);
  L.cnt = c.take((size_t)V * 4);
  L.S = c.take((size_t)V * 24);
  L.T = c.take((size_t)V * 24);
  L.ref = c.take((size_t)V * 4);
  L.fstate = c.take((size_t)F * 4);
  L.table = c.take((size_t)L.slots * 4);
  L.tot = c.take((size_t)nb * 4);
  L.base = c.take((size_t)nb * 4);
  L.scratch = c.take(8);
  L.total = c.o;
  return L;
}

int check_ms_dims(const int* dims3) {
  if (!dims3) return fail(NERF_HIP_ERR_ARG, "dims3 is null");
  long long n = 1;
  for (int c = 0; c < 3; ++c) {
    if (dims3[c] < 1 || dims3[c] > 2048) return fail(NERF_HIP_ERR_ARG, "dims[%d]=%d: the cluster lattice has 1 .. 2048 cells per axis", c, dims3[c]);
    n *= dims3[c];
  }
  if (n >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "dims=(%d, %d, %d): the cluster lattice must stay below 2^31 cells", dims3[0], dims3[1], dims3[2]);
  return NERF_HIP_OK;
}

int check_ms(int64_t V, int64_t F, const float* lo3, const float* cell3, const int* dims3, const void* ws, size_t ws_bytes, MsLayout* L) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_ms_dims(dims3)) return rc;
  if (!lo3 || !cell3) return fail(NERF_HIP_ERR_ARG, "lo3 / cell3 is null");
  if (int rc = check_finite3(lo3, "lo", "the cluster lattice's corner")) return rc;
  for (int c = 0; c < 3; ++c)
    if (!(cell3[c] > 0.0f) || !isfinite(cell3[c]))
      return fail(NERF_HIP_ERR_ARG, "cell[%d]=%g: the cluster lattice's cells must be > 0 and finite", c, (double)cell3[c]);
  *L = ms_layout(V, F, dims3);
  return check_ws(ws, ws_bytes, L->total);
}

MsArgs ms_args(const int32_t* faces, int64_t V, int64_t F, const float* lo3, const float* cell3, const int* dims3, void* ws, const MsLayout& L) {
  MsArgs a;
  memset(&a, 0, sizeof(a));
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.cell[c] = cell3[c];
    a.dims[c] = dims3[c];
  }
  a.ncell = L.ncell;
  a.slots = L.slots;
  a.occ = at<int>(ws, L.occ);
  a.vcl = at<int>(ws, L.vcl);
  a.cnt = at<int>(ws, L.cnt);
  a.S = at<long long>(ws, L.S);
  a.T = at<long long>(ws, L.T);
  a.ref = at<int>(ws, L.ref);
  a.fstate = at<int>(ws, L.fstate);
  a.table = at<int>(ws, L.table);
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  a.scratch = at<long long>(ws, L.scratch);
  return a;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_simplify_ws_bytes(int64_t V, int64_t F, const int* dims3, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_ms_dims(dims3)) return rc;
  *bytes = ms_layout(V, F, dims3).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_simplify_count(const float* verts, const float* normals, const int32_t* faces, int64_t V, int64_t F, const float* lo3,
                                 const float* cell3, const int* dims3, void* ws, size_t ws_bytes, int64_t* counts, void* stream) {
  MsLayout L;
  if (int rc = check_ms(V, F, lo3, cell3, dims3, ws, ws_bytes, &L)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  MsArgs a = ms_args(faces, V, F, lo3, cell3, dims3, ws, L);
  a.verts = verts;
  a.normals = normals;
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_ms_count(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_simplify_emit(const int32_t* faces, int64_t V, int64_t F, const float* lo3, const float* cell3, const int* dims3, void* ws,
                                size_t ws_bytes, float* out_verts, float* out_normals, int32_t* out_faces, int64_t max_v, int64_t max_f,
                                void* stream) {
  MsLayout L;
  if (int rc = check_ms(V, F, lo3, cell3, dims3, ws, ws_bytes, &L)) return rc;
  if (F > 0 && !faces) return fail(NERF_HIP_ERR_ARG, "faces is null");
  if (int rc = check_caps(max_v, max_f)) return rc;
  if (max_v > 0 && !out_verts) return fail(NERF_HIP_ERR_ARG, "out_verts is null");
  if (max_f > 0 && !out_faces) return fail(NERF_HIP_ERR_ARG, "out_faces is null");
  if (int rc = check_device()) return rc;
  MsArgs a = ms_args(faces, V, F, lo3, cell3, dims3, ws, L);
  a.out_verts = out_verts;
  a.out_normals = out_normals;
  a.out_faces = out_faces;
  a.max_v = max_v;
  a.max_f = max_f;
  HIP_TRY(launch_ms_emit(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the edge calls.  Per slot of the edge table 16 bytes (the key 8, count 4, tally 4; the power of two >= 4 F slots: 64 to
// 128 bytes per face); per face 24 more (the adjacency's 6 F entries); per vertex 36 (row offset 8, cursor 4, the normals' sums 24);
// and 16 bytes per CC_PTS vertices (the scan).
struct MeLayout {
  size_t keys, cnt, tally, off, cursor, adj, tot, base, T, total;
  long long slots;
};
MeLayout me_layout(long long V, long long F) {
  MeLayout L;
  L.slots = me_table_slots(F);
  const int nb = cc_blocks(V);
  Carve c;
  L.keys = c.take((size_t)L.slots * 8);
  L.cnt = c.take((size_t)L.slots * 4);
  L.tally = c.take((size_t)L.slots * 4);
  L.off = c.take(((size_t)V + 1) * 8);
  L.cursor = c.take((size_t)V * 4);
  L.adj = c.take((size_t)F * 6 * 4);
  L.tot = c.take((size_t)nb * 8);
  L.base = c.take((size_t)nb * 8);
  L.T = c.take((size_t)V * 24);
  L.total = c.o;
  return L;
}

int check_me_ws(int64_t V, int64_t F, const void* ws, size_t ws_bytes, MeLayout* L) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  *L = me_layout(V, F);
  return check_ws(ws, ws_bytes, L->total);
}

int check_me_box(const float* lo3, float scale) {
  if (!lo3) return fail(NERF_HIP_ERR_ARG, "lo3 is null");
  if (int rc = check_finite3(lo3, "lo", "the box's corner")) return rc;
  if (!(scale > 0.0f) || !isfinite(scale)) return fail(NERF_HIP_ERR_ARG, "scale=%g: the box's scale must be > 0 and finite", (double)scale);
  return NERF_HIP_OK;
}

MeArgs me_args(int64_t V, int64_t F, const void* ws, const MeLayout& L) {
  MeArgs a;
  memset(&a, 0, sizeof(a));
  void* w = const_cast<void*>(ws);
  a.V = (int)V;
  a.F = (int)F;
  a.slots = L.slots;
  a.cap = (long long)F * 6;
  a.keys = at<long long>(w, L.keys);
  a.cnt = at<int>(w, L.cnt);
  a.tally = at<int>(w, L.tally);
  a.off = at<long long>(w, L.off);
  a.cursor = at<int>(w, L.cursor);
  a.adj = at<int>(w, L.adj);
  a.tot = at<long long>(w, L.tot);
  a.base = at<long long>(w, L.base);
  a.T = at<long long>(w, L.T);
  return a;
}

void me_box(MeArgs* a, const float* lo3, float scale) {
  for (int c = 0; c < 3; ++c) a->lo[c] = lo3[c];
  a->scale = scale;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_edges_ws_bytes(int64_t V, int64_t F, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(V, F)) return rc;
  *bytes = me_layout(V, F).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_edges_build(const int32_t* faces, int64_t V, int64_t F, void* ws, size_t ws_bytes, int32_t* degree, int32_t* vert_flags,
                              int64_t* counts, void* stream) {
  MeLayout L;
  if (int rc = check_me_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (F > 0 && !faces) return fail(NERF_HIP_ERR_ARG, "faces is null");
  if (V > 0 && (!degree || !vert_flags)) return fail(NERF_HIP_ERR_ARG, "degree / vert_flags is null");
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  MeArgs a = me_args(V, F, ws, L);
  a.faces = faces;
  a.degree = degree;
  a.vflags = vert_flags;
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_me_build(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_smooth_step(const float* verts_in, float* verts_out, int64_t V, int64_t F, const float* lo3, float scale, double w,
                              const int32_t* vert_flags, const void* ws, size_t ws_bytes, int64_t max_v, void* stream) {
  MeLayout L;
  if (int rc = check_me_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (int rc = check_me_box(lo3, scale)) return rc;
  if (!isfinite(w)) return fail(NERF_HIP_ERR_ARG, "w=%g: a step's weight must be finite", w);
  if (int rc = check_cap("max_v", max_v)) return rc;
  const int64_t n = V < max_v ? V : max_v;
  if (V > 0 && !verts_in) return fail(NERF_HIP_ERR_ARG, "verts_in is null");
  if (n > 0 && !verts_out) return fail(NERF_HIP_ERR_ARG, "verts_out is null");
  if (n > 0) {  // a Jacobi step: the output may not alias the input
    const uintptr_t i0 = (uintptr_t)verts_in, i1 = i0 + (size_t)V * 12, o0 = (uintptr_t)verts_out, o1 = o0 + (size_t)n * 12;
    if (i0 < o1 && o0 < i1) return fail(NERF_HIP_ERR_ARG, "verts_in and verts_out overlap: a step reads only its input");
  }
  if (int rc = check_device()) return rc;
  MeArgs a = me_args(V, F, ws, L);
  me_box(&a, lo3, scale);
  a.verts = verts_in;
  a.out = verts_out;
  a.max_v = max_v;
  a.w = w;
  a.pin = vert_flags;
  HIP_TRY(launch_me_step(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, void* ws,
                                 size_t ws_bytes, float* normals, int64_t max_v, void* stream) {
  MeLayout L;
  if (int rc = check_me_ws(V, F, ws, ws_bytes, &L)) return rc;
  if (int rc = check_me_box(lo3, scale)) return rc;
  if (int rc = check_cap("max_v", max_v)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (V > 0 && max_v > 0 && !normals) return fail(NERF_HIP_ERR_ARG, "normals is null");
  if (int rc = check_device()) return rc;
  MeArgs a = me_args(V, F, ws, L);
  me_box(&a, lo3, scale);
  a.faces = faces;
  a.verts = verts;
  a.out = normals;
  a.max_v = max_v;
  HIP_TRY(launch_me_normals(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the sampling call: per face 8 bytes (the inclusive prefix of the weights) and 16 per CC_PTS faces (the scan).
struct MdSampleLayout {
  size_t cum, tot, base, total;
};
MdSampleLayout md_sample_layout(long long F) {
  MdSampleLayout L;
  const int nb = cc_blocks(F);
  Carve c;
  L.cum = c.take((size_t)F * 8);
  L.tot = c.take((size_t)nb * 8);
  L.base = c.take((size_t)nb * 8);
  L.total = c.o;
  return L;
}

int check_md_mesh(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_me_box(lo3, scale)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  return NERF_HIP_OK;
}

MdMeshArgs md_mesh_args(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale) {
  MdMeshArgs a;
  memset(&a, 0, sizeof(a));
  a.verts = verts;
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  for (int c = 0; c < 3; ++c) a.lo[c] = lo3[c];
  a.scale = scale;
  return a;
}

// Workspace of the nearest-point calls.  The reference points' grid: per cell 8 bytes (count / cursor 4, start 4), per reference point
// 16 (its record), and 8 per CC_PTS cells (the scan); then the queries' order: per cell 8 more, per query 16, and 8 for their total.
struct MdGridLayout {
  size_t cnt, start, rec, tot, base, qcnt, qstart, qrec, scratch, ref_total, total;
  long long ncell;
};
MdGridLayout md_grid_layout(long long M, long long N, const int* dims3) {
  MdGridLayout L;
  L.ncell = (long long)dims3[0] * dims3[1] * dims3[2];
  const int nb = cc_blocks(L.ncell);
  Carve c;
  L.cnt = c.take((size_t)L.ncell * 4);
  L.start = c.take(((size_t)L.ncell + 1) * 4);
  L.rec = c.take((size_t)M * 16);
  L.tot = c.take((size_t)nb * 4);
  L.base = c.take((size_t)nb * 4);
  L.ref_total = c.o;
  L.qcnt = c.take((size_t)L.ncell * 4);
  L.qstart = c.take(((size_t)L.ncell + 1) * 4);
  L.qrec = c.take((size_t)N * 16);
  L.scratch = c.take(8);
  L.total = c.o;
  return L;
}

int check_md_dims(const int* dims3) {
  if (!dims3) return fail(NERF_HIP_ERR_ARG, "dims3 is null");
  long long n = 1;
  for (int c = 0; c < 3; ++c) {
    if (dims3[c] < 1) return fail(NERF_HIP_ERR_ARG, "dims[%d]=%d: the grid has at least one cell per axis", c, dims3[c]);
    n *= dims3[c];
    if (n >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "dims=(%d, %d, %d): the grid must stay below 2^31 cells", dims3[0], dims3[1], dims3[2]);
  }
  return NERF_HIP_OK;
}

int check_md_grid(int64_t M, int64_t N, const float* lo3, float cell, const int* dims3) {
  if (int rc = check_mesh_sizes(M, N)) return rc;  // (point counts below 2^31, as vertices)
  if (int rc = check_md_dims(dims3)) return rc;
  if (!lo3) return fail(NERF_HIP_ERR_ARG, "lo3 is null");
  if (int rc = check_finite3(lo3, "lo", "the grid's corner")) return rc;
  if (!(cell > 0.0f) || !isfinite(cell)) return fail(NERF_HIP_ERR_ARG, "cell=%g: the grid's cell must be > 0 and finite", (double)cell);
  return NERF_HIP_OK;
}

MdGridArgs md_grid_args(int64_t M, int64_t N, const float* lo3, float cell, const int* dims3, void* ws, const MdGridLayout& L) {
  MdGridArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.dims[c] = dims3[c];
  }
  a.cell = cell;
  a.ncell = (int)L.ncell;
  a.M = (int)M;
  a.N = (int)N;
  a.cnt = at<int>(ws, L.cnt);
  a.start = at<int>(ws, L.start);
  a.rec = at<float4>(ws, L.rec);
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  a.qcnt = at<int>(ws, L.qcnt);
  a.qstart = at<int>(ws, L.qstart);
  a.qrec = at<float4>(ws, L.qrec);
  a.scratch = at<long long>(ws, L.scratch);
  return a;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_measure(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, int64_t* out,
                          void* stream) {
  if (int rc = check_md_mesh(verts, faces, V, F, lo3, scale)) return rc;
  if (int rc = check_out(out, "out", 8)) return rc;
  if (int rc = check_device()) return rc;
  MdMeshArgs a = md_mesh_args(verts, faces, V, F, lo3, scale);
  a.out = reinterpret_cast<long long*>(out);
  HIP_TRY(launch_md_measure(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_sample_ws_bytes(int64_t F, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(0, F)) return rc;
  *bytes = md_sample_layout(F).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_sample(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float scale, int64_t n,
                         uint32_t seed, void* ws, size_t ws_bytes, float* points, int32_t* face, int64_t cap_n, int64_t* info,
                         void* stream) {
  if (int rc = check_md_mesh(verts, faces, V, F, lo3, scale)) return rc;
  if (n < 0 || n >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "n=%lld: a sample count in [0, 2^31)", (long long)n);
  if (int rc = check_cap("cap_n", cap_n)) return rc;
  if (n > 0 && cap_n > 0 && (!points || !face)) return fail(NERF_HIP_ERR_ARG, "points / face is null");
  const MdSampleLayout L = md_sample_layout(F);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_out(info, "info", 8)) return rc;
  if (int rc = check_device()) return rc;
  MdMeshArgs a = md_mesh_args(verts, faces, V, F, lo3, scale);
  a.n = n;
  a.cap_n = cap_n;
  a.seed = seed;
  a.cum = at<long long>(ws, L.cum);
  a.tot = at<long long>(ws, L.tot);
  a.base = at<long long>(ws, L.base);
  a.info = reinterpret_cast<long long*>(info);
  a.points = points;
  a.face = face;
  HIP_TRY(launch_md_sample(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_points_nearest_ws_bytes(int64_t M, int64_t N, const int* dims3, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(M, N)) return rc;
  if (int rc = check_md_dims(dims3)) return rc;
  *bytes = md_grid_layout(M, N, dims3).total;
  return NERF_HIP_OK;
}

int nerf_hip_points_grid_build(const float* ref, int64_t M, const float* lo3, float cell, const int* dims3, void* ws, size_t ws_bytes,
                               int64_t* counts, void* stream) {
  if (int rc = check_md_grid(M, 0, lo3, cell, dims3)) return rc;
  if (M > 0 && !ref) return fail(NERF_HIP_ERR_ARG, "ref is null");
  const MdGridLayout L = md_grid_layout(M, 0, dims3);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  MdGridArgs a = md_grid_args(M, 0, lo3, cell, dims3, ws, L);
  a.ref = ref;
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_md_grid_build(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_points_nearest(const float* query, int64_t M, int64_t N, const float* lo3, float cell, const int* dims3, void* ws,
                            size_t ws_bytes, int sort_queries, int32_t* idx, double* dist2, int64_t cap_n, void* stream) {
  if (int rc = check_md_grid(M, N, lo3, cell, dims3)) return rc;
  if (int rc = check_cap("cap_n", cap_n)) return rc;
  if (N > 0 && !query) return fail(NERF_HIP_ERR_ARG, "query is null");
  if (N > 0 && cap_n > 0 && (!idx || !dist2)) return fail(NERF_HIP_ERR_ARG, "idx / dist2 is null");
  if (dist2 && ((uintptr_t)dist2 & 7) != 0) return fail(NERF_HIP_ERR_ARG, "dist2 must be 8-byte aligned");
  const MdGridLayout L = md_grid_layout(M, N, dims3);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  MdGridArgs a = md_grid_args(M, N, lo3, cell, dims3, ws, L);
  a.query = query;
  a.idx = idx;
  a.dist2 = dist2;
  a.cap_n = cap_n;
  HIP_TRY(launch_md_nearest(a, sort_queries != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_distance_stats(const double* dist2, int64_t N, double unit, const double* tau, int K, int64_t* out, void* stream) {
  if (N < 0 || N >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "N=%lld: a count in [0, 2^31)", (long long)N);
  if (K < 0 || K > MD_MAX_TAU) return fail(NERF_HIP_ERR_ARG, "K=%d: at most %d thresholds", K, MD_MAX_TAU);
  if (!(unit > 0.0) || !isfinite(unit) || !isfinite(unit * unit) || !(unit * unit > 0.0))
    return fail(NERF_HIP_ERR_ARG, "unit=%g: must be > 0 and finite, its square as well", unit);
  if (K > 0 && !tau) return fail(NERF_HIP_ERR_ARG, "tau is null");
  if (N > 0 && (!dist2 || ((uintptr_t)dist2 & 7) != 0)) return fail(NERF_HIP_ERR_ARG, "dist2 is null or not 8-byte aligned");
  if (int rc = check_out(out, "out", 8)) return rc;
  MdStatsArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < K; ++k) {
    if (!isfinite(tau[k]) || tau[k] < 0.0) return fail(NERF_HIP_ERR_ARG, "tau[%d]=%g: a threshold must be finite and >= 0", k, tau[k]);
    a.tau2[k] = tau[k] * tau[k];
  }
  if (int rc = check_device()) return rc;
  a.dist2 = dist2;
  a.N = N;
  a.unit = unit;
  a.K = K;
  a.out = reinterpret_cast<long long*>(out);
  HIP_TRY(launch_md_stats(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Workspace of the ray-casting calls: per cell 8 bytes (count / cursor 4, start 4), per entry 4 (a face index), per face 4 (the OUTSIDE
// list), 8 per CC_PTS cells or faces, whichever are more (the scans), and 16 for the two totals.
struct RcLayout {
  size_t cnt, start, entries, outside, tot, base, info, total;
  long long ncell;
};
RcLayout rc_layout(long long F, long long E, const int* dims3) {
  RcLayout L;
  L.ncell = (long long)dims3[0] * dims3[1] * dims3[2];
  const int nb = cc_blocks(L.ncell > F ? L.ncell : F);
  Carve c;
  L.cnt = c.take((size_t)L.ncell * 4);
  L.start = c.take(((size_t)L.ncell + 1) * 4);
  L.entries = c.take((size_t)E * 4);
  L.outside = c.take((size_t)F * 4);
  L.tot = c.take((size_t)nb * 4);
  L.base = c.take((size_t)nb * 4);
  L.info = c.take(16);
  L.total = c.o;
  return L;
}

int check_rc_entries(int64_t cap_entries) {
  if (cap_entries < 0 || cap_entries >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "cap_entries=%lld: the grid's entries in [0, 2^31)", (long long)cap_entries);
  return NERF_HIP_OK;
}

RcGridArgs rc_grid_args(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell, const int* dims3) {
  RcGridArgs a;
  memset(&a, 0, sizeof(a));
  a.verts = verts;
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.dims[c] = dims3[c];
  }
  a.cell = cell;
  a.ncell = dims3[0] * dims3[1] * dims3[2];
  return a;
}

void rc_grid_ws(RcGridArgs* a, int64_t cap_entries, void* ws, const RcLayout& L) {
  a->cap_entries = cap_entries;
  a->cnt = at<int>(ws, L.cnt);
  a->start = at<int>(ws, L.start);
  a->entries = at<int>(ws, L.entries);
  a->outside = at<int>(ws, L.outside);
  a->tot = at<int>(ws, L.tot);
  a->base = at<int>(ws, L.base);
  a->info = at<long long>(ws, L.info);
}

// Workspace of the face selection: per vertex 8 bytes (the used mark, the new index), 8 per CC_PTS vertices or faces, whichever are
// more (the scans), and 16 for emit's throw-away totals.
struct SelLayout {
  size_t used, newidx, tot, base, scratch, total;
};
SelLayout sel_layout(long long V, long long F) {
  SelLayout L;
  const int nb = cc_blocks(V > F ? V : F);
  Carve c;
  L.used = c.take((size_t)V * 4);
  L.newidx = c.take((size_t)V * 4);
  L.tot = c.take((size_t)nb * 4);
  L.base = c.take((size_t)nb * 4);
  L.scratch = c.take(16);
  L.total = c.o;
  return L;
}

int check_sel(const int32_t* faces, int64_t V, int64_t F, const uint8_t* keep, const void* ws, size_t ws_bytes, SelLayout* L) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (F > 0 && (!faces || !keep)) return fail(NERF_HIP_ERR_ARG, "faces / keep is null");
  *L = sel_layout(V, F);
  return check_ws(ws, ws_bytes, L->total);
}

SelArgs sel_args(const int32_t* faces, int64_t V, int64_t F, const uint8_t* keep, void* ws, const SelLayout& L) {
  SelArgs a;
  memset(&a, 0, sizeof(a));
  a.faces = faces;
  a.keep = keep;
  a.V = (int)V;
  a.F = (int)F;
  a.used = at<int>(ws, L.used);
  a.newidx = at<int>(ws, L.newidx);
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  return a;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_raycast_ws_bytes(int64_t F, int64_t cap_entries, const int* dims3, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(0, F)) return rc;
  if (int rc = check_rc_entries(cap_entries)) return rc;
  if (int rc = check_md_dims(dims3)) return rc;
  *bytes = rc_layout(F, cap_entries, dims3).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_raycast_grid_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell,
                                     const int* dims3, int64_t* counts, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (int rc = check_md_grid(0, 0, lo3, cell, dims3)) return rc;
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  RcGridArgs a = rc_grid_args(verts, faces, V, F, lo3, cell, dims3);
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_rc_grid_count(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_raycast_grid_fill(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell,
                                    const int* dims3, int64_t cap_entries, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (int rc = check_md_grid(0, 0, lo3, cell, dims3)) return rc;
  if (int rc = check_rc_entries(cap_entries)) return rc;
  const RcLayout L = rc_layout(F, cap_entries, dims3);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  RcGridArgs a = rc_grid_args(verts, faces, V, F, lo3, cell, dims3);
  rc_grid_ws(&a, cap_entries, ws, L);
  HIP_TRY(launch_rc_grid_fill(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_raycast(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* lo3, float cell, const int* dims3,
                          int64_t cap_entries, const void* ws, size_t ws_bytes, const float* origins, const float* dirs,
                          const int32_t* skip, int64_t N, double tmin, double tmax, int any_hit, double* t, double* uv, int32_t* face,
                          int8_t* side, uint8_t* occluded, int64_t cap_n, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (int rc = check_md_grid(0, 0, lo3, cell, dims3)) return rc;
  if (int rc = check_rc_entries(cap_entries)) return rc;
  if (N < 0 || N >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "N=%lld: a ray count in [0, 2^31)", (long long)N);
  if (int rc = check_cap("cap_n", cap_n)) return rc;
  if (tmin != tmin || tmax != tmax) return fail(NERF_HIP_ERR_ARG, "tmin=%g tmax=%g: the window's ends may be infinite, not NaN", tmin, tmax);
  if (N > 0 && (!origins || !dirs)) return fail(NERF_HIP_ERR_ARG, "origins / dirs is null");
  if (N > 0 && cap_n > 0) {
    if (any_hit) {
      if (!occluded) return fail(NERF_HIP_ERR_ARG, "occluded is null");
    } else {
      if (!t || !uv || !face || !side) return fail(NERF_HIP_ERR_ARG, "t / uv / face / side is null");
      if ((((uintptr_t)t | (uintptr_t)uv) & 7) != 0) return fail(NERF_HIP_ERR_ARG, "t and uv must be 8-byte aligned");
    }
  }
  const RcLayout L = rc_layout(F, cap_entries, dims3);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (int rc = check_device()) return rc;
  RcCastArgs a;
  memset(&a, 0, sizeof(a));
  a.g = rc_grid_args(verts, faces, V, F, lo3, cell, dims3);
  rc_grid_ws(&a.g, cap_entries, const_cast<void*>(ws), L);
  a.orig = origins;
  a.dir = dirs;
  a.skip = skip;
  a.N = N;
  a.cap_n = cap_n;
  a.tmin = tmin;
  a.tmax = tmax;
  a.t = t;
  a.uv = uv;
  a.face = face;
  a.side = reinterpret_cast<signed char*>(side);
  a.occluded = occluded;
  HIP_TRY(launch_rc_cast(a, any_hit != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_face_rays(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* cam_o3, const double* Q9, int H,
                            int W, float* orig, float* dir, uint8_t* valid, int64_t cap_f, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (!cam_o3 || !Q9) return fail(NERF_HIP_ERR_ARG, "cam_o3 / Q9 is null");
  if (int rc = check_finite3(cam_o3, "cam_o", "the camera's position")) return rc;
  for (int c = 0; c < 9; ++c)
    if (!isfinite(Q9[c])) return fail(NERF_HIP_ERR_ARG, "Q[%d]=%g: the camera's matrix must be finite", c, Q9[c]);
  if (H < 1 || W < 1) return fail(NERF_HIP_ERR_ARG, "H=%d W=%d: an image has at least one pixel", H, W);
  if (int rc = check_cap("cap_f", cap_f)) return rc;
  if (F > 0 && cap_f > 0 && (!orig || !dir || !valid)) return fail(NERF_HIP_ERR_ARG, "orig / dir / valid is null");
  if (int rc = check_device()) return rc;
  RcFaceRaysArgs a;
  memset(&a, 0, sizeof(a));
  a.verts = verts;
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  for (int c = 0; c < 3; ++c) a.cam[c] = cam_o3[c];
  for (int c = 0; c < 9; ++c) a.Q[c] = Q9[c];
  a.H = H;
  a.W = W;
  a.orig = orig;
  a.dir = dir;
  a.valid = valid;
  a.cap_f = cap_f;
  HIP_TRY(launch_rc_face_rays(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_select_faces_ws_bytes(int64_t V, int64_t F, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_mesh_sizes(V, F)) return rc;
  *bytes = sel_layout(V, F).total;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_select_faces_count(const int32_t* faces, int64_t V, int64_t F, const uint8_t* keep, void* ws, size_t ws_bytes,
                                     int64_t* counts, void* stream) {
  SelLayout L;
  if (int rc = check_sel(faces, V, F, keep, ws, ws_bytes, &L)) return rc;
  if (int rc = check_out(counts, "counts", 8)) return rc;
  if (int rc = check_device()) return rc;
  SelArgs a = sel_args(faces, V, F, keep, ws, L);
  a.counts = reinterpret_cast<long long*>(counts);
  HIP_TRY(launch_sel_count(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_select_faces_emit(const float* verts, const float* normals, const float* rgb, const int32_t* faces, int64_t V, int64_t F,
                                    const uint8_t* keep, void* ws, size_t ws_bytes, float* out_verts, float* out_normals, float* out_rgb,
                                    int32_t* out_faces, int64_t max_v, int64_t max_f, void* stream) {
  SelLayout L;
  if (int rc = check_sel(faces, V, F, keep, ws, ws_bytes, &L)) return rc;
  if (V > 0 && !verts) return fail(NERF_HIP_ERR_ARG, "verts is null");
  if (int rc = check_caps(max_v, max_f)) return rc;
  if (max_v > 0 && (!out_verts || (normals && !out_normals) || (rgb && !out_rgb))) return fail(NERF_HIP_ERR_ARG, "an output of max_v rows is null");
  if (max_f > 0 && !out_faces) return fail(NERF_HIP_ERR_ARG, "out_faces is null");
  if (int rc = check_device()) return rc;
  SelArgs a = sel_args(faces, V, F, keep, ws, L);
  a.verts = verts;
  a.normals = normals;
  a.rgb = rgb;
  a.counts = at<long long>(ws, L.scratch);
  a.out_verts = out_verts;
  a.out_normals = out_normals;
  a.out_rgb = out_rgb;
  a.out_faces = out_faces;
  a.max_v = max_v;
  a.max_f = max_f;
  HIP_TRY(launch_sel_emit(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

static_assert(TSDF_VIEWS == NERF_HIP_TSDF_VIEWS_PER_LAUNCH, "the header states the kernel's views per launch");

}  // extern "C"

namespace {

// nerf_hip_tsdf_integrate and, with with_color, nerf_hip_tsdf_integrate_color (a null color, or a null rgb with n > 0, is then refused)
int tsdf_integrate(float* tsdf, float* weight, float* color, bool with_color, int nx, int ny, int nz, const float* lo3, const float* step3,
                   const float* depth, const float* opacity, const float* rgb, int n, int H, int W, const float* cam_o, const double* Q,
                   double trunc, float min_opacity, int flags, void* stream) {
  if (int rc = check_grid(nx, ny, nz)) return rc;
  if (n < 0) return fail(NERF_HIP_ERR_ARG, "n=%d < 0", n);
  if (H < 1 || W < 1) return fail(NERF_HIP_ERR_ARG, "H=%d W=%d: an image has at least one pixel", H, W);
  // (H * W first: three 31-bit factors would not fit 64 bits)
  if ((long long)H * W >= (1ll << 31) || (long long)n * ((long long)H * W) >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "n=%d H=%d W=%d: the depth images must stay below 2^31 pixels", n, H, W);
  if ((flags & ~NERF_HIP_TSDF_CARVE) != 0) return fail(NERF_HIP_ERR_ARG, "flags=0x%x: the only flag is NERF_HIP_TSDF_CARVE", flags);
  if (!isfinite(trunc) || !(trunc > 0.0)) return fail(NERF_HIP_ERR_ARG, "trunc=%g: the truncation distance must be finite and > 0", trunc);
  if (min_opacity != min_opacity) return fail(NERF_HIP_ERR_ARG, "min_opacity is NaN");
  if (!tsdf || !weight || !lo3 || !step3) return fail(NERF_HIP_ERR_ARG, "tsdf / weight / lo3 / step3 is null");
  if (with_color) {
    if (int rc = check_out(color, "color", 16)) return rc;
  }
  if (int rc = check_finite3(lo3, "lo", "the lattice's corner")) return rc;
  if (int rc = check_finite3(step3, "step", "the lattice's step")) return rc;
  if (n == 0) return NERF_HIP_OK;  // (empty arrays may have null pointers)
  if (!depth || !cam_o || !Q) return fail(NERF_HIP_ERR_ARG, "depth / cam_o / Q is null");
  if (with_color && !rgb) return fail(NERF_HIP_ERR_ARG, "rgb is null");
  for (int c = 0; c < n; ++c) {
    if (int rc = check_finite3(cam_o + (size_t)c * 3, "cam_o", "a camera's position")) return rc;
    for (int e = 0; e < 9; ++e)
      if (!isfinite(Q[(size_t)c * 9 + e])) return fail(NERF_HIP_ERR_ARG, "Q[%d][%d]=%g: a camera's matrix must be finite", c, e, Q[(size_t)c * 9 + e]);
  }
  if (int rc = check_device()) return rc;
  TsdfArgs a;
  memset(&a, 0, sizeof(a));
  a.tsdf = tsdf;
  a.weight = weight;
  a.color = reinterpret_cast<float4*>(color);
  a.ny = ny;
  a.nz = nz;
  a.npts = nx * ny * nz;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.step[c] = step3[c];
  }
  a.H = H;
  a.W = W;
  a.carve = (flags & NERF_HIP_TSDF_CARVE) != 0;
  a.min_opacity = min_opacity;
  a.trunc = trunc;
  const size_t hw = (size_t)H * W;
  // launches in view order on one stream: each reads the state the one before it wrote
  for (int v0 = 0; v0 < n; v0 += TSDF_VIEWS) {
    a.nviews = n - v0 < TSDF_VIEWS ? n - v0 : TSDF_VIEWS;
    a.depth = depth + (size_t)v0 * hw;
    a.opacity = opacity ? opacity + (size_t)v0 * hw : nullptr;
    a.rgb = with_color ? rgb + (size_t)v0 * hw * 3 : nullptr;
    for (int c = 0; c < a.nviews; ++c) {
      for (int e = 0; e < 9; ++e) a.cam[c].Q[e] = Q[(size_t)(v0 + c) * 9 + e];
      for (int e = 0; e < 3; ++e) a.cam[c].o[e] = cam_o[(size_t)(v0 + c) * 3 + e];
    }
    HIP_TRY(launch_tsdf_integrate(a, static_cast<hipStream_t>(stream)));
  }
  return NERF_HIP_OK;
}

}  // namespace

extern "C" {

int nerf_hip_tsdf_integrate(float* tsdf, float* weight, int nx, int ny, int nz, const float* lo3, const float* step3, const float* depth,
                            const float* opacity, int n, int H, int W, const float* cam_o, const double* Q, double trunc, float min_opacity,
                            int flags, void* stream) {
  return tsdf_integrate(tsdf, weight, nullptr, false, nx, ny, nz, lo3, step3, depth, opacity, nullptr, n, H, W, cam_o, Q, trunc, min_opacity,
                        flags, stream);
}

int nerf_hip_tsdf_integrate_color(float* tsdf, float* weight, float* color, int nx, int ny, int nz, const float* lo3, const float* step3,
                                  const float* depth, const float* opacity, const float* rgb, int n, int H, int W, const float* cam_o,
                                  const double* Q, double trunc, float min_opacity, int flags, void* stream) {
  return tsdf_integrate(tsdf, weight, color, true, nx, ny, nz, lo3, step3, depth, opacity, rgb, n, H, W, cam_o, Q, trunc, min_opacity, flags,
                        stream);
}

int nerf_hip_tsdf_sample_color(const float* color, int nx, int ny, int nz, const float* lo3, const float* step3, const float* points,
                               int64_t M, float* rgb, uint8_t* valid, void* stream) {
  if (int rc = check_grid(nx, ny, nz)) return rc;
  if (M < 0) return fail(NERF_HIP_ERR_ARG, "M=%lld < 0", (long long)M);
  if (M >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "M=%lld: a call samples fewer than 2^31 points", (long long)M);
  if (!lo3 || !step3) return fail(NERF_HIP_ERR_ARG, "lo3 / step3 is null");
  if (int rc = check_out(color, "color", 16)) return rc;
  if (int rc = check_finite3(lo3, "lo", "the lattice's corner")) return rc;
  const int dims[3] = {nx, ny, nz};
  for (int c = 0; c < 3; ++c)
    if (dims[c] > 1 && !(step3[c] > 0.0f && isfinite(step3[c])))
      return fail(NERF_HIP_ERR_ARG, "step[%d] = %g: must be positive and finite along a dimension of more than one point", c, (double)step3[c]);
  if (M == 0) return NERF_HIP_OK;  // (empty arrays may have null pointers)
  if (!points || !rgb || !valid) return fail(NERF_HIP_ERR_ARG, "points / rgb / valid is null");
  if (int rc = check_device()) return rc;
  TsdfSampleArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points;
  a.color = reinterpret_cast<const float4*>(color);
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = lo3[c];
    a.step[c] = step3[c];
  }
  a.rgb = rgb;
  a.valid = valid;
  a.M = M;
  HIP_TRY(launch_tsdf_sample_color(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

struct AtlasDims {
  int c, Sx, Sy, W, H;
};

// rule TA's sizes of the atlas of F faces with charts of n texels, in integers, and its refusals
int atlas_dims(int64_t F, int n, AtlasDims* d) {
  if (n < 2) return fail(NERF_HIP_ERR_ARG, "n=%d: a chart has at least 2 texels along its edge", n);
  if (F < 0) return fail(NERF_HIP_ERR_ARG, "F=%lld < 0", (long long)F);
  if (F > ((1ll << 31) - 1) / 3) return fail(NERF_HIP_ERR_ARG, "F=%lld: the 3 F entries of the UV table must stay below 2^31", (long long)F);
  const long long c = (long long)n + 5, K = (F + 1) / 2;
  long long Sx = 0;
  while (Sx * Sx < K) ++Sx;  // (K < 2^29: at most 2^14.5 steps, on the host)
  const long long Sy = Sx > 0 ? (K + Sx - 1) / Sx : 0;
  const long long W = Sx * c, H = Sy * c;
  if (W >= (1ll << 31) || H >= (1ll << 31) || W * H >= (1ll << 31))
    return fail(NERF_HIP_ERR_ARG, "F=%lld n=%d: the atlas of %lld x %lld texels must stay below 2^31 texels", (long long)F, n, W, H);
  d->c = (int)c, d->Sx = (int)Sx, d->Sy = (int)Sy, d->W = (int)W, d->H = (int)H;
  return NERF_HIP_OK;
}

}  // namespace

extern "C" {

int nerf_hip_mesh_atlas_dims(int64_t F, int n, int* out5) {
  if (!out5) return fail(NERF_HIP_ERR_ARG, "out5 is null");
  AtlasDims d;
  if (int rc = atlas_dims(F, n, &d)) return rc;
  out5[0] = d.c, out5[1] = d.Sx, out5[2] = d.Sy, out5[3] = d.W, out5[4] = d.H;
  return NERF_HIP_OK;
}

int nerf_hip_mesh_atlas_texels(const float* verts, const float* normals, const int32_t* faces, int64_t V, int64_t F, int n, int row0,
                               int rows, float* points, float* dirs, uint8_t* mask, void* stream) {
  if (int rc = check_mesh_sizes(V, F)) return rc;
  AtlasDims d;
  if (int rc = atlas_dims(F, n, &d)) return rc;
  if (row0 < 0 || rows < 0 || (long long)row0 + rows > d.H)
    return fail(NERF_HIP_ERR_ARG, "row0=%d rows=%d: a band of the atlas's %d rows", row0, rows, d.H);
  if (int rc = check_mesh_ptrs(verts, faces, V, F)) return rc;
  if (V > 0 && !normals) return fail(NERF_HIP_ERR_ARG, "normals is null");
  const long long T = (long long)rows * d.W;
  if (T == 0) return NERF_HIP_OK;  // (empty arrays may have null pointers)
  if (!points || !dirs || !mask) return fail(NERF_HIP_ERR_ARG, "points / dirs / mask is null");
  if (int rc = check_device()) return rc;
  AtlasTexelsArgs a;
  memset(&a, 0, sizeof(a));
  a.verts = verts;
  a.normals = normals;
  a.faces = faces;
  a.V = (int)V;
  a.F = (int)F;
  a.n = n;
  a.c = d.c;
  a.Sx = d.Sx;
  a.W = d.W;
  a.row0 = row0;
  a.T = T;
  a.points = points;
  a.dirs = dirs;
  a.mask = mask;
  HIP_TRY(launch_atlas_texels(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_mesh_texture_sample(const float* image, int64_t F, int n, const int32_t* face, const double* uv, int64_t N,
                                 const float* background3, float* rgb, uint8_t* valid, void* stream) {
  AtlasDims d;
  if (int rc = atlas_dims(F, n, &d)) return rc;
  if (N < 0) return fail(NERF_HIP_ERR_ARG, "N=%lld < 0", (long long)N);
  if (N >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "N=%lld: a call makes fewer than 2^31 lookups", (long long)N);
  if (!background3) return fail(NERF_HIP_ERR_ARG, "background3 is null");
  if (N == 0) return NERF_HIP_OK;  // (empty arrays may have null pointers)
  if (F > 0 && !image) return fail(NERF_HIP_ERR_ARG, "image is null");
  if (!face || !rgb || !valid) return fail(NERF_HIP_ERR_ARG, "face / rgb / valid is null");
  if (int rc = check_out(uv, "uv", 8)) return rc;
  if (int rc = check_device()) return rc;
  TextureSampleArgs a;
  memset(&a, 0, sizeof(a));
  a.image = image;
  a.F = (int)F;
  a.n = n;
  a.c = d.c;
  a.Sx = d.Sx;
  a.W = d.W;
  a.face = face;
  a.uv = uv;
  a.N = N;
  for (int e = 0; e < 3; ++e) a.bg[e] = background3[e];
  a.rgb = rgb;
  a.valid = valid;
  HIP_TRY(launch_texture_sample(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"

namespace {

// Shapes of the image-metrics calls: H, W >= the SSIM window, a view's element count below 2^31.  Sets the tile counts.
int check_metrics_shape(int n, int H, int W, int* tiles_x, int* tiles) {
  if (n < 0) return fail(NERF_HIP_ERR_ARG, "n=%d < 0", n);
  if (H < MT_WIN || W < MT_WIN) return fail(NERF_HIP_ERR_ARG, "H=%d W=%d: SSIM's %d x %d window needs H, W >= %d", H, W, MT_WIN, MT_WIN, MT_WIN);
  const long long per_view = (long long)H * W * 3;
  // (with n < 2^31 the whole input then stays below 2^62 values)
  if (per_view >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "H=%d W=%d: the element count H * W * 3 of a view must stay below 2^31", H, W);
  *tiles_x = metrics_tiles_x(W);
  *tiles = *tiles_x * metrics_tiles_y(H);
  return NERF_HIP_OK;
}

void metrics_window(double g[MT_WIN]) {  // exp(-((k - 5) / 1.5)^2 / 2), normalised to sum 1 (summed in k order)
  double s = 0.0;
  for (int k = 0; k < MT_WIN; ++k) {
    const double u = (k - MT_WIN / 2) / 1.5;
    g[k] = exp(-0.5 * (u * u));
    s += g[k];
  }
  for (int k = 0; k < MT_WIN; ++k) g[k] /= s;
}

}  // namespace

extern "C" {

int nerf_hip_metrics_ws_bytes(int n, int H, int W, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  int tiles_x = 0, tiles = 0;
  if (int rc = check_metrics_shape(n, H, W, &tiles_x, &tiles)) return rc;
  *bytes = al((size_t)n * tiles * 2 * sizeof(double));
  return NERF_HIP_OK;
}

int nerf_hip_image_metrics(const float* pred, const float* gt, int n, int H, int W, double* mse, double* ssim, void* ws, size_t ws_bytes,
                           void* stream) {
  int tiles_x = 0, tiles = 0;
  if (int rc = check_metrics_shape(n, H, W, &tiles_x, &tiles)) return rc;
  if (n == 0) return NERF_HIP_OK;  // (empty buffers may have null pointers)
  if (!pred || !gt || !mse || !ssim) return fail(NERF_HIP_ERR_ARG, "null argument (pred, gt, mse and ssim are required)");
  if (int rc = check_ws(ws, ws_bytes, al((size_t)n * tiles * 2 * sizeof(double)))) return rc;
  if (int rc = check_device()) return rc;
  MetricsArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred;
  a.gt = gt;
  a.n = n;
  a.H = H;
  a.W = W;
  a.tiles_x = tiles_x;
  a.tiles = tiles;
  a.part = static_cast<double*>(ws);
  a.mse = mse;
  a.ssim = ssim;
  metrics_window(a.g);
  HIP_TRY(launch_image_metrics(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"
