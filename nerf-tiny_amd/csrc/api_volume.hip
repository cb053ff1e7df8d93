// api_volume.hip -- the SH radiance volume part of the extern "C" surface of libnerf_hip.so (include/nerf_hip.h: rules VA, VS, VO, VL,
// VR, VG, VU, VM, VT, VX, VP, VC, VCG, VCU, VCT, VI, VQ-A, VQ-U, VQ-D, VQ-X, VQ-G and VQ-V): host code only, as api_geometry.hip -- argument checks, workspace carve-up and kernel sequencing on
// the caller's stream.  No allocation, no host sync.
#include <math.h>

#include "api_common.h"

using namespace nerf;

namespace {

static_assert(VOL_MAX_STEPS == NERF_HIP_VOLUME_MAX_STEPS, "the header states the kernel's cap on the steps of a ray");

const float kDirs[NERF_HIP_VOLUME_NDIRS * 3] = NERF_HIP_VOLUME_DIRS;
const float kShB[NERF_HIP_VOLUME_NDIRS * 9] = NERF_HIP_VOLUME_SH_B;

struct VolLayout {
  size_t tot, base, count, total;
};
VolLayout vol_layout(long long npts) {
  VolLayout L;
  Carve c;
  const size_t nb = (size_t)cc_blocks(npts);
  L.tot = c.take(nb * 4);
  L.base = c.take(nb * 4);
  L.count = c.take(8);
  L.total = c.o;
  return L;
}

// the lattice of a volume: at least one cell per axis, below 2^31 points
int check_lattice(int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2) return fail(NERF_HIP_ERR_ARG, "volume %d x %d x %d: every dimension must be at least 2", nx, ny, nz);
  return check_grid(nx, ny, nz);
}

int check_degree(int degree) {
  if (degree < 0 || degree > 2) return fail(NERF_HIP_ERR_ARG, "degree=%d: 0, 1 or 2", degree);
  return NERF_HIP_OK;
}

int check_count(const char* name, int64_t n) {
  if (n < 0) return fail(NERF_HIP_ERR_ARG, "%s=%lld < 0", name, (long long)n);
  if (n >= (1ll << 31)) return fail(NERF_HIP_ERR_ARG, "%s=%lld: a call takes fewer than 2^31 items", name, (long long)n);
  return NERF_HIP_OK;
}

int check_lo_step(const float* lo3, const float* step3) {
  if (!lo3 || !step3) return fail(NERF_HIP_ERR_ARG, "lo3 / step3 is null");
  if (int rc = check_finite3(lo3, "lo", "the lattice's corner")) return rc;
  for (int c = 0; c < 3; ++c)
    if (!(step3[c] > 0.0f && isfinite(step3[c]))) return fail(NERF_HIP_ERR_ARG, "step[%d]=%g: the lattice's step must be finite and > 0", c, (double)step3[c]);
  return NERF_HIP_OK;
}

VolLattice lattice(int nx, int ny, int nz, const float* lo3, const float* step3) {
  VolLattice g;
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  for (int c = 0; c < 3; ++c) {
    g.lo[c] = lo3[c];
    g.step[c] = step3[c];
  }
  return g;
}

// blocks per axis of edge B: ceil((n - 1) / B)
int blocks_of(int n, int B) { return (int)(((long long)n - 1 + B - 1) / B); }

// rule VU's beta^step: by squaring, every product one fp64 rounding in this order
double pow_by_squaring(double beta, int64_t step) {
  double p = 1.0, b = beta;
  for (int64_t e = step; e > 0; e >>= 1) {
    if (e & 1) p = p * b;
    b = b * b;
  }
  return p;
}

// ---- rule VC's arguments ----

int check_half(int half) {
  if (half != 0 && half != 1) return fail(NERF_HIP_ERR_ARG, "half=%d: 0 (fp32 rows) or 1 (fp16 rows)", half);
  return NERF_HIP_OK;
}

// the rows of a compact volume: at most one per lattice point
int check_rows(int64_t n, int nx, int ny, int nz) {
  if (n < 0 || n > (int64_t)nx * ny * nz) return fail(NERF_HIP_ERR_ARG, "n=%lld: the rows of a %d x %d x %d lattice number 0 .. %lld", (long long)n, nx, ny, nz, (long long)nx * ny * nz);
  return NERF_HIP_OK;
}

// the arrays a lookup reads; without rows (n = 0) only the slot lattice is there
int check_compact(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n, int half, int nx, int ny, int nz) {
  if (int rc = check_half(half)) return rc;
  if (int rc = check_rows(n, nx, ny, nz)) return rc;
  if (int rc = check_out(slot, "slot", 4)) return rc;
  if (n > 0) {
    if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
    if (int rc = check_out(coef_rows, "coef_rows", half ? 8 : 4)) return rc;
  }
  return NERF_HIP_OK;
}

VolCompact compact(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n) {
  VolCompact c;
  c.slot = slot;
  c.sigma_rows = sigma_rows;
  c.coef_rows = coef_rows;
  c.n = n;
  return c;
}

// the per-row accumulators of rules VCG, VCU and VCT: without rows (n = 0) they may be null, never misaligned
int check_row_accumulators(const int64_t* acc_sigma_rows, const int64_t* acc_coef_rows, int64_t n) {
  if (n > 0 || acc_sigma_rows) {
    if (int rc = check_out(acc_sigma_rows, "acc_sigma_rows", 8)) return rc;
  }
  if (n > 0 || acc_coef_rows) {
    if (int rc = check_out(acc_coef_rows, "acc_coef_rows", 8)) return rc;
  }
  return NERF_HIP_OK;
}

// rule VQ's codebook: 1 .. 65536 codes (a code is a uint16)
static_assert(VQ_SHIFT == NERF_HIP_VOLUME_VQ_SHIFT && VQ_MAX_CODES == NERF_HIP_VOLUME_VQ_MAX_CODES, "the header states rule VQ's constants");
int check_codes(int64_t K) {
  if (K < 1 || K > VQ_MAX_CODES) return fail(NERF_HIP_ERR_ARG, "K=%lld: a codebook has 1 .. %d codes", (long long)K, VQ_MAX_CODES);
  return NERF_HIP_OK;
}

int active(const float* sigma, int nx, int ny, int nz, void* ws, size_t ws_bytes, int64_t* count, int32_t* index, int64_t max_n, bool emit,
           void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  const VolLayout L = vol_layout((long long)nx * ny * nz);
  if (int rc = check_ws(ws, ws_bytes, L.total)) return rc;
  if (emit) {
    if (int rc = check_cap("max_n", max_n)) return rc;
    if (max_n > 0) {
      if (int rc = check_out(index, "index", 4)) return rc;
    }
  } else {
    if (int rc = check_out(count, "count", 8)) return rc;
  }
  if (int rc = check_device()) return rc;
  VolActiveArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.tot = at<int>(ws, L.tot);
  a.base = at<int>(ws, L.base);
  a.count = emit ? at<long long>(ws, L.count) : reinterpret_cast<long long*>(count);
  a.index = index;
  a.max_n = max_n;
  HIP_TRY(launch_volume_active(a, emit, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // namespace

extern "C" {

int nerf_hip_volume_sh_table(float* dirs36, float* b108) {
  if (dirs36) memcpy(dirs36, kDirs, sizeof(kDirs));
  if (b108) memcpy(b108, kShB, sizeof(kShB));
  return NERF_HIP_OK;
}

int nerf_hip_volume_ws_bytes(int nx, int ny, int nz, size_t* bytes) {
  if (!bytes) return fail(NERF_HIP_ERR_ARG, "bytes is null");
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  *bytes = vol_layout((long long)nx * ny * nz).total;
  return NERF_HIP_OK;
}

int nerf_hip_volume_active_count(const float* sigma, int nx, int ny, int nz, void* ws, size_t ws_bytes, int64_t* count, void* stream) {
  return active(sigma, nx, ny, nz, ws, ws_bytes, count, nullptr, 0, false, stream);
}

int nerf_hip_volume_active_emit(const float* sigma, int nx, int ny, int nz, void* ws, size_t ws_bytes, int32_t* index, int64_t max_n,
                                void* stream) {
  return active(sigma, nx, ny, nz, ws, ws_bytes, nullptr, index, max_n, true, stream);
}

int nerf_hip_volume_points(const int32_t* index, int64_t n, int nx, int ny, int nz, const float* lo3, const float* step3, float* points,
                           void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(index, "index", 4)) return rc;
  if (int rc = check_out(points, "points", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolPointsArgs a;
  memset(&a, 0, sizeof(a));
  a.index = index;
  a.n = n;
  a.g = lattice(nx, ny, nz, lo3, step3);
  a.points = points;
  HIP_TRY(launch_volume_points(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_sh_accumulate(float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n, const float* rgb, int k,
                                  void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (k < 0 || k >= NERF_HIP_VOLUME_NDIRS) return fail(NERF_HIP_ERR_ARG, "k=%d: a quadrature direction, 0 .. %d", k, NERF_HIP_VOLUME_NDIRS - 1);
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(index, "index", 4)) return rc;
  if (int rc = check_out(rgb, "rgb", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolShArgs a;
  memset(&a, 0, sizeof(a));
  a.coef = coef;
  a.npts = (long long)nx * ny * nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.index = index;
  a.n = n;
  a.rgb = rgb;
  for (int m = 0; m < 9; ++m) a.b[m] = kShB[k * 9 + m];
  HIP_TRY(launch_volume_sh_accumulate(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_blocks(const float* sigma, int nx, int ny, int nz, int block, uint8_t* occ, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (int rc = check_device()) return rc;
  VolBlocksArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.B = block;
  a.bx = blocks_of(nx, block);
  a.by = blocks_of(ny, block);
  a.bz = blocks_of(nz, block);
  a.occ = occ;
  HIP_TRY(launch_volume_blocks(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_sample(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const float* lo3, const float* step3,
                           const float* points, const float* dirs, int64_t M, float* out_sigma, float* out_rgb, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("M", M)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (M == 0) return NERF_HIP_OK;
  if (int rc = check_out(points, "points", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(out_sigma, "out_sigma", 4)) return rc;
  if (int rc = check_out(out_rgb, "out_rgb", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolSampleArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.g = lattice(nx, ny, nz, lo3, step3);
  a.points = points;
  a.dirs = dirs;
  a.M = M;
  a.out_sigma = out_sigma;
  a.out_rgb = out_rgb;
  HIP_TRY(launch_volume_sample(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_render(const float* sigma, const float* coef, const uint8_t* occ, int nx, int ny, int nz, int degree, int block,
                           const float* lo3, const float* step3, const float* origins, const float* dirs, const float* tmin,
                           const float* tmax, int64_t N, float dt, float t_stop, const float* background3, float* rgb, float* maps,
                           int32_t* steps, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_count("N", N)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (!(dt > 0.0f && isfinite(dt))) return fail(NERF_HIP_ERR_ARG, "dt=%g: the step along the ray must be finite and > 0", (double)dt);
  if (!(t_stop >= 0.0f && t_stop < 1.0f)) return fail(NERF_HIP_ERR_ARG, "t_stop=%g: the transmittance to stop at lies in [0, 1)", (double)t_stop);
  if (!background3) return fail(NERF_HIP_ERR_ARG, "background3 is null");
  if (int rc = check_finite3(background3, "background", "the background colour")) return rc;
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (N == 0) return NERF_HIP_OK;
  if (int rc = check_out(origins, "origins", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(tmin, "tmin", 4)) return rc;
  if (int rc = check_out(tmax, "tmax", 4)) return rc;
  if (int rc = check_out(rgb, "rgb", 4)) return rc;
  if (int rc = check_out(maps, "maps", 4)) return rc;
  if (int rc = check_out(steps, "steps", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolRenderArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.occ = occ;
  a.g = lattice(nx, ny, nz, lo3, step3);
  a.B = block;
  a.bx = blocks_of(nx, block);
  a.by = blocks_of(ny, block);
  a.bz = blocks_of(nz, block);
  a.origins = origins;
  a.dirs = dirs;
  a.tmin = tmin;
  a.tmax = tmax;
  a.N = N;
  a.dt = dt;
  a.t_stop = t_stop;
  for (int c = 0; c < 3; ++c) a.bg[c] = background3[c];
  a.rgb = rgb;
  a.maps = maps;
  a.steps = steps;
  HIP_TRY(launch_volume_render(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_render_backward(const float* sigma, const float* coef, const uint8_t* occ, int nx, int ny, int nz, int degree,
                                    int block, const float* lo3, const float* step3, const float* origins, const float* dirs,
                                    const float* tmin, const float* tmax, int64_t N, float dt, float t_stop, const float* background3,
                                    const float* g_rgb, const float* g_maps, int64_t* acc_sigma, int64_t* acc_coef, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_count("N", N)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (!(dt > 0.0f && isfinite(dt))) return fail(NERF_HIP_ERR_ARG, "dt=%g: the step along the ray must be finite and > 0", (double)dt);
  if (!(t_stop >= 0.0f && t_stop < 1.0f)) return fail(NERF_HIP_ERR_ARG, "t_stop=%g: the transmittance to stop at lies in [0, 1)", (double)t_stop);
  if (!background3) return fail(NERF_HIP_ERR_ARG, "background3 is null");
  if (int rc = check_finite3(background3, "background", "the background colour")) return rc;
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (int rc = check_out(acc_sigma, "acc_sigma", 8)) return rc;
  if (int rc = check_out(acc_coef, "acc_coef", 8)) return rc;
  if (g_maps && ((uintptr_t)g_maps & 3) != 0) return fail(NERF_HIP_ERR_ARG, "g_maps must be 4-byte aligned");
  if (N == 0) return NERF_HIP_OK;
  if (int rc = check_out(origins, "origins", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(tmin, "tmin", 4)) return rc;
  if (int rc = check_out(tmax, "tmax", 4)) return rc;
  if (int rc = check_out(g_rgb, "g_rgb", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolGradArgs a;
  memset(&a, 0, sizeof(a));
  a.r.sigma = sigma;
  a.r.coef = coef;
  a.r.occ = occ;
  a.r.g = lattice(nx, ny, nz, lo3, step3);
  a.r.B = block;
  a.r.bx = blocks_of(nx, block);
  a.r.by = blocks_of(ny, block);
  a.r.bz = blocks_of(nz, block);
  a.r.origins = origins;
  a.r.dirs = dirs;
  a.r.tmin = tmin;
  a.r.tmax = tmax;
  a.r.N = N;
  a.r.dt = dt;
  a.r.t_stop = t_stop;
  for (int c = 0; c < 3; ++c) a.r.bg[c] = background3[c];
  a.g_rgb = g_rgb;
  a.g_maps = g_maps;
  a.acc_sigma = reinterpret_cast<long long*>(acc_sigma);
  a.acc_coef = reinterpret_cast<long long*>(acc_coef);
  HIP_TRY(launch_volume_render_backward(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_adam_step(float* sigma, float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                              int64_t* acc_sigma, int64_t* acc_coef, float* m, float* v, double grad_scale, int64_t step,
                              double lr_sigma, double lr_coef, double beta1, double beta2, double eps, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (step < 1) return fail(NERF_HIP_ERR_ARG, "step=%lld: the first update is step 1", (long long)step);
  if (!isfinite(grad_scale)) return fail(NERF_HIP_ERR_ARG, "grad_scale=%g must be finite", grad_scale);
  if (!isfinite(lr_sigma) || !isfinite(lr_coef)) return fail(NERF_HIP_ERR_ARG, "lr_sigma=%g lr_coef=%g: the rates must be finite", lr_sigma, lr_coef);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(NERF_HIP_ERR_ARG, "beta1=%g beta2=%g: both lie in [0, 1)", beta1, beta2);
  if (!(eps >= 0.0 && isfinite(eps))) return fail(NERF_HIP_ERR_ARG, "eps=%g must be finite and >= 0", eps);
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(acc_sigma, "acc_sigma", 8)) return rc;
  if (int rc = check_out(acc_coef, "acc_coef", 8)) return rc;
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(index, "index", 4)) return rc;
  if (int rc = check_out(m, "m", 4)) return rc;
  if (int rc = check_out(v, "v", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolAdamArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.npts = (long long)nx * ny * nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.index = index;
  a.n = n;
  a.acc_sigma = reinterpret_cast<long long*>(acc_sigma);
  a.acc_coef = reinterpret_cast<long long*>(acc_coef);
  a.m = m;
  a.v = v;
  a.grad_scale = grad_scale;
  a.lr_sigma = lr_sigma;
  a.lr_coef = lr_coef;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.c1 = 1.0 - pow_by_squaring(beta1, step);
  a.c2 = 1.0 - pow_by_squaring(beta2, step);
  HIP_TRY(launch_volume_adam_step(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_member_mask(const int32_t* index, int64_t n, int nx, int ny, int nz, uint8_t* member, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (int rc = check_out(member, "member", 1)) return rc;
  if (n > 0) {
    if (int rc = check_out(index, "index", 4)) return rc;
  }
  if (int rc = check_device()) return rc;
  VolMemberArgs a;
  memset(&a, 0, sizeof(a));
  a.index = index;
  a.n = n;
  a.npts = (long long)nx * ny * nz;
  a.member = member;
  HIP_TRY(launch_volume_member_mask(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_tv_backward(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                                const uint8_t* member, double w_sigma, double w_coef, double eps, int64_t* acc_sigma, int64_t* acc_coef,
                                void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (!(eps > 0.0 && isfinite(eps))) return fail(NERF_HIP_ERR_ARG, "eps=%g must be finite and > 0", eps);
  if (!(w_sigma >= 0.0 && w_sigma <= 65536.0) || !(w_coef >= 0.0 && w_coef <= 65536.0))
    return fail(NERF_HIP_ERR_ARG, "w_sigma=%g w_coef=%g: the weights lie in [0, 2^16]", w_sigma, w_coef);
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(member, "member", 1)) return rc;
  if (int rc = check_out(acc_sigma, "acc_sigma", 8)) return rc;
  if (int rc = check_out(acc_coef, "acc_coef", 8)) return rc;
  if (n == 0 || (w_sigma == 0.0 && w_coef == 0.0)) return NERF_HIP_OK;
  if (int rc = check_out(index, "index", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolTvArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.index = index;
  a.n = n;
  a.member = member;
  a.w_sigma = w_sigma;
  a.w_coef = w_coef;
  a.eps = eps;
  a.acc_sigma = reinterpret_cast<long long*>(acc_sigma);
  a.acc_coef = reinterpret_cast<long long*>(acc_coef);
  HIP_TRY(launch_volume_tv_backward(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_upsample(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, float* sigma2, float* coef2,
                             void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if ((2ll * nx - 1) * (2ll * ny - 1) >= (1ll << 31) || (2ll * nx - 1) * (2ll * ny - 1) * (2ll * nz - 1) >= (1ll << 31))
    return fail(NERF_HIP_ERR_ARG, "volume %d x %d x %d: the refined lattice must stay below 2^31 points", nx, ny, nz);
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(sigma2, "sigma2", 4)) return rc;
  if (int rc = check_out(coef2, "coef2", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolUpsampleArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.sigma2 = sigma2;
  a.coef2 = coef2;
  HIP_TRY(launch_volume_upsample(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_prune(float* sigma, float* coef, int nx, int ny, int nz, int degree, float threshold, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (!(threshold >= 0.0f && isfinite(threshold))) return fail(NERF_HIP_ERR_ARG, "threshold=%g must be finite and >= 0", (double)threshold);
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolPruneArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.threshold = threshold;
  HIP_TRY(launch_volume_prune(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_slots(const int32_t* index, int64_t n, int nx, int ny, int nz, int32_t* slot, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_rows(n, nx, ny, nz)) return rc;
  if (int rc = check_out(slot, "slot", 4)) return rc;
  if (n > 0) {
    if (int rc = check_out(index, "index", 4)) return rc;
  }
  if (int rc = check_device()) return rc;
  VolSlotsArgs a;
  memset(&a, 0, sizeof(a));
  a.index = index;
  a.n = n;
  a.npts = (long long)nx * ny * nz;
  a.slot = slot;
  HIP_TRY(launch_volume_compact_slots(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_pack(const float* sigma, const float* coef, int nx, int ny, int nz, int degree, const int32_t* index, int64_t n,
                                 int half, float* sigma_rows, void* coef_rows, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_half(half)) return rc;
  if (int rc = check_rows(n, nx, ny, nz)) return rc;
  if (n == 0) return NERF_HIP_OK;
  if (!index && n != (int64_t)nx * ny * nz) return fail(NERF_HIP_ERR_ARG, "n=%lld: without an index the rows are the lattice's %lld points", (long long)n, (long long)nx * ny * nz);
  if ((sigma == nullptr) != (sigma_rows == nullptr)) return fail(NERF_HIP_ERR_ARG, "sigma and sigma_rows: both, or both null");
  if (sigma) {
    if (int rc = check_out(sigma, "sigma", 4)) return rc;
    if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
  }
  if (int rc = check_out(coef, "coef", 4)) return rc;
  if (int rc = check_out(coef_rows, "coef_rows", half ? 8 : 4)) return rc;
  if (index) {
    if (int rc = check_out(index, "index", 4)) return rc;
  }
  if (int rc = check_device()) return rc;
  VolPackArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = const_cast<float*>(sigma);
  a.coef = const_cast<float*>(coef);
  a.npts = (long long)nx * ny * nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.index = index;
  a.n = n;
  a.sigma_rows = sigma_rows;
  a.coef_rows = coef_rows;
  HIP_TRY(launch_volume_compact_pack(a, half != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_unpack(const float* sigma_rows, const void* coef_rows, int half, const int32_t* index, int64_t n, int nx, int ny,
                                   int nz, int degree, float* sigma, float* coef, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_half(half)) return rc;
  if (int rc = check_rows(n, nx, ny, nz)) return rc;
  if ((coef == nullptr) != (coef_rows == nullptr) && n > 0) return fail(NERF_HIP_ERR_ARG, "coef and coef_rows: both, or both null");
  if (int rc = check_out(sigma, "sigma", 4)) return rc;
  if (coef) {
    if (int rc = check_out(coef, "coef", 4)) return rc;
  }
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
  if (coef) {
    if (int rc = check_out(coef_rows, "coef_rows", half ? 8 : 4)) return rc;
  }
  if (int rc = check_out(index, "index", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolPackArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma = sigma;
  a.coef = coef;
  a.npts = (long long)nx * ny * nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.index = index;
  a.n = n;
  a.sigma_rows = const_cast<float*>(sigma_rows);
  a.coef_rows = const_cast<void*>(coef_rows);
  HIP_TRY(launch_volume_compact_unpack(a, half != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_sample(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n, int half, int nx, int ny,
                                   int nz, int degree, const float* lo3, const float* step3, const float* points, const float* dirs,
                                   int64_t M, float* out_sigma, float* out_rgb, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("M", M)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (int rc = check_compact(slot, sigma_rows, coef_rows, n, half, nx, ny, nz)) return rc;
  if (M == 0) return NERF_HIP_OK;
  if (int rc = check_out(points, "points", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(out_sigma, "out_sigma", 4)) return rc;
  if (int rc = check_out(out_rgb, "out_rgb", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolCompactSampleArgs a;
  memset(&a, 0, sizeof(a));
  a.c = compact(slot, sigma_rows, coef_rows, n);
  a.g = lattice(nx, ny, nz, lo3, step3);
  a.points = points;
  a.dirs = dirs;
  a.M = M;
  a.out_sigma = out_sigma;
  a.out_rgb = out_rgb;
  HIP_TRY(launch_volume_compact_sample(a, (degree + 1) * (degree + 1), half != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_render(const int32_t* slot, const float* sigma_rows, const void* coef_rows, int64_t n, int half,
                                   const uint8_t* occ, int nx, int ny, int nz, int degree, int block, const float* lo3, const float* step3,
                                   const float* origins, const float* dirs, const float* tmin, const float* tmax, int64_t N, float dt,
                                   float t_stop, const float* background3, float* rgb, float* maps, int32_t* steps, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_count("N", N)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (!(dt > 0.0f && isfinite(dt))) return fail(NERF_HIP_ERR_ARG, "dt=%g: the step along the ray must be finite and > 0", (double)dt);
  if (!(t_stop >= 0.0f && t_stop < 1.0f)) return fail(NERF_HIP_ERR_ARG, "t_stop=%g: the transmittance to stop at lies in [0, 1)", (double)t_stop);
  if (!background3) return fail(NERF_HIP_ERR_ARG, "background3 is null");
  if (int rc = check_finite3(background3, "background", "the background colour")) return rc;
  if (int rc = check_compact(slot, sigma_rows, coef_rows, n, half, nx, ny, nz)) return rc;
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (N == 0) return NERF_HIP_OK;
  if (int rc = check_out(origins, "origins", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(tmin, "tmin", 4)) return rc;
  if (int rc = check_out(tmax, "tmax", 4)) return rc;
  if (int rc = check_out(rgb, "rgb", 4)) return rc;
  if (int rc = check_out(maps, "maps", 4)) return rc;
  if (int rc = check_out(steps, "steps", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolCompactRenderArgs a;
  memset(&a, 0, sizeof(a));
  a.c = compact(slot, sigma_rows, coef_rows, n);
  a.r.occ = occ;
  a.r.g = lattice(nx, ny, nz, lo3, step3);
  a.r.B = block;
  a.r.bx = blocks_of(nx, block);
  a.r.by = blocks_of(ny, block);
  a.r.bz = blocks_of(nz, block);
  a.r.origins = origins;
  a.r.dirs = dirs;
  a.r.tmin = tmin;
  a.r.tmax = tmax;
  a.r.N = N;
  a.r.dt = dt;
  a.r.t_stop = t_stop;
  for (int c = 0; c < 3; ++c) a.r.bg[c] = background3[c];
  a.r.rgb = rgb;
  a.r.maps = maps;
  a.r.steps = steps;
  HIP_TRY(launch_volume_compact_render(a, (degree + 1) * (degree + 1), half != 0, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_render_backward(const int32_t* slot, const float* sigma_rows, const float* coef_rows, int64_t n,
                                            const uint8_t* occ, int nx, int ny, int nz, int degree, int block, const float* lo3,
                                            const float* step3, const float* origins, const float* dirs, const float* tmin,
                                            const float* tmax, int64_t N, float dt, float t_stop, const float* background3,
                                            const float* g_rgb, const float* g_maps, int64_t* acc_sigma_rows, int64_t* acc_coef_rows,
                                            void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_count("N", N)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (!(dt > 0.0f && isfinite(dt))) return fail(NERF_HIP_ERR_ARG, "dt=%g: the step along the ray must be finite and > 0", (double)dt);
  if (!(t_stop >= 0.0f && t_stop < 1.0f)) return fail(NERF_HIP_ERR_ARG, "t_stop=%g: the transmittance to stop at lies in [0, 1)", (double)t_stop);
  if (!background3) return fail(NERF_HIP_ERR_ARG, "background3 is null");
  if (int rc = check_finite3(background3, "background", "the background colour")) return rc;
  if (int rc = check_compact(slot, sigma_rows, coef_rows, n, 0, nx, ny, nz)) return rc;
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (int rc = check_row_accumulators(acc_sigma_rows, acc_coef_rows, n)) return rc;
  if (g_maps && ((uintptr_t)g_maps & 3) != 0) return fail(NERF_HIP_ERR_ARG, "g_maps must be 4-byte aligned");
  if (N == 0 || n == 0) return NERF_HIP_OK;
  if (int rc = check_out(origins, "origins", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(tmin, "tmin", 4)) return rc;
  if (int rc = check_out(tmax, "tmax", 4)) return rc;
  if (int rc = check_out(g_rgb, "g_rgb", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolCompactGradArgs a;
  memset(&a, 0, sizeof(a));
  a.c = compact(slot, sigma_rows, coef_rows, n);
  a.r.occ = occ;
  a.r.g = lattice(nx, ny, nz, lo3, step3);
  a.r.B = block;
  a.r.bx = blocks_of(nx, block);
  a.r.by = blocks_of(ny, block);
  a.r.bz = blocks_of(nz, block);
  a.r.origins = origins;
  a.r.dirs = dirs;
  a.r.tmin = tmin;
  a.r.tmax = tmax;
  a.r.N = N;
  a.r.dt = dt;
  a.r.t_stop = t_stop;
  for (int c = 0; c < 3; ++c) a.r.bg[c] = background3[c];
  a.g_rgb = g_rgb;
  a.g_maps = g_maps;
  a.acc_sigma_rows = reinterpret_cast<long long*>(acc_sigma_rows);
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  HIP_TRY(launch_volume_compact_render_backward(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_adam_step(float* sigma_rows, float* coef_rows, int64_t n, int degree, int64_t* acc_sigma_rows,
                                      int64_t* acc_coef_rows, float* m, float* v, double grad_scale, int64_t step, double lr_sigma,
                                      double lr_coef, double beta1, double beta2, double eps, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (step < 1) return fail(NERF_HIP_ERR_ARG, "step=%lld: the first update is step 1", (long long)step);
  if (!isfinite(grad_scale)) return fail(NERF_HIP_ERR_ARG, "grad_scale=%g must be finite", grad_scale);
  if (!isfinite(lr_sigma) || !isfinite(lr_coef)) return fail(NERF_HIP_ERR_ARG, "lr_sigma=%g lr_coef=%g: the rates must be finite", lr_sigma, lr_coef);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(NERF_HIP_ERR_ARG, "beta1=%g beta2=%g: both lie in [0, 1)", beta1, beta2);
  if (!(eps >= 0.0 && isfinite(eps))) return fail(NERF_HIP_ERR_ARG, "eps=%g must be finite and >= 0", eps);
  if (int rc = check_row_accumulators(acc_sigma_rows, acc_coef_rows, n)) return rc;
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
  if (int rc = check_out(coef_rows, "coef_rows", 4)) return rc;
  if (int rc = check_out(m, "m", 4)) return rc;
  if (int rc = check_out(v, "v", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolCompactAdamArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma_rows = sigma_rows;
  a.coef_rows = coef_rows;
  a.ncoef = (degree + 1) * (degree + 1);
  a.n = n;
  a.acc_sigma_rows = reinterpret_cast<long long*>(acc_sigma_rows);
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  a.m = m;
  a.v = v;
  a.grad_scale = grad_scale;
  a.lr_sigma = lr_sigma;
  a.lr_coef = lr_coef;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.c1 = 1.0 - pow_by_squaring(beta1, step);
  a.c2 = 1.0 - pow_by_squaring(beta2, step);
  HIP_TRY(launch_volume_compact_adam_step(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_tv_backward(const int32_t* slot, const float* sigma_rows, const float* coef_rows, const int32_t* point,
                                        int64_t n, int nx, int ny, int nz, int degree, double w_sigma, double w_coef, double eps,
                                        int64_t* acc_sigma_rows, int64_t* acc_coef_rows, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (int rc = check_degree(degree)) return rc;
  if (!(eps > 0.0 && isfinite(eps))) return fail(NERF_HIP_ERR_ARG, "eps=%g must be finite and > 0", eps);
  if (!(w_sigma >= 0.0 && w_sigma <= 65536.0) || !(w_coef >= 0.0 && w_coef <= 65536.0))
    return fail(NERF_HIP_ERR_ARG, "w_sigma=%g w_coef=%g: the weights lie in [0, 2^16]", w_sigma, w_coef);
  if (int rc = check_compact(slot, sigma_rows, coef_rows, n, 0, nx, ny, nz)) return rc;
  if (int rc = check_row_accumulators(acc_sigma_rows, acc_coef_rows, n)) return rc;
  if (n == 0 || (w_sigma == 0.0 && w_coef == 0.0)) return NERF_HIP_OK;
  if (int rc = check_out(point, "point", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolCompactTvArgs a;
  memset(&a, 0, sizeof(a));
  a.c = compact(slot, sigma_rows, coef_rows, n);
  a.point = point;
  a.nx = nx;
  a.ny = ny;
  a.nz = nz;
  a.ncoef = (degree + 1) * (degree + 1);
  a.w_sigma = w_sigma;
  a.w_coef = w_coef;
  a.eps = eps;
  a.acc_sigma_rows = reinterpret_cast<long long*>(acc_sigma_rows);
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  HIP_TRY(launch_volume_compact_tv_backward(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_compact_importance(const int32_t* slot, const float* sigma_rows, int64_t n, const uint8_t* occ, int nx, int ny, int nz,
                                       int block, const float* lo3, const float* step3, const float* origins, const float* dirs,
                                       const float* tmin, const float* tmax, int64_t N, float dt, float t_stop, int64_t* imp_rows,
                                       int32_t* steps, void* stream) {
  if (int rc = check_lattice(nx, ny, nz)) return rc;
  if (block < 1) return fail(NERF_HIP_ERR_ARG, "block=%d: a block has at least one cell per axis", block);
  if (int rc = check_count("N", N)) return rc;
  if (int rc = check_lo_step(lo3, step3)) return rc;
  if (!(dt > 0.0f && isfinite(dt))) return fail(NERF_HIP_ERR_ARG, "dt=%g: the step along the ray must be finite and > 0", (double)dt);
  if (!(t_stop >= 0.0f && t_stop < 1.0f)) return fail(NERF_HIP_ERR_ARG, "t_stop=%g: the transmittance to stop at lies in [0, 1)", (double)t_stop);
  if (int rc = check_rows(n, nx, ny, nz)) return rc;
  if (int rc = check_out(slot, "slot", 4)) return rc;
  if (n > 0) {
    if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
  }
  if (n > 0 || imp_rows) {
    if (int rc = check_out(imp_rows, "imp_rows", 8)) return rc;
  }
  if (int rc = check_out(occ, "occ", 1)) return rc;
  if (N == 0) return NERF_HIP_OK;
  if (int rc = check_out(origins, "origins", 4)) return rc;
  if (int rc = check_out(dirs, "dirs", 4)) return rc;
  if (int rc = check_out(tmin, "tmin", 4)) return rc;
  if (int rc = check_out(tmax, "tmax", 4)) return rc;
  if (int rc = check_out(steps, "steps", 4)) return rc;
  if (int rc = check_device()) return rc;
  VolImportanceArgs a;
  memset(&a, 0, sizeof(a));
  a.c = compact(slot, sigma_rows, nullptr, n);
  a.r.occ = occ;
  a.r.g = lattice(nx, ny, nz, lo3, step3);
  a.r.B = block;
  a.r.bx = blocks_of(nx, block);
  a.r.by = blocks_of(ny, block);
  a.r.bz = blocks_of(nz, block);
  a.r.origins = origins;
  a.r.dirs = dirs;
  a.r.tmin = tmin;
  a.r.tmax = tmax;
  a.r.N = N;
  a.r.dt = dt;
  a.r.t_stop = t_stop;
  a.r.steps = steps;
  a.imp_rows = reinterpret_cast<long long*>(imp_rows);
  HIP_TRY(launch_volume_compact_importance(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_assign(const float* rows, int64_t m, const float* codebook, int64_t K, int degree, int32_t* assign, float* dist,
                              void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("m", m)) return rc;
  if (int rc = check_codes(K)) return rc;
  if (dist && ((uintptr_t)dist & 3) != 0) return fail(NERF_HIP_ERR_ARG, "dist must be 4-byte aligned");
  if (m == 0) return NERF_HIP_OK;
  if (int rc = check_out(rows, "rows", 4)) return rc;
  if (int rc = check_out(codebook, "codebook", 4)) return rc;
  if (int rc = check_out(assign, "assign", 4)) return rc;
  if (int rc = check_device()) return rc;
  VqAssignArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = rows;
  a.m = m;
  a.codebook = codebook;
  a.K = K;
  a.assign = assign;
  a.dist = dist;
  HIP_TRY(launch_volume_vq_assign(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_accumulate(const float* rows, int64_t m, int degree, const int64_t* weight, int64_t imax, const int32_t* assign,
                                  int64_t K, int64_t* sum, int64_t* cnt, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("m", m)) return rc;
  if (int rc = check_codes(K)) return rc;
  if (imax < 0) return fail(NERF_HIP_ERR_ARG, "imax=%lld < 0", (long long)imax);
  if (weight && ((uintptr_t)weight & 7) != 0) return fail(NERF_HIP_ERR_ARG, "weight must be 8-byte aligned");
  if (int rc = check_out(sum, "sum", 8)) return rc;
  if (int rc = check_out(cnt, "cnt", 8)) return rc;
  if (m == 0) return NERF_HIP_OK;
  if (int rc = check_out(rows, "rows", 4)) return rc;
  if (int rc = check_out(assign, "assign", 4)) return rc;
  if (int rc = check_device()) return rc;
  VqAccumulateArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = rows;
  a.m = m;
  a.words = 3 * (degree + 1) * (degree + 1);
  a.weight = reinterpret_cast<const long long*>(weight);
  a.imax = imax;
  a.assign = assign;
  a.K = K;
  a.sum = reinterpret_cast<long long*>(sum);
  a.cnt = reinterpret_cast<long long*>(cnt);
  HIP_TRY(launch_volume_vq_accumulate(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_update(float* codebook, int64_t K, int degree, const int64_t* sum, const int64_t* cnt, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_codes(K)) return rc;
  if (int rc = check_out(codebook, "codebook", 4)) return rc;
  if (int rc = check_out(sum, "sum", 8)) return rc;
  if (int rc = check_out(cnt, "cnt", 8)) return rc;
  if (int rc = check_device()) return rc;
  VqUpdateArgs a;
  memset(&a, 0, sizeof(a));
  a.codebook = codebook;
  a.K = K;
  a.words = 3 * (degree + 1) * (degree + 1);
  a.sum = reinterpret_cast<const long long*>(sum);
  a.cnt = reinterpret_cast<const long long*>(cnt);
  HIP_TRY(launch_volume_vq_update(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_decode(const uint8_t* cls, const int32_t* rank, int64_t n, const uint16_t* code, int64_t n_coded, const void* kept,
                              int64_t n_kept, const void* codebook, int64_t K, int degree, void* coef_rows, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (n_coded < 0 || n_kept < 0 || n_coded + n_kept > n) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld n_kept=%lld: classes of the %lld rows", (long long)n_coded, (long long)n_kept, (long long)n);
  if (K < 0 || K > VQ_MAX_CODES) return fail(NERF_HIP_ERR_ARG, "K=%lld: 0 .. %d codes", (long long)K, VQ_MAX_CODES);
  if (n_coded > 0 && K == 0) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld rows and no codebook", (long long)n_coded);
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(cls, "cls", 1)) return rc;
  if (int rc = check_out(rank, "rank", 4)) return rc;
  if (int rc = check_out(coef_rows, "coef_rows", 8)) return rc;
  if (n_coded > 0) {
    if (int rc = check_out(code, "code", 2)) return rc;
    if (int rc = check_out(codebook, "codebook", 8)) return rc;
  }
  if (n_kept > 0) {
    if (int rc = check_out(kept, "kept", 8)) return rc;
  }
  if (int rc = check_device()) return rc;
  VqDecodeArgs a;
  memset(&a, 0, sizeof(a));
  a.cls = cls;
  a.rank = rank;
  a.n = n;
  a.code = code;
  a.n_coded = n_coded;
  a.kept = static_cast<const unsigned long long*>(kept);
  a.n_kept = n_kept;
  a.codebook = static_cast<const unsigned long long*>(codebook);
  a.K = n_coded > 0 ? K : 0;
  a.stride = vol_half_stride((degree + 1) * (degree + 1));
  a.out = static_cast<unsigned long long*>(coef_rows);
  HIP_TRY(launch_volume_vq_decode(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

static_assert(VQT_CHUNK == NERF_HIP_VOLUME_VQ_REDUCE_CHUNK, "the header states rule VQ-G's chunk");

int nerf_hip_volume_vq_expand(const uint8_t* cls, const int32_t* rank, int64_t n, const uint16_t* code, int64_t n_coded, const float* kept32,
                              int64_t n_kept, const float* codebook32, int64_t K, int degree, float* coef_rows, int64_t* acc_coef_rows,
                              void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (n_coded < 0 || n_kept < 0 || n_coded + n_kept > n) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld n_kept=%lld: classes of the %lld rows", (long long)n_coded, (long long)n_kept, (long long)n);
  if (K < 0 || K > VQ_MAX_CODES) return fail(NERF_HIP_ERR_ARG, "K=%lld: 0 .. %d codes", (long long)K, VQ_MAX_CODES);
  if (n_coded > 0 && K == 0) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld rows and no codebook", (long long)n_coded);
  if (acc_coef_rows && ((uintptr_t)acc_coef_rows & 7) != 0) return fail(NERF_HIP_ERR_ARG, "acc_coef_rows must be 8-byte aligned");
  if (n == 0) return NERF_HIP_OK;
  if (int rc = check_out(cls, "cls", 1)) return rc;
  if (int rc = check_out(rank, "rank", 4)) return rc;
  if (int rc = check_out(coef_rows, "coef_rows", 4)) return rc;
  if (n_coded > 0) {
    if (int rc = check_out(code, "code", 2)) return rc;
    if (int rc = check_out(codebook32, "codebook32", 4)) return rc;
  }
  if (n_kept > 0) {
    if (int rc = check_out(kept32, "kept32", 4)) return rc;
  }
  if (int rc = check_device()) return rc;
  VqExpandArgs a;
  memset(&a, 0, sizeof(a));
  a.cls = cls;
  a.rank = rank;
  a.n = n;
  a.code = code;
  a.n_coded = n_coded;
  a.kept32 = kept32;
  a.n_kept = n_kept;
  a.codebook32 = codebook32;
  a.K = n_coded > 0 ? K : 0;
  a.words = 3 * (degree + 1) * (degree + 1);
  a.out = coef_rows;
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  HIP_TRY(launch_volume_vq_expand(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_grad_reduce(int64_t* acc_coef_rows, int64_t n, int degree, const int32_t* offset, const int32_t* member,
                                   int64_t n_coded, int64_t K, int64_t* acc_code, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (n_coded < 0 || n_coded > n) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld: the coded rows of %lld rows", (long long)n_coded, (long long)n);
  if (K < 0 || K > VQ_MAX_CODES) return fail(NERF_HIP_ERR_ARG, "K=%lld: 0 .. %d codes", (long long)K, VQ_MAX_CODES);
  if (n_coded > 0 && K == 0) return fail(NERF_HIP_ERR_ARG, "n_coded=%lld rows and no codebook", (long long)n_coded);
  if (acc_coef_rows && ((uintptr_t)acc_coef_rows & 7) != 0) return fail(NERF_HIP_ERR_ARG, "acc_coef_rows must be 8-byte aligned");
  if (acc_code && ((uintptr_t)acc_code & 7) != 0) return fail(NERF_HIP_ERR_ARG, "acc_code must be 8-byte aligned");
  if (n_coded == 0) return NERF_HIP_OK;
  if (int rc = check_out(acc_coef_rows, "acc_coef_rows", 8)) return rc;
  if (int rc = check_out(acc_code, "acc_code", 8)) return rc;
  if (int rc = check_out(offset, "offset", 4)) return rc;
  if (int rc = check_out(member, "member", 4)) return rc;
  if (int rc = check_device()) return rc;
  VqReduceArgs a;
  memset(&a, 0, sizeof(a));
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  a.n = n;
  a.offset = offset;
  a.member = member;
  a.n_coded = n_coded;
  a.K = K;
  a.acc_code = reinterpret_cast<long long*>(acc_code);
  HIP_TRY(launch_volume_vq_grad_reduce(a, (degree + 1) * (degree + 1), static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

int nerf_hip_volume_vq_adam_step(float* sigma_rows, int64_t n, float* kept32, const int32_t* kept_row, int64_t n_kept, float* codebook32,
                                 int64_t K, int degree, int64_t* acc_sigma_rows, int64_t* acc_coef_rows, int64_t* acc_code, float* m,
                                 float* v, double grad_scale, int64_t step, double lr_sigma, double lr_coef, double beta1, double beta2,
                                 double eps, void* stream) {
  if (int rc = check_degree(degree)) return rc;
  if (int rc = check_count("n", n)) return rc;
  if (n_kept < 0 || n_kept > n) return fail(NERF_HIP_ERR_ARG, "n_kept=%lld: the kept rows of %lld rows", (long long)n_kept, (long long)n);
  if (K < 0 || K > VQ_MAX_CODES) return fail(NERF_HIP_ERR_ARG, "K=%lld: 0 .. %d codes", (long long)K, VQ_MAX_CODES);
  if (step < 1) return fail(NERF_HIP_ERR_ARG, "step=%lld: the first update is step 1", (long long)step);
  if (!isfinite(grad_scale)) return fail(NERF_HIP_ERR_ARG, "grad_scale=%g must be finite", grad_scale);
  if (!isfinite(lr_sigma) || !isfinite(lr_coef)) return fail(NERF_HIP_ERR_ARG, "lr_sigma=%g lr_coef=%g: the rates must be finite", lr_sigma, lr_coef);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(NERF_HIP_ERR_ARG, "beta1=%g beta2=%g: both lie in [0, 1)", beta1, beta2);
  if (!(eps >= 0.0 && isfinite(eps))) return fail(NERF_HIP_ERR_ARG, "eps=%g must be finite and >= 0", eps);
  if (n > 0 || acc_sigma_rows) {
    if (int rc = check_out(acc_sigma_rows, "acc_sigma_rows", 8)) return rc;
  }
  if (acc_coef_rows && ((uintptr_t)acc_coef_rows & 7) != 0) return fail(NERF_HIP_ERR_ARG, "acc_coef_rows must be 8-byte aligned");
  if (acc_code && ((uintptr_t)acc_code & 7) != 0) return fail(NERF_HIP_ERR_ARG, "acc_code must be 8-byte aligned");
  if (n == 0 && K == 0) return NERF_HIP_OK;
  if (n > 0) {
    if (int rc = check_out(sigma_rows, "sigma_rows", 4)) return rc;
  }
  if (n_kept > 0) {
    if (int rc = check_out(kept32, "kept32", 4)) return rc;
    if (int rc = check_out(kept_row, "kept_row", 4)) return rc;
    if (int rc = check_out(acc_coef_rows, "acc_coef_rows", 8)) return rc;
  }
  if (K > 0) {
    if (int rc = check_out(codebook32, "codebook32", 4)) return rc;
    if (int rc = check_out(acc_code, "acc_code", 8)) return rc;
  }
  if (int rc = check_out(m, "m", 4)) return rc;
  if (int rc = check_out(v, "v", 4)) return rc;
  if (int rc = check_device()) return rc;
  VqAdamArgs a;
  memset(&a, 0, sizeof(a));
  a.sigma_rows = sigma_rows;
  a.n = n;
  a.kept32 = kept32;
  a.kept_row = kept_row;
  a.n_kept = n_kept;
  a.codebook32 = codebook32;
  a.K = K;
  a.words = 3 * (degree + 1) * (degree + 1);
  a.acc_sigma_rows = reinterpret_cast<long long*>(acc_sigma_rows);
  a.acc_coef_rows = reinterpret_cast<long long*>(acc_coef_rows);
  a.acc_code = reinterpret_cast<long long*>(acc_code);
  a.m = m;
  a.v = v;
  a.grad_scale = grad_scale;
  a.lr_sigma = lr_sigma;
  a.lr_coef = lr_coef;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.c1 = 1.0 - pow_by_squaring(beta1, step);
  a.c2 = 1.0 - pow_by_squaring(beta2, step);
  HIP_TRY(launch_volume_vq_adam_step(a, static_cast<hipStream_t>(stream)));
  return NERF_HIP_OK;
}

}  // extern "C"
