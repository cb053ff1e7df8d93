"""Plain-torch references of the per-ray stages between the MLP and the loss (ray_parts.h, ray_parts_bwd.h), for tests/test_gpu_ray_stages.py
and tests/test_ray_stages_cpu.py.  Everything runs on the CPU in the dtype of its operands: float64 is the reference, the SAME graph in float32
is the yardstick (`e32`: how far plain fp32 arithmetic is from fp64 on these operands), and autograd gives the backward.

  coarse_stage       sigma -> w, cdf, C_c, D_c, A_c and the inverse-CDF resampled t_f, given each fine sample's bin k (a discrete decision)
  decision_replica   the kernel's fp32 arithmetic for cdf, lo, hi, step, u, k from a given fp32 w_c, and which samples are AMBIGUOUS: u within
                     4 fp32 ulps of a cdf entry, where another rounding of the same formula may pick another bin
  merged_composite   w, C_f, D_f, A_f over a SORTED bundle; merged_grads un-sorts its autograd gradients through the permutations
  stable_order       the order the training sort must produce: torch.sort(stable=True) with -0 == +0 and every NaN last
  operands / CASES   the seeded operands of every (Nc, Nf) the two test files use

Only the oracle's formulas are imported (composite, coarse_depths; `weights` restates weights_from_sigma with one extra knob): the reference is
pinned to what the suite already trusts by tests/test_ray_stages_cpu.py.
"""
import torch

from nerf_oracle import EPSILON, coarse_depths, composite

B_RAYS = 6                                  # the last k_coarse / k_coarse_bwd workgroup (4 rays) has two waves behind the batch
DEPTHS = (0.1, 0.1, 3.0, 3.0, 50.0, 50.0)   # total optical depth per ray: thin, ordinary, opaque (transmittance underflows mid-ray)
LAST = 1e-4
AMBIGUOUS_ULPS = 4
AMBIGUOUS_MAX = 0.01                        # at most 1 % of a case's fine samples
EXP_ULP = 2.0 ** -24                        # one fp32 ulp just below 1, where exp(-s) of a thin sample lies

# (Nc, Nf) -> seed: the first seed from 0 up whose operands meet the 1 % condition on the replica's own fp32 weights (and, at (5, 3), raise
# the Q7 condition).  With 6 or 18 fine samples the condition allows no ambiguous sample at all, and at (2, 1) an opaque ray whose first
# sigma is not an exact zero, or any ray whose second one is, has lo == hi and u on a cdf entry: seed 148 is the first without such a ray.
CASES = {
    (2, 1): 148,
    (5, 3): 0,
    (31, 65): 0,
    (65, 63): 0,
    (64, 65): 0,
    (64, 128): 0,
    (128, 128): 0,
    (130, 200): 0,
    (1024, 1024): 0,
}


def operands(Nc, Nf, seed=None, B=B_RAYS):
    """float32 operands of one case: every ray its own near / far with t_c its linspace, rgb a sigmoid of normals, sigma = relu(normal) * scale
    (about half exact zeros, as a ReLU head gives) with the per-ray scale that puts the ray's total optical depth at DEPTHS; fine-sample
    sigma / rgb of the same make for the merge stage; random upstream gradients."""
    gen = torch.Generator().manual_seed(CASES[(Nc, Nf)] if seed is None else seed)
    near = 2.0 + torch.rand(B, generator=gen)
    far = near + 3.0 + 2.0 * torch.rand(B, generator=gen)
    t_c = coarse_depths(near, far, Nc)
    delta_c = (far - near) / Nc
    raw = torch.relu(torch.randn(B, Nc, generator=gen))
    depth = torch.tensor([DEPTHS[b % len(DEPTHS)] for b in range(B)])
    scale = depth / (raw.sum(1) * delta_c).clamp_min(1e-3)
    o = dict(Nc=Nc, Nf=Nf, near=near, far=far, t_c=t_c, delta0=float(t_c[0, 1] - t_c[0, 0]))
    o["sig_c"] = raw * scale[:, None]
    o["rgb_c"] = torch.sigmoid(torch.randn(B, Nc, 3, generator=gen))
    o["sig_f"] = torch.relu(torch.randn(B, Nf, generator=gen)) * scale[:, None]
    o["rgb_f"] = torch.sigmoid(torch.randn(B, Nf, 3, generator=gen))
    o["dC_c"] = torch.randn(B, 3, generator=gen)
    o["dC_f"] = torch.randn(B, 3, generator=gen)
    o["dt_f"] = torch.randn(B, Nf, generator=gen)
    o["dmaps"] = torch.randn(B, 4, generator=gen)
    return o


def tie_operands(Nc=65, Nf=63, B=B_RAYS, seed=0):
    """merge-stage operands with exact duplicate depths and a few duplicate sigma / rgb levels
    (as test_exact_ties_in_the_sorted_channels_do_not_change_the_forward builds them)"""
    gen = torch.Generator().manual_seed(seed)
    t_c = torch.sort(torch.rand(B, Nc, generator=gen) * 4 + 2, dim=1).values
    t_f = t_c[:, torch.randint(0, Nc, (Nf,), generator=gen)].clone()
    t_f[:, ::3] += 0.01
    o = dict(Nc=Nc, Nf=Nf, t_c=t_c, t_f=t_f)
    o["sig_c"] = torch.randint(0, 4, (B, Nc), generator=gen).float() * 0.5
    o["sig_f"] = torch.randint(0, 4, (B, Nf), generator=gen).float() * 0.5
    o["rgb_c"] = torch.randint(0, 3, (B, Nc, 3), generator=gen).float() * 0.25 + 0.25
    o["rgb_f"] = torch.randint(0, 3, (B, Nf, 3), generator=gen).float() * 0.25 + 0.25
    o["dC_f"] = torch.randn(B, 3, generator=gen)
    o["dmaps"] = torch.randn(B, 4, generator=gen)
    return o


def weights(delta, sigma, exp_low=0.0):
    """the oracle's weights_from_sigma (nerf.py:263-272; with exp_low = 0 the same operations, bit for bit: x - 0.0 is x): s = sigma delta,
    T_i = exp(-sum_{j<=i} s_j), w = T (1 - exp(-s)).  exp_low (a number, or [B,1]: one per ray): every exp(-s) of a sample with s != 0 comes out
    exp_low * EXP_ULP LOW -- the model of an expf whose rounding error does not average to zero.  1 - exp(-s) turns it into a same-sign error of
    every weight, which a sum over N samples adds up N-fold where unbiased rounding adds up sqrt(N)-fold.  exp(0) = 1 is
    exact on every device: samples with s == 0 keep their exact zero weight."""
    s = delta * sigma
    low = torch.where(s != 0, torch.as_tensor(exp_low * EXP_ULP, dtype=s.dtype).expand_as(s), torch.zeros_like(s))
    return torch.exp(-torch.cumsum(s, dim=1)) * (1 - (torch.exp(-s) - low))


def exp_low_of(exp_got, s32):
    """how low an implementation's exp(-s) comes out on the fp32 arguments s32 [B,N], per ray: the mean over the samples with s != 0 of its
    signed ABSOLUTE error against float64 (what reaches the weight), in units of EXP_ULP; positive = low -> [B,1], what `weights` takes as
    exp_low.  An expf within 1 ulp of the true value keeps it inside [-1, 1]: results are below 1, where an ulp is at most EXP_ULP."""
    ref = torch.exp(-s32.double())
    nz = s32 != 0
    err = torch.where(nz, ref - exp_got.double(), torch.zeros_like(ref))
    return (err.sum(1) / nz.sum(1).clamp_min(1) / EXP_ULP)[:, None]


# ---------------------------------------------------------------------------------------------------------------
# coarse stage
# ---------------------------------------------------------------------------------------------------------------
def coarse_stage(sigma_c, rgb_c, t_c, near, far, delta0, Nf, k, exp_low=0.0):
    """nerf.py:263-281 and 225-261 in the dtype of sigma_c; k [B,Nf] (long, inside [0, Nc-1]) is each fine sample's bin.  lo, hi and u carry no
    gradient (the reference builds u on the host); a sample in the last bin has slope 0."""
    dt = sigma_c.dtype
    B, Nc = sigma_c.shape
    near, far, t_c = near.to(dt), far.to(dt), t_c.to(dt)
    delta_c = ((far - near) / Nc)[:, None].expand(-1, Nc)
    w = weights(delta_c, sigma_c, exp_low)
    cdf = torch.cumsum(w, dim=1)
    lo, hi = cdf.min(dim=1).values.detach(), cdf.max(dim=1).values.detach()
    step = (hi - lo) / (Nf + 1)
    j = torch.arange(1, Nf + 1, dtype=dt)
    u = j[None, :] * step[:, None] + lo[:, None]
    slope = torch.cat((torch.as_tensor(delta0, dtype=dt) / (w[:, 1:] + EPSILON), torch.zeros(B, 1, dtype=dt)), dim=1)
    t_f = torch.gather(t_c, 1, k) + (u - torch.gather(cdf, 1, k)) * torch.gather(slope, 1, k)
    return dict(w=w, cdf=cdf, C_c=composite(w, rgb_c.to(dt)), D_c=(w * t_c).sum(1), A_c=w.sum(1), t_f=t_f)


def coarse_grads(o, k, dtype, dt_f, dmaps=None, exp_low=0.0):
    """autograd of sum(C_c dC_c) + sum(t_f dt_f) [+ sum(D_c dmaps[:,0] + A_c dmaps[:,1])] in `dtype` -> d sigma_c, d rgb_c"""
    sig = o["sig_c"].detach().to(dtype).clone().requires_grad_(True)
    rgb = o["rgb_c"].detach().to(dtype).clone().requires_grad_(True)
    s = coarse_stage(sig, rgb, o["t_c"], o["near"], o["far"], o["delta0"], o["Nf"], k, exp_low)
    loss = (s["C_c"] * o["dC_c"].to(dtype)).sum() + (s["t_f"] * dt_f.to(dtype)).sum()
    if dmaps is not None:
        loss = loss + (s["D_c"] * dmaps[:, 0].to(dtype)).sum() + (s["A_c"] * dmaps[:, 1].to(dtype)).sum()
    loss.backward()
    return sig.grad, rgb.grad


def decision_replica(w_c, Nf):
    """The kernel's decisions from ITS OWN fp32 weights w_c [B,Nc] (coarse_ray_weights / coarse_ray_resample): cdf_i = float(double prefix sum),
    lo / hi = min / max, step = (hi - lo) / float(Nf + 1), u_j = float(float((j + 1) * step) + lo) -- no fused multiply-add --, k = (number of
    cdf entries < u) - 1.  -> dict(k clamped to [0, Nc-1], bad = the condition of nerf.py:251 on the unclamped k, ambiguous, cdf, u)."""
    assert w_c.dtype == torch.float32
    Nc = w_c.shape[1]
    cdf = torch.cumsum(w_c.double(), dim=1).float()
    lo, hi = cdf.min(dim=1).values, cdf.max(dim=1).values
    step = (hi - lo) / torch.tensor(float(Nf + 1), dtype=torch.float32)
    prod = torch.arange(1, Nf + 1, dtype=torch.float32)[None, :] * step[:, None]   # rounded to fp32 here ...
    u = prod + lo[:, None]                                                         # ... and here
    k_raw = torch.searchsorted(cdf.contiguous(), u.contiguous()) - 1
    bad = (k_raw > Nf - 1) | (k_raw < 0)
    ulp = lambda x: torch.nextafter(x.abs(), torch.full_like(x, float("inf"))) - x.abs()
    gap = (u[:, :, None] - cdf[:, None, :]).abs()
    tol = AMBIGUOUS_ULPS * torch.maximum(ulp(u)[:, :, None], ulp(cdf)[:, None, :])
    return dict(k=k_raw.clamp(0, Nc - 1), bad=bad, ambiguous=(gap <= tol).any(dim=2), cdf=cdf, u=u)


# ---------------------------------------------------------------------------------------------------------------
# merged composite over a sorted bundle
# ---------------------------------------------------------------------------------------------------------------
def merged_composite(t_s, rgb_s, sig_s, last=LAST, exp_low=0.0):
    """nerf.py:309-321 over SORTED channels, in their dtype: delta_i = t_{i+1} - t_i with the last = `last` -> w, C_f, D_f, A_f"""
    delta = torch.cat((t_s[:, 1:] - t_s[:, :-1], torch.full((t_s.shape[0], 1), last, dtype=t_s.dtype)), dim=1)
    w = weights(delta, sig_s, exp_low)
    return dict(w=w, C_f=composite(w, rgb_s), D_f=(w * t_s).sum(1), A_f=w.sum(1))


def merged_grads(bundle, perm, Nc, dC_f, dtype, dmaps=None, last=LAST, exp_low=0.0):
    """autograd of sum(C_f dC_f) [+ sum(D_f dmaps[:,2] + A_f dmaps[:,3])] over bundle [B,N,5] in `dtype`, un-sorted through perm [B,5,N] (sorted
    position -> original slot): channel 4 is sigma, 1..3 rgb, 0 the depth, whose gradient only the fine slots (>= Nc) receive
    -> dsig_c, dsig_f, drgb_c, drgb_f, dt_f"""
    b = bundle.to(dtype)
    B, N, _ = b.shape
    t_s = b[:, :, 0].clone().requires_grad_(True)
    rgb_s = b[:, :, 1:4].clone().requires_grad_(True)
    sig_s = b[:, :, 4].clone().requires_grad_(True)
    m = merged_composite(t_s, rgb_s, sig_s, last, exp_low)
    loss = (m["C_f"] * dC_f.to(dtype)).sum()
    if dmaps is not None:
        loss = loss + (m["D_f"] * dmaps[:, 2].to(dtype)).sum() + (m["A_f"] * dmaps[:, 3].to(dtype)).sum()
    loss.backward()
    perm = perm.long()
    unsort = lambda g, c: torch.zeros(B, N, dtype=dtype).scatter_(1, perm[:, c], g)
    dsig = unsort(sig_s.grad, 4)
    drgb = torch.stack([unsort(rgb_s.grad[:, :, c], 1 + c) for c in range(3)], dim=2)
    dt = unsort(t_s.grad, 0)
    return dsig[:, :Nc], dsig[:, Nc:], drgb[:, :Nc], drgb[:, Nc:], dt[:, Nc:]


def stable_order(x):
    """indices of a stable ascending sort of x [.., N] along its last dimension in torch.sort's order: -0 and +0 are equal, every NaN (of
    either sign) is last, equal elements keep their original order"""
    x = torch.where(x == 0, torch.zeros_like(x), x)          # both zeros -> +0
    x = torch.where(torch.isnan(x), torch.full_like(x, float("nan")), x)  # one NaN
    return torch.sort(x, dim=-1, stable=True).indices


def l2_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
