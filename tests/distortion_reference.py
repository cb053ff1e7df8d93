"""Plain-torch restatement of rule DL (include/nerf_hip.h): the distortion loss of one pass of each ray, for tests/test_distortion_cpu.py and
tests/test_gpu_distortion.py.  Built on tests/ray_stage_reference.py (weights, merged_composite, coarse_stage, CASES, operands, tie_operands);
everything runs on the CPU in the dtype of its operands, float64 being the reference.

  midpoints          m_i, d_i of rule DL from the pass's depths
  distortion         the prefix form via cumsum: differentiable, and the form that fixes the sign at ties by index
  distortion_pairs   the O(N^2) definition  r (sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i)
  closed_form_grads  dL/dw and dL/dt as rule DL writes them out (what the backward kernels add)
  merged_grads / coarse_grads   R.merged_grads / R.coarse_grads whose loss also holds sum(L ddist)
"""
import torch

import ray_stage_reference as R


def midpoints(t):
    """t [B,N] -> m, d [B,N]: m_i = (t_i + t_{i+1}) / 2, d_i = t_{i+1} - t_i for i < N-1; m_{N-1} = t_{N-1}, d_{N-1} = 0"""
    m = torch.cat(((t[:, :-1] + t[:, 1:]) / 2, t[:, -1:]), dim=1)
    d = torch.cat((t[:, 1:] - t[:, :-1], torch.zeros_like(t[:, -1:])), dim=1)
    return m, d


def _exclusive(x):
    return torch.cat((torch.zeros_like(x[:, :1]), torch.cumsum(x, dim=1)[:, :-1]), dim=1)


def distortion(t, w, near, far):
    """rule DL's prefix form in the dtype of w -> L [B]"""
    dt = w.dtype
    t, near, far = t.to(dt), near.to(dt), far.to(dt)
    m, d = midpoints(t)
    r = 1 / (far - near)
    P = m * _exclusive(w) - _exclusive(w * m)
    return r * (2 * (w * P).sum(1) + (w * w * d).sum(1) / 3)


def distortion_pairs(t, w, near, far):
    """the O(N^2) definition in the dtype of w -> L [B]"""
    dt = w.dtype
    t, near, far = t.to(dt), near.to(dt), far.to(dt)
    m, d = midpoints(t)
    r = 1 / (far - near)
    pairs = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    return r * (pairs + (w * w * d).sum(1) / 3)


def closed_form_grads(t, w, near, far):
    """rule DL's written-out gradients in the dtype of w -> dL/dw [B,N], dL/dt [B,N]"""
    dt = w.dtype
    t, near, far = t.to(dt), near.to(dt), far.to(dt)
    m, d = midpoints(t)
    r = (1 / (far - near))[:, None]
    We, Se = _exclusive(w), _exclusive(w * m)
    W, S = w.sum(1, keepdim=True), (w * m).sum(1, keepdim=True)
    P = m * We - Se
    Rr = (S - Se - w * m) - m * (W - We - w)
    dw = r * (2 * (P + Rr) + 2 * w * d / 3)
    a = 2 * w * (We - (W - We - w))
    q = w * w / 3
    own = torch.cat((a[:, :-1] / 2 - q[:, :-1], a[:, -1:]), dim=1)                       # k < N-1 ? a_k / 2 - w_k^2 / 3 : a_k
    prev = torch.cat((torch.zeros_like(a[:, :1]), a[:, :-1] / 2 + q[:, :-1]), dim=1)     # k >= 1 ? a_{k-1} / 2 + w_{k-1}^2 / 3 : 0
    return dw, r * (own + prev)


def merged_grads(bundle, perm, Nc, dC_f, dtype, near, far, ddist, dmaps=None, last=R.LAST, exp_low=0.0):
    """R.merged_grads with sum(L_f ddist[:,1]) in the loss (L_f: the sorted depth channel with the composite's weights)
    -> dsig_c, dsig_f, drgb_c, drgb_f, dt_f"""
    b = bundle.to(dtype)
    B, N, _ = b.shape
    t_s = b[:, :, 0].clone().requires_grad_(True)
    rgb_s = b[:, :, 1:4].clone().requires_grad_(True)
    sig_s = b[:, :, 4].clone().requires_grad_(True)
    m = R.merged_composite(t_s, rgb_s, sig_s, last, exp_low)
    loss = (m["C_f"] * dC_f.to(dtype)).sum() + (distortion(t_s, m["w"], near, far) * ddist[:, 1].to(dtype)).sum()
    if dmaps is not None:
        loss = loss + (m["D_f"] * dmaps[:, 2].to(dtype)).sum() + (m["A_f"] * dmaps[:, 3].to(dtype)).sum()
    loss.backward()
    perm = perm.long()
    unsort = lambda g, c: torch.zeros(B, N, dtype=dtype).scatter_(1, perm[:, c], g)
    dsig = unsort(sig_s.grad, 4)
    drgb = torch.stack([unsort(rgb_s.grad[:, :, c], 1 + c) for c in range(3)], dim=2)
    dt = unsort(t_s.grad, 0)
    return dsig[:, :Nc], dsig[:, Nc:], drgb[:, :Nc], drgb[:, Nc:], dt[:, Nc:]


def coarse_grads(o, k, dtype, dt_f, ddist, dmaps=None, exp_low=0.0):
    """R.coarse_grads with sum(L_c ddist[:,0]) in the loss (t_c carries no gradient) -> d sigma_c, d rgb_c"""
    sig = o["sig_c"].detach().to(dtype).clone().requires_grad_(True)
    rgb = o["rgb_c"].detach().to(dtype).clone().requires_grad_(True)
    s = R.coarse_stage(sig, rgb, o["t_c"], o["near"], o["far"], o["delta0"], o["Nf"], k, exp_low)
    loss = (s["C_c"] * o["dC_c"].to(dtype)).sum() + (s["t_f"] * dt_f.to(dtype)).sum()
    loss = loss + (distortion(o["t_c"], s["w"], o["near"], o["far"]) * ddist[:, 0].to(dtype)).sum()
    if dmaps is not None:
        loss = loss + (s["D_c"] * dmaps[:, 0].to(dtype)).sum() + (s["A_c"] * dmaps[:, 1].to(dtype)).sum()
    loss.backward()
    return sig.grad, rgb.grad
