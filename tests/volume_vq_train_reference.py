"""numpy restatements of rules VQ-X, VQ-G and VQ-V of include/nerf_hip.h (fine-tuning a vector-quantised volume with its assignments
frozen: the expansion of the masters to fp32 rows, the reduction of the rows' int64 accumulators to the codes', the Adam step over
sigma, the kept rows and the codebook), each in a vectorised and in a scalar-loops form, of volume.vq_members, and of one whole step
composed from the restated compact march and its gradient.  Shared by tests/test_volume_vq_train_cpu.py and
tests/test_gpu_volume_vq_train.py.  Built on volume_grad_reference (V: the march, VG's closed form, VU's bracket),
volume_compact_train_reference (T: the lookups and the gradient through the slots), volume_compact_reference (X) and
volume_vq_reference (Q: quantize).
"""
import numpy as np

import volume_compact_reference as X
import volume_compact_train_reference as T
import volume_grad_reference as V
import volume_vq_reference as Q

F = np.float32
SHIFT = V.SHIFT
CHUNK = 256               # NERF_HIP_VOLUME_VQ_REDUCE_CHUNK
MAX_RAYS = 2 ** 20


def rank_of(cls):
    """a row's rank among the rows of its class, in row order (0 for a pruned row)"""
    cls = np.asarray(cls)
    coded, kept = cls == 1, cls == 2
    return np.where(coded, np.cumsum(coded) - 1, np.where(kept, np.cumsum(kept) - 1, 0)).astype(np.int32)


def members(cls, code, K):
    """volume.vq_members: (offset [K + 1] int32, member [n_coded] int32), the members of a code in row order"""
    rows = np.flatnonzero(np.asarray(cls) == 1)
    c = np.asarray(code, np.int64)
    order = np.argsort(c, kind="stable")
    counts = np.bincount(c, minlength=K)[:K]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), rows[order].astype(np.int32)


def random_classes(rng, n, K, degree, bad=True):
    """random classes with all three present, codes in [0, K), fp32 masters; with ``bad`` a few rows that must not check out"""
    W = 3 * (degree + 1) ** 2
    cls = rng.choice(np.asarray([0, 1, 1, 1, 2], np.uint8), n)
    cls[:3] = (0, 1, 2)
    n_coded, n_kept = int((cls == 1).sum()), int((cls == 2).sum())
    code = rng.integers(0, K, n_coded).astype(np.uint16)
    rank = rank_of(cls)
    if bad:
        cls[5] = 7                                         # an unknown class
        coded, kept = np.flatnonzero(cls == 1), np.flatnonzero(cls == 2)
        rank[coded[1]], rank[coded[2]] = -1, n_coded       # ranks outside the class
        rank[kept[1]], rank[kept[2]] = n_kept, -5
        code[rank[coded[3]]] = K                           # a code >= K
    kept32 = rng.normal(0.0, 1.0, (n_kept, W)).astype(F)
    book32 = rng.normal(0.0, 1.0, (K, W)).astype(F)
    return cls, rank, code, kept32, book32


# ---- rule VQ-X ----

def expand(cls, rank, code, kept32, codebook32, acc_rows=None):
    """-> rows [n, W] fp32; with acc_rows [n, W] int64 the words of every row that receives +0 are zeroed IN PLACE"""
    cls, rank, code = np.asarray(cls), np.asarray(rank, np.int64), np.asarray(code, np.int64)
    W = codebook32.shape[1] if codebook32.size or not kept32.size else kept32.shape[1]
    n, n_coded, n_kept, K = cls.size, code.size, kept32.shape[0], codebook32.shape[0]
    out = np.zeros((n, W), F)
    ok1 = (cls == 1) & (rank >= 0) & (rank < n_coded)
    j = np.where(ok1, code[np.clip(rank, 0, max(n_coded - 1, 0))] if n_coded else 0, K)
    ok1 &= j < K
    if ok1.any():
        out[ok1] = codebook32[j[ok1]]
    ok2 = (cls == 2) & (rank >= 0) & (rank < n_kept)
    if ok2.any():
        out[ok2] = kept32[rank[ok2]]
    if acc_rows is not None:
        acc_rows[~(ok1 | ok2)] = 0
    return out


def expand_loops(cls, rank, code, kept32, codebook32, acc_rows=None):
    W = codebook32.shape[1] if codebook32.size or not kept32.size else kept32.shape[1]
    out = np.zeros((len(cls), W), F)
    for r in range(len(cls)):
        k, zero = int(rank[r]), True
        if cls[r] == 1:
            if 0 <= k < len(code) and int(code[k]) < codebook32.shape[0]:
                out[r], zero = codebook32[int(code[k])], False
        elif cls[r] == 2:
            if 0 <= k < kept32.shape[0]:
                out[r], zero = kept32[k], False
        if zero and acc_rows is not None:
            acc_rows[r] = 0
    return out


# ---- rule VQ-G ----

def _ranges(offset, n_coded, K):
    """the clamped [a_j, b_j) of every code"""
    off = np.asarray(offset, np.int64)
    a = np.clip(off[:K], 0, n_coded)
    b = np.minimum(np.maximum(off[1:K + 1], a), n_coded)
    return a, b


def reduce(acc_rows, offset, member, acc_code):
    """IN PLACE: acc_code [K, W] += the sums of the members' words of acc_rows [n, W] (int64), which are then zeroed; a member outside
    [0, n) is skipped"""
    n, K = acc_rows.shape[0], acc_code.shape[0]
    member = np.asarray(member, np.int64)
    a, b = _ranges(offset, member.size, K)
    pos = np.arange(member.size)
    for_code = np.full(member.size, -1, np.int64)
    for j in np.flatnonzero(b > a):                         # (ascending offsets: the ranges are disjoint)
        for_code[a[j]:b[j]] = j
    ok = (for_code >= 0) & (member >= 0) & (member < n)
    np.add.at(acc_code, for_code[ok], acc_rows[member[ok]])
    acc_rows[member[ok]] = 0
    return pos[ok]


def reduce_loops(acc_rows, offset, member, acc_code):
    """the same with Python integers -> the new acc_code as a list of lists of ints (acc_rows is zeroed in place)"""
    n, K, W = acc_rows.shape[0], acc_code.shape[0], acc_rows.shape[1]
    out = [[int(x) for x in row] for row in acc_code]
    a, b = _ranges(offset, len(member), K)
    for j in range(K):
        for i in range(int(a[j]), int(b[j])):
            r = int(member[i])
            if r < 0 or r >= n:
                continue
            for w in range(W):
                out[j][w] += int(acc_rows[r, w])
                acc_rows[r, w] = 0
    return out


# ---- rule VQ-V ----

def _bracket(x, acc, m, v, lr, grad_scale, c1, c2, beta1, beta2, eps):
    """rule VU's word bracket on arrays -> (m', v', x') fp32"""
    g = (np.asarray(acc, np.float64) * 2.0 ** -SHIFT) * float(grad_scale)
    with np.errstate(all="ignore"):
        m1 = (beta1 * m.astype(np.float64) + (1.0 - beta1) * g).astype(F)
        v1 = (beta2 * v.astype(np.float64) + (1.0 - beta2) * (g * g)).astype(F)
        x1 = (x.astype(np.float64) - lr * ((m1.astype(np.float64) / c1) / (np.sqrt(v1.astype(np.float64) / c2) + eps))).astype(F)
    return m1, v1, x1


def update(sigma_rows, kept32, kept_row, codebook32, acc_sigma, acc_rows, acc_code, m, v, grad_scale, step, lr_sigma, lr_coef, beta1=0.9,
           beta2=0.999, eps=1e-8, lr_codebook=None):
    """Rule VQ-V IN PLACE on sigma_rows [n], kept32 [n_kept, W], codebook32 [K, W] (fp32), the moments m, v [n + n_kept W + K W] and the
    int64 accumulators.  lr_codebook: None (the rule: lr_coef), or the rate a PLANTED MISTAKE gives the codebook."""
    n, W = sigma_rows.shape[0], acc_rows.shape[1]
    n_kept, K = kept32.shape[0], codebook32.shape[0]
    c1, c2 = 1.0 - V.pow_by_squaring(beta1, step), 1.0 - V.pow_by_squaring(beta2, step)
    kw = dict(grad_scale=grad_scale, c1=c1, c2=c2, beta1=beta1, beta2=beta2, eps=eps)
    # (a) sigma, frozen support
    live = sigma_rows > 0
    m1, v1, x1 = _bracket(sigma_rows, acc_sigma, m[:n], v[:n], float(lr_sigma), **kw)
    with np.errstate(all="ignore"):
        x1 = np.fmax(x1, F(0))
    m[:n], v[:n] = np.where(live, m1, m[:n]), np.where(live, v1, v[:n])
    sigma_rows[...] = np.where(live, x1, sigma_rows)
    acc_sigma[...] = 0
    # (b) the kept rows
    kr = np.asarray(kept_row, np.int64)
    ok = (kr >= 0) & (kr < n)
    mk, vk = m[n:n + n_kept * W].reshape(n_kept, W), v[n:n + n_kept * W].reshape(n_kept, W)
    if ok.any():
        m1, v1, x1 = _bracket(kept32[ok], acc_rows[kr[ok]], mk[ok], vk[ok], float(lr_coef), **kw)
        mk[ok], vk[ok], kept32[ok] = m1, v1, x1
        acc_rows[kr[ok]] = 0
    # (c) the codebook
    mc, vc = m[n + n_kept * W:].reshape(K, W), v[n + n_kept * W:].reshape(K, W)
    m1, v1, x1 = _bracket(codebook32, acc_code, mc, vc, float(lr_coef if lr_codebook is None else lr_codebook), **kw)
    mc[...], vc[...], codebook32[...] = m1, v1, x1
    acc_code[...] = 0


def update_loops(sigma_rows, kept32, kept_row, codebook32, acc_sigma, acc_rows, acc_code, m, v, grad_scale, step, lr_sigma, lr_coef,
                 beta1=0.9, beta2=0.999, eps=1e-8):
    """the same word by word, in the kernel's order of words"""
    n, W = sigma_rows.shape[0], acc_rows.shape[1]
    n_kept, K = kept32.shape[0], codebook32.shape[0]
    c1, c2 = 1.0 - V.pow_by_squaring(beta1, step), 1.0 - V.pow_by_squaring(beta2, step)
    kf, cf, af = kept32.reshape(-1), codebook32.reshape(-1), acc_code.reshape(-1)
    for i in range(n + (n_kept + K) * W):
        sigma = i < n
        if sigma:
            x, acc, lr = sigma_rows[i], int(acc_sigma[i]), float(lr_sigma)
            acc_sigma[i] = 0
            if not x > 0:
                continue
        elif i < n + n_kept * W:
            q = i - n
            r = int(kept_row[q // W])
            if r < 0 or r >= n:
                continue
            x, acc, lr = kf[q], int(acc_rows[r, q % W]), float(lr_coef)
            acc_rows[r, q % W] = 0
        else:
            q = i - n - n_kept * W
            x, acc, lr = cf[q], int(af[q]), float(lr_coef)
            af[q] = 0
        g = (np.float64(acc) * 2.0 ** -SHIFT) * np.float64(grad_scale)
        with np.errstate(all="ignore"):
            m1 = F(beta1 * np.float64(m[i]) + (1.0 - beta1) * g)
            v1 = F(beta2 * np.float64(v[i]) + (1.0 - beta2) * (g * g))
            x1 = F(np.float64(x) - lr * ((np.float64(m1) / c1) / (np.sqrt(np.float64(v1) / c2) + eps)))
        if sigma:
            x1 = np.fmax(x1, F(0))
            sigma_rows[i] = x1
        elif i < n + n_kept * W:
            kf[i - n] = x1
        else:
            cf[i - n - n_kept * W] = x1
        m[i], v[i] = m1, v1


# ---- the state of a tuner, and one whole step ----

class State:
    """volume.VQFinetuner in numpy: the frozen classes, the fp32 masters, the working compact volume, the accumulators, the moments"""

    def __init__(self, shape, index, sigma_rows, cls, code, kept16, codebook16, degree):
        W = 3 * (degree + 1) ** 2
        self.cls, self.code, self.rank = np.asarray(cls, np.uint8), np.asarray(code, np.uint16), rank_of(cls)
        self.kept32 = np.ascontiguousarray(kept16[:, :W].astype(F))
        self.codebook32 = np.ascontiguousarray(codebook16[:, :W].astype(F))
        n, K = len(cls), self.codebook32.shape[0]
        self.kept_row = np.flatnonzero(self.cls == 2).astype(np.int32)
        self.offset, self.member = members(self.cls, self.code, K)
        rows = expand(self.cls, self.rank, self.code, self.kept32, self.codebook32)
        self.c = X.Compact(X.slots(index, shape), np.asarray(sigma_rows, F).copy(), rows, degree)
        self.acc_sigma, self.acc_rows = np.zeros(n, np.int64), np.zeros((n, W), np.int64)
        self.acc_code = np.zeros((K, W), np.int64)
        self.m = np.zeros(n + (self.kept32.shape[0] + K) * W, F)
        self.v = np.zeros_like(self.m)
        self.steps = 0

    def apply(self, grad_scale, lr_sigma=0.1, lr_coef=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
        """reduce, update, expand on whatever the accumulators hold"""
        reduce(self.acc_rows, self.offset, self.member, self.acc_code)
        self.steps += 1
        update(self.c.sigma, self.kept32, self.kept_row, self.codebook32, self.acc_sigma, self.acc_rows, self.acc_code, self.m, self.v,
               grad_scale, self.steps, lr_sigma, lr_coef, beta1, beta2, eps)
        self.c.coef[...] = expand(self.cls, self.rank, self.code, self.kept32, self.codebook32, self.acc_rows)


# ---- the learning case both test files run ----

LEARN_K = 2
LEARN_STEPS = 30
LEARN_MARGIN = 0.6        # the last loss must be below LEARN_MARGIN x the first (tests/test_volume_vq_train_cpu.py chose it)


def learning_case():
    """volume_grad_reference.learning_case()'s teacher (lattice (9, 8, 7), 64 rays, the target its fp64 render); the student is the
    teacher's rows quantised at K = 2 with every row coded (unit importance, three k-means iterations, rule VQ's restatement)"""
    case = V.learning_case()
    index = case["index"]
    nc = case["coef"].shape[3]
    words = np.ascontiguousarray(case["coef"].reshape(-1, 3 * nc)[index])
    q = Q.quantize(case["sigma"].reshape(-1)[index], words, np.full(len(index), 1 << 20, np.int64), LEARN_K, 3)
    case.update(q=q, degree=2)
    return case


def state_of(case):
    q = case["q"]
    return State(V.LEARN_SHAPE, case["index"], q["sigma"], q["cls"], q["code"], q["kept"], q["codebook"], case["degree"])


def learn(case, steps=LEARN_STEPS, lr_sigma=0.1, lr_coef=0.01):
    """VQFinetuner.step in the restatement: fp32 lookups through the slots, the fp64 composite, VCG's closed form (each word's SUM
    rounded to the fixed point once), VQ-G, VQ-V, VQ-X -> (the losses [steps + 1], the last one after the final update; the State)"""
    st = state_of(case)
    G, bg = case["G"], V.LEARN_BG
    n = st.c.sigma.shape[0]
    target = case["target"].astype(np.float64)
    losses = []
    for it in range(steps + 1):
        sig, raw = T.lookup32(st.c, G)
        col, mask = V.clamp_mask(raw)
        idx = V.pad(G, sig)
        _, w, Tn, valid = V.forward(G, sig, idx, np.float64, 0.0)
        rgb = V.composite(G, idx, valid, w, col, bg)[0].astype(F).astype(np.float64)
        diff = rgb - target
        losses.append(float((diff * diff).mean()))
        if it == steps:
            break
        dS, dC = T.vcg(st.c, G, idx, valid, w, Tn, col, mask, (2.0 * diff).astype(F), None, bg)
        st.acc_sigma += np.rint(dS * 2.0 ** SHIFT).astype(np.int64)
        st.acc_rows += np.rint(dC.reshape(n, -1) * 2.0 ** SHIFT).astype(np.int64)
        st.apply(1.0 / (3 * G.N), lr_sigma, lr_coef)
    return np.asarray(losses), st
