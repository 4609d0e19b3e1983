"""fp64 / integer references of the element-wise and reduction kernels (csrc/mtl_elem.hip), written out from the formulas in
include/mtl_hip.h.  Pure numpy / torch on the CPU; tests/test_elem_ref.py checks them against torch and a plain Python loop, and
tests/test_elem_edges_gpu.py checks the kernels against them."""
import numpy as np
import torch
import torch.nn.functional as F

AMAX_SLOTS, AMAX_STRIDE = 64, 32            # MTL_AMAX_SLOTS / MTL_AMAX_STRIDE: 64 slot heads, 32 floats (one 128-byte line) apart


def f32(v):
    """the fp32 value a C `float` argument takes, as a Python float"""
    return float(np.float32(v))


def slot_bound(amax):
    """max over the slot heads of one bound (a (2048,) float32 array / tensor): what the h2 kernels read"""
    a = np.asarray(amax, dtype=np.float32).reshape(-1)
    return np.float32(a[:AMAX_SLOTS * AMAX_STRIDE:AMAX_STRIDE].max())


def h2_scale(bound):
    """pow2_scale of csrc/mtl_h2.h: s = 2^(141 - e), e the biased exponent of the bound (so that bound * s lies in [2^14, 2^15)),
    exponent clamped to +-60; s = 1 for a zero / subnormal bound.  Returned as a Python float (exact: a power of two)."""
    e = (int(np.float32(bound).view(np.uint32)) >> 23) & 0xff
    k = 0 if e == 0 else min(max(141 - e, -60), 60)
    return 2.0 ** k


def h2_census(x, bound):
    """(non-zero elements, those with |x| s < 2^-3, those with |x| s < 2^-9) of the fp32 array x against `bound`, s = h2_scale(bound).
    The products are exact in fp64 (s is a power of two, fp32 subnormals times 2^60 stay far inside the fp64 range)."""
    a = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1)) * h2_scale(bound)
    nz = a > 0
    return int(nz.sum()), int((nz & (a < 2.0 ** -3)).sum()), int((nz & (a < 2.0 ** -9)).sum())


def softmax_limits(B, H, Tq, Tk, klen, causal):
    """(B, H, Tq) number of live keys per row: min(klen[b], Tk) (Tk without klen), and at most q + 1 when causal"""
    lim = torch.full((B, H, Tq), Tk, dtype=torch.int64)
    if klen is not None:
        lim = torch.minimum(lim, torch.as_tensor(klen, dtype=torch.int64).view(B, 1, 1).expand(B, H, Tq))
    if causal:
        lim = torch.minimum(lim, (torch.arange(Tq) + 1).view(1, 1, Tq).expand(B, H, Tq))
    return lim


def softmax_fwd(s, scale, lim, dtype=torch.float64):
    """P = softmax(s * scale) over the first lim keys of every row, exactly 0 behind them; a row without a live key is all zero
    (the kernel's pinned behaviour: torch.softmax of an all -inf row gives NaN).  s: (..., Tk), lim: (...)"""
    s = s.to(dtype) * scale
    live = torch.arange(s.shape[-1]) < lim.unsqueeze(-1)
    z = s.masked_fill(~live, -np.inf)
    mx = z.max(-1, keepdim=True)[0]
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.where(live, torch.exp(z - mx), torch.zeros_like(z))
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))


def softmax_bwd(P, dP, scale, keep=None, pscale=1.0, dtype=torch.float64):
    """dS = P (dP' - sum_k dP' P) scale with dP' = dP * keep * pscale (the gradient through the dropout on the probabilities)"""
    P, dP = P.to(dtype), dP.to(dtype)
    if keep is not None:
        dP = torch.where(keep != 0, dP * pscale, torch.zeros_like(dP))
    return P * (dP - (P * dP).sum(-1, keepdim=True)) * scale


def layernorm(x, res, gamma, beta, pe, keep, xmask, xscale, T, eps, rpg, dy=None, dtype=torch.float64, builtin=False):
    """y = (LayerNorm(z) gamma[g] + beta[g] (+ pe[row % T])) * keep[row], z = x * xmask * xscale (+ res), g = row // rpg; biased
    variance, eps inside the square root.  gamma / beta: (groups, d).  With dy also the gradients, by autograd in `dtype`:
    dz (of z: the residual branch), dx (of x: the dropped branch), dgamma / dbeta (groups, d), dsum = per-group column sums of dx.
    builtin=True normalises with F.layer_norm (the plain torch op) instead of the written-out formula."""
    c = lambda t: None if t is None else t.detach().to(dtype)
    x, res, pe = c(x).requires_grad_(True), c(res), c(pe)
    gamma, beta = c(gamma).requires_grad_(True), c(beta).requires_grad_(True)
    rows, d = x.shape
    z = x if xmask is None else torch.where(xmask != 0, x * xscale, torch.zeros_like(x))
    if res is not None:
        z = z + res
    z.retain_grad()
    grp = torch.arange(rows) // rpg
    if builtin:
        xhat, rstd = F.layer_norm(z, (d,), None, None, eps), None
    else:
        mean = z.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + eps)
        xhat = (z - mean) * rstd
    y = xhat * gamma[grp] + beta[grp]
    if pe is not None:
        y = y + pe[torch.arange(rows) % T]
    if keep is not None:
        y = y * keep.to(dtype).unsqueeze(1)
    out = dict(y=y.detach(), xhat=xhat.detach(), rstd=None if rstd is None else rstd.detach().squeeze(1))
    if dy is not None:
        y.backward(dy.to(dtype))
        groups = gamma.shape[0]
        dsum = torch.zeros(groups, d, dtype=dtype).index_add_(0, grp, x.grad)
        out.update(dz=z.grad if z is not x else x.grad, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dsum=dsum)
    return out


def cross_entropy(logits, gold, pad_id, smoothing, rowscale=None, dtype=torch.float64):
    """lse, per-row loss (0 on pad rows) and d(sum_r rowscale[r] loss[r]) / d logits of the label-smoothing formula restated in
    tests/test_trainer_gpu.py: target = (1 - eps) on gold, eps / V elsewhere (it sums to 1 - eps / V); plain NLL for eps = 0."""
    x = logits.detach().to(dtype).requires_grad_(True)
    V = x.shape[1]
    logp = F.log_softmax(x, dim=1)
    mask = gold.ne(pad_id)
    one_hot = torch.zeros_like(x).scatter(1, (mask.long() * gold).view(-1, 1), 1)
    if smoothing > 0:
        one_hot = one_hot * (1 - smoothing) + (1 - one_hot) * smoothing / V
    loss = -(one_hot * logp).sum(1) * mask.to(dtype)
    grad = None
    if rowscale is not None:
        (loss * rowscale.to(dtype)).sum().backward()
        grad = x.grad
    return torch.logsumexp(x.detach(), 1), loss.detach(), grad


def adam(theta, g, m, v, step, lr, b1, b2, eps):
    """one torch.optim.Adam step (defaults: no amsgrad, no weight decay) in fp64 from the fp32 values the kernel is given:
    m' = m b1 + (1 - b1) g ; v' = v b2 + (1 - b2) g^2 ; theta' = theta - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)"""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    theta, g, m, v = (t.double() for t in (theta, g, m, v))
    m1 = m * b1 + (1 - b1) * g
    v1 = v * b2 + (1 - b2) * g * g
    denom = torch.sqrt(v1) / np.sqrt(1 - b2 ** step) + eps
    u = lr / (1 - b1 ** step) * (m1 / denom)
    return theta - u, m1, v1, u, denom


def embed_chains(ids, rpg):
    """first / next of mtl_embed_bwd: next[r] = the next row of r's group with the same id (-1: none), first[r] = 1 on chain heads"""
    n = len(ids)
    first, nxt = [0] * n, [-1] * n
    for g0 in range(0, n, rpg):
        seen = {}
        for r in range(g0, min(g0 + rpg, n)):
            i = int(ids[r])
            if i in seen:
                nxt[seen[i]] = r
            else:
                first[r] = 1
            seen[i] = r
    return torch.tensor(first, dtype=torch.int32), torch.tensor(nxt, dtype=torch.int32)


def philox_shift_ok(a, b):
    """mask b drawn at counter offset + 1 is mask a (offset) shifted by one counter = 4 elements"""
    return torch.equal(a[4:], b[:a.numel() - 4])
