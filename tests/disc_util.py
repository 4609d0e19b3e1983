"""Accent-discriminator test helpers: an fp64 torch-CPU restatement of the formulas of include/mtl_hip.h "accent discriminator"
(written from the specification, not from the kernels), the fp32 error bounds the GPU tests assert, and loaders of tests/golden/D0.npz
(tools/make_golden_discriminator.py: the real reference's three discriminator modes on the F0 fixture)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('multitask', 'adversarial', 'adversarial_decay')
U = 2.0 ** -24                      # unit round-off of fp32


def mode_flags(mode):
    return dict(multitask=mode == 'multitask', adversarial=mode != 'multitask', beta_decay=mode == 'adversarial_decay')


# ---------------------------------------------------------------------------------------------------------------------
# restatement (fp64)
# ---------------------------------------------------------------------------------------------------------------------
def pool(enc):
    """enc (B, T, d) -> pooled (B, d): the sum over all T rows"""
    return enc.double().sum(dim=1)


def head(pooled, W, bias, accent_id, mode):
    """pooled (B, d), W (C, d), bias (C) -> logits (B, C), CE mean over B, MSE to 1/C as a mean over B C (None in mode 0)"""
    pooled, W, bias = pooled.double(), W.double(), bias.double()
    logits = pooled @ W.t() + bias
    B, C = logits.shape
    lse = torch.logsumexp(logits, dim=1)
    ce = (lse - logits[:, accent_id]).sum() / B
    mse = ((logits - 1.0 / C) ** 2).sum() / (B * C) if mode == 1 else None
    return logits, ce, mse


def dlogit(logits, accent_id, mode, a, b):
    """a (softmax - onehot) / B + b 2 (logit - 1/C) / (B C); the b term counts in mode 1 only"""
    logits = logits.double()
    B, C = logits.shape
    onehot = torch.zeros_like(logits)
    onehot[:, accent_id] = 1.0
    g = a * (torch.softmax(logits, dim=1) - onehot) / B
    if mode == 1:
        g = g + b * 2.0 * (logits - 1.0 / C) / (B * C)
    return g


def grads(pooled, logits, W, accent_id, mode, a, b):
    """-> dlogit (B, C), dW (C, d), dbias (C), dpool (B, d); denc[b, t, :] += dpool[b, :] for every t"""
    g = dlogit(logits, accent_id, mode, a, b)
    return g, g.t() @ pooled.double(), g.sum(dim=0), g @ W.double()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 error bounds (formulas; every one is `terms x 2^-24 x sum of magnitudes`, propagated through the products)
# ---------------------------------------------------------------------------------------------------------------------
def pooled_bound(enc):
    """fp32 sum of n = T terms in any order: |err| <= n u sum_t |x|, per element"""
    T = enc.shape[1]
    return T * U * enc.double().abs().sum(dim=1)


def logits_bound(enc, W, bias):
    """logit = sum_k pooled_k W_k + bias over d + 1 terms of fp32-rounded products, pooled carrying pooled_bound:
    (d + 2) u (|pooled| . |W| + |bias|) + pooled_bound . |W|, with |pooled| <= sum_t |x|"""
    d = enc.shape[2]
    mag = enc.double().abs().sum(dim=1)
    Wd = W.double().abs()
    return (d + 2) * U * (mag @ Wd.t() + bias.double().abs()) + pooled_bound(enc) @ Wd.t() * (1 + (d + 2) * U)


def softmax_rel_bound(logits, dl):
    """relative error of exp(z - max) / sum: the argument moves by <= 2 max(dl) + u |z - max|, expf / the division / the C-term sum
    add a few u each: 2 max dl + (|z - max|_max + C + 8) u, first order, per row"""
    z = logits.double()
    C = z.shape[1]
    spread = (z - z.max(dim=1, keepdim=True).values).abs().max(dim=1).values
    return 2.0 * dl.max(dim=1).values + (spread + C + 8) * U


def losses_bound(logits, dl, mode):
    """CE mean, formed as log(sum exp(z - max)) - (z_accent - max): per row the logits' error moves it by <= 2 max dl, the differences
    z - max round at |z - max| <= spread, expf, logf and the C-term sum add (C + 8) u at the magnitude 1 + |log sum| + spread; plus
    the B-term mean: (B + 2) u mean|row|.
    MSE mean over n = B C terms: 2 |z - 1/C| (dl + u (|z| + 1/C)) + (n + 4) u (z - 1/C)^2 each."""
    z = logits.double()
    B, C = z.shape
    mx = z.max(dim=1, keepdim=True).values
    spread = (z - mx).abs().max(dim=1).values
    row = 1.0 + torch.log(torch.exp(z - mx).sum(dim=1)).abs() + spread
    ce = (2.0 * dl.max(dim=1).values + (C + 8) * U * row).mean() + (B + 2) * U * row.mean()
    if mode != 1:
        return ce, None
    q = (z - 1.0 / C).abs()
    mse = (2.0 * q * (dl + U * (z.abs() + 1.0 / C)) + (B * C + 4) * U * q * q).sum() / (B * C)
    return ce, mse


def dlogit_bound(logits, dl, accent_id, mode, a, b):
    """|a| / B (p rel + 6 u (p + onehot)) + |b| 2 / (B C) (dl + 6 u (|z| + 1/C)): each term with its factor's error and the
    roundings of a / B, 1 / C, the difference, the product and the final sum (relative to the TERMS: they may cancel)"""
    z = logits.double()
    B, C = z.shape
    p = torch.softmax(z, dim=1)
    onehot = torch.zeros_like(z)
    onehot[:, accent_id] = 1.0
    out = abs(a) / B * (p * softmax_rel_bound(z, dl)[:, None] + 6 * U * (p + onehot))
    if mode == 1:
        out = out + abs(b) * 2.0 / (B * C) * (dl + 6 * U * (z.abs() + 1.0 / C))
    return out


def grads_bound(enc, logits, W, dl, accent_id, mode, a, b):
    """-> bounds of (dW, dbias, dpool): each a sum of n <= max(B, C) <= 64-term products of a dlogit (error dlogit_bound) with an
    exact or pooled_bound-carrying factor: sum |factor| dbound + sum |dlogit| factor_bound + (n + 2) u sum |dlogit| |factor|"""
    B, C = logits.shape
    g = dlogit(logits, accent_id, mode, a, b).abs()
    db = dlogit_bound(logits, dl, accent_id, mode, a, b)
    mag = enc.double().abs().sum(dim=1)                     # >= |pooled|
    pb = pooled_bound(enc)
    Wd = W.double().abs()
    dW = db.t() @ mag + g.t() @ pb + (B + 2) * U * (g.t() @ mag)
    dbias = db.sum(dim=0) + (B + 2) * U * g.sum(dim=0)
    dpool = db @ Wd + (C + 2) * U * (g @ Wd)
    return dW, dbias, dpool


# ---------------------------------------------------------------------------------------------------------------------
# D0
# ---------------------------------------------------------------------------------------------------------------------
class Packed:
    """tests/golden/D0.npz with its compact tensor records ('<prefix>/{l2,sum,numel,step,offsets,data}', one entry per model
    tensor) expanded into the keys tests/golden_util.check_digest reads ('<prefix>/<name>/{l2,full | sample,step}')."""

    def __init__(self, z):
        self._z = z
        self._extra = {}
        names = [str(s) for s in z['param_names']]
        for key in z.files:
            if not key.endswith('/offsets'):
                continue
            pre = key[:-len('/offsets')]
            off, data, step, l2 = z[key], z[pre + '/data'], z[pre + '/step'], z[pre + '/l2']
            for i, nm in enumerate(names):
                base = '%s/%s/' % (pre, nm)
                self._extra[base + 'l2'] = l2[i]
                chunk = data[off[i]:off[i + 1]]
                if int(step[i]) == 0:
                    self._extra[base + 'full'] = chunk
                else:
                    self._extra[base + 'sample'] = chunk
                    self._extra[base + 'step'] = step[i]
        self.files = list(z.files) + list(self._extra)

    def __getitem__(self, key):
        return self._extra[key] if key in self._extra else self._z[key]


_D0 = None


def load_d0():
    """-> (Packed record, cfg, spec) like tests/golden_util.load; read once and shared, never modified"""
    global _D0
    if _D0 is None:
        from tests import golden_util as gu
        z, cfg, spec = gu.load('D0')
        _D0 = (Packed(z), cfg, dict(spec, lr_disc=float(z['lr_disc']), num_class=int(z['num_class'])))
    return _D0


def ce_tolerance(ref, logits, accent_id, loss_rtol, logit_rtol):
    """Tolerance for a discriminator CE against the recorded `ref`, given the recorded logits (B, C), the relative tolerance of a loss
    `loss_rtol` and the relative tolerance `logit_rtol` that the compared LOGITS are held to (norm-wise, so element-wise
    |dz| <= logit_rtol ||z||_2):
        loss_rtol |ref|  +  4 * 2^-24  +  mean_b sum_c |softmax(z)[b][c] - onehot[b][c]| * logit_rtol ||z||_2
    The first term is the loss comparator of the J0 / golden tests.  The floor is the rounding of the sum of exponentials near 1 and
    of its logarithm, which the reference's own fp32 value (log_softmax: (z - max) - log sum exp(z - max)) carries.  The last term is
    the CE's first-order response to a difference of the logits, dCE = mean_b sum_c (softmax - onehot) dz: for a separated accent it
    is of the order of CE * logit_rtol * |z|, so a CE of 0 does not pass for one of 3e-4."""
    z = torch.as_tensor(np.asarray(logits)).double()
    onehot = torch.zeros_like(z)
    onehot[:, accent_id] = 1.0
    resp = float((torch.softmax(z, dim=1) - onehot).abs().sum(dim=1).mean())
    return loss_rtol * abs(float(ref)) + 4 * U + resp * logit_rtol * float(z.norm())


def line(z, mode, it):
    return bytes(z['%s/%d/line' % (mode, it)]).decode()
