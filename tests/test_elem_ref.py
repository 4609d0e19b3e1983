"""The references of tests/elem_ref.py against independent formulations: the h2 census against a plain Python loop on hand-picked
values, the softmax / LayerNorm / cross-entropy / Adam fp64 helpers against torch.  No GPU."""
import math
import struct

import numpy as np
import torch
import torch.nn.functional as F

from tests import elem_ref as R


def _f32(v):
    return struct.unpack('f', struct.pack('f', v))[0]


def _census_loop(values, bound):
    """the census spelled out per element with Python floats (doubles): exponent of the bound from its bit pattern"""
    bits = struct.unpack('I', struct.pack('f', bound))[0]
    e = (bits >> 23) & 0xff
    s = 1.0 if e == 0 else math.ldexp(1.0, min(max(141 - e, -60), 60))
    nz = b22 = b16 = 0
    for v in values:
        a = abs(_f32(v)) * s
        if a > 0:
            nz += 1
            if a < 0.125:
                b22 += 1
            if a < 0.001953125:
                b16 += 1
    return nz, b22, b16


def test_h2_scale_brings_the_bound_into_2_14_2_15():
    for b in (1.0, 8.0, float(np.nextafter(np.float32(8.0), np.float32(0))), 5.7, 3e-7, 4e5, 2.0 ** -40, 2.0 ** 70):
        s = R.h2_scale(b)
        assert 2.0 ** 14 <= _f32(b) * s < 2.0 ** 15, (b, s)
    assert R.h2_scale(0.0) == 1.0 and R.h2_scale(1e-42) == 1.0                 # zero / subnormal bound
    assert R.h2_scale(2.0 ** -120) == 2.0 ** 60 and R.h2_scale(2.0 ** 120) == 2.0 ** -60      # clamped exponent
    assert R.h2_scale(float(np.nextafter(np.float32(8.0), np.float32(0)))) == 2 * R.h2_scale(8.0)


def test_h2_census_equals_a_plain_loop_on_hand_picked_values():
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    for bound in (8.0, below(8.0), 5.7, 0.0, 8.0 * 1024, 3e-7):
        s = R.h2_scale(bound)
        t22, t16 = 0.125 / s, 0.001953125 / s
        vals = [0.0, -0.0, t22, -t22, below(t22), -below(t22), t16, -t16, below(t16), -below(t16), 2 * t22, t22 / 2, t16 / 2, -t16 / 2,
                float(np.nextafter(np.float32(t22), np.float32(1e30))), float(np.nextafter(np.float32(t16), np.float32(1e30))),
                1e-45, -1e-45, 1e-42, -3e-39, 1.1754942e-38, 1.17549435e-38, bound, -bound, bound / 3, 1.0, -1.0, 0.125, below(0.125),
                0.001953125, below(0.001953125), 3.4e38, -3.4e38, 1e-30, 7e-12, 2.5e-7, 6.1e-5, below(6.1e-5), 1e-3, 0.1, 0.5, 2.0, 100.0,
                -65504.0, 1e10, t22 * 1.5, t16 * 1.5, t22 * 0.75, t16 * 0.75, 0.0]
        assert len(vals) == 50
        x = np.array(vals, dtype=np.float32)
        assert R.h2_census(x, bound) == _census_loop(vals, bound), bound
        for n in (1, 3, 6, 49):
            assert R.h2_census(x[:n], bound) == _census_loop(vals[:n], bound)
    # elements exactly on a line are not counted, the next float below is
    assert R.h2_census(np.array([2.0 ** -14], np.float32), 8.0) == (1, 0, 0)
    assert R.h2_census(np.array([below(2.0 ** -14)], np.float32), 8.0) == (1, 1, 0)
    assert R.h2_census(np.array([2.0 ** -20], np.float32), 8.0) == (1, 1, 0)
    assert R.h2_census(np.array([below(2.0 ** -20)], np.float32), 8.0) == (1, 1, 1)
    assert R.h2_census(np.array([below(2.0 ** -14)], np.float32), below(8.0)) == (1, 0, 0)       # the scale doubled
    amax = np.zeros(2048, np.float32)
    amax[5 * 32], amax[5 * 32 + 1], amax[63 * 32] = 3.0, 99.0, 7.0
    assert R.slot_bound(amax) == 7.0                                          # slot heads only


def test_softmax_helpers_against_torch():
    g = torch.Generator().manual_seed(1)
    B, H, Tq, Tk = 3, 2, 5, 9
    s = torch.randn(B, H, Tq, Tk, generator=g) * 20
    for klen, causal in ((None, 0), ([1, Tk, Tk + 7], 0), ([4, 9, 2], 1)):
        lim = R.softmax_limits(B, H, Tq, Tk, klen, causal)
        blocked = torch.zeros(B, 1, Tq, Tk, dtype=torch.bool)
        if klen is not None:
            blocked = blocked | (torch.arange(Tk).view(1, 1, 1, Tk) >= torch.tensor(klen).view(B, 1, 1, 1))
        if causal:
            blocked = blocked | torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), 1)
        sr = s.double().clone().requires_grad_(True)
        pr = torch.softmax((sr * 0.25).masked_fill(blocked, -np.inf), -1)
        dp = torch.randn(pr.shape, generator=g)
        pr.backward(dp.double())
        P = R.softmax_fwd(s, 0.25, lim)
        assert float((P - pr.detach()).abs().max()) < 1e-15
        assert float(P.masked_select(blocked.expand_as(P)).abs().max() if blocked.any() else 0.0) == 0.0
        assert float((R.softmax_bwd(P, dp, 0.25) - sr.grad).abs().max()) < 1e-14
    # a row without a live key: zeros, not NaN
    P = R.softmax_fwd(s, 1.0, R.softmax_limits(B, H, Tq, Tk, [0, 3, Tk], 0))
    assert float(P[0].abs().max()) == 0.0 and bool(torch.isfinite(P).all())
    assert float(R.softmax_bwd(P, torch.ones_like(P), 1.0)[0].abs().max()) == 0.0


def test_layernorm_helper_against_torch():
    g = torch.Generator().manual_seed(2)
    rows, d, T, rpg = 13, 64, 4, 5
    x, res, dy = (torch.randn(rows, d, generator=g) for _ in range(3))
    gam, bet, pe = torch.randn(3, d, generator=g), torch.randn(3, d, generator=g), torch.randn(T, d, generator=g)
    keep = (torch.rand(rows, generator=g) > 0.3).int()
    xmask = (torch.rand(rows, d, generator=g) > 0.25).to(torch.uint8)
    a = R.layernorm(x, res, gam, bet, pe, keep, xmask, R.f32(1 / 0.75), T, 1e-5, rpg, dy)
    b = R.layernorm(x, res, gam, bet, pe, keep, xmask, R.f32(1 / 0.75), T, 1e-5, rpg, dy, builtin=True)
    for k in ('y', 'xhat', 'dz', 'dx', 'dgamma', 'dbeta', 'dsum'):
        assert float((a[k] - b[k]).abs().max()) < 1e-12, k
    # per group against F.layer_norm with that group's parameters
    z = (x.double() * xmask.double() * R.f32(1 / 0.75) + res.double())
    for t in range(3):
        sl = slice(t * rpg, min((t + 1) * rpg, rows))
        y = (F.layer_norm(z[sl], (d,), gam[t].double(), bet[t].double(), 1e-5) + pe.double()[torch.arange(rows)[sl] % T]) * keep[sl].double()[:, None]
        assert float((a['y'][sl] - y).abs().max()) < 1e-12
    assert float((a['rstd'] - 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)).abs().max()) < 1e-12
    assert float((a['dsum'].sum(0) - a['dx'].sum(0)).abs().max()) < 1e-12
    c = R.layernorm(x, None, gam[:1], bet[:1], None, None, None, 1.0, 1, 1e-5, rows, dy)       # every optional input absent
    xr = x.double().clone().requires_grad_(True)
    F.layer_norm(xr, (d,), gam[0].double(), bet[0].double(), 1e-5).backward(dy.double())
    assert float((c['dz'] - xr.grad).abs().max()) < 1e-12 and c['dz'] is c['dx']
    # a constant row: xhat = 0, rstd = 1 / sqrt(eps); its gradient is rstd (g - mean g), not zero
    c = R.layernorm(torch.full((1, d), 1.5), None, torch.ones(1, d), torch.zeros(1, d), None, None, None, 1.0, 1, 1e-5, 1, dy[:1])
    assert float(c['xhat'].abs().max()) == 0.0 and abs(float(c['rstd']) - 1e5 ** 0.5) < 1e-9
    assert float((c['dz'] - 1e5 ** 0.5 * (dy[:1].double() - dy[:1].double().mean())).abs().max()) < 1e-9


def test_cross_entropy_and_adam_helpers_against_torch():
    g = torch.Generator().manual_seed(3)
    rows, V = 9, 37
    logits, gold = torch.randn(rows, V, generator=g), torch.randint(1, V, (rows,), generator=g)
    gold[4] = 0
    w = torch.full((rows,), 0.125)
    lse, loss, grad = R.cross_entropy(logits, gold, 0, 0.0, w)
    lr = logits.double().clone().requires_grad_(True)
    ref = F.cross_entropy(lr, gold, ignore_index=0, reduction='none')
    (ref * 0.125).sum().backward()
    assert float((loss - ref.detach()).abs().max()) < 1e-13 and float((grad - lr.grad).abs().max()) < 1e-14
    assert float(loss[4]) == 0.0 and float(grad[4].abs().max()) == 0.0
    # smoothing: the closed form of the kernel, (1 - e) nll + e / V (sum_j -logp_j - nll), and its gradient tsum p - t
    lse, loss, grad = R.cross_entropy(logits, gold, 0, 0.1, w)
    logp = logits.double() - lse[:, None]
    nll = -logp.gather(1, gold[:, None]).squeeze(1)
    closed = torch.where(gold != 0, 0.9 * nll + 0.1 / V * (-logp.sum(1) - nll), torch.zeros_like(nll))
    assert float((loss - closed).abs().max()) < 1e-13
    t = torch.full((rows, V), 0.1 / V, dtype=torch.float64).scatter(1, gold[:, None], 0.9)
    closed_g = 0.125 * ((0.9 + (V - 1) * 0.1 / V) * logp.exp() - t) * (gold != 0).double()[:, None]
    assert float((grad - closed_g).abs().max()) < 1e-14
    # Adam: betas that fp32 holds exactly, so that torch.optim.Adam (Python-float betas) is given the same numbers
    n, b1, b2 = 50, 0.875, 1 - 2.0 ** -9
    th, gg, m = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3))
    v = torch.rand(n, generator=g, dtype=torch.float64)
    for step in (1, 1000):
        p = th.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=R.f32(1e-3), betas=(b1, b2), eps=R.f32(1e-8))
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        p.grad = gg.clone()
        opt.step()
        t1, m1, v1, _, _ = R.adam(th, gg, m, v, step, 1e-3, b1, b2, 1e-8)
        assert float((t1 - p.detach()).abs().max()) < 1e-14
        assert float((m1 - opt.state[p]['exp_avg']).abs().max()) < 1e-15 and float((v1 - opt.state[p]['exp_avg_sq']).abs().max()) < 1e-15


def test_embed_chains_and_mask_shift_helpers():
    first, nxt = R.embed_chains([3, 0, 3, 5, 3, 0, 5, 3], 4)
    assert first.tolist() == [1, 1, 0, 1, 1, 1, 1, 0] and nxt.tolist() == [2, -1, -1, -1, 7, -1, -1, -1]
    a = torch.arange(20, dtype=torch.uint8)
    assert R.philox_shift_ok(a, torch.cat([a[4:], torch.zeros(4, dtype=torch.uint8)])) and not R.philox_shift_ok(a, a)
