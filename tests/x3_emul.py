"""CPU emulation of the split-bf16 ("x3") arithmetic, restated in plain torch for the tests (no kernel code is copied).

Every fp32 operand is split exactly into three bf16 pieces and a product is the fp32 sum of six piece products
(a0 b0 + a0 b1 + a1 b0 + a1 b1 + a0 b2 + a2 b0).  The three second-order terms are each about 2^-18 of the product: losing one
of them is invisible at the tolerances of an fp32 comparison.  This module (1) emulates the products with any list of terms,
(2) builds the inputs of every case of tests/test_x3_precision_gpu.py, and (3) derives the bound of each case from the
emulation alone: half of what the cheapest dropped term costs (random inputs), or an eighth of it (probe inputs that cancel
the leading term, so that a second-order term weighs 2^-9 of the result).  tests/test_x3_emulation.py shows on the CPU that
every bound separates six terms from five; the GPU file holds the kernels to the same bounds through the same `check`."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))          # (piece of a, piece of b), smallest first: the kernels' list
SECOND_ORDER = ((2, 0), (1, 1), (0, 2))


def drops(terms=SIX):
    """the three five-term lists: one second-order term removed (a lost first-order term is caught by every test already)"""
    return [tuple(t for t in terms if t != d) for d in SECOND_ORDER]


def split3(x, rounding='rne'):
    """x (fp32) -> three fp32 tensors holding bf16 values whose sum is x exactly.
    'rne': each piece is the bf16 rounding of what the previous pieces left; 'trunc': the upper 16 bits of it."""
    assert x.dtype == torch.float32

    def lead(r):
        if rounding == 'rne':
            return r.bfloat16().float()
        assert rounding == 'trunc'
        return (r.contiguous().view(torch.int32) & -65536).view(torch.float32)
    p0 = lead(x)
    r1 = x - p0
    p1 = lead(r1)
    r2 = r1 - p1
    p2 = lead(r2)
    assert torch.equal(p0.double() + p1.double() + p2.double(), x.double()), 'the three-piece split must be exact'
    return p0, p1, p2


def piece_products(a, b, rounding='rne', terms=SIX):
    """{term: fp32 product of that pair of pieces} for a (.., M, K) @ b (.., K, N)"""
    pa, pb = split3(a, rounding), split3(b, rounding)
    return {t: pa[t[0]] @ pb[t[1]] for t in terms}


def sum_terms(prods, terms):
    out = None
    for t in terms:                                              # fp32 sum in list order (smallest first)
        out = prods[t].clone() if out is None else out + prods[t]
    return out


def mm_x3(a, b, terms=SIX, rounding='rne'):
    """the listed piece products, each formed in fp32, summed in fp32 smallest first"""
    return sum_terms(piece_products(a, b, rounding, terms), terms)


def rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def check(errs, bound, what=''):
    """THE assertion of both test files: every error of `errs` (name -> relative error) is below `bound`."""
    for name, e in errs.items():
        assert math.isfinite(e) and e < bound, '%s %s: %.3e is not below the bound %.3e' % (what, name, e, bound)


# ------------------------------------------------------------------------------------------------ probe builders
def const_lead(shape, eps=2.0 ** -8, g=None, rounding='rne', positive=False):
    """along the last axis the LEADING bf16 piece is one constant per row (r = randn.bfloat16()); the rest is r (1 + eps (rand - 1/2))
    ('trunc': r (1 + eps rand / 2), so that the upper 16 bits stay r).  The product of such a row with an antisymmetric column
    loses its a0 . b part exactly."""
    r = torch.randn(tuple(shape[:-1]) + (1,), generator=g).bfloat16().float()
    r = torch.where(r.abs() < 0.125, torch.full_like(r, 0.5), r)  # keep every row well away from zero
    if positive:
        r = r.abs()
    u = torch.rand(shape, generator=g)
    x = r * (1 + eps * ((u - 0.5) if rounding == 'rne' else 0.5 * u))
    assert torch.equal(split3(x, rounding)[0], r.expand(shape)), 'leading piece is not constant'
    return x


def antisym(shape, g=None):
    """x[..., 2t] = -x[..., 2t + 1]"""
    assert shape[-1] % 2 == 0
    h = torch.randn(tuple(shape[:-1]) + (shape[-1] // 2,), generator=g)
    return torch.stack([h, -h], dim=-1).reshape(shape)


# ------------------------------------------------------------------------------------------------ attention
ATTN_PRODUCTS = ('qk', 'pv', 'pdo', 'dov', 'dsk', 'dsq')       # Q K^T, P V, P^T dO, dO V^T, dS K, dS^T Q
ATTN_OUTPUTS = ('O', 'dq', 'dk', 'dv')
D_HEAD = 64


def attention(q, k, v, dO, causal, klens, keep, pscale, scale, mm):
    """forward and backward of scaled-dot-product attention written out on (B, H, T, d) tensors; mm(name, a, b) forms each of
    the six products.  Returns O, lse, dq, dk, dv."""
    Tq, Tk = q.shape[2], k.shape[2]
    blocked = torch.zeros(q.shape[0], 1, Tq, Tk, dtype=torch.bool)
    if klens is not None:
        blocked = blocked | (torch.arange(Tk).view(1, 1, 1, Tk) >= torch.tensor(klens).view(-1, 1, 1, 1))
    if causal:
        blocked = blocked | torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=1).view(1, 1, Tq, Tk)
    s = (mm('qk', q, k.transpose(2, 3)) * scale).masked_fill(blocked, -np.inf)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    pd = p * (keep.to(p.dtype) * pscale) if keep is not None else p
    O = mm('pv', pd, v)
    dv = mm('pdo', pd.transpose(2, 3), dO)
    dp = mm('dov', dO, v.transpose(2, 3))
    if keep is not None:
        dp = dp * (keep.to(p.dtype) * pscale)
    delta = (dO * O).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = mm('dsk', ds, k)
    dk = mm('dsq', ds.transpose(2, 3), q)
    return dict(O=O, lse=lse, dq=dq, dk=dk, dv=dv)


def attention_x3(q, k, v, dO, causal, klens, keep, pscale=1.0, scale=None, drop=None, rounding='rne', memo=None):
    """the six products through mm_x3; drop = (product, term) removes one term from one product.
    memo (a dict, optional) only saves time in a sweep over drops.  Invariant: an entry memo[product] = (a, b, piece products) is
    written once, by the first run that meets the product (the six-term run), and never replaced; a later run uses it only when
    both of its operands are bit-identical to the stored ones (a product upstream of the dropped term, or beside it), and forms
    the piece products afresh otherwise (a product downstream of the dropped term).  Results are the same with memo = None."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale

    def mm(name, a, b):
        terms = tuple(t for t in SIX if t != drop[1]) if drop is not None and drop[0] == name else SIX
        a, b = a.contiguous(), b.contiguous()
        if memo is None:
            return mm_x3(a, b, terms, rounding)
        if name not in memo or not (torch.equal(memo[name][0], a) and torch.equal(memo[name][1], b)):
            prods = piece_products(a, b, rounding)
            if name in memo:                                    # operands differ from the six-term run's: form afresh, keep the entry
                return sum_terms(prods, terms)
            memo[name] = (a, b, prods)
        return sum_terms(memo[name][2], terms)
    return attention(q, k, v, dO, causal, klens, keep, pscale, scale, mm)


def attention_plain(q, k, v, dO, causal, klens, keep, pscale=1.0, scale=None, dtype=torch.float64):
    """the same function with plain @: the fp64 reference (dtype = float64) or torch fp32 on the CPU (float32)"""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    q, k, v, dO = (t.to(dtype) for t in (q, k, v, dO))
    return attention(q, k, v, dO, causal, klens, keep, pscale, scale, lambda name, a, b: a @ b)


def heads(x, H):            # (B, T, H d) -> (B, H, T, d)
    return x.view(x.shape[0], x.shape[1], H, -1).transpose(1, 2)


def merge(x):               # (B, H, T, d) -> (B, T, H d)
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)


# name: (B, H, Tq, Tk, causal, klens, dropout, (B, H) of the slice the bound is taken from or None, strided)
ATTN_CASES = {
    'causal_ragged': (2, 2, 130, 130, 1, [130, 65], 0.0, None, False),
    'cross_ragged': (2, 2, 65, 130, 0, [130, 31], 0.0, None, False),
    'one_full_tile': (2, 2, 64, 64, 0, None, 0.0, None, False),
    'causal_dropout': (2, 4, 130, 130, 1, None, 0.25, None, False),
    'two_launch_backward': (11, 16, 130, 130, 1, None, 0.0, (1, 2), False),
    'strided': (2, 2, 130, 130, 1, [130, 97], 0.0, None, True),
}
# name: (probed product, which operand is constant-lead, probed outputs); B = 1, H = 2, T = 130, causal
ATTN_PROBES = {
    'qk_q_const': ('qk', 'a', ('O', 'lse')),
    'qk_k_const': ('qk', 'b', ('O', 'lse')),
    'dov_do_const': ('dov', 'a', ('dq', 'dk')),
    'dov_v_const': ('dov', 'b', ('dq', 'dk')),
}
PROBE_TERMS = {'a': ((1, 1), (2, 0)), 'b': ((1, 1), (0, 2))}    # the second-order terms a probe weighs at 2^-9 of the result


@functools.lru_cache(maxsize=None)
def attn_inputs(name):
    """q, k, v, dO as (B, T, H d) fp32 matrices (+ keep-mask, pscale, ldm, scale) of a random-input case or a probe"""
    if name in ATTN_CASES:
        B, H, Tq, Tk, causal, klens, drop, _, _ = ATTN_CASES[name]
        g = torch.Generator().manual_seed(1000 + sorted(ATTN_CASES).index(name))
        q = torch.randn(B, Tq, H * D_HEAD, generator=g)
        k = torch.randn(B, Tk, H * D_HEAD, generator=g)
        v = torch.randn(B, Tk, H * D_HEAD, generator=g)
        dO = torch.randn(B, Tq, H * D_HEAD, generator=g)
        ldm = (Tk + 3) // 4 * 4
        keep = (torch.rand(B, H, Tq, ldm, generator=g) >= drop).to(torch.uint8) if drop > 0 else None
        return dict(q=q, k=k, v=v, dO=dO, keep=keep, ldm=ldm, pscale=1.0 / (1 - drop), scale=1.0 / math.sqrt(D_HEAD), B=B, H=H, Tq=Tq,
                    Tk=Tk, causal=causal, klens=klens)
    prod, side, _ = ATTN_PROBES[name]
    B, H, T = 1, 2, 130
    g = torch.Generator().manual_seed(2000 + sorted(ATTN_PROBES).index(name))
    t = {n: torch.randn(B, H, T, D_HEAD, generator=g) for n in ('q', 'k', 'v', 'dO')}
    an, bn = ('q', 'k') if prod == 'qk' else ('dO', 'v')        # both products contract over the head dimension
    cn, sn = (an, bn) if side == 'a' else (bn, an)
    t[cn] = const_lead((B, H, T, D_HEAD), g=g)
    t[sn] = antisym((B, H, T, D_HEAD), g=g)
    if prod == 'qk':
        t['q'] = t['q'] * 2.0 ** 8                              # exact; the scores (carried by the second pieces) stay O(1)
    return dict(q=merge(t['q']), k=merge(t['k']), v=merge(t['v']), dO=merge(t['dO']), keep=None, ldm=(T + 3) // 4 * 4, pscale=1.0,
                scale=1.0 / math.sqrt(D_HEAD), B=B, H=H, Tq=T, Tk=T, causal=1, klens=None)


def attn_errors(out, ref):
    """relative L2 per output; lse as max |difference| / max |lse| (the form its bound takes)"""
    e = {n: rel(out[n], ref[n]) for n in ATTN_OUTPUTS}
    e['lse'] = float((out['lse'].double() - ref['lse'].double()).abs().max() / ref['lse'].double().abs().max())
    return e


def _attn_args(inp, sl=None):
    H = inp['H']
    q, k, v, dO = (heads(inp[n], H) for n in ('q', 'k', 'v', 'dO'))
    keep, klens = inp['keep'], inp['klens']
    if keep is not None:
        keep = keep[..., :inp['Tk']]
    if sl is not None:
        b, h = sl
        q, k, v, dO = (t[:b, :h] for t in (q, k, v, dO))
        keep = keep[:b, :h] if keep is not None else None
        klens = klens[:b] if klens is not None else None
    return (q, k, v, dO, inp['causal'], klens, keep), dict(pscale=inp['pscale'], scale=inp['scale'])


def attn_reference(name):
    """fp64 on the CPU from the identical fp32 inputs, in the (B, T, H d) layout of the kernels (lse: (B, H, Tq))"""
    args, kw = _attn_args(attn_inputs(name))
    ref = attention_plain(*args, **kw)
    return {n: (t if n == 'lse' else merge(t)) for n, t in ref.items()}


@functools.lru_cache(maxsize=None)
def attn_report(name):
    """errors against fp64 of the six-term emulation, of torch fp32 and of every five-term emulation, and the bound of the case"""
    inp = attn_inputs(name)
    probe = name in ATTN_PROBES
    args, kw = _attn_args(inp, None if probe else ATTN_CASES[name][7])
    ref = attention_plain(*args, **kw)
    memo = {}
    rep = dict(six=attn_errors(attention_x3(*args, memo=memo, **kw), ref), f32=attn_errors(attention_plain(*args, dtype=torch.float32, **kw), ref))
    if probe:
        prod, side, outs = ATTN_PROBES[name]
        rep['outputs'] = outs
        rep['drops'] = {(prod, t): attn_errors(attention_x3(*args, drop=(prod, t), memo=memo, **kw), ref) for t in PROBE_TERMS[side]}
        rep['bound'] = min(max(e[o] for o in outs) for e in rep['drops'].values()) / 8
    else:
        rep['outputs'] = ATTN_OUTPUTS
        rep['drops'] = {(p, t): attn_errors(attention_x3(*args, drop=(p, t), memo=memo, **kw), ref) for p in ATTN_PRODUCTS for t in SECOND_ORDER}
        rep['bound'] = min(max(e[o] for o in ATTN_OUTPUTS) for e in rep['drops'].values()) / 2
    return rep


# ------------------------------------------------------------------------------------------------ 3 x 3 convolutions
CONV_SHAPES = [(64, 64, 2, 21, 161), (64, 128, 2, 18, 80), (128, 128, 1, 9, 19)]           # (Cin, Cout, B, T, F)
CONV_TB = (64, 64, 2, 21, 161, 3)                                                           # ... + tasks (per-task weights)
CONV_PRODUCTS = ('fwd', 'dgrad', 'wgrad')


def conv3x3_x3(x, w, dy, mm):
    """the three products of a 3 x 3 / padding 1 convolution on unfold matrices, reference layout: x (B, Cin, F, T), w (Cout, Cin,
    3, 3), dy (B, Cout, F, T).  mm(name, a, b) forms each product.  Returns the pre-activation y (no bias), the data gradient
    (no input gate) and the weight gradient; ReLU, bias and pooling stay with the caller."""
    B, Cin, Fq, T = x.shape
    Cout = w.shape[0]
    ux = F.unfold(x, 3, padding=1)                                                   # (B, Cin 9, F T)
    y = mm('fwd', ux.transpose(1, 2), w.reshape(Cout, Cin * 9).t().unsqueeze(0)).transpose(1, 2).reshape(B, Cout, Fq, T)
    wd = w.flip(2, 3).transpose(0, 1).reshape(Cin, Cout * 9)
    udy = F.unfold(dy, 3, padding=1)                                                 # (B, Cout 9, F T)
    dx = mm('dgrad', udy.transpose(1, 2), wd.t().unsqueeze(0)).transpose(1, 2).reshape(B, Cin, Fq, T)
    dyp = dy.reshape(B, Cout, Fq * T).transpose(0, 1).reshape(Cout, B * Fq * T)      # the contraction runs over every pixel
    uxp = ux.transpose(1, 2).reshape(B * Fq * T, Cin * 9)
    dw = mm('wgrad', dyp, uxp).reshape(Cout, Cin, 3, 3)
    return dict(fwd=y, dgrad=dx, wgrad=dw)


def conv_outputs(x, b, pooled=False):
    """what the kernels add to the three products: fwd -> relu(y + bias) [-> 2 x 2 max-pool], dgrad -> gated by the input's ReLU"""
    def fwd(y):
        z = torch.relu(y + b.to(y.dtype).view(1, -1, 1, 1))
        return F.max_pool2d(z, 2, stride=2) if pooled else z
    return {'fwd': fwd, 'dgrad': lambda dx: dx * (x > 0), 'wgrad': lambda dw: dw}


def _conv_report(x, w, dy, post, probe=None):
    """per product: errors of six terms / torch fp32 / each five-term list against fp64 on the kernel's output (post[product] applied
    to every variant alike), and the bound.  probe = {product: side of the constant-lead operand}"""
    ref = conv3x3_x3(x.double(), w.double(), dy.double(), lambda n, a, b: a @ b)
    f32 = conv3x3_x3(x, w, dy, lambda n, a, b: a @ b)
    holder = {}

    def mm(name, a, b):
        holder[name] = piece_products(a.contiguous(), b.contiguous())
        return sum_terms(holder[name], SIX)
    six = conv3x3_x3(x, w, dy, mm)
    # the unfold matrices put the image on the `a` side of fwd / dgrad and on the `b` side of wgrad
    rep = {}
    for n in CONV_PRODUCTS:
        if probe is not None and n not in probe:
            continue
        shape, prods = six[n].shape, holder[n]

        def fin(m):
            return m.transpose(1, 2).reshape(shape) if n != 'wgrad' else m.reshape(shape)
        dropped = PROBE_TERMS[probe[n]] if probe is not None else SECOND_ORDER
        want = post[n](ref[n])
        r = dict(six=rel(post[n](six[n]), want), f32=rel(post[n](f32[n]), want),
                 drops={t: rel(post[n](fin(sum_terms(prods, tuple(s for s in SIX if s != t)))), want) for t in dropped})
        r['bound'] = min(r['drops'].values()) / (8 if probe is not None else 2)
        rep[n] = r
    return rep


def nhwc(t):                # reference (B, C, F, T) <-> the kernels' (B, T, F, C)
    return t.permute(0, 3, 2, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_inputs(shape, tasks=1):
    """random inputs in the reference layout: x >= 0 (a ReLU output), w, bias, the gradient of the dense output and of the pooled
    one; with tasks > 1 a leading task axis and per-task weights"""
    Cin, Cout, B, T, Fq = shape
    g = torch.Generator().manual_seed(3000 + Cin + Cout + T + tasks)
    x = torch.relu(torch.randn(tasks, B, Cin, Fq, T, generator=g))
    w = torch.randn(tasks, Cout, Cin, 3, 3, generator=g) * (1.0 / np.sqrt(9 * Cin))
    b = torch.randn(tasks, Cout, generator=g) * 0.1
    dy = torch.randn(tasks, B, Cout, Fq, T, generator=g)
    dp = torch.randn(tasks, B, Cout, Fq // 2, T // 2, generator=g)
    return dict(x=x, w=w, b=b, dy=dy, dp=dp)


@functools.lru_cache(maxsize=None)
def conv_reference(shape, tasks=1):
    """fp64 forward per task: y = relu(conv + b), its 2 x 2 max-pool, and the two gradients handed to the backward kernels in full
    resolution: dy gated by y > 0, and dp gated by p > 0 and scattered to the arg-max positions"""
    inp = conv_inputs(shape, tasks)
    out = []
    for t in range(tasks):
        y = torch.relu(F.conv2d(inp['x'][t].double(), inp['w'][t].double(), inp['b'][t].double(), padding=1))
        p, idx = F.max_pool2d(y, 2, stride=2, return_indices=True)
        dyg = (inp['dy'][t].double() * (y > 0)).float()
        dpg = (inp['dp'][t].double() * (p > 0)).float()
        out.append(dict(y=y, p=p, idx=idx, dyg=dyg, dpg=dpg))
    return out


def scatter_pooled(dpg, am, Fq, T):
    """pooled gradient (B, C, F/2, T/2) -> full resolution (B, C, F, T) at the positions of the arg-max codes am (same shape,
    bit 1 = f offset, bit 0 = t offset); odd trailing rows / columns stay zero"""
    B, C, Fp, Tp = dpg.shape
    full = torch.zeros(B, C, Fq, T, dtype=dpg.dtype)
    am = am.long()
    f = torch.arange(Fp).view(1, 1, Fp, 1) * 2 + (am >> 1)
    t = torch.arange(Tp).view(1, 1, 1, Tp) * 2 + (am & 1)
    full.view(B, C, Fq * T).scatter_(2, (f * T + t).view(B, C, -1), dpg.reshape(B, C, -1))
    return full


def codes_of(idx, T):
    """max_pool2d's flat indices -> the kernels' 2-bit arg-max codes"""
    f, t = idx // T, idx % T
    return ((f & 1) << 1 | (t & 1)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def conv_report(shape, tasks=1, pooled=False, task=0):
    """the bounds of one task of a random-input convolution case (dense: the gated dy; pooled: the scattered pooled gradient)"""
    Cin, Cout, B, T, Fq = shape
    inp, ref = conv_inputs(shape, tasks), conv_reference(shape, tasks)[task]
    dy = scatter_pooled(ref['dpg'], codes_of(ref['idx'], T), Fq, T) if pooled else ref['dyg']
    return _conv_report(inp['x'][task], inp['w'][task], dy, conv_outputs(inp['x'][task], inp['b'][task], pooled))


CONV_PROBE_SHAPE = (64, 64, 2, 21, 161)
CONV_PROBES = ('fwd', 'dgrad', 'wgrad')
CONV_PROBE_SIDE = {'fwd': 'a', 'dgrad': 'a', 'wgrad': 'b'}        # where the constant-lead operand sits in conv3x3_x3's products


@functools.lru_cache(maxsize=None)
def conv_probe_inputs(which):
    """fwd: x constant-lead over a whole sample and positive, w antisymmetric along cin pairs, bias 0.  dgrad: dy constant-lead
    over a whole sample, w antisymmetric along cout pairs.  wgrad: x constant-lead per (sample, channel), dy antisymmetric along
    adjacent f pairs with its outermost ring zero, so that every shifted sum cancels at the zero-padded border too."""
    Cin, Cout, B, T, Fq = CONV_PROBE_SHAPE
    g = torch.Generator().manual_seed(4000 + CONV_PROBES.index(which))
    x = torch.relu(torch.randn(B, Cin, Fq, T, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / np.sqrt(9 * Cin))
    dy = torch.randn(B, Cout, Fq, T, generator=g)
    if which == 'fwd':
        x = const_lead((B, Cin * Fq * T), g=g, positive=True).view(B, Cin, Fq, T)
        w = antisym((Cout, 3, 3, Cin), g=g).permute(0, 3, 1, 2).contiguous() * (1.0 / np.sqrt(9 * Cin))
    elif which == 'dgrad':
        dy = const_lead((B, Cout * Fq * T), g=g).view(B, Cout, Fq, T)
        w = antisym((Cin, 3, 3, Cout), g=g).permute(3, 0, 1, 2).contiguous() * (1.0 / np.sqrt(9 * Cin))
    else:
        x = const_lead((B, Cin, Fq * T), g=g, positive=True).view(B, Cin, Fq, T)
        inner = antisym((B, Cout, T - 2, Fq - 3), g=g).transpose(2, 3)               # f = 1 .. F-3 in pairs (F is odd), t = 1 .. T-2
        dy = torch.zeros(B, Cout, Fq, T)
        dy[:, :, 1:Fq - 2, 1:T - 1] = inner
    return dict(x=x, w=w, dy=dy)


@functools.lru_cache(maxsize=None)
def conv_probe_report(which):
    inp = conv_probe_inputs(which)
    post = conv_outputs(inp['x'], torch.zeros(inp['w'].shape[0]))
    return _conv_report(inp['x'], inp['w'], inp['dy'], post, probe={which: CONV_PROBE_SIDE[which]})[which]


# ------------------------------------------------------------------------------------------------ x3 GEMM engine (truncation split)
GEMM_PROBE_SHAPES = [(101, 252, 64), (100, 512, 2000)]
GEMM_RECORD_SHAPES = [(33, 36, 7), (101, 252, 64), (808, 100, 512), (100, 512, 2000)]        # K = 7, 64, 512, 2000 of the engine's test
GEMM_BOUND_FP32_TEST = 2e-6


@functools.lru_cache(maxsize=None)
def gemm_probe_inputs(M, N, K, side):
    """op(A) (M, K) and op(B) (K, N): side 'a' = A constant-lead along K and B antisymmetric along K; 'b' = the mirrored pair"""
    g = torch.Generator().manual_seed(5000 + M + N + K + (side == 'b'))
    if side == 'a':
        return const_lead((M, K), g=g, rounding='trunc'), antisym((N, K), g=g).t().contiguous()
    return antisym((M, K), g=g), const_lead((N, K), g=g, rounding='trunc').t().contiguous()


def _product_report(a, b, rounding, dropped, divisor):
    ref = a.double() @ b.double()
    prods = piece_products(a, b, rounding)
    r = dict(six=rel(sum_terms(prods, SIX), ref), f32=rel(a @ b, ref),
             drops={t: rel(sum_terms(prods, tuple(s for s in SIX if s != t)), ref) for t in dropped})
    r['bound'] = min(r['drops'].values()) / divisor
    return r


@functools.lru_cache(maxsize=None)
def gemm_probe_report(M, N, K, side):
    a, b = gemm_probe_inputs(M, N, K, side)
    return _product_report(a, b, 'trunc', PROBE_TERMS[side], 8)


@functools.lru_cache(maxsize=None)
def gemm_record_report(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    return _product_report(torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), 'trunc', SECOND_ORDER, 2)
