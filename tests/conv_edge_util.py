"""fp64 truths, a per-element error bound, a CPU emulation of the two-piece fp16 ("h2") product, the case table and truth mutators
for the edge-shape tests of the 3 x 3 convolution kernels (tests/test_conv_edge_ref.py on the CPU, tests/test_conv_edges_gpu.py on
the device).  No kernel code is copied; everything is restated in plain torch.

Layout: every activation / gradient tensor here is in the kernels' (B, T, F, C) layout; weights are (Cout, Cin, 3, 3) as in the
reference model, whose convolution runs over (B, C, F, T): kernel axis 2 (kh) walks F, axis 3 (kw) walks T.

The bound.  With S = the same operation applied to |operands| (+ |bias| for the forward) and K = the reduction length,
    bound = 2 ((K + 1) 2^-24 + c 2^-22) S                                  per element,
(K + 1) 2^-24 S: K fp32 additions + the bias / un-scaling, each rounding to half an ulp of a partial sum that |.|-sums bound by S;
c 2^-22 S: the operand splits -- h2 keeps 22 significand bits of either operand (2^-22 each, first order) and drops l l' (< 2^-22):
c = 3; x3 splits exactly and drops terms below 2^-23 in total: c = 1; the factor 2: the matrix instructions add the 16 (32) products
of a step in an order and with intermediate roundings of their own, which need not be those of sequential IEEE additions -- twice
the sequential bound covers any pairing of the same additions.  ReLU and max are 1-Lipschitz: the bound of a pooled element is the
largest bound in its window; a gate (act > 0) is exact.  Valid while every element that matters is within 2^17 of the supplied
operand bound (csrc/mtl_h2.h): relu(randn) data with one 40 x outlier, as in tests/test_ops_gpu.py."""
import functools
import math

import torch
import torch.nn.functional as F

C_SPLIT = {'h2': 3.0, 'x3': 1.0}


def ref(t):
    """(B, T, F, C) <-> (B, C, F, T); its own inverse"""
    return t.permute(0, 3, 2, 1).contiguous()


def bound(S, K, arith):
    return 2.0 * ((K + 1) * 2.0 ** -24 + C_SPLIT[arith] * 2.0 ** -22) * S


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ fp64 truths
def fwd_truth(x, w, b, relu=True):
    """y = ReLU(conv(x, w) + b) and S = conv(|x|, |w|) + |b|, both fp64 (B, T, F, Cout)"""
    xr, w64, b64 = ref(x.double()), w.double(), b.double()
    y = F.conv2d(xr, w64, b64, padding=1)
    S = F.conv2d(xr.abs(), w64.abs(), b64.abs(), padding=1)
    return ref(torch.relu(y) if relu else y), ref(S)


def windows(y):
    """(B, T, F, C) -> (B, T/2, F/2, C, 4): the candidates of every 2 x 2 floor-mode window at their codes 2 (f & 1) + (t & 1),
    which is also torch's scan order over the reference layout (F outer, T inner)"""
    B, T, Fq, C = y.shape
    Tp, Fp = T // 2, Fq // 2
    c = y[:, :2 * Tp, :2 * Fp].reshape(B, Tp, 2, Fp, 2, C)                       # [b, tp, t & 1, fp, f & 1, c]
    return torch.stack([c[:, :, 0, :, 0], c[:, :, 1, :, 0], c[:, :, 0, :, 1], c[:, :, 1, :, 1]], dim=-1)


def pool_first_max(y):
    """2 x 2 floor-mode max-pool with the code of the FIRST maximum in window order; any dtype (the device's fp32 output too)"""
    cand = windows(y)
    p = cand.max(dim=-1).values
    eq = cand == p.unsqueeze(-1)
    code = torch.where(eq[..., 0], 0, torch.where(eq[..., 1], 1, torch.where(eq[..., 2], 2, 3))).to(torch.uint8)
    return p, code


def pool_max(S):
    """the largest element of every window (the bound of a pooled element)"""
    return windows(S).max(dim=-1).values


def unique_max(y):
    """windows whose maximum occurs once"""
    cand = windows(y)
    return (cand == cand.max(dim=-1, keepdim=True).values).sum(-1) == 1


def unpool(dp, codes, T, Fq):
    """pooled (B, T/2, F/2, C) + codes -> dense (B, T, F, C); an odd last row / column stays zero"""
    B, Tp, Fp, C = dp.shape
    d = torch.zeros(B, Tp, 2, Fp, 2, C, dtype=dp.dtype)
    for code in range(4):
        d[:, :, code & 1, :, code >> 1] = torch.where(codes == code, dp, torch.zeros((), dtype=dp.dtype))
    out = torch.zeros(B, T, Fq, C, dtype=dp.dtype)
    out[:, :2 * Tp, :2 * Fp] = d.reshape(B, 2 * Tp, 2 * Fp, C)
    return out


def dgrad_truth(dy, w, act):
    """dx = conv_transpose(dy, w) gated by act > 0, from a DENSE dy (B, T, F, Cout) (un-pool first); S on |dy|, |w|.  fp64."""
    dyr, w64 = ref(dy.double()), w.double()
    gate = (act > 0).double()
    dx = ref(F.conv_transpose2d(dyr, w64, padding=1)) * gate
    S = ref(F.conv_transpose2d(dyr.abs(), w64.abs(), padding=1)) * gate
    return dx, S


def wgrad_truth(x, dy):
    """dw (Cout, Cin, 3, 3), its S, db (Cout), its S from a DENSE dy.  fp64."""
    xr, dyr = ref(x.double()), ref(dy.double())
    shape = (dy.shape[-1], x.shape[-1], 3, 3)
    dw = torch.nn.grad.conv2d_weight(xr, shape, dyr, padding=1)
    S = torch.nn.grad.conv2d_weight(xr.abs(), shape, dyr.abs(), padding=1)
    return dw, S, dy.double().sum((0, 1, 2)), dy.double().abs().sum((0, 1, 2))


# ------------------------------------------------------------------------------------------------ h2 emulation (CPU checks only)
H2_TERMS = ((0, 0), (0, 1), (1, 0))                                  # h h' + h l' + l h'; l l' is dropped


def h2_split(x):
    """x (fp32) -> (h, l, s): s the power of two that puts max|x| into [2^14, 2^15), h = fp16(x s), l = fp16(x s - h), as fp32"""
    m = float(x.abs().max())
    s = 2.0 ** (14 - math.floor(math.log2(m))) if m > 0 else 1.0
    xs = x * s
    h = xs.half().float()
    return h, (xs - h).half().float(), s


def fwd_h2_emul(x, w, b, terms=H2_TERMS):
    """ReLU(conv + b) with the h2 product: the listed piece products formed and summed in fp32, un-scaled exactly"""
    xh, xl, sx = h2_split(x)
    wh, wl, sw = h2_split(w)
    xp, wp = (ref(xh), ref(xl)), (wh, wl)
    acc = None
    for i, j in terms:
        t = F.conv2d(xp[i], wp[j], padding=1)
        acc = t if acc is None else acc + t
    return ref(torch.relu(acc * (1.0 / (sx * sw)) + b.view(1, -1, 1, 1)))


# ------------------------------------------------------------------------------------------------ the case table
# id: (kind, Cin, Cout, B, T, F); Cin / Cout are the FORWARD convolution's (a data gradient writes Cin channels)
CASES = {
    'P64': ('pool', 64, 64, 2, 18, 21),
    'R128': ('relu', 64, 128, 2, 33, 20),
    'P128': ('pool', 128, 128, 2, 17, 34),
    'D128p': ('dgrad_p', 128, 128, 2, 17, 35),
    'D128d': ('dgrad_d', 128, 128, 1, 33, 20),
    'MANY64': ('pool', 64, 64, 8, 256, 80),
    'MANY128': ('relu', 64, 128, 3, 96, 240),
}
ONE = [(kind, c, c, 1, T, Fq) for c in (64, 128)
       for kind, T, Fq in (('pool', 2, 2), ('relu', 1, 1), ('relu', 1, 17), ('dgrad_d', 1, 1), ('dgrad_d', 1, 17))]
TASK_CASES = ('P64', 'R128', 'P128', 'D128p')
WGRAD_EXTENTS = {'P64': (64, 64, 2, 18, 21), 'P128': (128, 128, 2, 17, 34), 'ONE': (64, 64, 1, 2, 2)}


def _seed(*key):
    return sum((i + 1) * 7919 * (hash(k) if not isinstance(k, str) else sum(map(ord, k))) for i, k in enumerate(key)) % (2 ** 31)


def corner_codes(am):
    """the four corner windows reach out to / away from the image border"""
    am[:, 0, 0], am[:, -1, -1], am[:, -1, 0], am[:, 0, -1] = 0, 3, 1, 2
    return am


@functools.lru_cache(maxsize=None)
def make_case(kind, cin, cout, B, T, Fq, nt=1, variant=''):
    """fp32 inputs of `nt` tasks of B samples (task k: its own weights / bias, operands 32^k larger) and the fp64 truths with their S.
    variant: '' | 'ZERO' (bias -10: every output is a ReLU zero) | 'CONST' (x one constant per channel over the image)."""
    g = torch.Generator().manual_seed(_seed(kind, cin, cout, B, T, Fq, nt, variant))
    n, Tp, Fp = nt * B, T // 2, Fq // 2
    w = torch.randn(nt, cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin) ** 0.5)
    scale = (32.0 ** torch.arange(nt)).repeat_interleave(B).view(n, 1, 1, 1)
    c = dict(kind=kind, w=w, nt=nt, B=B, T=T, F=Fq, cin=cin, cout=cout)
    if kind in ('relu', 'pool'):
        if variant == 'CONST':
            x = (torch.rand(cin, generator=g) + 0.5).expand(n, T, Fq, cin).contiguous()
        else:
            x = torch.relu(torch.randn(n, T, Fq, cin, generator=g))
            x[::B, 0, 0, 0] = 40.0                                       # every task's outlier, 10 x above its bulk
        x = x * scale
        b = torch.randn(nt, cout, generator=g) * 0.1 * (32.0 ** torch.arange(nt)).view(nt, 1)
        if variant == 'ZERO':
            b = torch.full((nt, cout), -10.0)
        ys = [fwd_truth(x[k * B:(k + 1) * B], w[k], b[k]) for k in range(nt)]
        c.update(x=x, b=b, y=torch.cat([y for y, _ in ys]), Sy=torch.cat([s for _, s in ys]))
        if kind == 'pool':
            c['p'], c['codes'] = pool_first_max(c['y'])
            c['Sp'] = pool_max(c['Sy'])
        return c
    act = torch.relu(torch.randn(n, T, Fq, cin, generator=g))
    if kind == 'dgrad_p':
        dy = torch.randn(n, Tp, Fp, cout, generator=g)
        am = corner_codes(torch.randint(0, 4, dy.shape, generator=g, dtype=torch.uint8))
    else:
        dy = torch.randn(n, T, Fq, cout, generator=g) * (torch.rand(n, T, Fq, cout, generator=g) > 0.5)
        am = None
    dy[::B, 0, 0, 0] = 40.0
    dy = dy * scale
    dense = unpool(dy, am, T, Fq) if am is not None else dy
    ds = [dgrad_truth(dense[k * B:(k + 1) * B], w[k], act[k * B:(k + 1) * B]) for k in range(nt)]
    c.update(act=act, dy=dy, am=am, dx=torch.cat([d for d, _ in ds]), Sdx=torch.cat([s for _, s in ds]))
    return c


@functools.lru_cache(maxsize=None)
def make_wgrad_case(cin, cout, B, T, Fq, nt, pooled):
    """x, a gradient with 30 % zeros (pooled: + arbitrary arg-max codes), task k's gradient 32^k larger; per task dw / db truths + S"""
    g = torch.Generator().manual_seed(_seed('wgrad', cin, cout, B, T, Fq, nt, pooled))
    n, Tp, Fp = nt * B, T // 2, Fq // 2
    x = torch.relu(torch.randn(n, T, Fq, cin, generator=g))
    dy = torch.randn((n, Tp, Fp, cout) if pooled else (n, T, Fq, cout), generator=g) * 1e-2
    dy[torch.rand(dy.shape, generator=g) < 0.3] = 0.0
    dy = dy * (32.0 ** torch.arange(nt)).repeat_interleave(B).view(n, 1, 1, 1)
    am = torch.randint(0, 4, dy.shape, generator=g, dtype=torch.uint8) if pooled else None
    dense = unpool(dy, am, T, Fq) if pooled else dy
    tr = [wgrad_truth(x[k * B:(k + 1) * B], dense[k * B:(k + 1) * B]) for k in range(nt)]
    return dict(x=x, dy=dy, am=am, dw=torch.stack([t[0] for t in tr]), Sdw=torch.stack([t[1] for t in tr]),
                db=torch.stack([t[2] for t in tr]), Sdb=torch.stack([t[3] for t in tr]))


# ------------------------------------------------------------------------------------------------ mutators (what a wrong kernel would give)
def mut_drop_tap(x, w, b, pix=(0, 1, 1), tap=(0, 2)):
    """the forward truth with ONE output pixel (b, t, f) computed without tap (kh, kw)"""
    y, _ = fwd_truth(x, w, b, relu=False)
    bi, t, f = pix
    kh, kw = tap
    tt, ff = t + kw - 1, f + kh - 1
    assert 0 <= tt < x.shape[1] and 0 <= ff < x.shape[2]
    y[bi, t, f] -= w[:, :, kh, kw].double() @ x[bi, tt, ff].double()
    return torch.relu(y)


def mut_neighbour_halo(x, w, b):
    """rows t = 0 of samples b >= 1 read the last row of sample b - 1 (its neighbour in memory) instead of the zero padding"""
    B, T, Fq, C = x.shape
    assert B > 1
    y, _ = fwd_truth(x, w, b)
    run, _ = fwd_truth(x.reshape(1, B * T, Fq, C), w, b)
    y[1:, 0] = run.view(B, T, Fq, -1)[1:, 0]
    return y


def mut_shift_windows(y):
    """pool windows taken one row late"""
    T = y.shape[1]
    return pool_first_max(y[:, 1:])[0][:, :T // 2 - 1], slice(0, T // 2 - 1)


def mut_swap_code_bits(codes):
    return ((codes & 1) << 1) | (codes >> 1)


def mut_odd_row_leaks(y):
    """T odd: the last window row also takes the row that has no window"""
    B, T, Fq, C = y.shape
    assert T & 1
    p = pool_first_max(y)[0].clone()
    extra = y[:, T - 1, :2 * (Fq // 2)].reshape(B, Fq // 2, 2, C).max(dim=2).values
    p[:, -1] = torch.maximum(p[:, -1], extra)
    return p


def mut_neighbour_bias(x, w, b_other):
    return fwd_truth(x, w, b_other)[0]
