"""Edge shapes of the HBM-bound kernels (csrc/mtl_elem.hip) against the fp64 / integer references of tests/elem_ref.py: scalar tails,
grid-stride wraps, every LayerNorm width, key lengths around the 64-lane trip, rows at every alignment, strided task slices, and the
h2 census pinned exactly on its threshold lines.

Conventions of every case: the reference is the same operation in fp64 from the fp32 values the kernel is given; integer / selection
outputs match bit for bit; every output lives inside a larger buffer pre-filled with NaN (0xA5 bytes) whose guards must survive;
every call runs twice and must repeat bit for bit; rejected arguments are asserted only where the entry point checks them before
launching.  Kernels without a reduction get a per-element bound counted from their roundings (e = 2^-24, half an ulp); kernels with
a reduction keep the norm-wise bars of tests/test_ops_gpu.py plus a per-element check measured against the plain torch fp32 op on the
same data (`ErrPair`: the kernel's largest element error against fp64 is at most 4 x torch's -- the factor allows for the other
summation tree; 2 ulp of the row's largest output where torch's error is exactly 0).  The figures in the docstrings are the ones
printed on an MI355X."""
import numpy as np
import pytest
import torch

from tests import elem_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096                      # elements in front of and behind every output (16 KiB of floats: keeps 16-byte alignment)
EINVAL = -22
E = 2.0 ** -24                    # one rounding to nearest: relative error of at most half an ulp
NAN_BITS = 0x7fc00000


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def dev(t):
    return t.cuda().contiguous()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """bit for bit (NaN payloads and signed zeros included)"""
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def all_nan_bits(t):
    return bool((bits(t.cpu().contiguous()) == NAN_BITS).all())


class Guarded:
    """n elements at offset GUARD + off of a device buffer pre-filled with NaN (floats), 0xA5 (bytes) or a sentinel (integers)"""

    def __init__(self, n, dtype=torch.float32, off=0, init=None):
        self.float = dtype.is_floating_point
        self.fill = float('nan') if self.float else (0xA5 if dtype == torch.uint8 else -0x5A5A5A5A)
        self.buf = torch.full((GUARD + off + n + GUARD,), self.fill, dtype=dtype).cuda()
        self.lo, self.n = GUARD + off, n
        self.v = self.buf[self.lo:self.lo + n]
        if init is not None:
            self.v.copy_(init.reshape(-1).to(dtype))

    @property
    def ptr(self):
        return self.v.data_ptr()

    def cpu(self):
        return self.v.cpu()

    def intact(self):
        b = self.buf.cpu()
        g = torch.cat([b[:self.lo], b[self.lo + self.n:]])
        return all_nan_bits(g) if self.float else bool((g == self.fill).all())


def ptr(g):
    return None if g is None else g.ptr


def ok(*gs):
    torch.cuda.synchronize()
    return all(g.intact() for g in gs if g is not None)


class ErrPair:
    """largest element error of the kernel and of the plain torch fp32 op against the same fp64 result, over everything add()ed"""

    def __init__(self, name):
        self.name, self.k, self.t, self.in_floor = name, 0.0, 0.0, True

    def add(self, got, ref64, t32):
        ref64 = ref64.double()
        ek = (got.double().cpu().reshape(ref64.shape) - ref64).abs()
        et = (t32.double().reshape(ref64.shape) - ref64).abs()
        assert not bool(torch.isnan(ek).any())
        self.k, self.t = max(self.k, float(ek.max())), max(self.t, float(et.max()))
        r2 = ref64.reshape(-1, ref64.shape[-1]) if ref64.dim() > 0 else ref64.reshape(1, 1)
        floor = torch.from_numpy(2 * np.spacing(r2.abs().max(1)[0].numpy().astype(np.float32)).astype(np.float64))
        self.in_floor = self.in_floor and bool((ek.reshape(r2.shape).max(1)[0] <= floor).all())
        return self

    def check(self):
        print('[elem] %s: kernel max|err| %.3e, torch fp32 max|err| %.3e' % (self.name, self.k, self.t))
        if self.t > 0:
            assert self.k <= 4 * self.t, (self.name, self.k, self.t)
        else:
            assert self.in_floor, (self.name, self.k)


def twice(fn):
    """run fn() (fresh outputs every time) twice: bit-for-bit repeatable; returns the first run's outputs"""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        if u is not None:
            assert same(u, v)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# 1. flat updates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, (1 << 21) + 1203])
def test_sgd_theta_prime_and_axpy_quads_tail_and_grid_wrap(L, n):
    """any n with 16-byte aligned pointers: n < 4 is tail only, 1027 and 2^21 + 1203 have n % 4 = 3, the last has more quads than
    2048 x 256 threads (grid-stride wrap).  theta - alpha g: fl(alpha g) errs by e |alpha g|, the subtraction by e (|theta| + |alpha g|)
    -> |got - ref| <= 2e (|theta| + |alpha g|), contracted to an FMA or not."""
    g = torch.Generator().manual_seed(n)
    th, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    alpha = 0.01
    dth, dgr = Guarded(n, init=th), Guarded(n, init=gr)

    def run():
        t1, y = Guarded(n), Guarded(n, init=th)
        assert L.mtl_sgd_theta_prime(st(), dth.ptr, dgr.ptr, alpha, t1.ptr, n) == 0
        assert L.mtl_axpy(st(), y.ptr, dgr.ptr, alpha, n) == 0
        assert ok(t1, y, dth, dgr)
        return t1.cpu(), y.cpu()
    t1, y = twice(run)
    p = R.f32(alpha) * gr.double()
    bound = 2 * E * (th.double().abs() + p.abs())
    assert bool(((t1.double() - (th.double() - p)).abs() <= bound).all())
    assert bool(((y.double() - (th.double() + p)).abs() <= bound).all())
    assert same(dth.cpu(), th) and same(dgr.cpu(), gr)
    out = Guarded(n)
    assert L.mtl_sgd_theta_prime(st(), dth.ptr + 4, dgr.ptr, alpha, out.ptr, n) == EINVAL
    assert L.mtl_sgd_theta_prime(st(), dth.ptr, dgr.ptr, alpha, out.ptr + 8, n) == EINVAL
    assert L.mtl_axpy(st(), out.ptr, dgr.ptr + 4, alpha, n) == EINVAL
    assert ok(out) and all_nan_bits(out.cpu())


@pytest.mark.parametrize('n', [1, 255, 257, (1 << 19) + 300 + 1])
def test_scale_host_and_device_coefficient_any_alignment(L, n):
    """y *= a is one rounding: |got - y a| <= e |y a|.  A non-null a_dev overrides a; pointers 4 bytes off a 16-byte boundary"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    a = 0.37
    coef = Guarded(1, init=torch.tensor([a]))
    for off in (0, 1):
        for use_dev in (False, True):
            def run():
                y = Guarded(n, off=off, init=x)
                assert L.mtl_scale(st(), y.ptr, 123.0 if use_dev else a, coef.ptr if use_dev else None, n) == 0
                assert ok(y, coef)
                return (y.cpu(),)
            y, = twice(run)
            ref = x.double() * R.f32(a)
            assert bool(((y.double() - ref).abs() <= E * ref.abs()).all())


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.875, 1 - 2.0 ** -9)])
@pytest.mark.parametrize('n', [1, 255, 257, (1 << 19) + 300 + 1])
def test_adam_step_first_and_late_steps(L, n, betas):
    """steps 1 and 1000 with non-zero m and v, elements with g = 0 (and with m = v = g = 0), theta / m / v 4 bytes off a 16-byte boundary.
    Reference: the fp64 formula of the kernel's header comment from the fp32 arguments.  Roundings (e = 2^-24, all positive terms in v):
      m' = fl(fl(m b1) + fl((1 - b1) g))                 |dm| <= 2e (|m b1| + |(1 - b1) g|)       (1 - b1 is exact in fp32: b1 >= 1/2)
      v' = fl(fl(v b2) + fl(fl((1 - b2) g) g))           |dv| <= e (2 v b2 + 3 (1 - b2) g^2) <= 3e v'
      denom = fl(fl(sqrt(v') / sqrt_bc2) + eps)          relative: 1.5e (v') + 0.5e (sqrt) + e (cast of sqrt_bc2) + e (divide) + e (add) = 5e
      u = fl(step fl(m' / denom)), step = fl(lr / bc1)   relative 2e (step: cast of bc1, divide) + e + e + 5e = 9e, plus step |dm| / denom
      theta' = fl(theta - u)                             |dtheta| <= e (|theta| + |u|) + 9e |u| + step |dm| / denom
    The second beta pair is exact in fp32, so torch.optim.Adam (Python-float betas) is given the same numbers; with the default pair
    torch's own result is further from the fp64 reference of the kernel's arguments ((1 - 0.999f) differs from 0.001 by 1.3e-5).
    MI355X, kernel / torch fp32 max|theta err| over both steps, n = 2^19 + 301: 2.36e-07 / 2.36e-07 (fp32-exact betas), 2.34e-07 / 7.87e-07
    (default betas); n = 255: 1.06e-07 / 1.06e-07 and 1.14e-07 / 1.24e-07; n = 1: 0 / 0."""
    g = torch.Generator().manual_seed(n)
    lr, (b1, b2), eps = 1e-3, betas, 1e-8
    th, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    v = torch.rand(n, generator=g)
    gr[::3] = 0.0
    m[::6] = 0.0
    v[::6] = 0.0
    dg = Guarded(n, init=gr)
    pair = ErrPair('adam theta n=%d betas=%s' % (n, betas))
    for step in (1, 1000):
        def run():
            w, dm, dv = Guarded(n, off=1, init=th), Guarded(n, off=1, init=m), Guarded(n, off=1, init=v)
            assert L.mtl_adam_step(st(), w.ptr, dg.ptr, dm.ptr, dv.ptr, step, lr, b1, b2, eps, n) == 0
            assert ok(w, dm, dv, dg)
            return w.cpu(), dm.cpu(), dv.cpu()
        w, m1, v1 = twice(run)
        t_ref, m_ref, v_ref, u, denom = R.adam(th, gr, m, v, step, lr, b1, b2, eps)
        fb1, fb2 = R.f32(b1), R.f32(b2)
        bm = 2 * E * ((m.double() * fb1).abs() + ((1 - fb1) * gr.double()).abs())
        bv = E * (2 * v.double() * fb2 + 3 * (1 - fb2) * gr.double() ** 2)
        bt = E * (th.double().abs() + 10 * u.abs()) + R.f32(lr) / (1 - fb1 ** step) * bm / denom
        assert bool(((m1.double() - m_ref).abs() <= bm).all())
        assert bool(((v1.double() - v_ref).abs() <= bv).all())
        assert bool(((w.double() - t_ref).abs() <= bt).all())
        assert same(w[::6], th[::6])                      # m = v = g = 0: the update is exactly zero
        p = th.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        p.grad = gr.clone()
        opt.step()
        pair.add(w, t_ref, p.detach())
    pair.check()
    assert L.mtl_adam_step(st(), dg.ptr, dg.ptr, dg.ptr, dg.ptr, 0, lr, b1, b2, eps, n) == EINVAL      # step < 1


@pytest.mark.parametrize('n', [4, 1028, 4 * ((1 << 20) + 77)])
def test_task_stack_updates_contiguous_and_strided(L, n):
    """3 tasks; the last n wraps a 4096-block grid.  theta' per task: the bound of the single-task kernel.  Sums: task-ascending, so
    the result is the fp32 left-to-right sum bit for bit (onto zero, or onto `out` when accumulating); the strided form reads slices
    task_stride = n + 52 apart and never the NaN between them."""
    nt, stride = 3, n + 52
    g = torch.Generator().manual_seed(n)
    th, gr = torch.randn(n, generator=g), torch.randn(nt, n, generator=g)
    out0 = torch.randn(n, generator=g)
    dth, dgr = Guarded(n, init=th), Guarded(nt * n, init=gr)
    stack = torch.full((nt, stride), float('nan'))
    stack[:, :n] = gr
    dstack = Guarded(nt * stride, init=stack)

    def run():
        t1 = Guarded(nt * n)
        assert L.mtl_sgd_theta_prime_tasks(st(), dth.ptr, dgr.ptr, 0.01, t1.ptr, n, nt) == 0
        outs = []
        for acc in (0, 1):
            a, b = Guarded(n, init=out0), Guarded(n, init=out0)
            assert L.mtl_sum_tasks(st(), a.ptr, dgr.ptr, n, nt, acc) == 0
            assert L.mtl_sum_tasks_strided(st(), b.ptr, dstack.ptr, n, nt, stride, acc) == 0
            assert ok(a, b)
            outs += [a.cpu(), b.cpu()]
        assert ok(t1, dth, dgr, dstack)
        return [t1.cpu()] + outs
    t1, s0, s0s, s1, s1s = twice(run)
    p = R.f32(0.01) * gr.double()
    assert bool(((t1.view(nt, n).double() - (th.double() - p)).abs() <= 2 * E * (th.double().abs() + p.abs())).all())
    want0, want1 = torch.zeros(n), out0.clone()
    for t in range(nt):
        want0, want1 = want0 + gr[t], want1 + gr[t]
    assert same(s0, want0) and same(s0s, want0) and same(s1, want1) and same(s1s, want1)
    assert same(dstack.cpu().view(nt, stride), stack)                              # slices and the gaps between them untouched
    o = Guarded(n)
    assert L.mtl_sum_tasks_strided(st(), o.ptr, dstack.ptr, n, nt, n - 4, 0) == EINVAL         # task_stride < n
    assert L.mtl_sum_tasks_strided(st(), o.ptr, dstack.ptr, n, nt, stride + 1, 0) == EINVAL    # task_stride % 4
    assert L.mtl_sum_tasks_strided(st(), o.ptr, dstack.ptr, n + 1, nt, stride, 0) == EINVAL    # n % 4
    assert L.mtl_sum_tasks_strided(st(), o.ptr + 4, dstack.ptr, n, nt, stride, 0) == EINVAL    # alignment
    assert L.mtl_sum_tasks(st(), o.ptr, dgr.ptr + 8, n, nt, 0) == EINVAL
    assert L.mtl_sgd_theta_prime_tasks(st(), dth.ptr, dgr.ptr, 0.01, o.ptr, n + 2, nt) == EINVAL
    assert L.mtl_sgd_theta_prime_tasks(st(), dth.ptr, dgr.ptr + 4, 0.01, o.ptr, n, nt) == EINVAL
    assert ok(o) and all_nan_bits(o.cpu())


@pytest.mark.parametrize('n', [1, 2047, 2049, (1 << 21) + 1203])
def test_sumsq_and_clip_coefficient(L, n):
    """mode 0 (sum of squares) and mode 2 (clip coefficient) on four independent vectors per n (2047 / 2049: one and two partial blocks;
    the last n: the 1024-block cap, nine grid-stride trips).  Norm-wise bar from the depth of the fixed summation tree, all terms
    positive: 9 trips x (square, add) + 6 + 3 in stage 1, 4 + 6 + 3 in stage 2 = 40 roundings -> 40 e relative.  A norm below `arg`
    gives exactly 1.0f; above it the coefficient is within the project's 1e-6 of fp64, and mtl_scale(a_dev = coef) then equals
    clip_grad_norm_ in fp64 within |x| 1e-6 + e |ref| per element.
    MI355X, kernel / torch fp32 max|err| of the four sums: n=1 6.99e-08 / 6.99e-08, n=2047 1.14e-03 / 1.14e-03, n=2049 1.52e-03 / 1.51e-03,
    n=2^21+1203 1.49 / 2.15 (sums of 1.9e7: one ulp is 2)."""
    g = torch.Generator().manual_seed(n)
    draws = 4
    xs = torch.randn(draws, n, generator=g) * 3
    ws = Guarded(1024)
    got, pair = [], ErrPair('sumsq n=%d' % n)
    for i in range(draws):
        dx = Guarded(n, init=xs[i])

        def run():
            s, c1, c2 = Guarded(1), Guarded(1), Guarded(1)
            norm = float(xs[i].double().norm())
            assert L.mtl_sumsq(st(), dx.ptr, n, s.ptr, ws.ptr, 0, 0.0) == 0
            assert L.mtl_sumsq(st(), dx.ptr, n, c1.ptr, ws.ptr, 2, 10 * norm) == 0
            assert L.mtl_sumsq(st(), dx.ptr, n, c2.ptr, ws.ptr, 2, 0.37 * norm) == 0
            y = Guarded(n, init=xs[i])
            assert L.mtl_scale(st(), y.ptr, 123.0, c2.ptr, n) == 0
            assert ok(s, c1, c2, y, dx, ws)
            return s.cpu(), c1.cpu(), c2.cpu(), y.cpu()
        s, c1, c2, y = twice(run)
        x64 = xs[i].double()
        ss = float((x64 * x64).sum())
        assert abs(float(s) - ss) <= 40 * E * ss
        assert float(c1) == 1.0
        arg = R.f32(0.37 * float(x64.norm()))
        coef = min(1.0, arg / (ss ** 0.5 + 1e-6))
        assert abs(float(c2) - coef) < 1e-6
        p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
        p.grad = x64.clone()
        torch.nn.utils.clip_grad_norm_([p], arg)
        assert bool(((y.double() - p.grad).abs() <= x64.abs() * 1e-6 + E * p.grad.abs()).all())
        got.append(s)
    pair.add(torch.cat(got), (xs.double() ** 2).sum(1), (xs * xs).sum(1)).check()


# ---------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _ln_case(seed, rows, d, T, groups=1, rpg=None, absent=(), p_drop=0.25):
    g = torch.Generator().manual_seed(seed)
    c = dict(rows=rows, d=d, T=T, rpg=rpg or rows, groups=groups, eps=1e-5)
    c['x'], c['res'], c['dy'] = (torch.randn(rows, d, generator=g) for _ in range(3))
    c['gamma'], c['beta'] = torch.randn(groups, d, generator=g), torch.randn(groups, d, generator=g)
    c['pe'] = torch.randn(T, d, generator=g)
    c['keep'] = (torch.rand(rows, generator=g) > 0.3).int()
    c['keep'][0] = 1
    c['xmask'] = (torch.rand(rows, d, generator=g) >= p_drop).to(torch.uint8)
    c['xscale'] = R.f32(1 / (1 - p_drop))
    c['dsum'] = c['dz2'] = True
    for k in absent:
        c[k] = None
    if c['xmask'] is None:
        c['xscale'] = 1.0
    return c


def _ln_ref(c, **kw):
    return R.layernorm(c['x'], c['res'], c['gamma'], c['beta'], c['pe'], c['keep'], c['xmask'], c['xscale'], c['T'], c['eps'], c['rpg'],
                       c['dy'], **kw)


def _ln_launch(L, c, grouped, defer, g0):
    """forward + backward of one case.  Parameters are packed like a flat buffer (gamma of group t at t sP, beta at t sP + d), gradients
    at t sG (+ d, + 2 d) on top of the non-zero g0.  Returns (table entries of the deferred reduction, finish() -> outputs on the CPU)"""
    rows, d, G, rpg = c['rows'], c['d'], c['groups'], c['rpg']
    sP, sG = 2 * d + 8, 3 * d + 4
    params = torch.full((G, sP), float('nan'))
    params[:, :d], params[:, d:2 * d] = c['gamma'], c['beta']
    opt = lambda k, dt=torch.float32: None if c[k] is None else Guarded(c[k].numel(), dtype=dt, init=c[k])
    dpar, dx, dres, dpe, ddy = Guarded(G * sP, init=params), opt('x'), opt('res'), opt('pe'), opt('dy')
    dkeep, dmask = opt('keep', torch.int32), opt('xmask', torch.uint8)
    y, xhat, rstd, dz = Guarded(rows * d), Guarded(rows * d), Guarded(rows), Guarded(rows * d)
    dzm = Guarded(rows * d) if dmask is not None else None
    dz2 = Guarded(rows * d) if c['dz2'] else None
    grads = Guarded(G * sG, init=g0)
    head = (st(), dx.ptr, ptr(dres), dpar.ptr, dpar.ptr + 4 * d, ptr(dpe), ptr(dkeep), ptr(dmask), c['xscale'], y.ptr, xhat.ptr, rstd.ptr,
            rows, d, c['T'], c['eps'])
    if grouped:
        assert L.mtl_layernorm_fwd_g(*head, rpg, sP) == 0
        nbytes = L.mtl_layernorm_bwd_g_workspace(rows, d, rpg)
    else:
        assert L.mtl_layernorm_fwd(*head) == 0
        nbytes = L.mtl_layernorm_bwd_workspace(rows, d)
    ws = Guarded(nbytes // 4)
    gp = grads.ptr
    back = (st(), ddy.ptr, xhat.ptr, rstd.ptr, dpar.ptr, ptr(dkeep), ptr(dmask), c['xscale'], dz.ptr, ptr(dzm), ptr(dz2), gp, gp + 4 * d,
            gp + 8 * d if c['dsum'] else None, ws.ptr, rows, d, 1 if defer else 0)
    if grouped:
        assert L.mtl_layernorm_bwd_g(*back, rpg, sP, sG) == 0
        nw = L.mtl_layernorm_bwd_g_waves(rpg)
    else:
        assert L.mtl_layernorm_bwd(*back) == 0
        nw = nbytes // (3 * d * 4)
    entries = [dict(part=ws.ptr + 4 * t * nw * 3 * d, dgamma=gp + 4 * t * sG, dbeta=gp + 4 * (t * sG + d),
                    dsum=gp + 4 * (t * sG + 2 * d) if c['dsum'] else None, nw=nw, d=d) for t in range(G)]
    held = [dpar, dx, dres, dpe, ddy, dkeep, dmask, y, xhat, rstd, dz, dzm, dz2, grads, ws]

    def finish():
        assert ok(*held)
        gr = grads.cpu().view(G, sG)
        assert same(gr[:, 3 * d:], g0.view(G, sG)[:, 3 * d:])                     # the floats between two groups' gradients
        cpu = lambda t: None if t is None else t.cpu()
        return dict(y=y.cpu().view(rows, d), xhat=xhat.cpu().view(rows, d), rstd=rstd.cpu(), dz=dz.cpu().view(rows, d),
                    dzm=None if dzm is None else dzm.cpu().view(rows, d), dz2=None if dz2 is None else dz2.cpu().view(rows, d),
                    dgamma=gr[:, :d], dbeta=gr[:, d:2 * d], dsum=gr[:, 2 * d:3 * d])
    return entries, finish


def _ln_reduce(L, entries, dmax):
    from mtl_amd import _lib
    table = (_lib.LnReduceDesc * len(entries))()
    for t, e in enumerate(entries):
        table[t].part, table[t].dgamma, table[t].dbeta, table[t].dsum, table[t].nw, table[t].d = (e['part'], e['dgamma'], e['dbeta'],
                                                                                                  e['dsum'], e['nw'], e['d'])
    tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    assert L.mtl_ln_param_reduce_batch(st(), tdev.data_ptr(), len(entries), dmax) == 0
    torch.cuda.synchronize()


def _ln_run(L, c, grouped=False, defer=0, seed=0):
    G, d = c['groups'], c['d']
    g0 = torch.randn(G * (3 * d + 4), generator=torch.Generator().manual_seed(1000 + seed))

    def run():
        entries, finish = _ln_launch(L, c, grouped, defer, g0)
        if defer:
            torch.cuda.synchronize()
            _ln_reduce(L, entries, d)
        o = finish()
        return [o[k] for k in ('y', 'xhat', 'rstd', 'dz', 'dzm', 'dz2', 'dgamma', 'dbeta', 'dsum')]
    o = dict(zip(('y', 'xhat', 'rstd', 'dz', 'dzm', 'dz2', 'dgamma', 'dbeta', 'dsum'), twice(run)))
    o['g0'] = g0.view(G, 3 * d + 4)
    return o


def _ln_check(c, o, pairs):
    """norm-wise bars of tests/test_ops_gpu.py (y 2e-6, gradients 1e-5) against fp64 autograd; exact zeros on keep = 0 rows; element
    errors into `pairs` (y, dz, dgamma, dbeta, dsum) against the plain torch fp32 op"""
    d = c['d']
    ref, t32 = _ln_ref(c), _ln_ref(c, dtype=torch.float32, builtin=True)
    g0 = o['g0']
    assert rel(o['y'], ref['y']) < 2e-6 and rel(o['xhat'], ref['xhat']) < 2e-6 and rel(o['rstd'], ref['rstd']) < 2e-6
    assert rel(o['dz'], ref['dz']) < 1e-5
    if c['xmask'] is not None:
        assert rel(o['dzm'], ref['dx']) < 1e-5
        assert float(o['dzm'][c['xmask'] == 0].abs().max() if bool((c['xmask'] == 0).any()) else 0.0) == 0.0
    if c['dz2']:
        assert same(o['dz2'], o['dz'])
    if c['keep'] is not None and bool((c['keep'] == 0).any()):
        dead = c['keep'] == 0
        assert float(o['y'][dead].abs().max()) == 0.0 and float(o['dz'][dead].abs().max()) == 0.0
    assert rel(o['dgamma'], g0[:, :d].double() + ref['dgamma']) < 1e-5 and rel(o['dbeta'], g0[:, d:2 * d].double() + ref['dbeta']) < 1e-5
    pairs['y'].add(o['y'], ref['y'], t32['y'])
    pairs['dz'].add(o['dz'], ref['dz'], t32['dz'])
    pairs['dgamma'].add(o['dgamma'], g0[:, :d].double() + ref['dgamma'], g0[:, :d] + t32['dgamma'])
    pairs['dbeta'].add(o['dbeta'], g0[:, d:2 * d].double() + ref['dbeta'], g0[:, d:2 * d] + t32['dbeta'])
    if c['dsum']:
        assert rel(o['dsum'], g0[:, 2 * d:3 * d].double() + ref['dsum']) < 1e-5
        pairs['dsum'].add(o['dsum'], g0[:, 2 * d:3 * d].double() + ref['dsum'], g0[:, 2 * d:3 * d] + t32['dsum'])
    else:
        assert same(o['dsum'], g0[:, 2 * d:3 * d])


def _ln_pairs(tag):
    return {k: ErrPair('layernorm %s %s' % (k, tag)) for k in ('y', 'dz', 'dgamma', 'dbeta', 'dsum')}


@pytest.mark.parametrize('rows', [1, 3, 4, 5, 9])
@pytest.mark.parametrize('d', [64, 128, 256, 512, 1024])
def test_layernorm_every_width_and_row_count(L, d, rows):
    """all five instantiations (d = 256 and 1024 read 16-byte quads, the others single columns), row counts around the 4 waves of a
    workgroup and the 4 rows of a backward wave, every optional input present, T = 1 (odd row counts) and T > rows.
    MI355X, largest kernel / torch fp32 max|err| over the 25 cases: y 1.07e-06 / 1.44e-06, dz 7.72e-07 / 6.59e-07, dgamma 1.32e-06 / 1.28e-06,
    dbeta 8.05e-07 / 8.05e-07, dsum 1.21e-06 / 1.19e-06; worst ratio within one case 1.84 (dz, d = 128, rows = 9)."""
    c = _ln_case(d + rows, rows, d, T=1 if rows % 2 else rows + 2)
    pairs = _ln_pairs('d=%d rows=%d' % (d, rows))
    _ln_check(c, _ln_run(L, c, seed=d + rows), pairs)
    for p in pairs.values():
        p.check()
    bad = dict(c, d=96)
    o = Guarded(rows * d)
    assert L.mtl_layernorm_fwd(st(), o.ptr, None, o.ptr, o.ptr, None, None, None, 1.0, o.ptr, o.ptr, o.ptr, rows, bad['d'], 1, 1e-5) == EINVAL
    assert L.mtl_layernorm_bwd(st(), o.ptr, o.ptr, o.ptr, o.ptr, None, None, 1.0, o.ptr, None, None, o.ptr, o.ptr, None, o.ptr, rows, 2048,
                               0) == EINVAL
    assert ok(o) and all_nan_bits(o.cpu())


@pytest.mark.parametrize('d', [128, 256])
@pytest.mark.parametrize('absent', ['res', 'pe', 'keep', 'xmask', 'dsum', 'dz2'])
def test_layernorm_each_optional_input_absent_once(L, absent, d):
    """rows = 5, T = 7 > rows; without `dsum` its slot of the gradient buffer stays bit for bit.
    MI355X, largest kernel / torch fp32 max|err| over the 12 cases: y 6.94e-07 / 9.62e-07, dz 7.49e-07 / 7.49e-07, dgamma 9.71e-07 / 9.71e-07,
    dbeta 6.71e-07 / 6.71e-07, dsum 9.53e-07 / 1.06e-06; worst ratio within a case 1.97 (dz, d = 256, without pe)."""
    c = _ln_case(d + len(absent), 5, d, T=7, absent=(absent,))
    pairs = _ln_pairs('d=%d without %s' % (d, absent))
    _ln_check(c, _ln_run(L, c, seed=d), pairs)
    for p in pairs.values():
        p.check()


@pytest.mark.parametrize('d', [64, 256])
def test_layernorm_constant_offset_and_dead_rows(L, d):
    """row 0 constant (its sums are exact in fp32): xhat exactly 0 and rstd = 1 / sqrt(eps) within two roundings; row 1 = 1000 + k / 8 with
    small integers k (mean 1e3, variance ~1, sums exact in fp32: E[x^2] - mean^2 would lose every digit of the variance); row 2 has
    keep = 0: y and dz exactly 0 and nothing of it in dgamma / dbeta.  The gradient of the constant row is rstd (g - mean g) with
    g = dy gamma -- not zero -- and is checked against fp64 like every other row.
    MI355X, largest kernel / torch fp32 max|err| of both widths: y 5.67e-07 / 2.79e-05, dz 2.27e-04 / 2.27e-04 (the constant row: rstd = 316),
    dgamma 8.03e-07 / 2.49e-05, dbeta 4.17e-07 / 4.17e-07, dsum 4.54e-04 / 4.54e-04."""
    c = _ln_case(d, 5, d, T=7, absent=('res', 'xmask'))
    g = torch.Generator().manual_seed(7)
    c['x'][0] = 1.5
    c['x'][1] = 1000 + torch.round(8 * torch.randn(d, generator=g)).clamp(-24, 24) / 8
    c['keep'] = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
    pairs = _ln_pairs('d=%d special rows' % d)
    o = _ln_run(L, c, seed=d)
    _ln_check(c, o, pairs)
    for p in pairs.values():
        p.check()
    ref = _ln_ref(c)
    assert float(o['xhat'][0].abs().max()) == 0.0
    r0 = 1 / R.f32(1e-5) ** 0.5
    assert abs(float(o['rstd'][0]) - r0) <= 2 * E * r0
    for r in (0, 1):
        assert rel(o['y'][r], ref['y'][r]) < 2e-6 and rel(o['dz'][r], ref['dz'][r]) < 1e-5 and rel(o['xhat'][r], ref['xhat'][r]) < 2e-6
    live = dict(c, x=c['x'][[0, 1, 3, 4]], dy=c['dy'][[0, 1, 3, 4]], keep=None, pe=None, rows=4, rpg=4)       # the dead row left out
    lref = _ln_ref(live)
    assert rel(o['dgamma'], o['g0'][:, :d].double() + lref['dgamma']) < 1e-5 and rel(o['dbeta'], o['g0'][:, d:2 * d].double() + lref['dbeta']) < 1e-5


def test_layernorm_deferred_reduction_of_two_widths_in_one_table(L):
    """d = 64 (9 rows) and d = 1024 (5 rows) leave their partials in their workspaces; ONE mtl_ln_param_reduce_batch with dmax = 1024 adds
    both (the blocks of columns >= 64 skip the narrow entry); the d = 1024 entry has no dsum.  Bit for bit the immediate reduction.
    MI355X, kernel / torch fp32 max|err|: y 9.58e-07 / 1.20e-06, dz 4.92e-07 / 3.46e-07, dgamma 1.19e-06 / 1.19e-06, dbeta 4.47e-07 / 4.47e-07,
    dsum 5.61e-07 / 3.43e-07."""
    ca, cb = _ln_case(1, 9, 64, T=1), _ln_case(2, 5, 1024, T=7, absent=('dsum',))
    now = [_ln_run(L, c, seed=i) for i, c in enumerate((ca, cb))]
    launched = [_ln_launch(L, c, False, 1, o['g0'].reshape(-1)) for c, o in zip((ca, cb), now)]
    torch.cuda.synchronize()
    before = [fin() for _, fin in launched]
    for b, o in zip(before, now):
        assert same(b['dgamma'], o['g0'][:, :b['dgamma'].shape[1]]) and same(b['dz'], o['dz'])      # deferred: nothing added yet
    _ln_reduce(L, launched[0][0] + launched[1][0], 1024)
    for (_, fin), o in zip(launched, now):
        after = fin()
        for k in ('dgamma', 'dbeta', 'dsum'):
            assert same(after[k], o[k]), k
    pairs = _ln_pairs('deferred')
    for c, o in zip((ca, cb), now):
        _ln_check(c, o, pairs)
    for p in pairs.values():
        p.check()


@pytest.mark.parametrize('defer', [0, 1])
@pytest.mark.parametrize('rpg', [1, 5, 7])
@pytest.mark.parametrize('d', [64, 256])
def test_layernorm_groups_with_a_short_last_group(L, d, rpg, defer):
    """rows = 3 rpg - 2: the last group is short (one group of one row for rpg = 1); group t reads gamma / beta at t sParam and adds
    its gradients at t sGrad (both non-zero), immediately or through the deferred table; against per-group fp64 autograd.
    MI355X, largest kernel / torch fp32 max|err| over the 12 cases: y 1.22e-06 / 1.02e-06, dz 5.60e-07 / 4.02e-07 (worst ratio within a case
    2.35: d = 64, rpg = 5), dgamma 1.03e-06 / 1.26e-06, dbeta 5.96e-07 / 9.39e-07, dsum 1.24e-06 / 1.12e-06."""
    rows = 3 * rpg - 2
    groups = (rows + rpg - 1) // rpg
    c = _ln_case(d + rpg, rows, d, T=4, groups=groups, rpg=rpg)
    pairs = _ln_pairs('d=%d rpg=%d defer=%d' % (d, rpg, defer))
    _ln_check(c, _ln_run(L, c, grouped=True, defer=defer, seed=rpg), pairs)
    for p in pairs.values():
        p.check()


# ---------------------------------------------------------------------------------------------------------------------
# 3. masked softmax
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_run(L, s, klen, causal, scale, ld, dp, drop=None):
    """S / dP / Pd rows of ld floats with NaN in the columns [Tk, ld).  Returns P, dS (and Pd with dropout) as (B, H, Tq, ld) on the CPU"""
    B, H, Tq, Tk = s.shape
    rows = B * H * Tq
    pad = lambda t: torch.cat([t, torch.full((B, H, Tq, ld - Tk), float('nan'))], -1) if ld > Tk else t
    dk = None if klen is None else Guarded(B, dtype=torch.int32, init=torch.tensor(klen, dtype=torch.int32))
    mask = None
    if drop is not None:
        mask = Guarded(rows * ld, dtype=torch.uint8)
        seed = torch.tensor([99], dtype=torch.int64).cuda()
        assert L.mtl_dropout_mask(st(), mask.ptr, rows * ld, drop, seed.data_ptr(), 3 << 40) == 0

    def run():
        S, D = Guarded(rows * ld, init=pad(s)), Guarded(rows * ld, init=pad(dp))
        Pd = Guarded(rows * ld) if mask is not None else None
        psc = 1.0 if drop is None else 1 / (1 - drop)
        assert L.mtl_softmax_mask_fwd(st(), S.ptr, ptr(dk), causal, scale, B, H, Tq, Tk, ld, ptr(mask), psc, ptr(Pd)) == 0
        assert L.mtl_softmax_bwd(st(), S.ptr, D.ptr, scale, rows, Tk, ld, ptr(mask), psc) == 0
        assert ok(S, D, Pd, dk, mask)
        v = lambda t: None if t is None else t.cpu().view(B, H, Tq, ld)
        return v(S), v(D), v(Pd)
    P, D, Pd = twice(run)
    for t in (P, D, Pd):
        if t is not None and ld > Tk:
            assert all_nan_bits(t[..., Tk:])                   # the padding columns of every row survive
    return P, D, Pd, (None if mask is None else mask.cpu().view(B, H, Tq, ld))


@pytest.mark.parametrize('ldk', ['Tk', 'up4', 'Tk+5'])
@pytest.mark.parametrize('Tk', [1, 63, 64, 65, 130])
def test_softmax_key_lengths_around_the_lane_trip_and_every_row_alignment(L, Tk, ldk):
    """Tk around one and two trips of the 64-lane loop, ld = Tk / Tk rounded up to 4 / Tk + 5 (rows then start at every alignment),
    (B, H, Tq) = (3, 2, 5): 30 rows, not a multiple of the 4 waves.  Masks: none; klen = 1, Tk, Tk + 7 (clamped to Tk); causal with
    Tq = Tk.  Scale 1 with sample 0 at randn x 3 and the others uniform in [-80, 80]: without the max subtraction exp overflows.
    Masked probabilities are exactly 0, live rows sum to 1 within 1e-6.
    MI355X, largest kernel / torch fp32 max|err| over the 15 cases: forward 2.50e-07 / 2.05e-07 (worst ratio within a case 1.73), backward
    3.59e-07 / 4.00e-07 (1.31)."""
    ld = {'Tk': Tk, 'up4': (Tk + 3) // 4 * 4, 'Tk+5': Tk + 5}[ldk]
    g = torch.Generator().manual_seed(Tk * 8 + ld)
    fwd, bwd = ErrPair('softmax fwd Tk=%d ld=%d' % (Tk, ld)), ErrPair('softmax bwd Tk=%d ld=%d' % (Tk, ld))
    for klen, causal, Tq in ((None, 0, 5), ([1, Tk, Tk + 7], 0, 5), ([Tk, max(Tk // 2, 1), Tk + 7], 1, Tk)):
        B, H = 3, 2
        s = (torch.rand(B, H, Tq, Tk, generator=g) * 2 - 1) * 80
        s[0] = torch.randn(H, Tq, Tk, generator=g) * 3
        dp = torch.randn(B, H, Tq, Tk, generator=g)
        P, D, _, _ = _softmax_run(L, s, klen, causal, 1.0, ld, dp)
        P, D = P[..., :Tk], D[..., :Tk]
        lim = R.softmax_limits(B, H, Tq, Tk, klen, causal)
        live = torch.arange(Tk) < lim.unsqueeze(-1)
        ref = R.softmax_fwd(s, 1.0, lim)
        assert rel(P, ref) < 2e-6
        assert float(P[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0 and float(D[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0
        assert float((P.double().sum(-1) - 1).abs().max()) < 1e-6
        dref = R.softmax_bwd(P, dp, 1.0)                       # from the fp32 probabilities the backward kernel is given
        assert rel(D, dref) < 1e-5
        p32 = torch.softmax(s.masked_fill(~live, -np.inf), -1)
        fwd.add(P, ref, p32)
        bwd.add(D, dref, R.softmax_bwd(P, dp, 1.0, dtype=torch.float32))
    fwd.check()
    bwd.check()
    o = Guarded(64)
    assert L.mtl_softmax_mask_fwd(st(), o.ptr, None, 0, 1.0, 1, 1, 1, 8, 7, None, 1.0, None) == EINVAL            # ld < Tk
    assert L.mtl_softmax_bwd(st(), o.ptr, o.ptr, 1.0, 1, 8, 7, None, 1.0) == EINVAL
    assert ok(o) and all_nan_bits(o.cpu())


@pytest.mark.parametrize('Tk,ld,causal', [(65, 70, 0), (130, 132, 1)])
def test_softmax_dropout_copy_is_exact_and_leaves_P_alone(L, Tk, ld, causal):
    """the dropout form: Pd is exactly P pscale (one fp32 product) where the mask keeps and 0 where it drops, S is bit for bit the run
    without dropout, the backward takes dP through the same mask.
    MI355X, kernel / torch fp32 max|err| of the backward: at most 1.95e-08 / 1.95e-08 (Tk = 130)."""
    B, H, Tq, p = 3, 2, Tk if causal else 5, 0.3
    g = torch.Generator().manual_seed(Tk)
    s, dp = torch.randn(B, H, Tq, Tk, generator=g) * 3, torch.randn(B, H, Tq, Tk, generator=g)
    klen = [Tk, 7, Tk + 7]
    P0, D0, _, _ = _softmax_run(L, s, klen, causal, 0.25, ld, dp)
    P, D, Pd, mask = _softmax_run(L, s, klen, causal, 0.25, ld, dp, drop=p)
    assert same(P, P0)
    assert rel(P[..., :Tk], R.softmax_fwd(s, 0.25, R.softmax_limits(B, H, Tq, Tk, klen, causal))) < 2e-6
    keep = mask[..., :Tk] != 0
    psc = torch.tensor(1 / (1 - p), dtype=torch.float32)
    assert same(Pd[..., :Tk], torch.where(keep, P[..., :Tk] * psc, torch.zeros(())))
    assert 0.5 < float(keep.float().mean()) < 0.9
    dref = R.softmax_bwd(P[..., :Tk], dp, 0.25, keep=keep, pscale=float(psc))
    assert rel(D[..., :Tk], dref) < 1e-5
    ErrPair('softmax bwd with dropout Tk=%d' % Tk).add(D[..., :Tk], dref, R.softmax_bwd(P[..., :Tk], dp, 0.25, keep=keep, pscale=psc,
                                                                                     dtype=torch.float32)).check()


def test_softmax_sample_without_a_live_key_gives_zero_rows(L):
    """klen = 0: the kernel writes an all-zero row where torch.softmax of an all -inf row gives NaN (include/mtl_hip.h pins it); no NaN or
    inf anywhere in the valid columns, and the backward of such a row is zero too"""
    B, H, Tq, Tk, ld = 3, 2, 5, 65, 68
    g = torch.Generator().manual_seed(0)
    s, dp = torch.randn(B, H, Tq, Tk, generator=g) * 3, torch.randn(B, H, Tq, Tk, generator=g)
    klen = [0, Tk, 3]
    P, D, _, _ = _softmax_run(L, s, klen, 0, 0.25, ld, dp)
    P, D = P[..., :Tk], D[..., :Tk]
    assert float(P[0].abs().max()) == 0.0 and float(D[0].abs().max()) == 0.0
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(D).all())
    ref = R.softmax_fwd(s, 0.25, R.softmax_limits(B, H, Tq, Tk, klen, 0))
    assert rel(P, ref) < 2e-6 and rel(D, R.softmax_bwd(P, dp, 0.25)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 4. cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def _ce_forward(L, flat_dev, gold_dev, rows, V, ld, smoothing, nn_):
    def run():
        lse, hyp, rowloss, loss = Guarded(rows), Guarded(rows, dtype=torch.int64), Guarded(rows), Guarded(1)
        assert L.mtl_ce_argmax_fwd(st(), flat_dev.ptr, gold_dev.ptr, rows, V, ld, 0, smoothing, nn_, None, lse.ptr, hyp.ptr, rowloss.ptr,
                                   loss.ptr) == 0
        assert ok(lse, hyp, rowloss, loss, flat_dev, gold_dev)
        return lse.cpu(), hyp.cpu(), rowloss.cpu(), loss.cpu()
    return twice(run)


def _ce_logits(g, rows, V, ld, off=0):
    """(rows, V) logits in a flat buffer of row stride ld that ENDS with the last valid logit (NaN guards behind and in front), a
    zeroed row 1 (every logit ties) and a tie between the last element and an early one in row 2"""
    logits = torch.randn(rows, V, generator=g)
    logits[1] = 0.0
    if V > 4 and rows > 2:
        logits[2, V - 1] = logits[2, 3] = logits[2].max() + 1.0
    flat = torch.cat([logits, torch.full((rows, ld - V), float('nan'))], 1).reshape(-1)[:rows * ld - (ld - V)]
    gold = torch.randint(1, V, (rows,), generator=g)
    gold[1] = 0
    return logits, Guarded(flat.numel(), off=off, init=flat), gold


@pytest.mark.parametrize('V,ld,rows', [(3765, 3765, 37), (5, 5, 9), (64, 67, 11), (1000, 1000, 13), (4093, 4093, 6), (4094, 4096, 5), (5000, 5003, 7)])
def test_ce_backward_row_widths_strides_and_smoothing(L, V, ld, rows):
    """mtl_ce_bwd at the (V, ld, rows) list of the forward's alignment test, ldd = V and V + 3 (gradient rows at every alignment, their
    columns [V, ldd) untouched), smoothing 0 and 0.1, gscale_dev null and non-null, a pad row (exact zeros); against fp64 autograd of
    the smoothing formula, 1e-5 norm-wise.
    MI355X, largest kernel / torch fp32 max|err| over the 7 cases: 3.66e-09 / 3.06e-09, worst ratio within a case 1.56 (V = 5)."""
    g = torch.Generator().manual_seed(V + ld)
    logits, dflat, gold = _ce_logits(g, rows, V, ld)
    dgold = Guarded(rows, dtype=torch.int64, init=gold)
    nn_ = int((gold != 0).sum())
    lse, hyp, _, _ = _ce_forward(L, dflat, dgold, rows, V, ld, 0.0, nn_)
    dlse = Guarded(rows, init=lse)
    gsc, gdv = (1.0 / 3) / nn_, 0.37
    gdev = Guarded(1, init=torch.tensor([gdv]))
    pair = ErrPair('ce bwd V=%d ld=%d' % (V, ld))
    for ldd in (V, V + 3):
        for smoothing in (0.0, 0.1):
            for use_dev in (False, True):
                def run():
                    d = Guarded(rows * ldd)
                    assert L.mtl_ce_bwd(st(), dflat.ptr, dlse.ptr, dgold.ptr, rows, V, ld, 0, smoothing, gsc, gdev.ptr if use_dev else None,
                                        d.ptr, ldd) == 0
                    assert ok(d, dflat, dlse, dgold, gdev)
                    return (d.cpu().view(rows, ldd),)
                d, = twice(run)
                if ldd > V:
                    assert all_nan_bits(d[:, V:])
                d = d[:, :V]
                scale = R.f32(gsc) * (R.f32(gdv) if use_dev else 1.0)
                w = torch.full((rows,), scale, dtype=torch.float64)
                _, _, ref = R.cross_entropy(logits, gold, 0, smoothing, w)
                _, _, t32 = R.cross_entropy(logits, gold, 0, smoothing, w, dtype=torch.float32)
                assert rel(d, ref) < 1e-5
                assert float(d[1].abs().max()) == 0.0
                pair.add(d, ref, t32)
    pair.check()


@pytest.mark.parametrize('off', [1, 2, 3])
@pytest.mark.parametrize('V', [5, 64, 4093])
def test_ce_forward_buffer_starting_off_a_16_byte_boundary(L, V, off):
    """the logits buffer starts 1, 2 or 3 floats past a 16-byte boundary: row 0's first quad straddles the buffer start and is read
    element by element -- NaN sits in front of the buffer (and behind its last logit) and nothing of it may reach a result.
    lse 2e-6, loss 5e-6 against fp64, arg-max exact with lowest-index ties.
    MI355X, largest kernel / torch fp32 max|err| over the 9 cases: lse 6.63e-07 / 5.10e-07 (worst ratio within a case 2.58, V = 5, off = 3),
    row loss 7.82e-07 / 1.74e-06 (2.20)."""
    rows = 3
    g = torch.Generator().manual_seed(V + off)
    logits, dflat, gold = _ce_logits(g, rows, V, V, off=off)
    assert dflat.ptr % 16 == 4 * off
    dgold = Guarded(rows, dtype=torch.int64, init=gold)
    nn_ = int((gold != 0).sum())
    plse, ploss = ErrPair('ce fwd lse V=%d off=%d' % (V, off)), ErrPair('ce fwd rowloss V=%d off=%d' % (V, off))
    for smoothing in (0.0, 0.1):
        lse, hyp, rowloss, loss = _ce_forward(L, dflat, dgold, rows, V, V, smoothing, nn_)
        assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(rowloss).all()) and bool(torch.isfinite(loss).all())
        w = torch.ones(rows, dtype=torch.float64)
        lse_ref, loss_ref, _ = R.cross_entropy(logits, gold, 0, smoothing, w)
        lse32, loss32, _ = R.cross_entropy(logits, gold, 0, smoothing, w, dtype=torch.float32)
        assert float((lse.double() - lse_ref).abs().max()) < 2e-6 * float(lse_ref.abs().max())
        assert float((rowloss.double() - loss_ref).abs().max()) < 5e-6 * float(loss_ref.abs().max())
        assert abs(float(loss) - float(loss_ref.sum() / nn_)) < 5e-6 * float(loss_ref.sum() / nn_)
        hyp_ref = torch.stack([(row == row.max()).nonzero()[0, 0] for row in logits])
        assert torch.equal(hyp, hyp_ref) and int(hyp[1]) == 0 and (V <= 4 or int(hyp[2]) == 3)
        assert float(rowloss[1]) == 0.0
        plse.add(lse, lse_ref, lse32)
        ploss.add(rowloss, loss_ref, loss32)
    plse.check()
    ploss.check()


@pytest.mark.parametrize('rpg', [1, 300])
def test_ce_grouped_forward_group_sums(L, rpg):
    """2 groups of V = 64 rows; 300 rows per group is the second stride trip of the 256-thread group sum.  Eight draws, so that the
    per-element check sees 16 group losses.  Loss per group 5e-6 against fp64.
    MI355X, kernel / torch fp32 max|err|: rpg=1 7.10e-07 / 7.66e-07, rpg=300 7.39e-07 / 6.84e-07."""
    V, groups = 64, 2
    rows = rpg * groups
    got, ref, t32 = [], [], []
    for draw in range(8):
        g = torch.Generator().manual_seed(draw * 1000 + rpg)
        logits = torch.randn(rows, V, generator=g)
        gold = torch.randint(1, V, (rows,), generator=g)
        if rpg > 1:
            gold[3] = gold[rpg + 7] = gold[rows - 1] = 0
        counts = (gold != 0).view(groups, rpg).sum(1)
        inv = 1.0 / counts.float()
        dl, dg, dinv = Guarded(rows * V, init=logits), Guarded(rows, dtype=torch.int64, init=gold), Guarded(groups, init=inv)

        def run():
            lse, hyp, rowloss, loss = Guarded(rows), Guarded(rows, dtype=torch.int64), Guarded(rows), Guarded(groups)
            assert L.mtl_ce_argmax_fwd_g(st(), dl.ptr, dg.ptr, rows, V, V, 0, 0.1, dinv.ptr, lse.ptr, hyp.ptr, rowloss.ptr, loss.ptr, rpg) == 0
            assert ok(lse, hyp, rowloss, loss, dl, dg, dinv)
            return lse.cpu(), hyp.cpu(), rowloss.cpu(), loss.cpu()
        lse, hyp, rowloss, loss = twice(run)
        w = torch.ones(rows, dtype=torch.float64)
        _, l64, _ = R.cross_entropy(logits, gold, 0, 0.1, w)
        _, l32, _ = R.cross_entropy(logits, gold, 0, 0.1, w, dtype=torch.float32)
        want = l64.view(groups, rpg).sum(1) * inv.double()
        assert bool(((loss.double() - want).abs() < 5e-6 * want.abs()).all())
        assert torch.equal(hyp, logits.argmax(1))
        got.append(loss), ref.append(want), t32.append(l32.view(groups, rpg).sum(1) * inv)
    ErrPair('ce grouped loss rpg=%d' % rpg).add(torch.cat(got), torch.cat(ref), torch.cat(t32)).check()
    assert L.mtl_ce_argmax_fwd_g(st(), dl.ptr, dg.ptr, rows, V, V, 0, 0.1, dinv.ptr, dl.ptr, dg.ptr, dl.ptr, dl.ptr, rows + 1) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# 5. embedding
# ---------------------------------------------------------------------------------------------------------------------
def _embed_ids(g, rows, V, same_id):
    if same_id:
        return torch.full((rows,), 7, dtype=torch.int64)                       # one chain through every row
    ids = torch.randint(1, 5, (rows,), generator=g)                            # few ids: long chains
    ids[0] = ids[rows // 2] = ids[rows - 1] = 0                                # pad rows at the head, in the middle and at the end
    return ids


@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('rows', [1, 21])
@pytest.mark.parametrize('d', [16, 100, 128])
def test_embedding_chains_pads_masks_and_groups(L, d, rows, groups):
    """T = 1 (every row adds pe[0]); every row the same id (one chain of 21) and a mix with pad ids at the head, middle and end; with
    and without a keep-mask; the backward accumulates onto a non-zero table and leaves the pad row and absent ids bit for bit.  Two
    groups: the same ids in both, chains per group, tables sParam = sGrad = V d + 24 apart with NaN between them.
    Forward: table[id] + pe is one rounding (and the mask's v mscale a second one) -- bit for bit the fp32 expression.
    Backward: 1e-6 norm-wise (tests/test_ops_gpu.py).  MI355X, largest kernel / torch fp32 max|err| over the 12 cases: 3.21e-06 / 3.21e-06, worst
    ratio within a case 1.34 (d = 100, rows = 21, 2 groups)."""
    V, T, pad = 11, 1, 0
    sP = V * d + 24
    g = torch.Generator().manual_seed(d + rows)
    n = rows * groups
    msc = R.f32(1 / 0.75)
    pair = ErrPair('embed bwd d=%d rows=%d groups=%d' % (d, rows, groups))
    for same_id in (True, False):
        for use_mask in (False, True):
            ids = _embed_ids(g, rows, V, same_id).repeat(groups)
            tabs = torch.full((groups, sP), float('nan'))
            tabs[:, :V * d] = torch.randn(groups, V * d, generator=g)
            pe, dout = torch.randn(T, d, generator=g), torch.randn(n, d, generator=g)
            mask = (torch.rand(n, d, generator=g) >= 0.25).to(torch.uint8) if use_mask else None
            first, nxt = R.embed_chains(ids.tolist(), rows)
            dids, dtab, dpe, ddo = Guarded(n, dtype=torch.int64, init=ids), Guarded(groups * sP, init=tabs), Guarded(T * d, init=pe), Guarded(n * d, init=dout)
            dmask = None if mask is None else Guarded(n * d, dtype=torch.uint8, init=mask)
            dfirst, dnext = Guarded(n, dtype=torch.int32, init=first), Guarded(n, dtype=torch.int32, init=nxt)

            def run():
                out, grad = Guarded(n * d), Guarded(groups * sP, init=tabs)
                if groups > 1:
                    assert L.mtl_embed_pe_fwd_g(st(), dids.ptr, dtab.ptr, dpe.ptr, out.ptr, n, T, d, ptr(dmask), msc, rows, sP) == 0
                    assert L.mtl_embed_bwd_g(st(), dids.ptr, dfirst.ptr, dnext.ptr, ddo.ptr, grad.ptr, n, d, pad, ptr(dmask), msc, rows, sP) == 0
                else:
                    assert L.mtl_embed_pe_fwd(st(), dids.ptr, dtab.ptr, dpe.ptr, out.ptr, n, T, d, ptr(dmask), msc) == 0
                    assert L.mtl_embed_bwd(st(), dids.ptr, dfirst.ptr, dnext.ptr, ddo.ptr, grad.ptr, n, d, pad, ptr(dmask), msc) == 0
                assert ok(out, grad, dids, dtab, dpe, ddo, dmask, dfirst, dnext)
                return out.cpu().view(n, d), grad.cpu().view(groups, sP)
            out, grad = twice(run)
            t3 = tabs[:, :V * d].reshape(groups, V, d)
            grp = torch.arange(n) // rows
            want = t3[grp, ids] + pe[0]
            dm32 = dout
            if mask is not None:
                want = torch.where(mask != 0, want * torch.tensor(msc), torch.zeros(()))
                dm32 = torch.where(mask != 0, dout * torch.tensor(msc), torch.zeros(()))
            assert same(out, want)
            dm64 = dout.double() if mask is None else torch.where(mask != 0, dout.double() * msc, torch.zeros((), dtype=torch.float64))
            livei = (ids != pad).nonzero().squeeze(1)
            slot = (grp * V + ids)[livei]
            ref = t3.double().reshape(groups * V, d).clone().index_add_(0, slot, dm64[livei])
            t32 = t3.reshape(groups * V, d).clone().index_add_(0, slot, dm32[livei])
            got = grad[:, :V * d].reshape(groups * V, d)
            assert all_nan_bits(grad[:, V * d:])
            assert rel(got, ref) < 1e-6
            touched = torch.zeros(groups * V, dtype=torch.bool)
            touched[slot] = True
            assert same(got[~touched], t3.reshape(groups * V, d)[~touched])       # the pad row and ids that do not occur
            pair.add(got, ref, t32)
    pair.check()


# ---------------------------------------------------------------------------------------------------------------------
# 6. column sums
# ---------------------------------------------------------------------------------------------------------------------
def _colsum_once(L, X, rows, cols, ld, out0, off=0):
    """X as rows of ld floats (NaN in the columns beyond cols), max|X| negative in the last row and column; with and without amax"""
    padded = torch.cat([X, torch.full((rows, ld - cols), float('nan'))], 1) if ld > cols else X
    dX = Guarded(rows * ld, off=off, init=padded)
    nws = L.mtl_colsum_workspace(rows, cols) // 4

    def run(with_amax=True):
        out, ws = Guarded(cols, init=out0), Guarded(nws)
        amax = Guarded(2048, init=torch.full((2048,), 1e30)) if with_amax else None
        assert L.mtl_colsum_accum(st(), dX.ptr, rows, cols, ld, out.ptr, ws.ptr, ptr(amax)) == 0
        assert ok(out, ws, amax, dX)
        return out.cpu(), (None if amax is None else amax.cpu())
    out, amax = twice(run)
    assert same(run(False)[0], out)                                   # the form without the bound sums in the same order
    heads = amax.view(64, 32)
    assert bool((heads[:, 0] == float(X.abs().max())).all()) and float(X[-1, -1]) == -float(X.abs().max())      # written, not accumulated
    assert bool((heads[:, 1:] == 1e30).all())
    return out


@pytest.mark.parametrize('cols', [1, 4, 63, 64, 65, 100, 256, 260])
def test_colsum_row_counts_column_tails_and_leading_dimension(L, cols):
    """rows 1 .. 1000 (fewer than 32 rows: one chunk; 33: a chunk of 17 and one of 16), column counts around the 64-lane block and the
    16-byte form (cols = 4 x 2^j <= 256 with ld = cols), ld = cols and cols + 3 (NaN in the columns beyond cols), accumulating onto
    a non-zero `out`; at cols = 64 also X one float past a 16-byte boundary (the scalar form).  2e-5 norm-wise against the fp64 sum.
    MI355X, kernel / torch fp32 max|err| over the (rows, ld) pairs of a case: 3.76e-06 / 3.76e-06 (cols = 1), 9.86e-06 / 1.19e-05 (64),
    1.41e-05 / 8.62e-06 (65), 1.30e-05 / 1.65e-05 (256), 2.94e-05 / 1.51e-05 (260: the worst ratio, 1.95)."""
    g = torch.Generator().manual_seed(cols)
    pair = ErrPair('colsum cols=%d' % cols)
    for rows in (1, 7, 31, 32, 33, 1000):
        for ld, off in [(cols, 0), (cols + 3, 0)] + ([(cols, 1)] if cols == 64 else []):
            X = torch.randn(rows, cols, generator=g)
            X[-1, -1] = -(float(X.abs().max()) + 1.0)
            out0 = torch.randn(cols, generator=g)
            out = _colsum_once(L, X, rows, cols, ld, out0, off)
            ref = out0.double() + X.double().sum(0)
            assert rel(out, ref) < 2e-5
            pair.add(out, ref, out0 + X.sum(0))
    pair.check()


@pytest.mark.parametrize('cols', [4, 16, 256])
def test_colsum_several_tasks_in_one_launch(L, cols):
    """3 tasks x 33 rows, per-task strides of `out` and of the bound.
    MI355X, kernel / torch fp32 max|err|: cols=4 1.34e-06 / 1.34e-06, cols=16 1.08e-06 / 1.51e-06, cols=256 2.38e-06 / 2.15e-06."""
    nt, rows, sOut, sAmax = 3, 33, cols + 8, 2048 + 32
    g = torch.Generator().manual_seed(cols)
    X = torch.randn(nt, rows, cols, generator=g)
    for t in range(nt):
        X[t, -1, -1] = -(float(X[t].abs().max()) + 1.0 + t)
    out0 = torch.randn(nt, sOut, generator=g)
    dX = Guarded(X.numel(), init=X)
    nws = nt * (L.mtl_colsum_workspace(rows, cols) // 4 + 4)

    def run():
        out, ws, amax = Guarded(nt * sOut, init=out0), Guarded(nws), Guarded(nt * sAmax, init=torch.full((nt * sAmax,), 1e30))
        assert L.mtl_colsum_accum_tb(st(), dX.ptr, rows, cols, out.ptr, ws.ptr, amax.ptr, nt, sOut, sAmax) == 0
        assert ok(out, ws, amax, dX)
        return out.cpu().view(nt, sOut), amax.cpu().view(nt, sAmax)
    out, amax = twice(run)
    ref = out0[:, :cols].double() + X.double().sum(1)
    assert rel(out[:, :cols], ref) < 2e-5 and same(out[:, cols:], out0[:, cols:])
    ErrPair('colsum_tb cols=%d' % cols).add(out[:, :cols], ref, out0[:, :cols] + X.sum(1)).check()
    for t in range(nt):
        heads = amax[t, :2048].view(64, 32)
        assert bool((heads[:, 0] == float(X[t].abs().max())).all()) and bool((heads[:, 1:] == 1e30).all()) and bool((amax[t, 2048:] == 1e30).all())
    o, ws = Guarded(nt * sOut), Guarded(nws)
    for bad in (12, 512, 6):                                                        # cols outside 4 x 2^j <= 256
        assert L.mtl_colsum_accum_tb(st(), dX.ptr, rows, bad, o.ptr, ws.ptr, None, nt, sOut, sAmax) == EINVAL
    assert L.mtl_colsum_accum_tb(st(), dX.ptr + 4, rows, cols, o.ptr, ws.ptr, None, nt, sOut, sAmax) == EINVAL
    assert ok(o, ws) and all_nan_bits(o.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# 7. bounds and the h2 census
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 5, 1027, (1 << 20) + 3])
def test_absmax_tail_elements_and_task_strides(L, n):
    """the maximum is the LAST element (in the n & 3 tail for every n here but 2^20 + 3, whose tail holds it too) and negative; the maximum
    over the slot heads equals max|x| exactly, the floats between the heads are not written.  Three tasks at sX = n rounded up to 4,
    plus 8: the floats in the stride gap are larger and must not count."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[-1] = -(float(x.abs().max()) + 1.0)
    dx = Guarded(n, init=x)

    def run():
        amax = Guarded(2048, init=torch.zeros(2048))
        assert L.mtl_absmax_f32(st(), dx.ptr, n, amax.ptr) == 0
        assert ok(amax, dx)
        return (amax.cpu(),)
    amax, = twice(run)
    assert float(R.slot_bound(amax.numpy())) == -float(x[-1]) and float(amax.view(64, 32)[:, 1:].abs().max()) == 0.0
    nt, sX, sA = 3, (n + 3) // 4 * 4 + 8, 2048
    xs = torch.full((nt, sX), 1e9)
    xs[:, :n] = torch.randn(nt, n, generator=g)
    for t in range(nt):
        xs[t, n - 1] = -(float(xs[t, :n].abs().max()) + 1.0 + t)
    dxs = Guarded(nt * sX, init=xs)

    def run_tb():
        amax = Guarded(nt * sA, init=torch.zeros(nt * sA))
        assert L.mtl_absmax_f32_tb(st(), dxs.ptr, n, amax.ptr, nt, sX, sA) == 0
        assert ok(amax, dxs)
        return (amax.cpu().view(nt, sA),)
    amax, = twice(run_tb)
    for t in range(nt):
        assert float(R.slot_bound(amax[t].numpy())) == -float(xs[t, n - 1]) and float(amax[t].view(64, 32)[:, 1:].abs().max()) == 0.0
    o = Guarded(2048)
    assert L.mtl_absmax_f32(st(), dx.ptr + 4, n, o.ptr) == EINVAL
    assert L.mtl_absmax_f32_tb(st(), dxs.ptr + 8, n, o.ptr, nt, sX, sA) == EINVAL
    assert L.mtl_absmax_f32_tb(st(), dxs.ptr, n, o.ptr, nt, sX + 1, sA) == EINVAL
    assert ok(o) and all_nan_bits(o.cpu())


def _below(v):
    return np.nextafter(np.float32(v), np.float32(0))


def _census_probes(bound):
    """values on and next to the two lines of `bound`: on a line is not counted, the next float below is; zeros, negatives, subnormals"""
    s = R.h2_scale(bound)
    t22, t16 = np.float32(0.125 / s), np.float32(0.001953125 / s)
    return np.array([0.0, -0.0, t22, -t22, _below(t22), -_below(t22), t16, -t16, _below(t16), -_below(t16), 2 * t22, t16 / 2, 1e-42, -1e-45,
                     1.0, -3.0], dtype=np.float32), t22, t16


@pytest.mark.parametrize('n', [1, 3, 6, 1027, (1 << 20) + 3])
def test_h2_census_counts_exactly_on_the_lines(L, n):
    """one tensor per bound: exactly 2^3, the float below it (the scale doubles), 5.7, and 0 (scale 1).  The bound sits in ONE slot head
    (a smaller value in another head, a huge one between the heads); elements are drawn from the probes on the lines, and the n & 3
    tail (the whole of a shorter vector) holds counted elements.  The three counters equal the numpy reference exactly, a second call
    doubles them, and the fourth word of the 4-word counter stride keeps its value."""
    rng = np.random.RandomState(n)
    for bound in (8.0, float(_below(8.0)), 5.7, 0.0):
        probes, t22, t16 = _census_probes(bound)
        x = probes[rng.randint(len(probes), size=n)]
        tail = max(n & 3, 1)
        x[n - tail:] = np.array([_below(t22), -_below(t16), _below(t22)], dtype=np.float32)[:tail]
        amax = np.zeros(2048, dtype=np.float32)
        amax[37 * 32], amax[0], amax[37 * 32 + 1] = bound, bound / 4, 1e30
        want = R.h2_census(x, R.slot_bound(amax))
        assert want[1] >= tail and want[0] >= want[1] >= want[2]
        dx, da = Guarded(n, init=torch.from_numpy(x)), Guarded(2048, init=torch.from_numpy(amax))

        def run():
            counts = Guarded(4, dtype=torch.int64, init=torch.tensor([0, 0, 0, -7]))
            assert L.mtl_h2_census(st(), dx.ptr, n, da.ptr, counts.ptr, 1, 0, 0, 4) == 0
            assert ok(counts, dx, da)
            first = counts.cpu()
            assert L.mtl_h2_census(st(), dx.ptr, n, da.ptr, counts.ptr, 1, 0, 0, 4) == 0
            assert ok(counts, dx, da)
            return first, counts.cpu()
        first, second = twice(run)
        assert first.tolist() == list(want) + [-7], (bound, first.tolist(), want)
        assert second.tolist() == [2 * w for w in want] + [-7]
        assert same(dx.cpu(), torch.from_numpy(x)) and same(da.cpu(), torch.from_numpy(amax))


@pytest.mark.parametrize('n', [1, 3, 6, 1027, (1 << 20) + 3])
def test_h2_census_every_task_against_its_own_bound(L, n):
    """3 tasks whose bounds differ by 2^10 (sAmax = 2048), tensors sX = n rounded up to 4, plus 8 apart with countable values in the gap,
    counters 4 words apart.  Every tensor is drawn from the probes of ALL three bounds, so a task counted against another task's
    bound, or one that reads into the gap, gets other numbers."""
    nt, sX = 3, (n + 3) // 4 * 4 + 8
    rng = np.random.RandomState(n + 1)
    bounds = [5.7 * 2.0 ** (10 * t) for t in range(nt)]
    sets = [_census_probes(b) for b in bounds]
    probes = np.concatenate([s[0] for s in sets])
    xs = np.full((nt, sX), _below(sets[0][2]), dtype=np.float32)               # the gap: below every line of every task
    amax = np.zeros((nt, 2048), dtype=np.float32)
    want = []
    for t in range(nt):
        xs[t, :n] = probes[rng.randint(len(probes), size=n)]
        tail = max(n & 3, 1)
        xs[t, n - tail:n] = np.array([_below(sets[t][1]), -_below(sets[t][2]), _below(sets[t][1])], dtype=np.float32)[:tail]
        amax[t, (5 + t) * 32] = bounds[t]
        want.append(R.h2_census(xs[t, :n], R.slot_bound(amax[t])))
    assert len(set(want)) == nt or n < 1000                                    # (the short vectors are all tail: equal counts)
    dx, da = Guarded(nt * sX, init=torch.from_numpy(xs)), Guarded(nt * 2048, init=torch.from_numpy(amax))

    def run():
        counts = Guarded(4 * nt, dtype=torch.int64, init=torch.tensor([0, 0, 0, -7] * nt))
        for _ in range(2):
            assert L.mtl_h2_census(st(), dx.ptr, n, da.ptr, counts.ptr, nt, sX, 2048, 4) == 0
        assert ok(counts, dx, da)
        return (counts.cpu().view(nt, 4),)
    counts, = twice(run)
    assert counts.tolist() == [[2 * w for w in want[t]] + [-7] for t in range(nt)], (counts.tolist(), want)
    o = Guarded(4, dtype=torch.int64)
    assert L.mtl_h2_census(st(), dx.ptr + 4, n, da.ptr, o.ptr, nt, sX, 2048, 4) == EINVAL
    assert L.mtl_h2_census(st(), dx.ptr, n, da.ptr, o.ptr, nt, sX + 2, 2048, 4) == EINVAL
    assert ok(o)


# ---------------------------------------------------------------------------------------------------------------------
# 8. masks, permutation, tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 1023])
def test_dropout_mask_prefix_and_counter_rule(L, n):
    """bytes beyond n untouched; the mask of n is the prefix of the mask of n + 9; counter = offset + i / 4, so the mask at offset + 1
    is the mask at offset shifted by 4 elements"""
    seed = torch.tensor([2 ** 40 + 17], dtype=torch.int64).cuda()
    off = 5 << 40

    def draw(m, o):
        def run():
            k = Guarded(m, dtype=torch.uint8)
            assert L.mtl_dropout_mask(st(), k.ptr, m, 0.3, seed.data_ptr(), o) == 0
            assert ok(k)
            return (k.cpu(),)
        return twice(run)[0]
    a, b, c = draw(n, off), draw(n + 9, off), draw(n + 9, off + 1)
    assert bool((a <= 1).all()) and bool((b <= 1).all())
    assert torch.equal(a, b[:n]) and R.philox_shift_ok(b, c)
    big = draw(4096, off)
    assert 0.6 < float(big.float().mean()) < 0.8 and torch.equal(big[:n], a)
    k = Guarded(8, dtype=torch.uint8)
    assert L.mtl_dropout_mask(st(), k.ptr, 8, 1.0, seed.data_ptr(), off) == EINVAL and ok(k)      # p must be < 1


@pytest.mark.parametrize('rows', [1, 5])
def test_permute_hc_scalar_path_for_two_tasks(L, rows):
    """C = 6, Hh = 3 (neither a multiple of 4: the element-wise LDS form), 2 tasks at strides that are no multiple of 4; forward with
    the bound riding along, and the accumulating inverse"""
    nt, C, Hh = 2, 6, 3
    n = C * Hh
    sSrc, sDst = rows * n + 2, rows * n + 5
    g = torch.Generator().manual_seed(rows)
    w = torch.full((nt, sSrc), float('nan'))
    w[:, :rows * n] = torch.randn(nt, rows * n, generator=g)
    dw = Guarded(nt * sSrc, init=w)
    w3 = w[:, :rows * n].reshape(nt, rows, C, Hh)

    def run():
        wp, amax = Guarded(nt * sDst), Guarded(nt * 2048, init=torch.zeros(nt * 2048))
        assert L.mtl_permute_hc_tb(st(), dw.ptr, wp.ptr, rows, C, Hh, 0, amax.ptr, nt, sSrc, sDst, 2048) == 0
        back = Guarded(nt * sSrc, init=torch.ones(nt * sSrc))
        assert L.mtl_permute_hc_tb(st(), wp.ptr, back.ptr, rows, C, Hh, 1, None, nt, sDst, sSrc, 0) == 0
        assert ok(wp, amax, back, dw)
        return wp.cpu().view(nt, sDst), amax.cpu().view(nt, 2048), back.cpu().view(nt, sSrc)
    wp, amax, back = twice(run)
    assert same(wp[:, :rows * n], w3.transpose(2, 3).reshape(nt, rows * n)) and all_nan_bits(wp[:, rows * n:])
    assert same(back[:, :rows * n], w[:, :rows * n] + 1) and same(back[:, rows * n:], torch.ones(nt, 2))
    for t in range(nt):
        assert float(R.slot_bound(amax[t].numpy())) == float(w3[t].abs().max())


def test_zero_tails_width_zero_width_beyond_T_and_odd_width(L):
    """a width of 0 clears every frame, a width beyond T none, an odd width with shift = 1 rounds down; rows of 8 floats"""
    per_task, T, row = 2, 7, 8
    widths = [0, 9, 5]
    n = per_task * len(widths)
    w = Guarded(len(widths), dtype=torch.int32, init=torch.tensor(widths, dtype=torch.int32))
    y0 = torch.randn(n, T, row, generator=torch.Generator().manual_seed(0))
    for shift in (0, 1):
        def run():
            y = Guarded(n * T * row, init=y0)
            assert L.mtl_zero_tails(st(), y.ptr, n, T, row, w.ptr, shift, per_task) == 0
            assert ok(y, w)
            return (y.cpu().view(n, T, row),)
        y, = twice(run)
        ref = y0.clone()
        for s in range(n):
            ref[s, min(widths[s // per_task] >> shift, T):] = 0
        assert same(y, ref)
        assert float(y[:2].abs().max()) == 0.0 and (shift == 1 or same(y[2:4], y0[2:4]))
    y = Guarded(n * T * row, init=y0)
    assert L.mtl_zero_tails(st(), y.ptr + 4, n, T, row, w.ptr, 0, per_task) == EINVAL
    assert L.mtl_zero_tails(st(), y.ptr, n, T, 6, w.ptr, 0, per_task) == EINVAL
    assert ok(y) and same(y.cpu(), y0.reshape(-1))
