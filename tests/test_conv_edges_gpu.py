"""Edge shapes of the 3 x 3 convolution kernels through the C ABI, against the fp64 truths and the PER-ELEMENT bound of
tests/conv_edge_util.py: the ReLU forward, the fused ReLU + 2 x 2 max-pool forward, the data gradients that write 128 channels, the
dense / x3 weight gradients -- in the two-piece fp16 ("h2") and the split-bf16 ("x3") arithmetic.

Route of dispatch_conv_x3 (csrc/mtl_mfma.hip) -> cases (table: conv_edge_util.CASES)
    <64, 2, ..., WN = 1>  h2 ReLU forward / pool, 64 channels        P64 (its un-pooled twin too), ONE 64, MANY64, TASKS P64, stacked P64
    <64, 1, ...>          x3 64 -> 64, 8 x 16 pixel tiles            P64 x3 (forward, pool), ONE 64 x3 (forward, pool, data gradient)
    <128, 2, RELU>        conv5 forward                              R128, P128's un-pooled twin, ONE 128, MANY128, TASKS R128, stacked R128
    <128, 2, POOL>        conv7 forward + pool                       P128, ONE 128, TASKS P128, stacked P128 (wshift = 1)
    <128, 2, UNPOOL>      conv7 data gradient, pooled source         D128p (odd F without the edge kernel), TASKS D128p, stacked D128p
    <128, 2, DGRAD>       the same route, dense source               D128d, ONE 128
    <64, 2, DGRAD, WN = 1> h2 dense data gradient, 64 channels       ONE 64 (one pixel; its edge suite is tests/test_conv_dgrad64_gpu.py)
    conv3x3_wgrad_x3_kernel<false, 2>, <*, 3>, the sparse form       test_wgrad_edges
Every case: return code 0, two runs bit-identical, NaN guards around the float outputs and 0xEE guards around the arg-max bytes intact,
the input inside a buffer of 1e4 max|x| (a halo taken from outside the tensor turns up in the values), no NaN, every element inside
the bound, the normwise criteria of tests/test_ops_gpu.py (h2: below 1e-6 and below twice the exact-fp32 kernel's error; x3: 3e-6 /
1e-5), amax_* outputs within [max|out|, 8 max|out|].  Pool forwards are compared BITWISE with the 2 x 2 first-maximum pooling of the
un-pooled forward of the same arithmetic.  One report line per case and task (collected in profiles/conv_edges/errors.txt)."""
import functools

import pytest
import torch

from tests import conv_edge_util as U

pytestmark = pytest.mark.gpu

S = 2048          # MTL_AMAX_FLOATS
GUARD = 4096      # NaN floats (0xEE bytes) in front of and behind every output
EINVAL = -22


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def padded(t):
    """a device copy of t in the middle of a buffer filled with 1e4 max|t|"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), 1e4 * max(float(t.abs().max()), 1.0)).cuda()
    v = buf[GUARD:GUARD + n].view(t.shape)
    v.copy_(t)
    return v


def guarded(shape, dtype=torch.float32, fill=None):
    n = 1
    for s in shape:
        n *= s
    buf = (torch.full((n + 2 * GUARD,), float('nan')) if dtype == torch.float32 else torch.full((n + 2 * GUARD,), 0xEE, dtype=torch.uint8)).cuda()
    v = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        v.fill_(fill)
    return buf, v


def guards_intact(buf):
    n = buf.numel() - 2 * GUARD
    edge = torch.cat([buf[:GUARD], buf[GUARD + n:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float32 else bool((edge == 0xEE).all())


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def prep_weights(L, arith, w):
    """per-task prepared weights of the arithmetic (byte stride nb) and of the exact-fp32 kernels"""
    nt, cout, cin = w.shape[:3]
    wdev = w.cuda()
    nb = (L.mtl_conv3x3_wprep_h2_bytes(cout, cin) + 15) // 16 * 16 if arith == 'h2' else 3 * 9 * cin * cout * 2
    pf, pd = torch.empty(nt, nb, dtype=torch.uint8).cuda(), torch.empty(nt, nb, dtype=torch.uint8).cuda()
    wf, wd = torch.empty(nt, 9, cin, cout).cuda(), torch.empty(nt, 9, cout, cin).cuda()
    prep = L.mtl_conv3x3_wprep_h2 if arith == 'h2' else L.mtl_conv3x3_wprep_x3
    for k in range(nt):
        assert prep(st(), wdev[k].data_ptr(), pf[k].data_ptr(), pd[k].data_ptr(), cout, cin) == 0
        assert L.mtl_conv3x3_wprep(st(), wdev[k].data_ptr(), wf[k].data_ptr(), wd[k].data_ptr(), cout, cin) == 0
    return dict(f=pf, d=pd, nb=nb, wf=wf, wd=wd)


def amax_of(t, nt, apart=True):
    """per-task operand bounds; apart: asserted more than 2^4 apart between neighbouring tasks"""
    B = t.shape[0] // nt
    a = torch.stack([t[k * B:(k + 1) * B].abs().max().reshape(1).repeat(S) for k in range(nt)]).contiguous()
    for k in range(1, nt if apart else 0):
        assert float(a[k, 0] / a[k - 1, 0]) > 16.0
    return a


def call(L, arith, kind, W, src, am_in, bias, act, out, am_out, ain, aout, dims, nt, widths=None, wshift=0, single=False):
    """one launch of the arithmetic's entry point for `kind`; dims = (B per task, T, F, Cin, Cout) of the forward convolution"""
    B, T, Fq, cin, cout = dims
    nb, wp = W['nb'], ptr(widths)
    if single:
        assert nt == 1 and widths is None
        if kind == 'relu':
            if arith == 'h2':
                return L.mtl_conv3x3_relu_fwd_h2(st(), ptr(src), ptr(ain), ptr(W['f']), ptr(bias), ptr(out), ptr(aout), B, T, Fq, cin, cout)
            return L.mtl_conv3x3_relu_fwd_x3(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), B, T, Fq, cin, cout)
        if kind == 'pool':
            if arith == 'h2':
                return L.mtl_conv3x3_relu_pool_fwd_h2(st(), ptr(src), ptr(ain), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), ptr(aout), B, T, Fq, cin, cout)
            return L.mtl_conv3x3_relu_pool_fwd_x3(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), B, T, Fq, cin, cout)
        if arith == 'h2':
            return L.mtl_conv3x3_dgrad_h2(st(), ptr(src), ptr(ain), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), ptr(aout), B, T, Fq, cin, cout)
        return L.mtl_conv3x3_dgrad_x3(st(), ptr(src), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), B, T, Fq, cin, cout)
    if kind == 'relu':
        if arith == 'h2':
            return L.mtl_conv3x3_relu_fwd_h2_tb(st(), ptr(src), ptr(ain), ptr(W['f']), ptr(bias), ptr(out), ptr(aout), B, T, Fq, cin, cout, nt, nb,
                                                cout, S, S, wp, wshift)
        return L.mtl_conv3x3_relu_fwd_x3_tb(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), B, T, Fq, cin, cout, nt, nb, cout, wp, wshift)
    if kind == 'pool':
        if arith == 'h2':
            return L.mtl_conv3x3_relu_pool_fwd_h2_tb(st(), ptr(src), ptr(ain), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), ptr(aout), B, T, Fq,
                                                     cin, cout, nt, nb, cout, S, S, wp, wshift)
        return L.mtl_conv3x3_relu_pool_fwd_x3_tb(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), B, T, Fq, cin, cout, nt, nb, cout,
                                                 wp, wshift)
    if arith == 'h2':
        return L.mtl_conv3x3_dgrad_h2_tb(st(), ptr(src), ptr(ain), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), ptr(aout), B, T, Fq, cin, cout, nt,
                                         nb, S, S, wp, wshift)
    return L.mtl_conv3x3_dgrad_x3_tb(st(), ptr(src), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), B, T, Fq, cin, cout, nt, nb, wp, wshift)


def call_fp32(L, kind, W, k, src, am_in, bias, act, out, am_out, dims):
    """the library's exact-fp32 kernel on task k's data"""
    B, T, Fq, cin, cout = dims
    if kind == 'relu':
        return L.mtl_conv3x3_relu_fwd(st(), ptr(src), W['wf'][k].data_ptr(), ptr(bias), ptr(out), B, T, Fq, cin, cout)
    if kind == 'pool':
        return L.mtl_conv3x3_relu_pool_fwd(st(), ptr(src), W['wf'][k].data_ptr(), ptr(bias), ptr(out), ptr(am_out), B, T, Fq, cin, cout)
    return L.mtl_conv3x3_dgrad(st(), ptr(src), ptr(am_in), W['wd'][k].data_ptr(), ptr(act), ptr(out), B, T, Fq, cin, cout)


def out_shape(kind, n, T, Fq, cin, cout):
    return (n, T // 2, Fq // 2, cout) if kind == 'pool' else (n, T, Fq, cout if kind == 'relu' else cin)


def launch_twice(L, arith, kind, W, dev, dims, nt, want_amax=True, **kw):
    """two launches into fresh guarded outputs: (out, arg-max codes or None, amax_out or None), bit-identical, guards intact"""
    B, T, Fq, cin, cout = dims
    runs = []
    for rep in range(2):
        buf, out = guarded(out_shape(kind, nt * B, T, Fq, cin, cout), fill=kw.get('fill'))
        abuf, am_out = guarded(out.shape, torch.uint8) if kind == 'pool' else (None, None)
        aout = torch.zeros(nt, S).cuda() if arith == 'h2' and want_amax else None
        rc = call(L, arith, kind, W, dev['src'], dev.get('am'), dev.get('bias'), dev.get('act'), out, am_out, dev.get('ain'), aout, dims, nt,
                  widths=kw.get('widths'), wshift=kw.get('wshift', 0), single=kw.get('single', False))
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(buf) and (abuf is None or guards_intact(abuf)), 'guard elements overwritten'
        runs.append((out.clone(), am_out.clone() if am_out is not None else None, aout))
    for a, b in zip(*runs):
        assert a is None or torch.equal(bits(a), bits(b)), 'not repeatable bit for bit'
    return runs[0]


def to_device(L, c, kind, nt):
    if kind in ('relu', 'pool'):
        return dict(src=padded(c['x']), bias=c['b'].cuda(), ain=amax_of(c['x'], nt).cuda())
    return dict(src=padded(c['dy']), am=c['am'].cuda() if c['am'] is not None else None, act=c['act'].cuda(), ain=amax_of(c['dy'], nt).cuda())


def compare(name, arith, kind, k, got, got32, want, bd):
    """the assertions on one task's output; returns the report line"""
    got, got32 = got.double().cpu(), got32.double().cpu()
    assert not bool(torch.isnan(got).any()), name
    err = (got - want).abs()
    pos = bd > 0
    ratio = float((err[pos] / bd[pos]).max()) if bool(pos.any()) else 0.0
    e, e32 = U.rel(got, want), U.rel(got32, want)
    line = 'conv_edges %s %s %s task %d: kernel %.2e, fp32 kernel %.2e, max error / bound %.4f' % (name, arith, kind, k, e, e32, ratio)
    print(line)
    assert bool((err <= bd).all()), line
    if arith == 'h2':
        assert e < 1e-6 and e < 2.0 * e32 + 1e-30, line
    else:
        assert e < (1e-5 if kind.startswith('dgrad') else 3e-6), line
    return line


def run_case(L, name, arith, kind, cin, cout, B, T, Fq, nt=1, variant='', single=False):
    c = U.make_case(kind, cin, cout, B, T, Fq, nt, variant)
    dims = (B, T, Fq, cin, cout)
    W = prep_weights(L, arith, c['w'])
    dev = to_device(L, c, kind, nt)
    want_amax = variant != 'ZERO'            # (all outputs zero: no [max, 8 max] interval to hold the bound to)
    out, codes, aout = launch_twice(L, arith, kind, W, dev, dims, nt, want_amax=want_amax, single=single)
    truth, Ssum = {'relu': ('y', 'Sy'), 'pool': ('p', 'Sp')}.get(kind, ('dx', 'Sdx'))
    K = 9 * (cin if kind in ('relu', 'pool') else cout)
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        _, o32 = guarded(out[sl].shape)
        c32 = torch.empty(o32.shape, dtype=torch.uint8).cuda() if kind == 'pool' else None
        assert call_fp32(L, kind, W, k, dev['src'][sl], dev['am'][sl] if dev.get('am') is not None else None,
                         dev['bias'][k] if 'bias' in dev else None, dev['act'][sl] if 'act' in dev else None, o32, c32, dims) == 0
        torch.cuda.synchronize()
        compare(name + (':' + variant if variant else ''), arith, kind, k, out[sl], o32, c[truth][sl], U.bound(c[Ssum][sl], K, arith))
        if aout is not None:
            m, bnd = float(out[sl].abs().max()), float(aout[k].view(-1, 32)[:, 0].max())
            assert m > 0 and m <= bnd <= 8.0 * m, ('amax output', name, k, m, bnd)
    if kind != 'pool':
        return out
    # the pooling rule: bitwise the 2 x 2 maxima and first-maximum codes of the un-pooled forward of the same arithmetic
    y, _, _ = launch_twice(L, arith, 'relu', W, dev, dims, nt, want_amax=False, single=single)
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        _, y32 = guarded(y[sl].shape)
        assert call_fp32(L, 'relu', W, k, dev['src'][sl], None, dev['bias'][k], None, y32, None, dims) == 0
        torch.cuda.synchronize()
        compare(name + (':' + variant if variant else '') + ':unpooled', arith, 'relu', k, y[sl], y32, c['y'][sl], U.bound(c['Sy'][sl], K, arith))
    p_own, codes_own = U.pool_first_max(y.cpu())
    assert torch.equal(bits(out.cpu()), bits(p_own)), 'pooled values are not the maxima of the un-pooled forward'
    assert torch.equal(codes.cpu(), codes_own), 'arg-max codes are not the first maximum in window order'
    if variant == 'ZERO':
        assert float(out.abs().max()) == 0.0 and int(codes.sum()) == 0
    if variant == 'CONST':       # windows whose 4 x 4 neighbourhood lies inside the image see the same 36 inputs per pixel: exact ties
        assert int(codes[:, 1:(T - 2) // 2, 1:(Fq - 2) // 2].sum()) == 0 and float(out.max()) > 0
    return out


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('name', ['P64', 'R128', 'P128', 'D128p', 'D128d'])
def test_edge_case(L, name, arith):
    run_case(L, name, arith, *U.CASES[name])


@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('kind,cin,cout,B,T,Fq', U.ONE)
def test_one_window_one_pixel(L, arith, kind, cin, cout, B, T, Fq):
    """every tap but the centre reads padding (T = 1, F = 17: the centre row of taps); the grid is one tile; single-task entry points"""
    run_case(L, 'ONE-%d-%dx%d' % (cin, T, Fq), arith, kind, cin, cout, B, T, Fq, single=True)


def test_many64_more_tiles_than_resident_workgroups(L):
    kind, cin, cout, B, T, Fq = U.CASES['MANY64']
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-(Fq // 2 * 2) // 16) * -(-(T // 2 * 2) // 16) * B > 2 * cus
    run_case(L, 'MANY64', 'h2', kind, cin, cout, B, T, Fq)


def test_many128_more_tiles_than_compute_units(L):
    kind, cin, cout, B, T, Fq = U.CASES['MANY128']
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-Fq // 16) * -(-T // 16) * B * (cout // 128) > cus
    run_case(L, 'MANY128', 'h2', kind, cin, cout, B, T, Fq)


@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('name', U.TASK_CASES)
def test_three_tasks_in_one_launch(L, name, arith):
    """per-task weights, bias and bounds (asserted more than 2^4 apart): a workgroup's tile sequence crosses the task boundaries"""
    kind, cin, cout, _, T, Fq = U.CASES[name]
    run_case(L, 'TASKS-' + name, arith, kind, cin, cout, 1, T, Fq, nt=3)


@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('variant', ['ZERO', 'CONST'])
@pytest.mark.parametrize('name', ['P64', 'P128'])
def test_pool_ties(L, name, variant, arith):
    """ZERO: every window is four ReLU zeros -- output 0, code 0.  CONST: interior windows are exact ties -- code 0."""
    run_case(L, name, arith, *U.CASES[name], variant=variant)


# ------------------------------------------------------------------------------------------------ stacked tasks against their own images
@functools.lru_cache(maxsize=None)
def stacked_case(name, wshift):
    """three tasks of B = 1 at a common T with frame counts of their own (given at full resolution): the stack with junk beyond every
    task's frames, and per task the fp64 result of its own cropped image"""
    kind, cin, cout, _, T, Fq = U.CASES[name]
    c = U.make_case(kind, cin, cout, 1, T, Fq, 3)
    widths = [T << wshift, (T << wshift) - (9 if wshift else 5), 4 << wshift]
    rows = [wd >> wshift for wd in widths]
    assert rows == [T, T - 5, 4]
    g = torch.Generator().manual_seed(T + Fq + wshift)
    truths = []
    if kind in ('relu', 'pool'):
        stack = dict(src=c['x'].clone())
        for k, r in enumerate(rows):
            stack['src'][k, r:] = torch.randn(T - r, Fq, cin, generator=g) * 100.0 * 32.0 ** k
            y, Sy = U.fwd_truth(c['x'][k:k + 1, :r], c['w'][k], c['b'][k])
            truths.append((U.pool_first_max(y)[0], U.pool_max(Sy)) if kind == 'pool' else (y, Sy))
        stack['ain'] = amax_of(c['x'], 3)
    else:
        stack = dict(src=c['dy'].clone(), act=c['act'].clone())
        for k, r in enumerate(rows):
            rp = widths[k] >> (wshift + 1)
            assert rp == r // 2
            stack['src'][k, rp:] = torch.randn(T // 2 - rp, Fq // 2, cout, generator=g) * 100.0 * 32.0 ** k
            stack['act'][k, r:] = torch.rand(T - r, Fq, cin, generator=g)
            dense = U.unpool(c['dy'][k:k + 1, :rp], c['am'][k:k + 1, :rp], r, Fq)
            truths.append(U.dgrad_truth(dense, c['w'][k], c['act'][k:k + 1, :r]))
        stack['ain'] = amax_of(c['dy'], 3)
    return c, widths, rows, stack, truths


@pytest.mark.parametrize('name,wshift,arith', [('P64', 0, 'h2'), ('R128', 1, 'h2'), ('P128', 1, 'h2'), ('D128p', 1, 'h2'),
                                               ('R128', 1, 'x3'), ('P128', 1, 'x3'), ('D128p', 1, 'x3')])
def test_stacked_tasks_meet_their_own_borders(L, name, wshift, arith):
    """mtl_zero_tails + the `widths` form of a launch give every task the convolution of its OWN image: rows below widths[k] >> wshift
    are inside the bound of the fp64 result of the cropped image; tile rows wholly beyond a task's frames are not written"""
    kind, cin, cout, _, T, Fq = U.CASES[name]
    c, widths, rows, stack, truths = stacked_case(name, wshift)
    dims = (1, T, Fq, cin, cout)
    W = prep_weights(L, arith, c['w'])
    wdev = torch.tensor(widths, dtype=torch.int32).cuda()
    dev = dict(src=padded(stack['src']), ain=stack['ain'].cuda())
    if kind.startswith('dgrad'):
        dev.update(am=c['am'].cuda(), act=padded(stack['act']))
        assert L.mtl_zero_tails(st(), dev['src'].data_ptr(), 3, T // 2, (Fq // 2) * cout, wdev.data_ptr(), wshift + 1, 1) == 0
        assert L.mtl_zero_tails(st(), dev['act'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), wshift, 1) == 0
    else:
        dev.update(bias=c['b'].cuda())
        assert L.mtl_zero_tails(st(), dev['src'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), wshift, 1) == 0
    for k, r in enumerate(rows):
        rr = r // 2 if kind.startswith('dgrad') else r
        assert float(dev['src'][k, rr:].abs().sum()) == 0.0 and torch.equal(dev['src'][k, :rr].cpu(), stack['src'][k, :rr])
    out, codes, aout = launch_twice(L, arith, kind, W, dev, dims, 3, widths=wdev, wshift=wshift, fill=-7.0)
    K = 9 * (cin if kind in ('relu', 'pool') else cout)
    div = 2 if kind == 'pool' else 1
    for k, r in enumerate(rows):
        want, Ssum = truths[k]
        got = out[k:k + 1, :r // div].double().cpu()
        assert got.shape == want.shape and not bool(torch.isnan(got).any())
        err, bd = (got - want).abs(), U.bound(Ssum, K, arith)
        pos = bd > 0
        print('conv_edges stacked-%s %s %s task %d (rows %d of %d, wshift %d): kernel %.2e, max error / bound %.4f'
              % (name, arith, kind, k, r, T, wshift, U.rel(got, want), float((err[pos] / bd[pos]).max())))
        assert bool((err <= bd).all()), (name, k)
        edge = -(-r // 16) * 16 // div                             # the first output row of the first tile row wholly beyond the frames
        assert bool((out[k, edge:] == -7.0).all()), (name, k)
        if aout is not None:
            assert float(got.abs().max()) <= float(aout[k].view(-1, 32)[:, 0].max())
    # (P128's pool extent is one tile row: nothing lies beyond it)
    assert bool((out[2, 16 // div:] == -7.0).all()) and (name == 'P128' or out[2, 16 // div:].numel() > 0)


@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('kind', ['relu', 'pool', 'dgrad_p'])
@pytest.mark.parametrize('wshift', [9, -1])
def test_wshift_out_of_range_is_refused(L, arith, kind, wshift):
    cin = cout = 64
    T, Fq = 4, 4
    c = U.make_case(kind, cin, cout, 1, T, Fq, 1)
    W = prep_weights(L, arith, c['w'])
    dev = to_device(L, c, kind, 1)
    wdev = torch.tensor([T], dtype=torch.int32).cuda()
    buf, out = guarded(out_shape(kind, 1, T, Fq, cin, cout), fill=-7.0)
    abuf, am_out = guarded(out.shape, torch.uint8)
    rc = call(L, arith, kind, W, dev['src'], dev.get('am'), dev.get('bias'), dev.get('act'), out, am_out, dev.get('ain'), None, (1, T, Fq, cin, cout), 1,
              widths=wdev, wshift=wshift)
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((out == -7.0).all()) and bool((am_out == 0xEE).all()) and guards_intact(buf) and guards_intact(abuf)


# ------------------------------------------------------------------------------------------------ weight gradients
def wgrad_call(L, arith, tb, dev, dw, db, ws, need, dims, nt):
    B, T, Fq, cin, cout = dims
    x, dy, am = dev['x'], dev['dy'], dev.get('am')
    if arith == 'h2':
        if tb:
            return L.mtl_conv3x3_wgrad_h2_tb(st(), ptr(x), ptr(dev['ax']), ptr(dy), ptr(dev['ady']), ptr(am), ptr(dw), ptr(db), ptr(ws), need, B, T, Fq,
                                             cin, cout, nt, S, S, 9 * cin * cout, cout)
        return L.mtl_conv3x3_wgrad_h2(st(), ptr(x), ptr(dev['ax']), ptr(dy), ptr(dev['ady']), ptr(am), ptr(dw), ptr(db), ptr(ws), need, B, T, Fq, cin, cout)
    if tb or db is not None:                                         # (the single-task x3 entry point has no bias gradient)
        return L.mtl_conv3x3_wgrad_x3_tb(st(), ptr(x), ptr(dy), ptr(am), ptr(dw), ptr(db), ptr(ws), need, B, T, Fq, cin, cout, nt, 9 * cin * cout, cout)
    return L.mtl_conv3x3_wgrad_x3(st(), ptr(x), ptr(dy), ptr(am), ptr(dw), ptr(ws), need, B, T, Fq, cin, cout)


@pytest.mark.parametrize('extent', ['P64', 'P128', 'ONE'])
@pytest.mark.parametrize('arith,pooled,nt', [('h2', False, 1), ('x3', False, 1), ('x3', True, 1), ('h2', False, 3), ('h2', True, 3), ('x3', True, 3)])
def test_wgrad_edges(L, extent, arith, pooled, nt):
    """dense / x3 (and, with three tasks, the sparse pooled) weight gradients at the edge extents: arbitrary arg-max codes, 30 % zeros,
    per tap normwise < 2e-6 and per element inside the bound; bias gradient; db = NULL; accumulation; workspace of exactly the reported size"""
    cin, cout, B, T, Fq = U.WGRAD_EXTENTS[extent]
    c = U.make_wgrad_case(cin, cout, B, T, Fq, nt, pooled)
    dims = (B, T, Fq, cin, cout)
    dev = dict(x=padded(c['x']), dy=padded(c['dy']), am=c['am'].cuda() if pooled else None)
    if arith == 'h2':
        dev['ax'], dev['ady'] = amax_of(c['x'], nt, apart=False).cuda(), amax_of(c['dy'], nt, apart=False).cuda()
    need = L.mtl_conv3x3_wgrad_x3_workspace(B, T, Fq, cin, cout, int(pooled))
    assert need > 0 and need % 4 == 0
    slabs = need // (9 * cin * cout * 4 + cout * 4)
    K = B * (T // 2 * 2 if pooled else T) * (Fq // 2 * 2 if pooled else Fq) + slabs
    bd_w, bd_b = U.bound(c['Sdw'], K, arith), U.bound(c['Sdb'], K, arith)

    def run(pre_w, pre_b, with_db):
        res = []
        for rep in range(2):
            wsbuf = torch.full((need // 4 + GUARD,), float('nan')).cuda()
            wbuf, dw = guarded((nt, cout, cin, 3, 3), fill=pre_w)
            bbuf, db = guarded((nt, cout), fill=pre_b)
            assert wgrad_call(L, arith, nt > 1, dev, dw, db if with_db else None, wsbuf, need, dims, nt) == 0
            torch.cuda.synchronize()
            assert bool(torch.isnan(wsbuf[need // 4:]).all()), 'workspace overrun'
            assert guards_intact(wbuf) and guards_intact(bbuf), 'guard elements overwritten'
            res.append((dw.clone(), db.clone()))
        assert torch.equal(bits(res[0][0]), bits(res[1][0])) and torch.equal(bits(res[0][1]), bits(res[1][1])), 'not repeatable bit for bit'
        return res[0]

    dw, db = run(0.0, 0.0, True)
    dw_nodb, db_nodb = run(0.0, 0.0, False)
    assert torch.equal(bits(dw), bits(dw_nodb)) and float(db_nodb.abs().max()) == 0.0            # db = NULL: the same dw, db untouched
    for k in range(nt):
        gw, gb = dw[k].double().cpu(), db[k].double().cpu()
        assert not bool(torch.isnan(gw).any()) and not bool(torch.isnan(gb).any())
        ew, eb = (gw - c['dw'][k]).abs(), (gb - c['db'][k]).abs()
        taps = max(U.rel(gw[:, :, kh, kw], c['dw'][k][:, :, kh, kw]) for kh in range(3) for kw in range(3))
        pw = bd_w[k] > 0
        print('conv_edges wgrad-%s %s %s task %d of %d: worst tap %.2e, db %.2e, max error / bound %.4f (dw) %.4f (db)'
              % (extent, arith, 'pooled' if pooled else 'dense', k, nt, taps, U.rel(gb, c['db'][k]),
                 float((ew[pw] / bd_w[k][pw]).max()), float((eb / bd_b[k].clamp_min(1e-300)).max())))
        assert taps < 2e-6
        assert bool((ew <= bd_w[k]).all()) and bool((eb <= bd_b[k]).all())
    # accumulation onto pre-fills: each of the slabs + 1 further additions rounds to half an ulp of a partial sum below |pre-fill| + S
    aw, ab = run(0.5, 0.25, True)
    for k in range(nt):
        ew, eb = (aw[k].double().cpu() - (0.5 + c['dw'][k])).abs(), (ab[k].double().cpu() - (0.25 + c['db'][k])).abs()
        assert bool((ew <= bd_w[k] + (slabs + 1) * 2.0 ** -23 * (0.5 + c['Sdw'][k])).all())
        assert bool((eb <= bd_b[k] + (slabs + 1) * 2.0 ** -23 * (0.25 + c['Sdb'][k])).all())


# ------------------------------------------------------------------------------------------------ empty extents
@pytest.mark.parametrize('arith', ['h2', 'x3'])
def test_empty_pool_extent_is_a_no_op(L, arith):
    """T = 1: a pooled forward has no output and a pooled weight gradient no window -- success, nothing written, no launch; the next call is sound"""
    cin = cout = 64
    T, Fq = 1, 5
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(1, T, Fq, cin, generator=g))
    W = prep_weights(L, arith, torch.randn(1, cout, cin, 3, 3, generator=g) * 0.05)
    dev = dict(src=padded(x), bias=torch.zeros(1, cout).cuda(), ain=amax_of(x, 1).cuda())
    for single in (True, False):
        buf, out = guarded((0,))
        abuf, am_out = guarded((0,), torch.uint8)
        aout = torch.zeros(1, S).cuda()
        rc = call(L, arith, 'pool', W, dev['src'], None, dev['bias'], None, buf[GUARD:], abuf[GUARD:], dev['ain'], aout if arith == 'h2' else None,
                  (1, T, Fq, cin, cout), 1, single=single)
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isnan(buf).all()) and bool((abuf == 0xEE).all()) and float(aout.abs().max()) == 0.0
    need = L.mtl_conv3x3_wgrad_x3_workspace(1, T, Fq, cin, cout, 1)
    ws = torch.full((need // 4,), float('nan')).cuda()
    wbuf, dw = guarded((cout, cin, 3, 3), fill=0.5)
    bbuf, db = guarded((cout,), fill=0.25)
    wdev = dict(x=dev['src'], dy=buf[GUARD:], am=abuf[GUARD:], ax=dev['ain'], ady=dev['ain'])
    assert wgrad_call(L, arith, False, wdev, dw, db, ws, need, (1, T, Fq, cin, cout), 1) == 0
    torch.cuda.synchronize()
    assert bool((dw == 0.5).all()) and bool((db == 0.25).all()) and guards_intact(wbuf) and guards_intact(bbuf) and bool(torch.isnan(ws).all())
    run_case(L, 'P64-after-empty', arith, *U.CASES['P64'])
