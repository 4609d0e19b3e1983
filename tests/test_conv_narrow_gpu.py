"""The 32-channel convolutions of the large_cnn front-end through the C ABI, against the fp64 truths and the PER-ELEMENT bound of
tests/conv_edge_util.py in the exact split ("x3"): (Cin, Cout) = (32, 32) -- ReLU + pool forward, un-pooling data gradient, pooled
weight gradient -- and (32, 64) -- ReLU forward, dense data gradient, dense weight gradient -- each in its single-task and its
several-task (`_tb`) form, and conv0 with 32 output channels.  csrc/mtl_conv_narrow.hip serves these shapes behind the x3 entry points.
Every case: return code 0, two runs bit-identical, NaN guards around the float outputs and 0xEE guards around the arg-max bytes intact,
the input inside a buffer of 1e4 max|x|, no NaN, every element inside bound(S, K, 'x3'), the normwise x3 criteria of
tests/test_conv_edges_gpu.py (3e-6 forward, 1e-5 data gradient).  Pool forwards are compared BITWISE with the 2 x 2 first-maximum
pooling of the kernel's own un-pooled forward.  That these assertions can fail: tests/test_conv_narrow_ref.py (CPU)."""
import functools

import pytest
import torch

from tests import conv_edge_util as U
from tests.narrow_cases import CASES, CONV0, ONE, STACKED, TASK_CASES, WGRAD
from tests.test_conv_edges_gpu import GUARD, bits, guarded, guards_intact, padded, ptr

pytestmark = pytest.mark.gpu
EINVAL = -22


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def prep_weights(L, w):
    """per-task prepared x3 weights (byte stride nb)"""
    nt, cout, cin = w.shape[:3]
    wdev = w.cuda()
    nb = 3 * 9 * cin * cout * 2
    pf, pd = torch.empty(nt, nb, dtype=torch.uint8).cuda(), torch.empty(nt, nb, dtype=torch.uint8).cuda()
    for k in range(nt):
        assert L.mtl_conv3x3_wprep_x3(st(), wdev[k].data_ptr(), pf[k].data_ptr(), pd[k].data_ptr(), cout, cin) == 0
    return dict(f=pf, d=pd, nb=nb)


def call(L, kind, W, dev, out, am_out, dims, nt, widths=None, wshift=0, single=False):
    """one launch of the x3 entry point for `kind`; dims = (B per task, T, F, Cin, Cout) of the forward convolution"""
    B, T, Fq, cin, cout = dims
    src, am_in, bias, act = dev['src'], dev.get('am'), dev.get('bias'), dev.get('act')
    if single:
        assert nt == 1 and widths is None
        if kind == 'relu':
            return L.mtl_conv3x3_relu_fwd_x3(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), B, T, Fq, cin, cout)
        if kind == 'pool':
            return L.mtl_conv3x3_relu_pool_fwd_x3(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), B, T, Fq, cin, cout)
        return L.mtl_conv3x3_dgrad_x3(st(), ptr(src), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), B, T, Fq, cin, cout)
    nb, wp = W['nb'], ptr(widths)
    if kind == 'relu':
        return L.mtl_conv3x3_relu_fwd_x3_tb(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), B, T, Fq, cin, cout, nt, nb, cout, wp, wshift)
    if kind == 'pool':
        return L.mtl_conv3x3_relu_pool_fwd_x3_tb(st(), ptr(src), ptr(W['f']), ptr(bias), ptr(out), ptr(am_out), B, T, Fq, cin, cout, nt, nb, cout,
                                                 wp, wshift)
    return L.mtl_conv3x3_dgrad_x3_tb(st(), ptr(src), ptr(am_in), ptr(W['d']), ptr(act), ptr(out), B, T, Fq, cin, cout, nt, nb, wp, wshift)


def out_shape(kind, n, T, Fq, cin, cout):
    return (n, T // 2, Fq // 2, cout) if kind == 'pool' else (n, T, Fq, cout if kind == 'relu' else cin)


def launch_twice(L, kind, W, dev, dims, nt, **kw):
    """two launches into fresh guarded outputs: (out, arg-max codes or None), bit-identical, guards intact"""
    B, T, Fq, cin, cout = dims
    runs = []
    for rep in range(2):
        buf, out = guarded(out_shape(kind, nt * B, T, Fq, cin, cout), fill=kw.get('fill'))
        abuf, am_out = guarded(out.shape, torch.uint8) if kind == 'pool' else (None, None)
        assert call(L, kind, W, dev, out, am_out, dims, nt, widths=kw.get('widths'), wshift=kw.get('wshift', 0), single=kw.get('single', False)) == 0
        torch.cuda.synchronize()
        assert guards_intact(buf) and (abuf is None or guards_intact(abuf)), 'guard elements overwritten'
        runs.append((out.clone(), am_out.clone() if am_out is not None else None))
    for a, b in zip(*runs):
        assert a is None or torch.equal(bits(a), bits(b)), 'not repeatable bit for bit'
    return runs[0]


def to_device(c, kind):
    if kind in ('relu', 'pool'):
        return dict(src=padded(c['x']), bias=c['b'].cuda())
    return dict(src=padded(c['dy']), am=c['am'].cuda() if c['am'] is not None else None, act=c['act'].cuda())


def task_slice(dev, k, B):
    sl = slice(k * B, (k + 1) * B)
    d = dict(src=dev['src'][sl])
    if 'bias' in dev:
        d['bias'] = dev['bias'][k]
    if 'act' in dev:
        d.update(act=dev['act'][sl], am=dev['am'][sl] if dev.get('am') is not None else None)
    return d


def compare(name, kind, k, got, want, bd):
    got = got.double().cpu()
    assert not bool(torch.isnan(got).any()), name
    err = (got - want).abs()
    pos = bd > 0
    ratio = float((err[pos] / bd[pos]).max()) if bool(pos.any()) else 0.0
    e = U.rel(got, want)
    line = 'conv_narrow %s x3 %s task %d: kernel %.2e, max error / bound %.4f' % (name, kind, k, e, ratio)
    print(line)
    assert bool((err <= bd).all()), line
    assert e < (1e-5 if kind.startswith('dgrad') else 3e-6), line


def run_case(L, name, kind, cin, cout, B, T, Fq, nt=1, variant='', single=False):
    c = U.make_case(kind, cin, cout, B, T, Fq, nt, variant)
    dims = (B, T, Fq, cin, cout)
    W = prep_weights(L, c['w'])
    dev = to_device(c, kind)
    out, codes = launch_twice(L, kind, W, dev, dims, nt, single=single)
    truth, Ssum = {'relu': ('y', 'Sy'), 'pool': ('p', 'Sp')}.get(kind, ('dx', 'Sdx'))
    K = 9 * (cin if kind in ('relu', 'pool') else cout)
    tag = name + (':' + variant if variant else '')
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        compare(tag, kind, k, out[sl], c[truth][sl], U.bound(c[Ssum][sl], K, 'x3'))
        if nt > 1:      # every task of the several-task launch: bit for bit its single-task launch
            Wk = dict(f=W['f'][k:k + 1], d=W['d'][k:k + 1], nb=W['nb'])
            o1, c1 = launch_twice(L, kind, Wk, task_slice(dev, k, B), dims, 1, single=True)
            assert torch.equal(bits(out[sl]), bits(o1)) and (codes is None or torch.equal(codes[sl], c1)), (tag, k)
    if kind != 'pool':
        return out
    # the pooling rule: bitwise the 2 x 2 maxima and first-maximum codes of the kernel's own un-pooled forward
    y, _ = launch_twice(L, 'relu', W, dev, dims, nt, single=single)
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        compare(tag + ':unpooled', 'relu', k, y[sl], c['y'][sl], U.bound(c['Sy'][sl], K, 'x3'))
    p_own, codes_own = U.pool_first_max(y.cpu())
    assert torch.equal(bits(out.cpu()), bits(p_own)), 'pooled values are not the maxima of the un-pooled forward'
    assert torch.equal(codes.cpu(), codes_own), 'arg-max codes are not the first maximum in window order'
    if variant == 'ZERO':
        assert float(out.abs().max()) == 0.0 and int(codes.sum()) == 0
    if variant == 'CONST':       # windows whose 4 x 4 neighbourhood lies inside the image see the same inputs per pixel: exact ties
        assert int(codes[:, 1:(T - 2) // 2, 1:(Fq - 2) // 2].sum()) == 0 and float(out.max()) > 0
    return out


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('name', ['P32', 'R64', 'D32p', 'D64d'])
def test_edge_case(L, name):
    run_case(L, name, *CASES[name])


@pytest.mark.parametrize('kind,cin,cout,B,T,Fq', ONE)
def test_one_window_one_pixel(L, kind, cin, cout, B, T, Fq):
    """every tap but the centre reads padding (T = 1, F = 17: the centre row of taps); the grid is one tile; single-task entry points"""
    run_case(L, 'ONE-%d-%dx%d' % (cout, T, Fq), kind, cin, cout, B, T, Fq, single=True)


def test_many32_more_tiles_than_resident_workgroups(L):
    kind, cin, cout, B, T, Fq = CASES['MANY32']
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-(Fq // 2 * 2) // 16) * -(-(T // 2 * 2) // 8) * B > 2 * cus
    run_case(L, 'MANY32', kind, cin, cout, B, T, Fq)


@pytest.mark.parametrize('name', TASK_CASES)
def test_three_tasks_in_one_launch(L, name):
    """per-task weights and bias, operands 32 x apart: a workgroup's tile sequence crosses the task boundaries (weights re-staged)"""
    kind, cin, cout, _, T, Fq = CASES[name]
    run_case(L, 'TASKS-' + name, kind, cin, cout, 1, T, Fq, nt=3)


@pytest.mark.parametrize('variant', ['ZERO', 'CONST'])
def test_pool_ties(L, variant):
    """ZERO: every window is four ReLU zeros -- output 0, code 0.  CONST: interior windows are exact ties -- code 0."""
    run_case(L, 'P32', *CASES['P32'], variant=variant)


# ------------------------------------------------------------------------------------------------ stacked tasks against their own images
@functools.lru_cache(maxsize=None)
def stacked_case(name, wshift):
    """three tasks of B = 1 at a common T with frame counts of their own (given at full resolution): the stack with junk beyond every
    task's frames, and per task the fp64 result of its own cropped image (as tests/test_conv_edges_gpu.stacked_case; dense sources too)"""
    kind, cin, cout, _, T, Fq = CASES[name]
    c = U.make_case(kind, cin, cout, 1, T, Fq, 3)
    widths = [T << wshift, (T << wshift) - (9 if wshift else 5), 4 << wshift]
    rows = [wd >> wshift for wd in widths]
    assert rows == [T, T - 5, 4]
    g = torch.Generator().manual_seed(T + Fq + wshift + cout)
    truths = []
    if kind in ('relu', 'pool'):
        stack = dict(src=c['x'].clone())
        for k, r in enumerate(rows):
            stack['src'][k, r:] = torch.randn(T - r, Fq, cin, generator=g) * 100.0 * 32.0 ** k
            y, Sy = U.fwd_truth(c['x'][k:k + 1, :r], c['w'][k], c['b'][k])
            truths.append((U.pool_first_max(y)[0], U.pool_max(Sy)) if kind == 'pool' else (y, Sy))
    else:
        stack = dict(src=c['dy'].clone(), act=c['act'].clone())
        for k, r in enumerate(rows):
            rs = r // 2 if kind == 'dgrad_p' else r                                   # rows of the task in the gradient it is given
            stack['src'][k, rs:] = torch.randn(stack['src'].shape[1] - rs, *stack['src'].shape[2:], generator=g) * 100.0 * 32.0 ** k
            stack['act'][k, r:] = torch.rand(T - r, Fq, cin, generator=g)
            dense = U.unpool(c['dy'][k:k + 1, :rs], c['am'][k:k + 1, :rs], r, Fq) if kind == 'dgrad_p' else c['dy'][k:k + 1, :r]
            truths.append(U.dgrad_truth(dense, c['w'][k], c['act'][k:k + 1, :r]))
    return c, widths, rows, stack, truths


@pytest.mark.parametrize('name,wshift', STACKED)
def test_stacked_tasks_meet_their_own_borders(L, name, wshift):
    """mtl_zero_tails + the `widths` form of a launch give every task the convolution of its OWN image: rows below widths[k] >> wshift
    are inside the bound of the fp64 result of the cropped image; tile rows wholly beyond a task's frames are not written (a tile row
    is at most 16 frames in every kernel behind these entry points)"""
    kind, cin, cout, _, T, Fq = CASES[name]
    c, widths, rows, stack, truths = stacked_case(name, wshift)
    dims = (1, T, Fq, cin, cout)
    W = prep_weights(L, c['w'])
    wdev = torch.tensor(widths, dtype=torch.int32).cuda()
    dev = dict(src=padded(stack['src']))
    if kind.startswith('dgrad'):
        dev.update(am=c['am'].cuda() if c['am'] is not None else None, act=padded(stack['act']))
        if kind == 'dgrad_p':
            assert L.mtl_zero_tails(st(), dev['src'].data_ptr(), 3, T // 2, (Fq // 2) * cout, wdev.data_ptr(), wshift + 1, 1) == 0
        else:
            assert L.mtl_zero_tails(st(), dev['src'].data_ptr(), 3, T, Fq * cout, wdev.data_ptr(), wshift, 1) == 0
        assert L.mtl_zero_tails(st(), dev['act'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), wshift, 1) == 0
    else:
        dev.update(bias=c['b'].cuda())
        assert L.mtl_zero_tails(st(), dev['src'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), wshift, 1) == 0
    for k, r in enumerate(rows):
        rr = r // 2 if kind == 'dgrad_p' else r
        assert float(dev['src'][k, rr:].abs().sum()) == 0.0 and torch.equal(dev['src'][k, :rr].cpu(), stack['src'][k, :rr])
    out, codes = launch_twice(L, kind, W, dev, dims, 3, widths=wdev, wshift=wshift, fill=-7.0)
    K = 9 * (cin if kind in ('relu', 'pool') else cout)
    div = 2 if kind == 'pool' else 1
    for k, r in enumerate(rows):
        want, Ssum = truths[k]
        got = out[k:k + 1, :r // div].double().cpu()
        assert got.shape == want.shape and not bool(torch.isnan(got).any())
        err, bd = (got - want).abs(), U.bound(Ssum, K, 'x3')
        pos = bd > 0
        print('conv_narrow stacked-%s x3 %s task %d (rows %d of %d, wshift %d): kernel %.2e, max error / bound %.4f'
              % (name, kind, k, r, T, wshift, U.rel(got, want), float((err[pos] / bd[pos]).max())))
        assert bool((err <= bd).all()), (name, k)
        edge = -(-r // 16) * 16 // div                             # the first output row of the first tile row wholly beyond the frames
        assert bool((out[k, edge:] == -7.0).all()), (name, k)
    assert bool((out[2, 16 // div:] == -7.0).all()) and out[2, 16 // div:].numel() > 0


@pytest.mark.parametrize('name', TASK_CASES)
@pytest.mark.parametrize('wshift', [9, -1])
def test_wshift_out_of_range_is_refused(L, name, wshift):
    kind, cin, cout = CASES[name][:3]
    T, Fq = 4, 4
    c = U.make_case(kind, cin, cout, 1, T, Fq, 1)
    W = prep_weights(L, c['w'])
    dev = to_device(c, kind)
    wdev = torch.tensor([T], dtype=torch.int32).cuda()
    buf, out = guarded(out_shape(kind, 1, T, Fq, cin, cout), fill=-7.0)
    abuf, am_out = guarded(out.shape, torch.uint8)
    rc = call(L, kind, W, dev, out, am_out, (1, T, Fq, cin, cout), 1, widths=wdev, wshift=wshift)
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((out == -7.0).all()) and bool((am_out == 0xEE).all()) and guards_intact(buf) and guards_intact(abuf)


def test_shapes_nobody_serves_are_still_refused(L):
    """(Cin, Cout) = (64, 32) and (32, 96) forwards, a (32, 128) weight gradient: MTL_EINVAL, nothing written"""
    T, Fq = 4, 4
    for cin, cout in ((64, 32), (32, 96)):
        x = torch.randn(1, T, Fq, cin).cuda()
        W = prep_weights(L, torch.randn(1, cout, cin, 3, 3) * 0.05)
        buf, out = guarded((1, T, Fq, cout), fill=-7.0)
        rc = L.mtl_conv3x3_relu_fwd_x3(st(), x.data_ptr(), W['f'].data_ptr(), torch.zeros(cout).cuda().data_ptr(), out.data_ptr(), 1, T, Fq, cin, cout)
        torch.cuda.synchronize()
        assert rc == EINVAL and bool((out == -7.0).all()) and guards_intact(buf)
    assert L.mtl_conv3x3_wgrad_x3_workspace(1, T, Fq, 32, 128, 0) == 0


# ------------------------------------------------------------------------------------------------ weight gradients
def wgrad_call(L, tb, dev, dw, db, ws, need, dims, nt):
    B, T, Fq, cin, cout = dims
    x, dy, am = dev['x'], dev['dy'], dev.get('am')
    if tb or db is not None:                                         # (the single-task x3 entry point has no bias gradient)
        return L.mtl_conv3x3_wgrad_x3_tb(st(), ptr(x), ptr(dy), ptr(am), ptr(dw), ptr(db), ptr(ws), need, B, T, Fq, cin, cout, nt, 9 * cin * cout, cout)
    return L.mtl_conv3x3_wgrad_x3(st(), ptr(x), ptr(dy), ptr(am), ptr(dw), ptr(ws), need, B, T, Fq, cin, cout)


@pytest.mark.parametrize('nt', [1, 3])
@pytest.mark.parametrize('cin,cout,B,T,Fq,pooled', WGRAD)
def test_wgrad_edges(L, cin, cout, B, T, Fq, pooled, nt):
    """arbitrary arg-max codes, 30 % zeros: dw and db per element inside bound(S, K = pixels, 'x3'), per tap normwise < 2e-6; db = NULL:
    the same dw bits, db untouched; accumulation onto pre-fills; workspace of exactly the reported size"""
    c = U.make_wgrad_case(cin, cout, B, T, Fq, nt, pooled)
    dims = (B, T, Fq, cin, cout)
    dev = dict(x=padded(c['x']), dy=padded(c['dy']), am=c['am'].cuda() if pooled else None)
    need = L.mtl_conv3x3_wgrad_x3_workspace(B, T, Fq, cin, cout, int(pooled))
    assert need > 0 and need % 4 == 0
    slabs = need // (9 * cin * cout * 4 + cout * 4)
    K = B * (T // 2 * 2 if pooled else T) * (Fq // 2 * 2 if pooled else Fq)
    bd_w, bd_b = U.bound(c['Sdw'], K, 'x3'), U.bound(c['Sdb'], K, 'x3')

    def run(pre_w, pre_b, with_db):
        res = []
        for rep in range(2):
            wsbuf = torch.full((need // 4 + GUARD,), float('nan')).cuda()
            wbuf, dw = guarded((nt, cout, cin, 3, 3), fill=pre_w)
            bbuf, db = guarded((nt, cout), fill=pre_b)
            assert wgrad_call(L, nt > 1, dev, dw, db if with_db else None, wsbuf, need, dims, nt) == 0
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
        print('conv_narrow wgrad-%dx%d-%dx%d x3 %s task %d of %d: worst tap %.2e, db %.2e, max error / bound %.4f (dw) %.4f (db)'
              % (cin, cout, T, Fq, 'pooled' if pooled else 'dense', k, nt, taps, U.rel(gb, c['db'][k]),
                 float((ew[pw] / bd_w[k][pw]).max()), float((eb / bd_b[k].clamp_min(1e-300)).max())))
        assert taps < 2e-6
        assert bool((ew <= bd_w[k]).all()) and bool((eb <= bd_b[k]).all())
    # accumulation onto pre-fills: the one further addition rounds to half an ulp of a sum below |pre-fill| + S
    aw, ab = run(0.5, 0.25, True)
    for k in range(nt):
        ew, eb = (aw[k].double().cpu() - (0.5 + c['dw'][k])).abs(), (ab[k].double().cpu() - (0.25 + c['db'][k])).abs()
        assert bool((ew <= bd_w[k] + 2.0 ** -23 * (0.5 + c['Sdw'][k])).all())
        assert bool((eb <= bd_b[k] + 2.0 ** -23 * (0.25 + c['Sdb'][k])).all())
    assert slabs >= nt


# ------------------------------------------------------------------------------------------------ empty extents
@pytest.mark.parametrize('T,Fq', [(1, 5), (5, 1)])
def test_empty_pool_extent_is_a_no_op(L, T, Fq):
    """T < 2 or F < 2: a pooled forward has no output and a pooled weight gradient no window -- success, nothing written; the next call is sound"""
    cin = cout = 32
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(1, T, Fq, cin, generator=g))
    W = prep_weights(L, torch.randn(1, cout, cin, 3, 3, generator=g) * 0.05)
    dev = dict(src=padded(x), bias=torch.zeros(1, cout).cuda())
    for single in (True, False):
        buf, out = guarded((0,))
        abuf, am_out = guarded((0,), torch.uint8)
        rc = call(L, 'pool', W, dev, buf[GUARD:], abuf[GUARD:], (1, T, Fq, cin, cout), 1, single=single)
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isnan(buf).all()) and bool((abuf == 0xEE).all())
    need = L.mtl_conv3x3_wgrad_x3_workspace(1, T, Fq, cin, cout, 1)
    ws = torch.full((need // 4,), float('nan')).cuda()
    wbuf, dw = guarded((cout, cin, 3, 3), fill=0.5)
    bbuf, db = guarded((cout,), fill=0.25)
    wdev = dict(x=dev['src'], dy=buf[GUARD:], am=abuf[GUARD:])
    assert wgrad_call(L, False, wdev, dw, db, ws, need, (1, T, Fq, cin, cout), 1) == 0
    torch.cuda.synchronize()
    assert bool((dw == 0.5).all()) and bool((db == 0.25).all()) and guards_intact(wbuf) and guards_intact(bbuf) and bool(torch.isnan(ws).all())
    run_case(L, 'P32-after-empty', *CASES['P32'])


# ------------------------------------------------------------------------------------------------ conv0 with 32 output channels
@functools.lru_cache(maxsize=None)
def conv0_case(T, Fq, nt, shared):
    """nt tasks of B samples: input (B, T, F, 1) per task (shared: one batch for all), weights (32, 1, 3, 3) and bias per task, a gradient with
    30 % zeros; fp64 truths per task"""
    B, C = CONV0['B'], CONV0['C']
    g = torch.Generator().manual_seed(7 * T + 13 * Fq + nt + 100 * shared)
    x = torch.randn(1 if shared else nt, B, T, Fq, 1, generator=g)
    w = torch.randn(nt, C, 1, 3, 3, generator=g) / 3.0
    b = torch.randn(nt, C, generator=g) * 0.1
    dy = torch.randn(nt, B, T, Fq, C, generator=g)
    dy[torch.rand(dy.shape, generator=g) < 0.3] = 0.0
    xs = [x[0 if shared else k] for k in range(nt)]
    fw = [U.fwd_truth(xs[k], w[k], b[k]) for k in range(nt)]
    wg = [U.wgrad_truth(xs[k], dy[k]) for k in range(nt)]
    return dict(x=x, w=w, b=b, dy=dy, fw=fw, wg=wg)


@pytest.mark.parametrize('nt,shared', [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize('Fq', CONV0['F'])
@pytest.mark.parametrize('T', CONV0['T'])
def test_conv0_with_32_channels(L, T, Fq, nt, shared):
    """forward + ReLU against fwd_truth (K = 9), weight / bias gradient against wgrad_truth (K = pixels): bound(S, K, 'x3') -- conv0 is plain
    fp32 FMA, the x3 constant is the looser; every task of the several-task launches bitwise its single-task forward"""
    B, C = CONV0['B'], CONV0['C']
    c = conv0_case(T, Fq, nt, shared)
    x_ref = padded(c['x'].reshape(-1, T, Fq, 1).permute(0, 3, 2, 1).contiguous())        # the reference's (B, 1, F, T)
    w, b, dy = c['w'].cuda(), c['b'].cuda(), padded(c['dy'].reshape(nt * B, T, Fq, C))
    sX = 0 if shared else B * T * Fq
    buf, y = guarded((nt * B, T, Fq, C))
    if nt > 1:
        assert L.mtl_conv0c_relu_fwd_tb(st(), x_ref.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, Fq, C, None, nt, sX, C * 9, C, 0) == 0
    else:
        assert L.mtl_conv0c_relu_fwd(st(), x_ref.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, Fq, C, None) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf)
    ws = torch.empty(L.mtl_conv0_wgrad_workspace() // 4).cuda()
    wbuf, dw = guarded((nt, C, 1, 3, 3), fill=0.0)
    bbuf, db = guarded((nt, C), fill=0.0)
    if nt > 1:
        assert L.mtl_conv0c_wgrad_tb(st(), x_ref.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, T, Fq, C, nt, sX, C * 9, C) == 0
    else:
        assert L.mtl_conv0c_wgrad(st(), x_ref.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), B, T, Fq, C) == 0
    torch.cuda.synchronize()
    assert guards_intact(wbuf) and guards_intact(bbuf)
    K = B * T * Fq
    for k in range(nt):
        yk = y[k * B:(k + 1) * B]
        want, S = c['fw'][k]
        err = (yk.double().cpu() - want).abs()
        print('conv_narrow conv0-32 %dx%d task %d of %d: forward %.2e' % (T, Fq, k, nt, U.rel(yk, want)))
        assert bool((err <= U.bound(S, 9, 'x3')).all())
        dw_t, Sdw, db_t, Sdb = c['wg'][k]
        assert bool(((dw[k].double().cpu() - dw_t).abs() <= U.bound(Sdw, K, 'x3')).all())
        assert bool(((db[k].double().cpu() - db_t).abs() <= U.bound(Sdb, K, 'x3')).all())
        if nt > 1:
            xk = x_ref[0:B] if shared else x_ref[k * B:(k + 1) * B]
            _, y1 = guarded((B, T, Fq, C))
            assert L.mtl_conv0c_relu_fwd(st(), xk.data_ptr(), w[k].data_ptr(), b[k].data_ptr(), y1.data_ptr(), B, T, Fq, C, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(bits(yk), bits(y1))
    assert L.mtl_conv0c_relu_fwd(st(), x_ref.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), B, T, Fq, 48, None) == EINVAL
