"""The un-pooling data gradients (pooled upstream gradient + one arg-max byte per element) through the C ABI, at the smallest shapes at
which the halo waves' indexing by POOLED source element can go wrong: a pooling window is fetched and split once and committed to the
up to four halo pixels it covers, so what can break is the window <-> halo-pixel map at the halo's and the image's borders.

    T x F     what it exercises
    2 x 2     one window, the halo almost entirely outside the image
    16 x 16   exactly one tile: every edge window of the halo contributes one row or column
    18 x 19   a second, nearly empty tile row; odd F: the last column has no window (Fp = 9) and receives only its neighbours' taps
    35 x 33   several tiles, odd in both directions
    33 x 33   with per-task frame counts (33, 17): the compacted tile index space

Layers: 64 -> 64 (conv2's route; odd F also runs the edge-column kernel) and 128 -> 128 (conv7's route), both arithmetics (h2: two fp16
pieces, x3: three bf16 pieces; x3's 64-channel route is the one-sub-tile form of the kernel).  Every case is ONE launch of two tasks of one
sample each, with weights of their own and upstream gradients 32 x apart, and one single-task launch of the first task, which must agree bit
for bit.  Arg-max codes are uniform over the four positions; one extra case has every code equal to 3, the position reached only through
the + 1 halo row and column.  Reference and bound: the fp64 gradient and the per-element bound of tests/conv_edge_util.py; the largest
error over the bound must be <= 1, as in tests/test_conv_edges_gpu.py."""
import functools

import pytest
import torch

from tests import conv_edge_util as U

pytestmark = pytest.mark.gpu

S = 2048          # MTL_AMAX_FLOATS
GUARD = 4096      # NaN floats in front of and behind dx
NT = 2

SHAPES = {
    'one-window': (2, 2, None, False),
    'one-tile': (16, 16, None, False),
    'odd-width': (18, 19, None, False),
    'odd-both': (35, 33, None, False),
    'widths': (33, 33, (33, 17), False),
    'all-codes-3': (35, 33, None, True),
}


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def make_case(ch, T, Fq, widths, all3):
    """two tasks of one sample: fp32 inputs (rows beyond a task's frames cleared, as the caller of a `widths` launch does) and per task
    the fp64 gradient of its own image with its S"""
    g = torch.Generator().manual_seed(7919 * ch + 131 * T + 17 * Fq + (5 if widths else 0) + (3 if all3 else 0))
    Tp, Fp = T // 2, Fq // 2
    w = torch.randn(NT, ch, ch, 3, 3, generator=g) * (1.0 / (9 * ch) ** 0.5)
    act = torch.relu(torch.randn(NT, T, Fq, ch, generator=g))
    dy = torch.randn(NT, Tp, Fp, ch, generator=g)
    am = torch.full(dy.shape, 3, dtype=torch.uint8) if all3 else torch.randint(0, 4, dy.shape, generator=g, dtype=torch.uint8)
    dy[:, 0, 0, 0] = 40.0                                                # every task's outlier, 10 x above its bulk
    dy = dy * (32.0 ** torch.arange(NT)).view(NT, 1, 1, 1)
    rows = list(widths) if widths else [T] * NT
    truths = []
    for k, r in enumerate(rows):
        dy[k, r // 2:] = 0.0
        act[k, r:] = 0.0
        dense = U.unpool(dy[k:k + 1, :r // 2], am[k:k + 1, :r // 2], r, Fq)
        truths.append(U.dgrad_truth(dense, w[k], act[k:k + 1, :r]))
    return w, act, dy, am, rows, truths


def launch(L, arith, W, nb, dy, ady, am, act, ch, T, Fq, nt, widths, fill):
    """one launch into a fresh guarded dx (nt = 0: the single-task entry point)"""
    n = act.numel()
    buf = torch.full((n + 2 * GUARD,), float('nan')).cuda()
    dx = buf[GUARD:GUARD + n].view(act.shape)
    if fill is not None:
        dx.fill_(fill)
    adx = torch.zeros(max(nt, 1), S).cuda()
    wp = widths.data_ptr() if widths is not None else None
    if arith == 'h2':
        if nt:
            rc = L.mtl_conv3x3_dgrad_h2_tb(st(), dy.data_ptr(), ady.data_ptr(), am.data_ptr(), W.data_ptr(), act.data_ptr(), dx.data_ptr(),
                                           adx.data_ptr(), 1, T, Fq, ch, ch, nt, nb, S, S, wp, 0)
        else:
            rc = L.mtl_conv3x3_dgrad_h2(st(), dy.data_ptr(), ady.data_ptr(), am.data_ptr(), W.data_ptr(), act.data_ptr(), dx.data_ptr(),
                                        adx.data_ptr(), 1, T, Fq, ch, ch)
    elif nt:
        rc = L.mtl_conv3x3_dgrad_x3_tb(st(), dy.data_ptr(), am.data_ptr(), W.data_ptr(), act.data_ptr(), dx.data_ptr(), 1, T, Fq, ch, ch, nt, nb, wp, 0)
    else:
        rc = L.mtl_conv3x3_dgrad_x3(st(), dy.data_ptr(), am.data_ptr(), W.data_ptr(), act.data_ptr(), dx.data_ptr(), 1, T, Fq, ch, ch)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'guard elements overwritten'
    return dx.clone(), adx


@pytest.mark.parametrize('arith', ['h2', 'x3'])
@pytest.mark.parametrize('ch', [64, 128])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_unpool_halo(L, shape, ch, arith):
    T, Fq, widths, all3 = SHAPES[shape]
    w, act, dy, am, rows, truths = make_case(ch, T, Fq, widths, all3)
    if all3:
        assert int(am.min()) == 3
    elif T * Fq > 4:
        assert sorted(am.unique().tolist()) == [0, 1, 2, 3]
    nb = (L.mtl_conv3x3_wprep_h2_bytes(ch, ch) + 15) // 16 * 16 if arith == 'h2' else 3 * 9 * ch * ch * 2
    prep = L.mtl_conv3x3_wprep_h2 if arith == 'h2' else L.mtl_conv3x3_wprep_x3
    wdev = w.cuda()
    pf, pd = torch.empty(NT, nb, dtype=torch.uint8).cuda(), torch.empty(NT, nb, dtype=torch.uint8).cuda()
    for k in range(NT):
        assert prep(st(), wdev[k].data_ptr(), pf[k].data_ptr(), pd[k].data_ptr(), ch, ch) == 0
    dyd, amd, actd = dy.cuda(), am.cuda(), act.cuda()
    ady = torch.stack([dyd[k].abs().max().reshape(1).repeat(S) for k in range(NT)]).contiguous()
    assert float(ady[1, 0] / ady[0, 0]) > 16.0                            # the tasks' operand scales differ
    wd = torch.tensor(widths, dtype=torch.int32).cuda() if widths else None
    fill = -7.0 if widths else None
    dx, adx = launch(L, arith, pd, nb, dyd, ady, amd, actd, ch, T, Fq, NT, wd, fill)
    again, _ = launch(L, arith, pd, nb, dyd, ady, amd, actd, ch, T, Fq, NT, wd, fill)
    assert torch.equal(dx.view(torch.int32), again.view(torch.int32)), 'not repeatable bit for bit'
    for k, r in enumerate(rows):
        want, Ssum = truths[k]
        got = dx[k:k + 1, :r].double().cpu()
        assert got.shape == want.shape and not bool(torch.isnan(got).any())
        err, bd = (got - want).abs(), U.bound(Ssum, 9 * ch, arith)
        pos = bd > 0
        ratio = float((err[pos] / bd[pos]).max()) if bool(pos.any()) else 0.0
        print('unpool_halo %s %d ch %s task %d (rows %d of %d): kernel %.2e, max error / bound %.4f' % (shape, ch, arith, k, r, T, U.rel(got, want), ratio))
        assert bool((err <= bd).all()) and ratio <= 1.0, (shape, ch, arith, k, ratio)
        assert float(got.abs().max()) > 0
        if arith == 'h2':
            assert float(got.abs().max()) <= float(adx[k].view(-1, 32)[:, 0].max()), ('amax_dx below max|dx|', k)
        if widths:       # whole tile rows beyond a task's frames are left out of the launch (8- or 16-row tiles: none reaches past 16 ceil(r / 16))
            assert bool((dx[k, -(-r // 16) * 16:] == -7.0).all()), k
    # the single-task entry point on the first task's operands: the same bits as that task's part of the two-task launch
    one, _ = launch(L, arith, pd[0], nb, dyd[:1], ady[:1], amd[:1], actd[:1], ch, T, Fq, 0, None, None)
    assert rows[0] == T
    assert torch.equal(one.view(torch.int32), dx[:1].view(torch.int32)), 'single-task and two-task launches differ on the shared task'
