"""What the SLIM addressing of the forward / pool epilogues and of conv7's un-pooling data gradient (csrc/mtl_mfma.hip: scalar base + one
32-bit lane offset per store, lane terms re-derived inside the epilogue, bias from a scalar base) can get wrong, on top of the edge suite
of tests/test_conv_edges_gpu.py whose conventions and helpers this file uses: the C ABI entry points, fp64 truths from the fp32 values
the kernel is given, the per-element bound of tests/conv_edge_util.py AND the bar of test_conv3x3_two_piece_fp16_is_fp32_class (normwise
below 1e-6 and below twice the exact-fp32 kernel's error), two bit-identical runs, NaN / 0xEE guards around the outputs, every task's
amax_out an upper bound of its max|out|, arg-max codes = the first maximum in window order of the device's own un-pooled values.

Routes (dispatch_conv_x3): (64, 64) pool / plain -> <64, 2, ., POOL / RELU, 2, WN = 1>; (64, 128) plain -> <128, 2, ., RELU, 2>;
(128, 128) pool -> <128, 2, ., POOL, 2>; (128, 128) un-pooling data gradient -> <128, 2, UNPOOL, DGRAD, 2>.
Shapes: 18 x 17 (odd width, ragged last tile row and column, a one-wide last pool window), 16 x 16 (one exact tile, fewer tiles than
workgroups, the single-task entry points), three tasks of one 34 x 33 image with weights, bias and scales of their own, the same with
frame counts of their own, and about 2.5 tiles per resident workgroup in two tasks (a workgroup's tile sequence crosses the task switch:
bias, scales and bounds are re-read inside it).
The launcher guard of the 32-bit lane offsets (x3h_lane_offsets_fit) is a constexpr function of the channel count; its values just
below and at the limit are static_asserts next to it, checked by every build."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_edge_util as U
from tests import test_conv_edges_gpu as E

pytestmark = pytest.mark.gpu

ROUTES = [('pool', 64, 64), ('relu', 64, 64), ('relu', 64, 128), ('pool', 128, 128), ('dgrad_p', 128, 128)]
IDS = ['%s-%d-%d' % r for r in ROUTES]


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


@pytest.mark.parametrize('kind,cin,cout', ROUTES, ids=IDS)
def test_ragged_tiles_odd_width(L, kind, cin, cout):
    E.run_case(L, 'SLIM-18x17', 'h2', kind, cin, cout, 2, 18, 17)


@pytest.mark.parametrize('kind,cin,cout', ROUTES, ids=IDS)
def test_one_exact_tile(L, kind, cin, cout):
    E.run_case(L, 'SLIM-16x16', 'h2', kind, cin, cout, 1, 16, 16, single=True)


@pytest.mark.parametrize('kind,cin,cout', ROUTES, ids=IDS)
def test_three_tasks_of_their_own_weights_bias_and_scales(L, kind, cin, cout):
    """three tasks of one 34 x 33 image, per-task weights, bias and scales, task k's data 32^k times larger.  (27 tiles are fewer than
    the workgroups of a launch: every tile starts from its own task's bias and scales; a workgroup that walks from one task INTO the
    next is test_more_tiles_than_resident_workgroups.)"""
    E.run_case(L, 'SLIM-TASKS-34x33', 'h2', kind, cin, cout, 1, 34, 33, nt=3)


@functools.lru_cache(maxsize=None)
def stacked(kind, cin, cout, T, Fq):
    """tests/test_conv_edges_gpu.py::stacked_case at a shape of its own (wshift 0): three tasks of B = 1 at a common T with frame
    counts of their own, junk beyond every task's frames, and per task the fp64 result of its own cropped image"""
    c = U.make_case(kind, cin, cout, 1, T, Fq, 3)
    widths = [T, T - 5, 4]
    g = torch.Generator().manual_seed(T + Fq + cin + cout)
    truths = []
    if kind in ('relu', 'pool'):
        stack = dict(src=c['x'].clone())
        for k, r in enumerate(widths):
            stack['src'][k, r:] = torch.randn(T - r, Fq, cin, generator=g) * 100.0 * 32.0 ** k
            y, Sy = U.fwd_truth(c['x'][k:k + 1, :r], c['w'][k], c['b'][k])
            truths.append((U.pool_first_max(y)[0], U.pool_max(Sy)) if kind == 'pool' else (y, Sy))
        stack['ain'] = E.amax_of(c['x'], 3)
    else:
        stack = dict(src=c['dy'].clone(), act=c['act'].clone())
        for k, r in enumerate(widths):
            rp = r // 2
            stack['src'][k, rp:] = torch.randn(T // 2 - rp, Fq // 2, cout, generator=g) * 100.0 * 32.0 ** k
            stack['act'][k, r:] = torch.rand(T - r, Fq, cin, generator=g)
            dense = U.unpool(c['dy'][k:k + 1, :rp], c['am'][k:k + 1, :rp], r, Fq)
            truths.append(U.dgrad_truth(dense, c['w'][k], c['act'][k:k + 1, :r]))
        stack['ain'] = E.amax_of(c['dy'], 3)
    return c, widths, stack, truths


@pytest.mark.parametrize('kind,cin,cout', ROUTES, ids=IDS)
def test_tasks_with_frame_counts_of_their_own(L, kind, cin, cout):
    """`widths` = 34, 29, 4 rows: task 1 ends inside its last tile row, task 2 has one tile row (the compacted tile index space).  Every
    task against the convolution of its OWN image, tile rows wholly beyond a task's frames untouched, bounds per task"""
    T, Fq = 34, 33
    c, widths, stack, truths = stacked(kind, cin, cout, T, Fq)
    dims = (1, T, Fq, cin, cout)
    W = E.prep_weights(L, 'h2', c['w'])
    wdev = torch.tensor(widths, dtype=torch.int32).cuda()
    dev = dict(src=E.padded(stack['src']), ain=stack['ain'].cuda())
    if kind.startswith('dgrad'):
        dev.update(am=c['am'].cuda(), act=E.padded(stack['act']))
        assert L.mtl_zero_tails(E.st(), dev['src'].data_ptr(), 3, T // 2, (Fq // 2) * cout, wdev.data_ptr(), 1, 1) == 0
        assert L.mtl_zero_tails(E.st(), dev['act'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), 0, 1) == 0
    else:
        dev.update(bias=c['b'].cuda())
        assert L.mtl_zero_tails(E.st(), dev['src'].data_ptr(), 3, T, Fq * cin, wdev.data_ptr(), 0, 1) == 0
    out, codes, aout = E.launch_twice(L, 'h2', kind, W, dev, dims, 3, widths=wdev, wshift=0, fill=-7.0)
    K = 9 * (cin if kind in ('relu', 'pool') else cout)
    div = 2 if kind == 'pool' else 1
    for k, r in enumerate(widths):
        want, Ssum = truths[k]
        got = out[k:k + 1, :r // div].double().cpu()
        assert got.shape == want.shape and not bool(torch.isnan(got).any())
        err, bd = (got - want).abs(), U.bound(Ssum, K, 'h2')
        e = U.rel(got, want)
        print('conv_fwd_epilogue stacked %s %d->%d task %d (rows %d of %d): kernel %.2e' % (kind, cin, cout, k, r, T, e))
        assert bool((err <= bd).all()) and e < 1e-6, (kind, k, e)
        edge = -(-r // 16) * 16 // div
        assert bool((out[k, edge:] == -7.0).all()), (kind, k)
        assert float(got.abs().max()) <= float(aout[k].view(-1, 32)[:, 0].max())
    if kind == 'pool':                                   # the codes of the computed windows, against the device's own un-pooled values
        y, _, _ = E.launch_twice(L, 'h2', 'relu', W, dev, dims, 3, want_amax=False, widths=wdev, wshift=0, fill=-7.0)
        for k, r in enumerate(widths):
            p_own, codes_own = U.pool_first_max(y[k:k + 1, :r].cpu())
            assert torch.equal(E.bits(out[k:k + 1, :r // 2].cpu()), E.bits(p_own)) and torch.equal(codes[k:k + 1, :r // 2].cpu(), codes_own)


def test_more_tiles_than_resident_workgroups(L):
    """(64, 64) + pool, two workgroups per compute unit resident, about 2.5 tiles each, the B = 2 images as two tasks with weights, bias
    and scales of their own (task 1's data 32 times larger): every workgroup runs the epilogue several times with a new scalar base,
    the last round only on some, and most walk from task 0 into task 1.  One fp64 convolution per task as the truth (the normwise bar)."""
    cin = cout = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nt, Fq = 2, 401
    ntf = -(-Fq // 16)
    ntt = -(-(5 * 2 * cus) // (2 * nt * ntf))            # 2.5 x (2 cus) tiles
    T = 16 * ntt - 14                                    # the last tile row holds one pool row
    assert nt * ntt * ntf > 2 * 2 * cus and T * Fq * nt * cin * 4 < 128 << 20
    g = torch.Generator().manual_seed(11)
    scale = (32.0 ** torch.arange(nt)).view(nt, 1, 1, 1)
    x = torch.relu(torch.randn(nt, T, Fq, cin, generator=g)) * scale
    w = torch.randn(nt, cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin) ** 0.5)
    b = torch.randn(nt, cout, generator=g) * 0.1 * scale.view(nt, 1)
    dims = (1, T, Fq, cin, cout)
    W = E.prep_weights(L, 'h2', w)
    dev = dict(src=E.padded(x), bias=b.cuda(), ain=E.amax_of(x, nt).cuda())
    out, codes, aout = E.launch_twice(L, 'h2', 'pool', W, dev, dims, nt)
    assert not bool(torch.isnan(out).any())
    for k in range(nt):
        want = U.pool_first_max(U.ref(torch.relu(F.conv2d(U.ref(x[k:k + 1].double()), w[k].double(), b[k].double(), padding=1))))[0]
        _, o32 = E.guarded(out[k:k + 1].shape)
        c32 = torch.empty(o32.shape, dtype=torch.uint8).cuda()
        assert E.call_fp32(L, 'pool', W, k, dev['src'][k:k + 1], None, dev['bias'][k], None, o32, c32, dims) == 0
        torch.cuda.synchronize()
        e, e32 = U.rel(out[k:k + 1], want), U.rel(o32, want)
        print('conv_fwd_epilogue MANY pool 64->64 task %d, %d x %d (%d tiles, %d compute units): kernel %.2e, fp32 kernel %.2e'
              % (k, T, Fq, nt * ntt * ntf, cus, e, e32))
        assert e < 1e-6 and e < 2.0 * e32 + 1e-30
        m, bnd = float(out[k].abs().max()), float(aout[k].view(-1, 32)[:, 0].max())
        assert 0 < m <= bnd <= 8.0 * m
    y, _, _ = E.launch_twice(L, 'h2', 'relu', W, dev, dims, nt, want_amax=False)
    p_own, codes_own = U.pool_first_max(y.cpu())
    assert torch.equal(E.bits(out.cpu()), E.bits(p_own)), 'pooled values are not the maxima of the un-pooled forward'
    assert torch.equal(codes.cpu(), codes_own), 'arg-max codes are not the first maximum in window order'
