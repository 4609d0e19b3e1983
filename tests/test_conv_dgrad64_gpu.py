"""The two-piece fp16 ("h2") data gradients with 64 output channels -- conv2's (un-pooling source, 64 -> 64) and conv5's (dense source, the
conv's Cin = 64, Cout = 128) -- through the C ABI (mtl_conv3x3_dgrad_h2 / mtl_conv3x3_dgrad_h2_tb), at the smallest shapes that reach
every branch of the kernel's tile walk and epilogue: ragged last tile row, odd width + edge column, all four arg-max positions, windows at
the image border, the task switch inside a workgroup's tile sequence, per-task frame counts, more tiles than resident workgroups, fewer
tiles than workgroups.

Reference: the fp64 gradient on the CPU (torch autograd of conv2d on the un-pooled upstream gradient, gated by the ReLU of the layer's
input activation), from the fp32 values the kernel is given.  Error bar: the one tests/test_ops_gpu.py applies to the h2 data gradient
(test_conv3x3_two_piece_fp16_is_fp32_class): normwise below 1e-6 and below twice the error of the library's exact-fp32 MFMA kernel on
the same data.  Every case runs twice (bit-identical), NaN guard elements around dx must survive, and every task's amax_dx must be an
upper bound of its max|dx|."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

S = 2048          # MTL_AMAX_FLOATS
GUARD = 4096      # NaN floats in front of and behind dx


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def nhwc(t):      # reference (B, C, F, T) <-> kernel (B, T, F, C)
    return t.permute(0, 3, 2, 1).contiguous()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def make_case(cin, cout, B, T, Fq, pooled, nt):
    """Inputs of `nt` tasks of B samples and the fp64 gradient; task k: its own weights, upstream gradient 32^k times larger."""
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + T + Fq + nt + int(pooled))
    x = torch.relu(torch.randn(nt * B, cin, Fq, T, generator=g))                      # the layer's input activation: its ReLU gates dx
    w = torch.randn(nt, cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin) ** 0.5)
    Tp, Fp = T // 2, Fq // 2
    if pooled:
        dy = torch.randn(nt * B, cout, Fp, Tp, generator=g)
        am = torch.randint(0, 4, dy.shape, generator=g, dtype=torch.uint8)           # bit 0: t parity, bit 1: f parity of the window's maximum
        am[:, :, 0, 0], am[:, :, -1, -1], am[:, :, 0, -1], am[:, :, -1, 0] = 0, 3, 1, 2   # corner windows reach out to / away from the border
    else:
        dy = torch.randn(nt * B, cout, Fq, T, generator=g) * (torch.rand(nt * B, cout, Fq, T, generator=g) > 0.5)
        am = None
    for k in range(nt):
        dy[k * B:(k + 1) * B] *= 32.0 ** k
    want = torch.empty(nt * B, cin, Fq, T, dtype=torch.float64)
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        if pooled:
            dense = torch.zeros(B, cout, Fq, T, dtype=torch.float64)
            a = am[sl].long()
            fi = torch.arange(Fp).view(1, 1, Fp, 1) * 2 + (a >> 1)
            ti = torch.arange(Tp).view(1, 1, 1, Tp) * 2 + (a & 1)
            dense.view(B, cout, -1).scatter_(2, (fi * T + ti).view(B, cout, -1), dy[sl].double().view(B, cout, -1))
        else:
            dense = dy[sl].double()
        x64 = x[sl].double().requires_grad_(True)
        F.conv2d(x64, w[k].double(), padding=1).backward(dense)
        want[sl] = x64.grad * (x[sl] > 0)
    return x, w, dy, am, want


def run_case(L, cin, cout, B, T, Fq, pooled, nt, widths=None, single_abi=False):
    x, w, dy, am, want = make_case(cin, cout, B, T, Fq, pooled, nt)
    xn, dyn = nhwc(x).cuda(), nhwc(dy).cuda()
    amn = nhwc(am).cuda() if pooled else None
    amp = amn.data_ptr() if pooled else None
    nb = (L.mtl_conv3x3_wprep_h2_bytes(cout, cin) + 15) // 16 * 16
    w2f, w2d = torch.empty(nt, nb, dtype=torch.uint8).cuda(), torch.empty(nt, nb, dtype=torch.uint8).cuda()
    wf, wd = torch.empty(nt, 9, cin, cout).cuda(), torch.empty(nt, 9, cout, cin).cuda()
    wdev = w.cuda()
    for k in range(nt):
        assert L.mtl_conv3x3_wprep_h2(st(), wdev[k].data_ptr(), w2f[k].data_ptr(), w2d[k].data_ptr(), cout, cin) == 0
        assert L.mtl_conv3x3_wprep(st(), wdev[k].data_ptr(), wf[k].data_ptr(), wd[k].data_ptr(), cout, cin) == 0
    ady = torch.stack([dyn[k * B:(k + 1) * B].abs().max().reshape(1).repeat(S) for k in range(nt)]).contiguous()
    assert nt == 1 or float(ady[1, 0] / ady[0, 0]) > 16.0                      # the tasks' bounds differ by more than 2^4
    wdp = torch.tensor(widths, dtype=torch.int32).cuda() if widths else None
    n = xn.numel()
    outs = []
    for rep in range(2):
        buf = torch.full((n + 2 * GUARD,), float('nan')).cuda()
        dx = buf[GUARD:GUARD + n].view(xn.shape)
        if widths:
            dx.fill_(-7.0)
        adx = torch.zeros(nt, S).cuda()
        if single_abi:
            assert nt == 1
            rc = L.mtl_conv3x3_dgrad_h2(st(), dyn.data_ptr(), ady.data_ptr(), amp, w2d.data_ptr(), xn.data_ptr(), dx.data_ptr(), adx.data_ptr(),
                                        B, T, Fq, cin, cout)
        else:
            rc = L.mtl_conv3x3_dgrad_h2_tb(st(), dyn.data_ptr(), ady.data_ptr(), amp, w2d.data_ptr(), xn.data_ptr(), dx.data_ptr(), adx.data_ptr(),
                                           B, T, Fq, cin, cout, nt, nb, S, S, wdp.data_ptr() if widths else None, 0)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'guard elements overwritten'
        outs.append((dx.clone(), adx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'not repeatable bit for bit'
    dx, adx = outs[0]
    dxf = torch.empty_like(xn)
    report = []
    for k in range(nt):
        sl = slice(k * B, (k + 1) * B)
        assert L.mtl_conv3x3_dgrad(st(), dyn[sl].data_ptr(), amn[sl].data_ptr() if pooled else None, wd[k].data_ptr(), xn[sl].data_ptr(),
                                   dxf[sl].data_ptr(), B, T, Fq, cin, cout) == 0
        torch.cuda.synchronize()
        rows = min(T, widths[k]) if widths else T
        got, got32, ref = dx[sl, :rows], dxf[sl, :rows], nhwc(want[sl])[:, :rows]
        assert not bool(torch.isnan(got).any())
        e2, e32 = rel(got, ref), rel(got32, ref)
        report.append('task %d: h2 %.2e, fp32 MFMA kernel %.2e' % (k, e2, e32))
        print('dgrad64 cin=%d cout=%d B=%d T=%d F=%d pooled=%s nt=%d widths=%s %s' % (cin, cout, B, T, Fq, pooled, nt, widths, report[-1]))
        assert e2 < 2.0 * e32 + 1e-30 and e2 < 1e-6, report
        assert float(got.abs().max()) > 0
        bound = float(adx[k].view(-1, 32)[:, 0].max())
        assert float(got.abs().max()) <= bound, ('amax_dx below max|dx|', k, bound)
        if widths:       # whole tile rows beyond a task's frames are left out of the launch: their outputs keep the caller's content
            edge = -(-widths[k] // 16) * 16
            assert bool((dx[sl, edge:] == -7.0).all()), k
    return dx


def test_pooled_64_ragged_rows_odd_width_edge_column(L):
    """64 -> 64 from a pooled source, B = 2, T = 18, F = 21: the second tile row holds two rows, the width is odd (the last column comes
    from the edge kernel), every arg-max position occurs, also in the windows at the image border; single-task entry point"""
    am = make_case(64, 64, 2, 18, 21, True, 1)[3]
    assert sorted(am.unique().tolist()) == [0, 1, 2, 3]
    run_case(L, 64, 64, 2, 18, 21, True, 1, single_abi=True)


@pytest.mark.parametrize('Fq', [16, 20])
def test_dense_conv5_form(L, Fq):
    """the conv's Cin = 64, Cout = 128 (the gradient reduces 128 channels into 64), dense source, B = 1, T = 33: three tile rows, the last of one row"""
    run_case(L, 64, 128, 1, 33, Fq, False, 1, single_abi=True)


@pytest.mark.parametrize('cin,cout,T,Fq,pooled', [(64, 64, 18, 21, True), (64, 128, 33, 20, False)])
def test_three_tasks_in_one_launch(L, cin, cout, T, Fq, pooled):
    """per-task weights and per-task bounds more than 16 x apart: a workgroup's tile sequence crosses the task boundaries"""
    run_case(L, cin, cout, 1, T, Fq, pooled, 3)


@pytest.mark.parametrize('cin,cout,T,Fq,pooled', [(64, 64, 34, 21, True), (64, 128, 33, 20, False)])
def test_three_tasks_with_widths(L, cin, cout, T, Fq, pooled):
    """... with frame counts of their own, one task much shorter"""
    run_case(L, cin, cout, 1, T, Fq, pooled, 3, widths=[T, T - 5, 4])


def test_more_tiles_than_resident_workgroups(L):
    """64 -> 64, pooled, B = 8, T = 256, F = 80: 640 tiles of 16 x 16 pixels for at most 2 x 256 workgroups -- a workgroup finishes a tile and starts another"""
    run_case(L, 64, 64, 8, 256, 80, True, 1)


def test_fewer_tiles_than_workgroups(L):
    """one tile (pooled) and two tiles (dense): the grid is the tile count"""
    run_case(L, 64, 64, 1, 10, 12, True, 1)
    run_case(L, 64, 128, 1, 20, 16, False, 1)
