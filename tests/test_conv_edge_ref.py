"""CPU checks of tests/conv_edge_util.py: (1) its fp64 truths are torch autograd's, (2) the emulated two-piece fp16 forward stays far
inside the per-element bound, (3) every mutator -- what a kernel with a wrong halo, window, tap, code or bias would produce -- pushes
at least one element beyond that bound, i.e. the assertions of tests/test_conv_edges_gpu.py can fail."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_edge_util as U

SHAPES = [(64, 64, 2, 18, 21), (128, 128, 1, 17, 34), (64, 128, 1, 33, 20)]          # (Cin, Cout, B, T, F)


def _inputs(cin, cout, B, T, Fq, seed=0):
    g = torch.Generator().manual_seed(100 + cin + cout + T + Fq + seed)
    x = torch.relu(torch.randn(B, T, Fq, cin, generator=g))
    x[0, 0, 0, 0] = 40.0
    w = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin) ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    return g, x, w, b


@pytest.mark.parametrize('cin,cout,B,T,Fq', [(8, 12, 2, 7, 9), (4, 4, 1, 2, 2), (6, 4, 2, 1, 5), (4, 8, 1, 8, 6)])
def test_truths_are_torch_autograd(cin, cout, B, T, Fq):
    g = torch.Generator().manual_seed(cin + cout + T + Fq)
    z = torch.randn(B, cin, Fq, T, generator=g, dtype=torch.float64).requires_grad_(True)       # reference layout
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_(True)
    x = torch.relu(z)
    y = torch.relu(F.conv2d(x, w, b, padding=1))
    xk = U.ref(x.detach())
    yk, _ = U.fwd_truth(xk, w.detach(), b.detach())
    assert float((yk - U.ref(y.detach())).abs().max()) <= 1e-12
    # dense backward
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    gz, gw, gb = torch.autograd.grad(y, (z, w, b), dy, retain_graph=True)
    dyk = U.ref(dy * (y.detach() > 0))                           # what the kernels are given: the gradient behind the layer's ReLU
    dx, _ = U.dgrad_truth(dyk, w.detach(), xk)
    dw, _, db, _ = U.wgrad_truth(xk, dyk)
    assert float((dx - U.ref(gz)).abs().max()) <= 1e-12 and float((dw - gw).abs().max()) <= 1e-12 and float((db - gb).abs().max()) <= 1e-12
    if T < 2 or Fq < 2:
        assert U.pool_first_max(yk)[0].numel() == 0
        return
    # pooled forward and backward
    p, idx = F.max_pool2d(y, 2, stride=2, return_indices=True)
    pk, codes = U.pool_first_max(yk)
    assert float((pk - U.ref(p.detach())).abs().max()) <= 1e-12
    tcodes = U.ref((((idx // T) & 1) << 1 | ((idx % T) & 1)).to(torch.uint8))
    uniq = U.unique_max(yk)
    assert bool(uniq.any()) and torch.equal(codes[uniq], tcodes[uniq])
    assert int(codes[(U.windows(yk) == 0).all(-1)].sum()) == 0                    # four ReLU zeros: the first wins, code 0
    dp = torch.randn(p.shape, generator=g, dtype=torch.float64)
    gz, gw, gb = torch.autograd.grad(p, (z, w, b), dp)
    dense = U.unpool(U.ref(dp * (p.detach() > 0)), tcodes, T, Fq)                 # torch's own decisions: one truth
    dx, _ = U.dgrad_truth(dense, w.detach(), xk)
    dw, _, db, _ = U.wgrad_truth(xk, dense)
    assert float((dx - U.ref(gz)).abs().max()) <= 1e-12 and float((dw - gw).abs().max()) <= 1e-12 and float((db - gb).abs().max()) <= 1e-12


@pytest.mark.parametrize('cin,cout,B,T,Fq', SHAPES)
def test_emulated_h2_forward_is_inside_the_bound(cin, cout, B, T, Fq):
    _, x, w, b = _inputs(cin, cout, B, T, Fq)
    y, S = U.fwd_truth(x, w, b)
    got = U.fwd_h2_emul(x, w, b).double()
    bd = U.bound(S, 9 * cin, 'h2')
    ratio = float(((got - y).abs() / bd).max())
    print('emulated h2 fwd (%d,%d,%d,%d,%d): normwise %.2e, max error / bound %.4f' % (cin, cout, B, T, Fq, U.rel(got, y), ratio))
    assert ratio < 1.0 and U.rel(got, y) < 1e-6
    # a lost first-order term (2^-11 per product, random signs) is the normwise criterion's to catch: the per-element bound carries
    # the full K 2^-24 of a worst-case accumulation chain and is the criterion for LOCAL faults (the mutators below)
    worse = U.fwd_h2_emul(x, w, b, terms=((0, 0), (0, 1))).double()
    assert U.rel(worse, y) > 1e-6


def _beyond(got, want, bd):
    return int(((got - want).abs() > bd).sum())


@pytest.mark.parametrize('cin,cout,B,T,Fq', SHAPES)
def test_every_mutator_leaves_the_bound(cin, cout, B, T, Fq):
    g, x, w, b = _inputs(cin, cout, B, T, Fq, seed=1)
    y, S = U.fwd_truth(x, w, b)
    bd = U.bound(S, 9 * cin, 'h2')                               # the wider of the two arithmetics' bounds
    for tap in ((0, 2), (1, 1), (2, 0)):
        ym = U.mut_drop_tap(x, w, b, pix=(0, 1, 1), tap=tap)
        assert _beyond(ym, y, bd) >= 1 and _beyond(ym, y, bd) <= cout, tap
    if B > 1:
        assert _beyond(U.mut_neighbour_halo(x, w, b), y, bd) >= 1
    b2 = torch.randn(cout, generator=g) * 0.1
    assert _beyond(U.mut_neighbour_bias(x, w, b2), y, bd) >= 1
    p, codes = U.pool_first_max(y)
    bp = U.pool_max(bd)
    pm, rows = U.mut_shift_windows(y)
    assert _beyond(pm, p[:, rows], bp[:, rows]) >= 1
    if T & 1:
        assert _beyond(U.mut_odd_row_leaks(y), p, bp) >= 1
    # swapped code bits: the codes differ from the first-maximum codes, and a gradient un-pooled with them leaves the bound
    swapped = U.mut_swap_code_bits(codes)
    assert int((swapped != codes).sum()) >= 1
    dp = torch.randn(p.shape, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin) ** 0.5)
    dx, Sdx = U.dgrad_truth(U.unpool(dp, codes, T, Fq), wt, x)
    dxm, _ = U.dgrad_truth(U.unpool(dp, swapped, T, Fq), wt, x)
    assert _beyond(dxm, dx, U.bound(Sdx, 9 * cout, 'h2')) >= 1
    dw, Sdw, _, _ = U.wgrad_truth(x, U.unpool(dp, codes, T, Fq))
    dwm, _, _, _ = U.wgrad_truth(x, U.unpool(dp, swapped, T, Fq))
    assert _beyond(dwm, dw, U.bound(Sdw, B * T * Fq + 64, 'h2')) >= 1


def test_case_table_reaches_the_edges_it_names():
    """properties of the table the GPU file relies on"""
    kind, cin, cout, B, T, Fq = U.CASES['P64']
    assert T % 16 == 2 and Fq % 16 == 5 and Fq & 1 and B == 2
    kind, cin, cout, B, T, Fq = U.CASES['R128']
    assert -(-T // 16) == 3 and T % 16 == 1 and Fq % 16 == 4 and cout == 128
    kind, cin, cout, B, T, Fq = U.CASES['P128']
    assert T & 1 and T // 2 * 2 == 16 and (Fq // 2 * 2) % 16 == 2 and cout == 128
    kind, cin, cout, B, T, Fq = U.CASES['D128p']
    assert Fq & 1 and T & 1 and cin == cout == 128
    c = U.make_case(*U.CASES['D128p'])
    assert sorted(c['am'].unique().tolist()) == [0, 1, 2, 3]
    assert (c['am'][:, 0, 0] == 0).all() and (c['am'][:, -1, -1] == 3).all() and (c['am'][:, -1, 0] == 1).all() and (c['am'][:, 0, -1] == 2).all()
    z = U.make_case('pool', 64, 64, 2, 18, 21, 1, 'ZERO')
    assert float(z['y'].abs().max()) == 0.0 and int(z['codes'].sum()) == 0
    k = U.make_case('pool', 64, 64, 2, 18, 21, 1, 'CONST')
    assert bool((k['x'] == k['x'][:, :1, :1]).all()) and float(k['p'].max()) > 0
