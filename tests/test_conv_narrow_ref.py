"""CPU twin of tests/test_conv_narrow_gpu.py: the assertions made there on the 32-channel shapes of the large_cnn front-end can fail.
Every mutator of tests/conv_edge_util.py -- what a kernel with a missing tap, a halo taken from the neighbouring sample, windows one
row late or swapped arg-max code bits would give -- applied to the fp64 truth of the narrow cases leaves the x3 bound (or differs in
the codes); the conv0 truths at 32 channels leave it when one tap is missing."""
import pytest
import torch

from tests import conv_edge_util as U
from tests.narrow_cases import CASES, CONV0, WGRAD


def _beyond(got, want, bd):
    return int(((got - want).abs() > bd).sum())


@pytest.mark.parametrize('name', ['P32', 'R64'])
def test_forward_mutators_leave_the_x3_bound(name):
    kind, cin, cout, B, T, Fq = CASES[name]
    c = U.make_case(kind, cin, cout, B, T, Fq)
    x, w, b, y = c['x'], c['w'][0], c['b'][0], c['y']
    bd = U.bound(c['Sy'], 9 * cin, 'x3')
    for tap in ((0, 2), (1, 1), (2, 0)):
        n = _beyond(U.mut_drop_tap(x, w, b, pix=(0, 1, 1), tap=tap), y, bd)
        assert 1 <= n <= cout, tap
    assert _beyond(U.mut_neighbour_halo(x, w, b), y, bd) >= 1
    p, codes = U.pool_first_max(y)
    bp = U.pool_max(bd)
    pm, rows = U.mut_shift_windows(y)
    assert _beyond(pm, p[:, rows], bp[:, rows]) >= 1
    swapped = U.mut_swap_code_bits(codes)
    assert int((swapped != codes).sum()) >= 1


@pytest.mark.parametrize('name', ['D32p', 'D64d'])
def test_gradient_mutators_leave_the_x3_bound(name):
    kind, cin, cout, B, T, Fq = CASES[name]
    c = U.make_case(kind, cin, cout, B, T, Fq)
    w, bd = c['w'][0], U.bound(c['Sdx'], 9 * cout, 'x3')
    if kind == 'dgrad_p':       # un-pooled with swapped code bits
        dxm, _ = U.dgrad_truth(U.unpool(c['dy'], U.mut_swap_code_bits(c['am']), T, Fq), w, c['act'])
        assert _beyond(dxm, c['dx'], bd) >= 1
        shifted = U.unpool(c['dy'], c['am'], T, Fq).roll(1, dims=1)               # windows one row late
        assert _beyond(U.dgrad_truth(shifted, w, c['act'])[0], c['dx'], bd) >= 1
    else:                       # a data gradient is the forward of the rotated taps: one tap of one pixel missing
        dense = c['dy']
        dxm = c['dx'].clone()
        dxm[0, 1, 1] -= (w[:, :, 0, 2].double().t() @ dense[0, 0, 2].double()) * (c['act'][0, 1, 1] > 0)      # tap (kh 0, kw 2) reaches dy[t - 1, f + 1]
        n = _beyond(dxm, c['dx'], bd)
        assert 1 <= n <= cin
    assert _beyond(U.dgrad_truth(c['dy'] if c['am'] is None else U.unpool(c['dy'], c['am'], T, Fq), w, torch.ones_like(c['act']))[0],
                   c['dx'], bd) >= 1                                                # the gate ignored


@pytest.mark.parametrize('cin,cout,B,T,Fq,pooled', WGRAD)
def test_weight_gradient_mutators_leave_the_x3_bound(cin, cout, B, T, Fq, pooled):
    c = U.make_wgrad_case(cin, cout, B, T, Fq, 1, pooled)
    K = B * (T // 2 * 2 if pooled else T) * (Fq // 2 * 2 if pooled else Fq)
    bd = U.bound(c['Sdw'][0], K, 'x3')
    dense = U.unpool(c['dy'], c['am'], T, Fq) if pooled else c['dy']
    if pooled:
        dwm = U.wgrad_truth(c['x'], U.unpool(c['dy'], U.mut_swap_code_bits(c['am']), T, Fq))[0]
        assert _beyond(dwm, c['dw'][0], bd) >= 1
    # one pixel's contribution to one tap missing
    dwm = c['dw'][0].clone()
    dwm[:, :, 1, 1] -= torch.outer(dense[0, 0, 0].double(), c['x'][0, 0, 0].double())
    assert _beyond(dwm, c['dw'][0], bd) >= 1
    # the bias gradient without one pixel
    assert _beyond(c['db'][0] - dense[0, 0, 0].double(), c['db'][0], U.bound(c['Sdb'][0], K, 'x3')) >= 1


@pytest.mark.parametrize('T,Fq', [(t, f) for t in CONV0['T'] for f in CONV0['F']])
def test_conv0_truth_without_one_tap_leaves_the_x3_bound(T, Fq):
    """conv0 (Cin = 1, K = 9): the x3 constant is the looser of the two arithmetics' and still far below one missing tap"""
    g = torch.Generator().manual_seed(T * 100 + Fq)
    x = torch.randn(CONV0['B'], T, Fq, 1, generator=g)
    w = torch.randn(32, 1, 3, 3, generator=g) / 3.0
    b = torch.randn(32, generator=g) * 0.1
    y, S = U.fwd_truth(x, w, b, relu=False)
    ym = y.clone()
    ym[0, 0, 0] -= w[:, 0, 1, 1].double() * float(x[0, 0, 0, 0])               # the centre tap exists at every extent
    assert _beyond(ym, y, U.bound(S, 9, 'x3')) >= 1


def test_narrow_case_table_reaches_the_edges_it_names():
    kind, cin, cout, B, T, Fq = CASES['P32']
    assert (cin, cout) == (32, 32) and T % 8 == 2 and Fq % 16 == 5 and Fq & 1 and B == 2
    kind, cin, cout, B, T, Fq = CASES['R64']
    assert (cin, cout) == (32, 64) and T % 8 == 1 and Fq % 16 == 4
    kind, cin, cout, B, T, Fq = CASES['D32p']
    assert Fq & 1 and T & 1 and cin == cout == 32
    c = U.make_case(*CASES['D32p'])
    assert sorted(c['am'].unique().tolist()) == [0, 1, 2, 3]
    kind, cin, cout, B, T, Fq = CASES['MANY32']
    assert -(-(Fq // 2 * 2) // 16) * -(-(T // 2 * 2) // 8) * B > 4 * 256           # more 8 x 16 tiles than any device has compute units
