"""CPU: the fp64 CTC oracle of the GPU tests (tests/ctc_ref.py) is pinned to torch.nn.functional.ctc_loss in fp64 on every case of the
shared table; the in_len rule of the engine's loss stage; the C ABI of the CTC entry points without a device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_ref as CR

CASES = CR.cases()


def torch_ctc(case, dtype, zero_infinity, reduction='mean'):
    """-> (loss / per-utterance nll, gradient w.r.t. the logits through log_softmax) of torch's CPU ctc_loss"""
    x = torch.from_numpy(case['logits']).to(dtype).requires_grad_(True)
    lp = F.log_softmax(x.transpose(0, 1), 2)
    out = F.ctc_loss(lp, torch.from_numpy(case['gold']), torch.from_numpy(case['in_len']).long(), torch.from_numpy(case['tgt_len']).long(),
                     blank=0, reduction=reduction, zero_infinity=zero_infinity)
    if reduction != 'mean':
        return out.detach().numpy(), None
    out.backward()
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_oracle_equals_torch_fp64(case):
    U = case['U']
    nll, loss, grad = CR.ctc(case['logits'], case['gold'], case['in_len'], case['tgt_len'])           # reduction='mean': one group
    t_nll, _ = torch_ctc(case, torch.float64, False, 'none')
    t_loss, _ = torch_ctc(case, torch.float64, False)
    _, t_grad = torch_ctc(case, torch.float64, True)
    inf = np.isinf(t_nll)
    assert (np.isinf(nll) == inf).all() and (nll[inf] > 0).all()                                      # +inf agreement, zero_infinity=False
    assert np.allclose(nll[~inf], t_nll[~inf], rtol=1e-12, atol=0)
    assert (np.isinf(loss[0]) and np.isinf(t_loss)) if inf.any() else abs(loss[0] - t_loss) <= 1e-12 * abs(t_loss)
    assert np.abs(grad - t_grad).max() <= 1e-12
    # the zeros are exact: rows beyond in_len, every row of an infeasible utterance
    for u in range(U):
        assert not grad[u, max(int(case['in_len'][u]), 0):].any()
        if inf[u]:
            assert not grad[u].any()
        assert inf[u] == (not CR.feasible(case['gold'][u, :case['tgt_len'][u]], int(case['in_len'][u])))


def test_label_equal_to_the_blank_is_an_ordinary_label():
    case = CR.blank_label_cases()[0]
    nll, _, grad = CR.ctc(case['logits'], case['gold'], case['in_len'], case['tgt_len'], per_group=1)
    t_nll, _ = torch_ctc(case, torch.float64, False, 'none')
    assert np.isfinite(nll).all() and np.allclose(nll, t_nll, rtol=1e-12, atol=0)
    # the gradient is the derivative of that value (central differences, fp64): per_group = 1 -> d(nll_u / L_u) / d logits
    rng = np.random.default_rng(5)
    x = case['logits'].astype(np.float64)
    for _ in range(40):
        u, t, c = int(rng.integers(case['U'])), int(rng.integers(case['T'])), int(rng.integers(case['V']))
        h = 1e-5
        xp, xm = x.copy(), x.copy()
        xp[u, t, c] += h
        xm[u, t, c] -= h
        fp = CR.ctc(xp, case['gold'], case['in_len'], case['tgt_len'], per_group=1)[1][u]
        fm = CR.ctc(xm, case['gold'], case['in_len'], case['tgt_len'], per_group=1)[1][u]
        assert abs((fp - fm) / (2 * h) - grad[u, t, c]) < 1e-8, (u, t, c)


def test_feasible_utterances_have_the_zero_infinity_false_gradient():
    """the one deviation (zero instead of NaN rows) touches infeasible utterances only: a feasible batch has the same gradient both ways"""
    case = [c for c in CASES if c['name'] == 'V3764-x1'][0]
    _, g_true = torch_ctc(case, torch.float64, True)
    _, g_false = torch_ctc(case, torch.float64, False)
    assert np.array_equal(g_true, g_false)


def test_task_groups_and_scales():
    base = [c for c in CASES if c['name'] == 'groups6-x1'][0]
    nll, loss6, g6 = CR.ctc(base['logits'], base['gold'], base['in_len'], base['tgt_len'], per_group=6)
    gs = np.array([0.5, 2.0])
    _, loss3, g3 = CR.ctc(base['logits'], base['gold'], base['in_len'], base['tgt_len'], per_group=3, gscale=0.25, gscale_dev=gs)
    L = np.maximum(base['tgt_len'], 1)
    assert np.isinf(loss6[0]) and np.isinf(loss3[1]) and np.isclose(loss3[0], (nll[:3] / L[:3]).mean(), rtol=1e-15)
    assert np.allclose(g3[:3], g6[:3] * 2 * 0.25 * 0.5, rtol=1e-14, atol=0) and np.allclose(g3[3:], g6[3:] * 2 * 0.25 * 2.0, rtol=1e-14, atol=0)


def test_label_outside_the_vocabulary_is_infeasible():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 6, 5))
    for bad in (5, -1, 1 << 40):
        nll, loss, g = CR.ctc(x, np.array([[1, bad, 0], [2, 3, 0]]), [6, 6], [2, 2])
        assert np.isinf(nll[0]) and np.isfinite(nll[1]) and np.isinf(loss[0]) and not g[0].any() and g[1].any()


def test_in_len_rule_is_the_reference_product():
    """sizes = src_percentages.mul_(Td).int(): an fp32 product, truncated -- for every pct = k / n a batch can bring"""
    ks, ns = np.meshgrid(np.arange(1, 41), np.arange(1, 41))
    keep = ks <= ns
    pct = (ks[keep] / ns[keep].astype(np.float64)).astype(np.float32)          # data.py: n / float(max_t) stored into a float32 tensor
    for Td in range(2, 61):
        want = torch.from_numpy(pct.copy()).mul_(Td).int().numpy()
        assert np.array_equal(CR.in_len_from_percentages(pct, Td), want)
        import mtl_amd
        assert np.array_equal(mtl_amd.engine.ctc_input_lengths(pct, Td), want)
    # the product is NOT the exact quotient: 0.7 (fp32) * 10 truncates to 7 only because the fp32 product rounds up
    assert int(CR.in_len_from_percentages([np.float32(7 / 10)], 10)[0]) == int(torch.tensor([7 / 10]).mul_(10).int())


# ---------------------------------------------------------------------------------------------------------------------------------
# C ABI (no device: every check happens before a launch)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    return ge.build()


def test_ctc_symbols_are_exported_and_recordable(built):
    h = ctypes.CDLL(built._lib.LIB_PATH)
    L = built._lib.lib()
    for name in ('mtl_ctc_workspace', 'mtl_ctc_fwd', 'mtl_ctc_bwd'):
        assert hasattr(h, name) and name in built._lib.SIGNATURES, name
    assert L.mtl_cmdlist_opcode(b'mtl_ctc_fwd') >= 0 and L.mtl_cmdlist_opcode(b'mtl_ctc_bwd') >= 0
    assert L.mtl_cmdlist_opcode(b'mtl_ctc_workspace') == -1                     # a size query: evaluated while recording


def test_ctc_workspace_values(built):
    L = built._lib.lib()
    assert L.mtl_ctc_workspace(8, 50, 49) == 8 * 50 * (99 + 2) * 4                     # the lattice and two row statistics per row
    assert L.mtl_ctc_workspace(1, 1, 1) == 20
    assert L.mtl_ctc_workspace(64, 1000, 1000) == 64 * 1000 * 2003 * 4          # beyond 2^31 bytes: long arithmetic
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, 5, 1401)):
        assert L.mtl_ctc_workspace(*bad) == -22, bad


def test_ctc_argument_validation_without_gpu(built):
    L = built._lib.lib()
    p = 4096                                                                     # any non-null address: nothing is dereferenced
    U, T, V, Lmax = 4, 5, 7, 3
    ws = L.mtl_ctc_workspace(U, T, Lmax)
    good_f = dict(stream=None, logits=p, gold=p, in_len=p, tgt_len=p, U=U, T=T, V=V, ld=V, ldg=4, Lmax=Lmax, blank=0, per_group=2,
                  ws=p, ws_bytes=ws, nll=p, loss_out=p)
    good_b = dict(stream=None, logits=p, gold=p, in_len=p, tgt_len=p, U=U, T=T, V=V, ld=V, ldg=4, Lmax=Lmax, blank=0, per_group=2,
                  ws=p, ws_bytes=ws, nll=p, gscale=1.0, gscale_dev=None, dlogits=p, ldd=8)
    bad_scalars = [dict(U=0), dict(T=0), dict(V=0), dict(Lmax=0), dict(Lmax=1401), dict(ld=V - 1), dict(ldg=0), dict(blank=-1), dict(blank=V),
                   dict(per_group=0), dict(per_group=3), dict(ws_bytes=ws - 1), dict(U=-4)]
    for fn, good, ptrs, extra in ((L.mtl_ctc_fwd, good_f, ('logits', 'gold', 'in_len', 'tgt_len', 'ws', 'nll', 'loss_out'), [dict(ws=p + 4)]),
                                  (L.mtl_ctc_bwd, good_b, ('logits', 'gold', 'in_len', 'tgt_len', 'ws', 'nll', 'dlogits'), [dict(ldd=V - 1), dict(ws=p + 4)])):
        for name in ptrs:
            assert fn(*dict(good, **{name: None}).values()) == -22, name
        for change in bad_scalars + extra:
            assert fn(*dict(good, **change).values()) == -22, change
    # a rejected call is not recorded
    cl = built._lib.CommandList()
    rec = built._lib.Recorder(L, cl)
    assert rec.mtl_ctc_fwd(*dict(good_f, U=0).values()) == -22 and len(cl.entries) == 0
