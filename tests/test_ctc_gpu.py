"""GPU: mtl_ctc_fwd / mtl_ctc_bwd against the fp64 oracle (tests/ctc_ref.py, pinned to torch's fp64 ctc_loss by tests/test_ctc_ref.py)
on the shared case table, and calculate_metrics(loss_type='ctc') on arbitrary tensors.

Tolerance: no fixed number.  The yardstick of a case is the error of torch's OWN fp32 CPU ctc_loss + autograd on the same inputs
against the fp64 result (the posterior is exp of a difference of logs of magnitude ~100, so fp32 loses digits there whatever the
code); the device may be 4 x as far off (another association order of the log-sum-exps, another row log-sum-exp), with a floor of
4 fp32 ulp of the value.  Zeros (rows beyond in_len, infeasible utterances, pad columns) and +inf are exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_ref as CR

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
CASES = CR.cases() + CR.blank_label_cases()
DEV = 'cuda:0'
WORST = {'nll': 0.0, 'loss': 0.0, 'grad': 0.0}


@pytest.fixture(scope='module')
def lib():
    import mtl_amd
    return mtl_amd._lib.lib()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def run_device(lib, case, per_group=None, ldd=None, gscale=1.0, gscale_dev=None, in_len=None, tgt_len=None, gold=None, guard=0, h=None):
    """-> nll (U), loss (U / per_group), dlogits (U, T, ldd) as numpy, [the guard bands around dlogits and the workspace]"""
    h = lib if h is None else h
    U, T, V = case['U'], case['T'], case['V']
    per_group = case['per_group'] if per_group is None else per_group
    ldd = V if ldd is None else ldd
    gold_np = case['gold'] if gold is None else gold
    ldg = gold_np.shape[1]
    Lmax = max(ldg, 1)
    x = torch.from_numpy(case['logits']).to(DEV).view(U * T, V).contiguous()
    g = torch.from_numpy(gold_np).to(DEV).contiguous()
    il = torch.from_numpy(np.asarray(case['in_len'] if in_len is None else in_len, dtype=np.int32)).to(DEV)
    tl = torch.from_numpy(np.asarray(case['tgt_len'] if tgt_len is None else tgt_len, dtype=np.int32)).to(DEV)
    ws_bytes = lib.mtl_ctc_workspace(U, T, Lmax)
    assert ws_bytes == U * T * (2 * Lmax + 3) * 4
    SENT = 12345.5
    ws_all = torch.full((ws_bytes // 4 + 2 * guard,), SENT, dtype=torch.float32, device=DEV)
    # (without guard bands dlogits starts as NaN: every element must be written)
    d_all = torch.full((U * T * ldd + 2 * guard,), SENT if guard else float('nan'), dtype=torch.float32, device=DEV)
    ws_ptr, d_ptr = ws_all.data_ptr() + 4 * guard, d_all.data_ptr() + 4 * guard
    nll = torch.full((U,), SENT, dtype=torch.float32, device=DEV)
    loss = torch.full((U // per_group,), SENT, dtype=torch.float32, device=DEV)
    gsd = None if gscale_dev is None else torch.tensor(gscale_dev, dtype=torch.float32, device=DEV)
    st = _stream()
    rc = h.mtl_ctc_fwd(st, x.data_ptr(), g.data_ptr(), il.data_ptr(), tl.data_ptr(), U, T, V, V, ldg, Lmax, 0, per_group,
                       ws_ptr, ws_bytes, nll.data_ptr(), loss.data_ptr())
    assert rc == 0, rc
    rc = h.mtl_ctc_bwd(st, x.data_ptr(), g.data_ptr(), il.data_ptr(), tl.data_ptr(), U, T, V, V, ldg, Lmax, 0, per_group,
                       ws_ptr, ws_bytes, nll.data_ptr(), float(gscale), None if gsd is None else gsd.data_ptr(), d_ptr, ldd)
    assert rc == 0, rc
    torch.cuda.synchronize()
    d = d_all.cpu().numpy()
    out = (nll.cpu().numpy(), loss.cpu().numpy(), d[guard:d.size - guard].reshape(U, T, ldd))
    if guard:
        w = ws_all.cpu().numpy()
        bands = np.concatenate([d[:guard], d[d.size - guard:], w[:guard], w[w.size - guard:]])
        return out + (bands, SENT)
    return out


_YARD = {}


def yardstick(case, rows):
    """torch's fp32 CPU ctc_loss + autograd on the utterances `rows` of the case as ONE batch (reduction='mean' over them), against
    the fp64 oracle: -> (worst relative error of a finite nll, relative error of the mean loss or None when it is +inf, worst absolute
    error of the gradient, max |gradient|)"""
    key = (case['name'], rows.start, rows.stop)
    if key not in _YARD:
        x = torch.from_numpy(case['logits'][rows]).requires_grad_(True)
        gold, il, tl = (torch.from_numpy(case[k][rows]).long() for k in ('gold', 'in_len', 'tgt_len'))
        lp = F.log_softmax(x.transpose(0, 1), 2)
        nll32 = F.ctc_loss(lp, gold, il, tl, blank=0, reduction='none', zero_infinity=False).detach().numpy()
        loss32 = float(F.ctc_loss(lp, gold, il, tl, blank=0, reduction='mean', zero_infinity=False).detach())
        F.ctc_loss(lp, gold, il, tl, blank=0, reduction='mean', zero_infinity=True).backward()
        nll64, loss64, g64 = CR.ctc(case['logits'][rows], case['gold'][rows], case['in_len'][rows], case['tgt_len'][rows])
        fin = np.isfinite(nll64)
        assert (np.isfinite(nll32) == fin).all()
        y_nll = float(np.max(np.abs(nll32[fin] - nll64[fin]) / np.maximum(np.abs(nll64[fin]), 1e-30), initial=0.0))
        y_loss = abs(loss32 - loss64[0]) / abs(loss64[0]) if np.isfinite(loss64[0]) and loss64[0] != 0 else None
        _YARD[key] = (y_nll, y_loss, float(np.abs(x.grad.numpy() - g64).max()), float(np.abs(g64).max()))
    return _YARD[key]


def check_against_oracle(case, got, per_group, ldd, gscale=1.0, gscale_dev=None, blank_labels=False):
    nll, loss, d = got
    U, T, V = case['U'], case['T'], case['V']
    nll64, loss64, g64 = CR.ctc(case['logits'], case['gold'], case['in_len'], case['tgt_len'], per_group=per_group, gscale=gscale,
                                gscale_dev=gscale_dev)
    # exact: +inf, the zero rows, the pad columns; nothing left unwritten
    assert np.array_equal(np.isinf(nll), np.isinf(nll64)) and (nll[np.isinf(nll)] > 0).all() and not np.isnan(nll).any()
    assert np.array_equal(np.isinf(loss), np.isinf(loss64)) and (loss[np.isinf(loss)] > 0).all() and not np.isnan(loss).any()
    assert not np.isnan(d).any()
    assert not d[:, :, V:].any()
    for u in range(U):
        assert not d[u, int(case['in_len'][u]):].any(), u
        if np.isinf(nll64[u]):
            assert not d[u].any(), u
    for g in range(U // per_group):
        rows = slice(g * per_group, (g + 1) * per_group)
        s = abs(gscale * (1.0 if gscale_dev is None else gscale_dev[g]))
        if blank_labels:
            # outside torch's contract (its gradient overwrites the last row's blank column): the yardstick is torch's fp32 error on
            # the sibling case with the same logits and lattice shape in which those labels are another symbol, 5, that no target uses
            live = np.arange(case['gold'].shape[1])[None, :] < case['tgt_len'][:, None]
            sibling = dict(case, name=case['name'] + '-sibling', gold=np.where(live & (case['gold'] == 0), 5, case['gold']))
            y_nll, y_loss, y_grad, gmax = yardstick(sibling, rows)
        else:
            y_nll, y_loss, y_grad, gmax = yardstick(case, rows)
        fin = np.isfinite(nll64[rows])
        e_nll = float(np.max(np.abs(nll[rows][fin] - nll64[rows][fin]) / np.maximum(np.abs(nll64[rows][fin]), 1e-30), initial=0.0))
        b_nll = max(4 * y_nll, 4 * EPS)
        e_grad = float(np.abs(d[rows, :, :V] - g64[rows]).max())
        b_grad = max(4 * y_grad, 4 * EPS * gmax) * s
        line = '%-16s group %d: nll rel %.2e (yardstick %.2e)' % (case['name'], g, e_nll, y_nll)
        WORST['nll'] = max(WORST['nll'], e_nll / max(b_nll / 4, 1e-300))
        if np.isfinite(loss64[g]) and loss64[g] != 0:
            e_loss = abs(float(loss[g]) - loss64[g]) / abs(loss64[g])
            b_loss = max(4 * (y_loss or 0.0), 4 * EPS)
            line += ' loss rel %.2e (%s)' % (e_loss, 'yardstick %.2e' % y_loss if y_loss is not None else 'floor')
            WORST['loss'] = max(WORST['loss'], e_loss / max(b_loss / 4, 1e-300))
        else:
            e_loss, b_loss = 0.0, 1.0
            assert float(loss[g]) == loss64[g]                      # +inf, or the exact 0 of an empty group
        WORST['grad'] = max(WORST['grad'], e_grad / max(b_grad / 4, 1e-300))
        print(line + ' grad abs %.2e (yardstick %.2e, |g|max %.2e); worst error / yardstick so far: nll %.2f loss %.2f grad %.2f'
              % (e_grad, y_grad * s, gmax * s, WORST['nll'], WORST['loss'], WORST['grad']))
        assert e_nll <= b_nll, (e_nll, b_nll)
        assert e_loss <= b_loss, (e_loss, b_loss)
        assert e_grad <= b_grad, (e_grad, b_grad)


def _ldd4(V):
    return (V + 3) // 4 * 4


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_kernels_against_the_fp64_oracle(lib, case):
    V = case['V']
    blank_labels = case['name'].startswith('blanklabel')
    for ldd in sorted({V, _ldd4(V)}):
        got = run_device(lib, case, ldd=ldd)
        check_against_oracle(case, got, case['per_group'], ldd, blank_labels=blank_labels)


@pytest.mark.parametrize('scale', [1, 12])
def test_task_groups_with_device_scales(lib, scale):
    case = [c for c in CASES if c['name'] == 'groups6-x%d' % scale][0]
    for pg in (6, 3, 1):
        gsd = [0.5, 2.0, 1.0, 0.25, 3.0, 1.5][:6 // pg]
        got = run_device(lib, case, per_group=pg, ldd=_ldd4(case['V']), gscale=0.75, gscale_dev=gsd)
        check_against_oracle(case, got, pg, _ldd4(case['V']), gscale=0.75, gscale_dev=gsd)
        plain = run_device(lib, case, per_group=pg, ldd=_ldd4(case['V']), gscale=0.75)
        check_against_oracle(case, plain, pg, _ldd4(case['V']), gscale=0.75)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])       # the forward does not see the scales


def test_run_to_run_bitwise_determinism(lib):
    for name in ('wide-x1', 'groups3-x12', 'repeats-x1'):
        case = [c for c in CASES if c['name'] == name][0]
        a = run_device(lib, case, ldd=_ldd4(case['V']))
        b = run_device(lib, case, ldd=_ldd4(case['V']))
        for p, q in zip(a, b):
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), name


def test_replay_through_a_command_list_is_bit_equal(lib):
    import mtl_amd
    case = [c for c in CASES if c['name'] == 'groups3-x1'][0]
    eager = run_device(lib, case, ldd=_ldd4(case['V']))
    cl = mtl_amd._lib.CommandList()
    rec = mtl_amd._lib.Recorder(lib, cl)
    recorded = run_device(lib, case, ldd=_ldd4(case['V']), h=rec)
    assert len(cl.entries) == 2
    for p, q in zip(eager, recorded):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    # the replay proper: the same two calls on buffers this test owns
    U, T, V, ldd = case['U'], case['T'], case['V'], _ldd4(case['V'])
    x = torch.from_numpy(case['logits']).to(DEV).view(U * T, V).contiguous()
    g = torch.from_numpy(case['gold']).to(DEV)
    il, tl = torch.from_numpy(case['in_len']).to(DEV), torch.from_numpy(case['tgt_len']).to(DEV)
    ldg = g.shape[1]
    ws_bytes = lib.mtl_ctc_workspace(U, T, ldg)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=DEV)
    nll = torch.zeros(U, dtype=torch.float32, device=DEV)
    loss = torch.zeros(U // 3, dtype=torch.float32, device=DEV)
    d = torch.full((U * T, ldd), float('nan'), dtype=torch.float32, device=DEV)
    cl2 = mtl_amd._lib.CommandList()
    rec2 = mtl_amd._lib.Recorder(lib, cl2)
    st = _stream()
    assert rec2.mtl_ctc_fwd(st, x.data_ptr(), g.data_ptr(), il.data_ptr(), tl.data_ptr(), U, T, V, V, ldg, ldg, 0, 3,
                            ws.data_ptr(), ws_bytes, nll.data_ptr(), loss.data_ptr()) == 0
    assert rec2.mtl_ctc_bwd(st, x.data_ptr(), g.data_ptr(), il.data_ptr(), tl.data_ptr(), U, T, V, V, ldg, ldg, 0, 3,
                            ws.data_ptr(), ws_bytes, nll.data_ptr(), 1.0, None, d.data_ptr(), ldd) == 0
    cl2.finish()
    torch.cuda.synchronize()
    nll.zero_(), loss.zero_(), d.fill_(float('nan')), ws.fill_(float('nan'))
    cl2.run()
    torch.cuda.synchronize()
    for p, q in zip(eager, (nll.cpu().numpy(), loss.cpu().numpy(), d.cpu().numpy().reshape(U, T, ldd))):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))


def test_garbage_lengths_and_labels_stay_inside_their_buffers(lib):
    """The kernels clamp in_len to [0, T] and tgt_len to [0, min(Lmax, ldg)], and a label outside [0, V) makes its utterance infeasible
    before anything is indexed with it: lengths and labels far outside run like their clamped values and touch nothing outside the
    buffers (guard bands around dlogits and the workspace)."""
    base = [c for c in CASES if c['name'] == 'groups6-x1'][0]
    U, T, V = base['U'], base['T'], base['V']
    ldg = base['gold'].shape[1]
    in_len = np.array([2 ** 31 - 1, 10 ** 9, -7, T + 1, 3, -2 ** 31], dtype=np.int64).astype(np.int32)
    tgt_len = np.array([2 ** 31 - 1, 3, 10 ** 9, -5, ldg + 1, 2], dtype=np.int64).astype(np.int32)
    rng = np.random.default_rng(3)
    gold = rng.integers(1, V, size=base['gold'].shape).astype(np.int64)                  # every entry a label: tgt_len may reach ldg
    for i in range(1, ldg):
        same = gold[:, i] == gold[:, i - 1]
        gold[same, i] = gold[same, i] % (V - 1) + 1
    gold[1, 1] = V                                                                       # one past the vocabulary
    clamped = dict(base, gold=gold, in_len=np.clip(in_len, 0, T).astype(np.int32), tgt_len=np.clip(tgt_len, 0, ldg).astype(np.int32))
    guard = 4096
    nll, loss, d, bands, sent = run_device(lib, base, in_len=in_len, tgt_len=tgt_len, gold=gold, guard=guard, ldd=_ldd4(V))
    assert (bands == sent).all()
    ref = run_device(lib, clamped, ldd=_ldd4(V))
    for p, q in zip((nll, loss, d), ref):
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    nll64, _, g64 = CR.ctc(clamped['logits'], gold, clamped['in_len'], clamped['tgt_len'])
    assert np.array_equal(np.isinf(nll), np.isinf(nll64)) and np.isinf(nll[1]) and not d[1].any()
    assert np.isfinite(nll64).sum() >= 2                                                 # (the test is not all-infeasible)
    for bad in (-1, 1 << 40, -(1 << 40)):
        gold[0, 0] = bad
        out = run_device(lib, dict(clamped, gold=gold), ldd=V)
        assert np.isinf(out[0][0]) and not out[2][0].any() and not np.isnan(out[2]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# calculate_metrics(loss_type='ctc') on arbitrary tensors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['groups6-x1', 'V3764-x12', 'short-x1'])
def test_calculate_metrics_ctc(lib, name):
    import mtl_amd
    case = [c for c in CASES if c['name'] == name][0]
    U, T, V = case['U'], case['T'], case['V']
    pred = torch.from_numpy(case['logits']).to(DEV).requires_grad_(True)
    gold = torch.from_numpy(case['gold']).to(DEV)
    il, tl = torch.from_numpy(case['in_len']), torch.from_numpy(case['tgt_len'])         # host tensors, as the loaders bring them
    out = mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=il, target_lengths=tl, smoothing=0.1, loss_type='ctc')
    assert isinstance(out, tuple) and len(out) == 2 and out[1] is None
    loss = out[0]
    assert loss.shape == () and loss.device == pred.device
    loss.backward(torch.tensor(0.5, device=DEV))
    torch.cuda.synchronize()
    nll64, loss64, _ = CR.ctc(case['logits'], case['gold'], case['in_len'], case['tgt_len'])
    dev_nll = np.where(np.isinf(nll64), np.inf, nll64).astype(np.float32)                # (nll is not returned: the loss and d(pred) are checked)
    check_against_oracle(case, (dev_nll, loss.detach().cpu().numpy().reshape(1), pred.grad.cpu().numpy()), U, V, gscale=0.5)


def test_calculate_metrics_ctc_argument_checks():
    import mtl_amd
    pred = torch.randn(2, 5, 7, device=DEV)
    gold = torch.tensor([[1, 2, 0], [3, 0, 0]], device=DEV)
    il, tl = torch.tensor([5, 4]), torch.tensor([2, 1])
    with pytest.raises(ValueError, match='input_lengths'):
        mtl_amd.calculate_metrics(pred, gold, 0, target_lengths=tl, loss_type='ctc')
    with pytest.raises(ValueError, match='target_lengths'):
        mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=il, loss_type='ctc')
    with pytest.raises(ValueError, match='input_lengths'):
        mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=torch.tensor([6, 4]), target_lengths=tl, loss_type='ctc')
    with pytest.raises(ValueError, match='target_lengths'):
        mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=il, target_lengths=torch.tensor([4, 1]), loss_type='ctc')
    with pytest.raises(ValueError, match='input_lengths'):
        mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=torch.tensor([5]), target_lengths=tl, loss_type='ctc')
    with pytest.raises(NotImplementedError):
        mtl_amd.calculate_metrics(pred, gold, 0, input_lengths=il, target_lengths=tl, loss_type='mwer')
    # the non_pad_mask behaviour is that of 'ce': gold is padded in place where the mask is False
    g2 = gold.clone()
    mask = torch.tensor([[True, False, False], [True, False, False]], device=DEV)
    loss, none = mtl_amd.calculate_metrics(pred, g2, 0, input_lengths=il, target_lengths=torch.tensor([1, 1]), non_pad_mask=mask, loss_type='ctc')
    assert none is None and g2.tolist() == [[1, 0, 0], [3, 0, 0]] and np.isfinite(float(loss))
