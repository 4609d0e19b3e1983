"""LM epoch training, joint training and fine-tuning on the device (lm.LMTrainer, lm.LMJointTrainer, lm.load_lm_checkpoint):
mtl_lm_window_chains integer-exact against LMEngine._chains, mtl_sgd_clip_step bitwise against mtl_scale + mtl_axpy, an epoch bitwise
against the same epoch composed from the earlier calls (tests/lm_train_util.py:parent_epoch), single steps and free runs against the
fp64 restatement, and train() / fine-tuning end to end.  One process, small shapes (V = 200, E = 32, H = 128: the shape of
test_gru_meta_step_matches_restatement, which the persistent kernels support)."""
import argparse

import numpy as np
import pytest
import torch

from tests import gru_ref as GR
from tests import lm_train_util as U

pytestmark = pytest.mark.gpu

EINVAL = -22
V, E, H, NL, B, BPTT = 200, 32, 128, 2, 4, 6
LR, CLIP = 2.0, 0.25


def _L():
    import mtl_amd
    return mtl_amd._lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _stream(S, seed=3, b=B, v=V):
    """(S, b) ids with repeats inside a window and across window boundaries"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, v, (S, b), generator=g)
    x[1] = x[0]
    x[BPTT] = x[BPTT - 1]
    return x


def _model(kind, tied, dropout=0.0, seed=11):
    import mtl_amd
    torch.manual_seed(seed)
    return mtl_amd.lm.RNNModel(kind, V, H if tied else E, H, NL, dropout, tie_weights=tied).cuda()


def _ref(model, dtype):
    ref = GR.RNNModel(model.rnn_type, V, model.ninp, H, NL, 0.0, model.tie_weights).to(dtype)
    _to_ref(ref, model, model.flat_parameters)
    return ref


def _to_ref(ref, model, flat):
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(model._layout.view(flat, n).cpu())


def _hid_list(h):
    return [h] if torch.is_tensor(h) else list(h)


def _hid_to(h, dtype):
    return h.cpu().to(dtype) if torch.is_tensor(h) else tuple(t.cpu().to(dtype) for t in h)


def _param_err(model, flat, ref):
    """tests/test_lm_gru_gpu.py's measure: max over tensors of max|got - want| / max(max|want|, 1e-3)"""
    e = 0.0
    for n, p in ref.named_parameters():
        q = model._layout.view(flat, n).cpu().double()
        p = p.detach().double()
        e = max(e, float((q - p).abs().max()) / max(float(p.abs().max()), 1e-3))
    return e


def _ref_param_err(a, b):
    return max(float((p.detach().double() - q.detach().double()).abs().max()) / max(float(q.detach().abs().max()), 1e-3)
               for (_, p), (_, q) in zip(a.named_parameters(), b.named_parameters()))


def _hid_err(a, b):
    return max(float((x.cpu().double() - y.double()).abs().max()) for x, y in zip(_hid_list(a), _hid_list(b)))


# ------------------------------------------------------------------------------------------------------------ mtl_lm_window_chains
def _chains_want(ids, bptt):
    """LMEngine._chains on CPU tensors for every window -> (first, next) over (S - 1) B rows"""
    import mtl_amd
    S, b = ids.shape
    first, nxt = [], []
    for i, T in U.schedule(S, bptt):
        c = mtl_amd.lm.LMEngine._chains(None, ids[i:i + T])
        first.append(c[0])
        nxt.append(c[1])
    return torch.cat(first), torch.cat(nxt)


def _chains_got(ids, bptt, fill=7):
    S, b = ids.shape
    d = ids.cuda()
    out = torch.full((2, (S - 1) * b + 8), fill, dtype=torch.int32, device='cuda')      # 8 guard ints after `next`
    rc = _L().mtl_lm_window_chains(_st(), d.data_ptr(), S, b, bptt, out[0].data_ptr(), out[1].data_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu()


@pytest.mark.parametrize('S,b,bptt,values', [(23, 4, 5, 40), (6, 1, 35, 4), (2, 3, 1, 2), (41, 20, 8, 3), (41, 20, 8, 50000)])
def test_window_chains_match_the_engine(S, b, bptt, values):
    g = torch.Generator().manual_seed(S * 100 + values)
    ids = torch.randint(0, values, (S, b), generator=g)
    if values == 3:
        for i in range(bptt, S - 1, bptt):
            ids[i] = ids[i - 1]                                            # the same id on both sides of every window boundary
    rc, out = _chains_got(ids, bptt)
    assert rc == 0
    first, nxt = _chains_want(ids, bptt)
    n = (S - 1) * b
    assert torch.equal(out[0, :n], first) and torch.equal(out[1, :n], nxt)
    assert bool((out[:, n:] == 7).all())                                   # nothing written past (S - 1) B
    if values == 3:
        assert int(nxt.max()) < bptt * b and int((first == 1).sum()) <= 3 * len(U.schedule(S, bptt))


def test_window_chains_at_and_above_the_row_cap():
    L = _L()
    cap = int(L.mtl_lm_window_chains_max_rows())
    assert cap >= 35 * 20 and cap % 64 == 0
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (cap // 64 + 3, 64), generator=g)        # a window of exactly `cap` rows, then one of 2 x 64
    rc, out = _chains_got(ids, cap // 64)
    first, nxt = _chains_want(ids, cap // 64)
    assert rc == 0 and torch.equal(out[0, :first.numel()], first) and torch.equal(out[1, :first.numel()], nxt)
    ids = torch.randint(0, 1000, (cap + 2, 1), generator=g)               # one row more than the cap: refused, outputs untouched
    rc, out = _chains_got(ids, cap + 1)
    assert rc == EINVAL and bool((out == 7).all())
    rc, _ = _chains_got(ids, cap)                                          # (the same stream in windows of `cap` rows is fine)
    assert rc == 0
    d, o = ids.cuda(), torch.zeros(2, 64, dtype=torch.int32, device='cuda')
    p, f, n = d.data_ptr(), o[0].data_ptr(), o[1].data_ptr()
    assert L.mtl_lm_window_chains(_st(), p, 1, 4, 5, f, n) == EINVAL
    assert L.mtl_lm_window_chains(_st(), p, 9, 0, 5, f, n) == EINVAL
    assert L.mtl_lm_window_chains(_st(), p, 9, 4, 0, f, n) == EINVAL
    assert L.mtl_lm_window_chains(_st(), None, 9, 4, 5, f, n) == EINVAL
    assert L.mtl_lm_window_chains(_st(), p, 9, 4, 5, None, n) == EINVAL
    assert L.mtl_lm_window_chains(_st(), p, 9, 4, 5, f, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((o == 0).all())


# --------------------------------------------------------------------------------------------------------------- mtl_sgd_clip_step
@pytest.mark.parametrize('n', [1, 5, 1024, 1027, 4 * 10 ** 6 + 3])        # (mtl_scale and mtl_axpy accept every one of these sizes)
@pytest.mark.parametrize('coef', [None, 1.0, 0.37])
def test_sgd_clip_step_is_scale_then_axpy_bit_for_bit(n, coef):
    L = _L()
    g = torch.Generator().manual_seed(n % 1000)
    pad = 8                                                                # guard floats after n: must stay as they are
    theta = torch.randn(n + pad, generator=g).cuda()
    grad = (torch.randn(n + pad, generator=g) * torch.logspace(-6, 2, n + pad)[torch.randperm(n + pad, generator=g)]).cuda()
    c = None if coef is None else torch.tensor([coef], dtype=torch.float32, device='cuda')
    cp = None if c is None else c.data_ptr()
    lr = 0.3
    t_want, g_want = theta.clone(), grad.clone()
    assert L.mtl_scale(_st(), g_want.data_ptr(), 1.0, cp, n) == 0
    assert L.mtl_axpy(_st(), t_want.data_ptr(), g_want.data_ptr(), -lr, n) == 0
    t_got, g_got = theta.clone(), grad.clone()
    assert L.mtl_sgd_clip_step(_st(), t_got.data_ptr(), g_got.data_ptr(), lr, cp, n, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(t_got, t_want)
    assert not torch.equal(t_got[:n], theta[:n])
    assert bool((g_got[:n] == 0).all()) and torch.equal(g_got[n:], grad[n:]) and torch.equal(t_got[n:], theta[n:])


def test_sgd_clip_step_accumulates_the_loss_in_fp32_and_checks_its_arguments():
    L = _L()
    theta, grad = torch.randn(64).cuda(), torch.randn(64).cuda()
    vals = np.array([1.0, 6e-8, 6e-8], dtype=np.float32)                  # (1 + 6e-8) + 6e-8 = 1 + 2 ulp, 1 + (6e-8 + 6e-8) = 1 + 1 ulp
    loss, acc = torch.zeros(1, device='cuda'), torch.zeros(1, device='cuda')
    for v in vals:
        loss.fill_(float(v))
        assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), grad.data_ptr(), 0.5, None, 64, loss.data_ptr(), acc.data_ptr()) == 0
    want = np.float32(np.float32(vals[0] + vals[1]) + vals[2])
    assert want != np.float32(vals[0] + np.float32(vals[1] + vals[2]))    # (the order of the additions shows in these values)
    assert np.float32(float(acc)) == want
    keep = theta.clone()
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), grad.data_ptr(), 0.5, None, 64, loss.data_ptr(), None) == 0   # one pointer: no add
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), grad.data_ptr(), 0.5, None, 64, None, acc.data_ptr()) == 0
    assert np.float32(float(acc)) == want and torch.equal(theta, keep)     # (g is zero by now: theta stays)
    assert L.mtl_sgd_clip_step(_st(), None, grad.data_ptr(), 0.5, None, 64, None, None) == EINVAL
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), None, 0.5, None, 64, None, None) == EINVAL
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), grad.data_ptr(), 0.5, None, 0, None, None) == EINVAL
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr() + 4, grad.data_ptr(), 0.5, None, 8, None, None) == EINVAL      # as mtl_axpy
    assert L.mtl_sgd_clip_step(_st(), theta.data_ptr(), grad.data_ptr() + 4, 0.5, None, 8, None, None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(theta, keep)


# ------------------------------------------------------------------------------------------------------- the epoch, bit for bit
def _epoch_bitwise(kind, tied, S):
    import mtl_amd
    src = _stream(S).cuda()
    a, b = _model(kind, tied), _model(kind, tied)
    assert torch.equal(a.flat_parameters, b.flat_parameters)
    tr = mtl_amd.lm.LMTrainer(a, lr=LR, clip=CLIP, bptt=BPTT)
    got = tr.train_epoch(src, log_interval=2)
    want = U.parent_epoch(b, src, BPTT, LR, CLIP, log_interval=2)
    assert got['windows'] == 6 and tuple(got['losses'].shape) == (6,)
    assert tr._tables[0][2].shape == (2, (S - 1) * B)                      # the chains came from the one table
    assert torch.equal(got['losses'], want['losses'])
    for x, y in zip(_hid_list(got['hidden']), _hid_list(want['hidden'])):
        assert torch.equal(x, y)
    assert torch.equal(a.flat_parameters, b.flat_parameters)
    assert bool((tr.g == 0).all())
    assert int(a.engine.sync_ws[1]) == 0 and int(b.engine.sync_ws[1]) == 0
    return a, tr, got


@pytest.mark.parametrize('kind,tied', [('LSTM', False), ('GRU', False), ('GRU', True)])
def test_epoch_equals_the_composed_earlier_calls_bitwise(kind, tied, capsys):
    """S = 33: five windows of 6 steps and one of 2"""
    _epoch_bitwise(kind, tied, 33)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('| epoch')]
    assert len(lines) == 2 and '    2/    5 batches' in lines[0] and '    4/    5 batches' in lines[1]


def test_epoch_is_reproducible_under_dropout():
    import mtl_amd
    src = _stream(33).cuda()
    runs = []
    for p in (0.2, 0.2, 0.0):
        m = _model('GRU', False, dropout=p)
        torch.manual_seed(99)
        out = mtl_amd.lm.LMTrainer(m, lr=LR, clip=CLIP, bptt=BPTT).train_epoch(src)
        runs.append((m.flat_parameters.clone(), out['losses'].clone()))
        assert m.training and int(m.engine.sync_ws[1]) == 0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][1], runs[2][1])


# ----------------------------------------------------------------------------------------------------------- against fp64
def _bound(fixed, dist):
    """the bound tests/test_lm_gru_gpu.py holds the meta step to; where it does not hold, four times the fp32-to-fp64 distance of the
    restatement for the same step (the margin covers the device's different summation order)"""
    return max(fixed, 4.0 * dist)


@pytest.mark.parametrize('kind,tied', [('LSTM', False), ('GRU', False), ('GRU', True)])
def test_every_window_step_matches_fp64(kind, tied):
    """each of the six windows re-based: the fp64 (and the fp32) restatement starts from the device's parameters and hidden state
    before the window, takes the step, and is compared after it"""
    import mtl_amd
    src = _stream(33)
    model = _model(kind, tied)
    eng = model.engine
    before, real = [], eng.forward

    def spy(theta, x, y, hidden, *a, **kw):
        before.append((theta.clone(), _hid_to(hidden, torch.float64)))
        return real(theta, x, y, hidden, *a, **kw)
    eng.forward = spy
    try:
        out = mtl_amd.lm.LMTrainer(model, lr=LR, clip=CLIP, bptt=BPTT).train_epoch(src.cuda())
    finally:
        del eng.forward
    assert len(before) == 6
    after = [b[0] for b in before[1:]] + [model.flat_parameters.clone()]
    hid_after = [b[1] for b in before[1:]] + [_hid_to(out['hidden'], torch.float64)]
    losses = out['losses'].cpu()
    r64, r32 = _ref(model, torch.float64), _ref(model, torch.float32)
    worst = [0.0, 0.0, 0.0]
    for w, (i, T) in enumerate(U.schedule(33, BPTT)):
        x, y = U.get_batch(src, i, BPTT)
        _to_ref(r64, model, before[w][0])
        _to_ref(r32, model, before[w][0])
        h64 = before[w][1]
        h32 = _hid_to(h64, torch.float32)
        l64, h64 = U.window_step(r64, h64, x, y, LR, CLIP)
        l32, h32 = U.window_step(r32, h32, x, y, LR, CLIP)
        e_l, d_l = abs(float(losses[w]) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64)
        e_p, d_p = _param_err(model, after[w], r64), _ref_param_err(r32, r64)
        e_h, d_h = _hid_err(hid_after[w], h64), _hid_err(h32, h64)
        print('lm_train step %s%s window %d (T=%d): loss %.3e (fp32 restatement %.3e) parameters %.3e (%.3e) hidden %.3e (%.3e)'
              % (kind, '-tied' if tied else '', w, T, e_l, d_l, e_p, d_p, e_h, d_h))
        worst = [max(a, b) for a, b in zip(worst, (e_l, e_p, e_h))]
        assert e_l < _bound(1e-5, d_l) and e_p < _bound(2e-5, d_p) and e_h < _bound(1e-5, d_h), w
    print('lm_train step %s%s worst: loss %.3e parameters %.3e hidden %.3e' % ((kind, '-tied' if tied else '') + tuple(worst)))
    assert int(eng.sync_ws[1]) == 0


def _free_run(kind, tied, S):
    """all windows without re-basing against the fp64 restatement; bound: four times the fp32-to-fp64 restatement distance at the end
    of the same run"""
    src = _stream(S)
    theta0 = _model(kind, tied).flat_parameters.clone()
    model, _, got = _epoch_bitwise(kind, tied, S)
    r64, r32 = _ref(model, torch.float64), _ref(model, torch.float32)
    _to_ref(r64, model, theta0)
    _to_ref(r32, model, theta0)
    l64, h64 = U.epoch(r64, src, BPTT, LR, CLIP)
    l32, h32 = U.epoch(r32, src, BPTT, LR, CLIP)
    losses = got['losses'].cpu()
    e_l = max(abs(float(a) - float(b)) / float(b) for a, b in zip(losses, l64))
    d_l = max(abs(float(a) - float(b)) / float(b) for a, b in zip(l32, l64))
    e_p, d_p = _param_err(model, model.flat_parameters, r64), _ref_param_err(r32, r64)
    e_h, d_h = _hid_err(got['hidden'], h64), _hid_err(h32, h64)
    print('lm_train free run %s%s S=%d: loss %.3e (fp32 restatement %.3e) parameters %.3e (%.3e) hidden %.3e (%.3e)'
          % (kind, '-tied' if tied else '', S, e_l, d_l, e_p, d_p, e_h, d_h))
    assert e_l < 4 * d_l and e_p < 4 * d_p and e_h < 4 * d_h
    assert int(model.engine.sync_ws[1]) == 0


@pytest.mark.parametrize('kind,tied', [('LSTM', False), ('GRU', False)])
def test_free_run_epoch_matches_fp64(kind, tied):
    _free_run(kind, tied, 33)


@pytest.mark.parametrize('mode', [True, False])
@pytest.mark.parametrize('kind', ['LSTM', 'GRU'])
def test_joint_free_run_matches_fp64(kind, mode):
    """two joint iterations of three tasks in each mode (one hidden state through all six forwards) against the fp64 restatement; as
    written, no backward is issued for the first two tasks"""
    import mtl_amd
    lm = mtl_amd.lm
    model = _model(kind, False)
    model.train()
    r64, r32 = _ref(model, torch.float64), _ref(model, torch.float32)
    args = argparse.Namespace(bptt=BPTT, batch_size=B, cuda=False)
    ds = lm.LMDataset([lm.synth_corpus(s, V, 331) for s in (1, 2, 3)], args)
    tr = lm.LMJointTrainer(model, lr=LR, clip=CLIP, ratio=0.8, reference_zero_grad=mode)
    eng, calls = model.engine, []
    real = eng.backward
    eng.backward = lambda grad, scale=1.0: (calls.append(scale), real(grad, scale))[1]
    h64, h32 = r64.init_hidden(B), r32.init_hidden(B)
    e_l = d_l = 0.0
    try:
        for it in (0, 1):
            batches = [ds.sample(i, it)[:2] for i in range(3)]
            loss, each = tr.run_iteration([(x.cuda(), y.cuda()) for x, y in batches])
            s64, l64, h64 = U.joint_iteration(r64, h64, batches, LR, CLIP, 0.8, mode)
            s32, l32, h32 = U.joint_iteration(r32, h32, batches, LR, CLIP, 0.8, mode)
            assert abs(loss - sum(w * v for w, v in zip(lm.task_weights(3, 0.8), each))) < 1e-6 * loss
            e_l = max([e_l, abs(loss - s64) / s64] + [abs(a - float(b)) / float(b) for a, b in zip(each, l64)])
            d_l = max([d_l, abs(s32 - s64) / s64] + [abs(float(a) - float(b)) / float(b) for a, b in zip(l32, l64)])
    finally:
        del eng.backward
    w = lm.task_weights(3, 0.8)
    assert calls == ([w[2]] * 2 if mode else w * 2)                        # as written: ONE backward per iteration, the last task's
    e_p, d_p = _param_err(model, model.flat_parameters, r64), _ref_param_err(r32, r64)
    e_h, d_h = _hid_err(tr.hidden, h64), _hid_err(h32, h64)
    print('lm_train joint %s reference_zero_grad=%s: loss %.3e (fp32 restatement %.3e) parameters %.3e (%.3e) hidden %.3e (%.3e)'
          % (kind, mode, e_l, d_l, e_p, d_p, e_h, d_h))
    assert e_l < 4 * d_l and e_p < 4 * d_p and e_h < 4 * d_h
    assert bool((tr.g == 0).all()) and int(eng.sync_ws[1]) == 0


def test_joint_train_uses_the_streams_chain_tables():
    """LMJointTrainer.train (chains sliced from one table per task stream) == run_iteration on sampled batches (the engine builds
    each window's chains itself), bit for bit; the two modes differ"""
    import mtl_amd
    lm = mtl_amd.lm
    args = argparse.Namespace(bptt=BPTT, batch_size=B, cuda=False)
    ds = lm.LMDataset([lm.synth_corpus(s, V, 331) for s in (1, 2, 3)], args)
    a, b, c = _model('GRU', True), _model('GRU', True), _model('GRU', True)
    ta = lm.LMJointTrainer(a, lr=LR, clip=CLIP)
    assert ta.train(ds, 0, 3) is None
    assert sorted(ta._tables) == [0, 1, 2]
    tb, tc = lm.LMJointTrainer(b, lr=LR, clip=CLIP), lm.LMJointTrainer(c, lr=LR, clip=CLIP, reference_zero_grad=False)
    b.train()
    c.train()
    for it in range(3):
        batches = [tuple(t.cuda() for t in ds.sample(i, it)[:2]) for i in range(3)]
        tb.run_iteration(batches)
        tc.run_iteration(batches)
    assert torch.equal(a.flat_parameters, b.flat_parameters) and torch.equal(ta.hidden, tb.hidden)
    assert not torch.equal(a.flat_parameters, c.flat_parameters)
    assert all(int(m.engine.sync_ws[1]) == 0 for m in (a, b, c))


# -------------------------------------------------------------------------------------------------------------------- train()
def _dictionary(n):
    import mtl_amd
    d = mtl_amd.lm.Dictionary()
    for w in ['<oov>', '<eos>'] + ['w%d' % i for i in range(n - 2)]:
        d.add_word(w)
    return d


def test_train_anneals_saves_reloads_and_fine_tunes(tmp_path):
    import mtl_amd
    lm = mtl_amd.lm
    torch.manual_seed(21)
    model = lm.RNNModel('LSTM', V, E, H, NL, 0.0).cuda()
    tr_data = lm.batchify(lm.synth_corpus(5, V, 330), 10).cuda()           # 33 rows
    va_data = lm.batchify(lm.synth_corpus(6, V, 210), 10).cuda()           # 21 rows
    assert tr_data.shape == (33, 10) and va_data.shape == (21, 10)
    d, path = _dictionary(V), str(tmp_path / 'lm.th')
    with pytest.raises(ValueError):
        lm.LMTrainer(model, lr=10.0, bptt=BPTT).train(tr_data, va_data, 1, save_path=path)             # save_path needs dictionary
    with pytest.raises(ValueError):
        lm.LMTrainer(model, lr=10.0, bptt=BPTT).train(tr_data, va_data, 1, dictionary=_dictionary(V + 1))
    trainer = lm.LMTrainer(model, lr=10.0, clip=CLIP, bptt=BPTT)           # lr 10: the validation loss rises at the second epoch
    out = trainer.train(tr_data, va_data, 3, test_data=va_data, save_path=path, dictionary=d)
    log = out['epochs']
    assert [e[0] for e in log] == [1, 2, 3] and not out['stopped_early']
    best, counter, lr, saves = None, 0, 10.0, []
    for (_, val, test, lr_after) in log:
        best, counter, lr, save, _ = lm.anneal_step(best, counter, lr, val, 5)
        saves.append(save)
        assert lr_after == lr and test == val
    assert saves[0] and not all(saves) and trainer.lr == lr < 10.0 and out['best_val_loss'] == best == min(e[1] for e in log)
    # the file: through the loader and through the rescoring LM; the model holds the best checkpoint's parameters again
    back, d2 = lm.load_lm_checkpoint(path)
    assert d2.word2idx == d.word2idx and back.rnn_type == 'LSTM'
    assert torch.equal(back.flat_parameters, model.flat_parameters)
    state = torch.load(path, map_location='cpu', weights_only=False)['model_state_dict']
    assert all(torch.equal(v.cpu(), state[k]) for k, v in model.state_dict().items())
    scorer = mtl_amd.lmscore.LM(path)
    assert torch.equal(scorer.model.flat_parameters, model.flat_parameters)
    assert out['final_val'] == lm.evaluate(back, va_data, BPTT) == out['final_test'] == best
    # fine-tuning on a second stream: load -> train_epoch x 3 at lr 2.0 lowers that stream's loss; deterministic at dropout 0
    ft_data = lm.batchify(lm.synth_corpus(8, V, 330), 10).cuda()
    runs = []
    for _ in range(2):
        m2, _ = lm.load_lm_checkpoint(path)
        before = lm.evaluate(m2, ft_data, BPTT)
        ft = lm.LMTrainer(m2, lr=2.0, clip=CLIP, bptt=BPTT)
        for ep in range(3):
            ft.train_epoch(ft_data, ep + 1)
        after = lm.evaluate(m2, ft_data, BPTT)
        assert after < before
        assert sorted(ft._tables) == [0] and int(m2.engine.sync_ws[1]) == 0
        runs.append(m2.flat_parameters.clone())
    assert torch.equal(runs[0], runs[1])
    assert int(model.engine.sync_ws[1]) == 0


# ------------------------------------------------------------------------------------------- last: the stream with a 1-step window
@pytest.mark.parametrize('kind,tied', [('LSTM', False), ('GRU', False), ('GRU', True)])
def test_epoch_with_a_one_step_last_window(kind, tied):
    """S = 32: five windows of 6 steps and one of ONE step (the persistent launches accept T = 1): bitwise against the composed
    earlier calls, and the free run against fp64"""
    _free_run(kind, tied, 32)
