"""GPU: --loss ctc through the engine's loss stage and the trainers, on the F0 golden configuration.

  * the in-engine path (prepare -> forward_device(loss_type='ctc') -> backward) against the drop-in path (model(...) ->
    calculate_metrics(ctc) -> loss.backward()), with the same comparison made for 'ce' (existing code) as the yardstick;
  * one ctc meta-iteration, task-batched against the per-task lanes, on tasks with ragged label widths (in_len must come from each
    task's OWN decoder width), eager / recorded / replayed, and never replaying a list recorded for ce;
  * the in-engine gradient against the fp64 oracle's d(pred) fed through the existing external-dpred backward;
  * TransientTrainer.train / JointTrainer.train with loss_type='ctc' and the in-loop validation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ctc_ref as CR
from tests import golden_util as gu
from tests.test_batched_gpu import _iteration, _tensor_errs
from tests.test_parity_gpu import make

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)


def _setup():
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    return mtl_amd, args, vocab, model.cuda(), cfg, spec


def _no_adjacent_repeats(y):
    """labels (B, L) >= 4 with every adjacent repeat broken (CTC needs a blank row between equal neighbours)"""
    y = y.clone()
    for i in range(1, y.shape[1]):
        same = (y[:, i] == y[:, i - 1]) & (y[:, i] != 0)
        y[same, i] = (y[same, i] - 4 + 1) % 8 + 4
    return y


def _engine_pass(model, x, lens, y, pct, tl, loss_type, dpred=None, want_dlog=False):
    eng = model._need_engine()
    theta = model.flat_parameters
    meta = eng.prepare(lens, y, x.shape[0], x.shape[3], percentages=pct, target_sizes=tl)
    out = eng.forward_device(theta, x, meta, loss_type=loss_type)
    g = torch.zeros_like(theta)
    eng.backward(g, 1.0, dpred=dpred)
    torch.cuda.synchronize()
    res = dict(g=g, loss=float(out['loss'][0]), hyp=out['hyp'].clone(), pred=out['pred'].clone(), meta=meta)
    if want_dlog:
        V = out['pred'].shape[2]
        res['dlog'] = eng.arena['_dpred'][:, :V].clone()
    return res


def _dropin_pass(mtl_amd, model, vocab, x, lens, y, pct, tl, loss_type):
    model.zero_grad()
    pred, gold, hyp = model(x, lens, y.cuda())
    sizes = pct.clone().mul_(int(pred.size(1))).int()
    loss, _ = mtl_amd.calculate_metrics(pred, gold, vocab.PAD_ID, input_lengths=sizes, target_lengths=tl, loss_type=loss_type)
    loss.backward()
    torch.cuda.synchronize()
    return dict(g=model.flat_grad.clone(), loss=float(loss.detach()), hyp=hyp.clone())


@pytest.mark.parametrize('variable', [True, False])
def test_in_engine_loss_stage_equals_the_drop_in_path(variable):
    """yardstick: the same two paths compared for 'ce' -- they share every kernel but the leading dimension of dlog (padded to a
    multiple of 4 in the engine), which may route the two products that read it differently.  ctc may differ 4 x as much per tensor."""
    mtl_amd, args, vocab, model, cfg, spec = _setup()
    x, lens, y = mtl_amd.synth_batch(40, spec['k'], spec['T'], 8, cfg['vocab_size'], variable=variable)
    y = _no_adjacent_repeats(y)
    x = x.cuda()
    pct, tl = lens.float() / x.shape[3], (y != 0).sum(1).to(torch.int32)
    d = {}
    for lt in ('ce', 'ctc'):
        a = _engine_pass(model, x, lens, y, pct, tl, lt)
        b = _dropin_pass(mtl_amd, model, vocab, x, lens, y, pct, tl, lt)
        assert torch.equal(a['hyp'], b['hyp'])
        assert (np.isinf(a['loss']) and np.isinf(b['loss']) and a['loss'] > 0) or abs(a['loss'] - b['loss']) <= 1e-6 * abs(b['loss']), (a['loss'], b['loss'])
        assert bool(torch.isfinite(a['g']).all()) and bool(torch.isfinite(b['g']).all())
        d[lt] = _tensor_errs(model, a['g'], b['g'])
        if lt == 'ctc':
            assert np.isfinite(a['loss']) == (not variable)          # (the ragged batch has utterances without an alignment)
            assert float(a['g'].norm()) > 0
    worst = max(d['ctc'], key=lambda nm: d['ctc'][nm] / max(d['ce'][nm], 1e-30))
    print('in-engine vs drop-in (variable=%s): worst ce %.2e, worst ctc %.2e; largest ctc / ce ratio %.2f (%s: %.2e vs %.2e)'
          % (variable, max(d['ce'].values()), max(d['ctc'].values()), d['ctc'][worst] / max(d['ce'][worst], 1e-30), worst, d['ctc'][worst], d['ce'][worst]))
    for nm in d['ce']:
        if d['ce'][nm] == 0:
            assert d['ctc'][nm] == 0, nm
        else:
            assert d['ctc'][nm] <= 4 * d['ce'][nm], (nm, d['ctc'][nm], d['ce'][nm])


def test_ctc_meta_iteration_batched_equals_lanes_and_is_keyed_apart_from_ce():
    """as tests/test_batched_gpu.py::test_task_batched_iteration_equals_per_task_lanes, with the ctc objective: the tasks' label widths
    differ (8, 5, 11, 8), the batched pass pads all to 12 positions, and every task's in_len must still be (pct * its own width).int()"""
    mtl_amd, args, vocab, model, cfg, spec = _setup()
    k, T, V = spec['k'], spec['T'], cfg['vocab_size']
    # percentages (1, 0.9): in_len = (9, 8), (6, 5), (12, 10), (9, 8) from the tasks' own widths 9, 6, 12, 9 -- every utterance has an
    # alignment and a finite loss -- where the padded width 12 would give (12, 10) to all; task 1 derives them (None, like the tests' tuples)
    pct = lambda m: None if m == 1 else torch.tensor([1.0, 0.9])
    as5 = lambda b, m: (b[0].cuda(), b[1], pct(m), _no_adjacent_repeats(b[2]), None)
    tasks = [as5(mtl_amd.synth_batch(40 + m, k, T, Lm, V, variable=True), m) for m, Lm in enumerate((8, 5, 11, 8))]
    val = as5(mtl_amd.synth_batch(99, k, T, 6, V, variable=True), 0)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    lanes, batched = mtl_amd.TransientTrainer(), mtl_amd.TransientTrainer()
    lanes.loss_type = batched.loss_type = 'ctc'
    G0, r0, _, log0 = _iteration(mtl_amd, model, vocab, args, tasks, val, 4, inner, False, tr=lanes, gates=True)
    G1, r1, tr, log1 = _iteration(mtl_amd, model, vocab, args, tasks, val, 4, inner, True, tr=batched, gates=True)
    assert lanes.last_schedule == 'lanes' and batched.last_schedule == 'batched'
    flips = 0
    for ga, gb in zip(log0, log1):
        for key in ga:
            a_, b_ = ga[key], gb[key]
            if a_.shape != b_.shape:
                a_ = a_.view(k, -1, a_.shape[-1])
                b_ = b_.view(k, -1, b_.shape[-1])[:, :a_.shape[1]]
            flips += int((a_ != b_).sum())
    for (l0, h0, g0), (l1, h1, g1) in zip(r0, r1):
        w = g0.shape[1]
        assert torch.equal(g0, g1[:, :w]) and torch.equal(h0, h1[:, :w])
        assert (np.isinf(l0) and np.isinf(l1) and l0 > 0 and l1 > 0) or abs(l0 - l1) <= 1e-6 * abs(l0), (l0, l1)
    assert [bool(np.isfinite(r[0])) for r in r0] == [True, True, False, True, True, True, True, True]   # (train, val) per task
    assert bool(torch.isfinite(G0).all()) and float(G0.norm()) > 0
    errs = _tensor_errs(model, G1, G0)
    worst = max(errs, key=errs.get)
    strict = {nm: e for nm, e in errs.items() if not nm.endswith('key_linear_b.bias')}
    ws_ = max(strict, key=strict.get)
    print('ctc batched vs lanes: %d differing branch decisions, worst tensor %.2e (%s), losses %s' % (flips, errs[worst], worst, [r[0] for r in r0]))
    assert flips <= 4
    assert strict[ws_] < (1.5e-5 if flips == 0 else 1e-2) and errs[worst] < (1e-4 if flips == 0 else 1e-2), (ws_, strict[ws_], worst, errs[worst], flips)
    for rnd in range(3):                                  # first sighting of the key (eager), recording, replay
        G2, r2, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, 4, inner, True, tr=tr)
        assert torch.equal(G2, G1)
        for (l1, h1, g1), (l2, h2, g2) in zip(r1, r2):
            assert (l1 == l2 or (np.isinf(l1) and np.isinf(l2))) and torch.equal(h1, h2) and torch.equal(g1, g2)
    assert any(k_[0] == 'batched' and 'ctc' in k_ and tr.replay.recorded(k_) for k_ in tr.replay.keys()), 'no ctc command list was recorded'
    # one trainer, the same shapes: ce lists and ctc lists never stand in for each other
    for sched in (True, False):
        one = mtl_amd.TransientTrainer()
        seen = {}
        for lt in ('ce', 'ctc', 'ce', 'ctc', 'ce', 'ctc'):          # warm, record, replay of both keys, interleaved
            one.loss_type = lt
            G, r, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, 4, inner, sched, tr=one)
            if lt in seen:
                assert torch.equal(G, seen[lt][0]), (sched, lt)
            seen[lt] = (G, r)
        assert not torch.equal(seen['ce'][0], seen['ctc'][0])
        assert all(np.isfinite(r[0]) for r in seen['ce'][1]) and seen['ce'][1][0][0] != seen['ctc'][1][0][0]
        assert sum(bool(one.replay.recorded(k_)) for k_ in one.replay.keys()) >= 2
    assert torch.equal(seen['ctc'][0], G0)                         # (the last round ran the lanes)


def _kernel_bound(pred, gold, in_len, tgt_len):
    """the kernel test's bound (tests/test_ctc_gpu.py) on the engine's own logits: 4 x the error of torch's fp32 CPU ctc_loss +
    autograd against the fp64 oracle, floor 4 fp32 ulp of the largest gradient element -> (bound, oracle d(pred) fp64, oracle nll)"""
    x = torch.from_numpy(pred).requires_grad_(True)
    lp = F.log_softmax(x.transpose(0, 1), 2)
    F.ctc_loss(lp, torch.from_numpy(gold), torch.from_numpy(in_len).long(), torch.from_numpy(tgt_len).long(), blank=0, reduction='mean',
               zero_infinity=True).backward()
    nll64, _, g64 = CR.ctc(pred, gold, in_len, tgt_len)
    y = float(np.abs(x.grad.numpy() - g64).max())
    return max(4 * y, 4 * EPS * float(np.abs(g64).max())), g64, nll64


@pytest.mark.parametrize('infeasible', [False, True])
def test_in_engine_gradient_against_the_fp64_oracle_end_to_end(infeasible):
    """d(pred) of the fp64 oracle on the device's own pred, fed through the existing external-dpred backward, against the in-engine
    ctc backward.  Three steps, each with its own bar:
      1. the engine's dlog against the oracle's: the kernel test's bound b (4 x torch's fp32 error on these logits);
      2. backward(oracle dlog) against backward(the engine's dlog), both through the external-dpred path (same launches): the
         backward is linear in dlog, so the difference is the backward of their difference, at most b per element -- bounded per
         tensor by 4 x the backward of a field of +-b on every live element (random signs give the typical, not the largest, image:
         hence the 4), plus the 4e-6 two fp32 runs of the same products on nearby inputs differ by (tests/test_batched_gpu.py; 1e-4
         for the key-projection biases, whose exact gradient is zero);
      3. backward(the engine's dlog) through the external path against the in-engine backward: the same numbers with another leading
         dimension, the bars of the batched-against-lanes comparison without a branch flip (1.5e-5, key biases 1e-4).
    infeasible: one utterance has fewer rows than labels: loss +inf, its dlog rows exactly 0, G finite and equal (by the same three
    steps) to the G of the oracle's dlog, whose rows for that utterance are zero."""
    mtl_amd, args, vocab, model, cfg, spec = _setup()
    k, T, V = spec['k'], spec['T'], cfg['vocab_size']
    x, lens, y = mtl_amd.synth_batch(41, k, T, 8, V, variable=False)
    y = _no_adjacent_repeats(y)
    x = x.cuda()
    pct = lens.float() / x.shape[3]
    if infeasible:
        pct[-1] = 0.5                                      # 9 decoder positions -> in_len 4 for 8 labels
    tl = (y != 0).sum(1).to(torch.int32)
    a = _engine_pass(model, x, lens, y, pct, tl, 'ctc', want_dlog=True)
    Td = a['pred'].shape[1]
    in_len = np.asarray(a['meta']['ctc_in_len_host'][0])
    assert np.array_equal(in_len, CR.in_len_from_percentages(pct.numpy(), Td)) and np.array_equal(a['meta']['ctc_tgt_len_host'][0], tl.numpy())
    gold = a['meta']['gold_host'].numpy()
    feas = [CR.feasible(gold[u, :int(tl[u])], int(in_len[u])) for u in range(k)]
    assert feas == [True] * (k - 1) + [not infeasible]
    pred = a['pred'].cpu().numpy()
    b, g64, nll64 = _kernel_bound(pred, gold, in_len, tl.numpy())
    assert np.isinf(a['loss']) == infeasible and bool(torch.isfinite(a['g']).all()) and float(a['g'].norm()) > 0
    dlog = a['dlog'].view(k, Td, V)
    e1 = float(np.abs(dlog.cpu().numpy() - g64).max())
    if infeasible:
        assert not bool(dlog[-1].any()) and not g64[-1].any() and np.isinf(nll64[-1])
    # every further pass reruns the same forward (dropout 0: the same bits), then backs an external d(pred) through it
    ext = lambda dp: _engine_pass(model, x, lens, y, pct, tl, 'ctc', dpred=dp.contiguous())
    o = ext(torch.from_numpy(g64.astype(np.float32)).cuda())
    s = ext(dlog)
    assert torch.equal(o['pred'], a['pred']) and torch.equal(s['pred'], a['pred'])
    gen = torch.Generator().manual_seed(3)
    live = torch.from_numpy((np.arange(Td)[None, :] < in_len[:, None]) & np.array(feas)[:, None]).view(k, Td, 1).float()
    field = (torch.randint(0, 2, (k, Td, V), generator=gen).float() * 2 - 1) * live * b
    p = ext(field.cuda())
    e2 = _tensor_errs(model, s['g'], o['g'])
    prop = {nm: float(model._layout.view(p['g'], nm).norm() / max(float(model._layout.view(o['g'], nm).norm()), 1e-4 * float(o['g'].norm())))
            for nm in model._layout.order}
    e3 = _tensor_errs(model, a['g'], s['g'])
    # (key-projection biases have an exactly-zero gradient -- softmax is shift-invariant -- and hold rounding noise: 1e-4, as everywhere)
    bound2 = {nm: 4 * prop[nm] + (1e-4 if nm.endswith('key_linear_b.bias') else 4e-6) for nm in e2}
    w2, w3 = max(e2, key=lambda nm: e2[nm] / bound2[nm]), max(e3, key=e3.get)
    print('ctc end to end (infeasible=%s): dlog abs err %.2e (bound %.2e); oracle-dlog vs engine-dlog backward: worst %.2e against its bound '
          '%.2e (%s), propagated part %.2e; external vs in-engine backward: worst %.2e (%s)'
          % (infeasible, e1, b, e2[w2], bound2[w2], w2, 4 * prop[w2], e3[w3], w3))
    assert e1 <= b, (e1, b)
    for nm in e2:
        assert e2[nm] <= bound2[nm], (nm, e2[nm], prop[nm])
        assert e3[nm] < (1e-4 if nm.endswith('key_linear_b.bias') else 1.5e-5), (nm, e3[nm])


class _Utterances(torch.utils.data.Dataset):
    """(spectrogram (F, T), transcript ids without adjacent repeats) items, as SpectrogramDataset.__getitem__ yields them"""

    def __init__(self, seed, n, V):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(n):
            T = int(torch.randint(24, 72, (1,), generator=g))
            L = int(torch.randint(2, 8, (1,), generator=g))
            self.items.append((torch.randn(161, T, generator=g), _no_adjacent_repeats(torch.randint(4, V, (1, L), generator=g))[0].tolist()))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _validation_loss(mtl_amd, trainer, model, vocab, loader, loss_type):
    model.eval()
    tot, nb = 0.0, 0
    with torch.no_grad():
        for src, trg, pct, src_lengths, trg_lengths in loader:
            loss, _, _ = trainer.forward_one_batch(model, vocab, src.cuda(), trg.cuda(), pct, src_lengths, trg_lengths, 0.0, loss_type)
            tot += loss.item()
            nb += 1
    model.train()
    return tot / nb


@pytest.mark.parametrize('which', ['transient', 'joint'])
def test_train_loops_with_ctc(tmp_path, which):
    """3 iterations with the in-loop validation on: both trainers complete, theta is finite and has moved (the synthetic tasks' ragged
    batches hold utterances without an alignment: their +inf loss is logged and never reaches theta), and the history holds the ctc
    validation loss (loader 0: one utterance per batch, finite; loader 1: pairs, the shorter utterance may have no alignment)."""
    mtl_amd, args, vocab, model, cfg, spec = _setup()
    args.save_folder, args.save_every, args.name = str(tmp_path), 10 ** 9, 'ctc'
    V = cfg['vocab_size']
    loaders = [mtl_amd.AudioDataLoader(vocab.PAD_ID, dataset=_Utterances(7, 3, V), batch_size=1),
               mtl_amd.AudioDataLoader(vocab.PAD_ID, dataset=_Utterances(8, 4, V), batch_size=2)]
    tasks = [mtl_amd.SyntheticTask(m, 2, 64, 8, V, variable=True) for m in range(3)]
    theta0 = model.flat_parameters.clone()
    if which == 'transient':
        tr = mtl_amd.TransientTrainer()
        tr.train(model, vocab, tasks, loaders, 'ctc', 0, 3, args, evaluate_every=1, early_stop='loss,100', is_copy_grad=True)
        assert tr.loss_type == 'ctc' and len(tr.loss_trace) == 3
    else:
        tr = mtl_amd.JointTrainer()
        tr.train(model, vocab, tasks, loaders, 'ctc', 0, 3, args, evaluate_every=1, early_stop='loss,100')
        assert len(tr.loss_trace) == 3
    theta = model.flat_parameters
    assert bool(torch.isfinite(theta).all()) and not torch.equal(theta, theta0)
    hist = tr.history
    assert len(hist) == 3 and all(len(h['valid_loss']) == 2 for h in hist)
    assert all(np.isfinite(h['valid_loss'][0]) and h['valid_loss'][0] > 0 for h in hist)
    assert hist[0]['valid_loss'][0] != hist[2]['valid_loss'][0]                                        # theta moved
    probe = mtl_amd.TransientTrainer()
    for i, loader in enumerate(loaders):
        want = _validation_loss(mtl_amd, probe, model, vocab, loader, 'ctc')
        got = hist[2]['valid_loss'][i]
        assert (np.isinf(got) and np.isinf(want)) or abs(got - want) <= 1e-6 * abs(want), (i, got, want)
    assert hist[2]['valid_loss'][0] != _validation_loss(mtl_amd, probe, model, vocab, loaders[0], 'ce')
    with pytest.raises(NotImplementedError):
        tr.train(model, vocab, tasks, loaders, 'mwer', 0, 1, args, **({'is_copy_grad': True} if which == 'transient' else {}))
