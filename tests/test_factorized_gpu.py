"""A model built with --is-factorized (factorized feed-forward blocks, input_linear_a / _b) through every path, on the MI355X, at the size
of tests/golden/FZ0.npz (written by the real reference: tools/make_golden_factorized.py) and against the restatement of
tests/factorized_util.py run live -- with the structure and the bars of tests/test_large_cnn_gpu.py, which are those of
tests/test_parity_gpu.py: labels bit-exact, loss within 1e-4, at most 8 ReLU / max-pool decisions different from the free-running
oracle (each a near-tie), and with the device's decisions replayed EVERY gradient tensor within 1e-4.  Both routes of the feed-forward
middle (PassEngine.ffn_mid_fused: csrc/mtl_ffn_lr.hip, or two product calls) run; and a dense model still issues the calls recorded in
tests/golden/calltrace.json.gz."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import factorized_util as FU
from tests import golden_util as gu
from tests.test_batched_gpu import _crop_gates, _decisions_differ, _iteration, _ragged_tasks, _tensor_errs
from tests.test_parity_gpu import CLEAN_MIN, GOLDEN_BAND, RTOL, _pass_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(fused=None, cfg_over=None, **over):
    import mtl_amd
    z, cfg, spec = gu.load('FZ0')
    cfg = dict(cfg, **(cfg_over or {}))
    model, vocab, args = FU.device_model(cfg, spec, **over)
    model = model.cuda()
    assert all(e.factorized for e in model.engines)
    if fused is not None:
        for e in model.engines:
            e.ffn_mid_fused = fused
    return mtl_amd, z, cfg, spec, args, vocab, model


def _as5(b):
    return (b[0].cuda(), b[1], None, b[2], None)


@pytest.mark.parametrize('fused,cfg_over', [(True, None), (False, None), (True, dict(r=36, dim_inner=72)), (False, dict(r=36, dim_inner=72))],
                         ids=['fused', 'two-call', 'fused-r36-inner72', 'two-call-r36-inner72'])
def test_every_pass_of_a_meta_step_against_live_oracle(fused, cfg_over):
    """train pass at theta0 and validation pass at theta' for every task of FZ0, each against the restatement at the SAME parameters"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(fused, cfg_over)
    assert model._layout.entries['encoder.layers.0.pos_ffn.linear_1_b.weight'][1] == (cfg['dim_inner'], cfg['r'])
    oracle = FU.build_model(cfg)
    tr, val = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    for m, batch in enumerate(tr):
        g_tr, _ = _pass_parity(model, oracle, batch, model.flat_parameters, 'FZ0 task %d train' % m)
        assert model.engine.saved['conv_mode'] == 'h2' and model.engine.saved['in_h2'] is True       # stage A of the input pair stays on h2
        theta1 = inner.theta_prime_from(model.flat_parameters, g_tr).clone()
        _pass_parity(model, oracle, val, theta1, 'FZ0 task %d valid' % m)


def test_fused_and_two_call_routes_agree():
    """one pass on either route: the same labels, losses to fp32 rounding, gradients to the summation-order bar"""
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    x, lens, y = gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][0]
    outs = []
    for fused in (False, True):
        model.engine.ffn_mid_fused = fused
        out = model.pass_forward(x.cuda(), lens, y)
        g = torch.zeros_like(model.flat_grad)
        model.pass_backward(g, 1.0)
        outs.append((float(out['loss']), out['hyp'].clone(), g))
    (l0, h0, g0), (l1, h1, g1) = outs
    assert torch.equal(h0, h1) and abs(l0 - l1) <= 2e-6 * abs(l0)
    assert float((g0 - g1).norm() / g0.norm()) < 1e-4


def test_forward_only_pass_keeps_no_inner_activation():
    mtl_amd, z, cfg, spec, args, vocab, model = make(True)
    x, lens, y = gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][0]
    ref = model.pass_forward(x.cuda(), lens, y)
    loss, hyp = float(ref['loss']), ref['hyp'].clone()
    eng = model.engine
    eng.forward_only = True
    try:
        out = model.pass_forward(x.cuda(), lens, y)
        assert float(out['loss']) == loss and torch.equal(out['hyp'], hyp)           # c is bitwise the same with and without h
        assert 'e0.ff.h1' not in eng.arena and 'd0.ff.h1' not in eng.arena
        with pytest.raises(RuntimeError, match='forward_only'):
            model.pass_backward(torch.zeros_like(model.flat_grad), 1.0)
    finally:
        eng.forward_only = False


def _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, it):
    captured = {}
    orig = trainer.meta_iteration

    def spy(*a, **kw):
        captured['reads'] = orig(*a, **kw)
        return captured['reads']
    trainer.meta_iteration = spy
    trainer.train(model, vocab, tasks, [], 'ce', it, it + 1, args, inner_opt=getattr(trainer, 'inner_opt', None),
                  outer_opt=getattr(trainer, 'outer_opt', None), evaluate_every=10 ** 9, early_stop='cer,200', is_copy_grad=True)
    trainer.meta_iteration = orig
    return captured['reads']


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two-call'])
def test_meta_step_matches_the_reference_golden(fused):
    """one meta-step of TransientTrainer.train (3 tasks, task-batched) against FZ0's labels, losses, G and theta1, in the bands
    tests/test_parity_gpu.py applies to F0"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(fused)
    names = [str(s) for s in z['param_names']]
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=spec['variable']) for m in range(spec['n_tasks'])]
    trainer = mtl_amd.TransientTrainer()
    reads = _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, 0)
    for m, (tr, va) in enumerate(reads):
        for j, rd in ((2 * m, tr), (2 * m + 1, va)):
            key = 'fwd/0/%d' % j
            assert np.array_equal(rd.gold_host.numpy(), z[key + '/gold']) and np.array_equal(rd.hyp.numpy(), z[key + '/hyp']), key
            ref = float(z[key + '/loss'])
            assert abs(float(rd.loss[0]) - ref) <= RTOL * abs(ref), key
    floor = 1e-4 * gu.global_l2(z, 'G/0', names)
    errs = [gu.check_digest(z, 'G/0', nm, model._layout.view(model._G, nm), rtol=GOLDEN_BAND['F0'], what='FZ0', floor=floor) for nm in names]
    clean = sum(e <= RTOL for e in errs)
    print('FZ0 it 0: %d/%d meta-gradient tensors within 1e-4, worst %.3e' % (clean, len(errs), max(errs)))
    assert clean >= CLEAN_MIN['F0'], (clean, len(errs))
    for (nm, p), e in zip(model.named_parameters(), errs):
        if float(z['G/0/%s/l2' % nm]) < floor * 1e-2:
            continue
        gu.check_digest(z, 'theta/1', nm, p, rtol=RTOL if e <= RTOL / 10 else GOLDEN_BAND['F0'], what='FZ0')


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two-call'])
def test_command_lists_equal_the_eager_step_bitwise(fused):
    """the task-batched step eager, recorded and replayed; and the lanes (one task per engine) to the summation-order bar"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(fused)
    tr_b, val_b = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    tasks, val, n = [_as5(b) for b in tr_b], _as5(val_b), len(tr_b)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    eager = mtl_amd.TransientTrainer()
    eager.use_cmdlists = False
    G0, r0, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, True, tr=eager)
    tr = mtl_amd.TransientTrainer()
    for rnd in range(3):                                  # first sighting of the key (eager), recording, replay
        G1, r1, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, True, tr=tr)
        assert torch.equal(G0, G1), rnd
        for (l0, h0, g0), (l1, h1, g1) in zip(r0, r1):
            assert l0 == l1 and torch.equal(h0, h1) and torch.equal(g0, g1)
    assert any(k_[0] == 'batched' and tr.replay.recorded(k_) for k_ in tr.replay.keys()), 'no command list was recorded'
    if fused:
        names = tr.replay.recorded()[0]._names()
        ops = {names[c.op] for cl in tr.replay.recorded() for c in cl.buf[:cl.n]}
        assert 'mtl_ffn_lr_mid_fwd' in ops, 'the recorded step does not replay the fused kernel'
    G2, r2, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, False)
    errs = _tensor_errs(model, G2, G0)
    assert max(errs.values()) < 1e-2 and float((G2 - G0).norm() / G0.norm()) < 1e-4, max(errs.values())
    for (l0, h0, g0), (l2, h2, g2) in zip(r0, r2):
        assert abs(l0 - l2) <= 2e-6 * abs(l0) and torch.equal(h0, h2)


@pytest.mark.parametrize('loss', ['ce', 'ctc'])
def test_joint_trainer_iteration_runs(loss):
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    args.loss = loss
    # (ctc: full-length utterances -- 16 encoder frames for 8 labels; a ragged batch has utterances without an alignment)
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=loss == 'ce') for m in range(spec['n_tasks'])]
    theta0 = model.flat_parameters.clone()
    tr = mtl_amd.JointTrainer()
    tr.train(model, vocab, tasks, [], loss, 0, 1, args, evaluate_every=10 ** 9, early_stop='cer,200')
    assert len(tr.loss_trace) == 1 and np.isfinite(tr.loss_trace[0]) and not torch.equal(theta0, model.flat_parameters)
    if loss == 'ce':
        oracle = FU.build_model(cfg)
        adam = R.AdamState(list(oracle.parameters()), spec['meta_lr'])
        batches = [R.synth_batch(10 * t, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], True) for t in range(spec['n_tasks'])]
        _, losses = R.joint_step(oracle, adam, batches)
        ref = sum(losses) / len(losses)
        assert abs(tr.loss_trace[0] - ref) <= RTOL * ref


@pytest.mark.parametrize('loss,dropout,fused', [('ctc', 0.0, False), ('ce', 0.1, False), ('ce', 0.1, True)], ids=['ctc', 'dropout', 'dropout-fused'])
def test_meta_step_with_ctc_and_with_dropout_runs(loss, dropout, fused):
    mtl_amd, z, cfg, spec, args, vocab, model = make(fused, dropout=dropout)
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=loss == 'ce') for m in range(spec['n_tasks'])]
    theta0 = model.flat_parameters.clone()
    trainer = mtl_amd.TransientTrainer()
    trainer.train(model, vocab, tasks, [], loss, 0, 1, args, evaluate_every=10 ** 9, early_stop='cer,200', is_copy_grad=True)
    assert bool(torch.isfinite(model._G).all()) and float(model._G.norm()) > 0 and not torch.equal(theta0, model.flat_parameters)


def test_greedy_and_beam_decoding_equal_the_restatement_and_the_golden():
    """the searches on merged feed-forward pairs: token for token the restatement's, and the reference's recorded in FZ0"""
    import json
    mtl_amd, z, cfg, spec, args, vocab, model = make(cuda=False)
    sp = json.loads(bytes(z['decode/spec']).decode())
    model = model.cpu()
    gu.perturb_output_layer(model.decoder.output_linear.weight, sp)      # (natural EOS terminations of different lengths)
    oracle = FU.build_model(cfg)
    gu.perturb_output_layer(oracle.decoder.output_linear.weight, sp)
    model = model.cuda()
    x, lens, y = R.synth_batch(sp['seed'], sp['k'], sp['T'], sp['L'], cfg['vocab_size'], True)
    steps = sp['greedy_steps']
    model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=steps)
    got = model.last_greedy_ids.t().contiguous()
    assert torch.equal(got, R.greedy_search(oracle, x, lens, vocab.SOS_ID, steps))
    assert np.array_equal(got.numpy(), z['decode/greedy_ids'].T)
    args.beam_width, args.beam_nbest, args.tgt_max_len = sp['beam_width'], sp['nbest'], cfg['tgt_max_len']
    nw = gu.label_words(vocab.id2label, [vocab.PAD_TOKEN, vocab.SOS_TOKEN, vocab.EOS_TOKEN])
    ref = R.beam_search(oracle, x, lens, vocab.SOS_ID, sp['beam_width'], sp['nbest'], cfg['tgt_max_len'], nw)
    golden = [[int(v) for v in row if v >= 0] for row in z['decode/beam_ids']]
    for device_ranking in (False, True):
        model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=vocab.SOS_ID, device_ranking=device_ranking)
        assert model.last_beam_ids == [seq for utt in ref for seq, _ in utt], device_ranking
        assert [list(map(int, s)) for s in model.last_beam_ids] == golden, device_ranking


def test_checkpoint_round_trip_continues_bitwise(tmp_path):
    """save_meta_model after one meta-step -> load_meta_model: the loaded model, with the loaded optimizers, takes the second step bit for bit"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(save_folder=str(tmp_path))
    mk = lambda: [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=True) for m in range(spec['n_tasks'])]
    tasks, trainer = mk(), mtl_amd.TransientTrainer()
    _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, 0)
    path = mtl_amd.save_meta_model(model, vocab, 1, trainer.inner_opt, trainer.outer_opt, {'avg_valid_cer': 1.0}, args)
    m2, v2, inner2, outer2, epoch, metrics, a2 = mtl_amd.load_meta_model(path)
    assert epoch == 1 and a2.is_factorized is True and a2.r == 100 and m2.is_factorized and all(e.factorized for e in m2.engines)
    assert m2.flat_parameters.is_cuda and torch.equal(m2.flat_parameters, model.flat_parameters)
    calls = tasks[0].calls
    _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, 1)
    tasks2, trainer2 = mk(), mtl_amd.TransientTrainer()
    for t in tasks2:
        t.calls = calls                                    # the data the first model's second step consumed
    trainer2.train(m2, v2, tasks2, [], 'ce', 1, 2, a2, inner_opt=inner2, outer_opt=outer2, evaluate_every=10 ** 9, early_stop='cer,200',
                   is_copy_grad=True)
    assert torch.equal(m2._G, model._G) and torch.equal(m2.flat_parameters, model.flat_parameters)
    assert os.path.exists(path)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two-call'])
def test_tasks_of_different_frame_counts_in_one_pass_equal_a_lane_per_task(fused):
    """a manifest-like batch: every task at its own frame count, stacked at the widest with `widths` -- the per-task passes' labels,
    losses and (decisions alike) gradients, as tests/test_batched_gpu.py asserts for the dense model"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(fused)
    k, V, frames, val_frames, widths = spec['k'], cfg['vocab_size'], (64, 53, 46), 60, (8, 5, 11)
    tasks = _ragged_tasks(mtl_amd, k, frames, widths, V, 140)
    val = _ragged_tasks(mtl_amd, k, (val_frames,), (6,), V, 199)[0]
    n = len(tasks)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    own = mtl_amd.TransientTrainer()
    own.pad_lanes = '0'                                   # the reference's schedule: every task at its own width
    G0, r0, _, log0 = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, False, tr=own, gates=True)
    tr = mtl_amd.TransientTrainer()
    G1, r1, tr, log1 = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, True, tr=tr, gates=True)
    assert tr.last_schedule == 'batched-ragged', 'the ragged tasks did not take the task-batched pass'
    flips = 0
    for i, (ga, gb) in enumerate(zip(log0, log1)):
        t, is_val = i // 2, i % 2
        crop, beyond = _crop_gates(gb, k, val_frames if is_val else frames[t], 7 if is_val else widths[t] + 1)
        assert beyond == 0 or is_val, (i, beyond)
        flips += _decisions_differ(ga, crop)
    for (l0, h0, g0), (l1, h1, g1) in zip(r0, r1):
        w = g0.shape[1]
        assert torch.equal(g0, g1[:, :w]) and torch.equal(h0, h1[:, :w]) and bool((h1[:, w:] == 0).all())
        assert abs(l0 - l1) <= 2e-6 * abs(l0), (l0, l1)
    errs = _tensor_errs(model, G1, G0)
    worst = max(errs, key=errs.get)
    print('FZ0 frames %s: stacked vs lanes: %d differing decisions, worst tensor %.2e (%s)' % (frames, flips, errs[worst], worst))
    assert flips <= 2 and errs[worst] < (1e-4 if flips == 0 else 1e-2), (worst, errs[worst], flips)
    for rnd in range(3):                                  # eager, recording, replay
        G2, _, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, True, tr=tr)
        assert torch.equal(G2, G1)


@pytest.mark.parametrize('kind', ['large_cnn', 'logfbank'])
def test_large_cnn_and_logfbank_factorized_models_run_a_meta_step(kind):
    """the flag combines with the front-ends as the dense model does: the 2560-wide input pair behind the narrow convolutions (exact
    split, no h2) and behind 80 filterbank bands (h2)"""
    over = dict(feat_extractor='large_cnn') if kind == 'large_cnn' else dict(feat='logfbank')
    mtl_amd, z, cfg, spec, args, vocab, model = make(True, **over)
    bins = 161 if kind == 'large_cnn' else 80
    assert args.dim_input == 2560 and model._layout.entries['encoder.input_linear_a.weight'][1] == (cfg['r'], 2560)
    k, V = spec['k'], cfg['vocab_size']
    tasks = [_as5(mtl_amd.synth_batch(70 + m, k, spec['T'], spec['L'], V, variable=True, freq_bins=bins)) for m in range(spec['n_tasks'])]
    val = _as5(mtl_amd.synth_batch(79, k, spec['T'], spec['L'], V, variable=True, freq_bins=bins))
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    G, reads, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, len(tasks), inner, True)
    assert model.engine.saved['in_h2'] is (kind == 'logfbank')
    assert bool(torch.isfinite(G).all()) and float(G.norm()) > 0 and all(np.isfinite(l) for l, _, _ in reads)
    for nm in ('encoder.input_linear_a.weight', 'encoder.input_linear_b.weight', 'encoder.input_linear_b.bias',
               'encoder.layers.0.pos_ffn.linear_1_a.weight', 'decoder.layers.0.pos_ffn.linear_2_b.bias'):
        assert float(model._layout.view(G, nm).norm()) > 0, nm
    G2, _, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, len(tasks), inner, False)      # a lane per task
    assert float((G2 - G).norm() / G.norm()) < 1e-4


def test_dense_model_issues_the_recorded_calls():
    """nothing existing moved: a non-factorized model's passes issue the calls of tests/golden/calltrace.json.gz, recorded before
    --is-factorized existed (the helper tests/test_calltrace_gpu.py uses)"""
    spec = importlib.util.spec_from_file_location('calltrace', os.path.join(ROOT, 'tools', 'calltrace.py'))
    calltrace = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(calltrace)
    want = calltrace.load()
    eng, theta = calltrace.fixture_model()
    assert not eng.factorized and not eng.forward_only
    got = calltrace.traces(eng, theta)
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], name
        assert not any(c[0].startswith('mtl_ffn_lr') for c in got[name])
