"""A model built with feat_extractor='large_cnn' through every path that runs the front-end, on the MI355X, at the size of
tests/golden/LC0.npz (written by the real reference: tools/make_golden_large_cnn.py) and against the restatement of
tests/large_cnn_util.py run live -- with the bars of tests/test_parity_gpu.py: labels bit-exact, loss within 1e-4, at most 8 ReLU /
max-pool decisions different from the free-running oracle (each a near-tie), and with the device's decisions replayed EVERY gradient
tensor within 1e-4."""
import os

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import golden_util as gu
from tests import large_cnn_util as LU
from tests.test_batched_gpu import _crop_gates, _decisions_differ, _iteration, _ragged_tasks, _tensor_errs
from tests.test_parity_gpu import CLEAN_MIN, GOLDEN_BAND, RTOL, _pass_parity

pytestmark = pytest.mark.gpu


def make(**over):
    import mtl_amd
    z, cfg, spec = gu.load('LC0')
    model, vocab, args = LU.device_model(cfg, spec, **over)
    return mtl_amd, z, cfg, spec, args, vocab, model.cuda()


def test_every_pass_of_a_meta_step_against_live_oracle():
    """train pass at theta0 and validation pass at theta' for every task of LC0, each against the restatement at the SAME parameters"""
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    assert all(e.conv_layers is mtl_amd.convstack.LAYERS_LARGE for e in model.engines)
    oracle = LU.build_model(cfg)
    tr, val = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    for m, batch in enumerate(tr):
        g_tr, _ = _pass_parity(model, oracle, batch, model.flat_parameters, 'LC0 task %d train' % m)
        assert model.engine.saved['conv_mode'] == 'x3' and model.engine.saved['in_h2'] is False
        theta1 = inner.theta_prime_from(model.flat_parameters, g_tr).clone()
        _pass_parity(model, oracle, val, theta1, 'LC0 task %d valid' % m)


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


def test_meta_step_matches_the_reference_golden():
    """one meta-step of TransientTrainer.train (3 tasks, task-batched) against LC0's labels, losses, G and theta1, in the bands
    tests/test_parity_gpu.py applies to F0"""
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    names = [str(s) for s in z['param_names']]
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=spec['variable']) for m in range(spec['n_tasks'])]
    trainer = mtl_amd.TransientTrainer()
    reads = _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, 0)
    assert trainer.h2_census is None                                       # no h2 operand: the census is skipped
    for m, (tr, va) in enumerate(reads):
        for j, rd in ((2 * m, tr), (2 * m + 1, va)):
            key = 'fwd/0/%d' % j
            assert np.array_equal(rd.gold_host.numpy(), z[key + '/gold']) and np.array_equal(rd.hyp.numpy(), z[key + '/hyp']), key
            ref = float(z[key + '/loss'])
            assert abs(float(rd.loss[0]) - ref) <= RTOL * abs(ref), key
    floor = 1e-4 * gu.global_l2(z, 'G/0', names)
    errs = [gu.check_digest(z, 'G/0', nm, model._layout.view(model._G, nm), rtol=GOLDEN_BAND['F0'], what='LC0', floor=floor) for nm in names]
    clean = sum(e <= RTOL for e in errs)
    print('LC0 it 0: %d/%d meta-gradient tensors within 1e-4, worst %.3e' % (clean, len(errs), max(errs)))
    assert clean >= CLEAN_MIN['F0'], (clean, len(errs))
    for (nm, p), e in zip(model.named_parameters(), errs):
        if float(z['G/0/%s/l2' % nm]) < floor * 1e-2:
            continue
        gu.check_digest(z, 'theta/1', nm, p, rtol=RTOL if e <= RTOL / 10 else GOLDEN_BAND['F0'], what='LC0')


def test_command_lists_equal_the_eager_step_bitwise():
    """the task-batched step eager, recorded and replayed"""
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    as5 = lambda b: (b[0].cuda(), b[1], None, b[2], None)
    tr_b, val_b = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    tasks, val, n = [as5(b) for b in tr_b], as5(val_b), len(tr_b)
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
    # ... and the lanes (one task per engine, single-task launches) give the batched step's G to the summation-order bar
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
        oracle = LU.build_model(cfg)
        adam = R.AdamState(list(oracle.parameters()), spec['meta_lr'])
        batches = [R.synth_batch(10 * t, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], True) for t in range(spec['n_tasks'])]
        _, losses = R.joint_step(oracle, adam, batches)
        ref = sum(losses) / len(losses)
        assert abs(tr.loss_trace[0] - ref) <= RTOL * ref


def test_meta_step_with_ctc_loss_runs():
    mtl_amd, z, cfg, spec, args, vocab, model = make()
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=False) for m in range(spec['n_tasks'])]
    theta0 = model.flat_parameters.clone()
    trainer = mtl_amd.TransientTrainer()
    trainer.train(model, vocab, tasks, [], 'ctc', 0, 1, args, evaluate_every=10 ** 9, early_stop='cer,200', is_copy_grad=True)
    assert bool(torch.isfinite(model._G).all()) and float(model._G.norm()) > 0 and not torch.equal(theta0, model.flat_parameters)


def test_greedy_and_beam_decoding_equal_the_restatement():
    mtl_amd, z, cfg, spec, args, vocab, model = make(cuda=False)
    bspec = gu.load_beam()[0]
    gu.perturb_output_layer(model.decoder.output_linear.weight, bspec)      # (natural EOS terminations of different lengths)
    oracle = LU.build_model(cfg)
    gu.perturb_output_layer(oracle.decoder.output_linear.weight, bspec)
    model = model.cuda()
    x, lens, y = R.synth_batch(5, 2, 72, 6, cfg['vocab_size'], True)
    steps = 24
    model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=steps)
    assert torch.equal(model.last_greedy_ids.t().contiguous(), R.greedy_search(oracle, x, lens, vocab.SOS_ID, steps))
    args.beam_width, args.beam_nbest, args.tgt_max_len = 4, 3, cfg['tgt_max_len']
    model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=vocab.SOS_ID)
    nw = gu.label_words(vocab.id2label, [vocab.PAD_TOKEN, vocab.SOS_TOKEN, vocab.EOS_TOKEN])
    ref = R.beam_search(oracle, x, lens, vocab.SOS_ID, 4, 3, cfg['tgt_max_len'], nw)
    assert model.last_beam_ids == [seq for utt in ref for seq, _ in utt]


def test_checkpoint_round_trip_continues_bitwise(tmp_path):
    """save_meta_model after one meta-step -> load_meta_model: the loaded model, with the loaded optimizers, takes the second step bit for bit"""
    mtl_amd, z, cfg, spec, args, vocab, model = make(save_folder=str(tmp_path))
    mk = lambda: [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=True) for m in range(spec['n_tasks'])]
    tasks, trainer = mk(), mtl_amd.TransientTrainer()
    _meta_step(mtl_amd, z, cfg, spec, args, vocab, model, trainer, tasks, 0)
    path = mtl_amd.save_meta_model(model, vocab, 1, trainer.inner_opt, trainer.outer_opt, {'avg_valid_cer': 1.0}, args)
    m2, v2, inner2, outer2, epoch, metrics, a2 = mtl_amd.load_meta_model(path)
    assert epoch == 1 and a2.feat_extractor == 'large_cnn' and m2.feat_extractor == 'large_cnn' and a2.dim_input == 2560
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


def test_tasks_of_different_frame_counts_in_one_pass_equal_a_lane_per_task():
    """a manifest-like batch: every task at its own frame count, stacked at the widest with `widths` -- the per-task passes' labels,
    losses and (decisions alike) gradients, as tests/test_batched_gpu.py asserts for the VGG stack"""
    mtl_amd, z, cfg, spec, args, vocab, model = make()
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
    print('LC0 frames %s: stacked vs lanes: %d differing decisions, worst tensor %.2e (%s)' % (frames, flips, errs[worst], worst))
    assert flips <= 2 and errs[worst] < (1e-4 if flips == 0 else 1e-2), (worst, errs[worst], flips)
    for rnd in range(3):                                  # eager, recording, replay
        G2, _, _, _ = _iteration(mtl_amd, model, vocab, args, tasks, val, n, inner, True, tr=tr)
        assert torch.equal(G2, G1)
