"""A model built with feat_extractor='none' on the MI355X: the two kernels of csrc/mtl_featproj.hip against fp64 at the bounds of
tests/x3_emul.py (tests/featnone_util.py; tests/test_featnone.py shows on the CPU that each bound separates six piece products from
five), and the model through the drop-in API, the trainers and the searches against tests/golden/N0.npz (written by the real
reference: tools/make_golden_featnone.py) and the restatement of tests/featnone_util.py run live, with the bars of
tests/test_parity_gpu.py: labels bit-exact, loss within 1e-4, and with the device's ReLU decisions replayed EVERY gradient tensor
within 1e-4."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import refimpl as R
from tests import featnone_util as U
from tests import golden_util as gu
from tests import x3_emul as X
from tests.test_parity_gpu import CLEAN_MIN, GOLDEN_BAND, RTOL, _rel_errs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}          # case -> kernel error / bound (printed by the last kernel test)


def _lib():
    import mtl_amd
    return mtl_amd._lib.lib(), torch.cuda.current_stream().cuda_stream


def _fwd(inp, shape, tasks, own_x, bias):
    """two launches of the forward on the first `tasks` tasks of inp -> (tasks, B T, N), asserted bit-identical"""
    lib, st = _lib()
    B, Fq, T, N = shape
    x = inp['x'][:tasks if own_x else 1].cuda().contiguous()
    theta = torch.cat([inp['w'][:tasks].reshape(tasks, -1), inp['bias'][:tasks]], 1).cuda().contiguous()      # a parameter stack: w, bias at one stride
    sW = theta.stride(0) if tasks > 1 else 0
    outs = []
    for _ in range(2):
        y = torch.full((tasks, B * T, N), float('nan'), device='cuda')
        rc = lib.mtl_featproj_fwd_tb(st, x.data_ptr(), theta.data_ptr(), theta.data_ptr() + 4 * N * Fq if bias else None, y.data_ptr(),
                                     B, Fq, T, N, tasks, B * Fq * T if own_x and tasks > 1 else 0, sW, B * T * N)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def _wgrad(inp, shape, tasks, own_x, first=0, prefill=True):
    """two launches of the weight gradient on tasks first .. first + tasks - 1 -> (tasks, N, F) accumulated onto dw0, bit-identical"""
    lib, st = _lib()
    B, Fq, T, N = shape
    x = inp['x'][first:first + tasks if own_x else first + 1].cuda().contiguous()
    dy = inp['dy'][first:first + tasks].cuda().contiguous()
    need = lib.mtl_featproj_wgrad_workspace(B, Fq, T, N, tasks)
    assert need > 0
    ws = torch.empty(need // 4 + 16, device='cuda')
    sG = N * Fq + 12                                   # a gradient stack with other tensors between the tasks' slices
    outs = []
    for _ in range(2):
        G = torch.zeros(tasks, sG, device='cuda')
        if prefill:
            G[:, :N * Fq] = inp['dw0'][first:first + tasks].reshape(tasks, -1).cuda()
        ws.fill_(float('nan'))
        rc = lib.mtl_featproj_wgrad_tb(st, x.data_ptr(), dy.data_ptr(), G.data_ptr(), ws.data_ptr(), need, B, Fq, T, N, tasks,
                                       B * Fq * T if own_x and tasks > 1 else 0, B * T * N, sG)
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((G[:, N * Fq:] == 0).all()), 'wrote between the tasks\' slices'
        outs.append(G[:, :N * Fq].reshape(tasks, N, Fq).cpu())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', U.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_kernel_against_fp64(shape, bias):
    """1 task; 3 tasks on a weight stack with one shared batch (sX = 0) and with their own batches"""
    inp = U.kernel_inputs(shape)
    for tasks, own_x in ((1, True), (U.TASKS, False), (U.TASKS, True)):
        y = _fwd(inp, shape, tasks, own_x, bias)
        for t in range(tasks):
            xt = t if own_x else 0
            rep = U.fwd_report(shape, t, bias, False, xt)
            err = X.rel(y[t], U.fwd_reference(inp, t, bias, xt))
            WORST['fwd %s tasks %d own_x %d bias %d' % (shape, tasks, own_x, bias)] = err / rep['bound']
            print('fwd %s tasks %d/%d own_x %d bias %d: %.3e (bound %.3e)' % (shape, t, tasks, own_x, bias, err, rep['bound']))
            X.check({'y': err}, rep['bound'], 'featproj fwd %s task %d' % (shape, t))


@pytest.mark.parametrize('shape', U.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_kernel_against_fp64(shape):
    """accumulation onto a pre-filled gradient; B T = 126, 130, 3 rows (one slice) and 514 (three); the 3-task launch equals three
    1-task launches bit for bit"""
    inp = U.kernel_inputs(shape)
    assert (shape[0] * shape[2] > 256) == (shape == U.SHAPES[3])          # row counts on both sides of the grid split
    for own_x in (False, True):
        dw = _wgrad(inp, shape, U.TASKS, own_x)
        for t in range(U.TASKS):
            xt = t if own_x else 0
            rep = U.wgrad_report(shape, t, False, xt)
            err = X.rel(dw[t], U.wgrad_reference(inp, t, xt))
            WORST['wgrad %s own_x %d' % (shape, own_x)] = max(WORST.get('wgrad %s own_x %d' % (shape, own_x), 0.0), err / rep['bound'])
            print('wgrad %s task %d own_x %d: %.3e (bound %.3e)' % (shape, t, own_x, err, rep['bound']))
            X.check({'dw': err}, rep['bound'], 'featproj wgrad %s task %d' % (shape, t))
            if own_x:
                assert torch.equal(_wgrad(inp, shape, 1, True, first=t)[0], dw[t]), 'task %d of the 3-task launch differs from its own launch' % t


def test_probe_cases_and_worst_errors():
    """a constant leading piece along the contraction index against an antisymmetric partner: a dropped second-order term weighs
    2^-9 of the result"""
    inp = U.probe_inputs('fwd')
    rep = U.fwd_report(U.FWD_PROBE, probe=True)
    err = X.rel(_fwd(inp, U.FWD_PROBE, 1, True, False)[0], U.fwd_reference(inp, 0, False))
    WORST['fwd probe'] = err / rep['bound']
    X.check({'y': err}, rep['bound'], 'featproj fwd probe')
    inp = U.probe_inputs('wgrad')
    rep = U.wgrad_report(U.WG_PROBE, probe=True)
    err = X.rel(_wgrad(inp, U.WG_PROBE, 1, True, prefill=False)[0], U.wgrad_reference(inp, 0, prefilled=False))
    WORST['wgrad probe'] = err / rep['bound']
    X.check({'dw': err}, rep['bound'], 'featproj wgrad probe')
    for k in sorted(WORST):
        print('worst error / bound  %-60s %.3f' % (k, WORST[k]))


# ------------------------------------------------------------------------------------------------------------------ the model
def make(fz=False, cfg_over=None, **over):
    import mtl_amd
    if fz:
        z, cfg, spec, d_in = U.load_fz()
        over = dict(dict(dim_input=d_in, is_factorized=True), **over)
    else:
        (z, cfg, spec), d_in = gu.load('N0'), 161
    cfg = dict(cfg, **(cfg_over or {}))
    model, vocab, args = U.device_model(cfg, spec, **over)
    model = model.cuda()
    assert all(e.conv_layers is None and e.time_shift == 0 for e in model.engines)
    return mtl_amd, z, cfg, spec, args, vocab, model, d_in


def _pass_parity(model, oracle, batch, theta, what, loss_fn=None, **fwd_kw):
    """tests/test_parity_gpu.py:_pass_parity for a model whose only branch points are the feed-forward ReLUs: labels bit-exact, logits,
    loss; with the device's decisions replayed EVERY gradient tensor within 1e-4"""
    x, lens, y = batch
    U.set_params(oracle, model, theta)
    out = model.pass_forward(x.cuda(), lens, y, theta=theta, **fwd_kw)
    g = torch.zeros_like(model.flat_grad)
    model.pass_backward(g, 1.0)
    gates = U.ffn_gates(model.engine)
    with torch.no_grad():
        pred_r, gold_r, hyp_r = oracle(x, lens, y)
    assert torch.equal(out['hyp'].cpu(), hyp_r) and torch.equal(out['gold'].cpu(), gold_r), what
    assert float((out['pred'].cpu() - pred_r).norm() / pred_r.norm()) < 1e-5, what
    flips = sum(int(((pre > 0) != gates[k]).sum()) for k, pre in _ffn_pre(oracle, x, lens, y).items())
    assert flips <= 8, (what, flips)
    pred_g, gold_g, _ = oracle(x, lens, y, gates=gates)
    loss_g = (loss_fn or R.ce_loss)(pred_g, gold_g)
    assert abs(float(out['loss']) - float(loss_g.detach())) < RTOL * float(loss_g.detach()), what
    grads = torch.autograd.grad(loss_g, list(oracle.parameters()))
    errs = _rel_errs(model, g, oracle, grads)
    worst = max(errs, key=errs.get)
    print('%s: %d near-ties decided differently; %d/%d gradient tensors within 1e-4, worst %.2e (%s)'
          % (what, flips, sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (what, worst, errs[worst], flips)
    return g, out


def _ffn_pre(oracle, x, lens, y):
    """the free-running restatement's feed-forward pre-activations, keyed like the engine's arena"""
    pre, hooks = {}, []
    ffns = [('e%d' % i, l.pos_ffn) for i, l in enumerate(oracle.encoder.layers)] + [('d%d' % i, l.pos_ffn) for i, l in enumerate(oracle.decoder.layers)]
    for tag, f in ffns:
        hooks.append(f.linear_1.register_forward_hook(lambda m, i, o, k=tag: pre.__setitem__(k + '.ff.h1', o.detach().reshape(-1, o.shape[-1]))))
    with torch.no_grad():
        oracle(x, lens, y)
    for h in hooks:
        h.remove()
    return pre


def test_drop_in_forward_against_the_golden():
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    (x, lens, y) = U.batches(cfg, spec, 0, z['data_call_index'])[0][0]
    pred, gold, hyp = model(x.cuda(), lens, y)
    loss, _ = mtl_amd.calculate_metrics(pred, gold, 0, smoothing=0.0, loss_type='ce')
    assert np.array_equal(hyp.cpu().numpy(), z['fwd/0/0/hyp']) and np.array_equal(gold.cpu().numpy(), z['fwd/0/0/gold'])
    ref = float(z['fwd/0/0/loss'])
    assert abs(float(loss.detach()) - ref) <= RTOL * ref
    gu.check_digest(z, 'fwd/0/0', 'pred', pred, rtol=1e-5, what='N0')
    assert lens.tolist()[-1] < spec['T'] and model.engine.encoder_output().shape == (spec['k'], spec['T'], cfg['dim_model'])
    mem = model.engine.encoder_output()
    assert not bool(mem[-1, int(lens[-1]):].any()) and bool(mem[-1, :int(lens[-1])].any())          # frames are positions: real padding is zeroed


@pytest.mark.parametrize('fz', [False, True], ids=['dense', 'factorized'])
def test_every_pass_of_a_meta_step_against_live_restatement(fz):
    mtl_amd, z, cfg, spec, args, vocab, model, d_in = make(fz)
    oracle = U.build_model(cfg, d_in, fz)
    tr, val = U.batches(cfg, spec, 0, z['data_call_index'], d_in)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    for m, batch in enumerate(tr):
        g_tr, _ = _pass_parity(model, oracle, batch, model.flat_parameters, 'N0 task %d train' % m)
        assert model.engine.saved['conv_mode'] == 'x3' and model.engine.saved['in_h2'] is False
        theta1 = inner.theta_prime_from(model.flat_parameters, g_tr).clone()
        _pass_parity(model, oracle, val, theta1, 'N0 task %d valid' % m)


def _train_one(mtl_amd, model, vocab, args, trainer, tasks, it, loss='ce'):
    captured = {}
    orig = trainer.meta_iteration

    def spy(*a, **kw):
        captured['reads'] = orig(*a, **kw)
        return captured['reads']
    trainer.meta_iteration = spy
    with U.capture_ffn_gates(model) as log:
        trainer.train(model, vocab, tasks, [], loss, it, it + 1, args, inner_opt=getattr(trainer, 'inner_opt', None),
                      outer_opt=getattr(trainer, 'outer_opt', None), evaluate_every=10 ** 9, early_stop='cer,200', is_copy_grad=True)
        torch.cuda.synchronize()
    trainer.meta_iteration = orig
    return captured['reads'], log


@pytest.mark.parametrize('fz,batched', [(False, False), (False, True), (True, False), (True, True)],
                         ids=['lanes', 'batched', 'factorized-lanes', 'factorized-batched'])
def test_meta_steps_against_the_golden_and_the_live_restatement(fz, batched):
    """labels, losses, G and theta against N0.npz in the bands tests/test_parity_gpu.py applies to F0 (its CLEAN_MIN as the same share
    of this model's tensors); and G of every step, every tensor, within 1e-4 of the live restatement started from the device's own
    parameters with the device's ReLU decisions replayed"""
    mtl_amd, z, cfg, spec, args, vocab, model, d_in = make(fz)
    names = [str(s) for s in z['param_names']]
    n = spec['n_tasks']
    tasks = [U.Task(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], spec['variable'], d_in) for m in range(n)]
    trainer = mtl_amd.TransientTrainer()
    trainer.batch_tasks = batched
    oracle = U.build_model(cfg, d_in, fz)
    clean_min = CLEAN_MIN['F0'] * len(names) // 68
    for it in range(spec['iters']):
        theta_in = model.flat_parameters.clone()
        reads, log = _train_one(mtl_amd, model, vocab, args, trainer, tasks, it)
        assert trainer.last_schedule == ('batched' if batched else 'lanes') and len(log) == 2 * n
        for m, (tr, va) in enumerate(reads):
            for j, rd in ((2 * m, tr), (2 * m + 1, va)):
                key = 'fwd/%d/%d' % (it, j)
                assert np.array_equal(rd.gold_host.numpy(), z[key + '/gold']) and np.array_equal(rd.hyp.numpy(), z[key + '/hyp']), key
                ref = float(z[key + '/loss'])
                assert abs(float(rd.loss[0]) - ref) <= RTOL * abs(ref), key
        floor = 1e-4 * gu.global_l2(z, 'G/%d' % it, names)
        errs = [gu.check_digest(z, 'G/%d' % it, nm, model._layout.view(model._G, nm), rtol=GOLDEN_BAND['F0'], what='N0', floor=floor) for nm in names]
        clean = sum(e <= RTOL for e in errs)
        print('N0 it %d: %d/%d meta-gradient tensors within 1e-4 of the golden, worst %.3e' % (it, clean, len(errs), max(errs)))
        if it == 0:
            assert clean >= clean_min, (clean, len(errs))
        for (nm, p), e in zip(model.named_parameters(), errs):
            if float(z['G/%d/%s/l2' % (it, nm)]) < floor * 1e-2:
                continue
            gu.check_digest(z, 'theta/%d' % (it + 1), nm, p, rtol=RTOL if e <= RTOL / 10 else GOLDEN_BAND['F0'], what='N0')
        U.set_params(oracle, model, theta_in)
        tr_b, val_b = U.batches(cfg, spec, it, z['data_call_index'], d_in)
        G_r, _, _, _ = R.meta_gradient(oracle, tr_b, val_b, spec['lr'], gates=log)
        live = _rel_errs(model, model._G, oracle, G_r)
        worst = max(live, key=live.get)
        print('N0 it %d against the live restatement: worst %.2e (%s)' % (it, live[worst], worst))
        assert live[worst] < RTOL, (it, worst, live[worst])


def test_long_masked_tails_and_several_key_blocks():
    """T 300 with lengths [300, 37]: 263 masked keys and zeroed rows in one utterance, several attention key blocks in the other"""
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 1, 161, 300, generator=g)
    x[1, :, :, 37:] = 0
    lens = torch.tensor([300, 37], dtype=torch.int32)
    y = torch.randint(4, cfg['vocab_size'], (2, 8), generator=g)
    y[1, 5:] = 0
    _, out = _pass_parity(model, U.build_model(cfg), (x, lens, y), model.flat_parameters, 'N0 T300')
    mem = model.engine.encoder_output()
    assert mem.shape[1] == 300 and not bool(mem[1, 37:].any())
    with pytest.raises(ValueError, match='positional'):
        model.pass_forward(torch.zeros(1, 1, 161, cfg['src_max_len'] + 1).cuda(), torch.tensor([5], dtype=torch.int32), y[:1])


def _ctc_loss_of_full_rows(pred, gold):
    """utils/metrics.py:127-148 for batches whose utterances fill the frame axis (percentages 1): every decoder position is an input
    row, the targets are the labels in front of the EOS"""
    import torch.nn.functional as F
    B, Td = pred.shape[0], pred.shape[1]
    return F.ctc_loss(F.log_softmax(pred, 2).transpose(0, 1), gold, torch.full((B,), Td, dtype=torch.long), (gold != 0).sum(1) - 1, blank=0,
                      reduction='mean')


def test_ctc_pass_against_live_restatement():
    """one pass with the CTC loss stage against torch's ctc_loss on the fp64 restatement: decisions replayed, every tensor within 1e-4"""
    import torch.nn.functional as F
    from tests.test_ctc_train_gpu import _no_adjacent_repeats
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    x, lens, y = R.synth_batch(41, spec['k'], spec['T'], 8, cfg['vocab_size'], False)
    y = _no_adjacent_repeats(y)
    pct, tl = lens.float() / x.shape[3], (y != 0).sum(1).to(torch.int32)
    in_len = mtl_amd.engine.ctc_input_lengths(pct.numpy(), 9)

    def ctc(pred, gold):
        return F.ctc_loss(F.log_softmax(pred, 2).transpose(0, 1), gold, torch.from_numpy(in_len).long(), tl.long(), blank=0, reduction='mean')
    oracle = U.build_model(cfg).double()
    _pass_parity(model, oracle, (x.double(), lens, y), model.flat_parameters, 'N0 ctc', loss_fn=ctc, loss_type='ctc', percentages=pct, target_sizes=tl)


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'lanes'])
def test_ctc_meta_step_against_live_restatement(batched, monkeypatch):
    """one --loss ctc meta-step (training passes at theta0, validation passes at each task's theta' -- the weight stack of the
    task-batched schedule) against oracle/refimpl.py's meta_gradient on the fp64 restatement with torch's ctc_loss in the place of its
    cross entropy and the device's ReLU decisions replayed: losses, and every tensor of G within 1e-4"""
    from tests.test_ctc_train_gpu import _no_adjacent_repeats
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    n, k, V = spec['n_tasks'], spec['k'], cfg['vocab_size']
    mk = lambda seed: (lambda b: (b[0], b[1], _no_adjacent_repeats(b[2])))(R.synth_batch(seed, k, spec['T'], 8, V, False))
    tr_b, val_b = [mk(700 + m) for m in range(n)], mk(799)
    as5 = lambda b: (b[0], b[1], b[1].float() / b[0].shape[3], b[2], (b[2] != 0).sum(1).to(torch.int32))
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    trainer = mtl_amd.TransientTrainer()
    trainer.batch_tasks = batched
    with U.capture_ffn_gates(model) as log:
        reads = trainer.meta_iteration(model, vocab, [as5(b) for b in tr_b], as5(val_b), n, inner, None, args, loss_type='ctc')
        torch.cuda.synchronize()
    assert trainer.last_schedule == ('batched' if batched else 'lanes') and len(log) == 2 * n
    oracle = U.build_model(cfg).double()
    U.set_params(oracle, model, model.flat_parameters)
    monkeypatch.setattr(R, 'ce_loss', _ctc_loss_of_full_rows)
    dbl = lambda b: (b[0].double(), b[1], b[2])
    G_r, trl, val_l, labels = R.meta_gradient(oracle, [dbl(b) for b in tr_b], dbl(val_b), spec['lr'], gates=log)
    for m, (rd_tr, rd_va) in enumerate(reads):
        for rd, (gold, hyp), loss in ((rd_tr, labels[2 * m], trl[m]), (rd_va, labels[2 * m + 1], val_l[m])):
            assert torch.equal(rd.hyp, hyp) and torch.equal(rd.gold_host, gold)
            assert np.isfinite(loss) and abs(float(rd.loss[0]) - loss) < RTOL * loss, (m, float(rd.loss[0]), loss)
    errs = _rel_errs(model, model._G, oracle, G_r)
    worst = max(errs, key=errs.get)
    print('N0 ctc meta-step (%s): %d/%d tensors within 1e-4, worst %.2e (%s)' % (trainer.last_schedule, sum(e < RTOL for e in errs.values()),
                                                                                len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (worst, errs[worst])


def test_clip_meta_step_against_live_restatement():
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    args.clip, args.max_norm = True, 3.0
    oracle = U.build_model(cfg)
    tr, val = U.batches(cfg, spec, 0, z['data_call_index'])
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    as5 = lambda b: (b[0], b[1], None, b[2], None)
    with U.capture_ffn_gates(model) as log:
        mtl_amd.TransientTrainer().meta_iteration(model, vocab, [as5(b) for b in tr], as5(val), len(tr), inner, None, args)
        torch.cuda.synchronize()
    G_r, _, _, _ = R.meta_gradient(oracle, tr, val, spec['lr'], max_norm=3.0, gates=log)
    errs = _rel_errs(model, model._G, oracle, G_r)
    assert max(errs.values()) < RTOL, max(errs.items(), key=lambda kv: kv[1])


def _crop(g, k, frames, dec_width):
    """feed-forward decisions of one task of a stacked pass -> the rows of its own pass (every frame an encoder position)"""
    return {key: v.view(k, -1, v.shape[-1])[:, :frames if key.startswith('e') else dec_width].reshape(-1, v.shape[-1]) for key, v in g.items()}


def test_tasks_of_widths_63_40_24_stacked_at_63_against_their_own_passes():
    """tests/test_batched_gpu.py:test_tasks_of_different_frame_counts_in_one_pass_against_live_oracle for frames that are positions: the
    stacked pass against the restatement run task by task at each task's own width, the device's decisions (cropped to the task's own
    extent) replayed: labels bit-exact, losses and every tensor of G within 1e-4"""
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    oracle = U.build_model(cfg)
    k, V = spec['k'], cfg['vocab_size']
    frames, widths, val_frames = (63, 40, 24), (8, 5, 11), 58
    cpu = [R.synth_batch(240 + m, k, T_m, L_m, V, True) for m, (T_m, L_m) in enumerate(zip(frames, widths))]
    val = R.synth_batch(299, k, val_frames, 6, V, True)
    as5 = lambda b: (b[0].cuda(), b[1], None, b[2], None)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    tr = mtl_amd.TransientTrainer()
    tr.ragged_quantum, tr.ragged_fill = 1, 0.0
    with U.capture_ffn_gates(model) as log:
        reads = tr.meta_iteration(model, vocab, [as5(b) for b in cpu], as5(val), 3, inner, None, args)
        torch.cuda.synchronize()
    assert tr.last_schedule == 'batched-ragged' and len(log) == 6
    assert model.engines[0].saved is not None
    gates = [_crop(g, k, val_frames if i % 2 else frames[i // 2], 7 if i % 2 else widths[i // 2] + 1) for i, g in enumerate(log)]
    G, trl, val_l, labels = R.meta_gradient(oracle, cpu, val, spec['lr'], gates=gates)
    for t in range(3):
        for rd, (gold, hyp), loss in ((reads[t][0], labels[2 * t], trl[t]), (reads[t][1], labels[2 * t + 1], val_l[t])):
            w = gold.shape[1]
            assert torch.equal(rd.hyp[:, :w], hyp) and torch.equal(rd.gold_host[:, :w], gold)
            assert abs(float(rd.loss[0]) - loss) < RTOL * loss
    errs = _rel_errs(model, model._G, oracle, G)
    worst = max(errs, key=errs.get)
    print('stacked 63 / 40 / 24 vs own passes: %d/%d tensors within 1e-4, worst %.2e (%s)' % (sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (worst, errs[worst])


def test_joint_trainer_against_the_golden_trace():
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    js = json.loads(bytes(z['joint/spec']).decode())
    args.lr, args.k_train, args.loss = js['lr'], js['k'], 'ce'
    tasks = [U.Task(m, js['k'], js['T'], js['L'], cfg['vocab_size'], True) for m in range(js['n_tasks'])]
    tr = mtl_amd.JointTrainer()
    tr.train(model, vocab, tasks, [], 'ce', 0, js['iters'], args, evaluate_every=10 ** 9, early_stop='cer,200')
    for it in range(js['iters']):
        ref = float(z['joint/losses'][it].mean())
        assert abs(tr.loss_trace[it] - ref) <= RTOL * ref, (it, tr.loss_trace[it], ref)


def test_joint_iteration_with_the_discriminator_against_live_restatement():
    """one JointTrainer iteration with the accent discriminator (--adversarial: weight 1/2 on its CE, the MSE to the uniform
    distribution as the encoder loss) on an encoder output of B x T x d with real padding, against the step written in torch on the
    restatement: the head of tests/disc_util.py (the sum over ALL T rows, masked rows being zero) on the restatement's encoder output,
    (tr + w ce + mse) / n back through both by autograd, the device's ReLU decisions replayed.  Per task the three losses; the
    discriminator's gradient and every tensor of the model's G within 1e-4."""
    from tests import disc_util as du
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    js = json.loads(bytes(z['joint/spec']).decode())
    n, C, w = js['n_tasks'], js['n_tasks'], 0.5
    args.lr, args.k_train, args.num_class, args.lr_disc, args.loss = js['lr'], js['k'], C, 1e-3, 'ce'
    for k_, v in du.mode_flags('adversarial').items():
        setattr(args, k_, v)
    torch.manual_seed(99)
    disc = mtl_amd.init_discriminator_model(args)
    W0, b0 = disc.linear.weight.detach().clone(), disc.linear.bias.detach().clone()
    disc = disc.cuda()
    theta0 = model.flat_parameters.clone()
    tasks = [U.Task(m, js['k'], js['T'], js['L'], cfg['vocab_size'], True) for m in range(n)]
    tr = mtl_amd.JointTrainer()
    got, orig = {}, tr.run_iteration

    def spy(model_, vocab_, batches, n_, opt, a, **kw):
        od, step, dstep = kw['opt_disc'], opt.step, kw['opt_disc'].step
        opt.step = lambda g: (got.__setitem__('G', g.clone()), step(g))[1]
        od.step = lambda: (got.__setitem__('dG', disc.flat_grad.clone()), dstep())[1]
        try:
            return orig(model_, vocab_, batches, n_, opt, a, **kw)
        finally:
            opt.step, od.step = step, dstep
    tr.run_iteration = spy
    with U.capture_ffn_gates(model) as log:
        tr.train(model, vocab, tasks, [], 'ce', 0, 1, args, evaluate_every=10 ** 9, early_stop='cer,200', discriminator=disc)
        torch.cuda.synchronize()
    assert len(log) == n and len(tr.task_losses) == n
    oracle = U.build_model(cfg)
    U.set_params(oracle, model, theta0)
    Wd, bd = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    params = list(oracle.parameters())
    G = [torch.zeros_like(p) for p in params]
    dW, db = torch.zeros_like(Wd), torch.zeros_like(bd)
    for m in range(n):
        x, lens, y = R.synth_batch(10 * m, js['k'], js['T'], js['L'], cfg['vocab_size'], True)
        assert int(lens.min()) < js['T']                                         # (real padding: zeroed rows inside the time sum)
        feats = x.reshape(x.shape[0], x.shape[2], x.shape[3]).transpose(1, 2).contiguous()
        mem = oracle.encoder(feats, lens, None, log[m])
        pred, gold = oracle.decoder(y, mem, lens, None, log[m])
        logits = mem.sum(dim=1) @ Wd.t() + bd
        ce = torch.nn.functional.cross_entropy(logits, torch.full((logits.shape[0],), m, dtype=torch.long))
        mse = ((logits - 1.0 / C) ** 2).mean()
        t_loss = R.ce_loss(pred, gold)
        _, ce64, mse64 = du.head(du.pool(mem.detach()), W0, b0, m, 1)             # the specification's fp64 form of the same head
        assert abs(float(ce) - float(ce64)) < 1e-5 * float(ce64) and abs(float(mse) - float(mse64)) < 1e-5 * float(mse64)
        t_dev, d_dev, e_dev = tr.task_losses[m]
        print('task %d: tr %.6f vs %.6f  disc %.6e vs %.6e  enc %.6e vs %.6e' % (m, t_dev, float(t_loss), d_dev, float(ce64), e_dev, float(mse64)))
        assert abs(t_dev - float(t_loss)) <= RTOL * float(t_loss)
        assert abs(d_dev - float(ce64)) <= du.ce_tolerance(float(ce64), logits.detach().numpy(), m, RTOL, RTOL)
        assert abs(e_dev - float(mse64)) <= RTOL * float(mse64)
        grads = torch.autograd.grad((t_loss + w * ce + mse) / n, params + [Wd, bd])
        for acc, g_ in zip(G, grads[:-2]):
            acc.add_(g_)
        dW.add_(grads[-2])
        db.add_(grads[-1])
    d = cfg['dim_model']
    for nm, ref, lo, hi in (('linear.weight', dW, 0, C * d), ('linear.bias', db, C * d, C * d + C)):
        err = float((got['dG'][lo:hi].cpu() - ref.reshape(-1)).norm() / ref.norm())
        print('discriminator gradient %s rel err %.3e' % (nm, err))
        assert err <= RTOL, (nm, err)
    errs = _rel_errs(model, got['G'], oracle, G)
    worst = max(errs, key=errs.get)
    print('joint + discriminator: %d/%d model gradient tensors within 1e-4, worst %.2e (%s)' % (sum(e < RTOL for e in errs.values()), len(errs),
                                                                                               errs[worst], worst))
    assert errs[worst] < RTOL, (worst, errs[worst])


def _decode_setup(tgt_max_len=None):
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make(cfg_over=dict(tgt_max_len=tgt_max_len) if tgt_max_len else None)
    sp = json.loads(bytes(z['decode/spec']).decode())
    model = model.cpu()
    gu.perturb_output_layer(model.decoder.output_linear.weight, sp)
    model = model.cuda()
    x, lens, y = R.synth_batch(sp['seed'], sp['k'], sp['T'], sp['L'], cfg['vocab_size'], True)
    return mtl_amd, z, cfg, spec, args, vocab, model, sp, (x, lens, y)


def _beam_ids(model, args, sp, batch, device_ranking):
    x, lens, y = batch
    args.beam_width, args.beam_nbest = sp['beam_width'], sp['nbest']
    model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=1, device_ranking=device_ranking)
    return [list(map(int, s)) for s in model.last_beam_ids]


def test_greedy_and_beam_tokens_equal_the_golden():
    mtl_amd, z, cfg, spec, args, vocab, model, sp, batch = _decode_setup()
    want = [[int(v) for v in r_ if v >= 0] for r_ in z['decode/beam_ids']]
    for ranking in (False, True):
        assert _beam_ids(model, args, sp, batch, ranking) == want, ranking
    x, lens, y = batch
    model.evaluate(x.cuda(), lens, y, args, beam_search=False, start_token=1, max_steps=sp['greedy_steps'])
    assert np.array_equal(model.last_greedy_ids.numpy()[:sp['greedy_steps']], z['decode/greedy_ids'])


def test_checkpoint_round_trip_and_the_references_checkpoint(tmp_path):
    mtl_amd, z, cfg, spec, args, vocab, model, sp, batch = _decode_setup()
    args.save_folder, args.name = str(tmp_path), 'rt'
    inner, outer = torch.optim.SGD(model.parameters(), lr=args.lr), torch.optim.Adam(model.parameters(), lr=args.meta_lr)
    path = mtl_amd.save_meta_model(model, vocab, 3, inner, outer, {'avg_valid_cer': 1.0}, args)
    m2, vocab2, _, _, epoch, _, args2 = mtl_amd.load_meta_model(path)
    assert epoch == 3 and args2.feat_extractor == 'none' and args2.dim_input == 161 and m2.feat_extractor == 'none'
    assert m2.flat_parameters.is_cuda and torch.equal(m2.flat_parameters, model.flat_parameters)
    assert _beam_ids(m2, args, sp, batch, True) == _beam_ids(model, args, sp, batch, True)
    # N0.th.gz: written by the reference's own save_meta_model
    raw = tmp_path / 'N0.th'
    with gzip.open(os.path.join(ROOT, 'tests', 'golden', 'N0.th.gz'), 'rb') as f, open(raw, 'wb') as g:
        shutil.copyfileobj(f, g)
    m3, vocab3, _, outer3, epoch3, metrics3, args3 = mtl_amd.load_meta_model(str(raw))
    assert epoch3 == 4 and args3.feat_extractor == 'none' and args3.dim_input == 21 and not hasattr(m3, 'conv')
    assert tuple(m3.encoder.input_linear.weight.shape) == (64, 21) and len(outer3.state) == len(list(m3.parameters()))
    # ... and it computes what the reference's model computed: the logits of a teacher-forced pass on the recorded batch
    cs = json.loads(bytes(z['ckpt/spec']).decode())
    m3 = m3.cuda()
    g = torch.Generator().manual_seed(cs['seed'])
    x = torch.randn(cs['k'], 1, cs['F'], cs['T'], generator=g)
    y = torch.randint(4, 64, (cs['k'], cs['L']), generator=g)
    lens = torch.tensor(cs['lens'], dtype=torch.int32)
    m3.eval()
    out = m3.pass_forward(x.cuda(), lens, y)
    ref = torch.from_numpy(z['ckpt/pred'])
    err = float((out['pred'].cpu() - ref).norm() / ref.norm())
    print('N0.th.gz: pred against the reference\'s: %.2e' % err)
    assert err < 1e-5
    top2 = ref.topk(2, dim=2).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-3 * ref.abs().max()              # labels whose margin is not rounding (patterned weights)
    assert np.array_equal(out['hyp'].cpu().numpy()[clear.numpy()], z['ckpt/hyp'][clear.numpy()])


def _manifest(tmp_path, z):
    """tests/golden/N0_manifest/ with its rows made absolute (a manifest names files by path), and the feature function that stands for
    the audio front-end: utterance I's features are the fixture's seeded batch"""
    sp = json.loads(bytes(z['manifest/spec']).decode())
    src = os.path.join(ROOT, 'tests', 'golden', 'N0_manifest')
    rows = [ln.split(',') for ln in open(os.path.join(src, 'test.csv')).read().split()]
    mp = tmp_path / 'test.csv'
    mp.write_text('\n'.join('%s,%s' % (tmp_path / w, os.path.join(src, t)) for w, t in rows) + '\n')
    utt = [R.synth_batch(seed, 1, T, L, 64, False) for seed, T, L in zip(sp['seeds'], sp['T'], sp['L'])]
    feats = lambda wav: utt[int(os.path.basename(wav)[1])][0][0, 0].clone()
    return sp, str(mp), utt, feats


def _dataset_args(manifest, k=2):
    import argparse
    a = argparse.Namespace(src_max_len=500, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', augment=False, input_type='char',
                           train_manifest_list=[manifest], train_partition_list=[1.0], k_train=k, noise_dir=None, noise_prob=0.4, noise_min=0.0,
                           noise_max=0.5)
    conf = dict(sample_rate=a.sample_rate, window_size=a.window_size, window_stride=a.window_stride, window=a.window, noise_dir=None,
                noise_prob=a.noise_prob, noise_levels=(a.noise_min, a.noise_max))
    return a, conf


def test_evaluate_test_set_on_the_two_utterance_manifest(tmp_path):
    """test.py's loop fed by SpectrogramDataset + AudioDataLoader over the manifest fixture, one utterance per batch (63 and 41 frames of
    161 features: every batch its own width): the hypotheses of BOTH utterances are the reference's, the totals those of its strings"""
    import argparse
    mtl_amd, z, cfg, spec, args, vocab, model, dsp, _ = _decode_setup()
    sp, manifest, utt, feats = _manifest(tmp_path, z)
    da, conf = _dataset_args(manifest)
    ds = mtl_amd.SpectrogramDataset(vocab, da, conf, manifest_filepath_list=[manifest], normalize=True, input_type='char', feature_fn=feats)
    assert len(ds) == 2 and tuple(ds[1][0].shape) == (161, sp['T'][1]) and ds[1][1] == [int(t) for t in utt[1][2][0]]
    loader = mtl_amd.AudioDataLoader(vocab.PAD_ID, dataset=ds, batch_size=1)
    ev = argparse.Namespace(beam_search=True, lm_rescoring=False, beam_width=sp['beam_width'], beam_nbest=sp['nbest'], lm_weight=0.0, c_weight=1.0,
                            verbose=False, tgt_max_len=cfg['tgt_max_len'], cuda=True)
    seen = []
    out = mtl_amd.evaluate_test_set(model, vocab, loader, ev, start_token=1, on_batch=lambda t: seen.append([list(map(int, s_)) for s_ in model.last_beam_ids]))
    want = [[int(v) for v in r_ if v >= 0] for r_ in z['manifest/beam_ids']]
    assert seen == [[want[0]], [want[1]]]
    cer = wer = chars = 0
    for ids, (_, _, y) in zip(want, utt):
        hyp = mtl_amd.post_process(model._post_process_hyp(ids), vocab.special_token_list)
        gold = mtl_amd.post_process(''.join(vocab.id2label[int(t)] for t in y[0]) + vocab.EOS_TOKEN, vocab.special_token_list)
        cer, wer, chars = cer + mtl_amd.calculate_cer(hyp.strip(), gold.strip()), wer + mtl_amd.calculate_wer(hyp, gold), chars + len(gold)
    assert (out['total_cer'], out['total_wer'], out['total_char']) == (cer, wer, chars) and out['line'].startswith('TEST CER:')


def test_meta_step_fed_by_manifest_datasets_of_different_widths(tmp_path):
    """TransientTrainer.train on two SpectrogramDataset tasks over the manifest fixture (utterances of 63 and 41 frames drawn with
    replacement, every batch padded to its own longest): the batches the datasets handed out, run task by task through the
    restatement with the device's decisions (cropped to each batch's own extent) replayed -- every tensor of G within 1e-4"""
    mtl_amd, z, cfg, spec, args, vocab, model, _ = make()
    sp, manifest, utt, feats = _manifest(tmp_path, z)
    da, conf = _dataset_args(manifest)
    k, handed = 2, []

    class Recording(mtl_amd.SpectrogramDataset):
        def sample(self, k_train, k_valid, manifest_id):
            out = super().sample(k_train, k_valid, manifest_id)
            handed.append((self, out))
            return out
    np.random.seed(4)                                           # (the datasets draw from the global RNG, as the reference's do)
    # (as the reference's entry script builds them: one dataset per training manifest, each over ALL manifests; task m samples manifest m)
    tasks = [Recording(vocab, da, conf, manifest_filepath_list=[manifest, manifest], normalize=True, input_type='char', is_train=True,
                       partitions=[1.0, 1.0], feature_fn=feats) for _ in range(2)]
    args.k_train = args.k_valid = k
    trainer = mtl_amd.TransientTrainer()
    _, log = _train_one(mtl_amd, model, vocab, args, trainer, tasks, 0)
    theta0 = U.build_model(cfg)                                 # (theta0 of the seeded build: the step started from it)
    used = [next(o for d_, o in handed if d_ is t_) for t_ in tasks]      # either task's first draw feeds iteration 0 (the next is prefetched)
    b3 = lambda b: (b[0], b[1], b[3])
    tr_b, val_b = [b3(u[0]) for u in used], b3(used[-1][1])
    widths = sorted({int(b[0].shape[3]) for b in tr_b + [val_b]})
    print('manifest-fed step: schedule %s, batch widths %s' % (trainer.last_schedule, [int(b[0].shape[3]) for b in tr_b + [val_b]]))
    assert len(log) == 4 and set(widths) <= set(sp['T'])
    dec = lambda y: int((y != 0).sum(1).max()) + 1
    gates = [_crop(g_, k, int((val_b if i % 2 else tr_b[i // 2])[0].shape[3]), dec((val_b if i % 2 else tr_b[i // 2])[2])) for i, g_ in enumerate(log)]
    G_r, _, _, _ = R.meta_gradient(theta0, tr_b, val_b, spec['lr'], gates=gates)
    errs = _rel_errs(model, model._G, theta0, G_r)
    worst = max(errs, key=errs.get)
    print('manifest-fed step: %d/%d tensors within 1e-4, worst %.2e (%s)' % (sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (worst, errs[worst])
