"""Whole-path parity on the MI355X, through the drop-in Python API over the C ABI:
  * against the committed goldens produced by the real reference (tests/golden/F0,F1,NS.npz);
  * against the CPU oracle run live on the same seeded inputs (full tensors, small sizes).
Bars (BASELINE.json north_star): label indices bit-exact; fp32 loss and meta-gradients within 1e-4 relative."""
import argparse
import hashlib

import numpy as np
import pytest
import torch

from tests import golden_util as gu

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # north_star: fp32 loss and meta-gradients within 1e-4 relative
# Against the reference GOLDENS the ReLU / max-pool decisions are frozen in the file: ~20 near-tie branch flips per north-star pass
# are expected between ANY two fp32 implementations (tests/test_oracle_golden.py: the CPU oracle itself reaches 148 / 176 tensors
# <= 1e-4 and all <= 1e-3 against NS.npz; two exact-fp32 convolution paths of the SAME oracle differ in 13 decisions and by 2.9e-4).
# The gates below are what this build MEASURES (deterministic: every kernel is bitwise reproducible), with the stated margins -- they
# move when a kernel's summation order changes (which near-ties flip), so a change of a kernel is expected to re-measure them:
#   measured, round 4 (sparse weight gradients, bf16-split attention):  F0 it 0: 67 / 68 clean, worst 1.9e-4; it 1: worst 3.7e-2
#                                                                       F1 it 0: 184 / 190 clean, worst 3.06e-3
#                                                                       NS it 0: 154 / 190 clean, worst 3.14e-4
# CLEAN_MIN: tensors within 1e-4 on the iteration that starts from bit-identical theta (measured minus a margin of ~10 %);
# GOLDEN_BAND: every tensor, every iteration (<= 2 x the measured worst; F0's second iteration -- zero-padded, variable lengths: a
# near-tie in the constant padded region flips a whole region after a 1e-3 Adam step -- 1.4 x).
# The 1e-4 bar on ALL tensors is asserted against the live oracle with the device path's own decisions replayed
# (test_single_pass_at_north_star_size_against_live_oracle, test_meta_gradient_at_north_star_size_with_branch_replay: 3 and 8 tasks).
#   measured, round 6:  T5 (T = 5000, B = 8, variable lengths, ONE task) it 0: 15 / 190 clean, worst 4.7e-3 (h2; 3.2e-3 with the exact x3
#                       operands): 62 near-ties (margin 1.9e-6) of ~1.25 G branch points fall the other way, each moving a tensor by
#                       ~1 / sqrt(its gradient's contributions); with the decisions replayed: 190 / 190 within 1e-4, worst 2.5e-5
#                       (test_long_utterance_full_batch_against_live_oracle); the CPU oracle itself meets T5.npz at 179 / 179, worst 3e-6
CLEAN_MIN = {'F0': 60, 'F1': 170, 'NS': 135, 'T5': 10}
GOLDEN_BAND = {'F0': 5e-2, 'F1': 6.2e-3, 'NS': 6.3e-4, 'T5': 9.5e-3}
NS_FLIP_BOUND = 120   # free-running ReLU / max-pool near-tie disagreements per north-star pass (measured ~25 of ~250 M branch points)


def make(cfg, spec, name='parity'):
    import mtl_amd
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
                              dropout=0.0, emb_trg_sharing=False, label_smoothing=0.0, name=name, lr=spec['lr'],
                              meta_lr=spec['meta_lr'], k_train=spec['k'], k_valid=spec['k'], clip=False, max_norm=400,
                              save_every=10 ** 9, save_folder='/tmp/mtl_ckpt', cuda=True,
                              **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    vocab = mtl_amd.synthetic_vocab(cfg['vocab_size'])
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    return mtl_amd, args, vocab, model


@pytest.mark.parametrize('name', ['F0', 'F1', 'NS', 'T5'])
def test_meta_iterations_match_reference_goldens(name):
    # (T5: BASELINE.json configs[3] at its FULL batch -- 8 utterances of up to 5000 frames, one task -- against the record the real
    # reference wrote, oracle/make_golden.py --t5000)
    z, cfg, spec = gu.load(name)
    mtl_amd, args, vocab, model = make(cfg, spec)
    names = [str(s) for s in z['param_names']]
    assert [n for n, _ in model.named_parameters()] == names
    h = hashlib.sha256()
    for _, p in model.named_parameters():
        h.update(p.detach().numpy().tobytes())
    assert h.hexdigest() == bytes(z['theta0_sha256']).decode()          # init draw order (Q4), bit-exact
    model = model.cuda()
    n = spec['n_tasks']
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=spec['variable'])
             for m in range(n)]
    trainer = mtl_amd.TransientTrainer()
    worst = 0.0
    for it in range(spec['iters']):
        captured = {}
        orig = trainer.meta_iteration

        def spy(*a, **kw):
            reads = orig(*a, **kw)
            captured['reads'] = reads
            return reads
        trainer.meta_iteration = spy
        trainer.train(model, vocab, tasks, [], 'ce', it, it + 1, args, inner_opt=getattr(trainer, 'inner_opt', None),
                      outer_opt=getattr(trainer, 'outer_opt', None), evaluate_every=10 ** 9, early_stop='cer,200',
                      is_copy_grad=True)
        trainer.meta_iteration = orig
        for m, (tr, va) in enumerate(captured['reads']):
            for j, rd in ((2 * m, tr), (2 * m + 1, va)):
                key = 'fwd/%d/%d' % (it, j)
                assert np.array_equal(rd.gold_host.numpy(), z[key + '/gold']), key
                assert np.array_equal(rd.hyp.numpy(), z[key + '/hyp']), key + ' hyp'        # label indices: bit-exact
                ref = float(z[key + '/loss'])
                assert abs(float(rd.loss[0]) - ref) <= RTOL * abs(ref), key
        floor = 1e-4 * gu.global_l2(z, 'G/%d' % it, names)
        errs = [gu.check_digest(z, 'G/%d' % it, nm, model._layout.view(model._G, nm), rtol=GOLDEN_BAND[name], what=name, floor=floor)
                for nm in names]
        worst = max(worst, max(errs))
        clean = sum(e <= RTOL for e in errs)
        print('%s it %d: %d/%d meta-gradient tensors within 1e-4, worst %.3e' % (name, it, clean, len(errs), max(errs)))
        # 1e-4 wherever no ReLU/max-pool branch flipped (oracle/branches.py); a flip moves single tensors into the band.  Counted
        # on the iteration that starts from bit-identical theta only: from the second iteration on theta already carries
        # Adam's lr*sign(g) response to the first iteration's rounding noise, and which near-ties flip depends on the
        # summation order of every kernel (fp32-MFMA and split-bf16 convolutions give 54 and 32 of 68 on F0) -- band only.
        if it == 0:
            assert clean >= CLEAN_MIN[name], (clean, len(errs))
        for (nm, p), e in zip(model.named_parameters(), errs):
            if float(z['G/%d/%s/l2' % (it, nm)]) < floor * 1e-2:
                continue        # Adam on an exactly-zero gradient: sign of rounding noise (see tests/test_oracle_golden.py)
            # Adam's first steps are ~ lr*sign(g): elements with |g| ~ eps inherit g's relative error one-for-one
            # (T5: zero-initialised LayerNorm / bias tensors move by -lr g / (|g| + eps) with |g| ~ eps = 1e-8: an element of g inside its
            # error band may change sign, which moves theta by 2 lr -- normwise ~ 2 sqrt(share of such elements) <= 3 sqrt(e))
            band = GOLDEN_BAND[name] if name != 'T5' else max(GOLDEN_BAND[name], 3.0 * float(np.sqrt(e)))
            gu.check_digest(z, 'theta/%d' % (it + 1), nm, p, rtol=RTOL if e <= RTOL / 10 else band, what=name)
    print('%s worst per-tensor meta-gradient rel err: %.3e' % (name, worst))


def _set_oracle_params(oracle, model, flat):
    with torch.no_grad():
        for nm, p in oracle.named_parameters():
            p.copy_(model._layout.view(flat, nm).cpu())


def _rel_errs(model, flat_g, oracle, grads):
    """per-tensor relative L2 error of the flat HIP gradient vs the oracle's list; exactly-zero tensors (key-projection biases:
    softmax is shift-invariant) are measured against 1e-4 of the global gradient norm"""
    gn = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    return {nm: float((model._layout.view(flat_g, nm).cpu() - t).norm() / max(float(t.norm()), 1e-4 * gn))
            for (nm, _), t in zip(oracle.named_parameters(), grads)}


def _pass_parity(model, oracle, batch, theta, what, max_flips=8):
    """One forward+backward of both implementations at IDENTICAL parameters.
    (1) free-running oracle: labels bit-exact, logits / loss, and the census of ReLU / max-pool decisions that differ (each
        must be a provable rounding near-tie, and there must be few);
    (2) oracle with the HIP pass's own branch decisions replayed (oracle.refimpl gates=): EVERY gradient tensor within 1e-4."""
    from oracle import refimpl as R
    from oracle import branches
    x, lens, y = batch
    _set_oracle_params(oracle, model, theta)
    out = model.pass_forward(x.cuda(), lens, y, theta=theta)
    g = torch.zeros_like(model.flat_grad)
    model.pass_backward(g, 1.0)
    gates = branches.gates_from_engine(model.engine)
    with torch.no_grad():
        (pred_r, gold_r, hyp_r), pre = branches.oracle_trace(oracle, x, lens, y)
        loss_r = R.ce_loss(pred_r, gold_r)
    assert torch.equal(out['hyp'].cpu(), hyp_r) and torch.equal(out['gold'].cpu(), gold_r), what   # bit-exact labels
    assert float((out['pred'].cpu() - pred_r).norm() / pred_r.norm()) < 1e-5, what
    assert abs(float(out['loss']) - float(loss_r)) < RTOL * float(loss_r), what
    flips, margin = branches.disagreements(model.engine, pre)
    assert flips <= max_flips, (what, flips)
    assert flips == 0 or margin < branches.NEAR_TIE, (what, flips, margin)
    del pre
    pred_g, gold_g, hyp_g = oracle(x, lens, y, gates=gates)
    loss_g = R.ce_loss(pred_g, gold_g)
    grads = torch.autograd.grad(loss_g, list(oracle.parameters()))
    assert torch.equal(hyp_g, hyp_r) and abs(float(loss_g) - float(loss_r)) < 1e-6 * float(loss_r), what
    errs = _rel_errs(model, g, oracle, grads)
    worst = max(errs, key=errs.get)
    print('%s: %d branch near-ties decided differently (margin %.1e); %d/%d gradient tensors within 1e-4, worst %.2e (%s)'
          % (what, flips, margin, sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (what, worst, errs[worst], flips)
    LAST_GATES[0] = gates
    return g, flips


LAST_GATES = [None]     # the device pass's own decisions of the latest _pass_parity call (the composition test compares schedules with them)


def _decisions_that_differ(log_a, log_b, k):
    """ReLU / max-pool decisions two runs of the same passes took differently (a task-batched pass pads every task's label axis to the
    widest task: decoder-side FFN masks are compared on the rows both have)"""
    n = 0
    for ga, gb in zip(log_a, log_b):
        for key in ga:
            a_, b_ = ga[key], gb[key]
            if a_.shape != b_.shape:
                a_ = a_.view(k, -1, a_.shape[-1])
                b_ = b_.view(k, -1, b_.shape[-1])
                w = min(a_.shape[1], b_.shape[1])
                a_, b_ = a_[:, :w], b_[:, :w]
            n += int((a_ != b_).sum())
    return n


@pytest.mark.parametrize('name', ['F0', 'F1'])
def test_every_pass_of_a_meta_step_against_live_oracle(name):
    """train pass at theta0 and validation pass at theta' for every task, each compared with the oracle evaluated at
    the SAME parameters; then the composed meta-gradient G against the sum of those passes."""
    from oracle import refimpl as R
    z, cfg, spec = gu.load(name)
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    oracle = R.build_model(cfg)
    tr, val = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    n = len(tr)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    G_sum = torch.zeros_like(model.flat_grad)
    single = []                                    # the single passes' own decisions, in the oracle's pass order
    for m, batch in enumerate(tr):
        g_tr, f_tr = _pass_parity(model, oracle, batch, model.flat_parameters, '%s task %d train' % (name, m))
        single.append(LAST_GATES[0])
        theta1 = inner.theta_prime_from(model.flat_parameters, g_tr).clone()
        ref_t1 = model.flat_parameters - spec['lr'] * g_tr                      # inner SGD step
        assert float((theta1 - ref_t1).abs().max()) <= 2.5e-7 * float(ref_t1.abs().max())   # fma vs mul+sub: 2 ulp
        g_val, f_val = _pass_parity(model, oracle, val, theta1, '%s task %d valid' % (name, m))
        single.append(LAST_GATES[0])
        G_sum += g_tr + g_val / n
    from oracle import branches
    trainer = mtl_amd.TransientTrainer()
    model.zero_copy_grad()
    as5 = lambda b: (b[0], b[1], None, b[2], None)
    # copy_grad composition.  The task-batched passes use other tile shapes (fp32 summation order: 1e-7 in g_tr, an ulp in theta'), so a
    # ReLU / max-pool decision at a rounding near-tie can fall the other way here; one such flip moves G by ~2e-5 (measured 2.3e-5 with one
    # near-tie of margin 5.6e-8).  The decisions of both runs are captured and COMPARED: the loose bound applies only when a decision actually
    # differs between the composed iteration and the single passes; with identical decisions the bound is the summation-order one.
    with branches.capture_gates(model) as log_b:
        trainer.meta_iteration(model, vocab, [as5(b) for b in tr], as5(val), n, inner, None, args)
        torch.cuda.synchronize()
    flips_b = _decisions_that_differ(single, log_b, spec['k'])
    comp = float((model._G - G_sum).norm() / G_sum.norm())
    print('%s composition (batched passes): |G - sum of passes| / |G| = %.2e, %d decisions differ from the single passes' % (name, comp, flips_b))
    assert len(log_b) == 2 * n and flips_b <= 4
    assert comp < (4e-6 if flips_b == 0 else 1e-4), (comp, flips_b)
    trainer.batch_tasks = False
    with branches.capture_gates(model) as log_l:
        trainer.meta_iteration(model, vocab, [as5(b) for b in tr], as5(val), n, inner, None, args)
        torch.cuda.synchronize()
    flips_l = _decisions_that_differ(single, log_l, spec['k'])
    comp_l = float((model._G - G_sum).norm() / G_sum.norm())
    print('%s composition (per-task lanes): %.2e, %d decisions differ' % (name, comp_l, flips_l))
    # per-task lanes: the same kernels as the single passes (the one-task input Linear as K slices is the same in both)
    assert comp_l < (2e-6 if flips_l == 0 else 1e-4), (comp_l, flips_l)


def test_single_pass_at_north_star_size_against_live_oracle():
    """190/190 gradient tensors within 1e-4 at the north-star size (k=8, T=1000, L=100, enc2/dec4 d512) with the HIP pass's
    ~250 M ReLU / max-pool decisions replayed in the oracle; the free-running census bounds how many of them differ (DESIGN 4:
    ~25 per pass, all rounding near-ties)."""
    from oracle import refimpl as R
    z, cfg, spec = gu.load('NS')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    oracle = R.build_model(cfg)
    batch = R.synth_batch(0, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], False)
    _pass_parity(model, oracle, batch, model.flat_parameters, 'NS single pass', max_flips=NS_FLIP_BOUND)


@pytest.mark.parametrize('n_tasks,conv', [(3, 'h2'), (8, 'h2'), (3, 'x3'), (8, 'x3')])
def test_meta_gradient_at_north_star_size_with_branch_replay(n_tasks, conv):
    """BASELINE.json configs[1] at full size: the meta-gradient G of TransientTrainer.meta_iteration (task-batched passes, side
    stream, fused inner step) against the LIVE oracle's G = sum_m [g_tr,m + g_val,m / n] computed with its own inner steps and
    the device path's branch decisions of all 2 n passes replayed: 190/190 tensors within 1e-4, losses within 1e-4, labels
    bit-exact.  (3, h2): configs[1] as the README runs it; (8, h2): the schedule bench.py times (8 tasks in ONE batched pass per
    phase); (3, x3) / (8, x3): the same steps with the convolutions on the exact 3-piece bf16 split (MTL_CONV=x3, bench.py's `conv_x3`: one
    launch per layer for all tasks as with h2)."""
    from oracle import refimpl as R
    from oracle import branches
    z, cfg, spec = gu.load('NS')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    for e in model.engines:
        e.conv_mode, e.conv_x3, e.conv_h2 = conv, True, conv == 'h2'
    torch.set_num_threads(min(32, torch.get_num_threads()))
    oracle = R.build_model(cfg)
    n = n_tasks
    tr = [R.synth_batch(10 * m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], False) for m in range(n)]
    val = R.synth_batch(10 * (n - 1) + 1, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], False)
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    as5 = lambda b: (b[0], b[1], None, b[2], None)
    trainer = mtl_amd.TransientTrainer()
    with branches.capture_gates(model) as log:
        reads = trainer.meta_iteration(model, vocab, [as5(b) for b in tr], as5(val), n, inner, None, args)
        torch.cuda.synchronize()
    assert len(log) == 2 * n
    with branches.record_preactivations(oracle) as pre_log:
        G_r, trl, val_l, labels = R.meta_gradient(oracle, tr, val, spec['lr'], gates=log)
    for m, (rd_tr, rd_va) in enumerate(reads):
        for rd, (gold, hyp), loss in ((rd_tr, labels[2 * m], trl[m]), (rd_va, labels[2 * m + 1], val_l[m])):
            assert torch.equal(rd.hyp, hyp) and torch.equal(rd.gold_host, gold)
            assert abs(float(rd.loss[0]) - loss) < RTOL * loss
    # the replayed decisions are not taken on trust: in every one of the six passes (training at theta0 and validation at theta')
    # the device's decisions differ from what the oracle's own pre-activations say only at a few rounding near-ties
    assert len(pre_log) == 2 * n
    census = [branches.replay_census(pre, gates) for pre, gates in zip(pre_log, log)]
    print('NS branch census per pass (differing decisions, largest margin): ' + ', '.join('%d / %.1e' % c for c in census))
    assert all(c[0] <= 120 and c[1] < branches.NEAR_TIE for c in census), census
    errs = _rel_errs(model, model._G, oracle, G_r)
    worst = max(errs, key=errs.get)
    print('NS %d-task meta-gradient (conv %s): %d/%d tensors within 1e-4, worst %.2e (%s)'
          % (n, conv, sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert len(errs) == 190 and errs[worst] < RTOL, (worst, errs[worst])


def test_one_local_task_of_eight_at_north_star_size_against_live_oracle():
    """What ONE rank of BASELINE.json configs[2] computes (8 tasks sharded one per GPU, SURVEY 8(e), transient_trainer.py:178-237): its
    single local task with the GLOBAL n = 8 in the validation term -- the lane schedule (no task batching), its local share
    G_r = g_tr + g_val / 8 against the live oracle with the device's branch decisions replayed: 190/190 tensors within 1e-4, labels
    bit-exact.  (The sum over ranks is the all-reduce: tests/test_dist_gloo.py.)"""
    from oracle import refimpl as R
    from oracle import branches
    z, cfg, spec = gu.load('NS')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    oracle = R.build_model(cfg)
    m = 5                                                        # the task rank 5 owns
    tr = R.synth_batch(10 * m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], False)
    val = R.synth_batch(10 * 7 + 1, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], False)      # the LAST task's validation batch
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    as5 = lambda b: (b[0], b[1], None, b[2], None)
    trainer = mtl_amd.TransientTrainer()
    with branches.capture_gates(model) as log:
        reads = trainer.meta_iteration(model, vocab, [as5(tr)], as5(val), 8, inner, None, args)
        torch.cuda.synchronize()
    assert len(log) == 2 and len(reads) == 1
    G_r, trl, val_l, labels = R.meta_gradient(oracle, [tr], val, spec['lr'], gates=log, n_tasks=8)
    for rd, (gold, hyp), loss in ((reads[0][0], labels[0], trl[0]), (reads[0][1], labels[1], val_l[0])):
        assert torch.equal(rd.hyp, hyp) and torch.equal(rd.gold_host, gold)
        assert abs(float(rd.loss[0]) - loss) < RTOL * loss
    errs = _rel_errs(model, model._G, oracle, G_r)
    worst = max(errs, key=errs.get)
    print('NS one local task of 8: %d/%d tensors within 1e-4, worst %.2e (%s)' % (sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert len(errs) == 190 and errs[worst] < RTOL, (worst, errs[worst])


def test_dropin_autograd_api_matches_oracle():
    """pred,gold,hyp = model(...); loss,_ = calculate_metrics(...); loss.backward() -- the reference's own call pattern."""
    from oracle import refimpl as R
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    oracle = R.build_model(cfg)
    (x, lens, y), _ = gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][0], None
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    opt.zero_grad()
    pred, gold, hyp = model(x.cuda(), lens, y)
    loss, ncorrect = mtl_amd.calculate_metrics(pred, gold, 0, smoothing=0.0, loss_type='ce')
    (loss / 3).backward()
    from oracle import branches
    pr, gr, hr = oracle(x, lens, y, gates=branches.gates_from_engine(model.engine))
    lref = R.ce_loss(pr, gr)
    (lref / 3).backward()
    assert abs(float(loss) - float(lref)) < RTOL * float(lref)
    assert ncorrect == int(((hr == gr) & (gr != 0)).sum())
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in oracle.parameters())))
    for (nm, p), (_, q) in zip(model.named_parameters(), oracle.named_parameters()):
        err = float((p.grad.cpu() - q.grad).norm() / max(float(q.grad.norm()), 1e-4 * gn))
        assert err < RTOL, (nm, err)
    # a second backward accumulates (torch .grad semantics, which SURVEY Q1 depends on)
    pred, gold, hyp = model(x.cuda(), lens, y)
    loss, _ = mtl_amd.calculate_metrics(pred, gold, 0)
    loss.backward()
    for (nm, p), (_, q) in zip(model.named_parameters(), oracle.named_parameters()):
        err = float((p.grad.cpu() - q.grad * 4).norm() / max(float(q.grad.norm() * 4), 4e-4 * gn))
        assert err < RTOL, (nm, err)


def test_round_trip_properties_full_size():
    """Size-independent properties at the north-star shapes: linearity of the backward in the loss scale and
    accumulate semantics, determinism (bitwise) of two identical passes."""
    z, cfg, spec = gu.load('NS')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    x, lens, y = mtl_amd.synth_batch(7, spec['k'], spec['T'], spec['L'], cfg['vocab_size'])
    g1, g2 = torch.zeros_like(model.flat_grad), torch.zeros_like(model.flat_grad)
    out = model.pass_forward(x.cuda(), lens, y)
    l1 = float(out['loss'])
    model.pass_backward(g1, 1.0)
    out = model.pass_forward(x.cuda(), lens, y)
    model.pass_backward(g2, 0.5)
    model.pass_backward(g2, 0.5)
    assert float(out['loss']) == l1                                   # deterministic forward
    assert float((g1 - g2).norm() / g1.norm()) < 1e-6                 # linear + accumulating backward
    g3 = torch.zeros_like(g1)
    model.pass_forward(x.cuda(), lens, y)
    model.pass_backward(g3, 1.0)
    assert torch.equal(g1, g3)                                        # fixed-order reductions: bitwise reproducible
    assert abs(l1 - np.log(cfg['vocab_size'])) < 0.5                  # CE at init ~ ln V


def test_joint_trainer_config0_against_reference_golden():
    """BASELINE.json configs[0] (joint_train.py) through the HIP path: loss trace, labels, gradients of both iterations."""
    z, cfg, spec = gu.load('J0')
    spec = dict(spec, meta_lr=spec['lr'])
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    names = [str(s) for s in z['param_names']]
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=True) for m in range(spec['n_tasks'])]
    tr = mtl_amd.JointTrainer()
    grads = []
    orig = tr.run_iteration

    def spy(model_, vocab_, batches, n, opt, a):
        step = opt.step
        opt.step = lambda g: (grads.append(g.clone()), step(g))[1]
        try:
            return orig(model_, vocab_, batches, n, opt, a)
        finally:
            opt.step = step
    tr.run_iteration = spy
    tr.train(model, vocab, tasks, [], 'ce', 0, spec['iters'], args, evaluate_every=10 ** 9, early_stop='cer,200')
    for it in range(spec['iters']):
        ref = sum(float(z['fwd/%d/%d/loss' % (it, j)]) for j in range(spec['n_tasks'])) / spec['n_tasks']
        assert abs(tr.loss_trace[it] - ref) <= RTOL * ref
        floor = 1e-4 * gu.global_l2(z, 'G/%d' % it, names)
        errs = [gu.check_digest(z, 'G/%d' % it, nm, model._layout.view(grads[it], nm), rtol=GOLDEN_BAND['F0'], what='J0', floor=floor)
                for nm in names]
        if it == 0:       # see test_meta_iterations_match_reference_goldens (measured: 67 / 68 clean, worst 1.7e-4; it 1: worst 1.7e-2)
            assert sum(e <= RTOL for e in errs) >= 60
        print('J0 it %d: %d/%d gradient tensors within 1e-4, worst %.2e' % (it, sum(e <= RTOL for e in errs), len(errs), max(errs)))


def test_clip_and_label_smoothing_meta_step_against_oracle():
    """--clip (transient_trainer.py:205-206,253-254) and --label-smoothing (utils/metrics.py:113-124) through train()."""
    from oracle import refimpl as R
    import torch.nn.functional as F
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    args.clip, args.max_norm = True, 3.0
    oracle = R.build_model(cfg)
    tr, val = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    from oracle import branches
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    as5 = lambda b: (b[0], b[1], None, b[2], None)
    with branches.capture_gates(model) as log:
        mtl_amd.TransientTrainer().meta_iteration(model, vocab, [as5(b) for b in tr], as5(val), len(tr), inner, None, args)
        torch.cuda.synchronize()
    G_r, _, _, _ = R.meta_gradient(oracle, tr, val, spec['lr'], max_norm=3.0, gates=log)
    errs = _rel_errs(model, model._G, oracle, G_r)
    assert max(errs.values()) < RTOL, max(errs.items(), key=lambda kv: kv[1])
    # label smoothing: loss + gradient of one pass against the reference formula restated in torch
    eps = 0.1
    x, lens, y = tr[0]
    out = model.pass_forward(x.cuda(), lens, y, smoothing=eps)
    g = torch.zeros_like(model.flat_grad)
    model.pass_backward(g, 1.0)
    pred, gold, _ = oracle(x, lens, y, gates=branches.gates_from_engine(model.engine))
    V = pred.size(2)
    p2, g2 = pred.view(-1, V), gold.view(-1)
    mask = g2.ne(0)
    one_hot = torch.zeros_like(p2).scatter(1, (mask.long() * g2).view(-1, 1), 1)
    one_hot = one_hot * (1 - eps) + (1 - one_hot) * eps / V
    loss = -(one_hot * F.log_softmax(p2, dim=1)).sum(1).masked_select(mask).sum() / int(mask.sum())
    grads = torch.autograd.grad(loss, list(oracle.parameters()))
    assert abs(float(out['loss']) - float(loss)) < RTOL * float(loss)
    errs = _rel_errs(model, g, oracle, grads)
    assert max(errs.values()) < RTOL, max(errs.items(), key=lambda kv: kv[1])


def test_long_utterance_stress_config():
    """BASELINE.json configs[3]: src-max-len 5000 (T' = 1250), dim-input 5120: runs, is finite, deterministic, and the
    backward is linear in the loss scale (size-independent properties; the oracle needs minutes at this size)."""
    z, cfg, spec = gu.load('NS')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    x, lens, y = mtl_amd.synth_batch(3, 8, 5000, 100, cfg['vocab_size'])
    lens[3], lens[5] = 300, 2500                      # exercises the raw-length masks on the pooled axis (Q2)
    x[3, :, :, 300:] = 0
    x[5, :, :, 2500:] = 0
    xd = x.cuda()
    out = model.pass_forward(xd, lens, y)
    l1 = float(out['loss'])
    g1 = torch.zeros_like(model.flat_grad)
    model.pass_backward(g1, 1.0)
    assert np.isfinite(l1) and bool(torch.isfinite(g1).all()) and abs(l1 - np.log(cfg['vocab_size'])) < 0.5
    out = model.pass_forward(xd, lens, y)
    g2 = torch.zeros_like(g1)
    model.pass_backward(g2, 0.25)
    assert float(out['loss']) == l1 and float((g1 * 0.25 - g2).norm() / g2.norm()) < 1e-6
    assert out['hyp'].shape == (8, 101) and int(out['hyp'].max()) < cfg['vocab_size']


def test_two_ranks_sharded_bench_equals_single_rank(tmp_path):
    """bench.py under torchrun with 2 ranks (sharing this box's single GPU over gloo): the sharded meta-step with ONE
    all-reduce of G must reproduce the single-rank step (same loss / CER of the last step), and so must what `--dump-outputs`
    writes of that step (theta, the meta-gradient, the last step's loss / CER read-back)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ['--steps', '2', '--warmup', '1', '--tasks', '4', '--k', '2', '--frames', '200', '--labels', '20', '--no-cpu-baseline']
    env = dict(os.environ, MTL_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    one = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--dump-outputs', str(tmp_path / 'one')] + common,
                         capture_output=True, text=True, env=env, timeout=240)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                          '127.0.0.1', '--master-port', '29733', os.path.join(root, 'bench.py'), '--gpus', '2',
                          '--dump-outputs', str(tmp_path / 'two')] + common, capture_output=True, text=True, env=env, timeout=240)
    assert two.returncode == 0, two.stderr[-2000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith('{')][-1])
    j2 = json.loads([l for l in two.stdout.splitlines() if l.startswith('{')][-1])
    assert j2['n_gpus'] == 2 and j1['n_gpus'] == 1 and j2['scaling'] == 'strong'
    assert j1['last_step']['chars'] == j2['last_step']['chars'] and j1['last_step']['cer_edits'] == j2['last_step']['cer_edits']
    assert abs(j1['last_step']['val_loss'] - j2['last_step']['val_loss']) < 1e-4 * abs(j1['last_step']['val_loss'])
    # the dumped outputs: the line's read-back, and theta / meta-gradient of the single-rank and the sharded run
    d = {w: {n: np.load(str(tmp_path / w / (n + '.npy'))) for n in ('theta', 'meta_grad', 'last_step')} for w in ('one', 'two')}
    for w, j in (('one', j1), ('two', j2)):
        assert d[w]['theta'].dtype == np.float32 and d[w]['meta_grad'].dtype == np.float32 and d[w]['last_step'].dtype == np.float64
        assert d[w]['theta'].size == d[w]['meta_grad'].size and np.isfinite(d[w]['meta_grad']).all() and float(np.abs(d[w]['meta_grad']).max()) > 0
        assert abs(d[w]['last_step'][0] / 4 - j['last_step']['val_loss']) <= 1e-6 * abs(j['last_step']['val_loss'])
        assert d[w]['last_step'][1:].tolist() == [j['last_step']['cer_edits'], j['last_step']['chars']]
    a64 = {w: {n: d[w][n].astype(np.float64) for n in ('theta', 'meta_grad')} for w in d}
    rel = float(np.linalg.norm(a64['two']['theta'] - a64['one']['theta']) / np.linalg.norm(a64['one']['theta']))
    cos = float(a64['two']['meta_grad'] @ a64['one']['meta_grad'] / np.linalg.norm(a64['two']['meta_grad']) / np.linalg.norm(a64['one']['meta_grad']))
    # (Adam turns the rounding noise of gradients that are zero in exact arithmetic -- the key-projection biases -- into full-size steps;
    # after the setup, warm-up and timed iterations theta agrees to that noise and the meta-gradient taken there keeps its direction)
    assert rel < 1e-3 and cos > 0.99, (rel, cos)
    # the default above all-reduced G group by group under the validation backward (dist.ChunkedAllReduce: decoder, encoder, conv);
    # with two ranks every element is a + b either way, so ONE collective after the backward must give the same bits of theta
    single = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                             '127.0.0.1', '--master-port', '29735', os.path.join(root, 'bench.py'), '--gpus', '2'] + common,
                            capture_output=True, text=True, env=dict(env, MTL_CHUNKED_ALLREDUCE='0'), timeout=240)
    assert single.returncode == 0, single.stderr[-2000:]
    j3 = json.loads([l for l in single.stdout.splitlines() if l.startswith('{')][-1])
    assert j2['theta_checksum'] == j3['theta_checksum'] and j2['last_step'] == j3['last_step'], (j2['theta_checksum'], j3['theta_checksum'])


def test_plain_bench_invocation_starts_its_own_ranks():
    """`python3 bench.py --gpus 2 ...` with NO launcher around it (the form the driver uses for N = 1): bench.py starts its two ranks
    itself (`self_launch_command`), stdout carries exactly ONE line -- rank 0's JSON -- and that line says n_gpus 2, two ranks, bit-identical
    replicas.  The N = 1 line carries the same `multi_gpu` keys, so a SCALE run's N = 1 entry can be held against the BENCH line."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ['--steps', '2', '--warmup', '1', '--tasks', '4', '--k', '2', '--frames', '200', '--labels', '20', '--no-cpu-baseline']
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MTL_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', MTL_POOL_GB='2')
    two = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2'] + common, capture_output=True, text=True,
                         env=env, timeout=400)
    assert two.returncode == 0, two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    j2 = json.loads(lines[0])
    mg = j2['multi_gpu']
    assert j2['n_gpus'] == 2 and mg['ranks'] == 2 and mg['replicas_bit_identical'] is True and mg['launcher'] == 'self'
    assert mg['tasks_per_rank'] == [2, 2] and len(mg['per_rank_ms_per_step']) == 2 and mg['allreduce_bytes_per_step'] > 0
    one = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--no-extras'] + common, capture_output=True,
                         text=True, env=env, timeout=300)
    assert one.returncode == 0, one.stderr[-2000:]
    lines1 = [l for l in one.stdout.splitlines() if l.strip()]
    assert len(lines1) == 1
    j1 = json.loads(lines1[0])
    assert set(j1) - {'cpu_baseline'} <= set(j2) | {'cpu_baseline'} and set(j1['multi_gpu']) == set(mg)
    assert j1['multi_gpu']['ranks'] == 1 and j1['multi_gpu']['launcher'] == 'none' and j1['multi_gpu']['collective'] == 'none'
    assert j1['last_step']['chars'] == j2['last_step']['chars'] and j1['last_step']['cer_edits'] == j2['last_step']['cer_edits']
    assert abs(j1['last_step']['val_loss'] - j2['last_step']['val_loss']) < 1e-4 * abs(j1['last_step']['val_loss'])


@pytest.mark.parametrize('world,tasks', [(4, 8), (4, 4)])
def test_sharded_bench_at_four_ranks_on_one_gpu(world, tasks):
    """bench.py's sharded step with the ranks sharing this box's single GPU over gloo: 8 tasks on 4 ranks (2 per rank: the task-batched
    schedule with the slice hooks) and 4 tasks on 4 ranks (ONE task per rank: the lane schedule a rank of the 8-GPU node runs) must
    reproduce the single-process step (labels / CER counts equal, loss within 1e-4), report the rank count and the per-rank step times
    in the `multi_gpu` block, and leave bit-identical replicas.  Four ranks, the launcher and this process are six processes holding
    the one device; eight ranks would be ten, more than a shared GPU node admits at once.  The configs[2] partition itself (8 tasks on
    8 ranks, the 8-way sliced all-reduce) is checked over gloo on CPU: tests/test_dist_gloo.py::test_world8_one_task_per_rank_three_iterations."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ['--steps', '2', '--warmup', '1', '--tasks', str(tasks), '--k', '2', '--frames', '120', '--labels', '12', '--no-cpu-baseline']
    env = dict(os.environ, MTL_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', MTL_POOL_GB='2')
    one = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--no-extras'] + common, capture_output=True, text=True,
                         env=env, timeout=300)
    assert one.returncode == 0, one.stderr[-2000:]
    many = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
                           '127.0.0.1', '--master-port', str(29750 + world), os.path.join(root, 'bench.py'), '--gpus', str(world)] + common,
                          capture_output=True, text=True, env=env, timeout=600)
    assert many.returncode == 0, many.stderr[-3000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith('{')][-1])
    jn = json.loads([l for l in many.stdout.splitlines() if l.startswith('{')][-1])
    assert jn['n_gpus'] == world and jn['scaling'] == 'strong' and jn['config']['collective'] == 'gloo'
    mg = jn['multi_gpu']
    assert mg['ranks'] == world and mg['replicas_bit_identical'] is True and mg['tasks_per_rank'] == [tasks // world] * world
    assert len(mg['per_rank_ms_per_step']) == world and all(t > 0 for t in mg['per_rank_ms_per_step'])
    assert j1['last_step']['chars'] == jn['last_step']['chars'] and j1['last_step']['cer_edits'] == jn['last_step']['cer_edits']
    assert abs(j1['last_step']['val_loss'] - jn['last_step']['val_loss']) < 1e-4 * abs(j1['last_step']['val_loss'])
    assert len(many.stdout.strip().splitlines()[-1]) < 4096


def test_sharded_bench_on_manifest_like_batches_equals_single_rank():
    """Two gloo ranks sharing this box's GPU, two tasks each, on batches padded to their OWN longest utterance with new shapes every step
    (`bench.py --ragged`): every rank stacks its tasks at its own widest (a different width per rank and step), the three slice
    all-reduces leave under the validation backward as in the fixed-shape case; the step must reproduce the single-process run
    (4 tasks in one stack) and leave bit-identical replicas."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ['--steps', '3', '--warmup', '1', '--tasks', '4', '--k', '2', '--frames', '150', '--labels', '12', '--no-cpu-baseline', '--no-extras', '--ragged']
    env = dict(os.environ, MTL_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', MTL_POOL_GB='2', MTL_RAGGED_QUANTUM='16')
    one = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1'] + common, capture_output=True, text=True, env=env, timeout=300)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', '29761', os.path.join(root, 'bench.py'), '--gpus', '2'] + common, capture_output=True, text=True,
                         env=env, timeout=600)
    assert two.returncode == 0, two.stderr[-3000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith('{')][-1])
    j2 = json.loads([l for l in two.stdout.splitlines() if l.startswith('{')][-1])
    assert j2['multi_gpu']['ranks'] == 2 and j2['multi_gpu']['replicas_bit_identical'] is True
    assert j1['last_step']['chars'] == j2['last_step']['chars'] and j1['last_step']['cer_edits'] == j2['last_step']['cer_edits']
    assert abs(j1['last_step']['val_loss'] - j2['last_step']['val_loss']) < 1e-4 * abs(j1['last_step']['val_loss'])
    assert abs(j1['theta_checksum'][0] - j2['theta_checksum'][0]) < 1e-5 * abs(j1['theta_checksum'][0])


def _dropout_pass_parity(cfg, spec, batch, on_model=None):
    """the body of test_dropout_pass_matches_oracle_with_the_same_masks for any model and batch (tests/test_unfused_attention_gpu.py
    runs it on a model the fused attention kernel does not serve); on_model(model) is called before the first pass
    -> (model, per-tensor gradient errors)"""
    from oracle import refimpl as R
    mtl_amd, args, vocab, model = make(cfg, spec)
    args.dropout = 0.1
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r']).cuda()
    model.train()
    if on_model is not None:
        on_model(model)
    oracle = R.build_model(cfg)
    (x, lens, y) = batch
    out = model.pass_forward(x.cuda(), lens, y)
    g = torch.zeros_like(model.flat_grad)
    model.pass_backward(g, 1.0)
    A = model.engine.arena
    B, Td = out['hyp'].shape
    h, d, sc = cfg['num_heads'], cfg['dim_model'], 1.0 / 0.9
    drop = {}
    for name, m in A.items():
        if name.endswith('.mP'):
            Tk = A[name[:-2] + 'k'].shape[0] // B
            drop[name] = m.cpu().float()[..., :Tk] * sc
        elif name.endswith('.mo') or name.endswith('.mf') or name == 'dec_in.me':
            drop[name] = m.cpu().float().view(B, -1, d) * sc
    assert len(drop) == 3 * cfg['num_enc_layers'] + 5 * cfg['num_dec_layers'] + 1
    keep_rate = float(torch.cat([v.reshape(-1) for v in drop.values()]).gt(0).float().mean())
    assert abs(keep_rate - 0.9) < 0.01
    from oracle import branches
    pred_r, gold_r, hyp_r = oracle(x, lens, y, drop=drop, gates=branches.gates_from_engine(model.engine))
    loss_r = R.ce_loss(pred_r, gold_r)
    grads = torch.autograd.grad(loss_r, list(oracle.parameters()))
    assert torch.equal(out['hyp'].cpu(), hyp_r)
    assert float((out['pred'].cpu() - pred_r).norm() / pred_r.norm()) < 1e-5
    assert abs(float(out['loss']) - float(loss_r)) < RTOL * float(loss_r)
    errs = _rel_errs(model, g, oracle, grads)
    assert max(errs.values()) < RTOL, max(errs.items(), key=lambda kv: kv[1])
    # fresh masks on the next pass, none in eval mode
    m0 = A['dec_in.me'].clone()
    model.pass_forward(x.cuda(), lens, y)
    assert not torch.equal(m0, model.engine.arena['dec_in.me'])
    model.eval()
    out_e = model.pass_forward(x.cuda(), lens, y)
    assert 'dec_in.me' not in model.engine.arena
    pr0, _, _ = oracle(x, lens, y)
    assert float((out_e['pred'].cpu() - pr0).norm() / pr0.norm()) < 1e-5
    return model, errs


def test_dropout_pass_matches_oracle_with_the_same_masks():
    """--dropout 0.1 (README config): the keep-masks the HIP pass drew are replayed inside the oracle, so
    forward and backward must agree exactly like the dropout-free pass (the masks themselves come from Philox, not from
    torch's RNG stream, which is why parity with the reference is defined only given the masks)."""
    z, cfg, spec = gu.load('F0')
    _dropout_pass_parity(cfg, spec, gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][0])


@pytest.mark.parametrize('dropout', [0.0, 0.1])
def test_command_list_replay_is_bitwise_equal_to_eager(dropout):
    """The per-task body recorded into a command list and replayed by mtl_cmdlist_run (the trainer's _lib.Replay, default on) must
    reproduce the eager meta-gradient bit for bit -- side-stream fork / join, re-pointed input batches and (with dropout) the
    per-pass Philox seeds read from device memory included -- also for batches it was not recorded on."""
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    args.dropout = dropout
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r']).cuda()
    as5 = lambda b: (b[0].cuda(), b[1], None, b[2], None)
    mk = lambda s0: [as5(mtl_amd.synth_batch(s0 + i, 2, 64, 8, cfg['vocab_size'])) for i in range(6)]
    val = as5(mtl_amd.synth_batch(77, 2, 64, 8, cfg['vocab_size']))
    inner = mtl_amd.FlatSGD(model, spec['lr'])
    model.zero_copy_grad()
    res = {}
    for mode in (False, True):
        tr = mtl_amd.TransientTrainer()
        tr.batch_tasks = False                     # the lanes' command lists (the batched step's: tests/test_batched_gpu.py)
        tr.use_cmdlists = mode
        outs = []
        for s0 in (100, 200, 300):                 # the third batch set runs purely on replays when command lists are on
            torch.manual_seed(s0)                  # the dropout seeds of the passes come from torch's CPU generator
            reads = tr.meta_iteration(model, vocab, mk(s0), val, 6, inner, None, args)
            torch.cuda.synchronize()
            outs.append((model._G.clone(), [(r.loss.clone(), r.hyp.clone()) for pair in reads for r in pair]))
        res[mode] = outs
        if mode:
            recorded = tr.replay.recorded()
            assert len(recorded) == min(model.n_lanes, 6) and all(cl.n > 100 for cl in recorded)      # one list per lane in use
    for (G0, r0), (G1, r1) in zip(res[False], res[True]):
        assert torch.equal(G0, G1)
        for (l0, h0), (l1, h1) in zip(r0, r1):
            assert torch.equal(l0, l1) and torch.equal(h0, h1)


@pytest.mark.parametrize('B,T,L,lens,tlens', [
    (1, 17, 1, [17], [1]),                       # single utterance, T' = 4, one label
    (3, 50, 5, [50, 13, 4], [5, 2, 1]),          # T not a multiple of 4/8; a row shorter than T/4; ragged targets
    (2, 129, 12, [129, 65], [12, 7]),            # odd T, pooled tails (129 -> 64 -> 32)
    (5, 36, 3, [36, 36, 9, 30, 1], [3, 3, 1, 2, 3]),   # a length-1 utterance (everything past key 0 masked)
])
def test_ragged_shapes_against_live_oracle(B, T, L, lens, tlens):
    """edge shapes of the path (empty/ragged inputs): tile tails of every kernel, Q2 masks, PAD/EOS handling"""
    from oracle import refimpl as R
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    oracle = R.build_model(cfg)
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, 1, 161, T, generator=g)
    y = torch.randint(4, cfg['vocab_size'], (B, L), generator=g)
    for i in range(B):
        x[i, :, :, lens[i]:] = 0
        y[i, tlens[i]:] = 0
    _pass_parity(model, oracle, (x, torch.tensor(lens, dtype=torch.int32), y), model.flat_parameters, 'ragged B%d T%d' % (B, T))


def test_greedy_decoding_matches_oracle():
    """Transformer.evaluate / Decoder.greedy_search -- token ids of every step, bit-exact, and the strings."""
    from oracle import refimpl as R
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    oracle = R.build_model(cfg)
    x, lens, y = R.synth_batch(5, 3, 72, 6, cfg['vocab_size'], True)
    steps = 24
    _, hyps, golds = model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=steps)
    ref = R.greedy_search(oracle, x, lens, vocab.SOS_ID, steps)             # (B, steps)
    assert torch.equal(model.last_greedy_ids.t().contiguous(), ref)
    # the steps of a decode are recorded into one command list at its second sighting and replayed from C afterwards: eager, recording and
    # two replays give the same tokens; a decode of another length in between does not disturb the recorded one
    for rep in range(3):
        _, hyps_r, _ = model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=steps)
        assert torch.equal(model.last_greedy_ids.t().contiguous(), ref) and hyps_r == hyps, rep
        if rep == 1:
            model.evaluate(x.cuda(), lens, y, args, start_token=vocab.SOS_ID, max_steps=steps - 5)
            assert torch.equal(model.last_greedy_ids.t().contiguous(), ref[:, :steps - 5])
    recorded = model.engine.replay_greedy.recorded()
    assert len(recorded) == 1 and recorded[0].n >= 12 * steps
    for b in range(3):
        exp = ''
        for t in ref[b].tolist():
            if t == vocab.EOS_ID:
                break
            exp += vocab.id2label[t]
        assert hyps[b] == exp
    _, gold_ref, _ = oracle(x, lens, y)
    assert golds == [''.join(vocab.id2label[int(t)] for t in row) for row in gold_ref]
    assert model.training                                                   # evaluate() restores the mode


def test_searches_record_again_after_the_scratch_buffer_moved():
    """eager, recorded, replayed; then eng.scratch() is asked for more than it holds (a new buffer and a new scratch_epoch: the recorded
    lists hold the old address) and the searches go eager, recorded, replayed again -- the same ids six times, and one list per unit
    under the key afterwards.  Greedy search (3 utterances, 8 steps) and the device-ranked beam search (2 utterances in one chunk, W = 3)."""
    from oracle import refimpl as R
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    model.eval()
    eng, theta = model.engine, model.flat_parameters
    x, lens, y = R.synth_batch(5, 3, 72, 6, cfg['vocab_size'], True)
    eng.widen = '0'
    model.pass_forward(x.cuda(), lens, y)
    mem, T4 = eng.encoder_output().clone(), (72 // 2) // 2
    steps, W = 8, 3

    def grow_scratch():
        held, epoch = eng.arena.get('_scratch'), eng.scratch_epoch
        eng.scratch((held.numel() * 4 if held is not None else 0) + 4096)
        assert eng.scratch_epoch == epoch + 1

    def six_times(search, replay):
        outs, lists = [], []
        for rnd in range(6):
            if rnd == 3:
                grow_scratch()
            outs.append(search())
            lists.append(len(replay.recorded(replay.keys()[-1])))
        assert len(replay.keys()) == 1 and lists[0] == lists[3] == 0 and lists[1] == lists[2] == lists[4] == lists[5] >= 1, lists
        return outs, lists[5]
    ids, n = six_times(lambda: eng.greedy_decode(theta, mem.data_ptr(), 3, T4, vocab.SOS_ID, steps).clone(), eng.replay_greedy)
    assert ids[0].shape == (steps, 3) and all(torch.equal(ids[0], other) for other in ids[1:])
    assert n == 1 and eng.replay_greedy.recorded()[0].n >= 12 * steps
    nbest, n = six_times(lambda: eng.beam_decode_batch(theta, mem.data_ptr(), 2, T4, vocab.SOS_ID, W, 2, cfg['tgt_max_len'], model._num_words,
                                                       vocab.EOS_ID, 1.0, chunk=2), eng.replay_beam_batch)
    assert len(nbest[0]) == 2 and all(nbest[0] == other for other in nbest[1:])
    assert n <= -(-T4 // eng.BEAM_POLL)                      # one list per block of positions that ran


def test_beam_search_matches_reference_golden_and_oracle():
    """Transformer.evaluate(beam_search=True) -> PassEngine.beam_decode reproduces the REAL reference's n-best id
    sequences and strings (tests/golden/B0.npz: natural EOS terminations of different lengths, n-best order) token for token,
    and a second input against the live oracle."""
    from oracle import refimpl as R
    bspec, ids, strs, eval_strs = gu.load_beam()
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    gu.perturb_output_layer(model.decoder.output_linear.weight, bspec)
    model = model.cuda()
    args.beam_width, args.beam_nbest, args.tgt_max_len = bspec['beam_width'], bspec['nbest'], cfg['tgt_max_len']
    x, lens, y = R.synth_batch(bspec['seed'], bspec['k'], bspec['T'], bspec['L'], cfg['vocab_size'], True)
    _, hyps, golds = model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=vocab.SOS_ID)
    assert model.last_beam_ids == ids
    assert hyps == strs == eval_strs
    # a different batch (other lengths, beam 4, n-best 3) against the oracle's restatement
    oracle = R.build_model(cfg)
    gu.perturb_output_layer(oracle.decoder.output_linear.weight, bspec)
    x, lens, y = R.synth_batch(909, 2, 80, 5, cfg['vocab_size'], True)
    args.beam_width, args.beam_nbest = 4, 3
    model.evaluate(x.cuda(), lens, y, args, beam_search=True, start_token=vocab.SOS_ID)
    nw = gu.label_words(vocab.id2label, [vocab.PAD_TOKEN, vocab.SOS_TOKEN, vocab.EOS_TOKEN])
    ref = R.beam_search(oracle, x, lens, vocab.SOS_ID, 4, 3, cfg['tgt_max_len'], nw)
    assert model.last_beam_ids == [seq for utt in ref for seq, _ in utt]
    assert model.training
