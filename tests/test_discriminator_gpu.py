"""MI355X: the accent discriminator (csrc/mtl_disc.hip) against the fp64 restatement of tests/disc_util.py within fp32 summation bounds,
bitwise repeatability, JointTrainer parity with the reference's record D0 in all three modes, the inert seam, training end to end with
checkpoints, and calculate_adversarial / calculate_multi_task as autograd functions."""
import os

import numpy as np
import pytest
import torch

from tests import disc_util as du
from tests import golden_util as gu
from tests.test_parity_gpu import make, RTOL, GOLDEN_BAND

pytestmark = pytest.mark.gpu
U = du.U
CHUNK = 16                      # MTL_DISC_CHUNK of include/mtl_hip.h: rows of one utterance per stage-1 workgroup
T1 = CHUNK + 1                  # one row more than a stage-1 workgroup covers
SHAPES = [(1, 1, 4, 1), (3, 7, 100, 2), (2, 16, 128, 3), (5, T1, 512, 64), (2, 2 * T1 + 3, 132, 5),     # one chunk, ragged last, several
          (2, 70, 8, 20), (1, 131, 4, 33)]      # the encoder-gradient pass takes 64 rows per workgroup from 17 classes, 128 from 33: two workgroups each
AB = [(1.0, 0.0), (0.5 / 3, 1.0 / 3), (0.0, 0.0)]


def _lib():
    import mtl_amd
    return mtl_amd._lib.lib()


def _inputs(B, T, d, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + T + d + C)
    enc = torch.randn(B, T, d, generator=g)
    W = torch.randn(C, d, generator=g) / float(np.sqrt(d * T))
    bias = torch.randn(C, generator=g)
    return enc, W, bias


def _fwd(enc, W, bias, accent, mode):
    L, st = _lib(), torch.cuda.current_stream().cuda_stream
    B, T, d = enc.shape
    C = W.shape[0]
    dev = dict(enc=enc.cuda(), W=W.cuda(), bias=bias.cuda(), pooled=torch.full((B, d), 7.0).cuda(), logits=torch.full((B, C), 7.0).cuda(),
               losses=torch.full((2,), -3.0).cuda())
    nbytes = L.mtl_disc_workspace(B, T, d)
    assert nbytes == B * -(-T // CHUNK) * d * 4
    ws = torch.full((nbytes // 4,), float('nan')).cuda()               # the workspace needs no initialisation
    rc = L.mtl_disc_fwd(st, dev['enc'].data_ptr(), B, T, d, dev['W'].data_ptr(), dev['bias'].data_ptr(), C, accent, mode,
                        dev['pooled'].data_ptr(), dev['logits'].data_ptr(), dev['losses'].data_ptr(), ws.data_ptr(), nbytes)
    assert rc == 0
    return dev


def _bwd(dev, accent, mode, a, b, B, T, d, C, seed=1):
    L, st = _lib(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(seed)
    pre = dict(dW=torch.randn(C, d, generator=g), dbias=torch.randn(C, generator=g), denc=torch.randn(B, T, d, generator=g))
    out = {k: v.cuda() for k, v in pre.items()}
    rc = L.mtl_disc_bwd(st, dev['pooled'].data_ptr(), dev['logits'].data_ptr(), dev['W'].data_ptr(), accent, B, T, d, C, mode, a, b,
                        out['dW'].data_ptr(), out['dbias'].data_ptr(), out['denc'].data_ptr())
    assert rc == 0
    return pre, out


def _within(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref.double()).abs()
    bound = torch.as_tensor(bound).double()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s: worst error / bound = %.3f (max error %.3e)' % (what, worst, float(err.max())))
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize('B,T,d,C', SHAPES)
def test_kernels_against_the_fp64_restatement(B, T, d, C):
    enc, W, bias = _inputs(B, T, d, C)
    accent = C - 1
    for mode in (0, 1):
        dev = _fwd(enc, W, bias, accent, mode)
        pooled64 = du.pool(enc)
        logits64, ce, mse = du.head(pooled64, W, bias, accent, mode)
        tag = '(%d,%d,%d,%d) mode %d' % (B, T, d, C, mode)
        # pooled sums: n u sum|x| with n = T terms
        _within(dev['pooled'], pooled64, du.pooled_bound(enc), tag + ' pooled')
        dl = du.logits_bound(enc, W, bias)
        _within(dev['logits'], logits64, dl, tag + ' logits')
        ce_b, mse_b = du.losses_bound(logits64, dl, mode)
        losses = dev['losses'].cpu()
        _within(losses[0], ce, ce_b, tag + ' CE')
        if mode == 1:
            _within(losses[1], mse, mse_b, tag + ' MSE')
        else:
            assert float(losses[1]) == -3.0                               # mode 0 leaves losses[1] alone
        for a, b in AB:
            pre, out = _bwd(dev, accent, mode, a, b, B, T, d, C)
            _, dW, dbias, dpool = du.grads(pooled64, logits64, W, accent, mode, a, b)
            bW, bb, bp = du.grads_bound(enc, logits64, W, dl, accent, mode, a, b)
            t2 = tag + ' a=%.3f b=%.3f' % (a, b)
            # `+=` onto the pre-filled values: one more rounding at the magnitude of the sum
            _within(out['dW'], pre['dW'].double() + dW, bW + U * (pre['dW'].abs() + dW.abs()), t2 + ' dW')
            _within(out['dbias'], pre['dbias'].double() + dbias, bb + U * (pre['dbias'].abs() + dbias.abs()), t2 + ' dbias')
            want = pre['denc'].double() + dpool[:, None, :]
            _within(out['denc'], want, bp[:, None, :] + U * (pre['denc'].abs() + dpool.abs()[:, None, :]), t2 + ' denc')
            if a == 0.0 and b == 0.0:
                assert torch.equal(out['denc'].cpu(), pre['denc']) and torch.equal(out['dW'].cpu(), pre['dW'])


@pytest.mark.parametrize('B,T,d,C', [SHAPES[3], SHAPES[4]])
def test_two_calls_are_bitwise_equal(B, T, d, C):
    enc, W, bias = _inputs(B, T, d, C, seed=3)
    runs = []
    for _ in range(2):
        dev = _fwd(enc, W, bias, 1, 1)
        _, out = _bwd(dev, 1, 1, 0.4, 0.3, B, T, d, C)
        runs.append([dev[k].cpu() for k in ('pooled', 'logits', 'losses')] + [out[k].cpu() for k in ('dW', 'dbias', 'denc')])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def _setup(mode, name='disc', folder=None):
    z, cfg, spec = du.load_d0()
    mtl_amd, args, vocab, model = make(cfg, spec, name=name)
    args.num_class, args.lr_disc, args.loss = spec['num_class'], spec['lr_disc'], 'ce'
    for k, v in du.mode_flags(mode).items():
        setattr(args, k, v)
    if folder is not None:
        args.save_folder = folder
    disc = mtl_amd.init_discriminator_model(args)                         # seeded after the model, like the record
    return z, cfg, spec, mtl_amd, args, vocab, model, disc


@pytest.mark.parametrize('mode', du.MODES)
def test_joint_trainer_matches_the_reference_record(mode, capsys):
    """Two iterations of JointTrainer from the F0 initialisation against D0: per-task losses, the discriminator's gradients, the
    model's gradient digests, both parameter sets after the two optimizer steps, and the printed iteration line (its figures carry
    four decimals: 1e-6 relative on ENC LOSS ~ 87; every figure is printed before it is asserted)."""
    z, cfg, spec, mtl_amd, args, vocab, model, disc = _setup(mode)
    for nm, p in disc.named_parameters():
        assert torch.equal(p.detach(), torch.from_numpy(z['disc_theta0/' + nm])), nm
    model, disc = model.cuda(), disc.cuda()
    names = [str(s) for s in z['param_names']]
    n, adv = spec['n_tasks'], mode != 'multitask'
    tasks = [mtl_amd.SyntheticTask(m, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], variable=True) for m in range(n)]
    tr = mtl_amd.JointTrainer()
    rec = []
    orig = tr.run_iteration

    def spy(model_, vocab_, batches, n_, opt, a, **kw):
        od, step, dstep, got = kw['opt_disc'], opt.step, kw['opt_disc'].step, {}
        opt.step = lambda g: (got.__setitem__('G', g.clone()), step(g))[1]
        od.step = lambda: (got.__setitem__('dG', disc.flat_grad.clone()), dstep())[1]
        try:
            out = orig(model_, vocab_, batches, n_, opt, a, **kw)
        finally:
            opt.step, od.step = step, dstep
        got.update(losses=list(tr.task_losses), theta=model.flat_parameters.clone(), dtheta=disc.flat_parameters.clone())
        rec.append(got)
        return out
    tr.run_iteration = spy
    tr.train(model, vocab, tasks, [], 'ce', 0, spec['iters'], args, evaluate_every=10 ** 9, early_stop='cer,200', discriminator=disc)
    printed = [ln for ln in capsys.readouterr().out.split('\n') if ln.startswith('(Iteration')]
    C, d = spec['num_class'], cfg['dim_model']
    lines_ok = True
    for it in range(spec['iters']):
        got = rec[it]
        for m in range(n):
            key = '%s/%d/%d' % (mode, it, m)
            t_loss, d_loss, e_loss = got['losses'][m]
            ref = float(z[key + '/tr'])
            print(key, 'tr %.7f vs %.7f  disc %.7e vs %.7e  enc %s' % (t_loss, ref, d_loss, float(z[key + '/disc']),
                                                                       (e_loss, float(z[key + '/enc_l'])) if adv else ''))
            assert abs(t_loss - ref) <= RTOL * ref, key
            # the J0 loss tolerance, plus the response of a CE to logits that agree within that tolerance (du.ce_tolerance)
            assert abs(d_loss - float(z[key + '/disc'])) <= du.ce_tolerance(z[key + '/disc'], z[key + '/logits'], m, RTOL, RTOL), key
            if adv:
                assert abs(e_loss - float(z[key + '/enc_l'])) <= RTOL * float(z[key + '/enc_l']), key
        pre = '%s/%d' % (mode, it)
        for nm, lo, hi in (('linear.weight', 0, C * d), ('linear.bias', C * d, C * d + C)):
            ref = z['%s/dG/%s' % (pre, nm)].reshape(-1).astype(np.float64)
            err = float(np.linalg.norm(got['dG'][lo:hi].cpu().numpy() - ref) / np.linalg.norm(ref))
            print('%s dG %s rel err %.3e' % (pre, nm, err))
            assert err <= RTOL, (pre, nm, err)
        floor = 1e-4 * gu.global_l2(z, pre + '/G', names)
        errs = [gu.check_digest(z, pre + '/G', nm, model._layout.view(got['G'], nm), rtol=GOLDEN_BAND['F0'], what='D0', floor=floor)
                for nm in names]
        print('%s: %d/%d model gradient tensors within 1e-4, worst %.2e' % (pre, sum(e <= RTOL for e in errs), len(errs), max(errs)))
        if it == 0:         # tests/test_parity_gpu.py::test_joint_trainer_config0_against_reference_golden
            assert sum(e <= RTOL for e in errs) >= 60
        for nm, e in zip(names, errs):
            if float(z['%s/G/%s/l2' % (pre, nm)]) < floor * 1e-2:
                continue    # Adam on an exactly-zero gradient: sign of rounding noise (tests/test_parity_gpu.py)
            gu.check_digest(z, pre + '/theta', nm, model._layout.view(got['theta'], nm), rtol=RTOL if e <= RTOL / 10 else GOLDEN_BAND['F0'],
                            what='D0')
        # the discriminator's Adam step: the UPDATE theta - theta_before against the recorded one.  Adam's step is a smooth function
        # of the gradients seen so far (each within RTOL, asserted above): relative error <= 2 RTOL per step taken, plus the rounding of
        # theta itself seen at the update's size (2 u ||theta|| / ||update||)
        for nm, lo, hi in (('linear.weight', 0, C * d), ('linear.bias', C * d, C * d + C)):
            ref = z['%s/dtheta/%s' % (pre, nm)].reshape(-1).astype(np.float64)
            before = (z['disc_theta0/' + nm] if it == 0 else z['%s/%d/dtheta/%s' % (mode, it - 1, nm)]).reshape(-1).astype(np.float64)
            upd_ref, upd = ref - before, got['dtheta'][lo:hi].cpu().numpy().astype(np.float64) - before
            err = float(np.linalg.norm(upd - upd_ref) / np.linalg.norm(upd_ref))
            tol = 2 * RTOL * (it + 1) + 2 * U * float(np.linalg.norm(ref) / np.linalg.norm(upd_ref))
            print('%s discriminator update %s rel err %.3e (tolerance %.2e, update / theta %.2e)'
                  % (pre, nm, err, tol, float(np.linalg.norm(upd_ref) / np.linalg.norm(ref))))
            assert err <= tol, (pre, nm, err)
        mine = printed[it].split(' TOTAL TIME:')[0]
        print('line  ', mine)
        print('record', du.line(z, mode, it))
        lines_ok = lines_ok and mine == du.line(z, mode, it)
    assert lines_ok


def test_moving_the_module_keeps_its_gradients():
    import mtl_amd
    disc = mtl_amd.Discriminator(8, 3)
    disc.flat_grad.copy_(torch.arange(27.0))
    disc.to_copy_grad()
    disc = disc.cuda()
    assert disc.flat_grad.is_cuda and torch.equal(disc.flat_grad.cpu(), torch.arange(27.0)) and disc.copy_grad[1].is_cuda
    assert disc.linear.bias.grad.data_ptr() == disc.flat_grad.data_ptr() + 4 * 24
    assert torch.equal(disc.cpu().flat_grad, torch.arange(27.0))


def test_the_seam_is_inert():
    z, cfg, spec, mtl_amd, args, vocab, model, disc = _setup('adversarial')
    model, disc = model.cuda(), disc.cuda()
    tr, _ = gu.batches_for(cfg, spec, 0, z['data_call_index'])
    x, lens, y = tr[1]
    g1, g2 = torch.zeros_like(model.flat_grad), torch.zeros_like(model.flat_grad)
    model.pass_forward(x.cuda(), lens, y)
    model.pass_backward(g1, 1.0)
    model.pass_forward(x.cuda(), lens, y)
    enc = model.engine.encoder_output()
    assert tuple(enc.shape) == (spec['k'], spec['T'] // 4, cfg['dim_model'])
    disc.head_forward(enc, 1, True)
    seen = []
    model.pass_backward(g2, 1.0, dmem_hook=lambda dmem: (seen.append(tuple(dmem.shape)), disc.head_backward(0.0, 0.0, dmem)))
    assert seen == [(spec['k'] * (spec['T'] // 4), cfg['dim_model'])]
    assert float(g1.abs().sum()) > 0 and torch.equal(g1, g2)
    # with a weight the head's gradient does arrive in the model's
    model.pass_forward(x.cuda(), lens, y)
    disc.head_forward(model.engine.encoder_output(), 1, True)
    g3 = torch.zeros_like(g1)
    model.pass_backward(g3, 1.0, dmem_hook=lambda dmem: disc.head_backward(0.5, 1.0, dmem))
    assert not torch.equal(g1, g3)
    # task-batched passes do not take a hook
    eng, L = model.engine, model._layout
    meta = eng.prepare_tasks([(b[1], b[2]) for b in tr], spec['k'], spec['T'])
    eng.forward_device(model.flat_parameters, torch.cat([b[0] for b in tr]).cuda(), meta)
    stack = torch.zeros(len(tr) * L.total, device='cuda')
    with pytest.raises(ValueError, match='single-task'):
        eng.backward(stack, 1.0, sG=L.total, dmem_hook=lambda dmem: None)
    eng.backward(stack, 1.0, sG=L.total)
    assert float(stack.abs().sum()) > 0


def test_forward_one_batch_tuples_and_one_backward_through_both(capsys):
    """joint_trainer.py:25-91 through autograd: the 4- and 5-tuples, and (tr + w disc + enc_l).backward() giving the gradients the
    trainer's fused path gives (the same kernels; the encoder-output gradient takes one more addition on the way)."""
    z, cfg, spec, mtl_amd, args, vocab, model, disc = _setup('adversarial')
    model, disc = model.cuda(), disc.cuda()
    x, lens, y = gu.batches_for(cfg, spec, 0, z['data_call_index'])[0][2]
    tr = mtl_amd.JointTrainer()
    tl = (y != 0).sum(1).to(torch.int32)
    out4 = tr.forward_one_batch(model, vocab, x.cuda(), y.cuda(), lens.float() / x.shape[3], lens, tl, 0.0, 'ce', discriminator=disc,
                                accent_id=2, multi_task=True)
    assert len(out4) == 4
    model.zero_grad()
    disc.zero_grad()
    loss, cer, nchar, d_loss, e_loss = tr.forward_one_batch(model, vocab, x.cuda(), y.cuda(), lens.float() / x.shape[3], lens, tl, 0.0, 'ce',
                                                            discriminator=disc, accent_id=2)
    assert float(out4[3]) == float(d_loss)
    (loss / 3 + 0.5 * d_loss / 3 + e_loss / 3).backward()
    g_auto, dg_auto = model.flat_grad.clone(), disc.flat_grad.clone()
    g = torch.zeros_like(g_auto)
    disc.zero_grad()
    o = model.pass_forward(x.cuda(), lens, y)
    losses = disc.head_forward(model.engine.encoder_output(), 2, True)
    model.pass_backward(g, 1.0 / 3, dmem_hook=lambda dmem: disc.head_backward(0.5 / 3, 1.0 / 3, dmem))
    assert float(losses[0]) == float(d_loss) and float(losses[1]) == float(e_loss) and float(o['loss'][0]) == pytest.approx(float(loss), rel=1e-6)
    assert float((g - g_auto).norm() / g.norm()) < 1e-5
    assert float((disc.flat_grad - dg_auto).norm() / dg_auto.norm()) < 1e-5


def test_train_end_to_end_and_resume_from_checkpoints(tmp_path):
    from tests.test_trainer_gpu import _ListDataset
    z, cfg, spec, mtl_amd, args, vocab, model, disc = _setup('adversarial_decay', name='e2e', folder=str(tmp_path))
    args.save_every = 1
    model, disc = model.cuda(), disc.cuda()
    V = cfg['vocab_size']
    loaders = [mtl_amd.AudioDataLoader(vocab.PAD_ID, dataset=_ListDataset(7, 4, V), batch_size=4)]
    tasks = [mtl_amd.SyntheticTask(m, 2, 64, 8, V, variable=True) for m in range(3)]
    tr = mtl_amd.JointTrainer()
    tr.train(model, vocab, tasks, loaders, 'ce', 0, 2, args, evaluate_every=1, early_stop='loss,5', discriminator=disc)
    folder = os.path.join(str(tmp_path), 'e2e')
    assert set(os.listdir(folder)) >= {'epoch_1.th', 'epoch_2.th', 'best_model.th', 'epoch_1_discriminator.th', 'epoch_2_discriminator.th',
                                       'best_discriminator.th'}
    raw = mtl_amd.functions.load_checkpoint_dict(os.path.join(folder, 'epoch_2.th'))
    assert sorted(raw) == ['args', 'epoch', 'metrics', 'model_state_dict', 'opt', 'vocab']              # the model's file is the model's
    m2, v2, opt2, epoch, metrics, a2 = mtl_amd.load_joint_model(os.path.join(folder, 'epoch_2.th'))
    d2, optd2 = mtl_amd.load_discriminator(os.path.join(folder, 'epoch_2_discriminator.th'))
    assert d2.flat_parameters.is_cuda and torch.equal(d2.flat_parameters, disc.flat_parameters)
    assert not torch.equal(d2.flat_parameters.cpu(), torch.cat([torch.from_numpy(z['disc_theta0/linear.weight']).reshape(-1),
                                                                torch.from_numpy(z['disc_theta0/linear.bias'])]))
    assert int(optd2.state_dict()['state'][0]['step']) == 2
    # the next iteration: resumed and uninterrupted agree exactly (deterministic kernels, the same Adam states)
    batches = [(b[0], b[1], None, b[2], None) for b in gu.batches_for(cfg, spec, 1, z['data_call_index'])[0]]
    resumed = mtl_amd.JointTrainer()
    resumed.beta = tr.beta
    r2 = resumed.run_iteration(m2, vocab, batches, 3, mtl_amd.FlatAdam.from_torch(m2, opt2), args, discriminator=d2, opt_disc=optd2)
    r1 = tr.run_iteration(model, vocab, batches, 3, tr.opt, args, discriminator=disc, opt_disc=tr.opt_disc)
    assert r1 == r2 and tr.task_losses == resumed.task_losses and len(r1) == 5
    assert torch.equal(d2.flat_parameters, disc.flat_parameters) and torch.equal(m2.flat_parameters, model.flat_parameters)


@pytest.mark.parametrize('B,C', [(1, 1), (5, 3), (300, 64)])
def test_losses_on_leaf_logits(B, C):
    import mtl_amd
    g = torch.Generator().manual_seed(B + C)
    logits = 3.0 * torch.randn(B, C, generator=g)
    accent, a, b = C // 2, 0.7, 1.3
    zero = torch.zeros(B, C, dtype=torch.float64)
    z64 = logits.double()
    ce = (torch.logsumexp(z64, 1) - z64[:, accent]).mean()
    mse = ((z64 - 1.0 / C) ** 2).mean()
    ce_b, mse_b = du.losses_bound(z64, zero, 1)
    pred = logits.cuda().requires_grad_(True)
    d_loss, e_loss = mtl_amd.calculate_adversarial(pred, accent)
    _within(d_loss, ce, ce_b, 'CE')
    _within(e_loss, mse, mse_b, 'MSE')
    (a * d_loss + b * e_loss).backward()
    want = du.dlogit(z64, accent, 1, a, b)
    # the two loss gradients are scaled and added by autograd: a few more roundings at the terms' magnitude
    bound = du.dlogit_bound(z64, zero, accent, 1, a, b) + 4 * U * (du.dlogit(z64, accent, 1, a, 0.0).abs() + du.dlogit(z64, accent, 1, 0.0, b).abs())
    _within(pred.grad, want, bound, 'dlogits')
    # multi-task form, on a non-leaf
    leaf = logits.cuda().requires_grad_(True)
    m_loss = mtl_amd.calculate_multi_task(leaf * 1.0, accent)
    assert float(m_loss) == float(d_loss)
    m_loss.backward()
    _within(leaf.grad, du.dlogit(z64, accent, 0, 1.0, 0.0), du.dlogit_bound(z64, zero, accent, 0, 1.0, 0.0) + 2 * U * du.dlogit(z64, accent, 0, 1.0, 0.0).abs(), 'CE dlogits')
