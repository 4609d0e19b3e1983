"""CPU: the accent discriminator's public surface (names, state dict, initial values, checkpoints), the argument validation of its
entry points without a device, and the fp64 restatement of tests/disc_util.py against the reference's record tests/golden/D0.npz."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import disc_util as du

LOSS_RTOL = 2e-6        # loss scalars against a reference golden on the CPU (tests/test_oracle_golden.py)
GRAD_RTOL = 2e-5        # gradient tensors against a reference golden on the CPU (tests/test_oracle_golden.py, check_digest's norm-wise error)


@pytest.fixture(scope='module')
def mtl_amd():
    import __graft_entry__ as ge
    return ge.build()


def _args(**kw):
    base = dict(dim_model=128, num_class=3, lr=1e-3, lr_disc=1e-3, save_folder='/tmp/mtl_disc', name='disc', cuda=False, loss='ce')
    base.update(kw)
    return argparse.Namespace(**base)


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return float((got - ref).norm() / ref.norm())


def test_names_are_exported(mtl_amd):
    for name in ('Discriminator', 'init_discriminator_model', 'save_discriminator', 'load_discriminator', 'calculate_adversarial',
                 'calculate_multi_task'):
        assert callable(getattr(mtl_amd, name)), name
    assert 'no discriminator' not in mtl_amd.JointTrainer.__doc__


def test_state_dict_and_initial_values_match_nn_linear(mtl_amd):
    torch.manual_seed(11)
    disc = mtl_amd.init_discriminator_model(_args(dim_model=132, num_class=5))
    after = torch.rand(3)
    torch.manual_seed(11)
    lin = torch.nn.Linear(132, 5)
    assert torch.equal(after, torch.rand(3))                               # the same RNG draws
    sd = disc.state_dict()
    assert list(sd.keys()) == ['linear.weight', 'linear.bias']
    assert tuple(sd['linear.weight'].shape) == (5, 132) and tuple(sd['linear.bias'].shape) == (5,)
    assert torch.equal(sd['linear.weight'], lin.weight) and torch.equal(sd['linear.bias'], lin.bias)
    # parameters and gradients are views into one flat buffer each
    assert disc.linear.weight.data_ptr() == disc.flat_parameters.data_ptr()
    assert disc.linear.bias.data_ptr() == disc.flat_parameters.data_ptr() + 4 * 5 * 132
    assert disc.linear.weight.grad.data_ptr() == disc.flat_grad.data_ptr()
    for fn in ('init_copy_grad_', 'zero_copy_grad', 'add_copy_grad', 'to_copy_grad', 'from_copy_grad'):
        assert callable(getattr(disc, fn))
    disc.flat_grad.fill_(2.0)
    disc.to_copy_grad()
    disc.add_copy_grad()
    disc.zero_grad()
    disc.from_copy_grad()
    assert float(disc.linear.bias.grad.sum()) == 4.0 * 5
    # an _apply that moves nothing (.float(), .cpu() on a CPU module) keeps the buffers and what they have accumulated
    ptr = disc.flat_grad.data_ptr()
    disc.float().cpu()
    assert disc.flat_grad.data_ptr() == ptr and disc.linear.weight.grad.data_ptr() == ptr and float(disc.flat_grad.min()) == 4.0
    with pytest.raises(RuntimeError, match='needs an MI355X'):
        disc(torch.zeros(2, 132))
    with pytest.raises(RuntimeError, match='needs an MI355X'):
        mtl_amd.calculate_adversarial(torch.zeros(2, 5), 1)


def test_checkpoint_round_trip(mtl_amd, tmp_path):
    args = _args(save_folder=str(tmp_path), name='ckpt')
    torch.manual_seed(5)
    disc = mtl_amd.init_discriminator_model(args)
    opt = torch.optim.Adam(disc.parameters(), lr=args.lr_disc)
    disc.flat_grad.copy_(torch.linspace(-1, 1, disc.flat_grad.numel()))
    opt.step()
    p1 = mtl_amd.save_discriminator(disc, 7, opt, args, best_model=False)
    p2 = mtl_amd.save_discriminator(disc, 7, opt, args, best_model=True)
    assert sorted(os.listdir(os.path.join(str(tmp_path), 'ckpt'))) == ['best_discriminator.th', 'epoch_7_discriminator.th']
    assert os.path.basename(p1) == 'epoch_7_discriminator.th' and os.path.basename(p2) == 'best_discriminator.th'
    raw = torch.load(p1, weights_only=False)
    assert sorted(raw) == ['args', 'epoch', 'model_state_dict', 'opt'] and raw['epoch'] == 7
    assert list(raw['model_state_dict']) == ['linear.weight', 'linear.bias'] and isinstance(raw['opt'], torch.optim.Adam)
    d2, opt2 = mtl_amd.load_discriminator(p1)
    assert torch.equal(d2.flat_parameters, disc.flat_parameters)
    assert d2.linear.weight.data_ptr() == d2.flat_parameters.data_ptr()
    s1, s2 = opt.state_dict(), opt2.state_dict()
    assert s2['param_groups'][0]['lr'] == args.lr_disc and len(s2['state']) == 2
    for k in s1['state']:
        assert int(s2['state'][k]['step']) == 1
        assert torch.equal(s1['state'][k]['exp_avg'], s2['state'][k]['exp_avg'])
        assert torch.equal(s1['state'][k]['exp_avg_sq'], s2['state'][k]['exp_avg_sq'])


def test_entry_points_reject_bad_arguments_without_a_device(mtl_amd):
    L = mtl_amd._lib.lib()
    p = 4096                                    # a non-null, 16-byte aligned stand-in: validation happens before any launch
    ws = L.mtl_disc_workspace(2, 17, 128)
    assert ws > 0 and L.mtl_disc_workspace(1, 1, 4) > 0

    def fwd(enc=p, B=2, T=17, d=128, W=p, bias=p, C=3, accent=0, mode=0, pooled=p, logits=p, losses=p, wsp=p, nbytes=ws):
        return L.mtl_disc_fwd(None, enc, B, T, d, W, bias, C, accent, mode, pooled, logits, losses, wsp, nbytes)

    def bwd(pooled=p, logits=p, W=p, accent=0, B=2, T=17, d=128, C=3, mode=0, dW=p, dbias=p, denc=p):
        return L.mtl_disc_bwd(None, pooled, logits, W, accent, B, T, d, C, mode, 1.0, 0.0, dW, dbias, denc)
    for kw in (dict(C=65), dict(C=0), dict(d=130), dict(B=0), dict(T=0), dict(accent=3), dict(mode=2), dict(enc=None), dict(W=None),
               dict(bias=None), dict(pooled=None), dict(logits=None), dict(losses=None), dict(wsp=None), dict(nbytes=ws - 1)):
        assert fwd(**kw) == -22, kw
    for kw in (dict(C=65), dict(d=130), dict(B=0), dict(T=0), dict(accent=-1), dict(pooled=None), dict(logits=None), dict(W=None),
               dict(dW=None), dict(dbias=None), dict(denc=None)):
        assert bwd(**kw) == -22, kw
    assert L.mtl_disc_workspace(2, 17, 130) == 0 and L.mtl_disc_workspace(0, 17, 128) == 0
    assert L.mtl_disc_loss_fwd(None, p, 2, 65, 0, 0, p) == -22 and L.mtl_disc_loss_fwd(None, None, 2, 3, 0, 0, p) == -22
    assert L.mtl_disc_loss_bwd(None, p, 2, 3, 3, 1, 1.0, 1.0, p) == -22
    assert L.mtl_disc_bwd_dlogits(None, p, None, p, 2, 17, 128, 3, p, p, p) == -22
    # one more chunk = more workspace: a chunk is MTL_DISC_CHUNK = 16 rows
    assert L.mtl_disc_workspace(2, 16, 128) == 2 * 128 * 4 and L.mtl_disc_workspace(2, 17, 128) == 2 * 2 * 128 * 4


@pytest.mark.parametrize('mode', du.MODES)
def test_restatement_reproduces_the_reference_record(mode):
    """From D0's recorded pooled sums the restatement gives the reference's logits, disc / enc_l and, summed over the tasks with the
    trainer's weights a = w / n, b = 1 / n, its discriminator gradients: fixture and restatement pinned against each other."""
    z, cfg, spec = du.load_d0()
    n, C = spec['n_tasks'], spec['num_class']
    adv = 0 if mode == 'multitask' else 1
    W = torch.from_numpy(z['disc_theta0/linear.weight'])
    bias = torch.from_numpy(z['disc_theta0/linear.bias'])
    for it in range(spec['iters']):
        dW, db = torch.zeros(W.shape, dtype=torch.float64), torch.zeros(bias.shape, dtype=torch.float64)
        for m in range(n):
            key = '%s/%d/%d' % (mode, it, m)
            pooled = torch.from_numpy(z[key + '/pooled'])
            logits, ce, mse = du.head(pooled, W, bias, m, adv)
            assert _rel(logits, z[key + '/logits']) <= GRAD_RTOL, key
            # LOSS_RTOL on the loss, plus what logits held to GRAD_RTOL (asserted above) can move it by: see ce_tolerance
            tol = du.ce_tolerance(z[key + '/disc'], z[key + '/logits'], m, LOSS_RTOL, GRAD_RTOL)
            print(key, 'CE %.7e vs %.7e, tolerance %.2e' % (float(ce), float(z[key + '/disc']), tol))
            assert abs(float(ce) - float(z[key + '/disc'])) <= tol, key
            w = float(z[key + '/w'])
            assert abs(w * float(ce) - float(z[key + '/disc_logged'])) <= w * tol + 2 * du.U * abs(w * float(ce)), key
            if adv:
                assert abs(float(mse) - float(z[key + '/enc_l'])) <= LOSS_RTOL * abs(float(mse)), key
            _, gW, gb, _ = du.grads(pooled, logits, W, m, adv, w / n, 1.0 / n)
            dW += gW
            db += gb
        assert _rel(dW, z['%s/%d/dG/linear.weight' % (mode, it)]) <= GRAD_RTOL
        assert _rel(db, z['%s/%d/dG/linear.bias' % (mode, it)]) <= GRAD_RTOL
        # the record's own consistency: the discriminator's Adam step, and the printed line
        W2, b2 = torch.from_numpy(z['%s/%d/dtheta/linear.weight' % (mode, it)]), torch.from_numpy(z['%s/%d/dtheta/linear.bias' % (mode, it)])
        assert float((W2 - W).abs().max()) <= 3.2 * spec["lr_disc"] and float((W2 - W).abs().max()) > 0
        line = du.line(z, mode, it)
        assert line.startswith('(Iteration %d) TRAIN LOSS:' % (it + 1)) and ('ENC LOSS:' in line) == bool(adv) and 'DISC LOSS:' in line
        tot = sum(float(z['%s/%d/%d/disc_logged' % (mode, it, m)]) for m in range(n)) / n
        assert 'DISC LOSS:{:.4f}'.format(tot) in line
        W, bias = W2, b2


def test_train_with_a_discriminator_on_a_cpu_model_needs_the_device(mtl_amd):
    from tests import golden_util as gu
    from tests.test_parity_gpu import make
    z, cfg, spec = gu.load('F0')
    _, args, vocab, model = make(cfg, spec)
    args.num_class, args.lr_disc, args.adversarial, args.multitask, args.beta_decay = 3, 1e-3, False, True, False
    disc = mtl_amd.init_discriminator_model(args)
    tasks = [mtl_amd.SyntheticTask(m, 2, 64, 8, cfg['vocab_size'], variable=True) for m in range(3)]
    with pytest.raises(RuntimeError, match='needs an MI355X'):
        mtl_amd.JointTrainer().train(model, vocab, tasks, [], 'ce', 0, 1, args, evaluate_every=10 ** 9, early_stop='cer,200',
                                     discriminator=disc)
