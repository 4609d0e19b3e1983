"""MI355X: the model shape of --feat logfbank (80 bands -> 20 pooled rows x 128 channels, dim_input 2560) through the whole path: loss
and every gradient tensor against the live oracle's SpeechTransformer(freq_bins=80) on ragged shapes in both convolution modes, one
meta-iteration on LogFBankDataset device batches against the same features from host tensors, and the checkpoint round trip.  The
method and the bounds of the single-pass comparison are those of tests/test_parity_gpu.py::_pass_parity at 161 bins, restated here."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import fbank_util as fu
from tests import golden_util as gu

pytestmark = pytest.mark.gpu
RTOL = 1e-4          # north_star: fp32 loss and gradients within 1e-4 relative
F = 80


def make(cfg, spec, name='logfbank', **kw):
    import mtl_amd
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='logfbank', dim_input=161,
                              dropout=0.0, emb_trg_sharing=False, label_smoothing=0.0, name=name, lr=spec['lr'],
                              meta_lr=spec['meta_lr'], k_train=spec['k'], k_valid=spec['k'], clip=False, max_norm=400,
                              save_every=10 ** 9, save_folder='/tmp/mtl_ckpt', cuda=True,
                              **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    for k, v in kw.items():
        setattr(args, k, v)
    vocab = mtl_amd.synthetic_vocab(cfg['vocab_size'])
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    assert args.dim_input == 2560 and model.encoder.input_linear.in_features == 2560
    return mtl_amd, args, vocab, model


def _oracle(cfg):
    from oracle import refimpl as R
    torch.manual_seed(123456)
    m = R.SpeechTransformer(cfg['vocab_size'], cfg['num_enc_layers'], cfg['num_dec_layers'], cfg['num_heads'], cfg['dim_model'],
                            cfg['dim_key'], cfg['dim_value'], cfg['dim_inner'], cfg['dim_emb'], cfg['src_max_len'], cfg['tgt_max_len'],
                            r=cfg.get('r', 100), freq_bins=F)
    m.train()
    return m


def _pass_parity(model, oracle, batch, theta, what, max_flips=8):
    """tests/test_parity_gpu.py::_pass_parity: one forward + backward of both implementations at IDENTICAL parameters.  (1) the
    free-running oracle: labels bit-exact, logits within 1e-5, loss within 1e-4, at most `max_flips` ReLU / max-pool decisions differ and
    each is a rounding near-tie; (2) the oracle with the device pass's own decisions replayed: EVERY gradient tensor within 1e-4."""
    from oracle import refimpl as R
    from oracle import branches
    x, lens, y = batch
    with torch.no_grad():
        for nm, p in oracle.named_parameters():
            p.copy_(model._layout.view(theta, nm).cpu())
    out = model.pass_forward(x.cuda(), lens, y, theta=theta)
    g = torch.zeros_like(model.flat_grad)
    model.pass_backward(g, 1.0)
    gates = branches.gates_from_engine(model.engine)
    with torch.no_grad():
        (pred_r, gold_r, hyp_r), pre = branches.oracle_trace(oracle, x, lens, y)
        loss_r = R.ce_loss(pred_r, gold_r)
    assert torch.equal(out['hyp'].cpu(), hyp_r) and torch.equal(out['gold'].cpu(), gold_r), what
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
    gn = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    errs = {nm: float((model._layout.view(g, nm).cpu() - t).norm() / max(float(t.norm()), 1e-4 * gn))
            for (nm, _), t in zip(oracle.named_parameters(), grads)}
    worst = max(errs, key=errs.get)
    print('%s: %d branch near-ties decided differently (margin %.1e); %d/%d gradient tensors within 1e-4, worst %.2e (%s)'
          % (what, flips, margin, sum(e < RTOL for e in errs.values()), len(errs), errs[worst], worst))
    assert errs[worst] < RTOL, (what, worst, errs[worst], flips)


@pytest.mark.parametrize('conv', ['h2', 'x3'])
@pytest.mark.parametrize('B,T,L,lens,tlens', [
    (1, 17, 1, [17], [1]),
    (3, 50, 5, [50, 13, 4], [5, 2, 1]),
    (2, 129, 12, [129, 65], [12, 7]),
])
def test_ragged_shapes_at_80_bands_against_live_oracle(B, T, L, lens, tlens, conv):
    z, cfg, spec = gu.load('F0')
    mtl_amd, args, vocab, model = make(cfg, spec)
    model = model.cuda()
    for e in model.engines:
        e.conv_mode, e.conv_x3, e.conv_h2 = conv, True, conv == 'h2'
    oracle = _oracle(cfg)
    assert [n for n, _ in oracle.named_parameters()] == [n for n, _ in model.named_parameters()]
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, 1, F, T, generator=g)
    y = torch.randint(4, cfg['vocab_size'], (B, L), generator=g)
    for i in range(B):
        x[i, :, :, lens[i]:] = 0
        y[i, tlens[i]:] = 0
    _pass_parity(model, oracle, (x, torch.tensor(lens, dtype=torch.int32), y), model.flat_parameters, 'logfbank %s B%d T%d' % (conv, B, T))


def _corpus(tmp_path, n=8):
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        y = fu.signal(('noise', 'tone', 'fade')[i % 3], 4000 + 900 * i, 200 + i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.rint(y.astype(np.float64) * 32768.0).astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


def test_meta_iteration_on_device_batches_equals_host_tensors_and_the_checkpoint_goes_round(tmp_path):
    z, cfg, spec = gu.load('F0')
    manifests = _corpus(tmp_path)
    losses = {}
    for mode in ('device', 'host'):
        mtl_amd, args, vocab, model = make(cfg, spec, name='fb_' + mode, save_folder=str(tmp_path), src_max_len=cfg['src_max_len'])
        model = model.cuda()
        audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.4)
        tasks = [mtl_amd.LogFBankDataset(vocab, args, audio_conf, manifest_filepath_list=manifests, normalize=True, is_train=True,
                                         seed=7 + m, device_batches=True) for m in range(2)]
        parts = [t.sample(2, 2, 0) for t in tasks]
        assert all(tr[0].is_cuda and tuple(tr[0].shape[:3]) == (2, 1, F) for tr, _ in parts)
        if mode == 'host':                                       # the same features, handed over as host tensors
            parts = [tuple((p[0].cpu(),) + tuple(p[1:]) for p in pair) for pair in parts]
            assert not parts[0][0][0].is_cuda
        inner = mtl_amd.FlatSGD(model, spec['lr'])
        model.zero_copy_grad()
        trainer = mtl_amd.TransientTrainer()
        reads = trainer.meta_iteration(model, vocab, [tr for tr, _ in parts], parts[-1][1], 2, inner, None, args)
        torch.cuda.synchronize()
        losses[mode] = [float(rd.loss[0]) for pair in reads for rd in pair]
        G = model._G.clone()
        assert bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
        losses[mode + '_G'] = G.cpu()
    print('logfbank meta-iteration losses:', losses['device'])
    assert len(losses['device']) == 4 and all(np.isfinite(v) and v > 0 for v in losses['device'])
    assert losses['device'] == losses['host'] and torch.equal(losses['device_G'], losses['host_G'])
    # the checkpoint of this model goes round through load_meta_model
    path = mtl_amd.save_meta_model(model, vocab, 1, torch.optim.SGD(model.parameters(), lr=args.lr),
                                   torch.optim.Adam(model.parameters(), lr=args.meta_lr), {'avg_valid_cer': 1.0}, args)
    m2, v2, _, _, epoch, _, a2 = mtl_amd.load_meta_model(path)
    assert epoch == 1 and a2.feat == 'logfbank' and a2.dim_input == 2560 and v2.id2label == vocab.id2label
    assert m2.encoder.input_linear.in_features == 2560 and next(m2.parameters()).is_cuda
    for (n1, p1), (n2, p2) in zip(model.named_parameters(), m2.named_parameters()):
        assert n1 == n2 and torch.equal(p1.cpu(), p2.cpu())
