"""Generate tests/golden/D0.npz: joint training with the accent discriminator (joint_train.py --multitask / --adversarial
[--beta-decay]; trainer/asr/joint_trainer.py:25-91, 197-271, modules/discriminator.py, utils/metrics.py:164-199) of the REAL reference.

Runs only where the reference checkout exists (it imports the reference's own modules through oracle/make_golden.py's bootstrap,
never copies them).  Model and batches: fixture F0 (enc1/dec1 d128, 3 tasks, k = 2, T = 64 so T' = 16, L = 8, variable lengths), Adam
at lr 1e-3 like J0; the Discriminator (num_class 3, lr_disc 1e-3) is built right after the model from the same RNG stream.  Each of
the three modes runs two iterations of the reference's task loop inside ONE train() call (it builds fresh optimizers per call).

    python tools/make_golden_discriminator.py
"""
import argparse
import contextlib
import io
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import bootstrap_reference, FIXTURES, tensor_digest  # noqa: E402

SPEC = dict(num_class=3, lr=1e-3, lr_disc=1e-3, iters=2)
MODES = {'multitask': dict(multitask=True, adversarial=False, beta_decay=False),
         'adversarial': dict(multitask=False, adversarial=True, beta_decay=False),
         'adversarial_decay': dict(multitask=False, adversarial=True, beta_decay=True)}


def pack_compact(prefix, named, store):
    """oracle.make_golden.pack with one array per FIELD instead of one per tensor and field (an .npz entry costs ~300 bytes of
    headers; 12 records of 68 tensors would be mostly headers): tests/disc_util.py expands it back into pack's keys."""
    tmp = {}
    names = []
    for name, t in named:
        names.append(name)
        for k, v in tensor_digest(t, full_below=256, nsample=64).items():
            tmp['%s/%s' % (name, k)] = v
    data = [tmp[n + '/full'] if n + '/full' in tmp else tmp[n + '/sample'] for n in names]
    store[prefix + '/l2'] = np.array([tmp[n + '/l2'] for n in names], dtype=np.float64)
    store[prefix + '/sum'] = np.array([tmp[n + '/sum'] for n in names], dtype=np.float64)
    store[prefix + '/numel'] = np.array([tmp[n + '/numel'] for n in names], dtype=np.int64)
    store[prefix + '/step'] = np.array([int(tmp.get(n + '/step', 0)) for n in names], dtype=np.int64)      # 0: the whole tensor
    store[prefix + '/offsets'] = np.cumsum([0] + [a.size for a in data]).astype(np.int64)
    store[prefix + '/data'] = np.concatenate(data).astype(np.float32)


def run_mode(torch, mode, flags, store):
    from utils.data import Vocab
    from utils.functions import init_transformer_model, init_discriminator_model
    from trainer.asr.joint_trainer import JointTrainer
    from oracle.refimpl import synth_batch
    f0 = FIXTURES['F0']
    cfg, n, k, T, L = f0['cfg'], f0['n_tasks'], f0['k'], f0['T'], f0['L']
    vocab = Vocab()
    for i in range(cfg['vocab_size'] - 4):
        vocab.add_token(chr(0x4e00 + i))
        vocab.add_label(chr(0x4e00 + i))
    args = argparse.Namespace(
        feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
        num_enc_layers=cfg['num_enc_layers'], num_dec_layers=cfg['num_dec_layers'], num_heads=cfg['num_heads'],
        dim_model=cfg['dim_model'], dim_key=cfg['dim_key'], dim_value=cfg['dim_value'], dim_inner=cfg['dim_inner'],
        dim_emb=cfg['dim_emb'], src_max_len=cfg['src_max_len'], tgt_max_len=cfg['tgt_max_len'], dropout=0.0,
        emb_trg_sharing=False, label_smoothing=0.0, name='golden_D0', lr=SPEC['lr'], lr_disc=SPEC['lr_disc'],
        num_class=SPEC['num_class'], k_train=k, cuda=False, clip=False, max_norm=400, save_every=10 ** 9,
        save_folder='/tmp/golden_ckpt', loss='ce', **flags)
    torch.manual_seed(123456)
    torch.set_num_threads(8)
    model = init_transformer_model(args, vocab, is_factorized=False, r=cfg['r'])
    disc = init_discriminator_model(args)
    names = [nm for nm, _ in model.named_parameters()]
    dnames = [nm for nm, _ in disc.named_parameters()]
    if 'param_names' not in store:
        store['param_names'] = np.array(names)
        store['disc_param_names'] = np.array(dnames)
        for nm, p in disc.named_parameters():
            store['disc_theta0/' + nm] = p.detach().numpy().copy()

    class FakeTask:
        def __init__(self, task):
            self.task, self.calls = task, 0

        def sample(self, k_train, k_valid, manifest_id):
            it = self.calls
            self.calls += 1
            if it > SPEC['iters'] + 1:          # (the reference's loop swallows exceptions and fetches again: never spin here)
                sys.stderr.write(text.getvalue()[-4000:] + '\nthe reference iteration failed\n')
                os._exit(1)
            out = []
            for part in (0, 1):
                x, lens, y = synth_batch(1000 * it + 10 * self.task + part, k, T, L, cfg['vocab_size'], f0['variable'])
                out.append((x, lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32)))
            return tuple(out)

    text = io.StringIO()
    tasks = [FakeTask(m) for m in range(n)]
    pooled, logits, fobs = [], [], []

    def disc_hook(mod, inp, outp):
        pooled.append(inp[0].detach().clone())
        logits.append(outp.detach().clone())
    disc.register_forward_hook(disc_hook)
    trainer = JointTrainer()
    orig_fob = trainer.forward_one_batch

    def fob(*a, **kw):
        out = orig_fob(*a, **kw)
        fobs.append([float(v.detach()) for v in (out[0], out[3]) + tuple(out[4:5])] + [int(out[1]), int(out[2]), int(kw['accent_id'])])
        return out
    trainer.forward_one_batch = fob
    model_ids = {id(p) for p in model.parameters()}
    steps = {'model': [], 'disc': []}
    orig_step = torch.optim.Adam.step

    def spy_step(self_opt, *a, **kw):
        which = 'model' if id(self_opt.param_groups[0]['params'][0]) in model_ids else 'disc'
        mod = model if which == 'model' else disc
        grads = [p.grad.detach().clone() for p in mod.parameters()]
        out = orig_step(self_opt, *a, **kw)
        steps[which].append((grads, [p.detach().clone() for p in mod.parameters()]))
        return out
    torch.optim.Adam.step = spy_step
    try:
        with contextlib.redirect_stdout(text):
            trainer.train(model, vocab, tasks, [], 'ce', 0, SPEC['iters'], args, evaluate_every=10 ** 9, early_stop='cer,200',
                          discriminator=disc)
    finally:
        torch.optim.Adam.step = orig_step
    lines = [ln for ln in text.getvalue().split('\n') if ln.startswith('(Iteration')]
    assert len(lines) == SPEC['iters'] and len(fobs) == n * SPEC['iters'] == len(pooled), text.getvalue()
    assert len(steps['model']) == len(steps['disc']) == SPEC['iters']
    beta = 1.0
    for it in range(SPEC['iters']):
        pre = '%s/%d' % (mode, it)
        store[pre + '/line'] = np.frombuffer(re.sub(r' TOTAL TIME:.*$', '', lines[it]).encode(), dtype=np.uint8)
        for m in range(n):
            rec = fobs[it * n + m]
            assert rec[-1] == m
            if flags['multitask']:
                w = 1.0
            elif flags['beta_decay']:
                beta = beta * 0.99997
                w = beta
            else:
                w = 0.5
            key = '%s/%d' % (pre, m)
            store[key + '/tr'] = np.float64(rec[0])
            store[key + '/disc'] = np.float64(rec[1])
            store[key + '/disc_logged'] = np.float64(float(torch.tensor(rec[1], dtype=torch.float32) * w))
            store[key + '/w'] = np.float64(w)
            if not flags['multitask']:
                store[key + '/enc_l'] = np.float64(rec[2])
            store[key + '/cer'] = np.array(rec[-3:-1], dtype=np.int64)
            store[key + '/pooled'] = pooled[it * n + m].numpy().copy()
            store[key + '/logits'] = logits[it * n + m].numpy().copy()
        for nm, g in zip(dnames, steps['disc'][it][0]):
            store['%s/dG/%s' % (pre, nm)] = g.numpy().copy()
        pack_compact(pre + '/G', zip(names, steps['model'][it][0]), store)
        pack_compact(pre + '/theta', zip(names, steps['model'][it][1]), store)
        for nm, t in zip(dnames, steps['disc'][it][1]):
            store['%s/dtheta/%s' % (pre, nm)] = t.numpy().copy()
    print(mode, [re.sub(r' TOTAL TIME:.*$', '', ln) for ln in lines])


def main():
    torch = bootstrap_reference()
    # utils/metrics.py:174-175 builds its targets as torch.cuda.*Tensor: in this process those two are the CPU constructors
    torch.cuda.LongTensor, torch.cuda.FloatTensor = torch.LongTensor, torch.FloatTensor
    f0 = FIXTURES['F0']
    cfg = f0['cfg']
    store = {'cfg_keys': np.array(sorted(cfg.keys())), 'cfg_vals': np.array([cfg[k_] for k_ in sorted(cfg.keys())], dtype=np.int64),
             'spec': np.array([f0['k'], f0['T'], f0['L'], f0['n_tasks'], SPEC['iters'], 1], dtype=np.int64),
             'lr': np.float64(SPEC['lr']), 'meta_lr': np.float64(SPEC['lr']), 'lr_disc': np.float64(SPEC['lr_disc']),
             'num_class': np.int64(SPEC['num_class']), 'data_call_index': np.arange(SPEC['iters'], dtype=np.int64),
             'modes': np.array(sorted(MODES))}
    for mode, flags in MODES.items():
        run_mode(torch, mode, flags, store)
    out = os.path.join(ROOT, 'tests', 'golden', 'D0.npz')
    np.savez_compressed(out, **store)
    print('D0 written: %d arrays, %d bytes' % (len(store), os.path.getsize(out)))


if __name__ == '__main__':
    main()
