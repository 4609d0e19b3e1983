"""tests/golden/N0.npz and tests/golden/N0.th.gz: a model the REAL reference builds with --feat_extractor none (utils/functions.py:
328-329 keeps the caller's dim_input; models/asr/transformer.py:93-94 views the (B, 1, F, T) batch as (B, F, T) and transposes it: the
encoder's input Linear runs on every frame, there is no convolution and no time reduction).

N0.npz: F0's model widths of oracle/make_golden.py (enc1 / dec1, d 128, inner 128, 8 heads of 16, r 100, V 64), dim_input 161, 3 tasks,
k 2, T 63, L 8, variable lengths, 2 --copy-grad meta-steps, recorded by make_golden.run_fixture;
  fz/...      the same record (one meta-step) of the model built with is_factorized=True, r 36, on 80 features per frame;
  joint/...   the loss trace of two JointTrainer iterations (no discriminator) on the dense model;
  decode/...  the reference's greedy (the first GREEDY_STEPS of Decoder.greedy_search's 300) and beam-3 (2-best) token sequences under
              the B0 perturbation of the vocabulary projection.
  manifest/.. the reference's beam search on each utterance of the two-utterance test set of tests/golden/N0_manifest/ (written here too);
  ckpt/...    a teacher-forced pass (pred, hyp) of the model saved in N0.th.gz on a seeded batch.
N0.th.gz: the reference's own save_meta_model of a tiny `none` model (width 64, 21 features; exact period-9 weight patterns, one Adam step).
The reference is imported through make_golden.bootstrap_reference(), never copied; only the two data files are committed.

    python tools/make_golden_featnone.py
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG      # noqa: E402
from oracle import refimpl as R           # noqa: E402

GREEDY_STEPS = 24
SPEC = dict(MG.FIXTURES['F0'], T=63, iters=2)
FZ = dict(r=36, dim_input=80, iters=1)
DECODE = dict(seed=500, k=3, T=63, L=8, beam_width=3, nbest=2, noise_seed=7, noise=0.5, eos_from=47, eos_gain=1.02, greedy_steps=GREEDY_STEPS)
JOINT = dict(k=2, T=63, L=8, n_tasks=3, lr=1e-3, iters=2)
# a two-utterance test set as a manifest (tests/golden/N0_manifest/: test.csv, one transcript file per utterance; the features of
# `uI.wav` are synth_batch(seeds[I], 1, T[I], L[I])): batches of one utterance, so every batch has a width of its own
MANIFEST = dict(seeds=[610, 611], T=[63, 41], L=[8, 5], beam_width=3, nbest=1, noise_seed=7, noise=0.5, eos_from=47, eos_gain=1.02)
CKPT = dict(seed=5, k=2, F=21, T=30, lens=[30, 11], L=5)


def _vocab(size):
    from utils.data import Vocab
    vocab = Vocab()
    for i in range(size - 4):
        vocab.add_token(chr(0x4e00 + i))
        vocab.add_label(chr(0x4e00 + i))
    return vocab


def _args(cfg, **over):
    a = dict(feat_extractor='none', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
             emb_trg_sharing=False, label_smoothing=0.0, name='golden_N0', cuda=False, is_factorized=False, r=cfg['r'])
    a.update({k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    a.update(over)
    return argparse.Namespace(**a)


def _frames(model, x):
    sz = x.size()
    return x.view(sz[0], sz[1] * sz[2], sz[3]).transpose(1, 2).contiguous()


def decode_records(torch, ref_init):
    """the reference's searches on the seeded `none` model with the B0 perturbation of decoder.output_linear"""
    cfg, sp = MG.FIXTURES['F0']['cfg'], DECODE
    vocab = _vocab(cfg['vocab_size'])
    x, lens, y = R.synth_batch(sp['seed'], sp['k'], sp['T'], sp['L'], cfg['vocab_size'], variable=True)
    out = {}
    for what, tgt_max_len in (('beam', cfg['tgt_max_len']), ('greedy', 320)):
        args = _args(dict(cfg, tgt_max_len=tgt_max_len), beam_width=sp['beam_width'], beam_nbest=sp['nbest'])
        torch.manual_seed(123456)
        torch.set_num_threads(8)
        model = ref_init(args, vocab, is_factorized=False, r=cfg['r'])
        g = torch.Generator().manual_seed(sp['noise_seed'])
        W = model.decoder.output_linear.weight
        W.data += sp['noise'] * torch.randn(W.shape, generator=g)
        W.data[2] = sp['eos_gain'] * W.data[sp['eos_from']]
        model.eval()
        with torch.no_grad():
            if what == 'beam':
                enc, _ = model.encoder(_frames(model, x), lens)
                ids, _strs = model.decoder.beam_search(enc, args, beam_width=sp['beam_width'], nbest=sp['nbest'], start_token=vocab.SOS_ID)
                arr = np.full((len(ids), max(len(r_) for r_ in ids)), -1, dtype=np.int64)
                for i, r_ in enumerate(ids):
                    arr[i, :len(r_)] = r_
                out['decode/beam_ids'] = arr
            else:
                steps = []
                hook = model.decoder.output_linear.register_forward_hook(
                    lambda m, i, o: steps.append(o[:, -1].max(dim=1)[1].clone()) if o.size(0) == sp['k'] else None)
                model.evaluate(x, lens, y, args, beam_search=False, start_token=vocab.SOS_ID)
                hook.remove()
                assert len(steps) == 300
                out['decode/greedy_ids'] = torch.stack(steps[:GREEDY_STEPS]).numpy().astype(np.int64)      # (steps, B)
    out['decode/spec'] = np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8)
    return out


def joint_record(torch, ref_init):
    """two JointTrainer iterations (trainer/asr/joint_trainer.py, no discriminator) inside one train() call: the per-forward losses"""
    from trainer.asr.joint_trainer import JointTrainer
    cfg, sp = MG.FIXTURES['F0']['cfg'], JOINT
    vocab = _vocab(cfg['vocab_size'])
    args = _args(cfg, name='golden_N0J', lr=sp['lr'], k_train=sp['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/golden_ckpt')
    torch.manual_seed(123456)
    torch.set_num_threads(8)
    model = ref_init(args, vocab, is_factorized=False, r=cfg['r'])
    names = [n for n, _ in model.named_parameters()]

    class FakeTask:
        def __init__(self, task):
            self.task, self.calls = task, 0

        def sample(self, k_train, k_valid, manifest_id):
            it = self.calls
            self.calls += 1
            out = []
            for part in (0, 1):
                x, lens, y = R.synth_batch(1000 * it + 10 * self.task + part, sp['k'], sp['T'], sp['L'], cfg['vocab_size'], True)
                out.append((x, lens, lens.float() / sp['T'], y, (y != 0).sum(1).to(torch.int32)))
            return tuple(out)

    tasks = [FakeTask(m) for m in range(sp['n_tasks'])]
    grads, fwd = [], []
    orig_step = torch.optim.Adam.step

    def spy_step(self_opt, *a, **kw):
        grads.append([p.grad.detach().clone() for p in model.parameters()])
        return orig_step(self_opt, *a, **kw)
    torch.optim.Adam.step = spy_step
    model.register_forward_hook(lambda m, i, o: fwd.append(float(torch.nn.functional.cross_entropy(
        o[0].detach().view(-1, o[0].size(2)), o[1].view(-1), ignore_index=0))))
    try:
        JointTrainer().train(model, vocab, tasks, [], 'ce', 0, sp['iters'], args, evaluate_every=10 ** 9, early_stop='cer,200')
    finally:
        torch.optim.Adam.step = orig_step
    assert len(grads) == sp['iters'] and len(fwd) == sp['iters'] * sp['n_tasks']
    out = {'joint/losses': np.asarray(fwd, dtype=np.float64).reshape(sp['iters'], sp['n_tasks']),
           'joint/spec': np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8)}
    return out


def manifest_records(torch, ref_init):
    """the reference's beam search (best hypothesis) on each utterance of the manifest fixture as a batch of its own, on the
    seeded model with the B0 perturbation; writes the manifest and the transcripts"""
    cfg, sp = MG.FIXTURES['F0']['cfg'], MANIFEST
    vocab = _vocab(cfg['vocab_size'])
    args = _args(cfg, beam_width=sp['beam_width'], beam_nbest=sp['nbest'])
    torch.manual_seed(123456)
    torch.set_num_threads(8)
    model = ref_init(args, vocab, is_factorized=False, r=cfg['r'])
    g = torch.Generator().manual_seed(sp['noise_seed'])
    W = model.decoder.output_linear.weight
    W.data += sp['noise'] * torch.randn(W.shape, generator=g)
    W.data[2] = sp['eos_gain'] * W.data[sp['eos_from']]
    model.eval()
    folder = os.path.join(MG.OUT, 'N0_manifest')
    os.makedirs(folder, exist_ok=True)
    rows, ids = [], []
    for i, (seed, T, L) in enumerate(zip(sp['seeds'], sp['T'], sp['L'])):
        x, lens, y = R.synth_batch(seed, 1, T, L, cfg['vocab_size'], variable=False)
        with open(os.path.join(folder, 'u%d.txt' % i), 'w', encoding='utf8') as f:
            f.write(''.join(vocab.id2label[int(t)] for t in y[0]))
        rows.append('u%d.wav,u%d.txt' % (i, i))
        with torch.no_grad():
            enc, _ = model.encoder(_frames(model, x), lens)
            got, _strs = model.decoder.beam_search(enc, args, beam_width=sp['beam_width'], nbest=sp['nbest'], start_token=vocab.SOS_ID)
        ids.append(list(got[0]))
    with open(os.path.join(folder, 'test.csv'), 'w') as f:
        f.write('\n'.join(rows) + '\n')
    arr = np.full((len(ids), max(len(r_) for r_ in ids)), -1, dtype=np.int64)
    for i, r_ in enumerate(ids):
        arr[i, :len(r_)] = r_
    return {'manifest/beam_ids': arr, 'manifest/spec': np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8)}


def checkpoint(torch, ref_functions, ref_init):
    cfg = dict(num_enc_layers=1, num_dec_layers=1, num_heads=4, dim_model=64, dim_key=16, dim_value=16, dim_inner=64, dim_emb=64,
               src_max_len=100, tgt_max_len=50, r=8)       # (width 64: the narrowest the device LayerNorm takes, so the file also decodes)
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    try:
        os.chdir(tmp)
        args = _args(cfg, dim_input=CKPT['F'], name='theirs', save_folder='save', lr=1e-2, meta_lr=1e-3, k_train=2, k_valid=2, clip=False,
                     max_norm=400, save_every=1)
        vocab = _vocab(64)
        torch.manual_seed(1)
        m = ref_init(args, vocab, is_factorized=False, r=cfg['r'])
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):             # exact period-9 patterns, different per tensor and per row (rows of 64, 21, 8): the file stays small
                p.copy_((((torch.arange(p.numel()) + 3 * i) % 9).float() - 4).view_as(p) / 64 + i / 1024)
        inner = torch.optim.SGD(m.parameters(), lr=args.lr)
        outer = torch.optim.Adam(m.parameters(), lr=args.meta_lr)
        for i, p in enumerate(m.parameters()):
            p.grad = torch.full_like(p, (i + 1) / 128)
        outer.step()
        ref_functions.save_meta_model(m, vocab, 4, inner, outer, {'avg_valid_cer': 1.5}, args)
        with open(os.path.join(tmp, 'save', 'theirs', 'epoch_4.th'), 'rb') as f, open(os.path.join(MG.OUT, 'N0.th.gz'), 'wb') as g:
            with gzip.GzipFile(filename='', mode='wb', fileobj=g, mtime=0, compresslevel=9) as z:
                z.write(f.read())
        # what the saved model computes: the logits and labels of a teacher-forced pass on a seeded batch, so that a loader which
        # mis-assigns a tensor cannot pass (no search: patterned weights give near-tied scores, whose order is rounding)
        sp = CKPT
        g = torch.Generator().manual_seed(sp['seed'])
        x = torch.randn(sp['k'], 1, sp['F'], sp['T'], generator=g)
        y = torch.randint(4, 64, (sp['k'], sp['L']), generator=g)
        lens = torch.tensor(sp['lens'], dtype=torch.int32)
        m.eval()
        with torch.no_grad():
            pred, gold, hyp = m(x, lens, y)
        return {'ckpt/pred': pred.numpy().astype(np.float32), 'ckpt/hyp': hyp.numpy().astype(np.int64),
                'ckpt/spec': np.frombuffer(json.dumps(sp).encode(), dtype=np.uint8)}
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)


def main():
    torch = MG.bootstrap_reference()
    import utils.functions as ref_functions          # the reference's
    ref_init = ref_functions.init_transformer_model
    ref_synth = R.synth_batch
    state = dict(fz=False)

    def init_none(args, vocab, **kw):
        """run_fixture passes vgg_cnn arguments and is_factorized=False: the switches this fixture changes"""
        args.feat_extractor = 'none'
        if state['fz']:
            args.dim_input = FZ['dim_input']
            kw['is_factorized'], kw['r'] = True, FZ['r']
        return ref_init(args, vocab, **kw)

    def synth(*a, **kw):
        if state['fz']:
            kw['freq_bins'] = FZ['dim_input']
        return ref_synth(*a, **kw)
    ref_functions.init_transformer_model = init_none
    R.synth_batch = synth
    try:
        MG.run_fixture('N0', SPEC, torch)
        state['fz'] = True
        MG.run_fixture('N0fz', dict(SPEC, iters=FZ['iters']), torch)
    finally:
        ref_functions.init_transformer_model = ref_init
        R.synth_batch = ref_synth
    path, path_fz = os.path.join(MG.OUT, 'N0.npz'), os.path.join(MG.OUT, 'N0fz.npz')
    store = dict(np.load(path))
    # (theta0 of the factorized record is pinned by its sha256 alone: every small array costs a zip entry, the file has a size limit)
    store.update({'fz/' + k: v for k, v in np.load(path_fz).items() if not k.startswith('theta0/')})
    store['fz/spec_fz'] = np.frombuffer(json.dumps(FZ).encode(), dtype=np.uint8)
    os.remove(path_fz)
    store.update(joint_record(torch, ref_init))
    store.update(decode_records(torch, ref_init))
    store.update(manifest_records(torch, ref_init))
    store.update(checkpoint(torch, ref_functions, ref_init))
    np.savez_compressed(path, **store)
    print('N0: greedy', store['decode/greedy_ids'].T.tolist(), 'beam', [[int(v) for v in r_ if v >= 0] for r_ in store['decode/beam_ids']])


if __name__ == '__main__':
    main()
