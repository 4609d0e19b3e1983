"""tests/golden/FZ0.npz and tests/golden/FZ0.th.gz: a model the REAL reference builds with --is-factorized (utils/functions.py:307-351:
FactorizedPositionwiseFeedForward in every layer, input_linear_a / _b in the encoder).

FZ0.npz: the F0 fixture of oracle/make_golden.py (enc1 / dec1, d 128, inner 128, 8 heads of 16, r 100, V 64, 3 tasks, k 2, T 64, L 8,
variable lengths, 2 --copy-grad meta-steps) recorded by make_golden.run_fixture on that model, plus the reference's greedy
(Decoder.greedy_search: the first GREEDY_STEPS of its 300 steps, on the same theta0 under tgt_max_len 320, which its fixed step count
needs) and beam-3 (Decoder.beam_search, 2-best) token sequences for the B0 fixture's utterances and perturbed vocabulary projection.
FZ0.th.gz: the reference's own save_meta_model of a tiny factorized model (width 16, r 8; exact period-8 weight patterns, one Adam
step), gzip-compressed like C0.th.gz: a state dict, an args namespace and optimizer state.
The reference is imported through make_golden.bootstrap_reference(), never copied; only the two data files are committed.

    python tools/make_golden_factorized.py
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

GREEDY_STEPS = 24
DECODE = dict(seed=500, k=3, T=64, L=8, beam_width=3, nbest=2, noise_seed=7, noise=0.5, eos_from=47, eos_gain=1.02, greedy_steps=GREEDY_STEPS)


def _vocab(size):
    from utils.data import Vocab
    vocab = Vocab()
    for i in range(size - 4):
        vocab.add_token(chr(0x4e00 + i))
        vocab.add_label(chr(0x4e00 + i))
    return vocab


def _args(cfg, **over):
    a = dict(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
             emb_trg_sharing=False, label_smoothing=0.0, name='golden_FZ0', cuda=False, is_factorized=True, r=cfg['r'])
    a.update({k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    a.update(over)
    return argparse.Namespace(**a)


def decode_records(torch, ref_init):
    """the reference's searches on the seeded factorized model with the B0 perturbation of decoder.output_linear"""
    from oracle.refimpl import synth_batch
    cfg, sp = MG.FIXTURES['F0']['cfg'], DECODE
    vocab = _vocab(cfg['vocab_size'])
    x, lens, y = synth_batch(sp['seed'], sp['k'], sp['T'], sp['L'], cfg['vocab_size'], variable=True)
    out = {}
    for what, tgt_max_len in (('beam', cfg['tgt_max_len']), ('greedy', 320)):
        args = _args(dict(cfg, tgt_max_len=tgt_max_len), beam_width=sp['beam_width'], beam_nbest=sp['nbest'])
        torch.manual_seed(123456)
        torch.set_num_threads(8)
        model = ref_init(args, vocab, is_factorized=True, r=cfg['r'])
        g = torch.Generator().manual_seed(sp['noise_seed'])
        W = model.decoder.output_linear.weight
        W.data += sp['noise'] * torch.randn(W.shape, generator=g)
        W.data[2] = sp['eos_gain'] * W.data[sp['eos_from']]
        model.eval()
        with torch.no_grad():
            if what == 'beam':
                f = model.conv(x)
                sz = f.size()
                enc, _ = model.encoder(f.view(sz[0], sz[1] * sz[2], sz[3]).transpose(1, 2).contiguous(), lens)
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


def checkpoint(torch, ref_functions, ref_init):
    cfg = dict(num_enc_layers=1, num_dec_layers=1, num_heads=2, dim_model=16, dim_key=8, dim_value=8, dim_inner=16, dim_emb=16,
               src_max_len=100, tgt_max_len=50, r=8)
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    try:
        os.chdir(tmp)
        args = _args(cfg, name='theirs', save_folder='save', lr=1e-2, meta_lr=1e-3, k_train=2, k_valid=2, clip=False, max_norm=400,
                     save_every=1)
        vocab = _vocab(64)
        torch.manual_seed(1)
        m = ref_init(args, vocab, is_factorized=True, r=cfg['r'])
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):             # exact period-8 patterns, different per tensor: the file compresses to a few KB
                p.copy_((((torch.arange(p.numel()) + 3 * i) % 8).float() - 3.5).view_as(p) / 64 + i / 1024)
        inner = torch.optim.SGD(m.parameters(), lr=args.lr)
        outer = torch.optim.Adam(m.parameters(), lr=args.meta_lr)
        for i, p in enumerate(m.parameters()):
            p.grad = torch.full_like(p, (i + 1) / 128)
        outer.step()
        ref_functions.save_meta_model(m, vocab, 4, inner, outer, {'avg_valid_cer': 1.5}, args)
        with open(os.path.join(tmp, 'save', 'theirs', 'epoch_4.th'), 'rb') as f, open(os.path.join(MG.OUT, 'FZ0.th.gz'), 'wb') as g:
            with gzip.GzipFile(filename='', mode='wb', fileobj=g, mtime=0, compresslevel=9) as z:
                z.write(f.read())
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)


def main():
    torch = MG.bootstrap_reference()
    import utils.functions as ref_functions          # the reference's
    ref_init = ref_functions.init_transformer_model

    def init_factorized(args, vocab, **kw):
        """run_fixture passes is_factorized=False: the one switch this fixture changes"""
        kw['is_factorized'] = True
        return ref_init(args, vocab, **kw)
    ref_functions.init_transformer_model = init_factorized
    MG.run_fixture('FZ0', dict(MG.FIXTURES['F0'], iters=2), torch)
    ref_functions.init_transformer_model = ref_init
    path = os.path.join(MG.OUT, 'FZ0.npz')
    store = dict(np.load(path))
    store.update(decode_records(torch, ref_init))
    np.savez_compressed(path, **store)
    print('FZ0: greedy', store['decode/greedy_ids'].T.tolist(), 'beam', [[int(v) for v in r_ if v >= 0] for r_ in store['decode/beam_ids']])
    checkpoint(torch, ref_functions, ref_init)


if __name__ == '__main__':
    main()
