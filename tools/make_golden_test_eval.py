"""Generate tests/golden/T0.npz: the REAL reference's test-set evaluation (test.py:112-171 `evaluate`) over two batches, for the greedy
search, the beam search (beam_nbest = 1) and the beam search with LM rescoring.

Runs only where the reference checkout exists.  It imports the reference's own test.py through oracle/make_golden.py's bootstrap
(test.py parses sys.argv at import, so it is set first; third-party modules its imports need but this machine lacks are stubbed in
THIS process) and copies none of its text.  Model, vocabulary and LM are R0's (tools/make_golden_lm_rescore.py): the F0 model with
the B0 perturbation of its vocabulary projection and a vocabulary that mixes CJK characters, Latin letters and ' ', so that WER and the
per-language CER are exercised -- with tgt_max_len 320, which the reference's 300-step greedy search needs (the positional table is
not a parameter: the weights are R0's).  What is recorded: per utterance the post-processed hypothesis and gold strings, the three
distances and the counts that test.py accumulates, the running totals after every batch and the printed line without its time field.

    python tools/make_golden_test_eval.py
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import bootstrap_reference, FIXTURES  # noqa: E402
from tests import lm_rescore_util as lu  # noqa: E402

TGT_MAX_LEN = 320
BATCHES = [dict(seed=500, k=6, T=64, L=8), dict(seed=517, k=4, T=96, L=12)]       # the first one is R0's batch
MODES = dict(greedy=dict(beam_search=False, lm_rescoring=False),
             beam=dict(beam_search=True, lm_rescoring=False),
             beam_lm=dict(beam_search=True, lm_rescoring=True))
TIME_FIELD = re.compile(r' TOTAL_TIME:[0-9.]+')
TOTALS = ('total_word', 'total_char', 'total_cer', 'total_wer', 'total_en_cer', 'total_zh_cer', 'total_en_char', 'total_zh_char',
          'total_hyp_char')


def import_reference_test(ref_root):
    """the reference's test.py as a module; modules it imports that are not installed here become empty stubs"""
    sys.argv = ['test.py']
    import scipy.signal
    import scipy.signal.windows
    for name in ('hamming', 'hann', 'blackman', 'bartlett'):                   # (the window functions' home in current scipy releases)
        if not hasattr(scipy.signal, name):
            setattr(scipy.signal, name, getattr(scipy.signal.windows, name))
    for _ in range(32):
        spec = importlib.util.spec_from_file_location('reference_test', os.path.join(ref_root, 'test.py'))
        mod = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(mod)
            return mod
        except ModuleNotFoundError as e:
            stub = types.ModuleType(e.name)
            stub.__getattr__ = lambda name: object
            stub.__path__ = []
            sys.modules[e.name] = stub
            for k in [k for k in sys.modules if k.startswith('utils.')]:        # half-imported reference modules: import them again
                del sys.modules[k]
    raise RuntimeError('the reference test.py does not import')


def main():
    torch = bootstrap_reference()
    ref_root = [p for p in sys.path if os.path.exists(os.path.join(p, 'test.py')) and os.path.exists(os.path.join(p, 'utils', 'lm.py'))][0]
    from utils.data import Vocab
    from utils.functions import init_transformer_model
    import utils.lm as ref_lm
    from oracle.refimpl import synth_batch
    ref_test = import_reference_test(ref_root)

    r0 = lu.load_r0()
    s = r0['spec']
    cfg = FIXTURES['F0']['cfg']
    vocab = Vocab()
    for c in r0['labels']:
        vocab.add_token(c)
        vocab.add_label(c)
    assert len(vocab.id2label) == cfg['vocab_size']
    spec = dict(tgt_max_len=TGT_MAX_LEN, beam_width=s['beam_width'], beam_nbest=1, lm_weight=s['lm_weight'], c_weight=s['c_weight'],
                batches=BATCHES, r0=True)
    margs = argparse.Namespace(
        feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
        num_enc_layers=cfg['num_enc_layers'], num_dec_layers=cfg['num_dec_layers'], num_heads=cfg['num_heads'],
        dim_model=cfg['dim_model'], dim_key=cfg['dim_key'], dim_value=cfg['dim_value'], dim_inner=cfg['dim_inner'],
        dim_emb=cfg['dim_emb'], src_max_len=cfg['src_max_len'], tgt_max_len=TGT_MAX_LEN, dropout=0.0,
        emb_trg_sharing=False, label_smoothing=0.0, name='golden_T0', cuda=False)
    torch.manual_seed(123456)
    torch.set_num_threads(8)
    model = init_transformer_model(margs, vocab, is_factorized=False, r=cfg['r'])
    g = torch.Generator().manual_seed(s['noise_seed'])
    W = model.decoder.output_linear.weight
    W.data += s['noise'] * torch.randn(W.shape, generator=g)
    W.data[2] = s['eos_gain'] * W.data[s['eos_from']]
    lm_path, sha = lu.r0_checkpoint(r0, '/tmp/golden_T0_lm.pt')
    assert sha == r0['lm_sha256']
    lm = ref_lm.LM(lm_path, argparse.Namespace(cuda=False))

    # the synthetic targets hardly ever hold a ' ' (so every gold word would count as Chinese): the second batch's targets are redrawn
    # as words -- Latin, CJK and mixed ones -- separated by single spaces, and stored in the fixture (the inputs come from the seeds)
    lid = vocab.label2id
    sp = lid[' ']
    latin = [lid[c] for c in 'abcdefghijklmnopqrstuvwxyz' if c in lid]
    cjk = [i for i, c in enumerate(vocab.id2label) if len(c) == 1 and ord(c) >= 0x4e00]
    loader, targets = [], []
    for bi, b in enumerate(BATCHES):
        x, lens, y = synth_batch(b['seed'], b['k'], b['T'], b['L'], cfg['vocab_size'], variable=True)
        if bi > 0:
            rng = np.random.RandomState(b['seed'])
            for row in y:
                n, prev_space = int((row != 0).sum()), True
                for t in range(n):
                    kind = rng.choice(3, p=[0.25, 0.4, 0.35]) if not prev_space and t < n - 1 else 1 + rng.choice(2)
                    row[t] = sp if kind == 0 else int(rng.choice(latin if kind == 1 else cjk))
                    prev_space = kind == 0
        loader.append((x, y, None, lens, None))
        targets.append(y.numpy().astype(np.int64))

    enc_str = lambda lst: np.frombuffer('\n'.join(lst).encode('utf-8'), dtype=np.uint8)
    store = dict(spec=np.frombuffer(json.dumps(spec).encode(), dtype=np.uint8))
    store.update({'target%d' % i: y for i, y in enumerate(targets)})
    ref_test.USE_CUDA = False
    for mode, kw in MODES.items():
        args = argparse.Namespace(beam_search=kw['beam_search'], lm_rescoring=kw['lm_rescoring'], beam_width=spec['beam_width'],
                                  beam_nbest=spec['beam_nbest'], lm_weight=spec['lm_weight'], c_weight=spec['c_weight'], verbose=False,
                                  tgt_max_len=TGT_MAX_LEN, cuda=False)
        log = dict(wer=[], cer=[], en_zh=[])
        real = dict(wer=ref_test.calculate_wer, cer=ref_test.calculate_cer, en_zh=ref_test.calculate_cer_en_zh)

        def spy(kind):
            def f(a, b):
                out = real[kind](a, b)
                log[kind].append((a, b, out))
                return out
            return f
        ref_test.calculate_wer, ref_test.calculate_cer, ref_test.calculate_cer_en_zh = spy('wer'), spy('cer'), spy('en_zh')
        out = io.StringIO()
        try:
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
                ref_test.evaluate(model, vocab, loader, args, lm=lm if kw['lm_rescoring'] else None, start_token=vocab.SOS_ID)
        finally:
            ref_test.calculate_wer, ref_test.calculate_cer, ref_test.calculate_cer_en_zh = real['wer'], real['cer'], real['en_zh']
        printed = out.getvalue().splitlines()
        assert not any('switch to greedy' in ln for ln in printed), 'the best hypothesis of a batch is empty'
        lines = [TIME_FIELD.sub('', ln) for ln in printed if ln.startswith('TEST CER:')]
        n_utt = sum(b['k'] for b in BATCHES)
        assert len(lines) == len(BATCHES) and len(log['wer']) == len(log['cer']) == len(log['en_zh']) == n_utt
        hyps, golds = [a for a, _b, _o in log['wer']], [b for _a, b, _o in log['wer']]
        per = np.array([[w[2], c[2], e[2][0], e[2][1], e[2][2], e[2][3], len(h), len(gd.split(' ')), len(gd)]
                        for w, c, e, h, gd in zip(log['wer'], log['cer'], log['en_zh'], hyps, golds)], dtype=np.int64)
        # running totals after every batch, in TOTALS order -- and they must reproduce the line the reference printed
        totals, t, i = [], dict.fromkeys(TOTALS, 0), 0
        for b, line in zip(BATCHES, lines):
            for row in per[i:i + b['k']]:
                wer, cer, en_cer, zh_cer, en_char, zh_char, hyp_char, words, chars = (int(v) for v in row)
                t['total_wer'] += wer
                t['total_cer'] += cer
                t['total_en_cer'] += en_cer
                t['total_zh_cer'] += zh_cer
                t['total_en_char'] += en_char
                t['total_zh_char'] += zh_char
                t['total_hyp_char'] += hyp_char
                t['total_word'] += words
                t['total_char'] += chars
            i += b['k']
            totals.append([t[k] for k in TOTALS])
            mine = 'TEST CER:{:.2f}% WER:{:.2f}% CER_EN:{:.2f}% CER_ZH:{:.2f}% TOTAL HYP CHAR:{:.2f}'.format(
                t['total_cer'] * 100 / t['total_char'], t['total_wer'] * 100 / t['total_word'], t['total_en_cer'] * 100 / max(1, t['total_en_char']),
                t['total_zh_cer'] * 100 / max(1, t['total_zh_char']), t['total_hyp_char'])
            assert mine == line, (mine, line)
        assert all('\n' not in v for v in hyps + golds)
        store.update({mode + '/hyp': enc_str(hyps), mode + '/gold': enc_str(golds), mode + '/per_utt': per,
                      mode + '/totals': np.array(totals, dtype=np.int64), mode + '/lines': enc_str(lines)})
        print('T0 %-8s %s' % (mode, lines[-1]))
        for h, gd in zip(hyps, golds):
            print('    %r | %r' % (h, gd))
    assert any(per_row[4] > 0 for per_row in store['beam/per_utt']) and any(per_row[5] > 0 for per_row in store['beam/per_utt'])
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'T0.npz'), **store)


if __name__ == '__main__':
    main()
