"""Helpers of the test-set evaluation tests: read tests/golden/T0.npz (tools/make_golden_test_eval.py) and rebuild its model, vocabulary,
batches and settings."""
import argparse
import json
import os

import numpy as np
import torch

from tests import golden_util as gu
from tests import lm_rescore_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('greedy', 'beam', 'beam_lm')
TOTALS = ('total_word', 'total_char', 'total_cer', 'total_wer', 'total_en_cer', 'total_zh_cer', 'total_en_char', 'total_zh_char',
          'total_hyp_char')


def load_t0():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'T0.npz'))
    dec = lambda k: bytes(z[k]).decode('utf-8').split('\n')
    out = dict(spec=json.loads(bytes(z['spec']).decode()))
    out['targets'] = [torch.from_numpy(z['target%d' % i]) for i in range(len(out['spec']['batches']))]
    for mode in MODES:
        out[mode] = dict(hyp=dec(mode + '/hyp'), gold=dec(mode + '/gold'), per_utt=z[mode + '/per_utt'], totals=z[mode + '/totals'],
                         lines=dec(mode + '/lines'))
    return out


def t0_vocab():
    return lu.r0_vocab(lu.load_r0())


def eval_args(spec, mode):
    """the fields of test.py's argument parser that its evaluate() and model.evaluate read"""
    return argparse.Namespace(beam_search=mode != 'greedy', lm_rescoring=mode == 'beam_lm', beam_width=spec['beam_width'],
                              beam_nbest=spec['beam_nbest'], lm_weight=spec['lm_weight'], c_weight=spec['c_weight'], verbose=False,
                              tgt_max_len=spec['tgt_max_len'], cuda=True)


def t0_model(mtl_amd, vocab, perturb=True, tgt_max_len=320):
    """R0's model (F0 with the B0 perturbation of the vocabulary projection) with T0's longer positional table, on the CPU"""
    z, cfg, spec = gu.load('F0')
    cfg = dict(cfg, tgt_max_len=tgt_max_len)
    args = argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
                              emb_trg_sharing=False, label_smoothing=0.0, name='t0', lr=spec['lr'], meta_lr=spec['meta_lr'],
                              k_train=spec['k'], k_valid=spec['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_ckpt',
                              cuda=True, **{k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    if perturb:
        gu.perturb_output_layer(model.decoder.output_linear.weight, lu.load_r0()['spec'])
    return model


def t0_loader(t0):
    """T0's batches as AudioDataLoader yields them: (src, trg, src_percentages, src_lengths, trg_lengths)"""
    from oracle import refimpl as R
    cfg = gu.load('F0')[1]
    out = []
    for b, y in zip(t0['spec']['batches'], t0['targets']):
        x, lens, _y = R.synth_batch(b['seed'], b['k'], b['T'], b['L'], cfg['vocab_size'], True)
        out.append((x, y, None, lens, None))
    return out
