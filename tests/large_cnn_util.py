"""A torch restatement of the reference's model with feat_extractor='large_cnn' (models/asr/transformer.py:60-72,
utils/functions.py:324-327) on the classes of oracle/refimpl.py: the VGG shape at half the width, d_in = (F // 4) * 64.  The
construction order (encoder, decoder, conv) and the Xavier pass over parameters() follow the reference, so a seeded build has the
reference's theta0 bit for bit (tests/test_large_cnn.py pins it to tests/golden/LC0.npz, written by tools/make_golden_large_cnn.py).
conv_stack / forward / the gate replay are SpeechTransformer's: they index the convolutions (0, 2, 5, 7), not their widths."""
import argparse

import torch
import torch.nn as nn

from oracle import refimpl as R


class LargeCnnTransformer(R.SpeechTransformer):
    def __init__(self, vocab_size, enc_layers, dec_layers, heads, d, dk, dv, inner, d_emb, src_max_len, trg_max_len, r=100, freq_bins=161):
        nn.Module.__init__(self)
        d_in = (freq_bins // 2 // 2) * 64                                  # utils/functions.py:324-327
        self.encoder = R.Enc(enc_layers, heads, d, dk, dv, d_in, inner, src_max_len, r)
        self.decoder = R.Dec(vocab_size, dec_layers, heads, d_emb, d, inner, dk, dv, trg_max_len, r)
        self.conv = nn.Sequential(                                         # transformer.py:60-72
            nn.Conv2d(1, 32, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(32, 32, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(32, 64, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(64, 64, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2))
        for p in self.parameters():                                        # transformer.py:74-76
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


def build_model(cfg, seed=123456):
    """R.build_model for large_cnn"""
    torch.manual_seed(seed)
    m = LargeCnnTransformer(cfg['vocab_size'], cfg['num_enc_layers'], cfg['num_dec_layers'], cfg['num_heads'], cfg['dim_model'],
                            cfg['dim_key'], cfg['dim_value'], cfg['dim_inner'], cfg['dim_emb'], cfg['src_max_len'], cfg['tgt_max_len'],
                            r=cfg.get('r', 100))
    m.train()
    return m


def device_args(cfg, spec, **over):
    """the argparse.Namespace of a device model at a fixture's configuration"""
    a = dict(feat_extractor='large_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
             emb_trg_sharing=False, label_smoothing=0.0, name='lc', lr=spec['lr'], meta_lr=spec['meta_lr'], k_train=spec['k'],
             k_valid=spec['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_lc', cuda=True, is_factorized=False,
             r=cfg.get('r', 100))
    a.update({k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    a.update(over)
    return argparse.Namespace(**a)


def device_model(cfg, spec, seed=123456, **over):
    """-> (model on the CPU, vocab, args): init_transformer_model of this package, seeded like the fixture"""
    import mtl_amd
    args = device_args(cfg, spec, **over)
    vocab = mtl_amd.synthetic_vocab(cfg['vocab_size'])
    torch.manual_seed(seed)
    return mtl_amd.init_transformer_model(args, vocab, r=cfg.get('r', 100)), vocab, args
