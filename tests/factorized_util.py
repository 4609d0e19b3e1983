"""A torch restatement of the reference's model with --is-factorized (utils/functions.py:307-351) on the classes of oracle/refimpl.py:
FactorizedPositionwiseFeedForward (modules/common_layers.py:134-158) in every encoder and decoder layer and the encoder's input pair
input_linear_a / _b (modules/encoder.py:40-44, 68-70).  Attribute names, construction order (encoder, decoder, conv) and the Xavier
pass over parameters() follow the reference, so a seeded build has the reference's theta0 bit for bit (tests/test_factorized.py pins it
to tests/golden/FZ0.npz, written by tools/make_golden_factorized.py).  The gate / dropout replay is refimpl.FFN's: gates[tag + 'h1'] is
the post-ReLU decision of the inner activation, drop[tag + 'mf'] the keep-mask in front of the residual add.  conv_stack / forward /
the searches are SpeechTransformer's."""
import argparse

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import refimpl as R


class FactorizedFFN(nn.Module):
    """common_layers.py:134-158"""

    def __init__(self, d, inner, r):
        super().__init__()
        self.linear_1_a = nn.Linear(d, r, bias=False)
        self.linear_1_b = nn.Linear(r, inner)
        self.linear_2_a = nn.Linear(inner, r, bias=False)
        self.linear_2_b = nn.Linear(r, d)
        self.layer_norm = nn.LayerNorm(d)

    @property
    def linear_1(self):
        """the module whose output is the ReLU's pre-activation: what oracle/branches.py:oracle_trace hooks"""
        return self.linear_1_b

    def forward(self, x, drop=None, tag='', gates=None):
        h = self.linear_1_b(self.linear_1_a(x))
        h = F.relu(h) if gates is None else R.relu_replay(h, gates[tag + 'h1'].reshape(h.shape))
        h = self.linear_2_b(self.linear_2_a(h))
        if drop is not None:
            h = h * drop[tag + 'mf']                                       # common_layers.py:156
        return self.layer_norm(h + x)


class FzEncLayer(R.EncLayer):
    """modules/encoder.py:83-106, is_factorized"""

    def __init__(self, heads, d, inner, dk, dv, r):
        nn.Module.__init__(self)
        self.self_attn = R.LowRankMHA(heads, d, dk, dv, r)
        self.pos_ffn = FactorizedFFN(d, inner, r)


class FzEnc(R.Enc):
    """modules/encoder.py:15-80, is_factorized"""

    def __init__(self, layers, heads, d, dk, dv, d_in, inner, src_max_len, r):
        nn.Module.__init__(self)
        self.input_linear_a = nn.Linear(d_in, r, bias=False)
        self.input_linear_b = nn.Linear(r, d)
        self.layer_norm_input = nn.LayerNorm(d)
        self.positional_encoding = R.PositionTable(d, src_max_len)
        self.layers = nn.ModuleList([FzEncLayer(heads, d, inner, dk, dv, r) for _ in range(layers)])

    def input_linear(self, feats):
        """(Enc.forward calls self.input_linear(feats): modules/encoder.py:68-70)"""
        return self.input_linear_b(self.input_linear_a(feats))


class FzDecLayer(R.DecLayer):
    """modules/decoder.py:293-323, is_factorized"""

    def __init__(self, d, inner, heads, dk, dv, r):
        nn.Module.__init__(self)
        self.self_attn = R.LowRankMHA(heads, d, dk, dv, r)
        self.encoder_attn = R.LowRankMHA(heads, d, dk, dv, r)
        self.pos_ffn = FactorizedFFN(d, inner, r)


class FzDec(R.Dec):
    """modules/decoder.py:14-115, is_factorized"""

    def __init__(self, vocab_size, layers, heads, d_emb, d, inner, dk, dv, trg_max_len, r):
        nn.Module.__init__(self)
        self.trg_embedding = nn.Embedding(vocab_size, d_emb, padding_idx=R.PAD_ID)
        self.positional_encoding = R.PositionTable(d, trg_max_len)
        self.layers = nn.ModuleList([FzDecLayer(d, inner, heads, dk, dv, r) for _ in range(layers)])
        self.output_linear = nn.Linear(d, vocab_size, bias=False)
        nn.init.xavier_normal_(self.output_linear.weight)


class FactorizedTransformer(R.SpeechTransformer):
    CONV = {'vgg_cnn': (64, 128), 'large_cnn': (32, 64)}

    def __init__(self, vocab_size, enc_layers, dec_layers, heads, d, dk, dv, inner, d_emb, src_max_len, trg_max_len, r=100, freq_bins=161,
                 feat_extractor='vgg_cnn', d_in=None):
        nn.Module.__init__(self)
        c1, c2 = self.CONV[feat_extractor]
        d_in = (freq_bins // 2 // 2) * c2 if d_in is None else d_in       # utils/functions.py:318-327
        self.encoder = FzEnc(enc_layers, heads, d, dk, dv, d_in, inner, src_max_len, r)
        self.decoder = FzDec(vocab_size, dec_layers, heads, d_emb, d, inner, dk, dv, trg_max_len, r)
        self.conv = nn.Sequential(                                         # transformer.py:47-72
            nn.Conv2d(1, c1, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(c1, c1, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(c1, c2, 3, stride=1, padding=1), nn.ReLU(),
            nn.Conv2d(c2, c2, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2))
        for p in self.parameters():                                        # transformer.py:74-76
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


def build_model(cfg, seed=123456, feat_extractor='vgg_cnn'):
    """R.build_model for --is-factorized"""
    torch.manual_seed(seed)
    m = FactorizedTransformer(cfg['vocab_size'], cfg['num_enc_layers'], cfg['num_dec_layers'], cfg['num_heads'], cfg['dim_model'],
                              cfg['dim_key'], cfg['dim_value'], cfg['dim_inner'], cfg['dim_emb'], cfg['src_max_len'], cfg['tgt_max_len'],
                              r=cfg.get('r', 100), feat_extractor=feat_extractor)
    m.train()
    return m


def device_args(cfg, spec, **over):
    """the argparse.Namespace of a device model at a fixture's configuration"""
    a = dict(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
             emb_trg_sharing=False, label_smoothing=0.0, name='fz', lr=spec['lr'], meta_lr=spec['meta_lr'], k_train=spec['k'],
             k_valid=spec['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_fz', cuda=True, is_factorized=True,
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
    return mtl_amd.init_transformer_model(args, vocab, is_factorized=args.is_factorized, r=args.r), vocab, args
