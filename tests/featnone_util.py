"""Test helpers for a model built with feat_extractor='none' (models/asr/transformer.py:88-94: the (B, 1, F, T) batch viewed as
(B, F, T), transposed, straight into the encoder whose input Linear takes F features per frame; no convolution, no time reduction).

(1) A torch restatement composed from oracle/refimpl.py's Enc / Dec (tests/factorized_util.py's pair for --is-factorized) by import:
    attribute names, construction order (encoder, decoder) and the Xavier pass follow the reference, so a seeded build has the
    reference's theta0 bit for bit.  tests/test_featnone.py pins it to tests/golden/N0.npz (tools/make_golden_featnone.py) on the CPU;
    the GPU tests then use it as the live fp32 / fp64 oracle at other shapes.
(2) The cases, inputs and bounds of the two kernels of csrc/mtl_featproj.hip.  Every bound comes from tests/x3_emul.py alone: half
    of what the cheapest dropped second-order term costs on random inputs, an eighth on the probe inputs."""
import argparse
import functools

import torch
import torch.nn as nn

from oracle import refimpl as R
from tests import factorized_util as FU
from tests import x3_emul as X


# ------------------------------------------------------------------------------------------------------------ (1) the restatement
class FrameTransformer(R.SpeechTransformer):
    """SpeechTransformer without convolutions: `conv` is the identity, so forward's view of the (B, C, H, W) = (B, 1, F, T) "feature
    map" as (B, C H, W) and its transpose are transformer.py:93-94, and refimpl's searches run on it unchanged"""

    def __init__(self, cfg, d_in, factorized=False):
        nn.Module.__init__(self)
        a = (cfg['num_heads'], cfg['dim_model'], cfg['dim_key'], cfg['dim_value'])
        enc, dec = (FU.FzEnc, FU.FzDec) if factorized else (R.Enc, R.Dec)
        self.encoder = enc(cfg['num_enc_layers'], *a, d_in, cfg['dim_inner'], cfg['src_max_len'], cfg['r'])
        self.decoder = dec(cfg['vocab_size'], cfg['num_dec_layers'], cfg['num_heads'], cfg['dim_emb'], cfg['dim_model'], cfg['dim_inner'],
                           cfg['dim_key'], cfg['dim_value'], cfg['tgt_max_len'], cfg['r'])
        self.conv = nn.Identity()
        for p in self.parameters():                                        # transformer.py:74-76
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def conv_stack(self, x, gates=None):
        return x


def build_model(cfg, d_in=161, factorized=False, seed=123456):
    torch.manual_seed(seed)
    m = FrameTransformer(cfg, d_in, factorized)
    m.train()
    return m


def device_args(cfg, spec, **over):
    a = dict(feat_extractor='none', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161, dropout=0.0,
             emb_trg_sharing=False, label_smoothing=0.0, name='featnone', lr=spec['lr'], meta_lr=spec['meta_lr'], k_train=spec['k'],
             k_valid=spec['k'], clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_featnone', cuda=True,
             is_factorized=False, r=cfg.get('r', 100))
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


def ffn_gates(engine):
    """the ReLU decisions of the engine's LAST forward in the layout refimpl's gate replay expects (the only branch points of such
    a model: the feed-forward blocks' inner activations)"""
    return {name: (t > 0).cpu() for name, t in engine.arena.items() if name.endswith('.ff.h1')}


def set_params(oracle, model, theta):
    with torch.no_grad():
        for (n, p) in oracle.named_parameters():
            p.copy_(model._layout.view(theta, n).cpu())


# ------------------------------------------------------------------------------------------------------------ (2) the kernels
SHAPES = [(2, 161, 63, 128), (1, 80, 130, 100), (3, 5, 1, 128), (2, 161, 257, 512)]         # (B, F, T, N)
TASKS = 3
FWD_PROBE = (2, 160, 63, 128)       # contraction over F (even for the antisymmetric partner): the frames constant-lead, the weight antisymmetric
WG_PROBE = (2, 161, 65, 128)        # contraction over the B T = 130 rows: dy constant-lead along them, the features antisymmetric


@functools.lru_cache(maxsize=None)
def kernel_inputs(shape):
    """x (TASKS, B, F, T), w (TASKS, N, F), bias (TASKS, N), dy (TASKS, B T, N), dw0 (TASKS, N, F) the pre-filled gradient"""
    B, Fq, T, N = shape
    g = torch.Generator().manual_seed(6000 + B + Fq + T + N)
    return dict(x=torch.randn(TASKS, B, Fq, T, generator=g), w=torch.randn(TASKS, N, Fq, generator=g) * Fq ** -0.5,
                bias=torch.randn(TASKS, N, generator=g) * 0.1, dy=torch.randn(TASKS, B * T, N, generator=g),
                dw0=torch.randn(TASKS, N, Fq, generator=g))


@functools.lru_cache(maxsize=None)
def probe_inputs(which):
    B, Fq, T, N = FWD_PROBE if which == 'fwd' else WG_PROBE
    g = torch.Generator().manual_seed(6100 + (which == 'wgrad'))
    inp = {k: v[:1].clone() for k, v in kernel_inputs((B, Fq, T, N)).items()}
    if which == 'fwd':
        inp['x'] = X.const_lead((B, T, Fq), g=g, rounding='trunc').transpose(1, 2).contiguous().unsqueeze(0)
        inp['w'] = X.antisym((N, Fq), g=g).unsqueeze(0)
    else:
        inp['dy'] = X.const_lead((N, B * T), g=g, rounding='trunc').t().contiguous().unsqueeze(0)
        inp['x'] = X.antisym((Fq, B * T), g=g).view(Fq, B, T).transpose(0, 1).contiguous().unsqueeze(0)
    return inp


def frames(x):          # (B, F, T) -> (B T, F): the rows the input Linear sees
    return x.transpose(1, 2).reshape(-1, x.shape[1])


def _report(a, b, add, probe):
    """errors against fp64 of a @ b + add: six terms, torch fp32, every five-term list; and the bound"""
    ref = a.double() @ b.double() + add.double()
    prods = X.piece_products(a, b, 'trunc')
    dropped = X.PROBE_TERMS['a'] if probe else X.SECOND_ORDER
    r = dict(six=X.rel(X.sum_terms(prods, X.SIX) + add, ref), f32=X.rel(a @ b + add, ref),
             drops={t: X.rel(X.sum_terms(prods, tuple(s for s in X.SIX if s != t)) + add, ref) for t in dropped})
    r['bound'] = min(r['drops'].values()) / (8 if probe else 2)
    return r


@functools.lru_cache(maxsize=None)
def fwd_report(shape, task=0, bias=True, probe=False, x_task=None):
    """x_task: the task whose batch the product reads (the shared batch of an sX = 0 launch is task 0's); default: its own"""
    inp = probe_inputs('fwd') if probe else kernel_inputs(shape)
    add = inp['bias'][task].unsqueeze(0) if bias and not probe else torch.zeros(1, shape[3])
    return _report(frames(inp['x'][task if x_task is None else x_task]), inp['w'][task].t().contiguous(), add, probe)


@functools.lru_cache(maxsize=None)
def wgrad_report(shape, task=0, probe=False, x_task=None):
    inp = probe_inputs('wgrad') if probe else kernel_inputs(shape)
    return _report(inp['dy'][task].t().contiguous(), frames(inp['x'][task if x_task is None else x_task]),
                   torch.zeros(1, shape[1]) if probe else inp['dw0'][task], probe)


def fwd_reference(inp, task, bias=True, x_task=None):
    out = frames(inp['x'][task if x_task is None else x_task]).double() @ inp['w'][task].double().t()
    return out + inp['bias'][task].double() if bias else out


def wgrad_reference(inp, task, x_task=None, prefilled=True):
    out = inp['dy'][task].double().t() @ frames(inp['x'][task if x_task is None else x_task]).double()
    return out + inp['dw0'][task].double() if prefilled else out


# ------------------------------------------------------------------------------------------------------------ (3) the fixture
class Sub:
    """the arrays of an npz under `prefix`, with the interface tests/golden_util.py's checks use"""

    def __init__(self, z, prefix):
        self.z, self.prefix = z, prefix
        self.files = [k[len(prefix):] for k in z.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self.z[self.prefix + k]


def batches(cfg, spec, it, data_call_index, freq_bins=161):
    """golden_util.batches_for at `freq_bins` features per frame"""
    call, n = int(data_call_index[it]), spec['n_tasks']
    mk = lambda seed: R.synth_batch(seed, spec['k'], spec['T'], spec['L'], cfg['vocab_size'], spec['variable'], freq_bins=freq_bins)
    return [mk(1000 * call + 10 * m) for m in range(n)], mk(1000 * call + 10 * (n - 1) + 1)


def load_fz():
    """the factorized record of N0.npz -> (arrays, cfg with its r, spec with its iteration count, features per frame)"""
    import json
    from tests import golden_util as gu
    z, cfg, spec = gu.load('N0')
    fz = json.loads(bytes(z['fz/spec_fz']).decode())
    return Sub(z, 'fz/'), dict(cfg, r=fz['r']), dict(spec, iters=fz['iters']), fz['dim_input']


class Task:
    """mtl_amd.SyntheticTask at `freq_bins` features per frame (the dataset contract of the trainers' train())"""

    def __init__(self, task_id, k, T, L, vocab_size, variable=False, freq_bins=161):
        self.task_id, self.k, self.T, self.L, self.V, self.variable, self.freq_bins, self.calls = task_id, k, T, L, vocab_size, variable, freq_bins, 0

    def sample(self, k_train, k_valid, manifest_id):
        it = self.calls
        self.calls += 1
        out = []
        for part, k in ((0, k_train), (1, k_valid)):
            x, lens, y = R.synth_batch(1000 * it + 10 * self.task_id + part, k, self.T, self.L, self.V, self.variable, freq_bins=self.freq_bins)
            out.append((x, lens, lens.float() / self.T, y, (y != 0).sum(1).to(torch.int32)))
        return tuple(out)


class capture_ffn_gates:
    """oracle/branches.py:capture_gates for a model without convolutions: with ... as log -> the feed-forward ReLU decisions of every
    forward in the ORACLE's pass order (task 0 train, task 0 validation, task 1 train, ...), one meta-iteration per capture"""

    def __init__(self, model):
        self.model, self.log, self._batched = model, [], []

    def __enter__(self):
        from oracle import branches

        def hook(eng):
            torch.cuda.current_stream(eng.device).synchronize()
            g = ffn_gates(eng)
            if eng.nt > 1:
                self._batched.append(branches.split_gates(g, eng.nt))
            else:
                self.log.append(g)
        for e in self.model.engines:
            e.forward_hook = hook
        return self.log

    def __exit__(self, *exc):
        for e in self.model.engines:
            e.forward_hook = None
        if self._batched:
            for t in range(len(self._batched[0])):
                for phase in self._batched:
                    self.log.append(phase[t])
        return False
