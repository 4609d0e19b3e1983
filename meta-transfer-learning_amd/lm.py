"""LM meta-transfer path on the MI355X (BASELINE.json configs[4]): drop-in pieces for `lm/model/rnn_model.py`,
`lm/util/data.py` and the training loop of `lm/main_meta_transfer.py:277-411`.

* `RNNModel('LSTM' | 'GRU', ntoken, ninp, nhid, nlayers, dropout, tie_weights)`: same constructor, parameter names (`encoder.weight`,
  `rnn.weight_ih_l0`, ..., `decoder.bias`), `init_weights` and RNG draw order as the reference (bit-identical initialisation); all
  parameters are views into ONE flat fp32 buffer, the compute runs in libmtl_hip.so (`LMEngine`): embedding gather + Philox dropout,
  per layer ONE GEMM for the input contributions of all T steps, per step the recurrent GEMM (small-product engine) + the fused
  LSTM cell kernel, vocabulary projection + fused cross-entropy; hand-written backward (BPTT over the bptt window), weight
  gradients as three products over all T steps with the bias gradients folded in.  A GRU (csrc/mtl_gru.hip) carries a single hidden
  tensor and has two gate-gradient tensors per layer; `tie_weights=True` makes `decoder.weight` the `encoder.weight` Parameter (one
  entry in the flat layout, both gradients accumulate into it).  `RNN_TANH` / `RNN_RELU` raise.
* `LMDataset`: `batchify` / `get_batch` / `sample(manifest_id, i)` with the reference's offsets.
* `LMMetaTrainer`: the meta step.  The reference's loop cannot run on torch >= 2 (it back-propagates through parameter storage it
  has overwritten, see oracle/lm_refimpl.py), so the semantics implemented are the documented first-order reading: per task
  train pass at theta0 (hidden state carried, detached), clipped inner SGD step lr / meta_lr_factor, validation pass at theta', G =
  sum_i w_i grad val_i (w = (1-ratio)/(n-1), ..., ratio), clipped, plain SGD outer step.  Tasks are sharded over ranks like the ASR
  loop with ONE all-reduce of the flat G.  **Parity unpinned** against the reference loop; pinned against the oracle restatement.
* `LMEngine.evaluate`, `evaluate`, `evaluate_test`: validation / test loss of a batchified stream and the losses by language
  transition (lm/test.py:189-368), windows chunked into one recurrent call, sums in fp64 on the device;
  `LMMetaTrainer.train(valid_interval=...)` evaluates periodically, anneals lr, stops early and saves.
* `LMTrainer`: epoch training on one corpus (lm/main.py:244-333) and, on a loaded model, fine-tuning (lm/finetune.py:266-378);
  `LMJointTrainer`: the joint baseline (lm/main_joint.py:267-379), as written (`reference_zero_grad=True`: only the last task's
  gradient reaches the step) or accumulating; both step with mtl_sumsq + ONE mtl_sgd_clip_step and take the occurrence chains of a
  whole stream from ONE mtl_lm_window_chains launch.  Single rank only.
* `Dictionary`, `Corpus`, `batchify`: lm/util/data.py:69-195; `save_lm_checkpoint`: the file lmscore.LM loads for rescoring;
  `load_lm_checkpoint`: that file back into a trainable model and its dictionary.
No CPU fallback: without a GPU / the built library every compute call raises.
"""
import ctypes
import math
import os
import random
import time

import torch
import torch.nn as nn

from . import _lib, dist as mdist
from .data import is_contain_chinese_word
from .engine import ParamLayout

check = _lib.check
ACCUM = 2
MAX_KEYS = 4096        # MTL_NLL_MAX_KEYS of include/mtl_hip.h



def synth_corpus(seed, ntoken, length):
    """Zipf-ish synthetic token stream for benchmarks (the reference's ./data/*.txt corpora do not ship with it)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(length, generator=g)
    return (torch.floor((ntoken - 1) * u * u)).to(torch.int64).clamp_(0, ntoken - 1)


class RNNModel(nn.Module):
    def __init__(self, rnn_type, ntoken, ninp, nhid, nlayers, dropout=0.5, tie_weights=False):
        super().__init__()
        if rnn_type not in ('LSTM', 'GRU'):
            raise NotImplementedError("accelerated LM path: rnn_type 'LSTM' or 'GRU' (got %r)" % (rnn_type,))
        self.drop = nn.Dropout(dropout)
        self.encoder = nn.Embedding(ntoken, ninp)
        self.rnn = getattr(nn, rnn_type)(ninp, nhid, nlayers, dropout=dropout)   # parameter container only (same init draws)
        self.decoder = nn.Linear(nhid, ntoken)
        if tie_weights:
            # (lm/model/rnn_model.py:38-41) ONE Parameter under both names: named_parameters() and the flat layout list it once, as
            # encoder.weight; state_dict() keeps both keys
            if nhid != ninp:
                raise ValueError('When using the tied flag, nhid must be equal to emsize')
            self.decoder.weight = self.encoder.weight
        self.tie_weights = bool(tie_weights)
        self.rnn_type, self.ntoken, self.ninp, self.nhid, self.nlayers, self.dropout_rate = rnn_type, ntoken, ninp, nhid, nlayers, dropout
        self.init_weights()
        self._layout = ParamLayout([(n, p.shape) for n, p in self.named_parameters()])
        self.engine = None
        self._flatten()

    def init_weights(self):
        initrange = 0.1
        self.encoder.weight.data.uniform_(-initrange, initrange)
        self.decoder.bias.data.fill_(0)
        self.decoder.weight.data.uniform_(-initrange, initrange)

    def _flatten(self):
        params = list(self.named_parameters())
        device = params[0][1].device
        theta = torch.zeros(self._layout.total, dtype=torch.float32, device=device)
        gflat = torch.zeros_like(theta)
        for name, p in params:
            v = self._layout.view(theta, name)
            v.copy_(p.data)
            p.data = v
            p.grad = self._layout.view(gflat, name)
        self._theta, self._gflat = theta, gflat
        self.engine = LMEngine(self, device) if device.type == 'cuda' else None

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._flatten()
        return out

    @property
    def flat_parameters(self):
        return self._theta

    @property
    def flat_grad(self):
        return self._gflat

    def init_hidden(self, bsz):
        """(h, c) for an LSTM, a single tensor for a GRU (lm/model/rnn_model.py:64-70)"""
        dev = self._theta.device
        if self.rnn_type == 'GRU':
            return torch.zeros(self.nlayers, bsz, self.nhid, device=dev)
        return (torch.zeros(self.nlayers, bsz, self.nhid, device=dev), torch.zeros(self.nlayers, bsz, self.nhid, device=dev))

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError('the LM lives on %s: the product path needs an MI355X (call .cuda()); there is no CPU fallback'
                               % self._theta.device)
        return self.engine

    def forward(self, input, hidden):
        """-> (decoded (T, B, ntoken), hidden) like lm/model/rnn_model.py:52-60 (no autograd graph: use LMEngine.backward)"""
        eng = self._need_engine()
        out = eng.forward(self._theta, input, None, hidden, self.dropout_rate if self.training else 0.0)
        eng.check_handoff()          # the caller consumes the logits: a timed-out persistent launch must not pass as a result
        return out['logits'].view(input.shape[0], input.shape[1], self.ntoken), out['hidden']


class LMEngine:
    """Forward + hand-written backward of the LSTM / GRU LM as library calls on the current stream (rows are ordered (t, b))."""

    def __init__(self, model, device):
        self.m, self.device, self.lib, self.L = model, device, _lib.lib(), model._layout
        self.pool, self.saved = {}, None
        self.ws = torch.empty(4 << 20, dtype=torch.float32, device=device)
        # all T steps of a layer in ONE launch per direction (csrc/mtl_lstm.hip, csrc/mtl_gru.hip) where the shape is supported; False
        # keeps the per-step recurrent product + cell kernel (tests compare the two; unsupported shapes take it anyway)
        self.persistent = True
        # LSTM only: the whole stack as one wavefront launch per direction (layers one step apart); False: one launch per layer and
        # direction (a GRU always runs one launch per layer and direction)
        self.stacked = True
        self.sync_ws = torch.zeros(int(self.lib.mtl_lstm_layer_workspace()) // 4, dtype=torch.int32, device=device)
        self._persistent_issued = False

    def off(self, name):
        """offset of a parameter in the flat buffers; a tied model holds ONE tensor for encoder.weight and decoder.weight"""
        return self.L.off('encoder.weight' if (name == 'decoder.weight' and self.m.tie_weights) else name)

    def check_handoff(self):
        """The persistent LSTM / GRU kernels bound every grid-wide wait and set a sticky error word instead of hanging the device
        (e.g. when their workgroups could not all become resident).  Called wherever results leave the engine: RNNModel.forward
        (evaluation / inference), LMMetaTrainer.run_iteration, and by direct LMEngine users through results().  One 4-byte
        read-back (a host sync) -- skipped when no persistent launch has been issued since the last check."""
        if not self._persistent_issued:
            return
        self._persistent_issued = False
        if int(self.sync_ws[1]) != 0:
            self.sync_ws[1] = 0
            raise RuntimeError('mtl_lstm / mtl_gru: a grid-wide wait of a persistent recurrent-layer launch timed out; its results are '
                               'invalid (LMEngine.stacked = False / LMEngine.persistent = False select the per-layer / per-step launches)')

    def buf(self, name, shape, dtype=torch.float32):
        key = (name, tuple(int(v) for v in shape), dtype)
        t = self.pool.get(key)
        if t is None:
            t = torch.empty(key[1], dtype=dtype, device=self.device)
            self.pool[key] = t
        return t

    @property
    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def gemm(self, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, flags=0, rowsum=None):
        check(self.lib.mtl_gemm_f32_ex(self.stream, ta, tb, M, N, K, 1.0, A, lda, B, ldb, C, ldc, bias, None, 0, flags, 1, 1, 0, 0, 0, 0,
                                       0, 0, 0, 1, 0, 0, rowsum, 0, self.ws.data_ptr(), self.ws.numel() * 4, 0, 0), 'mtl_gemm_f32_ex')

    def _chains(self, ids_host):
        """occurrence chains for the deterministic embedding scatter-add (mtl_embed_bwd); runs on the device `ids_host` lives on"""
        flat = ids_host.reshape(-1)
        order = torch.argsort(flat, stable=True)
        srt = flat[order]
        same = torch.zeros_like(srt, dtype=torch.bool)
        same[1:] = srt[1:] == srt[:-1]
        first = torch.empty_like(flat, dtype=torch.int32)
        first[order] = (~same).to(torch.int32)
        nxt = torch.full_like(flat, -1, dtype=torch.int32)
        nxt[order[:-1]] = torch.where(same[1:], order[1:], torch.full_like(order[1:], -1)).to(torch.int32)
        return torch.stack([first, nxt])

    def forward(self, theta, x, y, hidden, dropout_p=0.0, chains=None, loss_out=None):
        """x (T, B) int64, y (T*B) int64 or None, hidden (h, c) each (L, B, H) -- for a GRU the single tensor h.  -> dict(logits
        (T*B, V), loss (1,) or None, hidden (detached new state, in the form it came in)).  chains: None, or a (2, T*B) int32 device
        view holding what _chains(x) gives (a slice of the trainers' chain_table()): _chains is then not run.  loss_out: None, or a (1,)
        fp32 device tensor the loss is written to instead of the engine's own buffer."""
        rec = self._recurrent(theta, x, hidden, dropout_p, chains=chains)
        m, lib, st = self.m, self.lib, self.stream
        T, B, xin = rec['T'], rec['B'], rec['last']
        R, H, V = T * B, m.nhid, m.ntoken
        P = theta.data_ptr()
        o = lambda n: P + 4 * self.off(n)
        logits = self.buf('logits', (R, V))
        self.gemm(0, 1, R, V, H, xin.data_ptr(), H, o('decoder.weight'), H, logits.data_ptr(), V, bias=o('decoder.bias'))
        loss = None
        if y is not None:
            gold = self.buf('gold', (R,), torch.int64)
            gold.copy_(y.detach().reshape(-1).to(torch.int64), non_blocking=True)
            lse, hyp, rowloss = self.buf('lse', (R,)), self.buf('hyp', (R,), torch.int64), self.buf('rowloss', (R,))
            loss = self.buf('loss', (1,)) if loss_out is None else loss_out
            check(lib.mtl_ce_argmax_fwd(st, logits.data_ptr(), gold.data_ptr(), R, V, V, -1, 0.0, R, None, lse.data_ptr(), hyp.data_ptr(),
                                        rowloss.data_ptr(), loss.data_ptr()), 'ce_fwd')     # nn.CrossEntropyLoss(): mean over all T*B rows
        self.saved = dict(theta=theta, **rec)
        return dict(logits=logits, loss=loss, hidden=rec['hn'].clone() if rec['cn'] is None else (rec['hn'].clone(), rec['cn'].clone()))

    def sequence_nll(self, theta, ids, targets):
        """Summed next-word NLL of a ragged batch (LM rescoring, utils/lm.py:112-136 of the reference, batched): ids (T, B) int64,
        targets (T, B) int64 with -1 after a sequence's end.  Eval-mode forward from the zero state (the LSTM / GRU is causal: the padding
        after a sequence's end cannot change its valid positions), then ONE fused vocabulary projection + log-sum-exp
        (mtl_lm_nll_fwd; the T B x V logits are never written).  -> seq_nll (B,) fp32 on the device.  Reuses forward()'s buffers:
        a pending backward() is invalidated."""
        m, lib = self.m, self.lib
        T, B = int(ids.shape[0]), int(ids.shape[1])
        if tuple(targets.shape) != (T, B):
            raise ValueError('targets must have the shape of ids (T, B)')
        R, H, V, NL = T * B, m.nhid, m.ntoken, m.nlayers
        self.saved = None
        zero = self.buf('nll_h0', (NL, B, H))
        zero.zero_()
        rec = self._recurrent(theta, ids, zero if m.rnn_type == 'GRU' else (zero, zero), 0.0)
        self.saved = None
        tgt = self.buf('nll_tgt', (R,), torch.int64)
        tgt.copy_(targets.detach().reshape(-1).to(torch.int64), non_blocking=True)
        row, seq = self.buf('nll_row', (R,)), self.buf('nll_seq', (B,))
        need = int(lib.mtl_lm_nll_workspace(R, V))
        ws = self.ws if need <= self.ws.numel() * 4 else self.buf('nll_ws', ((need + 3) // 4,))
        P = theta.data_ptr()
        check(lib.mtl_lm_nll_fwd(self.stream, rec['last'].data_ptr(), H, P + 4 * self.off('decoder.weight'), P + 4 * self.off('decoder.bias'),
                                 tgt.data_ptr(), R, H, V, B, row.data_ptr(), seq.data_ptr(), ws.data_ptr(), ws.numel() * 4), 'mtl_lm_nll_fwd')
        self.check_handoff()          # the caller ranks hypotheses by these values
        return seq.clone()

    def evaluate(self, theta, source, bptt, lang=None, eos_id=None, chunk_windows=None, rows=False):
        """Evaluation loss of a batchified stream (lm/main_meta_transfer.py:214-267, lm/test.py:189-241 `evaluate`; with `lang` the
        language-transition sums of lm/test.py:243-368 `evaluate_test`).  source (S, B) int64 on the device.  Evaluation mode (no dropout,
        whatever model.training says; no random number is drawn), hidden state zero at the start and carried from window to window.
        Windows start at i = 0, bptt, ... < S - 1; window w has T_w = min(bptt, S - 1 - i) steps and the targets source[i+1 : i+1+T_w];
        loss = sum_w T_w mean_w / S with mean_w the mean row NLL of window w (the reference divides by len(data_source) = S, not by the
        S - 1 predictions: kept).

        `chunk_windows` windows at a time run as ONE call of the recurrent half (T = chunk_windows bptt; the carried state makes that
        the same recurrence), the state is handed from chunk to chunk and a window is never split; the default keeps at most 8192 rows
        per chunk.  Per chunk: mtl_lm_nll_fwd (no logits written), mtl_nll_key_sum over equal segments of bptt B rows for the window
        sums and, with `lang` ((V,) uint8 on the device, 1 = a Chinese word) and `eos_id`, mtl_lm_switch_keys + mtl_nll_key_sum over
        the four transition classes 0 zh->zh, 1 zh->en, 2 en->zh, 3 en->en (pairs that touch <eos> are skipped).  All sums are fp64 on
        the device; ONE read-back at the end, after check_handoff().

        -> dict(loss: float, combined on the host in fp64 from the window sums; window_sum (W,) float64; class_sum (4,) float64 and
        class_count (4,) int64, or None without `lang`; row_logp (S - 1, B) fp32 on the device = -row_nll, only with rows=True).
        Like sequence_nll it reuses forward()'s buffers: a pending backward() is invalidated."""
        m, lib = self.m, self.lib
        if source.dim() != 2 or int(source.shape[0]) < 2:
            raise ValueError('source must be a batchified (S, B) stream with S >= 2')
        if lang is not None and eos_id is None:
            raise ValueError('evaluate(lang=...) needs eos_id: pairs that touch <eos> are not counted')
        S, B, bptt = int(source.shape[0]), int(source.shape[1]), int(bptt)
        if bptt < 1:
            raise ValueError('bptt must be positive')
        H, V, NL = m.nhid, m.ntoken, m.nlayers
        seg, W = bptt * B, (S - 1 + bptt - 1) // bptt
        cw = max(8192 // seg, 1) if chunk_windows is None else int(chunk_windows)
        cw = max(1, min(cw, W, MAX_KEYS))
        nchunk = (W + cw - 1) // cw
        self.saved = None
        src = self.buf('eval_src', (S, B), torch.int64)
        src.copy_(source.detach().to(torch.int64), non_blocking=True)
        if lang is not None:
            if tuple(lang.shape) != (V,) or lang.dtype != torch.uint8 or lang.device != src.device:
                raise ValueError('lang must be a (ntoken,) uint8 tensor on the device')
            key = self.buf('eval_key', (min(cw * seg, (S - 1) * B),), torch.int32)
        # ONE result blob: [window sums W f64 | class sums nchunk x 4 f64 | window counts W i32 | class counts nchunk x 4 i32]
        o_cs, o_wc, o_cc = 8 * W, 8 * W + 32 * nchunk, 12 * W + 32 * nchunk
        out = self.buf('eval_out', (o_cc + 16 * nchunk,), torch.uint8)
        row = self.buf('eval_row', ((S - 1) * B if rows else min(cw * seg, (S - 1) * B),))
        zero = self.buf('nll_h0', (NL, B, H))
        zero.zero_()
        hidden = zero if m.rnn_type == 'GRU' else (zero, zero)
        P = theta.data_ptr()
        for c in range(nchunk):
            i0 = c * cw * bptt
            T = min(cw * bptt, S - 1 - i0)
            R, nw = T * B, min(cw, W - c * cw)
            rec = self._recurrent(theta, src[i0:i0 + T], hidden, 0.0, for_backward=False)
            hidden = rec['hn'].clone() if rec['cn'] is None else (rec['hn'].clone(), rec['cn'].clone())
            ids_p, tgt_p = src.data_ptr() + 8 * i0 * B, src.data_ptr() + 8 * (i0 + 1) * B
            row_p = row.data_ptr() + (4 * i0 * B if rows else 0)
            need = int(lib.mtl_lm_nll_workspace(R, V))
            ws = self.ws if need <= self.ws.numel() * 4 else self.buf('nll_ws', ((need + 3) // 4,))
            check(lib.mtl_lm_nll_fwd(self.stream, rec['last'].data_ptr(), H, P + 4 * self.off('decoder.weight'), P + 4 * self.off('decoder.bias'),
                                     tgt_p, R, H, V, B, row_p, None, ws.data_ptr(), ws.numel() * 4), 'mtl_lm_nll_fwd')
            kws = self.buf('eval_kws', ((int(lib.mtl_nll_key_sum_workspace(R, max(nw, 4))) + 7) // 8,), torch.float64)
            check(lib.mtl_nll_key_sum(self.stream, row_p, None, seg, R, nw, out.data_ptr() + 8 * c * cw, out.data_ptr() + o_wc + 4 * c * cw,
                                      kws.data_ptr(), kws.numel() * 8), 'mtl_nll_key_sum (windows)')
            if lang is not None:
                check(lib.mtl_lm_switch_keys(self.stream, ids_p, tgt_p, lang.data_ptr(), int(eos_id), R, V, key.data_ptr()), 'mtl_lm_switch_keys')
                check(lib.mtl_nll_key_sum(self.stream, row_p, key.data_ptr(), 1, R, 4, out.data_ptr() + o_cs + 32 * c,
                                          out.data_ptr() + o_cc + 16 * c, kws.data_ptr(), kws.numel() * 8), 'mtl_nll_key_sum (classes)')
        self.saved = None
        if rows:
            check(lib.mtl_scale(self.stream, row.data_ptr(), -1.0, None, (S - 1) * B), 'mtl_scale')
        self.check_handoff()
        host = out.cpu().numpy()                                   # the one read-back
        window_sum = host[:o_cs].view('<f8').copy()
        res = dict(loss=float(window_sum.sum(dtype='f8') / (B * S)), window_sum=window_sum, class_sum=None, class_count=None)
        if lang is not None:
            res['class_sum'] = host[o_cs:o_wc].view('<f8').reshape(nchunk, 4).sum(axis=0)
            res['class_count'] = host[o_cc:].view('<i4').reshape(nchunk, 4).astype('i8').sum(axis=0)
        if rows:
            res['row_logp'] = row.view(S - 1, B).clone()
        return res

    def _recurrent(self, theta, x, hidden, dropout_p, for_backward=True, chains=None):
        """the recurrent half of forward(): embedding (+ dropout) and the LSTM stack over x (T, B) from `hidden` -> dict with the top
        layer's (dropped) output `last` (T B, H) and what backward() needs (for_backward=False: without the occurrence chains of the
        embedding scatter-add, which only backward() reads; chains=(2, T B) int32 on the device: taken as they are)"""
        m, lib, st = self.m, self.lib, self.stream
        T, B = int(x.shape[0]), int(x.shape[1])
        R, H, E, V, NL = T * B, m.nhid, m.ninp, m.ntoken, m.nlayers
        gru = m.rnn_type == 'GRU'
        P = theta.data_ptr()
        o = lambda n: P + 4 * self.off(n)
        # token ids and the occurrence chains of the embedding scatter-add: where the batch already lives (a device batch is indexed
        # with device ops -- a read-back here would drain the stream once per pass and leave the GPU idle while the host enqueues)
        xh = x.detach().to(torch.int64).contiguous()
        ids = self.buf('ids', (R,), torch.int64)
        ids.copy_(xh.reshape(-1), non_blocking=True)
        if chains is not None:
            if tuple(chains.shape) != (2, R) or chains.dtype != torch.int32 or chains.device != theta.device or chains.stride(1) != 1:
                raise ValueError('chains must be a (2, T*B) int32 view on the device with contiguous rows')
        elif for_backward:
            chains = self.buf('chains', (2, R), torch.int32)
            chains.copy_(self._chains(xh), non_blocking=True)
        sc = 1.0 / (1.0 - dropout_p) if dropout_p > 0 else 1.0
        seed = self.buf('seed', (1,), torch.int64)
        if dropout_p > 0:
            # (drawn from the generator of the batch's device: a pageable host tensor would make the copy wait for the stream)
            seed.copy_(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=xh.device), non_blocking=True)

        def mask(name, n, site):
            if dropout_p <= 0:
                return None
            t = self.buf(name, (n,), torch.uint8)
            check(lib.mtl_dropout_mask(st, t.data_ptr(), n, float(dropout_p), seed.data_ptr(), site << 40), 'mtl_dropout_mask')
            return t

        zpe = self.buf('zero_pe', (R, E))
        if not getattr(self, '_zpe_ok', None) == (R, E):
            zpe.zero_()
            self._zpe_ok = (R, E)
        # with E == H the inputs of the weight-gradient products -- per layer x_l (R x H) and the previous states hall_l[:T] (R x H)
        # -- live in ONE arena [layer][x, hall] with constant strides, and the gate gradients in one [layer] stack: backward() then
        # forms all 2 NL weight gradients (+ bias gradients) with a single batched product instead of 2 NL small ones (LSTM only: a
        # GRU's two gate-gradient tensors differ, see _gru_backward)
        arena = self.buf('wg_arena', (NL, 2, (T + 1) * B * H)) if (E == H and NL > 1 and not gru) else None
        emb = arena[0, 0, :R * E].view(R, E) if arena is not None else self.buf('emb', (R, E))
        m_emb = mask('m_emb', R * E, 1)
        check(lib.mtl_embed_pe_fwd(st, ids.data_ptr(), o('encoder.weight'), zpe.data_ptr(), emb.data_ptr(), R, R, E,
                                   m_emb.data_ptr() if m_emb is not None else None, sc), 'embed')
        if gru:
            layers, last, hn, fused = self._gru_forward(o, hidden, emb, mask, sc, T, B)
            return dict(T=T, B=B, layers=layers, last=last, m_emb=m_emb, sc=sc, ids=ids, chains=chains, stacked=False, arena=None, hn=hn,
                        cn=None, fused=fused)
        h0, c0 = hidden
        layers = []
        xin, kin = emb, E
        hn, cn = self.buf('hn', (NL, B, H)), self.buf('cn', (NL, B, H))
        stacked = self.persistent and self.stacked and NL > 1 and bool(lib.mtl_lstm_stack_supported(B, H, NL))
        desc = _lib.LstmStack() if stacked else None
        for l in range(NL):
            hall = arena[l, 1].view(T + 1, B, H) if arena is not None else self.buf('hall%d' % l, (T + 1, B, H))
            call = self.buf('call%d' % l, (T + 1, B, H))
            hall[0].copy_(h0[l])
            call[0].copy_(c0[l])
            acts = self.buf('acts%d' % l, (R, 4 * H))
            # this layer's output after its dropout (next layer's / decoder's input)
            xout = arena[l + 1, 0, :R * H].view(R, H) if (arena is not None and l + 1 < NL) else self.buf('xout%d' % l, (R, H))
            msk = mask('m_l%d' % l, R * H, 2 + l)
            whh, bhh = o('rnn.weight_hh_l%d' % l), o('rnn.bias_hh_l%d' % l)
            layers.append(dict(x=xin, kin=kin, hall=hall, call=call, acts=acts, mask=msk))
            if stacked:
                # every layer in ONE wavefront launch below: only layer 0 takes its input contributions from a product over all steps
                desc.w_ih[l], desc.b_ih[l], desc.w_hh[l], desc.b_hh[l] = o('rnn.weight_ih_l%d' % l), o('rnn.bias_ih_l%d' % l), whh, bhh
                desc.hall[l], desc.call[l], desc.acts[l], desc.xout[l] = hall.data_ptr(), call.data_ptr(), acts.data_ptr(), xout.data_ptr()
                desc.mask[l] = msk.data_ptr() if msk is not None else None
                desc.gx[l] = self.buf('gx%d' % l, (R, 4 * H)).data_ptr()
                xin, kin = xout, H
                continue
            gx = self.buf('gx%d' % l, (R, 4 * H))
            self.gemm(0, 1, R, 4 * H, kin, xin.data_ptr(), kin, o('rnn.weight_ih_l%d' % l), kin, gx.data_ptr(), 4 * H, bias=o('rnn.bias_ih_l%d' % l))
            gh = self.buf('gh', (B, 4 * H))
            fused = self.persistent and bool(lib.mtl_lstm_layer_supported(B, H))
            if fused:
                self._persistent_issued = True
                check(lib.mtl_lstm_layer_fwd(st, gx.data_ptr(), whh, bhh, hall.data_ptr(), call.data_ptr(), acts.data_ptr(), xout.data_ptr(),
                                             msk.data_ptr() if msk is not None else None, sc, T, B, H, self.sync_ws.data_ptr()),
                      'lstm_layer_fwd')
            for t in range(0 if fused else T):
                self.gemm(0, 1, B, 4 * H, H, hall[t].data_ptr(), H, whh, H, gh.data_ptr(), 4 * H, bias=bhh)
                check(lib.mtl_lstm_cell_fwd(st, gx.data_ptr() + 16 * t * B * H, gh.data_ptr(), call[t].data_ptr(),
                                            acts.data_ptr() + 16 * t * B * H, call[t + 1].data_ptr(), hall[t + 1].data_ptr(),
                                            xout.data_ptr() + 4 * t * B * H, msk.data_ptr() + t * B * H if msk is not None else None, sc,
                                            B, H), 'lstm_cell_fwd')
            xin, kin = xout, H
        if stacked:
            gx = self.buf('gx0', (R, 4 * H))
            self.gemm(0, 1, R, 4 * H, E, emb.data_ptr(), E, o('rnn.weight_ih_l0'), E, gx.data_ptr(), 4 * H, bias=o('rnn.bias_ih_l0'))
            self._persistent_issued = True
            check(lib.mtl_lstm_stack_fwd(st, ctypes.byref(desc), sc, T, B, H, NL, self.sync_ws.data_ptr()), 'lstm_stack_fwd')
        for l in range(NL):
            hn[l].copy_(layers[l]['hall'][T])
            cn[l].copy_(layers[l]['call'][T])
        return dict(T=T, B=B, layers=layers, last=xin, m_emb=m_emb, sc=sc, ids=ids, chains=chains, stacked=stacked, arena=arena, hn=hn, cn=cn)

    def _gru_forward(self, o, hidden, emb, mask, sc, T, B):
        """the GRU stack of _recurrent() (csrc/mtl_gru.hip): per layer ONE product for the input contributions of all T steps (T B x 3H,
        gates r | z | n), then ONE persistent launch for the T steps -- or, for unsupported shapes / persistent = False, per step the
        recurrent product + the cell kernel.  Saved per step: r | z | n | q (T B x 4H).  -> (layers, last, hn, persistent launches ran)"""
        m, lib, st = self.m, self.lib, self.stream
        R, H, NL = T * B, m.nhid, m.nlayers
        fused = self.persistent and bool(lib.mtl_gru_layer_supported(B, H))
        layers, hn = [], self.buf('hn', (NL, B, H))
        xin, kin = emb, m.ninp
        for l in range(NL):
            hall = self.buf('hall%d' % l, (T + 1, B, H))
            hall[0].copy_(hidden[l])
            acts, xout, gx = self.buf('acts%d' % l, (R, 4 * H)), self.buf('xout%d' % l, (R, H)), self.buf('gru_gx', (R, 3 * H))
            msk = mask('m_l%d' % l, R * H, 2 + l)
            mp = msk.data_ptr() if msk is not None else None
            whh, bhh = o('rnn.weight_hh_l%d' % l), o('rnn.bias_hh_l%d' % l)
            layers.append(dict(x=xin, kin=kin, hall=hall, acts=acts, mask=msk))
            self.gemm(0, 1, R, 3 * H, kin, xin.data_ptr(), kin, o('rnn.weight_ih_l%d' % l), kin, gx.data_ptr(), 3 * H, bias=o('rnn.bias_ih_l%d' % l))
            if fused:
                self._persistent_issued = True
                check(lib.mtl_gru_layer_fwd(st, gx.data_ptr(), whh, bhh, hall.data_ptr(), acts.data_ptr(), xout.data_ptr(), mp, sc, T, B, H,
                                            self.sync_ws.data_ptr()), 'gru_layer_fwd')
            gh = self.buf('gru_gh', (B, 3 * H))
            for t in range(0 if fused else T):
                self.gemm(0, 1, B, 3 * H, H, hall[t].data_ptr(), H, whh, H, gh.data_ptr(), 3 * H, bias=bhh)
                check(lib.mtl_gru_cell_fwd(st, gx.data_ptr() + 12 * t * B * H, gh.data_ptr(), hall[t].data_ptr(), acts.data_ptr() + 16 * t * B * H,
                                           hall[t + 1].data_ptr(), xout.data_ptr() + 4 * t * B * H, mp + t * B * H if mp is not None else None,
                                           sc, B, H), 'gru_cell_fwd')
            hn[l].copy_(hall[T])
            xin, kin = xout, H
        return layers, xin, hn, fused

    def _gru_backward(self, S, dx, o, g):
        """the GRU stack of backward(): dx = gradient of the top layer's (dropped) output -> gradient of the embedding output.  Per
        layer the gate gradients of all steps as TWO (T B x 3H) tensors -- dgx = [da_r, da_z, da_n] (input side) and dgh = [da_r, da_z,
        dq] (recurrent side): they differ in their last third, so bias_ih and bias_hh get different gradients -- then two products
        per layer for the weight (+ bias) gradients, issued in a fixed order on the stream (deterministic), and one for the input
        gradient."""
        m, lib, st = self.m, self.lib, self.stream
        T, B, sc = S['T'], S['B'], S['sc']
        R, H, NL = T * B, m.nhid, m.nlayers
        dgx, dgh = self.buf('gru_dgx', (R, 3 * H)), self.buf('gru_dgh', (R, 3 * H))
        for l in reversed(range(NL)):
            Ly = S['layers'][l]
            kin, hall, acts = Ly['kin'], Ly['hall'], Ly['acts']
            mp = Ly['mask'].data_ptr() if Ly['mask'] is not None else None
            whh = o('rnn.weight_hh_l%d' % l)
            if S['fused']:
                self._persistent_issued = True
                check(lib.mtl_gru_layer_bwd(st, dx.data_ptr(), mp, sc, whh, acts.data_ptr(), hall.data_ptr(), dgx.data_ptr(), dgh.data_ptr(),
                                            T, B, H, self.sync_ws.data_ptr()), 'gru_layer_bwd')
            dh_rec, carry = self.buf('dh_rec', (B, H)), self.buf('gru_carry', (B, H))
            for t in reversed(range(0 if S['fused'] else T)):
                first = t == T - 1
                check(lib.mtl_gru_cell_bwd(st, dx.data_ptr() + 4 * t * B * H, mp + t * B * H if mp is not None else None, sc,
                                           None if first else dh_rec.data_ptr(), None if first else carry.data_ptr(),
                                           acts.data_ptr() + 16 * t * B * H, hall[t].data_ptr(), dgx.data_ptr() + 12 * t * B * H,
                                           dgh.data_ptr() + 12 * t * B * H, carry.data_ptr(), B, H), 'gru_cell_bwd')
                if t > 0:
                    self.gemm(0, 0, B, H, 3 * H, dgh.data_ptr() + 12 * t * B * H, 3 * H, whh, H, dh_rec.data_ptr(), H)
            self.gemm(1, 0, 3 * H, H, R, dgh.data_ptr(), 3 * H, hall.data_ptr(), H, g('rnn.weight_hh_l%d' % l), H, flags=ACCUM,
                      rowsum=g('rnn.bias_hh_l%d' % l))
            self.gemm(1, 0, 3 * H, kin, R, dgx.data_ptr(), 3 * H, Ly['x'].data_ptr(), kin, g('rnn.weight_ih_l%d' % l), kin, flags=ACCUM,
                      rowsum=g('rnn.bias_ih_l%d' % l))
            dxin = self.buf('dx_in%d' % l, (R, kin))
            self.gemm(0, 0, R, kin, 3 * H, dgx.data_ptr(), 3 * H, o('rnn.weight_ih_l%d' % l), kin, dxin.data_ptr(), kin)
            dx = dxin
        return dx

    def backward(self, grad, scale=1.0):
        """grad (flat) += scale * dLoss/dtheta of the last forward (truncated BPTT over the window: no gradient into the incoming
        hidden state, which the reference detaches with repackage_hidden).  Tied weights: the projection's weight gradient and the
        embedding scatter-add accumulate into the one gradient tensor, in stream order."""
        S = self.saved
        if S is None:
            raise RuntimeError('backward() without a preceding forward() with targets')
        m, lib, st, Lo = self.m, self.lib, self.stream, self.L
        T, B, sc = S['T'], S['B'], S['sc']
        R, H, E, V, NL = T * B, m.nhid, m.ninp, m.ntoken, m.nlayers
        P, G = S['theta'].data_ptr(), grad.data_ptr()
        o = lambda n: P + 4 * self.off(n)
        g = lambda n: G + 4 * self.off(n)
        ldd = (V + 3) // 4 * 4
        dlog = self.buf('dlog', (R, ldd))
        check(lib.mtl_ce_bwd(st, self.pool[('logits', (R, V), torch.float32)].data_ptr(), self.pool[('lse', (R,), torch.float32)].data_ptr(),
                             self.pool[('gold', (R,), torch.int64)].data_ptr(), R, V, V, -1, 0.0, float(scale) / R, None, dlog.data_ptr(), ldd),
              'ce_bwd')
        last = S['last']
        self.gemm(1, 0, V, H, R, dlog.data_ptr(), ldd, last.data_ptr(), H, g('decoder.weight'), H, flags=ACCUM, rowsum=g('decoder.bias'))
        dx = self.buf('dx_out', (R, H))
        self.gemm(0, 0, R, H, V, dlog.data_ptr(), ldd, o('decoder.weight'), H, dx.data_ptr(), H)
        if m.rnn_type == 'GRU':
            self._embed_backward(S, self._gru_backward(S, dx, o, g), g)
            return
        stacked, arena = S['stacked'], S['arena']
        dGs = self.buf('dG_all', (NL, R, 4 * H))
        if stacked:
            desc = _lib.LstmStack()
            for l in range(NL):
                Ly = S['layers'][l]
                desc.w_ih[l], desc.w_hh[l] = o('rnn.weight_ih_l%d' % l), o('rnn.weight_hh_l%d' % l)
                desc.call[l], desc.acts[l] = Ly['call'].data_ptr(), Ly['acts'].data_ptr()
                desc.dG[l] = dGs[l].data_ptr()
                desc.mask[l] = Ly['mask'].data_ptr() if Ly['mask'] is not None else None
            scratch = self.buf('stack_scratch', (int(lib.mtl_lstm_stack_scratch(T, B, H, NL)) // 4,))
            self._persistent_issued = True
            check(lib.mtl_lstm_stack_bwd(st, ctypes.byref(desc), dx.data_ptr(), sc, scratch.data_ptr(), T, B, H, NL, self.sync_ws.data_ptr()),
                  'lstm_stack_bwd')
        for l in reversed(range(NL)):
            Ly = S['layers'][l]
            kin = Ly['kin']
            dG = dGs[l]
            dh_rec, dc = self.buf('dh_rec', (B, H)), [self.buf('dc_a', (B, H)), self.buf('dc_b', (B, H))]
            whh = o('rnn.weight_hh_l%d' % l)
            msk = Ly['mask']
            fused = stacked or (self.persistent and bool(lib.mtl_lstm_layer_supported(B, H)))
            if fused and not stacked:
                self._persistent_issued = True
                check(lib.mtl_lstm_layer_bwd(st, dx.data_ptr(), msk.data_ptr() if msk is not None else None, sc, whh, Ly['acts'].data_ptr(),
                                             Ly['call'].data_ptr(), dG.data_ptr(), T, B, H, self.sync_ws.data_ptr()), 'lstm_layer_bwd')
            for t in reversed(range(0 if fused else T)):
                first = t == T - 1
                check(lib.mtl_lstm_cell_bwd(st, dx.data_ptr() + 4 * t * B * H, msk.data_ptr() + t * B * H if msk is not None else None, sc,
                                            None if first else dh_rec.data_ptr(), None if first else dc[(t + 1) & 1].data_ptr(),
                                            Ly['acts'].data_ptr() + 16 * t * B * H, Ly['call'][t + 1].data_ptr(), Ly['call'][t].data_ptr(),
                                            dG.data_ptr() + 16 * t * B * H, dc[t & 1].data_ptr(), B, H), 'lstm_cell_bwd')
                if t > 0:
                    self.gemm(0, 0, B, H, 4 * H, dG.data_ptr() + 16 * t * B * H, 4 * H, whh, H, dh_rec.data_ptr(), H)
            # parameter gradients over all T steps at once; both bias gradients are colsum(dG)
            if arena is None:
                self.gemm(1, 0, 4 * H, H, R, dG.data_ptr(), 4 * H, Ly['hall'].data_ptr(), H, g('rnn.weight_hh_l%d' % l), H, flags=ACCUM,
                          rowsum=g('rnn.bias_hh_l%d' % l))
                self.gemm(1, 0, 4 * H, kin, R, dG.data_ptr(), 4 * H, Ly['x'].data_ptr(), kin, g('rnn.weight_ih_l%d' % l), kin, flags=ACCUM,
                          rowsum=g('rnn.bias_ih_l%d' % l))
            elif l == 0:
                # all layers' (weight_ih, weight_hh, bias_ih, bias_hh) gradients as ONE product batched over [layer][ih, hh]: A = dG_l
                # (shared by the pair), B = arena[l][x_l | hall_l], C / row sums at the parameters' own offsets (constant strides
                # because every layer has input width H here)
                po = lambda n: Lo.off(n)
                lay = po('rnn.weight_ih_l1') - po('rnn.weight_ih_l0')
                assert all(po('rnn.%s_l%d' % (n, q)) - po('rnn.%s_l0' % n) == q * lay for q in range(NL)
                           for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
                half = (T + 1) * B * H
                check(lib.mtl_gemm_f32_ex(st, 1, 0, 4 * H, H, R, 1.0, dGs.data_ptr(), 4 * H, arena.data_ptr(), H, g('rnn.weight_ih_l0'), H,
                                          None, None, 0, ACCUM, 2 * NL, 2, R * 4 * H, 0, 2 * half, half, lay,
                                          po('rnn.weight_hh_l0') - po('rnn.weight_ih_l0'), 0, 1, 0, 0, g('rnn.bias_ih_l0'), lay,
                                          self.ws.data_ptr(), self.ws.numel() * 4, 0, po('rnn.bias_hh_l0') - po('rnn.bias_ih_l0')),
                      'lstm weight gradients')
            if stacked and l > 0:
                continue                                          # the stack kernel has handed the input gradient down itself
            dxin = self.buf('dx_in%d' % l, (R, kin))
            self.gemm(0, 0, R, kin, 4 * H, dG.data_ptr(), 4 * H, o('rnn.weight_ih_l%d' % l), kin, dxin.data_ptr(), kin)
            dx = dxin
        self._embed_backward(S, dx, g)

    def _embed_backward(self, S, dx, g):
        """dx (T B, E) = gradient of the (dropped) embedding output -> scatter-add into encoder.weight's gradient, duplicates in row order"""
        m_emb = S['m_emb']
        check(self.lib.mtl_embed_bwd(self.stream, S['ids'].data_ptr(), S['chains'][0].data_ptr(), S['chains'][1].data_ptr(), dx.data_ptr(),
                                     g('encoder.weight'), S['T'] * S['B'], self.m.ninp, -1, m_emb.data_ptr() if m_emb is not None else None,
                                     S['sc']), 'embed_bwd')


class LMDataset(object):
    """lm/util/data.py:12-67"""

    def __init__(self, task_list, args):
        self.bptt, self.batch_size, self.args = args.bptt, args.batch_size, args
        self.task_list = [self.batchify(t, self.batch_size) for t in task_list]

    def batchify(self, data, bsz):
        nbatch = data.size(0) // bsz
        data = data.narrow(0, 0, nbatch * bsz).view(bsz, -1).t().contiguous()
        return data.cuda() if getattr(self.args, 'cuda', False) else data

    def get_batch(self, source, i, evaluation=False):
        seq_len = min(self.bptt, len(source) - 1 - i)
        return source[i:i + seq_len], source[i + 1:i + 1 + seq_len].reshape(-1)

    def sample(self, manifest_id, i):
        ids = self.task_list[manifest_id]
        tr_ids = ((i * self.bptt) % len(ids)) - (((i * self.bptt) % len(ids)) % self.bptt)
        val_ids = (((i + 1) * self.bptt) % len(ids)) - ((((i + 1) * self.bptt) % len(ids)) % self.bptt)
        return self.get_batch(ids, tr_ids) + self.get_batch(ids, val_ids)


def task_weights(n, ratio):
    """lm/main_meta_transfer.py:346-349 for n = 3; generalised: the LAST task (the target corpus) weighs `ratio`"""
    return [ratio if i == n - 1 else (1.0 - ratio) / max(n - 1, 1) for i in range(n)]


class LMMetaTrainer:
    """The meta step of lm/main_meta_transfer.py:277-411 in its documented first-order reading (module docstring)."""

    def __init__(self, model, lr=20.0, meta_lr_factor=3.0, clip=0.25, ratio=0.8):
        self.model, self.lr, self.meta_lr_factor, self.clip, self.ratio = model, lr, meta_lr_factor, clip, ratio
        th = model.flat_parameters
        self.g, self.G, self.theta1 = torch.zeros_like(th), torch.zeros_like(th), torch.empty_like(th)
        self.coef = torch.empty(1, dtype=torch.float32, device=th.device)
        self.clip_ws = torch.empty(2048, dtype=torch.float32, device=th.device)
        self.hidden = None

    def _clip(self, grad):
        lib, st = _lib.lib(), torch.cuda.current_stream(grad.device).cuda_stream
        check(lib.mtl_sumsq(st, grad.data_ptr(), grad.numel(), self.coef.data_ptr(), self.clip_ws.data_ptr(), 2, float(self.clip)), 'mtl_sumsq')
        check(lib.mtl_scale(st, grad.data_ptr(), 1.0, self.coef.data_ptr(), grad.numel()), 'mtl_scale')

    def run_iteration(self, task_batches, val_batch, n_tasks=None, task_ids=None):
        """task_batches: this rank's [(x (T,B), y (T*B))] with their GLOBAL task ids; val_batch: (x, y).  One all-reduce of G.
        -> (weighted validation loss, [train losses])   (single device sync at the end)"""
        m = self.model
        eng = m._need_engine()
        lib, dev = _lib.lib(), m.flat_parameters.device
        st = lambda: torch.cuda.current_stream(dev).cuda_stream
        n = n_tasks or len(task_batches)
        task_ids = list(range(len(task_batches))) if task_ids is None else task_ids
        w = task_weights(n, self.ratio)
        p = m.dropout_rate if m.training else 0.0
        theta0 = m.flat_parameters
        if self.hidden is None:
            self.hidden = m.init_hidden(task_batches[0][0].shape[1])
        self.G.zero_()
        tr_losses, val_losses = [], []
        for (x, y), tid in zip(task_batches, task_ids):
            self.g.zero_()
            out = eng.forward(theta0, x, y, self.hidden, p)                                   # meta-train forward (:322)
            tr_losses.append(out['loss'].clone())
            self.hidden = out['hidden']
            eng.backward(self.g, 1.0)
            if self.clip:
                self._clip(self.g)                                                            # (:335-336)
            check(lib.mtl_sgd_theta_prime(st(), theta0.data_ptr(), self.g.data_ptr(), self.lr / self.meta_lr_factor,
                                          self.theta1.data_ptr(), theta0.numel()), 'sgd')     # inner step (:337-338)
            out = eng.forward(self.theta1, val_batch[0], val_batch[1], self.hidden, p)        # meta-validation at theta' (:341)
            val_losses.append(out['loss'].clone())
            eng.backward(self.G, w[tid])                                                      # G += w_i * grad val_i
        mdist.allreduce_sum_(self.G)
        if self.clip:
            self._clip(self.G)                                                                # (:366-367)
        check(lib.mtl_axpy(st(), theta0.data_ptr(), self.G.data_ptr(), -float(self.lr), theta0.numel()), 'outer sgd')   # (:368)
        torch.cuda.synchronize(dev)
        eng.check_handoff()
        batch_loss = sum(w[tid] * float(v) for v, tid in zip(val_losses, task_ids))
        return batch_loss, [float(t) for t in tr_losses]

    def train(self, dataset, start_it, num_it, log_interval=200, valid_interval=None, val_data=None, test_data=None, save_path=None,
              dictionary=None, eval_bptt=None, patience=5):
        """loop of lm/main_meta_transfer.py:277-411: per iteration every task's train batch `sample(i, it)`, the shared validation
        batch `sample(-1, it)`; tasks sharded over ranks.

        valid_interval=None: no periodic evaluation, returns None.  With valid_interval (:370-411): at it % valid_interval == 0 and
        it > 0 the loss of `val_data` (and of `test_data` if given; batchified (S, B) streams, windows of eval_bptt or the dataset's
        bptt) is evaluated and printed, `anneal_step` decides -- a first or better validation loss is saved to `save_path` with
        save_lm_checkpoint(model, dictionary, save_path), any other divides self.lr by 4 -- and the loop stops after `patience`
        evaluations without improvement in a row.  The logged running loss is then reset only at an evaluation and divided by
        it % valid_interval (valid_interval when that is 0), as the reference does.  An evaluation changes nothing the training
        reads (self.hidden, model.training, no random numbers).  Under several ranks every rank evaluates the same data -- the
        replicas are identical, so is the decision -- and rank 0 writes the file and prints.
        -> dict(best_val_loss, evaluations [(it, val, test or None, lr after the decision)], stopped_early)"""
        rank, world = mdist.rank(), mdist.world_size()
        n = len(dataset.task_list)
        mine = mdist.shard_tasks(n, rank, world)
        dev = self.model.flat_parameters.device

        def step(it):
            _, _, vx, vy = dataset.sample(-1, it)
            batches = [dataset.sample(i, it)[:2] for i in mine]
            loss, _ = self.run_iteration([(x.to(dev), y.to(dev)) for x, y in batches], (vx.to(dev), vy.to(dev)), n, mine)
            return mdist.allreduce_scalars([loss], dev)[0]

        return _iteration_loop(self, step, start_it, num_it, log_interval, valid_interval, val_data, test_data, save_path, dictionary,
                               eval_bptt or dataset.bptt, patience)


def _iteration_loop(trainer, step, start_it, num_it, log_interval, valid_interval, val_data, test_data, save_path, dictionary, bptt,
                    patience):
    """What LMMetaTrainer.train and LMJointTrainer.train share (lm/main_meta_transfer.py:370-411 = lm/main_joint.py:338-379): the
    iterations `step(it) -> logged loss` with the running-loss line, the periodic evaluation, annealing of trainer.lr, saving and
    early stopping -- documented at LMMetaTrainer.train."""
    rank = mdist.rank()
    model = trainer.model
    dev = model.flat_parameters.device
    if valid_interval is not None:
        if int(valid_interval) < 1 or val_data is None:
            raise ValueError('train(valid_interval=...) needs a positive interval and val_data')
        if save_path is not None and dictionary is None:
            raise ValueError('train(save_path=...) needs the dictionary the checkpoint carries')
        val_data = val_data.to(dev)
        test_data = test_data.to(dev) if test_data is not None else None
    best, counter, evaluations, stopped = None, 0, [], False
    total, t0 = 0.0, time.time()
    model.train()
    for it in range(start_it, num_it):
        total += step(it)
        if it % log_interval == 0 and it > 0 and rank == 0:
            cur = total / (log_interval if valid_interval is None else (it % valid_interval or valid_interval))
            print('| it {:3d} | lr {:02.2f} | ms/batch {:5.2f} | word_loss {:5.2f} | avg ppl {:8.2f}'.format(
                it, trainer.lr, (time.time() - t0) * 1000 / log_interval, cur, math.exp(min(cur, 50.0))))
            t0 = time.time()
            if valid_interval is None:
                total = 0.0
        if valid_interval is None or it % valid_interval != 0 or it == 0:
            continue
        val = evaluate(model, val_data, bptt)
        test = evaluate(model, test_data, bptt) if test_data is not None else None
        if rank == 0:
            print('it {} | val loss {:5f} | ppl {:5f}'.format(it, val, math.exp(min(val, 50.0))))
            if test is not None:
                print('it {} | test loss {:5f} | ppl {:5f}'.format(it, test, math.exp(min(test, 50.0))))
        best, counter, trainer.lr, save, stop = anneal_step(best, counter, trainer.lr, val, patience)
        if save and save_path is not None and rank == 0:
            save_lm_checkpoint(model, dictionary, save_path)
        evaluations.append((it, val, test, trainer.lr))
        total = 0.0
        if stop:
            stopped = True
            break
    if valid_interval is None:
        return None
    return dict(best_val_loss=best, evaluations=evaluations, stopped_early=stopped)


def window_schedule(S, bptt):
    """[(i, T)] of lm/main.py:256-258 for a batchified stream of S rows: windows start at i = 0, bptt, ... < S - 1 and have
    T = min(bptt, S - 1 - i) steps (the last one is shorter, down to T = 1)."""
    S, bptt = int(S), int(bptt)
    if S < 2 or bptt < 1:
        raise ValueError('a stream needs S >= 2 rows and bptt >= 1')
    return [(i, min(bptt, S - 1 - i)) for i in range(0, S - 1, bptt)]


def _single_rank(what):
    if mdist.world_size() > 1:
        raise NotImplementedError('%s under several ranks: one stream with one chained hidden state cannot be sharded over tasks '
                                  '(splitting the batch columns over ranks is not built)' % what)


class _ClippedSGD:
    """What LMTrainer and LMJointTrainer share: the flat gradient (zero between steps), the step mtl_sumsq (mode 2) +
    mtl_sgd_clip_step, the running loss on the device and the occurrence-chain tables of the streams trained on."""

    def __init__(self, model, lr, clip):
        _single_rank(type(self).__name__)
        self.model, self.lr, self.clip = model, lr, clip
        th = model.flat_parameters
        self.g = torch.zeros_like(th)
        self.coef = torch.empty(1, dtype=torch.float32, device=th.device)
        self.clip_ws = torch.empty(2048, dtype=torch.float32, device=th.device)
        self.loss_acc = torch.zeros(1, dtype=torch.float32, device=th.device)
        self._tables = {}

    def _step(self, loss):
        """clip (skipped when self.clip is falsy) and theta <- theta - lr g; g = 0; loss_acc += loss ((1,) fp32 on the device or None)"""
        lib, th = _lib.lib(), self.model.flat_parameters
        st = torch.cuda.current_stream(th.device).cuda_stream
        if self.clip:
            check(lib.mtl_sumsq(st, self.g.data_ptr(), self.g.numel(), self.coef.data_ptr(), self.clip_ws.data_ptr(), 2, float(self.clip)),
                  'mtl_sumsq')
        check(lib.mtl_sgd_clip_step(st, th.data_ptr(), self.g.data_ptr(), float(self.lr), self.coef.data_ptr() if self.clip else None,
                                    th.numel(), loss.data_ptr() if loss is not None else None,
                                    self.loss_acc.data_ptr() if loss is not None else None), 'mtl_sgd_clip_step')

    def chain_table(self, source, bptt, slot=0):
        """(2, (S - 1) B) int32: mtl_lm_window_chains over the whole stream `source` ((S, B) int64, contiguous, on the device), kept
        under `slot` while the same tensor (unmodified) comes back; None for a stream whose windows exceed the kernel's cap -- the
        engine then builds each window's chains itself."""
        lib = _lib.lib()
        S, B = int(source.shape[0]), int(source.shape[1])
        if min(int(bptt), S - 1) * B > int(lib.mtl_lm_window_chains_max_rows()):
            return None
        key = (source.data_ptr(), S, B, int(bptt), source._version)
        ent = self._tables.get(slot)
        if ent is not None and ent[0] is source and ent[1] == key:
            return ent[2]
        table = torch.empty(2, (S - 1) * B, dtype=torch.int32, device=source.device)
        check(lib.mtl_lm_window_chains(torch.cuda.current_stream(source.device).cuda_stream, source.data_ptr(), S, B, int(bptt),
                                       table[0].data_ptr(), table[1].data_ptr()), 'mtl_lm_window_chains')
        self._tables[slot] = (source, key, table)
        return table


class LMTrainer(_ClippedSGD):
    """Epoch training on one corpus: the loop of lm/main.py:244-333, which lm/finetune.py:266-378 repeats on a loaded model
    (fine-tuning = load_lm_checkpoint -> LMTrainer(model, ...).train(...)).  Per window: forward at theta from the carried
    (detached) hidden state with the model's dropout, mean cross-entropy, backward, clip with min(1, clip / (|g| + 1e-6)) (skipped
    when `clip` is falsy), theta <- theta - lr g.  On the device a window is LMEngine.forward / backward, mtl_sumsq (mode 2) and ONE
    mtl_sgd_clip_step (scale + update + zeroing of g + the running loss); the occurrence chains of all windows come from ONE
    mtl_lm_window_chains launch per stream.  No device value is read on the host between two log points."""

    def __init__(self, model, lr=20.0, clip=0.25, bptt=35):
        super().__init__(model, lr, clip)
        self.bptt = int(bptt)

    def train_epoch(self, train_data, epoch=1, log_interval=200):
        """One pass over `train_data`, a batchified (S, B) int64 stream on the model's device, in windows window_schedule(S, bptt).
        model.train(); the hidden state is zero at the start and carried.  The running loss is an fp32 sum on the device, read (one
        host sync, after check_handoff()) at batch % log_interval == 0 and batch > 0, divided by log_interval -- the first interval
        holds log_interval + 1 losses, as in the reference -- printed in the reference's format and reset.
        -> dict(windows, losses (W,) fp32 on the device, hidden)"""
        _single_rank('LMTrainer')
        m = self.model
        eng = m._need_engine()
        theta = m.flat_parameters
        dev = theta.device
        if train_data.dim() != 2 or train_data.device != dev or train_data.dtype != torch.int64:
            raise ValueError("train_data must be a batchified (S, B) int64 stream on the model's device")
        src = train_data if train_data.is_contiguous() else train_data.contiguous()
        S, B = int(src.shape[0]), int(src.shape[1])
        sched = window_schedule(S, self.bptt)
        table = self.chain_table(src, self.bptt)
        m.train()
        p = m.dropout_rate
        hidden = m.init_hidden(B)
        losses = torch.zeros(len(sched), dtype=torch.float32, device=dev)
        self.g.zero_()
        self.loss_acc.zero_()
        t0 = time.time()
        for batch, (i, T) in enumerate(sched):
            loss = losses[batch:batch + 1]
            out = eng.forward(theta, src[i:i + T], src[i + 1:i + 1 + T].reshape(-1), hidden, p,
                              chains=table[:, i * B:(i + T) * B] if table is not None else None, loss_out=loss)
            hidden = out['hidden']
            eng.backward(self.g, 1.0)
            self._step(loss)
            if batch % log_interval == 0 and batch > 0:
                eng.check_handoff()
                cur = float(self.loss_acc) / log_interval
                print('| epoch {:3d} | {:5d}/{:5d} batches | lr {:02.2f} | ms/batch {:5.2f} | word_loss {:5.2f} | ppl {:8.2f}'.format(
                    epoch, batch, S // self.bptt, self.lr, (time.time() - t0) * 1000 / log_interval, cur, math.exp(min(cur, 50.0))))
                self.loss_acc.zero_()
                t0 = time.time()
        torch.cuda.synchronize(dev)
        eng.check_handoff()
        return dict(windows=len(sched), losses=losses, hidden=hidden)

    def train(self, train_data, val_data, epochs, test_data=None, save_path=None, dictionary=None, eval_bptt=None, patience=5,
              log_interval=200):
        """lm/main.py:292-336 (lm/finetune.py:330-378): per epoch train_epoch, then the loss of `val_data` (and of `test_data` if
        given; windows of eval_bptt or self.bptt) with the reference's end-of-epoch lines; `anneal_step` decides -- a first or better
        validation loss is saved to `save_path` with save_lm_checkpoint(model, dictionary, save_path), any other divides self.lr by 4
        -- and the loop stops after `patience` non-improvements in a row.  After the loop the best checkpoint's parameters (if one was
        saved) are loaded back into the model in place, and validation and test are evaluated once more.  A `dictionary` whose size
        is not model.ntoken (a corpus that added words to a loaded model's dictionary) raises ValueError before any training.
        -> dict(best_val_loss, epochs [(epoch, val, test or None, lr after the decision)], stopped_early, final_val, final_test)"""
        _single_rank('LMTrainer')
        m = self.model
        if save_path is not None and dictionary is None:
            raise ValueError('train(save_path=...) needs the dictionary the checkpoint carries')
        if dictionary is not None and len(dictionary) != m.ntoken:
            raise ValueError('the dictionary holds %d words, the model %d: a corpus that adds words cannot train this model'
                             % (len(dictionary), m.ntoken))
        dev = m.flat_parameters.device
        train_data, val_data = train_data.to(dev), val_data.to(dev)
        test_data = test_data.to(dev) if test_data is not None else None
        bptt = eval_bptt or self.bptt
        best, counter, log, stopped, saved = None, 0, [], False, False
        for epoch in range(1, int(epochs) + 1):
            t0 = time.time()
            self.train_epoch(train_data, epoch, log_interval)
            val = evaluate(m, val_data, bptt)
            test = evaluate(m, test_data, bptt) if test_data is not None else None
            print('-' * 89 + '\n' + '| end of epoch {:3d} | time: {:5.2f}s | valid loss {:5.2f} | valid ppl {:8.2f}'.format(
                epoch, time.time() - t0, val, math.exp(min(val, 50.0))) + '-' * 89)
            if test is not None:
                print('-' * 89 + '\n' + '| end of epoch {:3d} | time: {:5.2f}s | test loss {:5.2f} | test ppl {:8.2f}'.format(
                    epoch, time.time() - t0, test, math.exp(min(test, 50.0))) + '-' * 89)
            best, counter, self.lr, save, stop = anneal_step(best, counter, self.lr, val, patience)
            if save and save_path is not None:
                save_lm_checkpoint(m, dictionary, save_path)
                saved = True
            log.append((epoch, val, test, self.lr))
            if stop:
                stopped = True
                break
        if saved:
            state = torch.load(save_path, map_location='cpu', weights_only=False)['model_state_dict']
            with torch.no_grad():
                for name, prm in m.named_parameters():
                    prm.copy_(state[name])
        final_val = evaluate(m, val_data, bptt)
        final_test = evaluate(m, test_data, bptt) if test_data is not None else None
        print('=' * 89 + '| End of training | val loss {:5.2f} | val ppl {:8.2f}'.format(final_val, math.exp(min(final_val, 50.0))) + '=' * 89)
        if final_test is not None:
            print('=' * 89 + '| End of training | test loss {:5.2f} | test ppl {:8.2f}'.format(final_test, math.exp(min(final_test, 50.0)))
                  + '=' * 89)
        return dict(best_val_loss=best, epochs=log, stopped_early=stopped, final_val=final_val, final_test=final_test)


class LMJointTrainer(_ClippedSGD):
    """The joint baseline of lm/main_joint.py:267-379: per iteration every task's batch through ONE model, each task's forward from
    the hidden state the previous task's forward returned (one `hidden` threads through all tasks and all iterations), losses
    weighted with task_weights(n, ratio), then one clip and one SGD step with lr.  The logged loss is sum_i w_i L_i.

    reference_zero_grad is a choice of SEMANTICS, not of speed.  True reproduces the reference as written: its forward_one_batch
    calls model.zero_grad() before EVERY task's forward (lm/main_joint.py:271), so when the optimiser steps (:336) only the LAST
    task's weighted gradient is left -- the earlier tasks contribute their loss to the log and their hidden state to the chain, and
    nothing to the update; their backward is therefore not run.  False accumulates G = sum_i w_i g_i, the evident intent."""

    def __init__(self, model, lr=20.0, clip=0.25, ratio=0.8, reference_zero_grad=True):
        super().__init__(model, lr, clip)
        self.ratio, self.reference_zero_grad = ratio, bool(reference_zero_grad)
        self.hidden = None

    def run_iteration(self, task_batches, chains=None):
        """task_batches: [(x (T, B), y (T*B))] in task order; chains: None or per task None / the (2, T*B) slice of chain_table().
        -> (sum_i w_i L_i, [L_i])   (single device sync at the end)"""
        _single_rank('LMJointTrainer')
        m = self.model
        eng = m._need_engine()
        theta = m.flat_parameters
        n = len(task_batches)
        w = task_weights(n, self.ratio)
        p = m.dropout_rate if m.training else 0.0
        if self.hidden is None:
            self.hidden = m.init_hidden(task_batches[0][0].shape[1])
        losses = torch.zeros(n, dtype=torch.float32, device=theta.device)
        for i, (x, y) in enumerate(task_batches):
            out = eng.forward(theta, x, y, self.hidden, p, chains=chains[i] if chains is not None else None, loss_out=losses[i:i + 1])
            self.hidden = out['hidden']
            if i == n - 1 or not self.reference_zero_grad:
                eng.backward(self.g, w[i])
        self._step(None)
        torch.cuda.synchronize(theta.device)
        eng.check_handoff()
        host = [float(v) for v in losses.cpu()]
        return sum(wi * li for wi, li in zip(w, host)), host

    def train(self, dataset, start_it, num_it, log_interval=200, valid_interval=None, val_data=None, test_data=None, save_path=None,
              dictionary=None, eval_bptt=None, patience=5):
        """loop of lm/main_joint.py:275-379: per iteration every task's batch `dataset.sample(i, it)[:2]`; the running-loss line, the
        periodic evaluation, annealing, saving and stopping are LMMetaTrainer.train's (the same code).
        -> None without valid_interval, else dict(best_val_loss, evaluations, stopped_early)"""
        _single_rank('LMJointTrainer')
        dev = self.model.flat_parameters.device
        n, bptt = len(dataset.task_list), dataset.bptt
        streams = [t.to(dev).contiguous() for t in dataset.task_list]

        def step(it):
            batches, chains = [], []
            for i in range(n):
                S, B = int(streams[i].shape[0]), int(streams[i].shape[1])
                off = ((it * bptt) % S) - (((it * bptt) % S) % bptt)                  # LMDataset.sample's offset: a multiple of bptt
                x, y = dataset.get_batch(streams[i], off)
                table = self.chain_table(streams[i], bptt, slot=i)
                batches.append((x, y))
                chains.append(table[:, off * B:(off + int(x.shape[0])) * B] if table is not None else None)
            return self.run_iteration(batches, chains)[0]

        return _iteration_loop(self, step, start_it, num_it, log_interval, valid_interval, val_data, test_data, save_path, dictionary,
                               eval_bptt or bptt, patience)


def anneal_step(best, counter, lr, val, patience=5):
    """The decision after a validation (lm/main_meta_transfer.py:397-408): `not best or val < best` -- a first value, a better one,
    and (the reference's quirk, kept) any value after a best of exactly 0 -- is saved and resets the counter; anything else divides
    lr by 4 and counts.  -> (best, counter, lr, save, stop) with stop = counter == patience."""
    if not best or val < best:
        return val, 0, lr, True, False
    counter += 1
    return best, counter, lr / 4.0, False, counter == patience


class Dictionary(object):
    """lm/util/data.py:69-81"""

    def __init__(self):
        self.word2idx = {}
        self.idx2word = {}

    def add_word(self, word):
        if word not in self.word2idx:
            self.idx2word[len(self.idx2word)] = word
            self.word2idx[word] = len(self.idx2word) - 1
        return self.word2idx[word]

    def __len__(self):
        return len(self.idx2word)


class Corpus(object):
    """lm/util/data.py:83-195: `.train`, `.valid`, `.test` int64 id streams and `.train_lang`, ... (1 = a word that contains a Chinese
    character, else 0).  '<oov>' is added first; per line strip().lower(), ONE replace('  ', ' '), split(), '<eos>' appended.  Only the
    training file adds words: unknown words of the other two map to '<oov>'.  A `dictionary` passed in is extended (the reference
    chains its corpora this way)."""

    def __init__(self, train_path, valid_path=None, test_path=None, dictionary=None, seed=1000):
        random.seed(seed)
        self.dictionary = Dictionary() if dictionary is None else dictionary
        self.train, self.train_lang = self.tokenize(train_path, True)
        if valid_path is not None:
            self.valid, self.valid_lang = self.tokenize(valid_path, False)
        if test_path is not None:
            self.test, self.test_lang = self.tokenize(test_path, False)

    def tokenize(self, path, save, randomize=False):
        assert os.path.exists(path)
        d = self.dictionary
        d.add_word('<oov>')
        ids, langs = [], []
        with open(path, 'r') as f:
            lines = [line.strip().lower().replace('  ', ' ').split() + ['<eos>'] for line in f]
        if save:
            for words in lines:
                for word in words:
                    d.add_word(word)
        oov = d.word2idx['<oov>']
        for words in lines:
            for word in words:
                ids.append(d.word2idx.get(word, oov))
                langs.append(1 if is_contain_chinese_word(word) else 0)
        return torch.tensor(ids, dtype=torch.int64), torch.tensor(langs, dtype=torch.int64)


def batchify(data, bsz):
    """lm/util/data.py:25-34 as a free function: (N,) -> (N // bsz, bsz), column b = the b-th contiguous part (on data's device)"""
    nbatch = data.size(0) // bsz
    return data.narrow(0, 0, nbatch * bsz).view(bsz, -1).t().contiguous()


def language_table(dictionary, ntoken, device):
    """(ntoken,) uint8: 1 where the dictionary's word contains a Chinese character (mtl_lm_switch_keys' `lang`)"""
    lang = torch.zeros(ntoken, dtype=torch.uint8)
    for i, w in dictionary.idx2word.items():
        if i < ntoken and is_contain_chinese_word(w):
            lang[i] = 1
    return lang.to(device)


def evaluate(model, data_source, bptt=35):
    """lm/main_meta_transfer.py:214-267 -> the loss (LMEngine.evaluate; data_source: a batchified (S, B) stream)"""
    eng = model._need_engine()
    return eng.evaluate(model.flat_parameters, data_source.to(model.flat_parameters.device), bptt)['loss']


def evaluate_test(model, data_source, dictionary, bptt=35):
    """lm/test.py:243-368 with type_evaluation='test' -> the reference's 6-tuple in its order: (loss, zh->zh mean, zh->en mean,
    en->zh mean, en->en mean, switch-point mean = (zh->en sum + en->zh sum) / (both counts)).  The reference NAMES the second entry
    `en_en`, but its source_lang is True for a Chinese word: the first class is zh->zh.  Deviations: an empty class gives nan (the
    reference raises ZeroDivisionError), and any batch width works (the reference's squeeze() works for a width of 1 only)."""
    eng = model._need_engine()
    dev = model.flat_parameters.device
    res = eng.evaluate(model.flat_parameters, data_source.to(dev), bptt, lang=language_table(dictionary, model.ntoken, dev),
                       eos_id=dictionary.word2idx['<eos>'])
    s, c = [float(v) for v in res['class_sum']], [int(v) for v in res['class_count']]
    mean = lambda a, b: a / b if b else float('nan')
    return (res['loss'], mean(s[0], c[0]), mean(s[1], c[1]), mean(s[2], c[2]), mean(s[3], c[3]), mean(s[1] + s[2], c[1] + c[2]))


def save_lm_checkpoint(model, dictionary, path):
    """The dict of lm/convert.py:431-446, which lmscore.LM (and the reference's utils/lm.py LM) reads: model_state_dict (host copies;
    a tied model keeps both encoder.weight and decoder.weight), word2idx, idx2word, ntoken, ninp, nhid, nlayers, dropout and
    tie_weights -- the model's real flag, where the reference hard-codes True -- plus rnn_type."""
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.save(dict(model_state_dict=state, word2idx=dictionary.word2idx, idx2word=dictionary.idx2word,
                    ntoken=int(model.encoder.weight.size(0)), ninp=int(model.encoder.weight.size(1)), nhid=model.nhid,
                    nlayers=model.nlayers, dropout=model.drop.p, tie_weights=bool(model.tie_weights), rnn_type=model.rnn_type), path)


def load_lm_checkpoint(path, cuda=True):
    """save_lm_checkpoint's file (the form of lm/convert.py:431-446) back into a trainable model: an RNNModel of the saved rnn_type
    ('LSTM' when the key is missing, as in the reference's files) with the saved tie_weights, ntoken, ninp, nhid, nlayers and dropout,
    its state loaded strictly, and a Dictionary of the saved word2idx / idx2word.  ValueError when the dictionary's size is not
    ntoken.  -> (model, dictionary); cuda=True moves the model to the device (the product path), False leaves it on the host."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    dictionary = Dictionary()
    dictionary.word2idx, dictionary.idx2word = dict(ck['word2idx']), dict(ck['idx2word'])
    if len(dictionary) != int(ck['ntoken']) or len(dictionary.word2idx) != int(ck['ntoken']):
        raise ValueError('checkpoint %s: its dictionary holds %d words, its model %d' % (path, len(dictionary), int(ck['ntoken'])))
    model = RNNModel(ck.get('rnn_type', 'LSTM'), int(ck['ntoken']), int(ck['ninp']), int(ck['nhid']), int(ck['nlayers']),
                     float(ck['dropout']), bool(ck['tie_weights']))
    model.load_state_dict(ck['model_state_dict'], strict=True)
    return (model.cuda() if cuda else model), dictionary
