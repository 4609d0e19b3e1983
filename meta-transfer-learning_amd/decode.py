"""Test-time decoding on a PassEngine: the K/V-cached decoder session, greedy search, beam search ranked on the host
and beam search ranked on the device (modules/decoder.py:131-291).

Every function takes the engine as its first argument and issues calls into libmtl_hip.so through it (eng.lib, eng.stream, eng.buf,
eng.gemm ...: read at call time, a profiling proxy may stand in for eng.lib); PassEngine binds them as methods.  The call sequences
of a search are fixed per key, so they go through the engine's _lib.Replay instances: eager, recorded, replayed from C.
"""
import math

import numpy as np
import torch

from . import passplan
from ._lib import check
from .batchmeta import EOS_ID, PAD_ID

BEAM_ROWS = 16      # rows of a batched beam-search session: U = BEAM_ROWS // W utterances per chunk (DESIGN.md "Test-set evaluation")
BEAM_POLL = 4       # positions between two reads of the done flags


class _DecodeSession:
    """See decode_session."""

    def __init__(self, eng, theta, mem, B, T4, S, shared_memory, groups=1):
        self.eng, self.B, self.T4, self.S = eng, B, T4, S
        # groups > 1 (batched beam search): the B rows are `groups` utterances of B / groups hypothesis rows each, every utterance's
        # rows sharing ITS encoder memory -- mem is (groups, T4, d)
        self.groups = int(groups) if shared_memory else 1
        if B % self.groups:
            raise ValueError('rows do not divide into %d groups' % self.groups)
        hp = eng.hp
        d, r, h, dk, dv, V = hp.d, hp.r, hp.h, hp.dk, hp.dv, hp.V
        hk, hv = h * dk, h * dv
        if S > eng.pe_dec.shape[0] + 1:
            raise ValueError('tgt_max_len too small for %d decoding positions' % S)
        self.P = theta.data_ptr()
        buf = eng.buf
        self.x = buf('g.x', (B, d))
        # fast path (head sizes of the fused attention kernel, h d_k = h d_v): q / k / v of a layer's self-attention live in ONE (3, B, S, h d_k)
        # block -- row t of [0] is the current query, [1] / [2] are the K / V caches -- so that the three low-rank projections are two
        # strided-batch launches writing row t, and the attention over the cache is ONE flash-attention launch (keys beyond the current
        # position masked by a per-step length: row t of `klen_self`) instead of product + softmax + product
        self.fast = bool(eng.fused_attn and hk == hv and hp.n_dec > 0 and
                         passplan.qkv_groups(eng.L, 'decoder.layers.0.self_attn.', 1, 1, 1, 1, hk, hv)[0][0] == 'qkv')
        if self.fast:
            self.qkv = [buf('g.qkv%d' % i, (3, B, S, hk)) for i in range(hp.n_dec)]
            for c in self.qkv:
                eng.zero_(c)                                        # (masked keys are multiplied by probability 0: they must be finite)
            self.kc, self.vc = [c[1] for c in self.qkv], [c[2] for c in self.qkv]
            self.klen_self = buf('g.klen', (S, B), torch.int32)
            self.klen_self.copy_(torch.arange(1, S + 1, dtype=torch.int32).view(S, 1).expand(S, B))
            self.klen_cross = buf('g.klenx', (B,), torch.int32)
            self.klen_cross.fill_(T4)
            self.lse = buf('g.lse', (B, h, 1))
            # the weights do not move during a decode: every rank-r pair  y = (x W_a^T) W_b^T  is applied as ONE product with
            # W_b W_a (h d_k x d: 1 MB instead of 0.4 MB streamed per step, but one dependent launch instead of two -- a step is a
            # chain of launches, not a bandwidth problem); merged once per session from the current theta (6 small products per layer)
            self.Wqkv = [buf('g.wqkv%d' % i, (3, hk, d)) for i in range(hp.n_dec)]
            self.Wso = [buf('g.wso%d' % i, (d, hv)) for i in range(hp.n_dec)]
            self.Wcq = [buf('g.wcq%d' % i, (hk, d)) for i in range(hp.n_dec)]
            self.Wco = [buf('g.wco%d' % i, (d, hv)) for i in range(hp.n_dec)]
            for i in range(hp.n_dec):
                pre = 'decoder.layers.%d.' % i
                o = lambda n, pre=pre: self.P + 4 * eng.L.off(pre + n)
                sA_, sB_ = (passplan.pstride(eng.L, pre + 'self_attn.', 'qkv', sfx) for sfx in ('_linear_a.weight', '_linear_b.weight'))
                eng.gemm(0, 0, hk, d, r, o('self_attn.query_linear_b.weight'), r, o('self_attn.query_linear_a.weight'), d, self.Wqkv[i].data_ptr(), d,
                         batch=3, sA=(sB_, 0), sB=(sA_, 0), sC=(hk * d, 0))
                for att, dst in (('self_attn.', self.Wso[i]), ('encoder_attn.', self.Wco[i])):
                    eng.gemm(0, 0, d, hv, r, o(att + 'output_linear_b.weight'), r, o(att + 'output_linear_a.weight'), hv, dst.data_ptr(), hv)
                eng.gemm(0, 0, hk, d, r, o('encoder_attn.query_linear_b.weight'), r, o('encoder_attn.query_linear_a.weight'), d,
                         self.Wcq[i].data_ptr(), d)
        else:
            self.kc = [buf('g.kc%d' % i, (B, S, hk)) for i in range(hp.n_dec)]
            self.vc = [buf('g.vc%d' % i, (B, S, hv)) for i in range(hp.n_dec)]
        # --is-factorized: the feed-forward pairs are merged the same way, once per session (linear_1_b . linear_1_a -> (inner, d),
        # linear_2_b . linear_2_a -> (d, inner)): a step runs the dense model's two calls per layer on them
        self.ffn = []
        for i in range(hp.n_dec):
            o = lambda n, i=i: self.P + 4 * eng.L.off('decoder.layers.%d.pos_ffn.%s' % (i, n))
            if eng.factorized:
                w1, w2 = buf('g.wf1%d' % i, (hp.inner, d)), buf('g.wf2%d' % i, (d, hp.inner))
                eng.gemm(0, 0, hp.inner, d, r, o('linear_1_b.weight'), r, o('linear_1_a.weight'), d, w1.data_ptr(), d)
                eng.gemm(0, 0, d, hp.inner, r, o('linear_2_b.weight'), r, o('linear_2_a.weight'), hp.inner, w2.data_ptr(), hp.inner)
                self.ffn.append((w1.data_ptr(), o('linear_1_b.bias'), w2.data_ptr(), o('linear_2_b.bias')))
            else:
                self.ffn.append((o('linear_1.weight'), o('linear_1.bias'), o('linear_2.weight'), o('linear_2.bias')))
        Bm = self.groups if shared_memory else B
        self.cross_stride = 0 if shared_memory else T4
        self.ck = [buf('g.ck%d' % i, (Bm * T4, hk)) for i in range(hp.n_dec)]
        self.cv = [buf('g.cv%d' % i, (Bm * T4, hv)) for i in range(hp.n_dec)]
        self.ta, self.tq = buf('g.ta', (max(Bm * T4, B), r)), buf('g.q', (B, hk))
        self.to, self.tob = buf('g.o', (B, hv)), buf('g.ob', (B, d))
        self.y1, self.y2, self.y3 = buf('g.y1', (B, d)), buf('g.y2', (B, d)), buf('g.y3', (B, d))
        self.h1, self.h2 = buf('g.h1', (B, hp.inner)), buf('g.h2', (B, d))
        self.xhat, self.rstd = buf('g.xhat', (B, d)), buf('g.rstd', (B,))
        self.ldS = (max(S, T4) + 3) // 4 * 4
        self.Sc = buf('g.S', (B, h, 1, self.ldS))
        self.logits = buf('g.logits', (B, V))
        self.junk = buf('g.junk', (3 * B + 4,))
        self.zero_gold = buf('g.zero', (B,), torch.int64)
        self.zero_gold.zero_()
        self.cur = [buf('g.cur0', (B, d)), buf('g.cur1', (B, d))]
        self.last = None
        for i in range(hp.n_dec):                                   # cross-attention keys / values of the encoder output, once
            pre = 'decoder.layers.%d.encoder_attn.' % i
            self._lowrank(pre, 'key', mem, Bm * T4, self.ck[i].data_ptr())
            self._lowrank(pre, 'value', mem, Bm * T4, self.cv[i].data_ptr(), width=hv)

    def _lowrank(self, pre, name, src, rows, dst, ldc=None, width=None):
        eng, hp = self.eng, self.eng.hp
        hk, hv = hp.h * hp.dk, hp.h * hp.dv
        width = hk if width is None else width
        o = lambda n: self.P + 4 * eng.L.off(pre + n)
        eng.linear_fwd(src, rows, hp.d if name != 'output' else hv, o(name + '_linear_a.weight'), None, self.ta.data_ptr(), hp.r)
        eng.gemm(0, 1, rows, width, hp.r, self.ta.data_ptr(), hp.r, o(name + '_linear_b.weight'), hp.r, dst, ldc or width,
                 bias=o(name + '_linear_b.bias'))

    def _attend(self, q, kbuf, vbuf, kv_rows, k_stride, v_stride, out):
        # one query row per (b, h): scores over kv_rows keys, softmax, weighted sum of the values; k_stride / v_stride: floats from one
        # row's keys / values to the next row's (rows of h d_k and of h d_v floats: two numbers unless d_k = d_v), 0 for a shared memory
        eng, hp, B = self.eng, self.eng.hp, self.B
        h, dk, dv = hp.h, hp.dk, hp.dv
        hk, hv, ldS = h * dk, h * dv, self.ldS
        eng.gemm(0, 1, 1, kv_rows, dk, q, hk, kbuf, hk, self.Sc.data_ptr(), ldS, batch=B * h, H=h, sA=(hk, dk), sB=(k_stride, dk),
                 sC=(h * ldS, ldS))
        check(eng.lib.mtl_softmax_mask_fwd(eng.stream, self.Sc.data_ptr(), None, 0, 1.0 / float(hp.temperature), B, h, 1, kv_rows,
                                           ldS, None, 1.0, None), 'softmax')
        eng.gemm(0, 0, 1, dv, kv_rows, self.Sc.data_ptr(), ldS, vbuf, hv, out, hv, batch=B * h, H=h, sA=(h * ldS, ldS),
                 sB=(v_stride, dv), sC=(hv, dv))

    def _attend_groups(self, q, kbuf, vbuf, kv_rows, out):
        # cross-attention of `groups` utterances with W = B / groups query rows each: the same two strided-batch products and softmax
        # as _attend, batch = (utterance, head) with M = W rows per item instead of (row, head) with M = 1
        eng, hp, B, U = self.eng, self.eng.hp, self.B, self.groups
        h, dk, dv, W = hp.h, hp.dk, hp.dv, self.B // self.groups
        hk, hv, ldS = h * dk, h * dv, self.ldS
        eng.gemm(0, 1, W, kv_rows, dk, q, hk, kbuf, hk, self.Sc.data_ptr(), h * ldS, batch=U * h, H=h, sA=(W * hk, dk),
                 sB=(kv_rows * hk, dk), sC=(W * h * ldS, ldS))
        check(eng.lib.mtl_softmax_mask_fwd(eng.stream, self.Sc.data_ptr(), None, 0, 1.0 / float(hp.temperature), B, h, 1, kv_rows,
                                           ldS, None, 1.0, None), 'softmax')
        eng.gemm(0, 0, W, dv, kv_rows, self.Sc.data_ptr(), h * ldS, vbuf, hv, out, hv, batch=U * h, H=h, sA=(W * h * ldS, ldS),
                 sB=(kv_rows * hv, dv), sC=(W * hv, dv))

    def step(self, t, tok_ptr):
        """Feed the B tokens at device address tok_ptr as position t; leaves the logits of that position in self.logits."""
        eng, hp, B, S, T4 = self.eng, self.eng.hp, self.B, self.S, self.T4
        d, V = hp.d, hp.V
        hk, hv = hp.h * hp.dk, hp.h * hp.dv
        L, lib, P = eng.L, eng.lib, self.P
        check(lib.mtl_embed_pe_fwd(eng.stream, tok_ptr, P + 4 * L.off('decoder.trg_embedding.weight'),
                                   eng.pe_dec.data_ptr() + 4 * t * d, self.x.data_ptr(), B, 1, d, None, 1.0), 'embed')
        cur = self.x
        for i in range(hp.n_dec):
            pre = 'decoder.layers.%d.' % i
            o = lambda n: P + 4 * L.off(pre + n)
            sa = pre + 'self_attn.'
            if self.fast:
                sb_ = passplan.pstride(L, sa, 'qkv', '_linear_b.bias')
                qkv = self.qkv[i].data_ptr()
                eng.gemm(0, 1, B, hk, d, cur.data_ptr(), d, self.Wqkv[i].data_ptr(), d, qkv + 4 * t * hk, S * hk,
                         bias=o('self_attn.query_linear_b.bias'), batch=3, sB=(hk * d, 0), sC=(B * S * hk, 0), sbias=sb_)
                check(lib.mtl_attn_fwd(eng.stream, qkv + 4 * t * hk, self.kc[i].data_ptr(), self.vc[i].data_ptr(), S * hk, hk, hv,
                                       self.klen_self.data_ptr() + 4 * t * B, 0, 1.0 / float(hp.temperature), B, hp.h, 1, S, hp.dk, hp.dv, None, 0,
                                       1.0, self.to.data_ptr(), hv, self.lse.data_ptr()), 'mtl_attn_fwd')
            else:
                self._lowrank(sa, 'query', cur.data_ptr(), B, self.tq.data_ptr())
                self._lowrank(sa, 'key', cur.data_ptr(), B, self.kc[i].data_ptr() + 4 * t * hk, ldc=S * hk)      # row t of the cache
                self._lowrank(sa, 'value', cur.data_ptr(), B, self.vc[i].data_ptr() + 4 * t * hv, ldc=S * hv, width=hv)
                self._attend(self.tq.data_ptr(), self.kc[i].data_ptr(), self.vc[i].data_ptr(), t + 1, S * hk, S * hv, self.to.data_ptr())
            if self.fast:
                eng.gemm(0, 1, B, d, hv, self.to.data_ptr(), hv, self.Wso[i].data_ptr(), hv, self.tob.data_ptr(), d,
                         bias=o('self_attn.output_linear_b.bias'))
            else:
                self._lowrank(sa, 'output', self.to.data_ptr(), B, self.tob.data_ptr(), width=d)
            eng.ln_fwd(self.tob.data_ptr(), cur.data_ptr(), o('self_attn.layer_norm.weight'), o('self_attn.layer_norm.bias'), None, None,
                       self.y1.data_ptr(), self.xhat.data_ptr(), self.rstd.data_ptr(), B, 1)
            ca = pre + 'encoder_attn.'
            if self.fast:
                eng.gemm(0, 1, B, hk, d, self.y1.data_ptr(), d, self.Wcq[i].data_ptr(), d, self.tq.data_ptr(), hk,
                         bias=o('encoder_attn.query_linear_b.bias'))
            else:
                self._lowrank(ca, 'query', self.y1.data_ptr(), B, self.tq.data_ptr())
            if self.fast and self.cross_stride:      # (every row has its own memory: greedy search; beam search shares one with stride 0)
                check(lib.mtl_attn_fwd(eng.stream, self.tq.data_ptr(), self.ck[i].data_ptr(), self.cv[i].data_ptr(), hk, hk, hv,
                                       self.klen_cross.data_ptr(), 0, 1.0 / float(hp.temperature), B, hp.h, 1, T4, hp.dk, hp.dv, None, 0, 1.0,
                                       self.to.data_ptr(), hv, self.lse.data_ptr()), 'mtl_attn_fwd')
            elif self.groups > 1:
                self._attend_groups(self.tq.data_ptr(), self.ck[i].data_ptr(), self.cv[i].data_ptr(), T4, self.to.data_ptr())
            else:
                self._attend(self.tq.data_ptr(), self.ck[i].data_ptr(), self.cv[i].data_ptr(), T4, self.cross_stride * hk,
                             self.cross_stride * hv, self.to.data_ptr())
            if self.fast:
                eng.gemm(0, 1, B, d, hv, self.to.data_ptr(), hv, self.Wco[i].data_ptr(), hv, self.tob.data_ptr(), d,
                         bias=o('encoder_attn.output_linear_b.bias'))
            else:
                self._lowrank(ca, 'output', self.to.data_ptr(), B, self.tob.data_ptr(), width=d)
            eng.ln_fwd(self.tob.data_ptr(), self.y1.data_ptr(), o('encoder_attn.layer_norm.weight'), o('encoder_attn.layer_norm.bias'), None,
                       None, self.y2.data_ptr(), self.xhat.data_ptr(), self.rstd.data_ptr(), B, 1)
            w1, b1, w2, b2 = self.ffn[i]
            eng.linear_fwd(self.y2.data_ptr(), B, d, w1, b1, self.h1.data_ptr(), hp.inner, relu=True)
            eng.linear_fwd(self.h1.data_ptr(), B, hp.inner, w2, b2, self.h2.data_ptr(), d)
            nxt = self.cur[i & 1]                  # (the layer's output lands where the next layer reads it: no copy)
            eng.ln_fwd(self.h2.data_ptr(), self.y2.data_ptr(), o('pos_ffn.layer_norm.weight'), o('pos_ffn.layer_norm.bias'), None, None,
                       nxt.data_ptr(), self.xhat.data_ptr(), self.rstd.data_ptr(), B, 1)
            cur = nxt
        eng.gemm(0, 1, B, V, d, cur.data_ptr(), d, P + 4 * L.off('decoder.output_linear.weight'), d, self.logits.data_ptr(), V)
        return self.logits

    def argmax_into(self, dst_ptr):
        """arg-max of the current logits (lowest index on ties) written as B int64 at dst_ptr; log-sum-exp lands in junk[0:B]."""
        eng, B, V = self.eng, self.B, self.eng.hp.V
        check(eng.lib.mtl_ce_argmax_fwd(eng.stream, self.logits.data_ptr(), self.zero_gold.data_ptr(), B, V, V, PAD_ID, 0.0, 1, None,
                                        self.junk.data_ptr(), dst_ptr, self.junk.data_ptr() + 4 * B, self.junk.data_ptr() + 8 * B),
              'argmax')

    def logits_and_lse(self):
        """(B,V) logits and (B,) log-sum-exp of the current position on the host (one synchronising copy each)."""
        hyp = self.eng.buf('g.hyp', (self.B,), torch.int64)
        self.argmax_into(hyp.data_ptr())
        return self.logits.cpu(), self.junk[:self.B].cpu()

    def reorder(self, rows, t):
        """caches[r, :t] <- caches[rows[r], :t] for every layer (beam search: row r continues hypothesis rows[r])."""
        if list(rows) == list(range(self.B)):
            return
        idx = torch.tensor(rows, dtype=torch.int64, device=self.logits.device)
        for c in self.kc + self.vc:
            c[:, :t] = c.index_select(0, idx)[:, :t]

    def gather_tables(self):
        """device tables of the K / V cache addresses for mtl_beam_gather: [(table, caches, width)], one entry when h d_k = h d_v"""
        eng, hp = self.eng, self.eng.hp
        hk, hv = hp.h * hp.dk, hp.h * hp.dv
        sets = [(self.kc + self.vc, hk)] if hk == hv else [(self.kc, hk), (self.vc, hv)]
        out = []
        for j, (caches, width) in enumerate(sets):
            tab = eng.buf('g.tab%d' % j, (len(caches),), torch.int64)
            tab.copy_(torch.tensor([c.data_ptr() for c in caches], dtype=torch.int64))
            out.append((tab, len(caches), width))
        self.gtmp = eng.buf('g.gtmp', (max(n for _t, n, _w in out) * self.B * self.S * max(hk, hv),))
        return out

    def gather(self, tables, parent_ptr, t):
        """caches[r, :t] <- caches[parent[r], :t] for every layer, parent (B,) int32 in device memory (reorder() without the host)"""
        eng = self.eng
        for tab, n, width in tables:
            check(eng.lib.mtl_beam_gather(eng.stream, tab.data_ptr(), n, parent_ptr, self.gtmp.data_ptr(), self.gtmp.numel(), self.B, t, width,
                                          self.S * width), 'mtl_beam_gather')


def beam_unpack(state, U, W, S, start_token, eos_id):
    """host side of mtl_beam_rank's state (include/mtl_hip.h): per utterance the ended hypotheses in the order they ended, as dicts
    with 'score' (numpy fp32) and 'yseq' (start token ... EOS), rebuilt from the back-pointer and token tables"""
    state = np.ascontiguousarray(state, dtype=np.int32)
    o_bp = 4 * U + U * W
    o_tk = o_bp + U * S * W
    o_en = o_tk + U * S * W
    bp = state[o_bp:o_tk].reshape(U, S, W)
    tk = state[o_tk:o_en].reshape(U, S, W)
    en = state[o_en:o_en + 5 * U * S * W].reshape(U, S * W, 5)
    out = []
    for u in range(U):
        def seq(i, r):
            rev = []
            while i > 0:
                rev.append(int(tk[u, i - 1, r]))
                r = int(bp[u, i - 1, r])
                i -= 1
            return [int(start_token)] + rev[::-1]
        ended = []
        for e in en[u, :int(state[4 * u + 2])]:
            yseq = seq(int(e[0]), int(e[2])) + [int(e[3])] + ([int(eos_id)] if e[4] else [])
            ended.append(dict(score=e[1:2].view(np.float32)[0], yseq=yseq))
        out.append(ended)
    return out


def decode_session(eng, theta, mem, B, T4, S, shared_memory=False, groups=1):
    """K/V-cached incremental decoder over `B` hypothesis rows and up to `S` positions (greedy and beam search share it).
    mem: device pointer of the encoder output, (B, T4, d) -- or (1, T4, d) with shared_memory=True, when all rows are
    hypotheses of ONE utterance (beam search) and address the same cross-attention keys / values with batch stride 0."""
    return _DecodeSession(eng, theta, mem, B, T4, S, shared_memory, groups)


def greedy_decode(eng, theta, mem, B, T4, start_token, max_steps=300):
    """Decoder.greedy_search (modules/decoder.py:131-185) on the device: max_steps arg-max steps from `start_token`,
    no padding masks (the reference passes dec_enc_attn_mask=None and an all-ones non_pad_mask), only causality.
    The reference re-runs the whole decoder on the growing prefix at every step; here each layer keeps a K/V cache
    and only the new position is computed (same per-row arithmetic), and the chosen token is fed back through device
    memory, so the 300 steps run without a single host synchronisation.  Returns the (max_steps, B) int64 token ids."""
    if max_steps + 1 > eng.hp.tgt_max_len:
        raise ValueError('tgt_max_len too small for %d decoding steps' % max_steps)
    ses = eng.decode_session(theta, mem, B, T4, max_steps + 1)          # (eager: cache zeroing, cross-attention keys / values)
    ys = eng.buf('g.ys', (max_steps + 1, B), torch.int64)
    ys[0].fill_(int(start_token))

    def steps():
        for t in range(max_steps):
            ses.step(t, ys.data_ptr() + 8 * t * B)
            ses.argmax_into(ys.data_ptr() + 8 * (t + 1) * B)
    # The ~64 launches of a step cost the host more (8 us each through ctypes) than the device (a decode was host-bound at 0.53 ms
    # per step): the calls of all steps are recorded once per (parameters, shapes, buffers) into ONE command list -- every address is
    # fixed: the session's buffers come from the pool by name and shape -- and replayed from C (_lib.Replay, as
    # the trainer's schedules do for a task body: metastep._run_tasks).
    key = (theta.data_ptr(), int(mem), B, T4, max_steps, ys.data_ptr(), eng.stream, ses.fast)
    eng.replay_greedy.begin(eng, key)(0, steps)
    return ys[1:]


def beam_decode(eng, theta, mem_row, T4, start_token, beam_width, nbest, tgt_max_len, num_words, eos_id=EOS_ID, c_weight=1.0,
                ended_out=None):
    """Decoder.beam_search (modules/decoder.py:187-291, no LM rescoring) for ONE utterance: the host keeps the reference's
    hypothesis bookkeeping verbatim in behaviour (expansion order, stable sorts, cumulative truncation to the beam, EOS
    forced at step T' - 1, final_score = score + sqrt(num_words) * c_weight, fp32 score arithmetic); the device runs one
    K/V-cached decoder step for all live hypotheses per iteration (caches re-ordered by parent) and returns the last
    position's logits and log-sum-exp.  num_words(yseq) -> int is the caller's word counter (it needs the vocabulary).
    -> list of (yseq incl. start token and EOS, final_score) sorted best first, at most nbest.
    ended_out: a list that receives EVERY ended hypothesis in the order it ended, as dicts with 'score' (fp32, the decoder's
    log-probability) and 'yseq' (the caller's LM rescoring re-ranks them, modules/decoder.py:248-256)."""
    W = int(beam_width)
    steps = int(tgt_max_len)
    if steps > eng.pe_dec.shape[0] or W < 1:
        raise ValueError('bad beam search arguments')
    ses = eng.decode_session(theta, mem_row, W, T4, steps, shared_memory=True)
    toks = eng.buf('b.tok', (W,), torch.int64)
    hyp_buf = eng.buf('g.hyp', (W,), torch.int64)

    def body(i):
        ses.step(i, toks.data_ptr())
        ses.argmax_into(hyp_buf.data_ptr())                   # (leaves the log-sum-exp of the W rows in ses.junk[:W])
    # the device side of position i (one decoder step for the W rows + log-sum-exp) is the same call sequence for every utterance
    # (as greedy_decode's steps are; here the host ranks the hypotheses between two positions, so there is one replay unit per position)
    run = eng.replay_beam.begin(eng, ('beam', theta.data_ptr(), W, T4, steps, toks.data_ptr(), eng.stream, ses.fast))
    hyps = [dict(score=np.float32(0.0), yseq=[int(start_token)], row=0)]
    ended = []
    for i in range(steps):
        n = len(hyps)
        rows = [h['row'] for h in hyps] + [0] * (W - n)
        if i > 0:
            ses.reorder(rows, i)                              # row r of the caches <- its parent's rows 0..i-1
        toks.copy_(torch.tensor([h['yseq'][-1] for h in hyps] + [int(eos_id)] * (W - n), dtype=torch.int64))
        run(i, lambda: body(i))
        logits, lse = ses.logits.cpu(), ses.junk[:W].cpu()
        local = (logits[:n] - lse[:n].unsqueeze(1))           # F.log_softmax of the last position, fp32
        kept = []
        for r, h in enumerate(hyps):
            best, ids = torch.topk(local[r], W)
            for j in range(W):
                kept.append(dict(score=np.float32(h['score'] + np.float32(best[j].item())), yseq=h['yseq'] + [int(ids[j])], row=r))
            kept = sorted(kept, key=lambda x: x['score'], reverse=True)[:W]
        hyps = kept
        if i == T4 - 1:
            for h in hyps:
                h['yseq'] = h['yseq'] + [int(eos_id)]
        live = []
        for h in hyps:
            if h['yseq'][-1] == eos_id:
                h['final_score'] = np.float32(h['score'] + np.float32(math.sqrt(num_words(h['yseq'])) * c_weight))
                ended.append(h)
            else:
                live.append(h)
        hyps = live
        if not hyps:
            break
    if ended_out is not None:
        ended_out.extend(dict(score=h['score'], yseq=list(h['yseq'])) for h in ended)
    out = sorted(ended, key=lambda x: x['final_score'], reverse=True)[:min(len(ended), int(nbest))]
    return [(h['yseq'], float(h['final_score'])) for h in out]


def beam_chunk(eng, beam_width):
    """utterances per chunk of beam_decode_batch: U W <= BEAM_ROWS keeps every product of a step on the engine (and within the one
    row tile) that the W-row session of beam_decode uses"""
    return max(1, eng.BEAM_ROWS // int(beam_width))


def beam_decode_batch(eng, theta, mem_ptr, U, T4, start_token, beam_width, nbest, tgt_max_len, num_words, eos_id=EOS_ID, c_weight=1.0,
                      ended_out=None, chunk=None):
    """Decoder.beam_search for U utterances with the hypothesis bookkeeping on the device: per position one K/V-cached decoder step
    for the rows of a whole chunk of utterances, the log-sum-exp, mtl_beam_rank (candidates, stable global top-W, forced EOS, split
    into ended / live, back-pointers) and mtl_beam_gather (caches re-ordered by the parents the ranking left in device memory).
    The host reads no logits: every BEAM_POLL positions it reads the chunk's done flags (one stream synchronisation on a pinned
    copy), and after the search the ended lists and back-pointer tables in one copy, from which it rebuilds every yseq.
    mem_ptr: device address of the (U, T4, d) encoder output.  -> per utterance the list beam_decode returns ((yseq, final_score),
    best first, at most nbest); final_score = fp32(score + fp32(sqrt(num_words(yseq)) c_weight)) and the n-best sort stay on the
    host (num_words needs the vocabulary's strings).  ended_out: a list of U lists; list u receives every ended hypothesis of
    utterance u in the order it ended, as dicts with 'score' (fp32) and 'yseq'.  If tgt_max_len < T4 the loop ends without the
    forced EOS and unended hypotheses are dropped, as in the reference.  chunk: utterances per session (default beam_chunk(W))."""
    W, steps, U = int(beam_width), int(tgt_max_len), int(U)
    if steps > eng.pe_dec.shape[0] or W < 1 or steps < 1 or U < 1 or (ended_out is not None and len(ended_out) != U):
        raise ValueError('bad beam search arguments')
    Uc_max = eng.beam_chunk(W) if chunk is None else max(1, int(chunk))
    results = []
    for u0 in range(0, U, Uc_max):
        Uc = min(Uc_max, U - u0)
        got = _beam_chunk_search(eng, theta, int(mem_ptr) + 4 * u0 * T4 * eng.hp.d, Uc, T4, int(start_token), W, steps, int(eos_id))
        for u, ended in enumerate(got):
            for h in ended:
                h['final_score'] = np.float32(h['score'] + np.float32(math.sqrt(num_words(h['yseq'])) * c_weight))
            if ended_out is not None:
                ended_out[u0 + u].extend(dict(score=h['score'], yseq=list(h['yseq'])) for h in ended)
            out = sorted(ended, key=lambda x: x['final_score'], reverse=True)[:min(len(ended), int(nbest))]
            results.append([(h['yseq'], float(h['final_score'])) for h in out])
    return results


def _beam_chunk_search(eng, theta, mem, Uc, T4, start_token, W, steps, eos_id):
    """one chunk of beam_decode_batch -> per utterance the ended hypotheses (dicts: score fp32, yseq) in the order they ended"""
    V, B = eng.hp.V, Uc * W
    npos = min(steps, T4)                                     # (EOS is forced at position T4 - 1: no position beyond it)
    words = eng.lib.mtl_beam_state_words(Uc, W, npos)         # the tables cover the positions that can run, not tgt_max_len
    if words < 0:
        raise ValueError('beam search beyond the limits of mtl_beam_rank (include/mtl_hip.h)')
    ses = eng.decode_session(theta, mem, B, T4, steps, shared_memory=True, groups=Uc)
    tables = ses.gather_tables()
    state = eng.buf('bb.state', (words,), torch.int32)
    toks = eng.buf('bb.tok', (B,), torch.int64)
    parent = eng.buf('bb.par', (B,), torch.int32)
    hyp_buf = eng.buf('g.hyp', (B,), torch.int64)
    head = 4 * Uc + Uc * W                                    # hdr + score: all a search needs initialised
    init = np.zeros(head, dtype=np.int32)
    init[0:4 * Uc:4] = 1                                      # one live row (the start token) with score 0
    state[:head].copy_(torch.from_numpy(init))
    t0 = np.full((Uc, W), eos_id, dtype=np.int64)
    t0[:, 0] = start_token
    toks.copy_(torch.from_numpy(t0.reshape(-1)))
    K = eng.BEAM_POLL

    def body(i0):
        for i in range(i0, min(i0 + K, npos)):
            ses.step(i, toks.data_ptr())
            ses.argmax_into(hyp_buf.data_ptr())               # (leaves the log-sum-exp of the rows in ses.junk[:B])
            check(eng.lib.mtl_beam_rank(eng.stream, ses.logits.data_ptr(), ses.junk.data_ptr(), state.data_ptr(), toks.data_ptr(),
                                        parent.data_ptr(), i, T4, Uc, W, V, npos, eos_id), 'mtl_beam_rank')
            if i + 1 < npos:
                ses.gather(tables, parent.data_ptr(), i + 1)
    # every address of a block of K positions is fixed: one replay unit per block
    run = eng.replay_beam_batch.begin(eng, ('beamb', theta.data_ptr(), Uc, W, T4, steps, start_token, eos_id, toks.data_ptr(),
                                            state.data_ptr(), eng.stream, ses.fast))
    pin = eng.beam_pin
    if pin is None or pin.numel() < 4 * Uc:
        pin = eng.beam_pin = torch.empty(4 * max(Uc, 16), dtype=torch.int32).pin_memory()
    for i0 in range(0, npos, K):
        run(i0, lambda: body(i0))
        if i0 + K < npos:
            pin[:4 * Uc].copy_(state[:4 * Uc], non_blocking=True)
            torch.cuda.current_stream(eng.device).synchronize()
            if bool((pin[:4 * Uc].view(Uc, 4)[:, 1] != 0).all()):
                break
    host = state.cpu().numpy()                                # (synchronises: the one read-back of the chunk)
    return beam_unpack(host, Uc, W, npos, start_token, eos_id)
