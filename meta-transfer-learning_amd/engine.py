"""Pass executor: one forward + hand-written backward of the VGG-CNN + Transformer speech recogniser,
issued as calls into libmtl_hip.so on the current HIP stream.

PyTorch is used for device memory (a buffer arena of caller-owned tensors) and the stream handle only; every
arithmetic op of the pass is a kernel from include/mtl_hip.h.  Parameters live in ONE flat fp32 buffer
(`theta`, layout from `ParamLayout`); a pass reads parameters from any buffer with that layout (theta0 or the
inner-loop theta') and ACCUMULATES gradients into a second flat buffer (`.backward()` semantics, which the
reference's meta-gradient definition relies on -- SURVEY.md Q1).

What a pass computes follows the reference line by line:
  models/asr/transformer.py:120-149 (forward), modules/encoder.py:53-106, modules/decoder.py:71-115,293-323,
  modules/common_layers.py:110-132,238-331, utils/metrics.py:96-126.
"""
import functools
import os

import numpy as np
import torch

from . import _lib, _trace, convstack, decode, passplan
from ._lib import check
from .batchmeta import PAD_ID, SOS_ID, EOS_ID, batch_meta, decoder_io, ctc_input_lengths, enc_extent      # noqa: F401  (callers import the ids and the two helpers from here)
from .convstack import CENSUS_NAMES, CENSUS_SLOTS      # noqa: F401  (the bound slots of the h2 operands; the trainer's h2 guard names them)
from .decode import beam_unpack                         # noqa: F401
from .passplan import ACCUM, RELU, FULL as _FULL, round_width      # noqa: F401  (metastep.py imports round_width from here)
from .pool import BufferPool, LAYER_BUF as _LAYER_BUF


class ParamLayout:
    """name -> (offset, shape) inside the flat fp32 parameter buffer; offsets are 16-byte aligned."""

    def __init__(self, named_shapes):
        self.entries = {}
        self.order = []
        off = 0
        for name, shape in named_shapes:
            n = 1
            for s in shape:
                n *= int(s)
            self.entries[name] = (off, tuple(int(s) for s in shape), n)
            self.order.append(name)
            off += (n + 3) // 4 * 4
        self.total = off

    def off(self, name):
        return self.entries[name][0]

    def view(self, flat, name):
        off, shape, n = self.entries[name]
        return flat[off:off + n].view(shape)

    def group_bounds(self):
        """{'encoder' | 'decoder' | 'conv': (first, end) offsets in floats} of the three parameter groups in the flat buffers --
        parameters() order of models/asr/transformer.py is encoder, decoder, conv, so each group is one contiguous slice."""
        out, prev = {}, None
        for name in self.order:
            grp = name.split('.')[0]
            if grp != prev:
                if grp in out:
                    raise RuntimeError('parameter group %s is not contiguous in the flat layout' % grp)
                out[grp] = [self.off(name), self.total]
                if prev is not None:
                    out[prev][1] = self.off(name)
                prev = grp
        return {k: tuple(v) for k, v in out.items()}


class Hyper:
    def __init__(self, **kw):
        self.__dict__.update(kw)


LOSS_TYPES = ('ce', 'ctc')
STAGE_RING = 6      # pinned staging buffers per slot (prepare_tasks): > pipeline depth (default 2) + 2


class PassEngine(BufferPool):
    def __init__(self, layout, hp, device, pe_enc, pe_dec):
        super().__init__(device, {'d': hp.n_dec, 'e': hp.n_enc})     # arena, pool, the device's shared budget, scratch_epoch: pool.py
        self.pe_enc, self.pe_dec = pe_enc, pe_dec   # (max_len, d) fp32 device tables (non-trainable buffers)
        self.L = layout
        self.hp = hp
        self.lib = _lib.lib()
        # stand-alone passes on batches whose width changes from call to call are widened to repeating widths ('auto': from the second
        # width on; '0' never -- Transformer.evaluate; '1' always), to a multiple of MTL_RAGGED_QUANTUM frames
        self.widen, self.widen_quantum = 'auto', int(os.environ.get('MTL_RAGGED_QUANTUM', '64'))
        self._first_width, self._widths_vary = {}, False
        self.saved = None
        self.gemm_ws = torch.empty(8 << 20, dtype=torch.float32, device=device) if device.type == 'cuda' else None  # split-K slabs
        # weight/bias-gradient kernels are off the critical path (nothing downstream in the backward reads them): they run
        # on a second HIP stream with their own workspaces, forked once per block and joined at the end of the backward
        self.side = torch.cuda.Stream(device) if device.type == 'cuda' else None
        self.gemm_ws_side = torch.empty(8 << 20, dtype=torch.float32, device=device) if device.type == 'cuda' else None
        self.scratch_side = torch.empty(4 << 20, dtype=torch.float32, device=device) if device.type == 'cuda' else None
        self.on_side = False
        self._stage, self._stage_turn = {}, {}   # pinned host staging of prepare()
        self._events, self._ev_next = [], 0    # fork / join events of the side stream (raw handles: recordable library calls)
        self.dropout_p = 0.0          # set by the model: hp.dropout when model.training else 0
        self._site = 0                # dropout site counter of the current pass (Philox offset = site << 40)
        self.forward_hook = None      # optional callable(engine) after every forward has been enqueued (tests capture the arena)
        # optional callable(tag), tag in ('decoder', 'encoder', 'conv'): called by backward() -- at ENQUEUE time, eager run or command-list
        # replay alike -- right after the last kernel that writes that parameter group's gradients has been enqueued (on the main or
        # the side stream): the trainer starts the group's share of the meta-gradient all-reduce there (slice_bounds())
        self.slice_hook = None
        # h2 guard: a (tasks, CENSUS_SLOTS, 4) int64 device tensor while the trainer samples the census of the h2 operands against their
        # bounds (mtl_h2_census: non-zero elements / fewer than 22 bits / fewer than 16 bits; TransientTrainer.h2_check_every), else None
        self.census = None
        self.deferred = []
        self._wlog = {}
        # the weight gradients of all layers of a stack run as one strided-batch launch per parameter kind (flush_layer_wgrads); the
        # decoder's prologue (embedding + layer 0's self-attention block) depends on the labels and theta only: it runs on the side
        # stream under the encoder, and its backward (which feeds parameter gradients only) under the encoder's backward
        self.use_side_stream = True
        # 3x3 convolutions (forward, data gradient, weight gradient), MTL_CONV: 'h2' (default) two fp16 pieces per fp32 operand
        # (3 MFMAs per step, per-tensor power-of-two scaling from device scalars the producers deliver; csrc/mtl_h2.h), 'x3' three
        # exact bf16 pieces (6 MFMAs), 'f32' the fp32-MFMA engine
        self.conv_mode = os.environ.get('MTL_CONV', 'h2')
        if self.conv_mode not in ('h2', 'x3', 'f32'):
            raise ValueError('MTL_CONV must be h2, x3 or f32')
        self.conv_x3 = self.conv_mode != 'f32'
        self.conv_h2 = self.conv_mode == 'h2'
        self.conv_layers = convstack.layers_for(layout)     # vgg_cnn or large_cnn (the latter: always 'x3', convstack.decide); None: no convolutions
        self.time_shift = convstack.time_shift(layout)      # T frames -> enc_extent(T) encoder positions: T >> 2 behind a conv stack, T without one
        self._ln_pending, self._ln_tables = [], {}
        # the encoder's input Linear (5120 -> 512) with its data / weight gradient: 'h2' with the h2 convolutions (two fp16 pieces, the
        # bounds ride along), else the product engines' own routing (x3 / fp32); bench.py's exact-fp32 leg sets 'f32'
        self.in_linear = 'h2'
        # scaled-dot-product attention as ONE flash-style kernel forward and two backward (no score tensor in HBM); head sizes
        # outside mtl_attn_supported() take the batched-GEMM + softmax path
        self.fused_attn = device.type == 'cuda' and bool(self.lib.mtl_attn_supported(hp.dk, hp.dv))
        # task batching: a pass may carry the batches of `nt` tasks of a meta-step (rows of task t follow those of task t - 1); task t
        # reads its parameters at theta + t * sP floats (0: all tasks share theta0 -- the training passes) and accumulates its
        # gradients at grad + t * sG (see forward_device / backward)
        self.nt, self.sP, self.sG = 1, 0, 0
        # --is-factorized (model-wide: Hyper.factorized): the feed-forward Linears and the encoder's input Linear are rank-r pairs.
        # ffn_mid_fused: the two inner products of the factorized block (r -> inner with bias + ReLU, inner -> r) as the one streamed
        # kernel of csrc/mtl_ffn_lr.hip instead of two product calls; OFF by default -- see DESIGN.md section 20 for the measurement the
        # default follows.  Shapes outside mtl_ffn_lr_mid_supported take the two calls either way.
        # forward_only (set around passes that no backward follows: in-loop validation, Transformer.evaluate): the fused kernel then
        # does not store the post-ReLU activation, and a backward() after such a pass raises
        self.factorized = bool(getattr(hp, 'factorized', False))
        self.ffn_mid_fused = False
        self.forward_only = False
        self.prof = None    # set (to anything) while a profiling proxy stands in for self.lib: replay / graphs / lane tricks are bypassed
        # recorded call sequences of the searches (decode.py): greedy (one unit per decode), host-ranked beam (one per position),
        # device-ranked beam (one per block of BEAM_POLL positions); beam_pin: pinned read-back of the latter's done flags
        self.replay_greedy, self.replay_beam, self.replay_beam_batch = (_lib.Replay(n) for n in (4, 2, 4))
        self.beam_pin = None
        if device.type != 'cuda':
            raise RuntimeError('PassEngine needs an MI355X device (got %s); there is no CPU product path' % device)

    # ---------------------------------------------------------------- plumbing
    def _pool_invalidated(self):
        self._ln_tables.clear()     # device tables keyed by buffer addresses (LayerNorm reductions): rebuilt on demand

    def trim_pool(self):
        """BufferPool.trim_pool (start of a pass: count it, evict while over budget), and the bound on the engine's own tables"""
        freed = super().trim_pool()
        if len(self._ln_tables) > 512:
            # descriptor tables are keyed by addresses AND extents: ragged batches bring new ones with every pass.  Recorded command
            # lists hold the tables' addresses, hence the epoch.
            self._ln_tables.clear()
            self.scratch_epoch += 1
        return freed

    def enc_extent(self, frames):
        """encoder positions of a batch `frames` wide (batchmeta.enc_extent at this model's time reduction)"""
        return enc_extent(int(frames), self.time_shift)

    def scratch(self, nbytes):
        if self.on_side:
            if nbytes > self.scratch_side.numel() * 4:
                raise RuntimeError('side-stream scratch too small for %d bytes' % nbytes)
            return self.scratch_side.data_ptr()
        return super().scratch(nbytes)

    @property
    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def gemm(self, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, gate=None, ldg=0, flags=0, alpha=1.0,
             batch=1, H=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), sbias=0, kbatch=1, sAk=0, sBk=0, rowsum=None, srow=0, sbias_h=0, srow_h=0,
             task=None):
        """kbatch / sAk / sBk: sum over several (A, B) pairs inside one launch; rowsum: += row sums of op(A) (bias gradient);
        sbias / srow stride the OUTER batch index z // H, sbias_h / srow_h the inner one z % H.
        task = (sAt, sBt, sCt, sbias_t, srow_t): strides of the task index of a task-batched pass (the product is issued once with
        `batch` items PER TASK; mandatory when the pass carries several tasks)."""
        wst = self.gemm_ws_side if self.on_side else self.gemm_ws
        if self.nt == 1:
            check(self.lib.mtl_gemm_f32_ex(self.stream, ta, tb, M, N, K, alpha, A, lda, B, ldb, C, ldc, bias, gate, ldg, flags,
                                           batch, H, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], sbias, kbatch, sAk, sBk, rowsum, srow,
                                           wst.data_ptr(), wst.numel() * 4, sbias_h, srow_h), 'mtl_gemm_f32_ex')
            return
        if task is None:
            raise RuntimeError('task strides missing for a product of a task-batched pass')
        check(self.lib.mtl_gemm_f32_tb(self.stream, ta, tb, M, N, K, alpha, A, lda, B, ldb, C, ldc, bias, gate, ldg, flags,
                                       batch * self.nt, H, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], sbias, kbatch, sAk, sBk, rowsum,
                                       srow, wst.data_ptr(), wst.numel() * 4, sbias_h, srow_h, self.nt, *task), 'mtl_gemm_f32_tb')

    # ---- byte-level helpers and flat-vector updates as LIBRARY calls (a task body made of library calls only can be recorded
    # into a command list and replayed from C; torch's own fill / copy kernels cannot)
    def zero_(self, t):
        check(self.lib.mtl_memset_zero(self.stream, t.data_ptr(), t.numel() * t.element_size()), 'mtl_memset_zero')

    def copy_(self, dst, src):
        assert dst.numel() * dst.element_size() == src.numel() * src.element_size()
        check(self.lib.mtl_memcpy_d2d(self.stream, dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size()), 'mtl_memcpy_d2d')

    def axpy_(self, y, x, a):
        check(self.lib.mtl_axpy(self.stream, y.data_ptr(), x.data_ptr(), float(a), y.numel()), 'mtl_axpy')

    def sgd_theta_prime(self, theta0, g, lr, out):
        check(self.lib.mtl_sgd_theta_prime(self.stream, theta0.data_ptr(), g.data_ptr(), float(lr), out.data_ptr(), theta0.numel()),
              'mtl_sgd_theta_prime')

    def _event(self):
        """next event handle of a small ring (an event may be re-recorded once its earlier waits have been ENQUEUED: a wait binds
        to the record that precedes it in host order)"""
        if not self._events:
            for _ in range(8):
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))       # materialises the hipEvent_t
                self._events.append(ev)
        ev = self._events[self._ev_next]
        self._ev_next = (self._ev_next + 1) % len(self._events)
        return ev.cuda_event

    # ---- weight gradients
    def wgrad(self, dy, x, rows, n_out, k_in, dw, db=None, kind=None):
        """dw (n_out x k_in) += dy^T x ; db += colsum(dy).  With `kind` (the parameter's name without its layer index) the product is
        only LOGGED: flush_layer_wgrads() issues the products of all layers of a stack as one strided-batch launch per kind.
        Otherwise it goes to the side stream as a single call."""
        if kind is not None:
            self.wgrad_job(kind, n_out, k_in, rows, dy, n_out, x, k_in, dw, k_in, rowsum=db)
            return
        self.defer(lambda: self.gemm(1, 0, n_out, k_in, rows, dy, n_out, x, k_in, dw, k_in, flags=ACCUM, rowsum=db,
                                     task=(rows * n_out, rows * k_in, self.sG, 0, self.sG)))

    def wgrad_job(self, kind, M, N, K, A, lda, B, ldb, C, ldc, n=1, sA=0, sB=0, sC=0, rowsum=None, srow=0):
        """log C_z (M x N) += A_z^T B_z (z < n, strides in floats), rowsum_z += row sums of A_z^T"""
        self._wlog.setdefault((kind, M, N, K, lda, ldb, ldc, n, sA, sB, sC, srow, rowsum is not None), []).append(
            (int(C), int(A), int(B), int(rowsum or 0)))

    def flush_layer_wgrads(self):
        """Issue the logged weight-gradient products on the side stream: one strided-batch launch per kind where the layers'
        pointers advance by constant strides (passplan.merge_wgrad_jobs)."""
        log, self._wlog = self._wlog, {}
        for a, kw in passplan.merge_wgrad_jobs(log, self.sG):
            self.defer(functools.partial(self.gemm, *a, **kw))
        self.flush_side()

    # ---- side stream: deferred parameter-gradient work
    def defer(self, fn):
        if self.use_side_stream:
            self.deferred.append(fn)
        else:
            fn()

    def flush_side(self):
        """Everything enqueued on the main stream so far is visible to the deferred jobs, which are now issued on the side
        stream.  Their inputs are per-block buffers that the main stream never rewrites within this backward."""
        if not self.deferred:
            return
        ev = self._event()
        check(self.lib.mtl_event_record(ev, self.stream), 'mtl_event_record')
        jobs, self.deferred = self.deferred, []
        self._issue_side(ev, jobs)

    def _issue_side(self, ev, jobs):
        check(self.lib.mtl_stream_wait_event(self.side.cuda_stream, ev), 'mtl_stream_wait_event')
        with torch.cuda.stream(self.side):
            self.on_side = True
            try:
                for fn in jobs:
                    fn()
            finally:
                self.on_side = False

    def run_on_side(self, fn):
        """fn() with the side stream current, behind everything the main stream has enqueued so far; returns (fn's result, event
        handle recorded on the side stream after it -- wait_side_event() makes the main stream wait for it)"""
        ev = self._event()
        check(self.lib.mtl_event_record(ev, self.stream), 'mtl_event_record')
        check(self.lib.mtl_stream_wait_event(self.side.cuda_stream, ev), 'mtl_stream_wait_event')
        with torch.cuda.stream(self.side):
            self.on_side = True
            try:
                out = fn()
            finally:
                self.on_side = False
            done = self._event()
            check(self.lib.mtl_event_record(done, self.side.cuda_stream), 'mtl_event_record')
        return out, done

    def wait_side_event(self, ev):
        check(self.lib.mtl_stream_wait_event(self.stream, ev), 'mtl_stream_wait_event')

    def join_side(self):
        self.flush_side()
        if self.use_side_stream:
            ev = self._event()
            check(self.lib.mtl_event_record(ev, self.side.cuda_stream), 'mtl_event_record')
            check(self.lib.mtl_stream_wait_event(self.stream, ev), 'mtl_stream_wait_event')

    def slice_bounds(self):
        """ParamLayout.group_bounds(): the three parameter groups' slices of the flat buffers"""
        return self.L.group_bounds()

    def _slice_done(self, tag):
        if self.slice_hook is None:
            return
        # every kernel that writes this group's gradients must have been ENQUEUED
        if self.deferred:
            raise RuntimeError('slice %r handed over with weight-gradient launches still pending' % tag)
        if isinstance(self.lib, _lib.Recorder):
            self.lib.segment_break(tag)        # the replay stops here and hands control to the same hook
        self.slice_hook(tag)

    def linear_fwd(self, x, rows, k_in, w, b, y, n_out, relu=False):
        """rows: per task; the rows of task t are x + t * rows * k_in, its weights w + t * sP"""
        self.gemm(0, 1, rows, n_out, k_in, x, k_in, w, k_in, y, n_out, bias=b, flags=RELU if relu else 0,
                  task=(rows * k_in, self.sP, rows * n_out, self.sP, 0))

    def linear_bwd(self, x, dy, rows, k_in, n_out, w, dw, db, dx, dx_accum, gate=None, kind=None):
        """dw += dy^T x ; db += colsum(dy) (db None: no bias, or already produced by the LayerNorm backward) ;
        dx (=|+=) dy.W  (gate: ReLU mask source for dx)"""
        self.wgrad(dy, x, rows, n_out, k_in, dw, db, kind=kind)     # db rides on the weight-gradient product (row sums of dy^T)
        if dx is not None:
            self.gemm(0, 0, rows, k_in, n_out, dy, n_out, w, k_in, dx, k_in, gate=gate, ldg=k_in,
                      flags=ACCUM if dx_accum else 0, task=(rows * n_out, self.sP, rows * k_in, 0, 0))

    def _census(self, slot, t, amax_ptr):
        """add the census of the stacked h2 operand `t` (tasks x equal shares) against bound slot `slot` of every task"""
        if self.census is None or amax_ptr is None:
            return
        n = t.numel() // self.nt
        check(self.lib.mtl_h2_census(self.stream, t.data_ptr(), n, amax_ptr, self.census.data_ptr() + 32 * slot, self.nt, n,
                                     convstack.AMAX_STRIDE, 4 * CENSUS_SLOTS), 'mtl_h2_census')

    def colsum(self, x, rows, cols, out, amax=None):
        ws = self.scratch(self.lib.mtl_colsum_workspace(rows, cols))
        check(self.lib.mtl_colsum_accum(self.stream, x, rows, cols, cols, out, ws, amax), 'mtl_colsum_accum')

    def drop_mask(self, name, shape):
        """u8 keep-mask for one dropout site of this pass (None when dropout is off); fresh Philox stream per site."""
        if self.dropout_p <= 0.0:
            self.arena.pop(name, None)
            return None
        m = self.buf(name, shape, torch.uint8)
        self._site += 1
        check(self.lib.mtl_dropout_mask(self.stream, m.data_ptr(), m.numel(), float(self.dropout_p), self._seed_ptr,
                                        self._site << 40), 'mtl_dropout_mask')
        return m

    @property
    def drop_scale(self):
        return 1.0 / (1.0 - self.dropout_p)

    def ln_fwd(self, x, res, g, b, pe, keep, y, xhat, rstd, rows, T, xmask=None):
        """rows: per task (the tasks' row blocks follow each other; task t normalises with g / b + t * sP)"""
        check(self.lib.mtl_layernorm_fwd_g(self.stream, x, res, g, b, pe, keep, xmask.data_ptr() if xmask is not None else None,
                                           self.drop_scale, y, xhat, rstd, rows * self.nt, self.hp.d, T, 1e-5, rows, self.sP),
              'mtl_layernorm_fwd_g')

    def ln_bwd(self, dy, xhat, rstd, g, keep, dz, dg, db, rows, dsum=None, xmask=None, dzm=None, dz2=None):
        """LayerNorm backward; the reduction of its per-wave partials into dgamma / dbeta / dsum is DEFERRED: every instance keeps
        its partials in its own buffer and flush_ln_reduce() adds all of them with one launch (17 launches of 5 us before)."""
        d, nt = self.hp.d, self.nt
        nbytes = self.lib.mtl_layernorm_bwd_g_workspace(rows * nt, d, rows)
        part = self.buf('lnpart.%x' % xhat, (nbytes // 4,))
        check(self.lib.mtl_layernorm_bwd_g(self.stream, dy, xhat, rstd, g, keep, xmask.data_ptr() if xmask is not None else None,
                                           self.drop_scale, dz, dzm, dz2, dg, db, dsum, part.data_ptr(), rows * nt, d, 1, rows, self.sP,
                                           self.sG), 'mtl_layernorm_bwd_g')
        if nt == 1:
            self._ln_pending.append((part.data_ptr(), dg, db, dsum or 0, nbytes // (3 * d * 4), d))
        else:       # task t: its partial rows, its slice of the gradient stack
            wpg = self.lib.mtl_layernorm_bwd_g_waves(rows)
            for t in range(nt):
                go = 4 * t * self.sG
                self._ln_pending.append((part.data_ptr() + 4 * t * wpg * 3 * d, dg + go, db + go, (dsum + go) if dsum else 0, wpg, d))

    def flush_ln_reduce(self):
        pend, self._ln_pending = tuple(self._ln_pending), []
        if not pend:
            return
        dev = self._ln_tables.get(pend)
        if dev is None:
            table = (_lib.LnReduceDesc * len(pend))()
            for t, (part, dg, db, dsum, nw, d) in zip(table, pend):
                t.part, t.dgamma, t.dbeta, t.dsum, t.nw, t.d = part, dg, db, dsum or None, nw, d
            dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
            self._ln_tables[pend] = dev
        check(self.lib.mtl_ln_param_reduce_batch(self.stream, dev.data_ptr(), len(pend), max(p[5] for p in pend)),
              'mtl_ln_param_reduce_batch')

    # ---------------------------------------------------------------- attention / ffn blocks
    def mha_fwd(self, tag, P, pre, xq, Bn, Tq, xkv, Tk, klen, causal, keep, kv_ready=None):
        """Bn: samples PER TASK; the pass carries self.nt tasks whose row blocks (Bn * Tq query rows, Bn * Tk key rows each) follow
        each other in every activation buffer."""
        hp, L, nt, sP = self.hp, self.L, self.nt, self.sP
        d, r, h, dk, dv = hp.d, hp.r, hp.h, hp.dk, hp.dv
        Mq, Mk = Bn * Tq, Bn * Tk                      # rows per task
        Rq = nt * Mq                                   # rows of the pass
        hk, hv = h * dk, h * dv
        o = lambda n: P + 4 * L.off(pre + n)
        t = {}
        # The three projections have identical shapes and their parameters sit at a constant stride in the flat theta / G
        # buffers, so projections that share their input run as ONE strided-batch GEMM per low-rank stage (self-attention:
        # q,k,v; encoder-decoder attention: k,v) instead of two launches (+ a split-K reduction) each.
        groups = passplan.qkv_groups(L, pre, xq, Mq, xkv, Mk, hk, hv)
        for names, src, rows in groups:
            n, f0 = len(names), _FULL[names[0]]
            wd = hv if names == 'v' else hk                  # groups of several projections exist only when hk == hv
            if kv_ready is not None and names == 'kv':          # projected for all layers at once by cross_kv_fwd
                a_all, b_all = kv_ready
                self.arena[tag + names + 'a'], self.arena[tag + names] = a_all, b_all
                for i, nm in enumerate(names):
                    self.arena[tag + nm + 'a'], self.arena[tag + nm] = a_all[i], b_all[i]
                    t[nm + 'a'], t[nm] = a_all[i], b_all[i]
                continue
            R = nt * rows
            a_all = self.buf(tag + names + 'a', (n, R, r))
            b_all = self.buf(tag + names, (n, R, wd))
            sa, sb, sbias = (passplan.pstride(L, pre, names, sfx) for sfx in ('_linear_a.weight', '_linear_b.weight', '_linear_b.bias'))
            self.gemm(0, 1, rows, r, d, src, d, o(f0 + '_linear_a.weight'), d, a_all.data_ptr(), r, batch=n, sB=(sa, 0),
                      sC=(R * r, 0), task=(rows * d, sP, rows * r, 0, 0))
            self.gemm(0, 1, rows, wd, r, a_all.data_ptr(), r, o(f0 + '_linear_b.weight'), r, b_all.data_ptr(), wd,
                      bias=o(f0 + '_linear_b.bias'), batch=n, sA=(R * r, 0), sB=(sb, 0), sC=(R * wd, 0), sbias=sbias,
                      task=(rows * r, sP, rows * wd, sP, 0))
            for i, nm in enumerate(names):
                self.arena[tag + nm + 'a'], self.arena[tag + nm] = a_all[i], b_all[i]
                t[nm + 'a'], t[nm] = a_all[i], b_all[i]
        self.arena[tag + 'groups'] = groups
        ldS = (Tk + 3) // 4 * 4
        Bn = nt * Bn                                   # the attention core sees one batch of all tasks' samples (no parameters)
        mP = self.drop_mask(tag + 'mP', (Bn, h, Tq, ldS))                       # dropout on the probabilities (:328)
        O = self.buf(tag + 'O', (Rq, hv))
        if self.fused_attn:
            lse = self.buf(tag + 'lse', (Bn, h, Tq))
            check(self.lib.mtl_attn_fwd(self.stream, t['q'].data_ptr(), t['k'].data_ptr(), t['v'].data_ptr(), hk, hk, hv, klen, causal,
                                        1.0 / float(hp.temperature), Bn, h, Tq, Tk, dk, dv, mP.data_ptr() if mP is not None else None,
                                        ldS, self.drop_scale, O.data_ptr(), hv, lse.data_ptr()), 'mtl_attn_fwd')
        else:
            if nt > 1:
                raise NotImplementedError('task-batched passes need the fused attention kernel (head sizes of mtl_attn_supported)')
            S = self.buf(tag + 'P', (Bn, h, Tq, ldS))
            self.gemm(0, 1, Tq, Tk, dk, t['q'].data_ptr(), hk, t['k'].data_ptr(), hk, S.data_ptr(), ldS, batch=Bn * h, H=h,
                      sA=(Tq * hk, dk), sB=(Tk * hk, dk), sC=(h * Tq * ldS, Tq * ldS))
            Pd = self.buf(tag + 'Pd', (Bn, h, Tq, ldS)) if mP is not None else S
            check(self.lib.mtl_softmax_mask_fwd(self.stream, S.data_ptr(), klen, causal, 1.0 / float(hp.temperature), Bn, h, Tq,
                                                Tk, ldS, mP.data_ptr() if mP is not None else None, self.drop_scale,
                                                Pd.data_ptr() if mP is not None else None), 'mtl_softmax_mask_fwd')
            self.gemm(0, 0, Tq, dv, Tk, Pd.data_ptr(), ldS, t['v'].data_ptr(), hv, O.data_ptr(), hv, batch=Bn * h, H=h,
                      sA=(h * Tq * ldS, Tq * ldS), sB=(Tk * hv, dv), sC=(Tq * hv, dv))
        self.arena[tag + 'attn'] = (klen, causal)
        oa = self.buf(tag + 'oa', (Rq, r))
        ob = self.buf(tag + 'ob', (Rq, d))
        self.linear_fwd(O.data_ptr(), Mq, hv, o('output_linear_a.weight'), None, oa.data_ptr(), r)
        self.linear_fwd(oa.data_ptr(), Mq, r, o('output_linear_b.weight'), o('output_linear_b.bias'), ob.data_ptr(), d)
        y = self.buf(tag + 'y', (Rq, d))
        xhat = self.buf(tag + 'xhat', (Rq, d))
        rstd = self.buf(tag + 'rstd', (Rq,))
        mo = self.drop_mask(tag + 'mo', (Rq, d))                                # dropout before the residual add (:303)
        self.ln_fwd(ob.data_ptr(), xq, o('layer_norm.weight'), o('layer_norm.bias'), None, keep, y.data_ptr(),
                    xhat.data_ptr(), rstd.data_ptr(), Mq, Tq, xmask=mo)
        return y

    def mha_bwd(self, tag, P, G, pre, dy, xq, Bn, Tq, xkv, Tk, keep, dxq, dxkv, dxkv_accum, dkv_hoisted=None):
        """dy: grad of the block output.  Writes dxq (overwrite) and dxkv (accumulate when dxkv is dxq or flagged).
        dkv_hoisted: (2, rows, h d_k) slice that receives dK / dV when the K / V projections' backward runs once for all decoder
        layers afterwards (cross_kv_bwd); dxkv is not touched then."""
        hp, L, A, nt, sP, sG = self.hp, self.L, self.arena, self.nt, self.sP, self.sG
        d, r, h, dk, dv = hp.d, hp.r, hp.h, hp.dk, hp.dv
        Mq, Mk = Bn * Tq, Bn * Tk                      # rows per task
        Rq = nt * Mq
        hk, hv = h * dk, h * dv
        o = lambda n: P + 4 * L.off(pre + n)
        g = lambda n: G + 4 * L.off(pre + n)
        ldS = (Tk + 3) // 4 * 4
        O, oa = A[tag + 'O'], A[tag + 'oa']
        kd = _LAYER_BUF.sub(r'\1*.\3', tag)              # 'd3.sa.' -> 'd*.sa.': the kind prefix of this block's weight gradients
        # LayerNorm(o + residual) * keep
        dzb = self.buf(tag + '_dz', (Rq, d))       # kept intact for the deferred dW GEMM; dxq = dz + projections
        mo, mP = A.get(tag + 'mo'), A.get(tag + 'mP')
        dzm = self.buf(tag + '_dzm', (Rq, d)) if mo is not None else None
        self.ln_bwd(dy, A[tag + 'xhat'].data_ptr(), A[tag + 'rstd'].data_ptr(), o('layer_norm.weight'), keep, dzb.data_ptr(),
                    g('layer_norm.weight'), g('layer_norm.bias'), Mq, dsum=g('output_linear_b.bias'), xmask=mo,
                    dzm=dzm.data_ptr() if dzm is not None else None, dz2=dxq)        # dxq = dz: the residual path
        dz = dzm.data_ptr() if dzm is not None else dzb.data_ptr()          # gradient of the (dropped) sub-layer branch
        doa = self.buf(tag + '_doa', (Rq, r))
        dO = self.buf(tag + '_dO', (Rq, hv))
        self.linear_bwd(oa.data_ptr(), dz, Mq, r, d, o('output_linear_b.weight'), g('output_linear_b.weight'),
                        None, doa.data_ptr(), False, kind=kd + 'ob')
        self.linear_bwd(O.data_ptr(), doa.data_ptr(), Mq, hv, r, o('output_linear_a.weight'), g('output_linear_a.weight'),
                        None, dO.data_ptr(), False, kind=kd + 'oa')
        q, k, v = A[tag + 'q'], A[tag + 'k'], A[tag + 'v']
        groups = A[tag + 'groups']
        dfull = {}                                       # gradients of the projected q / k / v, grouped like the forward
        for names, _src, rows in groups:
            d_all = (dkv_hoisted if (dkv_hoisted is not None and names == 'kv') else
                     self.buf(tag + '_d' + names, (len(names), nt * rows, hv if names == 'v' else hk)))
            for i, nm in enumerate(names):
                dfull[nm] = d_all[i]
            dfull[names] = d_all
        dq, dkk, dvv = dfull['q'], dfull['k'], dfull['v']
        if self.fused_attn:
            klen, causal = A[tag + 'attn']
            delta = self.buf('_delta.side' if self.on_side else '_delta', (nt * Bn * h * Tq,))
            check(self.lib.mtl_attn_bwd(self.stream, q.data_ptr(), k.data_ptr(), v.data_ptr(), hk, hk, hv, klen, causal,
                                        1.0 / float(hp.temperature), nt * Bn, h, Tq, Tk, dk, dv, mP.data_ptr() if mP is not None else None,
                                        ldS, self.drop_scale, O.data_ptr(), dO.data_ptr(), hv, A[tag + 'lse'].data_ptr(),
                                        delta.data_ptr(), dq.data_ptr(), dkk.data_ptr(), dvv.data_ptr(), hk, hk, hv), 'mtl_attn_bwd')
        else:
            Pm = A[tag + 'P']
            # (layer 0's decoder self-attention runs on the side stream under the encoder's backward: with Td = T4 the two would share one)
            dP = self.buf('_dP.side' if self.on_side else '_dP', (Bn, h, Tq, ldS))
            sS = (h * Tq * ldS, Tq * ldS)
            # dV = P^T dO ; dP = dO V^T ; dS = softmax'(P, dP)/temp ; dQ = dS K ; dK = dS^T Q
            Pv = A[tag + 'Pd'] if mP is not None else Pm                      # the probabilities that actually multiplied V
            self.gemm(1, 0, Tk, dv, Tq, Pv.data_ptr(), ldS, dO.data_ptr(), hv, dvv.data_ptr(), hv, batch=Bn * h, H=h,
                      sA=sS, sB=(Tq * hv, dv), sC=(Tk * hv, dv))
            self.gemm(0, 1, Tq, Tk, dv, dO.data_ptr(), hv, v.data_ptr(), hv, dP.data_ptr(), ldS, batch=Bn * h, H=h,
                      sA=(Tq * hv, dv), sB=(Tk * hv, dv), sC=sS)
            check(self.lib.mtl_softmax_bwd(self.stream, Pm.data_ptr(), dP.data_ptr(), 1.0 / float(hp.temperature),
                                           Bn * h * Tq, Tk, ldS, mP.data_ptr() if mP is not None else None, self.drop_scale),
                  'mtl_softmax_bwd')
            self.gemm(0, 0, Tq, dk, Tk, dP.data_ptr(), ldS, k.data_ptr(), hk, dq.data_ptr(), hk, batch=Bn * h, H=h,
                      sA=sS, sB=(Tk * hk, dk), sC=(Tq * hk, dk))
            self.gemm(1, 0, Tk, dk, Tq, dP.data_ptr(), ldS, q.data_ptr(), hk, dkk.data_ptr(), hk, batch=Bn * h, H=h,
                      sA=sS, sB=(Tq * hk, dk), sC=(Tk * hk, dk))
        kv_written = False
        for names, src, rows in groups:
            if dkv_hoisted is not None and names == 'kv':
                continue
            n, f0 = len(names), _FULL[names[0]]
            wd = hv if names == 'v' else hk
            a_all, d_all = A[tag + names + 'a'], dfull[names]
            R = nt * rows
            da_all = self.buf(tag + '_da' + names, (n, R, r))
            sa, sb, sbias = (passplan.pstride(L, pre, names, sfx) for sfx in ('_linear_a.weight', '_linear_b.weight', '_linear_b.bias'))
            a_ptr, d_ptr, da_ptr = a_all.data_ptr(), d_all.data_ptr(), da_all.data_ptr()

            # dW_b[i] += d[i]^T a[i]  and  db_b[i] += colsum(d[i])
            self.wgrad_job(kd + names + '.b', wd, r, rows, d_ptr, wd, a_ptr, r, g(f0 + '_linear_b.weight'), r, n=n, sA=R * wd,
                           sB=R * r, sC=sb, rowsum=g(f0 + '_linear_b.bias'), srow=sbias)
            # da[i] = d[i] . W_b[i]
            self.gemm(0, 0, rows, r, wd, d_ptr, wd, o(f0 + '_linear_b.weight'), r, da_ptr, r, batch=n, sA=(R * wd, 0),
                      sB=(sb, 0), sC=(R * r, 0), task=(rows * wd, sP, rows * r, 0, 0))

            # dW_a[i] += da[i]^T x
            self.wgrad_job(kd + names + '.a', r, d, rows, da_ptr, r, src, d, g(f0 + '_linear_a.weight'), d, n=n, sA=R * r, sB=0, sC=sa)
            # dx (+)= sum_i da[i] . W_a[i]: the items of a group accumulate into ONE tensor -> one K-batched launch
            if names[0] == 'q':
                dst, accum = dxq, True
            else:
                dst, accum = dxkv, (dxkv_accum or (dxkv == dxq) or kv_written)
                kv_written = True
            self.gemm(0, 0, rows, d, r, da_ptr, r, o(f0 + '_linear_a.weight'), d, dst, d, flags=ACCUM if accum else 0,
                      kbatch=n, sAk=R * r, sBk=sa, task=(rows * r, sP, rows * d, 0, 0))
        self.flush_side()

    # ---- encoder-decoder attention: K / V projections of all decoder layers in one go
    def cross_kv_fwd(self, P, mem, Mk):
        """k_l, v_l = W_b (W_a mem) (+ b) for every decoder layer l: two launches with batch = 2 n_dec (layers outer, k / v inner)."""
        plan = passplan.cross_kv_plan(self.L, self.hp.n_dec, self.hp.dk, self.hp.dv)
        self.arena['xkv.plan'] = plan
        if plan is None:
            return None
        hp, L, nt, sP = self.hp, self.L, self.nt, self.sP
        Ls, Ps = plan
        d, r, wd, NL = hp.d, hp.r, hp.h * hp.dk, hp.n_dec
        Rk = nt * Mk                                   # Mk: key rows per task
        o0 = lambda n: P + 4 * L.off('decoder.layers.0.encoder_attn.' + n)
        a_all = self.buf('xkv.a', (NL, 2, Rk, r))
        b_all = self.buf('xkv.b', (NL, 2, Rk, wd))
        self.gemm(0, 1, Mk, r, d, mem, d, o0('key_linear_a.weight'), d, a_all.data_ptr(), r, batch=2 * NL, H=2, sB=(Ls, Ps),
                  sC=(2 * Rk * r, Rk * r), task=(Mk * d, sP, Mk * r, 0, 0))
        self.gemm(0, 1, Mk, wd, r, a_all.data_ptr(), r, o0('key_linear_b.weight'), r, b_all.data_ptr(), wd, bias=o0('key_linear_b.bias'),
                  batch=2 * NL, H=2, sA=(2 * Rk * r, Rk * r), sB=(Ls, Ps), sC=(2 * Rk * wd, Rk * wd), sbias=Ls, sbias_h=Ps,
                  task=(Mk * r, sP, Mk * wd, sP, 0))
        return a_all, b_all

    def cross_kv_bwd(self, P, G, mem, Mk, dmem):
        """backward of cross_kv_fwd from the dK / dV of all layers ('xkv.d'): the two weight-gradient products (batch 2 n_dec, bias
        gradients folded in) on the side stream, da, and dmem = sum over layers and k / v of da . W_a (two K-batched launches)."""
        hp, L, A, nt, sP, sG = self.hp, self.L, self.arena, self.nt, self.sP, self.sG
        Ls, Ps = A['xkv.plan']
        d, r, wd, NL = hp.d, hp.r, hp.h * hp.dk, hp.n_dec
        Rk = nt * Mk
        o0 = lambda n: P + 4 * L.off('decoder.layers.0.encoder_attn.' + n)
        g0 = lambda n: G + 4 * L.off('decoder.layers.0.encoder_attn.' + n)
        a_ptr, d_ptr = A['xkv.a'].data_ptr(), A['xkv.d'].data_ptr()
        da = self.buf('xkv.da', (NL, 2, Rk, r))
        da_ptr = da.data_ptr()
        self.defer(lambda: self.gemm(1, 0, wd, r, Mk, d_ptr, wd, a_ptr, r, g0('key_linear_b.weight'), r, flags=ACCUM, batch=2 * NL, H=2,
                                     sA=(2 * Rk * wd, Rk * wd), sB=(2 * Rk * r, Rk * r), sC=(Ls, Ps), rowsum=g0('key_linear_b.bias'),
                                     srow=Ls, srow_h=Ps, task=(Mk * wd, Mk * r, sG, 0, sG)))
        self.gemm(0, 0, Mk, r, wd, d_ptr, wd, o0('key_linear_b.weight'), r, da_ptr, r, batch=2 * NL, H=2, sA=(2 * Rk * wd, Rk * wd),
                  sB=(Ls, Ps), sC=(2 * Rk * r, Rk * r), task=(Mk * wd, sP, Mk * r, 0, 0))
        self.defer(lambda: self.gemm(1, 0, r, d, Mk, da_ptr, r, mem, d, g0('key_linear_a.weight'), d, flags=ACCUM, batch=2 * NL, H=2,
                                     sA=(2 * Rk * r, Rk * r), sC=(Ls, Ps), task=(Mk * r, Mk * d, sG, 0, 0)))
        for pj, name in enumerate(('key', 'value')):      # dmem (=|+=) sum_l da[l, pj] . W_a[l, pj]
            self.gemm(0, 0, Mk, d, r, da_ptr + 4 * pj * Rk * r, r, o0(name + '_linear_a.weight'), d, dmem, d, flags=ACCUM if pj else 0,
                      kbatch=NL, sAk=2 * Rk * r, sBk=Ls, task=(Mk * r, sP, Mk * d, 0, 0))
        self.flush_side()

    def _ffn_lr_fwd(self, tag, o, x, rows, h2):
        """the factorized block's four Linears (modules/common_layers.py:134-158): x -> a1 (r) -> h1 (inner, bias + ReLU) -> c2 (r) ->
        h2 (d, bias); the middle two as one launch with ffn_mid_fused.  tag + 'h1' stays the post-ReLU inner activation."""
        hp, R = self.hp, self.nt * rows
        r, inner = hp.r, hp.inner
        a1 = self.buf(tag + 'a1', (R, r))
        c2 = self.buf(tag + 'c2', (R, r))
        self.linear_fwd(x, rows, hp.d, o('linear_1_a.weight'), None, a1.data_ptr(), r)
        if self.ffn_mid_fused and self.lib.mtl_ffn_lr_mid_supported(r, inner):
            if self.forward_only:
                self.arena.pop(tag + 'h1', None)
                h1p = None
            else:
                h1p = self.buf(tag + 'h1', (R, inner)).data_ptr()
            check(self.lib.mtl_ffn_lr_mid_fwd(self.stream, a1.data_ptr(), r, o('linear_1_b.weight'), o('linear_1_b.bias'),
                                              o('linear_2_a.weight'), h1p, c2.data_ptr(), r, rows, r, inner, self.nt, rows * r, self.sP,
                                              rows * inner, rows * r), 'mtl_ffn_lr_mid_fwd')
        else:
            h1 = self.buf(tag + 'h1', (R, inner))
            self.linear_fwd(a1.data_ptr(), rows, r, o('linear_1_b.weight'), o('linear_1_b.bias'), h1.data_ptr(), inner, relu=True)
            self.linear_fwd(h1.data_ptr(), rows, inner, o('linear_2_a.weight'), None, c2.data_ptr(), r)
        self.linear_fwd(c2.data_ptr(), rows, r, o('linear_2_b.weight'), o('linear_2_b.bias'), h2.data_ptr(), hp.d)

    def ffn_fwd(self, tag, P, pre, x, rows, T, keep):
        hp, L = self.hp, self.L
        o = lambda n: P + 4 * L.off(pre + n)
        R = self.nt * rows                             # rows: per task
        if self.factorized:
            h2 = self.buf(tag + 'h2', (R, hp.d))
            self._ffn_lr_fwd(tag, o, x, rows, h2)
        else:
            h1 = self.buf(tag + 'h1', (R, hp.inner))
            h2 = self.buf(tag + 'h2', (R, hp.d))
            self.linear_fwd(x, rows, hp.d, o('linear_1.weight'), o('linear_1.bias'), h1.data_ptr(), hp.inner, relu=True)
            self.linear_fwd(h1.data_ptr(), rows, hp.inner, o('linear_2.weight'), o('linear_2.bias'), h2.data_ptr(), hp.d)
        y = self.buf(tag + 'y', (R, hp.d))
        xhat = self.buf(tag + 'xhat', (R, hp.d))
        rstd = self.buf(tag + 'rstd', (R,))
        mf = self.drop_mask(tag + 'mf', (R, hp.d))                              # dropout before the residual add (:130)
        self.ln_fwd(h2.data_ptr(), x, o('layer_norm.weight'), o('layer_norm.bias'), None, keep, y.data_ptr(), xhat.data_ptr(),
                    rstd.data_ptr(), rows, T, xmask=mf)
        return y

    def ffn_bwd(self, tag, P, G, pre, dy, x, rows, keep, dx):
        hp, L, A = self.hp, self.L, self.arena
        o = lambda n: P + 4 * L.off(pre + n)
        g = lambda n: G + 4 * L.off(pre + n)
        R = self.nt * rows
        dzb = self.buf(tag + '_dz', (R, hp.d))
        mf = A.get(tag + 'mf')
        dzm = self.buf(tag + '_dzm', (R, hp.d)) if mf is not None else None
        self.ln_bwd(dy, A[tag + 'xhat'].data_ptr(), A[tag + 'rstd'].data_ptr(), o('layer_norm.weight'), keep, dzb.data_ptr(),
                    g('layer_norm.weight'), g('layer_norm.bias'), rows, dsum=g('linear_2_b.bias' if self.factorized else 'linear_2.bias'),
                    xmask=mf, dzm=dzm.data_ptr() if dzm is not None else None, dz2=dx)         # dx = dz: the residual path
        dbr = dzm.data_ptr() if dzm is not None else dzb.data_ptr()
        h1 = A[tag + 'h1']
        dh1 = self.buf(tag + '_dh1', (R, hp.inner))
        kd = _LAYER_BUF.sub(r'\1*.\3', tag)
        if self.factorized:
            # four Linears, last to first; linear_2_b.bias came from the LayerNorm backward's dsum, linear_1_b.bias rides on its
            # weight-gradient product; every weight gradient is logged under its kind, so the layers of a stack merge
            r = hp.r
            dc2, da1 = self.buf(tag + '_dc2', (R, r)), self.buf(tag + '_da1', (R, r))
            self.linear_bwd(A[tag + 'c2'].data_ptr(), dbr, rows, r, hp.d, o('linear_2_b.weight'), g('linear_2_b.weight'), None,
                            dc2.data_ptr(), False, kind=kd + 'w2b')
            self.linear_bwd(h1.data_ptr(), dc2.data_ptr(), rows, hp.inner, r, o('linear_2_a.weight'), g('linear_2_a.weight'), None,
                            dh1.data_ptr(), False, gate=h1.data_ptr(), kind=kd + 'w2a')
            self.linear_bwd(A[tag + 'a1'].data_ptr(), dh1.data_ptr(), rows, r, hp.inner, o('linear_1_b.weight'), g('linear_1_b.weight'),
                            g('linear_1_b.bias'), da1.data_ptr(), False, kind=kd + 'w1b')
            self.linear_bwd(x, da1.data_ptr(), rows, hp.d, r, o('linear_1_a.weight'), g('linear_1_a.weight'), None, dx, True,
                            kind=kd + 'w1a')
            self.flush_side()
            return
        self.linear_bwd(h1.data_ptr(), dbr, rows, hp.inner, hp.d, o('linear_2.weight'), g('linear_2.weight'),
                        None, dh1.data_ptr(), False, gate=h1.data_ptr(), kind=kd + 'w2')
        self.linear_bwd(x, dh1.data_ptr(), rows, hp.d, hp.inner, o('linear_1.weight'), g('linear_1.weight'),
                        g('linear_1.bias'), dx, True, kind=kd + 'w1')
        self.flush_side()

    # ---------------------------------------------------------------- the pass
    def prepare(self, lengths, target, B, T, slot=0, norm_count=None, width=None, frames=None, percentages=None, target_sizes=None):
        """Host-side integer prep of one batch (modules/decoder.py:55-69 target shifting; every mask is derived inside the
        kernels from these few integers) + asynchronous H2D into STATIC per-slot buffers.  Kept separate from the kernels so
        a captured hipGraph of the pass can be replayed for any batch of the same shape."""
        return self.prepare_tasks([(lengths, target)], B, T, slot, norm_count, width, frames=None if frames is None else [frames],
                                  percentages=None if percentages is None else [percentages],
                                  target_sizes=None if target_sizes is None else [target_sizes])

    def prepare_tasks(self, batches, B, T, slot=0, norm_count=None, width=None, frames=None, percentages=None, target_sizes=None):
        """prepare() for the batches [(lengths, target)] of several tasks that one task-batched pass carries (all B samples x T
        frames; the decoder width is the largest of the tasks' -- positions beyond a task's own width are padding like any other:
        masked as keys, zeroed as rows, ignored by the loss).  Everything per-sample is concatenated in task order; the loss
        normaliser 1 / n_nonpad and the embedding occurrence chains are per task.
        frames: the tasks' OWN frame counts when their batches were padded to different widths (data.py:77 pads a batch to its
        longest utterance) and stacked at the widest, T.  A task's encoder then has (frames // 2) // 2 positions as in its own
        pass: the positions beyond are padding (the reference compares RAW lengths with the positions it has, SURVEY Q2, so a wider
        pad would otherwise turn into live positions), and forward_device clears the convolution outputs beyond each task's frames.
        percentages / target_sizes: per task, what the CTC loss stage (forward_device(loss_type='ctc')) takes its lengths from
        (utils/metrics.py:129): in_len = (fp32 percentages * Td_own).int() with Td_own the task's OWN decoder width -- its longest
        target + 1, as in its own reference pass, whatever width this pass is padded to -- and tgt_len = target_sizes.  None:
        percentages = lengths / max(lengths) as data.py forms them, target_sizes = the count of non-PAD targets.  The two int32
        arrays (nt * B each) stand at the END of the meta block."""
        hp = self.hp
        bm = batch_meta(batches, B, T, hp.src_max_len, hp.tgt_max_len, norm_count, width, frames, percentages, target_sizes,
                        time_shift=self.time_shift)
        meta_np, off, Td, nt = bm['meta'], bm['off'], bm['Td'], len(batches)
        # dropout seed of this pass (torch CPU RNG): drawn once the batch has been accepted
        meta_np[off['seed']:off['seed'] + 2] = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).numpy().view(np.int32)
        n_meta, Bt = int(meta_np.shape[0]), nt * B
        # page-locked staging (a ring of STAGE_RING buffers per slot, each guarded by an event): the uploads are truly asynchronous
        # and the host never rewrites a staging buffer whose copy has not been consumed yet.  The ring is deeper than the host may
        # run ahead (pipeline depth + the iteration being resolved + 1), so the event wait never waits in the steady state.
        dev_i32 = self.buf('meta_i32.%d' % slot, (n_meta,), torch.int32)
        ids = self.buf('ids.%d' % slot, (2, Bt, Td), torch.int64)
        _trace.mark('prepare_numpy')
        # the ring holds raw pinned bytes sized for the largest batch seen so far (grown geometrically, the whole ring at once: a
        # page-locked allocation serialises against the device, so variable-length data must not bring one per new shape, and none
        # may happen a few iterations later inside somebody's timed region)
        need = 4 * n_meta + 16 + 16 * Bt * Td
        ring = self._stage.get(slot)
        if ring is None or ring[0]['raw'].numel() < need:
            cap = max(need + need // 2, 1 << 16)
            ring = [dict(raw=torch.empty(cap, dtype=torch.uint8).pin_memory(), ev=None) for _ in range(STAGE_RING)]
            self._stage[slot] = ring           # (an old ring's blocks return to torch's pinned allocator once their copies have completed)
            self._stage_turn[slot] = 0
        turn = self._stage_turn.get(slot, 0)
        self._stage_turn[slot] = (turn + 1) % STAGE_RING
        st = ring[turn]
        if st['ev'] is None:
            st['ev'] = torch.cuda.Event()
        else:
            st['ev'].synchronize()
        off_ids = (4 * n_meta + 15) // 16 * 16
        st_i32 = st['raw'][:4 * n_meta].view(torch.int32)
        st_ids = st['raw'][off_ids:off_ids + 16 * Bt * Td].view(torch.int64).view(2, Bt, Td)
        i32_np, ids_np = st_i32.numpy(), st_ids.numpy()          # views of the pinned memory
        _trace.mark('stage_wait')
        np.copyto(i32_np, meta_np)
        np.copyto(ids_np[0], bm['seq_in'])
        np.copyto(ids_np[1], bm['seq_out'])
        dev_i32.copy_(st_i32, non_blocking=True)
        ids.copy_(st_ids, non_blocking=True)
        st['ev'].record(torch.cuda.current_stream(self.device))
        _trace.mark('stage_upload')
        base = dev_i32.data_ptr()
        addr = {name: None if o is None else base + 4 * o for name, o in off.items()}     # device address of every field of the block
        return dict(addr, frames=bm['frames'], B=B, T=T, Td=Td, nt=nt, n_nonpad=bm['n_nonpads'][0], n_nonpads=bm['n_nonpads'],
                    gold_host=torch.from_numpy(bm['seq_out']), gold_hosts=bm['gold_hosts'], ids=ids,
                    ctc_in_len_host=bm['ctc_in_len_host'], ctc_tgt_len_host=bm['ctc_tgt_len_host'])

    def forward(self, theta, x, lengths, target, smoothing=0.0, slot=0, loss_type='ce', percentages=None, target_sizes=None):
        """x (B,1,F,T) fp32 on device; lengths (B) int; target (B,L) int64 PAD-padded.  Returns a dict with device
        tensors pred (B,Td,V), gold, hyp (B,Td) int64 and `loss` (1,) fp32; keeps what the backward needs.
        loss_type 'ctc': the CTC loss of prepare()'s percentages / target_sizes in place of the cross entropy (forward_device)."""
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError('expected (B,1,F,T) input')
        # stand-alone passes (validation loops, the joint trainer, the drop-in autograd call) on batches whose width changes from call
        # to call: widened to a repeating width like the trainer's lanes (own border and encoder length kept), from the second width on
        # (not while a test's forward hook reads the activations in the pass's own extent).  Exact with dropout off; with dropout on, the
        # keep-masks of a widened pass differ from the own-width pass's (the Philox element indices follow the buffer extents).
        T_own, frames = int(x.shape[3]), None
        if self.widen == 'auto' and not self._widths_vary:
            self._widths_vary = self._first_width.setdefault(slot, T_own) != T_own
        if self.widen_quantum > 1 and (self.widen == '1' or (self.widen == 'auto' and self._widths_vary and self.forward_hook is None)):
            Tq = max(min(round_width(T_own, self.widen_quantum), self.hp.src_max_len << self.time_shift), T_own)
            if Tq != T_own:
                xp = self.buf('fwd.x.%d' % slot, tuple(x.shape[:3]) + (Tq,))
                xp.zero_()
                xp[:, :, :, :T_own].copy_(x, non_blocking=True)
                x, frames = xp, T_own
        meta = self.prepare(lengths, target, x.shape[0], x.shape[3], slot, frames=frames, percentages=percentages, target_sizes=target_sizes)
        return self.forward_device(theta, x, meta, smoothing, loss_type=loss_type)

    def forward_device(self, theta, x, meta, smoothing=0.0, hyp_out=None, loss_out=None, sP=0, loss_type='ce'):
        """Kernel launches only (hipGraph-capturable): everything batch-dependent comes from `meta`'s device buffers.

        loss_type 'ctc' (utils/metrics.py:127-148): lse and hyp as for 'ce', then mtl_ctc_fwd writes one CTC loss per task into
        `loss` from the lengths prepare() left at the end of the meta block; the log-alpha lattice stays in the arena for
        backward(), which then forms d(logits) with mtl_ctc_bwd.  `smoothing` is ignored, as the reference ignores it.

        Task-batched pass (meta from prepare_tasks with nt > 1 tasks; trainer/asr/transient_trainer.py:178-237: the tasks of a
        meta-step are independent given theta0): x is (nt * B, 1, F, T) -- or (B, 1, F, T) when every task sees the SAME batch (the
        shared validation batch) -- and task t reads its parameters at theta + t * sP floats: sP = 0 for the training passes (all
        at theta0), sP = layout.total for the validation passes at the theta' stack.  Every transformer kernel runs ONCE over the
        rows of all tasks (task = outermost batch index of the products, row group of LayerNorm / embedding / loss); so do the
        convolutions and the products around the encoder's input Linear in the x3 and h2 modes: one launch over the samples of all
        tasks (convstack.py; the fp32 convolutions are issued per task).  loss is (nt,), hyp (nt * B, Td)."""
        hp, L, lib, st = self.hp, self.L, self.lib, self.stream
        nt = int(meta.get('nt', 1))
        self.trim_pool()
        assert theta.dtype == torch.float32 and theta.is_contiguous()
        assert theta.numel() == L.total * (nt if sP else 1) and (sP == 0 or sP == L.total)
        x = x.contiguous()
        if x.dtype != torch.float32 or x.device != self.device:
            raise ValueError('input must be fp32 on %s' % self.device)
        Bx, _, F, T = x.shape
        B = meta['B']
        if Bx not in (B, nt * B) or T != meta['T']:
            raise ValueError('input batch does not match the prepared batch')
        sX = B * F * T if Bx == nt * B and nt > 1 else 0          # task stride of the input (0: one batch shared by all tasks)
        if (F if self.conv_layers is None else F // 2 // 2 * self.conv_layers[-1].cout) != hp.d_in:
            raise ValueError('dim_input %d does not match %d frequency bins' % (hp.d_in, F))
        if loss_type not in LOSS_TYPES:
            raise NotImplementedError("loss_type must be 'ce' or 'ctc'")
        if loss_type == 'ctc':
            smoothing = 0.0
        self.nt, self.sP = nt, int(sP)
        try:
            return self._forward_device(theta, x, meta, smoothing, hyp_out, loss_out, nt, sX, F, T, loss_type)
        finally:
            self.nt, self.sP = 1, 0        # (the backward restores them from `saved`; an exception mid-pass must not leave nt > 1 behind)

    def _forward_device(self, theta, x, meta, smoothing, hyp_out, loss_out, nt, sX, F, T, loss_type='ce'):
        hp, L, lib, st = self.hp, self.L, self.lib, self.stream
        sP = self.sP
        B = meta['B']
        T4 = self.enc_extent(T)
        P = theta.data_ptr()
        o = lambda n: P + 4 * L.off(n)
        d, V = hp.d, hp.V
        Td, ids, n_nonpad = meta['Td'], meta['ids'], meta['n_nonpad']
        self._seed_ptr, self._site = meta['seed'], 0
        klen_enc, klen_dec, keep_enc, keep_dec = meta['klen_enc'], meta['klen_dec'], meta['keep_enc'], meta['keep_dec']
        Me, Md = B * T4, B * Td                                     # encoder / decoder rows PER TASK
        Bt = nt * B

        # ---- VGG front-end (convstack.py) ----
        # what this pass runs on is decided here, once: the backward goes by this record, not by the engine's attributes of its time
        S = dict(theta=theta, x=x, B=B, T=T, F=F, meta=meta, nt=nt, sP=sP, sX=sX, **convstack.decide(self, nt, meta.get('widths')))
        front = convstack.front_for(self, S)
        front.convs_fwd()

        # ---- encoder ----
        # decoder prologue: embedding (+ PE, dropout) and layer 0's self-attention block read the labels and theta only
        def dec_prologue():
            d0_ = self.buf('dec_in.y', (nt * Md, d))
            me = self.drop_mask('dec_in.me', (nt * Md, d))                      # dropout(emb + PE) (modules/decoder.py:96)
            check(lib.mtl_embed_pe_fwd_g(self.stream, ids.data_ptr(), o('decoder.trg_embedding.weight'), self.pe_dec.data_ptr(),
                                         d0_.data_ptr(), nt * Md, Td, d, me.data_ptr() if me is not None else None, self.drop_scale,
                                         Md, self.sP), 'embed')
            if hp.n_dec == 0:
                return d0_, None
            return d0_, self.mha_fwd('d0.sa.', P, 'decoder.layers.0.self_attn.', d0_.data_ptr(), B, Td, d0_.data_ptr(), Td, klen_dec, 1,
                                     keep_dec)
        pro_done = None
        S['dec0_on_side'] = bool(self.use_side_stream and hp.n_dec > 0)
        if S['dec0_on_side']:
            (d0, a0), pro_done = self.run_on_side(dec_prologue)      # under the input Linear and the encoder
        e0 = front.linear_fwd()
        ex = self.buf('enc_in.y', (nt * Me, d))
        self.ln_fwd(e0.data_ptr(), None, o('encoder.layer_norm_input.weight'), o('encoder.layer_norm_input.bias'),
                    self.pe_enc.data_ptr(), None, ex.data_ptr(), self.buf('enc_in.xhat', (nt * Me, d)).data_ptr(),
                    self.buf('enc_in.rstd', (nt * Me,)).data_ptr(), Me, T4)
        cur = ex
        enc_inputs = []
        for i in range(hp.n_enc):
            pre = 'encoder.layers.%d.' % i
            enc_inputs.append(cur)
            a = self.mha_fwd('e%d.sa.' % i, P, pre + 'self_attn.', cur.data_ptr(), B, T4, cur.data_ptr(), T4, klen_enc, 0, keep_enc)
            cur = self.ffn_fwd('e%d.ff.' % i, P, pre + 'pos_ffn.', a.data_ptr(), Me, T4, keep_enc)
        mem = cur

        # ---- decoder ----
        if pro_done is not None:
            self.wait_side_event(pro_done)
        else:
            d0, a0 = dec_prologue()
        cur = d0
        xkv = self.cross_kv_fwd(P, mem.data_ptr(), Me)
        for i in range(hp.n_dec):
            pre = 'decoder.layers.%d.' % i
            a = a0 if i == 0 else self.mha_fwd('d%d.sa.' % i, P, pre + 'self_attn.', cur.data_ptr(), B, Td, cur.data_ptr(), Td,
                                               klen_dec, 1, keep_dec)
            c = self.mha_fwd('d%d.ca.' % i, P, pre + 'encoder_attn.', a.data_ptr(), B, Td, mem.data_ptr(), T4, klen_enc, 0, keep_dec,
                             kv_ready=(xkv[0][i], xkv[1][i]) if xkv is not None else None)
            cur = self.ffn_fwd('d%d.ff.' % i, P, pre + 'pos_ffn.', c.data_ptr(), Md, Td, keep_dec)
        pred = self.buf('pred', (Bt, Td, V))
        self.gemm(0, 1, Md, V, d, cur.data_ptr(), d, o('decoder.output_linear.weight'), d, pred.data_ptr(), V,
                  task=(Md * d, self.sP, Md * V, 0, 0))

        # ---- loss + arg-max ----
        lse = self.buf('lse', (nt * Md,))
        # hyp_out / loss_out: caller-owned destinations (the trainer's per-pass read-back slots: no device copies afterwards)
        hyp = self.buf('hyp', (Bt, Td), torch.int64) if hyp_out is None else hyp_out
        rowloss = self.buf('rowloss', (nt * Md,))
        loss = self.buf('loss', (nt,)) if loss_out is None else loss_out
        gold_ptr = ids.data_ptr() + 8 * nt * Md
        if nt == 1:
            check(lib.mtl_ce_argmax_fwd(st, pred.data_ptr(), gold_ptr, Md, V, V, PAD_ID, float(smoothing), 0, meta['inv_count'],
                                        lse.data_ptr(), hyp.data_ptr(), rowloss.data_ptr(), loss.data_ptr()), 'ce_fwd')
        else:
            check(lib.mtl_ce_argmax_fwd_g(st, pred.data_ptr(), gold_ptr, nt * Md, V, V, PAD_ID, float(smoothing), meta['inv_count'],
                                          lse.data_ptr(), hyp.data_ptr(), rowloss.data_ptr(), loss.data_ptr(), Md), 'ce_fwd')
        ctc = None
        if loss_type == 'ctc':
            # one workgroup per utterance walks the (Td, 2 Lmax + 1) lattice of its labels (the first tgt_len entries of its gold
            # row); the lattice and the rows' log-sum-exp pairs are kept for the backward, so they are a buffer of the pass and not the
            # shared scratch (mtl_ctc_fwd forms its own row statistics: `lse` above is one fp32 per row, too coarse for x - lse near 0)
            Lmax = max(Td - 1, 1)
            ws_bytes = lib.mtl_ctc_workspace(Bt, Td, Lmax)
            if ws_bytes < 0:
                raise ValueError('ctc: %d decoder positions are beyond the kernels\' limit' % Td)
            ctc = dict(Lmax=Lmax, ws_bytes=ws_bytes, ws=self.buf('ctc.lattice', (ws_bytes // 4,)), nll=self.buf('ctc.nll', (Bt,)))
            check(lib.mtl_ctc_fwd(st, pred.data_ptr(), gold_ptr, meta['ctc_in_len'], meta['ctc_tgt_len'], Bt, Td, V, V, Td,
                                  Lmax, PAD_ID, B, ctc['ws'].data_ptr(), ws_bytes, ctc['nll'].data_ptr(), loss.data_ptr()), 'ctc_fwd')
        self.saved = dict(S, Td=Td, n_nonpad=n_nonpad, smoothing=float(smoothing), klen_enc=klen_enc, klen_dec=klen_dec, keep_enc=keep_enc,
                          keep_dec=keep_dec, dec_last=cur, enc_inputs=enc_inputs, loss_type=loss_type, ctc=ctc,
                          no_backward=bool(self.factorized and self.forward_only))
        if self.forward_hook is not None:
            self.forward_hook(self)
        # T4 / frames: the extent of the arena's encoder-side activations (a widened stand-alone pass, PassEngine.forward, carries
        # T // 4 >= own frames // 4 positions per utterance: readers of eng.arena index with T4, the batch's own extent is frames)
        return dict(pred=pred, gold=ids[1], hyp=hyp, loss=loss, gold_host=meta['gold_host'], n_nonpad=n_nonpad, T4=T4,
                    frames=meta.get('frames'))

    # ---------------------------------------------------------------- test-time decoding: decode.py, bound as methods
    BEAM_ROWS, BEAM_POLL = decode.BEAM_ROWS, decode.BEAM_POLL
    decode_session = decode.decode_session
    greedy_decode = decode.greedy_decode
    beam_decode = decode.beam_decode
    beam_decode_batch = decode.beam_decode_batch
    beam_chunk = decode.beam_chunk

    def encoder_output(self):
        """(B, T', d) view of the LAST forward's encoder memory (what the decoder attends to; `backward` calls it mem_ptr).  T' is the
        pass's own extent (a widened stand-alone pass carries more positions than the batch); rows at and beyond an utterance's
        length are zero.  Valid until the next forward of this engine."""
        S = self.saved
        if S is None:
            raise RuntimeError('encoder_output() without a preceding forward()')
        if S['nt'] != 1:
            raise ValueError('encoder_output() is defined for single-task passes')
        hp = self.hp
        mem = self.arena['e%d.ff.y' % (hp.n_enc - 1)] if hp.n_enc else self.arena['enc_in.y']
        return mem.view(S['B'], self.enc_extent(S['T']), hp.d)

    def backward(self, grad, scale=1.0, dpred=None, sG=0, dmem_hook=None):
        """Accumulate `scale` * dLoss/dtheta of the LAST forward into the flat buffer `grad` (+=).
        dpred: optional externally supplied gradient w.r.t. pred (B,Td,V) instead of the fused CE backward.
        Task-batched pass: task t accumulates into grad + t * sG floats (sG = layout.total: a stack of per-task gradients).
        dmem_hook: called with the (B * T', d) gradient of the encoder output once the decoder has completed it and before the
        encoder's backward reads it, on the pass's main stream: a further head on encoder_output() adds its gradient there
        (single-task passes only)."""
        S = self.saved
        if S is None:
            raise RuntimeError('backward() without a preceding forward()')
        if S.get('no_backward'):
            raise RuntimeError('backward() after a forward_only pass: its activations were not kept')
        hp, L, lib, st, A = self.hp, self.L, self.lib, self.stream, self.arena
        nt = S['nt']
        if dmem_hook is not None and nt > 1:
            raise ValueError('dmem_hook: a gradient enters at the encoder output of single-task passes only')
        self.nt, self.sP, self.sG = nt, S['sP'], int(sG) if nt > 1 else 0
        if nt > 1 and (sG != L.total or grad.numel() != nt * L.total or dpred is not None):
            raise ValueError('a task-batched backward accumulates into a (tasks, layout.total) gradient stack')
        assert grad.numel() == L.total * nt and grad.is_contiguous()
        sP, sG = self.sP, self.sG
        theta = S['theta']
        P, G = theta.data_ptr(), grad.data_ptr()
        o = lambda n: P + 4 * L.off(n)
        g = lambda n: G + 4 * L.off(n)
        B, T, Td = S['B'], S['T'], S['Td']
        T4 = self.enc_extent(T)
        Me, Md, d, V = B * T4, B * Td, hp.d, hp.V                   # rows PER TASK
        keep_enc, keep_dec = S['keep_enc'], S['keep_dec']

        if dpred is None:
            ldd = (V + 3) // 4 * 4        # padded leading dimension -> 16-byte operand loads in the two GEMMs below
            dlog = self.buf('_dpred', (nt * Md, ldd))
            gold_ptr = S['meta']['ids'].data_ptr() + 8 * nt * Md
            if S.get('loss_type', 'ce') == 'ctc':
                C = S['ctc']
                check(lib.mtl_ctc_bwd(st, A['pred'].data_ptr(), gold_ptr, S['meta']['ctc_in_len'],
                                      S['meta']['ctc_tgt_len'], nt * B, Td, V, V, Td, C['Lmax'], PAD_ID, B, C['ws'].data_ptr(),
                                      C['ws_bytes'], C['nll'].data_ptr(), float(scale), None, dlog.data_ptr(), ldd), 'ctc_bwd')
            else:
                check(lib.mtl_ce_bwd_g(st, A['pred'].data_ptr(), A['lse'].data_ptr(), gold_ptr, nt * Md, V, V, PAD_ID, S['smoothing'],
                                       float(scale), S['meta']['inv_count'], dlog.data_ptr(), ldd, Md), 'ce_bwd')
            dlog_ptr = dlog.data_ptr()
        else:
            ldd = V
            dlog = dpred.contiguous()
            if scale != 1.0:
                dlog = dlog * scale
            dlog_ptr = dlog.data_ptr()
        dA = self.buf('_dxA', (nt * Md, d))
        dB = self.buf('_dxB', (nt * Md, d))
        dmem = self.buf('_dmem', (nt * Me, d))
        last = S['dec_last']
        # vocab projection (no bias)
        self.defer(lambda: self.gemm(1, 0, V, d, Md, dlog_ptr, ldd, last.data_ptr(), d, g('decoder.output_linear.weight'), d,
                                     flags=ACCUM, task=(Md * ldd, Md * d, sG, 0, 0)))    # (lda = ldd != V: stays a single call)
        self.gemm(0, 0, Md, d, V, dlog_ptr, ldd, o('decoder.output_linear.weight'), d, dA.data_ptr(), d,
                  task=(Md * ldd, sP, Md * d, 0, 0))
        self.flush_side()
        dcur, dnext = dA, dB
        hoisted = A.get('xkv.plan') is not None
        mem_ptr = A['e%d.ff.y' % (hp.n_enc - 1)].data_ptr() if hp.n_enc else A['enc_in.y'].data_ptr()
        dkv_all = self.buf('xkv.d', (hp.n_dec, 2, nt * Me, hp.h * hp.dk)) if hoisted else None
        def embed_bwd(dx):
            me = A.get('dec_in.me')
            check(lib.mtl_embed_bwd_g(self.stream, S['meta']['ids'].data_ptr(), S['meta']['embed_first'], S['meta']['embed_next'],
                                      dx.data_ptr(), g('decoder.trg_embedding.weight'), nt * Md, d, PAD_ID,
                                      me.data_ptr() if me is not None else None, self.drop_scale, Md, sG), 'embed_bwd')
        embed_done = False
        for i in reversed(range(hp.n_dec)):
            pre = 'decoder.layers.%d.' % i
            x_in = A['dec_in.y'] if i == 0 else A['d%d.ff.y' % (i - 1)]
            sa_y, ca_y = A['d%d.sa.y' % i], A['d%d.ca.y' % i]
            self.ffn_bwd('d%d.ff.' % i, P, G, pre + 'pos_ffn.', dcur.data_ptr(), ca_y.data_ptr(), Md, keep_dec, dnext.data_ptr())
            dcur, dnext = dnext, dcur
            self.mha_bwd('d%d.ca.' % i, P, G, pre + 'encoder_attn.', dcur.data_ptr(), sa_y.data_ptr(), B, Td, mem_ptr, T4, keep_dec,
                         dnext.data_ptr(), dmem.data_ptr(), i != hp.n_dec - 1, dkv_hoisted=dkv_all[i] if hoisted else None)
            dcur, dnext = dnext, dcur
            if i == 0 and S['dec0_on_side']:
                # layer 0's self-attention block and the embedding feed parameter gradients only (the encoder's backward needs dmem,
                # which is complete): side stream, under the encoder's backward.  dcur / dnext are not touched by the main stream
                # again; the block's weight-gradient products are logged like every layer's and issued behind it on the same stream.
                def dec_epilogue(pre=pre, x_in=x_in, dcur=dcur, dnext=dnext):
                    self.mha_bwd('d0.sa.', P, G, pre + 'self_attn.', dcur.data_ptr(), x_in.data_ptr(), B, Td, x_in.data_ptr(), Td,
                                 keep_dec, dnext.data_ptr(), dnext.data_ptr(), True)
                    embed_bwd(dnext)
                self.run_on_side(dec_epilogue)
                embed_done = True
                continue
            self.mha_bwd('d%d.sa.' % i, P, G, pre + 'self_attn.', dcur.data_ptr(), x_in.data_ptr(), B, Td, x_in.data_ptr(), Td,
                         keep_dec, dnext.data_ptr(), dnext.data_ptr(), True)
            dcur, dnext = dnext, dcur
        if hoisted:
            self.cross_kv_bwd(P, G, mem_ptr, Me, dmem.data_ptr())
        self.flush_layer_wgrads()       # the decoder stack's weight gradients: one launch per parameter kind
        if not embed_done:
            embed_bwd(dcur)
        if self.slice_hook is not None:
            # every decoder-group gradient is enqueued (weights: side stream; LayerNorm partials: main, layer 0's on the side stream):
            # reduce the decoder's LayerNorm / bias partials now, BEHIND both, instead of with the encoder's at the end of the pass
            if self.use_side_stream:
                self.run_on_side(self.flush_ln_reduce)
            else:
                self.flush_ln_reduce()
            self._slice_done('decoder')

        if dmem_hook is not None:
            dmem_hook(dmem)
        # ---- encoder ----
        eA = self.buf('_deA', (nt * Me, d))
        dcur, dnext = dmem, eA
        for i in reversed(range(hp.n_enc)):
            pre = 'encoder.layers.%d.' % i
            x_in = A['enc_in.y'] if i == 0 else A['e%d.ff.y' % (i - 1)]
            self.ffn_bwd('e%d.ff.' % i, P, G, pre + 'pos_ffn.', dcur.data_ptr(), A['e%d.sa.y' % i].data_ptr(), Me, keep_enc,
                         dnext.data_ptr())
            dcur, dnext = dnext, dcur
            self.mha_bwd('e%d.sa.' % i, P, G, pre + 'self_attn.', dcur.data_ptr(), x_in.data_ptr(), B, T4, x_in.data_ptr(), T4,
                         keep_enc, dnext.data_ptr(), dnext.data_ptr(), True)
            dcur, dnext = dnext, dcur
        # input LayerNorm (+PE: no grad) and input_linear
        de0 = dnext
        self.ln_bwd(dcur.data_ptr(), A['enc_in.xhat'].data_ptr(), A['enc_in.rstd'].data_ptr(), o('encoder.layer_norm_input.weight'),
                    None, de0.data_ptr(), g('encoder.layer_norm_input.weight'), g('encoder.layer_norm_input.bias'), Me,
                    dsum=g('encoder.input_linear_b.bias' if self.factorized else 'encoder.input_linear.bias'))
        self.flush_layer_wgrads()       # the encoder stack's weight gradients
        # input Linear and VGG front-end (convstack.py), in the mode the forward recorded
        front = convstack.front_for(self, S, G, sG)
        front.linear_bwd(de0)
        if self.slice_hook is not None:
            self.flush_ln_reduce()         # the encoder's LayerNorms (+ the input LayerNorm): their partials were all produced on this stream
            self._slice_done('encoder')
        front.linear_dgrad(de0)
        self.flush_side()
        front.convs_bwd()
        self.join_side()
        self.flush_ln_reduce()     # the parameter / bias gradients of all 17 LayerNorms of the pass: one launch (after the join: one of
                                   # the 17 backward kernels ran on the side stream)
        if self.conv_layers is not None:       # (a model without convolutions has no third parameter group to hand over)
            self._slice_done('conv')
        self.nt, self.sP, self.sG = 1, 0, 0
