"""bench.py -- meta-steps/sec of the `--copy-grad` meta-transfer step on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: either launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`, or started plainly --
    without RANK / WORLD_SIZE in the environment the script starts its own N ranks under torch.distributed.run: `self_launch_command`)

One "step" = one meta-iteration of `TransientTrainer` (the reference's timed span, trainer/asr/transient_trainer.py:152-264):
every task does {train forward+backward at theta0, fused inner SGD, validation forward+backward at theta'}, copy_grad
accumulation, ONE all-reduce of the flat meta-gradient (N > 1), Adam, and the loss/CER read-back.

Workload (all N): 8 synthetic meta-tasks, k_train = k_valid = 8 utterances of 1000 frames x 161 bins, 100 labels,
enc2/dec4 d512 h8 r100 V=3765, fp32, dropout 0 -- tasks sharded round-robin over the ranks (8/N per GPU, strong scaling;
SURVEY.md 8(d)).  `value`: inputs resident in HBM when the timed region starts, nothing but the meta-steps
inside it (no profiling events).  A plain run sets up, warms up, times the K steps, writes the last step's outputs when
--dump-outputs is given (`dump_outputs`) and prints the line.  With --full it goes on, and reports in the same line: the same
steps with every batch uploaded from pinned host memory inside the timed span (`with_h2d`, what the reference's span
contains), the README-faithful 3-task / 1-GPU configuration (BASELINE.json configs[1]), the dropout-0.1 variant, and -- after the timed region -- a SERIAL profiling step that
brackets EVERY library launch with HIP events on its own stream: the `roofline` object names the kernel class with the largest
accumulated time over ALL classes (convolutions, GEMM engines, attention, LayerNorm, ...) and carries the per-class table.
`cpu_baseline` (--full): the CPU oracle on the host cores (bounded sample, N = 1 only).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CFG = dict(num_enc_layers=2, num_dec_layers=4, num_heads=8, dim_model=512, dim_key=64, dim_value=64, dim_inner=512,
           dim_emb=512, src_max_len=5000, tgt_max_len=2500, r=100, vocab_size=3765)
# /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_MFMA_TFLOPS = 157.3      # v_mfma_f32_32x32x2_f32 / 16x16x4_f32: exact fp32, no TF32 on gfx950
PEAK_BF16_MFMA_TFLOPS = 2516.6    # v_mfma_f32_32x32x16_bf16, dense
# the split-bf16 ("x3") convolution kernels issue SIX bf16 MFMAs per fp32-equivalent multiply-accumulate step, so the roof of
# their ALGORITHMIC (fp32-equivalent) FLOP rate is the dense bf16 peak / 6
PEAK_X3_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
# the two-piece fp16 ("h2") kernels issue THREE v_mfma_f32_32x32x16_f16 (same dense rate as bf16) per fp32-equivalent step
PEAK_H2_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 3.0
PEAK_HBM_GBS = 8000.0             # HBM3E spec (6.3 TB/s measured achievable)


class ResidentTask:
    """Synthetic task whose (train, valid) batches already live in HBM (the contract's `.sample` duck-type)."""

    def __init__(self, mtl, task_id, k, T, L, V, device):
        def mk(part):
            x, lens, y = mtl.synth_batch(10 * task_id + part, k, T, L, V)
            return (x.to(device), lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32))
        self.batches = (mk(0), mk(1))

    def sample(self, k_train, k_valid, manifest_id):
        return self.batches


class PinnedHostTask:
    """The same batches in page-locked HOST memory: the trainer uploads them (non-blocking) inside the timed span, like the
    reference's `.cuda()` calls at transient_trainer.py:182-184,210-212."""

    def __init__(self, mtl, task_id, k, T, L, V):
        def mk(part):
            x, lens, y = mtl.synth_batch(10 * task_id + part, k, T, L, V)
            return (x.pin_memory(), lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32))
        self.batches = (mk(0), mk(1))

    def sample(self, k_train, k_valid, manifest_id):
        return self.batches


class RaggedTask:
    """What a manifest-fed run hands over: every call a NEW batch padded to its own longest utterance (data.py:77) -- frame counts
    drawn per sample from [lo, hi], so the width differs from task to task and from step to step.  Resident in HBM."""

    def __init__(self, task_id, k, lo, hi, L, V, device, mode='ragged'):
        self.g = torch.Generator().manual_seed(77 + task_id)
        self.k, self.lo, self.hi, self.L, self.V, self.dev, self.mode = k, lo, hi, L, V, device, mode
        self.vary_labels = False          # (probe: label widths of L / 2 ... L, a new one per batch)

    def batch(self):
        if self.mode == 'fixed':
            T = (self.lo + self.hi) // 2
            lens = torch.full((self.k,), T, dtype=torch.int32)
        else:
            lens = torch.randint(self.lo, self.hi + 1, (self.k,), generator=self.g).to(torch.int32)
            T = int(lens.max()) if self.mode == 'ragged' else self.hi
        x = torch.randn(self.k, 1, 161, T, device=self.dev)
        for i in range(self.k):
            x[i, :, :, int(lens[i]):] = 0
        L = self.L if not self.vary_labels else int(torch.randint(max(self.L // 2, 1), self.L + 1, (1,), generator=self.g))
        y = torch.randint(4, self.V, (self.k, L), generator=self.g)
        return (x, lens, lens.float() / T, y, (y != 0).sum(1).to(torch.int32))

    def sample(self, k_train, k_valid, manifest_id):
        return self.batch(), self.batch()


def ragged_steps(trainer, model, vocab, tasks, n_tasks, inner, outer, args, steps, warmup, dev):
    """The production loop (pipelined enqueue, every iteration resolved inside the span) on batches that change shape every step.
    -> (seconds, frames processed, host enqueue ms per step)"""
    pending, host, frames, dt = [], [], 0, 0.0
    depth = max(getattr(trainer, 'pipeline_depth', 1), 1)
    for timed, n in ((False, warmup), (True, steps)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            local = [t.batch() for t in tasks]
            val = tasks[-1].batch()
            if timed:
                frames += sum(int(b[0].shape[0] * b[0].shape[3]) for b in local) + len(local) * int(val[0].shape[0] * val[0].shape[3])
            h0 = time.perf_counter()
            pending.append(trainer.enqueue_iteration(model, vocab, local, val, n_tasks, inner, outer, args))
            if timed:
                host.append((time.perf_counter() - h0) * 1e3)
            while len(pending) > depth:
                pending.pop(0).result()
        while pending:
            pending.pop(0).result()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
    return dt, frames, host


def make_args(k, lr=1e-4, meta_lr=1e-4):
    return argparse.Namespace(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='spectrogram', dim_input=161,
                              dropout=0.0, emb_trg_sharing=False, label_smoothing=0.0, name='bench', lr=lr, meta_lr=meta_lr,
                              k_train=k, k_valid=k, clip=False, max_norm=400, save_every=10 ** 9, save_folder='/tmp/mtl_bench',
                              cuda=True, **{a: b for a, b in CFG.items() if a not in ('vocab_size', 'r')})


# ------------------------------------------------------------------------------------------------------------------
# launch-level profiling: every library call that launches kernels, bracketed with HIP events on the stream it is given
# ------------------------------------------------------------------------------------------------------------------
_NOT_LAUNCHES = {'mtl_lstm_layer_supported', 'mtl_lstm_stack_supported', 'mtl_lstm_stack_scratch', 'mtl_gemm_x3_min_tiles', 'mtl_event_record', 'mtl_stream_wait_event', 'mtl_cmdlist_run', 'mtl_cmdlist_opcode', 'mtl_abi_version',
                 'mtl_attn_supported', 'mtl_gemm_f32_ex_route', 'mtl_levenshtein_u32', 'mtl_layernorm_bwd_g_waves'}


class LaunchProfiler:
    """Stands in for the ctypes handle of the engine(s) during ONE serial meta-step."""

    def __init__(self, handle, device):
        self._h, self._dev, self.records, self._streams, self._cache = handle, device, [], {}, {}

    def _stream(self, raw):
        raw = int(raw or 0)
        s = self._streams.get(raw)
        if s is None:
            s = torch.cuda.ExternalStream(raw, device=self._dev) if raw else torch.cuda.default_stream(self._dev)
            self._streams[raw] = s
        return s

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            real = getattr(self._h, name)
            if name in _NOT_LAUNCHES or name.endswith('_workspace') or name.endswith('_bytes'):
                fn = real
            else:
                def fn(*args, _real=real, _name=name):
                    s = self._stream(args[0])
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(s)
                    rc = _real(*args)
                    b.record(s)
                    self.records.append((_name, args, a, b))
                    return rc
            self._cache[name] = fn
        return fn


def _conv_layer(cin, cout):
    return {(64, 64): 2, (64, 128): 5, (128, 128): 7}.get((cin, cout), 0)




def single_task_form(name, a):
    """mtl_conv3x3_*_h2_tb (the samples of `tasks` meta-tasks in one launch) -> the name and argument tuple of the single-task entry
    point over tasks x B samples: same leading arguments, (B, T, F, Cin, Cout) last."""
    # (argument counts as in include/mtl_hip.h: a prototype that grows must fail HERE, not shift the dimensions silently -- round 5's
    # `widths, wshift` once turned the convolutions into zero-work launches and the roofline object into the GEMM family)
    arity = {'mtl_conv3x3_relu_fwd_h2_tb': 19, 'mtl_conv3x3_relu_pool_fwd_h2_tb': 20, 'mtl_conv3x3_dgrad_h2_tb': 19, 'mtl_conv3x3_wgrad_h2_tb': 20,
             'mtl_conv3x3_relu_fwd_x3_tb': 15, 'mtl_conv3x3_relu_pool_fwd_x3_tb': 16, 'mtl_conv3x3_dgrad_x3_tb': 15, 'mtl_conv3x3_wgrad_x3_tb': 16}
    if name in arity and len(a) != arity[name]:
        raise RuntimeError('%s called with %d arguments, classify() expects %d' % (name, len(a), arity[name]))
    if name in ('mtl_conv3x3_relu_fwd_h2_tb', 'mtl_conv3x3_relu_pool_fwd_h2_tb'):
        B, T, F, cin, cout, tasks = a[-12:-6]
        return name[:-3], tuple(a[:-12]) + (B * tasks, T, F, cin, cout)
    if name == 'mtl_conv3x3_dgrad_h2_tb':
        B, T, F, cin, cout, tasks = a[-11:-5]
        return name[:-3], tuple(a[:-11]) + (B * tasks, T, F, cin, cout)
    if name == 'mtl_conv3x3_wgrad_h2_tb':
        B, T, F, cin, cout, tasks = a[-10:-4]
        return name[:-3], tuple(a[:-10]) + (B * tasks, T, F, cin, cout)
    if name in ('mtl_conv3x3_relu_fwd_x3_tb', 'mtl_conv3x3_relu_pool_fwd_x3_tb'):      # (..., B, T, F, Cin, Cout, tasks, sW, sBias, widths, wshift)
        B, T, F, cin, cout, tasks = a[-10:-4]
        return name[:-3], tuple(a[:-10]) + (B * tasks, T, F, cin, cout)
    if name == 'mtl_conv3x3_dgrad_x3_tb':                                               # (..., B, T, F, Cin, Cout, tasks, sW, widths, wshift)
        B, T, F, cin, cout, tasks = a[-9:-3]
        return name[:-3], tuple(a[:-9]) + (B * tasks, T, F, cin, cout)
    if name == 'mtl_conv3x3_wgrad_x3_tb':                                               # (stream, x, dy, argmax, dw, db, ws, bytes, B, ..., tasks, sDw, sDb)
        B, T, F, cin, cout, tasks = a[-8:-2]
        return name[:-3], tuple(a[:4]) + (a[4],) + tuple(a[6:8]) + (B * tasks, T, F, cin, cout)
    return name, a


def classify(lib, name, a, conv_mode):
    """(class, algorithmic work, 'flop' | 'byte' | None, rocprofv3 kernel symbol(s)) of one library call; `a` = its arguments in
    the order of include/mtl_hip.h.  FLOPs are 2 x MACs of the dense extent of the reference op; bytes are the tensors the op
    must read and write once."""
    name, a = single_task_form(name, a)
    if name in ('mtl_gemm_f32_ex', 'mtl_gemm_f32', 'mtl_gemm_f32_tb'):
        M, N, K, batch = a[3], a[4], a[5], a[17]              # (mtl_gemm_f32_tb: batch counts the items of all tasks)
        kb, rs = (a[26], a[29]) if name != 'mtl_gemm_f32' else (1, None)
        route = lib.mtl_gemm_f32_ex_route(M, N, K, batch, kb, 1 if rs else 0) if name != 'mtl_gemm_f32' else 0
        if route == 2 and not (a[1] and a[2]):                # the bf16-split engine (the pass has no doubly transposed product)
            return 'gemm_x3', 2.0 * M * N * K * batch * kb, 'flop', 'gemm_x3_kernel<TA,TB,RS>'
        if route == 3 and not a[1] and a[2]:                  # few rows x every weight once (the decode session's products): weight streaming
            return 'gemm_rows', 4.0 * batch * (N * K + M * K + M * N), 'byte', 'gemm_rows_kernel<8|16>'
        small = route in (1, 3)
        return ('gemm_small' if small else 'gemm_big', 2.0 * M * N * K * batch * kb, 'flop',
                'gemm16_kernel<...>' if small else 'gemm_kernel<...> (+ splitk_reduce_kernel)')
    if name == 'mtl_gemm_h2_tb':
        return 'gemm_h2', 2.0 * a[2] * a[3] * a[4] * a[18], 'flop', 'gemm_x3_kernel<.,.,.,BM,2> (two fp16 pieces)'
    if name == 'mtl_gemm_h2_tn_tb':
        return 'gemm_h2', 2.0 * a[1] * a[2] * a[3] * a[14], 'flop', 'gemm_x3_kernel<.,.,.,BM,2> (two fp16 pieces)'
    if name.startswith('mtl_conv3x3_') and 'wprep' not in name:
        B, T, F, cin, cout = a[-5:]
        kind = 'wgrad' if 'wgrad' in name else ('dgrad' if 'dgrad' in name else ('fwd_pool' if 'pool' in name else 'fwd'))
        if name.endswith('_x3') or name.endswith('_h2'):
            sym = ('conv3x3_wgrad_x3_kernel<.,%d>' if kind == 'wgrad' else 'conv3x3_x3h_kernel<...,%d>') % (2 if name.endswith('_h2') else 3)
            if kind == 'wgrad' and name.endswith('_h2') and a[5]:
                sym = 'conv3x3_wgrad_sp_kernel (pooled layer: 2:4-sparse v_smfmac_f32_32x32x32_f16)'      # the arg-max map is given
        else:
            sym = 'conv3x3_wgrad_kernel' if kind == 'wgrad' else 'conv3x3_kernel'
        return ('conv%d_%s' % (_conv_layer(cin, cout), kind), 2.0 * B * T * F * 9 * cin * cout, 'flop', sym)
    if name == 'mtl_conv0_relu_fwd':
        B, T, F = a[-4:-1]
        return 'conv0_fwd', 4.0 * B * T * F * (1 + 64), 'byte', 'conv0_fwd_kernel'
    if name == 'mtl_conv0_relu_fwd_tb':                        # (..., B, T, F, amax_y, tasks, sX, sW, sBias, sAmax)
        B, T, F, tasks = a[5], a[6], a[7], a[9]
        return 'conv0_fwd', 4.0 * B * tasks * T * F * (1 + 64), 'byte', 'conv0_fwd_kernel'
    if name == 'mtl_conv0_wgrad':
        B, T, F = a[-3:]
        return 'conv0_wgrad', 4.0 * B * T * F * (1 + 64), 'byte', 'conv0_wgrad_kernel (+ final)'
    if name == 'mtl_conv0_wgrad_tb':                           # (..., B, T, F, tasks, sX, sDw, sDb)
        B, T, F, tasks = a[6], a[7], a[8], a[9]
        return 'conv0_wgrad', 4.0 * B * tasks * T * F * (1 + 64), 'byte', 'conv0_wgrad_kernel (+ final)'
    if name == 'mtl_colsum_accum_tb':                          # (stream, X, rows, cols, out, ws, amax, tasks, sOut, sAmax)
        return 'colsum', 4.0 * a[2] * a[3] * a[7], 'byte', 'colsum_partial_vec_kernel + colsum_final_kernel'
    if name in ('mtl_attn_fwd', 'mtl_attn_bwd'):
        causal, B, H, Tq, Tk, dk = a[8], a[10], a[11], a[12], a[13], a[14]
        prods = 2 if name == 'mtl_attn_fwd' else 7            # backward recomputes S: 2 x QK^T, dP, dV, dQ, dK (+ the second S)
        return (name[4:], prods * 2.0 * B * H * Tq * Tk * dk * (0.5 if causal else 1.0), 'flop',
                'attn_fwd_kernel' if prods == 2 else 'attn_bwd_kernel (key side + query side in one grid)')
    if name in ('mtl_layernorm_fwd', 'mtl_layernorm_fwd_g'):
        rows, d = a[12], a[13]
        return 'layernorm_fwd', 4.0 * rows * d * (4 if a[2] else 3), 'byte', 'layernorm_fwd_kernel'
    if name in ('mtl_layernorm_bwd', 'mtl_layernorm_bwd_g'):
        rows, d = a[15], a[16]
        return 'layernorm_bwd', 4.0 * rows * d * (4 if a[10] else 3), 'byte', 'layernorm_bwd_kernel (parameter reductions: ln_param_reduce_batch_kernel, once per pass)'
    if name in ('mtl_ce_argmax_fwd', 'mtl_ce_argmax_fwd_g'):
        return 'ce_fwd', 4.0 * a[3] * a[4], 'byte', 'ce_fwd_kernel'
    if name in ('mtl_ce_bwd', 'mtl_ce_bwd_g'):
        return 'ce_bwd', 8.0 * a[4] * a[5], 'byte', 'ce_bwd_kernel'
    if name == 'mtl_colsum_accum':
        return 'colsum', 4.0 * a[2] * a[3], 'byte', 'colsum_partial_kernel + colsum_final_kernel'
    if name in ('mtl_lstm_layer_fwd', 'mtl_lstm_layer_bwd'):
        T, B, H = a[-4:-1]             # the recurrent products of all T steps (forward h W_hh^T, backward dG W_hh)
        return name[4:], 2.0 * T * B * 4 * H * H, 'flop', name[4:] + '_kernel<H/8> (persistent: one launch per layer and direction)'
    if name in ('mtl_lstm_stack_fwd', 'mtl_lstm_stack_bwd'):
        T, B, H, NL = a[-5:-1]         # recurrent products of every layer + the input products of the layers above the first
        return name[4:], 2.0 * T * B * 4 * H * H * (2 * NL - 1), 'flop', name[4:] + '_kernel<H/8> (persistent wavefront: one launch per direction for all layers)'
    if name in ('mtl_lstm_cell_fwd', 'mtl_lstm_cell_bwd'):
        B, H = a[-2:]
        return name[4:], 4.0 * B * H * (15 if name.endswith('fwd') else 17), 'byte', name[4:] + '_kernel'
    if name in ('mtl_sgd_theta_prime', 'mtl_axpy'):
        return name[4:], 12.0 * a[-1], 'byte', name[4:] + '_kernel'
    if name == 'mtl_sgd_theta_prime_tasks':
        return 'sgd_theta_prime', 4.0 * a[5] * (1 + 2 * a[6]), 'byte', 'sgd_theta_prime_tasks_kernel'
    if name == 'mtl_sum_tasks':
        return 'sum_tasks', 4.0 * a[3] * (1 + a[4]), 'byte', 'sum_tasks_kernel'
    if name in ('mtl_embed_pe_fwd_g', 'mtl_embed_bwd_g'):
        return name[4:-2], None, None, name[4:-2] + '_kernel'
    if name == 'mtl_adam_step':
        return 'adam_step', 28.0 * a[-1], 'byte', 'adam_kernel'
    if name == 'mtl_permute_hc':
        return 'permute_hc', 8.0 * a[3] * a[4] * a[5], 'byte', 'permute_hc_kernel'
    if name == 'mtl_permute_hc_tb':
        return 'permute_hc', 8.0 * a[3] * a[4] * a[5] * a[8] + (4.0 * a[3] * a[4] * a[5] * a[8] if a[6] else 0.0), 'byte', 'permute_hc_kernel'
    if name in ('mtl_memcpy_d2d', 'mtl_copy_f32'):
        return 'copy', 2.0 * a[-1] * (4 if name == 'mtl_copy_f32' else 1), 'byte', '__amd_rocclr_copyBuffer'
    if name == 'mtl_memset_zero':
        return 'memset', 1.0 * a[-1], 'byte', '__amd_rocclr_fillBuffer'
    return name[4:], None, None, name[4:] + '_kernel'


# rocprofv3 kernel symbol (template name without its arguments) of every per-layer / per-shape class: the `roofline` object of the
# bench line aggregates by SYMBOL FAMILY -- what a `rocprofv3 --kernel-trace --stats` summary lists -- so that nine convolution
# classes (layer x direction) cannot hide behind one GEMM class that lumps thirteen shapes together
def family_of(cls, symbols):
    if cls.startswith('conv') and cls.endswith('_wgrad') and not cls.startswith('conv0'):
        return 'conv3x3_wgrad_sp_kernel' if 'wgrad_sp' in symbols else ('conv3x3_wgrad_x3_kernel' if 'wgrad_x3' in symbols else 'conv3x3_wgrad_kernel')
    if cls.startswith('conv') and not cls.startswith('conv0') and ('_fwd' in cls or '_dgrad' in cls):
        return 'conv3x3_x3h_kernel' if 'x3h' in symbols else 'conv3x3_kernel'
    return {'gemm_x3': 'gemm_x3_kernel<.,.,.,.,3>', 'gemm_h2': 'gemm_x3_kernel<.,.,.,.,2>', 'gemm_small': 'gemm16_kernel', 'gemm_big': 'gemm_kernel',
            'attn_fwd': 'attn_fwd_kernel', 'attn_bwd': 'attn_bwd_kernel', 'layernorm_fwd': 'layernorm_fwd_kernel',
            'layernorm_bwd': 'layernorm_bwd_kernel', 'conv0_fwd': 'conv0_fwd_kernel', 'conv0_wgrad': 'conv0_wgrad_kernel'}.get(cls, cls)


DTYPE = {'h2': 'f32 (emulated: 3x3 conv + input Linear on 2 x fp16 pieces "h2" = 22 significand bits, big GEMMs and '
               'attention (d_k = 64) on 3 x bf16 pieces "x3" = exact fp32 operands, small products on fp32 MFMA, element-wise on VALU; fp32 '
               'accumulation everywhere)',
         'x3': 'f32 (emulated: 3x3 conv + big GEMMs + attention (d_k = 64) on 3 x bf16 pieces "x3" = exact fp32 operands, input Linear on 2 x fp16 '
               'pieces, small products on fp32 MFMA, element-wise on VALU; fp32 accumulation everywhere)',
         'f32': 'f32 (every product on v_mfma_f32_*_f32 / VALU)'}


def algorithmic_bytes(name, a, unit, work):
    """Bytes a launch must move once (operands read once, results written once): the yardstick of `traffic`."""
    name, a = single_task_form(name, a)
    if unit == 'byte':
        return work
    if name.startswith('mtl_conv3x3_') and 'wprep' not in name:
        B, T, F, cin, cout = a[-5:]
        px = float(B) * T * F
        pooled_out = 'pool' in name                                   # forward: pooled map + one arg-max byte per pooled element
        if 'wgrad' in name:
            pooled_dy = bool(a[5] if name.endswith('_h2') else a[3])  # arg-max pointer: dy lives on the pooled grid
            return 4 * px * cin + (px / 4 * cout * 5 if pooled_dy else 4 * px * cout) + 4 * 9.0 * cin * cout
        if 'dgrad' in name:
            pooled_dy = bool(a[3] if name.endswith('_h2') else a[2])
            return (px / 4 * cout * 5 if pooled_dy else 4 * px * cout) + 8 * px * cin   # dy (+ arg-max) in, ReLU gate in + dx out
        return 4 * px * cin + (px / 4 * cout * 5 if pooled_out else 4 * px * cout)
    if name in ('mtl_gemm_f32_ex', 'mtl_gemm_f32_tb'):
        M, N, K, batch, kb = a[3], a[4], a[5], a[17], a[26]
        return 4.0 * batch * (M * K * kb + K * N * kb + M * N)
    if name == 'mtl_gemm_h2_tb':
        M, N, K, nt = a[2], a[3], a[4], a[18]
        return 4.0 * nt * (M * K + K * N + M * N)
    if name == 'mtl_gemm_h2_tn_tb':
        M, N, K, nt = a[1], a[2], a[3], a[14]
        return 4.0 * nt * (M * K + K * N + M * N)
    if name in ('mtl_attn_fwd', 'mtl_attn_bwd'):
        B, H, Tq, Tk, dk = a[10], a[11], a[12], a[13], a[14]
        return 4.0 * B * H * dk * ((2 * Tq + 2 * Tk) if name == 'mtl_attn_fwd' else (4 * Tq + 4 * Tk))
    return 0.0


# classes whose kernels issue SIX bf16 MFMAs per fp32-equivalent multiply-accumulate (operands as exact bf16 triples): the big GEMM
# engine and -- since round 4 -- the flash attention kernels at the supported head sizes (csrc/mtl_attn.hip, v_mfma_f32_16x16x32_bf16)
X3_CLASSES = ('gemm_x3', 'attn_fwd', 'attn_bwd')


def peak_of(cls, unit, conv_mode):
    if unit == 'byte':
        return PEAK_HBM_GBS, 'GB/s', 'hbm'
    if cls == 'gemm_h2':
        return PEAK_H2_TFLOPS, 'TFLOP/s', 'mfma'
    if cls in X3_CLASSES:
        return PEAK_X3_TFLOPS, 'TFLOP/s', 'mfma'
    if cls.startswith('conv') and conv_mode != 'f32':
        return (PEAK_H2_TFLOPS if conv_mode == 'h2' else PEAK_X3_TFLOPS), 'TFLOP/s', 'mfma'
    return PEAK_F32_MFMA_TFLOPS, 'TFLOP/s', 'mfma'


def dump_shapes(records):
    """diagnostics (MTL_BENCH_SHAPES=<file>): per-shape time of the product / attention / LayerNorm launches of the profiled step"""
    dump = os.environ.get('MTL_BENCH_SHAPES')
    if not dump:
        return
    shapes = {}
    for name, a, e0, e1 in records:
        if name in ('mtl_gemm_f32_ex', 'mtl_gemm_f32_tb'):
            route = sys.modules['mtl_amd']._lib.lib().mtl_gemm_f32_ex_route(a[3], a[4], a[5], a[17], a[26], 1 if a[29] else 0)
            key = 'gemm %-5s ta%d tb%d M%d N%d K%d b%d kb%d rs%d gflop %.2f' % (
                {0: 'big', 1: 'small', 2: 'x3', 3: 'rows'}.get(route, '?'), a[1], a[2], a[3], a[4], a[5], a[17], a[26], 1 if a[29] else 0,
                2e-9 * a[3] * a[4] * a[5] * a[17] * a[26])
        elif name in ('mtl_attn_fwd', 'mtl_attn_bwd', 'mtl_layernorm_fwd', 'mtl_layernorm_bwd', 'mtl_layernorm_fwd_g', 'mtl_layernorm_bwd_g'):
            key = name + ' ' + ' '.join(str(v) for v in a if isinstance(v, int) and 0 <= v < 100000)
        else:
            continue
        t = shapes.setdefault(key, [0, 0.0])
        t[0] += 1
        t[1] += e0.elapsed_time(e1) * 1e3
    with open(dump, 'w') as f:
        for key, (cnt, us) in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
            f.write('%8.1f us total  %3d x %6.1f us   %s\n' % (us, cnt, us / cnt, key))


def serial_profile(mtl, trainer, model, vocab, tasks, my_tasks, n_tasks, inner, outer, args, dev):
    """One extra meta-iteration with the side stream and command-list replay switched off (and one lane, where the tasks are not
    batched) and HIP events around EVERY launch: isolated durations (what rocprofv3 reports for a non-overlapped dispatch),
    grouped into kernel classes.  The step takes the schedule of the timed region: the task-batched passes when the trainer
    batches the local tasks."""
    lanes, model.n_lanes = model.n_lanes, 1
    prof = LaunchProfiler(mtl._lib.lib(), dev)
    saved = []
    for e in model.engines:
        saved.append((e.lib, e.use_side_stream))
        e.lib, e.use_side_stream, e.prof = prof, False, prof
    val = tasks[-1].sample(0, 0, 0)[1]
    local = [tasks[m].sample(0, 0, m)[0] for m in my_tasks]
    # The host needs ~15 us per launch here (Python + two event records), most kernels of the transformer half take less: on an
    # idle stream every [event, kernel, event] interval would contain the launch latency instead of the kernel.  A spin kernel
    # holds the stream while the host enqueues the whole step, so the launches then execute back to back and the intervals
    # are the kernels' own durations (+ the ~1.5 us dependent-launch boundary), as rocprofv3 reports them.
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(2000000)
    b.record()
    torch.cuda.synchronize(dev)
    per_count = max(a.elapsed_time(b) - 0.01, 1e-3) / 2000000.0          # ms per spin count
    hold_ms = 40.0 + 60.0 * max(len(local), 1)               # generous: ~60 ms of enqueue per task at this instrumentation level
    h0, h1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    h0.record()
    torch.cuda._sleep(int(hold_ms / per_count))
    h1.record()
    trainer.run_iteration(model, vocab, local, val, n_tasks, inner, outer, args)
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0 - h0.elapsed_time(h1) * 1e-3          # GPU-side time of the step once the hold ended
    for e, (lib_, side) in zip(model.engines, saved):
        e.lib, e.use_side_stream, e.prof = lib_, side, None
    model.n_lanes = lanes
    eng = model.engine
    classes = {}
    for name, a, e0, e1 in prof.records:
        cls, work, unit, sym = classify(mtl._lib.lib(), name, a, eng.conv_mode)
        c = classes.setdefault(cls, dict(time=0.0, work=0.0, unit=unit, launches=0, symbols=sym, abytes=0.0))
        c['time'] += e0.elapsed_time(e1) * 1e-3
        c['work'] += work or 0.0
        c['abytes'] += algorithmic_bytes(name, a, unit, work or 0.0)
        c['launches'] += 1
    dump_shapes(prof.records)
    return classes, len(prof.records), wall


HOST_ENQUEUE = {}
HOST = {}
PER_RANK = {}


TRACE = [] if os.environ.get('MTL_BENCH_TRACE') else None      # diagnostics: (seconds into the timed span, host enqueue ms) per step, to stderr


_SW = []


def stall_watch():
    """diagnostics (MTL_STALL_WATCH=<ms>): tools/probe/libstallwatch.so reports what the host thread is blocked in whenever one
    enqueue_iteration takes longer than <ms> (kernel-side state + native backtrace, to stderr)"""
    thr = os.environ.get('MTL_STALL_WATCH')
    if not thr:
        return None
    if not _SW:
        import ctypes
        lib = ctypes.CDLL(os.path.join(ROOT, 'tools', 'probe', 'libstallwatch.so'))
        lib.sw_start.argtypes = [ctypes.c_double, ctypes.c_int]
        lib.sw_start(float(thr), 2)
        _SW.append(lib)
    return _SW[0]


def timed_steps(trainer, model, vocab, tasks, my_tasks, n_tasks, inner, outer, args, steps, warmup, mdist, dev):
    fresh = hasattr(tasks[0], 'batch')            # --ragged: new batches (new shapes) every step
    state = {}

    def draw():
        if fresh:       # every rank draws EVERY task's batch (the generators stay in lock-step across the ranks, like the reference's loop)
            every = [t.batch() for t in tasks]
            state['val'] = tasks[-1].batch()
            state['local'] = [every[m] for m in my_tasks]
        elif not state:
            state['val'] = tasks[-1].sample(0, 0, 0)[1]
            state['local'] = [tasks[m].sample(0, 0, m)[0] for m in my_tasks]
        return state['local'], state['val']

    def one():
        local, val = draw()
        return trainer.run_iteration(model, vocab, local, val, n_tasks, inner, outer, args)
    for _ in range(warmup):
        one()
    mdist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    host = []
    # the loop of TransientTrainer.train: up to `pipeline_depth` iterations are enqueued beyond the one whose read-backs are being
    # resolved (loss, CER strings: host work that would otherwise be GPU idle time); every one of the K iterations is resolved INSIDE
    # the timed span
    pipelined = getattr(trainer, 'pipeline', False) and hasattr(trainer, 'enqueue_iteration')
    depth = max(getattr(trainer, 'pipeline_depth', 1), 1)
    pending = []
    sw = stall_watch()
    for _ in range(steps):
        if pipelined:
            local, val = draw()
            if sw is not None:
                sw.sw_enter()
            pending.append(trainer.enqueue_iteration(model, vocab, local, val, n_tasks, inner, outer, args))
            if sw is not None:
                sw.sw_exit()
            while len(pending) > depth:
                last = pending.pop(0).result()
        else:
            last = one()
        host.append(getattr(trainer, 'host_enqueue_s', 0.0) * 1e3)
        if TRACE is not None:
            TRACE.append((round(time.perf_counter() - t0, 3), round(getattr(trainer, 'host_enqueue_s', 0.0) * 1e3, 1)))
            ph = sys.modules['mtl_amd']._trace.steps
            if ph:
                print('phases step@%.3f: %s' % (time.perf_counter() - t0, json.dumps(ph[-1])), file=sys.stderr)
                del ph[:]
    while pending:
        last = pending.pop(0).result()
    # host time to enqueue a step (the rest of the span it waits for the GPU)
    HOST_ENQUEUE.update(mean=sum(host) / max(len(host), 1), median=sorted(host)[len(host) // 2] if host else 0.0, max=max(host) if host else 0.0)
    if TRACE is not None:
        try:
            age = time.time() - os.stat('/proc/1').st_ctime
        except OSError:
            age = -1.0
        print('trace: container age %.0f s; per step (t, host enqueue ms): %s' % (age, ' '.join('%s:%s' % p for p in TRACE)), file=sys.stderr)
        del TRACE[:]
    torch.cuda.synchronize(dev)
    mdist.barrier()
    dt = time.perf_counter() - t0
    if mdist.world_size() > 1:
        # MAX over the ranks is the step time; every rank's own figure (its local tasks + its wait for the collective) is reported too
        mine = torch.tensor([dt], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(mdist.world_size())]
        torch.distributed.all_gather(every, mine)
        PER_RANK['ms_per_step'] = [round(float(v) / steps * 1e3, 3) for v in every]
        dt = max(float(v) for v in every)
    return dt, last


def cpu_baseline(n_tasks, k, T, L, threads, timed_tasks):
    """The CPU oracle (restatement of the reference pinned to goldens generated from it) on the host cores.  Every
    task of a meta-step has the same shapes and costs the same, so `timed_tasks` tasks (train pass + validation pass, each
    forward + backward) are timed after one warm-up task, plus the Adam step, and scaled to the n_tasks of the step."""
    from oracle import refimpl as R
    torch.set_num_threads(threads)
    model = R.build_model(CFG)
    adam = R.AdamState(list(model.parameters()), 1e-4)
    tr = [R.synth_batch(0, k, T, L, CFG['vocab_size'])]
    val = R.synth_batch(1, k, T, L, CFG['vocab_size'])
    R.meta_gradient(model, tr, val, 1e-4)                      # warm-up (thread pools, oneDNN primitive cache)
    times = []
    for i in range(timed_tasks):
        t0 = time.perf_counter()
        G, _, _, _ = R.meta_gradient(model, [R.synth_batch(10 * (i + 1), k, T, L, CFG['vocab_size'])], val, 1e-4)
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    adam.step(list(model.parameters()), G)
    t_outer = time.perf_counter() - t0
    t_task = sum(times) / len(times)
    return dict(value=1.0 / (n_tasks * t_task + t_outer), unit='meta-steps/s', cores=threads, kind='port',
                sample='%d of %d tasks timed after 1 warm-up task (each = 2 forward+backward passes; %s s) + Adam step (%.3f s); '
                       'every task has the same shapes, scaled x%d/%d' % (timed_tasks, n_tasks, ', '.join('%.2f' % t for t in times),
                                                                          t_outer, n_tasks, timed_tasks),
                seconds_per_task=t_task)


def h2_frac(trainer):
    """the trainer's latest census of the h2 operands (TransientTrainer.h2_check_every: sampled on the first iteration and every 100th):
    the largest share, over the operands, of non-zero elements that keep fewer than 22 / fewer than 16 significand bits"""
    cen = getattr(trainer, 'h2_census', None)
    if not cen:
        return None
    return dict(lt22_bits=max(v[0] for v in cen.values()), lt16_bits=max(v[1] for v in cen.values()),
                worst_operand=max(cen, key=lambda k_: cen[k_][0]), limit_lt16=trainer.h2_limit, sampled_every=trainer.h2_check_every)


DUMP_SAMPLE = 1 << 22          # elements kept of a larger output (16 MB in float32): a fixed, seeded choice of positions


def dump_outputs(dirname, arrays):
    """--dump-outputs DIR: what the timed path handed its caller after the LAST timed step, one DIR/<name>.npy each -- `theta` (the
    flat parameters after the outer step), `meta_grad` (the flat meta-gradient that step applied, summed over the ranks) and
    `last_step` (float64: validation loss summed over the tasks, CER edits, characters).  Device tensors are written in float32;
    one of more than DUMP_SAMPLE elements is cut to DUMP_SAMPLE of them at positions drawn once from a fixed seed (sorted, the same
    positions in every run of the same size), so the files stay below 64 MB in all.  Inputs and initial parameters are seeded, so
    two builds run with the same arguments can be compared file by file."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, v in arrays.items():
        if isinstance(v, torch.Tensor):
            a = v.detach().float().reshape(-1).cpu().numpy()
            if a.size > DUMP_SAMPLE:
                a = a[np.sort(np.random.default_rng(12345).choice(a.size, DUMP_SAMPLE, replace=False))]
        else:
            a = np.asarray(v, dtype=np.float64).reshape(-1)
        np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a))


def eval_leg(mtl, trainer, model, vocab, args, k, frames, labels, dev, reps=4, decode_steps=300):
    """SURVEY 8(f) f2, measured: (a) what the in-loop validation runs per batch (transient_trainer.py:280-331: eval mode, no autograd,
    `forward_one_batch` = teacher-forced pass + loss + CER strings) and (b) test-time greedy decoding (Transformer.evaluate ->
    Decoder.greedy_search, modules/decoder.py:131-185: the reference's 300 fixed steps, here K/V-cached with the token fed back
    through device memory) at the north-star model, batch = k_valid utterances of `frames` frames resident in HBM.
    The decode steps are GEMV-shaped (8 rows): every step streams the decoder's weights once, so the step is priced against HBM."""
    V = CFG['vocab_size']
    x, lens, y = mtl.synth_batch(99001, k, frames, labels, V)
    x = x.to(dev)
    pct = lens.float() / frames
    tl = (y != 0).sum(1).to(torch.int32)
    model.eval()
    out = {}
    try:
        with torch.no_grad():
            for _ in range(2):
                trainer.forward_one_batch(model, vocab, x, y.to(dev), pct.clone(), lens, tl, 0.0, 'ce')
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n = 10
            for _ in range(n):
                loss, cer, nchar = trainer.forward_one_batch(model, vocab, x, y.to(dev), pct.clone(), lens, tl, 0.0, 'ce')
                float(loss.item())
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / n
        out['valid_loop'] = dict(utt_per_s=k / dt, ms_per_batch=dt * 1e3, batch=k,
                                 note='forward_one_batch in eval mode (teacher-forced pass + loss + host CER strings), the body of the '
                                      'in-loop validation, transient_trainer.py:280-331')
        model.evaluate(x, lens, y, args, start_token=vocab.SOS_ID, max_steps=8)                    # buffers
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            model.evaluate(x, lens, y, args, start_token=vocab.SOS_ID, max_steps=decode_steps)
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        dt = min(times)
        # one profiled decode: HIP events around every launch of the decode session (the encoder pass before it is not the subject)
        eng = model.engine
        prof = LaunchProfiler(mtl._lib.lib(), dev)
        real_greedy = eng.greedy_decode

        def profiled(*a_, **kw_):
            lib_, eng.lib, eng.prof = eng.lib, prof, prof
            try:
                return real_greedy(*a_, **kw_)
            finally:
                eng.lib, eng.prof = lib_, None
        eng.greedy_decode = profiled
        try:
            psteps = 32
            model.evaluate(x, lens, y, args, start_token=vocab.SOS_ID, max_steps=psteps)
            torch.cuda.synchronize(dev)
        finally:
            del eng.greedy_decode
        classes = {}
        for name, a_, e0, e1 in prof.records:
            cls, work, unit, sym = classify(mtl._lib.lib(), name, a_, eng.conv_mode)
            c = classes.setdefault(cls, dict(time=0.0, launches=0, symbols=sym))
            c['time'] += e0.elapsed_time(e1) * 1e-3
            c['launches'] += 1
        kt = sum(c['time'] for c in classes.values())
        dom = max(classes, key=lambda c_: classes[c_]['time'])
        lay = model._layout
        dec_bytes = 4 * sum(lay.entries[nm][2] for nm in lay.order if nm.startswith('decoder.'))
        step_ms = dt / decode_steps * 1e3
        out['greedy_decode'] = dict(utt_per_s=k / dt, ms_per_decode=dt * 1e3, ms_per_step=step_ms, steps=decode_steps, batch=k,
                                    launches_per_step=len(prof.records) / psteps, kernel_ms_per_step=kt / psteps * 1e3,
                                    dominant=dict(kernel=classes[dom]['symbols'], cls=dom, share=classes[dom]['time'] / kt,
                                                  us_per_launch=classes[dom]['time'] / classes[dom]['launches'] * 1e6),
                                    per_class={c_: dict(ms_per_step=v['time'] / psteps * 1e3, launches_per_step=v['launches'] / psteps)
                                               for c_, v in sorted(classes.items(), key=lambda kv: -kv[1]['time'])},
                                    roofline=dict(bound='hbm', achieved=dec_bytes / (step_ms * 1e-3) / 1e9, peak=PEAK_HBM_GBS, unit='GB/s',
                                                  frac=dec_bytes / (step_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                                                  algorithmic_bytes_per_step=dec_bytes,
                                                  note='a step multiplies %d hypothesis rows with every decoder weight once: the decoder '
                                                       'parameters (%.1f MB) are the algorithmic traffic of a step' % (k, dec_bytes / 1e6)),
                                    note='Transformer.evaluate greedy: encoder pass + %d K/V-cached decoder steps, token feedback on the '
                                         'device, one read-back (models/asr/transformer.py:162-202, modules/decoder.py:131-185)' % decode_steps)
        # beam search (modules/decoder.py:187-291, the reference's test-time default: width 3, 5 best): one utterance at a time, the
        # hypothesis bookkeeping on the host as in the reference, one K/V-cached device step per position for all live hypotheses
        bargs = argparse.Namespace(**vars(args))
        bargs.beam_width, bargs.beam_nbest = 3, 5
        nb = min(2, k)
        model.evaluate(x[:nb], lens[:nb], y[:nb], bargs, beam_search=True, start_token=vocab.SOS_ID)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        model.evaluate(x[:nb], lens[:nb], y[:nb], bargs, beam_search=True, start_token=vocab.SOS_ID)
        torch.cuda.synchronize(dev)
        dtb = time.perf_counter() - t0
        steps_b = max(len(h_) for h_ in model.last_beam_ids) - 1 if getattr(model, 'last_beam_ids', None) else 0
        out['beam_search'] = dict(utt_per_s=nb / dtb, ms_per_utterance=dtb / nb * 1e3, beam_width=3, nbest=5, utterances=nb, longest_hypothesis=steps_b,
                                  note='Transformer.evaluate(beam_search=True): per utterance up to T\' = %d positions, one device step + one '
                                       'read-back of the logits per position (the host ranks the hypotheses as the reference does)' % ((frames // 2) // 2))
    finally:
        model.train()
    return out


LM_CFG = dict(ntoken=10000, ninp=512, nhid=512, nlayers=2, bptt=35, batch_size=20, dropout=0.2, lr=1.0, meta_lr_factor=3.0, clip=0.25,
              ratio=0.8, corpus_len=40000)


def main_lm(a, mtl_amd, mdist, dev, rank, world):
    """BASELINE.json configs[4]: the LM meta loop (lm/main_meta_transfer.py) -- token-only, d512 2-layer LSTM, `--tasks` synthetic
    corpora sharded over the ranks, one all-reduce of the flat G.  One step = one meta-iteration (every task: train pass, clipped
    inner SGD step, validation pass at theta'; clipped outer SGD step).  Parity of this path is pinned to the oracle's documented
    first-order restatement only (the reference's loop does not run on torch >= 2)."""
    c = LM_CFG
    torch.manual_seed(1111)
    with contextlib.redirect_stdout(io.StringIO()):
        model = mtl_amd.lm.RNNModel('LSTM', c['ntoken'], c['ninp'], c['nhid'], c['nlayers'], c['dropout']).to(dev)
    model.train()
    n = a.tasks
    streams = [mtl_amd.lm.synth_corpus(100 + i, c['ntoken'], c['corpus_len']) for i in range(n)]
    ds = mtl_amd.lm.LMDataset(streams, argparse.Namespace(bptt=c['bptt'], batch_size=c['batch_size'], cuda=False))
    ds.task_list = [t.to(dev) for t in ds.task_list]
    mine = mdist.shard_tasks(n, rank, world)
    tr = mtl_amd.lm.LMMetaTrainer(model, c['lr'], c['meta_lr_factor'], c['clip'], c['ratio'])

    def one(it):
        vb = ds.sample(-1, it)[2:]
        return tr.run_iteration([ds.sample(i, it)[:2] for i in mine], vb, n, mine)
    for it in range(a.warmup):
        one(it)
    mdist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for it in range(a.warmup, a.warmup + a.steps):
        last = one(it)
    torch.cuda.synchronize(dev)
    mdist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, dict(theta=torch.cat([p_.detach().reshape(-1) for p_ in model.parameters()]),
                                          last_step=[float(last[0])] + [float(v) for v in last[1]]))
    out = None
    if rank == 0:
        out = dict(metric='meta-steps/sec', value=a.steps / dt, unit='meta-steps/s', n_gpus=world, steps=a.steps, warmup=a.warmup,
                   ms_per_step=dt / a.steps * 1e3, higher_is_better=True, scaling='strong', vs_baseline=None, dtype='f32', data='synthetic',
                   config=dict(workload='lm/main_meta_transfer.py meta loop (first-order reading, parity unpinned vs the reference loop): '
                                        '2-layer LSTM d%d V%d, bptt %d, batch %d, %d synthetic corpora (%d per GPU), dropout %.1f'
                                        % (c['nhid'], c['ntoken'], c['bptt'], c['batch_size'], n, len(mine), c['dropout']),
                               tasks=n, parallelism='task-sharded dp%d' % world, collective=mdist.backend_name(), **{k: c[k] for k in ('bptt', 'batch_size', 'nhid', 'ntoken')}),
                   last_step=dict(weighted_val_loss=last[0]))
    if not a.full:
        if rank == 0:
            emit(out)
        mdist.barrier()
        return
    # --full: serial profiling iteration: every launch bracketed with events (same scheme as the ASR workload)
    prof = LaunchProfiler(mtl_amd._lib.lib(), dev)
    eng = model.engine
    real = eng.lib
    eng.lib = prof
    torch.cuda.synchronize(dev)
    one(a.warmup + a.steps)
    torch.cuda.synchronize(dev)
    eng.lib = real
    dump_shapes(prof.records)
    classes = {}
    for name, args_, e0, e1 in prof.records:
        cls, work, unit, sym = classify(mtl_amd._lib.lib(), name, args_, 'f32')
        cc = classes.setdefault(cls, dict(time=0.0, work=0.0, unit=unit, launches=0, symbols=sym))
        cc['time'] += e0.elapsed_time(e1) * 1e-3
        cc['work'] += work or 0.0
        cc['launches'] += 1
    if rank == 0:
        passes = 2 * max(len(mine), 1)
        table = {}
        for cls, cc in sorted(classes.items(), key=lambda kv: -kv[1]['time']):
            row = dict(ms_per_pass=cc['time'] / passes * 1e3, launches_per_pass=cc['launches'] / passes, symbols=cc['symbols'])
            if cc['unit'] is not None and cc['work'] > 0:
                peak, unit, bound = peak_of(cls, cc['unit'], 'f32')
                ach = cc['work'] / cc['time'] / (1e12 if cc['unit'] == 'flop' else 1e9)
                row.update(bound=bound, achieved=ach, peak=peak, unit=unit, frac=ach / peak)
            table[cls] = row
        dom = next(k for k in table if 'frac' in table[k])
        dr, dc = table[dom], classes[dom]
        out['roofline'] = dict(bound=dr['bound'], kernel=dom, symbols=dr['symbols'], achieved=dr['achieved'], peak=dr['peak'], unit=dr['unit'],
                               frac=dr['frac'], traffic=None, work_per_launch=dc['work'] / dc['launches'],
                               avg_launch_ms=dc['time'] / dc['launches'] * 1e3, launches_timed=dc['launches'],
                               timing='HIP events around every library call of one serial meta-iteration', per_class=table)
        if world == 1 and not a.no_cpu_baseline:
            from oracle import lm_refimpl as LR           # checker-side restatement: the cpu_baseline leg only
            threads = a.cpu_threads or min(32, physical_cores(), HOST.get("effective_cpus") or 32)
            torch.set_num_threads(threads)
            oracle = LR.RNNModel(c['ntoken'], c['ninp'], c['nhid'], c['nlayers'], 0.0)
            otasks = [LR.batchify(s_, c['batch_size']) for s_ in streams]
            hid = oracle.init_hidden(c['batch_size'])
            nb = min(n, 3)
            batches = [LR.sample(otasks, i, 0, c['bptt'])[:2] for i in range(nb)]
            vb = LR.sample(otasks, -1, 0, c['bptt'])[2:]
            LR.meta_step(oracle, hid, batches[:1], vb, c['lr'], c['meta_lr_factor'], c['clip'], c['ratio'])     # warm-up
            t0 = time.perf_counter()
            LR.meta_step(oracle, hid, batches, vb, c['lr'], c['meta_lr_factor'], c['clip'], c['ratio'])
            tc = time.perf_counter() - t0
            out['cpu_baseline'] = dict(value=1.0 / (tc * n / nb), unit='meta-steps/s', cores=threads, kind='port',
                                       sample='%d of %d tasks of one meta-iteration timed after a 1-task warm-up (%.2f s), scaled x%d/%d'
                                              % (nb, n, tc, n, nb))
        emit(out)
    mdist.barrier()


def power_limited_ceiling(dev, achieved, peak):
    """The dense matrix rate the chip SUSTAINS on all CUs under its package power limit, measured live with the probe library
    (csrc/mtl_probe.hip -> libmtl_probe.so: back-to-back v_mfma_f32_32x32x16_f16, no HBM traffic), for operands that switch
    like the real ones (pseudo-random fp16, half of one operand zero = activations after a ReLU) and for zeros.  The nominal
    peak in `roofline.peak` assumes 2.4 GHz; with switching operands the clock is held far below it, so `frac` understates how
    close a matrix-bound kernel is to what the silicon delivers.  Reported next to it, never instead of it."""
    import ctypes
    import torch
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'meta-transfer-learning_amd', 'libmtl_probe.so')
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.mtl_probe_mfma_f16.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    sink = torch.zeros(4, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    steps = 3000

    def rate(mode, fill):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        lib.mtl_probe_mfma_f16(st, ncu, steps, mode, fill, sink.data_ptr())          # settle the clocks at this load
        ev[0].record()
        rc = lib.mtl_probe_mfma_f16(st, ncu, steps, mode, fill, sink.data_ptr())
        ev[1].record()
        torch.cuda.synchronize()
        if rc:
            return None
        return ncu * steps * 8 * 24 * 32768.0 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e12      # TFLOP/s of fp16 matrix work

    nominal = PEAK_H2_TFLOPS * 3                        # dense fp16 peak of the guide
    r = dict(registers_zeros=rate(0, 0), registers_random=rate(0, 1), lds_fed_random=rate(1, 1), lds_fed_post_relu=rate(1, 2),
             lds_fed_16x16x32_random=rate(4, 1), lds_fed_16x16x32_post_relu=rate(4, 2))
    if not all(r.values()):
        return None
    out = dict(unit='TFLOP/s of dense fp16 matrix instructions', nominal=nominal,
               sustained={k: v for k, v in r.items()}, sustained_frac_of_nominal={k: v / nominal for k, v in r.items()},
               note='sustained = all CUs issuing back-to-back fp16 matrix instructions for ~3 ms (registers_*: v_mfma_f32_32x32x16_f16 on register '
                    'operands; lds_fed_*: 16 ds_read_b128 per 64 x 64 x 32 wave-tile product and one s_barrier per step, the fragment traffic of '
                    'the convolution kernel, on 32x32x16 instructions or -- lds_fed_16x16x32_*, what conv3x3_x3h_kernel issues since round 4 -- on '
                    '16x16x32 ones); the package power limit, not the instruction stream, sets these rates')
    # the dominant kernel against the ceiling of ITS instruction mix and operand statistics
    scale = r['lds_fed_16x16x32_post_relu'] / nominal
    out['frac_of_sustained'] = achieved / (peak * scale)
    out['frac_note'] = 'roofline.achieved / (roofline.peak x lds_fed_16x16x32_post_relu / nominal)'
    return out


def roofline_object(classes, n_launch, serial_wall, passes, conv_mode, dev):
    """--full: the `roofline` object from the per-class launch timings of the serial profiling step (`serial_profile`): the kernel
    family with the largest accumulated time, its achieved rate against the roof of its instructions, the per-family and per-class
    tables, and the live power-limited ceiling of the probe library when that family is matrix-bound."""
    pmc = {}
    try:
        pmc = json.load(open(os.path.join(ROOT, 'profiles', 'pmc_traffic.json')))
    except Exception:
        pass
    table = {}
    for cls, c in sorted(classes.items(), key=lambda kv: -kv[1]['time']):
        # "pass" = forward + backward of ONE task's batch (a task-batched pass of nt tasks counts nt)
        row = dict(ms_per_pass=c['time'] / passes * 1e3, launches_per_pass=c['launches'] / passes, symbols=c['symbols'])
        if c['unit'] is not None and c['work'] > 0:
            peak, unit, bound = peak_of(cls, c['unit'], conv_mode)
            ach = c['work'] / c['time'] / (1e12 if c['unit'] == 'flop' else 1e9)
            row.update(bound=bound, achieved=ach, peak=peak, unit=unit, frac=ach / peak)
            if 'wgrad_sp' in c['symbols']:
                # `achieved` counts the ALGORITHMIC (dense-equivalent) FLOPs of the reference op; the kernel issues half of them as
                # 2:4-sparse instructions, whose peak is twice the dense one
                row.update(frac_of_sparse_peak=ach / (2 * peak), note='frac: dense-equivalent FLOPs / dense two-piece-fp16 peak (838.9 TF); '
                           'frac_of_sparse_peak: the same FLOPs / the 2:4-sparse peak (1677.7 TF) the instructions issue at')
        table[cls] = row
    for cls, row in table.items():
        if cls in pmc:
            row['traffic'] = pmc[cls]             # HBM bytes per launch (separate --pmc FETCH_SIZE / WRITE_SIZE passes, profiles/)
            ab = classes[cls].get('abytes', 0.0) / max(classes[cls]['launches'], 1)
            if ab > 0:
                row['algorithmic_bytes'] = ab
                row['traffic_over_algorithmic'] = pmc[cls] / ab
    # ---- aggregate by rocprofv3 symbol family; the dominant family (largest accumulated time) is the `roofline` object
    fams = {}
    for cls, c in classes.items():
        if c['unit'] is None or c['work'] <= 0:
            continue
        f = fams.setdefault(family_of(cls, c['symbols']), dict(time=0.0, work=0.0, launches=0, classes=[], unit=c['unit'], traffic=0.0,
                                                               traffic_known=True, abytes=0.0))
        f['abytes'] += c.get('abytes', 0.0)
        f['time'] += c['time']
        f['work'] += c['work']
        f['launches'] += c['launches']
        f['classes'].append(cls)
        if cls in pmc:
            f['traffic'] += pmc[cls] * c['launches']
        else:
            f['traffic_known'] = False
    fam_table = {}
    for name, f in sorted(fams.items(), key=lambda kv: -kv[1]['time']):
        peak, unit, bound = peak_of(f['classes'][0], f['unit'], conv_mode)
        ach = f['work'] / f['time'] / (1e12 if f['unit'] == 'flop' else 1e9)
        fam_table[name] = dict(ms_per_pass=f['time'] / passes * 1e3, launches_per_pass=f['launches'] / passes, bound=bound, achieved=ach,
                               peak=peak, unit=unit, frac=ach / peak, classes=f['classes'],
                               traffic=(f['traffic'] / f['launches']) if (f['traffic_known'] and f['launches']) else None)
        if name == 'conv3x3_wgrad_sp_kernel':
            fam_table[name]['frac_of_sparse_peak'] = ach / (2 * peak)
    dom = next(iter(fam_table))                      # (sorted by accumulated time)
    df, dr = fams[dom], fam_table[dom]
    arith = ('split-bf16 x3: 6 v_mfma_f32_32x32x16_bf16 per fp32-equivalent step, peak = dense bf16 / 6' if dr['peak'] == PEAK_X3_TFLOPS else (
        'two fp16 pieces (h2): 3 v_mfma_f32_32x32x16_f16 per fp32-equivalent step, peak = dense fp16 / 3' if dr['peak'] == PEAK_H2_TFLOPS else (
            'exact fp32 MFMA' if dr['bound'] == 'mfma' else 'HBM streaming')))
    roofline = dict(bound=dr['bound'], kernel=dom, symbols=dom, achieved=dr['achieved'], peak=dr['peak'], unit=dr['unit'],
                    frac=dr['frac'], traffic=dr['traffic'], algorithmic_bytes=df['abytes'] / max(df['launches'], 1),
                    work_per_launch=df['work'] / df['launches'], avg_launch_ms=df['time'] / df['launches'] * 1e3,
                    launches_timed=df['launches'], ms_per_pass=dr['ms_per_pass'], classes=dr['classes'],
                    selection='rocprofv3 symbol family with the largest accumulated time over ALL library launches of a serial meta-step '
                              '(per-layer / per-shape classes of one kernel template are summed: `per_family`; the split by layer and '
                              'direction stays in `per_class`)',
                    timing='HIP events on the launch stream around every library call, serial step after the timed region '
                           '(task lanes, side stream and command-list replay off)',
                    traffic_source='(2 x FETCH_SIZE + WRITE_SIZE) x 1024 bytes per launch, launch-weighted over the family; separate rocprofv3 '
                                   '--pmc passes (profiles/pmc_traffic.json)',
                    arithmetic=arith,
                    serial_step=dict(launches_per_pass=n_launch / passes, gpu_ms_per_pass=sum(c['time'] for c in classes.values()) / passes * 1e3,
                                     gpu_span_ms_per_pass=serial_wall / passes * 1e3),
                    per_family=fam_table, per_class=table)
    if dr['bound'] == 'mfma':
        try:
            roofline['power_limited'] = power_limited_ceiling(dev, dr['achieved'], dr['peak'])
        except Exception as e:                       # a measurement aid must never cost the bench line
            roofline['power_limited'] = dict(error=repr(e))
    return roofline


def physical_cores():
    try:
        import psutil
        return psutil.cpu_count(logical=False) or os.cpu_count() or 8
    except Exception:
        return os.cpu_count() or 8


def self_launch_command(gpus, argv, env):
    """`python bench.py --gpus N` started WITHOUT a launcher (no RANK / WORLD_SIZE in the environment) and N > 1: the command that
    starts the N ranks (one process per GPU, torch.distributed.run on the loopback address, a free rendezvous port), else None.
    Under torchrun (RANK set), with N = 1, or when WORLD_SIZE already says N the script runs as it is."""
    if gpus <= 1 or 'RANK' in env or int(env.get('WORLD_SIZE', '1')) > 1:
        return None
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(gpus), '--master-addr', '127.0.0.1',
            '--master-port', str(port), os.path.abspath(__file__)] + list(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--tasks', type=int, default=8)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--frames', type=int, default=1000)
    ap.add_argument('--labels', type=int, default=100)
    ap.add_argument('--full', action='store_true', help='after the headline: the serial roofline step, the extra legs and the CPU baseline '
                    '(a plain run measures the headline steps only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write what the last timed step computed as DIR/<name>.npy '
                    '(see dump_outputs)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full without the CPU baseline')
    ap.add_argument('--cpu-threads', type=int, default=0)
    ap.add_argument('--no-extras', action='store_true', help='--full without the extra legs: the headline timed region + the serial roofline step')
    ap.add_argument('--dropout', type=float, default=0.0, help='diagnostics: run the headline region and the serial profile with this dropout rate (the extras always report 0.1)')
    ap.add_argument('--lanes', action='store_true', help='per-task pass chains on concurrent lanes instead of task-batched passes (MTL_BATCH_TASKS=0)')
    ap.add_argument('--serial', action='store_true', help='no task lanes / side stream / replay (for rocprofv3 per-kernel durations)')
    ap.add_argument('--host-inputs', action='store_true', help='diagnostics: the headline region with every batch uploaded from pinned host memory per step (what the `with_h2d` leg measures)')
    ap.add_argument('--ragged', action='store_true', help='diagnostics: the headline region on manifest-like batches (every batch padded to its own longest utterance of 0.6 ... 1.0 x --frames, new shapes every step)')
    ap.add_argument('--eval-only', action='store_true', help='only the `eval` leg (validation-loop forward + greedy decoding), for rocprofv3')
    ap.add_argument('--workload', default='asr', choices=['asr', 'lm'], help="'lm': the LSTM-LM meta loop (BASELINE.json configs[4], SURVEY 8(f) f3)")
    a = ap.parse_args()

    cmd = self_launch_command(a.gpus, sys.argv[1:], os.environ)
    if cmd is not None:
        # the ranks inherit stdout: rank 0 prints the ONE line, the others print nothing there (their notes go to stderr)
        import subprocess
        if torch.cuda.is_available() and torch.cuda.device_count() < a.gpus and os.environ.get('MTL_DIST_BACKEND', 'nccl') == 'nccl':
            raise SystemExit('--gpus %d but this node shows %d device(s): RCCL needs one device per rank (MTL_DIST_BACKEND=gloo lets '
                             'ranks share a device for functional tests)' % (a.gpus, torch.cuda.device_count()))
        env = dict(os.environ)
        env.setdefault('OMP_NUM_THREADS', '1')           # (torchrun would set it, with a warning on stderr)
        env['MTL_BENCH_LAUNCHER'] = 'self'
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # (the host driver only supports dmabuf IPC: RCCL across processes needs it)
        raise SystemExit(subprocess.run(cmd, env=env).returncode)

    # stdout carries ONE line, rank 0's JSON: everything else any library writes to file descriptor 1 (gloo's C++ "[Gloo] Rank 0 is
    # connected to ..." at process-group creation, the model factory's prints) is sent to stderr; emit() writes to the saved descriptor
    global _STDOUT_FD
    sys.stdout.flush()
    _STDOUT_FD = os.dup(1)
    os.dup2(2, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        import mtl_amd
    mdist = mtl_amd.dist
    # torch sizes its CPU pool by the machine (128 threads on the GPU node); the container's CFS quota is 16 CPUs, and a 128-thread
    # OpenMP region inside it gets the whole process throttled for 50-100 ms at a time (meta-transfer-learning_amd/hostenv.py)
    HOST['torch_threads_default'] = torch.get_num_threads()
    HOST['torch_threads'] = mtl_amd.hostenv.bound_torch_threads()
    HOST['effective_cpus'] = mtl_amd.hostenv.effective_cpus()
    HOST['cgroup_cpu_quota'] = mtl_amd.hostenv.cgroup_cpu_quota()
    local_rank = mdist.init_from_env()
    world, rank = mdist.world_size(), mdist.rank()
    if world != a.gpus and not (a.gpus == 1 and world == 1):
        raise SystemExit('--gpus %d but WORLD_SIZE %d' % (a.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X: the product path has no CPU fallback')
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)

    if a.workload == 'lm':
        return main_lm(a, mtl_amd, mdist, dev, rank, world)
    args = make_args(a.k)
    vocab = mtl_amd.synthetic_vocab(CFG['vocab_size'])
    torch.manual_seed(123456)
    with contextlib.redirect_stdout(io.StringIO()):
        model = mtl_amd.init_transformer_model(args, vocab, r=CFG['r']).to(dev)
    if a.dropout > 0:
        model.encoder.dropout_rate = model.decoder.dropout_rate = a.dropout
        model.train()
    trainer = mtl_amd.TransientTrainer()
    if a.lanes:
        trainer.batch_tasks = False
    if a.serial:
        model.n_lanes = 1
        trainer.use_cmdlists = False
        trainer.pipeline = False
        for e in model.engines:
            e.use_side_stream = False
    if a.eval_only:
        ev = eval_leg(mtl_amd, trainer, model, vocab, args, a.k, a.frames, a.labels, dev)
        emit(dict(metric='eval utterances/sec (greedy decode)', value=ev['greedy_decode']['utt_per_s'], unit='utt/s', n_gpus=1, data='synthetic', eval=ev))
        return
    inner, outer = mtl_amd.FlatSGD(model, args.lr), mtl_amd.FlatAdam(model, args.meta_lr)
    model.zero_copy_grad()
    tasks = [ResidentTask(mtl_amd, m, a.k, a.frames, a.labels, CFG['vocab_size'], dev) for m in range(a.tasks)]
    if a.ragged:
        tasks = [RaggedTask(m, a.k, int(0.6 * a.frames), a.frames, a.labels, CFG['vocab_size'], dev) for m in range(a.tasks)]
    if a.host_inputs:
        tasks = [PinnedHostTask(mtl_amd, m, a.k, a.frames, a.labels, CFG['vocab_size']) for m in range(a.tasks)]
    my_tasks = mdist.shard_tasks(a.tasks, rank, world)

    # ---- setup: two iterations that allocate the buffer pool and record the command list (what a graph capture is elsewhere), so that
    # the W warm-up steps and the K timed steps run the steady-state schedule whatever W is; reported as config.setup
    # (depth + 2 iterations: the pipelined loop rotates through depth + 1 sets of pinned read-back buffers and resolves its first iteration
    # only once depth + 1 are in flight -- with 2 setup iterations the last set was allocated, and that path first taken, at the 3rd / 4th
    # TIMED step: a 20-180 ms host stall inside the timed region on a freshly started box)
    n_setup = max(2, getattr(trainer, 'pipeline_depth', 1) + 2)
    if not a.serial:
        timed_steps(trainer, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, n_setup, 0, mdist, dev)
    # ---- the headline number: K meta-steps, inputs resident, nothing else inside the timed region
    dt, last = timed_steps(trainer, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, a.steps, a.warmup, mdist, dev)
    host_stats = {k: round(v, 2) for k, v in HOST_ENQUEUE.items()}
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, dict(theta=model.flat_parameters, meta_grad=model._G, last_step=last))

    # (bit-level fingerprint of theta after the timed steps: tests compare schedules / collectives that must not change a single bit)
    th = model.flat_parameters
    theta_ck = [float(th.double().sum()), int(th.view(torch.int32).to(torch.int64).sum())]
    # self-check block, same keys at every N (the first SCALE run must be readable without a debugger, and its N = 1 line comparable
    # with the plain bench line): the rank count the process group reports, the backend ("nccl" = RCCL; "none" = no process group),
    # every rank's own step time, and that the replicas hold the same parameter BITS
    lo = hi = theta_ck[1]
    if world > 1:
        ck = torch.tensor([theta_ck[1]], dtype=torch.int64, device=dev)
        lo_t, hi_t = ck.clone(), ck.clone()
        torch.distributed.all_reduce(lo_t, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi_t, op=torch.distributed.ReduceOp.MAX)
        lo, hi = int(lo_t), int(hi_t)
    multi = dict(ranks=world, collective=mdist.backend_name(), chunked_allreduce=mdist.chunked_on(),
                 allreduce_bytes_per_step=4 * model._layout.total if mdist.collective_on() else 0,
                 tasks_per_rank=[len(mdist.shard_tasks(a.tasks, r, world)) for r in range(world)],
                 per_rank_ms_per_step=PER_RANK.get('ms_per_step') or [round(dt / a.steps * 1e3, 3)], replicas_bit_identical=bool(lo == hi),
                 launcher=os.environ.get('MTL_BENCH_LAUNCHER', 'external' if 'RANK' in os.environ else 'none'))
    # ---- --full: serial profiling step (every rank runs it: it contains the collective; only rank 0 reports)
    if a.full:
        classes, n_launch, serial_wall = serial_profile(mtl_amd, trainer, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, dev)
    out = None
    if rank == 0:
        passes = 2 * max(len(my_tasks), 1)
        ms = dt / a.steps * 1e3
        out = dict(metric='meta-steps/sec', value=a.steps / dt, unit='meta-steps/s', n_gpus=world, steps=a.steps, warmup=a.warmup,
                   ms_per_step=ms, higher_is_better=True, scaling='strong', vs_baseline=None, dtype=DTYPE[model.engine.conv_mode],
                   data='synthetic',
                   config=dict(workload='meta_transfer_train --copy-grad, enc2/dec4 d512 h8 r100 V3765, %d synthetic tasks '
                                        '(%d per GPU), k_train=k_valid=%d, %d frames x 161 bins, %d labels, dropout 0'
                                        % (a.tasks, len(my_tasks), a.k, a.frames, a.labels),
                               setup='%d untimed iterations before the warm-up (buffer pool and read-back buffer allocation, command-list recording)' % n_setup,
                               tasks=a.tasks, k_train=a.k, src_frames=a.frames, tgt_len=a.labels, parallelism='task-sharded dp%d' % world,
                               collective=mdist.backend_name(), ranks=world,
                               inputs='uploaded from pinned host memory inside the timed span (--host-inputs)' if a.host_inputs else 'resident in HBM before the timed region',
                               schedule=('serial, ' if a.serial else '') + (
                                   'the %d local tasks as ONE task-batched pass per phase (training passes at theta0, validation passes at the theta\' stack)'
                                   % len(my_tasks) if (trainer.batch_tasks and len(my_tasks) > 1) else '%d task lanes' % model.n_lanes) + (
                                   '' if a.serial else ' + side stream, command-list replay %s, host up to %d iteration(s) ahead'
                                   % ('on' if trainer.use_cmdlists else 'off', getattr(trainer, 'pipeline_depth', 0))),
                               conv_arithmetic={'h2': '3x3 convolutions on 2-way fp16 splits of power-of-two-scaled fp32 operands (22 '
                                                      'significand bits, 3 fp16 MFMAs per step), fp32 accumulate: error <= 2.5x that of an '
                                                      'fp32 convolution against fp64 (tests/test_ops_gpu.py), parity bar unchanged',
                                                'x3': '3x3 convolutions as exact 3-way bf16 splits of fp32 operands, fp32 accumulate '
                                                      '(fp32-class error, same test tolerances as the fp32-MFMA kernels)',
                                                'f32': 'fp32 MFMA'}[model.engine.conv_mode]),
                   h2_subnormal_frac=h2_frac(trainer), host_enqueue_ms=host_stats, host=dict(HOST), multi_gpu=multi, last_step=dict(val_loss=last[0] / a.tasks, cer_edits=last[1], chars=last[2]), theta_checksum=theta_ck)
        if a.full:
            out['roofline'] = roofline_object(classes, n_launch, serial_wall, passes, model.engine.conv_mode, dev)

    extras = a.full and world == 1 and not a.no_extras

    def run_extras():
        k3 = max(a.steps // 2, 3)
        # the reference's span includes the uploads: same workload, every batch uploaded from pinned host memory per step
        host_tasks = [PinnedHostTask(mtl_amd, m, a.k, a.frames, a.labels, CFG['vocab_size']) for m in range(a.tasks)]
        # (as many timed steps as the headline, after 4 untimed ones: the first iterations allocate the landing sets; with 10 timed steps the
        # leg read 1-2 % low -- same-box alternation of full-length legs: 51.53 / 51.48 ms resident, 51.66 / 51.50 uploaded, 52.52 in-stream)
        dth, _ = timed_steps(trainer, model, vocab, host_tasks, my_tasks, a.tasks, inner, outer, args, a.steps, 4, mdist, dev)
        out['with_h2d'] = dict(value=a.steps / dth, unit='meta-steps/s', ms_per_step=dth / a.steps * 1e3,
                               note='every train / validation batch uploaded from pinned host memory inside the timed span '
                                    '(transient_trainer.py:182-184,210-212)')
        del host_tasks
        # README-faithful configuration (BASELINE.json configs[1]): 3 tasks on one GPU, same run
        if a.tasks >= 3:
            dt3, _ = timed_steps(trainer, model, vocab, tasks[:3], [0, 1, 2], 3, inner, outer, args, k3, 3, mdist, dev)
            out['configs1_3task'] = dict(value=k3 / dt3, unit='meta-steps/s', ms_per_step=dt3 / k3 * 1e3,
                                         note='README-faithful: 3 tasks on one GPU, dropout 0 (parity setting)')
        # manifest-like batches: every task's batch padded to its OWN longest utterance, new frame counts every step (0.6 ... 1.0 of
        # --frames per utterance); the tasks run stacked at the widest in one pass per phase, each with its own border and length
        if a.tasks >= 2:
            rag = [RaggedTask(m, a.k, int(0.6 * a.frames), a.frames, a.labels, CFG['vocab_size'], dev) for m in range(a.tasks)]
            trr = mtl_amd.TransientTrainer()
            dtr, fr, hostr = ragged_steps(trr, model, vocab, rag, a.tasks, inner, outer, args, k3, 6, dev)
            out['ragged_frames'] = dict(value=k3 / dtr, unit='meta-steps/s', ms_per_step=dtr / k3 * 1e3, frames_per_step=fr // k3,
                                        schedule=trr.last_schedule, host_enqueue_ms=round(sum(hostr) / len(hostr), 2),
                                        note='every utterance %d ... %d frames, every batch padded to its own longest (data.py:77): '
                                             'new shapes every step; headline: %d frames per step' % (int(0.6 * a.frames), a.frames,
                                                                                                    2 * a.tasks * a.k * a.frames))
            del rag, trr
        # what ONE rank of the 8-GPU configuration runs per step: a single task, a single lane (no collective on one rank)
        tr1 = mtl_amd.TransientTrainer()
        dt1, _ = timed_steps(tr1, model, vocab, tasks[:1], [0], a.tasks, inner, outer, args, 2 * k3, 4, mdist, dev)
        out['one_task_per_gpu'] = dict(ms_per_step=dt1 / (2 * k3) * 1e3, schedule=tr1.last_schedule,
                                       note='1 of %d tasks on this GPU (configs[2] per-rank work, without the all-reduce): the two '
                                            'passes as one chain + side stream, one recorded command list' % a.tasks)
        del tr1
        # ... and what one rank of the 2- and 4-GPU configurations runs (4 / 2 of the 8 tasks, global n = 8, no collective): with the
        # headline (8 local tasks) and the one-task leg, the per-rank work of every N of the scaling curve, measured on ONE device
        per_rank = {str(a.tasks): ms, '1': out['one_task_per_gpu']['ms_per_step']}
        for local in (4, 2):
            if a.tasks % local == 0 and a.tasks > local:
                trl = mtl_amd.TransientTrainer()
                dtl, _ = timed_steps(trl, model, vocab, tasks[:local], list(range(local)), a.tasks, inner, outer, args, k3, 4, mdist, dev)
                per_rank[str(local)] = dtl / k3 * 1e3
                del trl
        out['per_rank_work_ms'] = dict(local_tasks=per_rank, note='step time of ONE rank holding this many of the %d tasks (global n = %d, no '
                                       'all-reduce): the compute side of the 1 / 2 / 4 / 8-GPU points; not a scaling measurement' % (a.tasks, a.tasks))
        # what the h2 guard costs: the same steps with the census taken on EVERY iteration (it is taken on one in `h2_check_every`)
        trc = mtl_amd.TransientTrainer()
        trc.h2_check_every = 1
        dtc, _ = timed_steps(trc, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, k3, 4, mdist, dev)
        if out.get('h2_subnormal_frac'):
            extra = dtc / k3 * 1e3 - ms
            out['h2_subnormal_frac'].update(census_step_extra_ms=extra, amortised_cost=max(extra, 0.0) / ms / max(trainer.h2_check_every, 1),
                                            per_operand={k_: dict(lt22_bits=v[0], lt16_bits=v[1]) for k_, v in (trc.h2_census or {}).items()})
        del trc
        # f2: the validation loop's forward and test-time greedy decoding at this model (after the training legs: own buffers)
        try:
            out['eval'] = eval_leg(mtl_amd, trainer, model, vocab, args, a.k, a.frames, a.labels, dev)
        except Exception as e:                           # a side leg must never cost the bench line
            out['eval'] = dict(error=repr(e))
        # the README trains with --dropout 0.1: same 8-task workload with the Philox dropout active
        model.encoder.dropout_rate = model.decoder.dropout_rate = 0.1
        model.train()
        dtd, _ = timed_steps(trainer, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, k3, 5, mdist, dev)     # (new buffers, eager + recording + replay: 5 untimed)
        out['dropout_0.1'] = dict(value=k3 / dtd, unit='meta-steps/s', ms_per_step=dtd / k3 * 1e3, tasks=a.tasks)
        model.encoder.dropout_rate = model.decoder.dropout_rate = 0.0
        model.train()
        # the same workload with EVERY product on the exact-fp32 matrix instructions (convolutions: v_mfma_f32_32x32x2_f32, no fp16 /
        # bf16 pieces anywhere): what the split arithmetic of the headline buys
        lib = mtl_amd._lib.lib()
        saved = [(e, e.conv_mode, e.conv_x3, e.conv_h2, e.in_linear) for e in model.engines]
        old_x3 = lib.mtl_gemm_x3_min_tiles(0)
        for e in model.engines:
            e.conv_mode, e.conv_x3, e.conv_h2, e.in_linear = 'f32', False, False, 'f32'
        tr32 = mtl_amd.TransientTrainer()              # (its own command lists: the recorded ones hold the h2 entry points)
        dtf, _ = timed_steps(tr32, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, k3, 4, mdist, dev)
        out['exact_f32'] = dict(value=k3 / dtf, unit='meta-steps/s', ms_per_step=dtf / k3 * 1e3,
                                note='same steps with every convolution and product on the fp32 MFMA (MTL_CONV=f32, bf16-split GEMM '
                                     'engine off, input Linear on the fp32 engine)')
        for e, cm, cx, ch, il in saved:
            e.conv_mode, e.conv_x3, e.conv_h2, e.in_linear = cm, cx, ch, il
        lib.mtl_gemm_x3_min_tiles(old_x3)
        # ... and the middle point: the convolutions on the EXACT 3-piece bf16 split (MTL_CONV=x3: every fp32 operand bit kept, six MFMAs
        # per step; the input Linear then runs on the x3 GEMM engine too) -- no two-piece fp16 operand anywhere in the step
        for e in model.engines:
            e.conv_mode, e.conv_x3, e.conv_h2 = 'x3', True, False
        trx3 = mtl_amd.TransientTrainer()
        dtx, _ = timed_steps(trx3, model, vocab, tasks, my_tasks, a.tasks, inner, outer, args, k3, 4, mdist, dev)
        out['conv_x3'] = dict(value=k3 / dtx, unit='meta-steps/s', ms_per_step=dtx / k3 * 1e3,
                              note='same steps with MTL_CONV=x3: 3x3 convolutions and the input Linear on exact 3 x bf16 splits (24 significand '
                                   'bits, 6 MFMAs per step) instead of 2 x fp16 (22 bits, 3 MFMAs); everything else as in the headline')
        for e, cm, cx, ch, il in saved:
            e.conv_mode, e.conv_x3, e.conv_h2, e.in_linear = cm, cx, ch, il
    if extras:
        try:
            run_extras()
        except Exception as e:                           # a side leg must never cost the headline (round 4 lost its measurement to the line's format)
            import traceback
            out['extras_error'] = repr(e)
            print('bench extras failed:\n' + traceback.format_exc(), file=sys.stderr, flush=True)
    if a.full and world == 1 and not a.no_cpu_baseline:
        # torch's CPU kernels do not scale to every core of a large host (measured on the 128-core GPU node: 11.1 s per task at
        # 128 threads, 3.9 s at 32, 4.2 s at 8), so the baseline is timed at the physical core count, at 32 and at 8 threads
        # (SURVEY's 8-core figure) and the FASTEST is reported as `value`, with its thread count in `cores`
        # (thread counts: the CPUs this container may actually use -- min(physical cores, CFS quota) -- and 8, SURVEY's figure; round 4
        # timed 128 threads under a 16-CPU quota, which only measured the throttling)
        phys = min(physical_cores(), HOST.get('effective_cpus') or physical_cores())
        counts = [a.cpu_threads] if a.cpu_threads else sorted({phys, min(32, phys), min(8, phys)}, reverse=True)
        runs = {n: cpu_baseline(a.tasks, a.k, a.frames, a.labels, n, timed_tasks=2)       # two full tasks per thread count
                for n in counts}
        best = max(runs, key=lambda n: runs[n]['value'])
        out['cpu_baseline'] = dict(runs[best])
        out['cpu_baseline']['host'] = dict(physical_cores=physical_cores(), logical_cpus=os.cpu_count(), usable_cpus=phys,
                                           cgroup_cpu_quota=HOST.get('cgroup_cpu_quota'))
        mtl_amd.hostenv.bound_torch_threads()
        out['cpu_baseline']['by_threads'] = {str(n): dict(value=r['value'], seconds_per_task=r['seconds_per_task'], sample=r['sample'])
                                             for n, r in runs.items()}
    if rank == 0:
        emit(out)
    mdist.barrier()


_STDOUT_FD = None       # main(): the process's real stdout (fd 1 itself is pointed at stderr for the run)
LINE_LIMIT = 4096        # bytes: the driver parses the LAST stdout line; round 4's 20 KB line came back as parsed = null


def _r(v, nd=4):
    return round(v, nd) if isinstance(v, float) else v


def compact_line(out):
    """The ONE stdout line (< LINE_LIMIT bytes): the contract's keys, the `roofline` and `cpu_baseline` objects without their
    tables, the extra legs as bare numbers.  Everything else (per_class / per_family tables, notes, by-thread CPU runs) goes to
    gpurun_out/bench_detail.json and stderr."""
    line = {k: _r(out[k]) for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                                    'vs_baseline', 'dtype', 'data') if k in out}
    cfg = out.get('config', {})
    line['config'] = {k: cfg[k] for k in ('workload', 'tasks', 'k_train', 'src_frames', 'tgt_len', 'parallelism', 'collective', 'ranks',
                                          'inputs', 'schedule', 'bptt', 'batch_size', 'nhid', 'ntoken') if k in cfg}
    rf = out.get('roofline')
    if rf:
        line['roofline'] = {k: _r(rf[k]) for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'algorithmic_bytes',
                                                   'avg_launch_ms', 'work_per_launch', 'launches_timed', 'ms_per_pass') if k in rf}
        pl = rf.get('power_limited') or {}
        if 'frac_of_sustained' in pl:
            line['roofline']['frac_of_sustained'] = _r(pl['frac_of_sustained'])
    cb = out.get('cpu_baseline')
    if cb:
        line['cpu_baseline'] = {k: _r(cb[k]) for k in ('value', 'unit', 'cores', 'kind', 'sample', 'seconds_per_task') if k in cb}
    hf = out.get('h2_subnormal_frac')
    if hf:
        line['h2_subnormal_frac'] = {k: (float('%.3g' % hf[k]) if isinstance(hf[k], float) else hf[k])
                                     for k in ('lt22_bits', 'lt16_bits', 'amortised_cost') if k in hf}
    if 'host_enqueue_ms' in out:
        line['host_enqueue_ms'] = out['host_enqueue_ms']
    if 'host' in out:
        line['host'] = out['host']
    for k in ('with_h2d', 'configs1_3task', 'ragged_frames', 'dropout_0.1', 'conv_x3', 'exact_f32'):
        if k in out:
            line[k] = _r(out[k]['value'], 3)
    if 'one_task_per_gpu' in out:
        line['one_task_per_gpu_ms'] = _r(out['one_task_per_gpu']['ms_per_step'], 3)
    if 'per_rank_work_ms' in out:
        line['per_rank_work_ms'] = {k_: _r(v_, 2) for k_, v_ in out['per_rank_work_ms']['local_tasks'].items()}
    ev = out.get('eval') or {}
    if 'greedy_decode' in ev:
        line['eval_utt_per_s'] = _r(ev['greedy_decode']['utt_per_s'], 2)
        line['valid_loop_utt_per_s'] = _r(ev['valid_loop']['utt_per_s'], 1)
    if 'beam_search' in ev:
        line['beam_utt_per_s'] = _r(ev['beam_search']['utt_per_s'], 2)
    for k in ('multi_gpu', 'last_step', 'theta_checksum', 'extras_error', 'detail'):
        if k in out:
            line[k] = out[k]
    return line


def emit(out):
    detail_path = os.path.join(ROOT, 'gpurun_out', 'bench_detail.json')
    try:
        os.makedirs(os.path.dirname(detail_path), exist_ok=True)
        with open(detail_path, 'w') as f:
            json.dump(out, f, indent=1)
        out['detail'] = 'gpurun_out/bench_detail.json (per_class / per_family tables, notes; also on stderr)'
    except OSError:
        out['detail'] = 'stderr'
    print('bench detail: ' + json.dumps(out), file=sys.stderr, flush=True)
    text = json.dumps(compact_line(out))
    if len(text) >= LINE_LIMIT:                       # never let a long note cost the line again: drop the free-text fields
        line = compact_line(out)
        line['config'] = {k: v for k, v in line['config'].items() if not isinstance(v, str) or len(v) < 80}
        line.get('cpu_baseline', {}).pop('sample', None)
        text = json.dumps(line)
    if _STDOUT_FD is not None:
        sys.stdout.flush()
        os.write(_STDOUT_FD, (text + '\n').encode())
    else:
        print(text, flush=True)


if __name__ == '__main__':
    main()
