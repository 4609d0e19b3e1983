"""`TransientTrainer`: drop-in for trainer/asr/transient_trainer.py (the `--copy-grad` meta-transfer loop).

Same `train(...)` / `forward_one_batch(...)` signatures, log lines and meta-gradient definition
    G = sum_m [ grad L_tr,m(theta0) + (1/n) grad L_val(theta0 - alpha grad L_tr,m(theta0)) ]      
but the iteration is restructured for the device:
  * theta0 is never mutated inside an iteration (theta' is materialised by one fused kernel into a second flat
    buffer), which removes deepcopy(state_dict) / n x load_state_dict (transient_trainer.py:155-160,237);
  * gradients, copy_grad, Adam moments are single flat fp32 buffers updated by one kernel each;
  * label/loss read-backs are asynchronous copies resolved once per iteration instead of ~1600 `int(x)` device
    syncs per forward (transient_trainer.py:29-35,46);
  * with torch.distributed initialised, tasks are sharded round-robin over ranks and the flat G is summed with ONE
    all-reduce (RCCL over xGMI) before the (replicated, deterministic) Adam step.
"""
import logging
import os
import threading
import time
from collections import deque

import torch

from . import _lib, _trace, dist as mdist, hostenv, metastep
from .metastep import PendingIteration, _Readback, _pinned
from .discriminator import calculate_adversarial, calculate_multi_task, save_discriminator
from .functions import post_process, save_joint_model, save_meta_model
from .metrics import calculate_cer, calculate_metrics

check = _lib.check


class FlatAdam:
    """torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) over the model's flat parameter buffer."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8):
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.m = torch.zeros_like(model.flat_parameters)
        self.v = torch.zeros_like(model.flat_parameters)
        self.step_count = 0
        self.param_groups = [{'lr': lr, 'betas': betas, 'eps': eps}]

    @classmethod
    def from_torch(cls, model, opt):
        """Import the state of a torch.optim.Adam built over model.parameters() (reference checkpoints pickle those)."""
        g = opt.param_groups[0]
        self = cls(model, g['lr'], tuple(g['betas']), g['eps'])
        lay = model._layout
        for name, p in zip(lay.order, opt.param_groups[0]['params']):
            st = opt.state.get(p, None)
            if st:
                lay.view(self.m, name).copy_(st['exp_avg'])
                lay.view(self.v, name).copy_(st['exp_avg_sq'])
                self.step_count = int(st['step'])
        return self

    def to_torch(self):
        opt = torch.optim.Adam(self.model.parameters(), lr=self.param_groups[0]['lr'], betas=self.betas, eps=self.eps)
        if self.step_count:
            lay = self.model._layout
            for name, p in zip(lay.order, self.model.parameters()):
                opt.state[p] = {'step': torch.tensor(float(self.step_count)), 'exp_avg': lay.view(self.m, name).clone(),
                                'exp_avg_sq': lay.view(self.v, name).clone()}
        return opt

    def zero_grad(self):
        self.model.zero_grad()

    def step(self, grad=None):
        m = self.model
        g = m.flat_grad if grad is None else grad
        self.step_count += 1
        th = m.flat_parameters
        check(_lib.lib().mtl_adam_step(torch.cuda.current_stream(th.device).cuda_stream, th.data_ptr(), g.data_ptr(),
                                       self.m.data_ptr(), self.v.data_ptr(), self.step_count, float(self.param_groups[0]['lr']),
                                       self.betas[0], self.betas[1], self.eps, th.numel()), 'mtl_adam_step')


class FlatSGD:
    """torch.optim.SGD(lr) (no momentum / weight decay) as theta' = theta0 - lr*g into a separate buffer."""

    def __init__(self, model, lr):
        self.model = model
        self.param_groups = [{'lr': lr}]
        self.theta_prime = torch.empty_like(model.flat_parameters)

    @classmethod
    def from_torch(cls, model, opt):
        return cls(model, opt.param_groups[0]['lr'])

    def to_torch(self):
        return torch.optim.SGD(self.model.parameters(), lr=self.param_groups[0]['lr'])

    def zero_grad(self):
        self.model.zero_grad()

    def theta_prime_from(self, theta0, grad, out=None):
        out = self.theta_prime if out is None else out
        check(_lib.lib().mtl_sgd_theta_prime(torch.cuda.current_stream(theta0.device).cuda_stream, theta0.data_ptr(),
                                             grad.data_ptr(), float(self.param_groups[0]['lr']), out.data_ptr(),
                                             theta0.numel()), 'mtl_sgd_theta_prime')
        return out


def clip_flat_grad_(model, grad, max_norm, lane=0):
    """torch.nn.utils.clip_grad_norm_ on the flat buffer: grad *= min(1, max_norm / (||grad|| + 1e-6)), no host sync."""
    model._need_engine()
    eng = model.engines[lane]
    ws = eng.scratch(8192)
    coef = eng.buf('_clip_coef', (1,))
    st = eng.stream
    check(eng.lib.mtl_sumsq(st, grad.data_ptr(), grad.numel(), coef.data_ptr(), ws, 2, float(max_norm)), 'mtl_sumsq')
    check(eng.lib.mtl_scale(st, grad.data_ptr(), 1.0, coef.data_ptr(), grad.numel()), 'mtl_scale')


def _strings(vocab, rows):
    return [''.join(vocab.id2label[int(t)] for t in row) for row in rows.tolist()]


def cer_counts(vocab, gold, hyp):
    """total edit distance / reference length over a batch, exactly as transient_trainer.py:29-35,52-64."""
    total_cer, total_char = 0, 0
    for g, h in zip(_strings(vocab, gold), _strings(vocab, hyp)):
        h = post_process(h, vocab.special_token_list).replace(' ', '')
        g = post_process(g, vocab.special_token_list).replace(' ', '')
        total_cer += calculate_cer(h, g)
        total_char += len(g)
    return total_cer, total_char


def sync_replicas_from_rank0(model, opts, discriminator=None):
    """Multi-rank start-up: broadcast theta and every optimizer's state (Adam m, v, step count) from rank 0, so that replicas are
    bit-identical whatever each rank's RNG / checkpoint state was.  From then on they stay identical by construction (same G
    after the all-reduce, deterministic Adam kernel); check_replicas() verifies that periodically.
    discriminator: its flat parameters join; a torch.optim optimizer among `opts` (opt_disc) sends whatever state tensors it holds
    (none when it was built for this train() call, on every rank alike)."""
    if mdist.world_size() <= 1:
        return
    import torch.distributed as td
    td.broadcast(model.flat_parameters, src=0)
    if discriminator is not None:
        td.broadcast(discriminator.flat_parameters, src=0)
    for opt in opts:
        if isinstance(opt, torch.optim.Optimizer):
            for group in opt.param_groups:
                for p in group['params']:
                    for k in sorted(k for k, v in opt.state.get(p, {}).items() if torch.is_tensor(v)):
                        v = opt.state[p][k].to(model.flat_parameters.device)
                        td.broadcast(v, src=0)
                        opt.state[p][k].copy_(v)
        if isinstance(opt, FlatAdam):
            td.broadcast(opt.m, src=0)
            td.broadcast(opt.v, src=0)
            step = torch.tensor([opt.step_count], dtype=torch.int64, device=model.flat_parameters.device)
            td.broadcast(step, src=0)
            opt.step_count = int(step.item())


def check_replicas(model, val_batch, it):
    """Cheap divergence check (two small all-reduces: float checksums of theta and the validation batch, bit-level integer
    checksums of theta): every rank must hold the same theta and must have drawn the same
    shared validation batch (ManifestTaskDataset(seed=...) / the seeding contract in INTEGRATION.md).  Raises on a mismatch
    instead of letting the all-reduced meta-gradient silently mix gradients taken at different parameters."""
    if mdist.world_size() <= 1:
        return
    import torch.distributed as td
    th = model.flat_parameters
    vx = val_batch[0]
    probe = torch.stack([th.double().sum(), th[::997].double().abs().sum(),
                         vx.to(th.device, non_blocking=True).double().sum() + float(val_batch[3].sum())])
    if not bool(torch.isfinite(probe).all()):
        # (MIN / MAX never compare equal on NaN: without this check a numerical blow-up would be reported as a seeding problem)
        raise RuntimeError('iteration %d: non-finite parameters or validation batch on rank %d (checksums %s): the run diverged '
                           'numerically, this is not a replica mismatch' % (it + 1, mdist.rank(), probe.tolist()))
    # float checksums: MAX of [p, -p] gives max and -min with one all-reduce
    t = torch.cat([probe, -probe])
    td.all_reduce(t, op=td.ReduceOp.MAX)
    hi, lo = t[:3], -t[3:]
    # bit-level checksums of theta (a localised or sign-cancelling divergence does not survive these): integer column sums of the
    # raw 32-bit words, plain and position-weighted (wrap-around int64 arithmetic is deterministic)
    bits = th.view(torch.int32)
    n = bits.numel() // 4096 * 4096
    cols = bits[:n].view(-1, 4096).sum(0, dtype=torch.int64)
    tail = bits[n:].sum(dtype=torch.int64)
    chk = torch.stack([cols.sum() + tail, (cols * torch.arange(1, 4097, dtype=torch.int64, device=th.device)).sum() + 7 * tail])
    u = torch.cat([chk, -chk])
    td.all_reduce(u, op=td.ReduceOp.MAX)
    if not torch.equal(lo, hi) or not torch.equal(u[:2], -u[2:]):
        raise RuntimeError('iteration %d: replicas diverged (theta / validation-batch checksums differ across ranks: %s vs %s, '
                           'parameter bit checksums %s vs %s); seed every rank identically (see INTEGRATION.md)'
                           % (it + 1, lo.tolist(), hi.tolist(), (-u[2:]).tolist(), u[:2].tolist()))


def run_validation(forward_one_batch, model, vocab, valid_loader_list, it, args, history, loss_type, save_fn, criteria, stop_val,
                   best, count_stop, rank):
    """The in-loop validation of both trainers (transient_trainer.py:280-360, joint_trainer.py:306-380): eval mode, no autograd,
    `forward_one_batch` over every batch of every loader (AudioDataLoader layout: src, trg, percentages, src_lengths,
    trg_lengths), per-loader loss = mean over batches, CER = edits*100/chars, metrics dict + history, save every
    args.save_every iterations, best-model save and early-stop counter on the chosen criterion.
    save_fn(metrics, best_model) writes a checkpoint (rank 0 only).  -> (stop, best, count_stop)"""
    say = print if rank == 0 else (lambda *a, **k: None)
    say('')
    logging.info('VALID')
    smoothing = float(getattr(args, 'label_smoothing', 0.0) or 0.0)
    dev = model.flat_parameters.device
    model.eval()
    final_losses, final_cers = [], []
    engines = getattr(model, 'engines', [])
    try:
        for e in engines:
            e.forward_only = True                   # PassEngine.forward_only: no backward follows these passes
        with torch.no_grad():
            for ind, loader in enumerate(valid_loader_list):
                tot_loss, tot_cer, tot_char, nb = 0.0, 0, 0, 0
                for data in loader:
                    src, trg, pct, src_lengths, trg_lengths = data
                    if getattr(args, 'cuda', True):
                        src, trg = src.to(dev), trg.to(dev)
                    loss, cer, nchar = forward_one_batch(model, vocab, src, trg, pct, src_lengths, trg_lengths, smoothing, loss_type)
                    tot_cer += cer
                    tot_char += nchar
                    tot_loss += loss.item()
                    nb += 1
                final_losses.append(tot_loss / max(nb, 1))
                final_cers.append(tot_cer * 100 / max(tot_char, 1))
                msg = '(Iteration {}) VALID SET {} LOSS:{:.4f} CER:{:.2f}%'.format((it + 1), ind, final_losses[-1], final_cers[-1])
                say(msg)
                logging.info(msg)
    finally:
        for e in engines:
            e.forward_only = False
        model.train()
    if not final_losses:
        return False, best, count_stop
    metrics = {'avg_valid_loss': sum(final_losses) / len(final_losses), 'avg_valid_cer': sum(final_cers) / len(final_cers),
               'valid_loss': final_losses, 'valid_cer': final_cers, 'history': history}
    history.append(metrics)
    msg = '(Iteration {}) AVG VALID LOSS:{:.4f} AVG CER:{:.2f}%'.format((it + 1), metrics['avg_valid_loss'], metrics['avg_valid_cer'])
    say(msg)
    logging.info(msg)
    if rank == 0 and (it + 1) % args.save_every == 0:
        save_fn(metrics, False)
    cur = metrics['avg_valid_cer'] if criteria == 'cer' else metrics['avg_valid_loss']
    say('CRITERIA: CER' if criteria == 'cer' else 'CRITERIA: LOSS')
    if best > cur:
        count_stop, best = 0, cur
        if rank == 0:
            save_fn(metrics, True)
    else:
        count_stop += 1
        say('count_stop:', count_stop)
    if count_stop >= stop_val:
        logging.info('EARLY STOP')
        say('EARLY STOP\n')
        return True, best, count_stop
    return False, best, count_stop


MAX_CONSECUTIVE_FAILURES = 20


def _sample_takes_need(ds):
    """Does ds.sample accept the `need=` keyword (this package's datasets: load only what the rank uses)?  Read from the
    signature: catching TypeError around the call would also swallow errors raised INSIDE sample() -- after the index stream
    has advanced -- and the retry would draw a second time, taking this rank out of lock-step with the others."""
    import inspect
    try:
        params = inspect.signature(ds.sample).parameters
    except (TypeError, ValueError):
        return False
    return 'need' in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _check_loss_type(loss_type):
    if loss_type not in ('ce', 'ctc'):
        raise NotImplementedError("loss_type must be 'ce' or 'ctc'")


class TransientTrainer():
    def __init__(self):
        logging.info('Transient Trainer is initialized')
        # Runtime switches read from the environment (INTEGRATION.md "Environment"): MTL_BATCH_TASKS, MTL_RAGGED_FILL,
        # MTL_RAGGED_QUANTUM, MTL_PIPELINE_DEPTH.  Everything else below is a plain attribute (tests and bench.py set them).
        # command lists: the library calls of a task body are recorded once per (lane, shapes, scalars) and then replayed from C with
        # one ctypes call per task (include/mtl_hip.h "command lists"): host cost per pass 4.4 -> ~1 ms
        # (the one eager / recorded / replayed rule of _lib.Replay, least recently used key out at 64: variable-length data brings keys
        # that rarely repeat).  The switch stays in front of it: off, or an engine with a profiler / forward hook, means plain calls.
        self.use_cmdlists = True
        self.replay = _lib.Replay(64, lru=True)
        # the local tasks of a meta-step as ONE task-batched pass per phase (training passes at theta0, validation passes at the
        # theta' stack) instead of one pass chain per task on concurrent lanes; MTL_BATCH_TASKS=0: the lanes
        self.batch_tasks = os.environ.get('MTL_BATCH_TASKS', '1') != '0'
        # tasks whose batches have different frame counts in one pass, stacked at the widest (False: one lane per task), as long as the
        # tasks' frames fill at least this share of the stack
        self.batch_ragged = True
        self.ragged_fill = float(os.environ.get('MTL_RAGGED_FILL', '0.4'))
        # ... and the stack's width (training and validation) rounded up to a multiple of this many frames: any width at or above the
        # widest task is exact (every task keeps its own border), and widths that repeat keep the buffer pool's allocations -- 11 GB
        # per width at the north-star size, otherwise re-allocated for every new widest utterance -- and the recorded command lists
        self.ragged_quantum = int(os.environ.get('MTL_RAGGED_QUANTUM', '64'))
        # the same rounding for a task that runs on a lane of its own (one task per rank; tasks too unequal to stack): 'auto' = from the
        # moment the lanes have seen two different widths (fixed-shape workloads are never padded), '1' always, '0' never
        self.pad_lanes = 'auto'
        self.label_quantum = 8      # ... and the decoder width to a multiple of this many positions
        self._lane_widths, self._lane_widths_vary = {}, False
        # train() enqueues iteration i + 1 before it resolves (logs) iteration i (enqueue_iteration).  MTL_PIPELINE_DEPTH: how many
        # iterations may be enqueued beyond the one being resolved (nothing the host needs to enqueue an iteration comes from the
        # device): 0 resolves at once, 1 hides the host's per-iteration work, 2 (default) also rides out host stalls of up to one
        # iteration's GPU time (shared hosts: measured enqueue times of 5 - 90 ms for the same iteration).  Read-back buffer sets:
        # depth + 1.
        self.pipeline_depth = max(0, int(os.environ.get('MTL_PIPELINE_DEPTH', '2')))
        self.pipeline = self.pipeline_depth > 0
        # batches handed over in host memory are uploaded on a separate stream, one iteration ahead of the kernels (task-batched passes)
        self.overlap_uploads = True
        self.pin_batches = True             # train(): batches drawn on the host are page-locked by the prefetch thread
        self.replica_check_every = 100      # several ranks: iterations between two bit-level divergence checks of the replicas
        # Guard of the two-piece fp16 ("h2") convolution arithmetic (csrc/mtl_h2.h: ONE power-of-two scale per tensor, so an element more
        # than ~2^17.5 below its tensor's maximum keeps fewer than 22 significand bits).  The reference's features are normalised per
        # utterance (utils/data_loader.py:84-94), which keeps every operand of the path in the full-precision regime -- this checks it
        # instead of assuming it: every `h2_check_every` iterations (the first included) the iteration also counts, for every h2 operand
        # of every pass (activations forward, gradients backward), the non-zero elements that keep fewer than 22 / fewer than 16 bits
        # (mtl_h2_census; ~5 % on that one iteration).  `h2_census` holds the latest fractions; when the share below 16 bits of any
        # operand exceeds `h2_limit`, `h2_guard` acts: 'x3' (default) moves the convolutions to the exact 3 x bf16 split for the rest of
        # the run, 'raise' stops, 'warn' only reports.  0 = never sample.
        self.h2_check_every, self.h2_limit, self.h2_guard = 100, 1e-3, 'x3'
        self.h2_census, self._h2_iter, self._h2_buf, self._census_on = None, 0, None, None
        self._turn = 0
        # state of the schedules (metastep.py): which one the last iteration took (diagnostics / tests); the (nt, P) gradient / theta'
        # stacks and the lanes' buffers with what they were sized for; the landing set and stream of the overlapped uploads; the
        # communication stream and collectives in flight of the chunked all-reduce, and whether they left model._G already reduced
        self.last_schedule = None
        self._stack_key, self._lane_key = None, None
        self._xset, self._upload_stream = 0, None
        self._comm_stream, self._chunks, self._G_reduced = None, None, False
        # the training objective of meta_iteration: 'ce', or 'ctc' (--loss ctc: the CTC loss of each batch's percentages and target
        # sizes, utils/metrics.py:127-148).  train() sets it from its loss_type; part of every command-list key.
        self.loss_type = 'ce'

    # ------------------------------------------------------------------ drop-in single-batch API
    def forward_one_batch(self, model, vocab, src, trg, src_percentages, src_lengths, trg_lengths, smoothing, loss_type,
                          verbose=False):
        """-> (loss tensor, total_cer, total_char); `loss.backward()` runs the HIP backward (transient_trainer.py:25-73).
        Same steps as the reference: model forward, calculate_metrics (label smoothing included), CER of the post-processed
        strings; the ~2*B*T per-element `int(x)` device syncs become one D2H copy of gold / hyp.
        loss_type 'ctc': the CTC loss of `sizes` decoder positions and `trg_lengths` labels per utterance (:38-41); a batch with an
        utterance that has no alignment returns +inf, as the reference does ("Found infinity loss")."""
        _check_loss_type(loss_type)
        pred, gold, hyp = model(src, src_lengths, trg, verbose=False)
        sizes = src_percentages.mul_(int(pred.size(1))).int()     # the reference scales the caller's tensor in place
        loss, _ = calculate_metrics(pred, gold, vocab.PAD_ID, input_lengths=sizes, target_lengths=trg_lengths,
                                    smoothing=smoothing, loss_type=loss_type)
        total_cer, total_char = cer_counts(vocab, gold.cpu(), hyp.cpu())
        if verbose:
            print('Total CER', total_cer)
            print('Total char', total_char)
        return loss, total_cer, total_char

    def get_lr(self, optimizer):
        for param_group in optimizer.param_groups:
            return param_group['lr']

    @property
    def _cmdlists(self):
        """Read-only view of `replay` in the form the trainer's own table had, for code that still reads it:
        {key: 'warm' (seen, nothing recorded yet) | dict(cl=the recorded CommandList)}, oldest key first."""
        return {key: dict(cl=lists[0]) if lists else 'warm' for key in self.replay.keys() for lists in [self.replay.recorded(key)]}

    # ------------------------------------------------------------------ one meta-iteration on the device: metastep.py, bound as methods
    meta_iteration = metastep.meta_iteration
    _can_batch, _widths_vary, _turns = metastep._can_batch, metastep._widths_vary, metastep._turns
    _chunk_hook, _chunk_join = metastep._chunk_hook, metastep._chunk_join
    _census_begin, _census_report = metastep._census_begin, metastep._census_report

    def enqueue_iteration(self, model, vocab, task_batches, val_data, n_tasks, inner_opt, outer_opt, args):
        """Enqueues one meta-iteration (transient_trainer.py:152-264: local tasks, ONE all-reduce of G, Adam) WITHOUT waiting for
        it and returns a PendingIteration whose result() resolves the loss / label read-backs.  Nothing the host needs to enqueue
        iteration i + 1 comes from the device, so train() (and bench.py) enqueue it before resolving iteration i: the host's
        per-iteration work (batch preparation, CER strings, logging: 1.3 - 2.9 ms, all of it GPU idle time when a rank holds a
        single 12 ms task) runs under the next iteration's kernels.  Read-back buffers rotate through pipeline_depth + 1 sets (`_turn`)."""
        dev = model.flat_parameters.device
        t_host = time.perf_counter()
        _trace.begin()
        self._turn = (self._turn + 1) % self._turns()
        outer_opt.zero_grad()
        _trace.mark('zero_grad')
        self._G_reduced = False
        census = self._census_begin(model, len(task_batches))
        try:
            reads = self.meta_iteration(model, vocab, task_batches, val_data, n_tasks, inner_opt, outer_opt, args)
        finally:
            self._census_on = None
            for e in model.engines:
                e.census = None
        _trace.mark('meta_iteration_rest')
        G = model._G
        if not self._G_reduced:                                  # (already summed over the ranks group by group, under the backward: _chunk_hook)
            self.reduce_meta_gradient(model)
        if args.clip:
            clip_flat_grad_(model, G, args.max_norm)             # (:253-254) on the summed meta-gradient
        outer_opt.step(G)                                        # from_copy_grad() + outer_opt.step()  (:248-255)
        _trace.mark('allreduce_adam')
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        _trace.mark('done_event')
        _trace.end()
        pend = None
        if census is not None:
            host = _pinned(('h2census', self._turn), census.shape, torch.int64, self._turns())
            host.copy_(census, non_blocking=True)
            done.record(torch.cuda.current_stream(dev))
            pend = (host, lambda counters, model=model: self._census_report(model, counters))
        self.host_enqueue_s = time.perf_counter() - t_host       # host side of the iteration (diagnostics: bench.py reports it)
        return PendingIteration(reads, done, vocab, dev, census=pend)

    def reduce_meta_gradient(self, model):
        """The collective of the path for an iteration whose backward did not hand G's groups over as it went (several differently
        shaped local tasks on lanes, no local task at all, chunking switched off).  Which schedule a rank takes depends
        on ITS data, so the sequence of collectives must not: with chunking on, every rank always posts the same three all-reduces
        (decoder, encoder, conv slices, the order _chunk_hook uses) -- here back to back on the current stream; with
        MTL_CHUNKED_ALLREDUCE=0 every rank posts the single all-reduce of the whole flat buffer."""
        G = model._G
        if mdist.chunked_on():
            bounds = model._layout.group_bounds()
            for tag in (t for t in mdist.SLICE_ORDER if t in bounds):      # (no 'conv' group in a model without convolutions)
                lo, hi = bounds[tag]
                mdist.allreduce_sum_(G[lo:hi])
        else:
            mdist.allreduce_sum_(G)
        self._G_reduced = True

    def run_iteration(self, model, vocab, task_batches, val_data, n_tasks, inner_opt, outer_opt, args):
        """The timed body of one meta-iteration, resolved: -> (sum val loss, CER edits, chars), global."""
        return self.enqueue_iteration(model, vocab, task_batches, val_data, n_tasks, inner_opt, outer_opt, args).result()

    def train(self, model, vocab, train_data_list, valid_loader_list, loss_type, start_it, num_it, args, inner_opt=None,
              outer_opt=None, evaluate_every=1000, window_size=100, last_summary_every=1000, last_metrics=None, early_stop=10,
              cpu_state_dict=False, is_copy_grad=False):
        _check_loss_type(loss_type)
        self.loss_type = loss_type                # what meta_iteration trains on; the validation loop gets it as an argument
        if not is_copy_grad:
            raise NotImplementedError('the accelerated path is the --copy-grad loop (is_copy_grad=True)')
        history = []
        best_valid_val = 1000000000
        early_stop_criteria, early_stop_val = early_stop.split(',')[0], int(early_stop.split(',')[1])
        count_stop = 0
        hostenv.bound_torch_threads()        # torch's CPU pool <= the CPUs this container may use (hostenv.py: quota throttling stalls the loop)
        logging.info('name ' + args.name)
        total_time = 0
        logging.info('TRAIN')
        rank, world = mdist.rank(), mdist.world_size()
        if rank == 0:
            print('TRAIN')
        model.train()

        if inner_opt is None:
            inner_opt = FlatSGD(model, args.lr)
        elif not isinstance(inner_opt, FlatSGD):
            inner_opt = FlatSGD.from_torch(model, inner_opt)
        if outer_opt is None:
            outer_opt = FlatAdam(model, args.meta_lr)
        elif not isinstance(outer_opt, FlatAdam):
            outer_opt = FlatAdam.from_torch(model, outer_opt)
        self.inner_opt, self.outer_opt = inner_opt, outer_opt
        model.zero_copy_grad()

        last_sum_loss, last_sum_cer, last_sum_char = deque(maxlen=window_size), deque(maxlen=window_size), deque(maxlen=window_size)
        k_train, k_valid = args.k_train, args.k_valid
        n_tasks = len(train_data_list)
        train_data_buffer = [[] for _ in range(n_tasks)]
        my_tasks = mdist.shard_tasks(n_tasks, rank, world)

        takes_need = [_sample_takes_need(ds) for ds in train_data_list]      # decided ONCE from the signature (never by catching)
        pin_batches = bool(getattr(args, 'cuda', True)) and torch.cuda.is_available() and self.pin_batches

        def fetch_train_batch(buf):
            # every rank DRAWS every task (the index streams stay in lock-step), but only what this rank uses is loaded and
            # featurised: its own tasks' training batches and the last task's validation batch, which all tasks share (:168)
            for manifest_id in range(n_tasks):
                need = (manifest_id in my_tasks, manifest_id == n_tasks - 1)
                ds = train_data_list[manifest_id]
                if takes_need[manifest_id]:
                    item = ds.sample(k_train, k_valid, manifest_id, need=need)
                else:                                                # a duck-typed dataset with the reference's 3-argument sample()
                    item = ds.sample(k_train, k_valid, manifest_id)
                if pin_batches:
                    # the feature tensors this rank will upload are page-locked HERE, on the prefetch thread: a copy from pageable
                    # memory holds the enqueueing thread for its whole duration (transient_trainer.py:182-184,210-212 upload inside
                    # the timed span); torch's caching host allocator re-uses the blocks from iteration to iteration
                    item = tuple(((part[0].pin_memory(),) + tuple(part[1:])) if (want and torch.is_tensor(part[0]) and not part[0].is_cuda
                                                                                 and not part[0].is_pinned()) else part
                                 for part, want in zip(item, need))
                buf[manifest_id].insert(0, item)

        prefetch = threading.Thread(target=fetch_train_batch, args=(train_data_buffer,))
        prefetch.start()
        dev = model.flat_parameters.device
        sync_replicas_from_rank0(model, [outer_opt])
        check_every = int(self.replica_check_every)
        it = start_it
        failures = 0
        pending = deque()                                 # enqueued, not yet resolved: (it, step), oldest first
        clock = [time.time()]
        self.loss_trace = []                              # (validation loss / n, CER edits, characters) of every resolved iteration

        def resolve(it_, step):
            nonlocal total_time
            total_loss, total_cer, total_char = step.result()
            last_sum_cer.append(total_cer)
            last_sum_char.append(total_char)
            last_sum_loss.append(total_loss / n_tasks)
            self.loss_trace.append((total_loss / n_tasks, total_cer, total_char))
            now = time.time()
            diff_time, clock[0] = now - clock[0], now    # iterations overlap: the time between two resolutions is one iteration
            total_time += diff_time
            self.last_iteration_seconds = diff_time
            msg = '(Iteration {}) TRAIN LOSS:{:.4f} CER:{:.2f}% LR:{:.7f} TOTAL TIME:{:.7f}'.format(
                (it_ + 1), total_loss / n_tasks, total_cer * 100 / max(total_char, 1), self.get_lr(outer_opt), total_time)
            if rank == 0:
                print(msg)
            logging.info(msg)
            if (it_ + 1) % last_summary_every == 0:
                msg = '(Summary Iteration {} | MA {}) TRAIN LOSS:{:.4f} CER:{:.2f}%'.format(
                    (it_ + 1), window_size, sum(last_sum_loss) / len(last_sum_loss), sum(last_sum_cer) * 100 / sum(last_sum_char))
                if rank == 0:
                    print(msg, flush=True)
                logging.info(msg)

        while it < num_it:
            # like the reference (:141-376) a failing iteration is reported and skipped (new data is fetched, `it` does not
            # advance); unlike it, MAX_CONSECUTIVE_FAILURES failures in a row re-raise instead of looping forever
            try:
                prefetch.join()
                prefetch = threading.Thread(target=fetch_train_batch, args=(train_data_buffer,))
                prefetch.start()

                _, val_data = train_data_buffer[-1][-1]                  # the LAST task's validation batch, shared by all (:168)
                popped = [train_data_buffer[m].pop() for m in range(n_tasks)]
                task_batches = [popped[m][0] for m in my_tasks]
                if world > 1 and (it == start_it or (check_every > 0 and (it + 1) % check_every == 0)):
                    check_replicas(model, val_data, it)
                step = self.enqueue_iteration(model, vocab, task_batches, val_data, n_tasks, inner_opt, outer_opt, args)
                pending.append((it, step))                # (the enqueued step is on record before anything else can raise)
                drain = not self.pipeline or (it + 1) % evaluate_every == 0 or it + 1 >= num_it
                while pending and (drain or len(pending) > self.pipeline_depth):
                    resolve(*pending.popleft())           # older iterations are logged while the device runs the newer ones

                if (it + 1) % evaluate_every == 0:
                    save_fn = lambda metrics, best_model: save_meta_model(model, vocab, (it + 1), inner_opt, outer_opt, metrics,
                                                                          args, best_model=best_model)
                    stop, best_valid_val, count_stop = run_validation(
                        self.forward_one_batch, model, vocab, valid_loader_list, it, args, history, loss_type, save_fn,
                        early_stop_criteria, early_stop_val, best_valid_val, count_stop, rank)
                    clock[0] = time.time()                # evaluation time is not training time
                    if stop:
                        break
                it += 1
                failures = 0
            except KeyboardInterrupt:
                raise
            except Exception as e:
                failures += 1
                if failures >= MAX_CONSECUTIVE_FAILURES or world > 1:     # ranks must not skip different iterations
                    raise
                print('Error: {}, fetching new data...'.format(e), flush=True)
                logging.info('Error: {}, fetching new data...'.format(e))
                torch.cuda.synchronize(dev)
                # an iteration that was enqueued before the failure is complete now: log it and advance past it BEFORE the retry
                # re-uses its read-back buffers (the failed enqueue has flipped the buffer set)
                while pending:
                    done_it, done_step = pending.popleft()
                    try:
                        resolve(done_it, done_step)
                    except Exception as e2:               # its Adam step has been applied either way
                        logging.info('Error while resolving iteration {}: {}'.format(done_it + 1, e2))
                    it = max(it, done_it + 1)
        while pending:
            resolve(*pending.popleft())
        prefetch.join()
        self.history = history


class JointTrainer():
    """Drop-in for trainer/asr/joint_trainer.py (BASELINE.json configs[0], joint_train.py): per iteration the gradient of
    sum_m L_tr,m / n over all tasks, optional clip, ONE Adam(lr=args.lr) step (joint_trainer.py:182-262).
    With a discriminator (--multitask / --adversarial [--beta-decay], joint_trainer.py:208-256) task m adds w CE(accent = m) / n
    [+ MSE(logits, 1/C) / n] of the accent head on its encoder output; the head's own Adam(lr=args.lr_disc) steps after the model's.
    Same engine and kernels as the meta loop; tasks shard over ranks the same way."""

    BETA_DECAY = 0.99997                                                # joint_trainer.py:156

    def __init__(self):
        logging.info('Joint Trainer is initialized')
        self.beta = 1.0                                                 # joint_trainer.py:155: carried across iterations

    def get_lr(self, optimizer):
        return optimizer.param_groups[0]['lr']

    def forward_one_batch(self, model, vocab, src, trg, src_percentages, src_lengths, trg_lengths, smoothing, loss_type, verbose=False,
                          discriminator=None, accent_id=None, multi_task=False):
        """joint_trainer.py:25-91 -> (loss, total_cer, total_char) | (..., disc_loss) with multi_task | (..., disc_loss, enc_loss):
        differentiable tensors, one backward through their sum reaches the model and the discriminator."""
        if discriminator is None:
            return TransientTrainer.forward_one_batch(self, model, vocab, src, trg, src_percentages, src_lengths, trg_lengths, smoothing,
                                                      loss_type, verbose=verbose)
        _check_loss_type(loss_type)
        pred, gold, hyp, enc_output = model.forward_with_encoder_output(src, src_lengths, trg)
        accent_pred = discriminator(enc_output)                         # discriminator(torch.sum(enc_output, dim=1))
        if multi_task:
            disc_loss = calculate_multi_task(accent_pred, accent_id)
        else:
            disc_loss, enc_loss = calculate_adversarial(accent_pred, accent_id)
        sizes = src_percentages.mul_(int(pred.size(1))).int()
        loss, _ = calculate_metrics(pred, gold, vocab.PAD_ID, input_lengths=sizes, target_lengths=trg_lengths, smoothing=smoothing,
                                    loss_type=loss_type)
        total_cer, total_char = cer_counts(vocab, gold.cpu(), hyp.cpu())
        if verbose:
            print('Total CER', total_cer)
            print('Total char', total_char)
        if multi_task:
            return loss, total_cer, total_char, disc_loss
        return loss, total_cer, total_char, disc_loss, enc_loss

    def run_iteration(self, model, vocab, task_batches, n_tasks, opt, args, discriminator=None, opt_disc=None, task_ids=None,
                      loss_type='ce'):
        """One iteration over this rank's task batches.  discriminator / opt_disc: the accent head and its optimizer; task_ids: the
        tasks' indices among all n_tasks (their accent ids; default 0, 1, ...).  -> [total_loss, total_cer, total_char] and, with a
        discriminator, total_disc_loss (weighted, as logged) and total_enc_loss.
        loss_type 'ctc': every task's loss is the CTC loss of its batch's percentages and target sizes (joint_trainer.py:38-41)."""
        dev = model.flat_parameters.device
        g = model.flat_grad
        smoothing = float(getattr(args, 'label_smoothing', 0.0) or 0.0)
        _check_loss_type(loss_type)
        loss_kw = lambda pct, sizes: dict(loss_type='ctc', percentages=pct, target_sizes=sizes) if loss_type == 'ctc' else {}
        g.zero_()                                                       # opt.zero_grad()
        reads = []
        if discriminator is None:
            for (tx, tsz, _tp, ty, _tl) in task_batches:
                out = model.pass_forward(tx.to(dev, non_blocking=True), tsz, ty, smoothing=smoothing, **loss_kw(_tp, _tl))
                reads.append(_Readback(out, ('joint', len(reads), 0)))
                model.pass_backward(g, 1.0 / n_tasks)                   # (tr_loss / n).backward()
        else:
            adversarial = bool(getattr(args, 'adversarial', False))
            decay = adversarial and bool(getattr(args, 'beta_decay', False))
            task_ids = list(range(len(task_batches))) if task_ids is None else list(task_ids)
            batch_of = dict(zip(task_ids, task_batches))
            discriminator.zero_grad()                                   # opt_disc.zero_grad()
            weights, disc_reads = [], []
            for m in range(n_tasks):                                    # beta decays at every task visit, whichever rank makes it
                if decay:
                    self.beta = self.beta * self.BETA_DECAY
                if m not in batch_of:
                    continue
                w = 1.0 if not adversarial else (self.beta if decay else 0.5)
                tx, tsz, _tp, ty, _tl = batch_of[m]
                out = model.pass_forward(tx.to(dev, non_blocking=True), tsz, ty, smoothing=smoothing, **loss_kw(_tp, _tl))
                reads.append(_Readback(out, ('joint', len(reads), 0)))
                losses = discriminator.head_forward(model.engine.encoder_output(), m, adversarial)
                host = _pinned(('disc', len(disc_reads), 0), (2,), torch.float32)
                host.copy_(losses, non_blocking=True)
                disc_reads.append(host)
                weights.append(w)
                # (tr_loss / n + w disc_loss / n [+ enc_loss / n]).backward(): the head's gradient enters at the encoder output
                model.pass_backward(g, 1.0 / n_tasks, dmem_hook=lambda dmem, w=w: discriminator.head_backward(
                    w / n_tasks, 1.0 / n_tasks if adversarial else 0.0, dmem))
            mdist.allreduce_sum_(discriminator.flat_grad)
        mdist.allreduce_sum_(g)
        if args.clip:
            clip_flat_grad_(model, g, args.max_norm)
        opt.step(g)
        if discriminator is not None:
            opt_disc.step()
        torch.cuda.synchronize(dev)
        total_loss, total_cer, total_char = 0.0, 0, 0
        for rd in reads:
            c, n = cer_counts(vocab, rd.gold_host, rd.hyp)
            total_cer += c
            total_char += n
            total_loss += float(rd.loss[0])
        if discriminator is None:
            return mdist.allreduce_scalars([total_loss, total_cer, total_char], dev)
        # the reference logs the WEIGHTED discriminator loss, formed in fp32 (joint_trainer.py:230-236)
        self.task_losses = [(float(rd.loss[0]), float(h[0]), float(h[1])) for rd, h in zip(reads, disc_reads)]
        total_disc = sum(float(torch.tensor(w, dtype=torch.float32) * h[0]) for w, h in zip(weights, disc_reads))
        total_enc = sum(float(h[1]) for h in disc_reads) if adversarial else 0.0
        return mdist.allreduce_scalars([total_loss, total_cer, total_char, total_disc, total_enc], dev)

    def train(self, model, vocab, train_data_list, valid_loader_list, loss_type, start_it, num_it, args, evaluate_every=1000,
              window_size=100, last_summary_every=1000, last_metrics=None, early_stop=10, cpu_state_dict=False, is_copy_grad=False,
              opt_name='adam', discriminator=None):
        _check_loss_type(loss_type)
        if opt_name != 'adam':
            raise NotImplementedError("accelerated joint training: opt_name='adam'")
        if discriminator is not None:
            model._need_engine()
        if discriminator is not None and discriminator.flat_parameters.device != model.flat_parameters.device:
            raise RuntimeError('the discriminator lives on %s, the model on %s: the product path needs both on one MI355X (call '
                               '.cuda())' % (discriminator.flat_parameters.device, model.flat_parameters.device))
        rank, world = mdist.rank(), mdist.world_size()
        if rank == 0:
            print('TRAIN')
        hostenv.bound_torch_threads()
        model.train()
        opt = FlatAdam(model, args.lr)                                  # the reference builds a fresh Adam per train() call
        self.opt = opt
        opt_disc = None
        if discriminator is not None:                                   # joint_trainer.py:125-126, 155
            opt_disc = torch.optim.Adam(discriminator.parameters(), lr=args.lr_disc)
            self.beta = 1.0
        self.opt_disc = opt_disc
        adversarial = discriminator is not None and bool(getattr(args, 'adversarial', False))
        n_tasks = len(train_data_list)
        my_tasks = mdist.shard_tasks(n_tasks, rank, world)
        buf = [[] for _ in range(n_tasks)]

        takes_need = [_sample_takes_need(ds) for ds in train_data_list]

        def fetch():
            for m in range(n_tasks):                         # all tasks are drawn; only this rank's training batches are loaded
                if takes_need[m]:
                    item = train_data_list[m].sample(args.k_train, 1, m, need=(m in my_tasks, False))
                else:
                    item = train_data_list[m].sample(args.k_train, 1, m)
                buf[m].insert(0, item)
        prefetch = threading.Thread(target=fetch)
        prefetch.start()
        total_time, it = 0, start_it
        self.loss_trace = []
        history = []
        best_valid_val, count_stop, failures = 1000000000, 0, 0
        early_stop_criteria, early_stop_val = early_stop.split(',')[0], int(early_stop.split(',')[1])
        last_sum_loss, last_sum_cer, last_sum_char = deque(maxlen=window_size), deque(maxlen=window_size), deque(maxlen=window_size)
        sync_replicas_from_rank0(model, [opt] if discriminator is None else [opt, opt_disc], discriminator=discriminator)
        fob = TransientTrainer.forward_one_batch.__get__(self)             # the two reference trainers share this method body
        while it < num_it:
            try:
                prefetch.join()
                prefetch = threading.Thread(target=fetch)
                prefetch.start()
                start_time = time.time()
                popped = [buf[m].pop() for m in range(n_tasks)]
                # (without a discriminator the call carries the six positional arguments it always has)
                disc_kw = {} if discriminator is None else dict(discriminator=discriminator, opt_disc=opt_disc, task_ids=my_tasks)
                if loss_type != 'ce':
                    disc_kw['loss_type'] = loss_type
                totals = self.run_iteration(model, vocab, [popped[m][0] for m in my_tasks], n_tasks, opt, args, **disc_kw)
                total_loss, total_cer, total_char = totals[:3]
                total_disc_loss, total_enc_loss = totals[3:] if discriminator is not None else (None, None)
                total_time += time.time() - start_time
                self.loss_trace.append(total_loss / n_tasks)
                last_sum_cer.append(total_cer)
                last_sum_char.append(total_char)
                last_sum_loss.append(total_loss)
                if discriminator is None:
                    msg = '(Iteration {}) TRAIN LOSS:{:.4f} CER:{:.2f}% LR:{:.7f} TOTAL TIME:{:.7f}'.format(
                        (it + 1), total_loss / n_tasks, total_cer * 100 / max(total_char, 1), self.get_lr(opt), total_time)
                elif adversarial:
                    msg = ('(Iteration {}) TRAIN LOSS:{:.4f} DISC LOSS:{:.4f} ENC LOSS:{:.4f} CER:{:.2f}% LR:{:.7f} TOTAL TIME:{:.7f}'
                           .format((it + 1), total_loss / n_tasks, total_disc_loss / n_tasks, total_enc_loss / n_tasks,
                                   total_cer * 100 / max(total_char, 1), self.get_lr(opt), total_time))
                else:
                    msg = '(Iteration {}) TRAIN LOSS:{:.4f} DISC LOSS:{:.4f} CER:{:.2f}% LR:{:.7f} TOTAL TIME:{:.7f}'.format(
                        (it + 1), total_loss / n_tasks, total_disc_loss / n_tasks, total_cer * 100 / max(total_char, 1),
                        self.get_lr(opt), total_time)
                if rank == 0:
                    print(msg)
                logging.info(msg)
                if (it + 1) % last_summary_every == 0:
                    msg = '(Summary Iteration {} | MA {}) TRAIN LOSS:{:.4f} CER:{:.2f}%'.format(
                        (it + 1), window_size, sum(last_sum_loss) / len(last_sum_loss), sum(last_sum_cer) * 100 / sum(last_sum_char))
                    if rank == 0:
                        print(msg, flush=True)
                    logging.info(msg)
                if (it + 1) % evaluate_every == 0:                         # joint_trainer.py:306-380
                    def save_fn(metrics, best_model):
                        save_joint_model(model, vocab, (it + 1), opt, metrics, args, best_model=best_model)
                        if discriminator is not None and rank == 0:       # joint_trainer.py:358-359, 369-370
                            save_discriminator(discriminator, (it + 1), opt_disc, args, best_model=best_model)
                    stop, best_valid_val, count_stop = run_validation(
                        fob, model, vocab, valid_loader_list, it, args, history, loss_type, save_fn, early_stop_criteria,
                        early_stop_val, best_valid_val, count_stop, rank)
                    if stop:
                        break
                it += 1
                failures = 0
            except KeyboardInterrupt:
                raise
            except Exception as e:                                          # joint_trainer.py:382-392: report, fetch new data
                failures += 1
                if failures >= MAX_CONSECUTIVE_FAILURES or world > 1:
                    raise
                print('Error: {}, fetching new data...'.format(e), flush=True)
                logging.info('Error: {}, fetching new data...'.format(e))
                torch.cuda.synchronize(model.flat_parameters.device)
        prefetch.join()
        self.history = history
