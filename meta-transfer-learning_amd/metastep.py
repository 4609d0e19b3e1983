"""One meta-iteration on the device (trainer/asr/transient_trainer.py:178-237): the two schedules of a rank's local tasks -- one pass
chain per task on concurrent lanes, or ONE task-batched pass per phase for all of them -- with their input staging, read-backs, the
chunked all-reduce hook and the h2 range census.

Every function takes the trainer as its first argument (its plain attributes are the configuration: batch_tasks, use_cmdlists,
pipeline_depth, pad_lanes, ragged_quantum ...); TransientTrainer binds them as methods.  Both schedules run the same task program
(_task_program), under one command-list key (command_list_key) through the trainer's one _lib.Replay.
"""
import collections
import logging

import torch

from . import _lib, _trace, convstack, dist as mdist
from . import trainer as _trainer     # (imports this module in turn: clip_flat_grad_, cer_counts are looked up at call time)
from .batchmeta import CONV_TIME_SHIFT, enc_extent
from .engine import CENSUS_NAMES, CENSUS_SLOTS, PAD_ID, round_width

check = _lib.check

_PINNED = collections.OrderedDict()
_PINNED_MAX = 512          # variable-length data brings new read-back shapes all the time: least recently used entries go


def _pinned(key, shape, dtype, turns=1):
    """Page-locked host buffer of a read-back call site: pin_memory() costs a host allocation + registration that serialises against
    the device, and the read-backs of one iteration are only consumed after that iteration's device sync, so the memory is re-used.
    `key` ends with the index of the read-back set (`_turn`).  The cache holds RAW bytes per (site, set), sized for the largest shape
    seen so far and grown geometrically for ALL `turns` sets at once: variable-length data brings a new shape with almost every batch
    and must not bring a page-locked allocation with it, and none may happen a few iterations later inside a timed region."""
    shape = tuple(int(v) for v in shape)
    nbytes = torch.empty((), dtype=dtype).element_size()
    for v in shape:
        nbytes *= v
    raw = _PINNED.get(key)
    if raw is None or raw.numel() < nbytes:
        cap = max(nbytes + nbytes // 2, 256)
        for turn in range(turns):
            _PINNED[(key[:-1] + (turn,)) if turns > 1 else key] = torch.empty(cap, dtype=torch.uint8).pin_memory()
        raw = _PINNED[key]
        while len(_PINNED) > _PINNED_MAX:
            _PINNED.popitem(last=False)
    else:
        _PINNED.move_to_end(key)
    return raw[:nbytes].view(dtype).view(shape)


def _label_width(targets, quantum, most):
    """decoder positions of a pass on these padded targets (longest label sequence + 1), rounded up to a multiple of `quantum`: label
    widths change from batch to batch like the frame counts, and a wider decoder is exact (positions beyond a sequence are padding:
    masked as keys, zeroed as rows, outside the loss; their PAD labels leave the CER strings)"""
    own = max(int((t != PAD_ID).sum(1).max()) for t in targets) + 1
    q = max(int(quantum), 1)
    return max(min(-(-own // q) * q, most), own)


def _padded_width(eng, T, q):
    """T frames rounded up to a width that repeats (round_width, quantum q; q <= 1: T itself): any width at or above the batch's own
    is exact, up to what the positional table allows for the encoder length"""
    return max(min(round_width(T, q), eng.hp.src_max_len << getattr(eng, 'time_shift', CONV_TIME_SHIFT)), T) if q > 1 else T


def _padded_labels(tr, eng, targets, q):
    """the decoder width that goes with _padded_width: label widths repeat like the frame counts (None: the targets' own)"""
    return _label_width(targets, tr.label_quantum, eng.hp.tgt_max_len) if q > 1 and tr.label_quantum > 1 else None


class PendingIteration:
    """An enqueued meta-iteration: result() waits for ITS end-of-iteration event (not for the device, which may already be
    running the next iteration), then computes the reference's log quantities from the read-backs."""

    def __init__(self, reads, done, vocab, dev, census=None):
        self.reads, self.done, self.vocab, self.dev = reads, done, vocab, dev
        self.census = census          # (pinned counters, callback) of an iteration that sampled the h2 census
        self._result = None

    def result(self):
        if self._result is None:
            self.done.synchronize()
            total_loss, total_cer, total_char = 0.0, 0, 0
            for tr_read, va_read in self.reads:
                c, n = _trainer.cer_counts(self.vocab, tr_read.gold_host, tr_read.hyp)    # the reference reports the TRAIN batches' CER
                total_cer += c
                total_char += n
                total_loss += float(va_read.loss[0])
            self._result = mdist.allreduce_scalars([total_loss, total_cer, total_char], self.dev)
            self.reads = None
            if self.census is not None:
                counters, report = self.census
                self.census = None
                report(counters)
        return self._result


class _Readback:
    """Asynchronous D2H of (gold, hyp, loss) of one forward; resolved after the iteration's single sync.  `key` names the
    call site (task index, pass) whose pinned buffers are re-used from iteration to iteration."""

    def __init__(self, out, key, turns=1):
        self.gold_host = out['gold_host']
        self.hyp = _pinned(('hyp',) + tuple(key), out['hyp'].shape, torch.int64, turns)
        self.loss = _pinned(('loss',) + tuple(key), (1,), torch.float32, turns)
        self.hyp.copy_(out['hyp'], non_blocking=True)
        self.loss.copy_(out['loss'], non_blocking=True)


class _TaskRead:
    """One task's share of a task-batched pass's read-backs: views into the pinned whole-pass buffers (valid once the
    iteration's end event has been waited for)."""

    def __init__(self, gold_host, hyp, loss):
        self.gold_host, self.hyp, self.loss = gold_host, hyp, loss


def _turns(tr):
    """read-back buffer sets: one per iteration the host may have in flight (pipeline depth) + the one being resolved"""
    return max(tr.pipeline_depth, 1) + 1


# ---------------------------------------------------------------------------------------------------------------------
# what both schedules share: the task program, its result slots, its command-list key
# ---------------------------------------------------------------------------------------------------------------------
# what an iteration fixes for all of its tasks
_Step = collections.namedtuple('_Step', 'model theta0 use_cmdlists loss_type n_tasks lr clip max_norm smoothing')


def _slots(eng, m_tr, m_va):
    """the four device buffers a task program leaves its results in: labels and one loss per task, of both passes"""
    return dict(hyp_tr=eng.buf('slot.hyp_tr', (m_tr['nt'] * m_tr['B'], m_tr['Td']), torch.int64), loss_tr=eng.buf('slot.loss_tr', (m_tr['nt'],)),
                hyp_va=eng.buf('slot.hyp_va', (m_va['nt'] * m_va['B'], m_va['Td']), torch.int64), loss_va=eng.buf('slot.loss_va', (m_va['nt'],)))


def command_list_key(tag, scalars, tensors):
    """The key a recorded task program is kept under: the schedule's tag, every scalar its calls bake in, and the ADDRESS of every
    tensor they bake in (None: a tensor the program does not use, e.g. no census on this iteration) -- a buffer that was
    re-allocated is another key, so nothing recorded against the old address is replayed."""
    return (tag,) + tuple(scalars) + tuple(None if t is None else t.data_ptr() for t in tensors)


def _task_program(step, eng, lane, nt, g, theta1, G, x_tr, m_tr, x_va, m_va, slots, chunk):
    """Kernels of trainer/asr/transient_trainer.py:188-229 on the current stream (eager, or recorded into a command list): train
    pass at theta0, fused inner SGD into theta', validation pass at theta', accumulation into G.
    nt None: ONE task on lane `lane` (g, theta', G flat).  nt tasks: one task-batched pass per phase -- g and theta' are (nt, P)
    stacks, task t reads its own theta'_t (task = outermost batch index of every product), G += sum_t g_t in task order.
    chunk: the hook that hands G's parameter groups to their all-reduce as the validation backward finishes them (it forms G)."""
    model, theta0, lt = step.model, step.theta0, step.loss_type
    total = model._layout.total
    stride = 0 if nt is None else total
    eng.zero_(g)                                                         # inner_opt.zero_grad()   (:198)
    eng.forward_device(theta0, x_tr, m_tr, step.smoothing, hyp_out=slots['hyp_tr'], loss_out=slots['loss_tr'], loss_type=lt)      # (:188)
    eng.backward(g, 1.0, sG=stride)                                      # tr_loss.backward()      (:199)
    if step.clip:                                                        # (:205-206), per task
        for g_t in ([g] if nt is None else [g[t * total:(t + 1) * total] for t in range(nt)]):
            _trainer.clip_flat_grad_(model, g_t, step.max_norm, lane=lane)
    if nt is None:                                                       # inner_opt.step()        (:207)
        eng.sgd_theta_prime(theta0, g, step.lr, theta1)
    else:
        check(eng.lib.mtl_sgd_theta_prime_tasks(eng.stream, theta0.data_ptr(), g.data_ptr(), step.lr, theta1.data_ptr(), total, nt),
              'mtl_sgd_theta_prime_tasks')
    eng.forward_device(theta1, x_va, m_va, step.smoothing, hyp_out=slots['hyp_va'], loss_out=slots['loss_va'], sP=stride, loss_type=lt)   # (:215)
    eng.slice_hook = chunk
    try:
        eng.backward(g, 1.0 / step.n_tasks, sG=stride)                   # (val_loss/n).backward(): g += g_val/n (Q1)
    finally:
        eng.slice_hook = None
    if chunk is None and nt is None:                                     # add_copy_grad()         (:229)
        eng.axpy_(G, g, 1.0)
    elif chunk is None:
        check(eng.lib.mtl_sum_tasks(eng.stream, G.data_ptr(), g.data_ptr(), total, nt, 0), 'mtl_sum_tasks')


def _run_tasks(tr, step, eng, tag, lane, nt, bufs, x_tr, m_tr, x_va, m_va, own, chunk, inputs=None):
    """The task program of one lane's task (nt None) or of the nt stacked tasks, on the current stream: call by call, or -- the
    trainer's switch in front of its Replay -- eager, recorded, replayed.  own: (bool, bool) do the passes carry frame counts of
    their own; inputs: (x_tr, x_va) where they move between replays.  -> the result slots"""
    slots = _slots(eng, m_tr, m_va)
    # row t of the census counters belongs to local task t of a task-batched pass, or to lane t
    eng.census = None if tr._census_on is None else tr._census_on[lane:lane + (nt or 1)]
    body = lambda: _task_program(step, eng, lane, nt, *bufs, x_tr, m_tr, x_va, m_va, slots, chunk)
    if not step.use_cmdlists:
        body()
        return slots
    scalars = (step.loss_type, lane, nt, tuple(x_tr.shape), tuple(x_va.shape)) + tuple(own) + (
        m_tr['Td'], m_va['Td'], step.n_tasks, step.clip, step.max_norm, step.smoothing, step.lr, eng.dropout_p, eng.use_side_stream,
        chunk is not None, eng.stream)
    key = command_list_key(tag, scalars, (step.theta0,) + tuple(bufs) + (eng.census,))
    tr.replay.begin(eng, key)(0, body, None if inputs is None else tuple(x.data_ptr() for x in inputs), chunk)
    return slots


# ---------------------------------------------------------------------------------------------------------------------
# the schedules
# ---------------------------------------------------------------------------------------------------------------------
def meta_iteration(tr, model, vocab, task_batches, val_batch, n_tasks, inner, outer, args, task_ids=None, loss_type=None):
    """task_batches: this rank's [(inputs, input_sizes, percentages, targets, target_sizes)], val_batch: same 5-tuple.
    loss_type: 'ce' or 'ctc' (default: tr.loss_type).  With 'ctc' every pass's loss is the CTC loss of its batch's percentages
    and target sizes (a None there is derived from the lengths / the targets, PassEngine.prepare_tasks); label smoothing is ignored.
    n_tasks is the GLOBAL task count (the 1/n of the validation loss).  Leaves G in model._G; returns the read-backs.
    With several ranks and chunking on, the schedules that hook the validation backward leave model._G ALREADY summed over
    the ranks and set tr._G_reduced (reset here on entry); a direct caller must check that flag -- or call
    reduce_meta_gradient(), which does -- before posting a collective of its own.

    All local tasks in one task-batched pass per phase where they can be stacked (_can_batch), else on the lanes."""
    tr._G_reduced = False
    lt = tr.loss_type if loss_type is None else loss_type
    _trainer._check_loss_type(lt)
    hooked = any(e.prof is not None or e.forward_hook is not None for e in model.engines)
    step = _Step(model, model.flat_parameters, tr.use_cmdlists and not hooked, lt, n_tasks, float(inner.param_groups[0]['lr']),
                 bool(args.clip), float(args.max_norm), float(getattr(args, 'label_smoothing', 0.0) or 0.0))
    tr.last_schedule = 'lanes'                               # (diagnostics / tests: which schedule the last iteration took)
    if tr._can_batch(model, task_batches, val_batch):
        frames = [int(tb[0].shape[3]) for tb in task_batches]
        tr.last_schedule = 'batched' if min(frames) == max(frames) else 'batched-ragged'
        return _batched_iteration(tr, step, task_batches, val_batch)
    return _lane_iteration(tr, step, task_batches, val_batch)


def _widened(eng, x, name, q):
    """-> (x or its copy in a zero-filled buffer of the rounded width, own frame count or None)"""
    T_own = int(x.shape[3])
    Tq = _padded_width(eng, T_own, q)
    if Tq == T_own:
        return x, None
    xp = eng.buf(name, tuple(x.shape[:3]) + (Tq,))
    xp.zero_()
    xp[:, :, :, :T_own].copy_(x, non_blocking=True)
    return xp, T_own


def _lane_iteration(tr, step, task_batches, val_batch):
    """Tasks are independent given theta0, so they are dealt round-robin onto the model's task lanes (own stream, buffer
    arena, gradient / theta' / G buffers): one task's many small transformer kernels fill the CUs another task's
    convolutions leave idle.  Lane accumulators are summed in lane order, so G stays run-to-run deterministic."""
    model, ctc = step.model, step.loss_type == 'ctc'
    dev = step.theta0.device
    n_lanes = min(model.n_lanes, max(len(task_batches), 1))
    if len(task_batches) > n_lanes:                      # several rounds: equal rounds (8 tasks on 6 lanes measured slower than on 3)
        rounds = -(-len(task_batches) // n_lanes)
        n_lanes = -(-len(task_batches) // rounds)
    bufs = _lane_buffers(tr, model, n_lanes)
    main = torch.cuda.current_stream(dev)
    vx = val_batch[0].to(dev, non_blocking=True)
    # widths that change from batch to batch (manifest-fed) would be enqueued call by call for ever: rounded up to a quantum they
    # repeat (recorded lists replay, the pool keeps its buffers); the batch keeps its own border and encoder length (prepare(frames))
    varies = tr._widths_vary([('lane', i, int(tb[0].shape[3])) for i, tb in enumerate(task_batches)] + [('lane', 'val', int(vx.shape[3]))])
    q = tr.ragged_quantum if varies else 0
    vx, v_own = _widened(model.engines[0], vx, 'lane.x_va', q)
    ready = torch.cuda.Event()
    ready.record(main)
    reads = [None] * len(task_batches)
    streams = [model.lane_streams[lane] if n_lanes > 1 else main for lane in range(n_lanes)]
    for lane in range(n_lanes):
        with torch.cuda.stream(streams[lane]):
            streams[lane].wait_event(ready)
            bufs[lane][2].zero_()
    ctc_kw = lambda pct, sizes: dict(percentages=pct, target_sizes=sizes) if ctc else {}
    for idx, (tx, tsz, _tp, ty, _tl) in enumerate(task_batches):      # enqueue task by task, alternating lanes
        lane = idx % n_lanes
        eng = model.engines[lane]
        with torch.cuda.stream(streams[lane]):
            tx, t_own = _widened(eng, tx.to(dev, non_blocking=True), 'lane.x_tr', q)
            m_tr = eng.prepare(tsz, ty, tx.shape[0], tx.shape[3], slot=0, frames=t_own, width=_padded_labels(tr, eng, [ty], q),
                               **ctc_kw(_tp, _tl))                      # host ints -> static device buffers
            m_va = eng.prepare(val_batch[1], val_batch[3], vx.shape[0], vx.shape[3], slot=1, frames=v_own,
                               width=_padded_labels(tr, eng, [val_batch[3]], q), **ctc_kw(val_batch[2], val_batch[4]))
            # a rank that holds ONE task (8 tasks on 8 GPUs): G = its g, handed to the all-reduce group by group under the backward
            chunk = None
            if n_lanes == 1 and len(task_batches) == 1:
                g_, G_ = bufs[lane][0], bufs[lane][2]
                chunk = tr._chunk_hook(model, eng, lambda lo, n, st, g_=g_, G_=G_: check(
                    _lib.lib().mtl_axpy(st, G_.data_ptr() + 4 * lo, g_.data_ptr() + 4 * lo, 1.0, n), 'mtl_axpy'))
            slots = _run_tasks(tr, step, eng, 'lanes', lane, None, bufs[lane], tx, m_tr, vx, m_va, (t_own is not None, v_own is not None),
                               chunk, inputs=(tx, vx))
            reads[idx] = (_Readback(dict(gold_host=m_tr['gold_host'], hyp=slots['hyp_tr'], loss=slots['loss_tr']), (idx, 0, tr._turn), tr._turns()),
                          _Readback(dict(gold_host=m_va['gold_host'], hyp=slots['hyp_va'], loss=slots['loss_va']), (idx, 1, tr._turn), tr._turns()))
    if streams[0] is not main:
        for lane in range(n_lanes):
            done = torch.cuda.Event()
            done.record(streams[lane])
            main.wait_event(done)
    tr._chunk_join(dev)
    if n_lanes > 1:                                           # (a single lane accumulated straight into model._G)
        model._G.copy_(bufs[0][2])
        for lane in range(1, n_lanes):
            model._axpy(model._G, bufs[lane][2], 1.0)
    return reads


def _lane_buffers(tr, model, n_lanes):
    """(grad, theta', G) per lane; lane 0 uses the model's own flat_grad / copy_grad buffers when it is the only lane."""
    key = (id(model.flat_parameters), n_lanes)
    if tr._lane_key != key:
        th = model.flat_parameters
        if n_lanes == 1:
            tr._lanes = [(model.flat_grad, torch.empty_like(th), model._G)]
        else:
            tr._lanes = [(torch.zeros_like(th), torch.empty_like(th), torch.zeros_like(th)) for _ in range(n_lanes)]
        tr._lane_key = key
    return tr._lanes


def _widths_vary(tr, sightings):
    """sightings: [(schedule, slot, frames)] of this iteration's batches.  -> whether batches are to be widened to repeating widths:
    pad_lanes '1' always, '0' never, 'auto' from the moment any slot (a task's position, the validation batch) has brought two
    different widths -- a fixed-shape workload is never padded, a manifest-fed one from its second iteration on."""
    if tr.pad_lanes != 'auto':
        return tr.pad_lanes == '1'
    if not tr._lane_widths_vary:
        for sched, slot, frames in sightings:
            if tr._lane_widths.setdefault((sched, slot), frames) != frames:
                tr._lane_widths_vary = True
                break
    return tr._lane_widths_vary


def _can_batch(tr, model, task_batches, val_batch):
    """All local tasks in one pass per phase: needs >= 2 tasks with identical batch shapes (samples x frames; label widths may
    differ) and the fused attention kernel."""
    if not tr.batch_tasks or len(task_batches) < 2:
        return False
    eng = model.engines[0]
    if not eng.fused_attn:
        return False
    if val_batch[0].dim() != 4 or any(tb[0].dim() != 4 for tb in task_batches):
        return False
    shape = tuple(task_batches[0][0].shape)
    if all(tuple(tb[0].shape) == shape for tb in task_batches):
        return True
    # manifest-fed batches: every task's batch is padded to its OWN longest utterance (data.py:77), so the frame counts differ.
    # They are stacked at the widest (engine.prepare_tasks(frames=...) keeps each task's own image border and encoder length) as
    # long as the padding does not outweigh what one pass for all tasks saves over a lane per task (which, on shapes that never
    # repeat, is enqueued call by call: ~88 ms of host time per 8-task north-star step against ~55 ms of kernels).
    if not tr.batch_ragged:
        return False
    if any(tuple(tb[0].shape[:3]) != shape[:3] for tb in task_batches):
        return False
    frames = [int(tb[0].shape[3]) for tb in task_batches]
    # (every task needs at least one encoder position: 4 frames behind a conv stack, 1 without one)
    return enc_extent(min(frames), getattr(eng, 'time_shift', CONV_TIME_SHIFT)) >= 1 and sum(frames) >= tr.ragged_fill * len(frames) * max(frames)


def _batched_iteration(tr, step, task_batches, val_batch):
    """trainer/asr/transient_trainer.py:178-237 for all local tasks at once.  The tasks of a meta-step are independent given
    theta0, so their training passes run as ONE pass over nt x k_train samples (shared parameters; per-task losses and a
    (nt, P) stack of per-task gradients), the nt inner steps as one kernel into a (nt, P) stack of theta', and their
    validation passes as ONE pass in which task t reads its own theta'_t.  G = sum_t (g_tr,t + g_val,t / n) in task order.
    The ~200 latency-bound transformer launches of a pass run once per phase instead of once per task."""
    model, theta0, ctc = step.model, step.theta0, step.loss_type == 'ctc'
    dev = theta0.device
    eng = model.engines[0]
    nt = len(task_batches)
    total = model._layout.total
    B = task_batches[0][0].shape[0]
    frames = [int(tb[0].shape[3]) for tb in task_batches]
    vx_in = val_batch[0]
    Bv, Tv_own = vx_in.shape[0], int(vx_in.shape[3])
    # (uniform across the tasks but changing from step to step -- a loader that pads all tasks alike -- is rounded as well, from the
    # second width on: `_widths_vary`)
    varies = tr._widths_vary([('batched', 'train', max(frames)), ('batched', 'val', Tv_own)]) and tr.batch_ragged
    q = tr.ragged_quantum if min(frames) != max(frames) or varies else 0
    T, Tv = _padded_width(eng, max(frames), q), _padded_width(eng, Tv_own, q)
    if tr._stack_key != (id(theta0), nt):
        tr._stack = (torch.zeros(nt * total, dtype=torch.float32, device=dev), torch.empty(nt * total, dtype=torch.float32, device=dev))
        tr._stack_key = (id(theta0), nt)
    g, theta1 = tr._stack
    Xtr, Xva = _stage_inputs(tr, eng, task_batches, vx_in, frames, T, Tv)
    _trace.mark('input_copies')
    own_tr = min(frames) != T                                # some task is narrower than the stack: borders / lengths of their own
    # ctc: every task's in_len comes from ITS percentages and ITS own decoder width, whatever width the stack is padded to
    ctc_tr = dict(percentages=[tb[2] for tb in task_batches], target_sizes=[tb[4] for tb in task_batches]) if ctc else {}
    ctc_va = dict(percentages=[val_batch[2]] * nt, target_sizes=[val_batch[4]] * nt) if ctc else {}
    m_tr = eng.prepare_tasks([(tsz, ty) for (_tx, tsz, _tp, ty, _tl) in task_batches], B, T, slot=0, frames=frames if own_tr else None,
                             width=_padded_labels(tr, eng, [tb[3] for tb in task_batches], q), **ctc_tr)
    m_va = eng.prepare_tasks([(val_batch[1], val_batch[3])] * nt, Bv, Tv, slot=1, frames=[Tv_own] * nt if Tv != Tv_own else None,
                             width=_padded_labels(tr, eng, [val_batch[3]], q), **ctc_va)
    _trace.mark('prepare_tasks')
    G = model._G
    # several ranks: G's three parameter groups are summed over the local tasks and all-reduced one by one, each as soon as the
    # validation backward has produced it (decoder first, conv last) -- on a communication stream, under the rest of the backward
    chunk = tr._chunk_hook(model, eng, lambda lo, n, st: check(
        _lib.lib().mtl_sum_tasks_strided(st, G.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, n, nt, total, 0), 'mtl_sum_tasks_strided'))
    # (the passes read the two static buffers: nothing moves between replays)
    slots = _run_tasks(tr, step, eng, 'batched', 0, nt, (g, theta1, G), Xtr, m_tr, Xva, m_va, (own_tr, Tv != Tv_own), chunk)
    _trace.mark('launches')
    tr._chunk_join(dev)
    # one read-back per slot, into the pinned buffer of its site ('tb.hyp' / 'tb.loss', pass 0 / 1, read-back set)
    host = {name: _pinned(('tb.' + name.split('_')[0], int(name.endswith('_va')), tr._turn), slots[name].shape, slots[name].dtype, tr._turns())
            for name in ('hyp_tr', 'hyp_va', 'loss_tr', 'loss_va')}
    for name, dst in host.items():
        dst.copy_(slots[name], non_blocking=True)
    _trace.mark('readback_copies')
    return [(_TaskRead(m_tr['gold_hosts'][t], host['hyp_tr'][t * B:(t + 1) * B], host['loss_tr'][t:t + 1]),
             _TaskRead(m_va['gold_hosts'][t], host['hyp_va'][t * Bv:(t + 1) * Bv], host['loss_va'][t:t + 1])) for t in range(nt)]


def _stage_inputs(tr, eng, task_batches, vx_in, frames, T, Tv):
    """-> (Xtr, Xva): the two STATIC buffers the task-batched passes read (recorded command lists hold their addresses, and addresses
    derived from them per task), filled with this iteration's batches: task t's frames[t] frames at the front of slab t of the
    (nt * B, 1, F, T) stack, the validation batch in Tv frames.
    Inputs that arrive in HOST memory (the reference uploads every batch inside its timed span, transient_trainer.py:182-184,210-212)
    go up on their own stream into one of two landing sets, so the copy engine moves iteration i + 1's batches under iteration i's
    kernels (the host enqueues ahead); the main stream waits for the set's `ready` event and moves it into the static buffers with
    one device copy each (~20 us).  A landing set is rewritten only after that device copy has run (`_xfree`).  Device-resident
    inputs are copied straight into the static buffers."""
    dev = eng.device
    nt = len(task_batches)
    B, _, F, _ = task_batches[0][0].shape
    Tv_own = int(vx_in.shape[3])
    main = torch.cuda.current_stream(dev)
    Xtr = eng.buf('tb.x_tr', (nt * B, 1, F, T))
    Xva = eng.buf('tb.x_va', tuple(vx_in.shape[:3]) + (Tv,))
    _trace.mark('setup')
    on_host = not vx_in.is_cuda or any(not tb[0].is_cuda for tb in task_batches)
    wide = min(frames) != T or Tv != Tv_own
    nv = vx_in.numel()

    def place(src_tr, src_va):
        """every task's frames at the front of its slab, zeros behind them (the border its own, narrower image ends in);
        src_tr(t) / src_va: device tensors of the batches' own shapes"""
        Xtr.zero_()
        X5 = Xtr.view(nt, B, 1, F, T)
        for t in range(nt):
            X5[t, :, :, :, :frames[t]].copy_(src_tr(t), non_blocking=True)
        if Tv != Tv_own:
            Xva.zero_()
        Xva[:, :, :, :Tv_own].copy_(src_va, non_blocking=True)
    if on_host and tr.overlap_uploads:
        xs = tr._xset = (tr._xset + 1) % 2
        if tr._upload_stream is None:
            tr._upload_stream, tr._xfree = torch.cuda.Stream(dev), {}
        Ltr = eng.buf('tb.land_tr.%d' % xs, (nt * B, 1, F, T))
        Lva = eng.buf('tb.land_va.%d' % xs, tuple(Xva.shape))
        L2 = Ltr.view(nt, -1)                            # a task's batch lands CONTIGUOUSLY at the front of its slab (its own shape)
        up = tr._upload_stream
        with torch.cuda.stream(up):
            free = tr._xfree.get((xs, Ltr.data_ptr(), Lva.data_ptr()))
            if free is not None:
                up.wait_event(free)
            else:
                up.wait_stream(main)                 # first use of this set: behind whatever produced / last used the memory
                Ltr.record_stream(up)                # (the pool may hand the block back to torch's allocator one day)
                Lva.record_stream(up)
            if vx_in.is_cuda or any(tb[0].is_cuda for tb in task_batches):
                # mixed residency (e.g. a cached device-resident validation batch beside host training batches): a device tensor
                # may have been produced on the main stream in this very iteration
                up.wait_stream(main)
            for t, (tx, _tsz, _tp, _ty, _tl) in enumerate(task_batches):
                L2[t, :tx.numel()].copy_(tx.reshape(-1), non_blocking=True)
            Lva.view(-1)[:nv].copy_(vx_in.reshape(-1), non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(up)
        main.wait_event(ready)
        if wide:
            place(lambda t: L2[t, :B * F * frames[t]].view(B, 1, F, frames[t]), Lva.view(-1)[:nv].view(vx_in.shape))
        else:
            Xtr.copy_(Ltr, non_blocking=True)
            Xva.copy_(Lva, non_blocking=True)
        free = torch.cuda.Event()
        free.record(main)
        tr._xfree = {(xs, Ltr.data_ptr(), Lva.data_ptr()): free, **{k_: v_ for k_, v_ in tr._xfree.items() if k_[0] != xs}}
    elif wide:
        place(lambda t: task_batches[t][0] if task_batches[t][0].is_cuda else task_batches[t][0].to(dev, non_blocking=True),
              vx_in if vx_in.is_cuda else vx_in.to(dev, non_blocking=True))
    else:
        for t, (tx, _tsz, _tp, _ty, _tl) in enumerate(task_batches):
            Xtr[t * B:(t + 1) * B].copy_(tx, non_blocking=True)
        Xva.copy_(vx_in, non_blocking=True)
    return Xtr, Xva


# ---------------------------------------------------------------------------------------------------------------------
# the chunked all-reduce under the validation backward
# ---------------------------------------------------------------------------------------------------------------------
def _chunk_hook(tr, model, eng, accumulate_slice):
    """-> callable(tag) for PassEngine.slice_hook (None when the meta-gradient is not all-reduced in chunks).  At the point where
    the validation backward has enqueued the last kernel of a parameter group, the hook -- on the communication stream, behind the
    engine's main AND side stream -- forms that group's slice of G from the local gradients (accumulate_slice(first, count, raw
    stream)) and starts its all-reduce (dist.ChunkedAllReduce); _chunk_join() makes the main stream wait for all three before the
    outer step.  Fixed slice order on every rank: decoder, encoder, conv (the order the backward finishes them in)."""
    if not mdist.chunked_on():
        tr._chunks = None
        return None
    dev = model.flat_parameters.device
    if tr._comm_stream is None:
        tr._comm_stream = torch.cuda.Stream(dev)
    bounds = eng.slice_bounds()
    if sorted(set(bounds) | {'conv'}) != ['conv', 'decoder', 'encoder']:      # (a model without convolutions has the other two only)
        raise RuntimeError('unexpected parameter groups %s' % sorted(bounds))
    tr._chunks = mdist.ChunkedAllReduce()
    G, comm = model._G, tr._comm_stream

    def hook(tag):
        lo, hi = bounds[tag]
        comm.wait_stream(torch.cuda.current_stream(dev))
        if eng.side is not None:
            comm.wait_stream(eng.side)
        with torch.cuda.stream(comm):
            accumulate_slice(lo, hi - lo, comm.cuda_stream)
            tr._chunks.issue(G[lo:hi])
    return hook


def _chunk_join(tr, dev):
    """the main stream waits for the chunked collectives (and the slice sums in front of them); marks G as already reduced"""
    if tr._chunks is None:
        return
    with torch.cuda.stream(tr._comm_stream):
        tr._chunks.wait()                        # comm stream waits for the collectives' stream
    torch.cuda.current_stream(dev).wait_stream(tr._comm_stream)
    tr._chunks = None
    tr._G_reduced = True


# ---------------------------------------------------------------------------------------------------------------------
# the h2 range census (TransientTrainer.__init__ describes the guard)
# ---------------------------------------------------------------------------------------------------------------------
def _census_begin(tr, model, n_local):
    """-> the zeroed counter buffer when this iteration samples the h2 census, else None.  Row t belongs to local task t of a
    task-batched pass, or to lane t of the lane schedule.  (The buffer grows with the rows; its address is part of every
    command-list key.)"""
    tr._census_on = None
    engs = getattr(model, 'engines', None)
    if not engs or tr.h2_check_every <= 0 or not all(e.conv_h2 for e in engs) or any(e.prof is not None for e in engs):
        return None
    if any(convstack.decide(e, 1, None)['conv_mode'] != 'h2' for e in engs):      # (a large_cnn model: no h2 operand to count)
        return None
    tr._h2_iter += 1
    if (tr._h2_iter - 1) % tr.h2_check_every:
        return None
    rows = max(len(engs), n_local, 1)
    dev = model.flat_parameters.device
    if tr._h2_buf is None or tr._h2_buf.shape[0] < rows or tr._h2_buf.device != dev:
        tr._h2_buf = torch.zeros(rows, CENSUS_SLOTS, 4, dtype=torch.int64, device=dev)
    engs[0].zero_(tr._h2_buf)
    tr._census_on = tr._h2_buf
    return tr._h2_buf


def _census_report(tr, model, counters):
    """the read-back counters of a census iteration -> tr.h2_census {operand: (share below 22 bits, share below 16 bits)} of
    the non-zero elements; acts per `h2_guard` when an operand's share below 16 bits exceeds `h2_limit`"""
    c = counters.numpy().reshape(-1, CENSUS_SLOTS, 4).sum(0)
    if mdist.world_size() > 1:
        # every rank samples on the same iterations: the counters are summed over the ranks (host collective), so that all of them
        # see the same shares and take the same decision
        flat = mdist.allreduce_scalars([float(v) for v in c.reshape(-1)], counters.device)
        c = torch.tensor(flat, dtype=torch.float64).view(CENSUS_SLOTS, 4).numpy()
    tr.h2_census = {CENSUS_NAMES[i]: (float(c[i, 1]) / max(int(c[i, 0]), 1), float(c[i, 2]) / max(int(c[i, 0]), 1))
                    for i in sorted(CENSUS_NAMES) if int(c[i, 0]) > 0}
    worst = max(tr.h2_census, key=lambda k_: tr.h2_census[k_][1], default=None)
    msg = 'H2 CENSUS share of non-zero elements below 22 / 16 significand bits: ' + ', '.join(
        '%s %.2e / %.2e' % (k_, v[0], v[1]) for k_, v in tr.h2_census.items())
    logging.info(msg)
    if worst is None or tr.h2_census[worst][1] <= tr.h2_limit:
        return
    what = ('%.2e of the non-zero elements of "%s" keep fewer than 16 significand bits under one scale per tensor (limit %.1e): '
            'the batch mixes magnitudes more than 2^22 apart (features not normalised per utterance?)' %
            (tr.h2_census[worst][1], worst, tr.h2_limit))
    if tr.h2_guard == 'raise':
        raise RuntimeError('h2 range guard: ' + what)
    if tr.h2_guard == 'x3' and all(e.conv_h2 for e in model.engines):
        for e in model.engines:
            e.conv_mode, e.conv_x3, e.conv_h2 = 'x3', True, False
        tr.replay.clear()                                # (the recorded lists hold the h2 entry points)
        what += '; the 3x3 convolutions and the input Linear run on the exact 3 x bf16 split from the next enqueued iteration on'
    logging.warning('h2 range guard: ' + what)
    print('WARNING: h2 range guard: ' + what, flush=True)
