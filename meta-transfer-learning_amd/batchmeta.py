"""Host-side integer preparation of a batch: the decoder's input / output ids and the int32 meta block from which the kernels derive
every mask (modules/decoder.py:55-69, utils/metrics.py:129).  numpy only, no device: PassEngine.prepare_tasks stages and uploads what
`batch_meta` returns."""
import numpy as np
import torch

PAD_ID, SOS_ID, EOS_ID = 0, 1, 2
CONV_TIME_SHIFT = 2         # the conv stacks' two 2 x 2 max-pools: T frames -> (T // 2) // 2 encoder positions


def enc_extent(frames, time_shift=CONV_TIME_SHIFT):
    """THE definition of the encoder's extent: positions the encoder holds for `frames` input frames (an int or an integer array).
    time_shift: log2 of the front-end's time reduction -- 2 behind the conv stacks ((T // 2) // 2 = T >> 2), 0 for a model without a
    feature extractor, whose frames ARE the positions (PassEngine.time_shift derives it from the parameter layout)."""
    return frames >> time_shift


def decoder_io(padded_target, pad_id=PAD_ID, sos_id=SOS_ID, eos_id=EOS_ID, width=None):
    """modules/decoder.py:55-69 on the host: seq_in = [SOS, y..] padded with EOS; seq_out = [y.., EOS] padded with PAD.
    width: at least this many decoder positions (a slice of a batch keeps the whole batch's width, so that the labels
    predicted at padded positions -- which the reference's CER strings include -- are the same)."""
    tgt = padded_target.detach().to('cpu', torch.int64).numpy()
    B, L = tgt.shape
    nonpad = tgt != pad_id
    lens = nonpad.sum(1)
    width = max(int(lens.max()) + 1, int(width or 0))
    # every row's non-pad labels moved to the front in their order (the reference drops pads wherever they stand): a stable
    # argsort of the pad flags; numpy on these few hundred integers costs a tenth of the per-row tensor indexing it replaces
    comp = np.take_along_axis(tgt, np.argsort(~nonpad, axis=1, kind='stable'), 1)
    m = min(L, width - 1)
    own = np.arange(m)[None, :] < lens[:, None]
    seq_in = np.full((B, width), eos_id, dtype=np.int64)
    seq_out = np.full((B, width), pad_id, dtype=np.int64)
    seq_in[:, 0] = sos_id
    seq_in[:, 1:m + 1] = np.where(own, comp[:, :m], eos_id)
    seq_out[:, :m] = np.where(own, comp[:, :m], pad_id)
    seq_out[np.arange(B), lens] = eos_id
    return torch.from_numpy(seq_in), torch.from_numpy(seq_out)


def ctc_input_lengths(percentages, Td):
    """utils/metrics.py:129 / transient_trainer.py:38: sizes = src_percentages.mul_(Td).int() -- an fp32 product, truncated (numpy in
    fp32 reproduces it bit for bit; the caller's tensor is not scaled in place here)."""
    return (np.asarray(percentages, dtype=np.float32) * np.float32(Td)).astype(np.int32)


def _occurrence_chains(flat_in, base):
    """occurrence chains of the decoder input ids (deterministic embedding scatter-add, mtl_embed_bwd): first[i] = 1 where i is the
    first position of its id, next[i] = base + the next position of the same id, -1 at the last"""
    order = np.argsort(flat_in, kind='stable')
    srt = flat_in[order]
    same_as_prev = np.zeros(srt.shape, dtype=bool)
    same_as_prev[1:] = srt[1:] == srt[:-1]
    first = np.empty(flat_in.shape, dtype=np.int32)
    first[order] = ~same_as_prev
    nxt = np.full(flat_in.shape, -1, dtype=np.int32)
    nxt[order[:-1]] = np.where(same_as_prev[1:], order[1:] + base, -1)
    return first, nxt


def batch_meta(batches, B, T, src_max_len, tgt_max_len, norm_count=None, width=None, frames=None, percentages=None, target_sizes=None,
               time_shift=CONV_TIME_SHIFT):
    """The host side of PassEngine.prepare_tasks (which documents the arguments) for the batches [(lengths, target)] of the tasks of one
    pass; src_max_len / tgt_max_len: rows of the positional tables; time_shift: the model's, see enc_extent (0: every frame is an encoder
    position, so klen_enc / keep_enc mask the batch's real padding).  -> dict with
      meta: the int32 block, fields in the order of `off`; its two seed words are left 0 for the caller to fill
      off: {field: word offset inside meta} for seed, inv_count, klen_enc, klen_dec, keep_enc, keep_dec, embed_first, embed_next,
           widths (None without per-task frames), ctc_in_len, ctc_tgt_len
      seq_in, seq_out: (nt * B, Td) int64 decoder input / gold ids, tasks concatenated
      Td, frames (normalised: None when every task fills T), n_nonpads, gold_hosts, ctc_in_len_host, ctc_tgt_len_host: per task."""
    nt = len(batches)
    T4 = enc_extent(T, time_shift)
    if frames is not None:
        frames = [int(f) for f in frames]
        if len(frames) != nt or max(frames) > T or enc_extent(min(frames), time_shift) < 1:
            raise ValueError('frames: one count per task, none above the padded width')
        if all(f == T for f in frames):
            frames = None
    ios = [decoder_io(target, width=width) for _lengths, target in batches]
    Td = max(io[0].shape[1] for io in ios)
    if nt > 1 and any(io[0].shape[1] != Td for io in ios):
        ios = [decoder_io(target, width=Td) for _lengths, target in batches]
    if T4 > src_max_len or Td > tgt_max_len:
        raise ValueError('sequence longer than the positional tables')
    pos = np.arange(T4)[None, :]
    dpos = np.arange(Td)[None, :]
    inv, klen_e, klen_d, keep_e, keep_d, firsts, nexts, n_nonpads = [], [], [], [], [], [], [], []
    ctc_in, ctc_tg = [], []
    for given in (percentages, target_sizes):
        if given is not None and len(given) != nt:
            raise ValueError('percentages / target_sizes: one entry per task')
    host = lambda v: v.detach().to('cpu').numpy() if torch.is_tensor(v) else np.asarray(v)
    for ti, ((lengths, _target), (seq_in_t, seq_out_t)) in enumerate(zip(batches, ios)):
        seq_in, seq_out = seq_in_t.numpy(), seq_out_t.numpy()
        if seq_in.shape[0] != B:
            raise ValueError('every task of a batched pass must bring %d samples' % B)
        lens = lengths.detach().to('cpu', torch.int64).numpy()
        n_lab = (seq_out != PAD_ID).sum(1) - 1                  # labels per utterance (seq_out = labels, EOS, PAD...)
        pct = host(percentages[ti]) if percentages is not None and percentages[ti] is not None else \
            (lens / float(max(int(lens.max()), 1))).astype(np.float32)
        sizes = host(target_sizes[ti]) if target_sizes is not None and target_sizes[ti] is not None else n_lab
        if pct.shape != (B,) or sizes.shape != (B,):
            raise ValueError('percentages / target_sizes: one value per sample')
        ctc_in.append(ctc_input_lengths(pct, int(n_lab.max()) + 1))
        ctc_tg.append(sizes.astype(np.int32))
        if frames is not None:
            lens = np.minimum(lens, enc_extent(frames[ti], time_shift))     # a position the task's own pass does not have is padding
        is_pad = seq_in == EOS_ID
        dec_len = (~is_pad).sum(1)
        if not bool((is_pad == (dpos >= dec_len[:, None])).all()):
            raise ValueError('EOS inside a target sequence is not supported')
        first, nxt = _occurrence_chains(seq_in.reshape(-1), ti * B * Td)   # row numbers of the whole pass; chains stay inside their task
        n_nonpad = int((seq_out != PAD_ID).sum())
        if norm_count is not None:        # this is a slice of a larger batch: normalise the loss by the WHOLE batch's token count
            n_nonpad = int(norm_count)
        n_nonpads.append(n_nonpad)
        inv.append(1.0 / n_nonpad)
        klen_e.append(np.minimum(lens, T4).astype(np.int32))               # (raw lengths)
        klen_d.append(dec_len.astype(np.int32))
        keep_e.append((pos < lens[:, None]).astype(np.int32).reshape(-1))
        keep_d.append((~is_pad).astype(np.int32).reshape(-1))
        firsts.append(first)
        nexts.append(nxt)
    # THE layout of the block: every field's word offset is where the concatenation below puts it
    fields = [('seed', [np.zeros(2, dtype=np.int32)]),                     # dropout seed of the pass: 8 bytes, 8-byte aligned
              ('inv_count', [np.asarray(inv, dtype=np.float32).view(np.int32),                 # 1 / n_nonpad (fp32 bits) per task
                             np.zeros(nt & 1, dtype=np.int32)]),                               # ... padded to an even word count
              ('klen_enc', klen_e), ('klen_dec', klen_d),                  # (nt B) each
              ('keep_enc', keep_e), ('keep_dec', keep_d),                  # (nt B T4), (nt B Td)
              ('embed_first', firsts), ('embed_next', nexts),              # (nt B Td) each
              ('widths', [np.asarray(frames, dtype=np.int32)] if frames is not None else []),
              ('ctc_in_len', ctc_in), ('ctc_tgt_len', ctc_tg)]             # (nt B) each, at the END of the block
    off, parts, words = {}, [], 0
    for name, arrays in fields:
        off[name] = words if arrays else None
        parts += arrays
        words += sum(int(a.shape[0]) for a in arrays)
    # (numpy from here to the upload: a torch CPU kernel on > 32768 elements -- the staging copy was one -- starts an OpenMP
    # region on torch's whole intra-op pool; in a CPU-quota'd container that stalls the enqueueing thread, hostenv.py)
    cat = lambda j: np.concatenate([io[j].numpy() for io in ios]) if nt > 1 else ios[0][j].numpy()
    return dict(meta=np.concatenate(parts), off=off, seq_in=cat(0), seq_out=cat(1), Td=Td, frames=frames, n_nonpads=n_nonpads,
                gold_hosts=[io[1] for io in ios], ctc_in_len_host=ctc_in, ctc_tgt_len_host=ctc_tg)
