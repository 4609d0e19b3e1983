"""Loss / CER / WER helpers with the reference's call signatures (utils/metrics.py:7-126), backed by the HIP cross-entropy kernels
and the C Levenshtein helper."""
import ctypes

import torch

from . import _lib
from .data import get_word_segments_per_language, is_contain_chinese_word

check = _lib.check


def calculate_cer(s1, s2):
    """utils/metrics.py:38-44 (python-Levenshtein replaced by mtl_levenshtein_u32)."""
    return _lib.levenshtein(s1, s2)


def calculate_wer(s1, s2):
    """utils/metrics.py:48-66: edit distance between the two sentences' word sequences (str.split()).  The words are numbered and
    the id sequences go to mtl_levenshtein_u32 as they are (the reference maps the ids to characters with chr() only because its
    Levenshtein package takes strings)."""
    w1, w2 = s1.split(), s2.split()
    ids = {}
    for w in w1 + w2:
        ids.setdefault(w, len(ids))
    arr = lambda ws: (ctypes.c_uint * max(len(ws), 1))(*[ids[w] for w in ws])
    a, b = arr(w1), arr(w2)
    d = _lib.lib().mtl_levenshtein_u32(ctypes.cast(a, ctypes.c_void_p), len(w1), ctypes.cast(b, ctypes.c_void_p), len(w2))
    if d < 0:
        raise RuntimeError('mtl_levenshtein_u32 failed: %d' % d)
    return d


def calculate_cer_en_zh(s1, s2):
    """utils/metrics.py:7-36: (hyp, gold) -> (English edit distance, Chinese edit distance, English gold characters, Chinese gold
    characters).  Both sentences are cut into word segments per language (get_word_segments_per_language); the segments holding a
    Chinese character are concatenated into the Chinese sequence, the others into the English one."""
    seqs = []
    for s in (s1, s2):
        en, zh = '', ''
        for segment in get_word_segments_per_language(s):
            if is_contain_chinese_word(segment):
                zh += segment
            else:
                en += segment
        seqs.append((en, zh))
    (en1, zh1), (en2, zh2) = seqs
    return calculate_cer(en1, en2), calculate_cer(zh1, zh2), len(en2), len(zh2)


class _CrossEntropyFn(torch.autograd.Function):
    """loss, hyp = CE(pred (B,T,V), gold (B,T)) on the device for ANY pred / gold pair (the model's own output, a slice of it,
    a re-used copy): forward = mtl_ce_argmax_fwd (utils/metrics.py:113-126 incl. label smoothing; lowest-index arg-max),
    backward = mtl_ce_bwd into d(pred), which autograd hands on to whatever produced `pred` (the HIP model's backward takes an
    external dpred).  Nothing here depends on the engine's last forward."""

    @staticmethod
    def forward(ctx, pred, gold, pad_id, smoothing):
        if pred.device.type != 'cuda':
            raise RuntimeError('calculate_metrics runs on the MI355X only (pred is on %s); there is no CPU fallback' % pred.device)
        if pred.dim() != 3 or pred.dtype != torch.float32:
            raise ValueError('pred must be (B, T, C) fp32')
        B, T, V = pred.shape
        p2 = pred.contiguous()
        g2 = gold.to(device=pred.device, dtype=torch.int64).contiguous().view(-1)
        rows = B * T
        n_nonpad = int((g2 != pad_id).sum().item())                  # the reference syncs here too (non_pad_mask.sum().item())
        if n_nonpad == 0:
            raise ValueError('cross entropy over a batch without a single non-PAD target')
        lib = _lib.lib()
        st = torch.cuda.current_stream(pred.device).cuda_stream
        lse = torch.empty(rows, dtype=torch.float32, device=pred.device)
        hyp = torch.empty(rows, dtype=torch.int64, device=pred.device)
        rowloss = torch.empty(rows, dtype=torch.float32, device=pred.device)
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        check(lib.mtl_ce_argmax_fwd(st, p2.data_ptr(), g2.data_ptr(), rows, V, V, int(pad_id), float(smoothing), n_nonpad, None,
                                    lse.data_ptr(), hyp.data_ptr(), rowloss.data_ptr(), loss.data_ptr()), 'mtl_ce_argmax_fwd')
        ctx.save_for_backward(p2, g2, lse)
        ctx.meta = (int(pad_id), float(smoothing), n_nonpad)
        hyp = hyp.view(B, T)
        ctx.mark_non_differentiable(hyp)
        return loss.reshape(()), hyp

    @staticmethod
    def backward(ctx, gout, _ghyp):
        p2, g2, lse = ctx.saved_tensors
        pad_id, smoothing, n_nonpad = ctx.meta
        B, T, V = p2.shape
        dpred = torch.empty_like(p2)
        g = gout.reshape(1).to(torch.float32).contiguous()
        st = torch.cuda.current_stream(p2.device).cuda_stream
        check(_lib.lib().mtl_ce_bwd(st, p2.data_ptr(), lse.data_ptr(), g2.data_ptr(), B * T, V, V, pad_id, smoothing,
                                    1.0 / n_nonpad, g.data_ptr(), dpred.data_ptr(), V), 'mtl_ce_bwd')
        return dpred, None, None, None


class _CTCFn(torch.autograd.Function):
    """loss = F.ctc_loss(log_softmax(pred (B,T,V)), gold (B,Lg), input_lengths, target_lengths, blank=pad_id, reduction='mean') on
    the device (utils/metrics.py:127-148): forward = mtl_ctc_fwd (row log-sum-exps and the alpha lattice), backward =
    mtl_ctc_bwd into d(pred).  An utterance without an alignment makes the loss +inf like torch (zero_infinity=False) but gets a
    zero gradient where torch writes NaN (its zero_infinity=True gradient); `nll` (B,) is reduction='none'."""

    @staticmethod
    def forward(ctx, pred, gold, in_len, tgt_len, pad_id, Lmax):
        if pred.device.type != 'cuda':
            raise RuntimeError('calculate_metrics runs on the MI355X only (pred is on %s); there is no CPU fallback' % pred.device)
        if pred.dim() != 3 or pred.dtype != torch.float32:
            raise ValueError('pred must be (B, T, C) fp32')
        B, T, V = pred.shape
        dev = pred.device
        p2 = pred.contiguous()
        g2 = gold.to(device=dev, dtype=torch.int64).contiguous()
        il = in_len.to(device=dev, dtype=torch.int32).contiguous()
        tl = tgt_len.to(device=dev, dtype=torch.int32).contiguous()
        ldg = int(g2.shape[1])                                                     # Lmax: the longest target (the lattice's width)
        lib = _lib.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = lib.mtl_ctc_workspace(B, T, Lmax)
        if ws_bytes < 0:
            raise ValueError('ctc: a target of %d labels is beyond the kernels\' limit' % Lmax)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.mtl_ctc_fwd(st, p2.data_ptr(), g2.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, V, V, ldg, Lmax,
                              int(pad_id), B, ws.data_ptr(), ws_bytes, nll.data_ptr(), loss.data_ptr()), 'mtl_ctc_fwd')
        ctx.save_for_backward(p2, g2, il, tl, ws, nll)
        ctx.meta = (int(pad_id), ldg, Lmax, ws_bytes)
        ctx.mark_non_differentiable(nll)
        return loss.reshape(()), nll

    @staticmethod
    def backward(ctx, gout, _gnll):
        p2, g2, il, tl, ws, nll = ctx.saved_tensors
        pad_id, ldg, Lmax, ws_bytes = ctx.meta
        B, T, V = p2.shape
        dpred = torch.empty_like(p2)
        g = gout.reshape(1).to(torch.float32).contiguous()
        st = torch.cuda.current_stream(p2.device).cuda_stream
        check(_lib.lib().mtl_ctc_bwd(st, p2.data_ptr(), g2.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, V, V, ldg, Lmax,
                                     pad_id, B, ws.data_ptr(), ws_bytes, nll.data_ptr(), 1.0, g.data_ptr(), dpred.data_ptr(), V),
              'mtl_ctc_bwd')
        return dpred, None, None, None, None, None


def _ctc_lengths(name, v, B, most, what):
    if v is None:
        raise ValueError("loss_type='ctc' needs %s" % name)
    v = torch.as_tensor(v)
    if v.dim() != 1 or v.shape[0] != B or v.dtype.is_floating_point or v.dtype == torch.bool:
        raise ValueError('%s must be %d integers, one per utterance' % (name, B))
    host = v.detach().to('cpu', torch.int64)
    if int(host.min()) < 0 or int(host.max()) > most:
        raise ValueError('%s must lie in [0, %d] (%s)' % (name, most, what))
    return v, int(host.max())


def calculate_metrics(pred, gold, pad_id, input_lengths=None, target_lengths=None, non_pad_mask=None, smoothing=0.0,
                      loss_type='ce'):
    """-> (loss tensor, num_correct) like utils/metrics.py:68-94 for loss_type='ce', (loss tensor, None) like :127-148 for 'ctc'.
    pred (B,T,C) fp32 and gold (B,T) on the device; `non_pad_mask` overrides gold.ne(pad_id) and, like the reference, pads
    `gold` IN PLACE where the mask is False.  `loss.backward()` produces d(pred) with mtl_ce_bwd / mtl_ctc_bwd and continues into
    the producer of `pred`.
    ctc: F.ctc_loss(log_softmax(pred), gold, input_lengths, target_lengths, blank=pad_id, reduction='mean'); utterance b uses the
    first target_lengths[b] entries of gold[b] and the first input_lengths[b] rows of pred[b] (both required, on any device).  A
    batch with an utterance that has no alignment returns +inf (as torch does; the reference prints "Found infinity loss") and that
    utterance's gradient rows are 0 instead of torch's NaN.  `smoothing` is ignored, as in the reference."""
    if loss_type not in ('ce', 'ctc'):
        raise NotImplementedError("loss_type must be 'ce' or 'ctc'")
    if non_pad_mask is None:
        non_pad_mask = gold.ne(pad_id)
    else:
        gold.masked_fill_(torch.logical_not(non_pad_mask), pad_id)
    if loss_type == 'ctc':
        if pred.dim() != 3 or gold.dim() != 2 or gold.shape[0] != pred.shape[0]:
            raise ValueError('ctc: pred must be (B, T, C) and gold (B, L)')
        B, T = int(pred.shape[0]), int(pred.shape[1])
        input_lengths, _ = _ctc_lengths('input_lengths', input_lengths, B, T, 'pred.size(1)')
        target_lengths, longest = _ctc_lengths('target_lengths', target_lengths, B, int(gold.shape[1]), 'gold.size(1)')
        loss, _nll = _CTCFn.apply(pred, gold, input_lengths, target_lengths, int(pad_id), max(longest, 1))
        return loss, None
    loss, hyp = _CrossEntropyFn.apply(pred, gold, pad_id, float(smoothing or 0.0))
    num_correct = int((hyp.eq(gold.to(hyp.device)) & non_pad_mask.to(hyp.device)).sum().item())
    return loss, num_correct
