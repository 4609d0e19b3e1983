"""CPU: batchmeta.batch_meta (the host side of PassEngine.prepare_tasks) against a per-element restatement in plain loops, every
field read by name at the word offset the function reports; and the ValueErrors of prepare_tasks with their messages."""
import numpy as np
import pytest
import torch

PAD, SOS, EOS = 0, 1, 2


def _bm():
    import importlib
    import mtl_amd                                              # noqa: F401
    return importlib.import_module('mtl_amd.batchmeta')


def restate(batches, B, T, norm_count=None, width=None, frames=None, percentages=None, target_sizes=None):
    """{field: list of python ints (fp32 fields as their bit patterns)} + seq_in / seq_out rows + Td, one sample and one position at a
    time: no sort, no concatenation"""
    nt, T4 = len(batches), (T // 2) // 2
    labels = [[[int(v) for v in row if int(v) != PAD] for row in target.tolist()] for _lengths, target in batches]
    own_Td = [max(len(r) for r in rows) + 1 for rows in labels]
    Td = max(own_Td + [int(width or 0)])
    out = dict(inv_count=[], klen_enc=[], klen_dec=[], keep_enc=[], keep_dec=[], embed_first=[], embed_next=[], ctc_in_len=[],
               ctc_tgt_len=[], seq_in=[], seq_out=[], Td=Td, n_nonpads=[])
    for t, ((lengths, _target), rows) in enumerate(zip(batches, labels)):
        lens = [int(v) for v in lengths.tolist()]
        n_nonpad = sum(len(r) + 1 for r in rows) if norm_count is None else int(norm_count)
        out['n_nonpads'].append(n_nonpad)
        out['inv_count'].append(int(np.float32(1.0 / n_nonpad).view(np.int32)))
        flat = []
        for b, r in enumerate(rows):
            own = lens[b] if frames is None else min(lens[b], (frames[t] // 2) // 2)
            out['klen_enc'].append(min(own, T4))
            out['klen_dec'].append(len(r) + 1)
            out['keep_enc'] += [1 if p < own else 0 for p in range(T4)]
            sin = [SOS] + r + [EOS] * (Td - 1 - len(r))
            out['keep_dec'] += [1 if v != EOS else 0 for v in sin]
            out['seq_in'].append(sin)
            out['seq_out'].append(r + [EOS] + [PAD] * (Td - 1 - len(r)))
            flat += sin
            pct = np.float32(lens[b] / float(max(max(lens), 1))) if percentages is None or percentages[t] is None \
                else np.float32(percentages[t][b])
            out['ctc_in_len'].append(int(pct * np.float32(own_Td[t])))           # the task's OWN width (fp32 product, truncated)
            out['ctc_tgt_len'].append(len(r) if target_sizes is None or target_sizes[t] is None else int(target_sizes[t][b]))
        for i, v in enumerate(flat):
            out['embed_first'].append(0 if v in flat[:i] else 1)
            later = [j for j in range(i + 1, len(flat)) if flat[j] == v]
            out['embed_next'].append(t * B * Td + later[0] if later else -1)
    if frames is not None and any(f != T for f in frames):
        out['widths'] = [int(f) for f in frames]
    return out


FIELDS = ('inv_count', 'klen_enc', 'klen_dec', 'keep_enc', 'keep_dec', 'embed_first', 'embed_next', 'ctc_in_len', 'ctc_tgt_len')


def compare(got, want, nt, B, T):
    meta, off, Td, T4 = got['meta'], got['off'], want['Td'], (T // 2) // 2
    assert meta.dtype == np.int32 and meta.ndim == 1 and got['Td'] == Td
    assert off['seed'] == 0 and off['inv_count'] == 2 and off['klen_enc'] == 2 + nt + (nt & 1)       # seed: 8 bytes, head: even words
    for name in FIELDS:
        n = len(want[name])
        assert meta[off[name]:off[name] + n].tolist() == want[name], name
    if 'widths' in want:
        assert meta[off['widths']:off['widths'] + nt].tolist() == want['widths'] and got['frames'] == want['widths']
    else:
        assert off['widths'] is None and got['frames'] is None
    assert off['ctc_tgt_len'] + nt * B == meta.shape[0]                                              # the CTC lengths end the block
    # the fields tile the block: sizes from the shapes alone
    sizes = dict(seed=2, inv_count=nt + (nt & 1), klen_enc=nt * B, klen_dec=nt * B, keep_enc=nt * B * T4, keep_dec=nt * B * Td,
                 embed_first=nt * B * Td, embed_next=nt * B * Td, widths=nt if 'widths' in want else 0, ctc_in_len=nt * B, ctc_tgt_len=nt * B)
    at = 0
    for name in ('seed', 'inv_count', 'klen_enc', 'klen_dec', 'keep_enc', 'keep_dec', 'embed_first', 'embed_next', 'widths', 'ctc_in_len',
                 'ctc_tgt_len'):
        if sizes[name]:
            assert off[name] == at, name
        at += sizes[name]
    assert at == meta.shape[0]
    assert got['seq_in'].dtype == np.int64 and got['seq_in'].tolist() == want['seq_in'] and got['seq_out'].tolist() == want['seq_out']
    assert got['n_nonpads'] == want['n_nonpads']
    assert [g.tolist() for g in got['gold_hosts']] == [want['seq_out'][t * B:(t + 1) * B] for t in range(nt)]
    assert [a.tolist() for a in got['ctc_in_len_host']] == [want['ctc_in_len'][t * B:(t + 1) * B] for t in range(nt)]
    assert [a.tolist() for a in got['ctc_tgt_len_host']] == [want['ctc_tgt_len'][t * B:(t + 1) * B] for t in range(nt)]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def test_one_task_with_repeated_ids():
    """B = 2, T = 8: two encoder positions; row 1 has no label after its first; id 5 repeats inside row 0 and across the rows"""
    bm = _bm()
    batches = [(_i32([2, 1]), torch.tensor([[5, 6, 5, 9], [5, 0, 0, 0]]))]
    want = restate(batches, 2, 8)
    got = bm.batch_meta(batches, 2, 8, 100, 100)
    compare(got, want, 1, 2, 8)
    Td = want['Td']
    assert Td == 5 and want['klen_dec'] == [5, 2] and want['keep_enc'] == [1, 1, 1, 0]
    # id 5 stands at flat positions 1, 3 and Td + 1: one chain of three that ends in -1; SOS: a chain of two; EOS: row 1's three pads
    assert want['embed_next'][1] == 3 and want['embed_next'][3] == Td + 1 and want['embed_next'][Td + 1] == -1
    assert want['embed_first'][1] == 1 and want['embed_first'][3] == 0 and want['embed_first'][Td + 1] == 0
    assert want['embed_next'][0] == Td and want['embed_next'][Td] == -1
    assert want['embed_next'][Td + 2:] == [Td + 3, Td + 4, -1]
    assert got['meta'][:2].tolist() == [0, 0]                                                        # the seed words are the caller's


def test_three_tasks_with_their_own_frames_and_widths():
    """an odd task count (one padding word in the head), decoder widths 4 / 6 / 2, frames 16 / 12 / 8 of T = 16: encoder lengths
    clipped to (frames // 2) // 2, the widths array present, chains numbered in the rows of the whole pass and closed per task"""
    bm = _bm()
    B, T, frames = 2, 16, [16, 12, 8]
    batches = [(_i32([4, 2]), torch.tensor([[7, 8, 7], [9, 0, 0]])),
               (_i32([4, 3]), torch.tensor([[7, 0, 8, 9, 10, 11], [8, 8, 0, 0, 0, 0]])),               # (a pad inside a row is dropped)
               (_i32([3, 1]), torch.tensor([[7], [8]]))]
    want = restate(batches, B, T, frames=frames)
    got = bm.batch_meta(batches, B, T, 100, 100, frames=frames)
    compare(got, want, 3, B, T)
    Td = want['Td']
    assert Td == 6 and got['off']['klen_enc'] == 6
    assert want['klen_enc'] == [4, 2, 3, 3, 2, 1] and want['widths'] == frames                       # 4 -> 3 and 3 -> 2: clipped
    nxt = got['meta'][got['off']['embed_next']:got['off']['embed_next'] + 3 * B * Td].tolist()
    for t in range(3):
        mine = nxt[t * B * Td:(t + 1) * B * Td]
        assert all(v == -1 or t * B * Td <= v < (t + 1) * B * Td for v in mine) and any(v > 0 for v in mine), t
    # frames given as tensors / numpy integers are normalised to python ints
    again = bm.batch_meta(batches, B, T, 100, 100, frames=[np.int64(f) for f in frames])
    assert again['frames'] == frames and np.array_equal(again['meta'], got['meta'])


def test_frames_that_all_fill_the_width_are_dropped():
    bm = _bm()
    batches = [(_i32([4, 2]), torch.tensor([[7, 8, 7], [9, 0, 0]])), (_i32([1, 4]), torch.tensor([[4, 4], [5, 0]]))]
    want = restate(batches, 2, 16, frames=[16, 16])
    got = bm.batch_meta(batches, 2, 16, 100, 100, frames=[16, 16])
    compare(got, want, 2, 2, 16)
    assert got['frames'] is None and got['off']['widths'] is None
    assert np.array_equal(got['meta'], bm.batch_meta(batches, 2, 16, 100, 100)['meta'])


def test_norm_count_and_given_ctc_lengths():
    """norm_count replaces every task's own count; task 0 brings percentages and target sizes, task 1 derives them; the CTC input
    lengths follow each task's OWN decoder width (3 and 5), not the pass's (7 with width=7)"""
    bm = _bm()
    B, T = 3, 12
    batches = [(_i32([3, 2, 1]), torch.tensor([[7, 8], [9, 0], [4, 5]])),
               (_i32([3, 3, 2]), torch.tensor([[7, 8, 9, 10], [8, 0, 0, 0], [6, 6, 6, 0]]))]
    pct = [torch.tensor([1.0, 0.7, 0.34]), None]
    sizes = [np.array([2, 1, 1]), None]
    want = restate(batches, B, T, norm_count=11, width=7, percentages=[[1.0, 0.7, 0.34], None], target_sizes=[[2, 1, 1], None])
    got = bm.batch_meta(batches, B, T, 100, 100, norm_count=11, width=7, percentages=pct, target_sizes=sizes)
    compare(got, want, 2, B, T)
    assert want['Td'] == 7 and got['n_nonpads'] == [11, 11]
    assert want['ctc_in_len'][:3] == [3, 2, 1] and want['ctc_tgt_len'] == [2, 1, 1, 4, 1, 3]           # int(0.7f * 3) = 2, int(0.34f * 3) = 1
    assert want['ctc_in_len'][3:] == [5, 5, 3]                                                       # lengths / 3 times the own width 5
    assert want['ctc_in_len'] != [int(np.float32(p) * np.float32(7)) for p in (1.0, 0.7, 0.34, 1.0, 1.0, 2 / 3)]


def test_rejected_batches_raise_what_prepare_tasks_raised():
    bm = _bm()
    ok = (_i32([4, 2]), torch.tensor([[7, 8, 7], [9, 0, 0]]))
    call = lambda batches=(ok, ok), B=2, T=16, src=100, tgt=100, **kw: bm.batch_meta(list(batches), B, T, src, tgt, **kw)
    call()
    for frames in ([16, 17], [16, 3], [16]):
        with pytest.raises(ValueError, match='^frames: one count per task, none above the padded width$'):
            call(frames=frames)
    for kw in (dict(percentages=[None]), dict(target_sizes=[None, None, None])):
        with pytest.raises(ValueError, match='^percentages / target_sizes: one entry per task$'):
            call(**kw)
    with pytest.raises(ValueError, match='^every task of a batched pass must bring 3 samples$'):
        call(B=3)
    for kw in (dict(percentages=[torch.ones(3), None]), dict(percentages=[torch.ones(2, 1), None]), dict(target_sizes=[None, np.ones(1)])):
        with pytest.raises(ValueError, match='^percentages / target_sizes: one value per sample$'):
            call(**kw)
    with pytest.raises(ValueError, match='^EOS inside a target sequence is not supported$'):
        call(batches=(ok, (_i32([4, 2]), torch.tensor([[7, EOS, 7], [9, 0, 0]]))))
    for kw in (dict(src=3), dict(tgt=3)):                     # T' = 4 encoder positions, 4 decoder positions
        with pytest.raises(ValueError, match='^sequence longer than the positional tables$'):
            call(**kw)
    call(src=4, tgt=4)
