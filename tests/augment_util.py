"""The tempo / gain augmentation restated in numpy and fp64: what `TempoGainAugment` and the kernels of csrc/mtl_tempo.hip are DEFINED to
compute (parity with sox unpinned: sox is no dependency and dithers).  Shared by tests/test_augment.py (CPU: the
restatement's own properties and the suitability of the inputs) and tests/test_augment_gpu.py (the device against it).  Nothing here
imports the package: the geometry, the lengths and the start positions are restated as well."""
import functools

import numpy as np

# (L, seed, tempo, gain_db, sample_rate): the `waveform` recipe of tests/test_frontend_batch_gpu.py snapped to the int16 grid
CASES = [
    (161, 10, 0.85, -6.0, 16000),       # one segment, zero-extended, no search
    (1547, 11, 0.937, 8.0, 16000),      # L = S + R, two segments, exact match at c = 188, clipping
    (4000, 12, 1.102, 3.3, 16000),
    (16037, 13, 0.9, -2.5, 16000),      # 16 segments
    (16037, 14, 1.15, 8.0, 16000),
    (9000, 15, 0.871, 5.123, 16000),
    (2240, 16, 1.0, 0.0, 16000),        # bypass, N = 2 H
    (4000, 17, 0.9, 0.0, 8000),         # at 8 kHz, 8 segments
]
MIN_MARGIN = 1e-6                       # every searched segment's best candidate beats the runner-up by at least this, relative
# (the samples are on the int16 grid, so a sum of O <= 256 squared differences -- multiples of 2^-30 below 2^10 -- is exact in fp64 in any
# order: the restatement's numpy sums and the kernel's index-order sums are the same numbers, and the margin guards nothing but the inputs)


def geometry(sample_rate):
    S = int(np.floor(sample_rate * 0.082 + 0.5))
    R = int(np.floor(sample_rate * 0.01468 + 0.5))
    O = max(int(np.floor(sample_rate * 0.012 + 4.5)), 16) // 8 * 8
    return S, R, O


def waveform(n, seed, rate=16000):
    """the recipe of tests/test_frontend_batch_gpu.py, snapped to the int16 grid (what a 16-bit wav file holds)"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    y = ((0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)) * np.linspace(0.2, 1.5, n)).astype(np.float32)
    return (np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def out_length(L, f):
    return int(L) if f == 1.0 else int(np.floor(L / f + 0.5))


def _read(x, start, n):
    """x[start : start + n] with zeros at and beyond len(x)"""
    out = np.zeros(n, dtype=np.float64)
    a, b = min(start, len(x)), min(start + n, len(x))
    out[:b - a] = x[a:b]
    return out


def wsola(x, f, sample_rate=16000):
    """-> dict(out float64 (N): the raw overlap-add, offsets int64 (M): o_m, margins float64 (M - 1): (runner-up - best) / runner-up of
    every searched segment (nan where best and runner-up are both exactly 0), tail / cur float64 (N): the two operands of every output sample (tail 0 where there is no cross-fade): the
    error bound of the fp32 expression is stated in them).  f == 1.0: the bypass, no segments."""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    S, R, O = geometry(sample_rate)
    H = S - O
    N = out_length(L, f)
    if f == 1.0:
        return dict(out=x.copy(), offsets=np.zeros(0, dtype=np.int64), margins=np.zeros(0), tail=np.zeros(N), cur=x.copy())
    M = -(-N // H)
    out, tails, curs = np.zeros(M * H), np.zeros(M * H), np.zeros(M * H)
    offsets, margins = np.zeros(M, dtype=np.int64), []
    fade = np.arange(O) / float(O)
    p_prev = o_prev = None
    for m in range(M):
        p = int(np.floor(f * float(m * H) + 0.5))
        if m == 0:
            o = R // 2
        else:
            tail = _read(x, p_prev + o_prev + H, O)
            window = _read(x, p, R + O)
            d = np.array([np.sum((tail - window[c:c + O]) ** 2) for c in range(R + 1)])
            o = int(np.argmin(d))                                   # (the first of equal minima: ties go to the smallest c)
            rest = np.delete(d, o)
            # a zero tail against candidates that are all zeros (the utterance has ended: segment 9 of the case of 9000 samples) is an
            # EXACT tie at 0 in any arithmetic, settled by the tie rule, not a near-tie: recorded as nan and left out of the margins
            margins.append((rest.min() - d[o]) / rest.min() if rest.min() > 0 else np.nan)
        seg = _read(x, p + o, H)
        curs[m * H:(m + 1) * H] = seg
        if m >= 1:
            tails[m * H:m * H + O] = tail
            seg = seg.copy()
            seg[:O] = tail + fade * (seg[:O] - tail)
        out[m * H:(m + 1) * H] = seg
        offsets[m] = o
        p_prev, o_prev = p, o
    return dict(out=out[:N], offsets=offsets, margins=np.array(margins), tail=tails[:N], cur=curs[:N])


def gain_quantize(t, gain_db):
    """-> int16 values (as int64): clip(rint(t g 32768), -32768, 32767), g = (float)10^(gain_db / 20)"""
    g = float(np.float32(10.0 ** (float(np.float32(gain_db)) / 20.0)))
    return np.clip(np.rint(np.asarray(t, dtype=np.float64) * g * 32768.0), -32768, 32767).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case, shared and left unchanged: dict(x float32, N, out, offsets, margins, tail, cur, q int64)"""
    L, seed, f, gain_db, rate = CASES[case]
    x = waveform(L, seed, rate)
    r = wsola(x, f, rate)
    assert len(r['out']) == out_length(L, f)
    assert all(m >= MIN_MARGIN for m in r['margins'] if not np.isnan(m)), (case, r['margins'])     # no choice is near a tie: the inputs are suitable
    r.update(x=x, N=len(r['out']), q=gain_quantize(r['out'], gain_db))
    return r
