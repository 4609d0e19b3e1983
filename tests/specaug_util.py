"""SpecAugment restated in numpy and fp64: what `SpecAugment.plan` and the kernel of csrc/mtl_specaug.hip are DEFINED to compute (DESIGN.md
section 23; no reference implementation is a dependency).  Shared by tests/test_specaug.py (CPU: the restatement's own properties and the
host side) and tests/test_specaug_gpu.py (the device against it).  Nothing here imports the package: the plan is restated as well."""
import numpy as np

MAX_MASKS = 8
MAX_FRAMES = 16384


def n_draws(freq_masks, time_masks):
    return 2 + 2 * freq_masks + 2 * time_masks


def plan_row(u, tau, F, time_warp=40, freq_masks=2, freq_width=27, time_masks=2, time_width=40, time_ratio=0.2):
    """the uniforms of one utterance (u_c, u_d, (u_f, u_f0)..., (u_t, u_t0)...), its frame count and the feature rows -> the table row
    [tau, c, w, (f0, f)..., (t0, t)...] as a list of python ints; fp64 and floor"""
    u = [float(v) for v in u]
    assert len(u) == n_draws(freq_masks, time_masks)
    W, row = time_warp, [int(tau), 0, 0]
    if W >= 1 and tau >= 2 * W + 1:
        c = W + int(np.floor(u[0] * (tau - 2 * W)))
        row[1], row[2] = c, c + int(np.floor(u[1] * (2 * W - 1))) - (W - 1)
    at = 2
    for _ in range(freq_masks):
        f = int(np.floor(u[at] * (freq_width + 1)))
        row += [int(np.floor(u[at + 1] * (F - f + 1))), f]
        at += 2
    cap = min(time_width, int(np.floor(time_ratio * tau)))
    for _ in range(time_masks):
        t = int(np.floor(u[at] * (cap + 1)))
        row += [int(np.floor(u[at + 1] * (tau - t + 1))), t]
        at += 2
    return row


def plan(draws, frames, F, **policy):
    """K rows of uniforms and the K frame counts -> the int32 table (K, 3 + 2 freq_masks + 2 time_masks)"""
    return np.array([plan_row(u, int(tau), F, **policy) for u, tau in zip(draws, frames)], dtype=np.int32)


def warp_map(tau, c, w):
    """the source position of every output frame j in [0, tau): (i0 int64 (tau), a float32 (tau)); python integers throughout (exact),
    a = (float)((double)r / (double)den).  w == c gives the identity (i0 = j, a = 0), which the device does not even evaluate."""
    i0, a = np.zeros(tau, dtype=np.int64), np.zeros(tau, dtype=np.float32)
    for j in range(tau):
        if j < w:
            num, den, base = (2 * j + 1) * c - w, 2 * w, 0
        else:
            num, den, base = (2 * (j - w) + 1) * (tau - c) - (tau - w), 2 * (tau - w), c
        q = num // den                                             # python's // is the floor division
        r = num - q * den
        i, frac = base + q, np.float32(np.float64(r) / np.float64(den))
        if i < 0:
            i, frac = 0, np.float32(0.0)
        if i >= tau - 1:
            i, frac = tau - 1, np.float32(0.0)
        i0[j], a[j] = i, frac
    return i0, a


def apply(x, table, freq_masks, time_masks):
    """x (K, F, Tmax) float32 and the table -> dict(out float64 (K, F, Tmax): the restatement, the warped elements formed in fp64 from
    the fp32 inputs and the fp32 weight; masked bool: elements that a mask zeroes; exact bool: elements that must be BITWISE the input
    (a == 0 in a warped row, every element of a row that is not warped, everything at and beyond tau; masked ones excluded);
    src float32: for an exact element the input element it must equal bit for bit; scale float64: max(|x[i0]|, |x[i0 + 1]|) of every
    warped element with a != 0, else 0)"""
    x = np.asarray(x, dtype=np.float32)
    K, F, Tmax = x.shape
    table = np.asarray(table).reshape(K, 3 + 2 * freq_masks + 2 * time_masks)
    out, src = x.astype(np.float64), x.copy()
    masked, exact, scale = np.zeros(x.shape, dtype=bool), np.ones(x.shape, dtype=bool), np.zeros(x.shape)
    for k in range(K):
        tau, c, w = (int(v) for v in table[k, :3])
        assert 0 <= tau <= Tmax
        if w != c:
            assert 1 <= w <= tau - 1 and 0 <= c <= tau
            i0, a = warp_map(tau, c, w)
            i1 = np.minimum(i0 + 1, tau - 1)
            x0, x1 = x[k][:, i0].astype(np.float64), x[k][:, i1].astype(np.float64)
            lerp = a != 0
            out[k][:, :tau] = np.where(lerp[None, :], x0 + a.astype(np.float64)[None, :] * (x1 - x0), x0)
            src[k][:, :tau] = x[k][:, i0]
            exact[k][:, :tau] = ~lerp[None, :]
            scale[k][:, :tau] = np.where(lerp[None, :], np.maximum(np.abs(x0), np.abs(x1)), 0.0)
        for m in range(freq_masks):
            f0, f = (int(v) for v in table[k, 3 + 2 * m:5 + 2 * m])
            assert 0 <= f0 and 0 <= f and f0 + f <= F
            masked[k, f0:f0 + f, :tau] = True
        for m in range(time_masks):
            t0, t = (int(v) for v in table[k, 3 + 2 * freq_masks + 2 * m:5 + 2 * freq_masks + 2 * m])
            assert 0 <= t0 and 0 <= t and t0 + t <= tau
            masked[k, :, t0:t0 + t] = True
    out[masked] = 0.0
    exact &= ~masked
    scale[masked] = 0.0
    return dict(out=out, masked=masked, exact=exact, src=src, scale=scale)


BOUND = 2.0 ** -22     # of max(|x[i0]|, |x[i0 + 1]|): one rounding of the difference and one of the fmaf, each at most 2^-24 of a
#                        magnitude of at most 2 max, is below 1.5 * 2^-23 max


def check(got, x, table, freq_masks, time_masks):
    """the criteria that the device is held to: every masked element +0.0 bitwise, every exact element bitwise its input element, every
    other (warped, a != 0) element within BOUND * max(|x[i0]|, |x[i0 + 1]|) of the fp64 restatement -> dict of counts"""
    got = np.asarray(got, dtype=np.float32).reshape(np.asarray(x).shape)
    r = apply(x, table, freq_masks, time_masks)
    bits, zero = got.view(np.uint32), np.uint32(0)
    assert (bits[r['masked']] == zero).all(), 'a masked element is not +0.0'
    assert np.array_equal(bits[r['exact']], r['src'].view(np.uint32)[r['exact']]), 'an element that must be bitwise the input is not'
    warped = ~r['masked'] & ~r['exact']
    err = np.abs(got.astype(np.float64) - r['out'])[warped]
    worst = float((err / r['scale'][warped]).max()) if warped.any() and (r['scale'][warped] > 0).all() else 0.0
    assert (err <= BOUND * r['scale'][warped]).all(), 'a warped element is %.3g of its scale off the restatement (bound %.3g)' % (worst, BOUND)
    return dict(masked=int(r['masked'].sum()), exact=int(r['exact'].sum()), warped=int(warped.sum()), worst=worst)
