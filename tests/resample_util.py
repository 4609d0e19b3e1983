"""The sample-rate conversion restated in numpy and fp64: the DEFINITION that the device is held to, parity with
sox unpinned.  Nothing here imports the package.

  ratio   g = gcd(r_in, r_out), up = r_out / g, down = r_in / g; L samples become N = ceil(L up / down); r_in == r_out is the bypass.
  taps    q = max(up, down), half = zeros q, n = -half .. half, fc = rolloff / q, h = fc sinc(fc n) kaiser(2 half + 1, beta), scaled so
          that sum(h) == up.
  output  y[j] = sum_i x[i] h[j down - i up + half] over 0 <= i < L with the tap index in [0, 2 half] (zero-phase, zero extension),
          summed in ascending i.
  file    clip(rint(y 32768), -32768, 32767) / 32768.
"""
import math

import numpy as np

MAX_RATIO = 1024
RATIOS = [(8000, 16000), (48000, 16000), (44100, 16000), (11025, 16000), (16000, 8000), (22050, 16000)]


def ratio(r_in, r_out):
    g = math.gcd(int(r_in), int(r_out))
    return int(r_out) // g, int(r_in) // g


def out_length(L, up, down):
    return -(-int(L) * up // down)


def taps(up, down, zeros=16, beta=8.6, rolloff=0.95):
    q = max(up, down)
    half = zeros * q
    n = np.arange(-half, half + 1).astype(np.float64)
    fc = rolloff / q
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
    return h * (up / h.sum())


def restate(x, up, down, h, js=None):
    """outputs `js` (default: all N) of x converted by up / down with the filter h -> (y fp64, sum_i |x[i]| |h[.]| fp64, terms int64): the
    terms of output j are i in [ceil((j down - half) / up), floor((j down + half) / up)] cut to [0, L), added in ascending i"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L, half = x.shape[0], (h.shape[0] - 1) // 2
    js = np.arange(out_length(L, up, down), dtype=np.int64) if js is None else np.asarray(js, dtype=np.int64)
    c = js * down
    i0 = np.where(c - half <= 0, 0, -(-(c - half) // up))
    i1 = np.minimum((c + half) // up, L - 1)
    terms = np.maximum(i1 - i0 + 1, 0)
    y, ab = np.zeros(js.shape[0]), np.zeros(js.shape[0])
    for m in range(int(terms.max()) if terms.size else 0):
        i = i0 + m
        ok = i <= i1
        i = np.where(ok, i, 0)
        p = np.where(ok, x[i] * h[np.where(ok, c + half - i * up, 0)], 0.0)
        y += p
        ab += np.abs(p)
    return y, ab, terms


def quantize(y):
    """the 16-bit file as int64 steps"""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int64)


def boundary_distance(y):
    """distance of y 32768 from the nearest rounding boundary (k + 1/2), in LSB"""
    v = np.asarray(y, dtype=np.float64) * 32768.0
    return np.abs(v - np.floor(v) - 0.5)


def waveform(n, seed, rate, level=0.3):
    """two tones and noise on the int16 grid, float32"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    y = level * (np.sin(2 * np.pi * 0.055 * rate * t + seed) + 0.5 * np.sin(2 * np.pi * 0.21 * rate * t)) + 0.05 * rng.standard_normal(n)
    return (np.clip(np.rint(y * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)
