"""The DEFINITION of the log-mel filterbank features, in fp64 numpy: what logfbank(sig, rate, nfilt=80) of
python_speech_features computes with its defaults, restated.  Parity with the library is unpinned (it is not installed here); the
device front-end is pinned to this restatement.  `restate32` is the same chain in fp32 with the DFT as a matrix product: its error
against `restate` is the floor that an honest fp32 implementation reaches on a case, whatever its summation order.

Nothing here imports the package under test."""
import math

import numpy as np

EPS = 2.220446049250313e-16
NFFT = 512


def geometry(rate):
    fl, fs = int(math.floor(0.025 * rate + 0.5)), int(math.floor(0.01 * rate + 0.5))
    if fl > NFFT:
        raise ValueError('a 25 ms frame at %r Hz is longer than %d samples' % (rate, NFFT))
    return fl, fs, NFFT


def frames(L, rate):
    fl, fs, _ = geometry(rate)
    assert L >= 1
    return 1 if L <= fl else 1 + -((fl - L) // fs)


def mel_bins(nfilt, nfft, rate):
    m = np.linspace(2595.0 * np.log10(1.0 + 0.0 / 700.0), 2595.0 * np.log10(1.0 + (rate / 2.0) / 700.0), nfilt + 2)
    return np.floor((nfft + 1) * (700.0 * (10.0 ** (m / 2595.0) - 1.0)) / rate)


def mel_table(nfilt=80, nfft=NFFT, rate=16000):
    b = mel_bins(nfilt, nfft, rate)
    fb = np.zeros((nfilt, nfft // 2 + 1), dtype=np.float64)
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def _frame_matrix(p, rate):
    fl, fs, _ = geometry(rate)
    T = frames(p.shape[0], rate)
    padded = np.zeros((T - 1) * fs + fl, dtype=p.dtype)
    padded[:p.shape[0]] = p
    return np.stack([padded[t * fs:t * fs + fl] for t in range(T)])


def energies(x, rate=16000, nfilt=80):
    """x: float waveform, value pcm16 / 32768 -> the band energies E (nfilt, T) in fp64, before the zero rule and the logarithm"""
    s = 32768.0 * np.asarray(x, dtype=np.float64)
    p = s.copy()
    p[1:] = s[1:] - 0.97 * s[:-1]
    fr = _frame_matrix(p, rate)
    spec = np.fft.rfft(fr, NFFT, axis=1)
    P = (spec.real ** 2 + spec.imag ** 2) / NFFT
    return mel_table(nfilt, NFFT, rate) @ P.T


def log_energies(E):
    return np.log(np.where(E == 0, EPS, E))


def normalise(v):
    """(v - mean) / std over all values of the utterance, unbiased std (torch's .std())"""
    return (v - v.mean()) / v.std(ddof=1)


def restate(x, rate=16000, nfilt=80, normalize=False):
    v = log_energies(energies(x, rate, nfilt))
    return normalise(v) if normalize else v


def energies32(x, rate=16000, nfilt=80):
    """the same chain in fp32: scale, pre-emphasis, the DFT as an fp32 matrix product against the fp32-rounded table, power, bands"""
    fl, _, _ = geometry(rate)
    s = np.float32(32768.0) * np.asarray(x, dtype=np.float32)
    p = s.copy()
    p[1:] = s[1:] - np.float32(0.97) * s[:-1]
    fr = _frame_matrix(p, rate)
    ang = 2.0 * np.pi * np.arange(fl, dtype=np.float64)[:, None] * np.arange(NFFT // 2 + 1, dtype=np.float64)[None, :] / NFFT
    re, im = fr @ np.cos(ang).astype(np.float32), fr @ (-np.sin(ang)).astype(np.float32)
    P = (re * re + im * im) * np.float32(1.0 / NFFT)
    E = mel_table(nfilt, NFFT, rate).astype(np.float32) @ P.T
    assert E.dtype == np.float32
    return E


def restate32(x, rate=16000, nfilt=80, normalize=False):
    E = energies32(x, rate, nfilt)
    v = np.log(np.where(E == 0, np.float32(EPS), E)).astype(np.float32)
    if not normalize:
        return v
    d = v.astype(np.float64)                                  # statistics in fp64, as the issue asks of an implementation
    return ((v - np.float32(d.mean())) * np.float32(1.0 / d.std(ddof=1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ signals
def _pcm(y):
    """int16-valued float32 waveform, as load_wav_pcm16 returns it"""
    return (np.clip(np.rint(y), -32768, 32767) / 32768.0).astype(np.float32)


def signal(kind, L, seed, rate=16000):
    rng = np.random.RandomState(seed)
    if kind == 'noise':
        y = 3000.0 * rng.standard_normal(L)
    elif kind == 'tone':
        y = 8000.0 * np.sin(2.0 * np.pi * 440.0 * np.arange(L) / rate) + 30.0 * rng.standard_normal(L)
    elif kind == 'fade':
        y = 3000.0 * rng.standard_normal(L) * np.linspace(0.0, 1.0, L + 1)[1:]     # (from 0, but the first sample is not silent)
    elif kind == 'gap':                                       # 1200 samples of exact zeros in the middle: whole silent frames
        y = 3000.0 * rng.standard_normal(L)
        if L >= 2400:
            y[L // 2 - 600:L // 2 + 600] = 0.0
    else:
        raise ValueError(kind)
    return _pcm(y)


# ------------------------------------------------------------------------------------------------------------------ comparison
ILL = 2.0 ** -20          # an element whose fp64 energy is below this share of its frame's total band energy is ill-conditioned


def conditioning(E):
    """E fp64 (nfilt, T) -> (ill mask, frame totals): ill = 0 < E < ILL * total of its frame.  The exactly-zero energies (ln(eps)
    elements) are never ill: they are compared like every other element."""
    tot = E.sum(axis=0, keepdims=True)
    return (E > 0) & (E < ILL * tot), tot


def log_errors(v, E):
    """v: log energies of an implementation (nfilt, T), E: the fp64 energies -> (max log error over the well-conditioned elements,
    max |exp(v) - E| / frame total over the ill-conditioned ones, share of ill-conditioned elements)"""
    ill, tot = conditioning(E)
    ref = log_energies(E)
    d = np.abs(np.asarray(v, dtype=np.float64) - ref)
    well = float(d[~ill].max())
    rel = np.abs(np.exp(np.asarray(v, dtype=np.float64)) - E) / np.where(tot > 0, tot, 1.0)
    return well, (float(rel[ill].max()) if ill.any() else 0.0), float(ill.mean())


def norm_errors(n, E):
    """n: normalised features of an implementation, E: the fp64 energies -> max error over the well-conditioned elements against
    the fp64 normalisation.  The reference is fp64 throughout and normalised with its OWN values, every element in its mean and
    std; nothing of the implementation enters it.  Only the maximum leaves the ill-conditioned elements out.  Their logarithms,
    which fp32 cancellation moves by 0.01 to 40 in any fp32 implementation, still reach every element of `n` through the
    implementation's mean and std: that is part of what this figure measures, and why its floor is rougher than the log domain's
    (test_fbank_gpu.NORM_FACTOR)."""
    ill, _ = conditioning(E)
    d = np.abs(np.asarray(n, dtype=np.float64) - normalise(log_energies(E)))
    return float(d[~ill].max())
