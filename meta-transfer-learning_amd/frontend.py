"""The audio front-end on the device: K waveforms in host memory -> one padded, normalised feature batch on the MI355X.

One pipeline (`BatchFrontEnd.batch`): up to three optional stages, always in this order -- rate conversion (`resample`), tempo and gain
(`tempo_gain`, `TempoGainAugment`), noise (`NoiseInjection`) -- and then the feature type's own launch: the spectrogram of
SpectrogramParser.parse_audio (`SpectrogramFrontEnd`, utils/data_loader.py:65-96) or the log-mel filterbank energies of
LogFBankDataset.parse_audio (`LogFBankFrontEnd`, utils/data_loader.py:145-155).  One more optional stage runs BEHIND that launch, on the
finished batch: `SpecAugment` (time warp, frequency and time masks).  A stage is a small object with a host part (pure
numpy: lengths and parameters -> tables and output lengths; the public `*_tables` / `*_plan` functions return exactly these tables)
and a device part (stage the tables, launch on a stream).  `data.py` holds the datasets that drive this; DESIGN.md sections 10-15 the
reasons.
"""
import logging
import os

import numpy as np
import torch


def _waveforms(waves, who):
    """K one-dimensional waveforms (numpy or tensors) -> (list of K float32 arrays, lengths int64 (K), offsets int64 (K + 1): the prefix
    sum of the lengths); `who` names the caller in the messages.  THE validator of every entry point that takes waveforms; a minimum
    length is a property of the feature type and is checked by the caller."""
    if len(waves) == 0:
        raise ValueError('%s: an empty list of waveforms' % who)
    arrs = []
    for i, w in enumerate(waves):
        a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError('%s: waveform %d is not one-dimensional (shape %s)' % (who, i, a.shape))
        arrs.append(a)
    lengths = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    return arrs, lengths, _prefix(lengths)


def _prefix(lengths):
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return offsets


def pack_waveforms(waves, hop, n_fft, max_frames=None):
    """K one-dimensional waveforms -> (flat float32 (sum of L_k), offsets int64 (K + 1), frames int32 (K), Tmax): the host side of
    `SpectrogramFrontEnd.batch`, pure numpy.  frames[k] = min(1 + L_k // hop, max_frames), Tmax = max(frames).  An utterance shorter
    than n_fft // 2 + 1 samples would need more than one reflection at its ends (numpy reflects repeatedly there): rejected."""
    arrs, lengths, offsets = _waveforms(waves, 'pack_waveforms')
    short = np.flatnonzero(lengths < n_fft // 2 + 1)
    if short.size:
        raise ValueError('pack_waveforms: utterance %d has %d samples, fewer than n_fft // 2 + 1 = %d (one reflection must suffice)'
                         % (short[0], lengths[short[0]], n_fft // 2 + 1))
    frames = _cut(1 + lengths // hop, max_frames)
    return np.concatenate(arrs), offsets, frames, int(frames.max())


def _cut(frames, max_frames):
    """frame counts cut to max_frames (None: as they are), int32"""
    return (frames if max_frames is None else np.minimum(frames, max_frames)).astype(np.int32)


class _Staging:
    """The pinned host buffers of one front-end, by name, grown on demand and never shrunk.  `upload` fills one from numpy arrays and
    issues ONE non-blocking copy into a new device tensor, which is allocated with the current stream: call it inside the stream
    context of the stream that the copy is to run on.  A buffer is reused by the next `upload` of its name, so the owner must have
    waited for the copy by then (`BatchFrontEnd.batch` waits on its event before it returns)."""

    def __init__(self):
        self._pin = {}

    def upload(self, name, parts, minimum, device):
        """`parts`: numpy arrays of one dtype that travel as one buffer, one after the other -> their device copy (flat).  `minimum`:
        the least number of elements that the pinned buffer is made with."""
        parts = [torch.from_numpy(p).reshape(-1) for p in parts]
        n, dtype = sum(p.numel() for p in parts), parts[0].dtype
        buf = self._pin.get(name)
        if buf is None or buf.numel() < n:
            buf = self._pin[name] = torch.empty(max(n, minimum), dtype=dtype).pin_memory()
        at = 0
        for p in parts:
            buf[at:at + p.numel()].copy_(p)
            at += p.numel()
        if n == 0:       # utterances without samples (`resample`, `tempo_gain`): one real element, an empty tensor's pointer is null
            return torch.zeros(1, dtype=dtype, device=device)
        dst = torch.empty(n, dtype=dtype, device=device)
        dst.copy_(buf[:n], non_blocking=True)
        return dst


def _run_stages(lib, stream, staging, device, stages, flat, offsets):
    """The device part of a stage list on `stream`, which must be the current one (every tensor made here belongs to its pool): upload
    the ORIGINAL samples, the FINAL offsets (those behind the last stage that changes lengths) and each stage's tables, then launch
    the stages in order.  A stage that changes lengths brings its own input offsets and writes at the offsets that the next such stage
    reads, the last one at the final offsets.  -> (the packed waveforms behind the last stage, the final offsets), on the device."""
    d_wav = staging.upload('wav', [flat], 1 << 16, device)
    d_off = staging.upload('off', [offsets], 64, device)
    for s in stages:
        s.upload(staging, device)
    for i, s in enumerate(stages):
        d_out = next((t.d_in for t in stages[i + 1:] if t.d_in is not None), d_off)
        d_wav = s.launch(lib, stream, d_wav, d_out, device)
    return d_wav, d_off


def _cuda(device, what):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('%s on the MI355X only (no CPU fallback)' % what)
    return dev


def _stage_alone(stage, arrs, dev):
    """one stage on the current stream of `dev` and the read-back: the unfused forms `resample` and `tempo_gain` -> list of K float32
    numpy arrays"""
    from . import _lib
    d_wav, _ = _run_stages(_lib.lib(), torch.cuda.current_stream(dev).cuda_stream, _Staging(), dev, [stage], np.concatenate(arrs),
                           stage.out_offsets)
    out, oo = d_wav.cpu().numpy(), stage.out_offsets
    return [out[oo[k]:oo[k + 1]].copy() for k in range(len(arrs))]


# ------------------------------------------------------------------------------------------------------------------
# Stage 1: sample-rate conversion (audio_with_sox / augment_audio_with_sox, utils/audio.py: `sox -r`); DESIGN.md section 14
# ------------------------------------------------------------------------------------------------------------------
RESAMPLE_MAX_RATIO = 1024
_RESAMPLE_TAPS = {}           # (up, down) -> the fp64 filter of `resample_taps` with its defaults (read-only arrays)


def resample_plan(lengths, rates, sample_rate):
    """K lengths and the K rates of their files -> (out_lengths, up, down), int64 (K) each: g = gcd(rate, sample_rate), up = sample_rate / g,
    down = rate / g, N = ceil(L up / down) in integers.  rate == sample_rate is the bypass (up = down = 1, N = L).  A ratio with
    max(up, down) > 1024 (44101 Hz to 16 kHz, say) raises ValueError: such a filter would have more than 32 k taps."""
    import math
    lengths = np.array(lengths, dtype=np.int64).reshape(-1)
    rates = np.array(rates).reshape(-1)
    if rates.shape != lengths.shape:
        raise ValueError('resample_plan: %d rates for %d waveforms' % (rates.shape[0], lengths.shape[0]))
    target = int(sample_rate)
    if target != sample_rate or target < 1:
        raise ValueError('resample_plan: the target rate must be a positive integer, got %r' % (sample_rate,))
    up, down = np.ones(len(lengths), dtype=np.int64), np.ones(len(lengths), dtype=np.int64)
    for k, r in enumerate(rates):
        if int(r) != r or int(r) < 1:
            raise ValueError('resample_plan: the rate of waveform %d must be a positive integer, got %r' % (k, r))
        g = math.gcd(int(r), target)
        up[k], down[k] = target // g, int(r) // g
        if max(up[k], down[k]) > RESAMPLE_MAX_RATIO:
            raise ValueError('resample_plan: %d Hz to %d Hz is the ratio %d / %d, beyond the %d that the conversion covers'
                             % (int(r), target, up[k], down[k], RESAMPLE_MAX_RATIO))
    return (lengths * up + down - 1) // down, up, down


def resample_taps(up, down, zeros=16, beta=8.6, rolloff=0.95):
    """the filter of the ratio up / down in fp64, 2 half + 1 taps: q = max(up, down), half = zeros q, n = -half .. half, fc = rolloff / q,
    h = fc sinc(fc n) kaiser(2 half + 1, beta), scaled so that sum(h) == up (unit gain at 0 Hz after the zero stuffing): `zeros` zero
    crossings of the sinc on either side, the cutoff at `rolloff` of the lower Nyquist frequency"""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError('resample_taps: up and down must be positive, got %d / %d' % (up, down))
    q = max(up, down)
    half = int(zeros) * q
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = float(rolloff) / q
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
    return h * (up / h.sum())


class _RateStage:
    """Utterance k from rates[k] to `sample_rate`.  Host part: `resample_tables` without the samples, from the K lengths alone.  Device
    part: the input offsets and the per-utterance plan in one buffer, the filters in another, then mtl_resample."""

    after = 'rate conversion'

    def __init__(self, lengths, rates, sample_rate, quantize=True):
        K, self.quantize = len(lengths), quantize
        self.out_lengths, up, down = resample_plan(lengths, rates, sample_rate)
        self.offsets, self.out_offsets = _prefix(lengths), _prefix(self.out_lengths)
        self.plan, base, filters, total = np.zeros((K, 4), dtype=np.int64), {}, [], 0
        for k in range(K):
            key = (int(up[k]), int(down[k]))
            self.plan[k, 0], self.plan[k, 1] = key
            if key[0] == key[1]:
                continue
            if key not in _RESAMPLE_TAPS:
                h = resample_taps(*key)
                h.setflags(write=False)
                _RESAMPLE_TAPS[key] = h
            if key not in base:
                base[key] = total
                filters.append(_RESAMPLE_TAPS[key])
                total += filters[-1].shape[0]
            self.plan[k, 2], self.plan[k, 3] = (_RESAMPLE_TAPS[key].shape[0] - 1) // 2, base[key]
        self.taps = np.concatenate(filters) if filters else np.zeros(1, dtype=np.float64)

    def tables(self):
        return dict(offsets=self.offsets, out_offsets=self.out_offsets, plan=self.plan, taps=self.taps)

    def upload(self, staging, device):
        K = self.plan.shape[0]
        d_tab = staging.upload('rate', [self.offsets, self.plan], 128, device)
        self.d_in, self.d_plan = d_tab[:K + 1], d_tab[K + 1:]
        self.d_taps = staging.upload('taps', [self.taps], 1 << 12, device)

    def launch(self, lib, stream, d_wav, d_out, device):
        """mtl_resample on `stream` (output allocated with the current stream) -> the converted packed waveforms"""
        from . import _lib
        total = int(self.out_offsets[-1])
        out = torch.empty(max(total, 1), dtype=torch.float32, device=device)
        _lib.check(lib.mtl_resample(stream, d_wav.data_ptr(), self.d_in.data_ptr(), d_out.data_ptr(), self.d_plan.data_ptr(),
                                    self.d_taps.data_ptr(), self.taps.shape[0], self.plan.shape[0], 1 if self.quantize else 0,
                                    out.data_ptr()), 'mtl_resample')
        return out[:total]


def resample_tables(waves, rates, sample_rate):
    """host side of the rate conversion, pure numpy: dict(flat float32 (sum of L_k), offsets int64 (K + 1), out_offsets int64 (K + 1) from
    `resample_plan`, plan int64 (K, 4): up, down, half and the base of the utterance's filter in taps, taps float64: the filters of the
    DISTINCT ratios of this call one after the other (a bypassed utterance has none: half = base = 0; never empty).  The filters are
    formed once per (up, down) and kept."""
    arrs, lengths, _ = _waveforms(waves, 'resample_tables')
    return dict(_RateStage(lengths, rates, sample_rate).tables(), flat=np.concatenate(arrs))


def resample(waves, rates, sample_rate=16000, quantize=True, device='cuda'):
    """K waveforms sampled at rates[k] converted to `sample_rate` on the device -> list of K float32 numpy arrays of
    ceil(L_k up_k / down_k) samples (`resample_plan`, `resample_taps` and DESIGN.md section 14 for the definition: a zero-phase
    Kaiser-windowed sinc with zero extension, fp64 sums; sox is not reproduced sample for sample).  quantize=True rounds to the 16-bit
    file that audio_with_sox leaves (without sox's dither), quantize=False returns the sums rounded once to fp32.  An utterance that is at
    `sample_rate` already is copied bit for bit either way.  The unfused form of `BatchFrontEnd.batch(rates=)`: the same stage, on the
    current stream."""
    dev = _cuda(device, 'sample rates are converted')
    arrs, lengths, _ = _waveforms(waves, 'resample_tables')
    return _stage_alone(_RateStage(lengths, rates, sample_rate, quantize), arrs, dev)


# ------------------------------------------------------------------------------------------------------------------
# Stage 2: tempo and gain (load_randomly_augmented_audio, utils/audio.py:35-61); DESIGN.md section 12
# ------------------------------------------------------------------------------------------------------------------
def wsola_geometry(sample_rate):
    """(segment S, search R, overlap O) in samples of the tempo change at `sample_rate`: 82 ms, 14.68 ms and 12 ms, the defaults that the
    documentation of sox's `tempo` effect gives, rounded as S = floor(sr 0.082 + 0.5), R = floor(sr 0.01468 + 0.5),
    O = max(floor(sr 0.012 + 4.5), 16) rounded down to a multiple of 8: (1312, 235, 192) at 16 kHz, (656, 117, 96) at 8 kHz."""
    S = int(np.floor(sample_rate * 0.082 + 0.5))
    R = int(np.floor(sample_rate * 0.01468 + 0.5))
    O = max(int(np.floor(sample_rate * 0.012 + 4.5)), 16) // 8 * 8
    return S, R, O


class TempoGainAugment(object):
    """load_randomly_augmented_audio (utils/audio.py:35-61) with the work on the device: a random tempo in `tempo_range` (pitch kept), then
    a random gain in `gain_range` dB, then the 16-bit file the reference reads back.  Pure numpy: the device part is
    `BatchFrontEnd.batch(augment=)` / `tempo_gain`.  The reference shells out to `sox`, which is no dependency of this project and dithers
    randomly when it writes 16 bits, so the behaviour is DEFINED by the restatement below, parity with sox unpinned (as with librosa in
    the front-end and `sox trim` in NoiseInjection); tests/augment_util.py holds it in numpy and fp64, DESIGN.md section 12 the reasons.

      draws       draw(rng): uniform(*tempo_range), then uniform(*gain_range) -- the reference's two draws, in its order; both reach sox
                  through "{:.3f}".format, so the values used are float('%.3f' % v).
      tempo f     WSOLA with `wsola_geometry(sample_rate)` = (S, R, O), H = S - O.  L samples become N = floor(L / f + 0.5) in
                  M = ceil(N / H) segments; segment m starts in the input at p_m = floor(f (m H) + 0.5) (fp64) shifted by o_m in [0, R]:
                  o_0 = R // 2, and for m >= 1 the c minimising sum_{i<O} (tail_{m-1}[i] - x[p_m + c + i])^2 over ALL R + 1 candidates
                  (fp64, the smallest c on a tie), tail_{m-1}[i] = x[p_{m-1} + o_{m-1} + H + i]; reads at or beyond L give 0.  Output
                  sample m H + i (i < H) is x[p_m + o_m + i], for m >= 1 and i < O cross-faded in fp32 as
                  tail_{m-1}[i] + (i / O) (x[p_m + o_m + i] - tail_{m-1}[i]).  f == 1.0 bypasses the effect (N = L, a copy), as sox does.
      gain, file  y = clip(rint(t g 32768), -32768, 32767) / 32768 with g = (float)10^(gain_db / 20) formed in fp64 and rounded once:
                  sox's 16-bit output without its dither, gain after tempo as in the reference's effect chain (+8 dB does clip)."""

    def __init__(self, tempo_range=(0.85, 1.15), gain_range=(-6, 8)):
        self.tempo_range, self.gain_range = tuple(tempo_range), tuple(gain_range)

    def draw(self, rng):
        """(tempo, gain_db), both rounded to three decimals: uniform(*tempo_range), then uniform(*gain_range), from `rng`"""
        tempo = rng.uniform(low=self.tempo_range[0], high=self.tempo_range[1])
        gain = rng.uniform(low=self.gain_range[0], high=self.gain_range[1])
        return float('{:.3f}'.format(tempo)), float('{:.3f}'.format(gain))

    @staticmethod
    def out_length(n_samples, tempo):
        """N = floor(L / tempo + 0.5); L itself for tempo == 1.0 (the bypass)"""
        if not tempo > 0.0:
            raise ValueError('TempoGainAugment: a tempo factor must be positive, got %r' % (tempo,))
        return int(n_samples) if tempo == 1.0 else int(np.floor(int(n_samples) / float(tempo) + 0.5))

    def plan(self, draws, lengths):
        """K draws and the K utterance lengths -> (tempo float64 (K), gain_db float32 (K), out_lengths int64 (K))"""
        tempo = np.array([d[0] for d in draws], dtype=np.float64)
        gain_db = np.array([d[1] for d in draws], dtype=np.float32)
        out_lengths = np.array([self.out_length(n, t) for n, t in zip(lengths, tempo)], dtype=np.int64)
        return tempo, gain_db, out_lengths


class _TempoGainStage:
    """Utterance k stretched to tempo[k] and amplified by gain_db[k].  Host part: `tempo_gain_tables` without the samples, from the K
    lengths alone (the lengths behind a rate conversion are known on the host, the samples exist on the device only).  Device part: the
    input offsets and the segment prefix in one buffer, the factors and the gains in one each, then mtl_tempo_search and
    mtl_tempo_render; `seg_off` keeps the searched offsets on the device."""

    after = 'tempo change'

    def __init__(self, lengths, tempo, gain_db, sample_rate, quantize=True):
        K, self.quantize = len(lengths), quantize
        self.tempo = np.ascontiguousarray(tempo, dtype=np.float64)
        gain_db = np.ascontiguousarray(gain_db, dtype=np.float32)
        if self.tempo.shape != (K,) or gain_db.shape != (K,):
            raise ValueError('tempo_gain_tables: %s tempo factors and %s gains for %d waveforms' % (self.tempo.shape, gain_db.shape, K))
        self.geometry = S, R, O = wsola_geometry(sample_rate)
        if R + 1 > 256 or O > 256:
            raise ValueError('tempo_gain_tables: a search of %d or an overlap of %d samples (sample rate %s) is beyond the 256 the kernel '
                             'covers' % (R, O, sample_rate))
        H = S - O
        lengths = np.array(lengths, dtype=np.int64)
        self.out_lengths = np.array([TempoGainAugment.out_length(n, t) for n, t in zip(lengths, self.tempo)], dtype=np.int64)
        self.offsets, self.out_offsets = _prefix(lengths), _prefix(self.out_lengths)
        self.seg_base = _prefix(np.where(self.tempo == 1.0, 0, (self.out_lengths + H - 1) // H))
        self.gain = (10.0 ** (gain_db.astype(np.float64) / 20.0)).astype(np.float32)

    def tables(self):
        return dict(offsets=self.offsets, out_offsets=self.out_offsets, seg_base=self.seg_base, tempo=self.tempo, gain=self.gain,
                    geometry=self.geometry)

    def upload(self, staging, device):
        K = self.tempo.shape[0]
        d_tab = staging.upload('tempo_off', [self.offsets, self.seg_base], 128, device)
        self.d_in, self.d_sbase = d_tab[:K + 1], d_tab[K + 1:]
        self.d_tempo = staging.upload('tempo', [self.tempo], 64, device)
        self.d_gain = staging.upload('gain', [self.gain], 64, device)

    def launch(self, lib, stream, d_wav, d_out, device):
        """mtl_tempo_search, then mtl_tempo_render on `stream` (outputs allocated with the current stream) -> the stretched packed
        waveforms"""
        from . import _lib
        K, (S, R, O), total, n_seg = self.tempo.shape[0], self.geometry, int(self.out_offsets[-1]), int(self.seg_base[-1])
        out = torch.empty(max(total, 1), dtype=torch.float32, device=device)
        seg_off = torch.empty(max(n_seg, 1), dtype=torch.int32, device=device)
        _lib.check(lib.mtl_tempo_search(stream, d_wav.data_ptr(), self.d_in.data_ptr(), d_out.data_ptr(), self.d_tempo.data_ptr(),
                                        self.d_sbase.data_ptr(), K, S, R, O, seg_off.data_ptr()), 'mtl_tempo_search')
        _lib.check(lib.mtl_tempo_render(stream, d_wav.data_ptr(), self.d_in.data_ptr(), d_out.data_ptr(), self.d_tempo.data_ptr(),
                                        self.d_gain.data_ptr(), self.d_sbase.data_ptr(), seg_off.data_ptr(), K, S, R, O,
                                        1 if self.quantize else 0, out.data_ptr()), 'mtl_tempo_render')
        self.seg_off = seg_off[:n_seg]
        return out[:total]


def tempo_gain_tables(waves, tempo, gain_db, sample_rate):
    """host side of the tempo / gain calls, pure numpy: dict(flat float32 (sum of L_k), offsets int64 (K + 1), out_offsets int64 (K + 1)
    from N_k = TempoGainAugment.out_length, seg_base int64 (K + 1): the prefix of the segments per utterance (ceil(N_k / H); none for
    tempo 1.0), tempo float64 (K), gain float32 (K): (float)10^(gain_db / 20), geometry (S, R, O))"""
    arrs, lengths, _ = _waveforms(waves, 'tempo_gain_tables')
    return dict(_TempoGainStage(lengths, tempo, gain_db, sample_rate).tables(), flat=np.concatenate(arrs))


def tempo_gain(waves, tempo, gain_db, sample_rate=16000, quantize=True, device='cuda'):
    """K waveforms stretched to tempo[k] and amplified by gain_db[k] on the device (TempoGainAugment for the semantics) ->
    (list of K float32 numpy arrays, seg_off int32 numpy: the offsets o_m of all segments, utterance after utterance; an utterance at
    tempo 1.0 has none).  quantize=False leaves out gain and the 16-bit rounding: the raw overlap-add.  The unfused form of
    `BatchFrontEnd.batch(augment=)`: the same stage, on the current stream."""
    dev = _cuda(device, 'tempo and gain are applied')
    arrs, lengths, _ = _waveforms(waves, 'tempo_gain_tables')
    stage = _TempoGainStage(lengths, tempo, gain_db, sample_rate, quantize)
    return _stage_alone(stage, arrs, dev), stage.seg_off.cpu().numpy()


def load_randomly_augmented_audio(path, sample_rate=16000, tempo_range=(0.85, 1.15), gain_range=(-6, 8)):
    """utils/audio.py:50-61 on the device: tempo and gain drawn from the global np.random like the reference, the utterance as float32
    numpy (16-bit PCM at `sample_rate`: no resampling here)"""
    from .data import load_wav_pcm16
    tempo, gain_db = TempoGainAugment(tempo_range, gain_range).draw(np.random)
    return tempo_gain([load_wav_pcm16(path)], [tempo], [gain_db], sample_rate)[0][0]


# ------------------------------------------------------------------------------------------------------------------
# Stage 3: noise (NoiseInjection.inject_noise_sample, utils/data_loader.py:383-399); DESIGN.md section 11
# ------------------------------------------------------------------------------------------------------------------
class _NoiseStage:
    """Utterance k mixed with the len(utterance k) samples of the injector's device-resident bank from noise_off[k] on at level[k]
    (noise_off[k] < 0: clean).  Host part: the checks of the plan (`NoiseInjection.plan`) against the K lengths and the bank.  Device
    part: the two tables in one buffer each, then mtl_wave_mix_coef; the mix itself belongs to the feature launch, which gets
    `mix` = (bank, bank_len, d_noff, coef).  Lengths and offsets are left as they are.  The bank is fetched at construction, outside
    the front-end's stream context: its one upload happens on the caller's stream, as `inject_noise_sample` would do it."""

    d_in = None                # (no offsets of its own: it reads and writes at the final ones)

    def __init__(self, lengths, noise, device):
        self.injector, noise_off, level = noise
        K = len(lengths)
        self.noise_off, self.level = np.ascontiguousarray(noise_off, dtype=np.int64), np.ascontiguousarray(level, dtype=np.float32)
        if self.noise_off.shape != (K,) or self.level.shape != (K,):
            raise ValueError('batch: the noise plan has %s offsets and %s levels for %d waveforms'
                             % (self.noise_off.shape, self.level.shape, K))
        if ((self.noise_off >= 0) & (self.noise_off + lengths > self.injector.bank_len)).any():
            raise ValueError('batch: a noise segment ends beyond the bank (%d samples)' % self.injector.bank_len)
        self.bank = self.injector.device_bank(device)

    def upload(self, staging, device):
        self.d_noff = staging.upload('noise_off', [self.noise_off], 64, device)
        self.d_level = staging.upload('noise_level', [self.level], 64, device)

    def launch(self, lib, stream, d_wav, d_off, device):
        from . import _lib
        K, bank_len = self.noise_off.shape[0], self.injector.bank_len
        ws_bytes = lib.mtl_wave_mix_coef_workspace(K)
        if ws_bytes < 0:
            raise RuntimeError('mtl_wave_mix_coef_workspace failed with code %d' % ws_bytes)
        coef = torch.empty(K, dtype=torch.float32, device=device)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
        _lib.check(lib.mtl_wave_mix_coef(stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.bank.data_ptr(), bank_len,
                                         self.d_noff.data_ptr(), self.d_level.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws_bytes),
                   'mtl_wave_mix_coef')
        self.mix = (self.bank, bank_len, self.d_noff, coef)
        return d_wav


class NoiseInjection(object):
    """utils/data_loader.py:367-399 with the mix on the device: `data += level * noise * rms(data) / rms(noise)`, `noise` being a
    segment of a randomly chosen noise file as long as the utterance.  The reference's constructor plus `device` and `bank_gb`;
    constructing needs no device (the device copy of the bank is made at first use and kept).  What the reference leaves to sox / soxi
    is pinned here:

      file list   `paths` = the sorted recursive list of *.wav under `path` (stands in for librosa.util.find_files).  Files are 16-bit
                  PCM at `sample_rate`; channels are averaged as load_wav_pcm16 does and rounded back to int16.  Any other sample width
                  or rate raises ValueError naming the file, a missing directory IOError (like the reference), an empty one ValueError,
                  a corpus of more than `bank_gb` GiB ValueError.  All files live in ONE int16 array (`bank`) with per-file
                  (`offsets`, `lengths`), in samples.
      draws       draw(rng, noise_prob): binomial(1, noise_prob) and, only when it gave 1, in this order choice(paths),
                  uniform(*noise_levels), rand() -- the reference's four draws (:73, :384-385, :391).
      placement   in samples: start = floor(u * (N_file - n)), segment [start, start + n) -- equal lengths by construction (the
                  reference hands seconds to `sox trim` and asserts the lengths afterwards).
      too long    an utterance longer than the chosen noise file stays clean (the reference would fail its assert): its draws are
                  consumed all the same, `skipped` is incremented and one logging.warning is issued per file.  A segment whose energy
                  is exactly zero leaves the utterance clean as well (the reference would produce inf / nan).
      arithmetic  S_d, S_n = sums of squares over the n samples in fp64, fixed order, no atomics; c = level * sqrt(S_d / n) /
                  sqrt(S_n / n) in fp64, rounded once to fp32; mixed = fmaf(c, noise, data) in fp32 with noise = (float)int16 / 32768
                  (exact).  Every kernel that mixes uses this one expression: fused and unfused paths agree bit for bit."""

    def __init__(self, path=None, sample_rate=16000, noise_levels=(0, 0.5), device='cuda', bank_gb=8.0):
        import glob
        import wave
        if path is None or not os.path.exists(path):
            print("Directory doesn't exist: {}".format(path))
            raise IOError("Directory doesn't exist: {}".format(path))
        self.paths = sorted(glob.glob(os.path.join(glob.escape(path), '**', '*.wav'), recursive=True))
        if not self.paths:
            raise ValueError('NoiseInjection: no *.wav file under %s' % path)
        self.sample_rate, self.noise_levels, self.device = sample_rate, tuple(noise_levels), torch.device(device)
        self.skipped, self._warned, self._bank = 0, set(), None
        lengths = []
        for p in self.paths:                                   # headers first: the bank limit is checked before anything is read
            with wave.open(p, 'rb') as w:
                if w.getsampwidth() != 2:
                    raise ValueError('NoiseInjection: %s has %d-byte samples, only 16-bit PCM is supported' % (p, w.getsampwidth()))
                if w.getframerate() != sample_rate:
                    raise ValueError('NoiseInjection: %s is sampled at %d Hz, the front-end at %d Hz (no resampling here)'
                                     % (p, w.getframerate(), sample_rate))
                lengths.append(w.getnframes())
        self.lengths = np.array(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.bank_len = int(self.lengths.sum())
        if self.bank_len == 0:
            raise ValueError('NoiseInjection: the *.wav files under %s hold no samples' % path)
        if 2 * self.bank_len > bank_gb * 2 ** 30:
            raise ValueError('NoiseInjection: the noise corpus under %s takes %.3f GiB as int16, more than bank_gb=%g'
                             % (path, 2 * self.bank_len / 2.0 ** 30, bank_gb))
        self.bank = np.empty(self.bank_len, dtype=np.int16)
        for p, o, n in zip(self.paths, self.offsets, self.lengths):
            with wave.open(p, 'rb') as w:
                ch = w.getnchannels()
                raw = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
            if ch > 1:                                         # load_wav_pcm16's channel mean (fp32), back on the int16 grid
                mean = (raw.astype(np.float32) / 32768.0).reshape(-1, ch).mean(axis=1).astype(np.float32)
                raw = np.clip(np.rint(mean * 32768.0), -32768, 32767).astype(np.int16)
            self.bank[o:o + n] = raw

    def device_bank(self, device=None):
        """the int16 bank on the device: uploaded at the first call and kept"""
        if self._bank is None:
            dev = torch.device(device) if device is not None else self.device
            if dev.type != 'cuda':
                raise RuntimeError('noise is mixed on the MI355X only (no CPU fallback)')
            self._bank = torch.from_numpy(self.bank).to(dev)
        return self._bank

    def draw(self, rng, noise_prob):
        """None (clean) | (file_index, level, u): binomial, then -- only if it gave 1 -- choice, uniform, rand, from `rng`"""
        if not rng.binomial(1, float(noise_prob)):
            return None
        path = rng.choice(self.paths)
        level = rng.uniform(*self.noise_levels)
        return self.paths.index(path), float(level), float(rng.rand())

    def place(self, draw, n_samples):
        """(bank_offset, level) of the segment [start, start + n_samples) of the drawn file, start = floor(u * (N_file - n_samples));
        None for a clean draw and for an utterance longer than the file (counted in `skipped`, one warning per file)"""
        if draw is None:
            return None
        fi, level, u = draw
        room = int(self.lengths[fi]) - int(n_samples)
        if room < 0:
            self.skipped += 1
            if fi not in self._warned:
                self._warned.add(fi)
                logging.warning('NoiseInjection: %s (%d samples) is shorter than an utterance of %d samples: such utterances stay clean',
                                self.paths[fi], int(self.lengths[fi]), int(n_samples))
            return None
        start = min(int(np.floor(u * room)), room)
        return int(self.offsets[fi]) + start, level

    def plan(self, draws, lengths):
        """K draws and the K utterance lengths -> (noise_off int64 (K), level float32 (K)); noise_off = -1 for a clean utterance"""
        noise_off, level = np.full(len(draws), -1, dtype=np.int64), np.zeros(len(draws), dtype=np.float32)
        for k, (d, n) in enumerate(zip(draws, lengths)):
            placed = self.place(d, n)
            if placed is not None:
                noise_off[k], level[k] = placed
        return noise_off, level

    def inject_noise(self, data):
        """utils/data_loader.py:383-386, draws from the global np.random like the reference"""
        noise_path = np.random.choice(self.paths)
        noise_level = np.random.uniform(*self.noise_levels)
        return self.inject_noise_sample(data, noise_path, noise_level)

    def inject_noise_sample(self, data, noise_path, noise_level, u=None):
        """utils/data_loader.py:388-399 on the device: mtl_wave_mix_coef and one mtl_wave_mix call with K = 1 -> the mixed waveform as
        float32 numpy (`data` itself is left alone).  u=None draws np.random.rand() as the reference does."""
        from . import _lib
        if u is None:
            u = np.random.rand()
        y = np.ascontiguousarray(data.detach().cpu() if torch.is_tensor(data) else data, dtype=np.float32).reshape(-1)
        placed = self.place((self.paths.index(str(noise_path)), float(noise_level), float(u)), y.shape[0])
        if placed is None or y.shape[0] == 0:
            return y.copy()
        lib, bank = _lib.lib(), self.device_bank()
        dev = bank.device
        wav = torch.from_numpy(y).to(dev)
        off = torch.tensor([0, y.shape[0]], dtype=torch.int64, device=dev)
        noff = torch.tensor([placed[0]], dtype=torch.int64, device=dev)
        lvl = torch.tensor([placed[1]], dtype=torch.float32, device=dev)
        coef, out = torch.empty(1, device=dev), torch.empty_like(wav)
        ws_bytes = lib.mtl_wave_mix_coef_workspace(1)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), 1, bank.data_ptr(), self.bank_len, noff.data_ptr(),
                                         lvl.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws_bytes), 'mtl_wave_mix_coef')
        _lib.check(lib.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), 1, bank.data_ptr(), self.bank_len, noff.data_ptr(),
                                    coef.data_ptr(), out.data_ptr()), 'mtl_wave_mix')
        return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# Stage 4, BEHIND the feature launch: SpecAugment (Park et al., 2019; not in the reference); DESIGN.md section 23
# ------------------------------------------------------------------------------------------------------------------
SPECAUG_MAX_MASKS = 8                      # MTL_SPECAUG_MAX_MASKS of include/mtl_hip.h: masks of either kind per utterance
SPECAUG_MAX_FRAMES = 16384                 # MTL_SPECAUG_MAX_FRAMES: the row of a warped utterance in 64 KB of LDS


class SpecPlan(np.ndarray):
    """the int32 table of `SpecAugment.plan`, (K, 3 + 2 freq_masks + 2 time_masks): an array that knows how its columns divide
    (`freq_masks`, `time_masks`); rows taken from it (`t[k:k + 1]`, `t[k]`) know it too"""

    def __new__(cls, table, freq_masks, time_masks):
        obj = np.ascontiguousarray(table, dtype=np.int32).view(cls)
        obj.freq_masks, obj.time_masks = int(freq_masks), int(time_masks)
        return obj

    def __array_finalize__(self, obj):
        self.freq_masks, self.time_masks = getattr(obj, 'freq_masks', None), getattr(obj, 'time_masks', None)


class SpecAugment(object):
    """SpecAugment (Park et al., 2019) on the device: a small time warp of the feature planes, then `freq_masks` frequency masks, then
    `time_masks` time masks.  Pure numpy: the device part is `BatchFrontEnd.batch(spec=)`, one launch of mtl_spec_augment behind the
    feature launch.  The reference has no such stage and no implementation is a dependency of this project, so the behaviour is DEFINED
    by the restatement below; tests/specaug_util.py holds it in numpy and fp64, DESIGN.md section 23 the reasons.

    The stage acts on the NORMALISED batch: the statistics are those of the clean utterance (a mask does not shift the mean of what is
    left), and the 0.0 that a mask writes IS the utterance mean -- the value the paper masks with.

      draws       draw(rng): rng.random_sample(2 + 2 freq_masks + 2 time_masks) -- warp (u_c, u_d), then (u_f, u_f0) per frequency mask,
                  then (u_t, u_t0) per time mask.  The number does not depend on the audio or on the widths (all ranks keep one stream);
                  time_warp=0 consumes its two warp draws all the same.
      plan        plan(draws, frames, F) -> int32 (K, 3 + 2 freq_masks + 2 time_masks): tau, c, w, (f0, f)..., (t0, t)...; tau is the
                  utterance's OWN frame count (frames[k], behind the cut to max_frames), not Tmax; fp64 and floor throughout, W = time_warp:
                    warp   iff W >= 1 and tau >= 2 W + 1: c = W + floor(u_c (tau - 2 W)), d = floor(u_d (2 W - 1)) - (W - 1), w = c + d
                           (1 <= w <= tau - 2); otherwise c = w = 0: no warp
                    freq   f = floor(u_f (freq_width + 1)), f0 = floor(u_f0 (F - f + 1))
                    time   t = floor(u_t (min(time_width, floor(time_ratio tau)) + 1)), t0 = floor(u_t0 (tau - t + 1))
      effect      on utterance k's plane x[F, Tmax], over columns [0, tau) only (the zero padding behind stays as it is, bit for bit),
                  in this order:
                    1. warp, when w != c, every row by the same map: source frame c lands on output frame w, linear on either side.
                       Output j < w: num = (2 j + 1) c - w, den = 2 w, base = 0; j >= w: num = (2 (j - w) + 1) (tau - c) - (tau - w),
                       den = 2 (tau - w), base = c; in integers q = floor(num / den), r = num - q den, i0 = base + q,
                       a = (float)((double)r / (double)den); i0 < 0: i0 = 0, a = 0; i0 >= tau - 1: i0 = tau - 1, a = 0;
                       out[j] = x[i0] when a == 0, else fmaf(a, x[i0 + 1] - x[i0], x[i0]) in fp32.  w == c leaves every bit alone.
                    2. rows [f0, f0 + f) become 0.0 over [0, tau)
                    3. frames [t0, t0 + t) become 0.0 in every row
                  Masks may overlap and may be empty."""

    def __init__(self, time_warp=40, freq_masks=2, freq_width=27, time_masks=2, time_width=40, time_ratio=0.2):
        for name, v in (('time_warp', time_warp), ('freq_masks', freq_masks), ('freq_width', freq_width), ('time_masks', time_masks),
                        ('time_width', time_width)):
            if int(v) != v or int(v) < 0:
                raise ValueError('SpecAugment: %s must be a non-negative integer, got %r' % (name, v))
        if int(freq_masks) > SPECAUG_MAX_MASKS or int(time_masks) > SPECAUG_MAX_MASKS:
            raise ValueError('SpecAugment: at most %d masks of either kind, got freq_masks=%d, time_masks=%d'
                             % (SPECAUG_MAX_MASKS, freq_masks, time_masks))
        if not 0.0 <= float(time_ratio) <= 1.0:
            raise ValueError('SpecAugment: time_ratio must lie in [0, 1], got %r' % (time_ratio,))
        self.time_warp, self.freq_masks, self.freq_width = int(time_warp), int(freq_masks), int(freq_width)
        self.time_masks, self.time_width, self.time_ratio = int(time_masks), int(time_width), float(time_ratio)

    @property
    def n_draws(self):
        return 2 + 2 * self.freq_masks + 2 * self.time_masks

    def draw(self, rng):
        """the n_draws uniforms of one utterance from `rng`, float64: (u_c, u_d), (u_f, u_f0)..., (u_t, u_t0)..."""
        return rng.random_sample(self.n_draws)

    def plan(self, draws, frames, F):
        """K draws, the K frame counts (the `input_sizes` of the batch, behind the cut to max_frames) and the feature rows F -> SpecPlan,
        int32 (K, 3 + 2 freq_masks + 2 time_masks): tau, c, w, (f0, f)..., (t0, t)..."""
        frames, F = np.array(frames, dtype=np.int64).reshape(-1), int(F)
        K, W, mF = len(frames), self.time_warp, self.freq_masks
        draws = np.array(draws, dtype=np.float64).reshape(K, -1)
        if draws.shape[1] != self.n_draws:
            raise ValueError('SpecAugment.plan: %d uniforms per utterance, this policy takes %d' % (draws.shape[1], self.n_draws))
        if self.freq_width > F:
            raise ValueError('SpecAugment.plan: freq_width=%d is more than the %d feature rows' % (self.freq_width, F))
        if (frames < 1).any():
            raise ValueError('SpecAugment.plan: an utterance without frames')
        if frames.max() > SPECAUG_MAX_FRAMES:
            raise ValueError('SpecAugment.plan: a batch of %d frames is beyond the %d that the kernel covers (a row in 64 KB of LDS)'
                             % (frames.max(), SPECAUG_MAX_FRAMES))
        table = np.zeros((K, 3 + self.n_draws - 2), dtype=np.int64)
        for k in range(K):
            tau, u = int(frames[k]), draws[k]
            table[k, 0] = tau
            if W >= 1 and tau >= 2 * W + 1:
                c = W + int(np.floor(u[0] * (tau - 2 * W)))
                table[k, 1], table[k, 2] = c, c + int(np.floor(u[1] * (2 * W - 1))) - (W - 1)
            for m in range(mF):
                f = int(np.floor(u[2 + 2 * m] * (self.freq_width + 1)))
                table[k, 3 + 2 * m], table[k, 4 + 2 * m] = int(np.floor(u[3 + 2 * m] * (F - f + 1))), f
            cap = min(self.time_width, int(np.floor(self.time_ratio * tau)))
            for m in range(self.time_masks):
                t = int(np.floor(u[2 + 2 * mF + 2 * m] * (cap + 1)))
                table[k, 3 + 2 * mF + 2 * m], table[k, 4 + 2 * mF + 2 * m] = int(np.floor(u[3 + 2 * mF + 2 * m] * (tau - t + 1))), t
        return SpecPlan(table, mF, self.time_masks)


class _SpecStage:
    """The SpecAugment table of a `batch` call.  Host part: the checks of the table against the K final frame counts.  Device part: the
    table in one pinned buffer, then mtl_spec_augment on the finished batch, in place."""

    def __init__(self, spec, frames):
        if isinstance(spec, tuple):
            spec = SpecPlan(*spec)
        mF, mT = getattr(spec, 'freq_masks', None), getattr(spec, 'time_masks', None)
        if mF is None or mT is None:
            raise ValueError('batch: spec= takes the table of SpecAugment.plan, or (table, freq_masks, time_masks)')
        self.table, self.freq_masks, self.time_masks = np.ascontiguousarray(spec, dtype=np.int32).reshape(-1, 3 + 2 * mF + 2 * mT), mF, mT
        if not (0 <= mF <= SPECAUG_MAX_MASKS and 0 <= mT <= SPECAUG_MAX_MASKS):
            raise ValueError('batch: at most %d masks of either kind, the spec table has %d and %d' % (SPECAUG_MAX_MASKS, mF, mT))
        if self.table.shape[0] != len(frames) or not np.array_equal(self.table[:, 0], frames):
            raise ValueError('batch: the spec table was made for the frame counts %s, the batch has %s (SpecAugment.plan takes the final '
                             'ones: behind rate conversion, tempo change and the cut to max_frames)'
                             % (self.table[:, 0].tolist(), np.asarray(frames).tolist()))
        if int(frames.max()) > SPECAUG_MAX_FRAMES:
            raise ValueError('batch: a batch of %d frames is beyond the %d that mtl_spec_augment covers' % (frames.max(), SPECAUG_MAX_FRAMES))

    def upload(self, staging, device):
        self.d_table = staging.upload('spec', [self.table], 256, device)

    def launch(self, lib, stream, inputs, K, F, tmax):
        from . import _lib
        _lib.check(lib.mtl_spec_augment(stream, inputs.data_ptr(), K, F, tmax, self.d_table.data_ptr(), self.freq_masks, self.time_masks),
                   'mtl_spec_augment')


# ------------------------------------------------------------------------------------------------------------------
# The pipeline, and the two feature types behind it
# ------------------------------------------------------------------------------------------------------------------
class BatchFrontEnd:
    """What the feature types share: the front-end's own stream, its pinned staging, the consumer stream and `batch`.  A feature type
    derives from this and supplies exactly four things:

      _min_samples                     the fewest samples an utterance may have in front of the feature launch
      _frame_counts(lengths)           int64 (K): the frames of utterances of these lengths, uncut
      _workspace_bytes(lib, lengths, K)  the bytes of fp64 workspace its launch needs
      _features_launch(...)            its last call(s) on `self.stream`: packed waveforms -> inputs

    and `F` (the feature rows), `_NAME` (in the messages) and its operands on `device`."""

    _NAME = None

    def __init__(self, sample_rate, normalize, device, consumer):
        """consumer: the stream on which the batches of `batch()` are read (default: the device's current stream at construction --
        the stream on which metastep._stage_inputs copies device-resident inputs into its static buffers)."""
        self.sample_rate, self.normalize, self.device = sample_rate, normalize, torch.device(device)
        self.consumer = consumer if consumer is not None or self.device.type != 'cuda' else torch.cuda.current_stream(self.device)
        self.stream = None                                     # batch()'s own stream, made at its first call
        self._staging = _Staging()                             # pinned staging of batch(), grown on demand

    def batch(self, waves, max_frames=None, noise=None, augment=None, rates=None, spec=None):
        """K waveforms -> (inputs (K, 1, F, Tmax) fp32 on the device, input_sizes (K) int32 on the host): what `collate` builds from
        K `__call__` results cut to max_frames, in one device pass -- one pinned staging copy of the concatenated samples and of the
        offsets (two H2D copies) and the feature type's launch (framing, transform, logarithm, per-utterance statistics over the WHOLE
        utterance, normalisation, zero padding).  With no optional stage only the workspace query and that one feature call are issued.

        Streams and lifetime: the front-end owns one stream.  `inputs` and every other device tensor are allocated with that stream
        current (their blocks belong to that stream's pool), the copies and launches run there, and the calling thread waits on an
        event recorded behind them: the batch is complete when this returns, whatever the training kernels queued on other streams
        are doing, and nothing here waits for them (no device-wide synchronisation).  `inputs.record_stream(consumer)` then tells the
        allocator that `consumer` reads the block: the trainer's host thread enqueues up to two iterations ahead, so the tensor is
        usually dropped while the trainer's copy of it is still pending -- without the record the next `batch` call could be handed
        the same memory and overwrite it under that copy.  The pinned staging buffers are reused by the next call only because every
        earlier call waited for its copies before it returned.

        The three optional stages run in this order, each on the packed waveforms that the one before left, on the same stream under
        the same event; input_sizes, Tmax and the feature type's minimum length refer to the lengths behind the last of them, and the
        plan of a later stage must have been made for the lengths behind the earlier ones (`resample_plan`, `TempoGainAugment.plan`):

        rates=K sample rates, those of the files that `waves` were read from (`load_wav_pcm16_rate`): utterance k is first converted
        from rates[k] to this front-end's sample rate as `resample` does -- ONE launch, mtl_resample, into a packed buffer of the
        converted waveforms at new offsets: the result is bitwise `batch(resample(waves, rates, sample_rate), ...)` with the same other
        arguments.  (Conversion first is this project's choice: the later stages are defined at the front-end's rate.  sox's own chain
        `tempo f gain g rate r` converts last.)  The original samples, the input offsets with the per-utterance plan and the filters
        travel through pinned staging.  No random draw is involved.  An utterance that is at the target rate already is copied bit for
        bit.

        augment=(tempo, gain_db), K values each (`TempoGainAugment.plan`): utterance k is stretched to tempo[k] and amplified by
        gain_db[k] as `tempo_gain` does -- mtl_tempo_search, then mtl_tempo_render into a packed buffer of the stretched waveforms at
        new offsets: the result is bitwise `batch(tempo_gain(waves, tempo, gain_db)[0], ...)`.  The offsets with the segment table's
        prefix, the factors and the gains travel through pinned staging like the noise tables.

        noise=(injector, noise_off, level), the output of `NoiseInjection.plan`: utterance k is mixed with as many samples of the
        injector's device-resident int16 bank as it has itself, from noise_off[k] on (noise_off[k] < 0: clean) at level[k], as
        NoiseInjection.inject_noise_sample does (utils/data_loader.py:383-399); the host does not touch the samples.  The two tables
        (K int64, K float32) travel through pinned staging like the offsets; the call is mtl_wave_mix_coef, and the feature launch
        mixes (the feature types say how).

        A fourth optional stage runs BEHIND the feature launch, on the finished batch, on the same stream under the same event:

        spec=the table of `SpecAugment.plan` (or (table, freq_masks, time_masks)), made for the K FINAL frame counts -- the input_sizes
        that this call returns, behind rate conversion, tempo change and the cut to max_frames: SpecAugment (time warp, frequency masks,
        time masks; `SpecAugment` for the definition) on the normalised (K, 1, F, Tmax) batch in place -- ONE launch, mtl_spec_augment.
        The result is `batch(waves, ...)` with the same other arguments put through that definition; columns at and beyond an
        utterance's own frame count stay the zeros they are.  The table (K int32 rows) travels through pinned staging like the other
        plans.  No random draw is involved here.  A batch of more than 16384 frames is refused (ValueError).

        Each of the four left at None issues exactly the calls of the others.  The library calls of one `batch`, in order, all on the
        front-end's stream: [mtl_resample], [mtl_tempo_search, mtl_tempo_render], [mtl_wave_mix_coef], then the feature launch --
        mtl_spect_batch, or mtl_spect_batch_noise behind a noise stage, for the spectrogram; [mtl_wave_mix behind a noise stage],
        mtl_fbank_batch for the filterbank (tests/test_frontend_pipeline_gpu.py holds every combination to this) -- and last
        [mtl_spec_augment] (tests/test_specaug_gpu.py)."""
        from . import _lib
        if self.device.type != 'cuda':
            raise RuntimeError('the %s front-end runs on the MI355X only (no CPU fallback)' % self._NAME)
        lib = _lib.lib()
        # 1. validate, build the stage list, fold the lengths through it: the samples that are uploaded are the original ones, everything
        #    downstream sees the converted / stretched lengths
        arrs, lengths, offsets = _waveforms(waves, 'batch')
        stages = []
        if rates is not None:
            stages.append(_RateStage(lengths, rates, self.sample_rate))
        if augment is not None:
            stages.append(_TempoGainStage(stages[-1].out_lengths if stages else lengths, augment[0], augment[1], self.sample_rate))
        if stages:
            lengths, offsets = stages[-1].out_lengths, stages[-1].out_offsets
        short = np.flatnonzero(lengths < self._min_samples)
        if short.size:
            raise ValueError('batch: utterance %d has %d samples after the %s, fewer than the %d that the %s front-end needs'
                             % (short[0], lengths[short[0]], stages[-1].after if stages else 'load', self._min_samples, self._NAME))
        if noise is not None:
            stages.append(_NoiseStage(lengths, noise, self.device))
        frames = _cut(self._frame_counts(lengths), max_frames)
        K, tmax = len(frames), int(frames.max())
        spec = None if spec is None else _SpecStage(spec, frames)
        ws_bytes = self._workspace_bytes(lib, lengths, K)
        if self.stream is None:
            self.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.stream):
            inputs = torch.empty(K, 1, self.F, tmax, device=self.device)
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
            # 2. stage everything, upload it and launch, in order
            if spec is not None:
                spec.upload(self._staging, self.device)
            d_wav, d_off = _run_stages(lib, self.stream.cuda_stream, self._staging, self.device, stages, np.concatenate(arrs), offsets)
            # 3. the feature launch, the stage behind it, the event, the wait and the record
            self._features_launch(lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, stages[-1].mix if noise is not None else None)
            if spec is not None:
                spec.launch(lib, self.stream.cuda_stream, inputs, K, self.F, tmax)
            done = torch.cuda.Event()
            done.record(self.stream)
        done.synchronize()                                     # host wait on this stream's event only
        inputs.record_stream(self.consumer)
        return inputs, torch.from_numpy(frames)

    def resample(self, waves, rates, quantize=True):
        """`resample` to this front-end's sample rate on its device: list of K converted float32 numpy arrays"""
        return resample(waves, rates, self.sample_rate, quantize, self.device)

    def tempo_gain(self, waves, tempo, gain_db, quantize=True):
        """`tempo_gain` at this front-end's sample rate and device: (list of K stretched float32 numpy arrays, seg_off)"""
        return tempo_gain(waves, tempo, gain_db, self.sample_rate, quantize, self.device)


class SpectrogramFrontEnd(BatchFrontEnd):
    """wav -> STFT (n_fft = win = sample_rate*window_size, hop = sample_rate*window_stride, symmetric Hamming window,
    center + reflect padding = librosa.stft defaults of the reference era) -> |.| -> log1p -> (x-mean)/std, all on the MI355X:
    the STFT is one fp32-MFMA GEMM (frames = overlapping rows of the padded waveform, lda = hop) against a windowed DFT basis.

    `batch` (BatchFrontEnd.batch) ends in the two launches of mtl_spect_batch (framing, STFT, log-magnitude, per-utterance statistics
    over the WHOLE utterance, normalisation, zero padding); input_sizes are 1 + L // hop, cut to max_frames.  An utterance needs
    n_fft // 2 + 1 samples: a shorter one would need more than one reflection at its ends (see `pack_waveforms`).  With noise= the last
    call is mtl_spect_batch_noise instead, which mixes while the samples are staged: no mixed waveform exists in memory."""

    _NAME = 'spectrogram'

    def __init__(self, sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming', normalize=True, device='cuda',
                 consumer=None):
        from scipy.signal import windows as sw
        super().__init__(sample_rate, normalize, device, consumer)
        self.n_fft = int(sample_rate * window_size)
        self.hop = int(sample_rate * window_stride)
        self.F = self.n_fft // 2 + 1
        self._min_samples = self.n_fft // 2 + 1                 # one reflection must suffice
        table = {'hamming': sw.hamming, 'hann': sw.hann, 'blackman': sw.blackman, 'bartlett': sw.bartlett}
        win = table[window](self.n_fft)                       # the reference passes the scipy FUNCTION -> symmetric window
        n = np.arange(self.n_fft)[:, None].astype(np.float64)
        f = np.arange(self.F)[None, :].astype(np.float64)
        ang = 2.0 * np.pi * n * f / self.n_fft
        self.ldb = (2 * self.F + 3) // 4 * 4
        basis = np.zeros((self.n_fft, self.ldb), dtype=np.float32)
        basis[:, :self.F] = (win[:, None] * np.cos(ang)).astype(np.float32)
        basis[:, self.F:2 * self.F] = (-win[:, None] * np.sin(ang)).astype(np.float32)
        self.basis = torch.from_numpy(basis).to(self.device)
        self.partials = torch.empty(512, dtype=torch.float64, device=self.device)

    def __call__(self, y):
        """y: 1-D float waveform (numpy or tensor) -> (F, T) fp32 tensor on the device, T = 1 + len(y) // hop."""
        from . import _lib
        if self.device.type != 'cuda':
            raise RuntimeError('the spectrogram front-end runs on the MI355X only (no CPU fallback)')
        lib = _lib.lib()
        y = np.asarray(y.detach().cpu() if torch.is_tensor(y) else y, dtype=np.float32).reshape(-1)
        pad = self.n_fft // 2
        yp = torch.from_numpy(np.pad(y, (pad, pad), mode='reflect')).to(self.device)
        T = 1 + y.shape[0] // self.hop
        reim = torch.empty(T, self.ldb, device=self.device)
        out = torch.empty(self.F, T, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.mtl_gemm_f32(st, 0, 0, T, 2 * self.F, self.n_fft, 1.0, yp.data_ptr(), self.hop, self.basis.data_ptr(), self.ldb,
                                    reim.data_ptr(), self.ldb, None, None, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, None, 0), 'stft gemm')
        _lib.check(lib.mtl_spect_logmag(st, reim.data_ptr(), self.ldb, T, self.F, out.data_ptr(), self.partials.data_ptr(),
                                        1 if self.normalize else 0), 'mtl_spect_logmag')
        return out

    def _frame_counts(self, lengths):
        return 1 + lengths // self.hop

    def _workspace_bytes(self, lib, lengths, K):
        ws_bytes = lib.mtl_spect_batch_workspace(int(self._frame_counts(lengths).sum()), K, self.F)
        if ws_bytes < 0:
            raise RuntimeError('mtl_spect_batch_workspace failed with code %d' % ws_bytes)
        return ws_bytes

    def _features_launch(self, lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, mix):
        """the last call of `batch` on its stream: packed waveforms -> inputs.  mix = (bank, bank_len, d_noff, coef) behind
        mtl_wave_mix_coef, or None for clean utterances"""
        from . import _lib
        if mix is None:
            _lib.check(lib.mtl_spect_batch(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.n_fft, self.hop,
                                           self.basis.data_ptr(), self.ldb, self.F, inputs.data_ptr(), tmax, 1 if self.normalize else 0,
                                           ws.data_ptr(), ws_bytes), 'mtl_spect_batch')
        else:
            bank, bank_len, d_noff, coef = mix
            _lib.check(lib.mtl_spect_batch_noise(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.n_fft, self.hop,
                                                 self.basis.data_ptr(), self.ldb, self.F, inputs.data_ptr(), tmax,
                                                 1 if self.normalize else 0, ws.data_ptr(), ws_bytes, bank.data_ptr(), bank_len,
                                                 d_noff.data_ptr(), coef.data_ptr()), 'mtl_spect_batch_noise')


# ------------------------------------------------------------------------------------------------------------------
# Log-mel filterbank front-end on the device (LogFBankDataset.parse_audio, utils/data_loader.py:145-155); DESIGN.md section 15
# ------------------------------------------------------------------------------------------------------------------
FBANK_EPS = 2.220446049250313e-16          # what an energy of exactly zero becomes before the logarithm


def fbank_geometry(rate):
    """(fl, fs, nfft) of the 25 ms / 10 ms framing at `rate`: fl = floor(0.025 R + 0.5), fs = floor(0.01 R + 0.5), nfft = 512 (400 / 160 at
    16 kHz, 200 / 80 at 8 kHz).  A rate whose frame is longer than the transform (R > 20480) raises ValueError: the library would cut the
    frames, and that is not reproduced."""
    import math
    fl, fs, nfft = int(math.floor(0.025 * rate + 0.5)), int(math.floor(0.01 * rate + 0.5)), 512
    if fl < 1 or fs < 1:
        raise ValueError('fbank_geometry: a sample rate of %r Hz has no 25 ms frame' % (rate,))
    if fl > nfft:
        raise ValueError('fbank_geometry: a 25 ms frame at %r Hz has %d samples, more than nfft = %d' % (rate, fl, nfft))
    return fl, fs, nfft


def fbank_frames(lengths, rate):
    """frames of utterances of `lengths` samples (each >= 1) at `rate`: 1 for L <= fl, else 1 + ceil((L - fl) / fs); int64 array"""
    fl, fs, _ = fbank_geometry(rate)
    lengths = np.array(lengths, dtype=np.int64).reshape(-1)
    if (lengths < 1).any():
        raise ValueError('fbank_frames: an utterance without samples')
    return np.where(lengths <= fl, 1, 1 + (lengths - fl + fs - 1) // fs).astype(np.int64)


def mel_filterbank(nfilt=80, nfft=512, rate=16000):
    """the dense (nfilt, nfft // 2 + 1) fp64 table of triangular mel bands: mel points linspace(mel(0), mel(R / 2), nfilt + 2) with
    mel(h) = 2595 log10(1 + h / 700), bins b[j] = floor((nfft + 1) hz(m_j) / R), band j rising over [b[j], b[j+1]) and falling over
    [b[j+1], b[j+2]).  At 16 kHz the bins begin 0, 0, 1, 2, 2, 3, so band 2 has no weight at all: kept, not repaired."""
    high = rate / 2.0
    m = np.linspace(2595.0 * np.log10(1.0 + 0.0 / 700.0), 2595.0 * np.log10(1.0 + high / 700.0), nfilt + 2)
    b = np.floor((nfft + 1) * (700.0 * (10.0 ** (m / 2595.0) - 1.0)) / rate)
    fb = np.zeros((nfilt, nfft // 2 + 1), dtype=np.float64)
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def mel_filterbank_sparse(fb):
    """dense table -> (band int32 (nfilt, 3): first bin, count, offset of the band's weights; weights float32, never empty): per band
    the range from its first to its last non-zero weight, rounded once to fp32.  A band without weight has count 0."""
    band, w = np.zeros((fb.shape[0], 3), dtype=np.int32), []
    for j in range(fb.shape[0]):
        nz = np.flatnonzero(fb[j])
        if nz.size:
            band[j] = nz[0], nz[-1] - nz[0] + 1, len(w)
            w.extend(fb[j, nz[0]:nz[-1] + 1])
    return band, np.array(w if w else [0.0], dtype=np.float32)


class LogFBankFrontEnd(BatchFrontEnd):
    """wav -> `nfilt` log mel filterbank energies per 25 ms frame every 10 ms (logfbank(sig, rate, nfilt=80) of python_speech_features
    with its defaults, restated in DESIGN.md section 15: scale to int16 values, pre-emphasis 0.97, rectangular 25 ms frames without
    centring, |DFT_512|^2 / 512, triangular mel bands, ln, energy 0 -> ln(2^-52)) -> (x - mean) / std over the utterance, all on the
    MI355X in the two launches of mtl_fbank_batch (staging with scaling and pre-emphasis, the 512-point DFT, power, bands, ln,
    per-utterance statistics over the WHOLE utterance, normalisation, zero padding).  No window, no STFT basis, no `partials`.

    `batch` (BatchFrontEnd.batch: streams, pinned staging, record_stream and the three optional stages, each of which leaves a packed
    waveform in front of the last call) -> (inputs (K, 1, nfilt, Tmax), input_sizes): input_sizes are `fbank_frames` of the lengths, cut
    to max_frames; an utterance needs one sample.  noise= is mtl_wave_mix_coef, then the UNFUSED mtl_wave_mix into a second packed
    buffer: the mix is not folded into this kernel's staging.  The result is bitwise `batch` of the waveforms that `resample`,
    `tempo_gain` and mtl_wave_mix give; frame counts and the one-sample minimum refer to the converted / stretched lengths."""

    _NAME = 'log-mel filterbank'
    _min_samples = 1

    def __init__(self, sample_rate=16000, nfilt=80, normalize=True, device='cuda', consumer=None):
        super().__init__(sample_rate, normalize, device, consumer)
        self.fl, self.fs, self.nfft = fbank_geometry(sample_rate)
        self.nfilt = self.F = int(nfilt)
        if self.nfilt < 1:
            raise ValueError('LogFBankFrontEnd: nfilt must be positive, got %r' % (nfilt,))
        nbins = self.nfft // 2 + 1
        ang = 2.0 * np.pi * np.arange(self.fl, dtype=np.float64)[:, None] * np.arange(nbins, dtype=np.float64)[None, :] / self.nfft
        self.ldb = (2 * nbins + 3) // 4 * 4
        basis = np.zeros((self.fl, self.ldb), dtype=np.float32)          # fp64, rounded once; only fl rows: the zero padding is free
        basis[:, :nbins] = np.cos(ang).astype(np.float32)
        basis[:, nbins:2 * nbins] = (-np.sin(ang)).astype(np.float32)
        self.filterbank = mel_filterbank(self.nfilt, self.nfft, sample_rate)
        band, w = mel_filterbank_sparse(self.filterbank)
        self.basis = torch.from_numpy(basis).to(self.device)
        self.band, self.band_w = torch.from_numpy(band).to(self.device), torch.from_numpy(w).to(self.device)

    def __call__(self, y):
        """y: 1-D float waveform (numpy or tensor, >= 1 sample) -> (nfilt, T) fp32 tensor on the device, T = fbank_frames([len(y)])"""
        return self.batch([y])[0][0, 0]

    def _frame_counts(self, lengths):
        return fbank_frames(lengths, self.sample_rate)

    def _workspace_bytes(self, lib, lengths, K):
        ws_bytes = lib.mtl_fbank_batch_workspace(K)
        if ws_bytes < 0:
            raise RuntimeError('mtl_fbank_batch_workspace failed with code %d' % ws_bytes)
        return ws_bytes

    def _features_launch(self, lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, mix):
        from . import _lib
        if mix is not None:                                    # the unfused mix: a packed buffer of the mixed waveforms, same offsets
            bank, bank_len, d_noff, coef = mix
            mixed = torch.empty_like(d_wav)
            _lib.check(lib.mtl_wave_mix(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, bank.data_ptr(), bank_len,
                                        d_noff.data_ptr(), coef.data_ptr(), mixed.data_ptr()), 'mtl_wave_mix')
            d_wav = mixed
        _lib.check(lib.mtl_fbank_batch(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.fl, self.fs, self.nfft,
                                       self.basis.data_ptr(), self.ldb, self.nfilt, self.band.data_ptr(), self.band_w.data_ptr(),
                                       self.band_w.numel(), inputs.data_ptr(), tmax, 1 if self.normalize else 0, ws.data_ptr(), ws_bytes),
                   'mtl_fbank_batch')
