"""MI355X: the stage pipeline of `BatchFrontEnd.batch` as a whole -- which library entry points a call issues and in which order for
every combination of the three optional stages, pinned staging that has to grow on a live front-end, and the log-mel filterbank
behind all three stages at once.  (What each stage computes is pinned by the tests of that stage.)"""
import itertools
import wave

import numpy as np
import pytest
import torch

from tests import resample_util as ru

pytestmark = pytest.mark.gpu

FRONT_ENDS = ('spectrogram', 'logfbank')


def _front_end(kind):
    import mtl_amd
    if kind == 'spectrogram':
        return mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=True)
    return mtl_amd.LogFBankFrontEnd(16000, 80, normalize=True)


@pytest.fixture(scope='module')
def inj(tmp_path_factory):
    """a noise bank of two files, 30000 and 40000 samples at 16 kHz"""
    import mtl_amd
    d = tmp_path_factory.mktemp('noise')
    for i, n in enumerate((30000, 40000)):
        with wave.open(str(d / ('n%d.wav' % i)), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.rint(ru.waveform(n, 70 + i, 16000)[::-1].astype(np.float64) * 32768.0).astype('<i2').tobytes())
    return mtl_amd.NoiseInjection(str(d), 16000, (0.1, 0.5))


def _plans(inj, lengths, rates, tempo, clean=()):
    """the keywords of a `batch` call with all three stages for utterances of `lengths` samples, the noise plan made for the converted
    and stretched lengths (every utterance noisy but those in `clean`) -> (dict(rates, augment, noise), the final lengths)"""
    import mtl_amd
    K = len(lengths)
    converted = mtl_amd.resample_plan(lengths, rates, 16000)[0]
    gain_db = np.linspace(-6.0, 8.0, K).astype(np.float32)
    final = [mtl_amd.TempoGainAugment.out_length(n, t) for n, t in zip(converted, tempo)]
    rng = np.random.RandomState(1)
    noise_off, level = inj.plan([inj.draw(rng, 1.0) for _ in range(K)], final)
    assert (noise_off >= 0).all()
    noise_off[list(clean)] = -1
    return dict(rates=list(rates), augment=(np.asarray(tempo, dtype=np.float64), gain_db), noise=(inj, noise_off, level)), final


# ------------------------------------------------------------------------------------------------------------------ call sequence
class _Recorder:
    """stands in front of the loaded library: records the name of every entry point that is called and forwards the call"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


STAGES = ('rates', 'augment', 'noise')
SUBSETS = [c for n in range(4) for c in itertools.combinations(STAGES, n)]


@pytest.mark.parametrize('kind', FRONT_ENDS)
@pytest.mark.parametrize('subset', SUBSETS, ids=['+'.join(s) or 'none' for s in SUBSETS])
def test_a_call_issues_exactly_the_entry_points_of_its_stages_in_order(monkeypatch, inj, kind, subset):
    import mtl_amd
    fe = _front_end(kind)
    waves = [ru.waveform(800, 3, 8000), ru.waveform(800, 4, 16000)]
    # the plans of the later stages are made for the lengths that the chosen earlier ones leave
    rates = [8000, 16000] if 'rates' in subset else [16000, 16000]
    tempo = [0.9, 1.1] if 'augment' in subset else [1.0, 1.0]
    kw, _ = _plans(inj, [800, 800], rates, tempo)
    kw = {k: kw[k] for k in subset}
    rec = _Recorder(mtl_amd._lib.lib())
    monkeypatch.setattr(mtl_amd._lib, 'lib', lambda: rec)
    inputs, sizes = fe.batch(waves, **kw)
    monkeypatch.undo()
    want = (['mtl_resample'] if 'rates' in subset else []) + (['mtl_tempo_search', 'mtl_tempo_render'] if 'augment' in subset else [])
    if kind == 'spectrogram':
        want += ['mtl_wave_mix_coef', 'mtl_spect_batch_noise'] if 'noise' in subset else ['mtl_spect_batch']
    else:
        want += (['mtl_wave_mix_coef', 'mtl_wave_mix'] if 'noise' in subset else []) + ['mtl_fbank_batch']
    assert [n for n in rec.names if not n.endswith('_workspace')] == want
    assert len([n for n in rec.names if n.endswith('_workspace')]) == 1 + ('noise' in subset)
    assert inputs.shape[:3] == (2, 1, fe.F) and inputs.shape[3] == int(sizes.max()) and bool(torch.isfinite(inputs).all())


# ------------------------------------------------------------------------------------------------------------------ staging regrowth
@pytest.mark.parametrize('kind', FRONT_ENDS)
def test_staging_that_grows_on_a_live_front_end_gives_the_bits_of_a_fresh_one(inj, kind):
    """every pinned buffer of `batch` starts at its minimum size in a small first call and has to grow in the second: more than 1 << 16
    samples, more than 64 utterances (so more than 128 entries of offsets with the segment prefix or the rate plan), and the 20481 taps
    of 11025 Hz -> 16 kHz (640 / 441), more than 1 << 12"""
    import mtl_amd
    small = [ru.waveform(800, 5, 16000)]
    K = 70
    cycle = (16000, 8000, 11025)
    rates = [cycle[k % 3] for k in range(K)]
    waves = [ru.waveform(1000, 10 + k, rates[k]) for k in range(K)]
    assert mtl_amd.resample_tables(waves[:3], rates[:3], 16000)['taps'].shape[0] > 1 << 12 and 1000 * K > 1 << 16
    tempo = [float('%.3f' % t) for t in np.linspace(0.85, 1.15, K)]
    assert 1.0 not in tempo
    kw, final = _plans(inj, [1000] * K, rates, tempo, clean=range(1, K, 2))
    live, fresh = _front_end(kind), _front_end(kind)
    first, first_sizes = live.batch(small)
    first = first.clone()
    a, sa = live.batch(waves, max_frames=12, **kw)
    b, sb = fresh.batch(waves, max_frames=12, **kw)
    assert sa.tolist() == sb.tolist() and max(sa.tolist()) == 12 and a.shape == b.shape == (K, 1, live.F, 12) and torch.equal(a, b)
    assert bool(torch.isfinite(a).all()) and len(set(final)) > 3
    again, again_sizes = live.batch(small)
    assert again_sizes.tolist() == first_sizes.tolist() and torch.equal(again, first)


def test_the_unfused_forms_take_utterances_without_samples():
    """nothing to upload: the library must still get a pointer that is not null, and nothing comes back"""
    import mtl_amd
    empty = [np.zeros(0, dtype=np.float32)]
    out = mtl_amd.resample(empty, [8000], 16000)
    assert len(out) == 1 and out[0].shape == (0,) and out[0].dtype == np.float32
    out, seg_off = mtl_amd.tempo_gain(empty, [0.9], [3.0], 16000)
    assert len(out) == 1 and out[0].shape == (0,) and seg_off.shape == (0,)
    # ... and next to an utterance that has samples
    y = ru.waveform(800, 6, 8000)
    both = mtl_amd.resample([empty[0], y], [8000, 8000], 16000)
    assert both[0].shape == (0,) and np.array_equal(both[1], mtl_amd.resample([y], [8000], 16000)[0])


# ------------------------------------------------------------------------------------------------------------------ all three, filterbank
def test_logfbank_with_all_three_stages_is_bitwise_batch_of_the_unfused_chain(inj):
    import mtl_amd
    L = mtl_amd._lib.lib()
    fb = _front_end('logfbank')
    rates = [8000, 16000, 8000]
    waves = [ru.waveform(n, 120 + j, r) for j, (n, r) in enumerate(zip((2100, 5000, 1700), rates))]
    kw, final = _plans(inj, [len(w) for w in waves], rates, [0.9, 1.0, 1.13], clean=[1])
    # the unfused chain: resample, tempo_gain, then mtl_wave_mix_coef + mtl_wave_mix on the packed waveforms
    stretched = mtl_amd.tempo_gain(mtl_amd.resample(waves, rates, 16000), *kw['augment'], 16000)[0]
    assert [len(s) for s in stretched] == final
    _, noise_off, level = kw['noise']
    offsets = np.concatenate([[0], np.cumsum(final)]).astype(np.int64)
    wav, off = torch.from_numpy(np.concatenate(stretched)).cuda(), torch.from_numpy(offsets).cuda()
    noff, lvl = torch.from_numpy(noise_off).cuda(), torch.from_numpy(level).cuda()
    bank, coef, out = inj.device_bank(), torch.empty(3, device='cuda'), torch.empty_like(wav)
    ws_bytes = L.mtl_wave_mix_coef_workspace(3)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert L.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), 3, bank.data_ptr(), inj.bank_len, noff.data_ptr(), lvl.data_ptr(),
                               coef.data_ptr(), ws.data_ptr(), ws_bytes) == 0
    assert L.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), 3, bank.data_ptr(), inj.bank_len, noff.data_ptr(), coef.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    mixed = [out.cpu().numpy()[offsets[k]:offsets[k + 1]] for k in range(3)]
    assert np.array_equal(mixed[1], stretched[1]) and not np.array_equal(mixed[0], stretched[0])
    for max_frames in (None, 20):
        a, sa = fb.batch(waves, max_frames=max_frames, **kw)
        b, sb = fb.batch(mixed, max_frames=max_frames)
        assert sa.tolist() == sb.tolist() and torch.equal(a, b)
    want = mtl_amd.fbank_frames(final, 16000).tolist()
    assert fb.batch(waves, **kw)[1].tolist() == want and sb.tolist() == [min(n, 20) for n in want]
    c, _ = fb.batch(stretched)
    a, _ = fb.batch(waves, **kw)
    assert not torch.equal(a, c) and torch.equal(a[1], c[1])                          # (the noise does matter; utterance 1 stays clean)
