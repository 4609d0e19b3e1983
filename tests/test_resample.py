"""CPU: host side of the sample-rate conversion (resample_plan, resample_taps, resample_tables, load_wav_pcm16_rate, the datasets'
constructor rules, draw stream and plans; the ABI surface) and the properties of the fp64 restatement in tests/resample_util.py that the
device is held to.  Nothing here needs a device."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import resample_util as ru


def write_wav(path, y, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.rint(np.asarray(y, dtype=np.float64) * 32768.0).astype('<i2').tobytes())


# ------------------------------------------------------------------------------------------------------------------ plan, taps, tables
def test_plan_lengths_bypass_and_the_ratio_limit():
    import mtl_amd
    n, up, down = mtl_amd.resample_plan([5, 161, 4001, 3000, 2000, 999, 4410, 4411], [22050, 8000, 48000, 44100, 11025, 16000, 44100, 44100],
                                        16000)
    assert n.dtype == up.dtype == down.dtype == np.int64
    assert up.tolist() == [320, 2, 1, 160, 640, 1, 160, 160] and down.tolist() == [441, 1, 3, 441, 441, 1, 441, 441]
    # ceil(L up / down): 5 * 320 / 441 = 3.63, 4001 / 3 = 1333.67, 3000 * 160 / 441 = 1088.4, 2000 * 640 / 441 = 2902.5; exact for 4410
    assert n.tolist() == [4, 322, 1334, 1089, 2903, 999, 1600, 1601]
    for L, r in ((1, 8000), (7, 48000), (12345, 44100), (441, 44100), (100, 16000)):
        u, d = ru.ratio(r, 16000)
        assert mtl_amd.resample_plan([L], [r], 16000)[0].tolist() == [ru.out_length(L, u, d)] == [int(np.ceil(L * u / d))]
    assert [a.tolist() for a in mtl_amd.resample_plan([77, 0], [8000, 8000], 8000)] == [[77, 0], [1, 1], [1, 1]]       # the bypass
    assert [a.tolist() for a in mtl_amd.resample_plan([100], [16000], 8000)] == [[50], [1], [2]]
    assert [a.tolist() for a in mtl_amd.resample_plan([2048], [131072], 16000)] == [[250], [125], [1024]]               # 1024 is covered
    for bad in (44101, 16001, 7999):
        with pytest.raises(ValueError, match='beyond the 1024'):
            mtl_amd.resample_plan([100], [bad], 16000)
    with pytest.raises(ValueError):
        mtl_amd.resample_plan([100, 100], [8000], 16000)
    with pytest.raises(ValueError):
        mtl_amd.resample_plan([100], [0], 16000)


@pytest.mark.parametrize('r_in,r_out', ru.RATIOS)
def test_taps_are_symmetric_sum_to_up_and_equal_the_restated_ones(r_in, r_out):
    import mtl_amd
    up, down = ru.ratio(r_in, r_out)
    h = mtl_amd.resample_taps(up, down)
    assert h.dtype == np.float64 and h.shape == (2 * 16 * max(up, down) + 1,)
    assert np.abs(h - h[::-1]).max() <= 4 * np.finfo(np.float64).eps * np.abs(h).max()
    assert abs(h.sum() - up) <= 1e-12 * up
    assert np.array_equal(h, ru.taps(up, down))
    assert h.argmax() == 16 * max(up, down)
    assert mtl_amd.resample_taps(up, down, zeros=4).shape == (2 * 4 * max(up, down) + 1,)


def test_tables_concatenate_the_distinct_filters_and_cache_them():
    import mtl_amd
    waves = [np.full(n, 0.25, dtype=np.float32) for n in (10, 20, 30, 40, 50)]
    tab = mtl_amd.resample_tables(waves, [8000, 16000, 48000, 8000, 48000], 16000)
    assert tab['flat'].dtype == np.float32 and tab['flat'].shape == (150,)
    assert tab['offsets'].tolist() == [0, 10, 30, 60, 100, 150] and tab['out_offsets'].tolist() == [0, 20, 40, 50, 130, 147]
    assert tab['plan'].dtype == np.int64 and tab['plan'].tolist() == [[2, 1, 32, 0], [1, 1, 0, 0], [1, 3, 48, 65], [2, 1, 32, 0], [1, 3, 48, 65]]
    assert tab['taps'].dtype == np.float64 and tab['taps'].shape == (65 + 97,)
    assert np.array_equal(tab['taps'][:65], ru.taps(2, 1)) and np.array_equal(tab['taps'][65:], ru.taps(1, 3))
    from mtl_amd import data
    assert data._RESAMPLE_TAPS[(2, 1)] is data._RESAMPLE_TAPS[(2, 1)] and not data._RESAMPLE_TAPS[(2, 1)].flags.writeable
    kept = data._RESAMPLE_TAPS[(1, 3)]
    mtl_amd.resample_tables(waves[:1], [48000], 16000)
    assert data._RESAMPLE_TAPS[(1, 3)] is kept                                       # formed once per ratio
    only = mtl_amd.resample_tables(waves[:2], [16000, 16000], 16000)               # all bypassed: a table that is never read, never empty
    assert only['taps'].shape == (1,) and only['plan'].tolist() == [[1, 1, 0, 0]] * 2 and only['out_offsets'].tolist() == [0, 10, 30]
    with pytest.raises(ValueError):
        mtl_amd.resample_tables([], [], 16000)
    with pytest.raises(ValueError):
        mtl_amd.resample_tables([np.zeros((2, 3), np.float32)], [8000], 16000)
    with pytest.raises(ValueError, match='beyond the 1024'):
        mtl_amd.resample_tables(waves[:1], [44101], 16000)


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('r_in,r_out', ru.RATIOS)
def test_restatement_agrees_with_scipy_resample_poly(r_in, r_out):
    from scipy.signal import resample_poly
    up, down = ru.ratio(r_in, r_out)
    h = ru.taps(up, down)
    for L in (1, 37, 1203):
        x = ru.waveform(L, 3 + L, r_in).astype(np.float64)
        y, ab, terms = ru.restate(x, up, down, h)
        ref = resample_poly(x, up, down, window=h / up)
        assert y.shape == ref.shape == (ru.out_length(L, up, down),)
        err = float(np.abs(y - ref).max())
        print('%d -> %d, L = %d: %d outputs, up to %d terms, max |restatement - scipy| = %.2e' % (r_in, r_out, L, len(y), terms.max(), err))
        assert err < 1e-12
        # a subset of the outputs is the same numbers
        js = np.array([0, len(y) // 2, len(y) - 1])
        assert np.array_equal(ru.restate(x, up, down, h, js)[0], y[js])


def test_restatement_reproduces_a_tone_and_removes_what_would_alias():
    n = np.arange(4000)
    y, _, _ = ru.restate(np.sin(2 * np.pi * 1000.0 * n / 8000.0), 2, 1, ru.taps(2, 1))
    want = np.sin(2 * np.pi * 1000.0 * np.arange(8000) / 16000.0)
    err = float(np.abs(y - want)[100:-100].max())
    n = np.arange(12000)
    z, _, _ = ru.restate(np.sin(2 * np.pi * 10000.0 * n / 48000.0), 1, 3, ru.taps(1, 3))
    residual = float(np.abs(z)[100:-100].max())
    print('1 kHz at 8 k -> 16 k: interior error %.2e; 10 kHz at 48 k -> 16 k: interior residual %.2e' % (err, residual))
    assert len(y) == 8000 and err < 1e-5
    assert len(z) == 4000 and residual < 1e-4
    # zero extension: the first output of an up-sampled utterance is x[0] h[half] alone plus nothing from before the start
    x = ru.waveform(50, 1, 8000).astype(np.float64)
    h = ru.taps(2, 1)
    assert ru.restate(x, 2, 1, h, [0])[2].tolist() == [17] and ru.restate(x, 2, 1, h, [40])[2].tolist() == [33]
    assert ru.quantize([0.5, -1.5, 1.0, 1.5 / 32768, 2.5 / 32768]).tolist() == [16384, -32768, 32767, 2, 2]


# ------------------------------------------------------------------------------------------------------------------ wav header
def test_load_wav_pcm16_rate_reads_the_header(tmp_path):
    import mtl_amd
    y = ru.waveform(300, 5, 8000)
    for rate in (8000, 16000, 44100):
        write_wav(tmp_path / 'a.wav', y, rate)
        got, r = mtl_amd.load_wav_pcm16_rate(str(tmp_path / 'a.wav'))
        assert r == rate and isinstance(r, int) and got.dtype == np.float32 and np.array_equal(got, y)
        assert np.array_equal(mtl_amd.load_wav_pcm16(str(tmp_path / 'a.wav')), y)      # (the rate-less loader is what it was)


# ------------------------------------------------------------------------------------------------------------------ datasets
def _corpus(tmp_path, n=8):
    """even utterances at 8 kHz, odd ones at 16 kHz"""
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        rate = 8000 if i % 2 == 0 else 16000
        write_wav(wp, ru.waveform((800 + 80 * i) * rate // 8000, 40 + i, rate), rate)
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


@pytest.fixture()
def noise_dir(tmp_path):
    d = tmp_path / 'noise'
    d.mkdir()
    write_wav(d / 'a.wav', ru.waveform(3000, 1, 16000))
    write_wav(d / 'b.wav', ru.waveform(5000, 2, 16000))
    return d


def _dataset(manifests, noise_dir=None, noise_prob=0.5, **kw):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=noise_prob,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                      is_train=True, **kw)


class _TodaysFrontEnd:
    """`batch` with the signature it had before rates existed: a call that hands it `rates` is a TypeError"""

    def __init__(self):
        self.calls = []

    def batch(self, waves, max_frames=None, noise=None, augment=None):
        self.calls.append(dict(lengths=[len(w) for w in waves], augment=None if augment is None else (augment[0].tolist(), augment[1].tolist()),
                               noise=None if noise is None else (noise[1].tolist(), noise[2].tolist()), max_frames=max_frames))
        return torch.zeros(len(waves), 1, 161, 7), torch.full((len(waves),), 7, dtype=torch.int32)

    def __call__(self, y):
        self.calls.append(dict(call=str(y)))
        return torch.zeros(161, 7)


class _RecordingFrontEnd(_TodaysFrontEnd):
    def batch(self, waves, max_frames=None, noise=None, augment=None, rates=None):
        out = super().batch(waves, max_frames, noise, augment)
        self.calls[-1]['rates'] = None if rates is None else [int(r) for r in rates]
        return out


def test_constructor_rules(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        _dataset(manifests, seed=7, resample=True, feature_fn=lambda p: torch.zeros(161, 3))
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01)
    vocab = mtl_amd.synthetic_vocab(64)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        mtl_amd.ManifestTaskDataset(vocab, args, manifests, feature_fn=lambda p: torch.zeros(161, 3), resample=True)
    for ds in (_dataset(manifests, seed=7, resample=True, device_batches=True), _dataset(manifests, seed=7, resample=True),
               mtl_amd.ManifestTaskDataset(vocab, args, manifests, device_batches=True, resample=True)):
        assert ds._resample is True and ds._rate == 16000
    for ds in (_dataset(manifests, seed=7), _dataset(manifests, seed=7, device_batches=True, resample=False),
               mtl_amd.ManifestTaskDataset(vocab, args, manifests, feature_fn=lambda p: torch.zeros(161, 3))):
        assert ds._resample is False
    # NoiseInjection keeps rejecting noise files at another rate
    d = tmp_path / 'noise8k'
    d.mkdir()
    write_wav(d / 'a.wav', ru.waveform(3000, 1, 8000), 8000)
    with pytest.raises(ValueError, match='no resampling here'):
        _dataset(manifests, str(d), seed=7, resample=True, device_batches=True)


@pytest.mark.parametrize('augment', [False, True])
def test_resample_off_is_todays_stream_picks_and_calls(tmp_path, noise_dir, augment):
    """resample=False: the same picks, the same draws and the same `batch` calls as a dataset built without the keyword -- `rates` is
    not even passed -- although the files' headers name two different rates"""
    manifests = _corpus(tmp_path)
    off = _dataset(manifests, str(noise_dir), seed=3, augment=augment, device_batches=True, resample=False)
    plain = _dataset(manifests, str(noise_dir), seed=3, augment=augment, device_batches=True)
    for ds in (off, plain):
        ds._fe_factory = _TodaysFrontEnd
        ds.feature_fn = lambda path, ds=ds: ds._front_end()(path)                   # (a clean utterance: recorded, no device needed)
        ds.sample(3, 2, 0)
        ds[1]
        ds.parse_audio(ds.ids_list[0][2][0])
    mirror = np.random.RandomState(3)
    picks = mirror.choice(np.arange(0, 8), 5, p=plain.proba[0], replace=True)
    lengths = [(800 + 80 * int(j)) * (1 if j % 2 == 0 else 2) for j in picks]         # the ORIGINAL lengths: nothing is converted
    assert [c['lengths'] for c in plain._fe.calls[:2]] == [lengths[:3], lengths[3:]]
    assert off._fe.calls == plain._fe.calls and len(off._fe.calls) >= 2
    assert off.rng.rand() == plain.rng.rand()


@pytest.mark.parametrize('augment', [False, True])
def test_plans_get_the_converted_lengths_and_batch_gets_the_rates(tmp_path, noise_dir, augment):
    import mtl_amd
    manifests = _corpus(tmp_path)
    ds = _dataset(manifests, str(noise_dir), noise_prob=1.0, seed=11, augment=augment, device_batches=True, resample=True)
    same_seed_off = _dataset(manifests, str(noise_dir), noise_prob=1.0, seed=11, augment=augment, device_batches=True)
    stub = _RecordingFrontEnd()
    ds._fe_factory = lambda: stub
    same_seed_off._fe_factory = _TodaysFrontEnd
    seen = dict(aug=[], noise=[])
    if augment:
        aug_plan = ds._augment.plan
        ds._augment.plan = lambda draws, lengths: (seen['aug'].append([int(n) for n in lengths]), aug_plan(draws, lengths))[1]
    noise_plan = ds.noiseInjector.plan
    ds.noiseInjector.plan = lambda draws, lengths: (seen['noise'].append([int(n) for n in lengths]), noise_plan(draws, lengths))[1]
    ds.sample(3, 2, 0)
    same_seed_off.sample(3, 2, 0)
    assert ds.rng.rand() == same_seed_off.rng.rand()                                # no draw is added
    mirror = np.random.RandomState(11)
    picks = [int(j) for j in mirror.choice(np.arange(0, 8), 5, p=ds.proba[0], replace=True)]
    assert any(j % 2 == 0 for j in picks) and any(j % 2 == 1 for j in picks)
    original = [(800 + 80 * j) * (1 if j % 2 == 0 else 2) for j in picks]
    rates = [8000 if j % 2 == 0 else 16000 for j in picks]
    converted = [(800 + 80 * j) * 2 for j in picks]                                  # 8 kHz doubles, 16 kHz stays
    assert len(stub.calls) == 2
    for call, sl in zip(stub.calls, (slice(0, 3), slice(3, 5))):
        assert call['lengths'] == original[sl] and call['rates'] == rates[sl] and call['max_frames'] == 50
    if augment:
        assert seen['aug'] == [converted[:3], converted[3:]]
        stretched = [mtl_amd.TempoGainAugment.out_length(n, t) for n, t in zip(converted, stub.calls[0]['augment'][0] + stub.calls[1]['augment'][0])]
        assert seen['noise'] == [stretched[:3], stretched[3:]]
    else:
        assert seen['aug'] == [] and seen['noise'] == [converted[:3], converted[3:]]
        assert all(c['augment'] is None for c in stub.calls)
    # the per-utterance path: an 8 kHz file goes through batch([y], rates=[8000]) and its noise segment is as long as the CONVERTED utterance
    del stub.calls[:], seen['noise'][:], seen['aug'][:]
    place = ds.noiseInjector.place
    placed = []
    ds.noiseInjector.place = lambda draw, n: (placed.append(int(n)), place(draw, n))[1]
    ds.parse_audio(ds.ids_list[0][2][0])
    assert len(stub.calls) == 1 and stub.calls[0]['lengths'] == [960] and stub.calls[0]['rates'] == [8000]
    want = 1920 if not augment else mtl_amd.TempoGainAugment.out_length(1920, stub.calls[0]['augment'][0][0])
    assert placed == [want]
    # ... a 16 kHz file takes the path it took before: no rates
    ds.parse_audio(ds.ids_list[0][1][0])
    assert stub.calls[1]['lengths'] == [1760] and stub.calls[1]['rates'] is None


def test_per_utterance_path_without_draws(tmp_path):
    """no injector, no augmentation, no device batches: the default feature function for a file at the target rate, one K = 1 batch with
    the rate for any other"""
    manifests = _corpus(tmp_path)
    ds = _dataset(manifests, seed=5, resample=True)
    stub = _RecordingFrontEnd()
    ds._fe = stub
    ds.feature_fn = lambda path: torch.full((161, 3), 2.0)
    a, _ = ds[0]                                                                     # u0: 8 kHz
    b, _ = ds[1]                                                                     # u1: 16 kHz
    assert stub.calls == [dict(lengths=[800], augment=None, noise=None, max_frames=None, rates=[8000])]
    assert a.shape == (161, 7) and b.shape == (161, 3)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_surface_lists_the_new_entry_point():
    import mtl_amd
    L = mtl_amd._lib.lib()
    assert 'mtl_resample' in mtl_amd._lib.SIGNATURES and L.mtl_cmdlist_opcode(b'mtl_resample') >= 0
    # bad arguments are rejected before any launch (no device needed)
    assert L.mtl_resample(None, None, None, None, None, None, 1, 1, 1, None) == -22
    buf = (np.zeros(8, dtype=np.float64)).ctypes.data
    assert L.mtl_resample(None, buf, buf, buf, buf, buf, 1, 0, 1, buf) == -22 and L.mtl_resample(None, buf, buf, buf, buf, buf, 0, 1, 1, buf) == -22
    assert L.mtl_resample(None, buf, buf, buf, buf, buf, 1, (1 << 20) + 1, 1, buf) == -22
    for name in ('resample', 'resample_plan', 'resample_taps', 'resample_tables', 'load_wav_pcm16_rate'):
        assert hasattr(mtl_amd, name)
    assert hasattr(mtl_amd.SpectrogramFrontEnd, 'resample')
