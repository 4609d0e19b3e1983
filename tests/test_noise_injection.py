"""CPU: host side of the noise injection (NoiseInjection: file list, draw stream, placement, plan; the datasets' draw order).
Nothing here needs a device: the bank's device copy is made at first use."""
import argparse
import logging
import wave

import numpy as np
import pytest
import torch


def waveform(n, seed, rate=16000):
    """the recipe of tests/test_frontend_batch_gpu.py"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    return ((0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)) * np.linspace(0.2, 1.5, n)).astype(np.float32)


def write_wav(path, pcm, rate=16000, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def pcm16(y):
    return (np.clip(y, -1, 1) * 32767).astype('<i2')


@pytest.fixture()
def noise_dir(tmp_path):
    """three files of 3000, 5000 and 4096 + 1000 samples; the second in a sub-directory (the list is recursive and sorted)"""
    d = tmp_path / 'noise'
    (d / 'sub').mkdir(parents=True)
    write_wav(d / 'a.wav', pcm16(waveform(3000, 1)))
    write_wav(d / 'sub' / 'b.wav', pcm16(waveform(5000, 2)))
    write_wav(d / 'z.wav', pcm16(waveform(5096, 3)))
    return d


def test_draw_consumes_the_four_reference_draws(noise_dir):
    import mtl_amd
    inj = mtl_amd.NoiseInjection(str(noise_dir), 16000, (0.1, 0.4))
    assert inj.paths == sorted(inj.paths) and [p[len(str(noise_dir)) + 1:] for p in inj.paths] == ['a.wav', 'sub/b.wav', 'z.wav']
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    got, want = [], []
    for _ in range(40):
        got.append(inj.draw(a, 0.4))
        # utils/data_loader.py:73, :384, :385, :391 restated
        if b.binomial(1, 0.4):
            path = b.choice(inj.paths)
            level = b.uniform(0.1, 0.4)
            want.append((inj.paths.index(path), level, b.rand()))
        else:
            want.append(None)
    assert got == want
    assert a.rand() == b.rand()                                   # both generators in the same state
    assert any(d is None for d in got) and any(d is not None for d in got)
    assert all(0.1 <= d[1] < 0.4 and 0.0 <= d[2] < 1.0 for d in got if d is not None)
    # a string noise_prob (the reference's flag has no type)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    assert [inj.draw(a, '0.4') for _ in range(10)] == [inj.draw(b, 0.4) for _ in range(10)]


def test_place_and_plan(noise_dir, caplog):
    import mtl_amd
    inj = mtl_amd.NoiseInjection(str(noise_dir), 16000, (0.0, 0.5))
    assert inj.lengths.tolist() == [3000, 5000, 5096] and inj.offsets.tolist() == [0, 3000, 8000] and inj.bank_len == 13096
    assert inj.bank.dtype == np.int16 and np.array_equal(inj.bank[3000:8000], pcm16(waveform(5000, 2)))
    below_one = np.nextafter(1.0, 0.0)
    assert inj.place(None, 100) is None
    assert inj.place((1, 0.25, 0.0), 1000) == (3000, 0.25)                          # u = 0: start 0
    assert inj.place((1, 0.25, 0.5), 1000) == (3000 + 2000, 0.25)                   # floor(0.5 * 4000)
    # u just below 1: start = floor(u (N - n)) in fp64 is N - n - 1, the last start a draw can reach -- u (N - n) is exact or rounds to a
    # double BELOW the integer N - n (the spacing of doubles under an integer is at most half the distance u leaves), also when N - n
    # is a power of two (4096 here).  start = N - n, the segment that ends on the file's last sample, takes the closed end u = 1, which
    # rand() never returns and only an explicit argument of inject_noise_sample can supply; it is accepted and stays inside the file.
    assert inj.place((1, 0.25, below_one), 1000) == (3000 + 3999, 0.25)
    assert inj.place((2, 0.25, below_one), 1000) == (8000 + 4095, 0.25)
    off, _ = inj.place((2, 0.25, 1.0), 1000)
    assert off == 8000 + 4096 and off + 1000 == inj.bank_len
    assert inj.place((0, 0.1, 0.73), 3000) == (0, 0.1) and inj.place((0, 0.1, below_one), 3000) == (0, 0.1)      # N == n: start 0
    assert inj.skipped == 0
    with caplog.at_level(logging.WARNING):
        assert inj.place((0, 0.1, 0.5), 3001) is None                               # N < n: clean, counted, warned once per file
        assert inj.skipped == 1 and len(caplog.records) == 1 and 'a.wav' in caplog.records[0].getMessage()
        assert inj.place((0, 0.1, 0.2), 4000) is None
        assert inj.skipped == 2 and len(caplog.records) == 1
        assert inj.place((1, 0.1, 0.2), 6000) is None
        assert inj.skipped == 3 and len(caplog.records) == 2
    noise_off, level = inj.plan([(0, 0.5, 0.0), None, (1, 0.25, 0.5), (2, 0.125, 0.25), None], [1000, 2000, 1000, 1000, 500])
    assert noise_off.dtype == np.int64 and level.dtype == np.float32
    assert noise_off.tolist() == [0, -1, 3000 + 2000, 8000 + 1024, -1] and level.tolist() == [0.5, 0.0, 0.25, 0.125, 0.0]


def test_construction_checks(tmp_path):
    import mtl_amd
    with pytest.raises(IOError):
        mtl_amd.NoiseInjection(str(tmp_path / 'missing'))
    empty = tmp_path / 'empty'
    empty.mkdir()
    (empty / 'notes.txt').write_text('no audio here')
    with pytest.raises(ValueError, match='no \\*.wav'):
        mtl_amd.NoiseInjection(str(empty))
    for name, kw in (('rate8k', dict(rate=8000)), ('width8', dict(width=1))):
        d = tmp_path / name
        d.mkdir()
        write_wav(d / 'ok.wav', pcm16(waveform(500, 1)))
        pcm = pcm16(waveform(500, 2)) if 'rate' in kw else (128 + 100 * np.sin(np.arange(500))).astype(np.uint8)
        write_wav(d / 'wrong.wav', pcm, **kw)
        with pytest.raises(ValueError, match='wrong.wav'):
            mtl_amd.NoiseInjection(str(d))
    # stereo: the channel mean of load_wav_pcm16, back on the int16 grid
    d = tmp_path / 'stereo'
    d.mkdir()
    left, right = pcm16(waveform(700, 4)), pcm16(waveform(700, 5))
    write_wav(d / 's.wav', np.stack([left, right], axis=1), channels=2)
    inj = mtl_amd.NoiseInjection(str(d))
    assert inj.lengths.tolist() == [700]
    mean = mtl_amd.load_wav_pcm16(str(d / 's.wav'))
    assert np.array_equal(inj.bank, np.rint(mean * 32768.0).astype(np.int16))
    assert np.abs(inj.bank.astype(np.float64) - (left.astype(np.float64) + right) / 2).max() <= 0.5
    # the bank limit: 700 samples = 1400 bytes
    with pytest.raises(ValueError, match='bank_gb'):
        mtl_amd.NoiseInjection(str(d), bank_gb=1399.0 / 2 ** 30)
    assert mtl_amd.NoiseInjection(str(d), bank_gb=1400.0 / 2 ** 30).bank_len == 700


def _corpus(tmp_path, n=8):
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        write_wav(wp, pcm16(waveform(1600 + 160 * i, 40 + i)))
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


def _dataset(manifests, noise_dir, noise_prob=0.5, **kw):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=noise_prob,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                      is_train=True, **kw)


def test_dataset_with_noise_dir_constructs_without_a_device(tmp_path, noise_dir):
    import mtl_amd
    manifests = _corpus(tmp_path)
    for device_batches in (False, True):
        ds = _dataset(manifests, str(noise_dir), noise_prob='0.4', seed=7, device_batches=device_batches)
        assert isinstance(ds.noiseInjector, mtl_amd.NoiseInjection) and ds.noiseInjector._bank is None and ds.noise_prob == '0.4'
        assert ds._noise == (ds.noiseInjector, 0.4) and ds.noiseInjector.noise_levels == (0.0, 0.5)
    with pytest.raises(NotImplementedError):
        _dataset(manifests, str(noise_dir), seed=7, feature_fn=lambda p: torch.zeros(161, 3))
    with pytest.raises(IOError):
        _dataset(manifests, str(tmp_path / 'missing'), seed=7)
    with pytest.raises(NotImplementedError):                      # still outside the accelerated path
        _dataset(manifests, str(noise_dir), seed=7, augment=True)
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01)
    inj = mtl_amd.NoiseInjection(str(noise_dir))
    ds = mtl_amd.ManifestTaskDataset(mtl_amd.synthetic_vocab(64), args, manifests, device_batches=True, seed=1, noise=(inj, '0.25'))
    assert ds._noise == (inj, 0.25)
    with pytest.raises(NotImplementedError):
        mtl_amd.ManifestTaskDataset(mtl_amd.synthetic_vocab(64), args, manifests, feature_fn=lambda p: torch.zeros(161, 3), noise=(inj, 0.25))


class _StubFrontEnd:
    """stands in for SpectrogramFrontEnd on a machine without a device: records the noise plans `batch` is handed"""

    def __init__(self):
        self.plans = []

    def __call__(self, y):
        return torch.zeros(161, 1 + len(y) // 160)

    def batch(self, waves, max_frames=None, noise=None):
        frames = np.array([1 + len(w) // 160 for w in waves])
        if max_frames is not None:
            frames = np.minimum(frames, max_frames)
        self.plans.append(None if noise is None else (noise[1].tolist(), noise[2].tolist()))
        return torch.zeros(len(waves), 1, 161, int(frames.max())), torch.from_numpy(frames.astype(np.int32))


@pytest.mark.parametrize('device_batches', [False, True])
def test_a_part_that_is_not_loaded_consumes_its_draws(tmp_path, noise_dir, device_batches):
    manifests = _corpus(tmp_path)
    skipping = _dataset(manifests, str(noise_dir), seed=11, device_batches=device_batches)
    loading = _dataset(manifests, str(noise_dir), seed=11, device_batches=device_batches)
    mirror = np.random.RandomState(11)
    stub = _StubFrontEnd()
    skipping._fe_factory = loading._fe_factory = lambda: stub
    loading.feature_fn = lambda path: stub(np.zeros(1600))       # (the clean per-utterance path of device_batches=False)
    assert skipping.sample(3, 2, 0, need=(False, False)) == (None, None) and stub.plans == []
    tr, va = loading.sample(3, 2, 0, need=(True, True))
    assert tr[0].shape[0] == 3 and va[0].shape[0] == 2
    # the stream restated: the choice of the indices, then per utterance the reference's draws
    mirror.choice(np.arange(0, 8), 5, p=loading.proba[0], replace=True)
    inj = loading.noiseInjector
    draws = [inj.draw(mirror, 0.5) for _ in range(5)]
    assert any(d is None for d in draws) and any(d is not None for d in draws)
    state = mirror.rand()
    assert skipping.rng.rand() == state and loading.rng.rand() == state
    noisy = [d for d in draws if d is not None]
    if device_batches:                               # one call per part: a plan with offset -1 for its clean utterances, or -- all clean -- none
        assert len(stub.plans) == 2
        for plan, part in zip(stub.plans, (draws[:3], draws[3:])):
            if all(d is None for d in part):
                assert plan is None
            else:
                assert [o >= 0 for o in plan[0]] == [d is not None for d in part]
                assert plan[1] == [0.0 if d is None else float(np.float32(d[1])) for d in part]
    else:                                                            # one K = 1 call per noisy utterance
        assert len(stub.plans) == len(noisy) and [p[1] for p in stub.plans] == [[float(np.float32(d[1]))] for d in noisy]


def test_getitem_and_parse_audio_draw_like_the_reference(tmp_path, noise_dir):
    """every parse_audio injects (validation / test loaders too): one draw per item from the dataset's stream"""
    manifests = _corpus(tmp_path)
    ds = _dataset(manifests, str(noise_dir), noise_prob=0.5, seed=3)
    stub = _StubFrontEnd()
    ds._fe_factory = lambda: stub
    ds.feature_fn = lambda path: stub(np.zeros(1600))
    mirror = np.random.RandomState(3)
    want = [ds.noiseInjector.draw(mirror, 0.5) for _ in range(12)]
    for i in range(6):
        spect, transcript = ds[i]
        assert spect.shape[0] == 161 and len(transcript) > 0
    for i in range(6):
        assert ds.parse_audio(ds.ids_list[0][i][0]).shape[0] == 161
    assert ds.rng.rand() == mirror.rand()
    assert len(stub.plans) == sum(d is not None for d in want) > 0
