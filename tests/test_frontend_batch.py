"""CPU: host side of the batched spectrogram front-end -- the pure-numpy packer and the `device_batches` switch of the datasets
(construction without a device, rejection of a feature_fn, an unchanged index stream)."""
import argparse
import wave

import numpy as np
import pytest
import torch


def test_pack_waveforms_offsets_frames_and_tmax():
    import mtl_amd
    for lengths, hop, n_fft in (([161, 480, 1121, 16037, 4000], 160, 320), ([81, 800, 1003], 80, 160)):
        rng = np.random.RandomState(len(lengths))
        waves = [rng.randn(n).astype(np.float32) for n in lengths]
        flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves, hop, n_fft)
        assert flat.dtype == np.float32 and offsets.dtype == np.int64 and frames.dtype == np.int32
        assert offsets.tolist() == [0] + list(np.cumsum(lengths)) and flat.shape == (sum(lengths),)
        assert frames.tolist() == [1 + n // hop for n in lengths] and tmax == max(1 + n // hop for n in lengths)
        for k, w in enumerate(waves):
            assert np.array_equal(flat[offsets[k]:offsets[k + 1]], w)
    waves = [np.ones(n, dtype=np.float32) for n in [161, 480, 1121, 16037, 4000]]
    flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves, 160, 320, max_frames=5)
    assert frames.tolist() == [2, 4, 5, 5, 5] and tmax == 5 and offsets[-1] == flat.shape[0]      # clipping touches only the frame counts
    # tensors are accepted like arrays
    assert mtl_amd.pack_waveforms([torch.ones(200)], 160, 320)[2].tolist() == [2]


def test_pack_waveforms_rejects_what_the_kernel_does_not_support():
    import mtl_amd
    with pytest.raises(ValueError):
        mtl_amd.pack_waveforms([], 160, 320)
    with pytest.raises(ValueError):
        mtl_amd.pack_waveforms([np.zeros((2, 400), dtype=np.float32)], 160, 320)
    with pytest.raises(ValueError, match='utterance 0'):
        mtl_amd.pack_waveforms([np.ones(160, dtype=np.float32), np.ones(400, dtype=np.float32)], 160, 320)
    with pytest.raises(ValueError, match='utterance 1'):
        mtl_amd.pack_waveforms([np.ones(400, dtype=np.float32), np.ones(100, dtype=np.float32)], 160, 320)
    mtl_amd.pack_waveforms([np.ones(161, dtype=np.float32)], 160, 320)                           # n_fft / 2 + 1 is the shortest accepted


def _corpus(tmp_path, n=12):
    """n seeded 16-bit wavs of 0.3-0.7 s + transcripts, split into two manifests"""
    rng = np.random.RandomState(3)
    rows = []
    for i in range(n):
        m = int(16000 * (0.3 + 0.4 * i / (n - 1)))
        t = np.arange(m) / 16000.0
        y = (0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(m)) * np.linspace(0.2, 1.5, m)
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((np.clip(y, -1, 1) * 32767).astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 60) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    manifests = []
    for m in range(2):
        p = tmp_path / ('train%d.csv' % m)
        p.write_text('\n'.join(rows[m::2]) + '\n')
        manifests.append(str(p))
    return manifests


def _dataset(manifests, **kw):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.4,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                      is_train=True, **kw)


def test_device_batches_needs_no_device_to_construct_and_rejects_a_feature_fn(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path)
    ds = _dataset(manifests, seed=7, device_batches=True)
    assert ds.device_batches and len(ds.ids_list) == 2
    assert not _dataset(manifests, seed=7).device_batches                                         # off by default
    with pytest.raises(ValueError, match='feature_fn'):
        _dataset(manifests, seed=7, device_batches=True, feature_fn=lambda p: torch.zeros(161, 3))
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01)
    with pytest.raises(ValueError, match='feature_fn'):
        mtl_amd.ManifestTaskDataset(mtl_amd.synthetic_vocab(64), args, manifests, feature_fn=lambda p: torch.zeros(161, 3), device_batches=True)
    assert mtl_amd.ManifestTaskDataset(mtl_amd.synthetic_vocab(64), args, manifests, device_batches=True, seed=1).device_batches


class _StubFrontEnd:
    """stands in for SpectrogramFrontEnd on a machine without a device: records what `batch` is handed"""

    def __init__(self):
        self.calls = []

    def batch(self, waves, max_frames=None):
        frames = np.minimum(np.array([1 + len(w) // 160 for w in waves]), max_frames).astype(np.int32)
        self.calls.append(([len(w) for w in waves], max_frames))
        return torch.zeros(len(waves), 1, 161, int(frames.max())), torch.from_numpy(frames)


def test_device_batches_draws_the_same_indices_and_makes_one_call_per_part(tmp_path, monkeypatch):
    import importlib
    data = importlib.import_module('mtl_amd.data')
    manifests = _corpus(tmp_path)
    loaded = []
    real_load = data.load_wav_pcm16
    monkeypatch.setattr(data, 'load_wav_pcm16', lambda p: (loaded.append(p), real_load(p))[1])
    plain = _dataset(manifests, seed=7, feature_fn=lambda p: (loaded.append(p), torch.zeros(161, 1 + len(real_load(p)) // 160))[1])
    batched = _dataset(manifests, seed=7, device_batches=True)
    stub = _StubFrontEnd()
    batched._fe_factory = lambda: stub
    for manifest_id, need in ((0, (True, True)), (1, (True, False)), (0, (False, True)), (1, (True, True))):
        del loaded[:]
        a = plain.sample(3, 2, manifest_id, need=need)
        want, n_calls = list(loaded), len(stub.calls)
        del loaded[:]
        b = batched.sample(3, 2, manifest_id, need=need)
        assert loaded == want                                       # the same utterances in the same order; an unused part is not loaded
        assert len(stub.calls) - n_calls == sum(need)               # ONE batch() call per part
        assert all(c[1] == 50 for c in stub.calls[n_calls:])        # cut to args.src_max_len
        for pa, pb, want_part in zip(a, b, need):
            assert (pa is None) == (pb is None) == (not want_part)
            if want_part:
                assert pb[0].shape == pa[0].shape
                for x, y in zip(pa[1:], pb[1:]):                    # input_sizes, input_percentages, targets, target_sizes
                    assert x.dtype == y.dtype and torch.equal(x, y)
