"""CPU: host side of the tempo / gain augmentation (TempoGainAugment: draw stream, lengths, plan; the datasets' draw order and
constructor rules; the ABI surface) and the properties of the fp64 restatement in tests/augment_util.py that the device is held to.
Nothing here needs a device."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import augment_util as au


def write_wav(path, y, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.rint(np.asarray(y, dtype=np.float64) * 32768.0).astype('<i2').tobytes())


def _corpus(tmp_path, n=8):
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        write_wav(wp, au.waveform(1600 + 160 * i, 40 + i))
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


@pytest.fixture()
def noise_dir(tmp_path):
    d = tmp_path / 'noise'
    d.mkdir()
    write_wav(d / 'a.wav', au.waveform(3000, 1))
    write_wav(d / 'b.wav', au.waveform(5000, 2))
    return d


def _dataset(manifests, noise_dir=None, noise_prob=0.5, **kw):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=noise_prob,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                      is_train=True, **kw)


class _StubFrontEnd:
    """stands in for SpectrogramFrontEnd on a machine without a device: records what `batch` is handed"""

    def __init__(self):
        self.calls = []

    def batch(self, waves, max_frames=None, noise=None, augment=None):
        lengths = [len(w) for w in waves]
        if augment is not None:
            import mtl_amd
            lengths = [mtl_amd.TempoGainAugment.out_length(n, t) for n, t in zip(lengths, augment[0])]
        frames = np.array([1 + n // 160 for n in lengths])
        if max_frames is not None:
            frames = np.minimum(frames, max_frames)
        self.calls.append(dict(lengths=[len(w) for w in waves], augment=None if augment is None else (augment[0].tolist(), augment[1].tolist()),
                               noise=None if noise is None else (noise[1].tolist(), noise[2].tolist())))
        return torch.zeros(len(waves), 1, 161, int(frames.max())), torch.from_numpy(frames.astype(np.int32))


# ------------------------------------------------------------------------------------------------------------------ draws, plan
def test_draw_takes_the_two_reference_draws_rounded_to_three_decimals():
    import mtl_amd
    aug = mtl_amd.TempoGainAugment()
    assert aug.tempo_range == (0.85, 1.15) and aug.gain_range == (-6, 8)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(50):
        tempo, gain = aug.draw(a)
        # utils/audio.py:55-58 and the "{:.3f}".format of :41-42 restated
        t = b.uniform(low=0.85, high=1.15)
        g = b.uniform(low=-6, high=8)
        assert (tempo, gain) == (float('{:.3f}'.format(t)), float('{:.3f}'.format(g)))
        assert 0.85 <= tempo <= 1.15 and -6.0 <= gain <= 8.0 and round(tempo, 3) == tempo and round(gain, 3) == gain
    assert a.rand() == b.rand()                                   # both generators in the same state
    other = mtl_amd.TempoGainAugment((0.9, 1.0), (0, 1))
    a, b = np.random.RandomState(6), np.random.RandomState(6)
    assert other.draw(a) == (float('%.3f' % b.uniform(0.9, 1.0)), float('%.3f' % b.uniform(0, 1)))


def test_out_length_plan_and_geometry():
    import mtl_amd
    assert mtl_amd.wsola_geometry(16000) == (1312, 235, 192) == au.geometry(16000)
    assert mtl_amd.wsola_geometry(8000) == (656, 117, 96) == au.geometry(8000)
    aug = mtl_amd.TempoGainAugment()
    assert aug.out_length(1547, 0.937) == 1651 and aug.out_length(161, 0.85) == 189 and aug.out_length(2240, 1.0) == 2240
    assert aug.out_length(16037, 1.15) == 13945 and aug.out_length(3, 1.15) == 3 and aug.out_length(0, 0.9) == 0
    for L, _, f, _, _ in au.CASES:
        assert aug.out_length(L, f) == au.out_length(L, f) == int(np.floor(L / f + 0.5)) or f == 1.0
    with pytest.raises(ValueError):
        aug.out_length(100, 0.0)
    tempo, gain_db, out_lengths = aug.plan([(0.937, 8.0), (1.0, 0.0), (1.102, 3.3)], [1547, 2240, 4000])
    assert tempo.dtype == np.float64 and gain_db.dtype == np.float32 and out_lengths.dtype == np.int64
    assert tempo.tolist() == [0.937, 1.0, 1.102] and gain_db.tolist() == [8.0, 0.0, float(np.float32(3.3))] and out_lengths.tolist() == [1651, 2240, 3630]
    # the tables of the device calls: the segment prefix (none for the bypass), the linear gain rounded once from fp64
    tab = mtl_amd.tempo_gain_tables([np.zeros(1547, np.float32), np.zeros(2240, np.float32), np.zeros(4000, np.float32)], tempo, gain_db, 16000)
    assert tab['offsets'].tolist() == [0, 1547, 3787, 7787] and tab['out_offsets'].tolist() == [0, 1651, 3891, 7521]
    assert tab['seg_base'].tolist() == [0, 2, 2, 6] and tab['geometry'] == (1312, 235, 192) and tab['flat'].shape == (7787,)
    assert tab['gain'].dtype == np.float32 and tab['gain'][0] == np.float32(10.0 ** 0.4) and tab['gain'][1] == 1.0
    with pytest.raises(ValueError):
        mtl_amd.tempo_gain_tables([np.zeros(100, np.float32)], [0.9, 1.0], [0.0, 0.0], 16000)
    with pytest.raises(ValueError):                               # a search of more than 255 samples is beyond the kernel
        mtl_amd.tempo_gain_tables([np.zeros(100, np.float32)], [0.9], [0.0], 22050)


def test_start_positions_are_plain_ieee_double_arithmetic():
    """p_m = floor(f (m H) + 0.5) with one rounding after the multiply and one after the add is what the host AND the kernel form (the
    kernel through non-contracted fp64 operations): on the factors of the cases it equals the exact rational value, so no case sits
    where a fused multiply-add could move a start position"""
    from fractions import Fraction
    for _, _, f, _, rate in au.CASES:
        S, R, O = au.geometry(rate)
        H = S - O
        for m in range(200):
            exact = Fraction('%.3f' % f) * (m * H) + Fraction(1, 2)
            assert int(np.floor(f * float(m * H) + 0.5)) == exact.numerator // exact.denominator, (f, m)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_identity_lengths_and_margins():
    for case, (L, seed, f, gain_db, rate) in enumerate(au.CASES):
        r = au.reference(case)                                    # (asserts len == N and the margins itself)
        S, R, O = au.geometry(rate)
        H = S - O
        assert r['N'] == len(r['out']) == len(r['q']) == au.out_length(L, f)
        assert len(r['offsets']) == (0 if f == 1.0 else -(-r['N'] // H))
        if f != 1.0:
            assert r['offsets'][0] == R // 2 and r['offsets'].min() >= 0 and r['offsets'].max() <= R
            real = r['margins'][~np.isnan(r['margins'])]
            print('case %d: %d segments, least margin %s' % (case, len(r['offsets']), real.min() if len(real) else None))
            assert (real >= au.MIN_MARGIN).all()
        assert np.abs(r['q']).max() <= 32768
    assert len(au.reference(0)['offsets']) == 1 and len(au.reference(3)['offsets']) == 16 and len(au.reference(7)['offsets']) == 8
    assert au.reference(1)['offsets'].tolist() == [117, 188] and au.reference(1)['margins'].tolist() == [1.0]      # the exact match
    clipped = np.mean(np.abs(au.reference(1)['q']) >= 32767)
    assert 0.01 < clipped < 0.1, clipped                          # +8 dB does clip
    # f == 1.0 is the bypass: the input itself, also through gain 0 dB and the 16-bit rounding (the samples are on the grid)
    r = au.reference(6)
    assert np.array_equal(r['out'], r['x'].astype(np.float64)) and np.array_equal(r['q'], np.rint(r['x'].astype(np.float64) * 32768))
    # ... without the bypass the definition would shift by R // 2: all offsets R // 2 and out = x[R // 2:]
    x = r['x'].astype(np.float64)
    shifted = au.wsola(x, np.nextafter(1.0, 2.0))
    assert (shifted['offsets'] == 235 // 2).all() and np.array_equal(shifted['out'][:2240 - 117], x[117:])
    # an input that repeats exactly with a period of 100 <= R samples: every searched offset continues the tail without a seam (the
    # smallest of the equal candidates), so the output is the same periodic signal, only longer
    period = np.sin(2 * np.pi * np.arange(100) / 100.0)
    out = au.wsola(np.tile(period, 60), 0.9)
    assert len(out['out']) == 6667 and (out['offsets'][1:4] < 100).all()
    assert np.array_equal(out['out'][:4000], period[(np.arange(4000) + 117) % 100])


# ------------------------------------------------------------------------------------------------------------------ datasets
def test_constructor_rules(tmp_path, noise_dir):
    import mtl_amd
    manifests = _corpus(tmp_path)
    with pytest.raises(NotImplementedError, match='device_batches=True'):
        _dataset(manifests, seed=7, augment=True)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        _dataset(manifests, seed=7, augment=True, feature_fn=lambda p: torch.zeros(161, 3))
    ds = _dataset(manifests, str(noise_dir), seed=7, augment=True, device_batches=True)       # no device needed
    assert isinstance(ds._augment, mtl_amd.TempoGainAugment) and ds.augment is True and ds._fe is None
    assert ds._augment.tempo_range == (0.85, 1.15) and ds._augment.gain_range == (-6, 8) and ds.noiseInjector._bank is None
    assert _dataset(manifests, seed=7, device_batches=True)._augment is None
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01)
    vocab, aug = mtl_amd.synthetic_vocab(64), mtl_amd.TempoGainAugment((0.9, 1.1), (-1, 1))
    assert mtl_amd.ManifestTaskDataset(vocab, args, manifests, device_batches=True, seed=1, augment=aug)._augment is aug
    with pytest.raises(NotImplementedError, match='device_batches=True'):
        mtl_amd.ManifestTaskDataset(vocab, args, manifests, seed=1, augment=aug)
    with pytest.raises(NotImplementedError):
        mtl_amd.ManifestTaskDataset(vocab, args, manifests, feature_fn=lambda p: torch.zeros(161, 3), augment=aug)


@pytest.mark.parametrize('with_noise', [False, True])
def test_sample_draws_per_utterance_tempo_gain_then_noise(tmp_path, noise_dir, with_noise):
    import mtl_amd
    manifests = _corpus(tmp_path)
    nd = str(noise_dir) if with_noise else None
    skipping = _dataset(manifests, nd, seed=11, augment=True, device_batches=True)
    loading = _dataset(manifests, nd, seed=11, augment=True, device_batches=True)
    stub = _StubFrontEnd()
    skipping._fe_factory = loading._fe_factory = lambda: stub
    assert skipping.sample(3, 2, 0, need=(False, False)) == (None, None) and stub.calls == []
    tr, va = loading.sample(3, 2, 0, need=(True, True))
    # the stream restated: the choice of the indices, then PER UTTERANCE tempo, gain and that utterance's noise draws
    mirror = np.random.RandomState(11)
    picks = mirror.choice(np.arange(0, 8), 5, p=loading.proba[0], replace=True)
    want = []
    for _ in range(5):
        tempo = float('{:.3f}'.format(mirror.uniform(low=0.85, high=1.15)))
        gain = float('{:.3f}'.format(mirror.uniform(low=-6, high=8)))
        nz = None
        if with_noise and mirror.binomial(1, 0.5):
            path = mirror.choice(loading.noiseInjector.paths)
            level = mirror.uniform(0.0, 0.5)
            nz = (loading.noiseInjector.paths.index(path), level, mirror.rand())
        want.append((tempo, gain, nz))
    state = mirror.rand()
    assert skipping.rng.rand() == state and loading.rng.rand() == state      # an unused part consumed its draws
    assert len(stub.calls) == 2                                             # ONE batch call per part
    lengths = [1600 + 160 * int(j) for j in picks]
    for call, sl, part in zip(stub.calls, (slice(0, 3), slice(3, 5)), (tr, va)):
        w = want[sl]
        assert call['lengths'] == lengths[sl]
        assert call['augment'] == ([d[0] for d in w], [float(np.float32(d[1])) for d in w])
        stretched = [mtl_amd.TempoGainAugment.out_length(n, d[0]) for n, d in zip(lengths[sl], w)]
        assert part[1].tolist() == [min(1 + n // 160, 50) for n in stretched]     # the sizes follow the STRETCHED lengths
        assert torch.equal(part[2], part[1].float() / float(part[0].size(3)))
        if not with_noise:
            assert call['noise'] is None
        else:                                                       # the noise plan is made for the STRETCHED lengths (all clean: none)
            off, lvl = loading.noiseInjector.plan([d[2] for d in w], stretched)
            assert call['noise'] == ((off.tolist(), lvl.tolist()) if (off >= 0).any() else None)
    if with_noise:
        assert any(d[2] is not None for d in want)
    # __getitem__ / parse_audio: the same per-utterance order, one K = 1 call each
    n_calls = len(stub.calls)
    spect, transcript = loading[0]
    assert spect.shape[0] == 161 and len(transcript) > 0 and loading.parse_audio(loading.ids_list[0][1][0]).shape[0] == 161
    assert len(stub.calls) == n_calls + 2 and all(len(c['lengths']) == 1 and c['augment'] is not None for c in stub.calls[n_calls:])
    for _ in range(2):
        skipping._draws(1)
    assert skipping.rng.rand() == loading.rng.rand()


def test_the_stream_without_augment_is_unchanged(tmp_path, noise_dir):
    """augment off: the draws are the noise draws alone, as a dataset built without the keyword takes them"""
    import mtl_amd
    manifests = _corpus(tmp_path)
    off = _dataset(manifests, str(noise_dir), seed=3, augment=False, device_batches=True)
    plain = _dataset(manifests, str(noise_dir), seed=3, device_batches=True)
    mirror = np.random.RandomState(3)
    for ds in (off, plain):
        ds._fe_factory = _StubFrontEnd
    for ds in (off, plain):
        ds.sample(3, 2, 0)
    mirror.choice(np.arange(0, 8), 5, p=plain.proba[0], replace=True)
    draws = [plain.noiseInjector.draw(mirror, 0.5) for _ in range(5)]
    assert any(d is not None for d in draws)
    state = mirror.rand()
    assert off.rng.rand() == state and plain.rng.rand() == state
    assert off._fe.calls == plain._fe.calls and all(c['augment'] is None for c in off._fe.calls)
    # no augmentation, no injector: no draws at all beside the indices
    bare = _dataset(manifests, seed=3, device_batches=True)
    bare._fe_factory = _StubFrontEnd
    bare.sample(3, 2, 0)
    mirror = np.random.RandomState(3)
    mirror.choice(np.arange(0, 8), 5, p=bare.proba[0], replace=True)
    assert bare.rng.rand() == mirror.rand() and bare._draws(2) is None


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_abi_surface_lists_the_new_entry_points():
    import mtl_amd
    L = mtl_amd._lib.lib()
    for name in ('mtl_tempo_search', 'mtl_tempo_render'):
        assert name in mtl_amd._lib.SIGNATURES and L.mtl_cmdlist_opcode(name.encode()) >= 0
    # bad arguments are rejected before any launch (no device needed)
    assert L.mtl_tempo_search(None, None, None, None, None, None, 1, 1312, 235, 192, None) == -22
    assert L.mtl_tempo_render(None, None, None, None, None, None, None, None, 1, 1312, 235, 192, 1, None) == -22
    for name in ('TempoGainAugment', 'load_randomly_augmented_audio', 'tempo_gain', 'wsola_geometry'):
        assert hasattr(mtl_amd, name)
    assert hasattr(mtl_amd.SpectrogramFrontEnd, 'tempo_gain')
