"""CPU: host side of SpecAugment (the policy's draws and plan, the datasets' draw order and constructor rules, the argument checks of the
entry point) and the properties of the numpy / fp64 restatement in tests/specaug_util.py that the device is held to.  Nothing here needs
a device."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import augment_util as au
from tests import specaug_util as su


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _producible(tau, W):
    """every (c, w) that the plan can give for tau frames and a warp of W"""
    if W < 1 or tau < 2 * W + 1:
        return [(0, 0)]
    return [(c, c + d) for c in range(W, tau - W) for d in range(-(W - 1), W)]


def test_the_warp_map_is_monotone_in_range_and_the_identity_without_a_shift():
    n = 0
    for tau in range(1, 40):
        for W in range(0, 6):
            for c, w in _producible(tau, W):
                if w == c:
                    if tau >= 2 and 1 <= w <= tau - 1:            # (the identity: what the device does not even evaluate)
                        i0, a = su.warp_map(tau, c, w)
                        assert np.array_equal(i0, np.arange(tau)) and not a.any()
                    continue
                assert 1 <= w <= tau - 2 and W <= c <= tau - W - 1
                i0, a = su.warp_map(tau, c, w)
                pos = i0 + a.astype(np.float64)
                assert (i0 >= 0).all() and (i0 <= tau - 1).all() and (a >= 0).all() and (a < 1).all()
                assert (pos <= tau - 1).all() and (np.diff(pos) >= 0).all()
                assert not a[i0 == tau - 1].any()                     # (nothing is read beyond the last frame)
                n += 1
    assert n > 5000


def test_apply_leaves_the_padding_unwarped_rows_and_empty_masks_alone():
    rng = np.random.RandomState(0)
    x = rng.randn(3, 5, 23).astype(np.float32)
    x[0, :, 20:] = 0
    x[1, :, 9:] = 0
    x[2, :, 1:] = 0
    # every mask of width 0, placed anywhere it may be (also at the very end), no warp: nothing changes
    table = np.array([[20, 0, 0, 5, 0, 0, 0, 20, 0, 3, 0], [9, 4, 4, 2, 0, 5, 0, 9, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]], dtype=np.int32)
    r = su.apply(x, table, 2, 2)
    assert np.array_equal(r['out'], x.astype(np.float64)) and r['exact'].all() and not r['masked'].any() and np.array_equal(r['src'], x)
    su.check(x, x, table, 2, 2)
    # a warp and masks on utterance 0 only: columns >= tau and the other utterances are untouched, masks win over the warp
    table[0] = [20, 10, 13, 1, 2, 2, 3, 18, 2, 0, 4]
    r = su.apply(x, table, 2, 2)
    assert np.array_equal(r['out'][0, :, 20:], x[0, :, 20:]) and r['exact'][0, :, 20:].all()
    assert np.array_equal(r['out'][1:], x[1:].astype(np.float64)) and r['exact'][1:].all()
    assert r['masked'][0, 1:5, :20].all() and not r['masked'][0, 0, 4:18].any() and r['masked'][0, :, 18:20].all() and r['masked'][0, :, :4].all()
    assert not r['out'][r['masked']].any() and not (r['masked'] & r['exact']).any()
    i0, a = su.warp_map(20, 10, 13)
    j = 7                                                         # an unmasked element of row 0, in front of w
    want = float(x[0, 0, i0[j]]) + float(a[j]) * (float(x[0, 0, i0[j] + 1]) - float(x[0, 0, i0[j]]))
    assert a[j] != 0 and r['out'][0, 0, j] == want and r['scale'][0, 0, j] == max(abs(x[0, 0, i0[j]]), abs(x[0, 0, i0[j] + 1]))
    # the landmark: the boundary in front of output frame w is the boundary in front of source frame c -- the last output frame in front
    # of it reads from in front of c, frame w itself from c on
    assert i0[12] + a[12] < 10 <= i0[13] + a[13] + 0.5
    with pytest.raises(AssertionError):
        su.check(x, x, table, 2, 2)                               # (the criteria do tell an untouched batch from an augmented one)


# ------------------------------------------------------------------------------------------------------------------ draws, plan
class _Counting:
    """a stream that counts the uniforms it hands out"""

    def __init__(self, seed):
        self.rng, self.n = np.random.RandomState(seed), 0

    def random_sample(self, size):
        self.n += int(size)
        return self.rng.random_sample(size)


@pytest.mark.parametrize('policy', [dict(), dict(time_warp=0), dict(freq_masks=0, time_masks=0), dict(freq_masks=8, time_masks=3, freq_width=0),
                                    dict(time_width=0, time_ratio=0.0, freq_masks=1)])
def test_draw_consumes_a_fixed_number_of_uniforms(policy):
    import mtl_amd
    sa = mtl_amd.SpecAugment(**policy)
    rng, mirror = _Counting(5), np.random.RandomState(5)
    d = sa.draw(rng)
    assert rng.n == 2 + 2 * sa.freq_masks + 2 * sa.time_masks == sa.n_draws == su.n_draws(sa.freq_masks, sa.time_masks)
    assert np.array_equal(d, mirror.random_sample(rng.n)) and d.dtype == np.float64
    assert rng.rng.rand() == mirror.rand()


def test_constructor_rules():
    import mtl_amd
    sa = mtl_amd.SpecAugment()
    assert (sa.time_warp, sa.freq_masks, sa.freq_width, sa.time_masks, sa.time_width, sa.time_ratio) == (40, 2, 27, 2, 40, 0.2)
    for bad in (dict(freq_masks=9), dict(time_masks=9), dict(time_ratio=1.5), dict(time_ratio=-0.1), dict(time_warp=-1), dict(freq_width=2.5)):
        with pytest.raises(ValueError):
            mtl_amd.SpecAugment(**bad)
    assert mtl_amd.SpecAugment(freq_masks=8, time_masks=8, time_ratio=1.0).n_draws == 34


def test_plan_respects_its_ranges_at_both_ends_of_the_draws():
    import mtl_amd
    one = np.nextafter(1.0, 0.0)
    policy = dict(time_warp=5, freq_masks=2, freq_width=27, time_masks=2, time_width=40, time_ratio=0.2)
    sa = mtl_amd.SpecAugment(**policy)
    F = 80
    for tau in (1, 2, 9, 10, 11, 12, 37, 100, 1000, 16384):
        cap = min(40, int(np.floor(0.2 * tau)))
        for u in (np.zeros(10), np.full(10, one), np.array([0, one] * 5), np.array([one, 0] * 5)):
            t = sa.plan([u], [tau], F)
            assert t.dtype == np.int32 and t.shape == (1, 11) and (t.freq_masks, t.time_masks) == (2, 2)
            assert t.tolist() == [su.plan_row(u, tau, F, **policy)]
            row = t[0].tolist()
            assert row[0] == tau
            if tau >= 11:
                assert 5 <= row[1] <= tau - 6 and 1 <= row[2] <= tau - 2 and abs(row[2] - row[1]) <= 4
                assert row[1] == (5 if u[0] == 0 else tau - 6) and row[2] - row[1] == (-4 if u[1] == 0 else 4)
            else:
                assert row[1] == row[2] == 0
            for f0, f in (row[3:5], row[5:7]):
                assert 0 <= f <= 27 and 0 <= f0 and f0 + f <= F
            assert row[4] == (0 if u[2] == 0 else 27) and row[3] == (0 if u[3] == 0 else F - row[4])
            for t0, w in (row[7:9], row[9:11]):
                assert 0 <= w <= cap and 0 <= t0 and t0 + w <= tau
            assert row[8] == (0 if u[6] == 0 else cap) and row[7] == (0 if u[7] == 0 else tau - row[8])


def test_plan_edge_cases_and_refusals():
    import mtl_amd
    one = np.nextafter(1.0, 0.0)
    W = 40
    sa = mtl_amd.SpecAugment(freq_width=80)                       # freq_width == F: applies, a mask may cover every row
    t = sa.plan([np.full(10, one), np.full(10, 0.5)], [2 * W, 2 * W + 1], 80)
    assert t[0].tolist()[:3] == [80, 0, 0]                        # tau = 2 W: no warp
    assert t[1].tolist()[:3] == [81, 40, 40]                      # tau = 2 W + 1: the warp applies, c has one value; d = floor(79 / 2) - 39 = 0
    assert t[0].tolist()[3:7] == [0, 80, 0, 80]
    assert sa.plan([[0.5, one] + [0.0] * 8], [81], 80)[0].tolist()[:3] == [81, 40, 79]
    assert sa.plan([[0.5, 0.0] + [0.0] * 8], [81], 80)[0].tolist()[:3] == [81, 40, 1]
    # tau = 1: no warp, floor(0.2) = 0 so no time mask either; the frequency masks apply
    assert sa.plan([np.full(10, one)], [1], 80).tolist() == [[1, 0, 0, 0, 80, 0, 80, 1, 0, 1, 0]]
    # time_warp = 0: its draws are read past, no warp
    assert mtl_amd.SpecAugment(time_warp=0).plan([np.full(10, 0.5)], [500], 80)[0].tolist()[:3] == [500, 0, 0]
    with pytest.raises(ValueError, match='freq_width'):
        mtl_amd.SpecAugment(freq_width=81).plan([np.zeros(10)], [100], 80)
    with pytest.raises(ValueError, match='16384'):
        sa.plan([np.zeros(10), np.zeros(10)], [100, 16385], 80)
    assert sa.plan([np.zeros(10)], [16384], 80).shape == (1, 11)
    with pytest.raises(ValueError):
        sa.plan([np.zeros(9)], [100], 80)                          # not this policy's draws
    # rows of a table know how its columns divide
    assert (t[1:2].freq_masks, t[1:2].time_masks, t[1].freq_masks) == (2, 2, 2)


def test_a_plan_from_random_draws_is_the_restatement(policy=dict(time_warp=7, freq_masks=3, freq_width=11, time_masks=4, time_width=9, time_ratio=0.3)):
    import mtl_amd
    sa, rng = mtl_amd.SpecAugment(**policy), np.random.RandomState(3)
    frames = rng.randint(1, 200, 64)
    draws = [sa.draw(rng) for _ in frames]
    t = sa.plan(draws, frames, 40)
    assert np.array_equal(t, su.plan(draws, frames, 40, **policy))
    x = rng.randn(64, 40, 199).astype(np.float32)
    su.apply(x, t, 3, 4)                                          # (every row passes the restatement's own range assertions)


# ------------------------------------------------------------------------------------------------------------------ datasets
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


def _dataset(manifests, noise_dir=None, noise_prob=0.5, cls='SpectrogramDataset', src_max_len=14, **kw):
    import mtl_amd
    args = argparse.Namespace(src_max_len=src_max_len, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=noise_prob,
                      noise_levels=(0.0, 0.5))
    return getattr(mtl_amd, cls)(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                 is_train=True, **kw)


class _StubFrontEnd:
    """stands in for SpectrogramFrontEnd on a machine without a device: the host geometry that the spec plan needs, and a record of what
    `batch` is handed"""
    F = 161

    def __init__(self):
        self.calls = []

    def _frame_counts(self, lengths):
        return 1 + lengths // 160

    def batch(self, waves, max_frames=None, noise=None, augment=None, spec=None):
        import mtl_amd
        lengths = [len(w) for w in waves]
        if augment is not None:
            lengths = [mtl_amd.TempoGainAugment.out_length(n, t) for n, t in zip(lengths, augment[0])]
        frames = np.array([1 + n // 160 for n in lengths])
        if max_frames is not None:
            frames = np.minimum(frames, max_frames)
        self.calls.append(dict(lengths=[len(w) for w in waves], max_frames=max_frames, noise=noise is not None,
                               spec=None if spec is None else (np.array(spec).tolist(), spec.freq_masks, spec.time_masks)))
        return torch.zeros(len(waves), 1, 161, int(frames.max())), torch.from_numpy(frames.astype(np.int32))


POLICY = dict(time_warp=3, freq_masks=2, freq_width=27, time_masks=1, time_width=5, time_ratio=0.5)


@pytest.mark.parametrize('with_noise', [False, True])
def test_the_stream_is_per_utterance_tempo_gain_noise_then_spec(tmp_path, noise_dir, with_noise):
    import mtl_amd
    manifests = _corpus(tmp_path)
    nd = str(noise_dir) if with_noise else None
    sa = mtl_amd.SpecAugment(**POLICY)
    skipping = _dataset(manifests, nd, seed=11, augment=True, device_batches=True, spec_augment=sa)
    loading = _dataset(manifests, nd, seed=11, augment=True, device_batches=True, spec_augment=sa)
    stub = _StubFrontEnd()
    skipping._fe_factory = loading._fe_factory = lambda: stub
    assert skipping.sample(3, 2, 0, need=(False, False)) == (None, None) and stub.calls == []
    tr, va = loading.sample(3, 2, 0, need=(True, True))
    mirror = np.random.RandomState(11)
    picks = mirror.choice(np.arange(0, 8), 5, p=loading.proba[0], replace=True)
    want = []
    for _ in range(5):
        tempo = float('{:.3f}'.format(mirror.uniform(low=0.85, high=1.15)))
        mirror.uniform(low=-6, high=8)
        if with_noise and mirror.binomial(1, 0.5):
            mirror.choice(loading.noiseInjector.paths)
            mirror.uniform(0.0, 0.5)
            mirror.rand()
        want.append((tempo, mirror.random_sample(8)))                # 2 + 2 * 2 + 2 * 1 uniforms, LAST
    state = mirror.rand()
    assert skipping.rng.rand() == state and loading.rng.rand() == state      # a part that is not loaded consumed its draws
    assert len(stub.calls) == 2
    lengths = [1600 + 160 * int(j) for j in picks]
    for call, sl, part in zip(stub.calls, (slice(0, 3), slice(3, 5)), (tr, va)):
        stretched = [mtl_amd.TempoGainAugment.out_length(n, d[0]) for n, d in zip(lengths[sl], want[sl])]
        frames = [min(1 + n // 160, 14) for n in stretched]           # the FINAL frame counts: stretched, cut to src_max_len
        assert call['lengths'] == lengths[sl] and call['max_frames'] == 14 and part[1].tolist() == frames
        assert call['spec'] == (su.plan([d[1] for d in want[sl]], frames, 161, **POLICY).tolist(), 2, 1)
    assert any(f == 14 for c in stub.calls for f in [r[0] for r in c['spec'][0]])          # (the cut does bind)
    # __getitem__ / parse_audio: the same per-utterance order, one K = 1 call each, the plan for the cut frames
    n_calls = len(stub.calls)
    loading[0]
    loading.parse_audio(loading.ids_list[0][1][0])
    assert len(stub.calls) == n_calls + 2
    assert all(len(c['lengths']) == 1 and c['max_frames'] == 14 and len(c['spec'][0]) == 1 for c in stub.calls[n_calls:])
    for _ in range(2):
        skipping._draws(1)
    assert skipping.rng.rand() == loading.rng.rand()


def test_the_stream_without_spec_augment_is_unchanged(tmp_path, noise_dir):
    manifests = _corpus(tmp_path)
    off = _dataset(manifests, str(noise_dir), seed=3, augment=True, device_batches=True, spec_augment=None)
    plain = _dataset(manifests, str(noise_dir), seed=3, augment=True, device_batches=True)
    for ds in (off, plain):
        ds._fe_factory = _StubFrontEnd
        ds.sample(3, 2, 0)
    mirror = np.random.RandomState(3)
    mirror.choice(np.arange(0, 8), 5, p=plain.proba[0], replace=True)
    draws = [(plain._augment.draw(mirror), plain.noiseInjector.draw(mirror, 0.5)) for _ in range(5)]
    state = mirror.rand()
    assert off.rng.rand() == state and plain.rng.rand() == state
    assert off._fe.calls == plain._fe.calls and all(c['spec'] is None for c in off._fe.calls)
    again = _dataset(manifests, str(noise_dir), seed=3, augment=True, device_batches=True)
    again.rng.choice(np.arange(0, 8), 5, p=plain.proba[0], replace=True)
    assert again._draws(5) == draws                               # pairs, as before: no third entry
    bare = _dataset(manifests, seed=3, device_batches=True)
    assert bare._draws(2) is None and bare._spec is None


@pytest.mark.parametrize('cls', ['SpectrogramDataset', 'LogFBankDataset'])
def test_dataset_constructor_rules_and_the_per_utterance_path(tmp_path, cls):
    import mtl_amd
    manifests = _corpus(tmp_path)
    sa = mtl_amd.SpecAugment(**POLICY)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        _dataset(manifests, cls=cls, seed=7, spec_augment=sa, feature_fn=lambda p: torch.zeros(161, 3))
    ds = _dataset(manifests, cls=cls, seed=7, spec_augment=sa)        # no device needed, and no device_batches either
    assert ds._spec is sa and ds._fe is None
    stub = _StubFrontEnd()
    ds._fe_factory = lambda: stub
    tr, va = ds.sample(2, 1, 0)                                   # rows of sample() without device_batches: one K = 1 call per utterance
    assert len(stub.calls) == 3 and all(len(c['lengths']) == 1 and c['max_frames'] == 14 and c['spec'] is not None for c in stub.calls)
    mirror = np.random.RandomState(7)
    picks = mirror.choice(np.arange(0, 8), 3, p=ds.proba[0], replace=True)
    for c, j in zip(stub.calls, picks):
        frames = [min(1 + (1600 + 160 * int(j)) // 160, 14)]
        assert c['spec'] == (su.plan([mirror.random_sample(8)], frames, 161, **POLICY).tolist(), 2, 1)
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01)
    vocab = mtl_amd.synthetic_vocab(64)
    assert mtl_amd.ManifestTaskDataset(vocab, args, manifests, device_batches=True, seed=1, spec_augment=sa)._spec is sa
    with pytest.raises(NotImplementedError, match='feature_fn'):
        mtl_amd.ManifestTaskDataset(vocab, args, manifests, feature_fn=lambda p: torch.zeros(161, 3), spec_augment=sa)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_rejects_bad_arguments_without_a_device():
    import mtl_amd
    L = mtl_amd._lib.lib()
    assert 'mtl_spec_augment' in mtl_amd._lib.SIGNATURES and L.mtl_cmdlist_opcode(b'mtl_spec_augment') >= 0
    x, t = 4096, 8192                                             # (any non-null values: every call below is refused before a launch)
    assert L.mtl_spec_augment(None, None, 1, 5, 37, t, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 37, None, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 37, t, 9, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 37, t, 2, 9) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 37, t, -1, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 16385, t, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 5, 0, t, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 0, 5, 37, t, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 1, 0, 37, t, 2, 2) == -22
    assert L.mtl_spec_augment(None, x, 1 << 20, 1 << 12, 37, t, 2, 2) == -22


def test_batch_refuses_a_table_that_is_not_this_batch_s():
    """the host checks of the stage, in front of anything that needs the device"""
    from mtl_amd import frontend as fe
    import mtl_amd
    sa = mtl_amd.SpecAugment(**POLICY)
    t = sa.plan([np.zeros(8), np.zeros(8)], [20, 30], 80)
    fe._SpecStage(t, np.array([20, 30], dtype=np.int32))
    fe._SpecStage((np.array(t), 2, 1), np.array([20, 30], dtype=np.int32))
    with pytest.raises(ValueError, match='frame counts'):
        fe._SpecStage(t, np.array([20, 31], dtype=np.int32))
    with pytest.raises(ValueError, match='frame counts'):
        fe._SpecStage(t, np.array([20], dtype=np.int32))
    with pytest.raises(ValueError, match='freq_masks'):
        fe._SpecStage(np.array(t), np.array([20, 30], dtype=np.int32))
