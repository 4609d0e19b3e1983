"""MI355X: SpecAugment on the device against the numpy / fp64 restatement of tests/specaug_util.py -- the entry point mtl_spec_augment on
synthetic planes through the C ABI, the stage behind both feature launches of `BatchFrontEnd.batch`, one call with all four stages, the
datasets and two training iterations.  The criteria (specaug_util.check): a masked element is +0.0 bitwise; an element at a == 0, in a row
that is not warped, or at and beyond tau is bitwise the input; a warped element lies within 2^-22 max(|x[i0]|, |x[i0 + 1]|) of the fp64
restatement."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import resample_util as ru
from tests import specaug_util as su
from tests.test_frontend_pipeline_gpu import _Recorder, _front_end, _plans, inj  # noqa: F401  (inj: the noise bank fixture)

pytestmark = pytest.mark.gpu

GUARD = 64          # floats in front of and behind the batch that no call may touch


def _augment(x, table, mF, mT):
    """mtl_spec_augment on a copy of x (K, F, Tmax) with guard floats on either side -> the augmented batch as numpy"""
    import mtl_amd
    L = mtl_amd._lib.lib()
    K, F, Tmax = x.shape
    table = np.ascontiguousarray(table, dtype=np.int32)
    assert table.shape == (K, 3 + 2 * mF + 2 * mT)
    buf = torch.full((GUARD + x.size + GUARD,), 7.0, device='cuda')
    buf[GUARD:GUARD + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
    d_table = torch.from_numpy(table).cuda()
    st = torch.cuda.current_stream().cuda_stream
    assert L.mtl_spec_augment(st, buf.data_ptr() + 4 * GUARD, K, F, Tmax, d_table.data_ptr(), mF, mT) == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:GUARD] == 7.0).all() and (out[GUARD + x.size:] == 7.0).all()
    return out[GUARD:GUARD + x.size].reshape(x.shape)


def _planes(K, F, Tmax, seed):
    """values without zeros anywhere, the columns beyond any tau included: what must stay untouched is seen to"""
    x = np.random.RandomState(seed).randn(K, F, Tmax).astype(np.float32)
    x[x == 0] = 1.0
    return x


# tau = 37, 36, 11, 1 with W = 5: c in [5, tau - 6], w in [c - 4, c + 4].  Columns: tau, c, w, (f0, f) x 2, (t0, t) x 2
TABLES_37 = {
    # c at its low end with w = c - W + 1, overlapping frequency masks, overlapping time masks one of which ends exactly at tau | c at its
    # high end with w = c + W - 1 = tau - 2, empty masks | w == c with overlapping time masks | a row of zeros (tau = 0: nothing at all)
    'extremes': [[37, 5, 1, 1, 2, 2, 2, 33, 4, 30, 5], [36, 30, 34, 0, 0, 5, 0, 36, 0, 0, 0], [11, 5, 5, 0, 0, 0, 0, 0, 3, 2, 4], [0] * 11],
    # w == c under a frequency mask over all rows | c low with w = c + W - 1, a time mask ending at tau | tau = 2 W + 1 (c has one value),
    # w = c - W + 1, the last row and the last frame masked | tau = 1: its one frame masked by a frequency mask
    'full_rows': [[37, 20, 20, 0, 5, 0, 0, 0, 0, 0, 0], [36, 5, 9, 0, 0, 0, 0, 32, 4, 0, 0], [11, 5, 1, 4, 1, 0, 0, 10, 1, 0, 0],
                  [1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0]],
    # c high with w = c - W + 1 | nothing asked for at full length | tau = 11 with w = c + W - 1 = tau - 2 | tau = 1 untouched
    'other_ends': [[37, 31, 27, 0, 0, 0, 0, 0, 0, 0, 0], [36, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [11, 5, 9, 2, 1, 2, 1, 3, 2, 4, 1],
                   [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]],
}


@pytest.mark.parametrize('name', sorted(TABLES_37))
def test_entry_point_on_misaligned_rows(name):
    """K = 4, F = 5, Tmax = 37: odd, so that row starts are not 16-byte aligned"""
    x, table = _planes(4, 5, 37, 1), np.array(TABLES_37[name], dtype=np.int32)
    got = _augment(x, table, 2, 2)
    n = su.check(got, x, table, 2, 2)
    print(name, n)
    assert n['exact'] > 0 and (name == 'other_ends' or n['masked'] > 0) and (n['warped'] > 0)
    if name == 'extremes':                                        # the zero row and the w == c utterance outside its time masks: untouched
        assert np.array_equal(got[3], x[3]) and np.array_equal(got[2][:, 6:], x[2][:, 6:]) and not got[2][:, :6].any()
    if name == 'full_rows':
        assert not got[0].any() and got[3, 0, 0] == 0 and np.array_equal(got[3][1:], x[3][1:])
    if name == 'other_ends':
        assert np.array_equal(got[1], x[1]) and np.array_equal(got[3], x[3])


def test_entry_point_with_more_frames_than_a_workgroup_has_lanes():
    """Tmax = 1031 (odd again), W = 40: both ends of c, both extremes of w, masks of both kinds on warped rows"""
    x = _planes(2, 3, 1031, 2)
    table = np.array([[1031, 40, 1, 1, 1, 0, 0, 1000, 31, 300, 40], [700, 659, 698, 0, 0, 2, 1, 0, 40, 20, 40]], dtype=np.int32)
    n = su.check(_augment(x, table, 2, 2), x, table, 2, 2)
    print(n)
    assert n['warped'] > 1000 and n['masked'] > 400 and n['exact'] >= 331 * 3


def test_entry_point_at_the_row_limit():
    """Tmax = 16384: the whole 64 KB of LDS; row 0 warped with a time mask ending at tau, row 1 under a frequency mask"""
    x = _planes(1, 2, 16384, 3)
    table = np.array([[16384, 16343, 16382, 1, 1, 16344, 40]], dtype=np.int32)
    got = _augment(x, table, 1, 1)
    n = su.check(got, x, table, 1, 1)
    print(n)
    assert n['warped'] > 16000 and not got[0, 1].any() and not got[0, 0, 16344:].any()
    # ... and the same plane with nothing asked for: not a bit moves
    table = np.array([[16384, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert np.array_equal(_augment(x, table, 1, 1), x)
    # no masks at all is a valid shape of the table
    table = np.array([[16384, 40, 79]], dtype=np.int32)
    assert su.check(_augment(x, table, 0, 0), x, table, 0, 0)['masked'] == 0


# ------------------------------------------------------------------------------------------------------------------ both front-ends
POLICY = dict(time_warp=40, freq_masks=2, freq_width=27, time_masks=2, time_width=40, time_ratio=0.2)


@pytest.mark.parametrize('max_frames', [None, 120])
@pytest.mark.parametrize('kind', ['spectrogram', 'logfbank'])
def test_batch_with_spec_is_the_clean_batch_through_the_restatement(kind, max_frames):
    import mtl_amd
    fe, sa = _front_end(kind), mtl_amd.SpecAugment(**POLICY)
    waves = [ru.waveform(n, 30 + j, 16000) for j, n in enumerate((16000, 24000, 8000))]      # the shortest has fewer than 2 W + 1 frames
    clean, sizes = fe.batch(waves, max_frames=max_frames)
    rng = np.random.RandomState(4)
    t = sa.plan([sa.draw(rng) for _ in waves], sizes.numpy(), fe.F)
    assert t[2, 1] == t[2, 2] == 0 and t[0, 1] != t[0, 2] and t[1, 1] != t[1, 2] and int(sizes.min()) < 81 and int(sizes.max()) == (max_frames or (151 if kind == 'spectrogram' else 149))
    none, sizes_none = fe.batch(waves, max_frames=max_frames, spec=None)
    assert torch.equal(none, clean) and torch.equal(sizes_none, sizes)
    got, sizes_spec = fe.batch(waves, max_frames=max_frames, spec=t)
    assert torch.equal(sizes_spec, sizes) and got.shape == clean.shape and got.is_cuda
    n = su.check(got.cpu().numpy()[:, 0], clean.cpu().numpy()[:, 0], t, 2, 2)
    print(kind, max_frames, n)
    assert n['warped'] > 0 and n['masked'] > 0
    for k in range(3):                                            # one utterance alone: bitwise its plane in the batched call
        one, size = fe.batch([waves[k]], max_frames=max_frames, spec=t[k:k + 1])
        assert int(size[0]) == int(sizes[k]) and torch.equal(one[0, 0], got[k, 0, :, :int(sizes[k])])
    with pytest.raises(ValueError, match='frame counts'):
        fe.batch(waves[:2], max_frames=max_frames, spec=t[1:3])


@pytest.mark.parametrize('kind', ['spectrogram', 'logfbank'])
def test_all_four_stages_end_with_the_feature_launch_and_the_spec_launch(monkeypatch, inj, kind):  # noqa: F811
    import mtl_amd
    fe, sa = _front_end(kind), mtl_amd.SpecAugment(time_warp=3, freq_masks=2, freq_width=27, time_masks=2, time_width=10, time_ratio=0.5)
    rates = [8000, 16000, 8000]
    waves = [ru.waveform(n, 50 + j, r) for j, (n, r) in enumerate(zip((3000, 5000, 2100), rates))]
    kw, _ = _plans(inj, [len(w) for w in waves], rates, [0.9, 1.0, 1.13], clean=[1])
    base, sizes = fe.batch(waves, **kw)
    rng = np.random.RandomState(6)
    t = sa.plan([sa.draw(rng) for _ in waves], sizes.numpy(), fe.F)
    rec = _Recorder(mtl_amd._lib.lib())
    monkeypatch.setattr(mtl_amd._lib, 'lib', lambda: rec)
    got, sizes_spec = fe.batch(waves, spec=t, **kw)
    monkeypatch.undo()
    names = [n for n in rec.names if not n.endswith('_workspace')]
    want = ['mtl_resample', 'mtl_tempo_search', 'mtl_tempo_render', 'mtl_wave_mix_coef']
    want += ['mtl_spect_batch_noise'] if kind == 'spectrogram' else ['mtl_wave_mix', 'mtl_fbank_batch']
    assert names == want + ['mtl_spec_augment']
    assert torch.equal(sizes_spec, sizes)
    n = su.check(got.cpu().numpy()[:, 0], base.cpu().numpy()[:, 0], t, 2, 2)
    print(kind, n)
    assert n['warped'] > 0 and n['masked'] > 0


# ------------------------------------------------------------------------------------------------------------------ datasets, training
def _corpus(tmp_path, n=12):
    """n seeded 16-bit wavs of 0.3-0.7 s + transcripts, split into two manifests (as tests/test_frontend_batch_gpu.py)"""
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.rint(ru.waveform(int(16000 * (0.3 + 0.4 * i / (n - 1))), 40 + i, 16000).astype(np.float64) * 32768.0)
                          .astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    manifests = []
    for m in range(2):
        p = tmp_path / ('train%d.csv' % m)
        p.write_text('\n'.join(rows[m::2]) + '\n')
        manifests.append(str(p))
    return manifests


DS_POLICY = dict(time_warp=5, freq_masks=2, freq_width=20, time_masks=2, time_width=10, time_ratio=0.3)


def _dataset(cls, vocab, manifests, spec_augment, device_batches=True):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.0)
    return getattr(mtl_amd, cls)(vocab, args, audio_conf, manifest_filepath_list=manifests, normalize=True, is_train=True, seed=7,
                                 device_batches=device_batches, spec_augment=spec_augment)


@pytest.mark.parametrize('cls,F', [('SpectrogramDataset', 161), ('LogFBankDataset', 80)])
def test_dataset_sample_is_the_plain_sample_through_the_restatement(tmp_path, cls, F):
    import mtl_amd
    vocab, manifests = mtl_amd.synthetic_vocab(64), _corpus(tmp_path)
    sa = mtl_amd.SpecAugment(**DS_POLICY)
    with_spec, plain, rows = _dataset(cls, vocab, manifests, sa), _dataset(cls, vocab, manifests, None), _dataset(cls, vocab, manifests, sa, False)
    a, b, c = with_spec.sample(3, 2, 0), plain.sample(3, 2, 0), rows.sample(3, 2, 0)
    # the documented stream: the choice of the indices, then per utterance (no augmentation, no injector) the spec draws alone
    mirror = np.random.RandomState(7)
    picks = mirror.choice(np.arange(0, 6), 5, p=plain.proba[0], replace=True)
    draws = [mirror.random_sample(10) for _ in range(5)]
    assert with_spec.rng.rand() == mirror.rand()
    alone = np.random.RandomState(7)
    alone.choice(np.arange(0, 6), 5, p=plain.proba[0], replace=True)
    assert plain.rng.rand() == alone.rand()                       # (without the keyword nothing but the indices was drawn)
    for pa, pb, pc, sl in zip(a, b, c, (slice(0, 3), slice(3, 5))):
        assert pa[0].is_cuda and pa[0].shape == pb[0].shape == (sl.stop - sl.start, 1, F, int(pb[1].max()))
        for x, y in zip(pa[1:], pb[1:]):                            # the same picks: sizes, percentages, targets, target sizes
            assert torch.equal(x, y)
        t = su.plan(draws[sl], pb[1].tolist(), F, **DS_POLICY)
        n = su.check(pa[0].cpu().numpy()[:, 0], pb[0].cpu().numpy()[:, 0], t, 2, 2)
        print(cls, n)
        assert n['masked'] > 0 and n['warped'] > 0
        # the rows of sample() without device_batches: batch([y], spec=row), the same planes on the host
        assert not pc[0].is_cuda and torch.equal(pc[0], pa[0].cpu()) and all(torch.equal(x, y) for x, y in zip(pc[1:], pa[1:]))
    assert len(set(picks.tolist())) > 1
    spect, transcript = with_spec[0]
    assert not spect.is_cuda and spect.shape[0] == F and 0 < spect.shape[1] <= 50 and len(transcript) > 0


def test_two_joint_training_iterations_from_a_dataset_with_spec_augment(tmp_path):
    import mtl_amd
    from tests.test_parity_gpu import make
    z, cfg, spec = gu.load('F0')
    manifests = _corpus(tmp_path)
    mtl_amd, args, vocab, model = make(cfg, spec, name='specaug')
    args.save_folder, args.k_train, args.k_valid, args.loss = str(tmp_path), 3, 2, 'ce'
    model = model.cuda()
    tasks = [_dataset('SpectrogramDataset', vocab, manifests, mtl_amd.SpecAugment(**DS_POLICY)) for _ in range(2)]
    tr = mtl_amd.JointTrainer()
    tr.train(model, vocab, tasks, [], 'ce', 0, 2, args, evaluate_every=10 ** 9, early_stop='loss,5')
    torch.cuda.synchronize()
    losses = [float(v) for v in tr.loss_trace]
    print('losses', losses)
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses)
