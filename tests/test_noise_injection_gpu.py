"""MI355X: noise injection mixed on the device (mtl_wave_mix_coef / mtl_wave_mix / mtl_spect_batch_noise, NoiseInjection,
SpectrogramFrontEnd.batch(noise=...), the datasets) against the fp64 formula of the reference's inject_noise_sample in numpy, against
the unfused path bit for bit, and against the numpy oracle of parse_audio at the front-end's own bar."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import golden_util as gu

pytestmark = pytest.mark.gpu

BAR = 2e-5                                      # tests/test_frontend_batch_gpu.py: BAR
LENGTHS_16K = [161, 480, 1121, 16037, 4000]     # both ends reflected in one tile | multiple of hop | ragged | two row tiles | mid
NOISE_LENGTHS = [20000, 16037]                  # the second: start 0 is the only placement of utterance 3, which ends on the bank's last sample
ZEROS = (8000, 12500)                           # a silent stretch of the first noise file
# utterance 1 clean between noisy neighbours; utterance 2 with u = 1: its segment ends exactly at its file's end; utterance 3 on the
# 16 037-sample file; utterance 4 at level 0
DRAWS = [(0, 0.5, 0.2), None, (0, 0.25, 1.0), (1, 0.1, 0.37), (0, 0.0, 0.1)]
OFFSETS = [3967, -1, 20000 - 1121, 20000, 1600]
LEVELS = [0.5, 0.0, 0.25, 0.1, 0.0]


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def waveform(n, seed, rate=16000):
    """the recipe of tests/test_frontend_batch_gpu.py"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    return ((0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)) * np.linspace(0.2, 1.5, n)).astype(np.float32)


def write_wav(path, y, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(y, -1, 1) * 32767).astype('<i2').tobytes())


def make_noise_dir(d, lengths, rate=16000, zeros=None):
    d.mkdir()
    for i, n in enumerate(lengths):
        y = waveform(n, 70 + i, rate=rate)[::-1].copy()
        if zeros is not None and i == 0:
            y[zeros[0]:zeros[1]] = 0.0
        write_wav(d / ('n%d.wav' % i), y, rate)
    return str(d)


@pytest.fixture(scope='module')
def inj16(tmp_path_factory):
    import mtl_amd
    inj = mtl_amd.NoiseInjection(make_noise_dir(tmp_path_factory.mktemp('noise') / 'bank', NOISE_LENGTHS, zeros=ZEROS))
    assert inj.lengths.tolist() == NOISE_LENGTHS and inj.bank_len == sum(NOISE_LENGTHS) and not inj.bank[ZEROS[0]:ZEROS[1]].any()
    return inj


@pytest.fixture(scope='module')
def waves16():
    return [waveform(n, 10 + i) for i, n in enumerate(LENGTHS_16K)]


@pytest.fixture(scope='module')
def plan16(inj16):
    noise_off, level = inj16.plan(DRAWS, LENGTHS_16K)
    assert noise_off.tolist() == OFFSETS and level.tolist() == [float(np.float32(v)) for v in LEVELS] and inj16.skipped == 0
    assert noise_off[2] + LENGTHS_16K[2] == NOISE_LENGTHS[0] and noise_off[3] + LENGTHS_16K[3] == inj16.bank_len
    return noise_off, level


def reference_mix(inj, waves, noise_off, level):
    """utils/data_loader.py:396-398 in fp64 on the same int16 noise -> per utterance (mixed fp64, |d| + |c n|)"""
    out = []
    for y, o, lv in zip(waves, noise_off, level):
        d = y.astype(np.float64)
        if o < 0:
            out.append((d, np.abs(d)))
            continue
        n = inj.bank[o:o + len(y)].astype(np.float64) / 32768.0
        assert len(n) == len(y)
        c = float(lv) * np.sqrt(d.dot(d) / d.size) / np.sqrt(n.dot(n) / n.size)
        out.append((d + c * n, np.abs(d) + np.abs(c * n)))
    return out


def device_mix(L, inj, waves, noise_off, level):
    """mtl_wave_mix_coef + mtl_wave_mix on the packed waveforms -> (list of mixed float32 arrays, coef)"""
    flat = np.concatenate(waves)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    K = len(waves)
    wav, off = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets).cuda()
    noff, lvl = torch.from_numpy(np.asarray(noise_off, dtype=np.int64)).cuda(), torch.from_numpy(np.asarray(level, dtype=np.float32)).cuda()
    bank = inj.device_bank()
    coef, out = torch.full((K,), 7.0, device='cuda'), torch.empty_like(wav)
    ws_bytes = L.mtl_wave_mix_coef_workspace(K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert L.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), K, bank.data_ptr(), inj.bank_len, noff.data_ptr(), lvl.data_ptr(),
                               coef.data_ptr(), ws.data_ptr(), ws_bytes) == 0
    assert L.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), K, bank.data_ptr(), inj.bank_len, noff.data_ptr(), coef.data_ptr(),
                          out.data_ptr()) == 0
    torch.cuda.synchronize()
    mixed = out.cpu().numpy()
    return [mixed[offsets[k]:offsets[k + 1]] for k in range(K)], coef.cpu().numpy()


@pytest.fixture(scope='module')
def mixed16(L, inj16, waves16, plan16):
    """computed once, shared and left unchanged"""
    return device_mix(L, inj16, waves16, *plan16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ 1. mix arithmetic
def test_mix_matches_the_fp64_formula(inj16, waves16, plan16, mixed16):
    """|out - ref| <= 2^-23 (|d| + |c n|): one rounding of the fma result (2^-24 |d + c n|) plus one rounding of c to fp32
    (2^-24 |c n|); the fp64 sums contribute about 1e-13 relative."""
    mixed, coef = mixed16
    ref = reference_mix(inj16, waves16, *plan16)
    for k, ((r, scale), m) in enumerate(zip(ref, mixed)):
        err = np.abs(m.astype(np.float64) - r)
        worst = float((err / np.maximum(scale, 1e-300)).max())
        print('utterance %d: coef %.9g, worst |out - ref| / (|d| + |c n|) = %.3e (bound %.3e)' % (k, coef[k], worst, 2.0 ** -23))
        assert (err <= 2.0 ** -23 * scale).all(), (k, worst)
    assert coef[1] == 0.0 and coef[4] == 0.0 and coef[0] > 0 and coef[2] > 0 and coef[3] > 0
    for k in (1, 4):                                                  # the clean and the level-0 utterance: bit-identical
        assert np.array_equal(bits(mixed[k]), bits(waves16[k])), k
    for k in (0, 2, 3):
        assert not np.array_equal(bits(mixed[k]), bits(waves16[k])), k


def test_a_silent_noise_segment_leaves_the_utterance_untouched(L, inj16, waves16):
    y = waves16[4].copy()
    y[7] = -0.0                                                       # signed zeros survive too
    mixed, coef = device_mix(L, inj16, [waves16[0], y], [ZEROS[0] + 50, ZEROS[0] + 100], [0.5, 0.5])
    assert coef.tolist() == [0.0, 0.0]
    assert np.array_equal(bits(mixed[0]), bits(waves16[0])) and np.array_equal(bits(mixed[1]), bits(y))


def test_inject_noise_sample_is_the_unfused_mix(inj16, waves16, mixed16):
    y = waves16[2].copy()
    got = inj16.inject_noise_sample(y, inj16.paths[0], 0.25, u=1.0)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(bits(y), bits(waves16[2]))
    assert np.array_equal(bits(got), bits(mixed16[0][2]))
    np.random.seed(3)
    a = inj16.inject_noise(waves16[0])
    np.random.seed(3)
    path, level, u = np.random.choice(inj16.paths), np.random.uniform(0, 0.5), np.random.rand()
    assert np.array_equal(bits(a), bits(inj16.inject_noise_sample(waves16[0], path, level, u=u)))
    assert not np.array_equal(bits(a), bits(waves16[0]))


# ------------------------------------------------------------------------------------------------------------ 2. fused = unfused
@pytest.fixture(scope='module')
def fe16():
    import mtl_amd
    return {norm: mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=norm) for norm in (True, False)}


@pytest.mark.parametrize('normalize,max_frames', [(True, None), (False, None), (True, 20)])
def test_fused_equals_unfused_bitwise(inj16, waves16, plan16, mixed16, fe16, normalize, max_frames):
    fe = fe16[normalize]
    a, sa = fe.batch(waves16, max_frames=max_frames, noise=(inj16,) + plan16)
    b, sb = fe.batch(mixed16[0], max_frames=max_frames)
    assert a.is_cuda and tuple(a.shape) == (5, 1, 161, 20 if max_frames else 101) and torch.equal(sa, sb)
    assert torch.equal(a, b)
    clean, _ = fe.batch(waves16, max_frames=max_frames)
    for k in range(5):
        assert torch.equal(a[k], clean[k]) == (k in (1, 4)), k      # the noise reached the noisy utterances, and only them


# ------------------------------------------------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize('normalize', [True, False])
def test_noisy_batch_matches_the_oracle(inj16, waves16, plan16, fe16, normalize):
    from oracle import frontend
    inputs, sizes = fe16[normalize].batch(waves16, noise=(inj16,) + plan16)
    assert sizes.tolist() == [2, 4, 8, 101, 26]
    for k, (y64, _) in enumerate(reference_mix(inj16, waves16, *plan16)):
        n = int(sizes[k])
        e = rel(inputs[k, 0, :, :n], frontend.parse_audio(y64.astype(np.float32), normalize=normalize))
        print('noisy batch vs oracle, normalize=%s, utterance %d: %.2e' % (normalize, k, e))
        assert e < BAR, (k, e)
        assert int(torch.count_nonzero(inputs[k, 0, :, n:])) == 0, k


# ------------------------------------------------------------------------------------------------------------ 4. other shapes
@pytest.mark.parametrize('rate,win,stride,n_fft,hop,lengths', [
    (8000, 0.02, 0.01, 160, 80, [81, 1003]),
    (16000, 0.004, 0.00625, 64, 100, [33, 7009]),                   # hop > n_fft: frames packed in LDS, samples skipped
])
def test_fused_equals_unfused_in_other_geometries(L, tmp_path, rate, win, stride, n_fft, hop, lengths):
    import mtl_amd
    inj = mtl_amd.NoiseInjection(make_noise_dir(tmp_path / 'bank', [9000, lengths[1]], rate=rate), sample_rate=rate)
    waves = [waveform(n, 20 + i, rate=rate) for i, n in enumerate(lengths)]
    noise_off, level = inj.plan([(0, 0.5, 1.0), (1, 0.3, 0.6)], lengths)
    assert noise_off.tolist() == [9000 - lengths[0], 9000]
    fe = mtl_amd.SpectrogramFrontEnd(rate, win, stride, 'hamming', normalize=True)
    assert (fe.n_fft, fe.hop) == (n_fft, hop)
    mixed, coef = device_mix(L, inj, waves, noise_off, level)
    assert (coef > 0).all()
    a, _ = fe.batch(waves, noise=(inj, noise_off, level))
    b, _ = fe.batch(mixed)
    clean, _ = fe.batch(waves)
    assert torch.equal(a, b) and not torch.equal(a[0], clean[0]) and not torch.equal(a[1], clean[1])


def test_a_batch_of_one_and_two_identical_calls(inj16, waves16, plan16, mixed16, fe16):
    fe, noise = fe16[True], (inj16,) + plan16
    one, size = fe.batch([waves16[2]], noise=(inj16, plan16[0][2:3], plan16[1][2:3]))
    assert tuple(one.shape) == (1, 1, 161, 8) and size.tolist() == [8]
    assert torch.equal(one, fe.batch([mixed16[0][2]])[0])
    a, _ = fe.batch(waves16, noise=noise)
    b, _ = fe.batch(waves16, noise=noise)
    assert torch.equal(a, b)
    assert torch.equal(one[0, 0], a[2, 0, :, :8])                     # an utterance's features do not depend on its neighbours
    with pytest.raises(ValueError):
        fe.batch(waves16[:2], noise=noise)                            # a plan for another number of utterances
    with pytest.raises(ValueError):
        fe.batch([waves16[4]], noise=(inj16, np.array([inj16.bank_len - 3999]), np.array([0.5], dtype=np.float32)))


# ------------------------------------------------------------------------------------------------------------ 5. ABI
def test_abi_rejects_bad_arguments_before_any_launch(L, inj16, waves16, plan16, fe16):
    import mtl_amd
    fe = fe16[True]
    flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves16[:3], fe.hop, fe.n_fft)
    K = len(frames)
    wav, off = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets).cuda()
    noff, lvl = torch.from_numpy(plan16[0][:K]).cuda(), torch.from_numpy(plan16[1][:K]).cuda()
    bank, blen = inj16.device_bank().data_ptr(), inj16.bank_len
    coef, mixed = torch.full((K,), 7.0, device='cuda'), torch.full_like(wav, 7.0)
    out = torch.full((K, 1, fe.F, tmax), 7.0, device='cuda')
    cneed, sneed = L.mtl_wave_mix_coef_workspace(K), L.mtl_spect_batch_workspace(int(frames.sum()), K, fe.F)
    assert cneed > 0 and L.mtl_wave_mix_coef_workspace(0) == -22 and L.mtl_wave_mix_coef_workspace(-3) == -22
    cws = torch.zeros(cneed // 8, dtype=torch.float64, device='cuda')
    sws = torch.zeros(sneed // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def coef_call(K_=K, bank_=bank, blen_=blen, ws_bytes=cneed, coef_=coef.data_ptr()):
        return L.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), K_, bank_, blen_, noff.data_ptr(), lvl.data_ptr(), coef_,
                                   cws.data_ptr(), ws_bytes)

    def mix_call(K_=K, bank_=bank, blen_=blen, out_=mixed.data_ptr()):
        return L.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), K_, bank_, blen_, noff.data_ptr(), coef.data_ptr(), out_)

    def spect_call(K_=K, bank_=bank, blen_=blen, ws_bytes=sneed, n_fft=fe.n_fft, coef_=coef.data_ptr()):
        return L.mtl_spect_batch_noise(st, wav.data_ptr(), off.data_ptr(), K_, n_fft, fe.hop, fe.basis.data_ptr(), fe.ldb, fe.F,
                                       out.data_ptr(), tmax, 1, sws.data_ptr(), ws_bytes, bank_, blen_, noff.data_ptr(), coef_)
    for call in (coef_call, mix_call, spect_call):
        assert call(bank_=None) == -22 and call(blen_=0) == -22 and call(blen_=-5) == -22 and call(K_=0) == -22, call.__name__
    assert coef_call(ws_bytes=cneed - 1) == -22 and coef_call(ws_bytes=0) == -22 and coef_call(coef_=None) == -22
    assert mix_call(out_=None) == -22
    assert spect_call(ws_bytes=sneed - 1) == -22 and spect_call(n_fft=fe.n_fft + 1) == -22 and spect_call(coef_=None) == -22
    torch.cuda.synchronize()
    assert bool((coef == 7.0).all()) and bool((mixed == 7.0).all()) and bool((out == 7.0).all())      # nothing was launched
    assert coef_call() == 0 and mix_call() == 0 and spect_call() == 0
    torch.cuda.synchronize()
    assert bool((coef != 7.0).all()) and bool((mixed != 7.0).all()) and bool((out != 7.0).all())


# ------------------------------------------------------------------------------------------------------------ 6. datasets / trainer
def _corpus(tmp_path, n=12):
    """n seeded 16-bit wavs of 0.3-0.7 s + transcripts, split into two manifests (as tests/test_frontend_batch_gpu.py)"""
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        write_wav(wp, waveform(int(16000 * (0.3 + 0.4 * i / (n - 1))), 40 + i))
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    manifests = []
    for m in range(2):
        p = tmp_path / ('train%d.csv' % m)
        p.write_text('\n'.join(rows[m::2]) + '\n')
        manifests.append(str(p))
    return manifests


def _dataset(vocab, manifests, device_batches, noise_dir, noise_prob):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=noise_prob,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(vocab, args, audio_conf, manifest_filepath_list=manifests, normalize=True, is_train=True, seed=7,
                                      device_batches=device_batches)


def test_dataset_with_noise_on_both_input_paths(tmp_path):
    import mtl_amd
    vocab = mtl_amd.synthetic_vocab(64)
    manifests = _corpus(tmp_path)
    noise_dir = make_noise_dir(tmp_path / 'bank', NOISE_LENGTHS)
    plain, batched = _dataset(vocab, manifests, False, noise_dir, 1.0), _dataset(vocab, manifests, True, noise_dir, 1.0)
    clean = _dataset(vocab, manifests, True, None, 1.0)
    for manifest_id in (0, 1):
        a, b, c = plain.sample(3, 2, manifest_id), batched.sample(3, 2, manifest_id), clean.sample(3, 2, manifest_id)
        for pa, pb, pc in zip(a, b, c):
            assert pb[0].is_cuda and not pa[0].is_cuda and pb[0].shape == pa[0].shape
            for x, y in zip(pa[1:], pb[1:]):                        # input_sizes, input_percentages, targets, target_sizes
                assert not y.is_cuda and x.dtype == y.dtype and torch.equal(x, y)
            for k in range(pa[0].size(0)):
                n = int(pa[1][k])
                e = rel(pb[0][k, 0, :, :n], pa[0][k, 0, :, :n])
                print('manifest %d, utterance %d: device batch vs per-utterance path %.2e' % (manifest_id, k, e))
                assert e < BAR, (manifest_id, k, e)
                assert int(torch.count_nonzero(pb[0][k, 0, :, n:])) == 0
            if manifest_id == 0:                                    # (the first call of the clean dataset picks the same utterances)
                assert pb[0].shape == pc[0].shape and not torch.equal(pb[0], pc[0])
    assert plain.noiseInjector.skipped == 0 and batched.noiseInjector.skipped == 0
    # noise_prob = 0: the draws are consumed, nothing is mixed -- bitwise the dataset without noise_dir, on both paths
    # (first calls are compared: afterwards the two index streams differ by the binomial draws)
    for mode in (False, True):
        for manifest_id in (0, 1):
            quiet, none = _dataset(vocab, manifests, mode, noise_dir, 0.0), _dataset(vocab, manifests, mode, None, 0.0)
            for pa, pb in zip(quiet.sample(3, 2, manifest_id), none.sample(3, 2, manifest_id)):
                assert all(torch.equal(x, y) for x, y in zip(pa, pb)), (mode, manifest_id)
    spect, transcript = plain[3]                                    # validation / test loaders inject too (every parse_audio)
    assert tuple(spect.shape[:1]) == (161,) and not spect.is_cuda and len(transcript) > 0


def test_two_train_iterations_with_noise_agree_between_the_two_input_paths(tmp_path):
    """The setup of test_two_train_iterations_agree_between_the_two_input_paths (tests/test_frontend_batch_gpu.py) with
    noise_prob = 1: finite losses, different from the clean run's (the noise reached the model), and EQUAL between host batches
    (per noisy utterance one batch([y], noise=...) call) and device batches (one call per part): both run the same kernel on the same
    staged samples, and an utterance's features do not depend on its neighbours."""
    from tests.test_parity_gpu import make
    z, cfg, spec = gu.load('F0')
    manifests = _corpus(tmp_path)
    noise_dir = make_noise_dir(tmp_path / 'bank', NOISE_LENGTHS)
    out = {}
    for name, mode, ndir in (('clean', True, None), ('host', False, noise_dir), ('device', True, noise_dir)):
        mtl_amd, args, vocab, model = make(cfg, spec, name='fe_noise_%s' % name)
        args.save_folder, args.k_train, args.k_valid = str(tmp_path), 3, 2
        model = model.cuda()
        tasks = [_dataset(vocab, manifests, mode, ndir, 1.0) for _ in range(2)]
        trainer = mtl_amd.TransientTrainer()
        trainer.train(model, vocab, tasks, [], 'ce', 0, 2, args, evaluate_every=10 ** 9, early_stop='cer,10', is_copy_grad=True)
        torch.cuda.synchronize()
        out[name] = [float(t[0]) for t in trainer.loss_trace]
    assert all(len(v) == 2 and all(np.isfinite(x) for x in v) for v in out.values()), out
    for a, b, c in zip(out['device'], out['host'], out['clean']):
        print('loss with device batches %.9g, with host batches %.9g (difference %.2e), clean %.9g' % (a, b, abs(a - b), c))
        assert a != c and b != c
        assert a == b, (a, b)
