"""MI355X: the batched spectrogram front-end (mtl_spect_batch / SpectrogramFrontEnd.batch / device_batches) against the numpy oracle
of the reference's parse_audio and against the per-utterance device path.  `rel` is taken PER UTTERANCE (a two-frame utterance is not
hidden behind a long one); the bar is the front-end's own 2e-5 (tests/test_ops_gpu.py, fp32 DFT-as-GEMM against a float32 FFT)."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import golden_util as gu

pytestmark = pytest.mark.gpu

BAR = 2e-5
LENGTHS_16K = [161, 480, 1121, 16037, 4000]     # 2 frames (both ends reflected in one tile) | multiple of hop | ragged | 101 frames: two row tiles | mid
LENGTHS_8K = [81, 800, 1003]


@pytest.fixture(scope='module')
def L():
    import mtl_amd
    assert torch.cuda.is_available()
    return mtl_amd._lib.lib()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def waveform(n, seed, rate=16000):
    """0.3 sin(2 pi 440 t) + 0.05 noise under a linear gain ramp 0.2 -> 1.5: the ramp makes 'normalise, then cut' and 'cut, then
    normalise' differ by order 1, so statistics taken over the wrong frames cannot pass"""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(rate)
    return ((0.3 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.randn(n)) * np.linspace(0.2, 1.5, n)).astype(np.float32)


@pytest.fixture(scope='module')
def waves16():
    return [waveform(n, 10 + i) for i, n in enumerate(LENGTHS_16K)]


@pytest.fixture(scope='module')
def oracle16(waves16):
    """computed once, shared and left unchanged: {normalize: [parse_audio(y) per utterance]}"""
    from oracle import frontend
    return {norm: [frontend.parse_audio(y, normalize=norm) for y in waves16] for norm in (True, False)}


@pytest.fixture(scope='module')
def fe16():
    import mtl_amd
    return {norm: mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=norm) for norm in (True, False)}


def check_padding(inputs, sizes):
    for k in range(inputs.size(0)):
        assert int(torch.count_nonzero(inputs[k, 0, :, int(sizes[k]):])) == 0, k


@pytest.mark.parametrize('normalize', [True, False])
def test_batch_matches_the_oracle_per_utterance(waves16, oracle16, fe16, normalize):
    inputs, sizes = fe16[normalize].batch(waves16)
    assert inputs.is_cuda and inputs.dtype == torch.float32 and tuple(inputs.shape) == (5, 1, 161, 101)
    assert not sizes.is_cuda and sizes.dtype == torch.int32 and sizes.tolist() == [2, 4, 8, 101, 26]
    for k, ref in enumerate(oracle16[normalize]):
        e = rel(inputs[k, 0, :, :int(sizes[k])], ref)
        print('batch vs oracle, normalize=%s, utterance %d (%d frames): %.2e' % (normalize, k, int(sizes[k]), e))
        assert e < BAR, (k, e)
    check_padding(inputs, sizes)


def test_padding_is_exact_zero_also_in_recycled_memory(waves16, fe16):
    fe = fe16[True]
    inputs, sizes = fe.batch(waves16)
    check_padding(inputs, sizes)
    torch.cuda.synchronize()
    del inputs                                                   # the allocator may hand the block (full of features) to the next batch
    short, ssz = fe.batch(waves16[:3])
    assert tuple(short.shape) == (3, 1, 161, 8) and ssz.tolist() == [2, 4, 8]
    check_padding(short, ssz)


def test_truncation_keeps_the_statistics_of_the_whole_utterance(waves16, oracle16, fe16):
    inputs, sizes = fe16[True].batch(waves16, max_frames=20)
    assert tuple(inputs.shape) == (5, 1, 161, 20) and sizes.tolist() == [2, 4, 8, 20, 20]
    for k, ref in enumerate(oracle16[True]):
        n = int(sizes[k])
        e = rel(inputs[k, 0, :, :n], ref[:, :n])
        print('batch(max_frames=20) vs oracle[:, :n], utterance %d: %.2e' % (k, e))
        assert e < BAR, (k, e)
    check_padding(inputs, sizes)


@pytest.mark.parametrize('window', ['hann', 'hamming'])
def test_another_geometry_8khz(window):
    """n_fft 160, hop 80, F 81, ldb 164: Hann against the per-utterance device path (the oracle's window is Hamming only), Hamming
    against the oracle as well"""
    import mtl_amd
    from oracle import frontend
    waves = [waveform(n, 20 + i, rate=8000) for i, n in enumerate(LENGTHS_8K)]
    fe = mtl_amd.SpectrogramFrontEnd(8000, 0.02, 0.01, window, normalize=True)
    assert (fe.n_fft, fe.hop, fe.F, fe.ldb) == (160, 80, 81, 164)
    inputs, sizes = fe.batch(waves)
    assert tuple(inputs.shape) == (3, 1, 81, 13) and sizes.tolist() == [2, 11, 13]
    for k, y in enumerate(waves):
        n = int(sizes[k])
        e = rel(inputs[k, 0, :, :n], fe(y))
        print('8 kHz %s, utterance %d: vs __call__ %.2e' % (window, k, e))
        assert e < BAR, (k, e)
        if window == 'hamming':
            e = rel(inputs[k, 0, :, :n], frontend.parse_audio(y, sample_rate=8000))
            print('8 kHz hamming, utterance %d: vs oracle %.2e' % (k, e))
            assert e < BAR, (k, e)
    check_padding(inputs, sizes)


@pytest.mark.parametrize('rate,win,stride,n_fft,hop,lengths,frames', [
    (16000, 0.064, 0.032, 1024, 512, [513, 3000, 40 * 512 + 5], [2, 6, 41]),        # span of 64 frames exceeds the LDS budget: 32-frame row tiles
    (16000, 0.064, 0.064, 1024, 1024, [513, 20 * 1024 + 3], [1, 21]),               # ... 16-frame row tiles, frames that just do not overlap
    (16000, 0.004, 0.00625, 64, 100, [33, 70 * 100 + 9], [1, 71]),                  # hop > n_fft: frames packed in LDS, samples skipped
])
def test_the_other_row_tile_widths_and_frames_that_do_not_overlap(rate, win, stride, n_fft, hop, lengths, frames):
    """The kernel picks 64-, 32- or 16-frame row tiles by what fits its LDS span and packs the frames when hop > n_fft; each case has
    an utterance of more than one row tile and one of the shortest accepted length.  Against the per-utterance path and the oracle at
    the front-end's bar: a k-ordered fp32 sum of K = 1024 products carries a rounding error of about sqrt(K) 2^-24 = 1.9e-6 of the
    operands' norm (4e-7 measured at K = 320), a tenth of the bar."""
    import mtl_amd
    from oracle import frontend
    waves = [waveform(n, 30 + i, rate=rate) for i, n in enumerate(lengths)]
    fe = mtl_amd.SpectrogramFrontEnd(rate, win, stride, 'hamming', normalize=True)
    assert (fe.n_fft, fe.hop) == (n_fft, hop)
    inputs, sizes = fe.batch(waves)
    assert sizes.tolist() == frames and tuple(inputs.shape) == (len(lengths), 1, n_fft // 2 + 1, max(frames))
    for k, y in enumerate(waves):
        n = int(sizes[k])
        e1 = rel(inputs[k, 0, :, :n], fe(y))
        e2 = rel(inputs[k, 0, :, :n], frontend.parse_audio(y, sample_rate=rate, window_size=win, window_stride=stride))
        print('n_fft %d hop %d, utterance %d (%d frames): vs __call__ %.2e, vs oracle %.2e' % (n_fft, hop, k, n, e1, e2))
        assert e1 < BAR and e2 < BAR, (k, e1, e2)
    check_padding(inputs, sizes)


def test_an_utterance_of_more_row_tiles_than_workgroups(fe16):
    """2101 frames = 33 row tiles of 64: the first of the utterance's 32 workgroups per frequency block stages and multiplies a
    second tile (the loop with its barriers), beside a short utterance whose workgroups mostly have nothing to do"""
    from oracle import frontend
    waves = [waveform(2100 * 160 + 7, 50), waveform(700, 51)]
    inputs, sizes = fe16[True].batch(waves)
    assert sizes.tolist() == [2101, 5] and tuple(inputs.shape) == (2, 1, 161, 2101)
    for k, y in enumerate(waves):
        e = rel(inputs[k, 0, :, :int(sizes[k])], frontend.parse_audio(y))
        print('2101 + 5 frames, utterance %d: vs oracle %.2e' % (k, e))
        assert e < BAR, (k, e)
    check_padding(inputs, sizes)


def test_a_batch_of_one(waves16, oracle16, fe16):
    y = waves16[2]
    inputs, sizes = fe16[True].batch([y])
    assert tuple(inputs.shape) == (1, 1, 161, 8) and sizes.tolist() == [8]
    assert rel(inputs[0, 0], fe16[True](y)) < BAR
    assert rel(inputs[0, 0], oracle16[True][2]) < BAR


def test_two_calls_are_bitwise_equal(waves16, fe16):
    a, _ = fe16[True].batch(waves16)
    b, _ = fe16[True].batch(waves16)
    assert torch.equal(a, b)
    c, sizes = fe16[True].batch(waves16, max_frames=20)          # cutting changes which frames are stored, not their values
    for k in range(5):
        assert torch.equal(c[k, 0, :, :int(sizes[k])], a[k, 0, :, :int(sizes[k])]), k


def test_abi_rejects_bad_arguments_before_any_launch(L, waves16, fe16):
    import mtl_amd
    fe = fe16[True]
    flat, offsets, frames, tmax = mtl_amd.pack_waveforms(waves16[:3], fe.hop, fe.n_fft)      # lengths through the host packer only
    K = len(frames)
    wav, off = torch.from_numpy(flat).cuda(), torch.from_numpy(offsets).cuda()
    out = torch.full((K, 1, fe.F, tmax), 7.0, device='cuda')
    need = L.mtl_spect_batch_workspace(int(frames.sum()), K, fe.F)
    assert need > 0 and L.mtl_spect_batch_workspace(0, K, fe.F) == -22 and L.mtl_spect_batch_workspace(10, 0, fe.F) == -22
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def call(K_=K, n_fft=fe.n_fft, F=fe.F, out_=out.data_ptr(), ws_bytes=need, hop=fe.hop, tmax_=tmax, ldb=fe.ldb):
        return L.mtl_spect_batch(st, wav.data_ptr(), off.data_ptr(), K_, n_fft, hop, fe.basis.data_ptr(), ldb, F, out_, tmax_, 1,
                                 ws.data_ptr(), ws_bytes)
    assert call(K_=0) == -22
    assert call(out_=None) == -22
    assert call(n_fft=fe.n_fft + 1) == -22 and call(n_fft=fe.n_fft + 1, F=fe.F + 1) == -22        # odd n_fft, whatever F claims
    assert call(ws_bytes=need - 1) == -22 and call(ws_bytes=0) == -22
    assert call(hop=0) == -22 and call(tmax_=0) == -22 and call(n_fft=2048, F=1025, ldb=2052) == -22 and call(ldb=2 * fe.F - 1) == -22
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())


# ------------------------------------------------------------------------------------------------------------ datasets / trainer
def _corpus(tmp_path, n=12):
    """n seeded 16-bit wavs of 0.3-0.7 s + transcripts, split into two manifests"""
    rows = []
    for i in range(n):
        y = waveform(int(16000 * (0.3 + 0.4 * i / (n - 1))), 40 + i)
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes((np.clip(y, -1, 1) * 32767).astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    manifests = []
    for m in range(2):
        p = tmp_path / ('train%d.csv' % m)
        p.write_text('\n'.join(rows[m::2]) + '\n')
        manifests.append(str(p))
    return manifests


def _dataset(vocab, manifests, device_batches):
    import mtl_amd
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.4,
                      noise_levels=(0.0, 0.5))
    return mtl_amd.SpectrogramDataset(vocab, args, audio_conf, manifest_filepath_list=manifests, normalize=True, is_train=True, seed=7,
                                      device_batches=device_batches)


def test_dataset_sample_on_the_device_equals_the_per_utterance_path(tmp_path):
    import mtl_amd
    vocab = mtl_amd.synthetic_vocab(64)
    manifests = _corpus(tmp_path)
    plain, batched = _dataset(vocab, manifests, False), _dataset(vocab, manifests, True)
    cut = 0
    for manifest_id in (0, 1, 0):
        a, b = plain.sample(3, 2, manifest_id), batched.sample(3, 2, manifest_id)
        for pa, pb in zip(a, b):
            assert pb[0].is_cuda and not pa[0].is_cuda and pb[0].shape == pa[0].shape
            for x, y in zip(pa[1:], pb[1:]):                        # input_sizes, input_percentages, targets, target_sizes
                assert not y.is_cuda and x.dtype == y.dtype and torch.equal(x, y)
            for k in range(pa[0].size(0)):
                n = int(pa[1][k])
                assert rel(pb[0][k, 0, :, :n], pa[0][k, 0, :, :n]) < BAR, (manifest_id, k)
            check_padding(pb[0], pb[1])
            cut += int((pa[1] == 50).sum())
    assert cut > 0                                                  # some utterance was longer than src_max_len: the cut path ran
    tr, va = batched.sample(3, 2, 1, need=(True, False))
    assert va is None and tr[0].is_cuda
    tr, va = batched.sample(3, 2, 1, need=(False, True))
    assert tr is None and tuple(va[0].shape[:3]) == (2, 1, 161)


def test_two_train_iterations_agree_between_the_two_input_paths(tmp_path):
    """TransientTrainer.train on the manifest dataset, once with host batches (per-utterance front-end, collate, upload) and once with
    device_batches=True, same seeds.  Measured on the MI355X against the device_batches=False run: the losses of
    both iterations are EQUAL (3.90819681 and 4.1102376 in either mode, difference 0) -- the exact-fp32 matrix instructions of both
    front-ends sum a frame's 320 products in the same order -- so equality is what is asserted."""
    from tests.test_parity_gpu import make
    z, cfg, spec = gu.load('F0')
    manifests = _corpus(tmp_path)
    out = {}
    for mode in (False, True):
        mtl_amd, args, vocab, model = make(cfg, spec, name='fe_batch_%d' % mode)
        args.save_folder, args.k_train, args.k_valid = str(tmp_path), 3, 2
        model = model.cuda()
        tasks = [_dataset(vocab, manifests, mode) for _ in range(2)]
        trainer = mtl_amd.TransientTrainer()
        trainer.train(model, vocab, tasks, [], 'ce', 0, 2, args, evaluate_every=10 ** 9, early_stop='cer,10', is_copy_grad=True)
        torch.cuda.synchronize()
        out[mode] = [float(t[0]) for t in trainer.loss_trace]
    assert len(out[False]) == len(out[True]) == 2 and all(np.isfinite(v) for v in out[False] + out[True])
    for a, b in zip(out[True], out[False]):
        print('loss with device batches %.9g, with host batches %.9g, relative difference %.2e' % (a, b, abs(a - b) / abs(b)))
        assert a == b, (a, b)
