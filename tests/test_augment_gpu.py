"""MI355X: the tempo / gain augmentation on the device (mtl_tempo_search / mtl_tempo_render, SpectrogramFrontEnd.tempo_gain and
batch(augment=), the datasets) against the fp64 restatement of tests/augment_util.py -- the DEFINITION of the behaviour, parity with
sox unpinned.  The references are computed once per case (augment_util.reference) and shared."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import augment_util as au

pytestmark = pytest.mark.gpu

CASES_16K = [i for i, c in enumerate(au.CASES) if c[4] == 16000]
CASES_8K = [i for i, c in enumerate(au.CASES) if c[4] == 8000]


@pytest.fixture(scope='module')
def fe():
    import mtl_amd
    assert torch.cuda.is_available()
    return {16000: mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=True),
            8000: mtl_amd.SpectrogramFrontEnd(8000, 0.02, 0.01, 'hamming', normalize=True)}


def _run(fe, cases, quantize):
    """one tempo_gain call over `cases` (all of one sample rate) -> ({case: stretched}, {case: seg_off})"""
    rate = au.CASES[cases[0]][4]
    waves = [au.reference(i)['x'] for i in cases]
    tempo, gain_db = [au.CASES[i][2] for i in cases], [au.CASES[i][3] for i in cases]
    outs, seg_off = fe[rate].tempo_gain(waves, tempo, gain_db, quantize=quantize)
    assert len(outs) == len(cases) and seg_off.dtype == np.int32
    segs, at = {}, 0
    for i in cases:
        n = len(au.reference(i)['offsets'])
        segs[i] = seg_off[at:at + n]
        at += n
    assert at == len(seg_off)
    return dict(zip(cases, outs)), segs


@pytest.fixture(scope='module')
def raw(fe):
    a, sa = _run(fe, CASES_16K, False)
    b, sb = _run(fe, CASES_8K, False)
    return {**a, **b}, {**sa, **sb}


@pytest.fixture(scope='module')
def quantized(fe):
    a, sa = _run(fe, CASES_16K, True)
    b, sb = _run(fe, CASES_8K, True)
    return {**a, **b}, {**sa, **sb}


@pytest.mark.parametrize('case', range(len(au.CASES)))
def test_every_offset_of_the_search_equals_the_restatement(raw, quantized, case):
    ref = au.reference(case)
    for _, segs in (raw, quantized):
        assert segs[case].tolist() == ref['offsets'].tolist(), case


@pytest.mark.parametrize('case', range(len(au.CASES)))
def test_raw_overlap_add_within_the_bound_of_the_fp32_expression(raw, case):
    ref, got = au.reference(case), raw[0][case]
    assert got.dtype == np.float32 and got.shape == (ref['N'],)
    err = np.abs(got.astype(np.float64) - ref['out'])
    bound = 4 * 2.0 ** -24 * (np.abs(ref['tail']) + np.abs(ref['cur']))
    worst = float((err / np.maximum(bound, 1e-300)).max()) if len(err) else 0.0
    print('case %d: %d samples, worst error / bound %.3f, samples not exact %d' % (case, ref['N'], worst, int((err > 0).sum())))
    assert (err <= bound).all(), (case, worst)


@pytest.mark.parametrize('case', range(len(au.CASES)))
def test_quantised_output_against_the_restatement(quantized, case):
    ref, got = au.reference(case), quantized[0][case]
    assert got.dtype == np.float32 and got.shape == (ref['N'],)
    q = got.astype(np.float64) * 32768.0
    assert np.array_equal(q, np.rint(q)) and q.min() >= -32768 and q.max() <= 32767      # on the int16 grid
    diff = np.abs(q.astype(np.int64) - ref['q'])
    share = float((diff > 0).mean())
    print('case %d: %d samples, largest step difference %d, share that differs %.2e' % (case, ref['N'], int(diff.max()), share))
    assert diff.max() <= 1, case
    assert share <= 2e-3, (case, share)


def _noise_bank(tmp_path):
    import mtl_amd
    d = tmp_path / 'noise'
    d.mkdir()
    for i, n in enumerate((30000, 40000)):
        with wave.open(str(d / ('n%d.wav' % i)), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.rint(au.waveform(n, 70 + i)[::-1].astype(np.float64) * 32768.0).astype('<i2').tobytes())
    return mtl_amd.NoiseInjection(str(d), 16000, (0.1, 0.5))


def test_batch_with_augment_is_bitwise_batch_of_the_stretched_waveforms(fe, quantized, tmp_path):
    f16 = fe[16000]
    cases = [i for i in CASES_16K if au.reference(i)['N'] >= f16.n_fft // 2 + 1]
    assert len(cases) == len(CASES_16K)
    waves = [au.reference(i)['x'] for i in cases]
    tempo = np.array([au.CASES[i][2] for i in cases])
    gain_db = np.array([au.CASES[i][3] for i in cases], dtype=np.float32)
    stretched = [quantized[0][i] for i in cases]
    a, sa = f16.batch(waves, augment=(tempo, gain_db))
    b, sb = f16.batch(stretched)
    assert sa.tolist() == sb.tolist() == [1 + au.reference(i)['N'] // 160 for i in cases] and a.shape == b.shape
    assert torch.equal(a, b)
    # ... with max_frames cutting the longest utterances
    a, sa = f16.batch(waves, max_frames=60, augment=(tempo, gain_db))
    b, sb = f16.batch(stretched, max_frames=60)
    assert sa.tolist() == sb.tolist() and max(sa.tolist()) == 60 and min(sa.tolist()) < 60 and torch.equal(a, b)
    # ... and with a noise plan on top, made for the stretched lengths (every utterance noisy)
    inj = _noise_bank(tmp_path)
    rng = np.random.RandomState(1)
    plan = inj.plan([inj.draw(rng, 1.0) for _ in cases], [len(s) for s in stretched])
    assert (plan[0] >= 0).all()
    a, sa = f16.batch(waves, max_frames=60, noise=(inj,) + plan, augment=(tempo, gain_db))
    b, sb = f16.batch(stretched, max_frames=60, noise=(inj,) + plan)
    c, _ = f16.batch(stretched, max_frames=60)
    assert sa.tolist() == sb.tolist() and torch.equal(a, b) and not torch.equal(a, c)
    # a noise plan made for the ORIGINAL lengths of slowed-down utterances can end beyond the bank: refused on the host
    with pytest.raises(ValueError, match='beyond the bank'):
        f16.batch([waves[3]], noise=(inj, np.array([inj.bank_len - 16037]), np.array([0.3], dtype=np.float32)), augment=(tempo[3:4], gain_db[3:4]))
    # the n_fft // 2 + 1 minimum applies to the stretched length: 180 samples at 1.15 become 157
    assert f16.batch([waves[2][:180]])[1].tolist() == [2]
    with pytest.raises(ValueError, match='after the tempo change'):
        f16.batch([waves[2][:180]], augment=(np.array([1.15]), np.array([0.0], dtype=np.float32)))


def test_abi_rejects_bad_arguments_before_any_launch(fe):
    import mtl_amd
    L = mtl_amd._lib.lib()
    ref = au.reference(2)
    tab = mtl_amd.tempo_gain_tables([ref['x']], [au.CASES[2][2]], [au.CASES[2][3]], 16000)
    d = {k: torch.from_numpy(tab[k]).cuda() for k in ('flat', 'offsets', 'out_offsets', 'seg_base', 'tempo', 'gain')}
    seg_off = torch.full((int(tab['seg_base'][-1]),), -7, dtype=torch.int32, device='cuda')
    out = torch.full((int(tab['out_offsets'][-1]),), 7.0, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def search(K=1, S=1312, R=235, O=192, seg=seg_off.data_ptr(), tempo=d['tempo'].data_ptr()):
        return L.mtl_tempo_search(st, d['flat'].data_ptr(), d['offsets'].data_ptr(), d['out_offsets'].data_ptr(), tempo, d['seg_base'].data_ptr(),
                                  K, S, R, O, seg)

    def render(K=1, S=1312, R=235, O=192, quantize=1, gain=d['gain'].data_ptr(), out_=out.data_ptr()):
        return L.mtl_tempo_render(st, d['flat'].data_ptr(), d['offsets'].data_ptr(), d['out_offsets'].data_ptr(), d['tempo'].data_ptr(), gain,
                                  d['seg_base'].data_ptr(), seg_off.data_ptr(), K, S, R, O, quantize, out_)
    assert search(K=0) == -22 and search(R=256) == -22 and search(O=257) == -22 and search(O=0) == -22 and search(S=192) == -22
    assert search(seg=None) == -22 and search(tempo=None) == -22 and search(R=-1) == -22
    assert render(K=0) == -22 and render(R=256) == -22 and render(O=0) == -22 and render(S=100) == -22 and render(out_=None) == -22
    assert render(gain=None) == -22
    torch.cuda.synchronize()
    assert bool((seg_off == -7).all()) and bool((out == 7.0).all())              # nothing was launched
    assert search() == 0 and render(gain=None, quantize=0) == 0                  # (the raw form does not read the gains)
    torch.cuda.synchronize()
    assert seg_off.cpu().tolist() == ref['offsets'].tolist() and bool((out != 7.0).any())


# ------------------------------------------------------------------------------------------------------------------ datasets
def _corpus(tmp_path, n=8):
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.rint(au.waveform(4800 + 700 * i, 40 + i).astype(np.float64) * 32768.0).astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


def test_dataset_sample_with_augment_and_noise(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path)
    inj = _noise_bank(tmp_path)
    noise_dir = str(tmp_path / 'noise')
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=noise_dir, noise_prob=0.5,
                      noise_levels=(0.1, 0.5))

    def dataset(augment):
        return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                          augment=augment, is_train=True, seed=7, device_batches=True)
    a, b, plain = dataset(True), dataset(True), dataset(False)
    # the stream restated: the lengths the sizes must follow
    mirror = np.random.RandomState(7)
    picks = mirror.choice(np.arange(0, 8), 5, p=a.proba[0], replace=True)
    stretched = []
    for j in picks:
        tempo = float('{:.3f}'.format(mirror.uniform(low=0.85, high=1.15)))
        mirror.uniform(low=-6, high=8)
        inj.draw(mirror, 0.5)
        stretched.append(mtl_amd.TempoGainAugment.out_length(4800 + 700 * int(j), tempo))
    ta, va = a.sample(3, 2, 0)
    tb, vb = b.sample(3, 2, 0)
    tp, vp = plain.sample(3, 2, 0)
    assert a.rng.rand() == b.rng.rand() == mirror.rand()
    for pa, pb, pp, want in ((ta, tb, tp, stretched[:3]), (va, vb, vp, stretched[3:])):
        sizes = [min(1 + n // 160, 50) for n in want]
        assert pa[0].is_cuda and tuple(pa[0].shape) == (len(want), 1, 161, max(sizes)) and pa[1].tolist() == sizes
        assert torch.equal(pa[2], pa[1].float() / float(max(sizes)))
        assert bool(torch.isfinite(pa[0]).all())
        for k in range(len(want)):
            assert int(torch.count_nonzero(pa[0][k, 0, :, sizes[k]:])) == 0
        for x, y in zip(pa, pb):                                    # a second dataset with the same seed: identical
            assert torch.equal(x, y)
        assert torch.equal(pa[3], pp[3]) and torch.equal(pa[4], pp[4])      # the same utterances ...
        assert pa[0].shape != pp[0].shape or not torch.equal(pa[0], pp[0])  # ... not the same features
    # the per-item path: K = 1 through the same calls
    spect, transcript = a[0]
    assert not spect.is_cuda and spect.shape[0] == 161 and 0 < spect.shape[1] <= 50 and len(transcript) > 0


def test_load_randomly_augmented_audio(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path, n=1)
    path = str(tmp_path / 'u0.wav')
    np.random.seed(3)
    y = mtl_amd.load_randomly_augmented_audio(path)
    mirror = np.random.RandomState(3)
    tempo = float('{:.3f}'.format(mirror.uniform(low=0.85, high=1.15)))
    gain = float('{:.3f}'.format(mirror.uniform(low=-6, high=8)))
    assert np.random.rand() == mirror.rand()
    x = mtl_amd.load_wav_pcm16(path)
    ref = au.gain_quantize(au.wsola(x, tempo)['out'], gain)
    assert y.dtype == np.float32 and y.shape == ref.shape == (au.out_length(4800, tempo),)
    diff = np.abs(np.rint(y.astype(np.float64) * 32768).astype(np.int64) - ref)
    assert diff.max() <= 1 and (diff > 0).mean() <= 2e-3
