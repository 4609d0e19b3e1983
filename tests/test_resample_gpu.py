"""MI355X: the sample-rate conversion on the device (mtl_resample, resample, SpectrogramFrontEnd.batch(rates=), the datasets) against the
fp64 restatement of tests/resample_util.py -- the DEFINITION of the behaviour, parity with sox unpinned.  The device results and the
restatements are computed once (module fixtures) and shared."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import resample_util as ru

pytestmark = pytest.mark.gpu

# (samples, rate) of one call to 16 kHz: every ratio of ru.RATIOS that ends there, two lengths at 8 kHz, and the bypass
TO_16K = [(5, 22050), (161, 8000), (1203, 8000), (4001, 48000), (3000, 44100), (2000, 11025), (999, 16000)]
TO_8K = [(1203, 16000)]            # a second call, K = 1
NEIGHBOURS = [(700, 8000), (500, 8000), (900, 48000)]       # loud, SILENT, loud


def _waves(cases, seed):
    return [ru.waveform(n, seed + i, r, level=0.45) for i, (n, r) in enumerate(cases)]


@pytest.fixture(scope='module')
def calls():
    """name -> (cases, target, waves, restatement per utterance (y, ab, terms)): the inputs of the three calls and what they must give"""
    out = {}
    for name, cases, target in (('to16k', TO_16K, 16000), ('to8k', TO_8K, 8000), ('neighbours', NEIGHBOURS, 16000)):
        waves = _waves(cases, 11)
        if name == 'neighbours':
            waves[1] = np.zeros_like(waves[1])
        ref = []
        for x, (n, r) in zip(waves, cases):
            up, down = ru.ratio(r, target)
            if up == down:
                ref.append((x.astype(np.float64), np.abs(x.astype(np.float64)), np.ones(n, dtype=np.int64)))
            else:
                ref.append(ru.restate(x, up, down, ru.taps(up, down)))
        out[name] = (cases, target, waves, ref)
    return out


@pytest.fixture(scope='module')
def device(calls):
    """(name, quantize) -> the list that `resample` returns"""
    import mtl_amd
    assert torch.cuda.is_available()
    return {(name, q): mtl_amd.resample(waves, [r for _, r in cases], target, quantize=q)
            for name, (cases, target, waves, _) in calls.items() for q in (True, False)}


@pytest.mark.parametrize('name', ['to16k', 'to8k', 'neighbours'])
def test_no_restated_sample_is_near_a_rounding_boundary(calls, name):
    """CPU part of the exact comparison below: the device's fp64 sums lie within 1e-10 LSB of the restatement's (about a hundred terms of
    at most 2^-53 relative each), so a sample rounds alike on both sides unless it sits on a boundary: none is within 2^-20 LSB"""
    for (n, r), (y, _, _) in zip(calls[name][0], calls[name][3]):
        d = float(ru.boundary_distance(y).min())
        print('%s: %d samples at %d Hz: closest to a rounding boundary %.3e LSB' % (name, n, r, d))
        assert d > 2.0 ** -20


@pytest.mark.parametrize('name', ['to16k', 'to8k', 'neighbours'])
def test_quantised_output_equals_the_restatement(calls, device, name):
    cases, target, waves, ref = calls[name]
    got = device[(name, True)]
    assert len(got) == len(cases)
    for k, ((n, r), (y, _, _)) in enumerate(zip(cases, ref)):
        up, down = ru.ratio(r, target)
        assert got[k].dtype == np.float32 and got[k].shape == (ru.out_length(n, up, down),), k
        if up == down:
            assert np.array_equal(got[k], waves[k]), k                                # the bypass: bit for bit
            continue
        q = got[k].astype(np.float64) * 32768.0
        assert np.array_equal(q, np.rint(q))                                          # on the int16 grid
        assert np.array_equal(q.astype(np.int64), ru.quantize(y)), (k, int(np.abs(q.astype(np.int64) - ru.quantize(y)).max()))
    if name == 'neighbours':                                                          # nothing of either neighbour leaks into the silence
        assert got[1].shape == (1000,) and not got[1].any() and np.abs(got[0]).max() > 0.3 and np.abs(got[2]).max() > 0.3
        assert not device[(name, False)][1].any()


@pytest.mark.parametrize('name', ['to16k', 'to8k', 'neighbours'])
def test_raw_output_within_the_bound_of_the_fp64_sum(calls, device, name):
    cases, target, waves, ref = calls[name]
    got = device[(name, False)]
    for k, ((n, r), (y, ab, terms)) in enumerate(zip(cases, ref)):
        assert got[k].dtype == np.float32 and got[k].shape == y.shape, k
        if ru.ratio(r, target) == (1, 1):
            assert np.array_equal(got[k], waves[k]), k
            continue
        err = np.abs(got[k].astype(np.float64) - y)
        bound = 2.0 ** -24 * np.abs(y) + (terms + 1) * 2.0 ** -53 * ab
        print('%s %d: %d samples, up to %d terms, worst error / bound %.3f' % (name, k, len(y), terms.max(), float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), k


def test_a_second_run_is_bitwise_the_first(calls, device):
    import mtl_amd
    cases, target, waves, _ = calls['to16k']
    for q in (True, False):
        again = mtl_amd.resample(waves, [r for _, r in cases], target, quantize=q)
        assert all(np.array_equal(a, b) for a, b in zip(again, device[('to16k', q)]))
    # K = 1 gives what the utterance gave inside the batch
    alone = mtl_amd.resample(waves[4:5], [cases[4][1]], target)
    assert len(alone) == 1 and np.array_equal(alone[0], device[('to16k', True)][4])


def test_indices_beyond_2_to_the_31(calls):
    """one utterance of 13.5 M samples at 44.1 kHz: j down passes 2^31 at output 4869578.  The first 64 outputs, the last 64 and the 64
    around that point against the restatement"""
    import mtl_amd
    L, up, down = 13500000, 160, 441
    rng = np.random.RandomState(5)
    x = (rng.randint(-12000, 12000, size=L).astype(np.float32) + np.float32(8000.0) * np.sin(np.arange(L, dtype=np.float32) * np.float32(0.37))) / 32768.0
    x = (np.rint(x * 32768.0) / 32768.0).astype(np.float32)
    N = ru.out_length(L, up, down)
    cross = 2 ** 31 // down
    assert N == 4897960 and (N - 1) * down > 2 ** 31 and cross * down < 2 ** 31 <= (cross + 1) * down
    js = np.concatenate([np.arange(64), np.arange(cross - 31, cross + 33), np.arange(N - 64, N)])
    y, _, terms = ru.restate(x, up, down, ru.taps(up, down), js)
    assert 88 <= terms.max() <= 89 and float(ru.boundary_distance(y).min()) > 2.0 ** -20
    got = mtl_amd.resample([x], [44100], 16000)[0]
    assert got.shape == (N,)
    q = np.rint(got[js].astype(np.float64) * 32768.0).astype(np.int64)
    assert np.array_equal(q, ru.quantize(y)), np.flatnonzero(q != ru.quantize(y))
    assert np.abs(q).max() > 1000 and np.abs(got).max() <= 1.0


def test_abi_rejects_bad_arguments_before_any_launch(calls):
    import mtl_amd
    L = mtl_amd._lib.lib()
    cases, target, waves, ref = calls['to8k']
    tab = mtl_amd.resample_tables(waves, [16000], 8000)
    d = {k: torch.from_numpy(tab[k]).cuda() for k in ('flat', 'offsets', 'out_offsets', 'plan', 'taps')}
    n = int(tab['out_offsets'][-1])
    out = torch.full((n + 64,), 7.0, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def run(K=1, n_taps=tab['taps'].shape[0], plan=d['plan'].data_ptr(), taps=d['taps'].data_ptr(), out_=out.data_ptr(), quantize=1):
        return L.mtl_resample(st, d['flat'].data_ptr(), d['offsets'].data_ptr(), d['out_offsets'].data_ptr(), plan, taps, n_taps, K, quantize, out_)
    assert run(K=0) == -22 and run(K=(1 << 20) + 1) == -22 and run(n_taps=0) == -22
    assert run(plan=None) == -22 and run(taps=None) == -22 and run(out_=None) == -22
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                   # nothing was launched
    # a table that claims more taps than were uploaded is not read: zeros, and nothing beyond the utterance is written
    assert run(n_taps=tab['taps'].shape[0] - 1) == 0
    torch.cuda.synchronize()
    assert bool((out[:n] == 0.0).all()) and bool((out[n:] == 7.0).all())
    assert run() == 0
    torch.cuda.synchronize()
    assert np.array_equal(np.rint(out[:n].cpu().numpy().astype(np.float64) * 32768).astype(np.int64), ru.quantize(ref[0][0]))
    assert bool((out[n:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ batch
@pytest.fixture(scope='module')
def fe():
    import mtl_amd
    return mtl_amd.SpectrogramFrontEnd(16000, 0.02, 0.01, 'hamming', normalize=True)


def _write_wav(path, y, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.rint(np.asarray(y, dtype=np.float64) * 32768.0).astype('<i2').tobytes())


def _noise_bank(tmp_path):
    import mtl_amd
    d = tmp_path / 'noise'
    d.mkdir()
    for i, n in enumerate((30000, 40000)):
        _write_wav(d / ('n%d.wav' % i), ru.waveform(n, 70 + i, 16000)[::-1], 16000)
    return mtl_amd.NoiseInjection(str(d), 16000, (0.1, 0.5))


def test_batch_with_rates_is_bitwise_batch_of_the_converted_waveforms(fe, calls, device, tmp_path):
    import mtl_amd
    cases, _, waves, _ = calls['to16k']
    keep = [k for k in range(len(cases)) if len(device[('to16k', True)][k]) >= fe.n_fft // 2 + 1]
    assert len(keep) == 6                                                             # all but the 5-sample utterance
    waves, rates = [waves[k] for k in keep], [cases[k][1] for k in keep]
    converted = [device[('to16k', True)][k] for k in keep]
    lengths = [len(c) for c in converted]
    assert lengths == [322, 2406, 1334, 1089, 2903, 999] == mtl_amd.resample_plan([len(w) for w in waves], rates, 16000)[0].tolist()
    a, sa = fe.batch(waves, rates=rates)
    b, sb = fe.batch(converted)
    assert sa.tolist() == sb.tolist() == [1 + n // 160 for n in lengths] and a.shape == b.shape and torch.equal(a, b)
    c, _ = fe.batch(waves[1:2])                                                       # (the rates do matter)
    assert c.shape != a[1:2].shape
    # ... with max_frames cutting the longest utterances
    a, sa = fe.batch(waves, max_frames=12, rates=rates)
    b, sb = fe.batch(converted, max_frames=12)
    assert sa.tolist() == sb.tolist() and max(sa.tolist()) == 12 and min(sa.tolist()) < 12 and torch.equal(a, b)
    # ... with tempo and gain behind the conversion
    tempo = np.array([0.9, 1.15, 1.0, 0.937, 1.102, 0.85])
    gain_db = np.array([3.0, -6.0, 0.0, 8.0, 1.5, -2.25], dtype=np.float32)
    a, sa = fe.batch(waves, augment=(tempo, gain_db), rates=rates)
    b, sb = fe.batch(converted, augment=(tempo, gain_db))
    stretched = [mtl_amd.TempoGainAugment.out_length(n, t) for n, t in zip(lengths, tempo)]
    assert sa.tolist() == sb.tolist() == [1 + n // 160 for n in stretched] and torch.equal(a, b)
    # ... and with a noise plan on top, made for the final lengths (every utterance noisy), all keywords at once
    inj = _noise_bank(tmp_path)
    rng = np.random.RandomState(1)
    draws = [inj.draw(rng, 1.0) for _ in waves]
    plan = inj.plan(draws, stretched)
    assert (plan[0] >= 0).all()
    a, sa = fe.batch(waves, max_frames=12, noise=(inj,) + plan, augment=(tempo, gain_db), rates=rates)
    b, sb = fe.batch(converted, max_frames=12, noise=(inj,) + plan, augment=(tempo, gain_db))
    c, _ = fe.batch(converted, max_frames=12, augment=(tempo, gain_db))
    assert sa.tolist() == sb.tolist() and torch.equal(a, b) and not torch.equal(a, c)
    plan = inj.plan(draws, lengths)
    a, sa = fe.batch(waves, noise=(inj,) + plan, rates=rates)
    b, sb = fe.batch(converted, noise=(inj,) + plan)
    assert sa.tolist() == sb.tolist() and torch.equal(a, b)
    # the n_fft // 2 + 1 minimum applies to the converted length: 400 samples at 48 kHz become 134, 100 at 8 kHz become 200
    with pytest.raises(ValueError, match='after the rate conversion'):
        fe.batch([ru.waveform(400, 1, 48000)], rates=[48000])
    assert fe.batch([ru.waveform(100, 1, 8000)], rates=[8000])[1].tolist() == [2]
    with pytest.raises(ValueError, match='beyond the 1024'):
        fe.batch(waves[:1], rates=[44101])


def test_rates_equal_to_the_target_are_bitwise_batch(fe):
    rng = np.random.RandomState(9)
    waves = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (1700, 163, 4000)]      # NOT on the int16 grid: copied, not rounded
    a, sa = fe.batch(waves, max_frames=20, rates=[16000] * 3)
    b, sb = fe.batch(waves, max_frames=20)
    assert sa.tolist() == sb.tolist() and torch.equal(a, b)
    assert all(np.array_equal(x, y) for x, y in zip(fe.resample(waves, [16000] * 3), waves))


# ------------------------------------------------------------------------------------------------------------------ datasets
def _corpus(tmp_path, n=8):
    """even utterances at 8 kHz, odd ones at 16 kHz, about 0.3 to 0.5 s each"""
    rows = []
    for i in range(n):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        rate = 8000 if i % 2 == 0 else 16000
        _write_wav(wp, ru.waveform((2400 + 350 * i) * rate // 8000, 40 + i, rate), rate)
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    return [str(p)]


def test_datasets_convert_mixed_rate_manifests(fe, tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path)
    args = argparse.Namespace(src_max_len=50, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming')

    def dataset(**kw):
        return mtl_amd.SpectrogramDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=manifests, normalize=True,
                                          is_train=True, seed=7, **kw)
    on, off, plain = dataset(device_batches=True, resample=True), dataset(device_batches=True, resample=False), dataset(device_batches=True)
    picks = np.random.RandomState(7).choice(np.arange(0, 8), 5, p=on.proba[0], replace=True)
    assert any(j % 2 == 0 for j in picks[:3]) and any(j % 2 == 1 for j in picks[:3])          # both rates in the training part
    loaded = [mtl_amd.load_wav_pcm16_rate(str(tmp_path / ('u%d.wav' % j))) for j in picks]
    pre = [y if r == 16000 else mtl_amd.resample([y], [r], 16000)[0] for y, r in loaded]
    assert [len(p) for p in pre] == [(2400 + 350 * int(j)) * 2 for j in picks]
    for part, sl in zip(on.sample(3, 2, 0), (slice(0, 3), slice(3, 5))):
        want, sizes = fe.batch(pre[sl], max_frames=50)
        assert part[0].is_cuda and torch.equal(part[0], want) and part[1].tolist() == sizes.tolist()
        assert torch.equal(part[2], part[1].float() / float(want.size(3)))
    # resample=False is today's output: the samples as they are in the files, whatever the headers say
    for a, b, sl in zip(off.sample(3, 2, 0), plain.sample(3, 2, 0), (slice(0, 3), slice(3, 5))):
        want, sizes = fe.batch([y for y, _ in loaded[sl]], max_frames=50)
        assert torch.equal(a[0], want) and torch.equal(b[0], want) and a[1].tolist() == b[1].tolist() == sizes.tolist()
    assert on.rng.rand() == off.rng.rand() == plain.rng.rand()
    # the per-utterance path: row 0 of a one-utterance batch of the file at its rate = of the converted file
    item = dataset(resample=True)
    for index in (0, 1):                                                              # u0 at 8 kHz, u1 at 16 kHz
        spect, transcript = item[index]
        y, r = mtl_amd.load_wav_pcm16_rate(str(tmp_path / ('u%d.wav' % index)))
        assert r == (8000, 16000)[index] and not spect.is_cuda and len(transcript) > 0
        if r == 16000:                                                                # at the target rate: the path it took before
            assert torch.equal(spect, fe(y).cpu()[:, :50])
            continue
        assert torch.equal(spect, fe.batch([y], rates=[r])[0][0, 0].cpu()[:, :50])
        assert torch.equal(spect, fe.batch(mtl_amd.resample([y], [r], 16000))[0][0, 0].cpu()[:, :50])
    assert item[0][0].shape == (161, 31) and dataset()[0][0].shape == (161, 16)     # 4800 converted samples against 2400 as they are
