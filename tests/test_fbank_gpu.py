"""MI355X: the log-mel filterbank front-end on the device (mtl_fbank_batch, LogFBankFrontEnd, LogFBankDataset) against the fp64
restatement of tests/fbank_util.py -- the DEFINITION of the behaviour, parity with python_speech_features unpinned.

Tolerance: none is fixed in advance.  Every case also runs the fp32 restatement (the same formulas, the DFT as an fp32 matrix product);
its largest error against fp64 on the case is the case's floor, and the device must stay within FACTOR = 4 floors (log domain): it adds the same
fl fp32 products per bin in another order, and a factor of 4 covers the order and nothing else.  normalize=False is compared in the log
domain, normalize=True after normalisation.  An element whose fp64 energy is below 2^-20 of its frame's total band energy is
ill-conditioned (fbank_util.conditioning: in practice band 0, the DC bin that pre-emphasis nearly cancels): it is left out of the
maximum of both comparisons, at most 2 % of a case may be, and it is still held in energy relative to the frame total: to 4 log-domain
floors as stated, and to 4 times the fp32 restatement's own energy error on the case's left-out elements, which is the bound that can
fail.  The ln(eps) elements are never left out.  The normalised reference is the fp64 restatement normalised with its own values, all
elements in its statistics (fbank_util.norm_errors); NORM_FACTOR below says why that comparison gets 16 floors.  A case is one `batch`
call (its floor and its device error are the largest over its utterances); rows are tied to the one-utterance call bit for bit by a
test of their own.

One report line per case (collected in profiles/fbank/errors.txt).  Device results and restatements are computed once and shared."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import fbank_util as fu

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# The normalised comparison gets 16 floors, the most that may be given, for this reason.  An ill-conditioned element's logarithm is the
# logarithm of what fp32 cancellation leaves of a sum of fl products, so it is off by 0.01 to 40, by an amount that depends on the
# summation order alone.  It is out of the maximum, but it is in the implementation's mean and std (as it must be: the reference keeps
# every element), and there one such element moves every normalised value of an utterance of N elements by its log error / (N std).
# About 1 % of the elements are ill, their errors are of either sign and largely cancel in the mean, and what is left over is the whole
# of the normalised error of both the fp32 restatement (the floor) and the device: each is one draw of a sum of a few dozen such terms,
# not a rounding bound, and their ratio is the ratio of two such draws.  Restated on the host with nothing but the order of the fl
# products changed (natural order in steps of 4, and three random orders), nine utterances of the base signals gave ratios to the
# matrix-product restatement of 0.27 to 5.6 and once 15.7, while the log-domain ratio of the same runs stayed below 4.  A factor of 4
# would therefore fail honest orders; 16 is the cap.
NORM_FACTOR = 16.0
KINDS = ('noise', 'tone', 'fade', 'gap')
LN_EPS32 = np.float32(np.log(fu.EPS))
EDGE = ['edges-%s' % k for k in KINDS]
WRAP = ['wrap-%s' % k for k in KINDS]
SINGLE = ['single-%s' % k for k in KINDS]
CASES = EDGE + WRAP + SINGLE + ['mixed-longest-first', 'mixed-longest-last', 'rate-8k']


def _constants():
    """TILE_FRAMES: frames that a workgroup takes at a time; WALK_TILES: tiles of one utterance that exist before a workgroup takes a
    second one (the workgroups that share an utterance) -- read from the library, so that the edge lengths follow the kernel"""
    import mtl_amd
    L = mtl_amd._lib.lib()
    return L.mtl_fbank_tile_frames(), L.mtl_fbank_slots()


def _length(T, rate):
    """the longest utterance of exactly T >= 2 frames: fl + (T - 1) fs samples (one sample more starts frame T + 1)"""
    fl, fs, _ = fu.geometry(rate)
    return fl + (T - 1) * fs


@pytest.fixture(scope='module')
def cases():
    """name -> (rate, list of waveforms)"""
    TILE_FRAMES, WALK_TILES = _constants()
    assert TILE_FRAMES >= 2 and WALK_TILES >= 1
    tile = [_length(TILE_FRAMES + d, 16000) for d in (-1, 0, 1)]
    walk = [_length(TILE_FRAMES * WALK_TILES + d, 16000) for d in (-1, 0, 1)]
    out = {}
    for i, kind in enumerate(KINDS):
        lengths = [1, 150, 399, 400, 401, 560, 561] + tile
        out['edges-%s' % kind] = (16000, [fu.signal(kind if n >= 2400 or kind != 'gap' else 'noise', n, 10 * i + j) for j, n in enumerate(lengths)])
        out['single-%s' % kind] = (16000, [fu.signal(kind, 12345, 50 + i)])
        out['wrap-%s' % kind] = (16000, [fu.signal(kind, n, 70 + 10 * i + j) for j, n in enumerate(walk)])
    mixed = [(9000, 'gap'), (401, 'noise'), (1, 'noise'), (3000, 'tone'), (560, 'fade')]
    out['mixed-longest-first'] = (16000, [fu.signal(k, n, 90 + j) for j, (n, k) in enumerate(mixed)])
    out['mixed-longest-last'] = (16000, out['mixed-longest-first'][1][::-1])
    out['rate-8k'] = (8000, [fu.signal(k, n, 95 + j, 8000) for j, (n, k) in enumerate([(1, 'noise'), (200, 'tone'), (201, 'fade'), (6000, 'gap')])])
    assert sorted(out) == sorted(CASES)
    return out


@pytest.fixture(scope='module')
def reference(cases):
    """name -> per utterance (E fp64, log energies fp32 restatement, normalised fp32 restatement)"""
    return {name: [(fu.energies(x, rate), fu.restate32(x, rate), fu.restate32(x, rate, normalize=True)) for x in waves]
            for name, (rate, waves) in cases.items()}


@pytest.fixture(scope='module')
def fes():
    import mtl_amd
    assert torch.cuda.is_available()
    return {(rate, norm): mtl_amd.LogFBankFrontEnd(rate, 80, normalize=norm) for rate in (16000, 8000) for norm in (False, True)}


@pytest.fixture(scope='module')
def device(cases, fes):
    """(name, normalize) -> (inputs on the host, sizes)"""
    out = {}
    for name, (rate, waves) in cases.items():
        for norm in (False, True):
            x, sizes = fes[(rate, norm)].batch(waves)
            out[(name, norm)] = (x.cpu().numpy(), sizes.tolist())
    return out


@pytest.mark.parametrize('name', CASES)
def test_batch_against_the_fp64_restatement(cases, reference, device, name):
    rate, waves = cases[name]
    (raw, sizes), (nrm, nsizes) = device[(name, False)], device[(name, True)]
    frames = [fu.frames(len(x), rate) for x in waves]
    assert sizes == nsizes == frames and raw.shape == nrm.shape == (len(waves), 1, 80, max(frames)) and raw.dtype == np.float32
    floor_log = floor_ill = floor_norm = dev_log = dev_ill = dev_norm = 0.0
    ill_count = total = 0
    for k, (E, v32, n32) in enumerate(reference[name]):
        T = frames[k]
        assert E.shape == (80, T)
        assert not raw[k, 0, :, T:].any() and not nrm[k, 0, :, T:].any()              # the padding columns are exactly 0
        f_well, f_ill, _ = fu.log_errors(v32, E)
        d_well, d_ill, share = fu.log_errors(raw[k, 0, :, :T], E)
        floor_log, floor_ill, dev_log, dev_ill = max(floor_log, f_well), max(floor_ill, f_ill), max(dev_log, d_well), max(dev_ill, d_ill)
        ill_count, total = ill_count + int(round(share * E.size)), total + E.size
        if rate == 16000:                                                             # the empty band, bit for bit
            assert (raw[k, 0, 2, :T] == LN_EPS32).all() and (E[2] == 0).all()
        assert np.isfinite(nrm[k]).all()
        floor_norm = max(floor_norm, fu.norm_errors(n32, E))
        dev_norm = max(dev_norm, fu.norm_errors(nrm[k, 0, :, :T], E))
    print('fbank %s: K %d, frames %d..%d, left out %.2f %%; log floor %.2e device %.2e (%.2f floors); left-out energy floor %.2e device %.2e '
          '(%.2f floors); normalised floor %.2e device %.2e (%.2f floors)' % (name, len(waves), min(frames), max(frames), 100.0 * ill_count / total,
                                                                             floor_log, dev_log, dev_log / floor_log, floor_ill, dev_ill,
                                                                             dev_ill / floor_ill if floor_ill else 0.0, floor_norm, dev_norm,
                                                                             dev_norm / floor_norm))
    assert ill_count <= 0.02 * total
    assert dev_log <= FACTOR * floor_log
    assert dev_ill <= FACTOR * floor_log                                              # as stated; three decades of room, so ...
    assert dev_ill <= FACTOR * floor_ill                                              # ... against the restatement's own energy error too
    assert dev_norm <= NORM_FACTOR * floor_norm


def test_silent_frames_are_ln_eps_in_every_row(cases, device):
    """a frame that lies inside the 1200 zeros (from their second sample on: the first still carries -0.97 s[i-1]) is ln(eps) in all rows"""
    checked = 0
    for name in ('single-gap', 'wrap-gap', 'mixed-longest-first'):
        x = cases[name][1][0]
        L = len(x)
        z0, z1 = L // 2 - 600, L // 2 + 600
        assert not x[z0:z1].any() and x[z0 - 1] != 0
        raw = device[(name, False)][0][0, 0]
        silent = [t for t in range(fu.frames(L, 16000)) if t * 160 >= z0 + 1 and t * 160 + 400 <= z1]
        assert len(silent) >= 4
        assert (raw[:, silent] == LN_EPS32).all()
        assert not (raw[3:, [silent[0] - 1, silent[-1] + 1]] == LN_EPS32).any()
        checked += len(silent)
    assert checked >= 12


def test_a_second_call_is_bitwise_the_first_and_rows_do_not_depend_on_the_batch(cases, device, fes):
    for name in ('edges-noise', 'mixed-longest-first', 'mixed-longest-last', 'rate-8k'):
        rate, waves = cases[name]
        for norm in (False, True):
            fe = fes[(rate, norm)]
            first, sizes = device[(name, norm)]
            again, _ = fe.batch(waves)
            assert np.array_equal(again.cpu().numpy(), first)
            if name == 'edges-noise':
                continue
            for k, x in enumerate(waves):
                alone, s1 = fe.batch([x])
                assert s1.tolist() == [sizes[k]]
                assert np.array_equal(alone.cpu().numpy()[0, 0], first[k, 0, :, :sizes[k]])
                assert torch.equal(fe(x), alone[0, 0])
    a, b = device[('mixed-longest-first', True)][0], device[('mixed-longest-last', True)][0]
    assert np.array_equal(a, b[::-1])


def test_max_frames_cuts_the_output_and_not_the_statistics(cases, device, fes):
    rate, waves = cases['mixed-longest-first']
    full, sizes = device[('mixed-longest-first', True)]
    assert sizes == [55, 2, 1, 18, 2]
    for norm in (True, False):
        cut, csizes = fes[(rate, norm)].batch(waves, max_frames=10)
        cut = cut.cpu().numpy()
        assert csizes.tolist() == [10, 2, 1, 10, 2] and cut.shape == (5, 1, 80, 10)
        want = device[('mixed-longest-first', norm)][0][..., :10]                     # statistics over the WHOLE utterance: the same bits
        assert np.array_equal(cut, want)
        for k, n in enumerate(csizes.tolist()):
            assert not cut[k, 0, :, n:].any()


# ------------------------------------------------------------------------------------------------------------------ composition
def _write_wav(path, y, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.rint(np.asarray(y, dtype=np.float64) * 32768.0).astype('<i2').tobytes())


@pytest.fixture(scope='module')
def trio():
    """K = 3, 8 kHz and 16 kHz mixed: (waves, rates)"""
    rates = [8000, 16000, 8000]
    return [fu.signal(k, n, 120 + j, r) for j, (n, k, r) in enumerate(zip((2100, 5000, 1700), ('noise', 'tone', 'fade'), rates))], rates


def test_batch_with_rates_is_bitwise_batch_of_the_converted_waveforms(fes, trio):
    import mtl_amd
    fe = fes[(16000, True)]
    waves, rates = trio
    converted = mtl_amd.resample(waves, rates, 16000)
    assert [len(c) for c in converted] == [4200, 5000, 3400]
    a, sa = fe.batch(waves, rates=rates)
    b, sb = fe.batch(converted)
    assert sa.tolist() == sb.tolist() == [fu.frames(n, 16000) for n in (4200, 5000, 3400)] and torch.equal(a, b)
    c, sc = fe.batch(waves)
    assert sc.tolist() != sa.tolist()                                                 # (the rates do matter)
    a, sa = fe.batch(waves, max_frames=20, rates=rates)
    b, sb = fe.batch(converted, max_frames=20)
    assert sa.tolist() == sb.tolist() == [20, 20, 20] and torch.equal(a, b)


def test_batch_with_augment_is_bitwise_batch_of_the_stretched_waveforms(fes, trio):
    import mtl_amd
    fe = fes[(16000, True)]
    waves = mtl_amd.resample(*trio, 16000)
    tempo, gain_db = np.array([0.9, 1.0, 1.13]), np.array([3.0, -6.0, 1.5], dtype=np.float32)
    stretched = mtl_amd.tempo_gain(waves, tempo, gain_db, 16000)[0]
    a, sa = fe.batch(waves, augment=(tempo, gain_db))
    b, sb = fe.batch(stretched)
    assert sa.tolist() == sb.tolist() == [fu.frames(len(s), 16000) for s in stretched] and torch.equal(a, b)
    assert sa.tolist() != fe.batch(waves)[1].tolist()
    # ... and behind a rate conversion, all in one call
    a, sa = fe.batch(trio[0], augment=(tempo, gain_db), rates=trio[1])
    assert sa.tolist() == sb.tolist() and torch.equal(a, b)


def test_batch_with_noise_is_bitwise_batch_of_the_unfused_mix(fes, trio, tmp_path):
    import mtl_amd
    L = mtl_amd._lib.lib()
    fe = fes[(16000, True)]
    waves = mtl_amd.resample(*trio, 16000)
    d = tmp_path / 'noise'
    d.mkdir()
    for i, n in enumerate((30000, 40000)):
        _write_wav(d / ('n%d.wav' % i), fu.signal('noise', n, 130 + i), 16000)
    inj = mtl_amd.NoiseInjection(str(d), 16000, (0.1, 0.5))
    rng = np.random.RandomState(1)
    noise_off, level = inj.plan([inj.draw(rng, 1.0) for _ in waves], [len(w) for w in waves])
    assert (noise_off >= 0).all()
    noise_off[1] = -1                                                                 # one utterance stays clean
    # mtl_wave_mix_coef + mtl_wave_mix on the packed waveforms
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    wav, off = torch.from_numpy(np.concatenate(waves)).cuda(), torch.from_numpy(offsets).cuda()
    noff, lvl = torch.from_numpy(noise_off).cuda(), torch.from_numpy(level).cuda()
    bank, coef, out = inj.device_bank(), torch.empty(3, device='cuda'), torch.empty_like(wav)
    ws_bytes = L.mtl_wave_mix_coef_workspace(3)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert L.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), 3, bank.data_ptr(), inj.bank_len, noff.data_ptr(), lvl.data_ptr(),
                               coef.data_ptr(), ws.data_ptr(), ws_bytes) == 0
    assert L.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), 3, bank.data_ptr(), inj.bank_len, noff.data_ptr(), coef.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    mixed = [out.cpu().numpy()[offsets[k]:offsets[k + 1]] for k in range(3)]
    assert np.array_equal(mixed[1], waves[1]) and not np.array_equal(mixed[0], waves[0])
    a, sa = fe.batch(waves, noise=(inj, noise_off, level))
    b, sb = fe.batch(mixed)
    c, _ = fe.batch(waves)
    assert sa.tolist() == sb.tolist() and torch.equal(a, b) and not torch.equal(a, c) and torch.equal(a[1], c[1])


def test_abi_rejects_bad_arguments_before_any_launch(fes):
    import mtl_amd
    L = mtl_amd._lib.lib()
    fe = fes[(16000, True)]
    x = fu.signal('noise', 900, 3)
    wav, off = torch.from_numpy(x).cuda(), torch.tensor([0, 900], dtype=torch.int64, device='cuda')
    out = torch.full((80 * 5 + 64,), 7.0, device='cuda')
    need = L.mtl_fbank_batch_workspace(1)
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def run(K=1, fl=fe.fl, fs=fe.fs, nfft=fe.nfft, nfilt=80, Tmax=5, out_=out.data_ptr(), ws_bytes=need, band=fe.band.data_ptr()):
        return L.mtl_fbank_batch(st, wav.data_ptr(), off.data_ptr(), K, fl, fs, nfft, fe.basis.data_ptr(), fe.ldb, nfilt, band,
                                 fe.band_w.data_ptr(), fe.band_w.numel(), out_, Tmax, 1, ws.data_ptr(), ws_bytes)
    assert run(K=0) == -22 and run(fl=0) == -22 and run(fl=513) == -22 and run(fs=0) == -22 and run(nfilt=0) == -22 and run(Tmax=0) == -22
    assert run(out_=None) == -22 and run(band=None) == -22 and run(ws_bytes=need - 1) == -22 and run(nfft=1024) == -22
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                   # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[80 * 5:] == 7.0).all()                                                # nothing beyond the batch is written
    want = fe.batch([x], max_frames=5)[0].cpu().numpy()
    assert np.array_equal(got[:400].reshape(1, 1, 80, 5), want)


# ------------------------------------------------------------------------------------------------------------------ dataset
def test_dataset_device_batches_equal_the_per_utterance_path(tmp_path):
    import mtl_amd
    rows = []
    for i in range(6):
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        _write_wav(wp, fu.signal(KINDS[i % 3], 3000 + 700 * i, 140 + i), 16000)
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 50) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    p = tmp_path / 'train.csv'
    p.write_text('\n'.join(rows) + '\n')
    args = argparse.Namespace(src_max_len=30, sample_rate=16000, window_size=.02, window_stride=.01, feat='logfbank')
    audio_conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.4)

    def dataset(**kw):
        return mtl_amd.LogFBankDataset(mtl_amd.synthetic_vocab(64), args, audio_conf, manifest_filepath_list=[str(p)], normalize=True,
                                       is_train=True, seed=7, **kw)
    batched, plain = dataset(device_batches=True), dataset()
    for a, b in zip(batched.sample(2, 2, 0), plain.sample(2, 2, 0)):
        assert a[0].is_cuda and not b[0].is_cuda and a[0].shape == b[0].shape and a[0].shape[:3] == (2, 1, 80)
        assert a[0].shape[3] == int(a[1].max()) <= 30
        assert torch.equal(a[0], b[0].cuda())
        for x, y in zip(a[1:], b[1:]):                                                # sizes, percentages, targets, target sizes
            assert x.dtype == y.dtype and torch.equal(x, y)
    assert batched.rng.rand() == plain.rng.rand()
    feat, transcript = plain[0]
    assert feat.shape == (80, fu.frames(3000, 16000)) and len(transcript) > 0
    # against the definition, at the bar of the cases above
    x = mtl_amd.load_wav_pcm16(str(tmp_path / 'u0.wav'))
    E = fu.energies(x)
    assert fu.norm_errors(feat.numpy(), E) <= NORM_FACTOR * fu.norm_errors(fu.restate32(x, normalize=True), E)
