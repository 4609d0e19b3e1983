"""CPU: host side of the log-mel filterbank front-end -- geometry, frame counts and the mel table against the restatement of
tests/fbank_util.py, the logfbank model shape, LogFBankDataset's index stream and rejections, and the argument checks of
mtl_fbank_batch (no device needed for any of it)."""
import argparse
import wave

import numpy as np
import pytest
import torch

from tests import fbank_util as fu
from tests import golden_util as gu


def test_mel_filterbank_at_16_khz_has_one_empty_band_and_equals_the_restatement():
    import mtl_amd
    fb = mtl_amd.mel_filterbank(80, 512, 16000)
    assert fb.dtype == np.float64 and fb.shape == (80, 257)
    assert fu.mel_bins(80, 512, 16000)[:6].tolist() == [0, 0, 1, 2, 2, 3]
    assert [j for j in range(80) if not fb[j].any()] == [2]                           # band 2 is empty and no other band is
    assert int((fb != 0).sum(axis=0).max()) == 2 and (fb >= 0).all() and fb.max() == 1.0       # a bin feeds at most two bands
    assert np.array_equal(fb, fu.mel_table(80, 512, 16000))
    # the sparse form holds the same weights, rounded once
    band, w = mtl_amd.mel_filterbank_sparse(fb)
    assert band.dtype == np.int32 and band.shape == (80, 3) and w.dtype == np.float32 and band[2].tolist() == [0, 0, 0]
    dense = np.zeros_like(fb)
    for j, (first, count, off) in enumerate(band):
        dense[j, first:first + count] = w[off:off + count]
        assert count == 0 or (w[off] != 0 and w[off + count - 1] != 0)
    assert np.array_equal(dense, fb.astype(np.float32).astype(np.float64)) and w.shape[0] == int(band[:, 1].sum())


def test_mel_filterbank_at_8_khz_has_no_empty_band():
    import mtl_amd
    fb = mtl_amd.mel_filterbank(80, 512, 8000)
    assert all(fb[j].any() for j in range(80)) and int((fb != 0).sum(axis=0).max()) <= 2
    assert np.array_equal(fb, fu.mel_table(80, 512, 8000))


def test_geometry_and_frame_counts():
    import mtl_amd
    assert mtl_amd.fbank_geometry(16000) == (400, 160, 512) == fu.geometry(16000)
    assert mtl_amd.fbank_geometry(8000) == (200, 80, 512) == fu.geometry(8000)
    assert mtl_amd.fbank_frames([1, 399, 400, 401, 560, 561], 16000).tolist() == [1, 1, 1, 2, 2, 3]
    assert mtl_amd.fbank_frames([1, 200, 201, 280, 281], 8000).tolist() == [1, 1, 2, 2, 3]
    for n in (1, 400, 401, 12345, 163440, 163441):
        assert int(mtl_amd.fbank_frames([n], 16000)[0]) == fu.frames(n, 16000)
    with pytest.raises(ValueError, match='nfft'):
        mtl_amd.fbank_geometry(22050)
    with pytest.raises(ValueError, match='nfft'):
        mtl_amd.fbank_frames([1000], 22050)
    with pytest.raises(ValueError, match='without samples'):
        mtl_amd.fbank_frames([400, 0], 16000)
    assert mtl_amd.fbank_geometry(20480)[0] == 512


def _args(cfg, **kw):
    base = dict(feat_extractor='vgg_cnn', sample_rate=16000, window_size=.02, feat='logfbank', dim_input=161, dropout=0.0,
                emb_trg_sharing=False, label_smoothing=0.0, name='t', lr=1e-2, meta_lr=1e-3, k_train=2, k_valid=2, clip=False,
                max_norm=400, save_every=1, save_folder='/tmp/mtl_ckpt_test', cuda=False, is_factorized=False, r=cfg.get('r', 100))
    base.update({k: v for k, v in cfg.items() if k not in ('vocab_size', 'r')})
    base.update(kw)
    return argparse.Namespace(**base)


def test_logfbank_model_has_the_2560_wide_input(tmp_path):
    """utils/functions.py:322-323: 80 bands pool to 20 rows of 128 channels"""
    import mtl_amd
    z, cfg, spec = gu.load('F0')
    args = _args(cfg, save_folder=str(tmp_path), name='fb')
    vocab = mtl_amd.synthetic_vocab(64)
    torch.manual_seed(123456)
    model = mtl_amd.init_transformer_model(args, vocab, r=cfg['r'])
    assert args.dim_input == 2560
    lin = model.encoder.input_linear
    assert lin.in_features == 2560 and lin.out_features == cfg['dim_model']
    spect = _args(cfg, feat='spectrogram')
    assert mtl_amd.init_transformer_model(spect, vocab, r=cfg['r']).encoder.input_linear.in_features == 5120 == spect.dim_input
    # a checkpoint whose args say logfbank goes round (no device: args.cuda is False)
    path = mtl_amd.save_meta_model(model, vocab, 3, torch.optim.SGD(model.parameters(), lr=args.lr),
                                   torch.optim.Adam(model.parameters(), lr=args.meta_lr), {'avg_valid_cer': 1.0}, args)
    m2, _, _, _, epoch, _, a2 = mtl_amd.load_meta_model(path)
    assert epoch == 3 and a2.feat == 'logfbank' and a2.dim_input == 2560 and m2.encoder.input_linear.in_features == 2560
    for (n1, p1), (n2, p2) in zip(model.named_parameters(), m2.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2)


def _corpus(tmp_path, n=12):
    rng = np.random.RandomState(3)
    rows = []
    for i in range(n):
        m = 2000 + 300 * i
        wp, tp = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        with wave.open(str(wp), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(rng.randint(-3000, 3000, size=m).astype('<i2').tobytes())
        tp.write_text(''.join(chr(0x4e00 + (5 * i + j) % 60) for j in range(2 + i % 4)), encoding='utf8')
        rows.append('%s,%s' % (wp, tp))
    manifests = []
    for m in range(2):
        p = tmp_path / ('train%d.csv' % m)
        p.write_text('\n'.join(rows[m::2]) + '\n')
        manifests.append(str(p))
    return manifests


ARGS = argparse.Namespace(src_max_len=20, sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', feat='logfbank')
CONF = dict(sample_rate=16000, window_size=.02, window_stride=.01, window='hamming', noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))


def test_dataset_has_the_reference_attributes_and_the_index_stream_of_the_spectrogram_dataset(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path)
    vocab = mtl_amd.synthetic_vocab(64)
    seen = {'fb': [], 'sp': []}

    def stub(key, F):
        return lambda path: (seen[key].append(path), torch.zeros(F, 1 + len(mtl_amd.load_wav_pcm16(path)) // 160))[1]
    fb = mtl_amd.LogFBankDataset(vocab, ARGS, CONF, manifest_filepath_list=manifests, normalize=True, is_train=True, seed=7,
                                 partitions=[0.5, 1.0], feature_fn=stub('fb', 80))
    sp = mtl_amd.SpectrogramDataset(vocab, ARGS, CONF, manifest_filepath_list=manifests, normalize=True, is_train=True, seed=7,
                                    partitions=[0.5, 1.0], feature_fn=stub('sp', 161))
    # utils/data_loader.py:114-129
    assert fb.max_size == len(fb) == 12 and len(fb.ids_list) == 2 and fb.input_type == 'char' and fb.manifest_filepath_list == manifests
    assert fb.normalize is True and fb.vocab is vocab and not fb.device_batches and fb.noiseInjector is None
    for manifest_id in (0, 1, 1, 0):
        a, b = fb.sample(3, 2, manifest_id), sp.sample(3, 2, manifest_id)
        assert seen['fb'] == seen['sp']                                               # the same utterances in the same order
        for pa, pb in zip(a, b):
            assert tuple(pa[0].shape[:3]) == (pa[0].shape[0], 1, 80) and pa[0].shape[3] == pb[0].shape[3] <= 20
            for x, y in zip(pa[1:], pb[1:]):
                assert torch.equal(x, y)
    assert fb.rng.rand() == sp.rng.rand()
    # __getitem__ interleaves the manifests (utils/data_loader.py:133-143)
    del seen['fb'][:]
    feat, transcript = fb[3]
    assert seen['fb'] == [fb.ids_list[1][1][0]] and feat.shape[0] == 80 and transcript == fb.parse_transcript(fb.ids_list[1][1][1])
    # constructing the batched form needs no device
    assert mtl_amd.LogFBankDataset(vocab, ARGS, CONF, manifest_filepath_list=manifests, device_batches=True, resample=True).device_batches


def test_dataset_rejects_what_the_spectrogram_dataset_rejects(tmp_path):
    import mtl_amd
    manifests = _corpus(tmp_path, n=4)
    vocab = mtl_amd.synthetic_vocab(64)
    fn = lambda path: torch.zeros(80, 3)

    def make(conf=CONF, **kw):
        return mtl_amd.LogFBankDataset(vocab, ARGS, conf, manifest_filepath_list=manifests, **kw)
    with pytest.raises(ValueError, match='feature_fn'):
        make(device_batches=True, feature_fn=fn)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        make(resample=True, feature_fn=fn)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        make(augment=True, feature_fn=fn)
    with pytest.raises(NotImplementedError, match='device_batches=True'):
        make(augment=True)
    with pytest.raises(NotImplementedError, match='feature_fn'):
        make(conf=dict(CONF, noise_dir=str(tmp_path)), feature_fn=fn)
    with pytest.raises(NotImplementedError, match='char'):
        make(input_type='bpe')
    with pytest.raises(ValueError, match='nfft'):
        make(conf=dict(CONF, sample_rate=44100))
    assert make(augment=True, device_batches=True)._augment is not None


def test_argument_validation_without_gpu():
    import __graft_entry__ as ge
    L = ge.build()._lib.lib()
    keep = np.zeros(64, dtype=np.float64)
    buf = keep.ctypes.data                                          # any non-null, 8-byte aligned address: nothing is dereferenced

    def run(K=1, fl=400, fs=160, nfft=512, nfilt=80, Tmax=4, ldb=516, n_w=425, ws_bytes=1 << 20, wav=buf, ws=buf):
        return L.mtl_fbank_batch(None, wav, buf, K, fl, fs, nfft, buf, ldb, nfilt, buf, buf, n_w, buf, Tmax, 1, ws, ws_bytes)
    for bad in (dict(K=0), dict(fl=0), dict(fl=513), dict(fs=0), dict(nfilt=0), dict(Tmax=0), dict(nfft=511), dict(nfft=1024, fl=600),
                dict(ldb=513), dict(n_w=0), dict(wav=None), dict(ws=None), dict(ws=buf + 4), dict(ws_bytes=8)):
        assert run(**bad) == -22, bad
    assert L.mtl_fbank_batch_workspace(0) == -22 and L.mtl_fbank_batch_workspace(3) == 3 * L.mtl_fbank_slots() * 16
    assert L.mtl_fbank_tile_frames() % 16 == 0 and L.mtl_fbank_slots() >= 1
