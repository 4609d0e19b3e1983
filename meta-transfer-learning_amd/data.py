"""Vocabulary, label/manifest loaders and the synthetic task source.

Mirrors: `Vocab` (utils/data.py:1-28), the label-JSON loading of meta_transfer_train.py:151-157, the manifest CSV
contract of utils/data_loader.py:191-195 and the batch layout returned by `SpectrogramDataset.sample`
(utils/data_loader.py:245-321).  Audio decoding / STFT (utils/data_loader.py:65-96) is outside the accelerated path
(SURVEY.md 8(f) f1): datasets here get features from a caller-supplied `feature_fn` or synthesize them.
"""
import csv
import json
import logging
import os
import unicodedata

import numpy as np
import torch


class Vocab(object):
    def __init__(self):
        self.PAD_TOKEN, self.SOS_TOKEN, self.EOS_TOKEN, self.OOV_TOKEN = '<PAD>', '<SOS>', '<EOS>', '<OOV>'
        self.PAD_ID, self.SOS_ID, self.EOS_ID, self.OOV_ID = 0, 1, 2, 3
        self.special_token_list = [self.PAD_TOKEN, self.SOS_TOKEN, self.EOS_TOKEN, self.OOV_TOKEN]
        self.token2id, self.id2token = {}, []
        self.label2id, self.id2label = {}, []
        for tok in self.special_token_list:
            self.add_token(tok)
            self.add_label(tok)

    def add_token(self, token):
        if token not in self.token2id:
            self.token2id[token] = len(self.token2id)
            self.id2token.append(token)

    def add_label(self, label):
        if label not in self.label2id:
            self.label2id[label] = len(self.label2id)
            self.id2label.append(label)


def load_vocab(labels_path):
    """labels JSON (a list of characters, e.g. data/labels/hkust_seame_labels.json) -> Vocab; specials first."""
    with open(labels_path, encoding='utf-8') as f:
        labels = json.load(f)
    vocab = Vocab()
    for label in labels:
        vocab.add_token(label)
        vocab.add_label(label)
    return vocab


def synthetic_vocab(size):
    """`size` ids in total (4 specials + size-4 distinct CJK code points), matching the reference's 3765 when size=3765."""
    vocab = Vocab()
    for i in range(size - 4):
        ch = chr(0x4e00 + i)
        vocab.add_token(ch)
        vocab.add_label(ch)
    return vocab


def is_chinese_char(cc):
    """utils/data.py:60-68: a character of Unicode category 'Lo' (other letter) counts as Chinese"""
    return unicodedata.category(cc) == 'Lo'


def is_contain_chinese_word(seq):
    """utils/data.py:70-81"""
    return any(is_chinese_char(c) for c in seq)


def get_word_segments_per_language(seq):
    """utils/data.py:84-127: split `seq` on single spaces and group consecutive words by language (a word holding any Chinese
    character is Chinese) -> list of segments, each the space-joined words of one run ('' words from double spaces included)"""
    cur_lang = -1                       # 0 English, 1 Chinese
    temp_words = ''
    word_segments = []
    for word in seq.split(' '):
        lang = 1 if is_contain_chinese_word(word) else 0
        if cur_lang == -1:
            temp_words = word
        elif cur_lang != lang:
            word_segments.append(temp_words)
            temp_words = word
        else:
            if temp_words != '':
                temp_words += ' '
            temp_words += word
        cur_lang = lang
    word_segments.append(temp_words)
    return word_segments


def read_manifest(path):
    """CSV without header, rows `wav_path,txt_path` (data/manifests/*.csv) -> list of [wav, txt]."""
    with open(path, newline='', encoding='utf-8') as f:
        return [row[:2] for row in csv.reader(f) if row]


def parse_transcript(vocab, transcript_path):
    """utils/data_loader.py:342-361 (char input): ' ' + lower-cased text -> ids of known labels (unknown chars and id 0 dropped)."""
    if transcript_path[-4:] == '.txt':
        with open(transcript_path, 'r', encoding='utf8') as f:
            text = ' ' + f.read().replace('\n', '').lower()
    else:
        text = transcript_path.replace('\n', '').lower()
    return [i for i in (vocab.label2id.get(ch) for ch in text) if i]


def collate(spects, transcripts, pad_id=0):
    """Zero-pad features to the batch max T and PAD-pad targets: the 5-tuple of utils/data_loader.py:284-297."""
    k = len(spects)
    max_t = max(s.size(1) for s in spects)
    freq = spects[0].size(0)
    max_l = max(len(t) for t in transcripts)
    inputs = torch.zeros(k, 1, freq, max_t)
    input_sizes = torch.zeros(k, dtype=torch.int32)
    input_percentages = torch.zeros(k, dtype=torch.float32)
    targets = torch.full((k, max_l), pad_id, dtype=torch.int64)
    target_sizes = torch.zeros(k, dtype=torch.int32)
    for i, (s, t) in enumerate(zip(spects, transcripts)):
        n = s.size(1)
        inputs[i, 0, :, :n] = s
        input_sizes[i] = n
        input_percentages[i] = n / float(max_t)
        targets[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
        target_sizes[i] = len(t)
    return inputs, input_sizes, input_percentages, targets, target_sizes


class ManifestTaskDataset:
    """`.sample(k_train, k_valid, manifest_id)` over manifest CSVs like SpectrogramDataset (utils/data_loader.py:171-321).

    feature_fn(wav_path) -> (F, T) float tensor replaces `parse_audio`; sampling uses np.random.choice with the same
    per-manifest probabilities (uniform, or uniform over the leading `partitions[i]` fraction).
    seed=None draws from the global np.random like the reference (seeded once by the entry script,
    meta_transfer_train.py:109-112); seed=<int> gives the dataset its own RandomState -- with several ranks every rank must
    see the same draws (tasks are sharded AFTER sampling, the validation batch is shared), so pass the same seed on all ranks.
    `__getitem__` / `__len__` follow utils/data_loader.py:323-340 (validation / test use: manifest 0 only unless is_train)."""

    def __init__(self, vocab, args, manifest_filepath_list, feature_fn=None, partitions=None, seed=None, is_train=False,
                 device_batches=False, noise=None, augment=None, resample=False):
        """device_batches=True: `sample()` featurises each part (train / validation) with ONE `SpectrogramFrontEnd.batch` call and
        returns `inputs` on the device (the trainers copy device-resident inputs straight into their static buffers); the sizes,
        percentages and targets stay host tensors as `collate` makes them, and the index stream is the same.  The front-end is
        built at the first `sample()`, so constructing the dataset needs no device.  `__getitem__` keeps the per-utterance path.

        noise=(NoiseInjection, noise_prob): every utterance is featurised as SpectrogramParser.parse_audio does with a noise
        injector (utils/data_loader.py:71-75).  The draws come from `self.rng`: `sample()` takes them per utterance in pick order
        (train part, then validation part) right after the `choice` of the indices, for parts that `need` leaves out as well (the
        number of draws does not depend on the audio, so all ranks keep one stream); `__getitem__` draws before it featurises.
        noise_prob may be a string (the reference's --noise-prob has no type): float() is taken.  Not with a feature_fn, which
        gets paths, not samples.

        augment=TempoGainAugment(...): every utterance is loaded as load_randomly_augmented_audio does (utils/audio.py:50-61: a random
        tempo, then a random gain, then the 16-bit file) before anything else happens to it, on the device, in the batched path only
        (device_batches=True; not with a feature_fn).  Per utterance the stream yields tempo, gain and THEN that utterance's noise
        draws, as parse_audio interleaves them (utils/data_loader.py:67-75); the noise segment is as long as the STRETCHED utterance.
        A part that `need` leaves out consumes these draws too.  augment=None leaves the stream exactly as it is without.

        resample=True: the sample rate in every wav header is read (`load_wav_pcm16_rate`) and an utterance at another rate than
        args.sample_rate is converted on the device before anything else happens to it (`SpectrogramFrontEnd.batch(rates=)`, `resample`
        for the definition): corpora at 8 kHz and at 16 kHz train together without an offline pass.  The batched path hands the rates
        of a part to its one `batch` call; the per-utterance path (`__getitem__`, the rows of `sample()` without device_batches) sends
        an utterance whose rate differs through `batch([y], rates=[rate])`.  The augmentation and noise plans are made for the
        CONVERTED lengths; no draw is added, so the stream is the same with and without.  Not with a feature_fn (which gets paths).
        resample=False (the default) never reads the header rate: every call and every output bit is as without the keyword."""
        if device_batches and feature_fn is not None:
            raise ValueError('device_batches=True featurises with the batched device front-end: it cannot be combined with a feature_fn')
        if noise is not None and feature_fn is not None:
            raise NotImplementedError('noise injection mixes samples on the device: it cannot be combined with a feature_fn (which gets paths)')
        if augment is not None and feature_fn is not None:
            raise NotImplementedError('tempo / gain augmentation runs on the device: it cannot be combined with a feature_fn (which gets paths)')
        if augment is not None and not device_batches:
            raise NotImplementedError('tempo / gain augmentation exists in the batched device path only: pass device_batches=True')
        if resample and feature_fn is not None:
            raise NotImplementedError('sample rates are converted on the device: resample=True cannot be combined with a feature_fn (which gets paths)')
        self._resample, self._rate = bool(resample), getattr(args, 'sample_rate', None)     # (a feature_fn needs no rate)
        self._noise = None if noise is None else (noise[0], float(noise[1]))
        self._augment = augment
        self.device_batches, self._fe = device_batches, None
        self._fe_factory = lambda: SpectrogramFrontEnd(args.sample_rate, args.window_size, args.window_stride,
                                                       getattr(args, 'window', 'hamming'), True)
        if device_batches:
            feature_fn = lambda path: self._front_end()(load_wav_pcm16(path)).cpu()
        elif feature_fn is None:
            # default: 16-bit PCM wav -> device spectrogram front-end (SpectrogramParser.parse_audio, normalize=True as in
            # meta_transfer_train.py:161), handed back on the host like the reference's parse_audio output
            fe = SpectrogramFrontEnd(args.sample_rate, args.window_size, args.window_stride, getattr(args, 'window', 'hamming'), True)
            feature_fn = lambda path: fe(load_wav_pcm16(path)).cpu()
            self._fe = fe
        self.vocab, self.args, self.feature_fn = vocab, args, feature_fn
        self.ids_list = [read_manifest(p) for p in manifest_filepath_list]
        self.rng = np.random if seed is None else np.random.RandomState(seed)
        self.is_train = is_train
        self.max_size = max(len(ids) for ids in self.ids_list) * len(self.ids_list)
        if is_train and len(self.ids_list) > 1:
            self.max_size = 30000                                   # utils/data_loader.py:198-203
        self.proba = []
        for i, ids in enumerate(self.ids_list):
            if partitions is not None:
                part = max(int(len(ids) * partitions[i]), 1)
                p = np.zeros(len(ids))
                p[:part] = 1 / part
            else:
                p = np.full(len(ids), 1 / len(ids))
            self.proba.append(p)

    def _rows(self, ids, picks, draws=None):
        spects, trans = [], []
        for i, j in enumerate(picks):
            wav, txt = ids[j][0], ids[j][1]
            spects.append(self._feature(wav, None if draws is None else draws[i])[:, :self.args.src_max_len])
            trans.append(parse_transcript(self.vocab, txt))
        return spects, trans

    def _feature(self, path, draw):
        """per-utterance path: feature_fn(path), or for an utterance whose draw = (augmentation, noise) asks for either
        `batch([y], augment=..., noise=...)[0][0, 0]`, handed back on the host like every feature; an utterance that `place` leaves clean
        (longer than its noise file) and is not augmented takes the clean path"""
        rate = None
        if self._resample:                                       # (a file at the front-end's own rate takes the paths below as it is)
            y, rate = load_wav_pcm16_rate(path)
            rate = None if rate == self._rate else rate
        if draw is None:
            draw = (None, None)
        if rate is None and draw[0] is None and draw[1] is None:
            return self.feature_fn(path)
        if not self._resample:
            y = load_wav_pcm16(path)
        kw, n = {}, y.shape[0]
        if rate is not None:
            kw['rates'], n = [rate], int(resample_plan([n], [rate], self._rate)[0][0])
        if draw[0] is not None:
            tempo, gain_db, out_lengths = self._augment.plan([draw[0]], [n])
            kw['augment'], n = (tempo, gain_db), int(out_lengths[0])
        placed = None if draw[1] is None else self._noise[0].place(draw[1], n)
        if placed is not None:
            kw['noise'] = (self._noise[0], np.array([placed[0]], dtype=np.int64), np.array([placed[1]], dtype=np.float32))
        if not kw:
            return self.feature_fn(path)
        return self._front_end().batch([y], **kw)[0][0, 0].cpu()

    def _draws(self, n):
        """the draws of n utterances, in order, from the dataset's stream: per utterance (augmentation draw | None, noise draw | None),
        tempo and gain before that utterance's noise draws (None without an augmentation and an injector)"""
        if self._noise is None and self._augment is None:
            return None
        out = []
        for _ in range(n):
            aug = None if self._augment is None else self._augment.draw(self.rng)
            out.append((aug, None if self._noise is None else self._noise[0].draw(self.rng, self._noise[1])))
        return out

    def _front_end(self):
        if self._fe is None:
            self._fe = self._fe_factory()
        return self._fe

    def _device_part(self, ids, picks, draws=None):
        """one part of a sampled batch through SpectrogramFrontEnd.batch: the 5-tuple of `collate` with `inputs` on the device
        (draws: one augmentation `plan` and one noise `plan` -- on the stretched lengths -- for the part; the noisy form of the call
        unless every utterance stays clean)"""
        if self._resample:
            waves, rates = zip(*[load_wav_pcm16_rate(ids[j][0]) for j in picks])
            waves = list(waves)
        else:
            waves = [load_wav_pcm16(ids[j][0]) for j in picks]
        trans = [parse_transcript(self.vocab, ids[j][1]) for j in picks]
        kw, lengths = {}, [w.shape[0] for w in waves]
        if self._resample:                                       # the plans below are made for the converted lengths
            kw['rates'], lengths = list(rates), resample_plan(lengths, rates, self._rate)[0]
        if draws is not None and self._augment is not None:
            tempo, gain_db, lengths = self._augment.plan([d[0] for d in draws], lengths)
            kw['augment'] = (tempo, gain_db)
        if draws is not None and self._noise is not None:
            noise_off, level = self._noise[0].plan([d[1] for d in draws], lengths)
            if (noise_off >= 0).any():
                kw['noise'] = (self._noise[0], noise_off, level)
        inputs, input_sizes = self._front_end().batch(waves, max_frames=self.args.src_max_len, **kw)
        k, max_t = len(trans), inputs.size(3)
        input_percentages = torch.zeros(k, dtype=torch.float32)
        targets = torch.full((k, max(len(t) for t in trans)), self.vocab.PAD_ID, dtype=torch.int64)
        target_sizes = torch.zeros(k, dtype=torch.int32)
        for i, t in enumerate(trans):
            input_percentages[i] = int(input_sizes[i]) / float(max_t)
            targets[i, :len(t)] = torch.tensor(t, dtype=torch.int64)
            target_sizes[i] = len(t)
        return inputs, input_sizes, input_percentages, targets, target_sizes

    def sample(self, k_train, k_val, manifest_id, need=(True, True)):
        """utils/data_loader.py:245-321.  need = (train part, validation part): a part that the caller will not use is still DRAWN
        (the index stream stays what the reference's is, and identical on every rank) but not loaded / featurised / collated --
        it is returned as None.  The meta loop uses only the LAST task's validation batch (transient_trainer.py:168) and, with
        several ranks, only its own tasks' training batches."""
        ids = self.ids_list[manifest_id]
        picks = self.rng.choice(np.arange(0, len(ids)), k_train + k_val, p=self.proba[manifest_id], replace=True)
        draws = self._draws(k_train + k_val)                         # (a part that is not needed has consumed its draws here)
        dtr, dva = (None, None) if draws is None else (draws[:k_train], draws[k_train:k_train + k_val])
        if self.device_batches:
            tr = self._device_part(ids, picks[:k_train], dtr) if need[0] else None
            va = self._device_part(ids, picks[k_train:k_train + k_val], dva) if need[1] else None
            return tr, va
        tr = collate(*self._rows(ids, picks[:k_train], dtr), pad_id=self.vocab.PAD_ID) if need[0] else None
        va = collate(*self._rows(ids, picks[k_train:k_train + k_val], dva), pad_id=self.vocab.PAD_ID) if need[1] else None
        return tr, va

    def __len__(self):
        return self.max_size

    def __getitem__(self, index):
        if self.is_train:
            ids = self.ids_list[index % len(self.ids_list)]
            row = ids[(index // len(self.ids_list)) % len(ids)]
        else:
            ids = self.ids_list[0]
            row = ids[index % len(ids)]
        draws = self._draws(1)
        return self._feature(row[0], None if draws is None else draws[0])[:, :self.args.src_max_len], parse_transcript(self.vocab, row[1])


def _wav_dataset_options(ds, audio_conf, feature_fn, augment, device_batches, resample, input_type, char_lines):
    """the rejections that SpectrogramDataset and LogFBankDataset share, in front of their base constructor, and the noise injector:
    sets ds.noiseInjector and returns the `noise=` of ManifestTaskDataset, (injector, noise_prob) or None"""
    if resample and feature_fn is not None:
        raise NotImplementedError('sample rates are converted on the device: resample=True cannot be combined with a feature_fn (which '
                                  'gets paths)')
    if device_batches and feature_fn is not None:
        raise ValueError('device_batches=True featurises with the batched device front-end: it cannot be combined with a feature_fn')
    if augment and feature_fn is not None:
        raise NotImplementedError('augment=True (tempo / gain perturbation, utils/data_loader.py:28-38) runs on the device: it cannot '
                                  'be combined with a feature_fn (which gets paths)')
    if augment and not device_batches:
        raise NotImplementedError('augment=True (tempo / gain perturbation, utils/data_loader.py:28-38) exists in the batched device '
                                  'path only: pass device_batches=True')
    noise = None
    if audio_conf.get('noise_dir') is not None:
        if feature_fn is not None:
            raise NotImplementedError("noise injection (audio_conf['noise_dir']) mixes samples on the device: it cannot be combined "
                                      "with a feature_fn (which gets paths)")
        ds.noiseInjector = NoiseInjection(audio_conf['noise_dir'], audio_conf['sample_rate'], audio_conf.get('noise_levels', (0, 0.5)))
        noise = (ds.noiseInjector, float(audio_conf.get('noise_prob')))
    else:
        ds.noiseInjector = None
    if input_type != 'char':
        raise NotImplementedError("only input_type='char' (utils/data_loader.py:%s)" % char_lines)
    return noise


def _wav_dataset_wiring(ds, noise, augment, resample, device_batches, front_end, manifest_filepath_list, input_type):
    """... and what both set behind it (after the base constructor: the default feature_fn is no user's)"""
    ds._noise = noise
    ds._augment = TempoGainAugment() if augment else None
    ds._resample, ds._rate = bool(resample), ds.sample_rate
    ds.device_batches, ds._fe_factory = device_batches, front_end       # (sample() of a part: one front_end().batch call)
    ds.manifest_filepath_list, ds.input_type = manifest_filepath_list, input_type


class SpectrogramDataset(ManifestTaskDataset):
    """utils/data_loader.py:171-236 with the reference's OWN constructor, so that its entry script builds the datasets unchanged
    (meta_transfer_train.py:159-175):

        SpectrogramDataset(vocab, args, audio_conf, manifest_filepath_list=..., normalize=True, augment=args.augment,
                           input_type=args.input_type, is_train=True, partitions=args.train_partition_list)

    audio_conf: dict(sample_rate, window_size, window_stride, window, noise_dir, noise_prob, noise_levels) (:141-147).  Features come
    from the device front-end (SpectrogramFrontEnd = SpectrogramParser.parse_audio, :65-96) unless `feature_fn` is given.  Same
    attributes as the reference object (max_size, ids_list, proba, part_len, input_type, manifest_filepath_list, is_train) and the
    same two console lines.  audio_conf['noise_dir'] builds a NoiseInjection over that directory (noise_levels, noise_prob as in
    :60-63; its device part is lazy, so construction needs no device) and every parse_audio -- `sample()`, `__getitem__` of validation
    and test loaders included, like the reference -- mixes noise on the device with probability noise_prob: see ManifestTaskDataset
    (noise=) for the draw stream and NoiseInjection for the semantics.  noise_dir with a feature_fn raises NotImplementedError (a
    feature function gets paths, not samples).  augment=True (load_randomly_augmented_audio in parse_audio, utils/data_loader.py:67-70)
    builds a TempoGainAugment with the reference's ranges: tempo and gain are applied on the device in the batched path, so it needs
    device_batches=True -- without it, and with a feature_fn, augment=True raises NotImplementedError.  See ManifestTaskDataset (augment=)
    for the draw stream and TempoGainAugment for the semantics (a restatement of ours: sox is not reproduced sample for sample).
    Outside the accelerated path and rejected loudly: input_type other than 'char' (the bpe / ipa branches are commented out in the
    reference too).
    device_batches=True: see ManifestTaskDataset (not part of the reference's constructor; default off).
    resample=True: files at another rate than audio_conf['sample_rate'] are converted on the device, see ManifestTaskDataset (not part of the
    reference's constructor either, which leaves this to sox; default off, and then the header rate is never read)."""

    def __init__(self, vocab, args, audio_conf, manifest_filepath_list, normalize=False, augment=False, input_type='char',
                 is_train=False, partitions=None, feature_fn=None, seed=None, device_batches=False, resample=False):
        noise = _wav_dataset_options(self, audio_conf, feature_fn, augment, device_batches, resample, input_type, '342-361')
        self.window_stride, self.window_size = audio_conf['window_stride'], audio_conf['window_size']
        self.sample_rate, self.window = audio_conf['sample_rate'], audio_conf.get('window', 'hamming')
        self.normalize, self.augment, self.noise_prob = normalize, augment, audio_conf.get('noise_prob')
        fe = []           # built at the first utterance: constructing the dataset must not need the device

        def front_end():
            if not fe:
                fe.append(SpectrogramFrontEnd(self.sample_rate, self.window_size, self.window_stride,
                                              self.window if self.window in ('hamming', 'hann', 'blackman', 'bartlett') else 'hamming',
                                              self.normalize))
            return fe[0]
        if feature_fn is None:
            def feature_fn(path):
                return front_end()(load_wav_pcm16(path)).cpu()
        super().__init__(vocab, args, manifest_filepath_list, feature_fn=feature_fn, partitions=partitions, seed=seed, is_train=is_train)
        _wav_dataset_wiring(self, noise, augment, resample, device_batches, front_end, manifest_filepath_list, input_type)
        # (the reference leaves part_len at the LAST manifest's partition size, or max_size without partitions: :211-222)
        self.part_len = (max(int(len(self.ids_list[-1]) * partitions[len(self.ids_list) - 1]), 1) if partitions is not None
                         else self.max_size)
        print('max_size:', self.max_size)
        print('input_type:', input_type)

    def parse_transcript(self, transcript_path):
        return parse_transcript(self.vocab, transcript_path)

    def parse_audio(self, audio_path):
        """utils/data_loader.py:65-96: with augmentation and / or a noise injector, this utterance's draws from the dataset's stream and
        the work on the device"""
        draws = self._draws(1)
        return self._feature(audio_path, None if draws is None else draws[0])


class BucketingSampler(torch.utils.data.Sampler):
    """utils/data_loader.py:480-500: consecutive bins of `batch_size` indices (the data is assumed sorted by length); iterating
    shuffles INSIDE each bin, shuffle(epoch) shuffles the ORDER of the bins -- both with the global np.random like the reference."""

    def __init__(self, data_source, batch_size=1):
        self.data_source = data_source
        ids = list(range(0, len(data_source)))
        self.bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch):
        np.random.shuffle(self.bins)


class AudioDataLoader(torch.utils.data.DataLoader):
    """utils/data_loader.py:401-440: a DataLoader over (spectrogram (F,T), transcript ids) items whose batches are sorted by
    descending frame count, zero-padded to the longest utterance / PAD-padded to the longest transcript, and returned as
    (inputs (B,1,F,T), targets (B,L) int64, input_percentages (B) f32, input_sizes (B) i32, target_sizes (B) i32) -- the layout
    the in-loop validation of TransientTrainer / JointTrainer consumes."""

    def __init__(self, pad_token_id, *args, **kwargs):
        self.pad_token_id = pad_token_id
        kwargs['collate_fn'] = self._collate
        super().__init__(*args, **kwargs)

    def _collate(self, batch):
        batch = sorted(batch, key=lambda sample: sample[0].size(1), reverse=True)
        inputs, input_sizes, input_percentages, targets, target_sizes = collate(
            [s for s, _ in batch], [t for _, t in batch], pad_id=self.pad_token_id)
        return inputs, targets, input_percentages, input_sizes, target_sizes


def synth_batch(seed, k, T, L, vocab_size, variable=False, freq_bins=161):
    """Seeded synthetic batch: N(0,1) 'spectrogram', labels in [4, V); optional ragged lengths."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(k, 1, freq_bins, T, generator=g)
    y = torch.randint(4, vocab_size, (k, L), generator=g)
    lens = torch.full((k,), T, dtype=torch.int32)
    if variable:
        lens = torch.randint(max(T // 8, 1), T + 1, (k,), generator=g).to(torch.int32)
        lens[0] = T
        if k > 1:
            lens[-1] = max(T // 8, 1)
        tl = torch.randint(max(L // 2, 1), L + 1, (k,), generator=g)
        tl[0] = L
        for i in range(k):
            x[i, :, :, int(lens[i]):] = 0
            y[i, int(tl[i]):] = 0
    return x, lens, y


class SyntheticTask:
    """Duck-types the dataset contract of `TransientTrainer.train`: seeded synthetic (train, valid) batches per call."""

    def __init__(self, task_id, k, T, L, vocab_size, variable=False, pin=False):
        self.task_id, self.k, self.T, self.L, self.V, self.variable, self.pin = task_id, k, T, L, vocab_size, variable, pin
        self.calls = 0

    def sample(self, k_train, k_valid, manifest_id):
        it = self.calls
        self.calls += 1
        out = []
        for part, k in ((0, k_train), (1, k_valid)):
            x, lens, y = synth_batch(1000 * it + 10 * self.task_id + part, k, self.T, self.L, self.V, self.variable)
            if self.pin:
                x = x.pin_memory()
            out.append((x, lens, lens.float() / self.T, y, (y != 0).sum(1).to(torch.int32)))
        return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# Spectrogram front-end on the device: SpectrogramParser.parse_audio, utils/data_loader.py:65-96
# ------------------------------------------------------------------------------------------------------------------
def load_wav_pcm16(path):
    """16-bit PCM .wav -> float32 mono in [-1, 1) (utils/audio.py:7-15 uses torchaudio.load(normalization=True); channels averaged)."""
    import wave
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2:
            raise ValueError('only 16-bit PCM wav files are supported here')
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float32) / 32768.0
        ch = w.getnchannels()
    return raw.reshape(-1, ch).mean(axis=1).astype(np.float32) if ch > 1 else raw


def load_wav_pcm16_rate(path):
    """(load_wav_pcm16(path), the sample rate in the file's header): what a front-end that converts rates needs (`resample`)"""
    import wave
    with wave.open(path, 'rb') as w:
        rate = w.getframerate()
    return load_wav_pcm16(path), int(rate)


def pack_waveforms(waves, hop, n_fft, max_frames=None):
    """K one-dimensional waveforms -> (flat float32 (sum of L_k), offsets int64 (K + 1), frames int32 (K), Tmax): the host side of
    `SpectrogramFrontEnd.batch`, pure numpy.  frames[k] = min(1 + L_k // hop, max_frames), Tmax = max(frames).  An utterance shorter
    than n_fft // 2 + 1 samples would need more than one reflection at its ends (numpy reflects repeatedly there): rejected."""
    if len(waves) == 0:
        raise ValueError('pack_waveforms: an empty list of waveforms')
    arrs = []
    for i, w in enumerate(waves):
        a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError('pack_waveforms: waveform %d is not one-dimensional (shape %s)' % (i, a.shape))
        if a.shape[0] < n_fft // 2 + 1:
            raise ValueError('pack_waveforms: utterance %d has %d samples, fewer than n_fft // 2 + 1 = %d (one reflection must suffice)'
                             % (i, a.shape[0], n_fft // 2 + 1))
        arrs.append(a)
    lengths = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    frames = 1 + lengths // hop
    if max_frames is not None:
        frames = np.minimum(frames, max_frames)
    frames = frames.astype(np.int32)
    return np.concatenate(arrs), offsets, frames, int(frames.max())


def wsola_geometry(sample_rate):
    """(segment S, search R, overlap O) in samples of the tempo change at `sample_rate`: 82 ms, 14.68 ms and 12 ms, the defaults that the
    documentation of sox's `tempo` effect gives, rounded as S = floor(sr 0.082 + 0.5), R = floor(sr 0.01468 + 0.5),
    O = max(floor(sr 0.012 + 4.5), 16) rounded down to a multiple of 8: (1312, 235, 192) at 16 kHz, (656, 117, 96) at 8 kHz."""
    S = int(np.floor(sample_rate * 0.082 + 0.5))
    R = int(np.floor(sample_rate * 0.01468 + 0.5))
    O = max(int(np.floor(sample_rate * 0.012 + 4.5)), 16) // 8 * 8
    return S, R, O


class TempoGainAugment(object):
    """load_randomly_augmented_audio (utils/audio.py:35-61) with the work on the device: a random tempo in `tempo_range` (pitch kept), then
    a random gain in `gain_range` dB, then the 16-bit file the reference reads back.  Pure numpy: the device part is
    `SpectrogramFrontEnd.batch(augment=)` / `tempo_gain`.  The reference shells out to `sox`, which is no dependency of this project and dithers
    randomly when it writes 16 bits, so the behaviour is DEFINED by the restatement below, parity with sox unpinned (as with librosa in
    the front-end and `sox trim` in NoiseInjection); tests/augment_util.py holds it in numpy and fp64, DESIGN.md section 12 the reasons.

      draws       draw(rng): uniform(*tempo_range), then uniform(*gain_range) -- the reference's two draws, in its order; both reach sox
                  through "{:.3f}".format, so the values used are float('%.3f' % v).
      tempo f     WSOLA with `wsola_geometry(sample_rate)` = (S, R, O), H = S - O.  L samples become N = floor(L / f + 0.5) in
                  M = ceil(N / H) segments; segment m starts in the input at p_m = floor(f (m H) + 0.5) (fp64) shifted by o_m in [0, R]:
                  o_0 = R // 2, and for m >= 1 the c minimising sum_{i<O} (tail_{m-1}[i] - x[p_m + c + i])^2 over ALL R + 1 candidates
                  (fp64, the smallest c on a tie), tail_{m-1}[i] = x[p_{m-1} + o_{m-1} + H + i]; reads at or beyond L give 0.  Output
                  sample m H + i (i < H) is x[p_m + o_m + i], for m >= 1 and i < O cross-faded in fp32 as
                  tail_{m-1}[i] + (i / O) (x[p_m + o_m + i] - tail_{m-1}[i]).  f == 1.0 bypasses the effect (N = L, a copy), as sox does.
      gain, file  y = clip(rint(t g 32768), -32768, 32767) / 32768 with g = (float)10^(gain_db / 20) formed in fp64 and rounded once:
                  sox's 16-bit output without its dither, gain after tempo as in the reference's effect chain (+8 dB does clip)."""

    def __init__(self, tempo_range=(0.85, 1.15), gain_range=(-6, 8)):
        self.tempo_range, self.gain_range = tuple(tempo_range), tuple(gain_range)

    def draw(self, rng):
        """(tempo, gain_db), both rounded to three decimals: uniform(*tempo_range), then uniform(*gain_range), from `rng`"""
        tempo = rng.uniform(low=self.tempo_range[0], high=self.tempo_range[1])
        gain = rng.uniform(low=self.gain_range[0], high=self.gain_range[1])
        return float('{:.3f}'.format(tempo)), float('{:.3f}'.format(gain))

    @staticmethod
    def out_length(n_samples, tempo):
        """N = floor(L / tempo + 0.5); L itself for tempo == 1.0 (the bypass)"""
        if not tempo > 0.0:
            raise ValueError('TempoGainAugment: a tempo factor must be positive, got %r' % (tempo,))
        return int(n_samples) if tempo == 1.0 else int(np.floor(int(n_samples) / float(tempo) + 0.5))

    def plan(self, draws, lengths):
        """K draws and the K utterance lengths -> (tempo float64 (K), gain_db float32 (K), out_lengths int64 (K))"""
        tempo = np.array([d[0] for d in draws], dtype=np.float64)
        gain_db = np.array([d[1] for d in draws], dtype=np.float32)
        out_lengths = np.array([self.out_length(n, t) for n, t in zip(lengths, tempo)], dtype=np.int64)
        return tempo, gain_db, out_lengths


def tempo_gain_tables(waves, tempo, gain_db, sample_rate):
    """host side of the tempo / gain calls, pure numpy: dict(flat float32 (sum of L_k), offsets int64 (K + 1), out_offsets int64 (K + 1)
    from N_k = TempoGainAugment.out_length, seg_base int64 (K + 1): the prefix of the segments per utterance (ceil(N_k / H); none for
    tempo 1.0), tempo float64 (K), gain float32 (K): (float)10^(gain_db / 20), geometry (S, R, O))"""
    if len(waves) == 0:
        raise ValueError('tempo_gain_tables: an empty list of waveforms')
    arrs = []
    for i, w in enumerate(waves):
        a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError('tempo_gain_tables: waveform %d is not one-dimensional (shape %s)' % (i, a.shape))
        arrs.append(a)
    tab = _tempo_gain_plan([a.shape[0] for a in arrs], tempo, gain_db, sample_rate)
    tab['flat'] = np.concatenate(arrs)
    return tab


def _tempo_gain_plan(lengths, tempo, gain_db, sample_rate):
    """`tempo_gain_tables` without the samples, from the K lengths alone (the lengths after a rate conversion are known on the host, the
    samples exist on the device only)"""
    K = len(lengths)
    tempo = np.ascontiguousarray(tempo, dtype=np.float64)
    gain_db = np.ascontiguousarray(gain_db, dtype=np.float32)
    if tempo.shape != (K,) or gain_db.shape != (K,):
        raise ValueError('tempo_gain_tables: %s tempo factors and %s gains for %d waveforms' % (tempo.shape, gain_db.shape, K))
    S, R, O = wsola_geometry(sample_rate)
    if R + 1 > 256 or O > 256:
        raise ValueError('tempo_gain_tables: a search of %d or an overlap of %d samples (sample rate %s) is beyond the 256 the kernel covers'
                         % (R, O, sample_rate))
    H = S - O
    lengths = np.array(lengths, dtype=np.int64)
    out_lengths = np.array([TempoGainAugment.out_length(n, t) for n, t in zip(lengths, tempo)], dtype=np.int64)
    offsets, out_offsets, seg_base = (np.zeros(K + 1, dtype=np.int64) for _ in range(3))
    np.cumsum(lengths, out=offsets[1:])
    np.cumsum(out_lengths, out=out_offsets[1:])
    np.cumsum(np.where(tempo == 1.0, 0, (out_lengths + H - 1) // H), out=seg_base[1:])
    gain = (10.0 ** (gain_db.astype(np.float64) / 20.0)).astype(np.float32)
    return dict(offsets=offsets, out_offsets=out_offsets, seg_base=seg_base, tempo=tempo, gain=gain, geometry=(S, R, O))


def _tempo_gain_launch(lib, stream, tab, d_wav, d_off, d_ooff, d_sbase, d_tempo, d_gain, quantize, device):
    """mtl_tempo_search, then mtl_tempo_render on `stream` (operands on the device, output allocated with the current stream) ->
    (stretched packed waveforms float32, seg_off int32)"""
    from . import _lib
    K, (S, R, O) = tab['tempo'].shape[0], tab['geometry']
    out = torch.empty(max(int(tab['out_offsets'][-1]), 1), dtype=torch.float32, device=device)
    seg_off = torch.empty(max(int(tab['seg_base'][-1]), 1), dtype=torch.int32, device=device)
    _lib.check(lib.mtl_tempo_search(stream, d_wav.data_ptr(), d_off.data_ptr(), d_ooff.data_ptr(), d_tempo.data_ptr(), d_sbase.data_ptr(), K,
                                    S, R, O, seg_off.data_ptr()), 'mtl_tempo_search')
    _lib.check(lib.mtl_tempo_render(stream, d_wav.data_ptr(), d_off.data_ptr(), d_ooff.data_ptr(), d_tempo.data_ptr(), d_gain.data_ptr(),
                                    d_sbase.data_ptr(), seg_off.data_ptr(), K, S, R, O, 1 if quantize else 0, out.data_ptr()),
               'mtl_tempo_render')
    return out[:int(tab['out_offsets'][-1])], seg_off[:int(tab['seg_base'][-1])]


def tempo_gain(waves, tempo, gain_db, sample_rate=16000, quantize=True, device='cuda'):
    """K waveforms stretched to tempo[k] and amplified by gain_db[k] on the device (TempoGainAugment for the semantics) ->
    (list of K float32 numpy arrays, seg_off int32 numpy: the offsets o_m of all segments, utterance after utterance; an utterance at
    tempo 1.0 has none).  quantize=False leaves out gain and the 16-bit rounding: the raw overlap-add.  The unfused form of
    `SpectrogramFrontEnd.batch(augment=)`, on the current stream."""
    from . import _lib
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('tempo and gain are applied on the MI355X only (no CPU fallback)')
    tab = tempo_gain_tables(waves, tempo, gain_db, sample_rate)
    lib = _lib.lib()
    d = {k: torch.from_numpy(tab[k]).to(dev) for k in ('flat', 'offsets', 'out_offsets', 'seg_base', 'tempo', 'gain')}
    if d['flat'].numel() == 0:
        d['flat'] = torch.zeros(1, device=dev)
    out, seg_off = _tempo_gain_launch(lib, torch.cuda.current_stream(dev).cuda_stream, tab, d['flat'], d['offsets'], d['out_offsets'],
                                      d['seg_base'], d['tempo'], d['gain'], quantize, dev)
    out, oo = out.cpu().numpy(), tab['out_offsets']
    return [out[oo[k]:oo[k + 1]].copy() for k in range(len(waves))], seg_off.cpu().numpy()


def load_randomly_augmented_audio(path, sample_rate=16000, tempo_range=(0.85, 1.15), gain_range=(-6, 8)):
    """utils/audio.py:50-61 on the device: tempo and gain drawn from the global np.random like the reference, the utterance as float32
    numpy (16-bit PCM at `sample_rate`: no resampling here)"""
    tempo, gain_db = TempoGainAugment(tempo_range, gain_range).draw(np.random)
    return tempo_gain([load_wav_pcm16(path)], [tempo], [gain_db], sample_rate)[0][0]


# ------------------------------------------------------------------------------------------------------------------
# Sample-rate conversion on the device (audio_with_sox / augment_audio_with_sox, utils/audio.py: `sox -r`); DESIGN.md section 14
# ------------------------------------------------------------------------------------------------------------------
RESAMPLE_MAX_RATIO = 1024
_RESAMPLE_TAPS = {}           # (up, down) -> the fp64 filter of `resample_taps` with its defaults (read-only arrays)


def resample_plan(lengths, rates, sample_rate):
    """K lengths and the K rates of their files -> (out_lengths, up, down), int64 (K) each: g = gcd(rate, sample_rate), up = sample_rate / g,
    down = rate / g, N = ceil(L up / down) in integers.  rate == sample_rate is the bypass (up = down = 1, N = L).  A ratio with
    max(up, down) > 1024 (44101 Hz to 16 kHz, say) raises ValueError: such a filter would have more than 32 k taps."""
    import math
    lengths = np.array(lengths, dtype=np.int64).reshape(-1)
    rates = np.array(rates).reshape(-1)
    if rates.shape != lengths.shape:
        raise ValueError('resample_plan: %d rates for %d waveforms' % (rates.shape[0], lengths.shape[0]))
    target = int(sample_rate)
    if target != sample_rate or target < 1:
        raise ValueError('resample_plan: the target rate must be a positive integer, got %r' % (sample_rate,))
    up, down = np.ones(len(lengths), dtype=np.int64), np.ones(len(lengths), dtype=np.int64)
    for k, r in enumerate(rates):
        if int(r) != r or int(r) < 1:
            raise ValueError('resample_plan: the rate of waveform %d must be a positive integer, got %r' % (k, r))
        g = math.gcd(int(r), target)
        up[k], down[k] = target // g, int(r) // g
        if max(up[k], down[k]) > RESAMPLE_MAX_RATIO:
            raise ValueError('resample_plan: %d Hz to %d Hz is the ratio %d / %d, beyond the %d that the conversion covers'
                             % (int(r), target, up[k], down[k], RESAMPLE_MAX_RATIO))
    return (lengths * up + down - 1) // down, up, down


def resample_taps(up, down, zeros=16, beta=8.6, rolloff=0.95):
    """the filter of the ratio up / down in fp64, 2 half + 1 taps: q = max(up, down), half = zeros q, n = -half .. half, fc = rolloff / q,
    h = fc sinc(fc n) kaiser(2 half + 1, beta), scaled so that sum(h) == up (unit gain at 0 Hz after the zero stuffing): `zeros` zero
    crossings of the sinc on either side, the cutoff at `rolloff` of the lower Nyquist frequency"""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError('resample_taps: up and down must be positive, got %d / %d' % (up, down))
    q = max(up, down)
    half = int(zeros) * q
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = float(rolloff) / q
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, beta)
    return h * (up / h.sum())


def resample_tables(waves, rates, sample_rate):
    """host side of the rate conversion, pure numpy: dict(flat float32 (sum of L_k), offsets int64 (K + 1), out_offsets int64 (K + 1) from
    `resample_plan`, plan int64 (K, 4): up, down, half and the base of the utterance's filter in taps, taps float64: the filters of the
    DISTINCT ratios of this call one after the other (a bypassed utterance has none: half = base = 0; never empty).  The filters are
    formed once per (up, down) and kept."""
    if len(waves) == 0:
        raise ValueError('resample_tables: an empty list of waveforms')
    arrs = []
    for i, w in enumerate(waves):
        a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError('resample_tables: waveform %d is not one-dimensional (shape %s)' % (i, a.shape))
        arrs.append(a)
    K = len(arrs)
    lengths = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    out_lengths, up, down = resample_plan(lengths, rates, sample_rate)
    offsets, out_offsets = np.zeros(K + 1, dtype=np.int64), np.zeros(K + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    np.cumsum(out_lengths, out=out_offsets[1:])
    plan, base, filters, total = np.zeros((K, 4), dtype=np.int64), {}, [], 0
    for k in range(K):
        key = (int(up[k]), int(down[k]))
        plan[k, 0], plan[k, 1] = key
        if key[0] == key[1]:
            continue
        if key not in _RESAMPLE_TAPS:
            h = resample_taps(*key)
            h.setflags(write=False)
            _RESAMPLE_TAPS[key] = h
        if key not in base:
            base[key] = total
            filters.append(_RESAMPLE_TAPS[key])
            total += filters[-1].shape[0]
        plan[k, 2], plan[k, 3] = (_RESAMPLE_TAPS[key].shape[0] - 1) // 2, base[key]
    taps = np.concatenate(filters) if filters else np.zeros(1, dtype=np.float64)
    return dict(flat=np.concatenate(arrs), offsets=offsets, out_offsets=out_offsets, plan=plan, taps=taps)


def _resample_launch(lib, stream, tab, d_wav, d_off, d_ooff, d_plan, d_taps, quantize, device):
    """mtl_resample on `stream` (operands on the device, output allocated with the current stream) -> the converted packed waveforms"""
    from . import _lib
    total = int(tab['out_offsets'][-1])
    out = torch.empty(max(total, 1), dtype=torch.float32, device=device)
    _lib.check(lib.mtl_resample(stream, d_wav.data_ptr(), d_off.data_ptr(), d_ooff.data_ptr(), d_plan.data_ptr(), d_taps.data_ptr(),
                                tab['taps'].shape[0], tab['plan'].shape[0], 1 if quantize else 0, out.data_ptr()), 'mtl_resample')
    return out[:total]


def resample(waves, rates, sample_rate=16000, quantize=True, device='cuda'):
    """K waveforms sampled at rates[k] converted to `sample_rate` on the device -> list of K float32 numpy arrays of
    ceil(L_k up_k / down_k) samples (`resample_plan`, `resample_taps` and DESIGN.md section 14 for the definition: a zero-phase
    Kaiser-windowed sinc with zero extension, fp64 sums; sox is not reproduced sample for sample).  quantize=True rounds to the 16-bit
    file that audio_with_sox leaves (without sox's dither), quantize=False returns the sums rounded once to fp32.  An utterance that is at
    `sample_rate` already is copied bit for bit either way.  The unfused form of `SpectrogramFrontEnd.batch(rates=)`, on the current stream."""
    from . import _lib
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('sample rates are converted on the MI355X only (no CPU fallback)')
    tab = resample_tables(waves, rates, sample_rate)
    lib = _lib.lib()
    d = {k: torch.from_numpy(tab[k]).to(dev) for k in ('flat', 'offsets', 'out_offsets', 'plan', 'taps')}
    if d['flat'].numel() == 0:
        d['flat'] = torch.zeros(1, device=dev)
    out = _resample_launch(lib, torch.cuda.current_stream(dev).cuda_stream, tab, d['flat'], d['offsets'], d['out_offsets'], d['plan'],
                           d['taps'], quantize, dev)
    out, oo = out.cpu().numpy(), tab['out_offsets']
    return [out[oo[k]:oo[k + 1]].copy() for k in range(len(waves))]


class SpectrogramFrontEnd:
    """wav -> STFT (n_fft = win = sample_rate*window_size, hop = sample_rate*window_stride, symmetric Hamming window,
    center + reflect padding = librosa.stft defaults of the reference era) -> |.| -> log1p -> (x-mean)/std, all on the MI355X:
    the STFT is one fp32-MFMA GEMM (frames = overlapping rows of the padded waveform, lda = hop) against a windowed DFT basis."""

    _NAME = 'spectrogram'                                      # (in the messages of `batch`, which LogFBankFrontEnd shares)

    def __init__(self, sample_rate=16000, window_size=0.02, window_stride=0.01, window='hamming', normalize=True, device='cuda',
                 consumer=None):
        """consumer: the stream on which the batches of `batch()` are read (default: the device's current stream at construction --
        the stream on which TransientTrainer._batched_iteration copies device-resident inputs into its static buffers)."""
        from scipy.signal import windows as sw
        self.sample_rate = sample_rate
        self.n_fft = int(sample_rate * window_size)
        self.hop = int(sample_rate * window_stride)
        self.F = self.n_fft // 2 + 1
        self.normalize = normalize
        self.device = torch.device(device)
        table = {'hamming': sw.hamming, 'hann': sw.hann, 'blackman': sw.blackman, 'bartlett': sw.bartlett}
        win = table[window](self.n_fft)                       # the reference passes the scipy FUNCTION -> symmetric window
        n = np.arange(self.n_fft)[:, None].astype(np.float64)
        f = np.arange(self.F)[None, :].astype(np.float64)
        ang = 2.0 * np.pi * n * f / self.n_fft
        self.ldb = (2 * self.F + 3) // 4 * 4
        basis = np.zeros((self.n_fft, self.ldb), dtype=np.float32)
        basis[:, :self.F] = (win[:, None] * np.cos(ang)).astype(np.float32)
        basis[:, self.F:2 * self.F] = (-win[:, None] * np.sin(ang)).astype(np.float32)
        self.basis = torch.from_numpy(basis).to(self.device)
        self.partials = torch.empty(512, dtype=torch.float64, device=self.device)
        self._init_batch_state(consumer)

    def _init_batch_state(self, consumer):
        self.consumer = consumer if consumer is not None or self.device.type != 'cuda' else torch.cuda.current_stream(self.device)
        self.stream = None                                     # batch()'s own stream, made at its first call
        self._pin_wav = self._pin_off = None                   # pinned staging of batch(), grown on demand
        self._pin_noff = self._pin_lvl = None                  # ... and of its two noise tables
        self._pin_aug = self._pin_tempo = self._pin_gain = None # ... and of the augmentation tables
        self._pin_rs = self._pin_taps = None                   # ... and of the rate conversion's tables

    def __call__(self, y):
        """y: 1-D float waveform (numpy or tensor) -> (F, T) fp32 tensor on the device, T = 1 + len(y) // hop."""
        from . import _lib
        if self.device.type != 'cuda':
            raise RuntimeError('the spectrogram front-end runs on the MI355X only (no CPU fallback)')
        lib = _lib.lib()
        y = np.asarray(y.detach().cpu() if torch.is_tensor(y) else y, dtype=np.float32).reshape(-1)
        pad = self.n_fft // 2
        yp = torch.from_numpy(np.pad(y, (pad, pad), mode='reflect')).to(self.device)
        T = 1 + y.shape[0] // self.hop
        reim = torch.empty(T, self.ldb, device=self.device)
        out = torch.empty(self.F, T, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(lib.mtl_gemm_f32(st, 0, 0, T, 2 * self.F, self.n_fft, 1.0, yp.data_ptr(), self.hop, self.basis.data_ptr(), self.ldb,
                                    reim.data_ptr(), self.ldb, None, None, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, None, 0), 'stft gemm')
        _lib.check(lib.mtl_spect_logmag(st, reim.data_ptr(), self.ldb, T, self.F, out.data_ptr(), self.partials.data_ptr(),
                                        1 if self.normalize else 0), 'mtl_spect_logmag')
        return out

    def batch(self, waves, max_frames=None, noise=None, augment=None, rates=None):
        """K waveforms -> (inputs (K, 1, F, Tmax) fp32 on the device, input_sizes (K) int32 on the host): what `collate` builds from
        K `__call__` results cut to max_frames, in one device pass -- one pinned staging copy of the concatenated samples and of the
        offsets (two H2D copies) and the two launches of mtl_spect_batch (framing, STFT, log-magnitude, per-utterance statistics over
        the WHOLE utterance, normalisation, zero padding).

        Streams and lifetime: the front-end owns one stream.  `inputs` is allocated with that stream current (its block belongs to
        that stream's pool), the copies and launches run there, and the calling thread waits on an event recorded behind them: the
        batch is complete when this returns, whatever the training kernels queued on other streams are doing, and nothing here
        waits for them (no device-wide synchronisation).  `inputs.record_stream(consumer)` then tells the allocator that `consumer`
        reads the block: the trainer's host thread enqueues up to two iterations ahead, so the tensor is usually dropped while the
        trainer's copy of it is still pending -- without the record the next `batch` call could be handed the same memory and
        overwrite it under that copy.

        noise=(injector, noise_off, level), the output of `NoiseInjection.plan` for these K waveforms: utterance k is mixed with the
        len(waves[k]) samples of the injector's device-resident int16 bank from noise_off[k] on (noise_off[k] < 0: clean) at
        level[k], as NoiseInjection.inject_noise_sample does (utils/data_loader.py:383-399), while the samples are staged -- no mixed
        waveform exists in memory and the host does not touch the samples.  The two tables (K int64, K float32) travel through
        pinned staging like the offsets; the calls are mtl_wave_mix_coef, then mtl_spect_batch_noise, on the same stream under the
        same event.  noise=None issues exactly the calls described above.

        augment=(tempo, gain_db), K values each (`TempoGainAugment.plan` for these K waveforms): utterance k is first stretched to
        tempo[k] and amplified by gain_db[k] as `tempo_gain` does -- mtl_tempo_search, then mtl_tempo_render into a packed buffer of the
        stretched waveforms at new offsets -- and the calls above run unchanged on THAT buffer and its offsets, all on the same stream
        under the same event: the result is bitwise `batch(tempo_gain(waves, tempo, gain_db)[0], ...)`.  input_sizes, Tmax and the
        n_fft // 2 + 1 minimum of `pack_waveforms` refer to the stretched lengths, and a noise plan must have been made for them.  The
        offsets, the segment table's prefix, the factors and the gains travel through pinned staging like the noise tables.
        augment=None issues exactly the calls described above.

        rates=K sample rates, those of the files that `waves` were read from (`load_wav_pcm16_rate`): utterance k is first converted
        from rates[k] to this front-end's sample rate as `resample` does -- ONE more launch, mtl_resample, in front of the tempo stage,
        into a packed buffer of the converted waveforms at new offsets -- and everything above (tempo and gain, noise, the STFT) runs
        unchanged on that buffer at the target rate, on the same stream under the same event: the result is bitwise
        `batch(resample(waves, rates, sample_rate), ...)` with the same other arguments.  (Conversion first is this project's choice: the
        later stages are defined at the front-end's rate.  sox's own chain `tempo f gain g rate r` converts last.)  input_sizes, Tmax and
        the n_fft // 2 + 1 minimum refer to the converted lengths (`resample_plan`), and the augmentation and noise plans must have been
        made for them.  The original samples, the input offsets with the per-utterance plan and the filters travel through pinned
        staging.  No random draw is involved.  An utterance that is at the target rate already is copied bit for bit.  rates=None
        issues exactly the calls described above."""
        from . import _lib
        if self.device.type != 'cuda':
            raise RuntimeError('the %s front-end runs on the MI355X only (no CPU fallback)' % self._NAME)
        lib = _lib.lib()
        aug = rs = None
        if augment is None and rates is None:
            flat, offsets, frames, tmax = self._pack(waves, max_frames)
        else:
            # the samples that are uploaded are the original ones; everything downstream sees the converted / stretched lengths
            if rates is not None:
                rs = resample_tables(waves, rates, self.sample_rate)
                flat, offsets = rs['flat'], rs['out_offsets']
            if augment is not None and rs is None:
                aug = tempo_gain_tables(waves, augment[0], augment[1], self.sample_rate)
                flat, offsets = aug['flat'], aug['out_offsets']
            elif augment is not None:
                aug = _tempo_gain_plan(np.diff(rs['out_offsets']), augment[0], augment[1], self.sample_rate)
                offsets = aug['out_offsets']
            self._check_lengths(np.diff(offsets), 'rate conversion' if aug is None else 'tempo change')
            frames = self._frame_counts(np.diff(offsets))
            if max_frames is not None:
                frames = np.minimum(frames, max_frames)
            frames = frames.astype(np.int32)
            tmax = int(frames.max())
        K = len(frames)
        ws_bytes = self._workspace_bytes(lib, np.diff(offsets), K)
        if self.stream is None:
            self.stream = torch.cuda.Stream(self.device)
        if self._pin_wav is None or self._pin_wav.numel() < flat.shape[0]:
            self._pin_wav = torch.empty(max(flat.shape[0], 1 << 16), dtype=torch.float32).pin_memory()
        if self._pin_off is None or self._pin_off.numel() < K + 1:
            self._pin_off = torch.empty(max(K + 1, 64), dtype=torch.int64).pin_memory()
        # the staging buffers are free again: every earlier call waited for its copies before it returned
        self._pin_wav[:flat.shape[0]].copy_(torch.from_numpy(flat))
        self._pin_off[:K + 1].copy_(torch.from_numpy(offsets))
        if noise is not None:
            injector, noise_off, level = noise
            noise_off, level = np.ascontiguousarray(noise_off, dtype=np.int64), np.ascontiguousarray(level, dtype=np.float32)
            if noise_off.shape != (K,) or level.shape != (K,):
                raise ValueError('batch: the noise plan has %s offsets and %s levels for %d waveforms' % (noise_off.shape, level.shape, K))
            lengths = np.diff(offsets)
            if ((noise_off >= 0) & (noise_off + lengths > injector.bank_len)).any():
                raise ValueError('batch: a noise segment ends beyond the bank (%d samples)' % injector.bank_len)
            bank = injector.device_bank(self.device)
            cws_bytes = lib.mtl_wave_mix_coef_workspace(K)
            if cws_bytes < 0:
                raise RuntimeError('mtl_wave_mix_coef_workspace failed with code %d' % cws_bytes)
            if self._pin_noff is None or self._pin_noff.numel() < K:
                self._pin_noff = torch.empty(max(K, 64), dtype=torch.int64).pin_memory()
                self._pin_lvl = torch.empty(max(K, 64), dtype=torch.float32).pin_memory()
            self._pin_noff[:K].copy_(torch.from_numpy(noise_off))
            self._pin_lvl[:K].copy_(torch.from_numpy(level))
        if aug is not None:
            if self._pin_aug is None or self._pin_aug.numel() < 2 * (K + 1):
                self._pin_aug = torch.empty(max(2 * (K + 1), 128), dtype=torch.int64).pin_memory()
                self._pin_tempo = torch.empty(max(K, 64), dtype=torch.float64).pin_memory()
                self._pin_gain = torch.empty(max(K, 64), dtype=torch.float32).pin_memory()
            self._pin_aug[:K + 1].copy_(torch.from_numpy(aug['offsets']))
            self._pin_aug[K + 1:2 * (K + 1)].copy_(torch.from_numpy(aug['seg_base']))
            self._pin_tempo[:K].copy_(torch.from_numpy(aug['tempo']))
            self._pin_gain[:K].copy_(torch.from_numpy(aug['gain']))
        if rs is not None:
            n_taps = rs['taps'].shape[0]
            if self._pin_rs is None or self._pin_rs.numel() < 5 * K + 1:
                self._pin_rs = torch.empty(max(5 * K + 1, 128), dtype=torch.int64).pin_memory()
            if self._pin_taps is None or self._pin_taps.numel() < n_taps:
                self._pin_taps = torch.empty(max(n_taps, 1 << 12), dtype=torch.float64).pin_memory()
            self._pin_rs[:K + 1].copy_(torch.from_numpy(rs['offsets']))
            self._pin_rs[K + 1:5 * K + 1].copy_(torch.from_numpy(rs['plan'].reshape(-1)))
            self._pin_taps[:n_taps].copy_(torch.from_numpy(rs['taps']))
        with torch.cuda.stream(self.stream):
            inputs = torch.empty(K, 1, self.F, tmax, device=self.device)
            d_wav = torch.empty(flat.shape[0], device=self.device)
            d_off = torch.empty(K + 1, dtype=torch.int64, device=self.device)
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
            d_wav.copy_(self._pin_wav[:flat.shape[0]], non_blocking=True)
            d_off.copy_(self._pin_off[:K + 1], non_blocking=True)
            if rs is not None:
                d_rs = torch.empty(5 * K + 1, dtype=torch.int64, device=self.device)
                d_taps = torch.empty(n_taps, dtype=torch.float64, device=self.device)
                d_rs.copy_(self._pin_rs[:5 * K + 1], non_blocking=True)
                d_taps.copy_(self._pin_taps[:n_taps], non_blocking=True)
            if aug is not None:                                 # d_wav holds the original samples, d_off the STRETCHED offsets
                d_aug = torch.empty(2 * (K + 1), dtype=torch.int64, device=self.device)
                d_tempo = torch.empty(K, dtype=torch.float64, device=self.device)
                d_gain = torch.empty(K, dtype=torch.float32, device=self.device)
                d_aug.copy_(self._pin_aug[:2 * (K + 1)], non_blocking=True)
                d_tempo.copy_(self._pin_tempo[:K], non_blocking=True)
                d_gain.copy_(self._pin_gain[:K], non_blocking=True)
            if rs is not None:                                  # the converted offsets are the next stage's input offsets
                d_wav = _resample_launch(lib, self.stream.cuda_stream, rs, d_wav, d_rs[:K + 1], d_off if aug is None else d_aug[:K + 1],
                                         d_rs[K + 1:], d_taps, True, self.device)
            if aug is not None:
                d_wav, _ = _tempo_gain_launch(lib, self.stream.cuda_stream, aug, d_wav, d_aug[:K + 1], d_off, d_aug[K + 1:], d_tempo, d_gain,
                                              True, self.device)
            if noise is None:
                self._features_launch(lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, None)
            else:
                d_noff = torch.empty(K, dtype=torch.int64, device=self.device)
                d_lvl = torch.empty(K, dtype=torch.float32, device=self.device)
                coef = torch.empty(K, dtype=torch.float32, device=self.device)
                cws = torch.empty(cws_bytes // 8, dtype=torch.float64, device=self.device)
                d_noff.copy_(self._pin_noff[:K], non_blocking=True)
                d_lvl.copy_(self._pin_lvl[:K], non_blocking=True)
                _lib.check(lib.mtl_wave_mix_coef(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, bank.data_ptr(),
                                                 injector.bank_len, d_noff.data_ptr(), d_lvl.data_ptr(), coef.data_ptr(), cws.data_ptr(),
                                                 cws_bytes), 'mtl_wave_mix_coef')
                self._features_launch(lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, (bank, injector.bank_len, d_noff, coef))
            done = torch.cuda.Event()
            done.record(self.stream)
        done.synchronize()                                     # host wait on this stream's event only
        inputs.record_stream(self.consumer)
        return inputs, torch.from_numpy(frames)

    # what `batch` asks of the feature type (LogFBankFrontEnd overrides these five and nothing else of `batch`)
    def _pack(self, waves, max_frames):
        return pack_waveforms(waves, self.hop, self.n_fft, max_frames)

    def _check_lengths(self, lengths, stage):
        short = np.flatnonzero(lengths < self.n_fft // 2 + 1)
        if short.size:
            raise ValueError('batch: utterance %d has %d samples after the %s, fewer than n_fft // 2 + 1 = %d (one reflection '
                             'must suffice)' % (short[0], lengths[short[0]], stage, self.n_fft // 2 + 1))

    def _frame_counts(self, lengths):
        return 1 + lengths // self.hop

    def _workspace_bytes(self, lib, lengths, K):
        ws_bytes = lib.mtl_spect_batch_workspace(int(self._frame_counts(lengths).sum()), K, self.F)
        if ws_bytes < 0:
            raise RuntimeError('mtl_spect_batch_workspace failed with code %d' % ws_bytes)
        return ws_bytes

    def _features_launch(self, lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, mix):
        """the last call of `batch` on its stream: packed waveforms -> inputs.  mix = (bank, bank_len, d_noff, coef) behind
        mtl_wave_mix_coef, or None for clean utterances"""
        from . import _lib
        if mix is None:
            _lib.check(lib.mtl_spect_batch(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.n_fft, self.hop,
                                           self.basis.data_ptr(), self.ldb, self.F, inputs.data_ptr(), tmax, 1 if self.normalize else 0,
                                           ws.data_ptr(), ws_bytes), 'mtl_spect_batch')
        else:
            bank, bank_len, d_noff, coef = mix
            _lib.check(lib.mtl_spect_batch_noise(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.n_fft, self.hop,
                                                 self.basis.data_ptr(), self.ldb, self.F, inputs.data_ptr(), tmax,
                                                 1 if self.normalize else 0, ws.data_ptr(), ws_bytes, bank.data_ptr(), bank_len,
                                                 d_noff.data_ptr(), coef.data_ptr()), 'mtl_spect_batch_noise')

    def resample(self, waves, rates, quantize=True):
        """`resample` to this front-end's sample rate on its device: list of K converted float32 numpy arrays"""
        return resample(waves, rates, self.sample_rate, quantize, self.device)

    def tempo_gain(self, waves, tempo, gain_db, quantize=True):
        """`tempo_gain` at this front-end's sample rate and device: (list of K stretched float32 numpy arrays, seg_off)"""
        return tempo_gain(waves, tempo, gain_db, self.sample_rate, quantize, self.device)


# ------------------------------------------------------------------------------------------------------------------
# Log-mel filterbank front-end on the device (LogFBankDataset.parse_audio, utils/data_loader.py:145-155); DESIGN.md section 15
# ------------------------------------------------------------------------------------------------------------------
FBANK_EPS = 2.220446049250313e-16          # what an energy of exactly zero becomes before the logarithm


def fbank_geometry(rate):
    """(fl, fs, nfft) of the 25 ms / 10 ms framing at `rate`: fl = floor(0.025 R + 0.5), fs = floor(0.01 R + 0.5), nfft = 512 (400 / 160 at
    16 kHz, 200 / 80 at 8 kHz).  A rate whose frame is longer than the transform (R > 20480) raises ValueError: the library would cut the
    frames, and that is not reproduced."""
    import math
    fl, fs, nfft = int(math.floor(0.025 * rate + 0.5)), int(math.floor(0.01 * rate + 0.5)), 512
    if fl < 1 or fs < 1:
        raise ValueError('fbank_geometry: a sample rate of %r Hz has no 25 ms frame' % (rate,))
    if fl > nfft:
        raise ValueError('fbank_geometry: a 25 ms frame at %r Hz has %d samples, more than nfft = %d' % (rate, fl, nfft))
    return fl, fs, nfft


def fbank_frames(lengths, rate):
    """frames of utterances of `lengths` samples (each >= 1) at `rate`: 1 for L <= fl, else 1 + ceil((L - fl) / fs); int64 array"""
    fl, fs, _ = fbank_geometry(rate)
    lengths = np.array(lengths, dtype=np.int64).reshape(-1)
    if (lengths < 1).any():
        raise ValueError('fbank_frames: an utterance without samples')
    return np.where(lengths <= fl, 1, 1 + (lengths - fl + fs - 1) // fs).astype(np.int64)


def mel_filterbank(nfilt=80, nfft=512, rate=16000):
    """the dense (nfilt, nfft // 2 + 1) fp64 table of triangular mel bands: mel points linspace(mel(0), mel(R / 2), nfilt + 2) with
    mel(h) = 2595 log10(1 + h / 700), bins b[j] = floor((nfft + 1) hz(m_j) / R), band j rising over [b[j], b[j+1]) and falling over
    [b[j+1], b[j+2]).  At 16 kHz the bins begin 0, 0, 1, 2, 2, 3, so band 2 has no weight at all: kept, not repaired."""
    high = rate / 2.0
    m = np.linspace(2595.0 * np.log10(1.0 + 0.0 / 700.0), 2595.0 * np.log10(1.0 + high / 700.0), nfilt + 2)
    b = np.floor((nfft + 1) * (700.0 * (10.0 ** (m / 2595.0) - 1.0)) / rate)
    fb = np.zeros((nfilt, nfft // 2 + 1), dtype=np.float64)
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def mel_filterbank_sparse(fb):
    """dense table -> (band int32 (nfilt, 3): first bin, count, offset of the band's weights; weights float32, never empty): per band
    the range from its first to its last non-zero weight, rounded once to fp32.  A band without weight has count 0."""
    band, w = np.zeros((fb.shape[0], 3), dtype=np.int32), []
    for j in range(fb.shape[0]):
        nz = np.flatnonzero(fb[j])
        if nz.size:
            band[j] = nz[0], nz[-1] - nz[0] + 1, len(w)
            w.extend(fb[j, nz[0]:nz[-1] + 1])
    return band, np.array(w if w else [0.0], dtype=np.float32)


class LogFBankFrontEnd(SpectrogramFrontEnd):
    """wav -> `nfilt` log mel filterbank energies per 25 ms frame every 10 ms (logfbank(sig, rate, nfilt=80) of python_speech_features
    with its defaults, restated in DESIGN.md section 15: scale to int16 values, pre-emphasis 0.97, rectangular 25 ms frames without
    centring, |DFT_512|^2 / 512, triangular mel bands, ln, energy 0 -> ln(2^-52)) -> (x - mean) / std over the utterance, all on the
    MI355X in the two launches of mtl_fbank_batch.  `batch` is SpectrogramFrontEnd.batch -- streams, pinned staging, record_stream, and the
    rate / tempo / noise stages in front of the last call -- with this feature type's frame count (`fbank_frames`), a minimum length of
    one sample, and mtl_fbank_batch as the last call (behind the unfused mtl_wave_mix when noise is given).  Only that method and its
    five hooks are shared: the base constructor is not called (no window, no STFT basis, no `partials`)."""

    _NAME = 'log-mel filterbank'

    def __init__(self, sample_rate=16000, nfilt=80, normalize=True, device='cuda', consumer=None):
        self.sample_rate = sample_rate
        self.fl, self.fs, self.nfft = fbank_geometry(sample_rate)
        self.nfilt = self.F = int(nfilt)
        if self.nfilt < 1:
            raise ValueError('LogFBankFrontEnd: nfilt must be positive, got %r' % (nfilt,))
        self.normalize = normalize
        self.device = torch.device(device)
        nbins = self.nfft // 2 + 1
        ang = 2.0 * np.pi * np.arange(self.fl, dtype=np.float64)[:, None] * np.arange(nbins, dtype=np.float64)[None, :] / self.nfft
        self.ldb = (2 * nbins + 3) // 4 * 4
        basis = np.zeros((self.fl, self.ldb), dtype=np.float32)          # fp64, rounded once; only fl rows: the zero padding is free
        basis[:, :nbins] = np.cos(ang).astype(np.float32)
        basis[:, nbins:2 * nbins] = (-np.sin(ang)).astype(np.float32)
        self.filterbank = mel_filterbank(self.nfilt, self.nfft, sample_rate)
        band, w = mel_filterbank_sparse(self.filterbank)
        self.basis = torch.from_numpy(basis).to(self.device)
        self.band, self.band_w = torch.from_numpy(band).to(self.device), torch.from_numpy(w).to(self.device)
        self._init_batch_state(consumer)

    def __call__(self, y):
        """y: 1-D float waveform (numpy or tensor, >= 1 sample) -> (nfilt, T) fp32 tensor on the device, T = fbank_frames([len(y)])"""
        return self.batch([y])[0][0, 0]

    def batch(self, waves, max_frames=None, noise=None, augment=None, rates=None):
        """K waveforms -> (inputs (K, 1, nfilt, Tmax) fp32 on the device, input_sizes (K) int32 on the host): what `collate` builds from
        K `__call__` results cut to max_frames, in one device pass -- one pinned staging copy of the concatenated samples and of the
        offsets and the two launches of mtl_fbank_batch (staging with scaling and pre-emphasis, the 512-point DFT, power, bands, ln,
        per-utterance statistics over the WHOLE utterance, normalisation, zero padding).  input_sizes are `fbank_frames` of the
        lengths, cut to max_frames; an utterance needs one sample.

        Streams, pinned staging and `record_stream` are those of SpectrogramFrontEnd.batch (it is that method), and so are the
        meanings of the three optional stages, each of which leaves a packed waveform in front of the last call:
        rates= converts utterance k from rates[k] to this front-end's rate (mtl_resample), augment=(tempo, gain_db) stretches and
        amplifies it (mtl_tempo_search, mtl_tempo_render), noise=(injector, noise_off, level) mixes it with the injector's bank
        (mtl_wave_mix_coef, then the UNFUSED mtl_wave_mix into a second packed buffer: the mix is not folded into this kernel's
        staging).  The result is bitwise `batch` of the waveforms that `resample`, `tempo_gain` and mtl_wave_mix give; frame counts and
        the one-sample minimum refer to the converted / stretched lengths.  With none of them exactly the calls above are issued."""
        return super().batch(waves, max_frames=max_frames, noise=noise, augment=augment, rates=rates)

    def _pack(self, waves, max_frames):
        if len(waves) == 0:
            raise ValueError('batch: an empty list of waveforms')
        arrs = []
        for i, w in enumerate(waves):
            a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError('batch: waveform %d is not one-dimensional (shape %s)' % (i, a.shape))
            arrs.append(a)
        lengths = np.array([a.shape[0] for a in arrs], dtype=np.int64)
        self._check_lengths(lengths, 'load')
        offsets = np.zeros(len(arrs) + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        frames = self._frame_counts(lengths)
        if max_frames is not None:
            frames = np.minimum(frames, max_frames)
        frames = frames.astype(np.int32)
        return np.concatenate(arrs), offsets, frames, int(frames.max())

    def _check_lengths(self, lengths, stage):
        short = np.flatnonzero(lengths < 1)
        if short.size:
            raise ValueError('batch: utterance %d has no samples after the %s' % (short[0], stage))

    def _frame_counts(self, lengths):
        return fbank_frames(lengths, self.sample_rate)

    def _workspace_bytes(self, lib, lengths, K):
        ws_bytes = lib.mtl_fbank_batch_workspace(K)
        if ws_bytes < 0:
            raise RuntimeError('mtl_fbank_batch_workspace failed with code %d' % ws_bytes)
        return ws_bytes

    def _features_launch(self, lib, d_wav, d_off, K, inputs, tmax, ws, ws_bytes, mix):
        from . import _lib
        if mix is not None:                                    # the unfused mix: a packed buffer of the mixed waveforms, same offsets
            bank, bank_len, d_noff, coef = mix
            mixed = torch.empty_like(d_wav)
            _lib.check(lib.mtl_wave_mix(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, bank.data_ptr(), bank_len,
                                        d_noff.data_ptr(), coef.data_ptr(), mixed.data_ptr()), 'mtl_wave_mix')
            d_wav = mixed
        _lib.check(lib.mtl_fbank_batch(self.stream.cuda_stream, d_wav.data_ptr(), d_off.data_ptr(), K, self.fl, self.fs, self.nfft,
                                       self.basis.data_ptr(), self.ldb, self.nfilt, self.band.data_ptr(), self.band_w.data_ptr(),
                                       self.band_w.numel(), inputs.data_ptr(), tmax, 1 if self.normalize else 0, ws.data_ptr(), ws_bytes),
                   'mtl_fbank_batch')


class LogFBankDataset(ManifestTaskDataset):
    """utils/data_loader.py:101-168 with the reference's OWN constructor (test.py:199-200):

        LogFBankDataset(vocab, args, audio_conf, manifest_filepath_list=..., normalize=True, augment=False, input_type='char')

    80 log mel filterbank energies per frame from the device front-end (LogFBankFrontEnd at audio_conf['sample_rate']) unless a
    `feature_fn` is given.  Same attributes as the reference object (max_size = longest manifest x manifests, ids_list, input_type,
    manifest_filepath_list, normalize, vocab), the same two console lines, and its __getitem__ (manifests interleaved by index).
    Beyond the reference: `sample()` and the keywords partitions, seed, device_batches, resample and feature_fn of the
    ManifestTaskDataset machinery -- for one seed the index and draw stream is that of SpectrogramDataset -- and audio_conf['noise_dir'] /
    augment=True, which the reference's class accepts and ignores, work as on SpectrogramDataset, with the same rejections."""

    def __init__(self, vocab, args, audio_conf, manifest_filepath_list, normalize=False, augment=False, input_type='char',
                 is_train=False, partitions=None, feature_fn=None, seed=None, device_batches=False, resample=False):
        noise = _wav_dataset_options(self, audio_conf, feature_fn, augment, device_batches, resample, input_type, '157-165')
        self.sample_rate = audio_conf.get('sample_rate', getattr(args, 'sample_rate', 16000))
        fbank_geometry(self.sample_rate)                             # a rate beyond the 512-point transform is rejected here
        self.normalize, self.augment, self.noise_prob = normalize, augment, audio_conf.get('noise_prob')
        fe = []           # built at the first utterance: constructing the dataset must not need the device

        def front_end():
            if not fe:
                fe.append(LogFBankFrontEnd(self.sample_rate, 80, self.normalize))
            return fe[0]
        if feature_fn is None:
            def feature_fn(path):
                return front_end()(load_wav_pcm16(path)).cpu()
        super().__init__(vocab, args, manifest_filepath_list, feature_fn=feature_fn, partitions=partitions, seed=seed, is_train=is_train)
        _wav_dataset_wiring(self, noise, augment, resample, device_batches, front_end, manifest_filepath_list, input_type)
        self.max_size = max(len(ids) for ids in self.ids_list) * len(self.ids_list)      # :114-122: no 30000 rule in this class
        print('max_size:', self.max_size)
        print('input_type:', input_type)

    def parse_transcript(self, transcript_path):
        return parse_transcript(self.vocab, transcript_path)

    def parse_audio(self, audio_path):
        """utils/data_loader.py:145-155; with augmentation and / or a noise injector, this utterance's draws from the dataset's stream"""
        draws = self._draws(1)
        return self._feature(audio_path, None if draws is None else draws[0])

    def __getitem__(self, index):
        """utils/data_loader.py:133-143: the manifests interleaved by index, whatever is_train says"""
        ids = self.ids_list[index % len(self.ids_list)]
        row = ids[(index // len(self.ids_list)) % len(ids)]
        draws = self._draws(1)
        return self._feature(row[0], None if draws is None else draws[0])[:, :self.args.src_max_len], parse_transcript(self.vocab, row[1])


class NoiseInjection(object):
    """utils/data_loader.py:367-399 with the mix on the device: `data += level * noise * rms(data) / rms(noise)`, `noise` being a
    segment of a randomly chosen noise file as long as the utterance.  The reference's constructor plus `device` and `bank_gb`;
    constructing needs no device (the device copy of the bank is made at first use and kept).  What the reference leaves to sox / soxi
    is pinned here:

      file list   `paths` = the sorted recursive list of *.wav under `path` (stands in for librosa.util.find_files).  Files are 16-bit
                  PCM at `sample_rate`; channels are averaged as load_wav_pcm16 does and rounded back to int16.  Any other sample width
                  or rate raises ValueError naming the file, a missing directory IOError (like the reference), an empty one ValueError,
                  a corpus of more than `bank_gb` GiB ValueError.  All files live in ONE int16 array (`bank`) with per-file
                  (`offsets`, `lengths`), in samples.
      draws       draw(rng, noise_prob): binomial(1, noise_prob) and, only when it gave 1, in this order choice(paths),
                  uniform(*noise_levels), rand() -- the reference's four draws (:73, :384-385, :391).
      placement   in samples: start = floor(u * (N_file - n)), segment [start, start + n) -- equal lengths by construction (the
                  reference hands seconds to `sox trim` and asserts the lengths afterwards).
      too long    an utterance longer than the chosen noise file stays clean (the reference would fail its assert): its draws are
                  consumed all the same, `skipped` is incremented and one logging.warning is issued per file.  A segment whose energy
                  is exactly zero leaves the utterance clean as well (the reference would produce inf / nan).
      arithmetic  S_d, S_n = sums of squares over the n samples in fp64, fixed order, no atomics; c = level * sqrt(S_d / n) /
                  sqrt(S_n / n) in fp64, rounded once to fp32; mixed = fmaf(c, noise, data) in fp32 with noise = (float)int16 / 32768
                  (exact).  Every kernel that mixes uses this one expression: fused and unfused paths agree bit for bit."""

    def __init__(self, path=None, sample_rate=16000, noise_levels=(0, 0.5), device='cuda', bank_gb=8.0):
        import glob
        import wave
        if path is None or not os.path.exists(path):
            print("Directory doesn't exist: {}".format(path))
            raise IOError("Directory doesn't exist: {}".format(path))
        self.paths = sorted(glob.glob(os.path.join(glob.escape(path), '**', '*.wav'), recursive=True))
        if not self.paths:
            raise ValueError('NoiseInjection: no *.wav file under %s' % path)
        self.sample_rate, self.noise_levels, self.device = sample_rate, tuple(noise_levels), torch.device(device)
        self.skipped, self._warned, self._bank = 0, set(), None
        lengths = []
        for p in self.paths:                                   # headers first: the bank limit is checked before anything is read
            with wave.open(p, 'rb') as w:
                if w.getsampwidth() != 2:
                    raise ValueError('NoiseInjection: %s has %d-byte samples, only 16-bit PCM is supported' % (p, w.getsampwidth()))
                if w.getframerate() != sample_rate:
                    raise ValueError('NoiseInjection: %s is sampled at %d Hz, the front-end at %d Hz (no resampling here)'
                                     % (p, w.getframerate(), sample_rate))
                lengths.append(w.getnframes())
        self.lengths = np.array(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.bank_len = int(self.lengths.sum())
        if self.bank_len == 0:
            raise ValueError('NoiseInjection: the *.wav files under %s hold no samples' % path)
        if 2 * self.bank_len > bank_gb * 2 ** 30:
            raise ValueError('NoiseInjection: the noise corpus under %s takes %.3f GiB as int16, more than bank_gb=%g'
                             % (path, 2 * self.bank_len / 2.0 ** 30, bank_gb))
        self.bank = np.empty(self.bank_len, dtype=np.int16)
        for p, o, n in zip(self.paths, self.offsets, self.lengths):
            with wave.open(p, 'rb') as w:
                ch = w.getnchannels()
                raw = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2')
            if ch > 1:                                         # load_wav_pcm16's channel mean (fp32), back on the int16 grid
                mean = (raw.astype(np.float32) / 32768.0).reshape(-1, ch).mean(axis=1).astype(np.float32)
                raw = np.clip(np.rint(mean * 32768.0), -32768, 32767).astype(np.int16)
            self.bank[o:o + n] = raw

    def device_bank(self, device=None):
        """the int16 bank on the device: uploaded at the first call and kept"""
        if self._bank is None:
            dev = torch.device(device) if device is not None else self.device
            if dev.type != 'cuda':
                raise RuntimeError('noise is mixed on the MI355X only (no CPU fallback)')
            self._bank = torch.from_numpy(self.bank).to(dev)
        return self._bank

    def draw(self, rng, noise_prob):
        """None (clean) | (file_index, level, u): binomial, then -- only if it gave 1 -- choice, uniform, rand, from `rng`"""
        if not rng.binomial(1, float(noise_prob)):
            return None
        path = rng.choice(self.paths)
        level = rng.uniform(*self.noise_levels)
        return self.paths.index(path), float(level), float(rng.rand())

    def place(self, draw, n_samples):
        """(bank_offset, level) of the segment [start, start + n_samples) of the drawn file, start = floor(u * (N_file - n_samples));
        None for a clean draw and for an utterance longer than the file (counted in `skipped`, one warning per file)"""
        if draw is None:
            return None
        fi, level, u = draw
        room = int(self.lengths[fi]) - int(n_samples)
        if room < 0:
            self.skipped += 1
            if fi not in self._warned:
                self._warned.add(fi)
                logging.warning('NoiseInjection: %s (%d samples) is shorter than an utterance of %d samples: such utterances stay clean',
                                self.paths[fi], int(self.lengths[fi]), int(n_samples))
            return None
        start = min(int(np.floor(u * room)), room)
        return int(self.offsets[fi]) + start, level

    def plan(self, draws, lengths):
        """K draws and the K utterance lengths -> (noise_off int64 (K), level float32 (K)); noise_off = -1 for a clean utterance"""
        noise_off, level = np.full(len(draws), -1, dtype=np.int64), np.zeros(len(draws), dtype=np.float32)
        for k, (d, n) in enumerate(zip(draws, lengths)):
            placed = self.place(d, n)
            if placed is not None:
                noise_off[k], level[k] = placed
        return noise_off, level

    def inject_noise(self, data):
        """utils/data_loader.py:383-386, draws from the global np.random like the reference"""
        noise_path = np.random.choice(self.paths)
        noise_level = np.random.uniform(*self.noise_levels)
        return self.inject_noise_sample(data, noise_path, noise_level)

    def inject_noise_sample(self, data, noise_path, noise_level, u=None):
        """utils/data_loader.py:388-399 on the device: mtl_wave_mix_coef and one mtl_wave_mix call with K = 1 -> the mixed waveform as
        float32 numpy (`data` itself is left alone).  u=None draws np.random.rand() as the reference does."""
        from . import _lib
        if u is None:
            u = np.random.rand()
        y = np.ascontiguousarray(data.detach().cpu() if torch.is_tensor(data) else data, dtype=np.float32).reshape(-1)
        placed = self.place((self.paths.index(str(noise_path)), float(noise_level), float(u)), y.shape[0])
        if placed is None or y.shape[0] == 0:
            return y.copy()
        lib, bank = _lib.lib(), self.device_bank()
        dev = bank.device
        wav = torch.from_numpy(y).to(dev)
        off = torch.tensor([0, y.shape[0]], dtype=torch.int64, device=dev)
        noff = torch.tensor([placed[0]], dtype=torch.int64, device=dev)
        lvl = torch.tensor([placed[1]], dtype=torch.float32, device=dev)
        coef, out = torch.empty(1, device=dev), torch.empty_like(wav)
        ws_bytes = lib.mtl_wave_mix_coef_workspace(1)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.mtl_wave_mix_coef(st, wav.data_ptr(), off.data_ptr(), 1, bank.data_ptr(), self.bank_len, noff.data_ptr(),
                                         lvl.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws_bytes), 'mtl_wave_mix_coef')
        _lib.check(lib.mtl_wave_mix(st, wav.data_ptr(), off.data_ptr(), 1, bank.data_ptr(), self.bank_len, noff.data_ptr(),
                                    coef.data_ptr(), out.data_ptr()), 'mtl_wave_mix')
        return out.cpu().numpy()
