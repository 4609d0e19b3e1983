"""Vocabulary, label/manifest loaders and the synthetic task source.

Mirrors: `Vocab` (utils/data.py:1-28), the label-JSON loading of meta_transfer_train.py:151-157, the manifest CSV
contract of utils/data_loader.py:191-195 and the batch layout returned by `SpectrogramDataset.sample`
(utils/data_loader.py:245-321).  Audio decoding / STFT (utils/data_loader.py:65-96) is outside the accelerated path
(SURVEY.md 8(f) f1): datasets here get features from a caller-supplied `feature_fn`, from the device front-end (frontend.py, whose
public names are re-exported here) or synthesize them.
"""
import csv
import json
import unicodedata

import numpy as np
import torch

from .frontend import (FBANK_EPS, RESAMPLE_MAX_RATIO, _RESAMPLE_TAPS, LogFBankFrontEnd, NoiseInjection, SpecAugment, SpectrogramFrontEnd,  # noqa: F401
                       TempoGainAugment, _cut, fbank_frames, fbank_geometry, load_randomly_augmented_audio, mel_filterbank, mel_filterbank_sparse,
                       pack_waveforms, resample, resample_plan, resample_taps, resample_tables, tempo_gain, tempo_gain_tables,
                       wsola_geometry)


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
                 device_batches=False, noise=None, augment=None, resample=False, spec_augment=None):
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
        resample=False (the default) never reads the header rate: every call and every output bit is as without the keyword.

        spec_augment=SpecAugment(...): every utterance's finished, normalised feature plane gets a small time warp, frequency masks and
        time masks on the device (`SpecAugment` for the definition, `BatchFrontEnd.batch(spec=)` for the launch; the reference has no
        such stage).  Per utterance the stream yields tempo, gain, that utterance's noise draws and THEN its spec draws, a fixed number
        of uniforms (`SpecAugment.draw`); a part that `need` leaves out consumes them too.  The plan is made for the FINAL frame counts:
        behind rate conversion, tempo change and the cut to args.src_max_len.  The batched path hands the plan of a part to its one
        `batch` call; the per-utterance path (`__getitem__`, the rows of `sample()` without device_batches) goes through
        `batch([y], max_frames=args.src_max_len, spec=...)`.  Not with a feature_fn (which gets paths).  Validation loaders are built
        without it by the caller, as with `augment`.  spec_augment=None leaves the stream and every call exactly as they are without."""
        _reject_options(feature_fn, device_batches, noise is not None, augment is not None, resample, spec_augment is not None)
        self._spec = spec_augment
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
            fe = self._fe = self._fe_factory()
            feature_fn = lambda path: fe(load_wav_pcm16(path)).cpu()
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
        """per-utterance path: feature_fn(path), or for an utterance whose draw = (augmentation, noise[, spec]) asks for any of them
        `batch([y], augment=..., noise=..., spec=...)[0][0, 0]`, handed back on the host like every feature; an utterance that `place`
        leaves clean (longer than its noise file) and is neither augmented nor spec-augmented takes the clean path"""
        rate = None
        if self._resample:                                       # (a file at the front-end's own rate takes the paths below as it is)
            y, rate = load_wav_pcm16_rate(path)
            rate = None if rate == self._rate else rate
        if rate is None and (draw is None or all(d is None for d in draw)):
            return self.feature_fn(path)
        if not self._resample:
            y = load_wav_pcm16(path)
        kw, _ = self._plan([y.shape[0]], None if rate is None else [rate], None if draw is None else [draw])
        if not kw:
            return self.feature_fn(path)
        if 'spec' in kw:                                         # (the plan was made for the frames behind the cut)
            kw['max_frames'] = self.args.src_max_len
        return self._front_end().batch([y], **kw)[0][0, 0].cpu()

    def _plan(self, lengths, rates, draws):
        """K lengths, their K rates | None, their K draws | None -> (the keywords of `batch` for these utterances, the K final lengths).
        THE chained-length rule, for both paths: the rates change the lengths, the tempo changes them again, and the noise plan is made
        for the result -- a noise segment is as long as the converted, stretched utterance.  `noise` is left out when every utterance
        stays clean (no noise draw, or `place` left it clean: longer than its noise file), so that such a call is the clean one.  The
        spec plan is made last, for the frames of the final lengths cut to args.src_max_len (the front-end says how many those are)."""
        kw = {}
        if rates is not None:
            kw['rates'], lengths = list(rates), resample_plan(lengths, rates, self._rate)[0]
        if draws is not None and self._augment is not None:
            tempo, gain_db, lengths = self._augment.plan([d[0] for d in draws], lengths)
            kw['augment'] = (tempo, gain_db)
        if draws is not None and self._noise is not None:
            noise_off, level = self._noise[0].plan([d[1] for d in draws], lengths)
            if (noise_off >= 0).any():
                kw['noise'] = (self._noise[0], noise_off, level)
        if draws is not None and self._spec is not None:
            fe = self._front_end()
            frames = _cut(fe._frame_counts(np.array(lengths, dtype=np.int64)), self.args.src_max_len)
            kw['spec'] = self._spec.plan([d[2] for d in draws], frames, fe.F)
        return kw, lengths

    def _draws(self, n):
        """the draws of n utterances, in order, from the dataset's stream: per utterance (augmentation draw | None, noise draw | None),
        tempo and gain before that utterance's noise draws (None without an augmentation, an injector and a SpecAugment); with a
        SpecAugment (augmentation draw | None, noise draw | None, spec draws), the spec draws last"""
        if self._noise is None and self._augment is None and self._spec is None:
            return None
        out = []
        for _ in range(n):
            aug = None if self._augment is None else self._augment.draw(self.rng)
            draw = (aug, None if self._noise is None else self._noise[0].draw(self.rng, self._noise[1]))
            out.append(draw if self._spec is None else draw + (self._spec.draw(self.rng),))
        return out

    def _front_end(self):
        if self._fe is None:
            self._fe = self._fe_factory()
        return self._fe

    def _device_part(self, ids, picks, draws=None):
        """one part of a sampled batch through SpectrogramFrontEnd.batch: the 5-tuple of `collate` with `inputs` on the device
        (draws: one augmentation `plan` and one noise `plan` -- on the stretched lengths -- for the part; the noisy form of the call
        unless every utterance stays clean)"""
        rates = None
        if self._resample:
            waves, rates = zip(*[load_wav_pcm16_rate(ids[j][0]) for j in picks])
            waves = list(waves)
        else:
            waves = [load_wav_pcm16(ids[j][0]) for j in picks]
        trans = [parse_transcript(self.vocab, ids[j][1]) for j in picks]
        kw, _ = self._plan([w.shape[0] for w in waves], rates, draws)
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


def _reject_options(feature_fn, device_batches, noise, augment, resample, spec_augment=False):
    """THE option rejections of every dataset here (noise, augment, spec_augment: whether they were asked for).  A feature_fn gets paths, not samples,
    so nothing that works on samples on the device goes with it; tempo and gain exist in the batched path only."""
    if device_batches and feature_fn is not None:
        raise ValueError('device_batches=True featurises with the batched device front-end: it cannot be combined with a feature_fn')
    if noise and feature_fn is not None:
        raise NotImplementedError("noise injection (noise=, audio_conf['noise_dir']) mixes samples on the device: it cannot be combined "
                                  "with a feature_fn (which gets paths)")
    if augment and feature_fn is not None:
        raise NotImplementedError('tempo / gain augmentation (augment=; load_randomly_augmented_audio, utils/data_loader.py:28-38) runs '
                                  'on the device: it cannot be combined with a feature_fn (which gets paths)')
    if augment and not device_batches:
        raise NotImplementedError('tempo / gain augmentation (augment=; load_randomly_augmented_audio, utils/data_loader.py:28-38) '
                                  'exists in the batched device path only: pass device_batches=True')
    if resample and feature_fn is not None:
        raise NotImplementedError('sample rates are converted on the device: resample=True cannot be combined with a feature_fn (which '
                                  'gets paths)')
    if spec_augment and feature_fn is not None:
        raise NotImplementedError('SpecAugment (spec_augment=) warps and masks the feature batch on the device: it cannot be combined with '
                                  'a feature_fn (which gets paths)')


class _WavDataset(ManifestTaskDataset):
    """What SpectrogramDataset and LogFBankDataset share: the reference's constructor arguments, the rejections, the noise injector and
    ONE lazy front-end, `make_front_end()` at the first utterance (constructing the dataset must not need the device), behind both the
    default feature_fn and the batched path (`sample()` of a part: one `batch` call of it).  `self.sample_rate` is the derived class's."""

    def __init__(self, make_front_end, char_lines, vocab, args, audio_conf, manifest_filepath_list, normalize, augment, input_type, is_train,
                 partitions, feature_fn, seed, device_batches, resample, spec_augment=None):
        noise_dir = audio_conf.get('noise_dir')
        _reject_options(feature_fn, device_batches, noise_dir is not None, augment, resample, spec_augment is not None)
        self.noiseInjector, noise = None, None
        if noise_dir is not None:
            self.noiseInjector = NoiseInjection(noise_dir, audio_conf['sample_rate'], audio_conf.get('noise_levels', (0, 0.5)))
            noise = (self.noiseInjector, float(audio_conf.get('noise_prob')))
        if input_type != 'char':
            raise NotImplementedError("only input_type='char' (utils/data_loader.py:%s)" % char_lines)
        self.normalize, self.augment, self.noise_prob = normalize, augment, audio_conf.get('noise_prob')
        made = []

        def front_end():
            if not made:
                made.append(make_front_end())
            return made[0]
        if feature_fn is None:
            def feature_fn(path):
                return front_end()(load_wav_pcm16(path)).cpu()
        super().__init__(vocab, args, manifest_filepath_list, feature_fn=feature_fn, partitions=partitions, seed=seed, is_train=is_train)
        # behind the base constructor, for which the default feature_fn above would be a user's
        self._noise, self._augment, self._spec = noise, TempoGainAugment() if augment else None, spec_augment
        self._resample, self._rate = bool(resample), self.sample_rate
        self.device_batches, self._fe_factory = device_batches, front_end
        self.manifest_filepath_list, self.input_type = manifest_filepath_list, input_type

    def parse_transcript(self, transcript_path):
        return parse_transcript(self.vocab, transcript_path)

    def parse_audio(self, audio_path):
        """utils/data_loader.py:65-96 and :145-155: with augmentation and / or a noise injector, this utterance's draws from the dataset's
        stream and the work on the device"""
        draws = self._draws(1)
        return self._feature(audio_path, None if draws is None else draws[0])


class SpectrogramDataset(_WavDataset):
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
    reference's constructor either, which leaves this to sox; default off, and then the header rate is never read).
    spec_augment=SpecAugment(...): time warp, frequency and time masks on the finished feature batch, see ManifestTaskDataset (the reference
    has no such stage; default None, and then the draw stream and every call are as without the keyword)."""

    def __init__(self, vocab, args, audio_conf, manifest_filepath_list, normalize=False, augment=False, input_type='char',
                 is_train=False, partitions=None, feature_fn=None, seed=None, device_batches=False, resample=False, spec_augment=None):
        self.window_stride, self.window_size = audio_conf['window_stride'], audio_conf['window_size']
        self.sample_rate, self.window = audio_conf['sample_rate'], audio_conf.get('window', 'hamming')
        super().__init__(lambda: SpectrogramFrontEnd(self.sample_rate, self.window_size, self.window_stride,
                                                     self.window if self.window in ('hamming', 'hann', 'blackman', 'bartlett') else 'hamming',
                                                     self.normalize),
                         '342-361', vocab, args, audio_conf, manifest_filepath_list, normalize, augment, input_type, is_train, partitions,
                         feature_fn, seed, device_batches, resample, spec_augment)
        # (the reference leaves part_len at the LAST manifest's partition size, or max_size without partitions: :211-222)
        self.part_len = (max(int(len(self.ids_list[-1]) * partitions[len(self.ids_list) - 1]), 1) if partitions is not None
                         else self.max_size)
        print('max_size:', self.max_size)
        print('input_type:', input_type)


class LogFBankDataset(_WavDataset):
    """utils/data_loader.py:101-168 with the reference's OWN constructor (test.py:199-200):

        LogFBankDataset(vocab, args, audio_conf, manifest_filepath_list=..., normalize=True, augment=False, input_type='char')

    80 log mel filterbank energies per frame from the device front-end (LogFBankFrontEnd at audio_conf['sample_rate']) unless a
    `feature_fn` is given.  Same attributes as the reference object (max_size = longest manifest x manifests, ids_list, input_type,
    manifest_filepath_list, normalize, vocab), the same two console lines, and its __getitem__ (manifests interleaved by index).
    Beyond the reference: `sample()` and the keywords partitions, seed, device_batches, resample, spec_augment and feature_fn of the
    ManifestTaskDataset machinery -- for one seed the index and draw stream is that of SpectrogramDataset -- and audio_conf['noise_dir'] /
    augment=True, which the reference's class accepts and ignores, work as on SpectrogramDataset, with the same rejections."""

    def __init__(self, vocab, args, audio_conf, manifest_filepath_list, normalize=False, augment=False, input_type='char',
                 is_train=False, partitions=None, feature_fn=None, seed=None, device_batches=False, resample=False, spec_augment=None):
        self.sample_rate = audio_conf.get('sample_rate', getattr(args, 'sample_rate', 16000))
        fbank_geometry(self.sample_rate)                             # a rate beyond the 512-point transform is rejected here
        super().__init__(lambda: LogFBankFrontEnd(self.sample_rate, 80, self.normalize), '157-165', vocab, args, audio_conf,
                         manifest_filepath_list, normalize, augment, input_type, is_train, partitions, feature_fn, seed, device_batches, resample,
                         spec_augment)
        self.max_size = max(len(ids) for ids in self.ids_list) * len(self.ids_list)      # :114-122: no 30000 rule in this class
        print('max_size:', self.max_size)
        print('input_type:', input_type)

    def __getitem__(self, index):
        """utils/data_loader.py:133-143: the manifests interleaved by index, whatever is_train says"""
        ids = self.ids_list[index % len(self.ids_list)]
        row = ids[(index // len(self.ids_list)) % len(ids)]
        draws = self._draws(1)
        return self._feature(row[0], None if draws is None else draws[0])[:, :self.args.src_max_len], parse_transcript(self.vocab, row[1])


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
# The wav loaders of the datasets above (the device front-end that the samples go to is frontend.py).  The datasets resolve these two
# names through this module's namespace at every call: a test that patches `data.load_wav_pcm16` is seen by them.
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
