"""MI355X-native meta-transfer training step (drop-in for the `--copy-grad` hot path of audioku/meta-transfer-learning).

Import as `mtl_amd` (see mtl_amd.py at the repository root; the directory name carries a hyphen).
"""
from . import _lib  # noqa: F401
from .data import (Vocab, SyntheticTask, ManifestTaskDataset, SpectrogramDataset, BucketingSampler, AudioDataLoader, LogFBankDataset,  # noqa: F401
                   load_wav_pcm16_rate, load_vocab, load_wav_pcm16, synthetic_vocab,
                   synth_batch, is_chinese_char, is_contain_chinese_word, get_word_segments_per_language)
from .frontend import (SpectrogramFrontEnd, LogFBankFrontEnd, fbank_geometry, fbank_frames, mel_filterbank, mel_filterbank_sparse,  # noqa: F401
                       NoiseInjection, TempoGainAugment, load_randomly_augmented_audio, tempo_gain, tempo_gain_tables, resample, resample_plan,
                       resample_taps, resample_tables, wsola_geometry, pack_waveforms, SpecAugment)
from .functions import (init_transformer_model, save_meta_model, load_meta_model, save_joint_model, load_joint_model,  # noqa: F401
                        post_process, compute_num_params)
from .discriminator import (Discriminator, init_discriminator_model, save_discriminator, load_discriminator,  # noqa: F401
                            calculate_adversarial, calculate_multi_task)
from .metrics import calculate_metrics, calculate_cer, calculate_wer, calculate_cer_en_zh  # noqa: F401
from .model import Transformer, Encoder, Decoder  # noqa: F401
from .trainer import TransientTrainer, JointTrainer, FlatAdam, FlatSGD  # noqa: F401
from . import dist  # noqa: F401
from . import hostenv  # noqa: F401
from . import lm  # noqa: F401
from .lmscore import LM, calculate_lm_score, lm_string  # noqa: F401
from .testset import evaluate_test_set  # noqa: F401
