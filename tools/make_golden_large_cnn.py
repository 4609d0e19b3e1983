"""tests/golden/LC0.npz: the F0 fixture of oracle/make_golden.py (enc1 / dec1, d 128, V 64, B 2, T 64, L 8, 3 tasks, one --copy-grad
meta-step) recorded on a model the REAL reference builds with --feat_extractor large_cnn (models/asr/transformer.py:60-72,
utils/functions.py:324-327).  Everything but the feature extractor is make_golden.run_fixture: the reference is imported through
its bootstrap_reference(), never copied; only the .npz is committed.

    python tools/make_golden_large_cnn.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG      # noqa: E402


def main():
    torch = MG.bootstrap_reference()
    import utils.functions as ref_functions          # the reference's
    ref_init = ref_functions.init_transformer_model

    def init_large_cnn(args, vocab, **kw):
        """run_fixture writes feat_extractor='vgg_cnn' into the arguments it builds: the one field this fixture changes"""
        args.feat_extractor = 'large_cnn'
        return ref_init(args, vocab, **kw)
    ref_functions.init_transformer_model = init_large_cnn
    MG.run_fixture('LC0', dict(MG.FIXTURES['F0'], iters=1), torch)


if __name__ == '__main__':
    main()
