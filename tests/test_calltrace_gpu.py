"""A pass issues the library calls it issued when tests/golden/calltrace.json.gz was recorded -- same calls, same order, same arguments
(tools/calltrace.py: 3 convolution modes x 5 schedules + the census, a slice hook and the fp32 input Linear under h2) -- and a
backward goes by the mode its forward recorded, not by the engine's attributes of its time.

After a change that MEANS to alter the calls of a pass, re-record the fixture on an MI355X with
    python tools/calltrace.py --out tests/golden/calltrace.json.gz
and say in that change which calls moved and why."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def calltrace():
    spec = importlib.util.spec_from_file_location('calltrace', os.path.join(ROOT, 'tools', 'calltrace.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_pass_issues_the_recorded_calls(calltrace):
    want = calltrace.load()
    got = calltrace.traces(*calltrace.fixture_model())
    assert list(got) == [c[0] for c in calltrace.CASES] and sorted(got) == sorted(want) and len(got) == 18
    bad = []
    for case in got:
        g, w = got[case], want[case]
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), None if len(g) == len(w) else min(len(g), len(w)))
        if first is not None:
            bad.append(case)
            print('%s: %d calls, fixture %d; first difference at call %d\n  now:     %s\n  fixture: %s' % (
                case, len(g), len(w), first, g[first] if first < len(g) else '(none)', w[first] if first < len(w) else '(none)'))
    assert not bad, 'call traces differ from tests/golden/calltrace.json.gz (see this module\'s docstring): %s' % bad


def test_backward_keeps_the_mode_of_its_forward(calltrace):
    """an h2 forward, the attributes flipped to x3 (as the trainer's h2 guard and bench.py flip them on live engines), the backward: bit
    for bit the gradient of an h2 pass nobody touched (the wd* weights and the bounds in the arena are the h2 forward's)"""
    import mtl_amd
    eng, theta = calltrace.fixture_model()
    x, lengths, target = mtl_amd.synth_batch(300, calltrace.B, calltrace.T, calltrace.LABELS, eng.hp.V)
    x = x.cuda()
    grads = []
    for flip in (False, True):
        eng.conv_mode, eng.conv_x3, eng.conv_h2 = 'h2', True, True
        meta = eng.prepare_tasks([(lengths, target)], calltrace.B, calltrace.T)
        eng.forward_device(theta, x, meta)
        if flip:
            eng.conv_mode, eng.conv_x3, eng.conv_h2 = 'x3', True, False
        g = torch.zeros_like(theta)
        eng.backward(g, 1.0)
        torch.cuda.synchronize()
        grads.append(g)
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0], grads[1])
