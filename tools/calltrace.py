"""Record the library calls of one forward_device + backward per schedule and convolution mode -> tests/golden/calltrace.json.gz

    python tools/calltrace.py [--out tests/golden/calltrace.json.gz]

tests/test_calltrace_gpu.py runs the same cases and compares with the fixture entry for entry: a pass must issue the same calls, in the
same order, with the same arguments as the commit that recorded the fixture.  Re-record the fixture (the command above, on an MI355X)
only with a change that MEANS to alter which calls a pass makes, and say so in that change.

Only PassEngine.prepare_tasks / forward_device / backward and the attributes lib, L, conv_mode, conv_x3, conv_h2, in_linear, census and
slice_hook are used, so the tool runs unchanged on older trees.

A call is [name, arg, ...]: integers verbatim, floats as their repr, pointers as 0 (null), ['theta' | 'grad' | 'x', offset in floats]
inside one of the pass's three caller-owned tensors, or 'p<n>' with n the order of the address's first appearance in the case's trace.
An equal trace therefore shows equal calls and equal aliasing, NOT right addresses: a wrong offset into an arena buffer is one more
distinct address with the ordinal the right one would have had; the bit-exact suites (tests/test_batched_gpu.py, test_ops_gpu.py) see those.
Calls that a command list cannot hold (size queries: *_workspace, *_bytes, ...) end with ['=', result].  Every case is run twice and the
second run is recorded: the scratch buffer has its final size by then, so equal ordinals mean equal buffers.
"""
import argparse
import gzip
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'calltrace.json.gz')
B, F, T, LABELS = 2, 161, 32, 6
# schedule -> tasks, a theta' stack (sP = L.total), one input batch shared by all tasks (sX = 0), the tasks' own frame counts
SCHEDULES = {'a': (1, False, False, None), 'b': (1, False, False, [21]), 'c': (3, False, False, None),
             'd': (3, True, True, [21, 21, 21]), 'e': (3, False, False, [32, 21, 14])}
CASES = [('%s-%s' % (mode, s), mode, s, None) for mode in ('h2', 'x3', 'f32') for s in 'abcde'] + [
    ('h2-c-census', 'h2', 'c', 'census'), ('h2-c-slice_hook', 'h2', 'c', 'slice_hook'), ('h2-a-in_linear_f32', 'h2', 'a', 'in_linear')]


class Tracer:
    """stands in for eng.lib: every call is executed and appended to `calls` in its normalised form"""

    def __init__(self, handle, regions):
        from mtl_amd import _lib
        self._h, self._lib, self._regions, self._ordinal, self._cache, self.calls = handle, _lib, regions, {}, {}, []

    def _pointer(self, v):
        v = int(v or 0)
        if not v:
            return 0
        for tag, lo, hi in self._regions:
            if lo <= v < hi:
                off = (v - lo) / 4
                return [tag, int(off) if off == int(off) else off]
        return 'p%d' % self._ordinal.setdefault(v, len(self._ordinal) + 1)

    def __getattr__(self, name):
        fn = self._cache.get(name)
        if fn is None:
            real = getattr(self._h, name)
            if name not in self._lib.SIGNATURES:
                return real
            kinds, query = self._lib._kinds(name), self._h.mtl_cmdlist_opcode(name.encode()) < 0

            def fn(*args):
                rc = real(*args)
                norm = {'p': self._pointer, 'd': lambda v: repr(float(v)), 'l': int}
                self.calls.append([name] + [norm[k](v) for k, v in zip(kinds, args)] + ([['=', int(rc)]] if query else []))
                return rc
            self._cache[name] = fn
        return fn


def run_case(eng, theta0, mode, schedule, extra):
    """one case on a PassEngine -> its list of calls"""
    import mtl_amd
    nt, stack, shared, frames = SCHEDULES[schedule]
    total, V = eng.L.total, eng.hp.V
    batches = [mtl_amd.synth_batch(300 + m, B, T, LABELS, V) for m in range(nt)]
    x = (batches[0][0] if shared else torch.cat([b[0] for b in batches])).cuda().contiguous()
    theta = theta0.repeat(nt).contiguous() if stack else theta0
    grad = torch.zeros(nt * total, dtype=torch.float32, device=theta0.device)
    eng.conv_mode, eng.conv_x3, eng.conv_h2 = mode, mode != 'f32', mode == 'h2'
    eng.in_linear = 'f32' if extra == 'in_linear' else 'h2'
    eng.census = torch.zeros(nt, mtl_amd.engine.CENSUS_SLOTS, 4, dtype=torch.int64, device=theta0.device) if extra == 'census' else None
    eng.slice_hook = (lambda tag: None) if extra == 'slice_hook' else None
    regions = [(tag, t.data_ptr(), t.data_ptr() + 4 * t.numel()) for tag, t in (('theta', theta), ('grad', grad), ('x', x))]
    real = eng.lib
    try:
        meta = eng.prepare_tasks([(b[1], b[2]) for b in batches], B, T, slot=0, frames=frames)
        for rep in range(2):
            tracer = Tracer(real, regions)
            eng.lib = tracer
            try:
                eng.forward_device(theta, x, meta, sP=total if stack else 0)
                eng.backward(grad, 1.0, sG=total if nt > 1 else 0)
            finally:
                eng.lib = real
        torch.cuda.synchronize()
    finally:
        eng.in_linear, eng.census, eng.slice_hook = 'h2', None, None
    return tracer.calls


def traces(eng, theta0):
    """{case: calls} of all CASES, in their order, on one engine (run them on a fresh engine: the side stream's event ring goes round)"""
    saved = eng.conv_mode, eng.conv_x3, eng.conv_h2
    try:
        return json.loads(json.dumps({name: run_case(eng, theta0, mode, s, extra) for name, mode, s, extra in CASES}))
    finally:
        eng.conv_mode, eng.conv_x3, eng.conv_h2 = saved


def fixture_model():
    """the F0 fixture's model on the device -> (engine, flat theta)"""
    from tests import golden_util as gu
    from tests.test_parity_gpu import make
    _z, cfg, spec = gu.load('F0')
    model = make(cfg, spec)[3].cuda()
    return model._need_engine(), model._theta


def load(path=FIXTURE):
    with gzip.open(path, 'rt') as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args()
    out = traces(*fixture_model())
    with open(a.out, 'wb') as raw, gzip.GzipFile(fileobj=raw, mode='wb', mtime=0, filename='') as f:
        f.write(json.dumps(out, separators=(',', ':')).encode())
    print('%s: %d cases, %d calls' % (a.out, len(out), sum(len(v) for v in out.values())))


if __name__ == '__main__':
    main()
