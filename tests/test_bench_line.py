"""bench.py's stdout contract, checked without a GPU: the LAST stdout line is what the driver parses (round 4's 20 KB line came back
as `parsed: null`), so it must stay small and round-trip through json; and every kernel class must be priced against the roof of the
matrix instructions it actually issues."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_line_is_small_and_parseable():
    bench = load_bench()
    # a complete round-4 output (20 KB: per_class / per_family tables, notes) stands in for `out`
    out = json.load(open(os.path.join(ROOT, 'profiles', 'r4', 'bench.json')))
    assert len(json.dumps(out)) > 15000
    out['host_enqueue_ms'] = dict(mean=4.61, median=4.6, max=9.87)
    out['detail'] = 'gpurun_out/bench_detail.json'
    text = json.dumps(bench.compact_line(out))
    assert len(text) < bench.LINE_LIMIT, len(text)
    line = json.loads(text)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline', 'host_enqueue_ms'):
        assert k in line, k
    assert 'workload' in line['config'] and 'model' not in line['config']
    for k in ('bound', 'kernel', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in line['roofline'], k
    assert abs(line['roofline']['frac'] - line['roofline']['achieved'] / line['roofline']['peak']) < 1e-3
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in line['cpu_baseline'], k
    assert 'per_class' not in line['roofline'] and 'per_family' not in line['roofline']
    assert isinstance(line['with_h2d'], float) and isinstance(line['one_task_per_gpu_ms'], float)
    # this round's complete output (bench_detail.json): the manifest-like leg rides in the line as a bare number
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r5', 'bench_detail.json')))
    text5 = json.dumps(bench.compact_line(full))
    assert len(text5) < bench.LINE_LIMIT and isinstance(json.loads(text5)['ragged_frames'], float)
    assert full['ragged_frames']['schedule'] == 'batched-ragged' and full['ragged_frames']['value'] > 0.9 * full['value']


def test_emit_prints_one_short_line_last(capsys, tmp_path, monkeypatch):
    bench = load_bench()
    monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
    out = json.load(open(os.path.join(ROOT, 'profiles', 'r4', 'bench.json')))
    out['roofline']['selection'] = 'x' * 6000           # a runaway note must not cost the line
    out['config']['schedule'] = 'y' * 5000
    bench.emit(out)
    cap = capsys.readouterr()
    lines = cap.out.strip().splitlines()
    assert len(lines) == 1 and len(lines[0]) < bench.LINE_LIMIT
    assert json.loads(lines[0])['value'] == round(out['value'], 4)
    detail = json.load(open(tmp_path / 'gpurun_out' / 'bench_detail.json'))
    assert 'per_class' in detail['roofline'] and 'per_family' in detail['roofline']
    assert 'bench detail: ' in cap.err


def test_every_class_is_priced_on_the_roof_of_its_instructions():
    bench = load_bench()
    x3, h2, f32 = bench.PEAK_X3_TFLOPS, bench.PEAK_H2_TFLOPS, bench.PEAK_F32_MFMA_TFLOPS
    assert abs(x3 - 419.4) < 0.1 and abs(h2 - 838.9) < 0.1
    # entry points on the bf16-triple instructions (six v_mfma_*_bf16 per fp32-equivalent step): the x3 GEMM engine and attention
    for cls in ('gemm_x3', 'attn_fwd', 'attn_bwd'):
        for conv_mode in ('h2', 'x3', 'f32'):
            assert bench.peak_of(cls, 'flop', conv_mode)[0] == x3, cls
    assert bench.peak_of('gemm_h2', 'flop', 'h2')[0] == h2
    for cls in ('conv2_fwd_pool', 'conv5_fwd', 'conv7_dgrad', 'conv2_wgrad'):
        assert bench.peak_of(cls, 'flop', 'h2')[0] == h2
        assert bench.peak_of(cls, 'flop', 'x3')[0] == x3
        assert bench.peak_of(cls, 'flop', 'f32')[0] == f32
    for cls in ('gemm_small', 'gemm_big', 'lstm_stack_fwd'):
        assert bench.peak_of(cls, 'flop', 'h2')[0] == f32
    for cls in ('layernorm_fwd', 'ce_fwd', 'colsum', 'adam_step', 'conv0_fwd'):
        assert bench.peak_of(cls, 'byte', 'h2') == (bench.PEAK_HBM_GBS, 'GB/s', 'hbm')
    # the classifier hands attention launches to those classes with the x3 kernel symbols
    a = [0] * 22
    a[8], a[10], a[11], a[12], a[13], a[14] = 0, 64, 8, 250, 250, 64
    cls, flops, unit, sym = bench.classify(None, 'mtl_attn_fwd', a, 'h2')
    assert cls == 'attn_fwd' and unit == 'flop' and flops == 2 * 2.0 * 64 * 8 * 250 * 250 * 64
    # the task-batched convolution launches are counted as the tasks x B samples they process
    one = (0, 1, 2, 3, 4, 5, 6, 7, 8, 500, 80, 128, 128)                       # relu_pool_fwd_h2: ..., B, T, F, Cin, Cout
    tb = one[:8] + (8, 500, 80, 128, 128, 8, 1024, 128, 2048, 2048, None, 0)    # ..._tb: ..., B, T, F, Cin, Cout, tasks, strides, widths, wshift
    c1 = bench.classify(None, 'mtl_conv3x3_relu_pool_fwd_h2', one, 'h2')
    c8 = bench.classify(None, 'mtl_conv3x3_relu_pool_fwd_h2_tb', tb, 'h2')
    assert c1[0] == c8[0] == 'conv7_fwd_pool' and c8[1] == 8 * c1[1] and c8[3] == c1[3]
    d1 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 500, 80, 64, 128)
    d8 = d1[:8] + (8, 500, 80, 64, 128, 8, 4096, 2048, 2048, None, 0)
    # the hand-built tuples above have the arity of the REAL prototypes (a prototype that grows must not shift the dimensions silently)
    import ctypes
    sys.path.insert(0, ROOT)
    import mtl_amd
    for nm, args_ in (('mtl_conv3x3_relu_pool_fwd_h2_tb', tb), ('mtl_conv3x3_dgrad_h2_tb', d8)):
        assert len(mtl_amd._lib.SIGNATURES[nm][1]) == len(args_), nm
    import pytest
    with pytest.raises(RuntimeError):
        bench.classify(None, 'mtl_conv3x3_dgrad_h2_tb', d8[:-2], 'h2')
    assert bench.classify(None, 'mtl_conv3x3_dgrad_h2_tb', d8, 'h2')[1] == 8 * bench.classify(None, 'mtl_conv3x3_dgrad_h2', d1, 'h2')[1]
    assert bench.algorithmic_bytes('mtl_conv3x3_dgrad_h2_tb', d8, 'flop', 1.0) == 8 * bench.algorithmic_bytes('mtl_conv3x3_dgrad_h2', d1, 'flop', 1.0)


def test_self_launch_only_when_started_without_a_launcher():
    """`python3 bench.py --gpus N` with N > 1 and no RANK / WORLD_SIZE starts its own N ranks (the driver's N = 1 command is the plain
    form; a SCALE run in the same form must yield a line, not `--gpus N but WORLD_SIZE 1`).  N = 1, or a run under torchrun, is left
    exactly as it is: no re-exec, same process, same line."""
    bench = load_bench()
    argv = ['--gpus', '4', '--steps', '5', '--warmup', '2']
    assert bench.self_launch_command(1, ['--gpus', '1'], {}) is None
    assert bench.self_launch_command(1, [], {'WORLD_SIZE': '1'}) is None
    assert bench.self_launch_command(4, argv, {'RANK': '0', 'WORLD_SIZE': '4', 'LOCAL_RANK': '0'}) is None
    assert bench.self_launch_command(4, argv, {'WORLD_SIZE': '4'}) is None
    cmd = bench.self_launch_command(4, argv, {'HOME': '/root'})
    assert cmd[0] == sys.executable and cmd[1:3] == ['-m', 'torch.distributed.run']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4' and cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert 0 < int(cmd[cmd.index('--master-port') + 1]) < 65536
    script = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[script + 1:] == argv                       # the ranks see the caller's own flags, `--gpus N` included
    # the plain N = 1 invocation does not reach the launcher at all (main() consults self_launch_command before anything else)
    src = open(os.path.join(ROOT, 'bench.py')).read()
    assert src.index('self_launch_command(a.gpus') < src.index('import mtl_amd\n    mdist')


def test_self_launch_starts_the_ranks_for_real(tmp_path):
    """The launcher end to end on CPU: two ranks come up under torch.distributed.run, each sees RANK / WORLD_SIZE = 2, and fails at the
    first thing bench.py needs that this container lacks (a GPU) with the product's own message -- not with `--gpus 2 but WORLD_SIZE 1`."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env['MTL_DIST_BACKEND'] = 'gloo'
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip('CPU-side check of the launcher; the GPU suite runs bench.py --gpus 2 for real')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--no-extras'],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert 'WORLD_SIZE 1' not in r.stderr and 'bench.py needs an MI355X' in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip() == ''


def test_bench_helpers_are_called_with_their_current_signatures():
    """bench.py's LM leg runs on the GPU only; a stale call of classify / peak_of there (round 6: two arguments too many after a switch was
    removed) would only show up as an empty bench line on the GPU box -- checked here on the source"""
    import ast
    import inspect
    bench = load_bench()
    tree = ast.parse(open(os.path.join(ROOT, 'bench.py')).read())
    want = {name: len(inspect.signature(getattr(bench, name)).parameters) for name in ('classify', 'peak_of', 'algorithmic_bytes', 'family_of', 'eval_leg', 'h2_frac')}
    seen = {k: 0 for k in want}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in want:
            n = len(node.args) + len(node.keywords)
            required = sum(p.default is inspect.Parameter.empty for p in inspect.signature(getattr(bench, node.func.id)).parameters.values())
            assert required <= n <= want[node.func.id], (node.func.id, node.lineno, n)
            seen[node.func.id] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_dump_outputs_are_float_arrays_of_a_fixed_sample(tmp_path):
    """--dump-outputs DIR: one DIR/<name>.npy per output, float32 for device tensors and float64 for the read-back scalars; an output
    larger than DUMP_SAMPLE elements is cut to DUMP_SAMPLE of them at the same sorted positions in every run, so two builds compare
    element for element and the files stay below 64 MB in all"""
    import numpy as np
    import torch
    bench = load_bench()
    n = bench.DUMP_SAMPLE * 3 + 7
    theta = torch.arange(n, dtype=torch.float32)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), dict(theta=theta, meta_grad=-theta, small=theta[:10], last_step=[12.5, 3, 40]))
    got = {f[:-4]: np.load(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))}
    assert sorted(got) == ['last_step', 'meta_grad', 'small', 'theta']
    assert got['theta'].dtype == got['meta_grad'].dtype == got['small'].dtype == np.float32 and got['last_step'].dtype == np.float64
    assert got['last_step'].tolist() == [12.5, 3.0, 40.0] and got['small'].tolist() == list(range(10))
    idx = got['theta'].astype(np.int64)                   # theta[i] == i: the values are the sampled positions
    assert idx.size == bench.DUMP_SAMPLE and (np.diff(idx) > 0).all() and idx[-1] < n and (got['meta_grad'] == -got['theta']).all()
    assert all(np.array_equal(np.load(str(tmp_path / 'b' / (f + '.npy'))), v) for f, v in got.items())
    assert sum(os.path.getsize(str(tmp_path / 'a' / (f + '.npy'))) for f in got) < 64 << 20
