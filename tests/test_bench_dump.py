"""bench.py --dump-outputs (CPU): the files dump_outputs() writes for the last timed step -- loss + parameter gradients, float32, a large gradient as a
fixed seeded sample, never more than the byte limit -- and the argument checks of --steps / --dump-outputs / --full."""
import importlib.util
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('_alm_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _params():
    g = torch.Generator().manual_seed(7)
    small = torch.nn.Parameter(torch.randn(3, 4, generator=g))
    big = torch.nn.Parameter(torch.randn(50, 40, generator=g))
    unused = torch.nn.Parameter(torch.randn(5, generator=g))
    small.grad = torch.randn(3, 4, generator=g)
    big.grad = torch.randn(40, 50, generator=g).t()              # a non-contiguous gradient (a view into another buffer)
    return [('head.small', small), ('layers.0.big', big), ('unused', unused)]


def test_dump_writes_loss_and_gradients_float32_with_a_fixed_sample(tmp_path):
    bench = _bench()
    named = _params()
    info = bench.dump_outputs(str(tmp_path / 'a'), torch.tensor(2.5, dtype=torch.float64), named, sample=256)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['grad.head.small.npy', 'grad.layers.0.big.npy', 'loss.npy']
    assert info['files'] == 3 and info['bytes'] == 4 * (1 + 12 + 256)
    loss = np.load(tmp_path / 'a' / 'loss.npy')
    assert loss.dtype == np.float32 and loss.shape == () and float(loss) == 2.5
    small = np.load(tmp_path / 'a' / 'grad.head.small.npy')
    assert small.dtype == np.float32 and np.array_equal(small, named[0][1].grad.reshape(-1).numpy())
    big = np.load(tmp_path / 'a' / 'grad.layers.0.big.npy')
    idx = torch.randint(2000, (256,), generator=torch.Generator().manual_seed(zlib.crc32(b'layers.0.big'))).sort().values
    assert big.dtype == np.float32 and np.array_equal(big, named[1][1].grad.reshape(-1)[idx].numpy())
    # the same positions in another run
    bench.dump_outputs(str(tmp_path / 'b'), torch.tensor(2.5), _params(), sample=256)
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))


def test_dump_refuses_more_than_the_byte_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 4 * 12)
    with pytest.raises(RuntimeError, match='limit'):
        bench.dump_outputs(str(tmp_path / 'a'), torch.tensor(1.0), _params(), sample=256)
    assert not os.path.exists(tmp_path / 'a')


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['ALM_BENCH_LAUNCH_CHECK'] = '1'
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_steps_must_be_positive_and_dump_outputs_is_accepted(tmp_path):
    r = _run(['--steps', '0'])
    assert r.returncode == 2 and '--steps' in r.stderr
    r = _run(['--steps', '3', '--warmup', '0', '--dump-outputs', str(tmp_path / 'out')])
    assert r.returncode == 0, r.stderr[-2000:]
    assert '"steps": 3' in r.stdout


def test_full_is_off_by_default():
    """a plain run measures the headline figure alone; the host-issue, roofline, optimiser and CPU-baseline legs run with --full"""
    ap = _bench().arg_parser()
    plain = ap.parse_args(['--gpus', '1', '--steps', '4', '--warmup', '2'])
    assert not plain.full
    full = ap.parse_args(['--full', '--no-cpu-baseline'])
    assert full.full and full.no_cpu_baseline and not full.no_optimizer_leg
    r = _run(['--steps', '3', '--warmup', '0', '--full'])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run(['--steps', '3', '--warmup', '0', '--no-cpu-baseline'])        # accepted, but said to do nothing without --full
    assert r.returncode == 0 and 'trim a --full run' in r.stderr, r.stderr[-2000:]


def test_every_process_builds_the_same_initial_weights():
    """the inputs of the timed step are the same in every run: two processes build the benchmark model (on the CPU) with identical weights,
    the hyper-connections' randomly drawn initial residual streams included"""
    code = ("import hashlib, sys, torch\nsys.path.insert(0, %r)\nimport bench\n"
            "W = bench.build('coarse1024', torch.device('cpu'), 0, None)\nh = hashlib.sha256()\n"
            "for k, v in sorted(W['model'].state_dict().items()):\n    h.update(k.encode() + v.detach().float().contiguous().numpy().tobytes())\n"
            "for k, v in sorted(W['inputs'].items()):\n    h.update(k.encode() + v.numpy().tobytes())\nprint('digest', h.hexdigest())\n") % ROOT
    out = []
    for _ in range(2):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append([l for l in r.stdout.splitlines() if l.startswith('digest')])
    assert len(out[0]) == 1 and out[0] == out[1]
