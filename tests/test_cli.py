"""CLI-contract tests: the reference's main.py / export.py / evaluate.py
entry points run end to end as subprocesses (reference main.py:9-17,
export.py:99-130, evaluate.py:245-290), and bench.py's result line and
--dump-outputs. Tiny synthetic configs on CPU."""

import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cli(args, cwd):
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    return subprocess.run(
        [sys.executable] + args, cwd=cwd, env=env,
        capture_output=True, text=True, timeout=900)


TRAIN_FLAGS = [
    '--train-flag', '--synthetic', '--synthetic-size', '4',
    '--gpu-no', '-1', '--batch-size', '2', '--end-epoch', '1',
    '--num-workers', '0', '--imsize', '64',
    '--num-stack', '1', '--hourglass-inch', '16', '--print-interval', '1',
    '--random-seed', '7',
]


def test_main_train_then_eval(tmp_path):
    save = str(tmp_path / 'run')
    r = run_cli([os.path.join(REPO, 'main.py')] + TRAIN_FLAGS +
                ['--save-path', save], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    ckpt = os.path.join(save, 'check_point_1.pth')
    assert os.path.isfile(ckpt), os.listdir(save)
    assert os.path.isfile(os.path.join(save, 'argument.pickle'))
    assert os.path.isfile(os.path.join(save, 'argument.txt'))
    # checkpoint keeps the reference dict format
    d = torch.load(ckpt, map_location='cpu', weights_only=False)
    for k in ('epoch', 'state_dict', 'optimizer', 'scheduler', 'scaler',
              'loss_log'):
        assert k in d, k

    # eval mode restores the architecture flags from argument.pickle
    r2 = run_cli([os.path.join(REPO, 'main.py'),
                  '--synthetic', '--synthetic-size', '2', '--gpu-no', '-1',
                  '--num-workers', '0', '--imsize', '64',
                  '--save-path', save, '--model-load', ckpt],
                 cwd=str(tmp_path))
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert os.path.isfile(os.path.join(save, 'prediction_results.pickle'))
    assert os.path.isdir(os.path.join(save, 'txt')), os.listdir(save)


def test_export_cli(tmp_path):
    save = str(tmp_path)
    r = run_cli([os.path.join(REPO, 'export.py'),
                 '--num-stack', '1', '--hourglass-inch', '16',
                 '--imsize', '64', '--save-path', save, '--gpu-no', '-1'],
                cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.isfile(os.path.join(save, 'jit_traced_model_cpu.pth'))
    m = torch.jit.load(os.path.join(save, 'jit_traced_model_cpu.pth'))
    with torch.no_grad():
        out = m(torch.randn(1, 3, 64, 64))
    assert len(out) == 3


BENCH_FLAGS = [
    '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch-size', '2',
    '--imsize', '64', '--hourglass-inch', '16',
]


def _run_bench(extra, cwd):
    """bench.py on CPU (devices hidden from the child); returns the parsed
    result line."""
    import json
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    env['CUDA_VISIBLE_DEVICES'] = ''
    env['HIP_VISIBLE_DEVICES'] = ''
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, 'bench.py')] + BENCH_FLAGS +
        extra, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_cli_dump_outputs(tmp_path):
    """bench.py contract: one JSON result line whose steps/ms_per_step
    follow --steps, --full accepted, and --dump-outputs writes the last
    timed step's arrays as float32 .npy, identical from run to run."""
    import numpy as np
    res = _run_bench(['--full', '--dump-outputs', str(tmp_path / 'a')],
                     cwd=str(tmp_path))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype',
              'ms_per_step'):
        assert k in res, k
    assert res['steps'] == 3 and res['warmup'] == 1
    assert res['metric'] == 'train imgs/sec' and res['unit'] == 'imgs/sec'
    assert res['ms_per_step'] > 0
    # value = batch * steps / elapsed and ms_per_step = elapsed / steps
    assert res['value'] == pytest.approx(2 * 1e3 / res['ms_per_step'],
                                         rel=1e-2)

    _run_bench(['--dump-outputs', str(tmp_path / 'b')], cwd=str(tmp_path))
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['loss.npy', 'outputs.npy', 'params.npy']
    assert sorted(os.listdir(tmp_path / 'b')) == names
    total = 0
    for n in names:
        a = np.load(tmp_path / 'a' / n)
        b = np.load(tmp_path / 'b' / n)
        assert a.dtype == np.float32
        assert np.isfinite(a).all(), n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / 'a' / 'outputs.npy').shape == (2, 1, 6, 16, 16)
    # nothing but the dump directories is written next to the run
    assert sorted(os.listdir(tmp_path)) == ['a', 'b']


def test_main_train_torchrun_2rank(tmp_path):
    """The exact multi-rank CLI path the 8-GPU run uses: torchrun launches
    main.py --train-flag, one worker per rank (gloo on CPU), bucketed
    all-reduce, rank-0 checkpoint."""
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    env.setdefault('MASTER_ADDR', '127.0.0.1')
    # CPU workers rendezvous over gloo; with a GPU visible the launcher
    # would pick nccl for them, so hide the devices from the children
    env['CUDA_VISIBLE_DEVICES'] = ''
    env['HIP_VISIBLE_DEVICES'] = ''
    r = subprocess.run(
        [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', '29641', 'main.py'] + TRAIN_FLAGS +
        ['--save-path', str(tmp_path) + '/'],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # rank-0 checkpoint with the reference dict format
    ckpt_path = tmp_path / 'check_point_1.pth'
    assert ckpt_path.exists(), r.stdout[-1500:]
    ckpt = torch.load(ckpt_path, map_location='cpu', weights_only=False)
    for k in ('epoch', 'state_dict', 'optimizer', 'scheduler', 'scaler',
              'loss_log'):
        assert k in ckpt, k
