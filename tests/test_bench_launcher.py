"""bench.py's multi-rank entry (the driver's `python bench.py --gpus N` and its torchrun form) without a GPU:
command construction, rendezvous on 127.0.0.1, max-over-ranks agreement, JSON relay, and the refusal of a
WORLD_SIZE that contradicts --gpus."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, 'bench.py')


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_launcher_starts_ranks_as_a_child_job_and_relays_rank0():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--backend', 'gloo', '--dry-run', '--steps', '7', '--warmup', '2'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert 'torch.distributed.run --nnodes=1 --nproc-per-node=2 --master-addr 127.0.0.1' in p.stderr
    d = _json_line(p.stdout)
    assert d['n_gpus'] == 2 and d['rccl_ranks_seen'] == 2 and d['backend'] == 'gloo' and d['dry_run'] is True
    assert d['steps'] == 7 and d['warmup'] == 2
    assert d['max_over_ranks_check'] == 2.0          # rank r contributes 1 + r: the MAX over ranks arrived on rank 0


def test_world_size_that_contradicts_gpus_is_refused():
    env = dict(os.environ, WORLD_SIZE='3', RANK='0')
    p = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--dry-run'], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and 'WORLD_SIZE=3' in (p.stderr + p.stdout)


def test_single_process_dry_run_prints_one_line():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK')}
    p = subprocess.run([sys.executable, BENCH, '--dry-run'], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    assert _json_line(p.stdout)['n_gpus'] == 1


def test_scatter_bytes_depend_on_whether_the_launch_carries_adam():
    sys.path.insert(0, REPO)
    import bench
    N, M, C = 8192, 2097152, 12
    n_grid = 160 ** 3 * 13
    with_adam = bench.algorithmic_bytes('dvgo_brick_accumulate', N, M, M, M, C, n_grid, True)
    dense = bench.algorithmic_bytes('dvgo_brick_accumulate', N, M, M, M, C, n_grid, False)
    assert with_adam - dense == 160 ** 3 * 13 * 4 * 5
    assert dense == M * (8 * 13 * 4 + 13 * 4) + 160 ** 3 * 13 * 4


def test_dumped_outputs_are_float_and_bounded_and_the_grid_sample_is_fixed(tmp_path):
    """--dump-outputs: the MLP parameters in full, the grids at a seeded voxel sample that is the same from run to run
    and is laid out voxel-major, every file float32 / float64, the whole within 64 MB."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    from directvoxgo_amd.dvgo import DirectVoxGO

    def model(world):
        torch.manual_seed(0)
        m = DirectVoxGO([-1] * 3, [1] * 3, num_voxels=world ** 3, num_voxels_base=world ** 3, alpha_init=1e-2,
                        fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=4,
                        rgbnet_direct=True)
        with torch.no_grad():
            m.density.normal_(); m.k0.normal_()
        return m

    for world in (12, 96):                  # all voxels / a sample of them
        m = model(world)
        out = bench.step_outputs(m, torch.tensor(0.25))
        bench.dump_outputs(out, str(tmp_path / str(world)))
        files = {f[:-4]: np.load(str(tmp_path / str(world) / f)) for f in os.listdir(tmp_path / str(world))}
        assert set(files) == set(out) and {'loss', 'density', 'k0', 'grid_sample_index', 'rgbnet.0.weight'} <= set(files)
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert float(files['loss']) == 0.25
        idx = files['grid_sample_index'].astype(np.int64)
        assert len(idx) == min(world ** 3, bench.DUMP_SAMPLE_VOXELS) and np.all(np.diff(idx) > 0)
        x, y, z = np.unravel_index(idx, (world,) * 3)
        np.testing.assert_array_equal(files['density'], m.density.detach().numpy()[0, 0, x, y, z])
        np.testing.assert_array_equal(files['k0'], m.k0.detach().numpy()[0][:, x, y, z].T)
        np.testing.assert_array_equal(files['rgbnet.3.weight'], m.rgbnet[3].weight.detach().numpy())
        np.testing.assert_array_equal(bench.step_outputs(model(world), torch.tensor(0.25))['grid_sample_index'], idx)


@pytest.mark.gpu
def test_bench_runs_the_steps_it_is_given_and_dumps_the_last_one(tmp_path):
    """A small bench run: the JSON line reports the --steps it was given, and --dump-outputs leaves finite arrays of the
    primary workload's last timed step."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '1', '--rays', '1024',
                        '--no-secondary', '--no-cpu-baseline', '--dump-outputs', str(tmp_path / 'out')],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    assert d['steps'] == 3 and d['warmup'] == 1
    assert d['kernels']['dvgo_march_density']['launches'] == 3          # (the per-kernel pass repeats the K steps)
    files = {f[:-4]: np.load(str(tmp_path / 'out' / f)) for f in os.listdir(tmp_path / 'out')}
    assert {'loss', 'density', 'k0', 'grid_sample_index'} <= set(files)
    n = len(files['grid_sample_index'])
    assert files['density'].shape == (n,) and files['k0'].shape == (n, 12)
    assert all(np.isfinite(a).all() for a in files.values()) and float(files['loss']) > 0
