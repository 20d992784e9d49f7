"""bench.py on the device: a plain run's result line and `--dump-outputs`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARDS, STEPS, WARMUP = 4500, 7, 3        # more envs than one dump holds (bench.DUMP_MAX_ENVS), 3 uneven groups


def _bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--boards", str(BOARDS), "--steps", str(STEPS),
           "--warmup", str(WARMUP)] + extra
    return subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _line(p):
    out, err = p.communicate(timeout=300)
    assert p.returncode == 0, err[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("api", ["raw", "vector"])
def test_dump_outputs_repeatable(tmp_path, api):
    """Two plain runs with the same arguments write the same outputs of the
    last timed step: float32 arrays, one row per sampled env, the same envs
    both times; the line reports the steps asked for and no CPU baseline."""
    import bench
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    procs = [_bench(["--api", api, "--dump-outputs", d]) for d in dirs]
    for line in [_line(p) for p in procs]:
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "env-steps/s"
        assert line["higher_is_better"] is True and line["dtype"] == "int8"
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 / BOARDS - 1) < 1e-2        # both rounded in the line
        assert line["cpu_baseline"] is None
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"env_index.npy", "obs_board.npy", "obs_num_moves_left.npy", "reward.npy", "info_action_mask.npy"} <= set(names)
    n = min(BOARDS, bench.DUMP_MAX_ENVS)
    total = 0
    for name in names:
        a, b = (np.load(os.path.join(d, name)) for d in dirs)
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == n, name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    idx = np.load(os.path.join(dirs[0], "env_index.npy"))
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < BOARDS
    board = np.load(os.path.join(dirs[0], "obs_board.npy"))
    assert board.shape == (n, 2, 10, 10)
    assert board[:, 0].min() >= 1 and board[:, 0].max() <= 4        # c2: 4 colours, no empty cell after a step
    left = np.load(os.path.join(dirs[0], "obs_num_moves_left.npy"))
    assert left.min() >= 0 and left.max() <= 30
    if api == "raw":
        assert len(np.unique(left)) == 3                            # 3 episode-phase blocks, 10 steps apart
    mask = np.load(os.path.join(dirs[0], "info_action_mask.npy"))
    assert mask.shape == (n, 180) and set(np.unique(mask)) <= {0.0, 1.0} and mask.any()
