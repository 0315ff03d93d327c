"""CPU: `python bench.py --gpus N` starts the N ranks itself (child processes, before anything touches a GPU) and relays
ONE JSON line; a failing rank makes the launcher exit non-zero. `--dry-launch` runs the same launch path on gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT, env=e)


@pytest.mark.timeout(900)
def test_gpus_2_spawns_two_ranks_and_emits_one_line():
    r = _bench("--gpus", "2", "--dry-launch")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["collective_ranks"] == 2 and d["dry_launch"] is True


@pytest.mark.timeout(900)
def test_gpus_8_dry_launch_is_one_node_of_eight_ranks():
    """The shape of the driver's scaling run (N = 8 on one node): eight ranks rendezvous on 127.0.0.1, one collective, ONE line."""
    r = _bench("--gpus", "8", "--dry-launch")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["collective_ranks"] == 8


@pytest.mark.timeout(900)
def test_launcher_refuses_more_ranks_than_gpus_and_propagates_failure():
    # no GPU in this container: the non-dry launcher must refuse instead of printing an n_gpus: 1 line
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with fewer than 2 GPUs")
    r = _bench("--gpus", "2", "--steps", "2", "--warmup", "1")
    assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_world_size_mismatch_is_an_error():
    r = _bench("--gpus", "2", "--dry-launch", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    # a torchrun environment is taken as is (no self-launch): the dry path reports what the environment says
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1


def test_dump_outputs_keeps_dtypes_and_the_size_bound(tmp_path):
    """--dump-outputs' writer: float64 stays float64, the rest becomes float32; an array over its share of the 64 MB is replaced by a fixed
    sample of its elements, the same one run after run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(20_000_000, dtype=torch.float32)
    arrs = dict(ret=torch.zeros(5, dtype=torch.int32), w=np.ones(3), big=big, none=None)
    bench.dump_outputs(str(tmp_path / "a"), arrs)
    bench.dump_outputs(str(tmp_path / "b"), arrs)
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"ret.npy", "w.npy", "big.npy"}
    assert got["ret.npy"].dtype == np.float32 and got["w.npy"].dtype == np.float64
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in got) <= 64e6
    s = got["big.npy"]
    assert 0 < s.size < big.numel() and (np.diff(s) >= 0).all() and np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
