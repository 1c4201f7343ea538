"""bench.py's N-rank path on the one-GPU box: `python bench.py --gpus 2` starts
two ranks itself (torch.distributed.run child; BGX_DIST_BACKEND=gloo so both
share GPU 0) and rank 0 prints the line.  Checks n_gpus, the value as the sum
over ranks over the max-over-ranks time, the PPO iteration over both ranks with
identical weights after the all-reduced update, and the host_mirror leg (--full).
RCCL itself (backend nccl, one rank per GPU) runs only on a multi-GPU node.
A plain one-GPU run: the headline alone, and --dump-outputs' files."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step(tmp_path):
    """A plain run (no --full) times the headline alone and, with --dump-outputs, writes the
    last timed step's rollout row and the lane records after it as float32 .npy files."""
    import numpy as np
    B, K = 8192, 6
    out = tmp_path / "dump"
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "2",
           "--burn-in", "40", "--batch", str(B), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == K and line["config"]["hip_graph"]["replays"] == K // 2
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(B * K / (line["ms_per_step"] * K * 1e-3), rel=1e-9)
    for leg in ("roofline", "host_mirror", "two_ply", "two_ply_h128", "one_ply_selfplay", "ppo_iteration", "cpu_baseline"):
        assert leg not in line, leg
    shapes = {"records": (B, 64), "action": (B,), "log_prob": (B,), "value": (B,), "reward": (B,), "done": (B,),
              "next_records": (B, 64)}
    assert sorted(p.name for p in out.iterdir()) == sorted(n + ".npy" for n in shapes)
    a = {n: np.load(out / (n + ".npy")) for n in shapes}
    for n, s in shapes.items():
        assert a[n].dtype == np.float32 and a[n].shape == s, n
    nm = a["records"][:, 60] + 256 * a["records"][:, 61]          # legal moves of the stored positions
    # a lane without a legal move samples from all 500 actions (bg_mlp.hip)
    assert np.all((a["action"] >= 0) & (a["action"] < np.where(nm > 0, np.minimum(nm, 500), 500)))
    assert np.all(a["log_prob"] <= 1e-6) and np.all(np.isfinite(a["value"]))
    assert set(np.unique(a["done"])) <= {0.0, 1.0} and np.all(np.abs(a["records"][:, 52]) <= 1)
    assert np.any(a["records"] != a["next_records"])               # the step moved the lanes on


def test_bench_two_ranks_gloo():
    env = dict(os.environ, BGX_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--burn-in", "5", "--batch", "8192", "--two-ply-batches", "1", "--c2-steps", "4", "--horizon", "4",
           "--mirror-steps", "4", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]           # rank 0 only
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["dist_backend"] == "gloo"
    pr = line["per_rank"]
    assert [p["rank"] for p in pr] == [0, 1]
    assert all(p["env_steps"] == 8192 * 5 for p in pr)
    el = max(p["seconds"] for p in pr)
    assert line["value"] == pytest.approx(sum(p["env_steps"] for p in pr) / el, rel=1e-9)
    assert line["config"]["global_batch"] == 2 * 8192
    ppo = line["ppo_iteration"]
    assert ppo["ranks"] == 2 and ppo["weights_identical_across_ranks"] is True
    assert all(v == v for v in ppo["losses_last"].values())
    assert line["host_mirror"]["env_steps_per_s"] > 0
    assert line["two_ply"]["root_decisions_per_s"] > 0 and line["one_ply_selfplay"]["env_steps_per_s"] > 0
