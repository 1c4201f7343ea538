"""Warm ms/step of Rollout.run_lanes in its ten modes, on two built trees alternately:

    python tools/rollout_modes_time.py PARENT_TREE [--runs 5] [--steps 100] [--out FILE.jsonl]

65,536 lanes, RandomPlayer, a seeded 40-unit value head, half the lanes from the opening and
half with both sides home (3..8 checkers, some inside the tables), so many games per lane that no
lane retires.  Every measurement is a child process of its own (one at a time) that imports the
tree's own package and library: one untimed run_lanes of --steps steps, then a timed one, wall
clock around it with the device idle before and after.  Prints and appends one JSON line per
measurement, then per mode the medians and min-max spreads of both trees.

    python tools/rollout_modes_time.py --child TREE MODE STEPS      (what the driver starts)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "mlp-ppo-2ply-p3_amd"
MODES = ("plain", "luck", "bearoff", "bearoff1", "cube", "cube_bearoff", "truncate", "truncate_luck", "cube_truncate",
         "cube_bearoff_truncate")
B = 65536


def child(tree, mode, steps):
    sys.path.insert(0, os.path.join(tree, PKG))
    import numpy as np
    import torch
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffDB, CubefulBearoffDB, OneSidedBearoffDB
    from bgx.cube import CubeRule, CubeTruncation
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    from bgx.truncate import Truncation
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    rule = dict(cube=CubeRule(vh, jacoby=True, double_at=0.13, pass_at=0.19, cap=4))
    kw = {"plain": {}, "luck": dict(luck=vh), "bearoff": lambda: dict(bearoff=BearoffDB(6)),
          "bearoff1": lambda: dict(bearoff=OneSidedBearoffDB(15)), "cube": rule,
          "cube_bearoff": lambda: dict(rule, cube_bearoff=CubefulBearoffDB(BearoffDB(6))),
          "truncate": dict(truncate=Truncation(vh, 8)), "truncate_luck": dict(truncate=Truncation(vh, 8), luck=vh),
          "cube_truncate": dict(rule, cube_truncate=CubeTruncation(vh, 8)),
          "cube_bearoff_truncate": lambda: dict(rule, cube_bearoff=CubefulBearoffDB(BearoffDB(6)),
                                                cube_truncate=CubeTruncation(vh, 8))}[mode]
    kw = kw() if callable(kw) else kw
    rng = np.random.RandomState(3)
    starts = np.zeros((B, 64), np.uint8)
    starts[:] = opening_record().numpy()
    for i in range(1, B, 2):                                # both sides home, distance d on points 24 - d / d - 1
        c = [np.bincount(rng.randint(0, 6, rng.randint(3, 9)), minlength=6) for _ in range(2)]
        starts[i] = 0
        starts[i, 23:17:-1], starts[i, 24:30] = c[0], c[1]
        starts[i, 50], starts[i, 51], starts[i, 52] = 15 - c[0].sum(), 15 - c[1].sum(), rng.randint(2)
    starts, group = torch.from_numpy(starts), torch.arange(B, dtype=torch.int32) // (B // 64)    # neighbours share a group
    ro = Rollout(B, seed=1)
    ms = []
    for _ in range(2):                                      # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ro.run_lanes(RandomPlayer(2), starts, group, 64, 1 << 20, max_steps=steps, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    assert ro.eng.error() == 0
    print(json.dumps(dict(mode=mode, steps=steps, ms_per_step=ms[1],
                          first_pass_ms_per_step=ms[0], games=int(sum(int(t[:, 0].sum()) for t in (out[0],) + out[3:])))))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trees = {"parent": os.path.realpath(a.parent), "new": ROOT}
    if trees["parent"] == os.path.realpath(ROOT):
        raise SystemExit("give the parent commit's built tree")
    got = {}
    for mode in a.modes.split(","):
        for run in range(a.runs):
            for name in (("parent", "new") if run % 2 == 0 else ("new", "parent")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", trees[name], mode, str(a.steps)],
                                   capture_output=True, text=True, timeout=300)
                if p.returncode != 0:                       # stop: nothing more runs on the device after a failure
                    raise SystemExit(f"{name} {mode}: exit status {p.returncode}\n{p.stderr[-2000:]}")
                line = dict(json.loads(p.stdout.strip().splitlines()[-1]), build=name, run=run)
                got.setdefault((mode, name), []).append(line["ms_per_step"])
                print(json.dumps(line), flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
    for mode in a.modes.split(","):
        p, n = got[(mode, "parent")], got[(mode, "new")]
        inside = statistics.median(n) <= max(p)
        print(f"{mode:14s} parent median {statistics.median(p):.4f} [{min(p):.4f}, {max(p):.4f}]  "
              f"new median {statistics.median(n):.4f} [{min(n):.4f}, {max(n):.4f}] ms/step  "
              f"{'ok' if inside else 'SLOWER than the parent spread'}", flush=True)


if __name__ == "__main__":
    main()
