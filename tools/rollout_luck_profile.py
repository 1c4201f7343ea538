#!/usr/bin/env python
"""Measure luck-adjusted rollouts (DESIGN.md §10 "Luck adjustment") on one MI355X and write
profiles/rollout_luck/summary.json.  Every measurement is a child process of its own and the
children run one after another: never more than one process with the GPU open.

    python tools/rollout_luck_profile.py [--updates 200] [--parent DIR] [--out FILE]

1. A checkpoint: a short `python -m bgx.train --returns selfplay` run (the command and the
   updates are recorded).  --net FILE uses an existing one instead.
2. Per player (policy, 1ply), 65,536 lanes from the opening with drawn first rolls, two games
   per lane, once without and once with luck: games/s of the warm loop (Rollout.run between
   device synchronisations, after an untimed run of the same shape), the raw and the adjusted
   standard error, the variance ratio, the fitted scale c, and the wall time either way to
   reach the adjusted run's standard error (plain: games x var_res / var_y at the plain rate).
3. The regression check (--parent DIR: a built checkout of the parent commit): the 2-ply legs
   of `bench.py --full` (H = 40 and H = 128 root decisions/s), this tree and the parent
   alternating, two runs each.
A part that is skipped (--skip-rollouts, no --parent) keeps what the output file already holds.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")
BATCH, TRIALS = 65536, 131072
BENCH = ["bench.py", "--full", "--steps", "20", "--warmup", "5", "--horizon", "0", "--c2-steps", "0", "--mirror-steps",
         "0", "--no-cpu-baseline"]


def child(cmd, cwd=ROOT, pkg=PKG, timeout=900):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)} (in {cwd})", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def worker(net_path: str, kind: str, luck: bool):
    """One timed rollout in this process; prints one JSON line."""
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import load_net, make_player
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    net = load_net(net_path, dev)
    player = make_player(kind, net, seed=3)
    vh = ValueHead(net) if luck else None
    ro = Rollout(BATCH, seed=1, max_moves=min(net.action_head.out_features, 500), device=dev)
    pos = opening_record()[None]
    ro.run(player, pos, TRIALS, first_roll="random", luck=vh)              # untimed: allocations, first launches
    steps0 = ro.steps
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r, = ro.run(player, pos, TRIALS, first_roll="random", luck=vh)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    keys = ("games", "unfinished", "plies_per_game", "equity", "equity_stderr") + \
        (("equity_luck", "equity_luck_stderr", "variance_ratio", "luck_scale", "luck_mean") if luck else ())
    print(json.dumps(dict(player=kind, luck=luck, seconds=dt, steps=ro.steps - steps0, games_per_s=r["games"] / dt,
                          ms_per_step=1e3 * dt / max(ro.steps - steps0, 1), **{k: r[k] for k in keys})), flush=True)


def rollouts(net_path: str) -> dict:
    out = {}
    for kind in ("policy", "1ply"):
        plain, lucky = (json.loads(child([os.path.abspath(__file__), "--worker", kind, str(int(luck)), "--net",
                                          net_path])[-1]) for luck in (False, True))
        ratio = lucky["variance_ratio"]
        out[kind] = dict(
            without_luck=plain, with_luck=lucky,
            games_per_s=dict(without=plain["games_per_s"], with_luck=lucky["games_per_s"]),
            stderr=dict(raw=lucky["equity_stderr"], adjusted=lucky["equity_luck_stderr"]),
            variance_ratio=ratio, fitted_c=lucky["luck_scale"],
            # the adjusted run's stderr, reached by plain games: 1 / ratio times as many
            seconds_to_equal_stderr=dict(target_stderr=lucky["equity_luck_stderr"], with_luck=lucky["seconds"],
                                         without=(lucky["games"] / ratio / plain["games_per_s"]) if ratio > 0 else None))
    return out


def bench_lines(parent: str) -> dict:
    def one(tree):
        line = json.loads(child(BENCH, cwd=tree, pkg=os.path.join(tree, "mlp-ppo-2ply-p3_amd"), timeout=1200)[-1])
        return dict(h40=line["two_ply"]["root_decisions_per_s"], h128=line["two_ply_h128"]["root_decisions_per_s"])
    runs = {"this": [], "parent": []}
    for _ in range(2):
        runs["parent"].append(one(parent))
        runs["this"].append(one(ROOT))
    return dict(command="python " + " ".join(BENCH), order="parent, this, parent, this", root_decisions_per_s=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=2, metavar=("PLAYER", "LUCK"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (the 2-ply regression check)")
    ap.add_argument("--skip-rollouts", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_luck", "summary.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.net, args.worker[0], bool(int(args.worker[1])))
    summary = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            summary = json.load(f)
    if not args.skip_rollouts:
        net = args.net
        if net is None:
            os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
            net = os.path.join(ROOT, "models", "rollout_luck_profile.pt")
            cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
                   str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", net]
            t0 = time.perf_counter()
            last = json.loads(child(cmd)[-1])
            summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_luck_profile.pt"]),
                                         updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0,
                                         last_update={k: v for k, v in last.items() if isinstance(v, (int, float))})
        summary["setup"] = dict(lanes=BATCH, games=TRIALS, positions="opening", first_roll="random",
                                luck_scale="fit", timed="a warm Rollout.run, after an untimed run of the same shape")
        summary["players"] = rollouts(net)
    if args.parent:
        summary["two_ply_regression"] = bench_lines(os.path.abspath(args.parent))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
