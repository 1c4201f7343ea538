#!/usr/bin/env python
"""Measure rollouts with the doubling cube on one MI355X and write
profiles/cube/summary.json.  Every measurement is a child process of its own and the children
run one after another: never more than one process with the GPU open.

    python tools/rollout_cube_profile.py [--updates 200] [--net FILE] [--out FILE]

1. A checkpoint: the recipe of tools/rollout_luck_profile.py, a short
   `python -m bgx.train --returns selfplay` run at H = 128.  --net FILE uses an existing one.
2. Per player (policy, 1ply), 65,536 lanes from the opening with drawn first rolls, two games
   per lane, once without and once with the cube (CubeRule's defaults on the checkpoint's value
   head): games/s and ms per step of the warm loop (Rollout.run between device
   synchronisations, after an untimed run of the same shape), the share of lanes whose side on
   roll may double per step, pass_share and doubles_per_game.
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


def child(cmd, timeout=900):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)}", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def worker(net_path: str, kind: str, with_cube: bool):
    """One timed rollout in this process; prints one JSON line."""
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import load_net, make_player
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    net = load_net(net_path, dev)
    player = make_player(kind, net, seed=3)
    rule = CubeRule(ValueHead(net)) if with_cube else None
    ro = Rollout(BATCH, seed=1, max_moves=min(net.action_head.out_features, 500), device=dev)
    pos = opening_record()[None]
    ro.run(player, pos, TRIALS, first_roll="random", cube=rule)            # untimed: allocations, first launches
    steps0 = ro.steps
    if rule is not None:
        rule.totals.update(calls=0, rows=0, leaves=0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r, = ro.run(player, pos, TRIALS, first_roll="random", cube=rule)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    steps = ro.steps - steps0
    out = dict(player=kind, cube=with_cube, seconds=dt, steps=steps, games=r["games"], unfinished=r["unfinished"],
               games_per_s=r["games"] / dt, ms_per_step=1e3 * dt / max(steps, 1), plies_per_game=r["plies_per_game"])
    if with_cube:
        out.update(dsel_share_per_step=rule.totals["rows"] / (max(steps, 1) * BATCH), equity_rows=rule.totals["rows"],
                   equity_leaves=rule.totals["leaves"],
                   **{k: r[k] for k in ("equity_cubeful", "equity_cubeful_stderr", "pass_share", "doubles_per_game",
                                        "mean_cube_log2")},
                   played_out_equity=r["played_out"]["equity"])
    else:
        out.update(equity=r["equity"], equity_stderr=r["equity_stderr"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=2, metavar=("PLAYER", "CUBE"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube", "summary.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.net, args.worker[0], bool(int(args.worker[1])))
    summary = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            summary = json.load(f)
    net = args.net
    if net is None:
        os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
        net = os.path.join(ROOT, "models", "rollout_cube_profile.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", net]
        t0 = time.perf_counter()
        child(cmd)
        summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_cube_profile.pt"]),
                                     updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=BATCH, games=TRIALS, positions="opening", first_roll="random",
                            rule="CubeRule defaults: scale 1, double_at 0.40, pass_at 0.50, too_good_at inf, cap 6",
                            timed="a warm Rollout.run, after an untimed run of the same shape")
    summary["players"] = {}
    for kind in ("policy", "1ply"):
        plain, cubed = (json.loads(child([os.path.abspath(__file__), "--worker", kind, str(int(c)), "--net", net])[-1])
                        for c in (False, True))
        summary["players"][kind] = dict(
            without_cube=plain, with_cube=cubed,
            games_per_s=dict(without=plain["games_per_s"], with_cube=cubed["games_per_s"]),
            ms_per_step=dict(without=plain["ms_per_step"], with_cube=cubed["ms_per_step"]),
            dsel_share_per_step=cubed["dsel_share_per_step"], pass_share=cubed["pass_share"],
            doubles_per_game=cubed["doubles_per_game"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
