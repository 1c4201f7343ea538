#!/usr/bin/env python
"""Measure luck-adjusted cubeful rollouts on one MI355X and write
profiles/cube_luck/summary.json.  Every group of measurements is a child process of its own and
the children run one after another: never more than one process with the GPU open.

    python tools/rollout_cube_luck_profile.py [--net FILE] [--out FILE] [--players policy,1ply,2ply]
                                              [--baseline-pkg DIR] [--bench-ab FILE]

1. A checkpoint: the recipe of tools/rollout_cube_profile.py, a short
   `python -m bgx.train --returns selfplay` run at H = 128.  --net FILE uses an existing one.
2. Per player (policy, 1ply, 2ply with --top-k 4), 65,536 lanes from the opening with drawn first
   rolls, two games per lane, CubeRule defaults: the `cube=` rollout from the package
   --baseline-pkg names (the parent commit's; default: this tree's, whose cube= path is the same
   code) and `cube=` with `cube_luck=` from this tree at x = 0, 0.68 and 1 (W = L = 1, value scale
   1, the coefficient fitted): games/s and ms per step of a warm Rollout.run (the median of three
   after an untimed run of the same shape), the standard error per game (stderr * sqrt(games)) raw
   and adjusted, variance_ratio, the fitted c, and the wall time this tree needs to reach the
   baseline run's raw standard error: games_needed = (adjusted stderr per game / that stderr)^2 at
   this tree's games/s, beside the baseline's own seconds.
3. --bench-ab FILE: the headline A/B (lines {"build": "parent" | "this", "result": bench.py's
   JSON line}) is summarised into the file as `headline_ab`.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")
BATCH, TRIALS, REPS = 65536, 131072, 3
XS = (0.0, 0.68, 1.0)


def child(cmd, pkg=PKG, timeout=900):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)}", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def timed(ro, player, pos, kw):
    import torch
    ro.run(player, pos, TRIALS, first_roll="random", **kw)            # untimed: allocations, first launches
    times = []
    for _ in range(REPS):
        steps0 = ro.steps
        torch.cuda.synchronize(ro.eng.device)
        t0 = time.perf_counter()
        r, = ro.run(player, pos, TRIALS, first_roll="random", **kw)
        torch.cuda.synchronize(ro.eng.device)
        times.append(time.perf_counter() - t0)
        steps = ro.steps - steps0
    dt = statistics.median(times)
    out = dict(seconds=dt, seconds_min=min(times), seconds_max=max(times), steps=steps, games=r["games"],
               unfinished=r["unfinished"], games_per_s=r["games"] / dt, ms_per_step=1e3 * dt / max(steps, 1),
               stderr_per_game=r["equity_cubeful_stderr"] * r["games"] ** 0.5,
               **{k: r[k] for k in ("equity_cubeful", "equity_cubeful_stderr", "pass_share", "doubles_per_game",
                                    "mean_cube_log2", "plies_per_game")})
    return out, r


def player_worker(net_path: str, kind: str, mode: str, pkg: str):
    """mode "cube": the cubeful rollout (any tree's package); "luck": this tree's cube_luck=
    configurations.  Prints one JSON line per configuration."""
    sys.path.insert(0, pkg)
    import torch
    from bgx.arena import load_net, make_player
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    net = load_net(net_path, dev)
    vh = ValueHead(net)
    pos = opening_record()[None]

    def fresh():
        player = make_player("2ply" if kind == "2ply" else kind, net, seed=3, top_k=4 if kind == "2ply" else None)
        return player, Rollout(BATCH, seed=1, max_moves=min(net.action_head.out_features, 500), device=dev)

    if mode == "cube":
        player, ro = fresh()
        out, _ = timed(ro, player, pos, dict(cube=CubeRule(vh)))
        print(json.dumps(dict(player=kind, cube_luck=None, **out)), flush=True)
        return
    from bgx.cube import CubeLife, CubeLuck
    for x in XS:
        player, ro = fresh()
        out, r = timed(ro, player, pos, dict(cube=CubeRule(vh), cube_luck=CubeLuck(vh, life=CubeLife(x))))
        print(json.dumps(dict(player=kind, cube_luck=True, cube_life=x, luck_scale=r["luck_scale"], luck_mean=r["luck_mean"],
                              variance_ratio=r["variance_ratio"], equity_cubeful_luck=r["equity_cubeful_luck"],
                              equity_cubeful_luck_stderr=r["equity_cubeful_luck_stderr"],
                              stderr_per_game_luck=r["equity_cubeful_luck_stderr"] * r["games"] ** 0.5, **out)), flush=True)
        print(f"  {kind} x={x}: {out['seconds']:.3f} s, variance ratio {r['variance_ratio']:.4f}", file=sys.stderr, flush=True)
        del ro, player


def headline(path):
    runs = {"parent": [], "this": []}
    with open(path) as f:
        for ln in f:
            if ln.strip():
                d = json.loads(ln)
                runs[d["build"]].append(d["result"]["value"] / 1e6)
    out = dict(command="python bench.py --gpus 1 --steps 1000 --warmup 10", unit="M env steps/s",
               file=os.path.relpath(path, ROOT))
    for k, v in runs.items():
        out[k] = dict(runs=v, median=statistics.median(v), min=min(v), max=max(v)) if v else None
    if runs["parent"] and runs["this"]:
        out["this_median_inside_parent_spread"] = min(runs["parent"]) <= statistics.median(runs["this"]) <= max(runs["parent"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=3, metavar=("PLAYER", "MODE", "PKG"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--players", default="policy,1ply,2ply")
    ap.add_argument("--baseline-pkg", default=PKG, help="the package directory whose cube= rollout is the baseline")
    ap.add_argument("--bench-ab", default=None, help="a .jsonl of bench.py lines of both builds to summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube_luck", "summary.json"))
    args = ap.parse_args()
    if args.worker:
        return player_worker(args.net, *args.worker)
    summary = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            summary = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")

    if args.bench_ab:
        summary["headline_ab"] = headline(args.bench_ab)
        save()
        if args.players == "":
            return
    net = args.net
    if net is None:
        os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
        net = os.path.join(ROOT, "models", "rollout_cube_luck_profile.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", net]
        t0 = time.perf_counter()
        child(cmd)
        summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_cube_luck_profile.pt"]),
                                     updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    baseline_is_parent = os.path.abspath(args.baseline_pkg) != PKG
    summary["setup"] = dict(lanes=BATCH, games=TRIALS, positions="opening", first_roll="random", two_ply="--top-k 4",
                            cube_lives=list(XS), win_value=1.0, loss_value=1.0, value_scale=1.0, luck_scale="fit",
                            rule="CubeRule defaults: scale 1, double_at 0.40, pass_at 0.50, too_good_at inf, cap 6, lookahead 1",
                            baseline="the parent commit's package" if baseline_is_parent
                            else "this tree's package (the cube= path is unchanged)",
                            timed="a warm Rollout.run, the median of three after an untimed run of the same shape",
                            stderr_per_game="stderr * sqrt(games)",
                            seconds_to_baseline_stderr="games * (stderr_per_game_luck / stderr_per_game of the baseline)^2 "
                                                       "/ games_per_s of the cube_luck run")
    me = os.path.abspath(__file__)
    summary.setdefault("players", {})
    for kind in [k for k in args.players.split(",") if k]:
        full = json.loads(child([me, "--worker", kind, "cube", os.path.abspath(args.baseline_pkg), "--net", net],
                                pkg=os.path.abspath(args.baseline_pkg))[-1])
        rows = [json.loads(ln) for ln in child([me, "--worker", kind, "luck", PKG, "--net", net]) if ln.startswith("{")]
        for r in rows:
            need = full["games"] * (r["stderr_per_game_luck"] / full["stderr_per_game"]) ** 2
            r["seconds_to_baseline_stderr"] = need / r["games_per_s"]
            r["speedup_to_baseline_stderr"] = full["seconds"] / r["seconds_to_baseline_stderr"]
        summary["players"][kind] = dict(cube=full, cube_luck=rows)
        save()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
