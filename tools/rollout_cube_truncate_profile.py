#!/usr/bin/env python
"""Measure truncated cubeful rollouts on one MI355X and write
profiles/cube_truncate/summary.json.  Every group of measurements is a child process of its own
and the children run one after another: never more than one process with the GPU open.

    python tools/rollout_cube_truncate_profile.py [--net FILE] [--out FILE] [--players policy,1ply,2ply]
                                                  [--baseline-pkg DIR] [--bench-ab FILE]

1. A checkpoint: the recipe of tools/rollout_cube_profile.py, a short
   `python -m bgx.train --returns selfplay` run at H = 128.  --net FILE uses an existing one.
2. Per player (policy, 1ply, 2ply with --top-k 4), 65,536 lanes from the opening with drawn first
   rolls, two games per lane, CubeRule defaults: the full `cube=` rollout -- from the package
   --baseline-pkg names (the parent commit's; default: this tree's, whose cube= path is the same
   code) -- and `cube=` with `cube_truncate=` at 8 plies with the rule and the truncation at
   lookahead 0 and at lookahead 1 (x = 0.68): games/s of a warm Rollout.run (the median of
   three after an untimed run of the same shape), equity_cubeful, its standard error and the
   standard error per game (stderr * sqrt(games)); at lookahead 0 also equity_cubeful for x in
   {0, 0.5, 0.68, 1}.
3. The rule's own error with a perfect net: over all pairs of the K = 6 cubeful table, with
   the table's cubeless 2 W - 1 as the value, the mean and maximum |e_Janowski - e_exact| per
   cube state (cen, own, opp) for the same x (bgx_cube_janowski against the table's planes).
4. --bench-ab FILE: the headline A/B (lines {"build": "parent" | "this", "result": bench.py's
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
BATCH, TRIALS, HORIZON, REPS = 65536, 131072, 8, 3
XS = (0.0, 0.5, 0.68, 1.0)


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
    """mode "cube": the full cubeful rollout (any tree's package); "truncate": this tree's
    cube_truncate= configurations.  Prints one JSON line per configuration."""
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
        print(json.dumps(dict(player=kind, cube_truncate=None, rule_lookahead=1, **out)), flush=True)
        return
    from bgx.cube import CubeLife, CubeTruncation
    for la, x in [(0, x) for x in XS] + [(1, 0.68)]:
        player, ro = fresh()
        kw = dict(cube=CubeRule(vh, lookahead=la),
                  cube_truncate=CubeTruncation(vh, HORIZON, lookahead=la, life=CubeLife(x)))
        out, r = timed(ro, player, pos, kw)
        print(json.dumps(dict(player=kind, cube_truncate=HORIZON, lookahead=la, cube_life=x,
                              truncated_share=r["truncated_share"],
                              truncated_equity_cubeful=r["truncated_equity_cubeful"], **out)), flush=True)
        print(f"  {kind} lookahead={la} x={x}: {out['seconds']:.3f} s", file=sys.stderr, flush=True)
        del ro, player


def rule_worker():
    """|e_Janowski - e_exact| over all K = 6 pairs per cube state and x; prints one JSON line."""
    sys.path.insert(0, PKG)
    import numpy as np
    import torch
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    from bgx.cube import CubeLife, pack, static_cube_decision
    dev = torch.device("cuda", 0)
    cdb = CubefulBearoffDB(BearoffDB(6, device=dev))
    n = cdb.n
    E = cdb.equity()[:, 1:, 1:].reshape(3, -1)                       # without the empty configurations
    value = (2.0 * cdb.db.table()[1:, 1:] - 1.0).reshape(-1).contiguous()
    m = value.numel()
    recs = torch.zeros(m, 64, dtype=torch.uint8, device=dev)         # PLAYER1 on roll; only the mover byte is read
    states = dict(cen=pack(0, 0), own=pack(1, 1), opp=pack(1, 2))
    res = dict(pairs=m, configurations=n - 1, cap=6)
    for x in XS:
        row = {}
        for s, (name, byte) in enumerate(states.items()):
            cube = torch.full((m,), byte, dtype=torch.uint8, device=dev)
            values, _ = static_cube_decision(recs, None, cube=cube, life=CubeLife(x), cap=6, value=value)
            err = (values[:, 2].double() - E[s].double()).abs()
            row[name] = dict(mean=float(err.mean()), max=float(err.max()))
        res[f"x={x:g}"] = row
    print(json.dumps(res), flush=True)


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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", nargs=3, metavar=("PLAYER", "MODE", "PKG"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rule-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--players", default="policy,1ply,2ply")
    ap.add_argument("--baseline-pkg", default=PKG, help="the package directory whose cube= rollout is the baseline")
    ap.add_argument("--bench-ab", default=None, help="a .jsonl of bench.py lines of both builds to summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cube_truncate", "summary.json"))
    args = ap.parse_args()
    if args.worker:
        return player_worker(args.net, *args.worker)
    if args.rule_worker:
        return rule_worker()
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
        net = os.path.join(ROOT, "models", "rollout_cube_truncate_profile.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", net]
        t0 = time.perf_counter()
        child(cmd)
        summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_cube_truncate_profile.pt"]),
                                     updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=BATCH, games=TRIALS, positions="opening", first_roll="random", two_ply="--top-k 4",
                            horizon=HORIZON, cube_lives=list(XS), win_value=1.0, loss_value=1.0,
                            rule="CubeRule defaults: scale 1, double_at 0.40, pass_at 0.50, too_good_at inf, cap 6; "
                                 "lookahead as given (the full rollout: 1)",
                            baseline="the parent commit's package" if os.path.abspath(args.baseline_pkg) != PKG
                            else "this tree's package (the cube= path is unchanged)",
                            timed="a warm Rollout.run, the median of three after an untimed run of the same shape",
                            stderr_per_game="equity_cubeful_stderr * sqrt(games)")
    me = os.path.abspath(__file__)
    summary["rule_error_k6"] = json.loads(child([me, "--rule-worker"])[-1])
    save()
    summary.setdefault("players", {})
    for kind in [k for k in args.players.split(",") if k]:
        full = json.loads(child([me, "--worker", kind, "cube", os.path.abspath(args.baseline_pkg), "--net", net],
                                pkg=os.path.abspath(args.baseline_pkg))[-1])
        rows = [json.loads(ln) for ln in child([me, "--worker", kind, "truncate", PKG, "--net", net]) if ln.startswith("{")]
        summary["players"][kind] = dict(
            cube=full, cube_truncate=rows,
            games_per_s=dict(cube=full["games_per_s"],
                             **{f"cube_truncate_lookahead_{la}": next(r["games_per_s"] for r in rows
                                                                      if r["lookahead"] == la and r["cube_life"] == 0.68)
                                for la in (0, 1)}))
        save()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
