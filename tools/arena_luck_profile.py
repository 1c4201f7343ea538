#!/usr/bin/env python
"""Measure luck-adjusted arena results on one MI355X and write
profiles/arena_luck/summary.json.  Every measurement is a child process of its own and the children
run one after another: never more than one process with the GPU open.

    python tools/arena_luck_profile.py --parent-pkg DIR [--a FILE] [--b FILE] [--rounds 2] [--out FILE]

1. Two nets at H = 128: A from `python -m bgx.train --returns selfplay`, 200 updates (the recipe of
   tools/arena_cube_profile.py; --a uses an existing one), B a fresh net (seeded initial weights).
2. Three match-ups at 65,536 lanes, two games per lane: policy against policy, 1-ply against
   1-ply, 2-ply top-k 4 against 2-ply top-k 4.  "Without" is the parent commit's package
   (--parent-pkg: a directory that holds its built bgx/), "with" this tree's with luck= on A's
   value head.  The two alternate, parent first, --rounds times; each child plays one untimed match
   and one timed one, and the case's time is the median of its timed matches.
3. Per match-up: games/s and ms per step of both, the raw and the adjusted standard error per game
   (stderr * sqrt(games)), variance_ratio, the fitted c, and the wall time in which the adjusted
   run reaches the raw run's standard error.
4. The share of var(L) that comes from opening rolls: the rolls' lucks are uncorrelated, so
   var(L) is the sum of the steps' mean squares; from a traced match at 512 lanes (the trace's
   limit) the sum of luck^2 over opening steps against the sum over all steps.
Nothing here is asserted; every figure is reported.
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
BATCH, GAMES_PER_LANE, MAX_STEPS, TIMED = 65536, 2, 4000, 1
MATCHUPS = {"policy": ("policy", None), "1ply": ("1ply", None), "2ply_top4": ("2ply", 4)}
SHARE_BATCH = 512


def child(cmd, pkg, timeout=900):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)}", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def setup(path_a, path_b, matchup, batch):
    import torch
    from bgx.arena import Arena, load_net, make_player
    dev = torch.device("cuda", 0)
    nets = [load_net(p, dev) for p in (path_a, path_b)]
    kind, top_k = MATCHUPS[matchup]
    players = [make_player(kind, n, seed=3 + i, top_k=top_k) for i, n in enumerate(nets)]
    ar = Arena(batch, GAMES_PER_LANE, seed=1, max_moves=min(n.action_head.out_features for n in nets), device=dev)
    return torch, dev, nets, ar, players


def worker(path_a, path_b, matchup, luck):
    """One untimed and TIMED timed matches in this process, with the package on PYTHONPATH; one JSON line."""
    torch, dev, nets, ar, players = setup(path_a, path_b, matchup, BATCH)
    kw = {}
    if luck:
        from bgx.arena import ArenaLuck
        from bgx.search import ValueHead
        kw = dict(luck=ArenaLuck(ValueHead(nets[0])))
    ar.play(*players, max_steps=MAX_STEPS, **kw)                           # untimed: allocations, first launches
    times = []
    for _ in range(TIMED):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = ar.play(*players, max_steps=MAX_STEPS, **kw)
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
    keys = ["steps", "games", "unfinished_lanes", "ppg_a", "ppg_stderr", "win_rate_a"]
    if luck:
        keys += ["ppg_luck_a", "ppg_luck_stderr", "variance_ratio", "luck_scale", "luck_mean", "luck_mean_stderr"]
    print(json.dumps(dict(matchup=matchup, luck=bool(luck), seconds=times, **{k: r[k] for k in keys})), flush=True)


def share_worker(path_a, path_b, matchup):
    """The opening rolls' share of var(L), from a traced match at SHARE_BATCH lanes."""
    torch, dev, nets, ar, players = setup(path_a, path_b, matchup, SHARE_BATCH)
    from bgx.arena import TRACE_LIMIT
    from bgx.search import ValueHead
    r, tr = ar.play(*players, max_steps=TRACE_LIMIT // (SHARE_BATCH * 21), trace=True, luck=ValueHead(nets[0]))
    on, op = tr["owner"] != 0, tr["luck_opening"] != 0
    sq = torch.where(on, tr["luck"], 0.0).double() ** 2
    print(json.dumps(dict(matchup=matchup, lanes=SHARE_BATCH, steps=r["steps"], games=r["games"],
                          unfinished_lanes=r["unfinished_lanes"], rolls=int(on.sum()), opening_rolls=int(op.sum()),
                          sum_luck2=float(sq.sum()), sum_luck2_opening=float(sq[op].sum()),
                          opening_share_of_var_luck=float(sq[op].sum() / sq.sum()))), flush=True)


def fresh_net(path, hidden):
    sys.path.insert(0, PKG)
    import torch
    from bgx.policy import PolicyNet
    torch.manual_seed(1)
    torch.save(PolicyNet(hidden_size=hidden).state_dict(), path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--matchup", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-pkg", default=None, help="the parent commit's built package directory (holds bgx/)")
    ap.add_argument("--a", default=None, help="an existing state_dict for A instead of training one")
    ap.add_argument("--b", default=None, help="... for B instead of a fresh net")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_luck", "summary.json"))
    args = ap.parse_args()
    if args.worker == "share":
        return share_worker(args.a, args.b, args.matchup)
    if args.worker:
        return worker(args.a, args.b, args.matchup, args.worker == "luck")
    if args.parent_pkg is None or not os.path.isdir(os.path.join(args.parent_pkg, "bgx")):
        ap.error("--parent-pkg must be the parent commit's built package directory")
    os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
    summary = {"checkpoints": {}}
    a, b = args.a, args.b
    if a is None:
        a = os.path.join(ROOT, "models", "arena_luck_profile_a.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", a]
        t0 = time.perf_counter()
        child(cmd, PKG)
        summary["checkpoints"]["a"] = dict(command="python " + " ".join(cmd[:-1] + ["models/arena_luck_profile_a.pt"]),
                                           updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    if b is None:
        b = os.path.join(ROOT, "models", "arena_luck_profile_b.pt")
        fresh_net(b, args.hidden)
        summary["checkpoints"]["b"] = dict(net="fresh: PolicyNet's initial weights, torch.manual_seed(1)", hidden=args.hidden)
    summary["setup"] = dict(
        lanes=BATCH, games_per_lane=GAMES_PER_LANE, max_steps=MAX_STEPS, luck_value="A's value head", luck_scale="fit",
        baseline="the parent commit's package, no luck", alternation=f"parent, this, {args.rounds} rounds",
        timed=f"warm Arena.play after an untimed match of the same shape, {TIMED} per child; the median of all",
        stderr_per_game="stderr * sqrt(games)",
        seconds_to_baseline_stderr="games * (stderr_per_game_luck / stderr_per_game of the baseline)^2 / games_per_s "
                                   "of the luck run")
    me = os.path.abspath(__file__)
    summary["matchups"] = {}
    for m in MATCHUPS:
        runs = {"parent": [], "luck": []}
        for _ in range(args.rounds):
            for case, pkg in (("parent", args.parent_pkg), ("luck", PKG)):
                runs[case].append(json.loads(child([me, "--worker", case, "--matchup", m, "--a", a, "--b", b], pkg)[-1]))
        out = {}
        for case, rs in runs.items():
            secs = [s for r in rs for s in r["seconds"]]
            med = statistics.median(secs)
            r = dict(rs[-1], seconds=med, seconds_min=min(secs), seconds_max=max(secs), seconds_all=secs)
            r.update(games_per_s=r["games"] / med, ms_per_step=1e3 * med / max(r["steps"], 1),
                     stderr_per_game=r["ppg_stderr"] * r["games"] ** 0.5)
            out[case] = r
        p, l = out["parent"], out["luck"]
        l["stderr_per_game_luck"] = l["ppg_luck_stderr"] * l["games"] ** 0.5
        l["luck_ms_per_step"] = l["ms_per_step"] - p["ms_per_step"]
        l["seconds_to_baseline_stderr"] = (l["games"] * (l["stderr_per_game_luck"] / p["stderr_per_game"]) ** 2
                                           / l["games_per_s"])
        l["speedup_to_baseline_stderr"] = p["seconds"] / l["seconds_to_baseline_stderr"]
        out["opening_share"] = json.loads(child([me, "--worker", "share", "--matchup", m, "--a", a, "--b", b], PKG)[-1])
        summary["matchups"][m] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
