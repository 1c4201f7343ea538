#!/usr/bin/env python
"""Measure match-score rollouts on one MI355X and write
profiles/rollout_match/summary.json.  Every measurement is a child process of its own and the
children run one after another: never more than one process with the GPU open.

    python tools/rollout_match_profile.py [--updates 200] [--net FILE] [--cube-tree DIR] [--out FILE]

1. A net at H = 128 from a short `python -m bgx.train --returns selfplay` run (200 updates); --net
   uses an existing one.
2. At 65,536 lanes from the opening (random first rolls, four games scheduled per lane so that the
   lanes stay busy), a match to 7 at 7-away / 7-away and at 2-away / 4-away, with the policy, the
   1-ply and the 2-ply top-k 4 players, MatchRule lookahead 0 and 1 on the same net's value head:
   games/s and ms per step of Rollout.run within the player's step budget (after a short untimed run
   of the same shape), the match-winning chance, and its standard error per game (mwc_stderr
   sqrt(games)).  Beside each player and lookahead, the money-cube rollout (--cube, CubeRule's
   defaults) at the same lanes, player and step budget: games/s, ms per step and the cubeful equity's
   standard error per game.  --cube-tree DIR runs those on another checkout with its own built
   library (the parent commit's): the worker's cube mode uses only what that tree has.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("BGX_PROFILE_PKG") or os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")
BATCH, LENGTH, GAMES_PER_LANE = 65536, 7, 4
SCORES = {"7away_7away": (7, 7), "2away_4away": (2, 4)}
PLAYERS = {"policy": dict(kind="policy", top_k=None, max_steps=1500), "1ply": dict(kind="1ply", top_k=None, max_steps=400),
           "2ply_top4": dict(kind="2ply", top_k=4, max_steps=150)}


def child(cmd, timeout=1100, env=None):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    pkg = (env or {}).get("BGX_PROFILE_PKG", PKG)
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)}", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def worker(path: str, player: str, mode: str, score: str, lookahead: int, batch: int):
    """One timed run in this process; prints one JSON line."""
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import load_net, make_player
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    net = load_net(path, dev)
    pl = PLAYERS[player]
    who = make_player(pl["kind"], net, seed=3, top_k=pl["top_k"])
    if mode == "match":
        from bgx.match import MatchRule, RolloutMatch
        stage = dict(match=RolloutMatch(LENGTH, MatchRule(ValueHead(net), lookahead=lookahead)), match_away=SCORES[score])
    else:
        from bgx.cube import CubeRule
        stage = dict(cube=CubeRule(ValueHead(net), lookahead=lookahead))
    ro = Rollout(batch, seed=1, max_moves=min(net.action_head.out_features, 500), device=dev)
    pos, trials = opening_record()[None], batch * GAMES_PER_LANE
    ro.run(who, pos, trials, first_roll="random", max_steps=10, **stage)       # untimed: allocations, first launches
    torch.cuda.synchronize(dev)
    steps0, t0 = ro.steps, time.perf_counter()
    r, = ro.run(who, pos, trials, first_roll="random", max_steps=pl["max_steps"], **stage)
    torch.cuda.synchronize(dev)
    dt, steps = time.perf_counter() - t0, ro.steps - steps0
    n = r["games"]
    out = dict(player=player, mode=mode, lookahead=lookahead, lanes=batch, max_steps=pl["max_steps"], seconds=dt, steps=steps,
               games=n, unfinished=r["unfinished"], games_per_s=n / dt, ms_per_step=1e3 * dt / max(steps, 1),
               pass_share=r["pass_share"], mean_cube_log2=r["mean_cube_log2"])
    if mode == "match":
        out.update(score=score, away=list(SCORES[score]), mwc=r["mwc"], mwc_stderr=r["mwc_stderr"],
                   stderr_per_game=r["mwc_stderr"] * math.sqrt(n) if r["mwc_stderr"] is not None else None,
                   mwc_normalized=r["mwc_normalized"], doubles_per_game_start=r["doubles_per_game_start"],
                   doubles_per_game_other=r["doubles_per_game_other"])
    else:
        from bgx import _lib
        out.update(equity_cubeful=r["equity_cubeful"], equity_cubeful_stderr=r["equity_cubeful_stderr"],
                   stderr_per_game=r["equity_cubeful_stderr"] * math.sqrt(n), doubles_per_game=r["doubles_per_game"],
                   library_build_id=_lib.embedded_build_id())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--player", default="policy", help=argparse.SUPPRESS)
    ap.add_argument("--score", default="7away_7away", help=argparse.SUPPRESS)
    ap.add_argument("--lookahead", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--lanes", type=int, default=BATCH)
    ap.add_argument("--cube-tree", default=None, help="the checkout the money-cube runs use (the parent commit's, built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_match", "summary.json"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.net, args.player, args.worker, args.score, args.lookahead, args.lanes)
    summary = {"checkpoint": {}}
    path = args.net
    if path is None:
        os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
        path = os.path.join(ROOT, "models", "rollout_match_profile.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", path]
        t0 = time.perf_counter()
        child(cmd)
        summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_match_profile.pt"]),
                                     updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=args.lanes, match_length=LENGTH, scores={k: list(v) for k, v in SCORES.items()},
                            position="the opening, random first rolls", games_scheduled_per_lane=GAMES_PER_LANE,
                            players=PLAYERS, rules="MatchRule / CubeRule defaults on the net's own value head",
                            timed="Rollout.run within the player's step budget, after an untimed 10-step run of the same shape",
                            stderr_per_game="the standard error of the mean times sqrt(games): MWC for match, points for cube",
                            cube_tree="the parent commit's checkout and library" if args.cube_tree else
                            "this tree (the money-cube path is unchanged: profiles/rollout_match/kernel_diff.txt)")
    me = os.path.abspath(__file__)
    summary["cases"] = {}
    for player in PLAYERS:
        for la in (0, 1):
            base = [me, "--player", player, "--lookahead", str(la), "--net", path, "--lanes", str(args.lanes)]
            for score in SCORES:
                summary["cases"][f"{player}/lookahead_{la}/match/{score}"] = json.loads(
                    child(base + ["--worker", "match", "--score", score])[-1])
            env = ({"BGX_PROFILE_PKG": os.path.join(os.path.abspath(args.cube_tree), "mlp-ppo-2ply-p3_amd")}
                   if args.cube_tree else None)
            summary["cases"][f"{player}/lookahead_{la}/cube"] = json.loads(child(base + ["--worker", "cube"], env=env)[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
