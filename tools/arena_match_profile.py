#!/usr/bin/env python
"""Measure match play in the arena on one MI355X and write
profiles/arena_match/summary.json.  Every measurement is a child process of its own and the
children run one after another: never more than one process with the GPU open.

    python tools/arena_match_profile.py [--updates 200] [--a FILE --b FILE] [--cube-tree DIR] [--out FILE]

1. Two nets at H = 128: A from a short `python -m bgx.train --returns selfplay` run (200 updates),
   B fresh (0 updates).  --a / --b use existing ones.
2. At 65,536 lanes, matches to 7, one match per lane, two pairs of players -- policy against policy
   and 2-ply top-k 4 against the same -- each with MatchRule lookahead 0 and 1 on each side's own
   value head: matches/s, games/s and ms per step of a warm Arena.play (after an untimed run of the
   same shape) within the pair's step budget, and the match result.  Beside each, the money-cube
   arena (--cube, CubeRule's defaults) at the same lanes, players, lookahead and step budget, with
   the games-per-lane that gives a lane as many games as a match has on average: games/s and ms
   per step.  --cube-tree DIR runs those on another checkout with its own built library (the parent
   commit's): the worker's cube mode uses only what that tree has.
3. The match kernels' launch times: 40 steps into a lookahead-0 match, each of sel, offer, respond,
   reseat, flush and retire 200 times in a row between two events, on the match's own state.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("BGX_PROFILE_PKG") or os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")
BATCH, LENGTH, MATCHES_PER_LANE, CUBE_GAMES_PER_LANE = 65536, 7, 1, 6
PAIRS = {"policy": dict(kind="policy", top_k=None, max_steps=6000), "2ply_top4": dict(kind="2ply", top_k=4, max_steps=150)}


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


def setup(path_a: str, path_b: str, pair: str, mode: str, lookahead: int, batch: int):
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import Arena, ArenaCube, load_net, make_player
    from bgx.cube import CubeRule
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    nets = [load_net(p, dev) for p in (path_a, path_b)]
    pr = PAIRS[pair]
    players = [make_player(pr["kind"], n, seed=3 + i, top_k=pr["top_k"]) for i, n in enumerate(nets)]
    if mode == "match":
        from bgx.match import ArenaMatch, MatchRule
        stage = dict(match=ArenaMatch(LENGTH, *[MatchRule(ValueHead(n), lookahead=lookahead) for n in nets]))
        per_lane = MATCHES_PER_LANE
    else:
        stage = dict(cube=ArenaCube(*[CubeRule(ValueHead(n), lookahead=lookahead) for n in nets]))
        per_lane = CUBE_GAMES_PER_LANE
    ar = Arena(batch, per_lane, seed=1, max_moves=min(n.action_head.out_features for n in nets), device=dev)
    return torch, dev, ar, players, stage


def worker(path_a: str, path_b: str, pair: str, mode: str, lookahead: int, batch: int):
    """One timed run in this process; prints one JSON line."""
    torch, dev, ar, players, stage = setup(path_a, path_b, pair, mode, lookahead, batch)
    steps = PAIRS[pair]["max_steps"]
    ar.play(*players, max_steps=steps, **stage)                            # untimed: allocations, first launches
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = ar.play(*players, max_steps=steps, **stage)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    out = dict(pair=pair, mode=mode, lookahead=lookahead, lanes=batch, max_steps=steps, seconds=dt, steps=r["steps"],
               games=r["games"], unfinished_lanes=r["unfinished_lanes"], games_per_s=r["games"] / dt,
               ms_per_step=1e3 * dt / max(r["steps"], 1))
    if mode == "match":
        out.update(matches_per_s=r["matches"] / dt,
                   **{k: r[k] for k in ("matches", "match_win_rate_a", "match_win_rate_stderr", "games_per_match",
                                        "doubles_per_game_a", "doubles_per_game_b", "take_share_a", "take_share_b",
                                        "pass_share", "mean_cube_log2", "crawford_share", "post_crawford_share")})
    else:
        from bgx import _lib
        out.update(ppg_cubeful_a=r["ppg_cubeful_a"], pass_share=r["pass_share"], library_build_id=_lib.embedded_build_id())
    print(json.dumps(out), flush=True)


def kernel_worker(path_a: str, path_b: str, batch: int, reps: int = 200):
    """The six per-step kernels' launch times on a match's own state, 40 steps in."""
    import ctypes
    torch, dev, ar, players, stage = setup(path_a, path_b, "policy", "match", 0, batch)
    from bgx import _lib
    from bgx.engine import _ptr, _stream
    match = stage["match"]
    ar.play(*players, max_steps=40, match=match)
    L, ms, st, recs = _lib.load(), ar.match_state, _stream(dev), ctypes.c_void_p(ar.eng.lanes_ptr())
    ra, rb, G = match.rule_a.struct(), match.rule_b.struct(), match.games_quota(MATCHES_PER_LANE)
    met, pc = (_ptr(t) for t in match.tables(dev))
    done = torch.zeros(batch, dtype=torch.uint8, device=dev)
    info = torch.zeros(batch, dtype=torch.int32, device=dev)
    p = {k: _ptr(v) for k, v in ms.items()}
    gd, sa, sb, tally = (_ptr(t) for t in (ar.games_done, ar.sel_a, ar.sel_b, ar.tally))
    lane = (p["away"], p["craw"], p["matches_done"], p["seat0"])
    calls = {
        "sel": lambda: L.bgx_arena_match_sel(recs, sa, sb, p["plies"], p["cube"], p["away"], p["craw"], batch, p["dsel_a"],
                                             p["dsel_b"], st),
        "offer": lambda: L.bgx_arena_match_offer(recs, sa, sb, p["dsel_a"], p["dsel_b"], p["eq_a"], p["eq_b"], ra, rb, met,
                                                 pc, LENGTH, p["plies"], p["cube"], p["away"], p["craw"], batch, p["off_a"],
                                                 p["off_b"], p["tally"], st),
        "respond": lambda: L.bgx_arena_match_respond(recs, p["off_a"], p["off_b"], p["er_a"], p["er_b"], ra, rb, met, pc,
                                                     LENGTH, batch, G, MATCHES_PER_LANE, p["cube"], p["plies"], *lane, gd,
                                                     sa, sb, tally, p["tally"], p["mask"], st),
        "reseat": lambda: L.bgx_arena_cube_reseat(recs, p["mask"], batch, G, gd, sa, sb, st),
        "flush": lambda: L.bgx_arena_match_flush(sa, sb, _ptr(done), _ptr(info), gd, batch, LENGTH, MATCHES_PER_LANE,
                                                 p["cube"], p["plies"], *lane, p["retire"], p["tally"], st),
        "retire": lambda: L.bgx_arena_match_retire(batch, G, p["retire"], gd, sa, sb, tally, st),
    }
    out = {"lanes": batch, "launches_per_kernel": reps, "state": "40 steps into a lookahead-0 match"}
    for name, call in calls.items():
        assert call() == 0
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize(dev)
        out[name + "_us"] = 1e3 * e0.elapsed_time(e1) / reps
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pair", default="policy", help=argparse.SUPPRESS)
    ap.add_argument("--lookahead", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--a", default=None, help="an existing state_dict for A instead of training one")
    ap.add_argument("--b", default=None, help="... for B")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--lanes", type=int, default=BATCH)
    ap.add_argument("--cube-tree", default=None, help="the checkout the money-cube runs use (the parent commit's, built)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_match", "summary.json"))
    args = ap.parse_args()
    if args.worker == "kernels":
        return kernel_worker(args.a, args.b, args.lanes)
    if args.worker:
        return worker(args.a, args.b, args.pair, args.worker, args.lookahead, args.lanes)
    summary = {"checkpoints": {}}
    paths = {}
    for side, given, updates in (("a", args.a, args.updates), ("b", args.b, 0)):
        paths[side] = given
        if given is None:
            os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
            paths[side] = os.path.join(ROOT, "models", f"arena_match_profile_{side}.pt")
            cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(updates), "--hidden",
                   str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", paths[side]]
            t0 = time.perf_counter()
            child(cmd)
            summary["checkpoints"][side] = dict(
                command="python " + " ".join(cmd[:-1] + [f"models/arena_match_profile_{side}.pt"]), updates=updates,
                hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=args.lanes, match_length=LENGTH, matches_per_lane=MATCHES_PER_LANE,
                            cube_games_per_lane=CUBE_GAMES_PER_LANE, pairs=PAIRS,
                            rules="MatchRule / CubeRule defaults on each side's own value head",
                            timed="a warm Arena.play within the pair's step budget, after an untimed run of the same shape",
                            cube_tree="the parent commit's checkout and library" if args.cube_tree else "this tree (the money-cube path is unchanged)")
    me = os.path.abspath(__file__)
    summary["cases"] = {}
    for pair in PAIRS:
        for la in (0, 1):
            for mode in ("match", "cube"):
                env = ({"BGX_PROFILE_PKG": os.path.join(os.path.abspath(args.cube_tree), "mlp-ppo-2ply-p3_amd")}
                       if mode == "cube" and args.cube_tree else None)
                cmd = [me, "--worker", mode, "--pair", pair, "--lookahead", str(la), "--a", paths["a"], "--b", paths["b"],
                       "--lanes", str(args.lanes)]
                summary["cases"][f"{pair}/lookahead_{la}/{mode}"] = json.loads(child(cmd, env=env)[-1])
    c = summary["cases"]
    summary["match_over_cube_ms_per_step"] = {
        f"{pair}/lookahead_{la}": c[f"{pair}/lookahead_{la}/match"]["ms_per_step"] - c[f"{pair}/lookahead_{la}/cube"]["ms_per_step"]
        for pair in PAIRS for la in (0, 1)}
    summary["match_kernels"] = json.loads(child([me, "--worker", "kernels", "--a", paths["a"], "--b", paths["b"],
                                                 "--lanes", str(args.lanes)])[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
