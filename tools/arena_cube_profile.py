#!/usr/bin/env python
"""Measure the arena with the doubling cube on one MI355X and write
profiles/arena_cube/summary.json.  Every measurement is a child process of its own and the
children run one after another: never more than one process with the GPU open.

    python tools/arena_cube_profile.py [--updates-a 200] [--updates-b 100] [--a FILE --b FILE] [--out FILE]

1. Two checkpoints: the recipe of tools/rollout_cube_profile.py, short
   `python -m bgx.train --returns selfplay` runs at H = 128.  --a / --b use existing ones.
2. Policy against policy at 65,536 lanes, two games per lane, three cases: no cube, the cube with
   lookahead 0 (bgx_value_lanes, sync-free) and with lookahead 1 (bgx_roll_luck's mean, one host
   read per call), CubeRule's defaults on each side's own value head: games/s and ms per step of
   the warm loop (Arena.play between device synchronisations, after an untimed match of the same
   shape), and the cubeful result.
3. The cube kernels' launch times: 40 steps into a lookahead-0 match, each of sel, offer,
   respond, reseat and flush 200 times in a row between two events, on the match's own state.
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
BATCH, GAMES_PER_LANE, MAX_STEPS = 65536, 2, 4000
CASES = {"no_cube": None, "lookahead_0": 0, "lookahead_1": 1}


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


def setup(path_a: str, path_b: str, lookahead):
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import Arena, ArenaCube, PolicyPlayer, load_net
    from bgx.cube import CubeRule
    from bgx.search import ValueHead
    dev = torch.device("cuda", 0)
    nets = [load_net(p, dev) for p in (path_a, path_b)]
    players = [PolicyPlayer(n, seed=3 + i) for i, n in enumerate(nets)]
    cube = None if lookahead is None else ArenaCube(*[CubeRule(ValueHead(n), lookahead=lookahead) for n in nets])
    ar = Arena(BATCH, GAMES_PER_LANE, seed=1, max_moves=min(n.action_head.out_features for n in nets), device=dev)
    return torch, dev, ar, players, cube


def worker(path_a: str, path_b: str, case: str):
    """One timed match in this process; prints one JSON line."""
    torch, dev, ar, players, cube = setup(path_a, path_b, CASES[case])
    ar.play(*players, max_steps=MAX_STEPS, cube=cube)                      # untimed: allocations, first launches
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = ar.play(*players, max_steps=MAX_STEPS, cube=cube)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    out = dict(case=case, seconds=dt, steps=r["steps"], games=r["games"], unfinished_lanes=r["unfinished_lanes"],
               games_per_s=r["games"] / dt, ms_per_step=1e3 * dt / max(r["steps"], 1))
    if cube is not None:
        out.update({k: r[k] for k in ("ppg_cubeful_a", "ppg_cubeful_stderr", "win_rate_cubeful_a", "pass_share",
                                      "doubles_per_game_a", "doubles_per_game_b", "take_share_a", "take_share_b",
                                      "mean_cube_log2")},
                   played_out_ppg_a=r["played_out"]["ppg_a"], equity_calls_a=cube.rule_a.totals["calls"],
                   equity_calls_b=cube.rule_b.totals["calls"])
    else:
        out.update(ppg_a=r["ppg_a"], ppg_stderr=r["ppg_stderr"], win_rate_a=r["win_rate_a"])
    print(json.dumps(out), flush=True)


def kernel_worker(path_a: str, path_b: str, reps: int = 200):
    """The five per-step kernels' launch times on a match's own state, 40 steps in."""
    import ctypes
    torch, dev, ar, players, cube = setup(path_a, path_b, 0)
    from bgx import _lib
    from bgx.engine import _ptr, _stream
    ar.play(*players, max_steps=40, cube=cube)
    L, cs, st, recs = _lib.load(), ar.cube_state, _stream(dev), ctypes.c_void_p(ar.eng.lanes_ptr())
    ra, rb = cube.rule_a.struct(), cube.rule_b.struct()
    done = torch.zeros(BATCH, dtype=torch.uint8, device=dev)
    info = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    p = {k: _ptr(v) for k, v in cs.items()}
    gd, sa, sb, tally = (_ptr(t) for t in (ar.games_done, ar.sel_a, ar.sel_b, ar.tally))
    calls = {
        "sel": lambda: L.bgx_arena_cube_sel(recs, sa, sb, p["plies"], p["cube"], BATCH, cube.cap, p["dsel_a"], p["dsel_b"], st),
        "offer": lambda: L.bgx_arena_cube_offer(recs, p["dsel_a"], p["dsel_b"], p["eq_a"], p["eq_b"], ra, rb, p["cube"],
                                                BATCH, p["off_a"], p["off_b"], p["tally"], st),
        "respond": lambda: L.bgx_arena_cube_respond(recs, p["off_a"], p["off_b"], p["er_a"], p["er_b"], ra, rb, BATCH,
                                                    GAMES_PER_LANE, p["cube"], p["plies"], gd, sa, sb, tally, p["tally"],
                                                    p["mask"], st),
        "reseat": lambda: L.bgx_arena_cube_reseat(recs, p["mask"], BATCH, GAMES_PER_LANE, gd, sa, sb, st),
        "flush": lambda: L.bgx_arena_cube_flush(sa, sb, _ptr(done), _ptr(info), gd, BATCH, int(cube.jacoby), cube.cap,
                                                p["cube"], p["plies"], p["tally"], st),
    }
    out = {"lanes": BATCH, "launches_per_kernel": reps, "state": "40 steps into a lookahead-0 match"}
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
    ap.add_argument("--a", default=None, help="an existing state_dict for A instead of training one")
    ap.add_argument("--b", default=None, help="... for B")
    ap.add_argument("--updates-a", type=int, default=200)
    ap.add_argument("--updates-b", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_cube", "summary.json"))
    args = ap.parse_args()
    if args.worker == "kernels":
        return kernel_worker(args.a, args.b)
    if args.worker:
        return worker(args.a, args.b, args.worker)
    summary = {"checkpoints": {}}
    paths = {}
    for side, given, updates in (("a", args.a, args.updates_a), ("b", args.b, args.updates_b)):
        paths[side] = given
        if given is None:
            os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
            paths[side] = os.path.join(ROOT, "models", f"arena_cube_profile_{side}.pt")
            cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(updates), "--hidden",
                   str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", paths[side]]
            t0 = time.perf_counter()
            child(cmd)
            summary["checkpoints"][side] = dict(
                command="python " + " ".join(cmd[:-1] + [f"models/arena_cube_profile_{side}.pt"]), updates=updates,
                hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=BATCH, games_per_lane=GAMES_PER_LANE, max_steps=MAX_STEPS, players="policy against policy",
                            rules="CubeRule defaults on each side's own value head: scale 1, double_at 0.40, "
                                  "pass_at 0.50, too_good_at inf, cap 6",
                            timed="a warm Arena.play, after an untimed match of the same shape")
    me = os.path.abspath(__file__)
    summary["cases"] = {case: json.loads(child([me, "--worker", case, "--a", paths["a"], "--b", paths["b"]])[-1])
                        for case in CASES}
    summary["games_per_s"] = {c: v["games_per_s"] for c, v in summary["cases"].items()}
    summary["ms_per_step"] = {c: v["ms_per_step"] for c, v in summary["cases"].items()}
    summary["cube_kernels"] = json.loads(child([me, "--worker", "kernels", "--a", paths["a"], "--b", paths["b"]])[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
