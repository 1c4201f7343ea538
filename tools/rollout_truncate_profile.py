#!/usr/bin/env python
"""Measure truncated rollouts on one MI355X and write
profiles/truncate/summary.json.  Every group of measurements is a child process of its own and
the children run one after another: never more than one process with the GPU open.

    python tools/rollout_truncate_profile.py [--updates 200] [--net FILE] [--out FILE]
                                             [--players policy,1ply,2ply]

1. A checkpoint: the recipe of tools/rollout_luck_profile.py, a short
   `python -m bgx.train --returns selfplay` run at H = 128.  --net FILE uses an existing one.
2. bgx_value_lanes on 65,536 lane records (an engine after 30 policy steps) with every lane,
   a random 1/8 and 1/64 of the lanes, no lane and the first 1/8 of the lanes selected (and
   without a selection): microseconds per call, the median over 7 batches of 200 calls
   between two events.  It says how far the cost follows the selected rows.
3. Per player (policy, 1ply, 2ply with --top-k 4), 65,536 lanes from the opening with drawn
   first rolls, two games per lane: plain, and truncated at 8 and 16 plies with lookahead 0 and 1,
   each without and with the luck adjustment: games/s and ms per step of the warm loop
   (Rollout.run between device synchronisations, the median of five after an untimed run of
   the same shape; the last run's results),
   truncated_share, equity and its standard error (equity_luck's with the adjustment), and the
   seconds to a standard error of 0.01, extrapolated as stderr^2 * games / 0.01^2 / rate.
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
BATCH, TRIALS = 65536, 131072
HORIZONS, LOOKAHEADS, TARGET, REPS = (8, 16), (0, 1), 0.01, 5


def child(cmd, timeout=1500):
    """Run one child to its end and return its stdout lines; its failure is this script's."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    # the child's stderr is this script's: a long child shows its progress there
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, timeout=timeout)
    print(f"[{time.perf_counter() - t0:7.1f} s] {' '.join(cmd)}", file=sys.stderr, flush=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:])
        raise SystemExit(f"{' '.join(cmd)}: exit status {r.returncode}")
    return r.stdout.strip().splitlines()


def value_worker(net_path: str):
    """bgx_value_lanes' time per call at four selections; prints one JSON line."""
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import load_net
    from bgx.engine import Engine
    from bgx.search import ValueHead, value_lanes
    dev = torch.device("cuda", 0)
    net = load_net(net_path, dev)
    vh = ValueHead(net)
    eng = Engine(batch=BATCH, max_moves=min(net.action_head.out_features, 500), seed=1, auto_reset=True, device=dev)
    eng.reset(want_obs=False)
    for i in range(30):
        a, _, _ = net.act(eng, seed=5, step=i)
        eng.step(a, want_obs=False, want_info=False)
    rec = eng.records().clone()
    out = torch.empty(BATCH, dtype=torch.float32, device=dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    res = {}
    plans = (("no_selection", None), ("all", 1.0), ("one_eighth", 1 / 8), ("one_64th", 1 / 64), ("none", 0.0),
             ("first_eighth", "head"))
    for name, share in plans:
        if share == "head":                                  # contiguous: the lanes of one position, say
            sel = (torch.arange(BATCH) < BATCH // 8).to(torch.uint8).to(dev)
        else:
            sel = None if share is None else (torch.rand(BATCH, generator=g) < share).to(torch.uint8).to(dev)
        for _ in range(20):
            value_lanes(rec, vh, sel=sel, out=out)
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                value_lanes(rec, vh, sel=sel, out=out)
            e1.record()
            torch.cuda.synchronize(dev)
            us.append(1e3 * e0.elapsed_time(e1) / 200)
        res[name] = dict(selected=BATCH if sel is None else int(sel.sum()), us_per_call=statistics.median(us),
                         us_min=min(us), us_max=max(us))
    print(json.dumps(res), flush=True)


def player_worker(net_path: str, kind: str):
    """Every configuration of one player in this process; prints one JSON line per configuration."""
    sys.path.insert(0, PKG)
    import torch
    from bgx.arena import load_net, make_player
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    from bgx.truncate import Truncation
    dev = torch.device("cuda", 0)
    net = load_net(net_path, dev)
    vh = ValueHead(net)
    pos = opening_record()[None]
    configs = [(None, None)] + [(n, la) for n in HORIZONS for la in LOOKAHEADS]
    for horizon, la in configs:
        for luck in (False, True):
            player = make_player("2ply" if kind == "2ply" else kind, net, seed=3, top_k=4 if kind == "2ply" else None)
            tc = Truncation(vh, horizon, lookahead=la) if horizon is not None else None
            ro = Rollout(BATCH, seed=1, max_moves=min(net.action_head.out_features, 500), device=dev)
            kw = dict(first_roll="random", truncate=tc, luck=vh if luck else None)
            ro.run(player, pos, TRIALS, **kw)              # untimed: allocations, first launches
            times = []
            for _ in range(REPS):                          # a truncated run is 10-400 ms: the median of five
                steps0 = ro.steps
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                r, = ro.run(player, pos, TRIALS, **kw)
                torch.cuda.synchronize(dev)
                times.append(time.perf_counter() - t0)
                steps = ro.steps - steps0
            dt = statistics.median(times)
            se = r["equity_luck_stderr"] if luck else r["equity_stderr"]
            rate = r["games"] / dt
            out = dict(player=kind, truncate=horizon, lookahead=la, luck=luck, seconds=dt, seconds_min=min(times),
                       seconds_max=max(times), steps=steps, games=r["games"],
                       unfinished=r["unfinished"], games_per_s=rate, ms_per_step=1e3 * dt / max(steps, 1),
                       plies_per_game=r["plies_per_game"], truncated_share=r.get("truncated_share", 0.0),
                       equity=r["equity"], equity_stderr=r["equity_stderr"],
                       seconds_to_stderr_0_01=se * se * r["games"] / (TARGET * TARGET) / rate)
            if luck:
                out.update(equity_luck=r["equity_luck"], equity_luck_stderr=r["equity_luck_stderr"],
                           variance_ratio=r["variance_ratio"], luck_scale=r["luck_scale"])
            if tc is not None:
                out.update(truncated_equity=r["truncated_equity"])
            print(json.dumps(out), flush=True)
            print(f"  {kind} truncate={horizon} lookahead={la} luck={luck}: {dt:.2f} s", file=sys.stderr, flush=True)
            del ro, player


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--net", default=None, help="an existing state_dict instead of training one")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--players", default="policy,1ply,2ply")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truncate", "summary.json"))
    args = ap.parse_args()
    if args.worker == "value":
        return value_worker(args.net)
    if args.worker:
        return player_worker(args.net, args.worker)
    summary = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            summary = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")

    net = args.net
    if net is None:
        os.makedirs(os.path.join(ROOT, "models"), exist_ok=True)
        net = os.path.join(ROOT, "models", "rollout_truncate_profile.pt")
        cmd = ["-m", "bgx.train", "--batch", "65536", "--horizon", "64", "--updates", str(args.updates), "--hidden",
               str(args.hidden), "--returns", "selfplay", "--seed", "0", "--save", net]
        t0 = time.perf_counter()
        child(cmd)
        summary["checkpoint"] = dict(command="python " + " ".join(cmd[:-1] + ["models/rollout_truncate_profile.pt"]),
                                     updates=args.updates, hidden=args.hidden, seconds=time.perf_counter() - t0)
    summary["setup"] = dict(lanes=BATCH, games=TRIALS, positions="opening", first_roll="random",
                            two_ply="--top-k 4", horizons=list(HORIZONS), lookaheads=list(LOOKAHEADS),
                            timed="a warm Rollout.run, the median of five after an untimed run of the same shape",
                            seconds_to_stderr_0_01="stderr^2 * games / 0.01^2 / games_per_s (equity_luck_stderr with luck)")
    me = os.path.abspath(__file__)
    summary["value_lanes"] = json.loads(child([me, "--worker", "value", "--net", net])[-1])
    save()
    summary.setdefault("players", {})
    for kind in [k for k in args.players.split(",") if k]:
        summary["players"][kind] = [json.loads(ln) for ln in child([me, "--worker", kind, "--net", net])
                                    if ln.startswith("{")]
        save()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
