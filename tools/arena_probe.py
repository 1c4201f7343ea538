"""The arena's performance figures (profiles/arena_summary.json), on one GPU:

  1. policy vs policy through the command line (python -m bgx.arena) at B = 65,536, G = 2:
     games/s and env steps/s;
  2. the time of one two_ply call at B = 4,096, H = 40 with every lane selected and with
     the lanes of one mover selected, alternating the two on the same positions;
  3. the arena loop's own kernels (merge + advance) per step at B = 65,536, from device
     events around a run of them.

    python tools/arena_probe.py [--out profiles/arena_summary.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd"))


def policy_match(batch, games, max_steps):
    from bgx import arena
    from bgx.policy import PolicyNet
    out = {}
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in (0, 1):
            torch.manual_seed(i)
            paths.append(os.path.join(d, f"net{i}.pt"))
            torch.save(PolicyNet(hidden_size=128).state_dict(), paths[-1])
        argv = ["--a", paths[0], "--b", paths[1], "--player-a", "policy", "--player-b", "policy", "--batch", str(batch),
                "--games-per-lane", str(games), "--max-steps", str(max_steps), "--seed", "1"]
        arena.main(["--a", paths[0], "--b", paths[1], "--batch", "4096", "--games-per-lane", "1", "--max-steps",
                    str(max_steps)])                                    # warm-up: code objects, allocator
        runs = [arena.main(argv) for _ in range(3)]
    keep = ("games", "steps", "unfinished_lanes", "seconds", "games_per_s", "env_steps_per_s", "win_rate_a", "plies")
    out["command"] = ("python -m bgx.arena --a net0.pt --b net1.pt --player-a policy --player-b policy "
                      f"--batch {batch} --games-per-lane {games} --max-steps {max_steps} --seed 1  "
                      "(net0 / net1: fresh PolicyNet(hidden_size=128) under torch.manual_seed(0 / 1); 3 runs)")
    out["runs"] = [{k: r[k] for k in keep} for r in runs]
    out["games_per_s_median"] = statistics.median(r["games_per_s"] for r in runs)
    out["env_steps_per_s_median"] = statistics.median(r["env_steps_per_s"] for r in runs)
    return out


def two_ply_selected(batch, reps):
    import bgx
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead, two_ply
    torch.manual_seed(0)
    net = PolicyNet(hidden_size=40).cuda()
    vh = ValueHead(net)
    eng = bgx.Engine(batch=batch, max_moves=500, seed=11, dice="philox", auto_reset=True)
    eng.reset(want_obs=False)
    from bgx.arena import RandomPlayer
    rp = RandomPlayer(5)
    for s in range(25):
        eng.step(rp.act(eng, None, s), want_obs=False)
    rec = eng.records()
    sels = {"all": torch.ones(batch, dtype=torch.uint8, device="cuda"), "player1": (rec[:, 52] == 0).to(torch.uint8),
            "player2": (rec[:, 52] == 1).to(torch.uint8)}
    ms = {k: [] for k in sels}
    stats = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(reps + 2):                       # two warm-up rounds, then alternate
        for k, sel in sels.items():
            torch.cuda.synchronize()
            ev[0].record()
            stats[k] = two_ply(eng, vh, sel=sel)[3]
            ev[1].record()
            torch.cuda.synchronize()
            if r >= 2:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    return {"command": f"python tools/arena_probe.py  (two_ply(eng, vh, sel=...) at B = {batch}, H = 40, 25 random "
                       f"steps in; {reps} alternating repetitions, device events around each call)",
            "lanes_selected": {k: int(v.sum()) for k, v in sels.items()}, "stats": stats,
            "ms_median": {k: statistics.median(v) for k, v in ms.items()},
            "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()},
            "half_over_full": (statistics.median(ms["player1"]) + statistics.median(ms["player2"])) / 2
                              / statistics.median(ms["all"])}


def loop_overhead(batch, steps):
    """merge + advance per step: the two launches alone, `steps` times, between device
    events (the lanes stand still; the kernels' work does not depend on the position)."""
    import ctypes
    from bgx import _lib
    from bgx.arena import Arena, _stream
    from bgx.engine import _ptr
    L = _lib.load()
    ar = Arena(batch, 1 << 20, seed=3)
    ar.eng.reset(want_obs=False)
    recs = ctypes.c_void_p(ar.eng.lanes_ptr())
    dev = ar.eng.device
    state = (_ptr(ar.games_done), _ptr(ar.sel_a), _ptr(ar.sel_b), _ptr(ar.tally))
    L.bgx_arena_begin(recs, batch, ar.G, *state, _stream(dev))
    act = torch.zeros(batch, dtype=torch.int32, device=dev)
    ar.eng.step(act, want_obs=False)
    done, info = ar.eng.done, ar.eng.info
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = []
    for r in range(4):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(steps):
            L.bgx_arena_merge(_ptr(ar.sel_a), _ptr(ar.sel_b), _ptr(act), _ptr(act), batch, _ptr(ar.actions),
                              _stream(dev))
            L.bgx_arena_advance(recs, _ptr(done), _ptr(info), batch, ar.G, *state, _stream(dev))
        ev[1].record()
        torch.cuda.synchronize()
        if r:
            res.append(ev[0].elapsed_time(ev[1]) * 1e3 / steps)
    out = {"command": f"python tools/arena_probe.py  (bgx_arena_merge + bgx_arena_advance x {steps} at B = {batch}, "
                      "device events around the run, 3 runs after a warm-up)",
           "merge_plus_advance_us_per_step": statistics.median(res), "runs_us": res}
    try:
        with open(os.path.join(ROOT, "profiles", "latest_summary.json")) as f:
            tw = json.load(f)["env_step"]["timed_window"]
        out["env_step_span_us_per_step"] = tw["span_ms_per_step"] * 1e3
        out["env_step_source"] = "profiles/latest_summary.json env_step.timed_window (4 shards x 16,384 lanes)"
        out["overhead_over_env_step"] = out["merge_plus_advance_us_per_step"] / out["env_step_span_us_per_step"]
    except (OSError, KeyError):
        pass
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_summary.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--max-steps", type=int, default=4000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "arena_probe needs the GPU"
    res = {"device": torch.cuda.get_device_name(0),
           "policy_vs_policy": policy_match(args.batch, 2, args.max_steps),
           "two_ply_selected": two_ply_selected(4096, 7),
           "loop_overhead": loop_overhead(args.batch, 500)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
