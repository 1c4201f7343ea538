"""The returns path's time on one GPU (profiles/selfplay_returns/timing.json; DESIGN.md §6
"Self-play returns"), on the buffers of a real rollout at T x B = 32 x 65,536, in one process:

  1. returns="lane" as update() forms R and adv: lane_returns + global_normalize + the
     subtraction of the stored values;
  2. returns="selfplay": selfplay_gae (bgx_selfplay_gae + bgx_normalize_adv);
  3. the bootstrap value pass that ends a selfplay rollout (one greedy policy pass per
     shard on the shards' streams, joined).

Device events around each, warm, alternating, the median of --reps repetitions.

    python tools/selfplay_returns_timing.py [--out profiles/selfplay_returns/timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selfplay_returns", "timing.json"))
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "selfplay_returns_timing needs the GPU"
    from bgx.ppo import global_normalize
    from bgx.train import PPOTrainer, lane_returns, selfplay_gae
    tr = PPOTrainer(batch=args.batch, horizon=args.horizon, seed=0, returns="selfplay")
    for _ in range(3):
        tr.rollout()
    b = tr.buf

    def parent():
        R = global_normalize(lane_returns(b["rewards"], b["dones"]).reshape(-1), None)
        return R, R - b["values"].reshape(-1)

    def new():
        return selfplay_gae(b["rewards"], b["dones"], b["records"], b["values"], b["boot_values"], b["boot_records"],
                            tr.gamma, tr.gae_lambda)

    def boot():
        cur = tr._streams[0]
        for st in tr._streams[1:]:
            st.wait_stream(cur)
        for k in range(tr.S):
            with torch.cuda.stream(tr._streams[k]):
                tr._boot_pass(k)
        for st in tr._streams[1:]:
            cur.wait_stream(st)

    legs = {"lane_returns_normalize_subtract": parent, "selfplay_gae_normalize": new, "bootstrap_pass": boot}
    ms = {k: [] for k in legs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(args.reps + 5):                   # five warm-up rounds, then alternate
        for k, fn in legs.items():
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if r >= 5:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    res = {"device": torch.cuda.get_device_name(0),
           "command": f"python tools/selfplay_returns_timing.py --batch {args.batch} --horizon {args.horizon} "
                      f"--reps {args.reps}  (device events around each call, 5 warm-up rounds, the legs alternating)",
           "T": args.horizon, "B": args.batch, "shards": tr.S,
           "ms_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_min": {k: min(v) for k, v in ms.items()}, "ms_max": {k: max(v) for k, v in ms.items()}}
    res["new_over_parent"] = (res["ms_median"]["selfplay_gae_normalize"]
                              / res["ms_median"]["lane_returns_normalize_subtract"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
