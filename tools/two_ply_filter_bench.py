"""The 2-ply search with and without its 1-ply move filter (DESIGN.md §5 "Move filter"):
the full two_ply against two_ply(top_k=k, margin=inf) on the same roots, the variants
interleaved in one process.

    python tools/two_ply_filter_bench.py --out profiles/two_ply_filter/summary.json

Roots: --batch Philox lanes advanced --steps-in random-policy steps from reset.  Weights:
the golden G5 value nets (tests/golden/mlp.npz) at H = 40 and H = 128, or --weights
H=file.pt state_dicts.  Each variant is warmed up, then timed --reps times in turn (a host
clock around a call that ends in a device synchronise: two_ply reads its statistics back).
Per variant: roots/s (median, min, max over the repetitions), kept and candidate rows,
leaves, the first round's enumeration / evaluation times (two_ply_timings) and what is
left of the call (the 1-ply pass, the filter, the row set-up and the reduce), the fraction
of roots whose choice equals the full search's, and the mean Q (of the full search) given
up by the other choices."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd"))


def load_net(H, weights):
    from bgx.policy import PolicyNet
    net = PolicyNet(hidden_size=H)
    if H in weights:
        net.load_state_dict(torch.load(weights[H], map_location="cpu", weights_only=True))
        src = weights[H]
    else:
        mlp, pre = dict(np.load(os.path.join(ROOT, "tests", "golden", "mlp.npz"))), f"h{H}_"
        net.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in mlp.items()
                             if k.startswith(pre) and not k.endswith(("logits", "values"))})
        src = "tests/golden/mlp.npz (G5)"
    return net.cuda().eval(), src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps-in", type=int, default=40)
    ap.add_argument("--hidden", type=int, nargs="+", default=[40, 128])
    ap.add_argument("--top-k", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", nargs="*", default=[], help="H=file.pt")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    import bgx
    from bgx.arena import RandomPlayer
    from bgx.search import ValueHead, two_ply, two_ply_timings
    weights = {int(w.split("=")[0]): w.split("=", 1)[1] for w in args.weights}
    eng = bgx.Engine(batch=args.batch, max_moves=500, seed=args.seed, dice="philox", auto_reset=True)
    eng.reset(want_obs=False)
    rnd = RandomPlayer(args.seed + 1)
    for t in range(args.steps_in):
        eng.step(rnd.act(eng, None, t), want_obs=False)
    n = eng.n_moves().to(torch.int64)
    has = n > 0
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "steps_in": args.steps_in, "seed": args.seed,
           "reps": args.reps, "warmup": args.warmup, "roots_with_moves": int(has.sum()),
           "legal_moves_mean": float(n.float().mean()), "by_hidden": {}}
    variants = [("full", None)] + [(f"top{k}", k) for k in args.top_k]
    for H in args.hidden:
        net, src = load_net(H, weights)
        vh = ValueHead(net)
        fbest, fbestq, fq, _ = two_ply(eng, vh, want_q=True)
        out = {"weights": src, "variants": {}}
        for name, k in variants:
            for _ in range(args.warmup):
                two_ply(eng, vh, top_k=k)
            best = two_ply(eng, vh, top_k=k)[0]
            chosen = fq.gather(1, best.to(torch.int64)[:, None])[:, 0]
            out["variants"][name] = {"top_k": k, "ms": [], "enum_ms": [], "eval_ms": [],
                                     "same_choice": float((best == fbest)[has].float().mean()),
                                     "mean_q_given_up": float((fbestq - chosen)[has].double().mean())}
        del fq
        for _ in range(args.reps):
            for name, k in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = two_ply(eng, vh, top_k=k)[3]
                torch.cuda.synchronize()
                v = out["variants"][name]
                v["ms"].append((time.perf_counter() - t0) * 1e3)
                en, ev = two_ply_timings(eng)
                v["enum_ms"].append(en)
                v["eval_ms"].append(ev)
                st.setdefault("candidates", st["afterstates"])      # the full search: every candidate
                v["stats"] = st
        base = statistics.median(out["variants"]["full"]["ms"])
        for name, _ in variants:
            v = out["variants"][name]
            med = statistics.median(v["ms"])
            v.update(ms_median=med, ms_min=min(v["ms"]), ms_max=max(v["ms"]),
                     roots_per_s=args.batch / med * 1e3, roots_per_s_min=args.batch / max(v["ms"]) * 1e3,
                     roots_per_s_max=args.batch / min(v["ms"]) * 1e3, enum_ms_median=statistics.median(v["enum_ms"]),
                     eval_ms_median=statistics.median(v["eval_ms"]), speedup_over_full=base / med)
            v["rest_ms_median"] = med - v["enum_ms_median"] - v["eval_ms_median"]
            print(f"H={H} {name}: {med:.2f} ms [{v['ms_min']:.2f}, {v['ms_max']:.2f}]  {v['roots_per_s'] / 1e6:.2f} M roots/s"
                  f"  enum {v['enum_ms_median']:.2f} eval {v['eval_ms_median']:.2f} rest {v['rest_ms_median']:.2f} ms"
                  f"  rows {v['stats']['afterstates']}/{v['stats']['candidates']}  same choice {v['same_choice']:.4f}"
                  f"  x{v['speedup_over_full']:.2f}", flush=True)
        res["by_hidden"][str(H)] = out
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
