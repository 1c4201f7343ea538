"""Fingerprint of the trainer's numbers, to compare two commits on one library (point the
other checkout at it with BGX_LIB): three iterations (rollout + update) of
PPOTrainer(batch=8192, horizon=4, seed=21) in five configurations, then one JSON line per
configuration with the sha256 of the parameters, the Adam moments, the GradScaler state
and the four loss parts of the third update.  --dump DIR also writes every tensor to
DIR/<config>.npz (to measure a difference where two runs of one commit already differ).

    python tools/ppo_state_hash.py [--dump DIR] [config ...]
"""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")]
from bgx.train import PPOTrainer  # noqa: E402

CONFIGS = {"graphed": {},                               # the fused head, graphed from update 2
           "eager": {"update_graphs": False},
           "manual_h40": {"hidden": 40},                # the manual fp16 epoch
           "fp32": {"amp": False},
           "selfplay": {"returns": "selfplay"}}
LOSSES = ("policy_loss", "value_loss", "entropy", "total_loss")


def state(name):
    tr = PPOTrainer(batch=8192, horizon=4, seed=21, **CONFIGS[name])
    for _ in range(3):
        tr.rollout()
        m = tr.update()
    torch.cuda.synchronize()
    out = {}
    for n, p in tr.net.named_parameters():
        out["param." + n] = p.detach().cpu().numpy()
        for k in ("exp_avg", "exp_avg_sq", "step"):
            out[f"adam.{k}.{n}"] = tr.opt.state[p][k].detach().cpu().numpy()
    for k in ("_scale", "_growth_tracker"):
        t = getattr(tr.scaler, k, None)
        if torch.is_tensor(t):
            out["scaler." + k] = t.detach().cpu().numpy()
    out["losses"] = np.array([m[k] for k in LOSSES], np.float64)
    return out


def digest(st, prefix):
    h = hashlib.sha256()
    for k in sorted(st):
        if k.startswith(prefix):
            h.update(k.encode() + b"\0" + struct.pack("<q", st[k].size) + np.ascontiguousarray(st[k]).tobytes())
    return h.hexdigest()


def main():
    args = sys.argv[1:]
    dump = None
    if "--dump" in args:
        i = args.index("--dump")
        dump = args[i + 1]
        del args[i:i + 2]
        os.makedirs(dump, exist_ok=True)
    for name in args or list(CONFIGS):
        st = state(name)
        if dump:
            np.savez(os.path.join(dump, name + ".npz"), **st)
        print(json.dumps({"config": name, "all": digest(st, ""), "params": digest(st, "param."),
                          "adam": digest(st, "adam."), "scaler": digest(st, "scaler."),
                          "losses": digest(st, "losses"), "loss_parts": st["losses"].tolist()}), flush=True)


if __name__ == "__main__":
    main()
