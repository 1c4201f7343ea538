"""Per-wave phase times of the rollout policy kernel (experiment; a -DBGX_POLICY_STAMPS build
of libbgx.so: python tools/build_variant.py scratch/libbgx_pstamp.so -DBGX_POLICY_STAMPS).

    BGX_LIB=scratch/libbgx_pstamp.so B=16384 [ROWBEST=0|1|2] python tools/policy_stamps.py

Stamps (s_memrealtime, 100 MHz): start, after the count-0 scan + record staging, after
GEMM1, after the output tiles; main waves (32 rows each) and the extra count-0 waves
separately: phase means and the kernel span.  Per wave also the tiles walked and the tiles
whose noise block (the Gumbel keys) some lane entered: for the main waves the share that
enters it on the value tile or on a tile at or past the wave's legal actions' tiles (o_s),
where no key can win, and the tile-phase time of those waves beside the others'.  ROWBEST
sets BGX_POLICY_ROWBEST (the noise guard's form) for the measured launches."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "mlp-ppo-2ply-p3_amd"))
import bgx  # noqa: E402
from bgx import _lib  # noqa: E402
from bgx.policy import PolicyNet  # noqa: E402

B = int(os.environ.get("B", 16384))
if os.environ.get("ROWBEST"):
    _lib.debug_option("BGX_POLICY_ROWBEST", os.environ["ROWBEST"])
torch.manual_seed(0)
net = PolicyNet(hidden_size=128).cuda()
net.pack()
eng = bgx.Engine(batch=B, dice="philox", seed=3, auto_reset=True)
eng.reset()
for i in range(60):
    a, _, _ = net.act(eng, seed=1, step=i)
    eng.step(a)
rec = eng.records().clone()
L = _lib.load()
fn = L.bgx_debug_policy_stamps
fn.restype = ctypes.c_int
fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
W = 8192
buf = np.zeros((W, 6), dtype=np.uint64)
out = {}
for rep in range(3):
    net.act(rec, seed=2, step=rep)
    torch.cuda.synchronize()
    fn(buf.ctypes.data_as(ctypes.c_void_p), W)          # read + clear
    net.act(rec, seed=2, step=10 + rep)
    torch.cuda.synchronize()
    fn(buf.ctypes.data_as(ctypes.c_void_p), W)
    used = buf[:, 4] != 0
    st = buf[used].astype(np.float64)
    t0 = st[:, 0].min()
    res = {}
    for name, flag in (("extra", 1), ("main", 2)):
        s = st[st[:, 4] == flag]
        if not len(s):
            continue
        res[name] = {"waves": int(len(s)),
                     "start_us_mean": float((s[:, 0] - t0).mean() / 100), "start_us_max": float((s[:, 0] - t0).max() / 100),
                     "stage_us": float((s[:, 1] - s[:, 0]).mean() / 100), "gemm1_us": float((s[:, 2] - s[:, 1]).mean() / 100),
                     "tiles_us": float((s[:, 3] - s[:, 2]).mean() / 100), "tiles_us_max": float((s[:, 3] - s[:, 2]).max() / 100),
                     "end_us_max": float((s[:, 3] - t0).max() / 100)}
        c = buf[used][st[:, 4] == flag][:, 5].astype(np.int64)
        tiles_us = (s[:, 3] - s[:, 2]) / 100
        waste = ((c >> 16) & 3) != 0
        res[name].update({"tiles_walked": float((c & 0xFF).mean()), "noise_tiles": float(((c >> 8) & 0xFF).mean()),
                          "noise_on_value_tile": float(((c >> 16) & 1).mean()),
                          "noise_past_o_s": float(((c >> 17) & 1).mean()), "noise_on_either": float(waste.mean()),
                          "tiles_us_noise_on_either": float(tiles_us[waste].mean()) if waste.any() else None,
                          "tiles_us_others": float(tiles_us[~waste].mean()) if (~waste).any() else None,
                          "tiles_walked_noise_on_either": float((c[waste] & 0xFF).mean()) if waste.any() else None,
                          "tiles_walked_others": float((c[~waste] & 0xFF).mean()) if (~waste).any() else None})
    res["span_us"] = float((st[:, 3].max() - t0) / 100)
    out[f"rep{rep}"] = res
print(json.dumps(out))
