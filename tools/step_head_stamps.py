"""Head-of-wave stamp of the env step: per wave, ticks (100 MHz) from the wave's
start to "move applied" and to its end, split into the heavy and the light launch.
A scratch build with profiles/step_block/stamp_head.patch applied packs both into the
second stamp word.  usage: BGX_LIB=that_build.so python tools/step_head_stamps.py OUT.json"""
import ctypes, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")]
import numpy as np, torch, bgx
from bgx._lib import debug_option
debug_option("BGX_STAMPS", 1)            # read at engine creation
from bgx.policy import PolicyNet
B = 16384                                # one shard of the headline workload
eng = bgx.Engine(batch=B, dice="philox", seed=5)
net = PolicyNet().cuda(); net.pack()
eng.reset(want_obs=False)
for i in range(160):
    rec = eng.records(); a, _, _ = net.act(rec, seed=1, step=i); eng.step(a, want_obs=False, want_info=False)
L = eng._lib; L.bgx_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
g = B / 6.0 + 4.0 * math.sqrt(B * 5.0 / 36.0) + 32.0
heavy = (int(g) + 7) & ~7
res = {"B": B, "heavy_grid": heavy, "steps": []}
acc = {"light": [], "heavy": []}
for k in range(8):
    rec = eng.records(); a, _, _ = net.act(rec, seed=1, step=1000 + k)
    perm, _, _ = eng.order()
    eng.step(a, want_obs=False, want_info=False)
    st = np.zeros((B, 2), np.uint64)
    assert L.bgx_debug_stamps(eng._h, st.ctypes.data_as(ctypes.c_void_p)) == 0
    head = (st[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tot = (st[:, 1] >> np.uint64(32)).astype(np.int64)
    hv = np.zeros(B, bool); hv[perm[:heavy]] = True
    dn = rec.cpu().numpy()[:, 55] != 0
    ok = ~dn
    for name, m in (("heavy", hv & ok), ("light", ~hv & ok)):
        acc[name].append((head[m], tot[m]))
for name, v in acc.items():
    h = np.concatenate([x[0] for x in v]) / 100.0
    t = np.concatenate([x[1] for x in v]) / 100.0
    res[name] = {"waves": int(len(h)), "head_us_mean": float(h.mean()), "head_us_median": float(np.median(h)),
                 "head_us_p10": float(np.percentile(h, 10)), "head_us_p90": float(np.percentile(h, 90)),
                 "life_us_mean": float(t.mean()), "life_us_median": float(np.median(t))}
    print(name, res[name])
del res["steps"]
json.dump(res, open(sys.argv[1], "w"), indent=1)
