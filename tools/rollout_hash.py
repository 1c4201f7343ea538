"""Fingerprint of a C3-style rollout, to compare two builds of libbgx.so (BGX_LIB): one
Philox engine at B = 65,536 (seed 1234), 40 steps from reset with the packed H = 128 policy
sampling the actions (torch seed 0; --linear: set_fork(False) first), then one JSON line
with the sha256 of the lane records, move counts and live moves, of the rewards and dones of
every step, and of order() (perm, classes, counters)."""
import hashlib
import json
import os
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlp-ppo-2ply-p3_amd")]
import bgx  # noqa: E402
from bgx.policy import PolicyNet  # noqa: E402

B, K = 65536, 40
dev = torch.device("cuda", 0)
e = bgx.Engine(batch=B, max_moves=500, seed=1234, dice="philox", auto_reset=True, device=dev)
if "--linear" in sys.argv[1:]:
    e.set_fork(False)
torch.manual_seed(0)
net = PolicyNet(hidden_size=128, action_size=500).to(dev)
net.pack()
act = torch.empty(B, dtype=torch.int32, device=dev)
logp = torch.empty(B, dtype=torch.float32, device=dev)
val = torch.empty(B, dtype=torch.float32, device=dev)
rew = torch.empty(K, B, dtype=torch.float32, device=dev)
done = torch.empty(K, B, dtype=torch.uint8, device=dev)
e.reset(want_obs=False)
for i in range(K):
    net.act(e, seed=4242, step=i, out=(act, logp, val))
    e.step(act, want_obs=False, want_info=False, out=(rew[i], done[i]))
rec, mv, nt = e.lanes()
live = torch.arange(500, device=dev)[None, :] < (rec[:, 60].long() | (rec[:, 61].long() << 8))[:, None]
mv = torch.where(live, mv, 0)
perm, cls, ctr = e.order()
assert e.error() == 0


def sha(*xs):
    h = hashlib.sha256()
    for x in xs:
        h.update((x.cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes())
    return h.hexdigest()[:16]


print(json.dumps({"lanes": sha(rec, nt, mv), "steps": sha(rew, done, act, logp, val), "order": sha(perm, cls, ctr),
                  "dones": int(done.sum())}))
