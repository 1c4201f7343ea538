"""Measurements of the one-sided bearoff database (profiles/bearoff1/summary.json):
the table's build time at K = 6, 8 and 15 (events on the stream around bgx_bearoff1_create),
its distance to the exact table at K = 5 and 6, and the §11 policy-player rollout from the
opening at 65,536 lanes with a fresh H = 128 net -- plain, with --bearoff 6 and with
--bearoff1 15, alternated in one process.

    python tools/bearoff1_profile.py OUT.jsonl

One JSON line per measurement, appended as it is taken."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from bgx import rollout
    from bgx.bearoff import BearoffDB, OneSidedBearoffDB
    from bgx.policy import PolicyNet
    out = sys.argv[1]
    open(out, "w").close()

    def emit(**kw):
        with open(out, "a") as f:
            f.write(json.dumps(kw) + "\n")
        print(json.dumps(kw), flush=True)

    OneSidedBearoffDB(2)                                 # module load, first launches
    torch.cuda.synchronize()
    for K in (6, 8, 15, 6, 8, 15):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        db = OneSidedBearoffDB(K)
        e1.record()
        torch.cuda.synchronize()
        dist = db.dist().cpu().numpy()
        sums = dist.astype(np.float64).sum(1)
        emit(what="build", K=K, n=db.n, stream_ms=e0.elapsed_time(e1), wall_ms=(time.perf_counter() - t0) * 1e3,
             table_mb=db.n * 32 * 4 / 2 ** 20, last_t=int(np.nonzero(dist.any(0))[0].max()),
             row_sum_min=float(sums.min()), row_sum_max=float(sums.max()),
             mean_all_on_six=float(db.mean()[db.index_of((0, 0, 0, 0, 0, K))]))
        del db
    for K in (5, 6):                                     # win1 against the exact table, every pair
        one, two = OneSidedBearoffDB(K), BearoffDB(K)
        cfg = two.configs().cpu().numpy()
        n = two.n
        recs = np.zeros((n - 1, n - 1, 64), np.uint8)
        recs[:, :, 23:17:-1] = cfg[1:, None, :]
        recs[:, :, 24:30] = cfg[None, 1:, :]
        recs[:, :, 50] = 15 - cfg[1:].sum(1)[:, None]
        recs[:, :, 51] = 15 - cfg[1:].sum(1)[None, :]
        _, win = one.lookup(torch.from_numpy(recs.reshape(-1, 64)).to(one.device))
        d = win.cpu().numpy().reshape(n - 1, n - 1).astype(np.float64) - two.table().cpu().numpy()[1:, 1:]
        emit(what="distance", K=K, pairs=int(d.size), max_abs=float(np.abs(d).max()), mean_abs=float(np.abs(d).mean()),
             min=float(d.min()), max=float(d.max()))
        del one, two
    torch.manual_seed(0)
    net = PolicyNet(hidden_size=128)
    with tempfile.TemporaryDirectory() as d:
        ckpt = os.path.join(d, "net.pt")
        torch.save(net.state_dict(), ckpt)
        policy = ["--net", ckpt, "--positions", "opening", "--seed", "0", "--batch", "65536", "--player", "policy",
                  "--trials", "131040", "--max-steps", "4000"]
        # the first rollout of a process pays its one-off work: a warm-up run, then each kind three times
        kinds = [("policy", []), ("policy+cut6", ["--bearoff", "6"]), ("policy+cut1_15", ["--bearoff1", "15"])]
        for name, extra in [("warmup", ["--bearoff1", "15"])] + kinds * 3:
            res, summary = rollout.main(policy + extra)
            r = res[0]
            emit(what="rollout", run=name, games=r["games"], unfinished=r["unfinished"], equity=r["equity"],
                 equity_stderr=r["equity_stderr"], plies_per_game=r["plies_per_game"],
                 cut_share=r.get("cut_share"), cut_games=r.get("cut_games"), seconds=summary["seconds"],
                 games_per_s=summary["games_per_s"], env_steps_per_s=summary["env_steps_per_s"], steps=summary["steps"],
                 batch=summary["batch"], trials=summary["trials"], max_steps=summary["max_steps"])


if __name__ == "__main__":
    main()
