"""Measurements of the bearoff database (profiles/bearoff/summary.json): the
table's build time at K = 6 and K = 8 (events on the stream around bgx_bearoff_create), and
rollouts from the opening at 65,536 lanes with a fresh H = 128 net -- the policy player with
and without the cut, the 2-ply top-4 player plain, with the table's player, and with both.

    python tools/bearoff_profile.py OUT.jsonl

One JSON line per measurement, appended as it is taken."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    from bgx import rollout
    from bgx.bearoff import BearoffDB
    from bgx.policy import PolicyNet
    out = sys.argv[1]
    open(out, "w").close()

    def emit(**kw):
        with open(out, "a") as f:
            f.write(json.dumps(kw) + "\n")
        print(json.dumps(kw), flush=True)

    BearoffDB(2)                                         # module load, first launches
    torch.cuda.synchronize()
    for K in (6, 8, 6, 8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        db = BearoffDB(K)
        e1.record()
        torch.cuda.synchronize()
        emit(what="build", K=K, n=db.n, stream_ms=e0.elapsed_time(e1), wall_ms=(time.perf_counter() - t0) * 1e3,
             succ_entries=int(db._succ_off[-1]), table_mb=db.n * db.n * 4 / 2 ** 20)
        del db
    torch.manual_seed(0)
    net = PolicyNet(hidden_size=128)
    with tempfile.TemporaryDirectory() as d:
        ckpt = os.path.join(d, "net.pt")
        torch.save(net.state_dict(), ckpt)
        base = ["--net", ckpt, "--positions", "opening", "--seed", "0", "--batch", "65536"]
        policy = ["--player", "policy", "--trials", "131040", "--max-steps", "4000"]
        two_ply = ["--player", "2ply", "--top-k", "4", "--trials", "65520", "--max-steps", "1500"]
        # the first rollout of a process pays its one-off work (first launches, first torch ops):
        # a warm-up run, then each pair twice
        runs = [("warmup", policy + ["--bearoff", "6"]),
                ("policy", policy), ("policy+cut6", policy + ["--bearoff", "6"]),
                ("policy", policy), ("policy+cut6", policy + ["--bearoff", "6"]),
                ("2ply_top4", two_ply), ("2ply_top4+play6", two_ply + ["--bearoff-play", "6"]),
                ("2ply_top4+play6+cut6", two_ply + ["--bearoff-play", "6", "--bearoff", "6"]),
                ("2ply_top4", two_ply), ("2ply_top4+play6", two_ply + ["--bearoff-play", "6"])]
        for name, extra in runs:
            res, summary = rollout.main(base + extra)
            r = res[0]
            emit(what="rollout", run=name, games=r["games"], unfinished=r["unfinished"], equity=r["equity"],
                 equity_stderr=r["equity_stderr"], plies_per_game=r["plies_per_game"],
                 cut_share=r.get("cut_share"), cut_games=r.get("cut_games"), seconds=summary["seconds"],
                 games_per_s=summary["games_per_s"], env_steps_per_s=summary["env_steps_per_s"], steps=summary["steps"],
                 batch=summary["batch"], trials=summary["trials"], max_steps=summary["max_steps"])


if __name__ == "__main__":
    main()
