"""Measurements of the cubeful bearoff table (profiles/cube_bearoff/summary.json):
the table's build time at K = 6 and K = 8 (events on the stream around bgx_bearoff_cube_create)
in both build layouts -- child values read from transposed working copies, the default, and from
the planes themselves (the debug option BGX_BOC_DIRECT) -- beside BearoffDB's own build time, and
`--cube` rollouts from the opening at 65,536 lanes with and without `--cube-bearoff 6`.

    python tools/cube_bearoff_profile.py OUT.json [CHECKPOINT.pt]

Without a checkpoint the net is a fresh H = 128 one, whose value head seldom doubles.  No number
here is a pass condition."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(make):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    obj = make()
    e1.record()
    torch.cuda.synchronize()
    return obj, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    from bgx import rollout
    from bgx._lib import debug_options
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    from bgx.policy import PolicyNet
    out = sys.argv[1]
    doc = {"build": [], "rollouts": [],
           "setup": {"lanes": 65536, "games": 131072, "positions": "opening", "first_roll": "random", "player": "policy",
                     "rule": "CubeRule defaults: scale 1, double_at 0.40, pass_at 0.50, too_good_at inf, cap 6",
                     "checkpoint": sys.argv[2] if len(sys.argv) > 2 else "a fresh H = 128 net",
                     "timed": "rollout.main's seconds (the tables' builds excluded), after a warm-up run"}}

    def emit(key, **kw):
        doc[key].append(kw)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps(kw), flush=True)

    CubefulBearoffDB(BearoffDB(2))                       # module load, first launches
    torch.cuda.synchronize()
    for K in (6, 8, 6, 8):
        db, ms, wall = timed(lambda: BearoffDB(K))
        emit("build", table="cubeless", K=K, n=db.n, stream_ms=ms, wall_ms=wall, table_mb=db.n * db.n * 4 / 2 ** 20)
        cdb, ms, wall = timed(lambda: CubefulBearoffDB(db))
        emit("build", table="cubeful", layout="transposed working copy", K=K, n=db.n, stream_ms=ms, wall_ms=wall,
             table_mb=5 * db.n * db.n * 4 / 2 ** 20, working_mb=3 * db.n * db.n * 4 / 2 ** 20)
        with debug_options(BGX_BOC_DIRECT=1):
            direct, ms, wall = timed(lambda: CubefulBearoffDB(db))
        same = bool(torch.equal(direct.equity().view(torch.int32), cdb.equity().view(torch.int32)) and
                    torch.equal(direct.nd().view(torch.int32), cdb.nd().view(torch.int32)))
        emit("build", table="cubeful", layout="direct (strided child reads)", K=K, n=db.n, stream_ms=ms, wall_ms=wall,
             same_bits_as_transposed=same)
        del cdb, direct, db
    with tempfile.TemporaryDirectory() as d:
        ckpt = sys.argv[2] if len(sys.argv) > 2 else os.path.join(d, "net.pt")
        if len(sys.argv) <= 2:
            torch.manual_seed(0)
            torch.save(PolicyNet(hidden_size=128).state_dict(), ckpt)
        base = ["--net", ckpt, "--positions", "opening", "--seed", "0", "--batch", "65536", "--player", "policy",
                "--trials", "131072", "--first-roll", "random", "--max-steps", "4000", "--cube"]
        cut = ["--cube-bearoff", "6"]
        for name, extra in (("warmup", cut), ("cube", []), ("cube+cut6", cut), ("cube", []), ("cube+cut6", cut)):
            res, summary = rollout.main(base + extra)
            r = res[0]
            emit("rollouts", run=name, games=r["games"], unfinished=r["unfinished"], equity_cubeful=r["equity_cubeful"],
                 equity_cubeful_stderr=r["equity_cubeful_stderr"], pass_share=r["pass_share"],
                 doubles_per_game=r["doubles_per_game"], plies_per_game=r["plies_per_game"],
                 cut_share=r.get("cut_share"), cut_games=r.get("cut_games"), seconds=summary["seconds"],
                 games_per_s=summary["games_per_s"], steps=summary["steps"])


if __name__ == "__main__":
    main()
