"""The HIP runtime calls of the engine's host layer, to compare two builds of libbgx.so.

    rocprofv3 --hip-runtime-trace -f csv json -d OUT -o trace -- python tools/host_call_trace.py run
    python tools/host_call_trace.py seq OUT > calls.txt

`run`: a Philox and a shared-dice engine at B = 256, each: reset, three forked steps,
set_fork(False), three steps, join, order, movegen, set_lanes.  Every tensor is made
before the sequence; three hipDeviceSynchronize in a row mark its begin and its end.
`seq`: the names of the calls between the marks in start order, one per line, with the
stream argument where the trace's JSON carries the arguments (streams numbered by first
appearance).  Run it with each library (BGX_LIB) and diff the two outputs."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    import torch
    sys.path[:0] = [os.path.join(ROOT, "mlp-ppo-2ply-p3_amd")]
    import bgx
    B = 256
    engines = [bgx.Engine(batch=B, max_moves=500, dice=d, seed=5, auto_reset=True) for d in ("philox", "shared")]
    act = torch.zeros(B, dtype=torch.int32, device="cuda")
    rec = torch.zeros(16, 64, dtype=torch.uint8, device="cuda")      # both sides on their ace points, roll 3-1
    rec[:, 23] = 15
    rec[:, 24] = 15
    rec[:, 53] = 3
    rec[:, 54] = 1
    boards, players = rec[:, :52].contiguous().view(torch.int8), rec[:, 52].contiguous()
    dice = rec[:, 53:55].contiguous()
    for _ in range(3):
        torch.cuda.synchronize()
    for e in engines:
        e.reset(want_obs=False)
        for _ in range(3):
            e.step(act, want_obs=False)
        e.set_fork(False)
        for _ in range(3):
            e.step(act, want_obs=False)
        e.join()
        e.order() if e.dice == "philox" else None
        e.movegen(boards, players, dice)
        e.set_lanes(rec[:8])
    for _ in range(3):
        torch.cuda.synchronize()
    assert all(e.error() == 0 for e in engines)


def seq(out_dir):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*hip_api_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    main = max({r["Thread_Id"] for r in rows}, key=lambda t: sum(r["Thread_Id"] == t for r in rows))
    rows = sorted((r for r in rows if r["Thread_Id"] == main), key=lambda r: int(r["Start_Timestamp"]))
    streams = {}                                           # correlation id -> stream argument
    for f in glob.glob(os.path.join(out_dir, "**", "*results.json"), recursive=True):
        for rs in json.load(open(f)).get("rocprofiler-sdk-tool", []):
            for r in rs["buffer_records"]["hip_api"]:
                for a in r.get("args") or []:
                    if a["name"] == "stream":
                        streams[str(r["correlation_id"]["internal"])] = a["value"]
    # the marks: three hipDeviceSynchronize with nothing but device getters / setters between
    idx = [i for i, r in enumerate(rows) if r["Function"] not in ("hipGetDevice", "hipSetDevice", "hipGetLastError")]
    marks = [k for k in range(len(idx) - 2) if all(rows[idx[k + j]]["Function"] == "hipDeviceSynchronize" for j in range(3))]
    lo, hi = idx[marks[0] + 2] + 1, idx[marks[-1]]
    seen = {}
    for r in rows[lo:hi]:
        s = streams.get(r["Correlation_Id"])
        print(r["Function"] + (f" s{seen.setdefault(s, len(seen))}" if s is not None else ""))


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else seq(sys.argv[2])
