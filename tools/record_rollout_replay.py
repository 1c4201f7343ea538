"""Record tests/golden/rollout_replay.npz: what tests/test_rollout_replay_cpu.py expects, from the
bgx package of the commit BEFORE a change to the host replays or the summaries (never from the
tree under test).  No GPU and no library are needed:

    git worktree add ../parent HEAD~1
    python tools/record_rollout_replay.py ../parent [OUT.npz]

The runs are `compute` of this tree's test module, on the parent's package.  Before writing, the
recorder checks that on the parent every tally of every reference (games_per_lane 1 and 3) has
games in at least two groups, and that the luck, cut, pass, double and truncation paths fired."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "mlp-ppo-2ply-p3_amd"
# the field that counts a tally's games, where it is not field 0
GAMES_FIELD = {"luck_tally": 3, "value": 3}


def check_fired(T, refs):
    """AssertionError unless the parent's results exercise every path of the replays."""
    fired = dict.fromkeys(("luck", "cut", "pass", "double", "trunc"), False)
    for name, res in refs.items():
        res = res if isinstance(res, dict) else {"value": res}
        G = int(name.split(".")[1][1:])
        for k, v in res.items():
            if v is None or not (k == "value" or k.endswith("tally")):
                continue
            games = v[:, GAMES_FIELD.get(k, 0)]
            if G == 0:                          # nothing is scheduled; the single call takes sel as it is given
                assert name.startswith("cube_bearoff_call") or not v.any(), f"{name}.{k}: games_per_lane 0 counted"
                continue
            assert (games != 0).sum() >= 2, f"{name}.{k}: games in fewer than two groups: {games.tolist()}"
            if k in ("luck_tally", "value"):
                fired["luck"] |= bool(v[:, 0].any() and v[:, 2].any())
            fired["cut"] |= k == "cut_tally"
            fired["trunc"] |= k in ("trunc_tally", "cube_trunc_tally")
            if k == "cube_tally":
                fired["pass"] |= bool(v[:, 4].sum() > 0)
                fired["double"] |= bool(v[:, 7].sum() > v[:, 4].sum())
        if name.startswith("truncate_luck.G3"):
            assert res["trunc_tally"][:, 4].any() and res["trunc_tally"][:, 6].any(), f"{name}: no luck in a truncated game"
    assert all(fired.values()), f"did not fire: {fired}"
    return fired


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    parent = os.path.realpath(sys.argv[1])
    if parent == os.path.realpath(ROOT) or not os.path.isdir(os.path.join(parent, PKG, "bgx")):
        raise SystemExit("give the PARENT commit's tree: the tree under test records nothing")
    sys.path[:0] = [os.path.join(parent, PKG), os.path.join(ROOT, "tests")]
    import bgx
    import test_rollout_replay_cpu as T
    assert os.path.realpath(bgx.__file__).startswith(parent + os.sep), bgx.__file__
    out_path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN_NPZ
    refs = T.references()
    print(check_fired(T, refs))
    for name, res in refs.items():
        print(name, {k: v.sum(0).tolist() for k, v in (res if isinstance(res, dict) else {"value": res}).items()
                     if v is not None and (k == "value" or k.endswith("tally"))})
    arrays = T.compute()
    assert all(len(v) >= 200 for v in T.summaries().values())
    np.savez_compressed(out_path, **arrays)
    print(out_path, len(arrays), "arrays", os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
