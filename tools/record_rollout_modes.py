"""Record tests/golden/rollout_modes.npz: what tests/test_gpu_rollout_modes.py expects, from the
library AND the bgx package of the commit BEFORE a change to the rollout loop or its kernels
(never from the tree under test):

    git worktree add ../parent HEAD~1 && (cd ../parent && python __graft_entry__.py)
    python tools/record_rollout_modes.py ../parent [OUT.npz]

The runs are `run_mode` of this tree's test module, on the parent's package.  Before writing,
the recorder checks that the parent finished every game of every mode and that each mode
actually fired: a cut (one of them after begin), a double and a pass, a truncation (cubeless or
cubeful), a nonzero luck sum, and a lane whose last game ended in a cut / decide / truncation kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "mlp-ppo-2ply-p3_amd"


def retired_in(tr, group, G, first, before, after, only=None):
    """Lanes whose G-th game ended in a kernel other than advance: `first` the trace key of the
    mask after begin (or None), `before` the per-step mask before the step, `after` the masks
    after advance (one key or several, in the stages' order); `only`: count the lanes retired by
    that mask alone.  Replays the counting: masks fire on active lanes only, a natural end is a
    done with a winner on an active lane."""
    games = np.zeros(len(group), np.int64)
    hit = np.zeros(len(group), bool)
    valid = group >= 0

    def end(m, key=None):
        m = m & valid & (games < G)
        games[m] += 1
        return m & (games >= G) & (only is None or key == only)
    after = (after,) if isinstance(after, str) else tuple(after or ())
    if first:
        hit |= end(tr[first].cpu().numpy() != 0, first)
    done, info = tr["done"].cpu().numpy(), tr["info"].cpu().numpy().astype(np.int64)
    masks = {k: tr[k].cpu().numpy() != 0 for k in (before,) + after if k}
    for t in range(done.shape[0]):
        if before:
            hit |= end(masks[before][t], before)
        end((done[t] != 0) & (((info[t] >> 8) & 0xFF) > 0))
        for k in after:
            hit |= end(masks[k][t], k)
    assert np.array_equal(games[valid], np.full(valid.sum(), G)), "the replay lost a game"
    return hit


def check_fired(mode, out, res, group, G):
    from bgx.cube import CUBE_FIELDS
    tr = out[2]
    assert not out[1].any() and tr["active"] == 0, f"{mode}: the parent left games unfinished"
    assert all(np.isfinite(v) for r in res for v in r.values() if isinstance(v, float)), f"{mode}: a NaN result"
    assert all(r["unfinished"] == 0 and r["games"] == 36 for r in res), mode
    fired = {}
    if "luck" in mode:
        fired["luck"] = bool(out[3][:, 0].any())
    tmask = "ctrunc" if "cube" in mode else "trunc"          # the horizon cut's mask, where the mode has one
    if "bearoff" in mode:
        cut_tally = out[4] if "truncate" in mode else out[-1]
        fired["cut"] = bool(cut_tally[:, 0].sum() > 0) and bool(tr["cut"].any())
        fired["cut0"] = bool(tr["cut0"].any())
        after = ("cut", tmask) if "truncate" in mode else "cut"
        fired["retired"] = bool(retired_in(tr, group, G, "cut0", "cube_mask" if "cube" in mode else None, after).any())
    if "cube" in mode:
        ct = out[3].cpu().numpy()
        fired["double"] = bool(ct[:, CUBE_FIELDS.index("doubles")].sum() > ct[:, CUBE_FIELDS.index("pass_games")].sum())
        fired["pass"] = bool(ct[:, CUBE_FIELDS.index("pass_games")].sum() > 0)
    if mode == "cube":
        fired["retired"] = bool(retired_in(tr, group, G, None, "cube_mask", None).any())
    if "truncate" in mode:
        fired["trunc"] = bool(out[-1][:, 0].sum() > 0) and bool(tr[tmask].any())
        fired["natural"] = bool(out[0][:, 0].sum() > 0)         # beside them, games played to the end
        fired["retired_trunc"] = bool(retired_in(tr, group, G, "cut0" if "bearoff" in mode else None,
                                                 "cube_mask" if "cube" in mode else None,
                                                 ("cut", tmask) if "bearoff" in mode else tmask, only=tmask).any())
    assert all(fired.values()), f"{mode}: did not fire: {fired}"
    return fired


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    parent = os.path.realpath(sys.argv[1])
    if parent == os.path.realpath(ROOT) or not os.path.isdir(os.path.join(parent, PKG, "bgx")):
        raise SystemExit("give the PARENT commit's built tree: the tree under test records nothing")
    os.environ["BGX_LIB"] = os.path.join(parent, PKG, "bgx", "libbgx.so")
    sys.path[:0] = [os.path.join(parent, PKG), os.path.join(ROOT, "tests")]
    import bgx
    import test_gpu_rollout_modes as T
    assert os.path.realpath(bgx.__file__).startswith(parent + os.sep), bgx.__file__
    out_path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN_NPZ
    arrays = {}
    for mode in T.MODES:
        out, res, group = T.run_mode(mode)
        fired = check_fired(mode, out, res, group, T.G)
        arrays.update(T.digest(mode, out, res))
        print(mode, "steps", int(out[2]["done"].shape[0]), "tallies", [o.sum(0).tolist() for o in (out[0],) + out[3:]], fired)
    np.savez_compressed(out_path, **arrays)
    print(out_path, len(arrays), "arrays", os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
