"""Rollout.run_lanes / run after the rollout loop became one loop over stages, and after the cut
kernels, the horizon stages, the host replays and the summaries became one skeleton each
(bgx/rollout.py, bgx/tally.py, csrc/bg_rollout.h; DESIGN.md "Start positions and rollouts"):
every mode computes exactly what the commit before the change computed.  The file was recorded
before the second change; its entries for the first eight modes equal, key by key, those recorded
before the first.  "cube_bearoff_truncate" is cube + cube_bearoff + cube_truncate.

tests/golden/rollout_modes.npz was recorded from the parent commit's library AND package
(tools/record_rollout_modes.py, which runs `run_mode` below on that tree, never on the tree
under test).  Per mode it holds every tally, `unfinished`, `games_done`, `active`, the step
count and the length of the result tuple in full, the SHA-256 of every trace field (dtype, shape
and bytes; NaN fills come from the same expressions, so their bits are stable) and the result
dicts of one Rollout.run call (2 positions, stratified first rolls, one pass).

The runs: 128 lanes (two waves), Philox dice, RandomPlayer, 2 games a lane, 3 groups of 40, 45
and 38 lanes with 5 idle lanes among them, so wave 0 holds two groups and group 1 spans both
waves.  Starts: group 0 the opening (long games), groups 1 and 2 both sides home with 3..8
checkers (some inside the K = 6 table and, in the cubeful mode, the K = 3 table at the start:
the cut after begin fires; "cube_bearoff_truncate" uses the cubeful mode's starts), every tenth
lane a one-checker mover against 15 checkers in their home board (a gammon).  Value head, cube
rule, horizon and tables are those of the GPU tests of each mode."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_modes.npz")
MODES = ("plain", "luck", "bearoff", "bearoff1", "cube", "cube_bearoff", "truncate", "truncate_luck", "cube_truncate",
         "cube_bearoff_truncate")
B, P, G = 128, 3, 2
MAX_STEPS = 8000
ROLLOUT_SEED, PLAYER_SEED = 5, 2
HORIZON = 8
# the cubeful truncation's horizons (a CubeTruncation on the same value head), chosen so that on
# the recording commit truncated and naturally finished games both occur in "cube_truncate", a
# table cut fires beside the truncation in "cube_bearoff_truncate" (whose starts are all short
# races), and in each a lane's last game ends in the truncation kernel
CUBE_HORIZON = 8
CUBE_BEAROFF_HORIZON = 3
CUBE_RULE = dict(double_at=0.13, pass_at=0.19, cap=4)        # test_gpu_cube.py's traced rule


def groups():
    g = np.repeat(np.arange(3), [40, 45, 38]).astype(np.int32)
    for k in (7, 30, 63, 64, 100):                            # idle lanes, two at the wave boundary
        g = np.insert(g, k, -1)
    assert len(g) == B
    return g


def home_record(c1, c2, mover, roll=(0, 0)):
    """uint8[64]: PLAYER1 with c1[d - 1] checkers at distance d (point 24 - d), PLAYER2 with c2
    (point d - 1), the rest of each side's 15 checkers off."""
    r = np.zeros(64, np.uint8)
    for d in range(1, 7):
        r[24 - d], r[24 + d - 1] = c1[d - 1], c2[d - 1]
    r[50], r[51], r[52] = 15 - sum(c1), 15 - sum(c2), mover
    r[53], r[54] = roll
    return r


def starts_for(mode):
    from bgx.rollout import opening_record
    lo = 3 if "cube_bearoff" in mode else 5                   # the K = 3 table needs <= 3 checkers a side
    hi = 6 if "cube_bearoff" in mode else 9
    rng = np.random.RandomState(21)
    group = groups()
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        c = [tuple(np.bincount(rng.randint(0, 6, rng.randint(lo, hi)), minlength=6)) for _ in range(2)]
        roll = (rng.randint(1, 7), rng.randint(1, 7)) if i % 2 else (0, 0)
        mover = rng.randint(2)
        if i % 10 == 3:
            c[mover], c[1 - mover] = (1, 0, 0, 0, 0, 0), (3, 3, 3, 2, 2, 2)
        s[i] = home_record(c[0], c[1], mover, roll)
        if group[i] == 0 and "cube_bearoff" not in mode:
            s[i] = opening_record().numpy()
            s[i, 52] = i & 1
    return s


def run_positions():
    return np.stack([home_record((0, 0, 0, 2, 2, 2), (0, 0, 0, 2, 2, 2), 0),
                     home_record((1, 2, 1, 2, 1, 1), (2, 1, 1, 1, 1, 1), 1)])


def by_lane(n):
    """test_gpu_cube_bearoff.py's callable equity: a take, a pass or no double by the lane."""
    import torch
    e = torch.tensor([0.45, 0.9, -1.0, 0.45, -1.0], dtype=torch.float32).repeat(n // 5 + 1)[:n].cuda().contiguous()
    return lambda eng, dsel: e


def mode_kwargs(mode, group):
    """run_lanes' keyword arguments of a mode (cube0 by the lane's group) and those of run."""
    import torch
    from bgx.bearoff import BearoffDB, CubefulBearoffDB, OneSidedBearoffDB
    from bgx.cube import CubeRule, CubeTruncation, pack
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead
    from bgx.truncate import Truncation
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    cube0 = torch.from_numpy(np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)])
    kw = {"plain": {}, "luck": dict(luck=vh),
          "bearoff": lambda: dict(bearoff=BearoffDB(6)),
          "bearoff1": lambda: dict(bearoff=OneSidedBearoffDB(15)),
          "cube": lambda: dict(cube=CubeRule(vh, jacoby=True, **CUBE_RULE)),
          "cube_bearoff": lambda: dict(cube=CubeRule(by_lane(B), cap=4), cube_bearoff=CubefulBearoffDB(BearoffDB(3))),
          "truncate": dict(truncate=Truncation(vh, HORIZON)),
          "truncate_luck": dict(truncate=Truncation(vh, HORIZON), luck=vh),
          "cube_truncate": lambda: dict(cube=CubeRule(vh, jacoby=True, **CUBE_RULE),
                                        cube_truncate=CubeTruncation(vh, CUBE_HORIZON)),
          "cube_bearoff_truncate": lambda: dict(cube=CubeRule(by_lane(B), cap=4),
                                                cube_bearoff=CubefulBearoffDB(BearoffDB(3)),
                                                cube_truncate=CubeTruncation(vh, CUBE_BEAROFF_HORIZON))}[mode]
    kw = kw() if callable(kw) else kw
    lanes = dict(kw, cube0=cube0) if "cube" in kw else kw
    run = dict(kw, cube_start=[(0, 0), (1, 2)]) if "cube" in kw else kw
    return lanes, run


def run_mode(mode):
    """(run_lanes' result tuple with trace=True, run's result dicts, group) from the loaded package."""
    import torch
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    group = groups()
    lanes_kw, run_kw = mode_kwargs(mode, group)
    ro = Rollout(B, seed=ROLLOUT_SEED)
    out = ro.run_lanes(RandomPlayer(PLAYER_SEED), torch.from_numpy(starts_for(mode)), torch.from_numpy(group), P, G,
                       max_steps=MAX_STEPS, trace=True, **lanes_kw)
    assert ro.eng.error() == 0
    ro2 = Rollout(B, seed=ROLLOUT_SEED + 1)
    res = ro2.run(RandomPlayer(PLAYER_SEED + 1), torch.from_numpy(run_positions()), 36, max_steps=MAX_STEPS, **run_kw)
    assert ro2.eng.error() == 0
    return out, res, group


def sha(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def digest(mode, out, res):
    """What is stored of a mode, under 'mode.name' keys."""
    tr = out[2]
    d = {"n_results": np.int64(len(out)), "unfinished": out[1].cpu().numpy(), "games_done": tr["games_done"].cpu().numpy(),
         "active": np.int64(tr["active"]), "steps": np.int64(tr["done"].shape[0]), "run": np.str_(json.dumps(res, sort_keys=True))}
    for j in [0] + list(range(3, len(out))):
        d[f"tally{j}"] = out[j].cpu().numpy()
    for k, v in tr.items():
        if k not in ("games_done", "active"):
            d[f"sha.{k}"] = np.str_(sha(v))
    return {f"{mode}.{k}": v for k, v in d.items()}


@pytest.fixture(scope="module")
def want():
    return dict(np.load(GOLDEN_NPZ))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_mode_equals_the_parent(want, mode):
    """Integers and digests equal, the result dicts equal with floats compared by ==, the set of
    trace keys and the length of the result tuple the recorded ones."""
    out, res, _ = run_mode(mode)
    got = digest(mode, out, res)
    assert sorted(got) == sorted(k for k in want if k.split(".")[0] == mode), (mode, sorted(got))
    for k, v in got.items():
        if k.endswith(".run"):
            ref = json.loads(str(want[k]))
            assert len(res) == len(ref), k
            for p, (a, b) in enumerate(zip(res, ref)):
                assert sorted(a) == sorted(b), (k, p)
                for f in a:
                    assert type(a[f]) is type(b[f]) and a[f] == b[f], (k, p, f, a[f], b[f])
        elif k.split(".")[1] == "sha":
            assert str(v) == str(want[k]), k
        else:
            assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), (k, v.tolist(), want[k].tolist())


def test_mode_list_is_the_recorded_one(want):
    assert sorted(MODES) == sorted({k.split(".")[0] for k in want})
    for mode in MODES:
        assert not want[f"{mode}.unfinished"].any() and want[f"{mode}.active"] == 0, mode
