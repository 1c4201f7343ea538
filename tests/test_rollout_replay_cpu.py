"""The host replays of position rollouts (bgx/replay.py and the six *_reference functions that
drive it) and the eight summarize* functions (bgx/tally.py) compute exactly what the commit
before they were unified computed.

tests/golden/rollout_replay.npz was recorded from the parent commit's package
(tools/record_rollout_replay.py, which runs `compute` below on that tree, never on the tree
under test; no GPU and no library are needed).  The inputs are seeded and synthetic, not traces
of real games: 96 lanes, 60 steps, 3 groups, with idle lanes (-1) and lanes out of range (>= P),
games_per_lane 0, 1 and 3, dones without a winner, scores outside 1..3, NaN / +-inf / values
beyond the clamps / exact .5 ties of the fixed point among the luck and the values, cube bytes
above the cap, the Jacoby rule on and off, and table lookups derived from a record byte.  Stored:
every tally and per-lane result in full, the SHA-256 of every per-step array, and the result
dicts of the summaries on 200 seeded rows each (n = 0, n = 1, all-equal results and
summarize_cube_truncated's cut_row= form among them) as JSON."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_replay.npz")
B, T, P = 96, 60, 3
GAMES = (0, 1, 3)
HORIZON, CAP = 4, 4
N_ROWS = 200
R_CUR, R_ROLL0 = 52, 53


# ---------------------------------------------------------------------------- the inputs --
def special_floats(rng, x, ties_one):
    """x with NaN, +-inf, values beyond every clamp and exact .5 ties of a 1 / ties_one fixed
    point scattered over it."""
    x = x.astype(np.float32)
    kind = rng.randint(0, 40, x.shape)
    x[kind == 0] = np.nan
    x[kind == 1] = np.inf
    x[kind == 2] = -np.inf
    x[kind == 3] = 1000.0
    x[kind == 4] = -1000.0
    tie = (2 * rng.randint(-3 * ties_one // 2, 3 * ties_one // 2, x.shape) + 1) / np.float32(2 * ties_one)
    return np.where((kind >= 5) & (kind < 10), tie.astype(np.float32), x).astype(np.float32)


def inputs():
    rng = np.random.RandomState(1234)
    group = rng.randint(0, P, B).astype(np.int32)
    group[rng.choice(B, 8, replace=False)] = -1
    group[[5, 50, 77]] = (P, P + 4, 2 ** 20)
    starts = rng.randint(0, 16, (B, 64)).astype(np.uint8)
    starts[:, R_CUR] = rng.randint(0, 2, B)
    starts[:, R_ROLL0] = np.where(rng.rand(B) < 0.5, 0, rng.randint(1, 7, B))
    done = (rng.rand(T, B) < 0.25).astype(np.uint8) * rng.randint(1, 3, (T, B)).astype(np.uint8)
    # info: bits 8-15 the winner + 1 (0 = none, 3 = neither side), bits 16-23 the score (0..5), noise around them
    info = (rng.randint(0, 256, (T, B)) | (rng.choice([0, 1, 2, 3], (T, B), p=[.2, .38, .38, .04]) << 8) |
            (rng.randint(0, 6, (T, B)) << 16) | (rng.randint(0, 128, (T, B)) << 24)).astype(np.int32)
    mover = rng.randint(0, 2, (T, B)).astype(np.uint8)
    luck = special_floats(rng, rng.randn(T, B) * 0.3, 65536)
    # a game of one step whose luck is a tie on its own: lanes with a free first roll end games at steps 0, 1 and 2
    for i in np.nonzero((group >= 0) & (group < P))[0][:12]:
        starts[i, R_ROLL0] = 0
        done[:3, i] = 1
        info[:3, i] = (1 + (i & 1)) << 8 | 1 << 16
        luck[:3, i] = (2 * rng.randint(-70000, 70000, 3) + 1) / np.float32(131072)
    tr = dict(mover=mover, done=done, info=info, luck=luck,
              trunc_value=special_floats(rng, rng.uniform(-1.5, 1.5, (T, B)), 65536),
              trunc_mover=rng.randint(0, 2, (T, B)).astype(np.uint8),
              cube_mover=rng.randint(0, 2, (T, B)).astype(np.uint8),
              cube_equity=special_floats(rng, rng.uniform(-0.3, 0.7, (T, B)), 65536),
              ctrunc_value=special_floats(rng, rng.uniform(-1.5, 1.5, (T, B)), 65536),
              ctrunc_mover=rng.randint(0, 2, (T, B)).astype(np.uint8),
              cut_records0=rng.randint(0, 256, (B, 64)).astype(np.uint8),
              cut_records=rng.randint(0, 256, (T, B, 64)).astype(np.uint8))
    tr["cut_records0"][:, R_CUR] &= 1
    tr["cut_records"][:, :, R_CUR] &= 1
    cube0 = rng.choice([0, 0x11, 0x21, 0x12, 0x24, 0x1F, 0x3A, 0x30, 0x08], B).astype(np.uint8)   # some above the cap, owner 3
    return dict(group=group, starts=starts, trace=tr, cube0=cube0)


def lookup(recs):
    """A table's test and win probability from record bytes: in the table one time in three; w
    a multiple of 1/255, an exact tie of the 2^-20 fixed point, or a value outside [0, 1]."""
    recs = np.asarray(recs)
    b = recs[:, 9].astype(np.float32)
    w = np.where(recs[:, 8] & 1, (2 * b + 1) / np.float32(1 << 21), b / np.float32(255))
    w = np.where(recs[:, 8] % 16 == 4, np.float32(1.5), np.where(recs[:, 8] % 16 == 6, np.float32(-0.25), w))
    return recs[:, 7] % 3 == 0, w.astype(np.float32)


def cube_lookup(recs, cube, cap):
    """cube_bearoff_cut_reference's `lookup` from record bytes: values f32[B, 4] with NaN, ties
    and values beyond +-1 among them."""
    recs = np.asarray(recs)
    in_db, w = lookup(recs)
    v = np.stack([2 * w - 1, 4 * w - 2, (recs[:, 10].astype(np.float32) - 128) / np.float32(100), 2 * w - 1], axis=1)
    v = v.astype(np.float32)
    v[recs[:, 11] % 16 == 0] = np.nan
    v[recs[:, 11] % 16 == 1, 2] = (2 * recs[recs[:, 11] % 16 == 1, 12].astype(np.float32) + 1) / np.float32(1 << 21)
    return in_db, v, np.zeros(len(recs), np.uint8)


# ---------------------------------------------------------------------- the six replays --
def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def digest(prefix, res):
    """What is stored of a reference's result: per-step arrays as SHA-256, the rest in full."""
    if not isinstance(res, dict):
        res = {"value": res}
    out = {}
    for k, v in res.items():
        if v is None:
            out[f"{prefix}.{k}"] = np.str_("None")
        elif isinstance(v, np.ndarray) and v.shape[:2] == (T, B):
            out[f"{prefix}.sha.{k}"] = np.str_(sha(v))
        else:
            out[f"{prefix}.{k}"] = np.asarray(v)
    return out


def references():
    """{name: result} of every reference on the inputs, for every games_per_lane."""
    from bgx.cube import (CubeLife, CubeRule, CubeTruncation, cube_bearoff_cut_reference, cube_reference,
                          cube_trunc_reference)
    from bgx.rollout import bearoff_cut_reference, luck_tally_reference
    from bgx.truncate import Truncation, truncate_reference

    def value(eng, sel):
        raise AssertionError("the replay calls no value")
    x = inputs()
    tr, starts, group, cube0 = x["trace"], x["starts"], x["group"], x["cube0"]
    no_luck = {k: v for k, v in tr.items() if k != "luck"}
    out = {}
    with np.errstate(all="ignore"):
        for G in GAMES:
            out[f"luck.G{G}"] = luck_tally_reference(tr["luck"], tr["mover"], tr["done"], tr["info"], starts, group, P, G)
            out[f"bearoff.G{G}"] = bearoff_cut_reference(tr["cut_records0"], tr["cut_records"], tr["done"], tr["info"],
                                                         starts, group, P, G, lookup=lookup)
            trunc = Truncation(value, HORIZON, scale=1.25)
            out[f"truncate.G{G}"] = truncate_reference(no_luck, starts, group, P, G, trunc)
            out[f"truncate_luck.G{G}"] = truncate_reference(tr, starts, group, P, G, trunc)
            for jacoby in (False, True):
                rule = CubeRule(value, scale=1.0, double_at=0.2, pass_at=0.45, too_good_at=0.65, cap=CAP, jacoby=jacoby)
                ct = CubeTruncation(value, HORIZON, scale=0.75, life=CubeLife(0.68, 1.4, 1.2))
                j = f"G{G}.j{int(jacoby)}"
                out[f"cube.{j}"] = cube_reference(tr, starts, group, P, G, rule, cube0=cube0)
                out[f"cube_none.{j}"] = cube_reference(tr, starts, group, P, G, rule)
                out[f"cube_cut.{j}"] = cube_reference(tr, starts, group, P, G, rule, cube0=cube0, cut_lookup=cube_lookup)
                out[f"cube_trunc.{j}"] = cube_trunc_reference(tr, starts, group, P, G, rule, ct, cube0=cube0)
                out[f"cube_cut_trunc.{j}"] = cube_trunc_reference(tr, starts, group, P, G, rule, ct, cube0=cube0,
                                                                  cut_lookup=cube_lookup)
            rng = np.random.RandomState(77 + G)
            out[f"cube_bearoff_call.G{G}"] = cube_bearoff_cut_reference(
                tr["cut_records"][3], rng.randint(0, 64, B).astype(np.uint8), rng.randint(0, 3, B), rng.randint(0, 4, B),
                rng.randint(0, 2, B).astype(np.uint8), starts, group, P, G, CAP, cube0, cube_lookup)
    return out


# ---------------------------------------------------------------------- the summaries --
def rows():
    """N_ROWS seeded sets of consistent tally rows, each built from its games: dict(tally, luck,
    cut, trunc, trunc_luckless, cube, cube_cut, cube_trunc, unfinished).  Row i % 8 == 0: no game
    at all; 1: one game; 2: every game with the same result (and the same luck)."""
    rng = np.random.RandomState(4321)
    out = []
    for i in range(N_ROWS):
        kind = i % 8
        n = dict(nat=0, cut=0, trunc=0, passed=0)
        if kind == 1:
            n[("nat", "cut", "trunc", "passed")[(i // 8) % 4]] = 1
        elif kind >= 2:
            n = {k: int(rng.randint(0, 40)) * int(rng.rand() < 0.8) for k in n}
        same = kind == 2
        # natural games: result +-1..3, plies, luck, the cube's k
        res = np.ones(n["nat"], np.int64) if same else rng.choice([-3, -2, -1, 1, 2, 3], n["nat"])
        k_nat = np.ones(n["nat"], np.int64) if same else rng.randint(0, 5, n["nat"])
        lq = np.full(n["nat"], 12345, np.int64) if same else rng.randint(-(1 << 21), (1 << 21) + 1, n["nat"])
        tally = [n["nat"], int(rng.randint(1, 200, n["nat"]).sum())]
        tally += [int((res == s).sum()) for s in (1, 2, 3)] + [int((res == -s).sum()) for s in (1, 2, 3)]
        luck = [int(lq.sum()), int((lq * lq).sum()), int((res * lq).sum()), n["nat"]]
        # cubeless cut games: Pq in [0, 2^20]; truncated games: Vq in +-3 * 2^16 with their luck
        pq = np.full(n["cut"], 1 << 20, np.int64) if same else rng.randint(0, (1 << 20) + 1, n["cut"])
        cut = [n["cut"], int(rng.randint(0, 50, n["cut"]).sum()), int(pq.sum()), int((pq * pq).sum())]
        vq = np.full(n["trunc"], 65536, np.int64) if same else rng.randint(-196608, 196609, n["trunc"])
        tl = np.full(n["trunc"], 12345, np.int64) if same else rng.randint(-(1 << 21), (1 << 21) + 1, n["trunc"])
        t_plies = int(rng.randint(1, 30, n["trunc"]).sum())
        trunc = [n["trunc"], t_plies, int(vq.sum()), int((vq * vq).sum()), int(tl.sum()), int((tl * tl).sum()),
                 int((vq * tl).sum())]
        # cubeful: natural games res 2^k, passed games +-2^k, cut Yq = q 2^k in 2^-20, truncated Yq in 2^-16
        k_pass = np.ones(n["passed"], np.int64) if same else rng.randint(0, 5, n["passed"])
        y_pass = (np.ones(n["passed"], np.int64) if same else rng.choice([-1, 1], n["passed"])) << k_pass
        y_nat = res << k_nat
        cube = [n["nat"] + n["passed"], int(y_nat.sum() + y_pass.sum()), int((y_nat ** 2).sum() + (y_pass ** 2).sum()),
                int(k_nat.sum() + k_pass.sum()), n["passed"], int(rng.randint(1, 60, n["passed"]).sum()),
                int((y_pass > 0).sum()), n["passed"] + int(rng.randint(0, 3, n["nat"] + n["passed"]).sum())]

        def six(count, one, clamp):
            k = np.ones(count, np.int64) if same else rng.randint(0, 5, count)
            y = (np.full(count, one, np.int64) if same else rng.randint(-clamp, clamp + 1, count)) << k
            y2 = [int(v) ** 2 for v in y]
            return [count, int(rng.randint(0, 50, count).sum()), int(y.sum()), sum(v & ((1 << 30) - 1) for v in y2),
                    sum(v >> 30 for v in y2), int(k.sum())]
        out.append(dict(tally=tally, luck=luck, cut=cut, trunc=trunc, trunc_luckless=trunc[:4] + [0, 0, 0], cube=cube,
                        cube_cut=six(n["cut"], 1 << 20, 1 << 20), cube_trunc=six(n["trunc"], 1 << 16, 3 << 16),
                        unfinished=int(rng.randint(0, 5))))
    return out


def summaries():
    """{name: [result dict per row]} of the eight summaries."""
    from bgx.cube import summarize_cube, summarize_cube_bearoff, summarize_cube_truncated
    from bgx.rollout import summarize, summarize_bearoff, summarize_luck
    from bgx.truncate import summarize_truncated, summarize_truncated_luck
    out = {}
    for i, r in enumerate(rows()):
        scale = ("fit", "fit", 1.0, 0.37)[(i // 8) % 4]
        u = r["unfinished"]
        got = dict(summarize=summarize(r["tally"], u), summarize_luck=summarize_luck(r["tally"], r["luck"], scale, u),
                   summarize_bearoff=summarize_bearoff(r["tally"], r["cut"], u),
                   summarize_truncated=summarize_truncated(r["tally"], r["trunc_luckless"], u),
                   summarize_truncated_luck=summarize_truncated_luck(r["tally"], r["luck"], r["trunc"], scale, u),
                   summarize_cube=summarize_cube(r["tally"], r["cube"], u),
                   summarize_cube_bearoff=summarize_cube_bearoff(r["tally"], r["cube"], r["cube_cut"], u),
                   summarize_cube_truncated=summarize_cube_truncated(r["tally"], r["cube"], r["cube_trunc"], u),
                   summarize_cube_truncated_cut=summarize_cube_truncated(r["tally"], r["cube"], r["cube_trunc"], u,
                                                                         cut_row=r["cube_cut"]))
        for k, v in got.items():
            out.setdefault(k, []).append(v)
    return out


def compute():
    """Everything the golden file holds, from the loaded package."""
    arrays = {}
    for name, res in references().items():
        arrays.update(digest(name, res))
    for name, res in summaries().items():
        arrays[f"summary.{name}"] = np.str_(json.dumps(res, sort_keys=True))
    return arrays


# ------------------------------------------------------------------------------ the tests --
def same(a, b, where):
    """Equal types and ==, through dicts and lists."""
    assert type(a) is type(b), (where, a, b)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            same(a[k], b[k], where + (k,))
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, where + (i,))
    else:
        assert a == b, (where, a, b)


@pytest.fixture(scope="module")
def want():
    return dict(np.load(GOLDEN_NPZ))


@pytest.fixture(scope="module")
def got():
    return compute()


def test_the_keys_are_the_recorded_ones(want, got):
    assert sorted(got) == sorted(want)


def test_references_equal_the_parent(want, got):
    for k, v in got.items():
        if k.startswith("summary."):
            continue
        if v.dtype.kind == "U":
            assert str(v) == str(want[k]), k
        else:
            assert v.dtype == want[k].dtype and v.shape == want[k].shape and np.array_equal(v, want[k]), k


def test_summaries_equal_the_parent(want, got):
    for k, v in got.items():
        if k.startswith("summary."):
            # the same round trip on both sides: a float's repr is exact
            same(json.loads(str(v)), json.loads(str(want[k])), (k,))


def test_summaries_survive_json():
    """The comparison above goes through JSON: every value is an int, a float, a str or a dict of them,
    and no float is lost in the round trip."""
    for name, res in summaries().items():
        same(json.loads(json.dumps(res)), res, (name,))


def test_record_offsets_are_the_engines():
    """replay.py imports nothing of the package but tally.py, so it states the two record offsets itself."""
    from bgx import engine, replay
    assert (replay.R_CUR, replay.R_ROLL0) == (engine.R_CUR, engine.R_ROLL0) == (R_CUR, R_ROLL0)
