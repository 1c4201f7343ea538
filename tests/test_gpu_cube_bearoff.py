"""The cubeful exact bearoff table on the device (csrc/bg_bearoff_cube.h behind
bgx_bearoff_cube_* and bgx_rollout_cube_bearoff_cut; bearoff.CubefulBearoffDB, Rollout.run_lanes /
run with cube_bearoff=): the table against the numpy recurrence bit for bit and against fp64, the
lookup on every K = 3 pair, the cut alone against its host replay, exact cube decisions through
the rollout, a traced run against cube.cube_reference, graph capture and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import bearoff_ref as BR
import cube_bearoff_ref as CR

pytestmark = pytest.mark.gpu

F = np.float32
CAP = 3                                       # the lookup and cut tests' cap: k = 3 is the dead cube


@pytest.fixture(scope="module")
def cdb3():
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    return CubefulBearoffDB(BearoffDB(3))


@pytest.fixture(scope="module")
def cdb6():
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    return CubefulBearoffDB(BearoffDB(6))


def host_configs(db):
    return [tuple(int(v) for v in c) for c in db.configs().cpu().numpy()]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def lookup_on(cdb, K):
    """cube_bearoff_cut_reference's lookup on the device table's own planes."""
    from bgx.bearoff import cube_lookup_reference
    cfg, E, ND = cdb.configs().cpu().numpy(), cdb.equity().cpu().numpy(), cdb.nd().cpu().numpy()
    W = cdb.db.table().cpu().numpy()
    return lambda recs, cube, cap: cube_lookup_reference(recs, cfg, E, ND, W, K, cube, cap)


# ------------------------------------------------------------------------- the table --
def test_table_k3_every_entry(cdb3):
    assert host_configs(cdb3) == list(CR.ordered_configs(3)) and cdb3.n == 84 and cdb3.K == 3 and cdb3.kind == "cubeful"
    E, ND = cdb3.equity().cpu().numpy(), cdb3.nd().cpu().numpy()
    assert E.shape == (3, 84, 84) and ND.shape == (2, 84, 84) and E.dtype == ND.dtype == np.float32
    W32, E32, ND32 = CR.references(3, "float32")
    assert bits_equal(cdb3.db.table().cpu().numpy(), W32)
    assert bits_equal(E, E32), int((E != E32).sum())
    assert bits_equal(ND, ND32), int((ND != ND32).sum())
    # against fp64: within 4 x the reference's own fp32-against-fp64 maximum
    W64, E64, ND64 = CR.references(3, "float64")
    for name, got, r32, r64 in (("equity", E, E32, E64), ("nd", ND, ND32, ND64)):
        bound = float(np.abs(r32.astype(np.float64) - r64).max())
        dist = float(np.abs(got.astype(np.float64) - r64).max())
        print(f"K = 3 {name}: device against fp64 {dist:.3e}, numpy fp32 against fp64 {bound:.3e}")
        assert 0 < bound < 2e-6 and dist <= 4 * bound, (name, dist, bound)


@pytest.mark.parametrize("K", [1, 2])
def test_table_smallest(K):
    """The smallest tables, which hold the roll that cannot be played (the empty configuration's)."""
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    cdb = CubefulBearoffDB(BearoffDB(K))
    assert host_configs(cdb) == list(CR.ordered_configs(K)) and cdb.n == (7, 28)[K - 1]
    _, E32, ND32 = CR.references(K, "float32")
    assert bits_equal(cdb.equity().cpu().numpy(), E32) and bits_equal(cdb.nd().cpu().numpy(), ND32)


def test_table_k6_sampled_and_subtable(cdb6, cdb3):
    from bgx.bearoff import CUBE_CHILD, ROLL_P
    n = cdb6.n
    assert n == 924
    E, ND = cdb6.equity().cpu().numpy(), cdb6.nd().cpu().numpy()
    rng = np.random.RandomState(6)
    pairs = np.stack([rng.randint(1, n, 2000), rng.randint(1, n, 2000)], 1)
    pairs[:8] = [(n - 1, n - 1), (n - 1, 1), (1, n - 1), (1, 1), (n - 2, 500), (500, n - 2), (2, 3), (900, 900)]
    succ = {}
    for a, b in pairs:
        a, b = int(a), int(b)
        if a not in succ:
            succ[a] = [np.asarray(s, np.int64) for s in cdb6.db.successors(a)]
        acc = [F(0)] * 3
        for r in range(21):
            s = succ[a][r]
            for st in range(3):
                v = np.where(s == 0, F(1), -E[CUBE_CHILD[st], b, s]).astype(F).max()
                acc[st] = F(acc[st] + F(ROLL_P[r] * v))
        cash = min(F(F(2) * acc[2]), F(1))
        want = (max(acc[0], cash), max(acc[1], cash), acc[2], acc[0], acc[1])
        got = (E[0, a, b], E[1, a, b], E[2, a, b], ND[0, a, b], ND[1, a, b])
        assert bits_equal(got, want), (a, b, got, want)
    assert (E[:, :, 0] == -1).all() and (E[:, 0, 1:] == 1).all() and (ND[:, :, 0] == -1).all() and (ND[:, 0, 1:] == 1).all()
    assert np.abs(E).max() <= 1 + 1e-6 and (E[2] <= E[0] + 1e-6).all() and (E[0] <= E[1] + 1e-6).all()
    # the K = 3 table is the sub-table of K = 6
    idx = np.array([cdb6.index_of(c) for c in host_configs(cdb3)])
    assert bits_equal(E[:, idx][:, :, idx], cdb3.equity().cpu().numpy())
    assert bits_equal(ND[:, idx][:, :, idx], cdb3.nd().cpu().numpy())


# ------------------------------------------------------------------------- the lookup --
def all_k3_records():
    n = 84
    pairs = [(a, b) for a in range(1, n) for b in range(1, n)]
    recs = np.concatenate([CR.records_of(3, pairs, [m] * len(pairs)) for m in (0, 1)])
    return recs, pairs


def test_lookup_every_k3_pair(cdb3):
    from bgx.cube import pack
    recs, pairs = all_k3_records()
    ref = lookup_on(cdb3, 3)
    d_recs = dev(recs)
    seen = set()
    # the three owners, k = 0, k = cap, and bytes that are no cube state (k above the cap, owner 3, an owner at k = 0)
    for byte in (0, pack(1, 1), pack(1, 2), pack(2, 1), pack(2, 2), pack(3, 1), pack(3, 2), 0x0F, 0x31, 0x20, 0x37):
        cube = np.full(len(recs), byte, np.uint8)
        in_db, values, flags = cdb3.lookup(d_recs, dev(cube), cap=CAP)
        w_in, w_values, w_flags = ref(recs, cube, CAP)
        assert in_db.cpu().numpy().all() and w_in.all()
        assert bits_equal(values.cpu().numpy(), w_values), byte
        assert np.array_equal(flags.cpu().numpy(), w_flags), byte
        seen |= set(w_flags.tolist())
    assert seen >= {1, 3, 5, 7, 0, 4, 8, 12}, seen          # every decision, with and without access, dead
    # the values are the planes' entries: mover 0, the cube centred
    in_db, values, flags = cdb3.lookup(d_recs)                                # cube=None: centred at 1
    w = ref(recs, None, 6)
    assert bits_equal(values.cpu().numpy(), w[1]) and np.array_equal(flags.cpu().numpy(), w[2])
    v = values.cpu().numpy()[:len(pairs)]
    a, b = np.array(pairs).T
    E, ND, W = cdb3.equity().cpu().numpy(), cdb3.nd().cpu().numpy(), cdb3.db.table().cpu().numpy()
    assert bits_equal(v[:, 0], ND[0, a, b]) and bits_equal(v[:, 1], F(2) * E[2, a, b]) and bits_equal(v[:, 2], E[0, a, b])
    assert bits_equal(v[:, 3], (F(2) * W[a, b]).astype(F) - F(1))
    # cap 0: the cube is dead from the start, every value but DT is the cubeless one
    in_db, values, flags = cdb3.lookup(d_recs[:500], cap=0)
    v = values.cpu().numpy()
    assert bits_equal(v[:, 0], v[:, 3]) and bits_equal(v[:, 2], v[:, 3]) and (flags.cpu().numpy() & 0xB == 8).all()


def test_lookup_refuses_and_arguments(cdb3):
    from bgx import _lib
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    good = BR.record((1, 1, 0, 0, 0, 1), (0, 2, 0, 0, 1, 0), 0)
    bad = []
    for change in ({55: 1}, {48: 1, 50: 11}, {49: 1, 51: 11}, {10: 1, 50: 11}, {40: 1, 51: 11}, {50: 11}, {51: 13},
                   {23: 2, 50: 11}, {23: 0, 22: 0, 18: 0, 50: 15}):
        r = good.copy()
        for k, v in change.items():
            r[k] = v
        bad.append(r)
    recs = np.stack([good] + bad + [good])
    in_db, values, flags = cdb3.lookup(dev(recs), dev(np.full(len(recs), 0x11, np.uint8)), cap=CAP)
    w = lookup_on(cdb3, 3)(recs, np.full(len(recs), 0x11, np.uint8), CAP)
    assert in_db.cpu().tolist() == [1] + [0] * len(bad) + [1] == w[0].astype(int).tolist()
    assert bits_equal(values.cpu().numpy(), w[1]) and np.isnan(values.cpu().numpy()[1:-1]).all()
    assert np.array_equal(flags.cpu().numpy(), w[2]) and not flags.cpu().numpy()[1:-1].any()
    # values and flags may be NULL; n = 0 is nothing
    L = _lib.load()
    d = dev(recs)
    o = torch.zeros(len(recs), dtype=torch.uint8).cuda()
    assert L.bgx_bearoff_cube_lookup(cdb3.handle(), ptr(d), None, len(recs), 6, ptr(o), None, None, None) == _lib.BGX_OK
    assert o.cpu().tolist() == [1] + [0] * len(bad) + [1]
    assert L.bgx_bearoff_cube_lookup(cdb3.handle(), None, None, 0, 6, None, None, None, None) == _lib.BGX_OK
    for args in ((None, ptr(d), None, 4, 6, ptr(o), None, None, None), (cdb3.handle(), None, None, 4, 6, ptr(o), None, None, None),
                 (cdb3.handle(), ptr(d), None, -1, 6, ptr(o), None, None, None),
                 (cdb3.handle(), ptr(d), None, 4, 11, ptr(o), None, None, None),
                 (cdb3.handle(), ptr(d), None, 4, -1, ptr(o), None, None, None),
                 (cdb3.handle(), ptr(d), None, 4, 6, None, None, None, None),
                 (cdb3.handle(), ctypes.c_void_p(d.data_ptr() + 4), None, 4, 6, ptr(o), None, None, None)):
        assert L.bgx_bearoff_cube_lookup(*args) == _lib.BGX_EINVAL, args
    h = ctypes.c_void_p()
    assert L.bgx_bearoff_cube_create(None, None, ctypes.byref(h)) == _lib.BGX_EINVAL and not h.value
    assert L.bgx_bearoff_cube_create(cdb3.db.handle(), None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_cube_destroy(None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_cube_buffers_get(None, None) == _lib.BGX_EINVAL
    with pytest.raises(ValueError):
        CubefulBearoffDB(object())
    with pytest.raises(ValueError):
        cdb3.lookup(d, cap=11)
    with pytest.raises(ValueError):
        cdb3.lookup(d, cube=torch.zeros(3, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError):
        cdb3.lookup(torch.from_numpy(recs))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ the cut alone --
def groups200():
    group = np.repeat(np.arange(5), [10, 50, 33, 64, 36]).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):            # 7 idle lanes, in the middle of waves and groups
        group = np.insert(group, k, -1)
    assert len(group) == 200 and (group < 0).sum() == 7
    return group


def cut_state(seed=9):
    """200 lanes of hand-set state: in-table (K = 3) and out-of-table records, plies 0 and > 0, all
    cube states and k = cap, retired lanes and lanes on their last game."""
    from bgx.cube import pack
    rng = np.random.RandomState(seed)
    B, G = 200, 2
    group = groups200()
    pairs = np.stack([rng.randint(1, 84, B), rng.randint(1, 84, B)], 1)
    mover = rng.randint(2, size=B)
    recs = CR.records_of(3, pairs, mover)
    outside = rng.rand(B) < 0.2
    recs[outside, 10], recs[outside, 50] = 1, recs[outside, 50] - 1       # a PLAYER1 checker in the outfield
    starts = recs.copy()
    starts[:, 52] = rng.randint(2, size=B)
    states = [0, pack(1, 1), pack(1, 2), pack(2, 1), pack(2, 2), pack(3, 1), pack(3, 2), 0x0F, 0x31]
    cube = np.array(states, np.uint8)[rng.randint(len(states), size=B)]
    cube0 = np.array(states[:5], np.uint8)[rng.randint(5, size=B)]
    plies = (rng.randint(0, 4, size=B) * (rng.rand(B) < 0.7)).astype(np.int32)
    games_done = rng.randint(0, 2, size=B).astype(np.int32)
    sel = ((group >= 0) & (rng.rand(B) < 0.85)).astype(np.uint8)
    games_done[(sel == 0) & (group >= 0)] = G
    return dict(recs=recs, starts=starts, group=group, cube=cube, cube0=cube0, plies=plies, games_done=games_done,
                sel=sel, G=G, P=5)


def run_cut(cdb, s, recs_dev=None, stream=None):
    from bgx import _lib
    d = {k: dev(s[k]) for k in ("starts", "group", "cube", "cube0", "plies", "games_done", "sel")}
    d["recs"] = dev(s["recs"]) if recs_dev is None else recs_dev
    B = len(s["group"])
    d["tally"] = torch.zeros(s["P"], 6, dtype=torch.int64).cuda()
    d["active"] = torch.tensor([int(s["sel"].sum())]).cuda()
    d["mask"] = torch.full((B,), 9, dtype=torch.uint8).cuda()
    rc = _lib.load().bgx_rollout_cube_bearoff_cut(cdb.handle(), ptr(d["recs"]), ptr(d["starts"]), ptr(d["group"]), B, s["P"],
                                                  s["G"], ptr(d["games_done"]), ptr(d["plies"]), ptr(d["sel"]),
                                                  ptr(d["tally"]), ptr(d["active"]), ptr(d["mask"]), CAP, ptr(d["cube0"]),
                                                  ptr(d["cube"]), stream)
    assert rc == _lib.BGX_OK
    return d


def test_cut_alone_equals_the_host_replay(cdb3):
    from bgx.cube import cube_bearoff_cut_reference, sanitise
    s = cut_state()
    ref = cube_bearoff_cut_reference(s["recs"], s["cube"], s["plies"], s["games_done"], s["sel"], s["starts"], s["group"],
                                     s["P"], s["G"], CAP, s["cube0"], lookup_on(cdb3, 3))
    runs = [run_cut(cdb3, s) for _ in range(2)]
    d = runs[0]
    torch.cuda.synchronize()
    m = ref["mask"]
    for name, got, want in (("tally", d["tally"], ref["cut_tally"]), ("mask", d["mask"], m.astype(np.uint8)),
                            ("games_done", d["games_done"], ref["games_done"]), ("plies", d["plies"], ref["plies"]),
                            ("sel", d["sel"], ref["sel"]), ("cube", d["cube"], np.where(m, sanitise(s["cube0"], CAP), s["cube"]))):
        assert np.array_equal(got.cpu().numpy(), want), name
    assert int(d["active"].item()) == int(s["sel"].sum()) - ref["retired"] and ref["retired"] > 5
    # every kind of lane occurs among the cut ones, every row is hit, negative and positive results
    from bgx.bearoff import cube_state_reference
    st, k = cube_state_reference(s["cube"], CAP, s["recs"][:, 52])
    assert set(st[m].tolist()) == {0, 1, 2, 3} and (s["plies"][m] == 0).any() and (s["plies"][m] > 0).any()
    assert (s["sel"] == 0).any() and not m[s["sel"] == 0].any() and not m[s["group"] < 0].any()
    out = s["recs"][:, 10] == 1
    assert (out & (s["sel"] != 0) & (s["group"] >= 0)).any() and not m[out].any()
    t = ref["cut_tally"]
    assert (t[:, 0] > 0).all() and t[:, 0].sum() == m.sum() > 80 and (t[:, 4] > 0).all() and t[:, 5].sum() > 50
    # run to run identical
    for key in ("tally", "mask", "games_done", "plies", "sel", "cube", "active"):
        assert torch.equal(runs[1][key], d[key]), key


def test_cut_arguments(cdb3):
    from bgx import _lib
    L = _lib.load()
    n = 64
    z = torch.zeros(n * 64, dtype=torch.uint8).cuda()
    i32 = lambda: torch.zeros(n, dtype=torch.int32).cuda()
    t = torch.zeros(8, dtype=torch.int64).cuda()
    gi, gd, pl = i32(), i32(), i32()
    good = [cdb3.handle(), ptr(z), ptr(z), ptr(gi), n, 1, 1, ptr(gd), ptr(pl), ptr(z), ptr(t), ptr(t[6:]), ptr(z), 6, ptr(z),
            ptr(z), None]
    assert L.bgx_rollout_cube_bearoff_cut(*good) == _lib.BGX_OK
    for idx, val in [(i, None) for i in (0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 14, 15)] + \
            [(4, 0), (5, 0), (6, -1), (13, -1), (13, 11), (1, ctypes.c_void_p(z.data_ptr() + 4))]:
        args = list(good)
        args[idx] = val
        assert L.bgx_rollout_cube_bearoff_cut(*args) == _lib.BGX_EINVAL, idx
    torch.cuda.synchronize()


# ------------------------------------------------------------------ through the rollout --
def never(eng, dsel):
    return torch.full((eng.batch,), -1.0, dtype=torch.float32, device=eng.device)


def test_cube_decision_is_the_tables(cdb3):
    """rollout_cube_decision on positions in the table, one game a lane: the cut after begin scores
    every game with the table's nd (the no-double rollout) and E_opp x 2 (the double-take one)."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CUBE_CUT_ONE, CubeRule, rollout_cube_decision
    from bgx.rollout import Rollout
    W, E, ND = CR.references(3, "float32")
    cfg = CR.ordered_configs(3)
    margin = np.abs(np.minimum(F(2) * E[2], F(1)) - ND)          # [2, n, n]: cen, own
    positions = [((0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0), 0, (0, 0)),        # the hand case: a double and a take
                 ((0, 0, 1, 1, 0, 1), (0, 1, 0, 0, 2, 0), 1, (0, 0)),
                 ((0, 1, 1, 0, 0, 0), (0, 0, 0, 1, 1, 1), 0, (0, 0)),        # far ahead
                 ((0, 0, 0, 1, 1, 1), (1, 1, 0, 0, 0, 0), 1, (1, 2)),        # far behind, PLAYER2 owns the cube at 2
                 ((0, 1, 0, 1, 0, 1), (0, 0, 2, 0, 1, 0), 0, (2, 1))]
    ro = Rollout(128, seed=1)
    rule = CubeRule(never)
    verdicts = set()
    for mine, theirs, mover, cube in positions:
        a, b = cfg.index(mine), cfg.index(theirs)
        s = 0 if cube[1] == 0 else 1
        assert margin[s, a, b] > 1e-4, (mine, theirs)            # the fixed point cannot flip the verdict
        rec = BR.record(mine, theirs, 0) if mover == 0 else BR.record(theirs, mine, 1)
        _, values, flags = cdb3.lookup(dev(rec[None]), dev(np.array([cube[0] | (cube[1] << 4)], np.uint8)), cap=6)
        v, fl = values.cpu().numpy()[0], int(flags[0])
        assert bits_equal(v[0], ND[s, a, b]) and bits_equal(v[1], F(2) * E[2, a, b]) and fl & 1
        d = rollout_cube_decision(ro, RandomPlayer(1), torch.from_numpy(rec), 36, rule, cube=cube, cube_bearoff=cdb3)
        q = lambda x: int(np.rint(F(x) * F(CUBE_CUT_ONE)))
        assert d["no_double"] == q(v[0]) / CUBE_CUT_ONE and d["double_take"] == 2 * q(E[2, a, b]) / CUBE_CUT_ONE
        assert d["no_double_stderr"] == d["double_take_stderr"] == 0.0
        assert d["double"] == bool(fl & 2) and d["take"] == bool(fl & 4)
        for r in d["rollouts"]:
            assert r["games"] == r["cut_games"] == 36 and r["cut_share"] == 1.0 and r["bearoff_kind"] == "cubeful"
            assert r["plies_per_game"] == 0.0 and r["unfinished"] == 0
        verdicts.add((d["double"], d["take"]))
    assert len(verdicts) >= 3, verdicts
    assert ro.eng.error() == 0


def near_k3_starts(B, seed):
    """Both sides home with 4 or 5 checkers: two or three plies from the K = 3 table."""
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        c = [np.bincount(rng.randint(0, 6, rng.randint(4, 6)), minlength=6) for _ in range(2)]
        s[i] = BR.record(tuple(c[0]), tuple(c[1]), rng.randint(2), (rng.randint(1, 7), rng.randint(1, 7)) if i % 2 else (0, 0))
    return s


def by_lane(B):
    """A cube rule's callable equity: a take (0.45), a pass (0.9) or no double (-1) by the lane."""
    e = torch.tensor([0.45, 0.9, -1.0, 0.45, -1.0], dtype=torch.float32).repeat(B // 5 + 1)[:B].cuda().contiguous()
    return lambda eng, dsel: e


def traced(cdb, B=64, seed=5):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule, pack
    from bgx.rollout import Rollout
    P, G = 3, 2
    group = np.repeat(np.arange(3), [20, 21, 20]).astype(np.int32)
    for k in (7, 30, 50):
        group = np.insert(group, k, -1)
    starts = near_k3_starts(B, 21)
    cube0 = np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)]
    rule = CubeRule(by_lane(B), cap=4)
    ro = Rollout(B, seed=seed)
    out = ro.run_lanes(RandomPlayer(2), torch.from_numpy(starts), torch.from_numpy(group), P, G, max_steps=400, trace=True,
                       cube=rule, cube0=torch.from_numpy(cube0), cube_bearoff=cdb)
    assert ro.eng.error() == 0 and len(out) == 5 and not out[1].any()
    return out, starts, group, cube0, rule, P, G


def test_traced_run_equals_the_host_replay(cdb3):
    from bgx.cube import cube_reference, summarize_cube_bearoff
    runs = [traced(cdb3) for _ in range(2)]
    (tally, unf, tr, ct, cct), starts, group, cube0, rule, P, G = runs[0]
    tally, ct, cct = tally.cpu().numpy(), ct.cpu().numpy(), cct.cpu().numpy()
    ref = cube_reference(tr, starts, group, P, G, rule, cube0, cut_lookup=lookup_on(cdb3, 3))
    assert np.array_equal(cct, ref["cut_tally"]) and np.array_equal(ct, ref["cube_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["cube"].cpu().numpy(), ref["cube"])
    assert np.array_equal(tr["cube_dsel"].cpu().numpy() != 0, ref["dsel"])
    assert np.array_equal(tr["cube_mask"].cpu().numpy() != 0, ref["mask"])
    assert np.array_equal(tr["cut"].cpu().numpy() != 0, ref["cut"]) and np.array_equal(tr["cut0"].cpu().numpy() != 0, ref["cut0"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    # cut games, passes and takes all occur; a cut with the cube turned; the invariant holds with the cut beside it
    takes = ct[:, 7].sum() - ct[:, 4].sum()
    assert cct[:, 0].sum() > 20 and ct[:, 4].sum() > 5 and takes > 5 and cct[:, 5].sum() > 0
    assert np.array_equal(ct[:, 0], tally[:, 0] + ct[:, 4])
    scheduled = np.bincount(group[group >= 0], minlength=P) * G
    assert np.array_equal(ct[:, 0] + cct[:, 0], scheduled)
    assert not tr["cut"][:, torch.from_numpy(group < 0).cuda()].any()
    for p in range(P):
        r = summarize_cube_bearoff(tally[p], ct[p], cct[p])
        assert r["games"] == scheduled[p] and 0 <= r["cut_share"] <= 1 and math.isfinite(r["equity_cubeful_stderr"])
    # run to run identical
    for j in (0, 3, 4):
        assert torch.equal(runs[1][0][j], runs[0][0][j]), j
    for k in ("cube", "cube_dsel", "cube_mask", "action", "cut", "cut_records", "done", "info"):
        assert torch.equal(runs[1][0][2][k], tr[k]), k


def test_none_is_the_parent_path():
    """cube_bearoff=None: the tallies, the trace and the result's shape of the run without it."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout
    B = 64
    starts, grp = torch.from_numpy(near_k3_starts(B, 3)), torch.zeros(B, dtype=torch.int32)
    outs = []
    for kw in ({}, dict(cube_bearoff=None)):
        ro = Rollout(B, seed=2)
        outs.append(ro.run_lanes(RandomPlayer(4), starts, grp, 1, 2, max_steps=400, trace=True, cube=CubeRule(by_lane(B)), **kw))
    assert len(outs[0]) == len(outs[1]) == 4 and "cut" not in outs[1][2]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][3], outs[1][3])
    for k in ("action", "done", "info", "cube", "cube_mask"):
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k
    assert int(outs[0][3][0, 0]) == 2 * B


def test_value_errors(cdb3):
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffDB
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout, opening_record
    from bgx.truncate import Truncation
    ro = Rollout(64, seed=0)
    rule = CubeRule(never)
    starts, grp = torch.from_numpy(near_k3_starts(64, 1)), torch.zeros(64, dtype=torch.int32)
    pos = opening_record()[None]
    with pytest.raises(ValueError, match="cube_bearoff without cube"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube_bearoff=cdb3)
    with pytest.raises(ValueError, match="cube_bearoff without cube"):
        ro.run(RandomPlayer(1), pos, 36, cube_bearoff=cdb3)
    trunc = Truncation(lambda eng, sel: None, 4)
    for kw, word in ((dict(luck=object()), "luck"), (dict(bearoff=cdb3.db), "bearoff"), (dict(truncate=trunc), "truncate")):
        with pytest.raises(ValueError, match=f"cube_bearoff together with {word}"):
            ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=rule, cube_bearoff=cdb3, **kw)
        with pytest.raises(ValueError, match=f"cube_bearoff together with {word}"):
            ro.run(RandomPlayer(1), pos, 36, cube=rule, cube_bearoff=cdb3, **kw)
    with pytest.raises(ValueError, match="CubefulBearoffDB"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=rule, cube_bearoff=cdb3.db)
    with pytest.raises(ValueError, match="cube together with bearoff"):          # the old refusal stays
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=rule, bearoff=cdb3.db)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- graph capture --
def test_graph_capture(cdb3):
    """The lookup and the cut captured into one graph replay to the eager results."""
    s = cut_state(seed=11)
    B = len(s["group"])
    d_recs, d_cube = dev(s["recs"]), dev(s["cube"])
    eager = run_cut(cdb3, s, d_recs)
    e_look = cdb3.lookup(d_recs, d_cube, cap=CAP)
    torch.cuda.synchronize()
    look = (torch.full((B,), 5, dtype=torch.uint8).cuda(), torch.full((B, 4), float("nan")).cuda(),
            torch.full((B,), 5, dtype=torch.uint8).cuda())
    state = {k: dev(s[k]) for k in ("starts", "group", "cube", "cube0", "plies", "games_done", "sel")}
    state.update(tally=torch.zeros(s["P"], 6, dtype=torch.int64).cuda(), active=torch.tensor([int(s["sel"].sum())]).cuda(),
                 mask=torch.full((B,), 9, dtype=torch.uint8).cuda())
    before = {k: v.clone() for k, v in state.items()}
    from bgx import _lib
    L = _lib.load()
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        cdb3.lookup(d_recs, d_cube, cap=CAP, out=look)
        rc = L.bgx_rollout_cube_bearoff_cut(cdb3.handle(), ptr(d_recs), ptr(state["starts"]), ptr(state["group"]), B, s["P"],
                                            s["G"], ptr(state["games_done"]), ptr(state["plies"]), ptr(state["sel"]),
                                            ptr(state["tally"]), ptr(state["active"]), ptr(state["mask"]), CAP,
                                            ptr(state["cube0"]), ptr(state["cube"]),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.BGX_OK
    torch.cuda.synchronize()
    for k, v in before.items():                            # the capture ran nothing
        assert torch.equal(state[k], v), k
    g.replay()
    torch.cuda.synchronize()
    for k in ("tally", "mask", "games_done", "plies", "sel", "cube", "active"):
        assert torch.equal(state[k], eager[k]), k
    assert torch.equal(look[0], e_look[0]) and torch.equal(look[2], e_look[2])
    assert torch.equal(look[1].view(torch.int32), e_look[1].view(torch.int32))
    assert int(state["tally"][:, 0].sum()) > 50


# ---------------------------------------------------------------------- the command line --
def test_command_line(tmp_path, capsys):
    from bgx import rollout
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    ckpt = str(tmp_path / "net.pt")
    torch.save(PolicyNet(hidden_size=40).state_dict(), ckpt)
    pos = str(tmp_path / "pos.json")
    rec = BR.record((0, 1, 1, 1, 1, 0), (1, 0, 1, 1, 0, 1), 0)             # four checkers a side: outside K = 3
    json.dump([{"board": rec[:52].tolist(), "player": 0}], open(pos, "w"))
    base = ["--net", ckpt, "--positions", pos, "--trials", "72", "--batch", "128", "--max-steps", "400", "--cube",
            "--cube-double", "0.13", "--cube-pass", "0.19", "--cube-cap", "4", "--cube-bearoff", "3"]
    rollout.main(base)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["position"] == 0 and lines[1]["summary"] and lines[1]["cube"] is True
    r, s = lines
    assert r["bearoff_kind"] == "cubeful" and s["bearoff_kind"] == "cubeful" and s["cube_bearoff"] == 3
    assert r["games"] + r["unfinished"] == 72 and r["games"] == r["played_out"]["games"] + r["pass_games"] + r["cut_games"]
    assert 0 < r["cut_share"] <= 1 and s["cut_share"] == r["cut_share"] and s["cut_games"] == r["cut_games"]
    for k in ("equity_cubeful", "equity_cubeful_stderr", "pass_share", "plies_per_game", "mean_cube_log2"):
        assert math.isfinite(r[k]), k
    # the decision of a position in the table is the table's
    rec3 = BR.record((0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0), 0)
    json.dump([{"board": rec3[:52].tolist(), "player": 0}], open(pos, "w"))
    rollout.main(base[:4] + ["--trials", "36"] + base[6:] + ["--cube-decision"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    d = lines[0]
    assert d["cube_decision"] is True and d["double"] is True and d["take"] is True
    assert abs(d["no_double"] - 0.5) < 2e-6 and d["double_take"] == 1.0 and d["no_double_stderr"] == 0.0
    assert lines[1]["cut_share"] == 1.0 and lines[1]["games"] == 72
