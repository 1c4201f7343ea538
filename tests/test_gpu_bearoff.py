"""The exact two-sided bearoff database on the device (csrc/bg_bearoff.h, bgx/bearoff.py):
successor sets and table against the oracle's move generator and a numpy evaluation of the
recurrence, lookup, perfect play, the rollout cut against its host replay, graph capture."""
import ctypes
import math

import numpy as np
import pytest
import torch

import bearoff_ref as BR
import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def db3():
    from bgx.bearoff import BearoffDB
    return BearoffDB(3)


@pytest.fixture(scope="module")
def db4():
    from bgx.bearoff import BearoffDB
    return BearoffDB(4)


@pytest.fixture(scope="module")
def db6():
    from bgx.bearoff import BearoffDB
    return BearoffDB(6)


@pytest.fixture(scope="module")
def oracle_succ4():
    """The oracle's successor sets of every configuration of at most 4 checkers (mover 0
    against a one-checker opponent), computed once: {config: [21 sets of configs]}."""
    return {c: BR.oracle_successors(c) for c in BR.all_configs(4)}


def host_configs(db):
    return [tuple(int(v) for v in c) for c in db.configs().cpu().numpy()]


# ------------------------------------------------------------------- successors --
def test_successors_k4(db4, oracle_succ4):
    cfg = host_configs(db4)
    assert db4.n == 210 == len(set(cfg)) and db4.K == 4 and cfg[0] == (0,) * 6
    pips = [sum((d + 1) * v for d, v in enumerate(c)) for c in cfg]
    assert pips == sorted(pips)                            # every pip count a contiguous range
    assert [db4.index_of(c) for c in cfg] == list(range(210))
    widest = 0
    for i, c in enumerate(cfg):
        got = db4.successors(i)
        assert len(got) == 21
        for r, (lst, want) in enumerate(zip(got, oracle_succ4[c])):
            assert lst == sorted(set(lst)), (c, r)
            assert {cfg[j] for j in lst} == want, (c, BR.ROLLS21[r])
            widest = max(widest, len(lst))
    assert widest == 15
    for i in range(1, 210, 7):                             # mover 1, another opponent placement
        want = BR.oracle_successors(cfg[i], mover=1, opp=(0, 2, 0, 1, 0, 0))
        assert [{cfg[j] for j in lst} for lst in db4.successors(i)] == want, cfg[i]
    with pytest.raises(IndexError):
        db4.successors(210)
    with pytest.raises(ValueError):
        db4.index_of((5, 0, 0, 0, 0, 0))


# ------------------------------------------------------------------ table, K = 3 --
def test_table_k3_every_entry(db3, oracle_succ4):
    from bgx.bearoff import table_reference
    cfg = host_configs(db3)
    n = db3.n
    assert n == 84
    succ = [[sorted(db3.index_of(s) for s in oracle_succ4[c][r]) for r in range(21)] for c in cfg]
    W = db3.table().cpu().numpy()
    assert W.shape == (n, n) and W.dtype == np.float32
    ref32 = table_reference(succ, n, np.float32)
    assert np.array_equal(W.view(np.uint32), ref32.view(np.uint32)), int((W != ref32).sum())
    ref64 = table_reference(succ, n, np.float64)
    dist = float(np.abs(W.astype(np.float64) - ref64).max())
    print("K = 3: fp32 table against fp64, max abs", dist)
    assert dist <= 2e-6, f"K = 3 fp32-against-fp64 distance {dist:.3e}"
    # boundary rows and known values
    assert not W[:, 0].any() and (W[0, 1:] == 1).all()
    # (exact in real arithmetic and to 1e-12 in fp64; the fp32 entries are the recurrence's own
    # roundings -- the 21 fp32 probabilities do not sum to 1.0f -- so they hold to the margin)
    six = db3.index_of((0, 0, 0, 0, 0, 1))
    assert abs(ref64[six, six] - 0.8125) < 1e-12 and abs(float(W[six, six]) - 0.8125) <= 2e-6
    assert abs(ref64[1:, 1:].min() - 1 / 36) < 1e-12 and abs(float(W[1:, 1:].min()) - 1 / 36) <= 2e-6
    assert abs(ref64[1:, 1:].max() - 1.0) < 1e-12 and abs(float(W[1:, 1:].max()) - 1.0) <= 2e-6


# ------------------------------------------------------------------ table, K = 6 --
def test_table_k6(db6, db3):
    from bgx.bearoff import ROLL_P
    n = db6.n
    assert n == 924 and db6.K == 6
    W = db6.table().cpu().numpy()
    rng = np.random.RandomState(6)
    for a, b in zip(rng.randint(1, n, 2000), rng.randint(1, n, 2000)):
        acc = F(0)
        for r, s in enumerate(db6.successors(a)):
            s = np.asarray(s)
            w = np.where(s == 0, F(1), (F(1) - W[b, s]).astype(F)).max()
            acc = F(acc + F(ROLL_P[r] * w))
        assert acc.view(np.uint32) == W[a, b].view(np.uint32), (a, b, float(acc), float(W[a, b]))
    # a value does not depend on K
    idx = [db6.index_of(c) for c in host_configs(db3)]
    W3 = db3.table().cpu().numpy()
    assert np.array_equal(W[np.ix_(idx, idx)].view(np.uint32), W3.view(np.uint32))
    # the recurrence's own fp32 roundings can leave [0, 1] by less than the margin (the 21 fp32
    # probabilities do not sum to 1.0f); the rollout cut clamps its fixed-point value
    assert not W[:, 0].any() and (W[0, 1:] == 1).all() and (W[1:, 1:] >= -2e-6).all() and (W[1:, 1:] <= 1 + 2e-6).all()


# ------------------------------------------------------------------------ lookup --
def test_lookup_every_k3_pair(db3):
    cfg = host_configs(db3)
    W = db3.table().cpu().numpy()
    recs, want = [], []
    for m in (0, 1):
        for i in range(1, db3.n):
            for j in range(1, db3.n):
                recs.append(BR.record(cfg[i], cfg[j], m, roll=((i % 6) + 1, (j % 6) + 1) if (i + j) % 3 else (0, 0)))
                want.append(W[i, j] if m == 0 else W[j, i])
    recs = torch.from_numpy(np.stack(recs)).cuda()
    in_db, win = db3.lookup(recs)
    assert bool(in_db.all()) and in_db.dtype == torch.uint8
    assert np.array_equal(win.cpu().numpy().view(np.uint32), np.asarray(want, F).view(np.uint32))
    # in_db alone (win_out NULL)
    only = torch.zeros(recs.shape[0], dtype=torch.uint8, device="cuda")
    from bgx._lib import check
    check(db3._lib.bgx_bearoff_lookup(db3.handle(), ctypes.c_void_p(recs.data_ptr()), recs.shape[0],
                                      ctypes.c_void_p(only.data_ptr()), None, None), "bgx_bearoff_lookup")
    torch.cuda.synchronize()
    assert bool(only.all())


def test_lookup_refuses(db3):
    from bgx.bearoff import lookup_reference
    good = BR.record((1, 1, 0, 0, 0, 1), (0, 2, 0, 0, 1, 0), 0)
    bad = {}
    r = good.copy(); r[23] -= 1; r[17] += 1; bad["a checker outside home"] = r
    r = good.copy(); r[24 + 1] -= 1; r[24 + 6] += 1; bad["a PLAYER2 checker outside home"] = r
    r = good.copy(); r[23] -= 1; r[48] += 1; bad["a checker on the bar"] = r
    r = good.copy(); r[24 + 1] -= 1; r[49] += 1; bad["a PLAYER2 checker on the bar"] = r
    bad["K + 1 checkers"] = BR.record((1, 1, 1, 0, 0, 1), (0, 2, 0, 0, 1, 0), 0)
    bad["K + 1 checkers, PLAYER2"] = BR.record((1, 1, 0, 0, 0, 1), (0, 2, 1, 0, 1, 0), 1)
    r = good.copy(); r[55] = 1; bad["game_over set"] = r
    bad["15 off"] = BR.record((0,) * 6, (0, 2, 0, 0, 1, 0), 1)
    r = good.copy(); r[50] -= 1; bad["an invalid sum"] = r
    r = good.copy(); r[51] += 1; bad["an invalid sum, PLAYER2"] = r
    recs = np.stack([good] + list(bad.values()))
    dev = torch.from_numpy(recs).cuda()
    in_db, win = db3.lookup(dev)
    in_db, win = in_db.cpu().numpy(), win.cpu().numpy()
    assert in_db[0] == 1 and not np.isnan(win[0])
    for k, name in enumerate(bad, start=1):
        assert in_db[k] == 0 and np.isnan(win[k]), name
    ref_in, ref_win = lookup_reference(recs, db3.configs().cpu().numpy(), db3.table().cpu().numpy(), 3)
    assert np.array_equal(ref_in, in_db != 0) and ref_win[0] == win[0]
    with pytest.raises(ValueError):
        db3.lookup(dev[:, :52])


# --------------------------------------------------------------------------- act --
def test_act_is_the_first_argmax(db4):
    from bgx.engine import Engine
    B = 208
    cfg = host_configs(db4)
    W = db4.table().cpu().numpy()
    rng = np.random.RandomState(4)
    recs = np.zeros((B, 64), np.uint8)
    one = (1, 0, 0, 0, 0, 0)
    for i in range(B):
        a, b = cfg[rng.randint(1, db4.n)], cfg[rng.randint(1, db4.n)]
        if i % 23 == 5:
            a = one if i % 2 else (0, 0, 1, 0, 0, 0)       # every play bears the last checker off
        recs[i] = BR.record(a, b, 0, BR.ROLLS21[i % 21]) if i % 2 == 0 else BR.record(b, a, 1, BR.ROLLS21[i % 21])
    off_table = [7, 60, 133]
    recs[7] = 0
    recs[7, :52] = O.INITIAL_BOARD52.view(np.uint8)
    recs[7, 53:55] = (3, 1)
    recs[60] = BR.record((1, 1, 1, 1, 1, 0), cfg[9], 0, (6, 5))        # 5 checkers: not in the K = 4 table
    recs[133] = BR.record(cfg[20], cfg[30], 1, (2, 2))
    recs[133, 24 + 9], recs[133, 51] = 1, recs[133, 51] - 1             # a PLAYER2 checker outside home
    sel = np.ones(B, np.uint8)
    unselected = [0, 33, 34, 100, 207]
    sel[unselected] = 0
    eng = Engine(batch=B, max_moves=500, seed=1, dice="philox")
    eng.reset(want_obs=False)
    eng.set_lanes(torch.from_numpy(recs))
    act = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    in_db = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    db4.act(eng, torch.from_numpy(sel).cuda(), act, in_db)
    lanes, moves, _ = eng.lanes()
    lanes, moves, act, in_db = lanes.cpu().numpy(), moves.cpu().numpy().view(np.uint64), act.cpu().numpy(), in_db.cpu().numpy()
    assert eng.error() == 0
    checked, last_off, rolls = 0, 0, set()
    for i in range(B):
        if i in unselected:
            assert act[i] == -7 and in_db[i] == 0, i
            continue
        if i in off_table:
            assert act[i] == -7 and in_db[i] == 0, i
            continue
        assert in_db[i] == 1, i
        mover = int(recs[i, 52])
        nm = int(lanes[i, 60]) | (int(lanes[i, 61]) << 8)
        assert nm > 0
        board = recs[i, :52].view(np.int8)
        opp = db4.index_of(BR.config_of(board, 1 - mover))
        vals = []
        for m in moves[i, :nm]:
            after = BR.config_of(O.apply_move(board, mover, int(m)), mover)
            vals.append(F(1) if not any(after) else F(1) - W[opp, db4.index_of(after)])
        assert act[i] == int(np.argmax(np.asarray(vals, F))), (i, vals, act[i])
        checked += 1
        last_off += all(v == 1 for v in vals)
        rolls.add((int(recs[i, 53]), int(recs[i, 54])))
    assert checked == B - len(unselected) - len(off_table) == 200 and last_off >= 5 and len(rolls) == 21
    # NULL selection = every lane; NULL in_db
    act2 = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    db4.act(eng, None, act2)
    act2 = act2.cpu().numpy()
    keep = np.array([i not in unselected for i in range(B)])
    assert np.array_equal(act2[keep], act[keep]) and (act2[[0, 33, 34, 100, 207]] >= 0).all()
    assert (act2[off_table] == -7).all()


# ------------------------------------------------------- perfect play is the table --
START = BR.record((0, 1, 0, 1, 1, 1), (1, 0, 1, 0, 1, 1), 0)


def test_perfect_play_wins_at_the_table_rate(db4):
    """4,096 games from one in-table position with drawn first rolls and the table's player on
    both sides: the win count within 5 binomial standard deviations of 4096 W."""
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffPlayer
    from bgx.rollout import Rollout
    w = float(db4.table()[db4.index_of((0, 1, 0, 1, 1, 1)), db4.index_of((1, 0, 1, 0, 1, 1))])
    assert 0.2 < w < 0.8
    ro = Rollout(1024, seed=11)
    player = BearoffPlayer(RandomPlayer(5), db4)
    assert player.sync_free
    r, = ro.run(player, torch.from_numpy(START[None]), 4096, first_roll="random")
    assert r["games"] == 4096 and r["unfinished"] == 0 and r["win1"] + r["loss1"] == 4096
    sd = math.sqrt(4096 * w * (1 - w))
    print("perfect play: wins", r["win1"], "expected", 4096 * w, "sd", sd)
    assert abs(r["win1"] - 4096 * w) <= 5 * sd
    assert ro.eng.error() == 0


def test_cut_from_a_table_position_is_exact(db4):
    from bgx.arena import RandomPlayer
    from bgx.rollout import CUT_ONE, Rollout
    w = db4.table()[db4.index_of((0, 1, 0, 1, 1, 1)), db4.index_of((1, 0, 1, 0, 1, 1))].cpu().numpy()
    pq = int(np.rint(F(w * F(CUT_ONE))))
    ro = Rollout(4096, seed=3)
    r, = ro.run(RandomPlayer(1), torch.from_numpy(START[None]), 4096, first_roll="random", bearoff=db4)
    assert r["games"] == r["cut_games"] == 4096 and r["natural_games"] == 0 and r["unfinished"] == 0
    assert r["cut_share"] == 1.0 and r["equity_stderr"] == 0.0 and r["plies_per_game"] == 0.0
    assert r["equity"] == (2 * pq - CUT_ONE) / CUT_ONE and abs(r["equity"] - (2 * float(w) - 1)) <= 2.0 ** -20
    assert r["win"] == pq / CUT_ONE
    # PLAYER2 on roll in the mirrored position: the same number
    mirror = BR.record((1, 0, 1, 0, 1, 1), (0, 1, 0, 1, 1, 1), 1)
    r2, = ro.run(RandomPlayer(1), torch.from_numpy(mirror[None]), 4096, first_roll="random", bearoff=db4)
    assert r2["equity"] == r["equity"] and r2["cut_share"] == 1.0
    assert ro.eng.error() == 0


# ---------------------------------------------------------------- cut bookkeeping --
def near_table_starts(B, seed):
    """Mid-game starts a few plies from the K = 6 table: both sides home, 5..8 checkers each
    (in the table already when both have at most 6), every other lane with a fixed roll; every
    tenth lane's mover bears its only checker off against 8 (a game that ends outside the table)."""
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        c = [np.bincount(rng.randint(0, 6, rng.randint(5, 9)), minlength=6) for _ in range(2)]
        roll = (rng.randint(1, 7), rng.randint(1, 7)) if i % 2 else (0, 0)
        mover = rng.randint(2)
        if i % 10 == 3:
            c[mover], c[1 - mover] = (1, 0, 0, 0, 0, 0), (2, 2, 1, 1, 1, 1)
        s[i] = BR.record(tuple(c[0]), tuple(c[1]), mover, roll)
    return s


def cut_run(db6, starts, group, P, G):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    ro = Rollout(len(group), seed=4)
    tally, unfinished, tr, cut_tally = ro.run_lanes(RandomPlayer(5), torch.from_numpy(starts), torch.from_numpy(group),
                                                    P, G, max_steps=300, trace=True, bearoff=db6)
    assert ro.eng.error() == 0
    return tally.cpu().numpy(), unfinished.cpu().numpy(), tr, cut_tally.cpu().numpy()


def test_cut_bookkeeping_equals_host_replay(db6):
    from bgx.rollout import bearoff_cut_reference, summarize_bearoff
    B, P, G = 200, 5, 2
    group = np.repeat(np.arange(P), [10, 50, 33, 64, 36]).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):             # 7 idle lanes, in the middle of waves and groups
        group = np.insert(group, k, -1)
    assert len(group) == B
    starts = near_table_starts(B, 12)
    runs = [cut_run(db6, starts, group, P, G) for _ in range(2)]
    tally, unfinished, tr, cut_tally = runs[0]
    ref = bearoff_cut_reference(tr["cut_records0"].cpu().numpy(), tr["cut_records"].cpu().numpy(),
                                tr["done"].cpu().numpy(), tr["info"].cpu().numpy(), starts, group, P, G,
                                db6.configs().cpu().numpy(), db6.table().cpu().numpy(), 6)
    assert np.array_equal(cut_tally, ref["cut_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    assert np.array_equal(tr["cut0"].cpu().numpy() != 0, ref["cut0"])
    assert np.array_equal(tr["cut"].cpu().numpy() != 0, ref["cut"])
    # both kinds of ending occur, at the start and later; idle lanes are never cut
    assert ref["cut0"].any() and ref["cut"].any() and cut_tally[:, 0].sum() > 100 and tally[:, 0].sum() > 10
    assert not tr["cut"].cpu().numpy()[:, group < 0].any() and not ref["cut0"][group < 0].any()
    # games + unfinished = what was scheduled
    scheduled = np.bincount(group[group >= 0], minlength=P) * G
    assert not unfinished.any()
    assert np.array_equal(tally[:, 0] + cut_tally[:, 0] + unfinished, scheduled)
    for p in range(P):
        r = summarize_bearoff(tally[p], cut_tally[p], unfinished[p])
        assert r["games"] == scheduled[p] and -1.0 <= r["equity"] <= 3.0 and 0 < r["cut_share"] <= 1
    # run to run identical
    assert np.array_equal(runs[1][3], cut_tally) and np.array_equal(runs[1][0], tally)
    for k in ("done", "info", "action", "mover", "cut", "cut_records"):
        assert torch.equal(runs[1][2][k], tr[k]), k


def posed(db6, B=192, seed=5):
    """An engine with a start table and lanes posed a few plies away from their starts (some
    in the K = 6 table, some not), and rollout state begun on it."""
    from bgx import _lib
    from bgx.engine import Engine
    starts = near_table_starts(B, seed)
    lanes = near_table_starts(B, seed + 1)
    lanes[:, 53:55] = np.where(lanes[:, 53:54] == 0, np.uint8(3), lanes[:, 53:55])    # a roll to play everywhere
    group = (np.arange(B) % 4).astype(np.int32)
    group[[5, 70, 71]] = -1
    eng = Engine(batch=B, max_moves=500, seed=2, dice="philox")
    eng.set_starts(torch.from_numpy(starts))
    eng.reset(want_obs=False)
    eng.set_lanes(torch.from_numpy(lanes))
    dev = lambda a: torch.from_numpy(a).cuda()
    st = dict(starts=dev(starts), group=dev(group), games_done=torch.zeros(B, dtype=torch.int32, device="cuda"),
              plies=torch.zeros(B, dtype=torch.int32, device="cuda"), sel=torch.zeros(B, dtype=torch.uint8, device="cuda"),
              tally=torch.zeros(4, 8, dtype=torch.int64, device="cuda"), active=torch.zeros(1, dtype=torch.int64, device="cuda"),
              cut_tally=torch.zeros(4, 4, dtype=torch.int64, device="cuda"), mask=torch.full((B,), 7, dtype=torch.uint8, device="cuda"))
    L = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(L.bgx_rollout_begin(ctypes.c_void_p(eng.lanes_ptr()), p(st["starts"]), p(st["group"]), B, 4, 3,
                                   p(st["games_done"]), p(st["plies"]), p(st["sel"]), p(st["tally"]), p(st["active"]),
                                   None), "bgx_rollout_begin")
    st["plies"] += 2
    torch.cuda.synchronize()
    return eng, st, starts, lanes, group


def run_cut(db, eng, st, stream=None):
    from bgx import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    B = st["group"].numel()
    _lib.check(_lib.load().bgx_rollout_bearoff_cut(db.handle(), ctypes.c_void_p(eng.lanes_ptr()), p(st["starts"]),
                                                   p(st["group"]), B, 4, 3, p(st["games_done"]), p(st["plies"]),
                                                   p(st["sel"]), p(st["cut_tally"]), p(st["active"]), p(st["mask"]),
                                                   stream), "bgx_rollout_bearoff_cut")


def test_a_cut_lane_restarts_from_its_start_record(db6):
    from bgx.bearoff import lookup_reference
    from bgx.rollout import CUT_ONE
    eng, st, starts, lanes, group = posed(db6)
    in_db, w = lookup_reference(lanes, db6.configs().cpu().numpy(), db6.table().cpu().numpy(), 6)
    want = in_db & (group >= 0)
    assert 20 < want.sum() < len(group) - 20
    run_cut(db6, eng, st)
    mask = st["mask"].cpu().numpy()
    assert np.array_equal(mask, want.astype(np.uint8))                 # written on every lane, 1 or 0
    assert np.array_equal(st["games_done"].cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(st["plies"].cpu().numpy(), np.where(want, 0, 2))
    w = np.where(want, w, F(0)).astype(F)
    q = np.where(lanes[:, 52] == starts[:, 52], w, (F(1) - w).astype(F))
    pq = np.rint((q * F(CUT_ONE)).astype(F)).astype(np.int64)
    ref = np.zeros((4, 4), np.int64)
    for f, v in enumerate((np.ones_like(pq), np.full_like(pq, 2), pq, pq * pq)):
        np.add.at(ref[:, f], group[want], v[want])
    assert np.array_equal(st["cut_tally"].cpu().numpy(), ref)
    assert int(st["active"]) == (group >= 0).sum() and bool((st["sel"].cpu().numpy() == (group >= 0)).all())
    eng.reset(lane_mask=st["mask"], want_obs=False)
    after = eng.records().cpu().numpy()
    assert np.array_equal(after[want, :53], starts[want, :53])
    fixed = want & (starts[:, 53] != 0)
    assert fixed.any() and np.array_equal(after[fixed, 53:55], starts[fixed, 53:55])
    drawn = after[want & (starts[:, 53] == 0), 53:55]
    assert drawn.size and ((drawn >= 1) & (drawn <= 6)).all()
    assert np.array_equal(after[~want, :55], lanes[~want, :55])        # the other lanes are untouched
    assert eng.error() == 0


# ------------------------------------------------------------------ graph capture --
def test_graph_capture(db6):
    """lookup, act and cut captured into one graph replay to the eager results."""
    eng, st, starts, lanes, group = posed(db6, seed=8)
    B = len(group)
    recs = eng.records()
    bufs = []
    for _ in range(2):
        bufs.append(dict(in_db=torch.full((B,), 5, dtype=torch.uint8, device="cuda"),
                         win=torch.full((B,), float("nan"), device="cuda"),
                         act=torch.full((B,), -3, dtype=torch.int32, device="cuda"),
                         in_db2=torch.full((B,), 5, dtype=torch.uint8, device="cuda")))
    state0 = {k: v.clone() for k, v in st.items()}

    def work(b):
        db6.lookup(recs, out=(b["in_db"], b["win"]))
        db6.act(eng, st["sel"], b["act"], b["in_db2"])
        run_cut(db6, eng, st, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    work(bufs[0])
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in st.items()}
    assert int(eager["cut_tally"][:, 0].sum()) > 20
    for k, v in state0.items():
        st[k].copy_(v)
    cap = torch.cuda.Stream()
    with torch.cuda.stream(cap):
        eng.join()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        work(bufs[1])
    torch.cuda.synchronize()
    for k, v in state0.items():                            # the capture ran nothing
        assert torch.equal(st[k], v), k
    g.replay()
    torch.cuda.synchronize()
    for k in bufs[0]:                                      # win by its bits: NaN where not in the table
        a, b = (bufs[j][k].view(torch.int32) if k == "win" else bufs[j][k] for j in (0, 1))
        assert torch.equal(a, b), k
    assert bool((bufs[1]["in_db"] <= 1).all()) and bool((bufs[1]["act"] >= 0).any())
    for k, v in eager.items():
        assert torch.equal(st[k], v), k
    assert eng.error() == 0


# ---------------------------------------------------------------------- refusals --
def test_refusals(db3):
    from bgx import _lib
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffDB
    from bgx.rollout import Rollout
    L = _lib.load()
    for k in (0, 9, -1):
        h = ctypes.c_void_p()
        assert L.bgx_bearoff_create(0, k, None, ctypes.byref(h)) == _lib.BGX_EINVAL and not h.value
        with pytest.raises(ValueError):
            BearoffDB(k)
    assert L.bgx_bearoff_create(0, 3, None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_destroy(None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_buffers_get(None, None) == _lib.BGX_EINVAL
    ro = Rollout(64, seed=0)
    with pytest.raises(ValueError, match="luck"):
        ro.run(RandomPlayer(1), torch.from_numpy(START[None]), 36, luck=object(), bearoff=db3)
    z = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = lambda x: x.data_ptr()
    good = [db3.handle(), ro.eng.lanes_ptr(), p(z), p(i32), 64, 1, 1, p(ro.games_done), p(ro.plies), p(ro.sel), p(t),
            p(ro.active), p(z), None]
    for idx, val in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, 0), (6, -1), (7, None), (8, None),
                     (9, None), (10, None), (11, None), (12, None), (1, ro.eng.lanes_ptr() + 4)):
        bad = list(good)
        bad[idx] = val
        assert L.bgx_rollout_bearoff_cut(*bad) == _lib.BGX_EINVAL, idx
    assert L.bgx_bearoff_lookup(None, p(z), 64, p(z), None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_lookup(db3.handle(), p(z), -1, p(z), None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_lookup(db3.handle(), p(z), 64, None, None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_act(None, db3.handle(), None, p(i32), None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_act(ro.eng._h, None, None, p(i32), None, None) == _lib.BGX_EINVAL
    assert L.bgx_bearoff_act(ro.eng._h, db3.handle(), None, None, None, None) == _lib.BGX_EINVAL
    torch.cuda.synchronize()
