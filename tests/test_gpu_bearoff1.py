"""The one-sided bearoff database on the device (csrc/bg_bearoff1.h, bgx/bearoff.py): every
entry at K = 5 against the numpy recurrence on BearoffDB's own successor sets and against the
exact table, the K = 15 build against the oracle's move generator on sampled rows, lookup, play,
the rollout cut against its host replay, nesting under the exact table, the command line."""
import json
import math

import numpy as np
import pytest
import torch

import bearoff_ref as BR

pytestmark = pytest.mark.gpu

F = np.float32
# the means of six and of fifteen checkers on the six point by the recurrence on the host
# (tools/bearoff1_host.cpp table 15; tests/test_bearoff1_cpu.py): 5.312426 and 12.266191
MEAN_6x6, MEAN_15x6 = 0x40A9FF65, 0x41444252


@pytest.fixture(scope="module")
def one5():
    from bgx.bearoff import OneSidedBearoffDB
    return OneSidedBearoffDB(5)


@pytest.fixture(scope="module")
def one15():
    from bgx.bearoff import OneSidedBearoffDB
    return OneSidedBearoffDB(15)


@pytest.fixture(scope="module")
def host15(one15):
    """The K = 15 table's buffers on the host, copied once."""
    return dict(configs=one15.configs().cpu().numpy(), dist=one15.dist().cpu().numpy(),
                surv=one15.surv().cpu().numpy(), mean=one15.mean().cpu().numpy(),
                choice=one15.choice().cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ table, K = 5 --
def test_k5_every_entry_and_distance_to_the_exact_table(one5):
    """Bit for bit the numpy recurrence fed with BearoffDB(5)'s successor sets; win1 over all
    pairs against the exact table: max |d| < 0.0137, mean |d| < 0.00085 (the fp32 recurrence
    against an fp64 exact table on the host gives 0.013534 and 0.00080; the device's two fp32
    tables give 0.0135334 and 0.00080170)."""
    from bgx.bearoff import BearoffDB, dist_reference, win1_reference
    db = BearoffDB(5)
    n = db.n
    assert one5.n == n == 462 and one5.K == 5
    assert torch.equal(one5.configs(), db.configs())
    dist, surv, mean, choice = dist_reference([db.successors(i) for i in range(n)], n)
    got = [t.cpu().numpy() for t in (one5.dist(), one5.surv(), one5.mean(), one5.choice())]
    assert got[0].shape == (n, 32) and got[1].shape == (n, 32) and got[2].shape == (n,) and got[3].shape == (n, 21)
    assert np.array_equal(got[3], choice), int((got[3] != choice).sum())
    for name, a, b in (("dist", got[0], dist), ("surv", got[1], surv), ("mean", got[2], mean)):
        assert np.array_equal(bits(a), bits(b)), (name, int((bits(a) != bits(b)).sum()))
    # win1 of every pair of non-empty configurations, through the device's lookup
    cfg = db.configs().cpu().numpy()
    recs = np.zeros((n - 1, n - 1, 64), np.uint8)
    recs[:, :, 23:17:-1] = cfg[1:, None, :]
    recs[:, :, 24:30] = cfg[None, 1:, :]
    recs[:, :, 50] = 15 - cfg[1:].sum(1)[:, None]
    recs[:, :, 51] = 15 - cfg[1:].sum(1)[None, :]
    in_db, win = one5.lookup(torch.from_numpy(recs.reshape(-1, 64)).cuda())
    assert bool((in_db == 1).all())
    win = win.cpu().numpy().reshape(n - 1, n - 1)
    assert np.array_equal(bits(win), bits(win1_reference(dist[1:, None, :], surv[None, 1:, :])))
    d = np.abs(win.astype(np.float64) - db.table().cpu().numpy()[1:, 1:].astype(np.float64))
    print("K = 5: win1 against the exact table, max", d.max(), "mean", d.mean())
    assert d.max() < 0.0137 and d.mean() < 0.00085, (d.max(), d.mean())


# ----------------------------------------------------------------- table, K = 15 --
def test_k15_build(one15, host15):
    n = one15.n
    assert n == 54264 == math.comb(21, 6) and one15.K == 15
    cfg, dist, mean = host15["configs"].astype(np.int64), host15["dist"], host15["mean"]
    pip = cfg @ np.arange(1, 7)
    key = cfg @ (16 ** np.arange(6))
    order = np.lexsort((key, pip))
    assert np.array_equal(order, np.arange(n)) and not cfg[0].any() and cfg.sum(1).max() == 15
    assert not dist[:, 31].any() and not dist[1:, 0].any() and dist[0, 0] == 1
    sums = dist.astype(np.float64).sum(1)
    print("K = 15: row sums", sums.min(), sums.max(), "last non-zero t", int(np.nonzero(dist.any(0))[0].max()))
    assert np.abs(sums - 1).max() <= 1e-6
    assert bits(mean[one15.index_of((0, 0, 0, 0, 0, 6))]) == MEAN_6x6
    assert bits(mean[one15.index_of((0, 0, 0, 0, 0, 15))]) == MEAN_15x6
    assert (host15["choice"][1:] < np.arange(1, n)[:, None]).all() and not host15["choice"][0].any()
    with pytest.raises(ValueError):
        one15.index_of((0, 0, 0, 0, 0, 16))


def test_k15_sampled_rows_against_the_oracle(one15, host15):
    """200 sampled configurations and fifteen on the six point: the choice row is the (mean,
    index) argmin over the oracle's successor sets, the dist row the numpy one-step recurrence
    from the device's lower rows.  The sample holds sets of more than 64 configurations."""
    from bgx.bearoff import row_reference
    dist, surv, mean, choice = (host15[k] for k in ("dist", "surv", "mean", "choice"))
    rng = np.random.RandomState(15)
    # half of the sample has 12..15 checkers spread over the points (the large sets)
    sample = [one15.index_of((0, 0, 0, 0, 0, 15)), one15.index_of((1, 2, 2, 3, 3, 4))]
    sample += list(rng.randint(1, one15.n, 100))
    while len(sample) < 201:
        c = np.bincount(rng.randint(0, 6, rng.randint(12, 16)), minlength=6)
        sample.append(one15.index_of(tuple(c)))
    widest = 0
    for a in sample:
        c = tuple(int(v) for v in host15["configs"][a])
        want = np.zeros(21, np.int32)
        for r, s in enumerate(BR.oracle_successors(c)):
            idx = [one15.index_of(x) for x in s]
            widest = max(widest, len(idx))
            want[r] = min((mean[i], i) for i in idx)[1]
        assert np.array_equal(choice[a], want), (c, choice[a], want)
        d, s, m = row_reference(dist[choice[a]])
        assert np.array_equal(bits(dist[a]), bits(d)) and np.array_equal(bits(surv[a]), bits(s)), c
        assert bits(mean[a]) == bits(m), c
    assert widest > 64, widest


# ------------------------------------------------------------------------ lookup --
def lookup_cases():
    good = BR.record((1, 1, 0, 2, 0, 1), (0, 2, 0, 0, 1, 0), 0)
    full = (2, 2, 2, 3, 3, 3)                               # all 15 on the board
    recs = {"in 1": good, "in 1, PLAYER2 on roll": BR.record((1, 1, 0, 2, 0, 1), (0, 2, 0, 0, 1, 0), 1, (3, 1)),
            "in 1, 14 against 9": BR.record((2, 2, 2, 3, 3, 2), (1, 1, 1, 2, 2, 2), 1),
            "in 2, PLAYER1 full": BR.record(full, (0, 2, 0, 0, 1, 0), 0),
            "in 2, PLAYER2 full, on roll": BR.record((0, 0, 0, 0, 0, 1), full, 1),
            "in 2, both full": BR.record(full, (0, 0, 0, 0, 0, 15), 0)}
    r = good.copy(); r[23] -= 1; r[17] += 1; recs["0: an outfield checker"] = r
    r = good.copy(); r[24 + 1] -= 1; r[24 + 6] += 1; recs["0: a PLAYER2 outfield checker"] = r
    r = good.copy(); r[23] -= 1; r[48] += 1; recs["0: a checker on the bar"] = r
    r = good.copy(); r[24 + 1] -= 1; r[49] += 1; recs["0: a PLAYER2 checker on the bar"] = r
    r = good.copy(); r[55] = 1; recs["0: game over"] = r
    recs["0: 15 off"] = BR.record((0,) * 6, (0, 2, 0, 0, 1, 0), 1)
    r = good.copy(); r[50] -= 1; recs["0: a wrong sum"] = r
    r = good.copy(); r[51] += 1; recs["0: a wrong sum, PLAYER2"] = r
    r = good.copy(); r[23] = 16; r[50] = 0; recs["0: 20 on the board"] = r
    return recs


def test_lookup(one15, one5, host15):
    from bgx.bearoff import lookup1_reference
    cases = lookup_cases()
    recs = np.stack(list(cases.values()))
    dev = torch.from_numpy(recs).cuda()
    in_db, win = one15.lookup(dev)
    in_db, win = in_db.cpu().numpy(), win.cpu().numpy()
    want = [int(name.split(":")[0].split(",")[0].replace("in ", "")) for name in cases]
    assert in_db.tolist() == want and in_db.dtype == np.uint8
    ref_in, ref_win = lookup1_reference(recs, host15["configs"], host15["dist"], host15["surv"], 15)
    assert np.array_equal(ref_in, in_db)
    assert np.array_equal(bits(win), bits(ref_win))            # NaN where not in the table: left unwritten
    # (a sure win or loss is 0 or 1 to the fp32 rest of the row sums)
    assert np.isnan(win[in_db == 0]).all() and ((win[in_db != 0] > -1e-6) & (win[in_db != 0] < 1 + 1e-6)).all()
    # entries not in the table keep what `out` held; in_db alone (win NULL)
    out = (torch.full((len(recs),), 9, dtype=torch.uint8, device="cuda"), torch.full((len(recs),), -5.0, device="cuda"))
    one15.lookup(dev, out=out)
    assert np.array_equal(out[0].cpu().numpy(), in_db) and (out[1].cpu().numpy()[in_db == 0] == -5).all()
    # K = 5: the larger configurations are outside, the values inside are the same
    in5, win5 = one5.lookup(dev)
    in5, win5 = in5.cpu().numpy(), win5.cpu().numpy()
    assert in5.tolist() == [1, 1] + [0] * (len(recs) - 2) and np.array_equal(bits(win5[:2]), bits(win[:2]))
    with pytest.raises(ValueError):
        one15.lookup(dev[:, :52])


# --------------------------------------------------------------------------- act --
def race_records(B, seed, lo=1, hi=15):
    """Home-board races with lo..hi checkers a side and a roll to play."""
    rng = np.random.RandomState(seed)
    recs = np.zeros((B, 64), np.uint8)
    for i in range(B):
        c = [tuple(np.bincount(rng.randint(0, 6, rng.randint(lo, hi + 1)), minlength=6)) for _ in range(2)]
        recs[i] = BR.record(c[0], c[1], i % 2, BR.ROLLS21[(i * 5) % 21])
    return recs


def host_best_moves(recs, lanes, moves, win_after):
    """Per lane the first argmax over the engine's move list of win_after(opponent's
    configuration, mover's afterstate configuration); -1 without a move."""
    import oracle as O
    out = []
    for i in range(len(recs)):
        mover = int(recs[i, 52])
        nm = int(lanes[i, 60]) | (int(lanes[i, 61]) << 8)
        board = recs[i, :52].view(np.int8)
        opp = BR.config_of(board, 1 - mover)
        vals = [win_after(opp, BR.config_of(O.apply_move(board, mover, int(m)), mover)) for m in moves[i, :nm]]
        out.append(int(np.argmax(np.asarray(vals, F))) if nm else -1)
    return out


def test_act_is_the_first_argmax(one15, host15):
    from bgx.bearoff import win1_reference
    from bgx.engine import Engine
    import oracle as O
    B = 64
    recs = race_records(B, 3)
    recs[5] = BR.record((0, 0, 0, 0, 0, 1), (1, 0, 0, 0, 0, 0), 0, (6, 6))     # every play bears the last checker off
    recs[9] = BR.record((2, 2, 2, 3, 3, 3), (0, 3, 0, 0, 1, 0), 0, (4, 2))     # in_db 2
    recs[11] = 0                                                            # outside the table: the opening
    recs[11, :52] = O.INITIAL_BOARD52.view(np.uint8)
    recs[11, 53:55] = (3, 1)
    recs[20] = BR.record((0, 0, 0, 0, 0, 2), (1, 0, 0, 0, 0, 0), 0, (2, 1))
    recs[20, 24], recs[20, 24 + 7] = 0, 1                                   # a PLAYER2 outfield checker
    sel = np.ones(B, np.uint8)
    unselected = [0, 33, 63]
    sel[unselected] = 0
    eng = Engine(batch=B, max_moves=500, seed=1, dice="philox")
    eng.reset(want_obs=False)
    eng.set_lanes(torch.from_numpy(recs))
    # a lane without a move (a race always has one): its count zeroed in the engine's record
    blocked = eng.records()[7:8].clone()
    blocked[0, 60:62] = 0
    eng.set_lanes(blocked, lane0=7, regen=False)
    act = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    in_db = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    one15.act(eng, torch.from_numpy(sel).cuda(), act, in_db)
    lanes, moves, _ = eng.lanes()
    lanes, moves = lanes.cpu().numpy(), moves.cpu().numpy().view(np.uint64)
    act, in_db = act.cpu().numpy(), in_db.cpu().numpy()
    assert eng.error() == 0
    dist, surv = host15["dist"], host15["surv"]

    def win_after(opp, after):
        if not any(after):
            return F(1)
        return F(F(1) - win1_reference(dist[one15.index_of(opp)], surv[one15.index_of(after)]))

    want = host_best_moves(recs, lanes, moves, win_after)
    assert (lanes[7, 60], lanes[7, 61]) == (0, 0) and want[7] == -1
    for i in range(B):
        if i in unselected or i in (11, 20):
            assert act[i] == -7 and in_db[i] == 0, i
        else:
            assert in_db[i] == 1 + (recs[i, 50] == 0 or recs[i, 51] == 0), i
            assert act[i] == (-7 if i == 7 else want[i]), (i, act[i], want[i])
    assert in_db[9] == 2 and (in_db == 1).sum() > 40
    # NULL selection = every lane; NULL in_db
    act2 = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    one15.act(eng, None, act2)
    act2 = act2.cpu().numpy()
    assert (act2[[7, 11, 20]] == -7).all() and all(act2[i] == want[i] for i in range(B) if i not in (7, 11, 20))


# ---------------------------------------------------------------- cut bookkeeping --
def cut_starts(B, seed):
    """Two positions: a race of 11..14 checkers a side a few plies in (cut at step 0), and one
    whose PLAYER1 still has all 15 checkers on the board (in the table, in_db 2: played on
    until a checker is off)."""
    pos = np.stack([BR.record((1, 2, 2, 3, 3, 2), (2, 2, 2, 2, 2, 1), 0),
                    BR.record((2, 2, 2, 3, 3, 3), (2, 2, 3, 2, 2, 2), 0)])
    group = (np.arange(B) >= B // 2).astype(np.int32)
    starts = pos[group].copy()
    rng = np.random.RandomState(seed)
    for i in range(1, B, 2):                                 # every other lane with a fixed roll
        starts[i, 53:55] = (rng.randint(1, 7), rng.randint(1, 7))
    group[[3, 40]] = -1
    return starts, group


def cut_run(db, starts, group, G):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    ro = Rollout(len(group), seed=4)
    tally, unfinished, tr, cut_tally = ro.run_lanes(RandomPlayer(5), torch.from_numpy(starts), torch.from_numpy(group),
                                                    2, G, max_steps=200, trace=True, bearoff=db)
    assert ro.eng.error() == 0
    return tally.cpu().numpy(), unfinished.cpu().numpy(), tr, cut_tally.cpu().numpy()


def test_cut_bookkeeping_equals_host_replay(one15, host15):
    from bgx.bearoff import lookup1_reference
    from bgx.rollout import bearoff_cut_reference, summarize_bearoff
    B, G = 64, 2
    starts, group = cut_starts(B, 2)
    runs = [cut_run(one15, starts, group, G) for _ in range(2)]
    tally, unfinished, tr, cut_tally = runs[0]

    def lookup(recs):
        in_db, w = lookup1_reference(recs, host15["configs"], host15["dist"], host15["surv"], 15)
        return in_db == 1, w

    ref = bearoff_cut_reference(tr["cut_records0"].cpu().numpy(), tr["cut_records"].cpu().numpy(),
                                tr["done"].cpu().numpy(), tr["info"].cpu().numpy(), starts, group, 2, G, lookup=lookup)
    assert np.array_equal(cut_tally, ref["cut_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    assert np.array_equal(tr["cut0"].cpu().numpy() != 0, ref["cut0"])
    assert np.array_equal(tr["cut"].cpu().numpy() != 0, ref["cut"])
    # position 0 is cut before a move; position 1 (15 checkers on the board) not at step 0, later yes
    cut0 = tr["cut0"].cpu().numpy() != 0
    assert cut0[group == 0].all() and not cut0[group != 0].any()
    assert cut_tally[1, 0] > 0 and cut_tally[1, 1] >= cut_tally[1, 0]
    scheduled = np.bincount(group[group >= 0], minlength=2) * G
    assert not unfinished.any() and np.array_equal(tally[:, 0] + cut_tally[:, 0], scheduled)
    r = summarize_bearoff(tally[0], cut_tally[0], unfinished[0])
    assert r["cut_share"] == 1.0 and r["games"] == scheduled[0]
    # run to run identical
    assert np.array_equal(runs[1][3], cut_tally) and np.array_equal(runs[1][0], tally)
    for k in ("done", "info", "action", "mover", "cut", "cut_records"):
        assert torch.equal(runs[1][2][k], tr[k]), k


def test_run_reports_the_kind(one15):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    pos = BR.record((1, 2, 2, 3, 3, 2), (2, 2, 2, 2, 2, 1), 0)
    ro = Rollout(64, seed=3)
    r, = ro.run(RandomPlayer(1), torch.from_numpy(pos[None]), 36, bearoff=one15)     # one game a lane: cut at the start
    assert r["bearoff_kind"] == "one-sided" and r["cut_share"] == 1.0 and r["games"] == 36
    assert r["equity_stderr"] == 0.0 and -1 < r["equity"] < 1
    with pytest.raises(ValueError, match="luck"):
        ro.run(RandomPlayer(1), torch.from_numpy(pos[None]), 36, luck=object(), bearoff=one15)


# ----------------------------------------------------------------------- nesting --
def test_nesting_plays_the_exact_table_inside(one15, host15):
    """BearoffPlayer(OneSidedPlayer(inner, db1), db6): lanes in the K = 6 table get the exact
    table's move, other races the one-sided table's, the rest the inner player's."""
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffDB, BearoffPlayer, OneSidedPlayer, win1_reference
    from bgx.engine import Engine
    import oracle as O
    B = 64
    recs = race_records(B, 21, lo=3, hi=9)
    recs[10] = 0
    recs[10, :52] = O.INITIAL_BOARD52.view(np.uint8)
    recs[10, 53:55] = (6, 4)
    db6 = BearoffDB(6)
    eng = Engine(batch=B, max_moves=500, seed=1, dice="philox")
    eng.reset(want_obs=False)
    eng.set_lanes(torch.from_numpy(recs))
    inner = RandomPlayer(9)
    player = BearoffPlayer(OneSidedPlayer(inner, one15), db6)
    assert player.sync_free == bool(getattr(inner, "sync_free", False))
    sel = torch.ones(B, dtype=torch.uint8, device="cuda")
    act = player.act(eng, sel, 0).cpu().numpy()
    inner_act = inner.act(eng, sel, 0).cpu().numpy()
    lanes, moves, _ = eng.lanes()
    lanes, moves = lanes.cpu().numpy(), moves.cpu().numpy().view(np.uint64)
    W = db6.table().cpu().numpy()
    dist, surv = host15["dist"], host15["surv"]
    exact = host_best_moves(recs, lanes, moves, lambda opp, after: F(1) if not any(after) else
                            F(1) - W[db6.index_of(opp), db6.index_of(after)] if sum(opp) <= 6 and sum(after) <= 6 else F(0))
    one = host_best_moves(recs, lanes, moves, lambda opp, after: F(1) if not any(after) else
                          F(F(1) - win1_reference(dist[one15.index_of(opp)], surv[one15.index_of(after)])) if sum(opp) else F(0))
    in6 = (recs[:, 18:24].sum(1) <= 6) & (recs[:, 24:30].sum(1) <= 6)
    in6[10] = False
    assert 10 < in6.sum() < B - 10
    differ = 0
    for i in range(B):
        if i == 10:
            assert act[i] == inner_act[i]
        elif in6[i]:
            assert act[i] == exact[i], i
            differ += exact[i] != one[i]
        else:
            assert act[i] == one[i], i
    print("nesting: lanes in the K = 6 table where the two tables' moves differ:", differ)


# ------------------------------------------------------------------ command line --
def test_command_line(tmp_path, capsys):
    from bgx import rollout as R
    pos = tmp_path / "pos.json"
    rec = BR.record((1, 2, 2, 3, 3, 2), (2, 2, 2, 2, 2, 1), 0)
    pos.write_text(json.dumps([{"board": [int(v) for v in rec[:52]], "player": 0}]))
    R.main(f"--net random --positions {pos} --trials 36 --batch 64 --bearoff1 15 --bearoff1-play --bearoff-play 4".split())
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2
    assert lines[0]["bearoff_kind"] == "one-sided" and lines[0]["cut_share"] == 1.0 and lines[0]["games"] == 36
    s = lines[1]
    assert s["summary"] and s["bearoff1"] == 15 and s["bearoff1_play"] == 15 and s["bearoff_play"] == 4
    assert s["bearoff"] is None and s["cut_games"] == 36
