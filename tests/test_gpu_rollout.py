"""Position rollouts (bgx/rollout.py on the engine's start table and the rollout kernels):
the device tallies against a host replay of the traced steps, positions whose result is known
exactly whoever plays, rollout_moves, the search players, the command line."""
import json

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

GAMES, PLIES, WIN1, LOSS1 = 0, 1, 2, 5


def record(p1, p2, mover, roll=(0, 0), bar=(0, 0)):
    """p1 / p2: {point byte: count}; off = 15 - the rest."""
    r = np.zeros(64, np.uint8)
    for k, v in list(p1.items()) + list(p2.items()):
        r[k] = v
    r[48], r[49] = bar
    r[50] = 15 - r[:24].sum() - r[48]
    r[51] = 15 - r[24:48].sum() - r[49]
    r[52] = mover
    r[53], r[54] = roll
    return r


CASE_A = record({18: 1}, {24: 1}, 0)                     # 27 of the 36 rolls bear the checker off
CASE_B = record({23: 1}, {29: 15}, 0)                    # always a gammon
CASE_C = record({23: 1}, {29: 14}, 0, bar=(0, 1))        # always a backgammon
CASE_D = record({23: 1}, {24 + 5: 1}, 1)                 # the mirror of (a), PLAYER2 on roll


def outcomes(board, mover, roll):
    """The set of results over the legal moves of one roll: the game's points when the move
    ends the game (exact_score), 0 when it does not; and the afterstates (a pass: the board)."""
    from bgx.rollout import exact_score
    moves, n = O.movegen(board, mover, roll)
    afters = [O.apply_move(board, mover, int(m)) for m in moves] if n else [np.array(board, np.int8)]
    return {exact_score(a, mover) for a in afters}, afters


def expected_tally(rec, per_roll):
    """The tally row of `per_roll` games on each of the 36 ordered first rolls of a position
    that is decided within two plies whatever the moves (asserted: no roll is "mixed")."""
    board, mover = rec[:52].view(np.int8), int(rec[52])
    t = np.zeros(8, np.int64)
    for a in range(1, 7):
        for b in range(1, 7):
            res, afters = outcomes(board, mover, (a, b))
            assert len(res) == 1, ("mixed first roll", a, b)
            s = res.pop()
            plies = 1
            if s == 0:                               # no move ends it: the opponent must win at once
                rep = set()
                for aft in afters:
                    for c in range(1, 7):
                        for d in range(1, 7):
                            rep |= outcomes(aft, 1 - mover, (c, d))[0]
                assert len(rep) == 1 and 0 not in rep, ("mixed reply", a, b, rep)
                s, plies = -rep.pop(), 2
            t[GAMES] += per_roll
            t[PLIES] += per_roll * plies
            t[(WIN1 if s > 0 else LOSS1) + abs(s) - 1] += per_roll
    return t


def row_of(res):
    from bgx.rollout import FIELDS
    return np.array([res[k] for k in FIELDS], np.int64)


# ------------------------------------------------------ kernels against numpy --
def small_starts(B, seed):
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        p1 = {18 + p: 1 for p in rng.choice(6, rng.randint(1, 4), replace=False)}
        p2 = {24 + p: 1 for p in rng.choice(6, rng.randint(1, 4), replace=False)}
        roll = (rng.randint(1, 7), rng.randint(1, 7)) if i % 2 else (0, 0)
        s[i] = record(p1, p2, rng.randint(2), roll)
    return s


def replay(tr, starts, group, P, G):
    done, info = tr["done"].cpu().numpy(), tr["info"].cpu().numpy()
    B = len(group)
    tally = np.zeros((P, 8), np.int64)
    gd, plies = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for t in range(done.shape[0]):
        for i in range(B):
            if group[i] < 0 or gd[i] >= G:
                continue
            plies[i] += 1
            winner, score = ((info[t, i] >> 8) & 0xFF) - 1, (info[t, i] >> 16) & 0xFF
            if done[t, i] and winner >= 0:
                row = tally[group[i]]
                row[GAMES] += 1
                row[PLIES] += plies[i]
                row[(WIN1 if winner == starts[i, 52] else LOSS1) + score - 1] += 1
                plies[i] = 0
                gd[i] += 1
    return tally, gd


def test_tallies_equal_host_replay():
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    B, P, G = 200, 5, 2
    sizes = [10, 50, 33, 64, 36]
    group = np.repeat(np.arange(P), sizes).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):            # 7 idle lanes, in the middle of waves and groups
        group = np.insert(group, k, -1)
    assert len(group) == B and (group < 0).sum() == 7
    starts = small_starts(B, 12)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=4)
        tally, unfinished, tr = ro.run_lanes(RandomPlayer(5), torch.from_numpy(starts), torch.from_numpy(group), P, G,
                                             max_steps=200, trace=True)
        assert ro.eng.error() == 0
        runs.append((tally.cpu().numpy(), unfinished.cpu().numpy(), tr))
    tally, unfinished, tr = runs[0]
    ref, gd = replay(tr, starts, group, P, G)
    assert np.array_equal(tally, ref)
    assert np.array_equal(tr["games_done"].cpu().numpy(), gd)
    assert tr["active"] == int(((group >= 0) & (gd < G)).sum()) == 0 and not unfinished.any()
    assert np.array_equal(tally[:, GAMES], np.bincount(group[group >= 0], minlength=P) * G)
    # idle lanes are given action 0 and belong to nobody; the lanes' movers are the records'
    assert not tr["action"].cpu().numpy()[:, group < 0].any()
    # run to run identical
    assert np.array_equal(runs[1][0], tally)
    for k in ("done", "info", "action", "mover"):
        assert torch.equal(runs[1][2][k], tr[k])


def test_argument_checks():
    from bgx import _lib
    from bgx.rollout import Rollout
    ro = Rollout(64, seed=0)
    L = _lib.load()
    z = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    grp = torch.zeros(64, dtype=torch.int32, device="cuda")
    t8 = torch.zeros(8, dtype=torch.int64, device="cuda")
    good = [ro.eng.lanes_ptr(), p(z), p(grp), 64, 1, 1, p(ro.games_done), p(ro.plies), p(ro.sel), p(t8), p(ro.active), None]
    assert L.bgx_rollout_begin(*good) == _lib.BGX_OK
    for idx, val in ((3, 0), (4, 0), (5, -1), (0, None), (1, None), (2, None), (6, None), (7, None), (8, None),
                     (9, None), (10, None)):
        bad = list(good)
        bad[idx] = val
        assert L.bgx_rollout_begin(*bad) == _lib.BGX_EINVAL, idx
    good = [ro.eng.lanes_ptr(), p(z), p(grp), p(ro.eng.done), p(ro.eng.info), 64, 1, 1, p(ro.games_done), p(ro.plies),
            p(ro.sel), p(t8), p(ro.active), None]
    for idx, val in ((5, 0), (6, 0), (7, -1), (0, None), (1, None), (2, None), (3, None), (4, None), (8, None),
                     (9, None), (10, None), (11, None), (12, None)):
        bad = list(good)
        bad[idx] = val
        assert L.bgx_rollout_advance(*bad) == _lib.BGX_EINVAL, idx
    torch.cuda.synchronize()


# ------------------------------------------------------------- exact results --
@pytest.fixture(scope="module")
def ro128():
    from bgx.rollout import Rollout
    return Rollout(128, seed=2)


def test_exact_positions_stratified(ro128):
    """Four positions in one run (36 x 4 units on 128 lanes: two passes, one lane per unit,
    two games per lane)."""
    from bgx.arena import RandomPlayer
    cases = np.stack([CASE_A, CASE_B, CASE_C, CASE_D])
    res = ro128.run(RandomPlayer(1), torch.from_numpy(cases), 72)
    want = [expected_tally(c, 2) for c in cases]
    assert want[0][WIN1] == 27 * 2 and want[0][LOSS1] == 9 * 2 and want[3][WIN1] == 27 * 2     # the counts known by hand
    for r, w in zip(res, want):
        assert np.array_equal(row_of(r), w), (r, w)
        assert r["unfinished"] == 0
    a, b, c, d = res
    assert a["equity"] == 0.5 and d["equity"] == 0.5 and a["win"] == 0.75
    assert b["win2"] == b["games"] == 72 and b["equity"] == 2.0 and b["equity_stderr"] == 0.0
    assert b["plies_per_game"] == 1.0
    assert c["win3"] == c["games"] == 72 and c["equity"] == 3.0
    assert ro128.eng.error() == 0


def test_random_first_rolls():
    """4,096 games of (a) with drawn first rolls: the win rate within 5 binomial standard
    deviations (5 x 0.0068) of 27 / 36."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    ro = Rollout(1024, seed=9)
    r, = ro.run(RandomPlayer(3), torch.from_numpy(CASE_A[None]), 4096, first_roll="random")
    assert r["games"] == 4096 and r["unfinished"] == 0
    assert r["win1"] + r["loss1"] == 4096
    print("win rate", r["win"])
    assert abs(r["win"] - 27 / 36) <= 5 * 0.0068
    assert ro.eng.error() == 0


# -------------------------------------------------------------- rollout_moves --
def test_rollout_moves_exact(ro128):
    from bgx.arena import RandomPlayer
    from bgx.rollout import rollout_moves
    dec = CASE_B.copy()
    dec[53:55] = (3, 1)
    out = rollout_moves(ro128, RandomPlayer(1), torch.from_numpy(dec), 36)
    moves, n = O.movegen(dec[:52].view(np.int8), 0, (3, 1))
    assert len(out) == n > 0 and {o["move"] for o in out} == {int(m) for m in moves}
    for o in out:
        assert o["exact"] and o["equity"] == 2.0 and o["games"] == 0


def test_rollout_moves_sorts_the_winner_first(ro128):
    from bgx.arena import RandomPlayer
    from bgx.rollout import rollout_moves
    # 2-1 to play with checkers on the 2- and 1-points: both off (wins), or 22 -> 23 -> off
    dec = record({22: 1, 23: 1}, {24: 1}, 0, roll=(2, 1))
    out = rollout_moves(ro128, RandomPlayer(1), torch.from_numpy(dec), 36)
    moves, n = O.movegen(dec[:52].view(np.int8), 0, (2, 1))
    wins = [int(m) for m in moves if O.apply_move(dec[:52].view(np.int8), 0, int(m))[50] == 15]
    assert len(out) == n and 0 < len(wins) < n
    assert [o["move"] for o in out[:len(wins)]] == wins or {o["move"] for o in out[:len(wins)]} == set(wins)
    for o in out:
        if o["move"] in wins:
            assert o["exact"] and o["equity"] == 1.0 and o["games"] == 0
        else:                                           # the opponent bears its last checker off at once
            assert not o["exact"] and o["equity"] == -1.0 and o["games"] == 36 and o["equity_stderr"] == 0.0
    assert ro128.eng.error() == 0


# -------------------------------------------------------------------- players --
@pytest.mark.parametrize("kind", ["1ply", "2ply"])
def test_search_players(ro128, kind):
    from bgx.arena import OnePlyPlayer, TwoPlyPlayer
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    net = PolicyNet(hidden_size=128).cuda()
    player = OnePlyPlayer(net) if kind == "1ply" else TwoPlyPlayer(net, top_k=2)
    cases = np.stack([CASE_A, CASE_D])
    res = ro128.run(player, torch.from_numpy(cases), 36)
    for r, c in zip(res, cases):
        assert np.array_equal(row_of(r), expected_tally(c, 1)), r
    assert ro128.eng.error() == 0


def test_policy_player(ro128):
    from bgx.arena import PolicyPlayer
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    net = PolicyNet(hidden_size=128).cuda()
    r, = ro128.run(PolicyPlayer(net, seed=3), torch.from_numpy(CASE_A[None]), 108)
    assert np.array_equal(row_of(r), expected_tally(CASE_A, 3))


# ----------------------------------------------------------------------- CLI --
def test_command_line(capsys):
    from bgx import rollout
    rollout.main(["--net", "random", "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps",
                  "4000"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["position"] == 0 and lines[1]["summary"]
    assert lines[0]["games"] + lines[0]["unfinished"] == 72
    assert lines[1]["games"] == lines[0]["games"] and lines[1]["games_per_s"] >= 0
    assert lines[0]["win1"] + lines[0]["win2"] + lines[0]["win3"] + lines[0]["loss1"] + lines[0]["loss2"] + \
        lines[0]["loss3"] == lines[0]["games"]
