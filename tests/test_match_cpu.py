"""Match play on the host (bgx/match.py, bgx/arena.py; no GPU): met_table's hand values and
shape, load_met, match_decision_reference against the money thresholds and the known scores,
summarize_match against numpy, arena_match_reference on a hand-made trace, the command-line flags,
the C ABI's declarations, the hand-set kernel state of tests/match_ref.py, and part 1 of
csrc/bg_match.h built as a host program (tools/match_host.cpp)."""
import ctypes
import json
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from bgx import _lib, arena as A, match as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")


def rule(**kw):
    return M.MatchRule(lambda eng, dsel: None, **kw)


# ---------------------------------------------------------------------- the table --
def test_met_table_hand_values():
    g, b = 0.26, 0.012
    met, pc = M.met_table(7, g, b)
    assert met.dtype == pc.dtype == np.float32 and met.shape == (8, 8) and pc.shape == (8,)
    assert met[1, 1] == F(0.5) and pc[1] == F(0.5) and pc[2] == F(0.5)
    assert met[1, 2] == F(0.5 + 0.25 * (1 - g - b))             # the Crawford leader against 2
    assert met[1, 3] == F(0.5 + 0.25 * (1 - b))                 # ... against 3
    assert met[2, 1] == F(1.0 - (0.5 + 0.25 * (1 - g - b)))
    m2, p2 = M.met_table(2, 0.0, 0.0)
    assert m2[2, 2] == F(0.5) and m2[1, 2] == F(0.75) and p2.tolist() == [1.0, 0.5, 0.5]
    m1, p1 = M.met_table(1)
    assert m1[1, 1] == F(0.5) and p1[1] == F(0.5)
    # the default rates
    assert np.array_equal(M.met_table(7)[0], met)
    assert "cubeless" in M.met_table.__doc__.lower()


@pytest.mark.parametrize("rates", [(0.26, 0.012), (0.0, 0.0)])
def test_met_table_symmetry_and_monotony(rates):
    """Monotony is a property of the table at the default rates and without gammons, not of the
    recurrence: after the Crawford game every game is played at 2 and before it at 1, so at extreme
    gammon rates (0.5 and 0.1) needing 6 against 1 comes out above needing 6 against 2."""
    for L in range(1, M.MAX_LENGTH + 1):
        met, pc = M.met_table(L, *rates)
        m = met[1:, 1:].astype(np.float64)
        assert np.abs(m + m.T - 1.0).max() <= 1e-6, L
        assert (m >= 0).all() and (m <= 1).all() and (pc >= 0).all() and (pc <= 1).all()
        assert (np.diff(m, axis=1) >= 0).all() and (np.diff(m, axis=0) <= 0).all(), L      # rises in j, falls in i
        assert (np.diff(pc[1:].astype(np.float64)) <= 0).all()
        M.check_met(L, met, pc)
    for bad in (0, 26, -1, 2.5, True):
        with pytest.raises(ValueError, match="length"):
            M.met_table(bad)
    with pytest.raises(ValueError, match="rates"):
        M.met_table(5, 0.9, 0.2)


def test_load_met_round_trip_and_refusals(tmp_path):
    met, pc = M.met_table(5)
    path = str(tmp_path / "met.json")
    M.save_met(path, 5, met, pc)
    L, met2, pc2 = M.load_met(path)
    assert L == 5 and met2.dtype == np.float32 and np.array_equal(met2[1:, 1:], met[1:, 1:])
    assert np.array_equal(pc2[1:], pc[1:])
    good = json.load(open(path))

    def refused(change, what):
        d = json.loads(json.dumps(good))
        change(d)
        p = str(tmp_path / "bad.json")
        json.dump(d, open(p, "w"))
        with pytest.raises(ValueError, match=what):
            M.load_met(p)

    refused(lambda d: d.pop("post_crawford"), "keys")
    refused(lambda d: d.update(length=4), "needs met")
    refused(lambda d: d.update(length=26), "length")
    refused(lambda d: d["met"].pop(), "needs met|rectangular")
    refused(lambda d: d["met"][2].__setitem__(3, 1.5), "probability")
    refused(lambda d: d["met"][2].__setitem__(3, -0.1), "probability")
    refused(lambda d: d["met"][2].__setitem__(3, d["met"][2][3] + 1e-4), "must be 1")
    refused(lambda d: d["post_crawford"].__setitem__(1, 0.4), "0.5")
    refused(lambda d: d["post_crawford"].__setitem__(3, 2.0), "probability")
    refused(lambda d: d["post_crawford"].append(0.1), "needs met")


# ------------------------------------------------------------------- the decisions --
class R:
    """A rule as match_decision_reference reads it."""

    def __init__(self, scale=1.0, window=0.65, win_gammons=0.0, loss_gammons=0.0):
        self.scale, self.window, self.win_gammons, self.loss_gammons = scale, window, win_gammons, loss_gammons


def linear_table(L=25, S=32):
    i = np.arange(L + 1)
    met = (0.5 + (i[None, :] - i[:, None]) / (2.0 * S)).astype(F)
    pc = np.full(L + 1, 0.5, F)
    return met, pc


def test_linear_table_gives_the_money_thresholds():
    """M(i, j) = 0.5 + (j - i) / 64 far from the end, no gammons: every number is a multiple of
    2^-12 below 1, so the fp32 arithmetic is exact and the decisions are the money dead-cube ones,
    offer iff 2p - 1 >= window (2 - 2p), pass iff p > 3/4."""
    met, pc = linear_table()
    M.check_met(25, met, pc)
    ps = [Fraction(n, 64) for n in range(0, 65)]
    vals = np.array([float(2 * p - 1) for p in ps], F)
    for k in (0, 1, 2):
        cube = k | (0 if k == 0 else 1 << 4)                    # centred, or owned by PLAYER1 = the mover
        for w in (Fraction(0), Fraction(1, 4), Fraction(1, 2), Fraction(3, 4), Fraction(1)):
            d = M.match_decision_reference(met, pc, 25, 20, 19, 0, cube, 0, 3, vals, R(window=float(w)))
            assert d["access"].all()
            assert np.array_equal(d["p"], np.array([float(p) for p in ps], F))
            assert d["offer"].tolist() == [2 * p - 1 >= w * (2 - 2 * p) for p in ps], (k, w)
            assert d["passes"].tolist() == [p > Fraction(3, 4) for p in ps], (k, w)
            assert np.array_equal(d["passed"], d["offer"] & d["passes"])
    # window 1 is the cash point, window 0 the dead-cube doubling point p = 1/2
    d = M.match_decision_reference(met, pc, 25, 20, 19, 0, 0, 0, 3, vals, R(window=0.0))
    assert d["offer"].tolist() == [p >= Fraction(1, 2) for p in ps]


def test_two_away_two_away():
    met, pc = M.met_table(2, 0.0, 0.0)
    ps = np.linspace(0, 1, 65)
    d = M.match_decision_reference(met, pc, 2, 2, 2, 0, 0, 1, 1, (2 * ps - 1).astype(F), R(window=0.0))
    assert d["access"].all() and d["offer"].tolist() == (ps >= 0.5).tolist()
    assert d["passes"].tolist() == (ps > 0.75).tolist()
    assert np.array_equal(d["dp"], np.full(65, 0.75, F)) and np.array_equal(d["dt"], ps.astype(F))


def test_post_crawford_and_crawford():
    met, pc = M.met_table(7, 0.0, 0.0)
    ps = np.linspace(0, 1, 65)
    v = (2 * ps - 1).astype(F)
    for w in (0.0, 0.65, 1.0):
        # the trailer needs 2: the free double at every p > 0, whatever the window
        d = M.match_decision_reference(met, pc, 7, 2, 1, 2, 0, 0, 2, v, R(window=w))
        # (at p = 0 nothing is gained, DT = ND = 0: only window 0, met with equality, doubles there)
        assert d["access"].all() and d["offer"].tolist() == ((ps > 0) | (w == 0.0)).tolist(), w
    # the trailer needs 3: 2 points are worth what 1 is, no double at 0.65 below p = 1
    d = M.match_decision_reference(met, pc, 7, 3, 1, 2, 0, 0, 2, v, R(window=0.65))
    assert d["access"].all() and d["offer"].tolist() == (ps >= 1).tolist()
    # the leader's cube is dead: x <= v
    d = M.match_decision_reference(met, pc, 7, 1, 3, 2, 0, 0, 2, v, R(window=0.0))
    assert not d["access"].any() and not d["offer"].any()
    # no offer in a Crawford game, at any score and value
    x, y = np.meshgrid(np.arange(1, 8), np.arange(1, 8))
    for val in (-1.0, 0.0, 0.5, 1.0):
        d = M.match_decision_reference(met, pc, 7, x, y, 1, 0, 0, 2, F(val), R(window=0.0))
        assert not d["access"].any() and not d["offer"].any()
    # no offer with x <= v: cube at 2 owned by the mover, every x <= 2; cube at 4, every x <= 4
    for k in (1, 2):
        d = M.match_decision_reference(met, pc, 7, x, y, 0, k | (1 << 4), 0, 2, F(0.5), R(window=0.0))
        assert np.array_equal(d["access"], x > (1 << k)) and not d["offer"][x <= (1 << k)].any()
    # first ply, a finished game, an idle lane, the other side's cube, the cap
    for kw in (dict(plies=0), dict(over=True), dict(active=False), dict(cube=1 | (2 << 4)), dict(cube=10), dict(cube=15)):
        a = dict(x=7, y=7, craw=0, cube=0, mover=0, plies=2)
        a.update(kw)
        d = M.match_decision_reference(met, pc, 7, value_offer=F(0.5), rule_offer=R(window=0.0), **a)
        assert not d["access"].any() and not d["offer"].any(), kw


def test_nan_never_offers_and_always_takes():
    met, pc = M.met_table(7)
    x, y = np.meshgrid(np.arange(1, 8), np.arange(1, 8))
    for craw in (0, 2):
        for r in (R(window=0.0), R(window=1.0, win_gammons=0.3, loss_gammons=0.2), R(scale=0.0)):
            d = M.match_decision_reference(met, pc, 7, x, y, craw, 0, 0, 2, F(NAN), r)
            if r.scale != 0.0:
                assert np.isnan(d["p"]).all()
                assert not d["offer"].any() and not d["passes"].any() and not d["passed"].any()
    # the infinities clamp to a sure win or loss
    d = M.match_decision_reference(met, pc, 7, 5, 5, 0, 0, 0, 2, np.array([INF, -INF], F), R(win_gammons=0.25, loss_gammons=0.25))
    assert d["p"].tolist() == [1.0, 0.0]


def test_scalar_rule_equals_the_array_reference():
    """tests/match_ref.py's scalar rule and match_decision_reference are written apart; on the
    hand-set kernel state they agree bit for bit."""
    import match_ref as ref
    for L in ref.LENGTHS:
        s = ref.make_state(L)
        t = (s["met"], s["pc"], L)
        for rl, key in ((ref.RULE_A, "eq_a"), (ref.RULE_B, "er_b")):
            d = M.match_decision_reference(s["met"], s["pc"], L, s["away"][:, 0], s["away"][:, 1], s["craw"], s["cube"],
                                           s["recs"][:, ref.R_CUR], s["plies"], s[key], R(*rl),
                                           over=s["recs"][:, ref.R_OVER] != 0)
            for i in range(ref.N):
                x, y, cr, k = ref.xyk(s, i, True)
                p = ref.match_p(rl[0], s[key][i], rl[2], rl[3])
                nd, dt, dp = ref.match_values(t, x, y, cr, k, p, rl[2], rl[3])
                got = np.array([d["p"][i], d["nd"][i], d["dt"][i], d["dp"][i]], F)
                assert np.array_equal(got.view(np.int32), np.array([p, nd, dt, dp], F).view(np.int32)), (L, i)
                acc = ref.lane_access(s, i, True, True)
                assert d["access"][i] == acc
                assert d["offer"][i] == (acc and ref.offers(t, x, y, cr, k, rl, s[key][i]))
                assert d["passes"][i] == ref.passes(t, x, y, cr, k, rl, s[key][i])


def test_kernel_state_reaches_every_branch():
    """The hand-set state of tests/test_gpu_match.py's kernel test, on the scalar rule alone: every
    branch and every counted field is reached, and the invariants hold."""
    import match_ref as ref
    assert ref.MATCH_FIELDS == M.MATCH_FIELDS and ref.CAP == M.MAX_CAP
    for L in ref.LENGTHS:
        out, seen = ref.run_reference(L)
        assert seen == ref.BRANCHES, (L, sorted(ref.BRANCHES - seen), sorted(seen - ref.BRANCHES))
        assert not seen & ref.UNREACHABLE
        mt = out["mt_flush"]
        assert all(mt != 0), mt
        s0, s1 = out["state0"], out["after_retire"]
        G = ref.games_quota(L)
        assert set(s0["craw"]) == {0, 1, 2} and set(s0["away"].ravel()) == set(range(1, L + 1))
        # a pass ends a game of its lane, never a match; lanes retired by a played-out last match
        assert mt[3] == mt[8] + mt[9] == int(out["mask"].sum())
        assert np.array_equal(out["after_respond"]["matches_done"], s0["matches_done"])
        retired = int(((s1["games_done"] >= G) & (s0["games_done"] < G)).sum())
        assert retired > 0 and out["tally"][13] == int((s0["games_done"] < G).sum()) - retired
        assert ((s1["away"] >= 1) & (s1["away"] <= L)).all() and (s1["craw"] <= 2).all() and not s1["retire"].any()
        assert M.summarize_match([mt[2] - mt[3]] + [0] * 15, mt, 1, 0)["matches"] == mt[0]
    assert ref.N > 256 and ref.N % 64 != 0


# ---------------------------------------------------------------------- the summary --
def match_tally(**kw):
    t = dict.fromkeys(M.MATCH_FIELDS, 0)
    t.update(kw)
    return [t[k] for k in M.MATCH_FIELDS]


def plain(games, wins_a=0):
    t = dict.fromkeys(A.FIELDS, 0)
    t.update(games=games, wins_a=wins_a, wins_b=games - wins_a, points_a=wins_a, points_b=games - wins_a)
    return [t[k] for k in A.FIELDS] + [0, 0]


def test_summarize_match_against_numpy():
    mt = match_tally(matches=10, match_wins_a=6, match_games=47, pass_games=7, match_points_a=40, match_points_b=31,
                     doubles_a=12, doubles_b=9, passes_a=3, passes_b=4, cube_log2=20, crawford_games=5,
                     post_crawford_games=8, pass_plies=70, match_wins_a_seat0=4, matches_seat0=5)
    r = M.summarize_match(plain(40, 22), mt, steps=900, unfinished=2)
    w = np.array([1] * 6 + [0] * 4, np.float64)
    assert r["matches"] == 10 and r["match_wins_a"] == 6 and r["match_win_rate_a"] == w.mean()
    assert r["match_win_rate_stderr"] == pytest.approx(w.std() / math.sqrt(10), rel=1e-12)
    assert r["games"] == 47 and r["games_per_match"] == 4.7
    assert (r["doubles_per_game_a"], r["doubles_per_game_b"]) == (12 / 47, 9 / 47)
    assert (r["take_share_a"], r["take_share_b"]) == (1 - 3 / 9, 1 - 4 / 12)
    assert r["pass_share"] == 7 / 47 and r["mean_cube_log2"] == 20 / 47
    assert (r["crawford_share"], r["post_crawford_share"]) == (5 / 47, 8 / 47)
    assert r["match_win_rate_a_first_seat"] == 0.8
    assert r["played_out"] == A.summarize(plain(40, 22), 900, 2) and r["unfinished_lanes"] == 2 and r["steps"] == 900
    assert all(r[k] == v for k, v in zip(M.MATCH_FIELDS, mt))
    json.dumps(r)
    # no matches, one match
    r0 = M.summarize_match([0] * 16, [0] * 16, 0, 3)
    assert r0["matches"] == 0 and r0["match_win_rate_a"] == 0.0 and r0["match_win_rate_stderr"] is None
    assert r0["games_per_match"] == 0.0 and r0["take_share_a"] == 0.0 and r0["match_win_rate_a_first_seat"] == 0.0
    r1 = M.summarize_match(plain(3, 2), match_tally(matches=1, match_wins_a=1, match_games=3, match_points_a=2,
                                                    match_points_b=1), 50, 0)
    assert r1["match_win_rate_a"] == 1.0 and r1["match_win_rate_stderr"] is None and r1["games_per_match"] == 3.0
    r2 = M.summarize_match(plain(6, 3), match_tally(matches=2, match_wins_a=1, match_games=6), 50, 0)
    assert r2["match_win_rate_stderr"] == pytest.approx(math.sqrt(0.25 / 2))


def test_summarize_match_broken_invariants():
    with pytest.raises(ValueError, match="wins"):
        M.summarize_match(plain(5), match_tally(matches=2, match_wins_a=3, match_games=5), 1, 0)
    with pytest.raises(ValueError, match="wins"):
        M.summarize_match(plain(5), match_tally(matches=2, match_wins_a=1, match_games=5, match_wins_a_seat0=2,
                                                matches_seat0=2), 1, 0)
    with pytest.raises(ValueError, match="doubles"):
        M.summarize_match(plain(4), match_tally(matches=1, match_games=5, pass_games=1, passes_a=1), 1, 0)
    with pytest.raises(ValueError, match="doubles"):
        M.summarize_match(plain(4), match_tally(matches=1, match_games=5, pass_games=1, passes_b=1, doubles_b=3), 1, 0)
    with pytest.raises(ValueError, match="passed games"):
        M.summarize_match(plain(4), match_tally(matches=1, match_games=5, pass_games=1, doubles_a=3), 1, 0)
    with pytest.raises(ValueError, match="plain tally"):
        M.summarize_match(plain(3), match_tally(matches=1, match_games=5), 1, 0)
    with pytest.raises(ValueError, match="entries"):
        M.summarize_match(plain(3), [0] * 9, 1, 0)


# ------------------------------------------------------------- the rule and the pair --
def test_match_rule_and_arena_match():
    from bgx.cube import CubeRule
    r = rule()
    assert isinstance(r, CubeRule) and M.MatchRule.equity is CubeRule.equity         # reused, not copied
    assert (r.scale, r.window, r.win_gammons, r.loss_gammons, r.lookahead, r.sync_free) == (1.0, 0.65, 0.25, 0.25, 1, False)
    s = rule(scale=2.0, window=0.0, win_gammons=1.0, loss_gammons=0.5, lookahead=0).struct()
    assert isinstance(s, _lib.BgxMatchRule) and (s.scale, s.window, s.win_gammons, s.loss_gammons) == (2.0, 0.0, 1.0, 0.5)
    for kw in (dict(window=-0.1), dict(window=1.1), dict(window=NAN), dict(win_gammons=1.5), dict(loss_gammons=-1),
               dict(loss_gammons=NAN)):
        with pytest.raises(ValueError, match="MatchRule"):
            rule(**kw)
    with pytest.raises(ValueError, match="scale is NaN"):
        rule(scale=NAN)
    with pytest.raises(ValueError, match="lookahead"):
        rule(lookahead=2)
    m = M.ArenaMatch(5)
    assert m.length == 5 and not m.has_a and not m.has_b and m.sync_free
    assert np.array_equal(m.met, M.met_table(5)[0]) and m.games_quota(3) == 27
    one = M.ArenaMatch(7, None, rule(), met=M.met_table(7, 0.2, 0.0))
    assert one.has_b and not one.has_a and one.sync_free is False and one.met[1, 2] == F(0.5 + 0.25 * 0.8)
    for bad in (0, 26, 2.5):
        with pytest.raises(ValueError, match="length"):
            M.ArenaMatch(bad)
    with pytest.raises(ValueError, match="MatchRule or None"):
        M.ArenaMatch(5, CubeRule(lambda eng, dsel: None))
    with pytest.raises(ValueError, match="needs met"):
        M.ArenaMatch(5, met=M.met_table(7))
    with pytest.raises(ValueError, match="int32"):
        M.ArenaMatch(25).games_quota(2 ** 26)
    assert "MATCHES per lane" in " ".join(A.Arena.play.__doc__.split())


# --------------------------------------------------------------- the traced replay --
def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def test_arena_match_reference_on_a_hand_made_trace():
    """Matches to 3, one per lane, on met_table(3, 0, 0): M[2][3] = 0.625, M[1][3] = M[1][2] = 0.75.
    Lane 0 (A is PLAYER1 in game 0): A doubles at 3-3 with p = 0.75 (ND 0.5625, DT 0.625 = DP) and B,
    seeing p = 0.95, passes: 2-3.  B wins a gammon: 2-1, the Crawford game; A wins it: 1-1, post
    Crawford; A wins the match and the lane retires.  Lane 1: A doubles, B (p = 0.5, DT 0.5 <= DP)
    takes, A wins a gammon at cube 2: 4 points, past the 3 it needed.  Lane 2 never finishes a game.
    Lane 3: B wins a backgammon."""
    T, B = 7, 4
    tr = dict(cube_mover=np.zeros((T, B), np.uint8), eq_offer=np.full((T, B), NAN, F), eq_resp=np.full((T, B), NAN, F),
              done=np.zeros((T, B), np.uint8), info=np.zeros((T, B), np.int32))
    # lane 0
    tr["eq_offer"][1, 0], tr["eq_resp"][1, 0] = 0.5, 0.9
    tr["done"][2, 0], tr["info"][2, 0] = 1, info(0, 2)             # game 1: A is PLAYER2, PLAYER1 = B wins a gammon
    tr["eq_offer"][4, 0] = 0.9                                      # the Crawford game: no access
    tr["done"][4, 0], tr["info"][4, 0] = 1, info(0, 1)             # game 2: A is PLAYER1
    tr["cube_mover"][6, 0], tr["eq_offer"][6, 0] = 1, 0.9           # post Crawford 1-1: the cube is dead
    tr["done"][6, 0], tr["info"][6, 0] = 1, info(1, 1)             # game 3: A is PLAYER2
    # lane 1: A is PLAYER2 in game 0
    tr["cube_mover"][1, 1], tr["eq_offer"][1, 1], tr["eq_resp"][1, 1] = 1, 0.5, 0.0
    tr["done"][2, 1], tr["info"][2, 1] = 1, info(1, 2)
    # lane 3: A is PLAYER2
    tr["done"][1, 3], tr["info"][1, 3] = 1, info(0, 3)
    no_g = dict(win_gammons=0.0, loss_gammons=0.0)
    match = M.ArenaMatch(3, rule(window=0.0, **no_g), rule(window=1.0, **no_g), met=M.met_table(3, 0.0, 0.0))
    out = M.arena_match_reference(tr, B, 1, match)
    G = 5
    assert out["games_done"].tolist() == [G, G, 0, G] and out["matches_done"].tolist() == [1, 1, 0, 1]
    want = dict(matches=3, match_wins_a=2, match_games=6, pass_games=1, match_points_a=7, match_points_b=5, doubles_a=2,
                doubles_b=0, passes_a=0, passes_b=1, cube_log2=1, crawford_games=1, post_crawford_games=1, pass_plies=1,
                match_wins_a_seat0=1, matches_seat0=1)
    assert dict(zip(M.MATCH_FIELDS, out["match_tally"].tolist())) == want
    t = dict(zip(A.FIELDS, out["tally"].tolist()))
    assert (t["games"], t["wins_a"], t["wins_b"], t["points_a"], t["points_b"], t["gammons_a"], t["gammons_b"],
            t["backgammons_b"], t["active_lanes"]) == (5, 3, 2, 4, 5, 1, 1, 1, 1)
    # at t = 2 B is on roll in the game after the pass and may double; its value there is NaN
    assert out["dsel"][:, 0].tolist() == [0, 1, 2, 0, 0, 0, 0] and out["offer"][:, 0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert out["passed"][:, 0].tolist() == [False, True] + [False] * 5
    # at t = 2 B, PLAYER1, holds the cube at 2 and needs 3: it may redouble
    assert out["dsel"][:, 1].tolist() == [0, 1, 2, 0, 0, 0, 0] and not out["passed"][:, 1].any()
    assert out["away"][:, 0].tolist() == [[3, 3], [3, 3], [2, 3], [2, 1], [2, 1], [1, 1], [1, 1]]
    assert out["craw"][:, 0].tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert out["cube"][:, 1].tolist() == [0, 0, 1 | (1 << 4), 0, 0, 0, 0]      # taken: 2, owned by PLAYER1 = B
    assert out["away"][:, 1].tolist() == [[3, 3]] * 7 and out["away"][:, 3].tolist() == [[3, 3]] * 7
    # lane 2 may double from its second ply on but holds NaN; lane 3 had access once, then retired
    assert out["dsel"][:, 2].tolist() == [0, 1, 1, 1, 1, 1, 1] and out["dsel"][:, 3].tolist() == [0, 2, 0, 0, 0, 0, 0]
    assert not out["offer"][:, 2:].any()
    r = M.summarize_match(out["tally"], out["match_tally"], T, 1)
    assert r["match_win_rate_a"] == 2 / 3 and r["games_per_match"] == 2.0 and r["unfinished_lanes"] == 1
    # two matches per lane: nobody retires, the second match starts at 3-3 with the other seat first
    out2 = M.arena_match_reference(tr, B, 2, match)
    assert out2["games_done"].tolist() == [4, 1, 0, 1] and out2["tally"][A.ACTIVE] == 4
    assert out2["match_tally"].tolist() == out["match_tally"].tolist()
    # without rules (their value is NaN) nobody doubles: lane 1's gammon is 2 points and its match goes on
    nan = np.full((T, B), NAN, F)
    out3 = M.arena_match_reference(dict(tr, eq_offer=nan, eq_resp=nan), B, 1, M.ArenaMatch(3))
    assert not out3["offer"].any() and out3["matches_done"].tolist() == [0, 0, 0, 1]
    assert out3["match_tally"][M.MATCH_FIELDS.index("cube_log2")] == 0


# ------------------------------------------------------------------------ the parser --
def test_parser_flags():
    ap = A.build_parser()
    base = "--a a.pt --b b.pt --max-steps 10 "
    ns = ap.parse_args(base.split())
    assert ns.match is None and ns.met is None
    ns = ap.parse_args((base + "--match 7").split())
    for side in "ab":
        assert [getattr(ns, f"{k}_{side}") for k in A.MATCH_SIDE_DEFAULTS] == [0.65, (0.25, 0.25), 1, None, 1.0]
    ns = ap.parse_args((base + "--match 5 --met t.json --match-window-a 0.5 --match-gammons-a 0.3,0.1 --match-lookahead-a 0 "
                        "--match-net-a v.pt --match-scale-a 2 --match-window-b 1 --match-lookahead-b 1").split())
    assert (ns.match, ns.met, ns.match_window_a, ns.match_gammons_a, ns.match_lookahead_a, ns.match_net_a,
            ns.match_scale_a) == (5, "t.json", 0.5, (0.3, 0.1), 0, "v.pt", 2.0)
    assert (ns.match_window_b, ns.match_gammons_b, ns.match_lookahead_b) == (1.0, (0.25, 0.25), 1)
    assert ap.parse_args("--a a.pt --b random --max-steps 10 --match 3 --match-window-a 0.3".split()).match_window_a == 0.3
    assert ap.parse_args("--a random --b random --max-steps 10 --match 1".split()).match == 1
    for bad in ("--match 7 --cube", "--match 7 --luck", "--match 0", "--match 26", "--match-window-a 0.5", "--met t.json",
                "--match-lookahead-b 0", "--match 7 --match-window-a 1.5", "--match 7 --match-window-b nan",
                "--match 7 --match-gammons-a 0.5", "--match 7 --match-gammons-a 0.5,1.5", "--match 7 --match-gammons-b x,y",
                "--match 7 --match-lookahead-a 2", "--match 7 --match-scale-a nan"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + bad).split())
    for bad in ("--a a.pt --b random --max-steps 10 --match 7 --match-window-b 0.3",
                "--a random --b b.pt --max-steps 10 --match 7 --match-net-a v.pt"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


# ------------------------------------------------------------------------- the C ABI --
ENTRIES = (("bgx_arena_match_begin", 11), ("bgx_arena_match_sel", 11), ("bgx_arena_match_offer", 21),
           ("bgx_arena_match_respond", 26), ("bgx_arena_match_flush", 17), ("bgx_arena_match_retire", 8))


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in ENTRIES:
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):                    # pointer / int32 / the rule by value, in the header's order
            want = _lib._P if "*" in p else _lib.BgxMatchRule if p.startswith("bgx_match_rule") else _lib._I32
            assert a is want, (name, p)
    fields = re.search(r"enum bgx_arena_match_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ARENA_MATCH_(\w+)\s*=\s*(\d+)", fields)
    rename = {"wins_a": "match_wins_a", "games": "match_games", "points_a": "match_points_a", "points_b": "match_points_b",
              "log2": "cube_log2", "wins_a_seat0": "match_wins_a_seat0"}
    assert [(rename.get(n.lower(), n.lower()), int(v)) for n, v in names] == [(f, i) for i, f in enumerate(M.MATCH_FIELDS)]
    assert re.search(r"typedef struct \{\s*float scale, window, win_gammons, loss_gammons;\s*\} bgx_match_rule;", header)
    assert [f for f, _ in _lib.BgxMatchRule._fields_] == ["scale", "window", "win_gammons", "loss_gammons"]
    # the device code is part 2 of csrc/bg_match.h, compiled with bg_returns.hip after bg_arena_cube.h, and only there
    csrc = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc")
    src = open(os.path.join(csrc, "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_arena_cube.h"') < src.index('#include "bg_match.h"')
    for f in os.listdir(csrc):
        if f not in ("bg_returns.hip", "bg_match.h"):
            assert "bg_match.h" not in open(os.path.join(csrc, f)).read(), f
    part1 = open(os.path.join(csrc, "bg_match.h")).read().split("#ifndef BGX_MATCH_PART1_ONLY")[0]
    code = re.sub(r"//[^\n]*", "", part1)
    assert "fminf" not in code and "fmaxf" not in code and "ct_mul" in code       # the clamp keeps a NaN
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name, _ in ENTRIES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def test_rule_host_program(tmp_path):
    """tools/match_host.cpp with AddressSanitizer + UBSan, a program of its own: every score of L =
    1..7, every Crawford state, cube byte and mover on both tables; the tables are heap blocks of
    their exact size, so a lookup outside them stops the program."""
    exe = str(tmp_path / "match_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "match_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, \
        out.stderr[-2000:]
    m = re.fullmatch(r"cases (\d+) access (\d+) offers (\d+) takes (\d+) passes (\d+) ends (\d+) matches (\d+)\n", out.stdout)
    assert m, out.stdout
    cases, access, offers, takes, passes, ends, matches = (int(v) for v in m.groups())
    states = sum(L * L for L in range(1, 8)) * 2 * 3 * 256 * 2
    assert cases == states * 3 * 3 * 12 and ends == states * 6 and 0 < matches < ends
    assert 0 < access < states and offers == takes + passes and min(takes, passes) > 0
