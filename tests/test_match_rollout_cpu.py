"""Match-score rollouts on the host (bgx/match.py, bgx/rollout.py; no GPU):
outcome_mwc by hand, summarize_match_rollout against numpy and its invariants, validate_score,
rollout_match_reference on a hand-made trace, the refused mode pairs, the command-line flags, the C
ABI's declarations, and part 1 of csrc/bg_match_rollout.h built as a host program
(tools/match_rollout_host.cpp)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bgx import _lib, match as M, rollout as R
from bgx.cube import pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN = float("nan")


def rule(**kw):
    return M.MatchRule(lambda eng, dsel: None, **kw)


def bin_of(won, kind, k):
    return won * 44 + kind * 11 + k


# -------------------------------------------------------------------- outcome_mwc --
def test_outcome_mwc_by_hand():
    met, pc = M.met_table(7)
    m64, p64 = met.astype(np.float64), pc.astype(np.float64)
    # 1-away / 1-away: whoever wins the game wins the match, at any cube and Crawford state
    for craw in (0, 1, 2):
        for s in (0, 1):
            o = M.outcome_mwc(met, pc, 7, (1, 1), craw, s)
            assert o.dtype == np.float64 and o.shape == (88,)
            assert (o[44:] == 1.0).all() and (o[:44] == 0.0).all()
    # a gammon at cube 2 from 3-away is 4 points: the match, whoever was ahead
    o = M.outcome_mwc(met, pc, 7, (3, 5), 0, 0)
    assert o[bin_of(1, 2, 1)] == 1.0
    assert o[bin_of(1, 1, 1)] == m64[1, 5]                       # a plain win at 2: 1-away, the Crawford row
    assert o[bin_of(1, 1, 0)] == m64[2, 5]
    assert o[bin_of(0, 1, 0)] == 1.0 - m64[4, 3]                 # the other side wins 1: it then needs 4
    assert o[bin_of(0, 3, 2)] == 0.0                             # 12 points to the other side
    # the start mover is PLAYER2: the same position seen from the other side
    o2 = M.outcome_mwc(met, pc, 7, (5, 3), 0, 1)
    assert np.array_equal(o, o2)
    # a pass at k = 1 from 5-away / 3-away: the doubler wins 2 points, the table's entry at 3 / 3
    o = M.outcome_mwc(met, pc, 7, (5, 3), 0, 0)
    assert o[bin_of(1, 0, 1)] == m64[3, 3] == 0.5
    assert o[bin_of(0, 0, 1)] == 1.0 - m64[1, 5]                 # it passed itself: the other side is 1-away
    assert o[bin_of(1, 0, 0)] == o[bin_of(1, 1, 0)]              # a pass and a plain win at the same cube
    # the Crawford transition reads row 1: 2-away / 4-away, a win of 1 point
    o = M.outcome_mwc(met, pc, 7, (2, 4), 0, 0)
    assert o[bin_of(1, 1, 0)] == m64[1, 4] and o[bin_of(0, 1, 0)] == 1.0 - m64[3, 2]
    # in the Crawford game (1-away / 4-away) the next game is post-Crawford: pc
    o = M.outcome_mwc(met, pc, 7, (1, 4), 1, 0)
    assert (o[44:] == 1.0).all()
    assert o[bin_of(0, 1, 0)] == 1.0 - p64[3] and o[bin_of(0, 2, 0)] == 1.0 - p64[2]
    assert o[bin_of(0, 3, 0)] == 1.0 - p64[1] == 0.5
    # ... and after it, from the trailer's side: it needs 4, wins 2 at the doubled cube
    o = M.outcome_mwc(met, pc, 7, (1, 4), 2, 1)
    assert o[bin_of(1, 1, 1)] == p64[2] and o[bin_of(1, 2, 1)] == 1.0 and (o[:44] == 0.0).all()
    assert M.met_after64(met, pc, 7, 1, 3, 2) == 1.0 - p64[3]
    # total: a score past the table reads its last row
    assert M.met_after64(met, pc, 7, 30, 2, 0) == m64[7, 2]


# -------------------------------------------------------- summarize_match_rollout --
def _random_rows(seed=0, start_k=1):
    rng = np.random.RandomState(seed)
    bins = rng.randint(0, 40, 88).astype(np.int64)
    bins[rng.rand(88) < 0.5] = 0
    by = bins.reshape(2, 4, 11).sum(axis=2)
    passes = int(by[:, 0].sum())
    hist = np.zeros(96, np.int64)
    hist[:88] = bins
    k = np.tile(np.arange(11), 8)
    hist[88:94] = (bins.sum(), passes, 17, 5, 3 * passes, int((bins * k).sum()))
    played = int(bins.sum()) - passes
    tally = np.asarray([played, 9 * played, *by[1, 1:], *by[0, 1:]], np.int64)
    return tally, hist, bins


def test_summarize_match_rollout_against_numpy():
    met, pc = M.met_table(7)
    mwc88 = M.outcome_mwc(met, pc, 7, (5, 6), 0, 0)
    tally, hist, bins = _random_rows()
    r = M.summarize_match_rollout(tally.tolist(), hist.tolist(), mwc88, 3, cube_k=1)
    sample = np.repeat(mwc88, bins)                              # one entry per game
    n = sample.size
    assert r["games"] == n == int(hist[88]) and r["unfinished"] == 3
    assert r["mwc"] == pytest.approx(sample.mean(), rel=1e-13)
    assert r["mwc_stderr"] == pytest.approx(math.sqrt(sample.var(ddof=1) / n), rel=1e-10)
    W, L = mwc88[bin_of(1, 1, 1)], mwc88[bin_of(0, 1, 1)]
    assert r["mwc_normalized"] == pytest.approx((2 * sample.mean() - (W + L)) / (W - L), rel=1e-12)
    assert r["pass_share"] == pytest.approx(hist[89] / n) and r["doubles_per_game_start"] == pytest.approx(17 / n)
    assert r["doubles_per_game_other"] == pytest.approx(5 / n) and r["mean_cube_log2"] == pytest.approx(hist[93] / n)
    assert r["match_hist"] == hist.tolist() and len(r["match_hist"]) == 96
    assert [r[f] for f in M.MATCH_HIST_FIELDS] == hist[88:94].tolist()
    assert r["played_out"]["games"] == int(tally[0]) and r["played_out"]["win2"] == int(tally[3])
    # every game the same outcome: no spread; W == L: no normalisation
    h1 = np.zeros(96, np.int64)
    h1[bin_of(1, 1, 0)] = h1[88] = 5
    r1 = M.summarize_match_rollout([5, 50, 5, 0, 0, 0, 0, 0], h1.tolist(), M.outcome_mwc(met, pc, 7, (1, 1), 0, 0))
    assert r1["mwc"] == 1.0 and r1["mwc_stderr"] == 0.0 and r1["mwc_normalized"] == 1.0
    r1 = M.summarize_match_rollout([5, 50, 5, 0, 0, 0, 0, 0], h1.tolist(), np.full(88, 0.5))
    assert r1["mwc"] == 0.5 and r1["mwc_normalized"] is None
    # below 2 games there is no standard error; without games the rates are 0
    h1[bin_of(1, 1, 0)] = h1[88] = 1
    assert M.summarize_match_rollout([1, 9, 1, 0, 0, 0, 0, 0], h1.tolist(), mwc88)["mwc_stderr"] is None
    r0 = M.summarize_match_rollout([0] * 8, [0] * 96, mwc88)
    assert r0["games"] == 0 and r0["mwc"] == 0.0 and r0["mwc_stderr"] is None and r0["pass_share"] == 0.0


def test_summarize_match_rollout_invariants():
    met, pc = M.met_table(7)
    mwc88 = M.outcome_mwc(met, pc, 7, (5, 6), 0, 0)
    tally, hist, bins = _random_rows(1)
    M.summarize_match_rollout(tally.tolist(), hist.tolist(), mwc88)
    i = int(np.nonzero(bins[11:22])[0][0]) + 11                  # a played-out loss of 1 point

    def broken(**kw):
        t, h = tally.copy(), hist.copy()
        for key, v in kw.items():
            (t if key[0] == "t" else h)[int(key[1:])] += v
        with pytest.raises(ValueError):
            M.summarize_match_rollout(t.tolist(), h.tolist(), mwc88)

    broken(h88=1)                                                # GAMES != the sum of the bins
    broken(**{f"h{i}": 1})                                       # a bin more than GAMES
    broken(**{f"h{i}": 1, "h88": 1})                             # GAMES != the plain games + PASS_GAMES
    broken(**{f"h{i}": 1, "h88": 1, "t0": 1})                    # the loss1 count disagrees
    broken(**{f"h{i}": 1, f"h{i + 11}": -1}) if bins[i + 11] else None      # a loss moved from 2 points to 1
    broken(h89=1, t0=-1)                                         # PASS_GAMES != the pass bins
    t, h = tally.copy(), hist.copy()
    z = int(np.nonzero(bins == 0)[0][0])
    h[z] -= 1
    h[i] += 1
    with pytest.raises(ValueError, match="negative"):
        M.summarize_match_rollout(t.tolist(), h.tolist(), mwc88)
    with pytest.raises(ValueError):
        M.summarize_match_rollout(tally.tolist(), hist.tolist()[:95], mwc88)
    with pytest.raises(ValueError):
        M.summarize_match_rollout(tally.tolist(), hist.tolist(), mwc88[:87])


# ------------------------------------------------------------------ validate_score --
def test_validate_score():
    assert M.validate_score(7, (3, 5)) == ((3, 5), 0)
    assert M.validate_score(7, np.asarray([7, 7], np.uint8), 0) == ((7, 7), 0)
    assert M.validate_score(7, (1, 5), 1) == ((1, 5), 1) and M.validate_score(7, [4, 1], 2) == ((4, 1), 2)
    for c in (0, 1, 2):
        assert M.validate_score(5, (1, 1), c) == ((1, 1), c)
    for away, craw in (((0, 3), 0), ((3, 8), 0), ((3,), 0), ((3, 4, 5), 0), ((2.5, 3), 0), ("ab", 0), (None, 0),
                       ((3, 5), 3), ((3, 5), -1), ((3, 5), True),
                       ((3, 5), 1), ((2, 2), 2),                 # a Crawford state with no side at 1
                       ((1, 5), 0), ((6, 1), 0)):                # a side at 1 before the Crawford game
        with pytest.raises(ValueError):
            M.validate_score(7, away, craw)
    with pytest.raises(ValueError):
        M.validate_score(26, (3, 5))
    with pytest.raises(ValueError):
        M.RolloutMatch(7, rule=object())
    with pytest.raises(ValueError):
        M.RolloutMatch(0, None)
    with pytest.raises(ValueError):
        M.RolloutMatch(5, None, met=M.met_table(7))
    m = M.RolloutMatch(5, None)
    assert not m.has_rule and m.sync_free and m.met.shape == (6, 6) and math.isnan(m.rule.struct().scale) is False
    assert M.RolloutMatch(5, rule(lookahead=0)).has_rule


# ------------------------------------------------- the replay on a hand-made trace --
def _pick(match, x, y, craw, cube, mover, want):
    """a value on which the rule's decision at that state is `want` (0 none, 1 take, 2 pass)"""
    for v in np.linspace(-1.0, 1.0, 81):
        d = M.match_decision_reference(match.met, match.pc, match.length, x, y, craw, cube, mover, 1, F(v), match.rule)
        assert bool(d["access"])
        act = 2 if d["passed"] else 1 if d["offer"] else 0
        if act == want:
            return float(v)
    raise AssertionError("no value gives that decision")


def test_rollout_match_reference_on_a_hand_made_trace():
    match = M.RolloutMatch(7, rule())
    away, craw = np.asarray([[5, 3], [2, 1]]), np.asarray([0, 1])
    T, B, G = 6, 6, 2
    group = np.asarray([0, 0, 0, 1, -1, 1])
    starts = np.zeros((B, 64), np.uint8)
    starts[:, 52] = [0, 1, 0, 0, 0, 1]                           # the start movers
    cube0 = np.asarray([0, pack(1, 2), pack(2, 2), 0, 0, 0], np.uint8)
    mover = np.zeros((T, B), np.uint8)
    mover[:] = (starts[:, 52][None] + np.arange(T)[:, None]) & 1  # the sides alternate
    value = np.full((T, B), 0.9, F)                              # a value that doubles wherever there is access
    done, info = np.zeros((T, B), np.uint8), np.zeros((T, B), np.int32)

    def ends(t, lane, winner, score):
        done[t, lane] = 1
        info[t, lane] = ((winner + 1) << 8) | (score << 16)

    # lane 0: PLAYER2 (3-away) doubles and is taken, PLAYER1 (5-away) redoubles at 2 and is passed;
    # the lane's second game is played out and lost; then the lane is retired
    v_take = _pick(match, 3, 5, 0, 0, 1, 1)
    v_pass = _pick(match, 5, 3, 0, pack(1, 1), 0, 2)
    v_none = _pick(match, 3, 5, 0, 0, 1, 0)
    value[:, 0] = [0.9, v_take, v_pass, v_none, _pick(match, 5, 3, 0, 0, 0, 0), 0.9]
    ends(4, 0, 1, 1)
    ends(5, 0, 0, 3)                                             # after its last game: not counted
    # lane 1: the start mover PLAYER2 owns the cube at 2 and wins a gammon: 4 points from 3-away;
    # its next game: a NaN with access decides nothing; a backgammon lost at 2
    value[4, 1] = NAN
    ends(1, 1, 1, 2)
    ends(5, 1, 0, 3)
    # lane 2: the cube at 4 is PLAYER2's, who needs 3: dead.  Lane 3, 5: the Crawford game.  Lane 4: idle.
    ends(3, 3, 0, 1)
    ends(2, 4, 0, 1)
    ends(4, 5, 0, 2)
    trace = dict(match_mover=mover, match_value=value, done=done, info=info)
    r = M.rollout_match_reference(trace, starts, group, 2, G, match, away, craw, cube0)

    action = np.zeros((T, B), np.uint8)
    action[1, 0], action[2, 0] = 1, 2
    assert np.array_equal(r["action"], action) and np.array_equal(r["mask"], action == 2)
    dsel = np.zeros((T, B), bool)
    dsel[1:5, 0] = True                                          # not on a first ply, not once retired
    dsel[4, 1] = True                                            # PLAYER2's own cube, past the first ply
    assert np.array_equal(r["dsel"], dsel)
    cube = np.tile(cube0, (T, 1))
    cube[2, 0] = pack(1, 1)                                      # the take: 2, owned by PLAYER1
    assert np.array_equal(r["cube"], cube)
    hist = np.zeros((2, 96), np.int64)
    for g, b in ((0, bin_of(1, 0, 1)), (0, bin_of(0, 1, 0)), (0, bin_of(1, 2, 1)), (0, bin_of(0, 3, 1)),
                 (1, bin_of(1, 1, 0)), (1, bin_of(0, 2, 0))):
        hist[g, b] += 1
    hist[0, 88:94] = (4, 1, 1, 1, 2, 3)                          # games, passes, doubles by / against, pass plies, log2
    hist[1, 88] = 2
    assert np.array_equal(r["match_hist"], hist)
    assert r["tally"].tolist() == [[3, 9, 0, 1, 0, 1, 0, 1], [2, 9, 1, 0, 0, 0, 1, 0]]
    assert r["games_done"].tolist() == [2, 2, 0, 1, 0, 1] and r["active"] == 3
    # the summary accepts what the replay counted; the overshoot is a won match
    mwc88 = M.outcome_mwc(match.met, match.pc, 7, away[0], 0, 0)
    s = M.summarize_match_rollout(r["tally"][0], r["match_hist"][0], mwc88, 2)
    assert s["games"] == 4 and s["pass_games"] == 1 and s["played_out"]["games"] == 3
    # lane 1's start mover is PLAYER2: its bins belong to another start mover, so only the counts are read here
    assert M.outcome_mwc(match.met, match.pc, 7, away[0], 0, 1)[bin_of(1, 2, 1)] == 1.0
    # no rule (its value is NaN everywhere): nobody doubles, the games are all played out at the starting cubes
    r0 = M.rollout_match_reference(dict(trace, match_value=np.full((T, B), NAN, F)), starts, group, 2, G,
                                   M.RolloutMatch(7, None), away, craw, cube0)
    assert not r0["action"].any() and r0["match_hist"][:, 89:93].sum() == 0
    assert np.array_equal(r0["cube"], np.tile(cube0, (T, 1)))


# ---------------------------------------------------------------- the refused modes --
def test_check_modes_refuses_match_with_every_other_mode():
    m = M.RolloutMatch(7, None)
    x = object()
    for name in ("luck", "bearoff", "cube", "truncate", "cube_bearoff", "cube_truncate", "cube_luck"):
        for where in ("run", "run_lanes"):
            with pytest.raises(ValueError, match=f"{where}: match together with {name}"):
                R._check_modes(where, match=m, **{name: x})
    R._check_modes("run", match=m)
    R._check_modes("run_lanes", match=m, cube0=x, types=True)    # cube0 goes with match
    with pytest.raises(ValueError, match="cube0 without cube"):
        R._check_modes("run_lanes", cube0=x, types=True)
    with pytest.raises(ValueError, match="match must be a match.RolloutMatch"):
        R._check_modes("run_lanes", match=x, types=True)
    R._check_modes("run")                                        # all None: nothing to refuse


# ---------------------------------------------------------------- the command line --
def test_parser_flags():
    ap = R.build_parser()
    base = "--net ckpt.pt --positions opening "
    ns = ap.parse_args(base.split())
    assert ns.match is None and ns.match_score is None and not ns.match_decision
    ns = ap.parse_args((base + "--match 7 --match-score 3,5").split())
    assert (ns.match, ns.match_score, ns.match_crawford, ns.met, ns.match_cube) == (7, (3, 5), 0, None, (0, 0))
    assert (ns.match_window, ns.match_gammons, ns.match_lookahead, ns.match_net, ns.match_scale) == \
        (0.65, (0.25, 0.25), 1, None, 1.0)
    ns = ap.parse_args((base + "--match 5 --match-score 1,4 --match-crawford 2 --met t.json --match-window 0.5 "
                        "--match-gammons 0.3,0.1 --match-lookahead 0 --match-net v.pt --match-scale 2 --match-cube 1,2 "
                        "--match-decision").split())
    assert (ns.match, ns.match_score, ns.match_crawford, ns.met, ns.match_window, ns.match_gammons, ns.match_lookahead,
            ns.match_net, ns.match_scale, ns.match_cube, ns.match_decision) == \
        (5, (1, 4), 2, "t.json", 0.5, (0.3, 0.1), 0, "v.pt", 2.0, (1, 2), True)
    assert ap.parse_args("--net random --positions opening --match 3 --match-score 3,3".split()).match == 3
    assert ap.parse_args("--net random --positions opening --match 3 --match-score 3,3 --match-net v.pt --match-window 0.2"
                         .split()).match_window == 0.2
    for bad in ("--match 7", "--match-score 3,5", "--match 0 --match-score 1,1", "--match 26 --match-score 3,5",
                "--match 7 --match-score 3,5 --cube", "--match 7 --match-score 3,5 --luck",
                "--match 7 --match-score 3,5 --bearoff 6", "--match 7 --match-score 3,5 --bearoff1 10",
                "--match 7 --match-score 3,5 --truncate 8", "--match 7 --match-score 3,5 --cube --cube-bearoff 6",
                "--match 7 --match-score 3,5 --cube --cube-truncate 8", "--match 7 --match-score 3,5 --cube --cube-luck",
                "--match 7 --match-score 3", "--match 7 --match-score 3,x", "--match 7 --match-score 0,5",
                "--match 7 --match-score 3,8", "--match 7 --match-score 1,5", "--match 7 --match-score 3,5 --match-crawford 1",
                "--match 7 --match-score 3,5 --match-crawford 3", "--match 7 --match-score 3,5 --match-window 1.5",
                "--match 7 --match-score 3,5 --match-window nan", "--match 7 --match-score 3,5 --match-gammons 0.5",
                "--match 7 --match-score 3,5 --match-gammons 0.5,1.5", "--match 7 --match-score 3,5 --match-lookahead 2",
                "--match 7 --match-score 3,5 --match-scale nan", "--match 7 --match-score 3,5 --match-cube 1,0",
                "--match 7 --match-score 3,5 --match-cube 0,1", "--match 7 --match-score 3,5 --match-cube 11,1",
                "--match-window 0.5", "--met t.json", "--match-decision", "--match-crawford 0", "--match-cube 0,0",
                "--match-net v.pt", "--match 7 --match-score 3,5 --cube-decision"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + bad).split())
    # a rule option without weights for it: nobody would double
    with pytest.raises(SystemExit):
        ap.parse_args("--net random --positions opening --match 7 --match-score 3,5 --match-window 0.3".split())


# ------------------------------------------------------------------------- the C ABI --
ENTRIES = (("bgx_rollout_match_sel", 11), ("bgx_rollout_match_decide", 23), ("bgx_rollout_match_flush", 11),
           ("bgx_match_decision", 13))


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
    fields = re.search(r"enum bgx_rollout_match_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ROLLOUT_MATCH_(\w+)\s*=\s*(\d+)", fields)
    rename = {"log2": "cube_log2"}
    assert [(rename.get(n.lower(), n.lower()), int(v)) for n, v in names] == \
        [(f, M.MATCH_BINS + i) for i, f in enumerate(M.MATCH_HIST_FIELDS)]
    assert re.search(r"#define BGX_ROLLOUT_MATCH_BINS 88\b", header) and re.search(r"#define BGX_ROLLOUT_MATCH_ROW 96\b", header)
    assert (M.MATCH_BINS, M.MATCH_HIST_ROW) == (88, 96)
    assert M.match_bin(1, 3, 10) == 87 and M.match_bin(0, 0, 0) == 0 and M.match_bin(True, 2, 1) == 67
    # the device code is part 2 of csrc/bg_match_rollout.h, compiled with bg_returns.hip after bg_match.h, and only there
    csrc = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc")
    src = open(os.path.join(csrc, "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_match.h"') < src.index('#include "bg_match_rollout.h"')
    for f in os.listdir(csrc):
        if f not in ("bg_returns.hip", "bg_match_rollout.h"):
            assert "bg_match_rollout.h" not in open(os.path.join(csrc, f)).read(), f
    # part 1 builds the decision from bg_match.h's functions, not copies of them
    text = open(os.path.join(csrc, "bg_match_rollout.h")).read()
    part1 = re.sub(r"//[^\n]*", "", text.split("#ifndef BGX_MATCH_ROLLOUT_PART1_ONLY")[0])
    for fn in ("match_access(", "match_offers(", "match_passes(", "cube_taken("):
        assert fn in part1, fn
    assert "ct_mul" not in part1 and "met_after" not in part1 and "__global__" not in part1
    part2 = text.split("#ifndef BGX_MATCH_ROLLOUT_PART1_ONLY")[1]
    assert "__shared__" not in part2 and "__syncthreads" not in part2 and "malloc" not in part2
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name, _ in ENTRIES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def test_rollout_rule_host_program(tmp_path):
    """tools/match_rollout_host.cpp with AddressSanitizer + UBSan, a program of its own: every
    score of L = 1..7, every Crawford state, cube byte and mover on both tables; the tables are
    heap blocks of their exact size, so a lookup outside them stops the program."""
    exe = str(tmp_path / "match_rollout_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "match_rollout_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, \
        out.stderr[-2000:]
    m = re.fullmatch(r"cases (\d+) nones (\d+) takes (\d+) passes (\d+)\n", out.stdout)
    assert m, out.stdout
    cases, nones, takes, passes = (int(v) for v in m.groups())
    # 2 tables x sum of L^2 scores x 3 Crawford states x 256 bytes x 2 movers x 3 windows x 3 shares x 12 values
    assert cases == 2 * sum(L * L for L in range(1, 8)) * 3 * 256 * 2 * 3 * 3 * 12
    assert nones + takes + passes == cases and takes > 0 and passes > 0


# ------------------------------------------- the hand-set state of the GPU test, on the host --
@pytest.mark.parametrize("L", [5, 7])
def test_hand_set_state_reaches_every_branch(L):
    import match_rollout_ref as ref
    s = ref.make_state(L)
    out, seen = ref.expected(s, *M.met_table(L))
    assert seen == ref.BRANCHES, ref.BRANCHES - seen
    assert out["hist_flush"][:, 88].sum() == out["hist_flush"][:, :88].sum() > out["hist"][:, 88].sum() > 0
    assert (out["flags"] & 8).any() and (out["flags"] & 2).any() and (out["flags"] & 4).any()
    assert np.isnan(out["values"][np.isnan(s["value"]), 0]).all() and not np.isnan(out["values"][:, 2]).any()


def test_forced_values_of_the_traced_runs():
    import match_rollout_ref as ref
    m = M.RolloutMatch(7, rule(window=0.0, win_gammons=0.0, loss_gammons=0.0))
    for away in ref.FORCED_SCORES:
        v, k = ref.forced_value(m, away, 1)
        assert 0.0 < v < 0.5 and k + 1 == 3, (away, v, k)        # the cube climbs to 8, dead for both: each needs less
        assert ref.forced_value(m, away, 2)[0] > v
    with pytest.raises(AssertionError):                          # at 5-away / 3-away no one value is taken at every cube
        ref.forced_value(m, (5, 3), 1)
    for r in (ref.RACE, ref.GAMMONISH):
        assert r[:24].sum() + r[50] == 15 and r[24:48].sum() + r[51] == 15
    assert ref.GAMMONISH[51] == 0
