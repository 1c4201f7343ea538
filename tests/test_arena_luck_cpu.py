"""Luck-adjusted arena results on the host (no GPU): the luck of a roll under the
mid-game and the opening distribution (arena.arena_roll_luck_reference, the numpy twin of part 1 of
csrc/bg_arena_luck.h), the summary (arena.summarize_luck) against numpy, the replay of the
bookkeeping (arena.arena_luck_reference) on a hand-made trace, the parser, the declarations, and
part 1 itself as a sanitised host program (tools/arena_luck_host.cpp)."""
import ctypes
import math
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from bgx import _lib, arena as A, cube as C, replay as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = 65536
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]
DOUBLES = [r for r, (a, b) in enumerate(ROLLS21) if a == b]
NAN, INF = float("nan"), float("inf")


def round_f32(q: Fraction):
    lo = F(float(q))                                         # within an ulp: the nearest is among its neighbours
    cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
    return min(cands, key=lambda t: (abs(Fraction(float(t)) - q), int(F(t).view(np.int32)) & 1))


def chain(v, opening):
    """The mean's FMA chain in exact rationals, every step rounded once to fp32: §10's over the 21
    rolls, or 1/15 over the 15 non-doubles."""
    mean = F(0)
    for r, (a, b) in enumerate(ROLLS21):
        if opening and a == b:
            continue
        p = F(1) / F(15) if opening else (F(1) / F(36) if a == b else F(2) / F(36))
        mean = round_f32(Fraction(float(p)) * Fraction(float(v[r])) + Fraction(float(mean)))
    return mean


def one(v, d0, d1, opening):
    luck, mean = A.arena_roll_luck_reference(np.asarray(v, F).reshape(1, 21), [d0], [d1], [opening])
    return luck[0], mean[0]


# --------------------------------------------------------------- the luck of a roll --
def test_hand_values():
    """v_r = 1 on the roll 6-5, else 0: mid-game the roll has probability 2/36, at an opening 1/15;
    v_r = 1 on 3-3 only: 1/36 mid-game, and nothing at an opening."""
    v = np.zeros(21, F)
    v[ROLLS21.index((5, 6))] = 1
    for d in ((6, 5), (5, 6)):                               # the dice in either order
        luck, mean = one(v, *d, 0)
        assert mean == F(2) / F(36) and luck == F(1) - F(2) / F(36)
        luck, mean = one(v, *d, 1)
        assert mean == F(1) / F(15) and luck == F(1) - F(1) / F(15)
    luck, mean = one(v, 2, 1, 1)
    assert mean == F(1) / F(15) and luck == -(F(1) / F(15))
    w = np.zeros(21, F)
    w[ROLLS21.index((3, 3))] = 1
    assert one(w, 3, 3, 0) == (F(1) - F(1) / F(36), F(1) / F(36))
    assert one(w, 4, 2, 1) == (F(0), F(0))
    # the 21 weights, and the 15, sum to 1: a linear v gives its plain mean
    lin = np.arange(21, dtype=F) / F(8)
    p = np.array([1 if a == b else 2 for a, b in ROLLS21]) / 36.0
    assert one(lin, 1, 2, 0)[1] == pytest.approx(float((p * lin).sum()), rel=1e-6)
    nd = [r for r in range(21) if r not in DOUBLES]
    assert one(lin, 1, 2, 1)[1] == pytest.approx(float(lin[nd].mean()), rel=1e-6)
    assert one(lin, 1, 2, 1)[0] == pytest.approx(float(lin[1] - lin[nd].mean()), abs=1e-6)


def test_mid_game_is_the_section_10_chain_bit_for_bit():
    rng = np.random.RandomState(5)
    for k in range(40):
        v = (rng.randn(21) * (10.0 ** rng.randint(-3, 3))).astype(F)
        d = ROLLS21[k % 21]
        for opening in (0, 1):
            want = chain(v, opening)
            luck, mean = one(v, d[1], d[0], opening)
            assert mean.view(np.int32) == F(want).view(np.int32), (k, opening)
            drawn = not (opening and d[0] == d[1])
            assert luck.view(np.int32) == (F(v[k % 21]) - want if drawn else F(0)).view(np.int32)
    # cube.fma32 itself against exact rationals, one step
    a, b, c = (rng.randn(2000) * 3).astype(F), rng.randn(2000).astype(F), (rng.randn(2000) * 1e-3).astype(F)
    got = C.fma32(a, b, c)
    for i in range(0, 2000, 7):
        want = round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want


def test_opening_gives_doubles_no_weight():
    rng = np.random.RandomState(6)
    v = rng.randn(8, 21).astype(F)
    w = v.copy()
    w[:, DOUBLES] = np.array([1e30, -1e30, NAN, INF, -INF, 7.0], F)
    roll = np.array([ROLLS21[r] for r in (1, 2, 3, 7, 8, 12, 16, 19)])
    l0, m0 = A.arena_roll_luck_reference(v, roll[:, 0], roll[:, 1], 1)
    l1, m1 = A.arena_roll_luck_reference(w, roll[:, 0], roll[:, 1], 1)
    assert np.array_equal(l0.view(np.int32), l1.view(np.int32)) and np.array_equal(m0.view(np.int32), m1.view(np.int32))
    # mid-game they have weight
    assert not np.array_equal(A.arena_roll_luck_reference(v, roll[:, 0], roll[:, 1], 0)[1], m0)


def test_opening_constant_values():
    """A position whose value does not depend on the roll has no luck.  At c = 0, +-0.5, +-1 (a game
    decided whatever the roll, in the value head's unit) the chain of 15 steps gives the constant
    back exactly: luck 0, the mean within 1 ulp.  For any other constant the 15 weights sum to 1
    only within rounding: fl(1/15) carries a relative error <= 2^-24 and each of the 15 FMA steps
    rounds a partial sum of magnitude <= |c| (1 + 2^-20), so |mean - c| <= 16 * 2^-24 |c| (1 + 2^-20)
    <= 16 ulp(c) and |luck| the same; measured on 10^5 normal constants the largest is 4 ulp (the
    mid-game chain of §10: 5 ulp)."""
    for c in (0.0, 0.5, -0.5, 1.0, -1.0):
        luck, mean = one(np.full(21, c, F), 4, 1, 1)
        assert luck == 0.0 and abs(float(mean) - c) <= float(np.spacing(F(abs(c)))), c
    cs = np.random.RandomState(7).randn(4000).astype(F)
    luck, mean = A.arena_roll_luck_reference(np.repeat(cs[:, None], 21, 1), 6, 2, 1)
    ulp = np.spacing(np.abs(cs)).astype(np.float64)
    assert (np.abs(mean.astype(np.float64) - cs) <= 16 * ulp).all() and (np.abs(luck.astype(np.float64)) <= 16 * ulp).all()


def test_double_at_an_opening_and_no_roll_give_zero():
    v = np.random.RandomState(8).randn(21).astype(F)
    for d in range(1, 7):
        luck, mean = one(v, d, d, 1)
        assert luck == 0.0 and mean == chain(v, 1)          # the mean is still the opening's
        assert one(v, d, d, 0)[0] == F(v[ROLLS21.index((d, d))]) - chain(v, 0)
    for d0, d1 in ((0, 0), (0, 3), (7, 1), (2, 255)):
        for opening in (0, 1):
            luck, mean = one(v, d0, d1, opening)
            assert luck == 0.0 and mean == chain(v, opening)
    # any non-zero `opening` is an opening
    assert one(v, 2, 1, 255) == one(v, 2, 1, 1)


def test_nan_and_infinity_propagate():
    base = np.random.RandomState(9).randn(21).astype(F)
    r12, r13 = ROLLS21.index((1, 2)), ROLLS21.index((1, 3))
    for opening in (0, 1):
        v = base.copy()
        v[r12] = NAN
        for d in ((1, 2), (1, 3)):
            luck, mean = one(v, *d, opening)
            assert math.isnan(luck) and math.isnan(mean)
        v[r12] = INF
        luck, mean = one(v, 1, 2, opening)
        assert math.isnan(luck) and mean == INF             # inf - inf
        assert one(v, 1, 3, opening)[0] == -INF
        v[r13] = -INF
        assert math.isnan(one(v, 4, 5, opening)[1])          # inf + -inf in the chain
    v = base.copy()
    v[DOUBLES[2]] = NAN                                      # in a double: mid-game only
    assert math.isnan(one(v, 1, 2, 0)[0]) and not math.isnan(one(v, 1, 2, 1)[0])


# ------------------------------------------------------------------------ the summary --
def plain_tally(results):
    """results: x = +-1 / 2 / 3 from A's side per game -> the 16 plain entries."""
    t = dict.fromkeys(A.FIELDS, 0)
    for x in results:
        s = "a" if x > 0 else "b"
        t["games"] += 1
        t["wins_" + s] += 1
        t["points_" + s] += abs(x)
        t["gammons_" + s] += abs(x) == 2
        t["backgammons_" + s] += abs(x) == 3
    return [t[f] for f in A.FIELDS] + [0, 0]


def luck_tally(results, lucks):
    lq = [int(q) for q in RP.luck_q(np.asarray(lucks, F))]
    sq = [q * q for q in lq]
    return [sum(lq), sum(s & ((1 << 30) - 1) for s in sq), sum(s >> 30 for s in sq),
            sum(x * q for x, q in zip(results, lq)), len(lq), 0, 0, 0], np.array(lq, np.float64) / ONE


GAMES = [1, 1, -1, 2, -2, 3, -3, -1, 1, 2, 1, -1, -1, 1, -2]
LUCKS = [0.8, 0.31, -0.6, 1.4, -1.1, 1.9, -2.2, 0.2, -0.1, 0.7, 1.2, -0.9, -0.3, 0.05, -1.6]


def numpy_summary(x, L, c):
    x, L = np.asarray(x, np.float64), np.asarray(L, np.float64)
    y = x - c * L
    n = len(x)
    return dict(ppg_luck_a=y.mean(), ppg_luck_stderr=y.std(ddof=1) / math.sqrt(n),
                variance_ratio=y.var(ddof=1) / x.var(ddof=1), luck_mean=L.mean(),
                luck_mean_stderr=L.std(ddof=1) / math.sqrt(n))


@pytest.mark.parametrize("scale", [1.0, 0.0, 1.7, -0.5, "fit"])
def test_summarize_luck_against_numpy(scale):
    lt, L = luck_tally(GAMES, LUCKS)
    r = A.summarize_luck(plain_tally(GAMES), lt, steps=11, unfinished=0, scale=scale)
    c = np.cov(GAMES, L)[0, 1] / np.var(L, ddof=1) if scale == "fit" else scale
    assert r["luck_scale"] == pytest.approx(c, rel=1e-12, abs=1e-15)
    for k, want in numpy_summary(GAMES, L, c).items():
        assert r[k] == pytest.approx(want, rel=1e-10, abs=1e-13), k
    plain = A.summarize(plain_tally(GAMES), 11, 0)
    assert all(r[k] == v for k, v in plain.items())          # summarize's entries as they are
    assert [r[f] for f in A.LUCK_FIELDS] == lt[:5]
    if scale == "fit":
        assert r["variance_ratio"] <= 1.0 + 1e-12
        other = A.summarize_luck(plain_tally(GAMES), lt, 11, 0, scale=c + 0.1)
        assert other["ppg_luck_stderr"] > r["ppg_luck_stderr"]       # the fit is the minimum


def test_summarize_luck_degenerate():
    # L == 0: nothing to fit, nothing changes
    lt, _ = luck_tally(GAMES, [0.0] * len(GAMES))
    r = A.summarize_luck(plain_tally(GAMES), lt, 3, 0)
    assert r["luck_scale"] == 0.0 and r["ppg_luck_a"] == r["ppg_a"] and r["variance_ratio"] == pytest.approx(1.0, abs=1e-12)
    assert r["ppg_luck_stderr"] == pytest.approx(r["ppg_stderr"], rel=1e-12) and r["luck_mean_stderr"] == 0.0
    # a constant result: cov = 0 exactly, the fit is 0 and the ratio 1.0 by definition
    lt, _ = luck_tally([2] * 6, LUCKS[:6])
    r = A.summarize_luck(plain_tally([2] * 6), lt, 3, 0)
    assert r["luck_scale"] == 0.0 and r["ppg_luck_a"] == 2.0 and r["variance_ratio"] == 1.0 and r["ppg_luck_stderr"] == 0.0
    r = A.summarize_luck(plain_tally([2] * 6), lt, 3, 0, scale=1.0)
    assert r["variance_ratio"] == 1.0 and r["ppg_luck_stderr"] > 0.0
    # n = 0 and n = 1
    r = A.summarize_luck([0] * 16, [0] * 8, 0, 4)
    assert r["games"] == 0 and r["unfinished_lanes"] == 4
    assert all(r[k] == 0.0 for k in ("ppg_luck_a", "ppg_luck_stderr", "luck_scale", "luck_mean", "luck_mean_stderr"))
    assert r["variance_ratio"] == 1.0
    lt, L = luck_tally([3], [0.75])
    r = A.summarize_luck(plain_tally([3]), lt, 1, 0, scale=2.0)
    assert r["ppg_luck_a"] == 3.0 - 2.0 * 0.75 and r["ppg_luck_stderr"] == 0.0 and r["luck_mean"] == 0.75
    assert r["variance_ratio"] == 1.0 and A.summarize_luck(plain_tally([3]), lt, 1, 0)["luck_scale"] == 0.0


def test_summarize_luck_needs_the_hi_part_and_counts_games():
    # |Lq| = 2^21 (the clamp): Lq^2 = 2^42 sits in LUCK2_HI alone; the smaller ones fill LUCK2_LO too
    xs, Ls = [1, -1, 2, -3], [40.0, -33.0, 0.30518, -12.75]
    lt, L = luck_tally(xs, Ls)
    assert L[0] == 32.0 and L[1] == -32.0 and lt[2] >= 2 * (1 << 12) and lt[1] > 0
    r = A.summarize_luck(plain_tally(xs), lt, 5, 0, scale=0.1)
    for k, want in numpy_summary(xs, L, 0.1).items():
        assert r[k] == pytest.approx(want, rel=1e-10), k
    wrong = list(lt)
    wrong[1], wrong[2] = lt[1] + (lt[2] << 30), 0            # the same sum in LO alone reads the same
    assert A.summarize_luck(plain_tally(xs), wrong, 5, 0, scale=0.1)["ppg_luck_stderr"] == r["ppg_luck_stderr"]
    with pytest.raises(ValueError, match="counts 4 games"):
        A.summarize_luck(plain_tally(xs + [1]), lt, 5, 0)
    with pytest.raises(ValueError, match="entries"):
        A.summarize_luck(plain_tally(xs), lt[:4], 5, 0)


# -------------------------------------------------------------------------- the replay --
def info_word(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def hand_trace():
    """Two lanes, two games each.  Lane 0: A is PLAYER1 in game 0, PLAYER2 in game 1; lane 1 the
    other way round.  [owner, done, info, roll] per step and lane; owner 0 = the lane is retired."""
    steps = [  # lane 0                                 lane 1
        ((1, 0, 0, (3, 1)),                   (2, 0, 0, (6, 4))),                   # both openings
        ((2, 1, info_word(1, 2), (2, 2)),     (1, 0, 0, (5, 5))),                   # lane 0: B (PLAYER2) wins a gammon
        ((2, 0, 0, (4, 3)),                   (2, 0, 0, (2, 1))),                   # lane 0: game 1's opening, B first
        ((2, 1, info_word(0, 1), (6, 6)),     (1, 1, info_word(1, 3), (1, 1))),     # lane 0's last game; lane 1: A (PLAYER2) wins 3
        ((0, 0, 0, (5, 2)),                   (1, 0, 0, (6, 5))),                   # lane 0 retired; lane 1: game 1's opening
        ((0, 0, 0, (1, 2)),                   (2, 1, 0, (3, 3))),                   # a done without a winner: not counted
        ((0, 1, info_word(0, 1), (1, 2)),     (1, 1, info_word(0, 2), (4, 2))),     # opening again; A (PLAYER1) wins 2
        ((0, 0, 0, (1, 2)),                   (0, 0, 0, (6, 1))),                   # nothing is added any more
    ]
    T = len(steps)
    rng = np.random.RandomState(11)
    tr = dict(owner=np.zeros((T, 2), np.uint8), done=np.zeros((T, 2), np.uint8), info=np.zeros((T, 2), np.int32),
              luck_roll=np.zeros((T, 2, 2), np.uint8), luck_values=rng.randn(T, 2, 21).astype(F))
    for t, row in enumerate(steps):
        for i, (o, d, inf, roll) in enumerate(row):
            tr["owner"][t, i], tr["done"][t, i], tr["info"][t, i], tr["luck_roll"][t, i] = o, d, inf, roll
    return tr


def test_reference_hand_made_trace():
    tr = hand_trace()
    out = A.arena_luck_reference(tr, 2, 2)
    want_open = np.array([[1, 1], [0, 0], [1, 0], [0, 0], [0, 1], [0, 0], [0, 1], [0, 0]], np.uint8)
    assert np.array_equal(out["opening"], want_open)
    assert np.array_equal(out["games_done"], [2, 2])
    v, roll = tr["luck_values"], tr["luck_roll"]

    def luck(t, i, opening):
        return one(v[t, i], roll[t, i, 0], roll[t, i, 1], opening)[0]

    # lane 0, game 0: A's roll at an opening, then B's mid-game double; game 1: B's opening roll, B's 6-6
    g00 = F(F(0) + luck(0, 0, 1)) - luck(1, 0, 0)
    g01 = F(F(0) - luck(2, 0, 1)) - luck(3, 0, 0)
    # lane 1, game 0: B's opening, A's 5-5, B's 2-1, A's 1-1; the uncounted game: A's opening 6-5, B's 3-3;
    # game 1: A's opening 4-2
    g10 = F(F(F(F(0) - luck(0, 1, 1)) + luck(1, 1, 0)) - luck(2, 1, 0)) + luck(3, 1, 0)
    g11 = F(0) + luck(6, 1, 1)
    games = [(g00, -2), (g01, -1), (g10, 3), (g11, 2)]
    lq = [int(RP.luck_q(np.array([g], F))[0]) for g, _ in games]
    assert all(q != 0 for q in lq)
    want = [sum(lq), sum((q * q) & ((1 << 30) - 1) for q in lq), sum((q * q) >> 30 for q in lq),
            sum(q * x for q, (_, x) in zip(lq, games)), 4, 0, 0, 0]
    assert out["luck_tally"].tolist() == want
    assert np.array_equal(out["lane_luck"], [0, 0])
    # the per-step luck: the twin on the traced values, NaN off the selection
    on = tr["owner"] != 0
    assert np.isnan(out["luck"][~on]).all() and np.isnan(out["mean"][~on]).all() and not np.isnan(out["luck"][on]).any()
    assert out["luck"][5, 1] == luck(5, 1, 0) and out["luck"][4, 1] == luck(4, 1, 1)
    assert out["luck"][1, 0] == luck(1, 0, 0) != 0              # a double mid-game has luck
    # an opening taken mid-game would differ
    assert luck(0, 0, 0) != luck(0, 0, 1)
    # G = 1: each lane stops after its first game
    out1 = A.arena_luck_reference(tr, 2, 1)
    lq1 = [lq[0], lq[2]]
    assert out1["luck_tally"][0] == sum(lq1) and out1["luck_tally"][4] == 2 and out1["games_done"].tolist() == [1, 1]


# -------------------------------------------------------------------------- ArenaLuck --
def test_arena_luck_arguments():
    from bgx.search import ValueHead
    vh = object.__new__(ValueHead)
    assert A.ArenaLuck(vh).scale == "fit" and A.ArenaLuck(vh, scale=2).scale == 2.0
    with pytest.raises(ValueError):
        A.ArenaLuck("net.pt")
    with pytest.raises(ValueError):
        A.ArenaLuck(vh, scale=NAN)
    with pytest.raises(ValueError):
        A.ArenaLuck(vh, scale="best")


# -------------------------------------------------------------------------- the parser --
def test_parser_flags():
    ap = A.build_parser()
    ns = ap.parse_args("--a a.pt --b b.pt --max-steps 10".split())
    assert ns.luck is False and ns.luck_net is None and ns.luck_scale == "fit"
    ns = ap.parse_args("--a a.pt --b random --max-steps 10 --luck".split())
    assert ns.luck is True and ns.luck_scale == "fit"
    ns = ap.parse_args("--a random --b random --max-steps 10 --luck --luck-net v.pt --luck-scale 1.5".split())
    assert ns.luck_net == "v.pt" and ns.luck_scale == 1.5
    assert ap.parse_args("--a random --b b.pt --max-steps 10 --luck --luck-scale fit".split()).luck_scale == "fit"
    for bad in ("--a a.pt --b b.pt --max-steps 10 --luck --cube",
                "--a random --b random --max-steps 10 --luck",
                "--a a.pt --b b.pt --max-steps 10 --luck --luck-scale nan",
                "--a a.pt --b b.pt --max-steps 10 --luck --luck-scale much",
                "--a a.pt --b b.pt --max-steps 10 --luck-scale 1.0",
                "--a a.pt --b b.pt --max-steps 10 --luck-net v.pt"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def test_luck_from_args_picks_the_net(monkeypatch):
    from bgx import search
    monkeypatch.setattr(search, "ValueHead", type("VH", (search.ValueHead,), {"__init__": lambda s, net: setattr(s, "net", net)}))
    monkeypatch.setattr(A, "load_net", lambda path, dev: "loaded:" + path)
    ap = A.build_parser()
    base = "--a a.pt --b b.pt --max-steps 10 --luck"
    assert A.luck_from_args(ap.parse_args("--a a.pt --b b.pt --max-steps 10".split()), ["A", "B"], None) is None
    assert A.luck_from_args(ap.parse_args(base.split()), ["A", "B"], None).value.net == "A"
    assert A.luck_from_args(ap.parse_args(base.split()), [None, "B"], None).value.net == "B"
    lk = A.luck_from_args(ap.parse_args((base + " --luck-net v.pt --luck-scale 0.5").split()), ["A", "B"], None)
    assert lk.value.net == "loaded:v.pt" and lk.scale == 0.5


def test_eval_metrics_carry_the_luck_keys():
    from bgx.train import eval_metrics
    lt, _ = luck_tally(GAMES, LUCKS)
    ev = A.summarize_luck(plain_tally(GAMES), lt, 9, 0)
    m = eval_metrics(ev)
    assert m["eval_ppg_luck"] == ev["ppg_luck_a"] and m["eval_ppg_luck_stderr"] == ev["ppg_luck_stderr"]
    assert m["eval_variance_ratio"] == ev["variance_ratio"] and m["eval_ppg"] == ev["ppg_a"]
    assert "eval_ppg_luck" not in eval_metrics(A.summarize(plain_tally(GAMES), 9, 0))


def test_train_refuses_eval_luck_with_eval_cube(monkeypatch, capsys):
    import sys
    from bgx import train
    monkeypatch.setattr(sys, "argv", ["bgx.train", "--eval-every", "1", "--eval-luck", "--eval-cube"])
    with pytest.raises(SystemExit):
        train.main()                                         # the parser's error, before any device is touched
    assert "--eval-luck" in capsys.readouterr().err


# ------------------------------------------------------------------------- the C ABI --
ENTRIES = (("bgx_arena_luck_begin", 5), ("bgx_arena_luck_add", 10), ("bgx_arena_luck_flush", 11))


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in ENTRIES:
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):
            assert a is (_lib._P if "*" in p else _lib._I32), (name, p)
            assert "*" in p or p.startswith("int32_t "), (name, p)
    enum = re.search(r"enum bgx_arena_luck_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ARENA_(\w+)\s*=\s*(\d+)", enum)
    assert [(n.lower(), int(v)) for n, v in names] == [("luck", 0)] + [(f, i) for i, f in enumerate(A.LUCK_FIELDS)][1:]
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_cube_luck.h"') < src.index('#include "bg_arena_luck.h"')
    hdr = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_arena_luck.h")).read()
    assert "BGX_ARENA_LUCK_PART1_ONLY" in hdr and "1.0f / 15.0f" in hdr
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in ENTRIES:
        assert name in integration, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name, _ in ENTRIES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def test_luck_host_program(tmp_path):
    """tools/arena_luck_host.cpp with AddressSanitizer + UBSan, a program of its own: arena_roll_luck
    for every roll in both orders, bytes that are no roll, opening 0, 1 and 255, on rows of values
    that rotate through zeros, ordinary values, huge ones, NaN and the infinities (so each lands on
    doubles and non-doubles, on the roll and off it).  Bit for bit arena_roll_luck_reference."""
    exe = str(tmp_path / "arena_luck_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "arena_luck_host.cpp"), "-o", exe], check=True)
    rolls = ROLLS21 + [(b, a) for a, b in ROLLS21] + [(0, 0), (0, 4), (7, 2), (3, 255)]
    rng = np.random.RandomState(12)
    pool = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 0.37, -0.61, 100.0, -1e30, 3e38, 1e-40, NAN, INF, -INF], F),
                           rng.randn(40).astype(F)])
    rows = []
    for n in range(len(rolls) * 3 * 8):
        roll, opening = rolls[n % len(rolls)], (0, 1, 255)[(n // len(rolls)) % 3]
        if n % 4 == 0:
            v = rng.randn(21).astype(F)                      # finite rows: a quarter of the cases
        else:
            v = pool[(n * 5 + 3 * np.arange(21)) % len(pool)]
        rows.append((roll, opening, v))
    cases = [f"{r[0]} {r[1]} {op} " + " ".join(bits(x) for x in v) for r, op, v in rows]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(rows)
    roll = np.array([r for r, _, _ in rows])
    luck, mean = A.arena_roll_luck_reference(np.stack([v for _, _, v in rows]), roll[:, 0], roll[:, 1],
                                             [op for _, op, _ in rows])
    want = [[bits(l), bits(m)] for l, m in zip(luck, mean)]

    def same(g, w):                                          # NaN: any payload
        return all(a == b or (math.isnan(struct.unpack("<f", struct.pack("<I", int(a, 16)))[0]) and
                              math.isnan(struct.unpack("<f", struct.pack("<I", int(b, 16)))[0])) for a, b in zip(g, w))
    bad = [(cases[j], got[j], want[j]) for j in range(len(rows)) if not same(got[j], want[j])]
    assert not bad, bad[:3]
    assert int((luck != 0).sum()) > len(rows) // 3 and int(np.isnan(luck).sum()) > 20
    # a short line is refused, not computed
    r = subprocess.run([exe], input="1 2 0 0 0\n", capture_output=True, text=True)
    assert r.returncode == 2
