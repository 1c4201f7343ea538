"""Luck-adjusted cubeful rollouts on the host: the cubeful luck of a roll
(cube.cube_roll_luck_reference, the numpy twin of part 1 of csrc/bg_cube_luck.h), the summary
(tally.summarize_cube_luck), the replay of the three bookkeeping steps (cube.cube_luck_reference),
the mode table, the parser, the declarations, and part 1 itself as a sanitised host program."""
import ctypes
import importlib.util
import itertools
import math
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from bgx import _lib, cube as C, replay as RP, rollout as R, tally as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = 65536
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]


def cube_luck(**kw):
    from bgx.search import ValueHead
    return C.CubeLuck(object.__new__(ValueHead), **kw)


def rule(**kw):
    return C.CubeRule(lambda eng, dsel: None, **kw)


def g_of(v, cube=0, mover=0, life=None, cap=6, jacoby=False, scale=1.0):
    """g of one value: the mean of a row of 21 equal values (the chain's weights sum to 1 within 2 ulp)."""
    life = C.CubeLife(1.0) if life is None else life
    luck, mean = C.cube_roll_luck_reference(np.full((1, 21), v, F), np.array([cube], np.uint8), [mover], [[0, 0]],
                                            scale, life, cap, jacoby)
    assert luck[0] == 0.0                                    # no roll: no luck
    return float(mean[0])


def chain(g):
    """fma(p_20, g_20, ... fma(p_0, g_0, 0)) in fp32, every step exact and rounded once."""
    mean = F(0)
    for r, (a, b) in enumerate(ROLLS21):
        p = F(1) / F(36) if a == b else F(2) / F(36)
        exact = Fraction(float(p)) * Fraction(float(g[r])) + Fraction(float(mean))
        mean = round_f32(exact)
    return mean


def round_f32(q: Fraction):
    lo = F(float(q))                                         # within an ulp: the nearest is among its neighbours
    cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
    return min(cands, key=lambda t: (abs(Fraction(float(t)) - q), int(F(t).view(np.int32)) & 1))


# --------------------------------------------------------------- the luck of a roll --
def test_hand_values_live_centred_cube():
    """W = L = 1, x = 1, the cube centred: the opponent, on roll after the move, sees p = (1 - v) / 2
    with TP = 0.2 and CP = 0.8; its e is -1 below TP, the line through (TP, -1) and (CP, 1) between
    them, 1 above CP (cashing never beats holding a fully live centred cube)."""
    for v, want in ((0.8, 1.0), (0.4, 2.0 / 3.0), (0.0, 0.0), (-0.4, -2.0 / 3.0), (-0.8, -1.0),
                    (0.62, 1.0), (0.58, 1.0 - 0.01 / 0.3), (-0.58, -(1.0 - 0.01 / 0.3)), (-0.62, -1.0)):
        assert g_of(v) == pytest.approx(want, abs=2e-6), v
    # values that are no equity: NaN counts as 0, infinities are clamped to -L and W
    assert g_of(math.nan) == pytest.approx(0.0, abs=1e-7)
    assert g_of(math.inf) == pytest.approx(1.0, abs=2e-6) and g_of(-math.inf) == pytest.approx(-1.0, abs=2e-6)
    # the scale turns the value's unit into points before anything else
    assert g_of(0.2, scale=2.0) == pytest.approx(2.0 / 3.0, abs=2e-6)


def test_hand_values_owners_and_movers():
    """x = 1, v = 0 (p = 0.5), k = 1: the mover owning the cube is worth +0.25 to it (the opponent on
    roll cannot double: E_opp = -0.25), the opponent owning it -0.25 (E_own = 0.25 beats cashing at
    2 E_opp = -0.5).  Owner 1 is PLAYER1 = mover byte 0; owner 3 reads as centred."""
    for mover in (0, 1):
        assert g_of(0.0, C.pack(1, mover + 1), mover) == pytest.approx(0.25, abs=1e-6)
        assert g_of(0.0, C.pack(1, 2 - mover), mover) == pytest.approx(-0.25, abs=1e-6)
        assert g_of(0.3, C.pack(1, 3), mover) == g_of(0.3, C.pack(1, 0), mover)
        assert g_of(0.0, 0, mover) == pytest.approx(0.0, abs=1e-7)


def test_hand_values_last_double_dead_cube_and_jacoby():
    # k + 1 = cap: the opponent owns the cube at 2^5 with cap 6; its double leaves a dead cube, DT = 2 c.
    # p = 0.7 (c = 0.4): E_own = -1 + 0.7 * 2.5 = 0.75 < min(0.8, 1): it doubles, e = 0.8
    assert g_of(-0.4, C.pack(5, 2), 0) == pytest.approx(-0.8, abs=2e-6)
    # one step lower the double is live: 2 E_opp = 2 (-1 + 0.5 * 2.5) = 0.5 < 0.75: it holds
    assert g_of(-0.4, C.pack(4, 2), 0) == pytest.approx(-0.75, abs=2e-6)
    # a dead cube (k >= cap, or cap 0): g is the clamped value itself, bit for bit
    for v in (0.37, -2.9, 3.0, -3.0, 5.0):
        want = F(np.clip(F(v), -3, 3))
        for cube, cap in ((0, 0), (C.pack(6, 1), 6), (C.pack(15, 2), 10)):
            luck, mean = C.cube_roll_luck_reference(np.full((1, 21), v, F), [cube], [0], [[3, 1]], 1.0,
                                                    C.CubeLife(0.68, 3.0, 3.0), cap)
            assert mean[0] == chain([want] * 21) and luck[0] == F(want - mean[0])
    # Jacoby, the cube centred, x = 0, W = L = 2: the opponent at c = -0.2 (p = 0.45) holds 2 p - 1 = -0.1
    # instead of c; cashing at 2 c = -0.4 is worse either way
    life = C.CubeLife(0.0, 2.0, 2.0)
    assert g_of(0.2, 0, 0, life, jacoby=True) == pytest.approx(0.1, abs=1e-6)
    assert g_of(0.2, 0, 0, life, jacoby=False) == pytest.approx(0.2, abs=1e-6)
    assert g_of(0.2, C.pack(1, 1), 0, life, jacoby=True) == pytest.approx(0.2, abs=1e-6)       # only while centred


def test_dead_cube_is_the_cubeless_luck_bit_for_bit():
    """cap = 0, W = L = 3, values inside +-3: g_r = v_r exactly, so mean and luck are bgx_roll_luck's."""
    rng = np.random.default_rng(5)
    v = (rng.uniform(-3, 3, (40, 21))).astype(F)
    rolls = np.array([ROLLS21[i % 21][::(1 if i % 2 else -1)] for i in range(40)], np.uint8)
    rolls[7] = (0, 0)
    luck, mean = C.cube_roll_luck_reference(v, None, np.arange(40) & 1, rolls, 1.0, C.CubeLife(0.68, 3.0, 3.0), 0)
    for i in range(40):
        m = chain(v[i])
        assert mean[i] == m
        want = F(0) if i == 7 else F(v[i, C.roll_index(rolls[i:i + 1])[0]] - m)
        assert luck[i] == want


def test_fma32_and_roll_index():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(3000).astype(F), rng.standard_normal(3000).astype(F)
    c = (rng.standard_normal(3000) * rng.choice([1e-9, 1e-3, 1.0, 1e5], 3000)).astype(F)
    # exact ties of the fp64 sum: c = -fp32(a b) leaves the product's low bits alone
    c[:500] = -(a[:500] * b[:500])
    got = C.fma32(a, b, c)
    for i in range(3000):
        assert got[i] == round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))), i
    assert C.roll_index([(a, b) for a, b in ROLLS21]).tolist() == list(range(21))
    assert C.roll_index([(b, a) for a, b in ROLLS21]).tolist() == list(range(21))
    assert C.roll_index([(0, 0), (0, 3), (7, 1), (6, 255)]).tolist() == [-1] * 4
    assert C.ROLL_P.sum() == pytest.approx(1.0, abs=1e-6) and C.ROLL_P[[0, 6, 11, 15, 18, 20]].tolist() == [F(1) / F(36)] * 6


@pytest.mark.parametrize("x,W,L", [(0.0, 1.0, 1.0), (0.68, 1.0, 1.0), (1.0, 1.0, 1.0), (0.68, 1.7, 1.4), (1.0, 3.0, 1.0),
                                   (0.3, 1.0, 3.0)])
@pytest.mark.parametrize("jacoby", [False, True])
def test_g_is_non_decreasing_in_v_fp64(x, W, L, jacoby):
    """In fp64, for every cube state as the opponent on roll sees it: e = max(E, min(2 E_opp, 1)) with
    access, E without, c when dead is non-decreasing in p, so g = -e(-v) is non-decreasing in v."""
    life = C.CubeLife(x, W, L)
    p = np.linspace(0.0, 1.0, 20001)
    c, cen, own, opp = C.janowski_equities(p, life, jacoby)
    cash = np.minimum(2.0 * opp, 1.0)
    for e in (np.maximum(cen, cash), np.maximum(own, cash), opp, c, np.maximum(cen, np.minimum(2.0 * c, 1.0)),
              np.maximum(own, np.minimum(2.0 * c, 1.0))):
        assert (np.diff(e) >= -1e-12).all()
    # and the fp32 twin follows it: g over rising v, every owner, both a live and the last double
    v = np.linspace(-W - 0.1, L + 0.1, 2001).astype(F)
    for cube, cap in ((0, 6), (C.pack(1, 1), 6), (C.pack(1, 2), 6), (C.pack(5, 2), 6), (C.pack(6, 1), 6)):
        vals, _ = C.janowski_reference(-v, np.full(v.shape, cube, np.uint8), np.ones(v.shape, np.int64), 1.0, life, cap,
                                       jacoby)
        # ten fp32 operations on magnitudes up to 6, at either of two neighbouring points: 2 x 10 x 2^-22
        assert (np.diff(-vals[:, 2].astype(np.float64)) >= -5e-6).all()
        # the same through the luck's own twin: a row of one value has that value's g as its mean
        _, mean = C.cube_roll_luck_reference(np.repeat(v[::50, None], 21, axis=1), np.full(v[::50].shape, cube, np.uint8),
                                             np.zeros(v[::50].shape, np.int64), np.zeros((len(v[::50]), 2), np.uint8), 1.0,
                                             life, cap, jacoby)
        assert (np.diff(mean.astype(np.float64)) >= -5e-6).all()


# --------------------------------------------------------------------- the summary --
def rows_of(y, k, passed, lq, plies=7):
    """The three rows of explicit games: results y (points), cubes k, passed flags, luck Lq."""
    y, k, passed = np.asarray(y, np.int64), np.asarray(k, np.int64), np.asarray(passed).astype(bool)
    lq = [int(v) for v in lq]
    n = len(lq)
    tally = [int((~passed).sum()), plies * int((~passed).sum())] + [0] * 6
    for yi, ki, pi in zip(y, k, passed):
        if not pi:
            s = abs(int(yi)) >> int(ki)
            tally[(2 if yi > 0 else 5) + s - 1] += 1
    cube = [n, int(y.sum()), int((y * y).sum()), int(k.sum()), int(passed.sum()), 3 * int(passed.sum()),
            int((passed & (y > 0)).sum()), int(k.sum())]
    sq = [v * v for v in lq]
    luck = [sum(lq), sum(v & (2 ** 30 - 1) for v in sq), sum(v >> 30 for v in sq), sum(int(a) * b for a, b in zip(y, lq)), n]
    return tally, cube, luck


def games(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 4, n)
    passed = rng.random(n) < 0.3
    s = np.where(passed, 1, rng.integers(1, 4, n))
    y = np.where(rng.random(n) < 0.55, 1, -1) * (s << k)
    lq = np.rint((0.6 * y + rng.standard_normal(n) * (1 << k)) * ONE).astype(np.int64)
    return y, k, passed, lq


@pytest.mark.parametrize("scale", ["fit", 1.0, 0.5, 0.0, -2.0])
def test_summarize_cube_luck_against_numpy(scale):
    y, k, passed, lq = games(400, 3)
    t, c, lk = rows_of(y, k, passed, lq)
    r = T.summarize_cube_luck(t, c, lk, scale, unfinished=2)
    plain = T.summarize_cube(t, c, 2)
    for key, v in plain.items():
        assert r[key] == v, key                              # summarize_cube's keys, untouched
    L = lq / ONE
    cc = np.cov(y, L)[0, 1] / np.var(L, ddof=1) if scale == "fit" else float(scale)
    a = y - cc * L
    assert r["luck_scale"] == pytest.approx(cc, rel=1e-9, abs=1e-12)
    assert r["equity_cubeful_luck"] == pytest.approx(a.mean(), rel=1e-9, abs=1e-12)
    assert r["equity_cubeful_luck_stderr"] == pytest.approx(a.std(ddof=1) / math.sqrt(len(y)), rel=1e-8)
    assert r["variance_ratio"] == pytest.approx(a.var(ddof=1) / y.var(ddof=1), rel=1e-8)
    assert r["luck_mean"] == pytest.approx(L.mean(), rel=1e-9)
    assert [r[f] for f in T.CUBE_LUCK_FIELDS] == lk and r["games"] == 400 and r["unfinished"] == 2
    if scale == "fit":
        assert r["variance_ratio"] < 0.8                     # these games' luck explains their results
    if scale == 0.0:
        assert r["equity_cubeful_luck"] == r["equity_cubeful"] and r["variance_ratio"] == pytest.approx(1.0, rel=1e-12)
        assert r["equity_cubeful_luck_stderr"] == pytest.approx(r["equity_cubeful_stderr"], rel=1e-9)


def test_summarize_cube_luck_edges():
    y, k, passed, lq = games(50, 4)
    # no luck at all: the fit is 0 and nothing changes
    r = T.summarize_cube_luck(*rows_of(y, k, passed, np.zeros(50, np.int64)))
    assert (r["luck_scale"], r["luck_mean"], r["variance_ratio"]) == (0.0, 0.0, 1.0)
    assert r["equity_cubeful_luck"] == r["equity_cubeful"]
    # a constant result: the fit's numerator is exactly 0, the ratio is 1 by definition
    r = T.summarize_cube_luck(*rows_of(np.full(50, 2), np.ones(50), np.ones(50), lq))
    assert (r["luck_scale"], r["variance_ratio"], r["equity_cubeful_luck"]) == (0.0, 1.0, 2.0)
    assert r["equity_cubeful_luck_stderr"] == 0.0
    r = T.summarize_cube_luck(*rows_of(np.full(50, 2), np.ones(50), np.ones(50), lq), 1.0)
    assert r["variance_ratio"] == 1.0 and r["equity_cubeful_luck"] == pytest.approx(2.0 - lq.mean() / ONE, rel=1e-12)
    # no game, one game
    r = T.summarize_cube_luck([0] * 8, [0] * 8, [0] * 5)
    assert (r["games"], r["equity_cubeful_luck"], r["equity_cubeful_luck_stderr"], r["variance_ratio"], r["luck_scale"]) \
        == (0, 0.0, 0.0, 1.0, 0.0)
    r = T.summarize_cube_luck(*rows_of([4], [1], [0], [3 * ONE // 2]), 1.0)
    assert (r["games"], r["equity_cubeful_luck"], r["equity_cubeful_luck_stderr"], r["variance_ratio"]) == (1, 2.5, 0.0, 1.0)
    assert T.summarize_cube_luck(*rows_of([4], [1], [0], [3 * ONE // 2]))["luck_scale"] == 0.0


def test_summarize_cube_luck_needs_the_high_part():
    """Lq at the clamp: Lq^2 = 2^62 is 2^32 in LUCK2_HI; three such games pass 2^63 in one sum."""
    big = T.CUBE_LUCK_CLAMP
    y, lq = [3072, -3072, 1024, 2], [big, -big, big, 12345]
    t, c, lk = rows_of(y, [10, 10, 10, 1], [0, 0, 1, 0], lq)
    assert lk[2] == 3 * 2 ** 32 and lk[1] == (12345 * 12345) & (2 ** 30 - 1) and lk[3] == (2 * 3072 + 1024) * big + 2 * 12345
    assert (lk[2] << 30) > 2 ** 63
    r = T.summarize_cube_luck(t, c, lk, 0.01)
    L = np.array(lq, np.float64) / ONE
    a = np.array(y, np.float64) - 0.01 * L
    assert r["equity_cubeful_luck"] == pytest.approx(a.mean(), rel=1e-12)
    assert r["equity_cubeful_luck_stderr"] == pytest.approx(a.std(ddof=1) / 2.0, rel=1e-9)
    fit = T.summarize_cube_luck(t, c, lk)
    assert fit["luck_scale"] == pytest.approx(np.cov(y, L)[0, 1] / np.var(L, ddof=1), rel=1e-12)
    assert T.CUBE_LUCK_ONE == ONE and T.CUBE_LUCK_CLAMP == 2 ** 31 and len(T.CUBE_LUCK_FIELDS) == 5


def test_summarize_cube_luck_mismatch():
    t, c, lk = rows_of(*games(20, 1))
    lk[4] -= 1
    with pytest.raises(ValueError, match="the luck row counts 19 games, the cube row 20"):
        T.summarize_cube_luck(t, c, lk)
    with pytest.raises(ValueError, match="5 entries"):
        T.summarize_cube_luck(t, c, lk + [0])
    c[0] += 1
    with pytest.raises(ValueError, match="summarize_cube"):
        T.summarize_cube_luck(t, c, lk)


# ------------------------------------------------------------------------ the replay --
def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def test_cube_luck_q():
    q = RP.cube_luck_q(np.array([0.5, -2.5, 1.5 / ONE, 2.5 / ONE, 32768.0, 40000.0, -1e30, np.inf, -np.inf, np.nan, 3e38], F))
    assert q.tolist() == [32768, -163840, 2, 2, 2 ** 31, 2 ** 31, -2 ** 31, 0, 0, 0, 0]


def test_cube_luck_reference_hand_made_trace():
    """Three lanes, four steps, cap 6.  Lane 0 (group 0, two games, PLAYER1 starts, drawn first rolls):
    its first game collects +0.5 and ends at step 1 by PLAYER2's passed double (y = -1, booked before
    the decision is applied); the second game starts in that step (+0.25 for the start mover after the
    reset), is doubled and taken at step 2 -- the roll's luck of that step, -0.125 for PLAYER2, counts
    at the new cube: +0.25 -- and ends at step 3 with a gammon at 2: +1.0 x 2, L = 2.5, y = 4; the
    lane's last game.  Lane 1 (group 1, one game, PLAYER2 starts on a fixed first roll and owns the
    cube at 2): the first step's luck is left out, then -0.5 x 2 and +0.25 x 2, a single win: y = 2;
    its second game begins at step 3 on the fixed roll again, whose luck is left out too.  Lane 2 is idle."""
    nan = float("nan")
    ru = rule(double_at=0.4, pass_at=0.5, cap=6)
    group = np.array([0, 1, -1], np.int32)
    starts = np.zeros((3, 64), np.uint8)
    starts[1, 52], starts[1, 53], starts[1, 54] = 1, 3, 1
    cube0 = np.array([0, C.pack(1, 2), 0], np.uint8)
    mover = np.array([[0, 1, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0]], np.uint8).T
    eq = np.array([[0.9, 0.9, 0.45, 0.0], [0.9, 0.9, 0.3, 0.9], [0.9] * 4], F).T
    lmover = mover.copy()
    lmover[1, 0] = 0                                         # after the pass's reset PLAYER1 is on roll again
    luck = np.array([[0.5, 0.25, -0.125, 1.0], [9.0, 0.5, 0.25, 7.0], [nan] * 4], F).T
    done, inf_ = np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.int32)
    done[3, 0], inf_[3, 0] = 1, info(0, 2)
    done[2, 1], inf_[2, 1] = 1, info(1, 1)
    tr = dict(cube_mover=mover, cube_equity=eq, done=done, info=inf_, cube_luck=luck, cube_luck_mover=lmover)
    out = C.cube_luck_reference(tr, starts, group, 2, 2, ru, cube0)
    assert out["cube_luck_tally"][0].tolist() == [32768 + 163840, 0, 1 + 25, -32768 + 4 * 163840, 2]
    assert out["cube_luck_tally"][1].tolist() == [-32768, 0, 1, -2 * 32768, 1]
    assert out["cube_tally"].tolist() == [[2, 3, 17, 1, 1, 1, 0, 2], [1, 2, 4, 1, 0, 0, 0, 0]]
    assert out["tally"].tolist() == [[1, 3, 0, 1, 0, 0, 0, 0], [1, 3, 1, 0, 0, 0, 0, 0]]
    assert np.argwhere(out["mask"]).tolist() == [[1, 0]]
    assert out["cube_luck_state"][:, 0].tolist() == [0, 0, C.pack(1, 1), C.pack(1, 1)]
    assert out["cube_luck_state"][:3, 1].tolist() == [C.pack(1, 2)] * 3
    assert out["games_done"].tolist() == [2, 1, 0] and out["lane_luck"].tolist() == [0.0, 0.0, 0.0]
    # the same trace without the luck: the cube replay is untouched, and has no luck tally
    plain = C.cube_reference(tr, starts, group, 2, 2, ru, cube0)
    assert "cube_luck_tally" not in plain
    for key in ("cube_tally", "tally", "mask", "dsel", "cube", "games_done"):
        assert np.array_equal(plain[key], out[key]), key
    for p in range(2):
        r = C.summarize_cube_luck(out["tally"][p], out["cube_tally"][p], out["cube_luck_tally"][p], 1.0)
        assert r["games"] == (2, 1)[p]
    assert C.summarize_cube_luck(out["tally"][0], out["cube_tally"][0], out["cube_luck_tally"][0], 1.0)[
        "equity_cubeful_luck"] == (3 - 3.0) / 2
    # a non-finite sum is booked as 0
    luck[0, 0] = np.inf
    out = C.cube_luck_reference(tr, starts, group, 2, 2, ru, cube0)
    assert out["cube_luck_tally"][0].tolist() == [163840, 0, 25, 4 * 163840, 2]


def test_lane_replay_cubeless_luck_is_untouched():
    """The replay's cubeless luck steps do what they did: luck_add and the flush in advance."""
    starts = np.zeros((2, 64), np.uint8)
    rp = RP.LaneReplay(starts, np.array([0, 0]), 1, 1)
    assert callable(rp.cube_luck_add) and callable(rp.cube_luck_book)
    rp.tally("luck_tally", T.LUCK_FIELDS)
    rp.luck_add(np.array([0.5, -0.25], F), np.array([0, 1]))
    rp.advance(np.array([1, 1]), np.array([info(0, 1), info(1, 3)]))
    assert rp.tallies["luck_tally"].tolist() == [[32768 + 16384, 32768 ** 2 + 16384 ** 2, 32768 - 3 * 16384, 2]]
    assert "cube_luck_tally" not in rp.tallies and rp.luck.tolist() == [0.0, 0.0]


def test_cube_luck_arguments():
    cl = cube_luck()
    assert (cl.scale, cl.life.x, cl.life.win_value, cl.life.loss_value) == (1.0, 0.68, 1.0, 1.0)
    assert cube_luck(scale=2, life=C.CubeLife(0.0, 2.0, 3.0)).life.loss_value == 3.0
    for bad in (dict(scale=math.nan), dict(scale="fit"), dict(scale=True), dict(life=0.68)):
        with pytest.raises(ValueError):
            cube_luck(**bad)
    for wrong in (3.0, lambda eng, sel: None, None):
        with pytest.raises(ValueError, match="value must be a search.ValueHead"):
            C.CubeLuck(wrong)


# ------------------------------------------------------------------------- the modes --
def _old_table():
    spec = importlib.util.spec_from_file_location("_modes_table", os.path.join(ROOT, "tests", "test_rollout_modes_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


OLD = _old_table()

NEW = {
    (): "cube_luck without cube",
    ("luck",): "cube_luck without cube",
    ("truncate",): "cube_luck without cube",
    ("cube_bearoff",): "cube_luck without cube",
    ("cube_truncate",): "cube_luck without cube",
    ("cube",): OLD.OK,
    ("cube", "luck"): "cube_luck together with luck is not supported",
    ("cube", "bearoff"): "cube_luck together with bearoff is not supported",
    ("cube", "truncate"): "cube_luck together with truncate is not supported",
    ("cube", "cube_bearoff"): "cube_luck together with cube_bearoff is not supported",
    ("cube", "cube_truncate"): "cube_luck together with cube_truncate is not supported",
    ("cube", "cube_bearoff", "cube_truncate"): "cube_luck together with cube_bearoff is not supported",
    ("cube", "luck", "bearoff", "truncate", "cube_bearoff", "cube_truncate"): "cube_luck together with luck is not supported",
    ("cube", "truncate", "cube_truncate"): "cube_luck together with truncate is not supported",
}


def typed(modes):
    from bgx.search import ValueHead
    well = dict(OLD.well_typed(), cube_truncate=C.CubeTruncation(object.__new__(ValueHead), 8))
    return {n: well[n] for n in modes}


@pytest.mark.parametrize("modes", sorted(NEW))
def test_new_mode_refusals(modes):
    kw = dict(typed(modes), cube_luck=cube_luck())
    ro = object.__new__(R.Rollout)
    assert OLD.first_message(R.Rollout.run, ro, None, None, 36, **kw) == OLD.prefixed("run", NEW[modes])
    assert OLD.first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, **kw) == OLD.prefixed("run_lanes", NEW[modes])
    for where in ("run", "run_lanes"):
        assert OLD.first_message(R._check_modes, where, types=where == "run_lanes", **kw) == OLD.prefixed(where, NEW[modes])


@pytest.mark.parametrize("modes", sorted(OLD.EXPECTED)[::3])
def test_old_combinations_without_the_keyword(modes):
    """A sample of the table of tests/test_rollout_modes_cpu.py, called without cube_luck and with
    cube_luck=None: the keyword's default changes nothing."""
    import inspect
    assert list(inspect.signature(R._check_modes).parameters)[-1] == "cube_luck"       # the trailing keyword
    kw = {n: OLD.well_typed()[n] for n in modes}
    plain, with_cube0 = OLD.EXPECTED[modes]
    for extra in ({}, {"cube_luck": None}):
        assert OLD.first_message(R._check_modes, "run", **kw, **extra) == OLD.prefixed("run", plain)
        assert OLD.first_message(R._check_modes, "run_lanes", cube0=object(), types=True, **kw, **extra) \
            == OLD.prefixed("run_lanes", with_cube0)
    ro = object.__new__(R.Rollout)
    assert OLD.first_message(R.Rollout.run, ro, None, None, 36, cube_luck=None, **kw) == OLD.prefixed("run", plain)


def test_new_mode_type_check():
    ro = object.__new__(R.Rollout)
    for wrong in (8, object(), C.CubeLife()):
        assert OLD.first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, cube=object(), cube_luck=wrong) \
            == "run_lanes: cube_luck must be a cube.CubeLuck"
    assert OLD.first_message(R._check_modes, "run", cube=object(), cube_luck=8) == OLD.OK      # run leaves it to the lanes
    # the wrong type comes after the refusals
    assert OLD.first_message(R._check_modes, "run_lanes", cube=object(), luck=object(), types=True, cube_luck=8) \
        == "run_lanes: cube_luck together with luck is not supported"
    assert OLD.first_message(R._check_modes, "run_lanes", cube0=object(), types=True, cube_luck=cube_luck()) \
        == "run_lanes: cube_luck without cube"
    # the pinned refusal of the cubeless luck with a cube stays what it was
    assert OLD.first_message(R._check_modes, "run", cube=object(), luck=object()) \
        == "run: cube together with luck is not supported"


def test_summary_choice():
    assert R._summary(None, None, object(), None, None, None, object()) is T.summarize_cube_luck
    assert R._summary(None, None, object(), None, None, None) is T.summarize_cube
    assert R._summary(None, None, object(), None, None) is T.summarize_cube
    assert C.summarize_cube_luck is T.summarize_cube_luck and R.CUBE_LUCK_FIELDS is T.CUBE_LUCK_FIELDS


# --------------------------------------------------------------------------- the parser --
def messages(ap, line, capsys):
    with pytest.raises(SystemExit):
        ap.parse_args(line.split())
    return capsys.readouterr().err


def test_parser_flags(capsys):
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.cube_luck is False and ns.cube_luck_net is None and ns.cube_luck_scale == "fit"
    assert (ns.cube_luck_life, ns.cube_luck_win_value, ns.cube_luck_loss_value, ns.cube_luck_value_scale) \
        == (0.68, 1.0, 1.0, 1.0)
    ns = ap.parse_args("--net ckpt.pt --positions opening --cube --cube-decision --cube-luck --cube-luck-scale 0.9 "
                       "--cube-luck-life 0.5 --cube-luck-win-value 1.4 --cube-luck-loss-value 1.2 "
                       "--cube-luck-value-scale 2 --cube-luck-net v.pt".split())
    assert ns.cube_luck is True and ns.cube_luck_scale == 0.9 and ns.cube_luck_net == "v.pt"
    assert (ns.cube_luck_life, ns.cube_luck_win_value, ns.cube_luck_loss_value, ns.cube_luck_value_scale) == (0.5, 1.4, 1.2, 2.0)
    assert ap.parse_args("--net ckpt.pt --positions opening --cube --cube-luck".split()).cube_luck_scale == "fit"
    assert ap.parse_args("--net random --positions opening --cube --cube-net c.pt --cube-luck --cube-luck-net v.pt"
                         .split()).cube_luck
    base = "--net ckpt.pt --positions opening "
    need = "need --cube-luck"
    for bad, text in (("--cube-luck", "--cube-luck needs --cube"),
                      ("--cube --cube-luck --cube-bearoff 6", "--cube-luck and --cube-bearoff cannot be combined"),
                      ("--cube --cube-luck --cube-truncate 8", "--cube-luck and --cube-truncate cannot be combined"),
                      ("--cube --cube-luck --luck", "cannot be combined"),
                      ("--cube --cube-luck --bearoff 6", "cannot be combined"),
                      ("--cube --cube-luck --bearoff1 15", "cannot be combined"),
                      ("--cube --cube-luck --truncate 8", "cannot be combined"),
                      ("--cube --cube-luck --cube-luck-life 1.5", "--cube-luck-life takes a number in [0, 1]"),
                      ("--cube --cube-luck --cube-luck-life nan", "--cube-luck-life takes a number in [0, 1]"),
                      ("--cube --cube-luck --cube-luck-win-value 0.5", "--cube-luck-win-value takes a number in [1, 3]"),
                      ("--cube --cube-luck --cube-luck-loss-value 3.5", "--cube-luck-loss-value takes a number in [1, 3]"),
                      ("--cube --cube-luck --cube-luck-value-scale nan", "--cube-luck-value-scale must be a number"),
                      ("--cube --cube-luck --cube-luck-scale best", "--cube-luck-scale takes 'fit' or a number"),
                      ("--cube --cube-luck --cube-luck-scale inf", "--cube-luck-scale must be finite"),
                      ("--cube --cube-luck-scale 1.0", need), ("--cube --cube-luck-life 0.5", need),
                      ("--cube --cube-luck-win-value 1.5", need), ("--cube --cube-luck-loss-value 1.5", need),
                      ("--cube --cube-luck-value-scale 2", need), ("--cube --cube-luck-net v.pt", need),
                      ("--cube-luck-life 0.5", need)):
        assert text in messages(ap, base + bad, capsys), bad
    assert "--cube-luck needs --net with weights or --cube-luck-net" in messages(
        ap, "--net random --positions opening --cube --cube-net c.pt --cube-luck", capsys)
    # what existed stays refused, with its text
    assert "--cube and --luck cannot be combined" in messages(ap, base + "--cube --luck", capsys)
    assert "--luck-scale takes 'fit' or a number" in messages(ap, base + "--luck --luck-scale best", capsys)
    assert "--truncate and --cube cannot be combined" in messages(ap, base + "--truncate 8 --cube", capsys)


# ------------------------------------------------------------------------- the C ABI --
NEW_ENTRIES = (("bgx_roll_values", 8), ("bgx_cube_roll_luck", 12), ("bgx_rollout_cube_luck_add", 10),
               ("bgx_rollout_cube_luck_pass", 12), ("bgx_rollout_cube_luck_flush", 13))


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):
            want = (_lib._P if "*" in p else ctypes.c_float if p.startswith("float") else
                    _lib.BgxCubeLife if p.startswith("bgx_cube_life") else
                    _lib.BgxCubeRule if p.startswith("bgx_cube_rule") else _lib._I32)
            assert a is want, (name, p)
            assert "*" in p or p.startswith(("float ", "int32_t ", "bgx_cube_life ", "bgx_cube_rule ")), (name, p)
    # bgx_roll_values is bgx_roll_luck with one output for two
    luck, values = _lib.SIGNATURES["bgx_roll_luck"][1], _lib.SIGNATURES["bgx_roll_values"][1]
    assert values == luck[:5] + luck[6:]
    enum = re.search(r"enum bgx_rollout_cube_luck_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ROLLOUT_(CUBE_\w+)\s*=\s*(\d+)", enum)
    assert [(n.lower(), int(v)) for n, v in names] == [(f, i) for i, f in enumerate(T.CUBE_LUCK_FIELDS)]
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_cube_trunc.h"') < src.index('#include "bg_cube_luck.h"')
    hdr = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_cube_luck.h")).read()
    assert "BGX_CUBE_LUCK_PART1_ONLY" in hdr and "2^20 games" in hdr
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in NEW_ENTRIES:
        assert name in integration, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name, _ in NEW_ENTRIES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def test_luck_host_program(tmp_path):
    """tools/cube_luck_host.cpp with AddressSanitizer + UBSan, a program of its own: cube_roll_luck and
    cube_luck_q over every cube byte, both movers, caps 0, 1, 6 and 10, Jacoby on and off and three
    (x, W, L).  A case's 21 values rotate through the list below: each breakpoint of the opponent's
    view (TP, CP, the Jacoby form's 0.2 and 0.8, the ends, as the mover's cubeless values) with its
    fp32 neighbours, the clamps, zeros, NaN and infinities.  The rolls rotate through all 21, both
    orders, and bytes that are no roll.  Bit for bit cube_roll_luck_reference and replay.cube_luck_q."""
    exe = str(tmp_path / "cube_luck_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cube_luck_host.cpp"), "-o", exe], check=True)
    up, down = lambda v: F(np.nextafter(F(v), F(np.inf))), lambda v: F(np.nextafter(F(v), F(-np.inf)))
    lives = [(0.68, 1.0, 1.0), (1.0, 1.3, 1.2), (0.0, 3.0, 3.0)]
    caps, scale = (0, 1, 6, 10), 1.0

    def values_for(W, L):
        vals = [F(0.0), F(-0.0), up(0.0), F(0.37), F(-0.61), F(100.0), F(-1e30), F(math.nan), F(math.inf), F(-math.inf)]
        D = W + L + 0.5
        for p in ((L - 0.5) / D, (L + 1.0) / D, 0.2, 0.8, 0.0, 1.0, 0.5):
            e = F(-(p * (W + L) - L))                       # the mover's value where the opponent sits at p
            vals += [e, up(e), down(e)]
        return np.array(vals, F)

    rolls = ROLLS21 + [(b, a) for a, b in ROLLS21] + [(0, 0), (0, 4), (7, 2), (3, 255)]
    sums = [F(v) for v in (0.0, 0.5, -2.5, 1.5 / ONE, 2.5 / ONE, 32768.0, 40000.0, -1e30, math.inf, -math.inf, math.nan,
                           3e38, 0.1234567, -31.75)]
    rows = []                                                # (byte, cap, mover, jacoby, life index, roll, sum, values)
    for n, (byte, mover, cap, jac, li) in enumerate(itertools.product(range(256), (0, 1), caps, (0, 1), range(len(lives)))):
        vals = values_for(*lives[li][1:])
        v = vals[(n * 21 + 5 * np.arange(21)) % len(vals)]
        rows.append((byte, cap, mover, jac, li, rolls[n % len(rolls)], sums[n % len(sums)], v))
    cases = [f"{b} {cap} {m} {j} {r[0]} {r[1]} {bits(scale)} " + " ".join(bits(F(q)) for q in lives[li]) + f" {bits(s)} "
             + " ".join(bits(x) for x in v) for b, cap, m, j, li, r, s, v in rows]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr and len(cases) == 256 * 2 * 4 * 2 * 3
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(rows)
    arr = np.array([(b, cap, m, j, li, r[0], r[1]) for b, cap, m, j, li, r, _, _ in rows], np.int64)
    vals = np.stack([r[7] for r in rows])
    lq = RP.cube_luck_q(np.array([r[6] for r in rows], F))
    nonzero = 0
    for cap, jac, li in itertools.product(caps, (0, 1), range(len(lives))):
        idx = np.nonzero((arr[:, 1] == cap) & (arr[:, 3] == jac) & (arr[:, 4] == li))[0]
        luck, mean = C.cube_roll_luck_reference(vals[idx], arr[idx, 0].astype(np.uint8), arr[idx, 2], arr[idx, 5:7], scale,
                                                C.CubeLife(*lives[li]), cap, bool(jac))
        want = [[bits(luck[i]), bits(mean[i]), str(int(lq[j]))] for i, j in enumerate(idx)]
        bad = [(cases[j], got[j], w) for j, w in zip(idx, want) if got[j] != w]
        assert not bad, bad[:3]
        nonzero += int((luck != 0).sum())
    assert nonzero > len(rows) // 2
    # an out-of-range case is refused, not computed
    r = subprocess.run([exe], input="0 11 0 0 1 1 " + " ".join(["0"] * 26) + "\n", capture_output=True, text=True)
    assert r.returncode == 2
