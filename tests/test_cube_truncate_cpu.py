"""Truncated cubeful rollouts' host side (bgx/cube.py, bgx/rollout.py; no GPU):
janowski_reference on hand values and on the rule's structural properties in fp32 and fp64,
janowski_points against the closed forms, summarize_cube_truncated against numpy,
cube_trunc_reference on a hand-made trace, the new mode's refusals beside the unchanged old ones,
the command line, the C ABI's declarations, and part 1 of csrc/bg_cube_trunc.h built as a host
program (tools/cube_trunc_host.cpp)."""
import ctypes
import importlib.util
import itertools
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from bgx import _lib, cube as C, rollout as R
from bgx.truncate import Truncation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = 65536
LIVES = [(1.0, 1.0), (1.3, 1.2), (3.0, 3.0), (1.0, 3.0), (3.0, 1.0)]
XS = (0.0, 0.5, 0.68, 1.0)
GRID = np.linspace(0.0, 1.0, 2001)
CEN, OWN0, OPP0 = 0, C.pack(1, 1), C.pack(1, 2)            # as mover 0 sees them


def rule(**kw):
    return C.CubeRule(lambda eng, dsel: None, **kw)


def ctrunc(plies=2, **kw):
    return C.CubeTruncation(lambda eng, tsel: None, plies, **kw)


def ref(c, byte, life, cap=6, jacoby=False, mover=0, scale=1.0):
    c = np.atleast_1d(np.asarray(c, F))
    return C.janowski_reference(c, np.full(c.shape, byte, np.uint8), np.full(c.shape, mover), scale, life, cap, jacoby)


# ------------------------------------------------------------------------------ the rule --
def test_hand_values_live_cube():
    life = C.CubeLife(1.0)
    assert float(F(F(0.5) / F(2.5))) == float(F(0.2)) and float(F(F(2.0) / F(2.5))) == float(F(0.8))       # TP, CP
    p08 = F(F(0.8) * F(2) - F(1))                          # c with p = 0.8f up to the last bit
    v, fl = ref([0.0], CEN, life)
    assert v[0, 0] == 0.0 and v[0, 3] == 0.0               # E_cen(0.5) = 0
    v, fl = ref([p08], OWN0, life)
    assert v[0, 0] == pytest.approx(1.0, abs=4e-7)         # E_own(0.8) = 1
    assert v[0, 1] == pytest.approx(1.0, abs=8e-7)         # 2 E_opp(0.8) = 1
    v, fl = ref([-p08], OPP0, life)
    assert v[0, 0] == pytest.approx(-1.0, abs=4e-7)        # E_opp(0.2) = -1
    assert fl[0] & 1 == 0 and v[0, 2] == v[0, 0]           # no access: e = nd
    # c = 0.75: p = 0.875, dt = 2 E_opp = 2 (0.5 + 0.075 * 2.5) = 1.375: a pass; cashing beats nd = 1
    v, fl = ref([0.75], CEN, life)
    assert v[0, 1] == pytest.approx(1.375, abs=1e-6) and v[0, 0] == pytest.approx(1.0, abs=4e-7)
    assert fl[0] & 4 == 0 and v[0, 2] == max(v[0, 0], 1.0)
    # at p = 1 everything is W, dt = 2: a pass, and nd = 1 ties the cash: no double
    v, fl = ref([1.0], CEN, life)
    assert v[0].tolist() == [1.0, 2.0, 1.0, 1.0] and fl[0] == 1
    # p = 0.75: dt = 2 (-1 + 0.55 * 2.5) = 0.75, a take; e and the double flag follow from nd and dt
    v, fl = ref([0.5], CEN, life)
    assert v[0, 1] == pytest.approx(2 * (-1 + 0.55 * 2.5), abs=1e-6) and fl[0] & 4
    assert bool(fl[0] & 2) == bool(min(v[0, 1], 1.0) > v[0, 0])
    assert v[0, 2] == (min(v[0, 1], F(1)) if fl[0] & 2 else v[0, 0])


@pytest.mark.parametrize("W,L", LIVES)
def test_dead_cube_life_is_the_cubeless_equity(W, L):
    life = C.CubeLife(0.0, W, L)
    c = (GRID * (W + L) - L).astype(F)
    for byte, mover in ((CEN, 0), (OWN0, 0), (OPP0, 0), (OWN0, 1), (C.pack(3, 2), 1)):
        v, fl = ref(c, byte, life, mover=mover)
        cl = np.clip(c, F(-L), F(W))
        assert np.array_equal(v[:, 0], cl) and np.array_equal(v[:, 3], cl)
        assert np.array_equal(v[:, 1], (F(2) * cl).astype(F))


@pytest.mark.parametrize("W,L", LIVES)
@pytest.mark.parametrize("x", XS)
def test_structure_fp64(W, L, x):
    life = C.CubeLife(x, W, L)
    D = W + L + 0.5
    TP, CP = (L - 0.5) / D, (L + 1.0) / D
    assert 0 < TP < CP < 1
    c, cen, own, opp = C.janowski_equities(GRID, life)
    for e in (cen, own, opp):
        assert np.all(np.diff(e) >= -1e-12)                          # non-decreasing
        assert np.all(np.abs(np.diff(e)) <= 9.0 * (GRID[1] - GRID[0]) + 1e-12)       # no jump: every slope is below 9
        assert e.min() >= -L - 1e-12 and e.max() <= W + 1e-12
    assert np.all(opp <= cen + 1e-12) and np.all(cen <= own + 1e-12)
    for b in (TP, CP):                                               # continuous at the breakpoints
        sides = C.janowski_equities(np.array([b - 1e-10, b + 1e-10]), life)[1:]
        assert all(abs(e[1] - e[0]) < 1e-8 for e in sides)
    if W == L:
        assert np.allclose(cen, -cen[::-1], atol=1e-12) and np.allclose(own, -opp[::-1], atol=1e-12)
    assert np.allclose(c, GRID * (W + L) - L)


@pytest.mark.parametrize("W,L", LIVES)
@pytest.mark.parametrize("x", XS)
def test_structure_fp32_and_against_fp64(W, L, x):
    """The float32 rule keeps the properties up to a few ulp of 3 (2.4e-7 each), through slopes
    below 9 on a p that is itself rounded."""
    tol = 16 * 3 * 2.0 ** -24
    life = C.CubeLife(x, W, L)
    c32 = (GRID * (W + L) - L).astype(F)
    p64 = (c32.astype(np.float64) + L) / (W + L)
    _, cen64, own64, opp64 = C.janowski_equities(np.clip(p64, 0.0, 1.0), C.CubeLife(float(F(x)), float(F(W)), float(F(L))))
    cen, own, opp = (ref(c32, b, life)[0][:, 0] for b in (CEN, OWN0, OPP0))
    for e, e64 in ((cen, cen64), (own, own64), (opp, opp64)):
        assert e.dtype == F and np.abs(e - e64).max() <= tol
        assert np.all(np.diff(e.astype(np.float64)) >= -tol)
        assert e.min() >= -L - tol and e.max() <= W + tol
    assert np.all(opp <= cen + tol) and np.all(cen <= own + tol)
    if W == L:
        assert np.abs(cen + cen[::-1]).max() <= tol and np.abs(own + opp[::-1]).max() <= tol
    # the mover's view: PLAYER2 on roll sees owner 2 as its own
    assert np.array_equal(ref(c32, OPP0, life, mover=1)[0], ref(c32, OWN0, life, mover=0)[0])
    # dt and e, flags
    v, fl = ref(c32, CEN, life)
    assert np.array_equal(v[:, 1], (F(2) * opp).astype(F))
    cash = np.minimum(v[:, 1], F(1))
    assert np.array_equal(fl & 2 != 0, cash > v[:, 0]) and np.array_equal(fl & 4 != 0, v[:, 1] <= 1)
    assert np.array_equal(v[:, 2], np.where(cash > v[:, 0], cash, v[:, 0])) and np.all(fl & 1 == 1) and np.all(fl & 8 == 0)


def test_dead_state_last_double_and_jacoby():
    life = C.CubeLife(0.68, 1.5, 1.25)
    c = np.linspace(-1.25, 1.5, 111).astype(F)
    # dead: k >= cap, whoever owns it; also cap 0
    for byte, cap in ((C.pack(3, 1), 3), (C.pack(5, 2), 3), (CEN, 0), (C.pack(15, 3), 10)):
        v, fl = ref(c, byte, life, cap=cap)
        assert np.array_equal(v[:, 0], c) and np.array_equal(v[:, 2], c) and np.array_equal(v[:, 3], c)
        assert np.array_equal(v[:, 1], (F(2) * c).astype(F))
        assert np.array_equal(fl, np.where(v[:, 1] <= 1, 12, 8))
    # k + 1 = cap: the doubled cube is dead, dt = 2 c; nd is still the live form
    v, fl = ref(c, OWN0, life, cap=2)
    assert np.array_equal(v[:, 1], (F(2) * c).astype(F))
    assert np.array_equal(v[:, 0], ref(c, OWN0, life, cap=6)[0][:, 0]) and np.all(fl & 1 == 1)
    # Jacoby: only the centred nd changes, formed with W = L = 1 on the same p
    vj, flj = ref(c, CEN, life, jacoby=True)
    v0, _ = ref(c, CEN, life)
    p = (c.astype(np.float64) + 1.25) / 2.75
    want = C.janowski_equities(p, C.CubeLife(float(F(0.68))))[1]
    assert np.abs(vj[:, 0] - want).max() < 2e-6 and not np.array_equal(vj[:, 0], v0[:, 0])
    assert np.array_equal(vj[:, 1], v0[:, 1]) and np.array_equal(vj[:, 3], v0[:, 3])
    assert np.array_equal(C.janowski_equities(p, C.CubeLife(0.68, 1.5, 1.25), jacoby=True)[1],
                          C.janowski_equities(p, C.CubeLife(0.68))[1])
    for byte in (OWN0, OPP0, C.pack(6, 1)):
        assert np.array_equal(ref(c, byte, life, jacoby=True)[0], ref(c, byte, life)[0])
    # owner 3 reads as centred, k above the cap as the cap
    assert np.array_equal(ref(c, C.pack(0, 3), life)[0], v0)
    assert np.array_equal(ref(c, C.pack(9, 1), life, cap=4)[0], ref(c, C.pack(4, 1), life, cap=4)[0])


def test_values_that_are_no_equity():
    life = C.CubeLife(0.5, 2.0, 1.5)
    v, fl = ref([math.nan, math.inf, -math.inf, 100.0, -100.0, 2.0, -1.5], CEN, life)
    assert v[:, 3].tolist() == [0.0, 2.0, -1.5, 2.0, -1.5, 2.0, -1.5]
    assert not np.isnan(v).any()
    assert v[1].tolist() == [2.0, 4.0, 2.0, 2.0] and v[2].tolist() == [-1.5, -3.0, -1.5, -1.5]
    # the scale is one fp32 product before the clamp; a NaN product (0 * inf) counts 0
    v, _ = ref([0.3, math.inf], OWN0, life, scale=0.0)
    assert v[:, 3].tolist() == [0.0, 0.0]
    v, _ = ref([0.3], OWN0, life, scale=-2.0)
    assert v[0, 3] == F(-2.0) * F(0.3)
    for bad in (dict(x=-0.01), dict(x=1.01), dict(x=math.nan), dict(win_value=0.99), dict(win_value=3.01),
                dict(loss_value=math.nan), dict(loss_value=4), dict(x="0.5"), dict(x=True)):
        with pytest.raises(ValueError, match="CubeLife"):
            C.CubeLife(**bad)
    s = C.CubeLife(0.25, 2, 3).struct()
    assert (s.cube_life, s.win_value, s.loss_value) == (0.25, 2.0, 3.0) and ctypes.sizeof(s) == 12


def test_cut_fixed_point():
    e = np.array([0.5, -0.5, 3.0, -3.0, 3.5, math.nan, 1.5 / ONE, 2.5 / ONE, 1e-9], F)
    k = np.array([0, 1, 10, 10, 2, 3, 0, 0, 5])
    same = np.array([1, 1, 1, 0, 1, 1, 1, 0, 1], bool)
    got = C.cube_trunc_fixed_reference(e, same, k)
    assert got.tolist() == [32768, -65536, 3 * ONE << 10, 3 * ONE << 10, 3 * ONE << 2, 0, 2, -2, 0]
    assert int(got[2]) ** 2 < 2 ** 63 and (int(got[2]) ** 2 >> 30) > 0


# ---------------------------------------------------------------------- janowski_points --
@pytest.mark.parametrize("x", XS + (0.25, 0.9))
def test_points_closed_forms(x):
    pt = C.janowski_points(C.CubeLife(x))
    assert pt["p_take"] == pytest.approx((3 + x) / (4 + x), abs=1e-12)
    assert pt["p_double_centred"] == pytest.approx((3 + x) / (6 - x), abs=1e-12)
    assert pt["p_redouble"] == pytest.approx((2 + 2 * x) / (4 + x), abs=1e-12)
    for name in ("take", "double_centred", "redouble"):
        assert pt[name] == pytest.approx(2 * pt["p_" + name] - 1, abs=1e-12)
    assert "too_good" not in pt


def test_points_table_and_gammons():
    table = {0.0: (0.75, 0.5, 0.5), 0.5: (None, 0.6364, 0.6667), 0.68: (0.7863, 0.6917, 0.7179), 1.0: (0.8, 0.8, 0.8)}
    for x, (take, dc, rd) in table.items():
        pt = C.janowski_points(C.CubeLife(x))
        if take is not None:
            assert round(pt["p_take"], 4) == take
        assert (round(pt["p_double_centred"], 4), round(pt["p_redouble"], 4)) == (dc, rd)
    assert C.janowski_points(C.CubeLife(0.0))["take"] == pytest.approx(0.5, abs=1e-12)         # CubeRule's pass_at
    # with gammons: the roots satisfy their equations, in order, and too_good exists
    life = C.CubeLife(0.68, 1.3, 1.2)
    pt = C.janowski_points(life)
    eq = lambda p: [float(v) for v in C.janowski_equities(np.float64(p), life)]
    assert 2 * eq(pt["p_take"])[3] == pytest.approx(1.0, abs=1e-12)
    assert 2 * eq(pt["p_double_centred"])[3] == pytest.approx(eq(pt["p_double_centred"])[1], abs=1e-12)
    assert 2 * eq(pt["p_redouble"])[3] == pytest.approx(eq(pt["p_redouble"])[2], abs=1e-12)
    assert eq(pt["p_too_good"])[1] == pytest.approx(1.0, abs=1e-12)
    assert pt["double_centred"] < pt["redouble"] < pt["take"] < pt["too_good"] < 1.3
    assert pt["take"] == pytest.approx(pt["p_take"] * 2.5 - 1.2, abs=1e-12)
    # live cube, gammons: too good from the cash point on
    assert C.janowski_points(C.CubeLife(1.0, 2.0, 1.0))["p_too_good"] == pytest.approx(2.0 / 3.5, abs=1e-12)


def test_gammon_values():
    s = R.summarize([10, 100, 3, 2, 1, 2, 2, 0])
    assert C.gammon_values(s) == ((3 + 4 + 3) / 6, (2 + 4) / 4)
    assert C.gammon_values(R.summarize([3, 9, 0, 0, 0, 1, 1, 1])) == (1.0, 2.0)
    assert C.gammon_values(R.summarize([0] * 8)) == (1.0, 1.0)
    W, L = C.gammon_values(R.summarize([5, 9, 0, 0, 5, 0, 0, 0]))
    C.CubeLife(0.5, W, L)


# ----------------------------------------------------------------- the summary --
def rows_of(games):
    """games: (kind, y or yq, k, plies, res): kind "end" (y in points; res the cubeless result),
    "pass" (y), "trunc" (yq in 2^-16), "cut" (yq in 2^-20) -> tally, cube, trunc and cut rows."""
    t, c, tr, cu = np.zeros(8, np.int64), np.zeros(8, np.int64), [0] * 6, [0] * 6
    for kind, y, k, plies, res in games:
        if kind in ("end", "pass"):
            c[0] += 1; c[1] += y; c[2] += y * y; c[3] += k
            if kind == "pass":
                c[4] += 1; c[5] += plies; c[6] += y > 0
            else:
                t[0] += 1; t[1] += plies; t[(2 if res > 0 else 5) + abs(res) - 1] += 1
        else:
            row = tr if kind == "trunc" else cu
            for f, v in enumerate((1, plies, y, (y * y) & ((1 << 30) - 1), (y * y) >> 30, k)):
                row[f] += v
    return t, c, tr, cu


GAMES = [("end", 4, 1, 30, 2), ("pass", -1, 0, 9, 0), ("trunc", 20000, 0, 8, 0), ("trunc", -3 * ONE << 10, 10, 8, 0),
         ("end", -8, 2, 60, -2), ("trunc", 123456 << 3, 3, 8, 0), ("pass", 2, 1, 12, 0), ("trunc", -1, 0, 8, 0)]
CUTS = [("cut", (1 << 20) << 10, 10, 17, 0), ("cut", -333333 << 2, 2, 21, 0), ("cut", 5, 0, 3, 0)]


def points(games):
    return np.array([g[1] / ONE if g[0] == "trunc" else g[1] / (1 << 20) if g[0] == "cut" else g[1] for g in games],
                    np.float64)


def test_summarize_cube_truncated_against_numpy():
    t, c, tr, _ = rows_of(GAMES)
    c[7] = 11
    assert tr[4] > 0                                        # a Y2 sum that needs the HI part
    r = C.summarize_cube_truncated(t, c, tr, unfinished=2)
    y = points(GAMES)
    assert (r["games"], r["truncated_games"], r["unfinished"], r["cube_games"]) == (8, 4, 2, 4)
    assert r["equity_cubeful"] == pytest.approx(y.mean(), rel=1e-14)
    assert r["equity_cubeful_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(8), rel=1e-12)
    assert r["truncated_share"] == 0.5 and r["pass_share"] == 0.25 and r["doubles_per_game"] == 11 / 8
    assert r["truncated_equity_cubeful"] == pytest.approx(y[[2, 3, 5, 7]].mean(), rel=1e-14)
    assert r["mean_cube_log2"] == pytest.approx((1 + 0 + 0 + 10 + 2 + 3 + 1 + 0) / 8)
    assert r["plies_per_game"] == pytest.approx((30 + 9 + 8 + 8 + 60 + 8 + 12 + 8) / 8)
    assert [r[f] for f in C.CUBE_TRUNC_FIELDS] == tr and [r[f] for f in C.CUBE_FIELDS] == c.tolist()
    assert r["played_out"] == R.summarize(t, 2) and "cut_share" not in r
    # no truncated game: summarize_cube's numbers
    z = [0] * 6
    r0, rc = C.summarize_cube_truncated(t, c, z), C.summarize_cube(t, c)
    for f in ("games", "equity_cubeful", "equity_cubeful_stderr", "pass_share", "mean_cube_log2", "plies_per_game"):
        assert r0[f] == pytest.approx(rc[f], rel=1e-15), f
    assert r0["truncated_share"] == 0.0 and r0["truncated_equity_cubeful"] == 0.0


def test_summarize_cube_truncated_with_cut_row():
    games = GAMES + CUTS
    t, c, tr, cu = rows_of(games)
    assert cu[4] > 0
    r = C.summarize_cube_truncated(t, c, tr, 1, cut_row=cu)
    y = points(games)
    assert (r["games"], r["truncated_games"], r["cut_games"], r["unfinished"]) == (11, 4, 3, 1)
    assert r["equity_cubeful"] == pytest.approx(y.mean(), rel=1e-14)
    assert r["equity_cubeful_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(11), rel=1e-12)
    assert r["cut_share"] == 3 / 11 and r["truncated_share"] == 4 / 11
    assert r["mean_cube_log2"] == pytest.approx((17 + 12) / 11) and r["plies_per_game"] == pytest.approx((143 + 41) / 11)
    assert [r[f] for f in C.CUBE_CUT_FIELDS] == cu
    # without truncated games it is summarize_cube_bearoff
    rb, r0 = C.summarize_cube_bearoff(t, c, cu), C.summarize_cube_truncated(t, c, [0] * 6, cut_row=cu)
    for f in ("games", "equity_cubeful", "equity_cubeful_stderr", "cut_share", "mean_cube_log2", "plies_per_game"):
        assert r0[f] == pytest.approx(rb[f], rel=1e-15), f


def test_summarize_cube_truncated_small_and_mismatch():
    z8, z6 = np.zeros(8, np.int64), [0] * 6
    for kw in ({}, dict(cut_row=z6)):
        r = C.summarize_cube_truncated(z8, z8, z6, **kw)
        assert r["games"] == 0 and r["equity_cubeful"] == 0.0 and r["equity_cubeful_stderr"] == 0.0
        assert r["truncated_share"] == 0.0 and r["plies_per_game"] == 0.0
    t, c, tr, cu = rows_of([("trunc", -98304 << 1, 1, 8, 0)])
    r = C.summarize_cube_truncated(t, c, tr)
    assert r["games"] == 1 and r["equity_cubeful"] == -3.0 and r["equity_cubeful_stderr"] == 0.0
    # equal results of every kind: exactly their value, standard error 0
    t, c, tr, cu = rows_of([("end", 2, 1, 5, 1), ("trunc", 2 * ONE, 1, 8, 0), ("cut", 2 << 20, 1, 3, 0), ("pass", 2, 1, 4, 0)])
    r = C.summarize_cube_truncated(t, c, tr, cut_row=cu)
    assert r["games"] == 4 and r["equity_cubeful"] == 2.0 and r["equity_cubeful_stderr"] == 0.0
    c[0] += 1
    with pytest.raises(ValueError, match="counts 3 games"):
        C.summarize_cube_truncated(t, c, tr)
    c[0] -= 1
    with pytest.raises(ValueError, match="6 entries"):
        C.summarize_cube_truncated(t, c, tr[:5])
    with pytest.raises(ValueError, match="6 entries"):
        C.summarize_cube_truncated(t, c, tr, cut_row=cu + [0])


# ------------------------------------------------------------ cube_trunc_reference --
def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def test_cube_trunc_reference_hand_made_trace():
    """Four lanes, four steps, horizon 2, cap 3, x = 0.5, W = L = 1.  Lane 0 (two games): its first
    game ends by a passed double at step 1, its second is doubled and taken at step 2 and
    truncated after that step with PLAYER2 on roll owning the cube at 2 -- the lane's last game.
    Lane 1 (cube 2 owned by PLAYER2, who starts): truncated after step 1 with PLAYER2 on roll and
    after step 3 with PLAYER1 on roll, both with a NaN value, which counts as c = 0.  Lane 2 (two
    games): wins a gammon at step 1, then is truncated after step 3 with +inf, clamped to W.  Lane
    3 is idle."""
    nan, inf = float("nan"), float("inf")
    ru = rule(double_at=0.4, pass_at=0.5, cap=3)
    tc = ctrunc(2, life=C.CubeLife(0.5))
    group = np.array([0, 1, 1, -1], np.int32)
    starts = np.zeros((4, 64), np.uint8)
    starts[1, 52] = 1
    cube0 = np.array([0, C.pack(1, 2), 0, 0], np.uint8)
    mover = np.array([[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 0, 0]], np.uint8).T
    eq = np.array([[0.9, 0.9, 0.45, 0.9], [0.9, 0.9, 0.9, 0.9], [0.0] * 4, [0.9] * 4], F).T
    done, inf_ = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int32)
    done[1, 2], inf_[1, 2] = 1, info(0, 2)
    tval = np.full((4, 4), nan, F)
    tmover = np.zeros((4, 4), np.uint8)
    tval[2, 0], tmover[2, 0] = 0.25, 1
    tval[1, 1], tmover[1, 1] = nan, 1
    tval[3, 2], tmover[3, 2] = inf, 0
    tr = dict(cube_mover=mover, cube_equity=eq, done=done, info=inf_, ctrunc_value=tval, ctrunc_mover=tmover)
    out = C.cube_trunc_reference(tr, starts, group, 2, 2, ru, tc, cube0)
    # lane 0's truncated game: p = 0.625, own: 0.5 * 0.25 + 0.5 * 0.5625 = 0.40625 > min(dt, 1) = 0.3125
    v0, f0 = C.janowski_reference([0.25], [C.pack(1, 2)], [1], 1.0, tc.life, 3)
    assert v0[0, 2] == pytest.approx(0.40625, abs=1e-6) and v0[0, 1] == pytest.approx(0.3125, abs=1e-6) and f0[0] == 5
    y0 = -int(np.rint(F(v0[0, 2] * F(ONE)))) * 2
    assert abs(y0 + 53248) <= 2
    # lane 1: c = 0, k = 1.  PLAYER2, the start mover, sees its own cube: 0.5 * 0.25 = 0.125; PLAYER1
    # sees the opponent's: -0.125, which is +0.125 for the start mover.  Lane 2: e = W = 1.
    v1, f1 = C.janowski_reference([nan, nan], [C.pack(1, 2)] * 2, [1, 0], 1.0, tc.life, 3)
    assert v1[:, 2].tolist() == [0.125, -0.125] and f1.tolist() == [5, 4]
    ys = [[y0], [16384, 16384, ONE]]
    lo, hi = lambda v: (v * v) & (2 ** 30 - 1), lambda v: (v * v) >> 30
    assert out["cube_trunc_tally"].tolist() == [[1, 2, y0, lo(y0), hi(y0), 1],
                                                [3, 6, sum(ys[1]), sum(map(lo, ys[1])), sum(map(hi, ys[1])), 2]]
    assert hi(y0) == 2 and hi(ONE) == 4
    assert out["cube_tally"].tolist() == [[1, -1, 1, 0, 1, 1, 0, 2], [1, 2, 4, 0, 0, 0, 0, 0]]
    assert out["tally"].tolist() == [[0] * 8, [1, 2, 0, 1, 0, 0, 0, 0]]
    assert out["games_done"].tolist() == [2, 2, 2, 0] and out["active"] == 0
    assert np.argwhere(out["ctrunc"]).tolist() == [[1, 1], [2, 0], [3, 1], [3, 2]]
    assert np.argwhere(out["mask"]).tolist() == [[1, 0]]
    assert out["ctrunc_cube"][2, 0] == C.pack(1, 2) and out["ctrunc_cube"][1, 1] == C.pack(1, 2)
    assert out["cube"][:, 0].tolist() == [0, 0, 0, 0]        # before each decision: the start cube came back
    for p in range(2):
        r = C.summarize_cube_truncated(out["tally"][p], out["cube_tally"][p], out["cube_trunc_tally"][p])
        assert r["games"] == (2, 4)[p]
    # a longer horizon: nothing is truncated and the replay is cube_reference's
    far = C.cube_trunc_reference(tr, starts, group, 2, 2, ru, ctrunc(9), cube0)
    plain = C.cube_reference(tr, starts, group, 2, 2, ru, cube0)
    assert not far["ctrunc"].any() and not far["cube_trunc_tally"].any()
    assert np.array_equal(far["cube_tally"], plain["cube_tally"]) and np.array_equal(far["tally"], plain["tally"])
    assert "cube_trunc_tally" not in plain


def test_cube_truncation_arguments():
    t = ctrunc(8, scale=2.0, lookahead=1)
    assert isinstance(t, Truncation) and (t.plies, t.scale, t.lookahead) == (8, 2.0, 1)
    assert (t.life.x, t.life.win_value, t.life.loss_value) == (0.68, 1.0, 1.0) and not t.sync_free
    assert ctrunc(1, life=C.CubeLife(0.1, 2.0, 3.0)).life.loss_value == 3.0
    for bad in (dict(plies=0), dict(plies=2, life=0.5), dict(plies=2, scale=math.nan), dict(plies=2, lookahead=2)):
        with pytest.raises(ValueError):
            ctrunc(**bad)
    with pytest.raises(ValueError, match="value must be"):
        C.CubeTruncation(3.0, 8)


# ------------------------------------------------------------------------- the modes --
def _old_table():
    spec = importlib.util.spec_from_file_location("_modes_table", os.path.join(ROOT, "tests", "test_rollout_modes_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


OLD = _old_table()


@pytest.mark.parametrize("modes", sorted(OLD.EXPECTED))
def test_existing_combinations_keep_their_first_message(modes):
    """All 32 combinations of today's modes, cube_truncate=None given explicitly: the messages of
    tests/test_rollout_modes_cpu.py's table."""
    kw = {n: OLD.well_typed()[n] for n in modes}
    ro = object.__new__(R.Rollout)
    plain, with_cube0 = OLD.EXPECTED[modes]
    assert OLD.first_message(R.Rollout.run, ro, None, None, 36, cube_truncate=None, **kw) == OLD.prefixed("run", plain)
    assert OLD.first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, cube_truncate=None, **kw) \
        == OLD.prefixed("run_lanes", plain)
    assert OLD.first_message(R._check_modes, "run_lanes", cube0=object(), types=True, cube_truncate=None, **kw) \
        == OLD.prefixed("run_lanes", with_cube0)


NEW = {
    (): "cube_truncate without cube",
    ("luck",): "cube_truncate without cube",
    ("truncate",): "cube_truncate without cube",
    ("cube_bearoff",): "cube_truncate without cube",
    ("cube",): OLD.OK,
    ("cube", "cube_bearoff"): OLD.OK,
    ("cube", "luck"): "cube_truncate together with luck is not supported",
    ("cube", "bearoff"): "cube_truncate together with bearoff is not supported",
    ("cube", "truncate"): "cube_truncate together with truncate is not supported",
    ("cube", "luck", "bearoff", "truncate"): "cube_truncate together with luck is not supported",
    ("cube", "cube_bearoff", "luck"): "cube_truncate together with luck is not supported",
    ("cube", "cube_bearoff", "truncate"): "cube_truncate together with truncate is not supported",
}


@pytest.mark.parametrize("modes", sorted(NEW))
def test_new_mode_refusals(modes):
    kw = {n: OLD.well_typed()[n] for n in modes}
    kw["cube_truncate"] = ctrunc(8)
    ro = object.__new__(R.Rollout)
    assert OLD.first_message(R.Rollout.run, ro, None, None, 36, **kw) == OLD.prefixed("run", NEW[modes])
    assert OLD.first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, **kw) == OLD.prefixed("run_lanes", NEW[modes])
    assert OLD.first_message(R._check_modes, "run", **kw) == OLD.prefixed("run", NEW[modes])


def test_new_mode_type_check_and_cube0():
    ro = object.__new__(R.Rollout)
    for wrong in (8, Truncation(lambda eng, tsel: None, 8), object()):
        assert OLD.first_message(R.Rollout.run_lanes, ro, None, None, None, 1, 1, cube=object(), cube_truncate=wrong) \
            == "run_lanes: cube_truncate must be a cube.CubeTruncation"
    assert OLD.first_message(R._check_modes, "run", cube=object(), cube_truncate=8) == OLD.OK          # run leaves it to the lanes
    assert OLD.first_message(R._check_modes, "run_lanes", cube0=object(), types=True, cube_truncate=ctrunc(8)) \
        == "run_lanes: cube_truncate without cube"
    assert OLD.first_message(R._check_modes, "run_lanes", cube=object(), cube0=object(), types=True,
                             cube_truncate=ctrunc(8)) == OLD.OK
    # the wrong type comes after the refusals, as cube_bearoff's does
    assert OLD.first_message(R._check_modes, "run_lanes", cube=object(), luck=object(), types=True, cube_truncate=8) \
        == "run_lanes: cube_truncate together with luck is not supported"


# --------------------------------------------------------------------------- the parser --
def test_parser_flags():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.cube_truncate is None and ns.cube_truncate_net is None
    assert (ns.cube_life, ns.cube_win_value, ns.cube_loss_value, ns.cube_truncate_scale, ns.cube_truncate_lookahead) \
        == (0.68, 1.0, 1.0, 1.0, 0)
    ns = ap.parse_args("--net ckpt.pt --positions opening --cube --cube-truncate 8 --cube-life 0.5 --cube-win-value 1.4 "
                       "--cube-loss-value 1.2 --cube-truncate-lookahead 1 --cube-truncate-scale 2 --cube-truncate-net v.pt "
                       "--cube-decision --cube-bearoff 6".split())
    assert (ns.cube_truncate, ns.cube_life, ns.cube_win_value, ns.cube_loss_value) == (8, 0.5, 1.4, 1.2)
    assert (ns.cube_truncate_lookahead, ns.cube_truncate_scale, ns.cube_truncate_net) == (1, 2.0, "v.pt")
    assert ap.parse_args("--net random --positions opening --cube --cube-net c.pt --cube-truncate 1".split()).cube_truncate == 1
    base = "--net ckpt.pt --positions opening "
    for bad in ("--cube-truncate 8", "--cube --cube-truncate 0", "--cube --cube-truncate -3",
                "--cube --cube-truncate 8 --luck", "--cube --cube-truncate 8 --bearoff 6",
                "--cube --cube-truncate 8 --bearoff1 15", "--cube --cube-truncate 8 --truncate 8",
                "--cube-truncate 8 --truncate 8", "--cube --cube-truncate 8 --cube-life 1.5",
                "--cube --cube-truncate 8 --cube-life nan", "--cube --cube-truncate 8 --cube-win-value 0.5",
                "--cube --cube-truncate 8 --cube-loss-value 3.5", "--cube --cube-truncate 8 --cube-truncate-scale nan",
                "--cube --cube-truncate 8 --cube-truncate-lookahead 2", "--cube --cube-life 0.5",
                "--cube --cube-win-value 1.5", "--cube --cube-loss-value 1.5", "--cube --cube-truncate-net v.pt",
                "--cube --cube-truncate-lookahead 1", "--cube --cube-truncate-scale 2", "--cube-life 0.5"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + bad).split())
    # what existed stays refused
    for bad in ("--truncate 8 --cube", "--cube --luck"):
        with pytest.raises(SystemExit):
            ap.parse_args((base + bad).split())


# ------------------------------------------------------------------------- the C ABI --
def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in (("bgx_cube_janowski", 12), ("bgx_rollout_cube_trunc_cut", 21)):
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):
            want = (_lib._P if "*" in p else ctypes.c_float if p.startswith("float") else
                    _lib.BgxCubeLife if p.startswith("bgx_cube_life") else _lib._I32)
            assert a is want and ("*" in p or p.startswith(("float ", "int32_t ", "bgx_cube_life "))), (name, p)
    m = re.search(r"typedef struct \{([^}]*)\} bgx_cube_life;", header)
    fields = re.findall(r"(float)\s+(\w+);", m.group(1))
    assert [(n, ctypes.c_float) for _, n in fields] == list(_lib.BgxCubeLife._fields_) and len(fields) == 3
    enum = re.search(r"enum bgx_rollout_cube_trunc_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ROLLOUT_(CUBE_TRUNC_\w+)\s*=\s*(\d+)", enum)
    assert [(n.lower(), int(v)) for n, v in names] == [(f, i) for i, f in enumerate(C.CUBE_TRUNC_FIELDS)]
    assert C.CUBE_TRUNC_ONE == ONE
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_trunc.h"') < src.index('#include "bg_cube_trunc.h"')
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bgx_cube_janowski", "bgx_rollout_cube_trunc_cut"):
        assert name in integration, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, "bgx_cube_janowski") and hasattr(lib, "bgx_rollout_cube_trunc_cut")


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def test_rule_host_program(tmp_path):
    """tools/cube_trunc_host.cpp with AddressSanitizer + UBSan, a program of its own:
    cube_trunc_values and cube_trunc_q over every cube byte, both movers, caps 0, 1, 6 and 10,
    Jacoby on and off and four (x, W, L), with values that rotate through the list below; then
    every state's bytes with every value: each breakpoint (TP, CP and the Jacoby form's 0.2 and
    0.8, as cubeless equities) with its fp32 neighbours, the clamps, zeros, NaN and infinities.
    Bit for bit janowski_reference and cube_trunc_fixed_reference."""
    exe = str(tmp_path / "cube_trunc_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cube_trunc_host.cpp"), "-o", exe], check=True)
    up, down = lambda v: F(np.nextafter(F(v), F(np.inf))), lambda v: F(np.nextafter(F(v), F(-np.inf)))
    lives = [(0.68, 1.0, 1.0), (1.0, 1.3, 1.2), (0.0, 3.0, 3.0), (0.5, 1.0, 3.0)]
    caps, scale = (0, 1, 6, 10), 1.0

    def values_for(W, L):
        vals = [F(0.0), F(-0.0), up(0.0), F(0.37), F(-0.61), F(100.0), F(-1e30), F(math.nan), F(math.inf), F(-math.inf)]
        D = W + L + 0.5
        for p in ((L - 0.5) / D, (L + 1.0) / D, 0.2, 0.8, 0.0, 1.0, 0.5):
            e = F(p * (W + L) - L)
            vals += [e, up(e), down(e)]
        return np.array(vals, F)

    rows = []                                                # (byte, cap, mover, start, jacoby, life index, value)
    n = 0
    for byte, mover, cap, jac, li in itertools.product(range(256), (0, 1), caps, (0, 1), range(len(lives))):
        vals = values_for(*lives[li][1:])
        for j in range(3):
            rows.append((byte, cap, mover, n & 1, jac, li, vals[(n * 3 + j) % len(vals)]))
        n += 1
    states = [0] + [C.pack(k, o) for k in (0, 1, 5, 6, 9, 10) for o in (1, 2)] + [C.pack(2, 3), 255]
    for byte, mover, cap, jac, li in itertools.product(states, (0, 1), caps, (0, 1), range(len(lives))):
        for v in values_for(*lives[li][1:]):
            rows.append((byte, cap, mover, (byte + mover) & 1, jac, li, v))
    cases = [f"{b} {cap} {m} {s} {j} {bits(scale)} {bits(v)} " + " ".join(bits(F(q)) for q in lives[li])
             for b, cap, m, s, j, li, v in rows]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr and len(cases) > 60000
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert len(got) == len(rows)
    arr = np.array([(b, cap, m, s, j, li) for b, cap, m, s, j, li, _ in rows], np.int64)
    vals = np.array([r[6] for r in rows], F)
    seen = set()
    for cap, jac, li in itertools.product(caps, (0, 1), range(len(lives))):
        idx = np.nonzero((arr[:, 1] == cap) & (arr[:, 4] == jac) & (arr[:, 5] == li))[0]
        v, fl = C.janowski_reference(vals[idx], arr[idx, 0].astype(np.uint8), arr[idx, 2], scale, C.CubeLife(*lives[li]),
                                     cap, bool(jac))
        k = np.minimum(arr[idx, 0] & 15, cap)
        yq = C.cube_trunc_fixed_reference(v[:, 2], arr[idx, 2] == arr[idx, 3], k)
        want = [[str(int(k[i])), str(int(fl[i]))] + [bits(x) for x in v[i]] + [str(int(yq[i]))] for i in range(len(idx))]
        bad = [(cases[i], got[i], w) for i, w in zip(idx, want) if got[i] != w]
        assert not bad, bad[:5]
        seen |= set(fl.tolist())
    assert seen == {0, 1, 3, 4, 5, 7, 8, 12}                 # every reachable flag combination occurred
