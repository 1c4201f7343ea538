"""Truncated rollouts' host side (bgx/truncate.py, bgx/rollout.py; no GPU): the two summaries
against numpy on explicit games, truncate_reference on a hand-made trace, Truncation's and the
command line's refusals, the C ABI's declarations, and part 1 of csrc/bg_trunc.h built as a host
program (tools/trunc_host.cpp)."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from bgx import _lib, rollout as R, truncate as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = 65536


def trunc(plies=8, **kw):
    return T.Truncation(lambda eng, tsel: None, plies, **kw)


# ------------------------------------------------------------------- the summaries --
def rows_of(games):
    """games: (res, vq, plies, lq): a natural game has res in +-1..3 and vq None, a truncated one
    res None and its Vq; lq = the game's luck in 2^-16 -> (tally row, luck row, trunc row)."""
    t, k, c = np.zeros(8, np.int64), np.zeros(4, np.int64), np.zeros(7, np.int64)
    for res, vq, plies, lq in games:
        if vq is None:
            t[0] += 1; t[1] += plies; t[(2 if res > 0 else 5) + abs(res) - 1] += 1
            k[0] += lq; k[1] += lq * lq; k[2] += res * lq; k[3] += 1
        else:
            c[0] += 1; c[1] += plies; c[2] += vq; c[3] += vq * vq
            c[4] += lq; c[5] += lq * lq; c[6] += vq * lq
    return t, k, c


GAMES = [(2, None, 30, 9000), (-1, None, 41, -20000), (None, 20000, 8, 15000), (None, -50000, 8, -31000),
         (3, None, 7, 70000), (None, 196608, 8, 2097152), (-2, None, 60, -64000), (None, -1, 8, 0), (1, None, 5, 100)]


def values_of(games):
    y = np.array([g[0] if g[1] is None else g[1] / ONE for g in games], np.float64)
    return y, np.array([g[3] / ONE for g in games], np.float64)


def test_summarize_truncated_against_numpy():
    t, _, c = rows_of(GAMES)
    r = T.summarize_truncated(t, c, unfinished=2)
    y, _ = values_of(GAMES)
    assert (r["games"], r["natural_games"], r["truncated_games"], r["unfinished"]) == (9, 5, 4, 2)
    assert r["truncated_share"] == 4 / 9
    assert r["equity"] == pytest.approx(y.mean(), rel=1e-14)
    assert r["equity_stderr"] == pytest.approx(y.std(ddof=1) / 3.0, rel=1e-12)
    assert r["truncated_equity"] == pytest.approx((20000 - 50000 + 196608 - 1) / 4 / ONE, rel=1e-15)
    assert r["plies_per_game"] == pytest.approx((143 + 32) / 9)
    # the rates are those of the natural games alone
    nat = R.summarize(t)
    for f in ("win", "win_gammon", "win_backgammon", "loss", "loss_gammon", "loss_backgammon"):
        assert r[f] == nat[f]
    assert r["win"] == pytest.approx(3 / 5, rel=1e-15) and r["loss_gammon"] == pytest.approx(1 / 5, rel=1e-15)
    assert [r[f] for f in T.TRUNC_FIELDS] == c.tolist()
    assert "NATURAL games alone" in T.summarize_truncated.__doc__


def test_summarize_truncated_luck_against_numpy():
    t, k, c = rows_of(GAMES)
    y, L = values_of(GAMES)
    n = len(y)
    r = T.summarize_truncated_luck(t, k, c, "fit", unfinished=1)
    cfit = np.cov(y, L, ddof=1)[0, 1] / L.var(ddof=1)
    assert r["luck_scale"] == pytest.approx(cfit, rel=1e-12)
    adj = y - cfit * L
    assert r["equity_luck"] == pytest.approx(adj.mean(), rel=1e-11)
    assert r["equity_luck_stderr"] == pytest.approx(adj.std(ddof=1) / math.sqrt(n), rel=1e-9)
    assert r["variance_ratio"] == pytest.approx(adj.var(ddof=1) / y.var(ddof=1), rel=1e-9)
    assert r["luck_mean"] == pytest.approx(L.mean(), rel=1e-14)
    assert r["equity"] == T.summarize_truncated(t, c, 1)["equity"] and r["unfinished"] == 1
    r = T.summarize_truncated_luck(t, k, c, 0.5)
    adj = y - 0.5 * L
    assert r["luck_scale"] == 0.5 and r["equity_luck"] == pytest.approx(adj.mean(), rel=1e-12)
    assert r["equity_luck_stderr"] == pytest.approx(adj.std(ddof=1) / math.sqrt(n), rel=1e-10)
    k[3] += 1
    with pytest.raises(ValueError, match="counts 6 games"):
        T.summarize_truncated_luck(t, k, c)
    with pytest.raises(ValueError, match="7 entries"):
        T.summarize_truncated(t, c[:6])
    with pytest.raises(ValueError, match="4 entries"):
        T.summarize_truncated_luck(t, k[:3], c)


def test_summaries_small_cases():
    z8, z4, z7 = np.zeros(8, np.int64), np.zeros(4, np.int64), np.zeros(7, np.int64)
    # no game
    r = T.summarize_truncated_luck(z8, z4, z7)
    assert r["games"] == 0 and r["equity"] == 0.0 and r["equity_stderr"] == 0.0 and r["truncated_share"] == 0.0
    assert r["truncated_equity"] == 0.0 and r["equity_luck"] == 0.0 and r["equity_luck_stderr"] == 0.0
    assert r["variance_ratio"] == 1.0 and r["luck_scale"] == 0.0 and r["plies_per_game"] == 0.0
    # one game of each kind
    t, k, c = rows_of([(None, -98304, 8, 4096)])
    r = T.summarize_truncated_luck(t, k, c)
    assert (r["games"], r["natural_games"], r["truncated_games"]) == (1, 0, 1)
    assert r["equity"] == -1.5 and r["equity_stderr"] == 0.0 and r["truncated_equity"] == -1.5
    assert r["truncated_share"] == 1.0 and r["equity_luck"] == -1.5 and r["equity_luck_stderr"] == 0.0
    assert r["win"] == 0.0 and r["plies_per_game"] == 8.0
    t, k, c = rows_of([(-3, None, 20, 0)])
    r = T.summarize_truncated(t, c)
    assert r["equity"] == -3.0 and r["equity_stderr"] == 0.0 and r["truncated_share"] == 0.0 and r["loss_backgammon"] == 1.0
    # only natural games: summarize and summarize_luck
    nat = [g for g in GAMES if g[1] is None]
    t, k, c = rows_of(nat)
    r, s = T.summarize_truncated(t, c, 4), R.summarize(t, 4)
    for f, v in s.items():
        assert r[f] == pytest.approx(v, rel=1e-15, abs=0), f
    assert r["truncated_games"] == 0 and r["natural_games"] == 5
    for scale in ("fit", 0.75):
        r, s = T.summarize_truncated_luck(t, k, c, scale, 4), R.summarize_luck(t, k, scale, 4)
        for f, v in s.items():
            assert r[f] == pytest.approx(v, rel=1e-13, abs=1e-15), f
    # only truncated games
    tru = [g for g in GAMES if g[1] is not None]
    t, k, c = rows_of(tru)
    y, L = values_of(tru)
    r = T.summarize_truncated_luck(t, k, c)
    assert r["natural_games"] == 0 and r["truncated_share"] == 1.0 and r["win"] == 0.0 and r["loss"] == 0.0
    assert r["equity"] == pytest.approx(y.mean(), rel=1e-14) == r["truncated_equity"]
    assert r["equity_stderr"] == pytest.approx(y.std(ddof=1) / 2.0, rel=1e-12)
    cfit = np.cov(y, L, ddof=1)[0, 1] / L.var(ddof=1)
    assert r["equity_luck"] == pytest.approx((y - cfit * L).mean(), rel=1e-10)
    # equal values: exactly their value, a standard error of exactly 0 -- also mixed with natural
    # games of the same result, and with the luck adjustment fitted
    t, k, c = rows_of([(None, 21845, 8, 5)] * 7)
    r = T.summarize_truncated_luck(t, k, c)
    assert r["equity"] == 21845 / ONE and r["equity_stderr"] == 0.0
    assert r["luck_scale"] == 0.0 and r["equity_luck"] == 21845 / ONE and r["equity_luck_stderr"] == 0.0
    t, k, c = rows_of([(None, 131072, 8, 100), (2, None, 9, -300), (None, 131072, 8, 77), (2, None, 30, 1)])
    r = T.summarize_truncated_luck(t, k, c)
    assert r["equity"] == 2.0 and r["equity_stderr"] == 0.0 and r["luck_scale"] == 0.0
    assert r["equity_luck"] == 2.0 and r["equity_luck_stderr"] == 0.0 and r["variance_ratio"] == 1.0


# ------------------------------------------------------------------- value_q and the reference --
def test_value_q_rule():
    nan, inf = float("nan"), float("inf")
    v = np.array([0.25, 0.25, nan, inf, -inf, 1.6, -1.6, 0.1, 0.5 / ONE / 2, 1.5 / ONE / 2, -2.5 / ONE / 2], np.float32)
    same = np.array([1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1], bool)
    want = [32768, -32768, 0, 196608, 196608, 196608, -196608, -13107, 0, 2, -2]       # halves go to even
    assert T.value_q(2.0, v, same).tolist() == want
    assert T.value_q(0.0, np.array([inf, 3.0], np.float32), [True, True]).tolist() == [0, 0]   # 0 * inf is a NaN


def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def hand_trace():
    """Four lanes, four steps, horizon 2, two games a lane, scale 2 (the movers at a cut are free
    data here: both sign branches occur).  Lane 0: a gammon won after 2 plies, before the horizon
    counts; then a truncation on its last game at 0.25 from the start mover's side.  Lane 1:
    +inf seen by the other side (-3), then a NaN (0).  Lane 2 (start mover PLAYER2): -2 clamps to
    -3; -inf seen by the other side gives +3.  Lane 3: 0.1 seen by the other side, then a single
    game lost after one ply."""
    nan, inf = float("nan"), float("inf")
    starts = np.zeros((4, 64), np.uint8)
    starts[2, 52] = 1
    mover = np.array([[0, 1, 0, 1], [0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1]], np.uint8).T
    tmover = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [1, 1, 1, 1]], np.uint8).T
    tval = np.array([[nan, nan, nan, 0.25], [nan, inf, nan, nan], [nan, -2.0, nan, -inf], [nan, 0.1, nan, nan]],
                    np.float32).T
    luck = np.array([[0.5, 0.25, 0.125, -0.5], [1.0, 1.0, 40.0, 0.0], [0.5, 0.25, nan, 0.0], [0.0, 0.0, -0.5, 0.0]],
                    np.float32).T
    done, inf_ = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int32)
    for t, i, w, s in ((1, 0, 0, 2), (2, 3, 1, 1)):
        done[t, i], inf_[t, i] = 1, info(w, s)
    return dict(mover=mover, done=done, info=inf_, trunc_value=tval, trunc_mover=tmover), luck, starts


def test_truncate_reference_hand_made_trace():
    tr, luck, starts = hand_trace()
    group = np.array([0, 0, 1, 1], np.int32)
    tc = trunc(2, scale=2.0)
    out = T.truncate_reference(tr, starts, group, 2, 2, tc)
    assert out["tally"].tolist() == [[1, 2, 0, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 1, 0, 0]]
    assert out["trunc_tally"].tolist() == [[3, 6, 32768 - 196608, 32768 ** 2 + 196608 ** 2, 0, 0, 0],
                                           [3, 6, -13107, 2 * 196608 ** 2 + 13107 ** 2, 0, 0, 0]]
    assert out["luck_tally"] is None
    assert out["games_done"].tolist() == [2, 2, 2, 2] and out["active"] == 0
    assert out["trunc"].T.tolist() == [[False, False, False, True], [False, True, False, True],
                                       [False, True, False, True], [False, True, False, False]]
    # with luck: lane 0's first game flushes 0.25, its second is truncated with 0.625; lane 1's
    # second sum clamps at 2^21; lane 2's second is a NaN (0); lane 3 loses with -0.5
    out = T.truncate_reference(dict(tr, luck=luck), starts, group, 2, 2, tc)
    assert out["luck_tally"].tolist() == [[16384, 16384 ** 2, 2 * 16384, 1], [-32768, 32768 ** 2, 32768, 1]]
    assert out["trunc_tally"].tolist() == [
        [3, 6, 32768 - 196608, 32768 ** 2 + 196608 ** 2, 40960 + (1 << 21), 40960 ** 2 + (1 << 42), 32768 * 40960],
        [3, 6, -13107, 2 * 196608 ** 2 + 13107 ** 2, 16384, 16384 ** 2, -196608 * 16384]]
    for p in range(2):
        T.summarize_truncated_luck(out["tally"][p], out["luck_tally"][p], out["trunc_tally"][p])
    # one game a lane: lane 0 retires with its natural game, the others with their first cut
    out = T.truncate_reference(tr, starts, group, 2, 1, tc)
    assert out["games_done"].tolist() == [1, 1, 1, 1] and out["trunc_tally"][:, 0].tolist() == [1, 2]
    # a horizon no game reaches, three games a lane: natural games only, lanes still active
    out = T.truncate_reference(tr, starts, group, 2, 3, trunc(5))
    assert out["trunc_tally"].tolist() == [[0] * 7] * 2 and out["tally"][:, 0].tolist() == [1, 1]
    assert out["games_done"].tolist() == [1, 0, 0, 1] and out["active"] == 4 and not out["trunc"].any()
    # an idle lane and a group outside the rows are never counted
    out = T.truncate_reference(tr, starts, np.array([0, -1, 5, 1]), 2, 2, tc)
    assert out["trunc_tally"][:, 0].tolist() == [1, 1] and out["games_done"].tolist() == [2, 0, 0, 2]
    assert not out["trunc"][:, 1:3].any()


# ------------------------------------------------------------------- refusals --
def test_truncation_arguments():
    t = trunc(8)
    assert (t.plies, t.scale, t.lookahead, t.is_head, t.sync_free) == (8, 1.0, 0, False, False)
    assert trunc(1, scale=-2.0, lookahead=1).scale == -2.0
    for kw in (dict(plies=0), dict(plies=-3), dict(plies=2.5), dict(plies=True), dict(scale=math.nan),
               dict(lookahead=2), dict(lookahead=-1), dict(lookahead=True)):
        with pytest.raises(ValueError):
            trunc(**{"plies": 8, **kw})
    with pytest.raises(ValueError):
        T.Truncation(3.0, 8)
    assert R.Truncation is T.Truncation and R.summarize_truncated is T.summarize_truncated


def test_parser_flags():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.truncate is None and ns.truncate_net is None
    assert (ns.truncate_scale, ns.truncate_lookahead) == (1.0, 0)
    ns = ap.parse_args("--net ckpt.pt --positions opening --truncate 8 --truncate-scale 2 --truncate-lookahead 1 "
                       "--luck".split())
    assert (ns.truncate, ns.truncate_scale, ns.truncate_lookahead, ns.luck) == (8, 2.0, 1, True)
    assert ap.parse_args("--net random --positions opening --truncate 1 --truncate-net v.pt".split()).truncate_net == "v.pt"
    for bad in ("--net random --positions opening --truncate 8",
                "--net ckpt.pt --positions opening --truncate 0",
                "--net ckpt.pt --positions opening --truncate -4",
                "--net ckpt.pt --positions opening --truncate 8 --bearoff 6",
                "--net ckpt.pt --positions opening --truncate 8 --bearoff1 15",
                "--net ckpt.pt --positions opening --truncate 8 --cube",
                "--net ckpt.pt --positions opening --truncate 8 --truncate-lookahead 2",
                "--net ckpt.pt --positions opening --truncate 8 --truncate-scale nan",
                "--net ckpt.pt --positions opening --truncate-lookahead 1",
                "--net ckpt.pt --positions opening --truncate-net v.pt"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


# ------------------------------------------------------------------------- the C ABI --
def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in (("bgx_value_lanes", 8), ("bgx_rollout_trunc_sel", 10), ("bgx_rollout_trunc_cut", 17)):
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):                    # pointer / float / int32, in the header's order
            want = _lib._P if "*" in p else ctypes.c_float if p.startswith("float") else _lib._I32
            assert a is want and ("*" in p or p.startswith(("float ", "int32_t "))), (name, p)
    fields = re.search(r"enum bgx_rollout_trunc_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ROLLOUT_(TRUNC_\w+)\s*=\s*(\d+)", fields)
    assert [(n.lower(), int(v)) for n, v in names] == [(f, i) for i, f in enumerate(T.TRUNC_FIELDS)]
    # the device code is part 2 of csrc/bg_trunc.h, compiled with bg_returns.hip after bg_cube.h
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_cube.h"') < src.index('#include "bg_trunc.h"')
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("bgx_value_lanes", "bgx_rollout_trunc_sel", "bgx_rollout_trunc_cut"):
        assert name in integration, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in _lib.SIGNATURES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", x))[0]


def test_value_rule_host_program(tmp_path):
    """tools/trunc_host.cpp with AddressSanitizer + UBSan, a program of its own: trunc_value_q
    over three scales, both sides and values on, beside and far from 0, the clamp +-3 / scale
    and the halves of 2^-16, NaN and the infinities, against value_q."""
    exe = str(tmp_path / "trunc_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "trunc_host.cpp"), "-o", exe], check=True)
    up, down = lambda v: F(np.nextafter(F(v), F(np.inf))), lambda v: F(np.nextafter(F(v), F(-np.inf)))
    cases, want = [], []
    for scale in (1.0, 0.5, -2.0):
        vals = [F(0.0), F(-0.0), up(0.0), down(0.0), F(0.37), F(-1.9), F(100.0), F(-1e30), F(1e-30),
                F(math.nan), F(math.inf), F(-math.inf)]
        for edge in (3.0 / scale, -3.0 / scale):
            vals += [F(edge), up(edge), down(edge)]
        for k in (0, 1, 2, 7, 196607, -1, -2, -3, -196608):            # e * 2^16 = k + 1/2 exactly
            h = F((k + 0.5) / ONE / scale)
            assert float(h) * scale * ONE == k + 0.5
            vals += [h, up(h), down(h)]
        v = np.array(vals, np.float32)
        for same in (1, 0):
            want += T.value_q(scale, v, np.full(v.shape, bool(same))).tolist()
            cases += [f"{bits(scale)} {bits(float(x))} {same}" for x in v]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr and len(cases) == 3 * 2 * 45
    got = [int(ln) for ln in out.stdout.splitlines()]
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:5]
    assert max(got) == 196608 and min(got) == -196608 and 0 in got and {1, -1, 2, -2} <= set(got)
