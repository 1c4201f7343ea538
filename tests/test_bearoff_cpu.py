"""The bearoff database's host side (bgx/bearoff.py, bgx/rollout.py; no GPU): the estimator of
the rollout cut, the host replay of the cut bookkeeping, the command-line flags, the C ABI's
declarations, and the successor enumeration of csrc/bg_bearoff.h built as a host program
(tools/bearoff_succ.cpp) against the oracle's move generator."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bearoff_ref as BR
from bgx import _lib, arena as A, rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = R.CUT_ONE


# ------------------------------------------------------------ summarize_bearoff --
def test_summarize_all_cut():
    pq = 851968                                            # 0.8125
    r = R.summarize_bearoff([0] * 8, [10, 30, 10 * pq, 10 * pq * pq])
    assert r["games"] == r["cut_games"] == 10 and r["natural_games"] == 0 and r["cut_share"] == 1.0
    assert r["equity"] == 2 * 0.8125 - 1 and r["equity_stderr"] == 0.0
    assert r["win"] == 0.8125 and r["loss"] == 1 - 0.8125 and r["win_gammon"] == 0.0
    assert r["plies_per_game"] == 3.0 and r["unfinished"] == 0


def test_summarize_none_cut_is_summarize():
    row = [12, 100, 5, 1, 0, 4, 1, 1]
    r, s = R.summarize_bearoff(row, [0, 0, 0, 0], unfinished=3), R.summarize(row, 3)
    assert r["cut_games"] == 0 and r["cut_share"] == 0.0 and r["natural_games"] == 12
    for k, v in s.items():
        assert r[k] == pytest.approx(v, rel=1e-12, abs=0), k


def test_summarize_mixed():
    """Two natural games (+1, -2) and two cut games with P = 0.25 and 0.75."""
    pa, pb = ONE // 4, 3 * ONE // 4
    r = R.summarize_bearoff([2, 9, 1, 0, 0, 0, 1, 0], [2, 5, pa + pb, pa * pa + pb * pb])
    ys = np.array([1.0, -2.0, -0.5, 0.5])
    assert r["games"] == 4 and r["cut_games"] == 2 and r["cut_share"] == 0.5
    assert r["equity"] == ys.mean() == -0.25
    assert r["equity_stderr"] == pytest.approx(ys.std(ddof=1) / 2.0, rel=1e-15)
    assert r["win"] == (1 + 0.25 + 0.75) / 4 and r["loss"] == (1 + 0.75 + 0.25) / 4
    assert r["loss_gammon"] == 0.25 and r["win_gammon"] == 0.0       # natural games only, over all games
    assert r["plies_per_game"] == 14 / 4


def test_summarize_zero_and_one_game():
    r = R.summarize_bearoff([0] * 8, [0] * 4)
    assert r["games"] == 0 and r["equity"] == 0.0 and r["equity_stderr"] == 0.0 and r["cut_share"] == 0.0
    assert r["win"] == 0.0 and r["plies_per_game"] == 0.0
    r = R.summarize_bearoff([0] * 8, [1, 0, ONE, ONE * ONE])
    assert r["games"] == 1 and r["equity"] == 1.0 and r["equity_stderr"] == 0.0
    with pytest.raises(ValueError):
        R.summarize_bearoff([0] * 8, [0] * 3)


# -------------------------------------------------------- bearoff_cut_reference --
def _info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


A1, B6 = (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1)            # one checker on the ace point / the six-point
CONFIGS = np.array([(0,) * 6, A1, B6], np.int8)
# W by hand: the ace-point checker always bears off; the six-point one in 27 of 36 rolls
TABLE = np.array([[0, 1, 1], [0, 1, 1], [0, 0.75, 0.75 + 0.25 * 0.25]], np.float32)


def test_lookup_reference():
    from bgx.bearoff import lookup_reference
    recs = np.stack([BR.record(B6, B6, 0), BR.record(A1, B6, 1), BR.record(A1, B6, 0)])
    over = BR.record(A1, B6, 0)
    over[55] = 1
    two = BR.record((2, 0, 0, 0, 0, 0), B6, 0)
    in_db, win = lookup_reference(np.stack([*recs, over, two]), CONFIGS, TABLE, 1)
    assert in_db.tolist() == [True, True, True, False, False]
    assert win[:3].tolist() == [0.8125, 0.75, 1.0] and np.isnan(win[3:]).all()


def test_cut_reference_hand_trace():
    """Three lanes, two steps, two games a lane.  Lane 0 (group 0, start mover 0) starts in the
    table and is cut at once, then again after one ply with the other side on roll; lane 1
    (group 1, start mover 1) wins a gammon outside the table, then is cut one ply into its
    second game; lane 2 is idle, in the table all the time and never counted."""
    out = np.zeros(64, np.uint8)                           # not in the table: a PLAYER1 checker on point 10
    out[10], out[50], out[24], out[51], out[52] = 1, 14, 1, 14, 1
    starts = np.stack([BR.record(B6, B6, 0), out, BR.record(A1, A1, 0)])
    group = np.array([0, 1, -1])
    idle = BR.record(A1, A1, 0)
    records0 = np.stack([starts[0], out, idle])
    records = np.stack([np.stack([BR.record(A1, B6, 1), out, idle]),
                        np.stack([BR.record(A1, B6, 1), BR.record(B6, A1, 1), idle])])
    done = np.array([[0, 1, 1], [1, 0, 0]], np.uint8)
    info = np.array([[0, _info(1, 2), _info(0, 1)], [_info(0, 1), 0, 0]], np.int32)
    ref = R.bearoff_cut_reference(records0, records, done, info, starts, group, 2, 2, CONFIGS, TABLE, 1)
    p0, p1 = 851968, 262144                                # 0.8125, and 1 - 0.75 for the other side on roll
    assert ref["cut_tally"].tolist() == [[2, 1, p0 + p1, p0 * p0 + p1 * p1], [1, 1, ONE, ONE * ONE]]
    assert ref["tally"].tolist() == [[0] * 8, [1, 1, 0, 1, 0, 0, 0, 0]]
    assert ref["games_done"].tolist() == [2, 2, 0] and ref["active"] == 0
    assert ref["cut0"].tolist() == [True, False, False]
    assert ref["cut"].tolist() == [[True, False, False], [False, True, False]]
    res = R.summarize_bearoff(ref["tally"][0], ref["cut_tally"][0])
    assert res["equity"] == ((2 * 0.8125 - 1) + (2 * 0.25 - 1)) / 2 and res["cut_share"] == 1.0


# ----------------------------------------------------------------- command line --
def test_rollout_parser():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.bearoff is None and ns.bearoff_play is None
    ns = ap.parse_args("--net random --positions opening --bearoff 6".split())
    assert ns.bearoff == 6 and ns.bearoff_play is None
    ns = ap.parse_args("--net ckpt.pt --player 2ply --top-k 4 --positions opening --bearoff-play".split())
    assert ns.bearoff is None and ns.bearoff_play == 6
    ns = ap.parse_args("--net random --positions opening --bearoff 8 --bearoff-play 5".split())
    assert (ns.bearoff, ns.bearoff_play) == (8, 5)
    for bad in ("--net ckpt.pt --positions opening --luck --bearoff 6",
                "--net random --positions opening --bearoff 0",
                "--net random --positions opening --bearoff 9",
                "--net random --positions opening --bearoff-play 9",
                "--net random --positions opening --bearoff six"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def test_arena_parser():
    ap = A.build_parser()
    ns = ap.parse_args("--a random --b random --max-steps 10".split())
    assert ns.bearoff_a is None and ns.bearoff_b is None
    ns = ap.parse_args("--a random --b random --max-steps 10 --bearoff-a 6 --bearoff-b 4".split())
    assert (ns.bearoff_a, ns.bearoff_b) == (6, 4)
    for bad in ("--a random --b random --max-steps 10 --bearoff-a 0",
                "--a random --b random --max-steps 10 --bearoff-b 9"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())
    assert A.PLAYER_KINDS == ("policy", "greedy", "1ply", "2ply")


def test_run_refuses_bearoff_with_luck():
    """Refused before anything touches the device."""
    ro = object.__new__(R.Rollout)
    with pytest.raises(ValueError, match="luck"):
        R.Rollout.run(ro, None, None, 36, luck=object(), bearoff=object())
    with pytest.raises(ValueError, match="luck"):
        R.Rollout.run_lanes(ro, None, None, None, 1, 1, luck=object(), bearoff=object())


# ------------------------------------------------------------------------ C ABI --
SYMBOLS = {"bgx_bearoff_create": 4, "bgx_bearoff_buffers_get": 2, "bgx_bearoff_destroy": 1, "bgx_bearoff_lookup": 6,
           "bgx_bearoff_act": 6, "bgx_rollout_bearoff_cut": 14}


def test_symbols_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, argc in SYMBOLS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == argc, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == argc, name
    for field in ("BGX_ROLLOUT_CUT_GAMES = 0", "BGX_ROLLOUT_CUT_PLIES = 1", "BGX_ROLLOUT_CUT_P = 2",
                  "BGX_ROLLOUT_CUT_P2 = 3"):
        assert field in txt
    assert [f for f, _ in _lib.BgxBearoffBuffers._fields_] == ["table", "configs", "succ_off", "succ", "n",
                                                               "max_checkers"]
    assert R.CUT_FIELDS == ("cut_games", "cut_plies", "cut_p", "cut_p2")
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in SYMBOLS:
            assert hasattr(lib, name), name


# ---------------------------------------------- the successor enumeration, on the host --
def test_successors_equal_the_oracle(tmp_path):
    """K = 4: for all 210 configurations x 21 rolls and both movers, the sets of
    csrc/bg_bearoff.h (compiled for the host with AddressSanitizer + UBSan) are the oracle's."""
    exe = str(tmp_path / "bearoff_succ")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bearoff_succ.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "widest 15 " in r.stderr

    def key(c):
        return sum(v * 9 ** d for d, v in enumerate(c))
    got = {}
    for line in r.stdout.splitlines():
        v = [int(x) for x in line.split()]
        assert v[3] == len(v) - 4
        got[(v[0], v[1], v[2])] = set(v[4:])
    configs = BR.all_configs(4)
    assert len(configs) == 210 == math.comb(10, 6) and len(got) == 210 * 21
    for c in configs:
        for mover in (0, 1):
            for roll, want in zip(BR.ROLLS21, BR.oracle_successors(c, mover)):
                assert got[(key(c),) + roll] == {key(s) for s in want}, (c, mover, roll)
