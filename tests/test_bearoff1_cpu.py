"""The one-sided bearoff database's host side (bgx/bearoff.py, bgx/rollout.py; no GPU): the numpy
references of the recurrence, of win1 and of the lookup on hand-made tables, the K = 2 table
from the oracle's move generator, the command-line flags, the C ABI's declarations, and the
play visitor of csrc/bg_bearoff1.h built as a host program (tools/bearoff1_host.cpp)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bearoff_ref as BR
from bgx import _lib, arena as A, bearoff as BO, rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# the means of six and of fifteen checkers on the six point (tools/bearoff1_host.cpp table 15):
# 5.312426 and 12.266191
MEAN_6x6, MEAN_15x6 = 0x40A9FF65, 0x41444252


def key16(c):
    return sum(v * 16 ** d for d, v in enumerate(c))


def pips(c):
    return sum((d + 1) * v for d, v in enumerate(c))


# ------------------------------------------------------------------- hand-made tables --
DOUBLES = [r for r, (a, b) in enumerate(BO.ROLLS21) if a == b]
# configuration 1 goes to the empty one with every roll; 2 does so with doubles only (where it
# may also go to 1: the empty one has the smaller mean) and to 1 otherwise
SUCC3 = [[[0]] * 21, [[0]] * 21, [[1, 0] if r in DOUBLES else [1] for r in range(21)]]


def seq_sum(values):
    acc = F(0)
    for v in values:
        acc = F(acc + F(v))
    return acc


def test_dist_reference_by_hand():
    dist, surv, mean, choice = BO.dist_reference(SUCC3, 3)
    assert dist.shape == surv.shape == (3, 32) and dist.dtype == surv.dtype == mean.dtype == np.float32
    assert choice.shape == (3, 21) and choice.dtype == np.int32
    p = BO.ROLL_P
    all_p = seq_sum(p)                                          # the 21 fp32 probabilities, not 1.0f
    assert abs(float(all_p) - 1) < 3e-7
    assert dist[0].tolist() == [1] + [0] * 31 and surv[0].tolist() == [1] + [0] * 31 and mean[0] == 0
    assert not choice[:2].any()
    assert dist[1, 1] == all_p and not dist[1, 2:].any() and dist[1, 0] == 0
    assert mean[1] == all_p
    assert surv[1, :2].tolist() == [1, 1] and (surv[1, 2:] == F(F(1) - all_p)).all()
    assert choice[2].tolist() == [0 if r in DOUBLES else 1 for r in range(21)]
    d1 = seq_sum(p[r] if r in DOUBLES else F(0) for r in range(21))
    d2 = seq_sum(F(p[r] * all_p) if r not in DOUBLES else F(0) for r in range(21))
    assert dist[2, 1] == d1 and dist[2, 2] == d2 and not dist[2, 3:].any()
    # d2 carries all_p's 2.4e-7 and up to 15 roundings of 2^-24 each
    assert abs(float(d1) - 1 / 6) < 1e-7 and abs(float(d2) - 5 / 6) < 1e-6
    assert mean[2] == F(F(F(1) * d1) + F(F(2) * d2))
    s2 = F(F(1) - d1)
    assert surv[2, :3].tolist() == [1, 1, s2] and (surv[2, 3:] == F(s2 - d2)).all()


def test_choice_ties_go_to_the_smaller_index():
    succ = [[[0]] * 21, [[0]] * 21, [[0]] * 21, [[2, 1]] * 21, [[2, 1, 1, 2]] * 21]
    dist, surv, mean, choice = BO.dist_reference(succ, 5)
    assert mean[1] == mean[2] and (choice[3] == 1).all() and (choice[4] == 1).all()
    assert np.array_equal(dist[3], dist[4])


def test_win1_reference_by_hand():
    dist, surv, mean, choice = BO.dist_reference(SUCC3, 3)
    # 2 on roll against 2 wins when it is off with its first roll, or with its second when the
    # other was not off with its first
    want = F(F(dist[2, 1] * F(1)) + F(dist[2, 2] * surv[2, 2]))
    assert BO.win1_reference(dist[2], surv[2]) == want and abs(float(want) - (1 / 6 + 5 / 6 * 5 / 6)) < 1e-6
    # 1 on roll always wins (to the rounding of the 21 probabilities); against 1, 2 wins with doubles
    assert BO.win1_reference(dist[1], surv[2]) == dist[1, 1]
    assert BO.win1_reference(dist[2], surv[1]) == F(dist[2, 1] + F(dist[2, 2] * surv[1, 2]))
    # broadcast: all pairs at once
    allp = BO.win1_reference(dist[1:, None, :], surv[None, 1:, :])
    assert allp.shape == (2, 2) and allp[1, 1] == want and allp[0, 1] == dist[1, 1]


A1, B6, F15 = (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 0, 15)


def test_lookup1_reference():
    dist, surv, mean, choice = BO.dist_reference(SUCC3, 3)
    # a fourth row, fifteen on the six point, made up: off with exactly 7 rolls
    d15, s15 = np.zeros(32, F), np.zeros(32, F)
    d15[7], s15[:8] = 1, 1
    configs = np.array([(0,) * 6, A1, B6, F15], np.int8)
    dist, surv = np.vstack([dist, d15]), np.vstack([surv, s15])
    over = BR.record(A1, B6, 0)
    over[55] = 1
    bar = BR.record(A1, B6, 0)
    bar[23], bar[48] = 0, 1
    outfield = BR.record(A1, B6, 1)
    outfield[24], outfield[24 + 9] = 0, 1
    short = BR.record(A1, B6, 0)
    short[50] = 13
    recs = np.stack([BR.record(B6, B6, 0), BR.record(A1, B6, 1), BR.record(A1, B6, 0), BR.record(F15, A1, 0),
                     BR.record(B6, F15, 0), BR.record(B6, F15, 1), over, bar, outfield, short])
    in_db, win = BO.lookup1_reference(recs, configs, dist, surv, 15)
    assert in_db.dtype == np.uint8 and in_db.tolist() == [1, 1, 1, 2, 2, 2, 0, 0, 0, 0]
    assert np.isnan(win[6:]).all() and not np.isnan(win[:6]).any()
    assert win[0] == BO.win1_reference(dist[2], surv[2])
    assert win[1] == BO.win1_reference(dist[2], surv[1]) and win[2] == BO.win1_reference(dist[1], surv[2])
    # fifteen on roll wins when the other still needs a seventh roll: S[.][7], the fp32 rest of 1
    assert win[3] == surv[1, 7] and abs(float(win[3])) < 3e-7
    assert win[4] == BO.win1_reference(dist[2], surv[3]) == F(dist[2, 1] + dist[2, 2])
    assert win[5] == surv[2, 7] and abs(float(win[5])) < 1e-6
    # with K = 1 the fifteen-checker records are outside, and so are two checkers
    recs = np.vstack([recs, BR.record((2, 0, 0, 0, 0, 0), B6, 0)[None]])
    in_db, win = BO.lookup1_reference(recs, configs, dist, surv, 1)
    assert in_db.tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]


def test_cut_reference_takes_a_lookup():
    """bearoff_cut_reference with the one-sided lookup: a lane in the table with 15 checkers of a
    side on the board (in_db 2) is not cut."""
    dist, surv, mean, choice = BO.dist_reference(SUCC3, 3)
    d15, s15 = np.zeros(32, F), np.zeros(32, F)
    d15[7], s15[:8] = 1, 1
    configs = np.array([(0,) * 6, A1, B6, F15], np.int8)
    dist, surv = np.vstack([dist, d15]), np.vstack([surv, s15])

    def lookup(recs):
        in_db, w = BO.lookup1_reference(recs, configs, dist, surv, 15)
        return in_db == 1, w

    starts = np.stack([BR.record(B6, B6, 0), BR.record(F15, B6, 1)])
    group = np.array([0, 1])
    done, info = np.zeros((1, 2), np.uint8), np.zeros((1, 2), np.int32)
    ref = R.bearoff_cut_reference(starts, starts[None], done, info, starts, group, 2, 2, lookup=lookup)
    pq = int(np.rint(F(BO.win1_reference(dist[2], surv[2]) * F(R.CUT_ONE))))
    assert ref["cut_tally"].tolist() == [[2, 1, 2 * pq, 2 * pq * pq], [0, 0, 0, 0]]
    assert ref["cut0"].tolist() == [True, False] and ref["games_done"].tolist() == [2, 0] and ref["active"] == 1


# ------------------------------------------------------------- K = 2 from the oracle --
def test_k2_rows():
    cfg = sorted(BR.all_configs(2), key=lambda c: (pips(c), key16(c)))
    n = len(cfg)
    assert n == 28 == math.comb(8, 6) and cfg[0] == (0,) * 6
    index = {c: i for i, c in enumerate(cfg)}
    succ = [[sorted(index[s] for s in row) for row in BR.oracle_successors(c)] for c in cfg]
    dist, surv, mean, choice = BO.dist_reference(succ, n)
    sums = dist.astype(np.float64).sum(1)
    assert np.abs(sums - 1).max() <= 1e-6, sums
    assert not dist[1:, 0].any() and dist[0, 0] == 1 and not dist[:, 31].any()
    assert (choice[1:] < np.arange(1, n)[:, None]).all()
    # one checker on the ace point is off with one roll; S is the tail sum of D
    assert mean[index[A1]] == dist[index[A1], 1] and abs(float(mean[index[A1]]) - 1) < 3e-7
    tail = dist.astype(np.float64)[:, ::-1].cumsum(1)[:, ::-1]
    assert np.abs(surv[1:, 1:] - tail[1:, 1:]).max() < 1e-6
    # the approximation is exact where one side cannot choose: one checker each
    w = BO.win1_reference(dist[index[B6]], surv[index[B6]])
    assert abs(float(w) - (0.75 + 0.25 * 0.25)) < 1e-6


# ----------------------------------------------------------------- command line --
def test_rollout_parser():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.bearoff1 is None and ns.bearoff1_play is None
    ns = ap.parse_args("--net random --positions opening --bearoff1 15".split())
    assert ns.bearoff1 == 15 and ns.bearoff1_play is None and ns.bearoff is None
    ns = ap.parse_args("--net random --positions opening --bearoff1-play".split())
    assert ns.bearoff1_play == 15 and ns.bearoff1 is None
    ns = ap.parse_args("--net random --positions opening --bearoff1 9 --bearoff1-play 12 --bearoff-play".split())
    assert (ns.bearoff1, ns.bearoff1_play, ns.bearoff_play) == (9, 12, 6)
    for bad in ("--net random --positions opening --bearoff 6 --bearoff1 15",
                "--net ckpt.pt --positions opening --luck --bearoff1 15",
                "--net random --positions opening --bearoff1 0",
                "--net random --positions opening --bearoff1 16",
                "--net random --positions opening --bearoff1-play 16",
                "--net random --positions opening --bearoff1 all"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def test_arena_parser():
    ap = A.build_parser()
    ns = ap.parse_args("--a random --b random --max-steps 10".split())
    assert ns.bearoff1_a is None and ns.bearoff1_b is None
    ns = ap.parse_args("--a random --b random --max-steps 10 --bearoff1-a 15 --bearoff1-b 9 --bearoff-a 6".split())
    assert (ns.bearoff1_a, ns.bearoff1_b, ns.bearoff_a) == (15, 9, 6)
    for bad in ("--a random --b random --max-steps 10 --bearoff1-a 0",
                "--a random --b random --max-steps 10 --bearoff1-b 16"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def test_refusals_before_the_device():
    with pytest.raises(ValueError, match="1..15"):
        BO.OneSidedBearoffDB(16)
    with pytest.raises(ValueError, match="1..15"):
        BO.OneSidedBearoffDB(0)
    assert BO.OneSidedBearoffDB.kind == "one-sided" and BO.BearoffDB.kind == "two-sided"
    assert issubclass(BO.OneSidedPlayer, BO.BearoffPlayer)


# ------------------------------------------------------------------------ C ABI --
SYMBOLS = {"bgx_bearoff1_create": 4, "bgx_bearoff1_buffers_get": 2, "bgx_bearoff1_destroy": 1,
           "bgx_bearoff1_lookup": 6, "bgx_bearoff1_act": 6, "bgx_rollout_bearoff1_cut": 14}


def test_symbols_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, argc in SYMBOLS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", txt, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == argc, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == argc, name
    assert _lib.SIGNATURES["bgx_rollout_bearoff1_cut"] == _lib.SIGNATURES["bgx_rollout_bearoff_cut"]
    assert [f for f, _ in _lib.BgxBearoff1Buffers._fields_] == ["dist", "surv", "mean", "choice", "configs", "n",
                                                                "max_checkers"]
    m = re.search(r"typedef struct \{([^}]*)\} bgx_bearoff1_buffers;", txt)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == ["dist", "surv", "mean", "choice", "configs", "n", "max_checkers"]
    assert BO.OneSidedBearoffDB.cut_entry in SYMBOLS and BO.OneSidedBearoffDB.lookup_entry in SYMBOLS
    # the device code is part 2 of csrc/bg_bearoff1.h, compiled with bg_returns.hip
    csrc = os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc")
    assert '#include "bg_bearoff1.h"' in open(os.path.join(csrc, "bg_returns.hip")).read()
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in SYMBOLS:
            assert hasattr(lib, name), name


# --------------------------------------------------------- the visitor, on the host --
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tools/bearoff1_host.cpp with AddressSanitizer + UBSan, a program of its own."""
    exe = str(tmp_path_factory.mktemp("bearoff1") / "bearoff1_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bearoff1_host.cpp"), "-o", exe], check=True)
    return exe


def fields(line):
    v = line.split()
    return {v[i]: v[i + 1] for i in range(0, len(v) - 1) if not v[i][0].isdigit() and v[i] not in ("rowsum", "means")}, v


def test_visitor_equals_bo_successors(host_program):
    """K = 6: for all 924 configurations x 21 rolls the distinct plays of the visitor with the
    largest number of sub-moves are bo_successors' set."""
    r = subprocess.run([host_program, "succ", "6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    f, _ = fields(r.stdout)
    assert (f["K"], f["sets"], f["mismatches"], f["widest"]) == ("6", str(924 * 21), "0", "35"), r.stdout


def test_k15_table_on_the_host(host_program):
    r = subprocess.run([host_program, "table", "15"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    f, v = fields(r.stdout)
    assert f["n"] == "54264" == str(math.comb(21, 6)) and f["widest"] == "108" and f["total"] == "9208660"
    assert f["last_t"] == "30"
    lo, hi = (float(x) for x in v[v.index("rowsum") + 1:v.index("rowsum") + 3])
    assert 1.0 <= lo <= hi <= 1 + 6.5e-7
    means = v[v.index("means") + 1:]
    assert means == ["5.312426", f"0x{MEAN_6x6:08x}", "12.266191", f"0x{MEAN_15x6:08x}"]
