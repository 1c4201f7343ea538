"""The cubeful exact bearoff table's host side (bgx/bearoff.py, bgx/cube.py,
bgx/rollout.py; no GPU): the recurrence's numpy form against a plain restatement and by hand, its
structure at K = 3, summarize_cube_bearoff against numpy, the cut's host replay on a hand-made
trace, the command-line flags, the C ABI's declarations, and part 1 of csrc/bg_bearoff_cube.h
built as a host program (tools/cube_bearoff_host.cpp)."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bearoff_ref as BR
import cube_bearoff_ref as CR
from bgx import _lib, bearoff as BO, cube as C, rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ONE = C.CUBE_CUT_ONE
A1, B6 = (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1)            # one checker on the ace point / the six-point


# ------------------------------------------------------------------- the recurrence --
def restated(succ, cfg, f):
    """The recurrence of include/bgx.h pair by pair, by total pip count, in scalars of type f."""
    n = len(cfg)
    pip = [sum((d + 1) * v for d, v in enumerate(c)) for c in cfg]
    p = [f(1.0 / 36.0) if a == b else f(2.0 / 36.0) for a, b in BR.ROLLS21]
    E, ND = np.zeros((3, n, n), f), np.zeros((2, n, n), f)
    for s in range(3):
        for i in range(n):
            E[s, i, 0] = f(-1)
            if i:
                E[s, 0, i] = f(1)
    ND[:] = E[:2]
    child = {0: 0, 1: 2, 2: 1}
    for a, b in sorted(((a, b) for a in range(1, n) for b in range(1, n)), key=lambda ab: pip[ab[0]] + pip[ab[1]]):
        acc = [f(0), f(0), f(0)]
        for r in range(21):
            for s in range(3):
                best = max(f(1) if ap == 0 else f(-E[child[s], b, ap]) for ap in succ[a][r])
                acc[s] = f(acc[s] + f(p[r] * best))
        dt = f(f(2) * acc[2])
        cash = min(dt, f(1))
        ND[0, a, b], ND[1, a, b] = acc[0], acc[1]
        E[0, a, b], E[1, a, b], E[2, a, b] = max(acc[0], cash), max(acc[1], cash), acc[2]
    return E, ND


def test_recurrence_k2_against_a_restatement_and_by_hand():
    cfg, succ = CR.ordered_configs(2), CR.oracle_succ(2)
    n = len(cfg)
    assert n == 28 and cfg[0] == (0,) * 6 and cfg[1] == A1
    E, ND = BO.cube_table_reference(succ, n, np.float32)
    E2, ND2 = restated(succ, cfg, np.float32)
    assert E.dtype == np.float32 and E.shape == (3, n, n) and ND.shape == (2, n, n)
    assert np.array_equal(E.view(np.uint32), E2.view(np.uint32)) and np.array_equal(ND.view(np.uint32), ND2.view(np.uint32))
    E64, ND64 = BO.cube_table_reference(succ, n, np.float64)
    assert E64.dtype == np.float64 and np.abs(E64 - E).max() < 1e-6 and np.abs(ND64 - ND).max() < 1e-6
    W = CR.references(2, "float32")[0]
    # one checker on the six-point against one on the ace point, roller first: it wins with 27 rolls of 36
    a, b = cfg.index(B6), cfg.index(A1)
    for Ex, NDx in ((E, ND), (E64, ND64)):
        assert abs(NDx[0, a, b] - 0.5) < 1e-6 and abs(NDx[1, a, b] - 0.5) < 1e-6 and abs(2 * Ex[2, a, b] - 1.0) < 1e-6
        assert abs(Ex[0, a, b] - 1.0) < 1e-6 and abs(Ex[1, a, b] - 1.0) < 1e-6 and abs(Ex[2, a, b] - 0.5) < 1e-6
    assert F(2) * E[2, a, b] < F(1)                          # in fp32 DT comes out just below 1 ...
    for s in (0, 1):                                         # ... so: a double and a take
        v, fl = BO.cube_values_reference(s, ND[s, a, b], E[2, a, b], W[a, b])
        assert fl == 1 | 2 | 4 and v[1] == F(2) * E[2, a, b] and v[2] == v[1] and abs(v[3] - 0.5) < 1e-6
    v, fl = BO.cube_values_reference(2, 0.0, E[2, a, b], W[a, b])
    assert fl == 4 and v[0] == v[2] == E[2, a, b]           # no access: e = nd = E_opp
    v, fl = BO.cube_values_reference(3, 0.0, E[2, a, b], W[a, b])
    assert fl == 4 | 8 and v[0] == v[2] == v[3]             # dead: the cubeless value
    # a = one checker on the ace point: a certain win, every value +1, and no double (a tie)
    a = cfg.index(A1)
    # (+1 up to the fp32 sum of the 21 roll probabilities, 1 + 2^-22, which W has as well)
    assert (np.abs(E[:, a, 1:] - 1) < 1e-6).all() and (np.abs(ND[:, a, 1:] - 1) < 1e-6).all()
    assert (E64[:, a, 1:] == 1).all() or (np.abs(E64[:, a, 1:] - 1) < 1e-15).all()
    for s in (0, 1):
        for b in range(1, n):
            v, fl = BO.cube_values_reference(s, ND[s, a, b], E[2, a, b], W[a, b])
            assert np.abs(v - np.array([1, 2, 1, 1])).max() < 1e-6 and fl == 1 and v[2] == v[0]
    # boundaries
    assert (E[:, :, 0] == -1).all() and (E[:, 0, 1:] == 1).all() and (ND[:, :, 0] == -1).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_structure_k3(dtype):
    W, E, ND = CR.references(3, dtype)
    n = W.shape[0]
    assert n == 84
    f = E.dtype.type
    inner = (slice(1, n), slice(1, n))
    cash = np.minimum(f(2) * E[2], f(1))
    for s in (0, 1):
        assert np.array_equal(E[s][inner], np.maximum(ND[s], cash)[inner])
    cl = 2 * W.astype(np.float64) - 1
    e = E.astype(np.float64)
    assert (e[2] <= e[0] + 1e-6)[inner].all() and (e[0] <= e[1] + 1e-6)[inner].all()
    assert (e[2] <= cl + 1e-6)[inner].all() and (cl <= e[1] + 1e-6)[inner].all()
    assert (np.abs(e) <= 1 + 1e-6).all()
    assert (e[1] - e[2])[inner].max() > 0.3                 # owning the cube is worth something somewhere


def test_fp32_against_fp64_k3_numbers():
    """The maxima DESIGN.md §15 quotes (the GPU test bounds the device table by 4 x these)."""
    W32, E32, ND32 = CR.references(3, "float32")
    W64, E64, ND64 = CR.references(3, "float64")
    dist = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((E32, E64), (ND32, ND64), (W32, W64))]
    print("K = 3 fp32 against fp64: equity %.3e nd %.3e W %.3e" % tuple(dist))
    assert all(0 < d < 2e-6 for d in dist), dist
    # the verdicts: double agrees on every pair, take on all but a few (the pairs within rounding of DT = 1)
    dbl = [np.minimum(2 * E[2], 1)[1:, 1:] > ND[0][1:, 1:] for E, ND in ((E32, ND32), (E64, ND64))]
    take = [(2 * E[2] <= 1)[1:, 1:] for E in (E32, E64)]
    print("verdicts that differ: double", int((dbl[0] != dbl[1]).sum()), "take", int((take[0] != take[1]).sum()))
    assert (dbl[0] != dbl[1]).sum() <= 2 and (take[0] != take[1]).sum() <= 2


# ------------------------------------------------------------- summarize_cube_bearoff --
def rows_of(games):
    """games: (kind, y, k, plies, cubeless score signed); kind "end" | "pass" | "cut", y in points
    (a cut game's: a multiple of 2^-20) -> (tally row, cube row, cut row)."""
    t, c, u = np.zeros(8, np.int64), [0] * 8, [0] * 6
    for kind, y, k, plies, res in games:
        if kind == "cut":
            yq = int(round(y * ONE))
            assert yq == y * ONE
            u[0] += 1; u[1] += plies; u[2] += yq; u[3] += (yq * yq) & ((1 << 30) - 1); u[4] += (yq * yq) >> 30; u[5] += k
            continue
        c[0] += 1; c[1] += y; c[2] += y * y; c[3] += k
        if kind == "pass":
            c[4] += 1; c[5] += plies; c[6] += y > 0
        else:
            t[0] += 1; t[1] += plies; t[(2 if res > 0 else 5) + abs(res) - 1] += 1
    return t, c, u


def test_summarize_cube_bearoff_against_numpy():
    games = [("end", 4, 1, 30, 2), ("end", -2, 1, 41, -1), ("pass", 1, 0, 7, 0), ("cut", 0.3125, 0, 12, 0),
             ("cut", -1.75, 1, 20, 0), ("cut", 3.999996185302734375, 2, 33, 0), ("pass", -2, 1, 9, 0)]
    t, c, u = rows_of(games)
    c[7] = 5
    r = C.summarize_cube_bearoff(t, c, u, unfinished=2)
    y = np.array([g[1] for g in games], np.float64)
    assert r["games"] == 7 and r["cut_games"] == 3 and r["cut_share"] == 3 / 7 and r["unfinished"] == 2
    assert r["equity_cubeful"] == pytest.approx(y.mean(), rel=1e-15)
    assert r["equity_cubeful_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(7), rel=1e-12)
    assert r["pass_share"] == 2 / 7 and r["doubles_per_game"] == 5 / 7 and r["cut_plies"] == 65
    assert r["mean_cube_log2"] == pytest.approx(6 / 7) and r["plies_per_game"] == pytest.approx((71 + 16 + 65) / 7)
    assert r["played_out"] == R.summarize(t, 2) and [r[f] for f in C.CUBE_CUT_FIELDS] == u
    assert [r[f] for f in C.CUBE_FIELDS] == c


def test_summarize_cube_bearoff_edge_cases():
    # no cut game: summarize_cube's numbers
    t, c, u = rows_of([("end", 4, 1, 30, 2), ("pass", 1, 0, 7, 0), ("end", -6, 1, 20, -3)])
    r, s = C.summarize_cube_bearoff(t, c, u), C.summarize_cube(t, c)
    assert r["cut_share"] == 0.0 and r["cut_games"] == 0
    for k, v in s.items():
        assert r[k] == pytest.approx(v, rel=1e-12, abs=0) if isinstance(v, float) else r[k] == v, k
    # only cut games of one value: exactly that value, a standard error of exactly 0
    y = 0.8125 + 2.0 ** -20
    t, c, u = rows_of([("cut", y, 0, 3, 0)] * 11)
    r = C.summarize_cube_bearoff(t, c, u)
    assert r["games"] == 11 and r["equity_cubeful"] == y and r["equity_cubeful_stderr"] == 0.0 and r["cut_share"] == 1.0
    # a Y2 sum that needs the HI part: |Yq| = 2^30 (a certain win with the cube at 1024)
    t, c, u = rows_of([("cut", 1024.0, 10, 1, 0), ("cut", -1024.0, 10, 1, 0), ("cut", 1024.0, 10, 2, 0)])
    assert u[3] == 0 and u[4] == 3 << 30
    r = C.summarize_cube_bearoff(t, c, u)
    ys = np.array([1024.0, -1024.0, 1024.0])
    assert r["equity_cubeful"] == ys.mean() and r["equity_cubeful_stderr"] == pytest.approx(ys.std(ddof=1) / math.sqrt(3), rel=1e-15)
    assert r["mean_cube_log2"] == 10.0
    # nothing at all, one game, the mismatch, a short row
    r = C.summarize_cube_bearoff([0] * 8, [0] * 8, [0] * 6)
    assert r["games"] == 0 and r["equity_cubeful"] == 0.0 and r["cut_share"] == 0.0
    t, c, u = rows_of([("cut", -0.5, 0, 4, 0)])
    r = C.summarize_cube_bearoff(t, c, u)
    assert r["games"] == 1 and r["equity_cubeful"] == -0.5 and r["equity_cubeful_stderr"] == 0.0
    t, c, u = rows_of([("end", 2, 1, 5, 1), ("cut", 0.5, 0, 4, 0)])
    c[0] += 1                                              # the cut game counted with the plain ones
    with pytest.raises(ValueError, match="counts 2 games"):
        C.summarize_cube_bearoff(t, c, u)
    c[0] -= 1
    with pytest.raises(ValueError, match="6 entries"):
        C.summarize_cube_bearoff(t, c, u[:5])


# -------------------------------------------------------------------- the cut's replay --
def test_cut_reference_hand_made_trace():
    """Seven lanes on the K = 2 table, cap 2, two games a lane.  Lane 0: a first-ply lane, centred
    (nd, not e).  Lane 1: centred, later ply (e = DT just below 1).  Lane 2: the mover owns the
    cube at 2.  Lane 3: the opponent owns it, and the start mover is the other side (-E_opp x 2).
    Lane 4: a dead cube (k = cap: the cubeless value x 4) on the lane's last game.  Lane 5: a record
    outside the table.  Lane 6: idle."""
    cfg = CR.ordered_configs(2)
    W, E, ND = CR.references(2, "float32")
    a, b = cfg.index(B6), cfg.index(A1)

    def lookup(recs, cube, cap):
        return BO.cube_lookup_reference(recs, np.array(cfg, np.int8), E, ND, W, 2, cube, cap)

    out = np.zeros(64, np.uint8)                           # not in the table: a PLAYER1 checker on point 10
    out[10], out[50], out[24], out[51] = 1, 14, 1, 14
    race = BR.record(B6, A1, 0)                            # PLAYER1 (six-point) on roll against the ace point
    recs = np.stack([race] * 5 + [out, race])
    starts = recs.copy()
    starts[3, 52] = 1
    cube = np.array([0, 0, C.pack(1, 1), C.pack(1, 2), C.pack(2, 1), 0, 0], np.uint8)
    cube0 = np.array([0, 0, C.pack(1, 1), C.pack(1, 2), C.pack(1, 1), 0, 0], np.uint8)
    plies = np.array([0, 3, 2, 5, 7, 4, 1])
    games = np.array([0, 0, 1, 0, 1, 0, 0])
    group = np.array([0, 0, 0, 1, 1, 1, -1])
    ref = C.cube_bearoff_cut_reference(recs, cube, plies, games, np.array([1, 1, 1, 1, 1, 1, 0], np.uint8), starts, group,
                                       2, 2, 2, cube0, lookup)
    q = lambda x: int(np.rint(F(x) * F(ONE)))
    nd, dt, e_opp, cl = ND[0, a, b], F(2) * E[2, a, b], E[2, a, b], F(2) * W[a, b] - F(1)
    assert abs(nd - 0.5) < 1e-6 and dt < 1 and abs(cl - 0.5) < 1e-6
    y = [q(nd), q(dt), 2 * q(E[1, a, b]), -2 * q(e_opp), 4 * q(cl)]
    assert y[1] == ONE and abs(y[0] - ONE // 2) <= 1        # DT rounds to 1 at the fixed point
    want0 = [3, 5, sum(y[:3]), sum(v * v for v in y[:3]) & (2 ** 30 - 1), sum((v * v) >> 30 for v in y[:3]), 1]
    want1 = [2, 12, y[3] + y[4], (y[3] ** 2 & (2 ** 30 - 1)) + (y[4] ** 2 & (2 ** 30 - 1)), (y[3] ** 2 >> 30) + (y[4] ** 2 >> 30), 3]
    assert ref["cut_tally"].tolist() == [want0, want1]
    assert ref["mask"].tolist() == [True] * 5 + [False, False]
    assert ref["games_done"].tolist() == [1, 1, 2, 1, 2, 0, 0] and ref["plies"].tolist() == [0, 0, 0, 0, 0, 4, 1]
    assert ref["sel"].tolist() == [1, 1, 0, 1, 0, 1, 0] and ref["retired"] == 2
    assert ref["cube"].tolist() == cube0.tolist()
    r = C.summarize_cube_bearoff([0] * 8, [0] * 8, ref["cut_tally"][0])
    assert r["games"] == 3 and r["equity_cubeful"] == sum(y[:3]) / (3 * ONE)


def test_cube_state_and_fixed_references():
    st, k = BO.cube_state_reference(np.array([0, 0x11, 0x21, 0x13, 0x3F, 0x31, 0x06], np.uint8), 3, np.array([0, 0, 0, 1, 0, 1, 0]))
    assert st.tolist() == [0, 1, 2, 3, 3, 0, 3] and k.tolist() == [0, 1, 1, 3, 3, 1, 3]
    assert BO.cube_state_reference(0, 0, 0)[0] == 3           # cap 0: dead from the start
    y = BO.cube_fixed_reference(np.array([1.0, -1.0, 1.5, np.nan, 0.5 + 2.0 ** -21, -0.3], np.float32),
                                np.array([True, False, True, True, True, False]), np.array([0, 10, 3, 2, 0, 1]))
    assert y.tolist() == [ONE, ONE << 10, ONE << 3, 0, ONE // 2, 2 * int(np.rint(F(0.3) * F(ONE)))]


# ------------------------------------------------------------------------- the parser --
def test_parser_flags():
    ap = R.build_parser()
    assert ap.parse_args("--net random --positions opening".split()).cube_bearoff is None
    ns = ap.parse_args("--net ckpt.pt --positions opening --cube --cube-bearoff 6".split())
    assert ns.cube and ns.cube_bearoff == 6 and ns.bearoff is None
    assert ap.parse_args("--net ckpt.pt --positions opening --cube --cube-bearoff 3 --cube-decision".split()).cube_decision
    for bad in ("--net ckpt.pt --positions opening --cube-bearoff 6",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 0",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 9",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 6 --luck",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 6 --bearoff 6",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 6 --bearoff1 15",
                "--net ckpt.pt --positions opening --cube --cube-bearoff 6 --truncate 8",
                "--net ckpt.pt --positions opening --cube --bearoff 6",          # the old errors are still errors
                "--net ckpt.pt --positions opening --cube --bearoff1 15"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


# ------------------------------------------------------------------------- the C ABI --
NEW = {"bgx_bearoff_cube_create": 3, "bgx_bearoff_cube_buffers_get": 2, "bgx_bearoff_cube_destroy": 1,
       "bgx_bearoff_cube_lookup": 9, "bgx_rollout_cube_bearoff_cut": 17}


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params) == nargs, name
        for p, a in zip(params, args):                    # pointer / int32, in the header's order
            want = ctypes.POINTER(_lib._P) if "**" in p else _lib._P if "*" in p else _lib._I32
            assert a is want, (name, p)
    # the cut's arguments are bgx_rollout_bearoff_cut's, then cap, cube0, cube
    old = re.search(r"^int\s+bgx_rollout_bearoff_cut\s*\(([^;]*)\);", header, re.M).group(1)
    new = re.search(r"^int\s+bgx_rollout_cube_bearoff_cut\s*\(([^;]*)\);", header, re.M).group(1)
    names = lambda s: [re.findall(r"\w+", p)[-1] for p in s.split(",")]
    assert names(new)[1:] == names(old)[1:10] + ["cube_cut_tally_dev"] + names(old)[11:13] + ["cap", "cube0_dev", "cube_dev", "stream"]
    m = re.search(r"typedef struct \{([^}]*)\} bgx_bearoff_cube_buffers;", header)
    assert re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1))) == [f for f, _ in _lib.BgxBearoffCubeBuffers._fields_]
    fields = re.search(r"enum bgx_rollout_cube_cut_field \{([^}]*)\}", header).group(1)
    got = re.findall(r"BGX_ROLLOUT_CUBE_CUT_(\w+)\s*=\s*(\d+)", fields)
    assert [("cut_" + n.lower(), int(v)) for n, v in got] == [(f, i) for i, f in enumerate(C.CUBE_CUT_FIELDS)]
    # the device code is part 2 of csrc/bg_bearoff_cube.h, compiled with bg_returns.hip after bg_cube.h
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_cube.h"') < src.index('#include "bg_bearoff_cube.h"')
    import __graft_entry__ as G
    assert len(G.HIP_SOURCES) == 7
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integ, name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in NEW:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", x))[0]


def test_part1_host_program(tmp_path):
    """tools/cube_bearoff_host.cpp with AddressSanitizer + UBSan, a program of its own: the state,
    the values, the flags and the cut's fixed point over every cube byte, both movers and start
    movers, caps 0, 1, 3, 6 and 10, plies 0 and 1 and table entries on and beside +-1, and NaN,
    against the numpy forms of bgx/bearoff.py."""
    exe = str(tmp_path / "cube_bearoff_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cube_bearoff_host.cpp"), "-o", exe], check=True)
    up, down = lambda v: float(np.nextafter(F(v), F(np.inf))), lambda v: float(np.nextafter(F(v), F(-np.inf)))
    # (nd_cen, nd_own, e_opp, w)
    entries = [(0.5, 0.5, down(0.5), 0.75), (1.0, 1.0, 1.0, 1.0), (-1.0, -1.0, -1.0, 0.0), (down(1.0), 1.0, 0.5, up(0.5)),
               (0.3, 0.6, 0.5, 0.7), (0.3, 0.6, up(0.5), 0.7), (up(-1.0), down(1.0), down(1.0), down(1.0)),
               (0.25, -0.125, 0.125, 0.4), (math.nan, 0.2, 0.1, 0.5), (0.2, 0.1, math.nan, math.nan),
               (up(1.0), 1.5, 0.75, 1.0), (-0.75, -0.5, -0.25, 0.25), (0.0, 0.0, 0.0, 0.5)]
    byte, cap, mover, start, plies, ent = (x.ravel() for x in np.meshgrid(
        np.arange(256), [0, 1, 3, 6, 10], [0, 1], [0, 1], [0, 1], np.arange(len(entries)), indexing="ij"))
    ev = np.array(entries, np.float32)[ent]
    cases = [f"{b} {c} {m} {s} {p} " + " ".join(bits(float(x)) for x in e)
             for b, c, m, s, p, e in zip(byte, cap, mover, start, plies, ev)]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr and len(cases) == 256 * 5 * 8 * len(entries)
    got = np.array([[int(v, 16) if 3 <= j <= 6 else int(v) for j, v in enumerate(ln.split())]
                    for ln in out.stdout.splitlines()], np.int64)
    assert got.shape == (len(cases), 8)
    seen_states = set()
    for c in (0, 1, 3, 6, 10):
        on = cap == c
        state, k = BO.cube_state_reference(byte[on], c, mover[on])
        seen_states |= set(state.tolist())
        nd_s = np.where(state == 0, ev[on, 0], np.where(state == 1, ev[on, 1], F(0))).astype(np.float32)
        values, flags = BO.cube_values_reference(state, nd_s, ev[on, 2], ev[on, 3])
        v = np.where(plies[on] == 0, values[:, 0], values[:, 2])
        yq = BO.cube_fixed_reference(v, mover[on] == start[on], k)
        g = got[on]
        assert np.array_equal(g[:, 0], state) and np.array_equal(g[:, 1], k) and np.array_equal(g[:, 2], flags), c
        gv, wv = g[:, 3:7].astype(np.uint32).view(np.float32), values
        same = (gv.view(np.uint32) == wv.view(np.uint32)) | (np.isnan(gv) & np.isnan(wv))
        assert same.all(), (c, np.argwhere(~same)[:5].tolist())
        assert np.array_equal(g[:, 7], yq), (c, np.argwhere(g[:, 7] != yq)[:5].tolist())
        assert np.abs(g[:, 7]).max() <= ONE << c
    assert seen_states == {0, 1, 2, 3} and set(got[:, 2].tolist()) >= {0, 1, 3, 4, 5, 7, 8, 12}
