"""The doubling cube's host side (bgx/cube.py, bgx/rollout.py; no GPU): summarize_cube against
numpy, cube_reference on a hand-made trace, the cube0 validation, the command-line flags, the C
ABI's declarations, and part 1 of csrc/bg_cube.h built as a host program (tools/cube_host.cpp)."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from bgx import _lib, cube as C, rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def rule(**kw):
    return C.CubeRule(lambda eng, dsel: None, **kw)


# ------------------------------------------------------------------- summarize_cube --
def rows_of(games):
    """games: (y, k, plies, passed, cubeless score signed) -> (tally row, cube row)."""
    t, c = np.zeros(8, np.int64), np.zeros(8, np.int64)
    for y, k, plies, passed, res in games:
        c[0] += 1; c[1] += y; c[2] += y * y; c[3] += k
        if passed:
            c[4] += 1; c[5] += plies; c[6] += y > 0
        else:
            t[0] += 1; t[1] += plies; t[(2 if res > 0 else 5) + abs(res) - 1] += 1
    return t, c


def test_summarize_cube_against_numpy():
    games = [(4, 1, 30, False, 2), (-2, 1, 41, False, -1), (1, 0, 7, True, 0), (-1, 0, 9, True, 0), (24, 3, 55, False, 3),
             (2, 1, 12, True, 0), (-8, 2, 60, False, -2)]
    t, c = rows_of(games)
    c[7] = 9
    r = C.summarize_cube(t, c, unfinished=3)
    y = np.array([g[0] for g in games], np.float64)
    assert r["games"] == 7 and r["unfinished"] == 3
    assert r["equity_cubeful"] == pytest.approx(y.mean(), rel=1e-15)
    assert r["equity_cubeful_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(7), rel=1e-12)
    assert r["pass_share"] == 3 / 7 and r["doubles_per_game"] == 9 / 7
    assert r["mean_cube_log2"] == pytest.approx(8 / 7) and r["plies_per_game"] == pytest.approx(214 / 7)
    assert r["played_out"] == R.summarize(t, 3) and r["played_out"]["games"] == 4
    assert [r[f] for f in C.CUBE_FIELDS] == c.tolist()


def test_summarize_cube_small_and_mismatch():
    z = np.zeros(8, np.int64)
    r = C.summarize_cube(z, z)
    assert r["games"] == 0 and r["equity_cubeful"] == 0.0 and r["equity_cubeful_stderr"] == 0.0
    assert r["pass_share"] == 0.0 and r["plies_per_game"] == 0.0
    t, c = rows_of([(-6, 1, 20, False, -3)])
    r = C.summarize_cube(t, c)
    assert r["games"] == 1 and r["equity_cubeful"] == -6.0 and r["equity_cubeful_stderr"] == 0.0
    t, c = rows_of([(2, 1, 5, True, 0)])
    assert C.summarize_cube(t, c)["pass_share"] == 1.0
    c[0] += 1
    with pytest.raises(ValueError, match="counts 2 games"):
        C.summarize_cube(t, c)
    with pytest.raises(ValueError, match="8 entries"):
        C.summarize_cube(t, c[:7])
    # equal results: exactly their value, standard error 0
    t, c = rows_of([(2, 1, 5, False, 1)] * 5)
    r = C.summarize_cube(t, c)
    assert r["equity_cubeful"] == 2.0 and r["equity_cubeful_stderr"] == 0.0


# ------------------------------------------------------------------- cube_reference --
def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def test_cube_reference_hand_made_trace():
    """Four lanes, six steps, cap 2, Jacoby on.  Lane 0: no action on the first ply, a take (e
    exactly pass_at... takes), a redouble, the cap, then a lost gammon at 4.  Lane 1: two gammons
    with the cube untouched, reduced to 1 point each.  Lane 2 (cube 2 owned by PLAYER2): a win at
    2, then PLAYER2's double is passed on the lane's last game.  Lane 3 (cube 2 owned by PLAYER1):
    PLAYER2 has no access, a NaN never doubles, e exactly double_at doubles."""
    nan = float("nan")
    ru = rule(double_at=0.4, pass_at=0.5, cap=2, jacoby=True)
    group = np.array([0, 0, 1, 1], np.int32)
    starts = np.zeros((4, 64), np.uint8)
    cube0 = np.array([0, 0, C.pack(1, 2), C.pack(1, 1)], np.uint8)
    mover = np.array([[0, 1, 0, 1, 0, 1], [0, 1, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0], [0, 1, 0, 1, 0, 1]], np.uint8).T
    eq = np.array([[0.45, 0.45, 0.5, 0.9, 0.9, 0.1], [0.0] * 6, [0.9, 0.9, 0.8, 0.9, 0.9, 0.9],
                   [0.9, 0.9, nan, 0.9, F(0.4), 0.9]], np.float32).T
    done, inf = np.zeros((6, 4), np.uint8), np.zeros((6, 4), np.int32)
    for t, i, w, s in ((3, 0, 1, 2), (2, 1, 0, 2), (5, 1, 0, 3), (0, 2, 0, 1), (4, 2, 0, 1)):
        done[t, i], inf[t, i] = 1, info(w, s)
    tr = dict(cube_mover=mover, cube_equity=eq, done=done, info=inf)
    out = C.cube_reference(tr, starts, group, 2, 2, ru, cube0)
    assert out["cube_tally"].tolist() == [[3, -6, 66, 2, 0, 0, 0, 2], [2, 0, 8, 2, 1, 1, 0, 2]]
    assert out["tally"].tolist() == [[3, 10, 0, 1, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0, 0, 0]]
    assert out["games_done"].tolist() == [1, 2, 2, 0] and out["active"] == 2
    assert out["cube"][:, 0].tolist() == [0, 0, C.pack(1, 1), C.pack(2, 2), 0, 0]
    assert out["cube"][:, 3].tolist() == [C.pack(1, 1)] * 5 + [C.pack(2, 2)]
    assert out["cube"][:, 2].tolist() == [C.pack(1, 2)] * 6
    assert np.argwhere(out["mask"]).tolist() == [[2, 2]]
    assert out["dsel"].T.tolist() == [[False, True, True, False, False, True], [False, True, True, False, True, True],
                                      [False, False, True, False, False, False],
                                      [False, False, True, False, True, False]]
    for row, t in zip(out["cube_tally"], out["tally"]):
        C.summarize_cube(t, row)                          # CUBE_GAMES = GAMES + PASS_GAMES
    # Jacoby off: lane 1's gammons count 2 and 3
    out2 = C.cube_reference(tr, starts, group, 2, 2, rule(double_at=0.4, pass_at=0.5, cap=2), cube0)
    assert out2["cube_tally"].tolist() == [[3, -3, 77, 2, 0, 0, 0, 2], [2, 0, 8, 2, 1, 1, 0, 2]]
    # an idle lane and a group outside the rows are never counted
    out3 = C.cube_reference(tr, starts, np.array([0, -1, 5, 1]), 2, 2, ru, cube0)
    assert out3["cube_tally"].tolist() == [[1, -8, 64, 2, 0, 0, 0, 2], [0, 0, 0, 0, 0, 0, 0, 1]]
    assert not out3["dsel"][:, 1:3].any()


def test_decide_reference_rule():
    ru = rule(scale=2.0, double_at=0.4, pass_at=0.5, too_good_at=0.8, cap=3)
    e = np.array([0.19, 0.2, 0.25, 0.26, 0.4, 0.41, np.nan, -1.0], np.float32)
    act, nxt, access = C.decide_reference(np.zeros(8, np.uint8), np.zeros(8, np.int64), e, ru)
    assert act.tolist() == [0, 1, 1, 2, 2, 0, 0, 0] and access.all()
    assert nxt.tolist() == [0, C.pack(1, 2), C.pack(1, 2), 0, 0, 0, 0, 0]
    # the byte as the kernels read it: k above the cap is the cap, owner 3 is centred
    assert C.sanitise(np.array([0x0F, 0x31, 0x25], np.uint8), 3).tolist() == [3, 1, 0x23]


# ----------------------------------------------------------------------- validation --
def test_cube0_validation_messages():
    ok = torch.tensor([0, C.pack(1, 1), C.pack(6, 2), C.pack(3, 1)], dtype=torch.uint8)
    C.validate_cube0(ok, 6)
    for lane, byte, cap in ((2, C.pack(7, 1), 6), (1, C.pack(1, 3), 6), (3, C.pack(0, 1), 6), (0, C.pack(2, 0), 6),
                            (1, C.pack(1, 1), 0)):
        bad = ok.clone() if cap else torch.zeros(4, dtype=torch.uint8)
        bad[lane] = byte
        with pytest.raises(ValueError, match=f"cube0: lane {lane} holds {byte} "):
            C.validate_cube0(bad, cap)
    bad = ok.clone()
    bad[1], bad[3] = C.pack(0, 2), C.pack(9, 1)
    with pytest.raises(ValueError, match="lane 1 "):           # the first bad lane
        C.validate_cube0(bad, 6)


def test_cube_rule_arguments():
    r = rule()
    assert (r.scale, r.double_at, r.pass_at, r.too_good_at, r.cap, r.jacoby) == (1.0, 0.40, 0.50, math.inf, 6, False)
    s = r.struct()
    assert (s.cap, s.jacoby) == (6, 0) and s.double_at == F(0.4) and s.too_good_at == math.inf
    for kw in (dict(scale=math.nan), dict(double_at=math.nan), dict(pass_at=math.nan), dict(cap=11), dict(cap=-1),
               dict(cap=2.5)):
        with pytest.raises(ValueError):
            rule(**kw)
    with pytest.raises(ValueError):
        C.CubeRule(3.0)
    assert "mover's-view" in C.CubeRule.__doc__


# ------------------------------------------------------------------------- the parser --
def test_parser_flags():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.cube is False and ns.cube_decision is False and ns.jacoby is False and ns.cube_net is None
    assert (ns.cube_double, ns.cube_pass, ns.cube_too_good, ns.cube_scale, ns.cube_cap) == (0.40, 0.50, math.inf, 1.0, 6)
    ns = ap.parse_args("--net ckpt.pt --positions opening --cube --cube-double 0.3 --cube-pass 0.6 --cube-too-good 0.9 "
                       "--cube-scale 2 --cube-cap 4 --jacoby --cube-decision".split())
    assert ns.cube and ns.jacoby and ns.cube_decision
    assert (ns.cube_double, ns.cube_pass, ns.cube_too_good, ns.cube_scale, ns.cube_cap) == (0.3, 0.6, 0.9, 2.0, 4)
    assert ap.parse_args("--net random --positions opening --cube --cube-net v.pt".split()).cube_net == "v.pt"
    for bad in ("--net random --positions opening --cube",
                "--net ckpt.pt --positions opening --cube --luck",
                "--net ckpt.pt --positions opening --cube --bearoff 6",
                "--net ckpt.pt --positions opening --cube --bearoff1 15",
                "--net ckpt.pt --positions opening --cube-decision",
                "--net ckpt.pt --positions opening --cube --cube-cap 11",
                "--net ckpt.pt --positions opening --cube --cube-double nan"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


# ------------------------------------------------------------------------- the C ABI --
def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in (("bgx_rollout_cube_begin", 5), ("bgx_rollout_cube_sel", 10), ("bgx_rollout_cube_decide", 18),
                        ("bgx_rollout_cube_flush", 12)):
        assert name in _lib.SIGNATURES
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(params) == nargs, name
        for p, a in zip(params, args):                    # pointer / int32 / the rule by value, in the header's order
            want = _lib._P if "*" in p else _lib.BgxCubeRule if p.startswith("bgx_cube_rule") else _lib._I32
            assert a is want, (name, p)
    m = re.search(r"typedef struct \{([^}]*)\} bgx_cube_rule;", header)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == [f for f, _ in _lib.BgxCubeRule._fields_]
    assert struct.calcsize("4f2i") == 24 == __import__("ctypes").sizeof(_lib.BgxCubeRule)
    fields = re.search(r"enum bgx_rollout_cube_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ROLLOUT_CUBE_(\w+)\s*=\s*(\d+)", fields)
    assert [(("" if n.startswith(("PASS", "DOUBLES")) else "cube_") + n.lower(), int(v)) for n, v in names] == \
        [(f, i) for i, f in enumerate(C.CUBE_FIELDS)]
    # the device code is part 2 of csrc/bg_cube.h, compiled with bg_returns.hip after bg_bearoff1.h
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_bearoff1.h"') < src.index('#include "bg_cube.h"')
    import __graft_entry__ as G
    assert len(G.HIP_SOURCES) == 7
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in _lib.SIGNATURES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def bits(x):
    return "%x" % struct.unpack("<I", struct.pack("<f", x))[0]


def test_decision_rule_host_program(tmp_path):
    """tools/cube_host.cpp with AddressSanitizer + UBSan, a program of its own: cube_decision over
    every state byte's k and owner (the invalid ones too), both movers, five caps, three
    threshold sets and equities on, beside and far from the thresholds, NaN and the infinities,
    against decide_reference."""
    exe = str(tmp_path / "cube_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cube_host.cpp"), "-o", exe], check=True)
    up, down = lambda v: float(np.nextafter(F(v), F(np.inf))), lambda v: float(np.nextafter(F(v), F(-np.inf)))
    rules = [dict(scale=1.0, double_at=0.4, pass_at=0.5, too_good_at=math.inf),
             dict(scale=1.5, double_at=0.3, pass_at=0.6, too_good_at=0.9),
             dict(scale=1.0, double_at=math.inf, pass_at=0.5, too_good_at=math.inf)]
    eqs = [-1.0, 0.0, down(0.4), float(F(0.4)), up(0.4), 0.45, down(0.5), 0.5, up(0.5), float(F(0.2)), float(F(0.4)) / 1.5,
           0.6, up(0.6), 0.95, 3.0, math.nan, math.inf, -math.inf]
    cases, want = [], []
    for ru in rules:
        for cap in (0, 1, 3, 6, 10):
            r = rule(cap=cap, **ru)
            byte = np.repeat(np.arange(64, dtype=np.uint8), 2 * len(eqs))            # k 0..15, owner 0..3
            mover = np.tile(np.repeat(np.arange(2), len(eqs)), 64)
            e = np.tile(np.array(eqs, np.float32), 128)
            act, nxt, access = C.decide_reference(byte, mover, e, r)
            want += list(zip(act.tolist(), nxt.tolist(), access.astype(int).tolist()))
            head = " ".join(bits(r.struct().__getattribute__(f)) for f in ("double_at", "pass_at", "too_good_at"))
            cases += [f"{b} {cap} {m} {bits(r.scale)} {bits(float(x))} {head}" for b, m, x in zip(byte, mover, e)]
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert f"cases {len(cases)}" in out.stderr and len(cases) == 3 * 5 * 64 * 2 * len(eqs)
    got = [tuple(int(v) for v in ln.split()) for ln in out.stdout.splitlines()]
    assert len(got) == len(want)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g[:3] != w]
    assert not bad, bad[:5]
    # every action occurs, and the take's new state is k + 1 owned by the other side
    assert {g[0] for g in got} == {0, 1, 2}
    assert all(g[1] == (g[3] + 1) | ((2 - int(c.split()[2])) << 4) for c, g in zip(cases, got) if g[0] == 1)
    assert all(g[3] <= int(c.split()[1]) and g[4] <= 2 for c, g in zip(cases, got))
