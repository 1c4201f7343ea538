"""The arena's doubling cube on the host (bgx/arena.py, bgx/cube.py; no GPU): summarize's
ppg_stderr and summarize_cube against numpy, arena_cube_reference on a hand-made trace, the
command-line flags, the C ABI's declarations, CubeRule's lookahead, and part 1 of
csrc/bg_arena_cube.h built as a host program (tools/arena_cube_host.cpp)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bgx import _lib, arena as A, cube as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")


def rule(**kw):
    return C.CubeRule(lambda eng, dsel: None, **kw)


def plain_tally(results):
    """results: (x = +-1 / 2 / 3 from A's side, a_p1) per game -> the 16 plain entries."""
    t = dict.fromkeys(A.FIELDS, 0)
    for x, a_p1 in results:
        s = "a" if x > 0 else "b"
        t["games"] += 1
        t["wins_" + s] += 1
        t["points_" + s] += abs(x)
        if abs(x) == 2:
            t["gammons_" + s] += 1
        if abs(x) == 3:
            t["backgammons_" + s] += 1
        t["games_a_p1"] += a_p1
        t["wins_a_p1"] += a_p1 and x > 0
        t["wins_p1"] += (x > 0) == bool(a_p1)
    return [t[f] for f in A.FIELDS] + [0, 0]


# ---------------------------------------------------------------------- summaries --
def test_ppg_stderr_against_numpy():
    xs = [1, 1, -1, 2, -2, 3, -3, -1, 1, 2, 1, -1, -1]
    r = A.summarize(plain_tally([(x, i & 1) for i, x in enumerate(xs)]), steps=9, unfinished=0)
    x = np.array(xs, np.float64)
    assert r["ppg_a"] == pytest.approx(x.mean(), rel=1e-15)
    assert r["ppg_stderr"] == pytest.approx(x.std(ddof=1) / math.sqrt(len(xs)), rel=1e-12)
    # every earlier key is still there
    assert {"win_rate_a", "win_rate_stderr", "ppg_a", "steps", "unfinished_lanes", *A.FIELDS} <= set(r)
    assert A.summarize([0] * 16, 0, 0)["ppg_stderr"] == 0.0
    assert A.summarize(plain_tally([(3, 1)]), 1, 0)["ppg_stderr"] == 0.0
    assert A.summarize(plain_tally([(2, 1)] * 7), 1, 0)["ppg_stderr"] == 0.0          # equal results


def cube_tallies(games, doubles=(0, 0)):
    """games: (y from A's side, k, plies, passed by: None / "a" / "b", cubeless x) -> (tally, cube tally)."""
    c = dict.fromkeys(A.CUBE_FIELDS, 0)
    played = []
    for y, k, plies, passed, x in games:
        c["cube_games"] += 1; c["cube_points_a"] += y; c["cube_points2"] += y * y; c["cube_wins_a"] += y > 0
        c["cube_log2"] += k
        if passed:
            c["pass_games"] += 1; c["pass_plies"] += plies; c["passes_" + passed] += 1
        else:
            played.append((x, 1))
    c["doubles_a"], c["doubles_b"] = doubles
    return plain_tally(played), [c[f] for f in A.CUBE_FIELDS] + [0] * 5


def test_summarize_cube_against_numpy():
    games = [(4, 1, 30, None, 2), (-2, 1, 41, None, -1), (1, 0, 7, "b", 0), (-1, 0, 9, "a", 0), (24, 3, 55, None, 3),
             (2, 1, 12, "b", 0), (-8, 2, 60, None, -2)]
    t, c = cube_tallies(games, doubles=(6, 4))
    r = A.summarize_cube(t, c, steps=77, unfinished=3)
    y = np.array([g[0] for g in games], np.float64)
    assert r["games"] == 7 and r["steps"] == 77 and r["unfinished_lanes"] == 3
    assert r["ppg_cubeful_a"] == pytest.approx(y.mean(), rel=1e-15)
    assert r["ppg_cubeful_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(7), rel=1e-12)
    assert r["win_rate_cubeful_a"] == 4 / 7 and r["pass_share"] == 3 / 7
    assert r["doubles_per_game_a"] == 6 / 7 and r["doubles_per_game_b"] == 4 / 7
    assert r["take_share_a"] == 1 - 1 / 4 and r["take_share_b"] == 1 - 2 / 6
    assert r["mean_cube_log2"] == pytest.approx(8 / 7)
    assert r["played_out"] == A.summarize(t, 77, 3) and r["played_out"]["games"] == 4
    assert [r[f] for f in A.CUBE_FIELDS] == c[:11]


def test_summarize_cube_small_and_mismatch():
    r = A.summarize_cube([0] * 16, [0] * 16, 0, 5)
    assert r["games"] == 0 and r["ppg_cubeful_a"] == 0.0 and r["ppg_cubeful_stderr"] == 0.0
    assert r["pass_share"] == 0.0 and r["take_share_a"] == 0.0 and r["unfinished_lanes"] == 5
    t, c = cube_tallies([(-6, 1, 20, None, -3)], doubles=(0, 1))
    r = A.summarize_cube(t, c, 20, 0)
    assert r["games"] == 1 and r["ppg_cubeful_a"] == -6.0 and r["ppg_cubeful_stderr"] == 0.0
    assert r["take_share_a"] == 1.0 and r["take_share_b"] == 0.0
    t, c = cube_tallies([(2, 1, 5, "b", 0)], doubles=(2, 1))
    assert A.summarize_cube(t, c, 5, 0)["pass_share"] == 1.0
    bad = list(c)
    bad[0] += 1                                               # CUBE_GAMES != GAMES + PASS_GAMES
    with pytest.raises(ValueError, match="counts 2 games"):
        A.summarize_cube(t, bad, 5, 0)
    bad = list(c)
    bad[A.CUBE_FIELDS.index("passes_a")] += 1                 # PASS_GAMES != PASSES_A + PASSES_B
    with pytest.raises(ValueError, match="passed games"):
        A.summarize_cube(t, bad, 5, 0)
    with pytest.raises(ValueError, match="entries"):
        A.summarize_cube(t, c[:10], 5, 0)


# ----------------------------------------------------------- arena_cube_reference --
def info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def hand_trace():
    """Six lanes, eight steps, two games a lane.  A: double 0.4, pass 0.5, too good 0.8.  B: scale 2,
    double 0.3, pass 0.6.  Cap 2.  A is PLAYER1 (mover 0) in game g of lane i iff i + g is even.
    Lane 0: no action on the first ply; B doubles, A takes; B has no access to A's cube; A is too
      good; A redoubles, B takes; the cap; B wins a gammon at 4: -8.  Game 2: first ply, a NaN.
    Lane 1: A doubles, B passes (+1); the seats flip -- mover 0 is now A --, A doubles again, B
      passes the lane's last game.  A later done of the retired lane counts nothing.
    Lane 2: two gammons with the cube untouched: Jacoby makes them +1 and -1.
    Lane 3: B doubles, A passes (-1); after the flip A doubles at exactly double_at, B takes at
      exactly pass_at, B redoubles, A takes, the cap holds, A wins a single at 4.
    Lane 4: a done without a winner only resets cube and plies; then a lost gammon at 2: -4; the
      second game's -inf never doubles.
    Lane 5: B takes on a NaN; B redoubles on +inf, A passes (-2); A doubles, B passes (+1)."""
    mover = np.array([[0, 1, 1, 0, 0, 1, 0, 1], [0, 1, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 1, 0, 1, 0],
                      [0, 1, 0, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 0, 0, 0]], np.uint8).T
    eq_offer = np.array([[.45, .2, .9, .9, .5, .9, .9, NAN], [.9, .6, .45, .9, .9, .9, .9, .9],
                         [0, 0, .1, .3, .9, .1, .3, .1], [.9, .2, .4, F(.4), .5, .9, .9, .9],
                         [.9, .3, .3, .9, .7, .1, .9, -INF], [.9, .5, INF, .1, .41, .9, .9, .9]], np.float32).T
    eq_resp = np.full((8, 6), NAN, np.float32)
    for t, i, v in ((1, 0, .45), (4, 0, .25), (1, 1, .35), (2, 1, .31), (2, 3, .55), (3, 3, .3), (4, 3, .5), (1, 4, .1),
                    (4, 4, .2), (2, 5, .6), (4, 5, .9)):
        eq_resp[t, i] = v
    done, inf = np.zeros((8, 6), np.uint8), np.zeros((8, 6), np.int32)
    for t, i, w, s in ((5, 0, 1, 2), (4, 1, 0, 1), (3, 2, 0, 2), (7, 2, 0, 3), (7, 3, 0, 1), (2, 4, -1, 0), (5, 4, 1, 2)):
        done[t, i], inf[t, i] = 1, info(w, s)
    return dict(cube_mover=mover, eq_offer=eq_offer, eq_resp=eq_resp, done=done, info=inf)


def hand_rules(jacoby=True):
    return (rule(double_at=0.4, pass_at=0.5, too_good_at=0.8, cap=2, jacoby=jacoby),
            rule(scale=2.0, double_at=0.3, pass_at=0.6, cap=2, jacoby=jacoby))


def test_reference_hand_made_trace():
    tr = hand_trace()
    out = A.arena_cube_reference(tr, 6, 2, *hand_rules())
    P = C.pack
    #                                  games pts  pts2 wins log2 pass plies pa pb da db
    assert out["cube_tally"].tolist() == [10, -8, 106, 5, 6, 5, 8, 2, 3, 7, 5, 0, 0, 0, 0, 0]
    #                             games wa wb pa pb ga gb ba bb ap1 wap1 wp1 plies active
    assert out["tally"].tolist() == [5, 2, 3, 3, 7, 1, 2, 0, 1, 4, 2, 3, 38, 2, 0, 0]
    assert out["games_done"].tolist() == [1, 2, 2, 2, 1, 2]
    assert out["dsel"][:, 0].tolist() == [0, 2, 0, 1, 1, 0, 0, 1]              # first ply, owner, cap
    assert out["offer"][:, 0].tolist() == [0, 2, 0, 0, 1, 0, 0, 0]             # too good at 3, NaN at 7
    assert out["cube"][:, 0].tolist() == [0, 0, P(1, 1), P(1, 1), P(1, 1), P(2, 2), 0, 0]
    assert out["cube"][:, 3].tolist() == [0, 0, 0, 0, P(1, 2), P(2, 1), P(2, 1), P(2, 1)]
    assert out["cube"][:, 4].tolist() == [0, 0, P(1, 1), 0, 0, P(1, 2), 0, 0]  # a done without a winner resets
    assert out["cube"][:, 5].tolist() == [0, 0, P(1, 1), 0, 0, 0, 0, 0]
    assert np.argwhere(out["passed"]).tolist() == [[1, 1], [2, 1], [2, 3], [2, 5], [4, 5]]
    # the seat flip after a pass: lane 1's mover 0 is B in game 1, A in game 2
    assert out["dsel"][:, 1].tolist() == [0, 1, 1, 0, 0, 0, 0, 0] and out["offer"][:, 1].tolist() == [0, 1, 1] + [0] * 5
    assert out["dsel"][:, 3].tolist() == [0, 1, 2, 1, 2, 0, 0, 0]
    res = A.summarize_cube(out["tally"], out["cube_tally"], 8, 2)              # both invariants hold
    assert res["games"] == 10 and res["ppg_cubeful_a"] == -0.8 and res["pass_share"] == 0.5
    assert res["take_share_a"] == 1 - 2 / 5 and res["take_share_b"] == 1 - 3 / 7
    # Jacoby off: lane 2's gammon and backgammon count 2 and 3
    out2 = A.arena_cube_reference(tr, 6, 2, *hand_rules(jacoby=False))
    assert out2["cube_tally"].tolist() == [10, -9, 117, 5, 6, 5, 8, 2, 3, 7, 5, 0, 0, 0, 0, 0]
    assert out2["tally"].tolist() == out["tally"].tolist()
    # a side without a rule never doubles and takes everything
    out3 = A.arena_cube_reference(tr, 6, 2, None, hand_rules()[1])
    assert out3["cube_tally"][A.CUBE_FIELDS.index("doubles_a")] == 0
    assert out3["cube_tally"][A.CUBE_FIELDS.index("passes_a")] == 0
    # one game a lane: every lane retires after its first game
    out4 = A.arena_cube_reference(tr, 6, 1, *hand_rules())
    assert out4["games_done"].tolist() == [1] * 6 and out4["tally"][A.ACTIVE] == 0
    A.summarize_cube(out4["tally"], out4["cube_tally"], 8, 0)


def test_arena_cube_rules():
    ra, rb = hand_rules()
    ac = A.ArenaCube(ra, rb)
    assert (ac.cap, ac.jacoby, ac.has_a, ac.has_b) == (2, True, True, True) and not ac.sync_free
    with pytest.raises(ValueError, match="belong to the game"):
        A.ArenaCube(ra, rule(cap=3, jacoby=True))
    with pytest.raises(ValueError, match="belong to the game"):
        A.ArenaCube(ra, rule(cap=2, jacoby=False))
    with pytest.raises(ValueError, match="CubeRule or None"):
        A.ArenaCube(ra, 0.5)
    one = A.ArenaCube(None, rb)
    assert (one.cap, one.jacoby, one.has_a) == (2, True, False)
    assert one.rule_a.double_at == INF and one.rule_a.pass_at == INF and one.rule_a.sync_free
    none = A.ArenaCube()
    assert none.cap == 6 and none.jacoby is False and none.sync_free


def test_kernel_state_reaches_every_branch():
    """The hand-set state of tests/test_gpu_arena_cube.py's kernel test, on the scalar rule alone:
    every branch and every counted field is reached, and the invariants hold."""
    import arena_cube_ref as ref
    out, seen = ref.run_reference()
    assert seen == ref.BRANCHES, (sorted(ref.BRANCHES - seen), sorted(seen - ref.BRANCHES))
    ct = out["ct_flush"]
    assert ref.CUBE_FIELDS == A.CUBE_FIELDS and all(ct[:11] != 0) and not ct[11:].any(), ct
    assert out["tally"][A.ACTIVE] < int((out["state0"]["games_done"] < ref.G).sum())       # lanes retired by a pass
    assert ct[5] == ct[7] + ct[8] == int(out["mask"].sum())
    # two blocks and a partial last wave, as the kernels are launched
    assert ref.N > 256 and ref.N % 64 != 0


# ------------------------------------------------------------------- the cube rule --
def test_cube_rule_lookahead_arguments():
    r = rule()
    assert r.lookahead == 1 and r.sync_free is False
    assert rule(lookahead=0).lookahead == 0 and rule(lookahead=0).sync_free is False    # a callable declares it

    class Declared:
        sync_free = True

        def __call__(self, eng, dsel):
            return None

    assert C.CubeRule(Declared()).sync_free is True
    for bad in (2, -1, True, None, 0.5, "0"):
        with pytest.raises(ValueError, match="lookahead"):
            rule(lookahead=bad)
    assert "lookahead" in C.CubeRule.__doc__ and "bgx_value_lanes" in C.CubeRule.__doc__


# ------------------------------------------------------------------------ the parser --
def test_parser_flags():
    ap = A.build_parser()
    ns = ap.parse_args("--a a.pt --b b.pt --max-steps 10".split())
    assert ns.cube is False and ns.jacoby is False and ns.cube_cap == 6
    ns = ap.parse_args("--a a.pt --b b.pt --max-steps 10 --cube".split())
    for side in "ab":
        assert [getattr(ns, f"{k}_{side}") for k in A.CUBE_SIDE_DEFAULTS] == [0.40, 0.50, math.inf, 1.0, None, 1]
    ns = ap.parse_args("--a a.pt --b b.pt --max-steps 10 --cube --cube-cap 4 --jacoby --cube-double-a 0.3 --cube-pass-a 0.6 "
                       "--cube-too-good-a 0.9 --cube-scale-a 2 --cube-net-a v.pt --cube-lookahead-a 0 "
                       "--cube-double-b 0.2 --cube-lookahead-b 1".split())
    assert ns.cube and ns.jacoby and ns.cube_cap == 4
    assert (ns.cube_double_a, ns.cube_pass_a, ns.cube_too_good_a, ns.cube_scale_a, ns.cube_net_a,
            ns.cube_lookahead_a) == (0.3, 0.6, 0.9, 2.0, "v.pt", 0)
    assert (ns.cube_double_b, ns.cube_pass_b, ns.cube_lookahead_b) == (0.2, 0.50, 1)
    # a random side has no rule; the other side keeps its options
    ns = ap.parse_args("--a a.pt --b random --max-steps 10 --cube --cube-double-a 0.3".split())
    assert ns.cube_double_a == 0.3
    assert ap.parse_args("--a random --b random --max-steps 10 --cube".split()).cube
    for bad in ("--a a.pt --b b.pt --max-steps 10 --cube-double-a 0.3",
                "--a a.pt --b b.pt --max-steps 10 --cube-lookahead-b 0",
                "--a a.pt --b b.pt --max-steps 10 --cube-net-a v.pt",
                "--a a.pt --b b.pt --max-steps 10 --jacoby",
                "--a a.pt --b b.pt --max-steps 10 --cube-cap 4",
                "--a a.pt --b b.pt --max-steps 10 --cube --cube-cap 11",
                "--a a.pt --b b.pt --max-steps 10 --cube --cube-lookahead-a 2",
                "--a a.pt --b b.pt --max-steps 10 --cube --cube-pass-b nan",
                "--a a.pt --b random --max-steps 10 --cube --cube-double-b 0.3",
                "--a random --b b.pt --max-steps 10 --cube --cube-net-a v.pt",
                "--a random --b b.pt --max-steps 10 --cube --cube-lookahead-a 0"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


# ------------------------------------------------------------------------- the C ABI --
ENTRIES = (("bgx_arena_cube_begin", 5), ("bgx_arena_cube_sel", 10), ("bgx_arena_cube_offer", 13),
           ("bgx_arena_cube_respond", 18), ("bgx_arena_cube_reseat", 8), ("bgx_arena_cube_flush", 12))


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
            want = _lib._P if "*" in p else _lib.BgxCubeRule if p.startswith("bgx_cube_rule") else _lib._I32
            assert a is want, (name, p)
    fields = re.search(r"enum bgx_arena_cube_field \{([^}]*)\}", header).group(1)
    names = re.findall(r"BGX_ARENA_CUBE_(\w+)\s*=\s*(\d+)", fields)
    assert [(("" if n.startswith(("PASS", "DOUBLES")) else "cube_") + n.lower(), int(v)) for n, v in names] == \
        [(f, i) for i, f in enumerate(A.CUBE_FIELDS)]
    # the device code is part 2 of csrc/bg_arena_cube.h, compiled with bg_returns.hip after bg_cube.h
    src = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_returns.hip")).read()
    assert 0 < src.index('#include "bg_cube.h"') < src.index('#include "bg_arena_cube.h"')
    eng = open(os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc", "bg_engine.hip")).read()
    assert "bg_arena_cube.h" not in eng
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name, _ in ENTRIES:
            assert hasattr(lib, name), name


# ------------------------------------------------------- part 1 on the host, sanitised --
def test_offer_respond_identity_host_program(tmp_path):
    """tools/arena_cube_host.cpp with AddressSanitizer + UBSan, a program of its own: cube_offers
    followed by cube_passes / cube_taken is cube_decision, over every byte, both movers, the caps
    0..10, four threshold sets and 22 equities each."""
    exe = str(tmp_path / "arena_cube_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tools", "arena_cube_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    m = re.fullmatch(r"cases (\d+) none (\d+) take (\d+) pass (\d+)\n", out.stdout)
    assert m, out.stdout
    cases, none, take, pas = (int(v) for v in m.groups())
    assert cases == 4 * 11 * 256 * 2 * 22 == none + take + pas and min(none, take, pas) > 0
