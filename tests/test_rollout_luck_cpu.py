"""CPU-side checks of the luck-adjusted rollout (bgx/rollout.py summarize_luck and
luck_tally_reference, the three C entry points' declarations, the command line): no GPU."""
import math
import os
import re

import numpy as np
import pytest

from bgx import _lib
from bgx import rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536


def rows_of(res, L):
    """(tally row, luck row) of explicit games: res in +-(1|2|3), L a multiple of 2^-16."""
    res = np.asarray(res, np.int64)
    lq = np.rint(np.asarray(L, np.float64) * ONE).astype(np.int64)
    assert np.array_equal(lq / ONE, np.asarray(L, np.float64))
    t = [len(res), 7 * len(res)] + [int((res == k).sum()) for k in (1, 2, 3, -1, -2, -3)]
    return t, [int(lq.sum()), int((lq * lq).sum()), int((res * lq).sum()), len(res)]


def games(n, seed):
    rng = np.random.RandomState(seed)
    res = rng.choice([1, 2, 3, -1, -2, -3], n, p=[0.4, 0.1, 0.02, 0.35, 0.1, 0.03])
    # luck correlated with the result, in another unit (the net's reward scale), quantised
    L = np.rint((0.3 * res + rng.normal(0, 0.2, n)) * ONE) / ONE
    return res, L


@pytest.mark.parametrize("scale", [1.0, 0.0, 2.5, "fit"])
def test_summarize_luck_against_numpy(scale):
    res, L = games(500, 3)
    t, k = rows_of(res, L)
    r = R.summarize_luck(t, k, scale, unfinished=2)
    base = R.summarize(t, 2)
    for key, v in base.items():
        assert r[key] == v, key
    c = np.cov(res, L, ddof=1)[0, 1] / np.var(L, ddof=1) if scale == "fit" else float(scale)
    y = res - c * L
    assert r["luck_scale"] == pytest.approx(c, rel=1e-10, abs=1e-15)
    assert r["luck_mean"] == pytest.approx(L.mean(), rel=1e-12)
    assert r["equity_luck"] == pytest.approx(y.mean(), rel=1e-10, abs=1e-13)
    assert r["equity_luck_stderr"] == pytest.approx(y.std(ddof=1) / math.sqrt(len(y)), rel=1e-8)
    assert r["variance_ratio"] == pytest.approx(y.var(ddof=1) / res.var(ddof=1), rel=1e-8)
    if scale == 0.0:
        assert r["equity_luck"] == base["equity"] and r["variance_ratio"] == 1.0
        assert r["equity_luck_stderr"] == pytest.approx(base["equity_stderr"], rel=1e-12)
    if scale == "fit":                       # the fitted scale never does worse than none on its own games
        assert r["variance_ratio"] < 0.5 and r["equity_luck_stderr"] < base["equity_stderr"]


def test_summarize_luck_corner_cases():
    res, _ = games(64, 1)
    t, k = rows_of(res, np.zeros(64))                        # L == 0: nothing to fit, nothing changes
    for scale in ("fit", 1.0):
        r = R.summarize_luck(t, k, scale)
        assert r["equity_luck"] == r["equity"] and r["variance_ratio"] == 1.0 and r["luck_mean"] == 0.0
        assert r["equity_luck_stderr"] == pytest.approx(r["equity_stderr"], rel=1e-12)
    assert R.summarize_luck(t, k, "fit")["luck_scale"] == 0.0
    # a constant result: the fit is c = 0, the equity exact, the stderr 0
    _, L = games(64, 2)
    t, k = rows_of(np.full(64, 2), L)
    r = R.summarize_luck(t, k, "fit")
    assert r["luck_scale"] == 0.0 and r["equity_luck"] == 2.0 and r["equity_luck_stderr"] == 0.0
    assert r["variance_ratio"] == 1.0
    # no game, one game
    z = R.summarize_luck([0] * 8, [0] * 4)
    assert z["games"] == 0 and z["equity_luck"] == 0.0 and z["equity_luck_stderr"] == 0.0 and z["luck_scale"] == 0.0
    assert z["variance_ratio"] == 1.0 and z["luck_mean"] == 0.0
    t, k = rows_of([-2], [0.25])
    one = R.summarize_luck(t, k, 1.0)
    assert one["equity_luck"] == -2.25 and one["equity_luck_stderr"] == 0.0
    assert R.summarize_luck(t, k, "fit")["equity_luck"] == -2.0
    # the two rows must count the same games
    with pytest.raises(ValueError):
        R.summarize_luck(t, [k[0], k[1], k[2], 2])
    with pytest.raises(ValueError):
        R.summarize_luck(t, k[:3])


def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name, nargs in (("bgx_roll_luck", 9), ("bgx_rollout_luck_add", 8), ("bgx_rollout_luck_flush", 10)):
        assert name in _lib.SIGNATURES
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert R.LUCK_FIELDS == ("luck", "luck2", "resluck", "luck_games") and len(R.FIELDS) == 8
    assert re.search(r"BGX_ROLLOUT_LUCK_GAMES\s*=\s*3", header)


def test_luck_workspace_layout(tmp_path):
    """LuckLayout (csrc/bg_workspace.h) on the host, a stand-alone program under ASan + UBSan."""
    import subprocess
    exe = str(tmp_path / "luck_workspace_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "mlp-ppo-2ply-p3_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "luck_workspace_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "luck workspace ok" in r.stdout and "runtime error" not in r.stderr


def test_parser():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening".split())
    assert ns.luck is False and ns.luck_scale == "fit"
    assert (ns.player, ns.first_roll, ns.trials, ns.batch, ns.top_k) == ("policy", "stratified", 1296, 4096, None)
    ns = ap.parse_args("--net ckpt.pt --positions opening --luck".split())
    assert ns.luck is True and ns.luck_scale == "fit"
    ns = ap.parse_args("--net ckpt.pt --positions opening --luck --luck-scale 0.5".split())
    assert ns.luck_scale == 0.5
    assert ap.parse_args("--net ckpt.pt --positions opening --luck --luck-scale fit".split()).luck_scale == "fit"
    for bad in ("--net random --positions opening --luck",
                "--net ckpt.pt --positions opening --luck --luck-scale best",
                "--net ckpt.pt --positions opening --luck --luck-scale nan"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def _info(winner, score):
    return ((winner + 1) << 8) | (score << 16)


def test_luck_tally_reference_hand_trace():
    """Three lanes, four steps.  Lane 0 (start mover 0, drawn first roll) plays two games; lane
    1 (start mover 1, first roll fixed by its start record) one; lane 2 is idle."""
    f = np.float32
    starts = np.zeros((3, 64), np.uint8)
    starts[1, 52] = 1
    starts[1, 53:55] = (3, 1)
    group = np.array([1, 0, -1], np.int32)
    nan = np.nan
    # lane 0: game 1 = steps 0, 1 (movers 0, 1; won 2 points); game 2 = step 2 (a tie in
    # rint: 1.5 * 2^-16 -> 2, half to even); then retired (G = 2): step 3 is ignored.
    # lane 1: step 0 left out (fixed roll), a done without a winner at step 1 zeroes the sum,
    # steps 2, 3 (movers 1, 0): lost 3 points with the sum beyond the clamp.
    luck = np.array([[0.1, 5.0, nan], [0.7, 9.0, nan], [1.5 / ONE, 40.0, nan], [3.0, -1.0, nan]], f)
    mover = np.array([[0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
    done = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 0], [1, 1, 1]], np.uint8)
    info = np.array([[0, 0, 0], [_info(0, 2), 0, 0], [_info(1, 1), 0, 0], [_info(0, 1), _info(0, 3), _info(0, 1)]],
                    np.int32)
    got = R.luck_tally_reference(luck, mover, done, info, starts, group, 2, 2)
    # lane 0, game 1: fp32(0.1) - fp32(0.7) in fp32, times 65536 in fp32, to nearest
    l1 = int(np.rint(f(f(f(0.0) + f(0.1)) - f(0.7)) * f(ONE)))
    assert l1 == int(np.rint((float(f(0.1)) - float(f(0.7))) * ONE)) == -39322
    # lane 1: +40 as mover 1 (its start mover), then -(-1): 41 points, clamped to 32
    want = np.array([[1 << 21, 1 << 42, -3 * (1 << 21), 1],
                     [l1 + 2, l1 * l1 + 4, 2 * l1 - 1 * 2, 2]], np.int64)
    assert np.array_equal(got, want), (got, want)
    # non-finite sums count as 0
    luck[2, 1] = np.inf
    got = R.luck_tally_reference(luck, mover, done, info, starts, group, 2, 2)
    assert np.array_equal(got[0], [0, 0, 0, 1]) and np.array_equal(got[1], want[1])
    # round half to even the other way: 2.5 * 2^-16 -> 2
    got = R.luck_tally_reference(np.array([[2.5 / ONE]], f), np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8),
                                 np.array([[_info(0, 1)]], np.int32), np.zeros((1, 64), np.uint8),
                                 np.zeros(1, np.int32), 1, 1)
    assert np.array_equal(got, [[2, 4, 2, 1]])
