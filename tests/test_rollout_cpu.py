"""CPU-side checks of the rollout module (bgx/rollout.py) and of the start-table record
rules (bgx.engine.validate_starts): no GPU needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

from bgx import _lib
from bgx import rollout as R
from bgx.engine import validate_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ summarize --
def test_summarize_equity_and_stderr():
    # games, plies, win1..3, loss1..3
    row = [100, 640, 40, 10, 2, 30, 15, 3]
    r = R.summarize(row, unfinished=4)
    assert r["games"] == 100 and r["unfinished"] == 4 and r["plies_per_game"] == 6.4
    eq = (40 + 2 * 10 + 3 * 2 - 30 - 2 * 15 - 3 * 3) / 100
    assert r["equity"] == pytest.approx(eq, abs=1e-15)
    sq = 40 + 30 + 4 * (10 + 15) + 9 * (2 + 3)
    assert r["equity_stderr"] == pytest.approx(math.sqrt((sq - 100 * eq * eq) / 99 / 100), rel=1e-12)
    assert r["win"] == 0.52 and r["win_gammon"] == 0.12 and r["win_backgammon"] == 0.02
    assert r["loss"] == 0.48 and r["loss_gammon"] == 0.18 and r["loss_backgammon"] == 0.03
    # the same from the games themselves
    x = np.repeat([1, 2, 3, -1, -2, -3], row[2:]).astype(np.float64)
    assert r["equity"] == pytest.approx(x.mean(), abs=1e-15)
    assert r["equity_stderr"] == pytest.approx(x.std(ddof=1) / math.sqrt(100), rel=1e-12)


def test_summarize_no_games_and_one_game():
    z = R.summarize([0] * 8)
    assert z["games"] == 0
    assert all(z[k] == 0.0 for k in ("equity", "equity_stderr", "win", "loss", "win_gammon", "loss_gammon",
                                     "win_backgammon", "loss_backgammon", "plies_per_game"))
    one = R.summarize([1, 7, 0, 0, 0, 0, 1, 0])
    assert one["equity"] == -2.0 and one["equity_stderr"] == 0.0 and one["loss_gammon"] == 1.0
    assert one["plies_per_game"] == 7.0
    allsame = R.summarize([50, 50, 0, 50, 0, 0, 0, 0])
    assert allsame["equity"] == 2.0 and allsame["equity_stderr"] == 0.0
    with pytest.raises(ValueError):
        R.summarize([0] * 7)


# --------------------------------------------------------------------- layout --
def _unit_lanes(group, roll):
    """{(position, r0, r1): lanes} over every pass."""
    out = {}
    for k in range(group.shape[0]):
        for g, (a, b) in zip(group[k], roll[k]):
            if g >= 0:
                out[(int(g), int(a), int(b))] = out.get((int(g), int(a), int(b)), 0) + 1
    return out


@pytest.mark.parametrize("P,trials,batch", [(1, 72, 128), (3, 100, 128), (2, 36, 4096), (1, 37, 64), (5, 36, 64),
                                            (1, 36 * 1000, 256)])
def test_layout_stratified(P, trials, batch):
    group, roll, G, passes = R.layout(P, trials, "stratified", batch)
    assert group.shape == (passes, batch) and roll.shape == (passes, batch, 2) and group.dtype == np.int32
    units = _unit_lanes(group, roll)
    # every (position, ordered roll) pair, each with the same number of lanes
    assert set(units) == {(p, a, b) for p in range(P) for a in range(1, 7) for b in range(1, 7)}
    lanes = set(units.values())
    assert len(lanes) == 1
    per_roll = lanes.pop() * G
    share = -(-trials // 36)                        # trials rounded up to a multiple of 36
    assert per_roll >= share and per_roll - share < units[(0, 1, 1)]
    if share <= batch // min(36 * P, batch):        # the share fits on lanes: exactly one game each
        assert G == 1 and per_roll == share
    # idle lanes only behind the used ones; a pass holds whole lanes of a unit side by side
    for k in range(passes):
        used = group[k] >= 0
        assert not used[np.argmin(used):].any() or used.all()
        assert (np.diff(group[k][used]) >= 0).all()


def test_layout_random_and_spill():
    group, roll, G, passes = R.layout(2, 1000, "random", 64)
    assert not roll.any()                                   # roll bytes 0: drawn at every reset
    assert passes == 1 and (group[0] >= 0).sum() * G >= 2000
    assert (np.bincount(group[0][group[0] >= 0]) * G >= 1000).all()
    assert G == -(-1000 // 32)                              # 32 lanes per position: several games per lane
    # more games than lanes: games per lane first, one pass
    _, _, G, passes = R.layout(1, 36 * 50, "stratified", 72)
    assert (G, passes) == (25, 1)
    # more units than lanes: several passes, one lane per unit
    group, _, G, passes = R.layout(4, 72, "stratified", 100)
    assert (G, passes) == (2, 2) and (group >= 0).sum() == 144
    with pytest.raises(ValueError):
        R.layout(1, 36, "fixed", 64)
    with pytest.raises(ValueError):
        R.layout(0, 36, "random", 64)


# --------------------------------------------------------- record validation --
def _bearoff():
    r = torch.zeros(1, 64, dtype=torch.uint8)
    r[0, 18] = 1
    r[0, 50] = 14
    r[0, 24] = 1
    r[0, 51] = 14
    return r


def test_validate_starts_accepts():
    validate_starts(_bearoff())
    validate_starts(R.opening_record()[None])
    ok = _bearoff()
    ok[0, 53:55] = torch.tensor([6, 6], dtype=torch.uint8)
    ok[0, 55:] = 255                                         # bytes 55..63 are ignored
    validate_starts(ok)


@pytest.mark.parametrize("name,edit,why", [
    ("14 checkers", lambda r: r[0].__setitem__(50, 13), "sum to 15"),
    ("shared point", lambda r: (r[0].__setitem__(42, 1), r[0].__setitem__(51, 13)), "both sides"),
    ("off = 15", lambda r: (r[0].__setitem__(18, 0), r[0].__setitem__(50, 15)), "15 checkers off"),
    ("mover 2", lambda r: r[0].__setitem__(52, 2), "mover"),
    ("roll (3, 0)", lambda r: r[0].__setitem__(53, 3), "roll"),
])
def test_validate_starts_rejects(name, edit, why):
    good = _bearoff()
    bad = _bearoff()
    edit(bad)
    recs = torch.cat([good, good, bad, good])
    with pytest.raises(ValueError, match=r"lane 2.*" + re.escape(why)):
        validate_starts(recs)


def test_validate_starts_shape():
    with pytest.raises(ValueError):
        validate_starts(torch.zeros(4, 52, dtype=torch.uint8))
    with pytest.raises(ValueError):
        validate_starts(torch.zeros(4, 64, dtype=torch.int32))


# ------------------------------------------------------------------ C ABI, CLI --
def test_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "bgx.h")).read()
    for name in ("bgx_engine_set_starts", "bgx_rollout_begin", "bgx_rollout_advance"):
        assert name in _lib.SIGNATURES
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), name
    assert len(_lib.SIGNATURES["bgx_engine_set_starts"][1]) == 3
    assert len(_lib.SIGNATURES["bgx_rollout_begin"][1]) == 12
    assert len(_lib.SIGNATURES["bgx_rollout_advance"][1]) == 14
    assert len(R.FIELDS) == 8 and re.search(r"BGX_ROLLOUT_LOSS3\s*=\s*7", header)


def test_parser():
    ap = R.build_parser()
    ns = ap.parse_args("--net random --positions opening --trials 72 --batch 128 --max-steps 4000".split())
    assert (ns.player, ns.first_roll, ns.trials, ns.batch, ns.top_k) == ("policy", "stratified", 72, 128, None)
    ns = ap.parse_args("--net ckpt.pt --player 2ply --top-k 3 --positions p.json --first-roll random".split())
    assert ns.top_k == 3 and ns.first_roll == "random"
    for bad in ("--net ckpt.pt --player 1ply --top-k 3 --positions opening",
                "--net ckpt.pt --top-k 3 --positions opening",
                "--net random --player 2ply --top-k 3 --positions opening",
                "--net ckpt.pt --player 2ply --top-k 0 --positions opening",
                "--net ckpt.pt --positions opening --first-roll fixed"):
        with pytest.raises(SystemExit):
            ap.parse_args(bad.split())


def test_load_positions(tmp_path):
    import json
    op = R.load_positions("opening")
    assert op.shape == (1, 64) and int(op[0, :24].sum()) == 15 and int(op[0, 24:48].sum()) == 15
    board = [0] * 52
    board[18], board[50], board[24], board[51] = 1, 14, 1, 14
    f = tmp_path / "p.json"
    f.write_text(json.dumps([{"board": board, "player": 1}, {"board": board, "player": 0}]))
    p = R.load_positions(str(f))
    assert p.shape == (2, 64) and p[0, 52] == 1 and p[1, 52] == 0 and torch.equal(p[0, :52], _bearoff()[0, :52])
    f.write_text(json.dumps([{"board": board[:51], "player": 0}]))
    with pytest.raises(ValueError):
        R.load_positions(str(f))


def test_exact_score():
    b = np.zeros(52, np.int8)
    b[50] = 15
    b[24 + 5] = 15                      # PLAYER2: 15 on its own 6-point, none off
    assert R.exact_score(b, 0) == 2
    b2 = b.copy()
    b2[24 + 5], b2[49] = 14, 1          # a PLAYER2 checker on the bar
    assert R.exact_score(b2, 0) == 3
    b3 = b.copy()
    b3[24 + 5], b3[24 + 20] = 14, 1     # a PLAYER2 checker in PLAYER1's home board (points 18..23)
    assert R.exact_score(b3, 0) == 3
    b4 = b.copy()
    b4[24 + 5], b4[51] = 14, 1
    assert R.exact_score(b4, 0) == 1
    b5 = b.copy()
    b5[50] = 14
    b5[23] = 1
    assert R.exact_score(b5, 0) == 0
    m = np.zeros(52, np.int8)           # the mirror: PLAYER2 has won, PLAYER1 on the bar
    m[51], m[48], m[20] = 15, 1, 14
    assert R.exact_score(m, 1) == 3
