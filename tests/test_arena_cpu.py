"""The arena's host-side arithmetic and command line (bgx/arena.py); no GPU."""
import math

import pytest


def _tally(**kw):
    from bgx.arena import FIELDS
    t = [0] * 16
    for k, v in kw.items():
        t[FIELDS.index(k)] = v
    return t


def test_summarize_rates():
    from bgx.arena import summarize
    # 100 games: A won 60 (45 singles, 10 gammons, 5 backgammons = 80 points), B won 40
    # (30 singles, 10 gammons = 50 points)
    r = summarize(_tally(games=100, wins_a=60, wins_b=40, points_a=80, points_b=50, gammons_a=10, gammons_b=10,
                         backgammons_a=5, games_a_p1=50, wins_a_p1=33, wins_p1=55, plies=9000), steps=321,
                  unfinished=0)
    assert r["games"] == 100 and r["wins_a"] == 60 and r["wins_b"] == 40 and r["plies"] == 9000
    assert r["gammons_a"] == 10 and r["backgammons_a"] == 5 and r["backgammons_b"] == 0
    assert r["games_a_p1"] == 50 and r["wins_a_p1"] == 33 and r["wins_p1"] == 55
    assert r["steps"] == 321 and r["unfinished_lanes"] == 0
    assert r["win_rate_a"] == 0.6
    assert r["ppg_a"] == pytest.approx(0.3, abs=1e-15)
    assert r["win_rate_stderr"] == pytest.approx(math.sqrt(0.6 * 0.4 / 100), rel=1e-15)


def test_summarize_extremes():
    from bgx.arena import summarize
    r = summarize(_tally(games=8, wins_b=8, points_b=24, backgammons_b=8, active_lanes=3), steps=40, unfinished=3)
    assert r["win_rate_a"] == 0.0 and r["win_rate_stderr"] == 0.0 and r["ppg_a"] == -3.0
    assert r["unfinished_lanes"] == 3 and r["active_lanes"] == 3
    # no finished game: no division error, all rates zero
    z = summarize([0] * 16, steps=0, unfinished=64)
    assert z["games"] == 0 and z["win_rate_a"] == 0.0 and z["ppg_a"] == 0.0 and z["win_rate_stderr"] == 0.0
    assert z["unfinished_lanes"] == 64
    with pytest.raises(ValueError):
        summarize([0] * 5, 0, 0)


def test_cli_requires_max_steps(capsys):
    from bgx.arena import build_parser
    ap = build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--a", "random", "--b", "random"])
    assert "--max-steps" in capsys.readouterr().err
    a = ap.parse_args(["--a", "x.pt", "--b", "random", "--player-a", "2ply", "--max-steps", "900"])
    assert a.max_steps == 900 and a.player_a == "2ply" and a.player_b == "policy" and a.games_per_lane == 2
    with pytest.raises(SystemExit):
        ap.parse_args(["--a", "random", "--b", "random", "--max-steps", "9", "--player-b", "3ply"])


def test_arena_entry_points_declared():
    """The lane-selected searches and the arena's kernels are part of the C ABI table."""
    from bgx._lib import SIGNATURES
    for s in ("bgx_one_ply_sel", "bgx_two_ply_sel", "bgx_arena_begin", "bgx_arena_merge", "bgx_arena_advance",
              "bgx_random_act"):
        assert s in SIGNATURES


def test_evaluate_refuses_a_process_group():
    """Multi-rank evaluation is out of scope: a trainer with a process group says so
    before it touches anything."""
    from bgx.train import PPOTrainer
    tr = PPOTrainer.__new__(PPOTrainer)
    tr.group = object()
    with pytest.raises(NotImplementedError, match="multi-rank"):
        tr.evaluate("random")
