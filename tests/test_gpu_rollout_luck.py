"""Luck-adjusted rollouts (Rollout.run_lanes / run with luck=, bgx_rollout_luck_add / _flush):
the device's luck tally against the host replay of the traced steps, the stratified
first-roll rule, unbiasedness on positions of known equity, rollout_moves, the players and
the command line."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES = 0
LUCK, LUCK2, RESLUCK, LUCK_GAMES = 0, 1, 2, 3


def record(p1, p2, mover, roll=(0, 0), bar=(0, 0)):
    r = np.zeros(64, np.uint8)
    for k, v in list(p1.items()) + list(p2.items()):
        r[k] = v
    r[48], r[49] = bar
    r[50] = 15 - r[:24].sum() - r[48]
    r[51] = 15 - r[24:48].sum() - r[49]
    r[52] = mover
    r[53], r[54] = roll
    return r


# the positions of tests/test_gpu_rollout.py and their exact equities
CASE_A = record({18: 1}, {24: 1}, 0)                     # 27 of the 36 rolls bear the checker off: 0.5
CASE_B = record({23: 1}, {29: 15}, 0)                    # always a gammon
CASE_C = record({23: 1}, {29: 14}, 0, bar=(0, 1))        # always a backgammon
CASE_D = record({23: 1}, {24 + 5: 1}, 1)                 # the mirror of (a), PLAYER2 on roll
EXACT = (0.5, 2.0, 3.0, 0.5)


@pytest.fixture(scope="module")
def net():
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    return PolicyNet(hidden_size=40).cuda()


@pytest.fixture(scope="module")
def vh(net):
    from bgx.search import ValueHead
    return ValueHead(net)


def small_starts(B, seed, fixed_rolls):
    """1-3 checkers a side in the home boards; fixed_rolls: every other lane's start record
    fixes its first roll."""
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        p1 = {18 + p: 1 for p in rng.choice(6, rng.randint(1, 4), replace=False)}
        p2 = {24 + p: 1 for p in rng.choice(6, rng.randint(1, 4), replace=False)}
        roll = (rng.randint(1, 7), rng.randint(1, 7)) if fixed_rolls and i % 2 else (0, 0)
        s[i] = record(p1, p2, rng.randint(2), roll)
    return s


def groups200():
    group = np.repeat(np.arange(5), [10, 50, 33, 64, 36]).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):            # 7 idle lanes, in the middle of waves and groups
        group = np.insert(group, k, -1)
    assert len(group) == 200 and (group < 0).sum() == 7
    return group


def host_tally(tr, starts, group, P, G):
    from bgx.rollout import luck_tally_reference
    return luck_tally_reference(tr["luck"].cpu().numpy(), tr["mover"].cpu().numpy(), tr["done"].cpu().numpy(),
                                tr["info"].cpu().numpy(), starts, group, P, G)


@pytest.mark.parametrize("fixed_rolls", [False, True])
def test_luck_tally_equals_host_replay(vh, fixed_rolls):
    """200 lanes, five unequal groups, seven idle lanes, two games per lane; fixed_rolls: the
    same with every other start record fixing its first roll (no luck on ply 0 there)."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    B, P, G = 200, 5, 2
    group, starts = groups200(), small_starts(200, 12, fixed_rolls)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=4)
        tally, unfinished, tr, ltally = ro.run_lanes(RandomPlayer(5), torch.from_numpy(starts), torch.from_numpy(group),
                                                     P, G, max_steps=200, trace=True, luck=vh)
        assert ro.eng.error() == 0 and not unfinished.any()
        runs.append((tally.cpu().numpy(), ltally.cpu().numpy(), tr))
    tally, ltally, tr = runs[0]
    assert ltally.shape == (P, 4) and ltally.dtype == np.int64
    ref = host_tally(tr, starts, group, P, G)
    assert np.array_equal(ltally, ref), (ltally, ref)
    assert np.array_equal(ltally[:, LUCK_GAMES], tally[:, GAMES])
    assert (ltally[:, LUCK2] > 0).all()                       # the luck is not trivially zero
    # run to run identical
    assert np.array_equal(runs[1][1], ltally) and torch.equal(runs[1][2]["luck"].nan_to_num(7.0),
                                                              tr["luck"].nan_to_num(7.0))
    # idle lanes never get a luck value
    assert torch.isnan(tr["luck"][:, torch.from_numpy(group < 0).cuda()]).all()
    # luck does not change the games: the 8-field tally and the steps of a run without it
    ro = Rollout(B, seed=4)
    out = ro.run_lanes(RandomPlayer(5), torch.from_numpy(starts), torch.from_numpy(group), P, G, max_steps=200,
                       trace=True)
    assert len(out) == 3 and "luck" not in out[2]
    assert np.array_equal(out[0].cpu().numpy(), tally)
    n = tr["done"].shape[0]                 # the luck run reads the active count every step and stops at once
    assert out[2]["done"].shape[0] >= n
    for k in ("done", "info", "action", "mover"):
        assert torch.equal(out[2][k][:n], tr[k])


def test_fixed_first_roll_has_no_luck(vh):
    """The one-checker bear-off from the 6-point on the 36 ordered first rolls, one lane and
    one tally row per roll: a game that ends on its first, fixed roll has L = 0 exactly; a
    game that goes on carries the luck of the reply alone (the opponent bears its last
    checker off with any roll, so that luck is zero to rounding)."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import ROLLS36, Rollout
    starts = np.repeat(CASE_A[None], 64, axis=0)
    starts[:36, 53:55] = np.asarray(ROLLS36, np.uint8)
    group = np.where(np.arange(64) < 36, np.arange(64), -1).astype(np.int32)
    ro = Rollout(64, seed=1)
    tally, unfinished, tr, ltally = ro.run_lanes(RandomPlayer(2), torch.from_numpy(starts), torch.from_numpy(group), 36, 1,
                                                 max_steps=50, trace=True, luck=vh)
    tally, ltally = tally.cpu().numpy(), ltally.cpu().numpy()
    assert np.array_equal(tally[:, GAMES], np.ones(36)) and not unfinished.any()
    first = tally[:, 1] == 1                                  # PLIES: over on the first roll
    assert first.sum() == 27
    assert not ltally[first][:, :3].any() and (ltally[:, LUCK_GAMES] == 1).all()
    luck = tr["luck"].cpu().numpy()
    assert np.abs(luck[0, :36]).max() > 0                     # the fixed rolls have a luck; it is left out
    # the other nine: L = -(the reply's luck), the start mover's own roll not counted
    want = np.rint(-luck[1, :36][~first].astype(np.float32) * np.float32(65536)).astype(np.int64)
    assert np.array_equal(ltally[~first][:, LUCK], want)
    assert np.array_equal(ltally, host_tally(tr, starts, group, 36, 1))


@pytest.fixture(scope="module")
def known(vh):
    """4,096 games with drawn first rolls of each of the four positions, once per scale."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    cases = torch.from_numpy(np.stack([CASE_A, CASE_B, CASE_C, CASE_D]))
    out = {}
    for scale in (1.0, "fit"):
        ro = Rollout(1024, seed=9)
        out[scale] = ro.run(RandomPlayer(3), cases, 4096, first_roll="random", luck=vh, luck_scale=scale)
        assert ro.eng.error() == 0
    return out


def test_unbiased_on_known_equities(known):
    for r, exact in zip(known[1.0], EXACT):
        print({k: r[k] for k in ("equity", "equity_stderr", "equity_luck", "equity_luck_stderr", "variance_ratio",
                                 "luck_mean")})
        assert r["games"] == 4096 and r["unfinished"] == 0 and r["luck_scale"] == 1.0
        assert abs(r["equity_luck"] - exact) <= 5 * r["equity_luck_stderr"]
    for r1, rf in zip(known[1.0], known["fit"]):               # the same games, whatever the scale
        assert all(r1[k] == rf[k] for k in ("games", "win1", "win2", "win3", "loss1", "loss2", "loss3", "equity"))
    for i in (1, 2):                                            # a certain result: nothing to fit
        rf = known["fit"][i]
        assert rf["luck_scale"] == 0.0 and rf["equity_luck"] == EXACT[i] and rf["equity_luck_stderr"] == 0.0
    for i in (0, 3):
        rf = known["fit"][i]
        assert abs(rf["equity_luck"] - EXACT[i]) <= 5 * rf["equity_luck_stderr"] + 5.0 / 4096     # O(1/n) fit bias
        assert rf["variance_ratio"] <= 1.0 + 1e-12


def test_rollout_moves_with_luck(vh):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout, rollout_moves
    ro = Rollout(128, seed=2)
    # 2-1 to play with checkers on the 2- and 1-points: both off (wins), or 22 -> 23 -> off
    dec = record({22: 1, 23: 1}, {24: 1}, 0, roll=(2, 1))
    out = rollout_moves(ro, RandomPlayer(1), torch.from_numpy(dec), 36, luck=vh)
    plain = rollout_moves(Rollout(128, seed=2), RandomPlayer(1), torch.from_numpy(dec), 36)
    assert {o["move"] for o in out} == {o["move"] for o in plain} and len(out) == len(plain)
    assert any(o["exact"] for o in out) and any(not o["exact"] for o in out)
    byp = {o["move"]: o for o in plain}
    for o in out:
        assert {"equity", "equity_stderr", "equity_luck", "equity_luck_stderr", "luck_scale", "variance_ratio"} <= set(o)
        assert o["equity"] == byp[o["move"]]["equity"] and o["exact"] == byp[o["move"]]["exact"]
        if o["exact"]:
            assert o["equity_luck"] == o["equity"] == 1.0 and o["equity_luck_stderr"] == 0.0 and o["games"] == 0
        else:                                   # the opponent bears its last checker off at once: certain
            assert o["equity_luck"] == -1.0 and o["equity_luck_stderr"] == 0.0 and o["games"] == 36
    assert [o["equity_luck"] for o in out] == sorted((o["equity_luck"] for o in out), reverse=True)
    assert all("equity_luck" not in o for o in plain)
    assert ro.eng.error() == 0


@pytest.mark.parametrize("kind", ["1ply", "2ply"])
def test_search_players_with_luck(net, vh, kind):
    from bgx.arena import OnePlyPlayer, TwoPlyPlayer
    from bgx.rollout import Rollout
    player = OnePlyPlayer(net) if kind == "1ply" else TwoPlyPlayer(net, top_k=2)
    cases = torch.from_numpy(np.stack([CASE_A, CASE_D]))
    ro = Rollout(128, seed=2)
    res = ro.run(player, cases, 36, luck=vh)
    plain = Rollout(128, seed=2).run(player, cases, 36)
    for r, p in zip(res, plain):
        assert r["games"] == 36 and r["equity"] == 0.5 and all(r[k] == p[k] for k in p)
        assert np.isfinite(r["equity_luck"]) and r["equity_luck_stderr"] >= 0.0
    assert ro.eng.error() == 0


def test_command_line(net, capsys, tmp_path):
    from bgx import rollout
    ckpt = str(tmp_path / "net.pt")
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, ckpt)
    new = {"luck_scale", "luck_mean", "equity_luck", "equity_luck_stderr", "variance_ratio"}
    args = ["--net", ckpt, "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps", "4000"]
    rollout.main(args)
    plain = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    rollout.main(args + ["--luck", "--luck-scale", "fit"])
    lucky = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(plain) == len(lucky) == 2
    assert set(lucky[0]) == set(plain[0]) | new and not new & set(plain[0])
    assert set(lucky[1]) == set(plain[1]) | {"luck", "luck_scale"} and lucky[1]["luck"] is True
    assert all(lucky[0][k] == plain[0][k] for k in plain[0])           # the same games
    assert lucky[0]["games"] + lucky[0]["unfinished"] == 72
    assert lucky[0]["equity_luck_stderr"] <= lucky[0]["equity_stderr"] * (1 + 1e-9)
