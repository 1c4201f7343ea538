"""Truncated position rollouts (Rollout.run_lanes / run with truncate=, the two
bgx_rollout_trunc_* kernels of csrc/bg_trunc.h): the kernels alone against the rule written out
lane by lane, exact runs from the opening, a traced run with both kinds of ending against
truncate.truncate_reference (with and without the luck adjustment, both lookaheads), the
estimator against an exact bearoff table, rollout_moves and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES, PLIES = 0, 1
TG, TP, TV, TV2, TL, TL2, TVL = range(7)
F = np.float32
ONE = 65536


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


# two checkers on each side's 4-, 5- and 6-points, nine off
RACE = record({18: 2, 19: 2, 20: 2}, {24 + 5: 2, 24 + 4: 2, 24 + 3: 2}, 0)
RACE_EQUITY = 0.308428                                   # the side on roll wins 0.654214 (exact K = 6 table)


def opening(mover, B):
    from bgx.rollout import opening_record
    r = opening_record().clone()
    r[52] = mover
    return r[None].repeat(B, 1)


def groups200():
    group = np.repeat(np.arange(5), [10, 50, 33, 64, 36]).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):            # 7 idle lanes, in the middle of waves and groups
        group = np.insert(group, k, -1)
    assert len(group) == 200 and (group < 0).sum() == 7
    return group


def by_mover(p1, p2):
    """A callable value that depends on the side on roll alone."""
    def value(eng, tsel):
        m = eng.records()[:, 52]
        return torch.where(m == 0, float(p1), float(p2)).to(torch.float32).contiguous()
    return value


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------ 1. kernels against the host rule --
def lane_rule(scale, v, same):
    """Part 1 of csrc/bg_trunc.h on scalars."""
    e = F(F(scale) * F(v))
    e = F(0) if math.isnan(e) else min(max(e, F(-3)), F(3))
    y = e if same else F(-e)
    return int(np.rint(F(y * F(ONE))))


def luck_rule(x):
    x = F(F(x) * F(ONE))
    if not math.isfinite(x):
        return 0
    return int(np.rint(min(max(x, F(-2097152)), F(2097152))))


@pytest.mark.parametrize("with_luck", [True, False])
def test_kernels_equal_the_host_rule(with_luck):
    from bgx import _lib
    L = _lib.load()
    B, P, G, H, scale = 200, 5, 3, 6, 1.5
    group = groups200()
    rng = np.random.RandomState(7)
    recs = np.zeros((B, 64), np.uint8)
    recs[:, 52] = rng.randint(0, 2, B)
    recs[:, 55] = rng.rand(B) < 0.1                                      # game_over records
    starts = np.zeros((B, 64), np.uint8)
    starts[:, 52] = rng.randint(0, 2, B)
    plies = rng.choice([0, 1, H - 1, H, H + 1, 40], B, p=[0.1, 0.1, 0.2, 0.3, 0.2, 0.1]).astype(np.int32)
    games_done = rng.randint(0, G, B).astype(np.int32)                   # G - 1: the lane's last game
    sel = ((group >= 0) & (rng.rand(B) < 0.85)).astype(np.uint8)         # some retired lanes
    games_done[(sel == 0) & (group >= 0)] = G
    value = rng.uniform(-2.5, 2.5, B).astype(np.float32)
    value[rng.rand(B) < 0.08] = np.nan
    value[rng.rand(B) < 0.05] = np.inf
    value[rng.rand(B) < 0.05] = -np.inf
    value[rng.rand(B) < 0.05] = 7.0
    lane_luck = rng.uniform(-1, 1, B).astype(np.float32)
    lane_luck[rng.rand(B) < 0.06] = np.nan
    lane_luck[rng.rand(B) < 0.06] = np.inf
    lane_luck[rng.rand(B) < 0.06] = -100.0                               # beyond the clamp 2^21 / 2^16 = 32
    sel[3], plies[3] = 1, H                                              # an idle lane that looks ready: never set
    d_recs, d_starts, d_group = dev(recs), dev(starts), dev(group)
    d_plies, d_sel, d_gd = dev(plies), dev(sel), dev(games_done)
    d_tsel = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    d_count = torch.tensor([5], dtype=torch.int64, device="cuda")
    assert L.bgx_rollout_trunc_sel(ptr(d_recs), ptr(d_group), B, P, H, ptr(d_plies), ptr(d_sel), ptr(d_tsel), ptr(d_count),
                                   stream()) == 0
    want_tsel = np.array([int(sel[i] != 0 and group[i] >= 0 and recs[i, 55] == 0 and plies[i] >= H) for i in range(B)],
                         np.uint8)
    assert np.array_equal(d_tsel.cpu().numpy(), want_tsel)
    assert int(d_count) == 5 + int(want_tsel.sum()) and 40 < want_tsel.sum() < 150
    # every case occurs among the lanes that are cut, and among those that are not
    cut = want_tsel != 0
    assert (plies[cut] == H).any() and (plies[cut] > H).any() and ((plies == H - 1) & (sel != 0) & (group >= 0)).any()
    assert ((recs[:, 55] != 0) & (plies >= H) & (sel != 0) & (group >= 0)).any() and ((sel == 0) & (plies >= H)).any()
    same = recs[:, 52] == starts[:, 52]
    assert same[cut].any() and (~same[cut]).any() and (games_done[cut] == G - 1).any() and (games_done[cut] < G - 1).any()
    assert np.isnan(value[cut]).any() and np.isposinf(value[cut]).any() and np.isneginf(value[cut]).any()
    assert (value[cut] == 7.0).any() and np.isnan(lane_luck[cut]).any() and (lane_luck[cut] == -100.0).any()
    # a count of NULL is allowed
    assert L.bgx_rollout_trunc_sel(ptr(d_recs), ptr(d_group), B, P, H, ptr(d_plies), ptr(d_sel), ptr(d_tsel), None,
                                   stream()) == 0
    assert np.array_equal(d_tsel.cpu().numpy(), want_tsel)

    d_value, d_luck = dev(value), dev(lane_luck)
    d_tally = torch.zeros(P, 7, dtype=torch.int64, device="cuda")
    d_active = torch.tensor([1000], dtype=torch.int64, device="cuda")
    d_mask = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    assert L.bgx_rollout_trunc_cut(ptr(d_recs), ptr(d_starts), ptr(d_group), ptr(d_tsel), ptr(d_value), scale, B, P, G,
                                   ptr(d_gd), ptr(d_plies), ptr(d_sel), ptr(d_luck) if with_luck else None, ptr(d_tally),
                                   ptr(d_active), ptr(d_mask), stream()) == 0
    w_tally = np.zeros((P, 7), np.int64)
    w_gd, w_plies, w_sel, w_luck = games_done.copy(), plies.copy(), sel.copy(), lane_luck.copy()
    retired = 0
    for i in range(B):
        if not want_tsel[i]:
            continue
        vq = lane_rule(scale, value[i], bool(same[i]))
        lq = luck_rule(lane_luck[i]) if with_luck else 0
        row = w_tally[group[i]]
        row[TG] += 1; row[TP] += plies[i]; row[TV] += vq; row[TV2] += vq * vq
        row[TL] += lq; row[TL2] += lq * lq; row[TVL] += vq * lq
        if with_luck:
            w_luck[i] = 0.0
        w_gd[i] += 1
        w_plies[i] = 0
        if w_gd[i] >= G:
            w_sel[i] = 0
            retired += 1
    assert np.array_equal(d_tally.cpu().numpy(), w_tally) and retired > 5
    assert np.array_equal(d_mask.cpu().numpy(), want_tsel)
    assert np.array_equal(d_gd.cpu().numpy(), w_gd) and np.array_equal(d_plies.cpu().numpy(), w_plies)
    assert np.array_equal(d_sel.cpu().numpy(), w_sel) and int(d_active) == 1000 - retired
    assert np.array_equal(d_luck.cpu().numpy().view(np.int32), w_luck.view(np.int32))
    if not with_luck:
        assert not w_tally[:, TL:].any()
    assert np.abs(w_tally[:, TV]).max() > 0 and (w_tally[:, TG] > 0).all()


def test_argument_checks():
    from bgx import _lib
    L = _lib.load()
    B, P = 64, 2
    z8 = torch.zeros(B, 64, dtype=torch.uint8, device="cuda")
    u8 = torch.zeros(B, dtype=torch.uint8, device="cuda")
    i32 = torch.zeros(B, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(B, dtype=torch.float32, device="cuda")
    tally = torch.zeros(P, 7, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = stream()
    ok = [ptr(z8), ptr(i32), B, P, 1, ptr(i32), ptr(u8), ptr(u8.clone()), ptr(cnt), s]
    assert L.bgx_rollout_trunc_sel(*ok) == 0
    for k, v in ((0, None), (1, None), (2, 0), (3, 0), (4, 0), (4, -7), (5, None), (6, None), (7, None)):
        a = list(ok)
        a[k] = v
        assert L.bgx_rollout_trunc_sel(*a) == _lib.BGX_EINVAL, (k, v)
    ok = [ptr(z8), ptr(z8), ptr(i32), ptr(u8), ptr(f32), 1.0, B, P, 1, ptr(i32.clone()), ptr(i32.clone()), ptr(u8.clone()),
          ptr(f32.clone()), ptr(tally), ptr(cnt), ptr(u8.clone()), s]
    assert L.bgx_rollout_trunc_cut(*ok) == 0
    for k, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, math.nan), (6, 0), (7, 0), (8, -1), (9, None),
                 (10, None), (11, None), (13, None), (14, None), (15, None)):
        a = list(ok)
        a[k] = v
        assert L.bgx_rollout_trunc_cut(*a) == _lib.BGX_EINVAL, (k, v)
    a = list(ok)
    a[12] = None                                                         # no lane_luck: allowed
    assert L.bgx_rollout_trunc_cut(*a) == 0
    torch.cuda.synchronize()
    assert not tally.any()


# ------------------------------------------------------------ 2. exact runs, the opening --
B128, G2 = 128, 2


def run128(trunc, start_mover=0, trace=False, seed=3, max_steps=6000):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    ro = Rollout(B128, seed=seed)
    out = ro.run_lanes(RandomPlayer(11), opening(start_mover, B128), torch.zeros(B128, dtype=torch.int32), 1, G2,
                       max_steps=max_steps, trace=trace, truncate=trunc)
    assert ro.eng.error() == 0 and len(out) == (3 if trunc is None else 4) and not out[1].any()     # unfinished == 0
    if trunc is not None and max_steps >= trunc.plies * G2:
        assert ro.steps <= trunc.plies * G2
    return out, ro


@pytest.mark.parametrize("start_mover", [0, 1])
@pytest.mark.parametrize("plies", [1, 2])
def test_every_game_truncated(plies, start_mover):
    """plies = 1: the opponent is on roll at the cut, its value negated; plies = 2: the start
    mover's own value."""
    from bgx.truncate import Truncation, summarize_truncated, value_q
    p = (0.3, -0.7)                                                      # the value of PLAYER1 / PLAYER2 on roll
    (tally, _, _, tt), ro = run128(Truncation(by_mover(*p), plies), start_mover)
    n = B128 * G2
    cut_mover = start_mover if plies == 2 else 1 - start_mover
    vq = int(value_q(1.0, F(p[cut_mover]), cut_mover == start_mover))
    assert vq == {(1, 0): 45875, (1, 1): -19661, (2, 0): 19661, (2, 1): -45875}[(plies, start_mover)]
    assert not tally.any() and ro.steps == plies * G2
    assert tt.cpu().numpy()[0].tolist() == [n, n * plies, n * vq, n * vq * vq, 0, 0, 0]
    r = summarize_truncated(tally[0].tolist(), tt[0].tolist())
    assert r["equity"] == vq / ONE and r["equity_stderr"] == 0.0 and r["truncated_share"] == 1.0


def test_a_horizon_never_reached_changes_nothing():
    from bgx.truncate import Truncation
    (t0, _, tr0), ro0 = run128(None, trace=True)
    (t1, _, tr1, tt), ro1 = run128(Truncation(by_mover(0.3, -0.7), 2 ** 30), trace=True)
    assert torch.equal(t0, t1) and not tt.any() and int(t0[0, GAMES]) == B128 * G2
    # the plain run reads its active-lane count every SYNC_EVERY steps only: its last steps are idle
    s = ro1.steps
    assert torch.equal(tr0["games_done"], tr1["games_done"]) and 0 <= ro0.steps - s < 16
    assert torch.equal(tr0["action"][:s], tr1["action"]) and torch.equal(tr0["done"][:s], tr1["done"])
    assert not tr0["action"][s:].any()
    assert not tr1["trunc"].any() and bool(torch.isnan(tr1["trunc_value"]).all())


def test_max_steps_leaves_games_unfinished():
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    from bgx.truncate import Truncation
    ro = Rollout(B128, seed=3)
    tally, unf, _, tt = ro.run_lanes(RandomPlayer(11), opening(0, B128), torch.zeros(B128, dtype=torch.int32), 1, G2,
                                     max_steps=5, truncate=Truncation(by_mover(0.3, -0.7), 4))
    assert ro.steps == 5 and int(tt[0, TG]) == B128 and int(unf[0]) == B128 and not tally.any()


# ------------------------------------------------- 3. a traced run with both kinds of ending --
def traced(lookahead, luck):
    from bgx.arena import RandomPlayer
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout
    from bgx.search import ValueHead
    from bgx.truncate import Truncation
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=128).cuda())
    B, P, G = 64, 3, 4
    group = np.repeat(np.arange(3), [20, 21, 20]).astype(np.int32)
    for k in (7, 30, 50):
        group = np.insert(group, k, -1)
    starts = torch.from_numpy(RACE)[None].repeat(B, 1)
    tc = Truncation(vh, 8, lookahead=lookahead)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=5)
        out = ro.run_lanes(RandomPlayer(2), starts, torch.from_numpy(group), P, G, max_steps=6000, trace=True,
                           truncate=tc, luck=vh if luck else None)
        assert ro.eng.error() == 0 and not out[1].any() and len(out) == (5 if luck else 4)
        runs.append(out)
    return runs, starts, group, P, G, tc


@pytest.mark.parametrize("luck", [False, True])
@pytest.mark.parametrize("lookahead", [0, 1])
def test_traced_run_equals_truncate_reference(lookahead, luck):
    from bgx.truncate import summarize_truncated, summarize_truncated_luck, truncate_reference
    runs, starts, group, P, G, tc = traced(lookahead, luck)
    tally, _, tr, tt = runs[0][0], None, runs[0][2], runs[0][-1]
    tally, tt = tally.cpu().numpy(), tt.cpu().numpy()
    ref = truncate_reference(tr, starts, group, P, G, tc)
    assert np.array_equal(tally, ref["tally"]) and np.array_equal(tt, ref["trunc_tally"])
    assert np.array_equal(tr["trunc"].cpu().numpy() != 0, ref["trunc"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    n_nat, n_t = int(tally[:, GAMES].sum()), int(tt[:, TG].sum())
    n = 61 * G
    print(f"lookahead {lookahead} luck {luck}: natural {n_nat}, truncated {n_t} of {n}; trunc_tally {tt.tolist()}")
    assert n_nat + n_t == n and n_nat >= 0.1 * n and n_t >= 0.1 * n
    assert not tr["trunc"][:, torch.from_numpy(group < 0).cuda()].any()
    v = tr["trunc_value"]
    assert bool((torch.isnan(v) == (tr["trunc"] == 0)).all()) and np.abs(tt[:, TV]).sum() > 0
    # a truncated game ran exactly 8 plies
    assert np.array_equal(tt[:, TP], 8 * tt[:, TG])
    if luck:
        lt = runs[0][3].cpu().numpy()
        assert np.array_equal(lt, ref["luck_tally"]) and np.array_equal(lt[:, 3], tally[:, GAMES])
        assert np.abs(tt[:, TL]).sum() > 0 and np.abs(tt[:, TVL]).sum() > 0 and (tt[:, TL2] > 0).all()
        for p in range(P):
            r = summarize_truncated_luck(tally[p], lt[p], tt[p])
            assert r["games"] == [20, 21, 20][p] * G and 0.0 < r["variance_ratio"] and math.isfinite(r["equity_luck"])
    else:
        assert not tt[:, TL:].any()
        for p in range(P):
            r = summarize_truncated(tally[p], tt[p])
            assert r["games"] == [20, 21, 20][p] * G and r["truncated_games"] == tt[p, TG]
    # run to run identical
    for a, b in zip(runs[0], runs[1]):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)
    for k in ("trunc", "trunc_mover", "action", "done"):
        assert torch.equal(runs[1][2][k], tr[k]), k
    assert torch.equal(runs[1][2]["trunc_value"].nan_to_num(7.0), v.nan_to_num(7.0))


# ------------------------------------------------ 4. the estimator is right when the value is --
@pytest.fixture(scope="module")
def db6():
    from bgx.bearoff import BearoffDB
    return BearoffDB(6)


@pytest.mark.parametrize("start_mover", [0, 1])
def test_estimator_against_the_exact_table(db6, start_mover):
    """Perfect play on both sides and the table's own equity as value: the value is a martingale,
    so the truncated estimate is unbiased at every horizon (a wrong sign or side would miss by
    about 0.6), and its spread is below the played-out games'."""
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffPlayer
    from bgx.rollout import Rollout, summarize
    from bgx.truncate import Truncation, summarize_truncated
    B = 4096
    start = RACE.copy()
    start[52] = start_mover
    starts = torch.from_numpy(start)[None].repeat(B, 1)
    in_db, win = db6.lookup(starts[:1].cuda())
    exact = 2.0 * float(win[0]) - 1.0
    assert int(in_db[0]) == 1 and exact == pytest.approx(RACE_EQUITY, abs=2e-6)

    def value(eng, tsel):
        return (2.0 * db6.lookup(eng.records())[1] - 1.0).contiguous()

    grp = torch.zeros(B, dtype=torch.int32)
    ro = Rollout(B, seed=9)
    tally, unf, _ = ro.run_lanes(BearoffPlayer(RandomPlayer(4), db6), starts, grp, 1, 1, max_steps=200)
    plain = summarize(tally[0].tolist(), int(unf[0]))
    assert plain["games"] == B and abs(plain["equity"] - exact) < 5 * plain["equity_stderr"]
    for plies in (3, 4):                                  # the opponent / the start mover on roll at the cut
        ro = Rollout(B, seed=9)
        tally, unf, _, tt = ro.run_lanes(BearoffPlayer(RandomPlayer(4), db6), starts, grp, 1, 1, max_steps=200,
                                         truncate=Truncation(value, plies))
        r = summarize_truncated(tally[0].tolist(), tt[0].tolist(), int(unf[0]))
        print(f"mover {start_mover} plies {plies}: equity {r['equity']:.5f} +- {r['equity_stderr']:.5f} (exact {exact:.6f}; "
              f"plain {plain['equity']:.5f} +- {plain['equity_stderr']:.5f}), truncated_share {r['truncated_share']:.3f}")
        assert r["games"] == B and r["unfinished"] == 0 and r["truncated_share"] > 0.5
        assert abs(r["equity"] - exact) < 5 * r["equity_stderr"]
        assert 0.0 < r["equity_stderr"] < plain["equity_stderr"]


# ------------------------------------------------------------------------- 5. other checks --
def test_rollout_moves_ranks_the_winning_move_first():
    """PLAYER1 has two checkers left (its 2- and 1-points) and rolls 2-1: bearing both off wins
    at once -- scored exactly, no lanes -- while 2-point to 1-point, then off, leaves a checker;
    that move's rollout is truncated after the opponent's ply at PLAYER1's value 0.25."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout, rollout_moves
    from bgx.truncate import Truncation
    rec = record({22: 1, 23: 1}, {24 + 5: 3}, 0, roll=(2, 1))
    ro = Rollout(256, seed=1)
    steps0 = ro.steps
    out = rollout_moves(ro, RandomPlayer(3), torch.from_numpy(rec), 72, truncate=Truncation(by_mover(0.25, -0.5), 1))
    exact = [d for d in out if d["exact"]]
    assert 1 <= len(exact) < len(out) and out[:len(exact)] == exact          # the winning order(s) of play first
    for d in exact:
        assert d["equity"] == 1.0 and d["games"] == 0 and d["truncated_share"] == 0.0 and d["equity_stderr"] == 0.0
    for d in out[len(exact):]:
        # the opponent bears its three checkers off with 6-6 only: else the cut, at +0.25 for PLAYER1
        assert not d["exact"] and d["games"] == 72 and d["truncated_share"] >= 0.9 and d["unfinished"] == 0
        assert 0.25 - 1.25 * (1 - d["truncated_share"]) == pytest.approx(d["equity"], abs=1e-12)
    assert ro.steps - steps0 == 1                          # one ply per game, and only the open move's games


def test_unsupported_combinations():
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout, opening_record
    from bgx.truncate import Truncation
    ro = Rollout(64, seed=0)
    tc = Truncation(by_mover(0.1, 0.1), 4)
    starts, grp = opening(0, 64), torch.zeros(64, dtype=torch.int32)

    class FakeDB:                               # the combination is refused before the table is looked at
        pass

    for kw, word in ((dict(bearoff=FakeDB()), "bearoff"), (dict(cube=CubeRule(by_mover(0.1, 0.1))), "cube")):
        with pytest.raises(ValueError, match=f"truncate together with {word}"):
            ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, truncate=tc, **kw)
        with pytest.raises(ValueError, match=f"truncate together with {word}"):
            ro.run(RandomPlayer(1), opening_record()[None], 36, truncate=tc, **kw)
    with pytest.raises(ValueError, match="truncate.Truncation"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, truncate=8)
    with pytest.raises(ValueError, match="float32"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1,
                     truncate=Truncation(lambda eng, tsel: torch.zeros(64).double().cuda(), 1))
    torch.cuda.synchronize()


def test_command_line(tmp_path, capsys):
    from bgx import rollout
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    ckpt = str(tmp_path / "net.pt")
    torch.save(PolicyNet(hidden_size=40).state_dict(), ckpt)
    base = ["--net", ckpt, "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps", "6000",
            "--truncate", "8"]
    rollout.main(base)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["position"] == 0 and lines[1]["summary"] and lines[1]["truncate"] == 8
    r = lines[0]
    assert r["games"] == 72 and r["unfinished"] == 0 and r["truncated_games"] == 72 and r["truncated_share"] == 1.0
    assert r["natural_games"] == 0 and r["plies_per_game"] == 8.0 and lines[1]["steps"] <= 8 + 16
    for k in ("equity", "equity_stderr", "truncated_equity"):
        assert math.isfinite(r[k]), k
    assert (lines[1]["truncated_share"], lines[1]["truncate_lookahead"], lines[1]["truncate_scale"]) == (1.0, 0, 1.0)
    rollout.main(base + ["--luck", "--truncate-lookahead", "1", "--truncate-net", ckpt, "--truncate-scale", "2"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    r = lines[0]
    assert r["games"] == 72 and r["truncated_games"] == 72 and lines[1]["luck"] is True
    for k in ("equity_luck", "equity_luck_stderr", "variance_ratio", "luck_scale"):
        assert math.isfinite(r[k]), k
    assert (lines[1]["truncate_lookahead"], lines[1]["truncate_scale"], lines[1]["truncate_net"]) == (1, 2.0, ckpt)
