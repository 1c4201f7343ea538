"""The doubling cube in position rollouts (Rollout.run_lanes / run with cube=, the four
bgx_rollout_cube_* kernels of csrc/bg_cube.h): the kernels alone against a scalar host rule,
runs from the opening whose cubeful sums are known exactly from the plain tally, a traced run
against cube.cube_reference, the cube decision and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES, PLIES, WIN1, LOSS1 = 0, 1, 2, 5
CG, CP, CP2, CLOG, PG, PP, PW, DBL = range(8)
F = np.float32


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


CASE_B = record({23: 1}, {29: 15}, 0)                    # always a gammon for PLAYER1, on its first roll


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
    """A cube rule's callable value that depends on the side on roll alone."""
    def value(eng, dsel):
        m = eng.records()[:, 52]
        return torch.where(m == 0, float(p1), float(p2)).to(torch.float32).contiguous()
    return value


def points(tally):
    """sum_k k (WINk - LOSSk) and sum_k k^2 (WINk + LOSSk) of plain tally rows."""
    t = np.asarray(tally, np.int64).reshape(-1, 8)
    k = np.arange(1, 4)
    return int(((t[:, 2:5] - t[:, 5:8]) * k).sum()), int(((t[:, 2:5] + t[:, 5:8]) * k * k).sum())


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------ kernels against the host rule --
def test_kernels_equal_the_host_rule():
    """cube_begin, cube_sel and cube_decide at 200 lanes (five unequal groups, seven idle lanes)
    on hand-set state and a synthetic equity, lane by lane against the rule written out in
    scalar Python; then cube_flush on hand-set done / info."""
    from bgx import _lib
    from bgx.cube import CubeRule, pack
    L = _lib.load()
    B, P, G, cap = 200, 5, 2, 3
    rule = CubeRule(lambda e, d: None, scale=1.0, double_at=0.4, pass_at=0.5, too_good_at=0.9, cap=cap, jacoby=True)
    rs = rule.struct()
    da, pa, tg = F(0.4), F(0.5), F(0.9)
    rng = np.random.RandomState(7)
    group = groups200()
    recs, starts = np.zeros((B, 64), np.uint8), np.zeros((B, 64), np.uint8)
    recs[:, 52], starts[:, 52] = rng.randint(2, size=B), rng.randint(2, size=B)
    recs[rng.choice(B, 6, replace=False), 55] = 1                      # game_over records
    states = [0, pack(1, 1), pack(1, 2), pack(2, 1), pack(2, 2), pack(3, 1), pack(3, 2)]       # k = cap among them
    cube0 = np.array(states, np.uint8)[rng.randint(len(states), size=B)]
    cube0[[5, 77, 150]] = [0x0F, 0x31, 0x07]                           # not cube states: read as (3, 0), (1, 0), (3, 0)
    palette = np.array([da, pa, np.nan, F(0.95), np.nextafter(da, F(0)), np.nextafter(pa, F(1)), tg, np.nextafter(tg, F(1)),
                        F(0.45), F(0.7), F(-0.3), F(np.inf)], np.float32)
    equity = palette[rng.randint(len(palette), size=B)]
    plies = rng.randint(0, 4, size=B).astype(np.int32)                 # a quarter on their first ply
    games_done = rng.randint(0, 2, size=B).astype(np.int32)
    sel = ((group >= 0) & (rng.rand(B) < 0.85)).astype(np.uint8)       # some retired lanes
    games_done[(sel == 0) & (group >= 0)] = G

    d_c0, d_cube = dev(cube0), torch.full((B,), 0xAA, dtype=torch.uint8).cuda()
    d_recs, d_starts, d_group = dev(recs), dev(starts), dev(group)
    d_plies, d_gd, d_sel = dev(plies), dev(games_done), dev(sel)
    d_eq, d_dsel, d_mask = dev(equity), torch.full((B,), 9, dtype=torch.uint8).cuda(), torch.full((B,), 9, dtype=torch.uint8).cuda()
    d_tally, d_active = torch.zeros(P, 8, dtype=torch.int64).cuda(), torch.tensor([int(sel.sum())]).cuda()
    assert L.bgx_rollout_cube_begin(ptr(d_c0), B, cap, ptr(d_cube), None) == _lib.BGX_OK
    c0 = d_cube.cpu().numpy()
    k0, o0 = np.minimum(cube0 & 15, cap), np.where(cube0 >> 4 == 3, 0, cube0 >> 4)
    assert np.array_equal(c0, k0 | (o0 << 4)) and c0[5] == 3 and c0[77] == 0x01 and c0[150] == 3
    assert L.bgx_rollout_cube_sel(ptr(d_recs), ptr(d_group), P, ptr(d_plies), ptr(d_sel), ptr(d_cube), B, cap,
                                  ptr(d_dsel), None) == _lib.BGX_OK
    assert L.bgx_rollout_cube_decide(ptr(d_recs), ptr(d_starts), ptr(d_group), ptr(d_dsel), ptr(d_eq), B, P, G, rs,
                                     ptr(d_c0), ptr(d_cube), ptr(d_gd), ptr(d_plies), ptr(d_sel), ptr(d_tally),
                                     ptr(d_active), ptr(d_mask), None) == _lib.BGX_OK
    # the rule, one lane at a time
    w_dsel, w_mask = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    w_cube, w_gd, w_plies, w_sel = c0.copy(), games_done.copy(), plies.copy(), sel.copy()
    w_tally, w_active = np.zeros((P, 8), np.int64), int(sel.sum())
    seen = set()
    for i in range(B):
        k, owner, m = int(c0[i] & 15), int(c0[i] >> 4), int(recs[i, 52])
        if not sel[i]:
            seen.add("retired")
        if not (sel[i] and group[i] >= 0 and plies[i] > 0 and recs[i, 55] == 0):
            seen.add("first ply" if sel[i] and plies[i] == 0 else "off")
            continue
        if k >= cap:
            seen.add("cap")
            continue
        if owner not in (0, m + 1):
            seen.add("owner mismatch")
            continue
        w_dsel[i] = 1
        e = F(1.0) * equity[i]
        if math.isnan(e):
            seen.add("nan")
        if e > tg:
            seen.add("too good")
        if not (e >= da and e <= tg):
            continue
        row = w_tally[group[i]]
        row[DBL] += 1
        if e > pa:
            y = (1 if m == starts[i, 52] else -1) * (1 << k)
            row[CG] += 1; row[CP] += y; row[CP2] += y * y; row[CLOG] += k
            row[PG] += 1; row[PP] += plies[i]; row[PW] += y > 0
            w_gd[i] += 1
            w_plies[i] = 0
            if w_gd[i] >= G:
                w_sel[i] = 0
                w_active -= 1
                seen.add("last game")
            w_cube[i], w_mask[i] = c0[i], 1
            seen.add("pass")
        else:
            w_cube[i] = (k + 1) | ((2 - m) << 4)
            seen.add("take at pass_at" if e == pa else "take")
        if e == da:
            seen.add("double at double_at")
    assert seen >= {"retired", "first ply", "cap", "owner mismatch", "nan", "too good", "pass", "take", "last game",
                    "take at pass_at", "double at double_at"}, seen
    for name, got, want in (("dsel", d_dsel, w_dsel), ("cube", d_cube, w_cube), ("games_done", d_gd, w_gd),
                            ("plies", d_plies, w_plies), ("sel", d_sel, w_sel), ("mask", d_mask, w_mask),
                            ("tally", d_tally, w_tally)):
        assert np.array_equal(got.cpu().numpy(), want), name
    assert int(d_active.item()) == w_active
    assert (w_tally[:, [CG, PG, DBL]] > 0).all() and w_tally[:, DBL].sum() > 2 * w_tally[:, PG].sum()   # every row is hit

    # cube_flush: a done with a winner is scored at the cube (Jacoby: 1 point while centred), any
    # done of a selected lane puts cube0 back, unselected and idle lanes are left alone
    done = (rng.rand(B) < 0.6).astype(np.uint8)
    winner, score = rng.randint(-1, 2, size=B), rng.randint(1, 4, size=B)
    info = (((winner + 1) << 8) | (score << 16)).astype(np.int32)
    before = d_tally.cpu().numpy().copy()
    assert L.bgx_rollout_cube_flush(ptr(d_starts), ptr(d_group), ptr(d_sel), ptr(dev(done)), ptr(dev(info)), B, P, rs,
                                    ptr(d_c0), ptr(d_cube), ptr(d_tally), None) == _lib.BGX_OK
    f_tally, f_cube = before.copy(), w_cube.copy()
    jac = 0
    for i in range(B):
        if not (w_sel[i] and done[i]):
            continue
        k = int(w_cube[i] & 15)
        if winner[i] >= 0:
            s = 1 if k == 0 else int(score[i])
            jac += k == 0 and score[i] > 1
            y = (1 if winner[i] == starts[i, 52] else -1) * (s << k)
            row = f_tally[group[i]]
            row[CG] += 1; row[CP] += y; row[CP2] += y * y; row[CLOG] += k
        f_cube[i] = c0[i]
    assert jac > 0 and np.array_equal(d_tally.cpu().numpy(), f_tally) and np.array_equal(d_cube.cpu().numpy(), f_cube)
    assert (f_tally[:, CG] > before[:, CG]).all() and (f_tally[:, 4:] == before[:, 4:]).all()


def test_argument_checks():
    from bgx import _lib
    from bgx.cube import CubeRule
    L = _lib.load()
    n = 64
    u8 = lambda: torch.zeros(n * 64, dtype=torch.uint8).cuda()
    i32 = lambda: torch.zeros(n, dtype=torch.int32).cuda()
    t = torch.zeros(8, dtype=torch.int64).cuda()
    eq = torch.zeros(n, dtype=torch.float32).cuda()
    bufs = [u8() for _ in range(8)] + [i32() for _ in range(3)]
    a, b, c, d, e, f, g, h = (ptr(x) for x in bufs[:8])
    gi, pi, gd = (ptr(x) for x in bufs[8:])
    ok = CubeRule(lambda *_: None).struct()

    def bad_rule(**kw):
        r = CubeRule(lambda *_: None).struct()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    good = [a, n, 6, b, None]
    assert L.bgx_rollout_cube_begin(*good) == _lib.BGX_OK
    for idx, val in ((0, None), (1, 0), (2, -1), (2, 11), (3, None)):
        args = list(good)
        args[idx] = val
        assert L.bgx_rollout_cube_begin(*args) == _lib.BGX_EINVAL, idx
    good = [a, gi, 1, pi, c, b, n, 6, d, None]
    assert L.bgx_rollout_cube_sel(*good) == _lib.BGX_OK
    for idx, val in ((0, None), (1, None), (2, 0), (3, None), (4, None), (5, None), (6, 0), (7, 11), (7, -1), (8, None)):
        args = list(good)
        args[idx] = val
        assert L.bgx_rollout_cube_sel(*args) == _lib.BGX_EINVAL, idx
    good = [a, e, gi, d, ptr(eq), n, 1, 1, ok, f, b, gd, pi, c, ptr(t), ptr(t[4:]), g, None]
    assert L.bgx_rollout_cube_decide(*good) == _lib.BGX_OK
    rules = [bad_rule(scale=math.nan), bad_rule(double_at=math.nan), bad_rule(pass_at=math.nan), bad_rule(cap=11),
             bad_rule(cap=-1)]
    for idx, val in [(i, None) for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16)] + [(5, 0), (6, 0), (7, -1)] + \
            [(8, r) for r in rules]:
        args = list(good)
        args[idx] = val
        assert L.bgx_rollout_cube_decide(*args) == _lib.BGX_EINVAL, idx
    assert L.bgx_rollout_cube_decide(*(good[:8] + [bad_rule(too_good_at=math.inf)] + good[9:])) == _lib.BGX_OK
    good = [e, gi, c, h, gd, n, 1, ok, f, b, ptr(t), None]
    assert L.bgx_rollout_cube_flush(*good) == _lib.BGX_OK
    for idx, val in [(i, None) for i in (0, 1, 2, 3, 4, 8, 9, 10)] + [(5, 0), (6, 0)] + [(7, r) for r in rules]:
        args = list(good)
        args[idx] = val
        assert L.bgx_rollout_cube_flush(*args) == _lib.BGX_EINVAL, idx
    torch.cuda.synchronize()


# ------------------------------------------------------------ exact runs, the opening --
B128, G2 = 128, 2


def run128(value, start_mover=0, starts=None, trace=False, seed=3, **kw):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout
    ro = Rollout(B128, seed=seed)
    rule = CubeRule(value, **kw)
    starts = opening(start_mover, B128) if starts is None else starts
    out = ro.run_lanes(RandomPlayer(11), starts, torch.zeros(B128, dtype=torch.int32), 1, G2, max_steps=6000,
                       trace=trace, cube=rule)
    assert ro.eng.error() == 0 and len(out) == 4 and not out[1].any()
    tally, ct = out[0].cpu().numpy()[0], out[3].cpu().numpy()[0]
    assert ct[CG] == tally[GAMES] + ct[PG] == B128 * G2                 # the invariant, and every game ended
    return tally, ct, out[2], ro


def test_every_game_passed_after_one_ply():
    tally, ct, _, _ = run128(by_mover(1.0, -1.0), start_mover=1)
    n = B128 * G2
    assert ct.tolist() == [n, -n, n, 0, n, n, 0, n] and not tally.any()


def test_one_take_per_game():
    tally, ct, _, _ = run128(by_mover(0.45, -1.0))
    n = B128 * G2
    s1, s2 = points(tally)
    assert tally[GAMES] == n and ct.tolist() == [n, 2 * s1, 4 * s2, n, 0, 0, 0, n]


def test_redoubles_up_to_the_cap():
    tally, ct, _, _ = run128(by_mover(0.45, 0.45), cap=3)
    n = B128 * G2
    s1, s2 = points(tally)
    assert tally[GAMES] == n and ct.tolist() == [n, 8 * s1, 64 * s2, 3 * n, 0, 0, 0, 3 * n]


@pytest.mark.parametrize("jacoby", [True, False])
def test_jacoby_reduces_an_undoubled_gammon(jacoby):
    starts = torch.from_numpy(CASE_B)[None].repeat(B128, 1)
    tally, ct, _, _ = run128(by_mover(-1.0, -1.0), starts=starts, jacoby=jacoby)
    n = B128 * G2
    assert tally.tolist() == [n, n, 0, n, 0, 0, 0, 0]
    assert ct.tolist() == [n, n if jacoby else 2 * n, n if jacoby else 4 * n, 0, 0, 0, 0, 0]


def test_no_double_leaves_the_games_alone():
    """double_at = +inf with a net's value head: the equity is computed, nobody doubles, and the
    plain tally, games_done and the traced actions are those of the run without the cube."""
    from bgx.arena import RandomPlayer
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout
    from bgx.search import ValueHead
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    tally, ct, tr, _ = run128(vh, trace=True, double_at=math.inf)
    s1, s2 = points(tally)
    assert ct.tolist() == [B128 * G2, s1, s2, 0, 0, 0, 0, 0]
    assert tr["cube_dsel"].any() and not tr["cube_mask"].any() and not tr["cube"].any()
    on = tr["cube_dsel"] != 0
    assert torch.isfinite(tr["cube_equity"][on]).all() and torch.isnan(tr["cube_equity"][~on]).all()
    ro = Rollout(B128, seed=3)
    plain = ro.run_lanes(RandomPlayer(11), opening(0, B128), torch.zeros(B128, dtype=torch.int32), 1, G2, max_steps=6000,
                         trace=True)
    assert len(plain) == 3 and "cube" not in plain[2]
    assert np.array_equal(plain[0].cpu().numpy()[0], tally)
    assert torch.equal(plain[2]["games_done"], tr["games_done"])
    n = tr["done"].shape[0]                 # the cube run reads the active count every step and stops at once
    assert plain[2]["done"].shape[0] >= n
    for k in ("action", "mover", "done", "info"):
        assert torch.equal(plain[2][k][:n], tr[k]), k


# --------------------------------------------------- a traced run against the host replay --
# A fresh net's value says little about the position: on the opening's early plies the side on
# roll's 21-roll mean lies between 0.09 and 0.24, with the quartiles at 0.145, 0.16 and 0.18 (the
# quantiles the test prints).  The thresholds sit inside that range, so that most decisions are
# doubles and a fifth of them passes; the test asserts that takes, passes and redoubles all occur.
TRACED = dict(double_at=0.13, pass_at=0.19, cap=4)


def test_traced_run_equals_cube_reference():
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule, cube_reference, pack
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout
    from bgx.search import ValueHead
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    B, P, G = 64, 3, 2
    group = np.repeat(np.arange(3), [20, 21, 20]).astype(np.int32)
    for k in (7, 30, 50):
        group = np.insert(group, k, -1)
    starts = opening(0, B)
    starts[1::2, 52] = 1
    cube0 = np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)]
    rule = CubeRule(vh, jacoby=True, **TRACED)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=5)
        out = ro.run_lanes(RandomPlayer(2), starts, torch.from_numpy(group), P, G, max_steps=6000, trace=True, cube=rule,
                           cube0=torch.from_numpy(cube0))
        assert ro.eng.error() == 0 and not out[1].any()
        runs.append(out)
    tally, _, tr, ct = runs[0]
    tally, ct = tally.cpu().numpy(), ct.cpu().numpy()
    e = tr["cube_equity"][tr["cube_dsel"] != 0].cpu().numpy()
    print("cube equity quantiles", np.quantile(e, [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1]).tolist(), "tally", ct.tolist())
    ref = cube_reference(tr, starts, group, P, G, rule, cube0)
    assert np.array_equal(ct, ref["cube_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["cube"].cpu().numpy(), ref["cube"])
    assert np.array_equal(tr["cube_dsel"].cpu().numpy() != 0, ref["dsel"])
    assert np.array_equal(tr["cube_mask"].cpu().numpy() != 0, ref["mask"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    assert np.array_equal(ct[:, CG], tally[:, GAMES] + ct[:, PG])
    # takes, passes and redoubles all occur
    takes = ct[:, DBL].sum() - ct[:, PG].sum()
    assert ct[:, PG].sum() > 0 and takes > 0 and (tr["cube"].cpu().numpy() & 15).max() >= 3
    assert not tr["cube_dsel"][:, torch.from_numpy(group < 0).cuda()].any()
    # run to run identical
    assert torch.equal(runs[1][3], runs[0][3]) and torch.equal(runs[1][0], runs[0][0])
    for k in ("cube", "cube_dsel", "cube_mask", "action"):
        assert torch.equal(runs[1][2][k], tr[k]), k
    assert torch.equal(runs[1][2]["cube_equity"].nan_to_num(7.0), tr["cube_equity"].nan_to_num(7.0))


# ------------------------------------------------------------------------- other checks --
@pytest.mark.parametrize("owner", [1, 2])
def test_cube_start(owner):
    """Every game starts at 2 owned by `owner`; only PLAYER1 would ever double (E = 0.45 against
    -1): owned by PLAYER1 there is one more take a game, owned by PLAYER2 none."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout, opening_record
    ro = Rollout(B128, seed=6)
    r, = ro.run(RandomPlayer(1), opening_record()[None], 72, max_steps=6000, cube=CubeRule(by_mover(0.45, -1.0)),
                cube_start=(1, owner))
    n = r["games"]
    assert n == 72 and r["unfinished"] == 0 and r["pass_games"] == 0 and r["played_out"]["games"] == n
    k = 2 if owner == 1 else 1
    assert r["doubles"] == (n if owner == 1 else 0) and r["cube_log2"] == k * n and r["mean_cube_log2"] == k
    assert r["equity_cubeful"] == pytest.approx((1 << k) * r["played_out"]["equity"], rel=1e-12)
    assert r["plies_per_game"] == pytest.approx(r["played_out"]["plies_per_game"], rel=1e-12)


def test_cube_decision_forced():
    """A callable equity forces the answer.  The opponent (PLAYER2) always feels -1 and never
    redoubles; PLAYER1's rollouts are the cubeless games times the cube, so double_take = 2 x
    no_double up to the two samples' noise: on a certain gammon (CASE_B, 2 points a game) that is
    no_double = 2, double_take = 4: a double and a pass."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule, rollout_cube_decision
    from bgx.rollout import Rollout
    ro = Rollout(B128, seed=6)
    rule = CubeRule(by_mover(-1.0, -1.0))
    d = rollout_cube_decision(ro, RandomPlayer(1), torch.from_numpy(CASE_B), 72, rule)
    assert (d["no_double"], d["double_take"], d["double_pass"]) == (2.0, 4.0, 1.0)
    assert d["no_double_stderr"] == d["double_take_stderr"] == 0.0
    assert d["double"] is False and d["take"] is False           # too good to double: 2 > min(4, 1); a take would cost 4
    assert [r["games"] for r in d["rollouts"]] == [72, 72] and d["rollouts"][1]["cube_log2"] == 72
    # with the cube at 2 in the mover's hands the units halve the same way
    d2 = rollout_cube_decision(ro, RandomPlayer(1), torch.from_numpy(CASE_B), 72, rule, cube=(1, 1))
    assert (d2["no_double"], d2["double_take"]) == (2.0, 4.0) and d2["rollouts"][0]["equity_cubeful"] == 4.0
    # PLAYER2 on roll and sure to lose a gammon at once: no double, and a take is right
    lost = CASE_B.copy()
    lost[52] = 1
    lost[24 + 5], lost[24 + 12] = 0, 15                      # PLAYER2's 15 checkers in the outfield: none gets off in time
    d3 = rollout_cube_decision(ro, RandomPlayer(1), torch.from_numpy(lost), 72, rule)
    assert (d3["no_double"], d3["double_take"]) == (-2.0, -4.0) and d3["double"] is False and d3["take"] is True
    for bad in ((0, 1), (1, 2), (6, 1)):                       # not a state / the opponent's cube / at the cap
        with pytest.raises(ValueError):
            rollout_cube_decision(ro, RandomPlayer(1), torch.from_numpy(CASE_B), 72, rule, cube=bad)


def test_unsupported_combinations():
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout, opening_record
    from bgx.search import ValueHead
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    ro = Rollout(64, seed=0)
    rule = CubeRule(vh)
    starts, grp = opening(0, 64), torch.zeros(64, dtype=torch.int32)

    class FakeDB:                               # the combination is refused before the table is looked at
        pass

    for kw, word in ((dict(luck=vh), "luck"), (dict(bearoff=FakeDB()), "bearoff")):
        with pytest.raises(ValueError, match=f"cube together with {word}"):
            ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=rule, **kw)
        with pytest.raises(ValueError, match=f"cube together with {word}"):
            ro.run(RandomPlayer(1), opening_record()[None], 36, cube=rule, **kw)
    with pytest.raises(ValueError, match="cube0 without cube"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube0=torch.zeros(64, dtype=torch.uint8))
    bad = torch.zeros(64, dtype=torch.uint8)
    bad[9] = 0x13                               # owner 1 with k = 3 is fine; k = 3 centred is not
    bad[12] = 0x03
    with pytest.raises(ValueError, match="cube0: lane 12 holds 3 "):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=rule, cube0=bad)
    with pytest.raises(ValueError, match="float32"):
        ro.run_lanes(RandomPlayer(1), starts, grp, 1, 1, cube=CubeRule(lambda eng, dsel: torch.zeros(64).double().cuda()))
    torch.cuda.synchronize()


def test_command_line(tmp_path, capsys):
    from bgx import rollout
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    ckpt = str(tmp_path / "net.pt")
    torch.save(PolicyNet(hidden_size=40).state_dict(), ckpt)
    base = ["--net", ckpt, "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps", "6000",
            "--cube", "--cube-double", "0.13", "--cube-pass", "0.19", "--cube-cap", "4", "--jacoby"]
    rollout.main(base)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["position"] == 0 and lines[1]["summary"] and lines[1]["cube"] is True
    r = lines[0]
    assert r["games"] + r["unfinished"] == 72 and r["games"] == r["played_out"]["games"] + r["pass_games"]
    for k in ("equity_cubeful", "equity_cubeful_stderr", "pass_share", "doubles_per_game", "mean_cube_log2",
              "plies_per_game"):
        assert math.isfinite(r[k]), k
    assert lines[1]["games"] == r["games"] and lines[1]["pass_share"] == r["pass_share"]
    assert (lines[1]["cube_cap"], lines[1]["jacoby"], lines[1]["cube_double"]) == (4, True, 0.13)
    rollout.main(base + ["--cube-decision", "--cube-net", ckpt])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["cube_decision"] is True and lines[1]["cube_decision"] is True
    d = lines[0]
    assert d["double_pass"] == 1.0 and d["double"] == (min(d["double_take"], 1.0) > d["no_double"])
    assert d["take"] == (d["double_take"] <= 1.0) and len(d["rollouts"]) == 2
    assert lines[1]["games"] == sum(x["games"] for x in d["rollouts"]) and lines[1]["positions"] == 1
