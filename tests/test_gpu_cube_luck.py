"""Luck-adjusted cubeful rollouts on the device: bgx_roll_values against
bgx_roll_luck, bgx_cube_roll_luck against cube.cube_roll_luck_reference bit for bit, the three
bookkeeping kernels of csrc/bg_cube_luck.h against the host replay, a dead cube against the cubeless
luck= run, a traced run against cube.cube_luck_reference, mean zero, the cube decision, graph
capture and the command line."""
import ctypes
import importlib.util
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 65536
CG, CP, CP2, CLOG, PG, PP, PW, DBL = range(8)
LUCK, LO, HI, YLUCK, LGAMES = range(5)
ROLLS21 = [(a, b) for a in range(1, 7) for b in range(a, 7)]
# the thresholds of tests/test_gpu_cube.py's traced run: a fresh H = 40 net's 21-roll mean on the
# opening's early plies lies between 0.09 and 0.24, so most decisions double and a fifth passes
TRACED = dict(double_at=0.13, pass_at=0.19, cap=4)


def _module(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                          name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.int32)


def same(a, b):
    """Bit for bit, except that a NaN is a NaN (its sign and payload are the adder's own business)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def opening(mover, B):
    from bgx.rollout import opening_record
    r = opening_record().clone()
    r[52] = mover
    return r[None].repeat(B, 1)


@pytest.fixture(scope="module")
def net():
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    return PolicyNet(hidden_size=40).cuda()


@pytest.fixture(scope="module")
def vh(net):
    from bgx.search import ValueHead
    return ValueHead(net)


def chain_exact(g):
    """fma(p_20, g_20, ... fma(p_0, g_0, 0)) in fp32 with rationals, one rounding per step."""
    mean = F(0)
    for r, (a, b) in enumerate(ROLLS21):
        p = F(1) / F(36) if a == b else F(2) / F(36)
        q = Fraction(float(p)) * Fraction(float(g[r])) + Fraction(float(mean))
        lo = F(float(q))
        cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        mean = min(cands, key=lambda t: (abs(Fraction(float(t)) - q), int(F(t).view(np.int32)) & 1))
    return mean


# --------------------------------------------------------------------- 1. bgx_roll_values --
@pytest.mark.parametrize("H", [40, 128])
def test_roll_values_are_roll_lucks(golden, H):
    """B = 256 on the posed records of tests/test_gpu_roll_luck.py: the exact FMA chain over a row of
    values is bgx_roll_luck's mean, the row's entry of the lane's roll minus it its luck, bit for bit."""
    from bgx import _lib
    from bgx.cube import ROLL_P, fma32, roll_index
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead, roll_luck, roll_values
    RL = _module("test_gpu_roll_luck")
    B = RL.B
    net = PolicyNet(hidden_size=H).cuda()
    pre = f"h{H}_"
    net.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in golden("mlp").items()
                         if k.startswith(pre) and not k.endswith(("logits", "values"))})
    vh = ValueHead(net)
    eng = RL.make_engine()
    rec = eng.records().cpu().numpy()
    assert np.array_equal(rec[:3, :55], RL.POSED[:, :55])
    luck, mean, st_l = roll_luck(eng, vh)
    values, st_v = roll_values(eng, vh)
    assert values.shape == (B, 21) and values.dtype == torch.float32 and st_v == st_l and st_v["rows"] == B
    v = values.cpu().numpy()
    assert np.isfinite(v).all()
    m = np.zeros(B, F)
    for r in range(21):
        m = fma32(ROLL_P[r], v[:, r], m)
    assert np.array_equal(bits(m), bits(mean.cpu().numpy()))
    for i in (0, 1, 2, 17, 255):                            # the vectorised chain against rationals
        assert chain_exact(v[i]) == m[i]
    idx = roll_index(rec[:, 53:55])
    assert (idx >= 0).all()
    assert np.array_equal(bits((v[np.arange(B), idx] - m).astype(F)), bits(luck.cpu().numpy()))
    # nobody enters from the bar: every roll's value is the position's own; the others are not degenerate
    assert np.ptp(v[0]) == 0.0 and np.ptp(v[1]) > 0 and np.ptp(v[2]) > 0
    # a selection: the selected rows bit for bit, the others keep the caller's sentinel (or NaN)
    rng = np.random.RandomState(3)
    sel = torch.from_numpy((rng.rand(B) < 0.4).astype(np.uint8)).cuda()
    on = sel.bool()
    v2, st2 = roll_values(eng, vh, sel=sel)
    assert torch.isnan(v2[~on]).all() and torch.equal(v2[on], values[on])
    assert st2["rows"] == int(on.sum()) and st2["jobs"] == 21 * st2["rows"] and 0 < st2["leaves"] < st_v["leaves"]
    keep = torch.full((B, 21), 7.0, device="cuda")
    v3, _ = roll_values(eng, vh, sel=sel, out=keep)
    assert v3 is keep and bool((keep[~on] == 7.0).all()) and torch.equal(keep[on], values[on])
    v4, st4 = roll_values(eng, vh, sel=torch.zeros(B, dtype=torch.uint8, device="cuda"), out=keep.clone())
    assert torch.equal(v4, keep) and st4 == {"leaves": 0, "jobs": 0, "rows": 0}
    with pytest.raises(ValueError, match="float32\\[B, 21\\]"):
        roll_values(eng, vh, out=torch.zeros(B, 20, device="cuda"))
    # the C entry point's argument checks: bgx_roll_luck's
    L = _lib.load()
    out = torch.zeros(B, 21, device="cuda")
    good = [eng._h, vh.packed.data_ptr(), vh.hidden, vh.bias, None, out.data_ptr(), None, None]
    assert L.bgx_roll_values(*good) == _lib.BGX_OK
    for k, val in ((0, None), (1, None), (5, None), (2, 0), (2, 129)):
        bad = list(good)
        bad[k] = val
        assert L.bgx_roll_values(*bad) == _lib.BGX_EINVAL, k
    torch.cuda.synchronize()
    assert torch.equal(out, values) and eng.error() == 0


# ------------------------------------------------------------------ 2. bgx_cube_roll_luck --
LIVES = [(0.68, 1.0, 1.0, 6, 1.0), (1.0, 1.3, 1.2, 10, 1.3), (0.0, 3.0, 3.0, 1, 1.0)]        # x, W, L, cap, scale


def luck_inputs(n, W, L, seed):
    rng = np.random.RandomState(seed)
    recs = np.zeros((n, 64), np.uint8)
    recs[:, 52] = rng.randint(2, size=n)
    recs[:, 53:55] = rng.randint(1, 7, size=(n, 2))
    recs[rng.choice(n, 12, replace=False), 53:55] = [(0, 0), (0, 3), (7, 2)] * 4          # no roll
    recs[rng.choice(n, 9, replace=False), 55] = 1                                          # game_over
    cube = rng.randint(256, size=n).astype(np.uint8)
    cube[::5] = np.array([0, 0x11, 0x21, 0x12, 0x25, 0x16, 0x2A, 0x31], np.uint8)[rng.randint(8, size=len(cube[::5]))]
    v = rng.uniform(-1.5 * W, 1.5 * L, size=(n, 21)).astype(F)
    up, down = lambda e: np.nextafter(F(e), F(np.inf)), lambda e: np.nextafter(F(e), F(-np.inf))
    D = W + L + 0.5
    special = [F(np.nan), F(np.inf), F(-np.inf), F(0.0), F(-0.0)]
    for p in ((L - 0.5) / D, (L + 1.0) / D, 0.2, 0.8, 0.0, 1.0):
        e = F(-(p * (W + L) - L))                           # the mover's value where the opponent sits at p
        special += [e, up(e), down(e)]
    special = np.array(special, F)
    for k, i in enumerate(range(3, n, 4)):                  # every fourth row sits on the breakpoints
        v[i] = special[(k * 7 + 3 * np.arange(21)) % len(special)]
    v[rng.randint(n, size=40), rng.randint(21, size=40)] = special[rng.randint(5, size=40)]
    sel = (rng.rand(n) < 0.85).astype(np.uint8)
    return recs, cube, v, sel


@pytest.mark.parametrize("jacoby", [0, 1])
@pytest.mark.parametrize("li", range(len(LIVES)))
def test_cube_roll_luck_bit_for_bit(li, jacoby):
    from bgx import _lib
    from bgx.cube import CubeLife, cube_roll_luck_reference
    L = _lib.load()
    n = 300
    x, W, Lv, cap, scale = LIVES[li]
    life = CubeLife(x, W, Lv)
    recs, cube, v, sel = luck_inputs(n, W, Lv, 10 + li)
    d_recs, d_cube, d_v, d_sel = dev(recs), dev(cube), dev(v), dev(sel)
    wrote = 0
    for use_cube, use_sel, use_mean in ((1, 1, 1), (0, 1, 1), (1, 0, 0), (0, 0, 1)):
        want_l, want_m = cube_roll_luck_reference(v, cube if use_cube else None, recs[:, 52], recs[:, 53:55], scale, life,
                                                  cap, bool(jacoby))
        on = (recs[:, 55] == 0) & ((sel != 0) | (not use_sel))
        luck, mean = torch.full((n,), 7.0).cuda(), torch.full((n,), 9.0).cuda()
        assert L.bgx_cube_roll_luck(ptr(d_recs), ptr(d_cube) if use_cube else None, ptr(d_v), n, scale, life.struct(), cap,
                                    jacoby, ptr(d_sel) if use_sel else None, ptr(luck), ptr(mean) if use_mean else None,
                                    None) == _lib.BGX_OK
        gl, gm = luck.cpu().numpy(), mean.cpu().numpy()
        assert np.array_equal(bits(gl[on]), bits(want_l[on])) and (gl[~on] == 7.0).all()
        assert np.array_equal(bits(gm[on]), bits(want_m[on])) if use_mean else (gm == 9.0).all()
        assert (gm[~on] == 9.0).all() and 0 < (~on).sum() < n
        noroll = on & ((recs[:, 53:55].min(axis=1) < 1) | (recs[:, 53:55].max(axis=1) > 6))
        assert noroll.sum() >= 5 and (gl[noroll] == 0.0).all()
        wrote += int((gl[on] != 0).sum())
    assert wrote > 600
    good = [ptr(d_recs), ptr(d_cube), ptr(d_v), n, 1.0, life.struct(), 6, jacoby, ptr(d_sel), ptr(luck), ptr(mean), None]
    assert L.bgx_cube_roll_luck(*good) == _lib.BGX_OK
    bad_lives = [_lib.BgxCubeLife(1.5, 1.0, 1.0), _lib.BgxCubeLife(-0.1, 1.0, 1.0), _lib.BgxCubeLife(0.5, 0.5, 1.0),
                 _lib.BgxCubeLife(0.5, 1.0, 3.5), _lib.BgxCubeLife(0.5, 1.0, math.nan), _lib.BgxCubeLife(math.nan, 1.0, 1.0)]
    for k, val in [(0, None), (2, None), (9, None), (3, 0), (3, -5), (4, math.nan), (6, -1), (6, 11)] + \
            [(5, b) for b in bad_lives]:
        args = list(good)
        args[k] = val
        assert L.bgx_cube_roll_luck(*args) == _lib.BGX_EINVAL, k
    torch.cuda.synchronize()


# ------------------------------------------------------------- 3. add, pass and flush alone --
def book_state(seed=7):
    """300 lanes: six unequal groups that share waves, seven idle lanes and three with a group beyond
    n_groups, retired lanes, last games, every cube state up to k = cap = 10, sums at the clamp and
    not finite."""
    from bgx.cube import pack
    rng = np.random.RandomState(seed)
    B, P, G, cap = 300, 6, 2, 10
    group = np.repeat(np.arange(6), [10, 50, 33, 64, 36, 100]).astype(np.int32)
    for k in (3, 40, 41, 99, 130, 131, 190):
        group = np.insert(group, k, -1)
    assert len(group) == B
    group[[20, 150, 280]] = P + 3
    valid = (group >= 0) & (group < P)
    recs, starts = np.zeros((B, 64), np.uint8), np.zeros((B, 64), np.uint8)
    recs[:, 52], starts[:, 52] = rng.randint(2, size=B), rng.randint(2, size=B)
    recs[:, 53:55] = rng.randint(1, 7, size=(B, 2))
    starts[1::3, 53:55] = rng.randint(1, 7, size=(len(starts[1::3]), 2))              # fixed first rolls
    states = [0] + [pack(k, o) for k in (1, 2, 5, 9, 10) for o in (1, 2)]
    cube = np.array(states, np.uint8)[rng.randint(len(states), size=B)]
    cube[[8, 88, 188]] = [0x0F, 0x31, 0x07]                                            # read as (10, 0), (1, 0), (7, 0)
    cube0 = np.array(states, np.uint8)[rng.randint(len(states), size=B)]
    plies = rng.randint(0, 4, size=B).astype(np.int32)
    games_done = rng.randint(0, G, size=B).astype(np.int32)
    games_done[valid & (rng.rand(B) < 0.12)] = G                                       # retired lanes
    sel = (valid & (games_done < G)).astype(np.uint8)
    lane_luck = (rng.standard_normal(B) * 3).astype(F)
    lane_luck[lane_luck == 0] = F(0.5)
    lane_luck[[12, 60, 61, 200, 201, 250]] = [40000.0, -40000.0, np.inf, np.nan, -np.inf, 32767.99]
    luck = rng.standard_normal(B).astype(F)
    luck[[5, 70]] = [np.nan, np.inf]
    palette = np.array([0.4, 0.5, np.nan, 0.95, np.nextafter(F(0.5), F(1)), 0.9, 0.45, 0.7, -0.3, np.inf, 0.6, 0.55], F)
    equity = palette[rng.randint(len(palette), size=B)]
    done = (rng.rand(B) < 0.6).astype(np.uint8)
    winner, score = rng.randint(-1, 2, size=B), rng.randint(1, 4, size=B)
    # k = 10 with three points, for either side, with the sums that matter
    for i, w in ((12, 0), (60, 1), (61, 0), (250, 1)):
        cube[i], done[i], winner[i], score[i], plies[i], equity[i] = pack(10, 1 + (i & 1)), 1, w, 3, 2, -0.3
        games_done[i], sel[i] = G - 1, 1
        assert valid[i]
    info = (((winner + 1) << 8) | (score << 16)).astype(np.int32)
    return dict(B=B, P=P, G=G, cap=cap, group=group, recs=recs, starts=starts, cube=cube, cube0=cube0, plies=plies,
                games_done=games_done, sel=sel, lane_luck=lane_luck, luck=luck, equity=equity, done=done, info=info)


def book_rule():
    from bgx.cube import CubeRule
    return CubeRule(lambda e, d: None, scale=1.0, double_at=0.4, pass_at=0.5, too_good_at=0.9, cap=10, jacoby=True)


def book_device(s):
    t = {k: dev(s[k]) for k in ("group", "recs", "starts", "cube", "cube0", "plies", "games_done", "sel", "lane_luck", "luck",
                                "equity", "done", "info")}
    B, P = s["B"], s["P"]
    t.update(dsel=torch.full((B,), 9, dtype=torch.uint8).cuda(), mask=torch.full((B,), 9, dtype=torch.uint8).cuda(),
             cube_tally=torch.zeros(P, 8, dtype=torch.int64).cuda(), luck_tally=torch.zeros(P, 5, dtype=torch.int64).cuda(),
             active=torch.tensor([int(s["sel"].sum())]).cuda())
    return t


def book_calls(L, s, t, st=None, snapshots=None):
    """cube_sel; cube_luck_pass, cube_decide; cube_luck_add; cube_luck_flush, cube_flush -- the loop's
    order without the players.  `snapshots`: the lane sums after each luck kernel."""
    from bgx import _lib
    B, P, G, cap = s["B"], s["P"], s["G"], s["cap"]
    rs = book_rule().struct()
    snap = (lambda name: snapshots.__setitem__(name, t["lane_luck"].clone())) if snapshots is not None else (lambda name: None)
    ok = _lib.BGX_OK
    assert L.bgx_rollout_cube_sel(ptr(t["recs"]), ptr(t["group"]), P, ptr(t["plies"]), ptr(t["sel"]), ptr(t["cube"]), B, cap,
                                  ptr(t["dsel"]), st) == ok
    assert L.bgx_rollout_cube_luck_pass(ptr(t["recs"]), ptr(t["starts"]), ptr(t["group"]), ptr(t["dsel"]), ptr(t["equity"]),
                                        B, P, rs, ptr(t["cube"]), ptr(t["lane_luck"]), ptr(t["luck_tally"]), st) == ok
    snap("pass")
    if snapshots is not None:
        snapshots["pass_tally"] = t["luck_tally"].clone()
    assert L.bgx_rollout_cube_decide(ptr(t["recs"]), ptr(t["starts"]), ptr(t["group"]), ptr(t["dsel"]), ptr(t["equity"]), B,
                                     P, G, rs, ptr(t["cube0"]), ptr(t["cube"]), ptr(t["games_done"]), ptr(t["plies"]),
                                     ptr(t["sel"]), ptr(t["cube_tally"]), ptr(t["active"]), ptr(t["mask"]), st) == ok
    assert L.bgx_rollout_cube_luck_add(ptr(t["recs"]), ptr(t["starts"]), ptr(t["plies"]), ptr(t["sel"]), ptr(t["cube"]),
                                       ptr(t["luck"]), B, cap, ptr(t["lane_luck"]), st) == ok
    snap("add")
    assert L.bgx_rollout_cube_luck_flush(ptr(t["starts"]), ptr(t["group"]), ptr(t["sel"]), ptr(t["done"]), ptr(t["info"]), B,
                                         P, cap, 1, ptr(t["cube"]), ptr(t["lane_luck"]), ptr(t["luck_tally"]), st) == ok
    snap("flush")
    assert L.bgx_rollout_cube_flush(ptr(t["starts"]), ptr(t["group"]), ptr(t["sel"]), ptr(t["done"]), ptr(t["info"]), B, P, rs,
                                    ptr(t["cube0"]), ptr(t["cube"]), ptr(t["cube_tally"]), st) == ok


def test_bookkeeping_kernels_equal_the_host_replay():
    from bgx import _lib
    from bgx.cube import decide_reference, sanitise
    from bgx.replay import LaneReplay, cube_luck_q
    from bgx.tally import CUBE_FIELDS, CUBE_LUCK_FIELDS
    L = _lib.load()
    s = book_state()
    rule = book_rule()
    B, P, G, cap = s["B"], s["P"], s["G"], s["cap"]
    runs = []
    for _ in range(2):
        t, snaps = book_device(s), {}
        book_calls(L, s, t, snapshots=snaps)
        torch.cuda.synchronize()
        runs.append((t, snaps))
    t, snaps = runs[0]
    # the replay, from the same state
    rp = LaneReplay(s["starts"], s["group"], P, G, cap=cap, c0=sanitise(s["cube0"], cap), jacoby=True)
    rp.tally("cube_tally", CUBE_FIELDS)
    rp.tally("cube_luck_tally", CUBE_LUCK_FIELDS)
    rp.cube, rp.plies, rp.games = s["cube"].copy(), s["plies"].astype(np.int64), s["games_done"].astype(np.int64)
    rp.luck = s["lane_luck"].copy()
    assert np.array_equal(rp.sel, s["sel"] != 0)
    mover = s["recs"][:, 52]
    dsel, passed = rp.decide(mover, *decide_reference(rp.cube, mover, s["equity"], rule))
    assert np.array_equal(t["dsel"].cpu().numpy() != 0, dsel)
    # the pass kernel saw what cube_decide then did: the lanes it cleared are the reset mask, on every lane
    after_pass = snaps["pass"].cpu().numpy()
    mask = t["mask"].cpu().numpy()
    assert np.array_equal(mask != 0, passed) and passed.sum() > 20
    assert np.array_equal(after_pass == 0, mask != 0)
    assert np.array_equal(bits(after_pass[~passed]), bits(s["lane_luck"][~passed]))
    assert np.array_equal(snaps["pass_tally"].cpu().numpy(), rp.tallies["cube_luck_tally"])
    assert rp.tallies["cube_luck_tally"][:, LGAMES].sum() == passed.sum()
    rp.cube_luck_add(s["luck"], mover)
    assert same(snaps["add"].cpu().numpy(), rp.luck)
    changed = bits(snaps["add"].cpu().numpy()) != bits(after_pass)
    skipped = rp.sel & (rp.plies == 0) & (s["starts"][:, 53] != 0)
    assert skipped.sum() > 10 and not changed[skipped].any() and not changed[~rp.sel].any() and changed.sum() > 100
    sel_before_flush = rp.sel.copy()
    rp.advance(s["done"], s["info"])
    assert np.array_equal(t["luck_tally"].cpu().numpy(), rp.tallies["cube_luck_tally"])
    assert np.array_equal(t["cube_tally"].cpu().numpy(), rp.tallies["cube_tally"])
    assert np.array_equal(t["luck_tally"].cpu().numpy()[:, LGAMES], t["cube_tally"].cpu().numpy()[:, CG])
    assert same(snaps["flush"].cpu().numpy(), rp.luck)
    dn = sel_before_flush & (s["done"] != 0)
    assert (snaps["flush"].cpu().numpy()[dn] == 0).all() and dn.sum() > 50
    assert np.array_equal(t["cube"].cpu().numpy(), rp.cube)
    # the cases the state was built for: |y| = 3072 against a sum at the clamp, and sums that are not finite
    lt = t["luck_tally"].cpu().numpy()
    assert cube_luck_q(s["lane_luck"][[12, 60, 61, 200, 201]]).tolist() == [2 ** 31, -2 ** 31, 0, 0, 0]
    assert lt[:, HI].max() >= 2 ** 32 and np.abs(t["cube_tally"].cpu().numpy()[:, CP2]).max() >= 3072 ** 2
    assert (lt[:, LGAMES] > 0).all() and (lt[:, LO] > 0).all()
    # lanes that are idle, beyond n_groups or retired were never touched
    off = s["sel"] == 0
    assert off.sum() > 30 and np.array_equal(bits(snaps["flush"].cpu().numpy()[off]), bits(s["lane_luck"][off]))
    # run to run identical
    for k in ("luck_tally", "cube_tally", "lane_luck", "cube", "mask"):
        assert torch.equal(runs[1][0][k].view(torch.uint8), t[k].view(torch.uint8)), k


def test_bookkeeping_argument_checks():
    from bgx import _lib
    L = _lib.load()
    s = book_state()
    t = book_device(s)
    B, P = s["B"], s["P"]
    rs = book_rule().struct()

    def bad_rule(**kw):
        r = book_rule().struct()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    rules = [bad_rule(scale=math.nan), bad_rule(double_at=math.nan), bad_rule(pass_at=math.nan), bad_rule(cap=11),
             bad_rule(cap=-1)]
    good = [ptr(t[k]) for k in ("recs", "starts", "plies", "sel", "cube", "luck")] + [B, 10, ptr(t["lane_luck"]), None]
    assert L.bgx_rollout_cube_luck_add(*good) == _lib.BGX_OK
    for k, val in [(i, None) for i in (0, 1, 2, 3, 4, 5, 8)] + [(6, 0), (7, -1), (7, 11)]:
        args = list(good)
        args[k] = val
        assert L.bgx_rollout_cube_luck_add(*args) == _lib.BGX_EINVAL, k
    good = [ptr(t[k]) for k in ("recs", "starts", "group", "dsel", "equity")] + [B, P, rs] + \
        [ptr(t[k]) for k in ("cube", "lane_luck", "luck_tally")] + [None]
    t["dsel"].zero_()
    assert L.bgx_rollout_cube_luck_pass(*good) == _lib.BGX_OK
    for k, val in [(i, None) for i in (0, 1, 2, 3, 4, 8, 9, 10)] + [(5, 0), (6, 0)] + [(7, r) for r in rules]:
        args = list(good)
        args[k] = val
        assert L.bgx_rollout_cube_luck_pass(*args) == _lib.BGX_EINVAL, k
    good = [ptr(t[k]) for k in ("starts", "group", "sel", "done", "info")] + [B, P, 10, 1] + \
        [ptr(t[k]) for k in ("cube", "lane_luck", "luck_tally")] + [None]
    t["done"].zero_()
    assert L.bgx_rollout_cube_luck_flush(*good) == _lib.BGX_OK
    for k, val in [(i, None) for i in (0, 1, 2, 3, 4, 9, 10, 11)] + [(5, 0), (6, 0), (7, -1), (7, 11)]:
        args = list(good)
        args[k] = val
        assert L.bgx_rollout_cube_luck_flush(*args) == _lib.BGX_EINVAL, k
    torch.cuda.synchronize()
    assert not t["luck_tally"].any()


# ------------------------------------------------------ 4. a dead cube is the cubeless luck --
def test_dead_cube_is_the_cubeless_luck(vh):
    """cap = 0: nobody can double and Janowski's equity is the clamped value itself; with W = L = 3,
    scale 1 and a net whose values stay inside +-3 the cubeful luck of every roll is the cubeless one,
    so the tallies of a cube_luck= run are those of the luck= run on the same seed, integer for integer."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLife, CubeLuck, CubeRule
    from bgx.rollout import Rollout
    from bgx.search import roll_values
    B, P, G = 128, 2, 2
    group = (np.arange(B) >= 70).astype(np.int32)
    starts = opening(0, B)
    starts[1::2, 52] = 1
    starts[::3, 53], starts[::3, 54] = 4, 2                  # fixed first rolls on a third of the lanes
    ro = Rollout(B, seed=8)
    tally_l, unf_l, tr_l, lt = ro.run_lanes(RandomPlayer(4), starts, torch.from_numpy(group), P, G, max_steps=6000, trace=True,
                                            luck=vh)
    ro = Rollout(B, seed=8)
    cl = CubeLuck(vh, scale=1.0, life=CubeLife(0.68, 3.0, 3.0))
    tally_c, unf_c, tr_c, ct, clt = ro.run_lanes(RandomPlayer(4), starts, torch.from_numpy(group), P, G, max_steps=6000,
                                                 trace=True, cube=CubeRule(vh, cap=0), cube_luck=cl)
    assert ro.eng.error() == 0 and not unf_l.any() and not unf_c.any()
    vals = tr_c["cube_luck_values"]
    seen = ~torch.isnan(vals)
    assert bool(seen.any()) and float(vals[seen].abs().max()) < 3.0         # inside +-3: the clamp never acts
    assert float(roll_values(ro.eng, vh)[0].abs().max()) < 3.0
    assert torch.equal(tally_c, tally_l) and torch.equal(tr_c["action"], tr_l["action"])
    n = tr_c["done"].shape[0]
    assert tr_l["done"].shape[0] == n
    assert torch.equal(tr_c["cube_luck"].view(torch.int32), tr_l["luck"].view(torch.int32))      # every step's luck
    lt, clt, ct = lt.cpu().numpy(), clt.cpu().numpy(), ct.cpu().numpy()
    assert np.array_equal(clt[:, LUCK], lt[:, 0]) and np.array_equal(clt[:, YLUCK], lt[:, 2])
    assert np.array_equal((clt[:, HI] << 30) + clt[:, LO], lt[:, 1]) and (lt[:, 1] > 0).all()
    assert np.array_equal(clt[:, LGAMES], lt[:, 3]) and np.array_equal(clt[:, LGAMES], ct[:, CG])
    assert not ct[:, DBL].any() and not tr_c["cube_dsel"].any() and clt[:, LGAMES].sum() == (70 + 58) * G


# ------------------------------------------------------- 5. a traced run against the replay --
def test_traced_run_equals_cube_luck_reference(vh):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLife, CubeLuck, CubeRule, cube_luck_reference, cube_roll_luck_reference, pack
    from bgx.rollout import Rollout
    B, P, G, steps = 64, 3, 2, 160
    group = np.repeat(np.arange(3), [20, 21, 20]).astype(np.int32)
    for k in (7, 30, 50):
        group = np.insert(group, k, -1)
    starts = opening(0, B)
    starts[1::2, 52] = 1
    starts[::4, 53], starts[::4, 54] = 3, 1                  # a quarter of the lanes on a fixed first roll
    cube0 = np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)]
    rule = CubeRule(vh, jacoby=True, **TRACED)
    life = CubeLife(0.68, 1.2, 1.1)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=5)
        out = ro.run_lanes(RandomPlayer(2), starts, torch.from_numpy(group), P, G, max_steps=steps, trace=True, cube=rule,
                           cube0=torch.from_numpy(cube0), cube_luck=CubeLuck(vh, scale=1.5, life=life))
        assert ro.eng.error() == 0 and len(out) == 5
        runs.append(out)
    tally, _, tr, ct, clt = runs[0]
    tally, ct, clt = tally.cpu().numpy(), ct.cpu().numpy(), clt.cpu().numpy()
    assert clt.shape == (P, 5) and clt.dtype == np.int64
    ref = cube_luck_reference(tr, starts, group, P, G, rule, cube0)
    assert np.array_equal(clt, ref["cube_luck_tally"]), (clt, ref["cube_luck_tally"])
    assert np.array_equal(ct, ref["cube_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["cube_luck_state"].cpu().numpy(), ref["cube_luck_state"])
    assert np.array_equal(tr["cube_mask"].cpu().numpy() != 0, ref["mask"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"])
    assert np.array_equal(bits(ro.lane_luck.cpu().numpy()), bits(ref["lane_luck"]))
    assert np.array_equal(clt[:, LGAMES], ct[:, CG]) and (clt[:, LGAMES] > 0).all() and (clt[:, LO] > 0).all()
    takes = ct[:, DBL].sum() - ct[:, PG].sum()
    assert ct[:, PG].sum() > 0 and takes > 0                 # at least one pass and one take within the run
    # every step's luck from the traced values, cube, mover and roll, on the lanes selected there
    T = tr["done"].shape[0]
    lk, vals = tr["cube_luck"].cpu().numpy(), tr["cube_luck_values"].cpu().numpy()
    state, mover, roll = (tr[k].cpu().numpy() for k in ("cube_luck_state", "cube_luck_mover", "cube_luck_roll"))
    on = ref["cube_luck_sel"]
    want, _ = cube_roll_luck_reference(np.nan_to_num(vals.reshape(-1, 21)), state.reshape(-1), mover.reshape(-1),
                                       roll.reshape(-1, 2), 1.5, life, rule.cap, True)
    want = want.reshape(T, B)
    assert on.sum() > 1000 and np.array_equal(bits(lk[on]), bits(want[on])) and np.isfinite(vals[on]).all()
    assert np.isnan(lk[:, group < 0]).all() and np.abs(lk[on]).max() > 0.01
    # run to run identical
    assert torch.equal(runs[1][4], runs[0][4]) and torch.equal(runs[1][3], runs[0][3])
    assert torch.equal(runs[1][2]["cube_luck"].view(torch.int32), tr["cube_luck"].view(torch.int32))
    # the games are those of the same run without cube_luck
    ro = Rollout(B, seed=5)
    plain = ro.run_lanes(RandomPlayer(2), starts, torch.from_numpy(group), P, G, max_steps=steps, trace=True, cube=rule,
                         cube0=torch.from_numpy(cube0))
    assert len(plain) == 4 and "cube_luck" not in plain[2]
    assert torch.equal(plain[0], runs[0][0]) and torch.equal(plain[3], runs[0][3]) and torch.equal(plain[1], runs[0][1])
    for k in ("action", "done", "info", "cube", "cube_mask", "games_done"):
        assert torch.equal(plain[2][k], tr[k]), k


# ------------------------------------------------------------------------- 6. mean zero --
def mean_and_sigmas(luck, lo, hi, n):
    """(sum L / n, its standard error sqrt(var(L) / n)) in points from a row's integer sums."""
    mean = luck / n / ONE
    var = max(((hi << 30) + lo) / n / ONE ** 2 - mean * mean, 0.0) * n / (n - 1)
    return mean, math.sqrt(var / n)


def test_luck_has_mean_zero(net, vh):
    """2,048 lanes x 2 games from the opening with drawn first rolls, the policy player, a rule that
    doubles, takes and passes: |sum L / n| within 5 of its own standard errors (§10's criterion; the
    seed is fixed).  Then per group with stratified first rolls, whose luck is left out."""
    from bgx.arena import PolicyPlayer
    from bgx.cube import CubeLuck, CubeRule
    from bgx.rollout import Rollout, opening_record
    B, G = 2048, 2
    rule = CubeRule(vh, **TRACED)
    ro = Rollout(B, seed=11)
    tally, unf, _, ct, clt = ro.run_lanes(PolicyPlayer(net, seed=3), opening(0, B), torch.zeros(B, dtype=torch.int32), 1, G,
                                          max_steps=4000, cube=rule, cube_luck=CubeLuck(vh))
    assert ro.eng.error() == 0 and not unf.any()
    ct, clt = ct.cpu().numpy()[0], clt.cpu().numpy()[0]
    n = int(clt[LGAMES])
    assert n == B * G == ct[CG] and ct[PG] > 0 and ct[DBL] > ct[PG]
    mean, se = mean_and_sigmas(int(clt[LUCK]), int(clt[LO]), int(clt[HI]), n)
    print("mean zero, drawn first rolls:", mean, "+-", se, "passes", int(ct[PG]), "doubles", int(ct[DBL]))
    assert se > 0 and abs(mean) <= 5 * se
    pos = opening_record()[None].repeat(2, 1)
    pos[1, 52] = 1
    ro = Rollout(B, seed=12)
    res = ro.run(PolicyPlayer(net, seed=4), pos, 36 * 56, first_roll="stratified", max_steps=4000, cube=rule,
                 cube_luck=CubeLuck(vh))
    assert ro.eng.error() == 0
    for r in res:
        assert r["unfinished"] == 0 and r["games"] == r["cube_luck_games"] == 36 * 56
        mean, se = mean_and_sigmas(r["cube_luck"], r["cube_luck2_lo"], r["cube_luck2_hi"], r["games"])
        print("mean zero, stratified:", mean, "+-", se, "variance ratio", r["variance_ratio"], "c", r["luck_scale"])
        assert se > 0 and abs(mean) <= 5 * se and r["luck_mean"] == pytest.approx(mean, rel=1e-12, abs=1e-15)
        assert r["variance_ratio"] <= 1.0 + 1e-12            # the fitted coefficient never raises the sample's variance


# -------------------------------------------------------------------- 7. the cube decision --
def test_cube_decision_with_luck(vh):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLuck, CubeRule, rollout_cube_decision
    from bgx.rollout import Rollout, opening_record
    rule = CubeRule(vh, **TRACED)
    plain = rollout_cube_decision(Rollout(128, seed=6), RandomPlayer(1), opening_record(), 72, rule, max_steps=6000)
    d = rollout_cube_decision(Rollout(128, seed=6), RandomPlayer(1), opening_record(), 72, rule, max_steps=6000,
                              cube_luck=CubeLuck(vh))
    new = {"no_double_luck", "no_double_luck_stderr", "double_take_luck", "double_take_luck_stderr", "double_luck", "take_luck"}
    assert set(d) == set(plain) | new and not new & set(plain)
    for k in plain:
        if k != "rollouts":
            assert d[k] == plain[k], k                      # the raw keys, bit-equal
    for a, b in zip(d["rollouts"], plain["rollouts"]):
        assert all(a[k] == b[k] for k in b) and a["games"] == 72 == a["cube_luck_games"]
    assert d["no_double_luck"] == d["rollouts"][0]["equity_cubeful_luck"]
    assert d["double_take_luck"] == d["rollouts"][1]["equity_cubeful_luck"]
    assert d["double_take_luck_stderr"] == d["rollouts"][1]["equity_cubeful_luck_stderr"]
    assert d["double_luck"] is (min(d["double_take_luck"], 1.0) > d["no_double_luck"])
    assert d["take_luck"] is (d["double_take_luck"] <= 1.0)
    for k in new - {"double_luck", "take_luck"}:
        assert math.isfinite(d[k]), k
    # the units are the cube's: from 2 in the mover's hands the adjusted equities halve like the raw ones
    d2 = rollout_cube_decision(Rollout(128, seed=6), RandomPlayer(1), opening_record(), 72, rule, cube=(1, 1), max_steps=6000,
                               cube_luck=CubeLuck(vh), cube_luck_scale=1.0)
    assert d2["no_double_luck"] == d2["rollouts"][0]["equity_cubeful_luck"] / 2.0
    assert d2["rollouts"][0]["luck_scale"] == 1.0


# ----------------------------------------------------------------------- 8. graph capture --
def test_graph_capture():
    """cube_roll_luck and the three bookkeeping kernels (with the cube kernels between them) captured as
    one linear chain on one stream: the replay gives the eager results."""
    from bgx import _lib
    from bgx.cube import CubeLife
    L = _lib.load()
    s = book_state(seed=9)
    B = s["B"]
    life = CubeLife(0.68, 1.2, 1.1).struct()
    values = dev(np.random.RandomState(1).uniform(-1.5, 1.5, size=(B, 21)).astype(F))

    def chain(t, st):
        assert L.bgx_cube_roll_luck(ptr(t["recs"]), ptr(t["cube"]), ptr(values), B, 1.0, life, s["cap"], 1, ptr(t["sel"]),
                                    ptr(t["luck"]), None, st) == _lib.BGX_OK
        book_calls(L, s, t, st=st)

    eager = book_device(s)
    chain(eager, None)
    torch.cuda.synchronize()
    t = book_device(s)
    before = {k: v.clone() for k, v in t.items()}
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        chain(t, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, v in before.items():                              # the capture ran nothing
        assert torch.equal(t[k].view(torch.uint8), v.view(torch.uint8)), k
    g.replay()
    torch.cuda.synchronize()
    for k in ("luck", "lane_luck", "luck_tally", "cube_tally", "cube", "mask", "sel", "games_done", "plies", "active"):
        assert torch.equal(t[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    assert int(t["luck_tally"][:, LGAMES].sum()) > 50 and not torch.equal(t["luck"], before["luck"])


# ----------------------------------------------------------------------- 9. the command line --
def test_command_line(net, tmp_path, capsys):
    from bgx import rollout
    ckpt = str(tmp_path / "net.pt")
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, ckpt)
    base = ["--net", ckpt, "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps", "6000", "--cube",
            "--cube-double", "0.13", "--cube-pass", "0.19", "--cube-cap", "4"]
    rollout.main(base)
    plain = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    rollout.main(base + ["--cube-luck"])
    lucky = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(plain) == len(lucky) == 2
    new = {"luck_scale", "luck_mean", "equity_cubeful_luck", "equity_cubeful_luck_stderr", "variance_ratio", "cube_luck",
           "cube_luck2_lo", "cube_luck2_hi", "cube_yluck", "cube_luck_games"}
    assert set(lucky[0]) == set(plain[0]) | new and not new & set(plain[0])
    assert all(lucky[0][k] == plain[0][k] for k in plain[0])                       # the same games
    r, sm = lucky
    assert r["games"] == 72 == r["cube_luck_games"] and r["unfinished"] == 0
    assert r["equity_cubeful_luck_stderr"] <= r["equity_cubeful_stderr"] * (1 + 1e-9) and r["variance_ratio"] <= 1 + 1e-12
    assert set(sm) == set(plain[1]) | {"cube_luck", "cube_luck_net", "cube_luck_scale", "cube_luck_life", "cube_luck_win_value",
                                       "cube_luck_loss_value", "cube_luck_value_scale"}
    assert (sm["cube_luck"], sm["cube_luck_scale"], sm["cube_luck_life"], sm["cube_luck_net"]) == (True, "fit", 0.68, None)
    rollout.main(base + ["--cube-decision", "--cube-luck", "--cube-luck-scale", "1.0", "--cube-luck-life", "0.5",
                         "--cube-luck-win-value", "1.4", "--cube-luck-loss-value", "1.2", "--cube-luck-value-scale", "2",
                         "--cube-luck-net", ckpt])
    d, sm = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert d["cube_decision"] is True and d["double_luck"] == (min(d["double_take_luck"], 1.0) > d["no_double_luck"])
    assert d["take_luck"] == (d["double_take_luck"] <= 1.0) and len(d["rollouts"]) == 2
    assert all(x["luck_scale"] == 1.0 and x["cube_luck_games"] == 72 for x in d["rollouts"])
    assert (sm["cube_luck_scale"], sm["cube_luck_life"], sm["cube_luck_win_value"], sm["cube_luck_loss_value"],
            sm["cube_luck_value_scale"], sm["cube_luck_net"]) == (1.0, 0.5, 1.4, 1.2, 2.0, ckpt)
    assert sm["games"] == 144
