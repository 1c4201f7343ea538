"""Truncated cubeful rollouts and the static cube evaluator on the device (DESIGN.md §17;
csrc/bg_cube_trunc.h behind bgx_cube_janowski and bgx_rollout_cube_trunc_cut; cube.CubeTruncation,
Rollout.run_lanes / run with cube_truncate=): the evaluator bit for bit against
cube.janowski_reference, the cut alone against its host replay, the argument checks, a dead cube
against a plain truncated run integer for integer, the estimator against the exact table, traced
runs against cube.cube_trunc_reference (alone and with the cubeful table cut), forced cube
decisions, graph capture and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import bearoff_ref as BR
import cube_bearoff_ref as CR

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 65536
GAMES, PLIES = 0, 1
N300 = 300                                    # a block and 44 lanes: a partial last wave
LIVES = [(0.68, 1.0, 1.0), (1.0, 1.3, 1.2), (0.25, 3.0, 3.0)]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def life_of(t):
    from bgx.cube import CubeLife
    return CubeLife(*t)


def opening(mover, B):
    from bgx.rollout import opening_record
    r = opening_record().clone()
    r[52] = mover
    return r[None].repeat(B, 1)


def by_mover(p1, p2):
    """A callable value that depends on the side on roll alone."""
    def value(eng, sel):
        m = eng.records()[:, 52]
        return torch.where(m == 0, float(p1), float(p2)).to(torch.float32).contiguous()
    return value


def by_position(eng, sel):
    """A callable value in [-1, 1] that depends on the board and the side on roll."""
    r = eng.records().to(torch.int64)
    h = (r[:, :48] * torch.arange(1, 49, device=r.device)).sum(1) * 37 + r[:, 52] * 101
    return ((h % 201).to(torch.float32) / 100.0 - 1.0).contiguous()


def never(eng, dsel):
    return torch.full((eng.batch,), -1.0, dtype=torch.float32, device=eng.device)


def edge_values(rng, n, W, L):
    """Cubeless values at and beside every breakpoint of the rule (the take and cash points, the
    Jacoby form's 0.2 and 0.8, p = 0, 1/2 and 1), the clamps, NaN and the infinities, then noise."""
    up, down = lambda v: F(np.nextafter(F(v), F(np.inf))), lambda v: F(np.nextafter(F(v), F(-np.inf)))
    D = W + L + 0.5
    vals = [F(math.nan), F(math.inf), F(-math.inf), F(100.0), F(-100.0), F(0.0), F(-0.0)]
    for p in ((L - 0.5) / D, (L + 1.0) / D, 0.2, 0.8, 0.0, 1.0, 0.5):
        e = F(p * (W + L) - L)
        vals += [e, up(e), down(e)]
    v = rng.uniform(-L - 0.2, W + 0.2, n).astype(np.float32)
    at = rng.permutation(n)[:3 * len(vals)]
    v[at] = np.tile(np.array(vals, np.float32), 3)
    return v


# --------------------------------------------------------- 1. the static evaluator --
def janowski_state(seed=4):
    from bgx.cube import pack
    rng = np.random.RandomState(seed)
    n = N300
    recs = np.zeros((n, 64), np.uint8)
    recs[:, 52] = rng.randint(0, 2, n)
    recs[:, 55] = rng.rand(n) < 0.1                                      # game_over records
    states = [0] + [pack(k, o) for k in range(0, 11) for o in (1, 2)]     # every byte the kernels can leave
    states += [0x0F, 0x3F, 0x31, 0x30, 0x1B, 0x2C, 0xC0, 0xFF, 0x47]      # k above 10, owner 3, bits 6-7 set
    cube = np.array(states, np.uint8)[np.arange(n) % len(states)]
    cube = cube[rng.permutation(n)]
    sel = (rng.rand(n) < 0.8).astype(np.uint8)
    return rng, recs, cube, sel


@pytest.mark.parametrize("jacoby", [False, True])
@pytest.mark.parametrize("life", LIVES)
def test_janowski_equals_the_reference(life, jacoby):
    from bgx import _lib
    from bgx.cube import janowski_reference, static_cube_decision
    L = _lib.load()
    rng, recs, cube, sel = janowski_state()
    n = N300
    value = edge_values(rng, n, life[1], life[2])
    d_recs, d_cube, d_sel, d_value = dev(recs), dev(cube), dev(sel), dev(value)
    live = recs[:, 55] == 0
    seen = set()
    for cap, scale, with_cube, with_sel in ((6, 1.0, True, True), (10, 1.0, True, False), (3, -0.5, True, True),
                                            (6, 1.0, False, True), (0, 2.0, False, False), (1, 1.0, True, False)):
        values = torch.full((n, 4), 77.0, dtype=torch.float32, device="cuda")
        flags = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
        rc = L.bgx_cube_janowski(ptr(d_recs), ptr(d_cube) if with_cube else None, ptr(d_value), n, scale,
                                 life_of(life).struct(), cap, int(jacoby), ptr(d_sel) if with_sel else None, ptr(values),
                                 ptr(flags), stream())
        assert rc == _lib.BGX_OK
        w_values, w_flags = janowski_reference(value, cube if with_cube else None, recs[:, 52], scale, life_of(life), cap,
                                               jacoby)
        on = live & ((sel != 0) if with_sel else np.ones(n, bool))
        got_v, got_f = values.cpu().numpy(), flags.cpu().numpy()
        assert bits_equal(got_v[on], w_values[on]), (cap, scale, with_cube, with_sel)
        assert np.array_equal(got_f, np.where(on, w_flags, 0)), (cap, scale, with_cube, with_sel)
        assert (got_v[~on] == 77.0).all() and (~on).sum() > 20               # un-selected rows keep the sentinel
        assert not np.isnan(got_v[on]).any()
        seen |= set(w_flags[on].tolist())
        # the Python face, values given: the same call
        pv, pf = static_cube_decision(d_recs, None, cube=d_cube if with_cube else None, scale=scale, life=life_of(life),
                                      cap=cap, jacoby=jacoby, sel=d_sel if with_sel else None, value=d_value)
        assert bits_equal(pv.cpu().numpy()[on], w_values[on]) and np.isnan(pv.cpu().numpy()[~on]).all()
        assert np.array_equal(pf.cpu().numpy(), got_f)
    assert seen == {0, 1, 3, 4, 5, 7, 8, 12}, seen
    # values_out or flags_out may be NULL
    flags = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    assert L.bgx_cube_janowski(ptr(d_recs), ptr(d_cube), ptr(d_value), n, 1.0, life_of(life).struct(), 6, int(jacoby), None,
                               None, ptr(flags), stream()) == _lib.BGX_OK
    assert np.array_equal(flags.cpu().numpy(), np.where(live, janowski_reference(value, cube, recs[:, 52], 1.0, life_of(life),
                                                                               6, jacoby)[1], 0))
    assert L.bgx_cube_janowski(ptr(d_recs), ptr(d_cube), ptr(d_value), n, 1.0, life_of(life).struct(), 6, int(jacoby), None,
                               None, None, stream()) == _lib.BGX_OK
    torch.cuda.synchronize()


def test_static_cube_decision_on_an_engine():
    """The Python face on an engine's own lane records with a net's value head: value_lanes, then
    the rule; a contiguous copy of the records gives the same."""
    import bgx
    from bgx.cube import CubeLife, janowski_reference, pack, static_cube_decision
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead, value_lanes
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    B = 192
    eng = bgx.Engine(batch=B, max_moves=500, seed=3, auto_reset=True, device="cuda:0")
    eng.reset()
    rng = np.random.RandomState(0)
    for _ in range(6):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    recs = eng.records()
    cube = dev(np.array([0, pack(1, 1), pack(2, 2)], np.uint8)[np.arange(B) % 3])
    life = CubeLife(0.68, 1.2, 1.1)
    values, flags = static_cube_decision(eng, vh, cube=cube, life=life, cap=6)
    v = value_lanes(eng, vh).cpu().numpy()
    w_values, w_flags = janowski_reference(v, cube.cpu().numpy(), recs[:, 52].cpu().numpy(), 1.0, life, 6)
    assert bits_equal(values.cpu().numpy(), w_values) and np.array_equal(flags.cpu().numpy(), w_flags)
    v2, f2 = static_cube_decision(recs.contiguous(), vh, cube=cube, life=life, cap=6)
    assert torch.equal(v2.view(torch.int32), values.view(torch.int32)) and torch.equal(f2, flags)
    assert set(w_flags.tolist()) & {1, 3, 5, 7} and set(w_flags.tolist()) & {0, 4}
    for bad in (dict(cap=11), dict(life=0.5), dict(scale=math.nan), dict(cube=cube[:5]), dict(sel=cube.float())):
        with pytest.raises(ValueError):
            static_cube_decision(eng, vh, **bad)
    with pytest.raises(ValueError):
        static_cube_decision(recs.cpu(), vh)


# ------------------------------------------------------------------ 2. the cut alone --
def cut_state(seed=9):
    """300 lanes of hand-set state: five groups that share waves, idle lanes and lanes whose
    group is out of range with tsel set all the same, every cube state and k up to 10 (cap 10),
    retired lanes, lanes on their last game, and +-inf values at W = L = 3 (|q| = 3)."""
    from bgx.cube import pack
    rng = np.random.RandomState(seed)
    B, G, P = N300, 3, 5
    group = np.repeat(np.arange(5), [10, 70, 53, 94, 73]).astype(np.int32)
    group = group[:B]
    for k in (3, 40, 41, 99, 130, 131, 190, 260):
        group[k] = -1
    for k in (5, 77, 201, 299):
        group[k] = (7, 5, -3, 1 << 20)[k % 4]                          # outside [0, P)
    recs = np.zeros((B, 64), np.uint8)
    recs[:, 52] = rng.randint(0, 2, B)
    starts = np.zeros((B, 64), np.uint8)
    starts[:, 52] = rng.randint(0, 2, B)
    states = [0] + [pack(k, o) for k in (1, 2, 5, 9, 10) for o in (1, 2)] + [0x0F, 0x31]
    cube = np.array(states, np.uint8)[rng.randint(len(states), size=B)]
    cube0 = np.array(states[:5], np.uint8)[rng.randint(5, size=B)]
    plies = rng.randint(1, 9, size=B).astype(np.int32)
    games_done = rng.randint(0, G, size=B).astype(np.int32)              # G - 1: the lane's last game
    sel = ((group >= 0) & (group < P) & (rng.rand(B) < 0.85)).astype(np.uint8)
    games_done[sel == 0] = G
    tsel = ((sel != 0) & (rng.rand(B) < 0.7)).astype(np.uint8)
    tsel[[3, 40, 5, 77, 201, 299]] = 1                                   # a tsel of another origin: the group decides
    value = edge_values(rng, B, 3.0, 3.0)
    big = np.nonzero((cube & 15) >= 9)[0]
    value[big[::2]], value[big[1::2]] = np.inf, -np.inf
    return dict(recs=recs, starts=starts, group=group, cube=cube, cube0=cube0, plies=plies, games_done=games_done,
                sel=sel, tsel=tsel, value=value, G=G, P=P)


CUT_KW = dict(life=(0.68, 3.0, 3.0), cap=10, jacoby=1, scale=1.0)


def cut_replay(s, life, cap, jacoby, scale):
    """bgx_rollout_cube_trunc_cut lane by lane on the host."""
    from bgx.cube import cube_trunc_fixed_reference, janowski_reference, sanitise
    B, P, G = len(s["group"]), s["P"], s["G"]
    values, _ = janowski_reference(s["value"], s["cube"], s["recs"][:, 52], scale, life_of(life), cap, bool(jacoby))
    k = np.minimum(s["cube"].astype(np.int64) & 15, cap)
    yq = cube_trunc_fixed_reference(values[:, 2], s["recs"][:, 52] == s["starts"][:, 52], k)
    tally = np.zeros((P, 6), np.int64)
    gd, plies, sel, cube = s["games_done"].copy(), s["plies"].copy(), s["sel"].copy(), s["cube"].copy()
    mask, retired = np.zeros(B, np.uint8), 0
    c0 = sanitise(s["cube0"], cap)
    for i in range(B):
        g = int(s["group"][i])
        if not s["tsel"][i] or not 0 <= g < P:
            continue
        y = int(yq[i])
        row = tally[g]
        row[0] += 1; row[1] += plies[i]; row[2] += y; row[3] += (y * y) & ((1 << 30) - 1); row[4] += (y * y) >> 30
        row[5] += k[i]
        gd[i] += 1
        plies[i] = 0
        if gd[i] >= G:
            sel[i] = 0
            retired += 1
        cube[i] = c0[i]
        mask[i] = 1
    return dict(tally=tally, games_done=gd, plies=plies, sel=sel, cube=cube, mask=mask, retired=retired, yq=yq)


def run_cut(s, life, cap, jacoby, scale, st=None):
    from bgx import _lib
    d = {k: dev(s[k]) for k in ("recs", "starts", "group", "cube", "cube0", "plies", "games_done", "sel", "tsel", "value")}
    B = len(s["group"])
    d["tally"] = torch.zeros(s["P"], 6, dtype=torch.int64).cuda()
    d["active"] = torch.tensor([int(s["sel"].sum())]).cuda()
    d["mask"] = torch.full((B,), 9, dtype=torch.uint8).cuda()
    rc = call_cut(d, s, life, cap, jacoby, scale, st)
    assert rc == _lib.BGX_OK
    return d


def call_cut(d, s, life, cap, jacoby, scale, st=None):
    from bgx import _lib
    B = len(s["group"])
    return _lib.load().bgx_rollout_cube_trunc_cut(
        ptr(d["recs"]), ptr(d["starts"]), ptr(d["group"]), ptr(d["tsel"]), ptr(d["value"]), scale, life_of(life).struct(),
        B, s["P"], s["G"], ptr(d["games_done"]), ptr(d["plies"]), ptr(d["sel"]), ptr(d["tally"]), ptr(d["active"]),
        ptr(d["mask"]), cap, jacoby, ptr(d["cube0"]), ptr(d["cube"]), st if st is not None else stream())


def test_cut_alone_equals_the_host_replay():
    s = cut_state()
    ref = cut_replay(s, **CUT_KW)
    runs = [run_cut(s, **CUT_KW) for _ in range(2)]
    d = runs[0]
    torch.cuda.synchronize()
    for name in ("tally", "mask", "games_done", "plies", "sel", "cube"):
        assert np.array_equal(d[name].cpu().numpy(), ref[name]), name
    assert int(d["active"].item()) == int(s["sel"].sum()) - ref["retired"] and ref["retired"] > 20
    for name in ("recs", "starts", "group", "cube0", "tsel", "value"):            # inputs stay
        assert np.array_equal(d[name].cpu().numpy().view(np.uint8), np.ascontiguousarray(s[name]).view(np.uint8)), name
    m = ref["mask"] != 0
    # every kind of lane occurs: rows shared inside a wave, invalid groups with tsel, retired lanes, last games
    assert len(set(s["group"][64:128].tolist()) - {-1, 5}) >= 2 and m.sum() > 150
    bad_group = (s["group"] < 0) | (s["group"] >= s["P"])
    assert (s["tsel"][bad_group] != 0).any() and not m[bad_group].any() and not m[s["sel"] == 0].any()
    assert ((s["sel"] != 0) & (s["tsel"] == 0)).any() and (s["games_done"][m] == s["G"] - 1).any()
    # |q| = 3 at k = 10: the square needs the HI part, and fits
    y = ref["yq"][m]
    assert np.abs(y).max() == 3 * ONE << 10 and (y == 3 * ONE << 10).any() and (y == -(3 * ONE << 10)).any()
    assert (ref["tally"][:, 4] > 0).all() and (ref["tally"][:, 0] > 0).all() and ref["tally"][:, 5].sum() > 100
    same = s["recs"][:, 52] == s["starts"][:, 52]
    assert same[m].any() and (~same[m]).any()
    # a second call on the same state reproduces the first
    for key in ("tally", "mask", "games_done", "plies", "sel", "cube", "active"):
        assert torch.equal(runs[1][key], d[key]), key
    # another rule: no Jacoby, a smaller cap (more dead cubes), a negative scale
    kw = dict(life=(1.0, 1.3, 1.2), cap=5, jacoby=0, scale=-0.5)
    ref2, d2 = cut_replay(s, **kw), run_cut(s, **kw)
    for name in ("tally", "mask", "games_done", "plies", "sel", "cube"):
        assert np.array_equal(d2[name].cpu().numpy(), ref2[name]), name
    assert not np.array_equal(ref2["tally"], ref["tally"])


# ------------------------------------------------------------------ 3. the arguments --
def test_argument_checks():
    from bgx import _lib
    L = _lib.load()
    B, P = 64, 2
    z8 = torch.zeros(B, 64, dtype=torch.uint8, device="cuda")
    u8 = lambda: torch.zeros(B, dtype=torch.uint8, device="cuda")
    i32 = lambda: torch.zeros(B, dtype=torch.int32, device="cuda")
    f32 = torch.zeros(B, dtype=torch.float32, device="cuda")
    out = torch.zeros(B, 4, dtype=torch.float32, device="cuda")
    tally = torch.zeros(P, 6, dtype=torch.int64, device="cuda")
    act = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = stream()
    life = lambda x=0.68, w=1.0, l=1.0: _lib.BgxCubeLife(x, w, l)
    bad_lives = [life(x=-0.1), life(x=1.5), life(x=math.nan), life(w=0.5), life(w=3.5), life(w=math.nan), life(l=0.99),
                 life(l=math.inf), life(l=math.nan)]
    cube, flags, sel = u8(), u8(), u8()
    ok = [ptr(z8), ptr(cube), ptr(f32), B, 1.0, life(), 6, 0, ptr(sel), ptr(out), ptr(flags), s]
    assert L.bgx_cube_janowski(*ok) == _lib.BGX_OK
    for k, v in [(0, None), (2, None), (3, 0), (3, -4), (4, math.nan), (6, -1), (6, 11),
                 (9, ctypes.c_void_p(out.data_ptr() + 4))] + [(5, b) for b in bad_lives]:
        a = list(ok)
        a[k] = v
        assert L.bgx_cube_janowski(*a) == _lib.BGX_EINVAL, (k, v)
    for good in (life(0.0, 1.0, 3.0), life(1.0, 3.0, 1.0)):
        a = list(ok)
        a[5] = good
        assert L.bgx_cube_janowski(*a) == _lib.BGX_OK
    gd, pl, se, mask, c0, cb, tsel = i32(), i32(), u8(), u8(), u8(), u8(), u8()
    ok = [ptr(z8), ptr(z8), ptr(i32()), ptr(tsel), ptr(f32), 1.0, life(), B, P, 1, ptr(gd), ptr(pl), ptr(se), ptr(tally),
          ptr(act), ptr(mask), 6, 0, ptr(c0), ptr(cb), s]
    assert L.bgx_rollout_cube_trunc_cut(*ok) == _lib.BGX_OK
    for k, v in [(i, None) for i in (0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 18, 19)] + \
            [(5, math.nan), (7, 0), (7, -1), (8, 0), (9, -1), (16, -1), (16, 11)] + [(6, b) for b in bad_lives]:
        a = list(ok)
        a[k] = v
        assert L.bgx_rollout_cube_trunc_cut(*a) == _lib.BGX_EINVAL, (k, v)
    torch.cuda.synchronize()
    assert not tally.any() and not mask.any() and int(act) == 0           # tsel was 0 everywhere: nothing counted


# ------------------------------------------- 4. a dead cube is the plain truncation --
B128, G2, H4 = 128, 2, 90


def run_opening(seed=3, start_mover=0, **kw):
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    ro = Rollout(B128, seed=seed)
    out = ro.run_lanes(RandomPlayer(11), opening(start_mover, B128), torch.zeros(B128, dtype=torch.int32), 1, G2,
                       max_steps=6000, **kw)
    assert ro.eng.error() == 0 and not out[1].any()
    return out


def test_dead_cube_equals_the_plain_truncation():
    """x = 0, W = L = 1, a rule that never doubles, and the cube dead from the start (the cap is
    the starting k: with a live cube the mover's right to double next ply is worth something even
    at x = 0, e = max(c, min(2 c, 1))): the cubeful run counts, integer for integer, what a fresh
    same-seed truncate= run counts, times the cube."""
    from bgx.cube import CubeLife, CubeRule, CubeTruncation, pack
    from bgx.truncate import Truncation
    tally, _, _, tt = run_opening(truncate=Truncation(by_position, H4))
    t, tt = tally.cpu().numpy()[0], tt.cpu().numpy()[0]
    res = sum((j + 1) * (int(t[2 + j]) - int(t[5 + j])) for j in range(3))
    plain = res * ONE + int(tt[2])
    assert t[GAMES] + tt[0] == B128 * G2 and t[GAMES] > 0 and tt[0] > 20 and tt[2] != 0      # both kinds of ending
    life = CubeLife(0.0, 1.0, 1.0)
    for k, owner, cap in ((0, 0, 0), (2, 1, 2)):
        rule = CubeRule(by_position, double_at=math.inf, cap=cap)
        cube0 = torch.full((B128,), pack(k, owner), dtype=torch.uint8)
        out = run_opening(cube=rule, cube0=cube0, cube_truncate=CubeTruncation(by_position, H4, life=life))
        assert len(out) == 5
        ct, ctt = out[3].cpu().numpy()[0], out[4].cpu().numpy()[0]
        assert np.array_equal(out[0].cpu().numpy()[0], t)                    # the same games end naturally
        assert (ct[0], ctt[0], ctt[1]) == (t[GAMES], tt[0], tt[1]) and ct[4] == 0 and ct[7] == 0
        assert int(ct[1]) * ONE + int(ctt[2]) == (1 << k) * plain
        assert int(ctt[2]) == (1 << k) * int(tt[2]) and int(ctt[5]) == k * int(tt[0])
        assert (int(ctt[4]) << 30) + int(ctt[3]) == (1 << 2 * k) * int(tt[3])


# ------------------------------------------------- 5. against the exact table --
RACE = BR.record((0, 0, 0, 2, 2, 2), (0, 0, 0, 2, 2, 2), 0)
RACE_EQUITY = 0.308428                                   # the side on roll wins 0.654214 (exact K = 6 table)


@pytest.fixture(scope="module")
def db6():
    from bgx.bearoff import BearoffDB
    return BearoffDB(6)


@pytest.mark.parametrize("start_mover", [0, 1])
def test_estimator_against_the_exact_table(db6, start_mover):
    """tests/test_gpu_truncate.py's test_estimator_against_the_exact_table with a dead cube at 2
    (cap = k = 1): perfect play, the table's own 2 W - 1 as the value, so the truncated cubeful
    estimate over 2^k is unbiased for the exact cubeless value: within that test's 5 standard
    errors, on its 4096 lanes."""
    from bgx.arena import RandomPlayer
    from bgx.bearoff import BearoffPlayer
    from bgx.cube import CubeLife, CubeRule, CubeTruncation, pack, summarize_cube_truncated
    from bgx.rollout import Rollout
    B, k = 4096, 1
    start = RACE.copy()
    start[52] = start_mover
    starts = torch.from_numpy(start)[None].repeat(B, 1)
    in_db, win = db6.lookup(starts[:1].cuda())
    exact = 2.0 * float(win[0]) - 1.0
    assert int(in_db[0]) == 1 and exact == pytest.approx(RACE_EQUITY, abs=2e-6)

    def value(eng, tsel):
        return (2.0 * db6.lookup(eng.records())[1] - 1.0).contiguous()

    grp = torch.zeros(B, dtype=torch.int32)
    cube0 = torch.full((B,), pack(k, 1 + (start_mover ^ 1)), dtype=torch.uint8)
    for plies in (3, 4):                                  # the opponent / the start mover on roll at the cut
        ro = Rollout(B, seed=9)
        tally, unf, _, ct, ctt = ro.run_lanes(BearoffPlayer(RandomPlayer(4), db6), starts, grp, 1, 1, max_steps=200,
                                              cube=CubeRule(never, cap=k), cube0=cube0,
                                              cube_truncate=CubeTruncation(value, plies, life=CubeLife(0.68)))
        r = summarize_cube_truncated(tally[0].tolist(), ct[0].tolist(), ctt[0].tolist(), int(unf[0]))
        eq, se = r["equity_cubeful"] / 2 ** k, r["equity_cubeful_stderr"] / 2 ** k
        print(f"mover {start_mover} plies {plies}: equity_cubeful / 2^k {eq:.5f} +- {se:.5f} (exact {exact:.6f}), "
              f"truncated_share {r['truncated_share']:.3f}")
        assert r["games"] == B and r["unfinished"] == 0 and r["truncated_share"] > 0.5 and r["doubles"] == 0
        assert r["mean_cube_log2"] == k and se > 0.0
        assert abs(eq - exact) < 5 * se


# ------------------------------------------------ 6. a traced run with a real net --
TRACED = dict(double_at=0.13, pass_at=0.19, cap=4)          # tests/test_gpu_cube.py: inside a fresh net's value range


def group64():
    group = np.repeat(np.arange(3), [20, 21, 20]).astype(np.int32)
    for k in (7, 30, 50):
        group = np.insert(group, k, -1)
    return group


@pytest.mark.parametrize("lookahead", [0, 1])
def test_traced_run_equals_the_host_replay(lookahead):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLife, CubeRule, CubeTruncation, cube_trunc_reference, pack, summarize_cube_truncated
    from bgx.policy import PolicyNet
    from bgx.rollout import Rollout
    from bgx.search import ValueHead
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    B, P, G, H = 64, 3, 4, 3
    group = group64()
    starts = opening(0, B)
    starts[1::2, 52] = 1
    cube0 = np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)]
    rule = CubeRule(vh, jacoby=True, **TRACED)
    tc = CubeTruncation(vh, H, lookahead=lookahead, life=CubeLife(0.68, 1.3, 1.2))
    assert tc.sync_free == (lookahead == 0)
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=5)
        out = ro.run_lanes(RandomPlayer(2), starts, torch.from_numpy(group), P, G, max_steps=200, trace=True, cube=rule,
                           cube0=torch.from_numpy(cube0), cube_truncate=tc)
        assert ro.eng.error() == 0 and not out[1].any() and len(out) == 5 and ro.steps <= H * G
        runs.append(out)
    tally, _, tr, ct, ctt = runs[0]
    tally, ct, ctt = tally.cpu().numpy(), ct.cpu().numpy(), ctt.cpu().numpy()
    ref = cube_trunc_reference(tr, starts, group, P, G, rule, tc, cube0)
    assert np.array_equal(ctt, ref["cube_trunc_tally"]) and np.array_equal(ct, ref["cube_tally"])
    assert np.array_equal(tally, ref["tally"]) and not tally.any()
    assert np.array_equal(tr["cube"].cpu().numpy(), ref["cube"])
    assert np.array_equal(tr["cube_mask"].cpu().numpy() != 0, ref["mask"])
    assert np.array_equal(tr["ctrunc"].cpu().numpy() != 0, ref["ctrunc"])
    on = ref["ctrunc"]
    assert np.array_equal(tr["ctrunc_cube"].cpu().numpy()[on], ref["ctrunc_cube"][on])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    v = tr["ctrunc_value"]
    assert bool((torch.isnan(v) == (tr["ctrunc"] == 0)).all())
    passes, takes = int(ct[:, 4].sum()), int(ct[:, 7].sum() - ct[:, 4].sum())
    print(f"lookahead {lookahead}: passes {passes}, takes {takes}, truncated {int(ctt[:, 0].sum())}; ctt {ctt.tolist()}")
    assert passes > 0 and takes > 0 and ctt[:, 0].sum() > 100 and ctt[:, 5].sum() > 0
    assert np.array_equal(ctt[:, 1], H * ctt[:, 0])                         # a truncated game ran exactly H plies
    assert not tr["ctrunc"][:, torch.from_numpy(group < 0).cuda()].any()
    scheduled = np.bincount(group[group >= 0], minlength=P) * G
    assert np.array_equal(ct[:, 0] + ctt[:, 0], scheduled)
    for p in range(P):
        r = summarize_cube_truncated(tally[p], ct[p], ctt[p])
        assert r["games"] == scheduled[p] and 0 < r["truncated_share"] <= 1 and math.isfinite(r["equity_cubeful_stderr"])
    # run to run identical
    for j in (0, 3, 4):
        assert torch.equal(runs[1][j], runs[0][j]), j
    for key in ("cube", "cube_mask", "action", "ctrunc", "ctrunc_mover", "ctrunc_cube"):
        assert torch.equal(runs[1][2][key], tr[key]), key
    assert torch.equal(runs[1][2]["ctrunc_value"].nan_to_num(7.0), v.nan_to_num(7.0))


# --------------------------------------- 7. the table cut and the truncation together --
@pytest.fixture(scope="module")
def cdb3():
    from bgx.bearoff import BearoffDB, CubefulBearoffDB
    return CubefulBearoffDB(BearoffDB(3))


def lookup_on(cdb, K):
    from bgx.bearoff import cube_lookup_reference
    cfg, E, ND = cdb.configs().cpu().numpy(), cdb.equity().cpu().numpy(), cdb.nd().cpu().numpy()
    W = cdb.db.table().cpu().numpy()
    return lambda recs, cube, cap: cube_lookup_reference(recs, cfg, E, ND, W, K, cube, cap)


def near_k3_starts(B, seed):
    """Both sides home with 4 or 5 checkers: two or three plies from the K = 3 table."""
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        c = [np.bincount(rng.randint(0, 6, rng.randint(4, 6)), minlength=6) for _ in range(2)]
        s[i] = BR.record(tuple(c[0]), tuple(c[1]), rng.randint(2), (rng.randint(1, 7), rng.randint(1, 7)) if i % 2 else (0, 0))
    return s


def by_lane(B):
    """A cube rule's callable equity: a take (0.45), a pass (0.9) or no double (-1) by the lane."""
    e = torch.tensor([0.45, 0.9, -1.0, 0.45, -1.0], dtype=torch.float32).repeat(B // 5 + 1)[:B].cuda().contiguous()
    return lambda eng, dsel: e


def test_table_cut_and_truncation_together(cdb3):
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLife, CubeRule, CubeTruncation, cube_trunc_reference, pack, summarize_cube_truncated
    from bgx.rollout import Rollout
    B, P, G, H = 64, 3, 3, 3
    group = group64()
    starts = near_k3_starts(B, 21)
    cube0 = np.array([0, pack(1, 1), pack(1, 2)], np.uint8)[np.maximum(group, 0)]
    rule = CubeRule(by_lane(B), cap=4)
    tc = CubeTruncation(by_position, H, life=CubeLife(0.5, 1.0, 1.0))
    ro = Rollout(B, seed=5)
    out = ro.run_lanes(RandomPlayer(2), torch.from_numpy(starts), torch.from_numpy(group), P, G, max_steps=400, trace=True,
                       cube=rule, cube0=torch.from_numpy(cube0), cube_bearoff=cdb3, cube_truncate=tc)
    assert ro.eng.error() == 0 and len(out) == 6 and not out[1].any()
    tally, _, tr, ct, cct, ctt = out
    tally, ct, cct, ctt = (t.cpu().numpy() for t in (tally, ct, cct, ctt))
    ref = cube_trunc_reference(tr, starts, group, P, G, rule, tc, cube0, cut_lookup=lookup_on(cdb3, 3))
    assert np.array_equal(ctt, ref["cube_trunc_tally"]) and np.array_equal(cct, ref["cut_tally"])
    assert np.array_equal(ct, ref["cube_tally"]) and np.array_equal(tally, ref["tally"])
    assert np.array_equal(tr["cut"].cpu().numpy() != 0, ref["cut"]) and np.array_equal(tr["ctrunc"].cpu().numpy() != 0, ref["ctrunc"])
    assert np.array_equal(tr["cube"].cpu().numpy(), ref["cube"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), ref["games_done"]) and tr["active"] == ref["active"] == 0
    # exact where the table reaches, Janowski elsewhere; never both on one lane in one step
    assert not (tr["cut"].bool() & tr["ctrunc"].bool()).any()
    print(f"cut {cct[:, 0].tolist()}, truncated {ctt[:, 0].tolist()}, passed {ct[:, 4].tolist()}")
    assert cct[:, 0].sum() > 10 and ctt[:, 0].sum() > 10
    scheduled = np.bincount(group[group >= 0], minlength=P) * G
    assert np.array_equal(ct[:, 0] + cct[:, 0] + ctt[:, 0], scheduled)
    for p in range(P):
        r = summarize_cube_truncated(tally[p], ct[p], ctt[p], cut_row=cct[p])
        assert r["games"] == scheduled[p] and math.isfinite(r["equity_cubeful"]) and 0 < r["cut_share"] + r["truncated_share"] <= 1
    # through run(): the summary with cut_row
    ro = Rollout(128, seed=1)
    res = ro.run(RandomPlayer(1), torch.from_numpy(starts[:2]), 36, max_steps=400, cube=CubeRule(by_lane(128), cap=4),
                 cube_bearoff=cdb3, cube_truncate=tc)
    for r in res:
        assert r["games"] == 36 == r["played_out"]["games"] + r["pass_games"] + r["cut_games"] + r["truncated_games"]
        assert r["bearoff_kind"] == "cubeful"


# ------------------------------------------------------------ 8. forced cube decisions --
def test_cube_decision_forced_through_the_truncation():
    """Horizon 1: every game stops after one ply with the opponent on roll, whose value is forced;
    x = 0 and a live cube below the cap, so its e = max(c, min(2 c, 1)) in both rollouts (centred
    in "no double", its own cube at 2 in "double, take").  c = -0.2: nd = 0.2, dt = 0.4, double and
    take; c = -0.8: nd = 0.8, dt = 1.6, double and pass; c = 0.3: e = 0.6, nd = -0.6, dt = -1.2, no
    double (and a take)."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeLife, CubeRule, CubeTruncation, rollout_cube_decision
    from bgx.rollout import Rollout, opening_record
    ro = Rollout(B128, seed=6)
    rule = CubeRule(never)
    q = lambda x: int(np.rint(F(F(x) * F(ONE)))) / ONE
    verdicts = set()
    for c, e, double, take in ((-0.2, -0.2, True, True), (-0.8, -0.8, True, False), (0.3, F(2) * F(0.3), False, True)):
        tc = CubeTruncation(by_mover(9.0, c), 1, life=CubeLife(0.0))
        d = rollout_cube_decision(ro, RandomPlayer(1), opening_record(), 36, rule, cube_truncate=tc)
        assert d["no_double"] == -q(e) and d["double_take"] == -2 * q(e), (c, d["no_double"], d["double_take"])
        assert d["no_double_stderr"] == d["double_take_stderr"] == 0.0
        assert (d["double"], d["take"]) == (double, take), c
        for r in d["rollouts"]:
            assert r["games"] == r["truncated_games"] == 36 and r["truncated_share"] == 1.0 and r["plies_per_game"] == 1.0
        assert d["rollouts"][1]["mean_cube_log2"] == 1.0
        verdicts.add((d["double"], d["take"]))
    assert len(verdicts) == 3
    # with the cube at 2 in the mover's hands the units are the cube's
    tc = CubeTruncation(by_mover(-0.2, 9.0), 1, life=CubeLife(0.0))
    rec = opening_record()
    rec[52] = 1
    d = rollout_cube_decision(ro, RandomPlayer(1), rec, 36, rule, cube=(1, 2), cube_truncate=tc)
    assert (d["no_double"], d["double_take"], d["double"], d["take"]) == (q(0.2), 2 * q(0.2), True, True)
    assert d["rollouts"][0]["equity_cubeful"] == 2 * q(0.2)


# ------------------------------------------------------ 9. None is the parent path --
def test_none_is_the_parent_path():
    """cube_truncate=None: the tallies, the trace and the result's shape of the run without it."""
    from bgx.arena import RandomPlayer
    from bgx.cube import CubeRule
    from bgx.rollout import Rollout
    B = 64
    starts, grp = torch.from_numpy(near_k3_starts(B, 3)), torch.zeros(B, dtype=torch.int32)
    outs = []
    for kw in ({}, dict(cube_truncate=None)):
        ro = Rollout(B, seed=2)
        outs.append(ro.run_lanes(RandomPlayer(4), starts, grp, 1, 2, max_steps=400, trace=True, cube=CubeRule(by_lane(B)), **kw))
    assert len(outs[0]) == len(outs[1]) == 4 and "ctrunc" not in outs[1][2]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][3], outs[1][3])
    for k in ("action", "done", "info", "cube", "cube_mask", "mover"):
        assert torch.equal(outs[0][2][k], outs[1][2][k]), k
    assert int(outs[0][3][0, 0]) == 2 * B
    ro = Rollout(B, seed=2)
    with pytest.raises(ValueError, match="cube_truncate without cube"):
        ro.run_lanes(RandomPlayer(4), starts, grp, 1, 2, cube_truncate=object())
    with pytest.raises(ValueError, match="cube.CubeTruncation"):
        ro.run_lanes(RandomPlayer(4), starts, grp, 1, 2, cube=CubeRule(by_lane(B)), cube_truncate=8)
    # the old refusal stays
    from bgx.truncate import Truncation
    with pytest.raises(ValueError, match="truncate together with cube"):
        ro.run_lanes(RandomPlayer(4), starts, grp, 1, 2, cube=CubeRule(by_lane(B)), truncate=Truncation(never, 4))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- 10. graph capture --
def test_graph_capture():
    """The evaluator and the cut captured into one graph replay to the eager results."""
    from bgx import _lib
    L = _lib.load()
    s = cut_state(seed=11)
    B = len(s["group"])
    eager = run_cut(s, **CUT_KW)
    life = life_of(CUT_KW["life"]).struct()
    e_values = torch.full((B, 4), float("nan")).cuda()
    e_flags = torch.full((B,), 5, dtype=torch.uint8).cuda()
    assert L.bgx_cube_janowski(ptr(eager["recs"]), ptr(dev(s["cube"])), ptr(eager["value"]), B, 1.0, life, 10, 1,
                               ptr(eager["tsel"]), ptr(e_values), ptr(e_flags), stream()) == _lib.BGX_OK
    torch.cuda.synchronize()
    state = {k: dev(s[k]) for k in ("recs", "starts", "group", "cube", "cube0", "plies", "games_done", "sel", "tsel", "value")}
    state.update(tally=torch.zeros(s["P"], 6, dtype=torch.int64).cuda(), active=torch.tensor([int(s["sel"].sum())]).cuda(),
                 mask=torch.full((B,), 9, dtype=torch.uint8).cuda())
    values = torch.full((B, 4), float("nan")).cuda()
    flags = torch.full((B,), 5, dtype=torch.uint8).cuda()
    before = {k: v.clone() for k, v in state.items()}
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.bgx_cube_janowski(ptr(state["recs"]), ptr(state["cube"]), ptr(state["value"]), B, 1.0, life, 10, 1,
                                   ptr(state["tsel"]), ptr(values), ptr(flags), st) == _lib.BGX_OK
        assert call_cut(state, s, st=st, **CUT_KW) == _lib.BGX_OK
    torch.cuda.synchronize()
    for k, v in before.items():                            # the capture ran nothing (bytes: the values hold NaNs)
        assert torch.equal(state[k].view(torch.uint8), v.view(torch.uint8)), k
    assert bool(torch.isnan(values).all())
    g.replay()
    torch.cuda.synchronize()
    for k in ("tally", "mask", "games_done", "plies", "sel", "cube", "active"):
        assert torch.equal(state[k], eager[k]), k
    assert torch.equal(flags, e_flags) and torch.equal(values.view(torch.int32), e_values.view(torch.int32))
    assert int(state["tally"][:, 0].sum()) > 100 and int((flags != 0).sum()) > 100


# ---------------------------------------------------------------------- 11. the command line --
def test_command_line(tmp_path, capsys):
    from bgx import rollout
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    ckpt = str(tmp_path / "net.pt")
    torch.save(PolicyNet(hidden_size=40).state_dict(), ckpt)
    base = ["--net", ckpt, "--positions", "opening", "--trials", "72", "--batch", "128", "--max-steps", "6000", "--cube",
            "--cube-double", "0.13", "--cube-pass", "0.19", "--cube-cap", "4", "--cube-truncate", "8"]
    rollout.main(base)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["position"] == 0 and lines[1]["summary"] and lines[1]["cube"] is True
    r, s = lines
    assert r["games"] == 72 and r["unfinished"] == 0
    assert r["games"] == r["played_out"]["games"] + r["pass_games"] + r["truncated_games"] and r["truncated_games"] > 0
    assert s["steps"] <= 8 + 16 and r["plies_per_game"] <= 8.0
    for k in ("equity_cubeful", "equity_cubeful_stderr", "truncated_equity_cubeful", "pass_share", "mean_cube_log2"):
        assert math.isfinite(r[k]), k
    assert (s["cube_truncate"], s["cube_life"], s["cube_win_value"], s["cube_loss_value"]) == (8, 0.68, 1.0, 1.0)
    assert (s["cube_truncate_lookahead"], s["cube_truncate_scale"], s["cube_truncate_net"]) == (0, 1.0, None)
    assert s["truncated_games"] == r["truncated_games"] and s["truncated_share"] == r["truncated_share"]
    rollout.main(base + ["--cube-decision", "--cube-life", "0.5", "--cube-win-value", "1.4", "--cube-loss-value", "1.2",
                         "--cube-truncate-lookahead", "1", "--cube-truncate-net", ckpt, "--cube-truncate-scale", "2"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 2 and lines[0]["cube_decision"] is True
    d, s = lines
    assert d["double_pass"] == 1.0 and d["double"] == (min(d["double_take"], 1.0) > d["no_double"])
    assert d["take"] == (d["double_take"] <= 1.0) and len(d["rollouts"]) == 2
    assert all(r["truncated_games"] > 0 and r["games"] == 72 for r in d["rollouts"])         # both rollouts are truncated
    assert (s["cube_life"], s["cube_win_value"], s["cube_loss_value"]) == (0.5, 1.4, 1.2)
    assert (s["cube_truncate_lookahead"], s["cube_truncate_scale"], s["cube_truncate_net"]) == (1, 2.0, ckpt)
    assert s["games"] == 144 and s["truncated_share"] > 0
