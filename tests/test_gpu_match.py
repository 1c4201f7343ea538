"""Match play in the arena (Arena.play with match=, the bgx_arena_match_* kernels of
csrc/bg_match.h): the kernels alone against the rule written out in scalar Python
(tests/match_ref.py), a captured graph, the argument checks, forced runs with known invariants and
traced runs of two different nets, all against match.arena_match_reference, and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import match_ref as ref

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def struct(rule):
    from bgx._lib import BgxMatchRule
    return BgxMatchRule(*rule)


def fresh_net(seed, H=40):
    from bgx.policy import PolicyNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = PolicyNet(hidden_size=H)
    return net.cuda().eval()


class Const:
    """A rule's callable value: the same on every lane; with two values, the first on a step's
    first call (the offer: the side's own roll) and the second on its second (the answer)."""
    sync_free = True

    def __init__(self, *v):
        self.v, self.t, self.calls = [float(x) for x in v], {}, 0

    def __call__(self, eng, dsel):
        v = self.v[self.calls % len(self.v)]
        self.calls += 1
        if v not in self.t or self.t[v].numel() != eng.batch:
            self.t[v] = torch.full((eng.batch,), v, dtype=torch.float32, device=eng.device)
        return self.t[v]


# ------------------------------------------------------ kernels against the scalar rule --
class Device:
    """The hand-set state on the device and the entry points on it."""
    U8 = ("dsel_a", "dsel_b", "off_a", "off_b", "mask")

    def __init__(self, s, L):
        from bgx import _lib
        self.lib, self.OK, self.Lm, self.G = _lib.load(), _lib.BGX_OK, L, ref.games_quota(L)
        self.t = {k: dev(s[k]) for k in ("recs", "games_done", "matches_done", "sel_a", "sel_b", "away", "craw", "cube",
                                         "plies", "seat0", "retire", "eq_a", "eq_b", "er_a", "er_b", "done", "info", "pc")}
        self.t["met"] = dev(s["met"].reshape(-1))
        self.t.update({k: torch.zeros(ref.N, dtype=torch.uint8).cuda() for k in self.U8})
        self.t["tally"] = torch.zeros(16, dtype=torch.int64).cuda()
        self.t["tally"][13] = int((s["games_done"] < self.G).sum())
        self.t["mt"] = torch.zeros(16, dtype=torch.int64).cuda()
        self.ra, self.rb = struct(ref.RULE_A), struct(ref.RULE_B)

    def p(self, *names):
        return [ptr(self.t[k]) for k in names]

    def sel(self, st=None):
        assert self.lib.bgx_arena_match_sel(*self.p("recs", "sel_a", "sel_b", "plies", "cube", "away", "craw"), ref.N,
                                            *self.p("dsel_a", "dsel_b"), st) == self.OK

    def offer(self, st=None):
        assert self.lib.bgx_arena_match_offer(*self.p("recs", "sel_a", "sel_b", "dsel_a", "dsel_b", "eq_a", "eq_b"), self.ra,
                                              self.rb, *self.p("met", "pc"), self.Lm,
                                              *self.p("plies", "cube", "away", "craw"), ref.N,
                                              *self.p("off_a", "off_b", "mt"), st) == self.OK

    def respond(self, st=None):
        assert self.lib.bgx_arena_match_respond(*self.p("recs", "off_a", "off_b", "er_a", "er_b"), self.ra, self.rb,
                                                *self.p("met", "pc"), self.Lm, ref.N, self.G, ref.M,
                                                *self.p("cube", "plies", "away", "craw", "matches_done", "seat0",
                                                        "games_done", "sel_a", "sel_b", "tally", "mt", "mask"), st) == self.OK

    def reseat(self, st=None):
        assert self.lib.bgx_arena_cube_reseat(*self.p("recs", "mask"), ref.N, self.G,
                                              *self.p("games_done", "sel_a", "sel_b"), st) == self.OK

    def flush(self, st=None):
        assert self.lib.bgx_arena_match_flush(*self.p("sel_a", "sel_b", "done", "info", "games_done"), ref.N, self.Lm, ref.M,
                                              *self.p("cube", "plies", "away", "craw", "matches_done", "seat0", "retire",
                                                      "mt"), st) == self.OK

    def retire(self, st=None):
        assert self.lib.bgx_arena_match_retire(ref.N, self.G, *self.p("retire", "games_done", "sel_a", "sel_b", "tally"),
                                               st) == self.OK

    def get(self, *names):
        return [self.t[k].cpu().numpy() for k in names]


def same(got, want, what):
    for g, w, name in zip(got, want, what):
        w = np.asarray(w).astype(g.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist())


@pytest.mark.parametrize("L", ref.LENGTHS)
def test_kernels_equal_the_scalar_rule(L):
    """begin, sel, offer, respond, reseat, flush and retire at 300 lanes (two 256-thread blocks, a
    partial last wave) on a hand-set state -- matches to 5 and to 7, every Crawford state, away 1..L
    on both sides, cube bytes that are no cube states and dead cubes, retired lanes, game_over
    records, both seats, synthetic values with NaN and the infinities, lanes whose last match ends
    -- against the rule one lane at a time.  The reference reaches every branch and every counted
    field (asserted here and, without a GPU, in test_match_cpu.py)."""
    out, seen = ref.run_reference(L)
    assert seen == ref.BRANCHES and all(out["mt_flush"] != 0)
    d = Device(out["state0"], L)
    # begin, on arrays of its own
    junk = [torch.full(shape, 77, dtype=dt).cuda()
            for shape, dt in (((ref.N, 2), torch.uint8), ((ref.N,), torch.uint8), ((ref.N,), torch.uint8),
                              ((ref.N,), torch.int32), ((ref.N,), torch.int32), ((ref.N,), torch.uint8),
                              ((ref.N,), torch.uint8), ((16,), torch.int64))]
    assert d.lib.bgx_arena_match_begin(ref.N, L, *[ptr(x) for x in junk], None) == d.OK
    away, craw, cube, plies, matches, seat0, retire, mt = [x.cpu().numpy() for x in junk]
    assert (away == L).all() and not any(x.any() for x in (craw, cube, plies, matches, retire, mt))
    assert np.array_equal(seat0, (np.arange(ref.N) & 1) == 0)
    d.sel()
    same(d.get("dsel_a", "dsel_b"), out["dsel"], ("dsel_a", "dsel_b"))
    for k, v in zip(("dsel_a", "dsel_b"), out["dsel_forced"]):          # a dsel of another origin
        d.t[k].copy_(dev(v))
    d.offer()
    same(d.get("off_a", "off_b", "mt"), (*out["off"], out["mt_offer"]), ("off_a", "off_b", "match_tally"))
    d.respond()
    same(d.get(*ref.LANE), [out["after_respond"][k] for k in ref.LANE], ref.LANE)
    same(d.get("mask", "mt", "tally"), (out["mask"], out["mt_respond"], out["tally_respond"]),
         ("mask", "match_tally", "tally"))
    d.t["recs"].copy_(dev(out["recs_reset"]))                          # the masked reset's new records
    d.reseat()
    same(d.get("sel_a", "sel_b"), [out["after_reseat"][k] for k in ("sel_a", "sel_b")], ("sel_a", "sel_b"))
    d.flush()
    same(d.get(*ref.LANE), [out["after_flush"][k] for k in ref.LANE], ref.LANE)
    same(d.get("mt", "tally"), (out["mt_flush"], out["tally_respond"]), ("match_tally", "tally"))
    d.retire()
    same(d.get(*ref.LANE), [out["after_retire"][k] for k in ref.LANE], ref.LANE)
    same(d.get("mt", "tally"), (out["mt_flush"], out["tally"]), ("match_tally", "tally"))
    assert out["tally"][13] < out["tally_respond"][13]                  # lanes whose last match ended played out
    torch.cuda.synchronize()


def test_kernels_in_one_graph_equal_eager():
    """The per-step kernels captured in one linear graph and replayed on the hand-set state equal
    the eager calls (the records stay as they are between respond and reseat in both)."""
    L = 7
    s = ref.make_state(L)
    names = ref.LANE + Device.U8 + ("mt", "tally")
    eager = Device(s, L)
    for step in (eager.sel, eager.offer, eager.respond, eager.reseat, eager.flush, eager.retire):
        step()
    want = eager.get(*names)
    assert want[names.index("mask")].any() and want[names.index("mt")].all()
    d = Device(s, L)
    start = {k: d.t[k].clone() for k in names}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for step in (d.sel, d.offer, d.respond, d.reseat, d.flush, d.retire):
            step(st)
    same(d.get(*names), [v.cpu().numpy() for v in start.values()], names)   # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    same(d.get(*names), want, names)


def test_argument_checks():
    from bgx import _lib
    lib, n, L = _lib.load(), 64, 5
    bufs = [torch.zeros(n * 64, dtype=torch.uint8).cuda() for _ in range(12)] + \
        [torch.zeros(n, dtype=torch.int32).cuda() for _ in range(3)] + \
        [torch.zeros(n, dtype=torch.float32).cuda() for _ in range(2)] + \
        [torch.zeros(16, dtype=torch.int64).cuda() for _ in range(2)]             # alive until the test ends
    from bgx.match import met_table
    met, pc = (dev(x.reshape(-1)) for x in met_table(L))
    u8, i32, f32 = [ptr(x) for x in bufs[:12]], [ptr(x) for x in bufs[12:15]], [ptr(x) for x in bufs[15:17]]
    t, mt, pm, pp = ptr(bufs[17]), ptr(bufs[18]), ptr(met), ptr(pc)
    ok = struct(ref.RULE_A)
    rules = [struct((NAN, .5, .2, .2)), struct((1, NAN, .2, .2)), struct((1, -.1, .2, .2)), struct((1, 1.1, .2, .2)),
             struct((1, .5, NAN, .2)), struct((1, .5, 1.5, .2)), struct((1, .5, .2, -.5)), struct((1, .5, .2, NAN))]

    def each(fn, good, bad):
        assert fn(*good) == _lib.BGX_OK, fn.__name__
        for idx, val in bad:
            args = list(good)
            args[idx] = val
            assert fn(*args) == _lib.BGX_EINVAL, (fn.__name__, idx, val)

    lengths = (0, -1, 26)
    each(lib.bgx_arena_match_begin, [n, L, u8[0], u8[1], u8[2], i32[0], i32[1], u8[3], u8[4], mt, None],
         [(0, 0), (0, -1)] + [(1, v) for v in lengths] + [(i, None) for i in range(2, 10)])
    each(lib.bgx_arena_match_sel, [u8[0], u8[1], u8[2], i32[0], u8[3], u8[4], u8[5], n, u8[6], u8[7], None],
         [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 8, 9)] + [(7, 0)])
    good = [u8[0], u8[1], u8[2], u8[3], u8[4], f32[0], f32[1], ok, ok, pm, pp, L, i32[0], u8[5], u8[6], u8[7], n, u8[8],
            u8[9], mt, None]
    each(lib.bgx_arena_match_offer, good, [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 9, 10, 12, 13, 14, 15, 17, 18, 19)] +
         [(16, 0)] + [(11, v) for v in lengths] + [(7, r) for r in rules] + [(8, r) for r in rules])
    assert lib.bgx_arena_match_offer(*(good[:7] + [struct((-INF, 0.0, 1.0, 0.0)), struct((INF, 1.0, 0.0, 1.0))] +
                                       good[9:])) == _lib.BGX_OK                       # the ends of the ranges
    G = 2 * (2 * L - 1)
    each(lib.bgx_arena_match_respond,
         [u8[0], u8[1], u8[2], f32[0], f32[1], ok, ok, pm, pp, L, n, G, 2, u8[3], i32[0], u8[4], u8[5], i32[1], u8[6],
          i32[2], u8[7], u8[8], t, mt, u8[9], None],
         [(i, None) for i in (0, 1, 2, 3, 4, 7, 8, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24)] + [(10, 0)] +
         [(9, v) for v in lengths] + [(11, G + 1), (11, 2), (12, -1), (12, 3)] + [(5, r) for r in rules] +
         [(6, r) for r in rules])
    each(lib.bgx_arena_match_flush,
         [u8[0], u8[1], u8[2], i32[0], i32[1], n, L, 2, u8[3], i32[2], u8[4], u8[5], i32[0], u8[6], u8[7], mt, None],
         [(i, None) for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14, 15)] + [(5, 0), (7, -1)] + [(6, v) for v in lengths])
    each(lib.bgx_arena_match_retire, [n, G, u8[0], i32[0], u8[1], u8[2], t, None],
         [(0, 0), (1, -1)] + [(i, None) for i in range(2, 7)])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- forced runs --
B128, M2 = 128, 2


def forced(length, rule_a, rule_b, seed=3, max_steps=14000):
    """Random players, 128 lanes, 2 matches per lane, traced: the run equals the host replay."""
    from bgx.arena import Arena, FIELDS, RandomPlayer
    from bgx.match import MATCH_FIELDS, ArenaMatch, arena_match_reference
    match = ArenaMatch(length, rule_a, rule_b)
    ar = Arena(B128, M2, seed=seed)
    res, tr = ar.play(RandomPlayer(11), RandomPlayer(12), max_steps=max_steps, trace=True, match=match)
    assert ar.eng.error() == 0
    tr = {k: v.cpu().numpy() for k, v in tr.items()}
    out = arena_match_reference(tr, B128, M2, match)
    assert [res[k] for k in MATCH_FIELDS] == out["match_tally"].tolist()
    assert [res["played_out"][k] for k in FIELDS] == out["tally"][:14].tolist()
    assert np.array_equal(ar.games_done.cpu().numpy(), out["games_done"])
    assert np.array_equal(ar.match_state["matches_done"].cpu().numpy(), out["matches_done"])
    for k in ("away", "craw", "cube", "dsel", "offer"):
        assert np.array_equal(tr[k], out[k]), k
    assert np.array_equal(tr["passed"] != 0, out["passed"])
    assert res["unfinished_lanes"] == int((out["matches_done"] < M2).sum()) == out["tally"][13]
    assert res["matches"] == int(out["matches_done"].sum()) > B128 and res["games"] == res["played_out"]["games"] + res["pass_games"]
    return res, tr, out


def mrule(*v, **kw):
    from bgx.match import MatchRule
    return MatchRule(Const(*v), **kw)


def test_no_rules_length_1_is_one_game_a_match():
    res, tr, _ = forced(1, None, None, max_steps=8000)
    p = res["played_out"]
    assert res["matches"] == res["games"] == p["games"] and res["match_wins_a"] == p["wins_a"]
    assert res["doubles_a"] == res["doubles_b"] == res["pass_games"] == res["cube_log2"] == 0
    assert res["crawford_games"] == res["post_crawford_games"] == 0 and not tr["dsel"].any()
    assert res["match_win_rate_a"] == p["win_rate_a"]


def test_no_rules_length_3_is_plain_points_to_3():
    res, tr, out = forced(3, None, None)
    assert not tr["cube"].any() and not tr["offer"].any() and res["cube_log2"] == 0 and res["pass_games"] == 0
    # the matches, counted apart from the replay: plain points per lane up to 3
    pts, matches, wins_a = np.zeros((B128, 2), np.int64), np.zeros(B128, np.int64), 0
    games = np.zeros(B128, np.int64)
    lane = np.arange(B128)
    for t in range(tr["done"].shape[0]):
        fin = (tr["owner"][t] != 0) & (tr["done"][t] != 0) & (((tr["info"][t] >> 8) & 0xFF) > 0)
        for i in np.nonzero(fin)[0]:
            assert tr["away"][t, i].tolist() == [3 - pts[i, 0], 3 - pts[i, 1]]
            a_won = ((((tr["info"][t, i] >> 8) & 0xFF) - 1) == 0) == (((lane[i] + games[i]) & 1) == 0)
            w = 0 if a_won else 1
            pts[i, w] += (tr["info"][t, i] >> 16) & 0xFF
            games[i] += 1
            if pts[i, w] >= 3:                                  # exactly when a side's points reach 3
                matches[i] += 1
                wins_a += a_won
                pts[i] = 0
    assert np.array_equal(matches, out["matches_done"]) and matches.max() == M2
    assert res["matches"] == matches.sum() and res["match_wins_a"] == wins_a
    assert res["match_points_a"] == res["played_out"]["points_a"] and res["match_points_b"] == res["played_out"]["points_b"]
    assert res["crawford_games"] > 0 and res["post_crawford_games"] > 0 and set(np.unique(tr["craw"])) == {0, 1, 2}


def test_a_always_doubles_b_always_takes():
    """A sees a sure win without gammons and doubles at window 0 wherever two points are worth no
    less than one (DT >= ND; ND = DP up to rounding); B has no rule: it never doubles and takes.
    At every offer 2^k is below A's away, and none in a Crawford game."""
    res, tr, _ = forced(5, mrule(1.0, window=0.0, win_gammons=0.0, loss_gammons=0.0), None)
    off = tr["offer"] == 1
    assert not (off & (tr["dsel"] != 1)).any() and off.sum() == res["doubles_a"] > B128
    assert res["doubles_b"] == 0 == res["pass_games"] and res["take_share_b"] == 1.0 and not (tr["offer"] == 2).any()
    k = np.minimum(tr["cube"] & 15, 10)
    assert ((1 << k[off]) < tr["away"][..., 0][off]).all() and (tr["craw"][off] != 1).all()
    assert res["cube_log2"] > 0 and k.max() >= 1
    assert np.array_equal(np.isnan(tr["eq_offer"]), tr["dsel"] != 1) and np.isnan(tr["eq_resp"]).all()   # B's value is NaN


def test_b_always_passes():
    """A doubles whenever it may; B never doubles (NaN on its own roll) and, seeing a sure win of
    the doubler with gammons in it, passes every double: every game A doubles in is worth 1 point."""
    res, tr, _ = forced(5, mrule(1.0, window=0.0, win_gammons=0.0, loss_gammons=0.0),
                        mrule(NAN, INF, loss_gammons=0.5))
    off = tr["offer"] == 1
    assert not (off & (tr["dsel"] != 1)).any() and np.array_equal(tr["passed"] != 0, off)
    assert res["doubles_a"] == res["passes_b"] == res["pass_games"] == off.sum() > B128
    assert res["doubles_b"] == res["passes_a"] == res["cube_log2"] == 0 and not tr["cube"].any()
    assert res["take_share_b"] == 0.0
    # the pass gives A one point and ends no match: one less to go at the lane's next step
    t, i = np.nonzero(off[:-1])
    assert np.array_equal(tr["away"][t + 1, i, 0], tr["away"][t, i, 0] - 1)
    assert np.array_equal(tr["away"][t + 1, i, 1], tr["away"][t, i, 1])
    p = res["played_out"]
    assert res["match_points_a"] == res["pass_games"] + p["points_a"] and res["match_points_b"] == p["points_b"]


# ------------------------------------------------------------------------- traced runs --
@pytest.fixture(scope="module")
def nets():
    return fresh_net(1), fresh_net(2)


# The value heads of these fresh nets start with a negative offset (8 V_a has quartiles near -1.0,
# -0.7, -0.4 on the lanes A may double on, 6 V_b near -1.1, -0.9, -0.7: test_gpu_arena_cube.py), so
# negative scales put the win probabilities around the doubling window and the take point.
RULES = (dict(scale=-8.0, window=0.65, win_gammons=0.25, loss_gammons=0.25),
         dict(scale=-4.0, window=0.3, win_gammons=0.3, loss_gammons=0.1))


@pytest.mark.parametrize("lookahead", [0, 1])
def test_traced_run_equals_reference(nets, lookahead):
    """Two different nets, each with its own MatchRule on its own value head: both device tallies,
    matches_done and the traced states equal the host replay, and a second run equals the first."""
    from bgx.arena import Arena, FIELDS, PolicyPlayer
    from bgx.match import MATCH_FIELDS, ArenaMatch, MatchRule, arena_match_reference
    from bgx.search import ValueHead
    B, Mn, L, steps = 64, 1, 3, 2500
    assert B * steps * 2 <= 1 << 22
    runs = []
    for _ in range(2):
        ra = MatchRule(ValueHead(nets[0]), lookahead=lookahead, **RULES[0])
        rb = MatchRule(ValueHead(nets[1]), lookahead=lookahead, **RULES[1])
        assert ra.sync_free == (lookahead == 0)
        match = ArenaMatch(L, ra, rb)
        ar = Arena(B, Mn, seed=7)
        res, tr = ar.play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=steps, trace=True,
                          match=match)
        assert ar.eng.error() == 0
        runs.append((res, {k: v.cpu().numpy() for k, v in tr.items()}, ar.games_done.cpu().numpy(),
                     ar.match_state["matches_done"].cpu().numpy()))
    res, tr, games_done, matches_done = runs[0]
    print({k: res[k] for k in ("matches", "games", "steps", "unfinished_lanes", "pass_games", "doubles_a", "doubles_b",
                                "passes_a", "passes_b", "cube_log2", "crawford_games", "post_crawford_games")})
    out = arena_match_reference(tr, B, Mn, match)
    assert [res[k] for k in MATCH_FIELDS] == out["match_tally"].tolist()
    assert [res["played_out"][k] for k in FIELDS] == out["tally"][:14].tolist()
    assert np.array_equal(games_done, out["games_done"]) and np.array_equal(matches_done, out["matches_done"])
    assert res["unfinished_lanes"] == out["tally"][13] == int((out["matches_done"] < Mn).sum())
    for k in ("away", "craw", "cube", "dsel", "offer"):
        assert np.array_equal(tr[k], out[k]), k
    assert np.array_equal(tr["passed"] != 0, out["passed"])
    assert np.array_equal(np.isnan(tr["eq_offer"]), tr["dsel"] == 0)
    assert np.array_equal(np.isnan(tr["eq_resp"]), tr["offer"] == 0)
    # the run has cube action to compare: doubles of both sides, takes and passes
    assert res["doubles_a"] > 0 and res["doubles_b"] > 0 and res["matches"] > 0
    assert 0 < res["pass_games"] < res["doubles_a"] + res["doubles_b"]
    assert res == runs[1][0]
    for k in tr:
        assert np.array_equal(tr[k], runs[1][1][k], equal_nan=True), k


def test_match_none_is_the_plain_path(nets):
    from bgx.arena import Arena, ArenaCube, PolicyPlayer
    from bgx.match import ArenaMatch
    a = Arena(64, 1, seed=9).play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=300, trace=True)
    b = Arena(64, 1, seed=9).play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=300, trace=True,
                                  match=None)
    assert a[0] == b[0] and "ppg_stderr" in a[0] and "matches" not in b[0]
    assert sorted(a[1]) == sorted(b[1]) == ["action", "done", "info", "mover", "n_moves", "owner"]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    ar, pl = Arena(64, 1), (PolicyPlayer(nets[0]), PolicyPlayer(nets[1]))
    with pytest.raises(ValueError, match="cube or luck"):
        ar.play(*pl, max_steps=10, match=ArenaMatch(3), cube=ArenaCube())
    from bgx.search import ValueHead
    with pytest.raises(ValueError, match="cube or luck"):
        ar.play(*pl, max_steps=10, match=ArenaMatch(3), luck=ValueHead(nets[0]))
    with pytest.raises(ValueError, match="ArenaMatch or None"):
        ar.play(*pl, max_steps=10, match=3)
    with pytest.raises(ValueError, match="x 2"):                 # the two-wide field counts
        ar.play(*pl, max_steps=(1 << 22) // 64 // 2 + 1, trace=True, match=ArenaMatch(3))


# ----------------------------------------------------------------------- command lines --
def test_command_line(tmp_path, capsys):
    from bgx import arena
    from bgx.match import met_table, save_met
    paths = []
    for i, net in enumerate((fresh_net(1), fresh_net(2))):
        paths.append(str(tmp_path / f"net{i}.pt"))
        torch.save(net.state_dict(), paths[-1])
    met = str(tmp_path / "met.json")
    save_met(met, 3, *met_table(3, 0.2, 0.01))
    res = arena.main(["--a", paths[0], "--b", paths[1], "--batch", "128", "--games-per-lane", "1", "--max-steps", "4000",
                      "--seed", "3", "--match", "3", "--met", met, "--match-scale-a", "-8", "--match-scale-b", "-4",
                      "--match-window-b", "0.3", "--match-gammons-b", "0.3,0.1", "--match-lookahead-a", "0",
                      "--match-lookahead-b", "0", "--match-net-b", paths[0]])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert (line["match"], line["met"], line["match_scale_a"], line["match_window_a"], line["match_window_b"],
            line["match_gammons_b"], line["match_lookahead_a"], line["match_net_b"]) == \
        (3, met, -8.0, 0.65, 0.3, [0.3, 0.1], 0, paths[0])
    assert line["matches"] + line["unfinished_lanes"] == 128 and line["games"] == line["played_out"]["games"] + line["pass_games"]
    assert line["games"] >= line["matches"] > 0 and line["doubles_a"] + line["doubles_b"] > 0
    for k in ("match_win_rate_a", "match_win_rate_stderr", "games_per_match", "doubles_per_game_a", "doubles_per_game_b",
              "take_share_a", "take_share_b", "pass_share", "mean_cube_log2", "crawford_share", "post_crawford_share",
              "match_win_rate_a_first_seat", "matches_per_s", "games_per_s"):
        assert math.isfinite(line[k]), k
    # a table for another length is refused; a random side has no rule: it never doubles
    with pytest.raises(ValueError, match="matches to 3"):
        arena.main(["--a", paths[0], "--b", paths[1], "--max-steps", "10", "--match", "5", "--met", met])
    res = arena.main(["--a", paths[0], "--b", "random", "--batch", "128", "--games-per-lane", "1", "--max-steps", "4000",
                      "--match", "3", "--match-scale-a", "-8", "--match-lookahead-a", "0"])
    capsys.readouterr()
    assert res["doubles_b"] == 0 and res["passes_b"] == 0 and "match_window_b" not in res and res["matches"] > 0
