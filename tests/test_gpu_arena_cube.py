"""The doubling cube in the arena (Arena.play with cube=, the bgx_arena_cube_* kernels of
csrc/bg_arena_cube.h): the kernels alone against the rule written out in scalar Python
(tests/arena_cube_ref.py), forced runs whose cubeful sums are known exactly from the plain tally,
traced runs of two different nets against arena.arena_cube_reference, CubeRule's lookahead 0, a
captured graph, the command line and the trainer's evaluation."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import arena_cube_ref as ref

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def struct(rule, cap=ref.CAP, jacoby=ref.JACOBY):
    from bgx._lib import BgxCubeRule
    scale, double_at, pass_at, too_good = rule
    return BgxCubeRule(scale, double_at, pass_at, too_good, cap, jacoby)


def fresh_net(seed, H=40):
    from bgx.policy import PolicyNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = PolicyNet(hidden_size=H)
    return net.cuda().eval()


class Const:
    """A cube rule's callable value: the same equity on every lane."""
    sync_free = True

    def __init__(self, v):
        self.v, self.t = float(v), None

    def __call__(self, eng, dsel):
        if self.t is None or self.t.numel() != eng.batch:
            self.t = torch.full((eng.batch,), self.v, dtype=torch.float32, device=eng.device)
        return self.t


# ------------------------------------------------------ kernels against the scalar rule --
class Device:
    """The hand-set state on the device and the six entry points on it."""

    def __init__(self, s):
        from bgx import _lib
        self.L, self.OK = _lib.load(), _lib.BGX_OK
        self.t = {k: dev(s[k]) for k in ("recs", "games_done", "sel_a", "sel_b", "cube", "plies", "eq_a", "eq_b", "er_a",
                                         "er_b", "done", "info")}
        self.t.update({k: torch.zeros(ref.N, dtype=torch.uint8).cuda() for k in ("dsel_a", "dsel_b", "off_a", "off_b",
                                                                                  "mask")})
        self.t["tally"] = torch.zeros(16, dtype=torch.int64).cuda()
        self.t["tally"][13] = int((s["games_done"] < ref.G).sum())
        self.t["ct"] = torch.zeros(16, dtype=torch.int64).cuda()
        self.ra, self.rb = struct(ref.RULE_A), struct(ref.RULE_B)

    def p(self, *names):
        return [ptr(self.t[k]) for k in names]

    def sel(self, st=None):
        assert self.L.bgx_arena_cube_sel(*self.p("recs", "sel_a", "sel_b", "plies", "cube"), ref.N, ref.CAP,
                                         *self.p("dsel_a", "dsel_b"), st) == self.OK

    def offer(self, st=None):
        assert self.L.bgx_arena_cube_offer(*self.p("recs", "dsel_a", "dsel_b", "eq_a", "eq_b"), self.ra, self.rb,
                                           *self.p("cube"), ref.N, *self.p("off_a", "off_b", "ct"), st) == self.OK

    def respond(self, st=None):
        assert self.L.bgx_arena_cube_respond(*self.p("recs", "off_a", "off_b", "er_a", "er_b"), self.ra, self.rb, ref.N,
                                             ref.G, *self.p("cube", "plies", "games_done", "sel_a", "sel_b", "tally",
                                                            "ct", "mask"), st) == self.OK

    def reseat(self, st=None):
        assert self.L.bgx_arena_cube_reseat(*self.p("recs", "mask"), ref.N, ref.G,
                                            *self.p("games_done", "sel_a", "sel_b"), st) == self.OK

    def flush(self, st=None):
        assert self.L.bgx_arena_cube_flush(*self.p("sel_a", "sel_b", "done", "info", "games_done"), ref.N, ref.JACOBY,
                                           ref.CAP, *self.p("cube", "plies", "ct"), st) == self.OK

    def get(self, *names):
        return [self.t[k].cpu().numpy() for k in names]


def same(got, want, what):
    for g, w, name in zip(got, want, what):
        assert np.array_equal(g, np.asarray(w).astype(g.dtype)), (name, np.flatnonzero(g != np.asarray(w))[:8])


def test_kernels_equal_the_scalar_rule():
    """sel, offer, respond, reseat and flush at 300 lanes (two 256-thread blocks, a partial last
    wave) on a hand-set state -- retired lanes, game_over records, bytes that are no cube states,
    both seats, synthetic equities -- against the rule one lane at a time.  The reference reaches
    every branch and every counted field (asserted here and, without a GPU, in
    test_arena_cube_cpu.py)."""
    out, seen = ref.run_reference()
    assert seen == ref.BRANCHES and all(out["ct_flush"][:11] != 0)
    d = Device(out["state0"])
    # begin, on arrays of its own
    junk = [torch.full((ref.N,), 77, dtype=dt).cuda() for dt in (torch.uint8, torch.int32)] + \
        [torch.full((16,), 5, dtype=torch.int64).cuda()]
    assert d.L.bgx_arena_cube_begin(ref.N, *[ptr(x) for x in junk], None) == d.OK
    assert all(not bool(x.any()) for x in junk)
    d.sel()
    same(d.get("dsel_a", "dsel_b"), out["dsel"], ("dsel_a", "dsel_b"))
    for k, v in zip(("dsel_a", "dsel_b"), out["dsel_forced"]):          # a dsel of another origin
        d.t[k].copy_(dev(v))
    d.offer()
    same(d.get("off_a", "off_b", "ct"), (*out["off"], out["ct_offer"]), ("off_a", "off_b", "cube_tally"))
    d.respond()
    names = ("cube", "plies", "games_done", "sel_a", "sel_b")
    same(d.get(*names), [out["after_respond"][k] for k in names], names)
    same(d.get("mask", "ct", "tally"), (out["mask"], out["ct_respond"], out["tally"]), ("mask", "cube_tally", "tally"))
    d.t["recs"].copy_(dev(out["recs_reset"]))                          # the masked reset's new records
    d.reseat()
    same(d.get("sel_a", "sel_b"), [out["after_reseat"][k] for k in ("sel_a", "sel_b")], ("sel_a", "sel_b"))
    d.flush()
    same(d.get("cube", "plies", "ct"), (out["after_flush"]["cube"], out["after_flush"]["plies"], out["ct_flush"]),
         ("cube", "plies", "cube_tally"))
    same(d.get("games_done", "tally"), (out["after_respond"]["games_done"], out["tally"]), ("games_done", "tally"))
    # every pass is a finished game of its lane
    assert int((out["after_respond"]["games_done"] - out["state0"]["games_done"]).sum()) == out["ct_flush"][5]
    torch.cuda.synchronize()


def test_kernels_in_one_graph_equal_eager():
    """The five per-step kernels captured in one linear graph and replayed on the hand-set state
    equal the eager calls (the records stay as they are between respond and reseat in both)."""
    s = ref.make_state()
    names = ("cube", "plies", "games_done", "sel_a", "sel_b", "dsel_a", "dsel_b", "off_a", "off_b", "mask", "ct", "tally")
    eager = Device(s)
    for step in (eager.sel, eager.offer, eager.respond, eager.reseat, eager.flush):
        step()
    want = eager.get(*names)
    assert want[names.index("mask")].any() and want[names.index("ct")][:11].all()
    d = Device(s)
    start = {k: d.t[k].clone() for k in names}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for step in (d.sel, d.offer, d.respond, d.reseat, d.flush):
            step(st)
    same(d.get(*names), [v.cpu().numpy() for v in start.values()], names)   # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    same(d.get(*names), want, names)


def test_argument_checks():
    from bgx import _lib
    L, n = _lib.load(), 64
    bufs = [torch.zeros(n * 64, dtype=torch.uint8).cuda() for _ in range(8)] + \
        [torch.zeros(n, dtype=torch.int32).cuda() for _ in range(3)] + \
        [torch.zeros(n, dtype=torch.float32).cuda() for _ in range(2)] + \
        [torch.zeros(16, dtype=torch.int64).cuda() for _ in range(2)]             # alive until the test ends
    u8, i32, f32 = [ptr(x) for x in bufs[:8]], [ptr(x) for x in bufs[8:11]], [ptr(x) for x in bufs[11:13]]
    t, ct = ptr(bufs[13]), ptr(bufs[14])
    ok = struct(ref.RULE_A)
    rules = [struct((math.nan, .4, .5, .8)), struct((1, math.nan, .5, .8)), struct((1, .4, math.nan, .8)),
             struct(ref.RULE_A, cap=11), struct(ref.RULE_A, cap=-1)]

    def each(fn, good, bad):
        assert fn(*good) == _lib.BGX_OK, fn.__name__
        for idx, val in bad:
            args = list(good)
            args[idx] = val
            assert fn(*args) == _lib.BGX_EINVAL, (fn.__name__, idx)

    each(L.bgx_arena_cube_begin, [n, u8[0], i32[0], ct, None], [(0, 0), (0, -1), (1, None), (2, None), (3, None)])
    each(L.bgx_arena_cube_sel, [u8[0], u8[1], u8[2], i32[0], u8[3], n, 3, u8[4], u8[5], None],
         [(i, None) for i in (0, 1, 2, 3, 4, 7, 8)] + [(5, 0), (6, -1), (6, 11)])
    good = [u8[0], u8[1], u8[2], f32[0], f32[1], ok, ok, u8[3], n, u8[4], u8[5], ct, None]
    each(L.bgx_arena_cube_offer, good, [(i, None) for i in (0, 1, 2, 3, 4, 7, 9, 10, 11)] + [(8, 0)] +
         [(5, r) for r in rules] + [(6, r) for r in rules] +
         [(6, struct(ref.RULE_A, cap=ref.CAP - 1)), (6, struct(ref.RULE_A, jacoby=0))])    # the game's cap and Jacoby
    assert L.bgx_arena_cube_offer(*(good[:5] + [struct(ref.RULE_B)] * 2 + good[7:])) == _lib.BGX_OK   # too_good = inf
    each(L.bgx_arena_cube_respond,
         [u8[0], u8[1], u8[2], f32[0], f32[1], ok, ok, n, 2, u8[3], i32[0], i32[1], u8[4], u8[5], t, ct, u8[6], None],
         [(i, None) for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16)] + [(7, 0), (8, -1)] +
         [(5, r) for r in rules] + [(6, r) for r in rules] + [(5, struct(ref.RULE_A, cap=ref.CAP + 1)),
                                                              (5, struct(ref.RULE_A, jacoby=0))])
    each(L.bgx_arena_cube_reseat, [u8[0], u8[1], n, 2, i32[0], u8[2], u8[3], None],
         [(i, None) for i in (0, 1, 4, 5, 6)] + [(2, 0), (3, -1)])
    each(L.bgx_arena_cube_flush, [u8[0], u8[1], u8[2], i32[0], i32[1], n, 1, 3, u8[3], i32[2], ct, None],
         [(i, None) for i in (0, 1, 2, 3, 4, 8, 9, 10)] + [(5, 0), (7, -1), (7, 11)])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- forced runs --
B200, G2 = 200, 2


def forced(rule_a, rule_b, seed=3):
    from bgx.arena import Arena, ArenaCube, RandomPlayer
    ar = Arena(B200, G2, seed=seed)
    res = ar.play(RandomPlayer(11), RandomPlayer(12), max_steps=6000, cube=ArenaCube(rule_a, rule_b))
    assert ar.eng.error() == 0 and res["unfinished_lanes"] == 0 and res["games"] == B200 * G2
    assert res["cube_games"] == res["played_out"]["games"] + res["pass_games"]
    assert res["pass_games"] == res["passes_a"] + res["passes_b"]
    return res


def rule_of(v, **kw):
    from bgx.cube import CubeRule
    return CubeRule(Const(v), **kw)


def test_a_always_doubles_b_always_takes():
    r = forced(rule_of(0.45), None)
    p = r["played_out"]
    assert r["doubles_a"] == r["games"] == p["games"] and r["doubles_b"] == 0 and r["pass_games"] == 0
    assert r["cube_points_a"] == 2 * (p["points_a"] - p["points_b"])
    assert r["cube_log2"] == r["games"] and r["take_share_b"] == 1.0 and r["cube_wins_a"] == p["wins_a"]
    assert r["ppg_cubeful_a"] == 2 * p["ppg_a"] and r["ppg_cubeful_stderr"] == pytest.approx(2 * p["ppg_stderr"], rel=1e-12)


def test_b_always_passes():
    r = forced(rule_of(0.45), rule_of(0.9, double_at=math.inf))
    assert r["pass_games"] == r["passes_b"] == r["doubles_a"] == r["games"] and r["passes_a"] == 0
    assert r["ppg_cubeful_a"] == 1.0 and r["ppg_cubeful_stderr"] == 0.0 and r["win_rate_cubeful_a"] == 1.0
    assert r["played_out"]["games"] == 0 and r["played_out"]["wins_a"] + r["played_out"]["wins_b"] == 0
    assert r["pass_share"] == 1.0 and r["take_share_b"] == 0.0 and r["cube_log2"] == 0
    # a pass comes at A's first turn after the game's first ply: 1 or 2 plies in
    assert r["games"] <= r["pass_plies"] <= 2 * r["games"]


def test_redoubles_reach_the_cap():
    r = forced(rule_of(0.45, cap=3), rule_of(0.45, cap=3))
    assert r["pass_games"] == 0 and r["cube_log2"] == 3 * r["games"] and r["mean_cube_log2"] == 3.0
    assert r["doubles_a"] + r["doubles_b"] == 3 * r["games"] and abs(r["doubles_a"] - r["doubles_b"]) <= r["games"]
    p = r["played_out"]
    assert r["cube_points_a"] == 8 * (p["points_a"] - p["points_b"])


def test_jacoby_on_and_off():
    on = forced(rule_of(0.0, jacoby=True), rule_of(0.0, jacoby=True))
    off = forced(rule_of(0.0), rule_of(0.0))
    p = on["played_out"]
    assert p == off["played_out"] and p["gammons_a"] + p["gammons_b"] + p["backgammons_a"] + p["backgammons_b"] > 0
    assert on["cube_points_a"] == p["wins_a"] - p["wins_b"] and on["cube_points2"] == p["games"]
    assert off["cube_points_a"] == p["points_a"] - p["points_b"] and off["cube_points2"] > p["games"]
    assert on["doubles_a"] + on["doubles_b"] == 0 == on["cube_log2"]


def test_no_rules_is_the_plain_match():
    from bgx.arena import Arena, RandomPlayer
    r = forced(None, None)
    p = r["played_out"]
    assert r["cube_points_a"] == p["points_a"] - p["points_b"] and r["cube_wins_a"] == p["wins_a"]
    assert r["doubles_a"] == r["doubles_b"] == 0 == r["pass_games"] and r["ppg_cubeful_a"] == p["ppg_a"]
    assert r["ppg_cubeful_stderr"] == pytest.approx(p["ppg_stderr"], rel=1e-12)
    # and the games are those of the match without a cube
    plain = Arena(B200, G2, seed=3).play(RandomPlayer(11), RandomPlayer(12), max_steps=6000)
    assert plain == p


def test_rules_of_two_games_are_refused():
    from bgx.arena import Arena, ArenaCube, RandomPlayer
    with pytest.raises(ValueError, match="belong to the game"):
        ArenaCube(rule_of(0.0, cap=3), rule_of(0.0, cap=4))
    with pytest.raises(ValueError, match="ArenaCube or None"):
        Arena(64, 1).play(RandomPlayer(1), RandomPlayer(2), max_steps=10, cube=rule_of(0.0))


# ------------------------------------------------------------------------- traced runs --
@pytest.fixture(scope="module")
def nets():
    return fresh_net(1), fresh_net(2)


@pytest.mark.parametrize("lookahead", [0, 1])
def test_traced_run_equals_reference(nets, lookahead):
    """Two different nets, each doubling and answering by its own value head and thresholds: the
    device tallies and the traced states equal the host replay, and a second run equals the first.
    The thresholds sit inside the range of these fresh nets' scaled values, whose heads start with
    a negative offset (8 V_a has quartiles near -1.0, -0.7, -0.4 on the lanes A may double on, 6 V_b
    near -1.1, -0.9, -0.7), so that both sides double and some doubles are taken, some passed."""
    from bgx.arena import Arena, ArenaCube, FIELDS, CUBE_FIELDS, PolicyPlayer, arena_cube_reference
    from bgx.cube import CubeRule
    from bgx.search import ValueHead
    B, G = 64, 2
    runs = []
    for _ in range(2):
        ra = CubeRule(ValueHead(nets[0]), scale=8.0, double_at=-0.4, pass_at=-0.6, too_good_at=2.0, cap=3, lookahead=lookahead)
        rb = CubeRule(ValueHead(nets[1]), scale=6.0, double_at=-0.4, pass_at=-0.85, cap=3, lookahead=lookahead)
        assert ra.sync_free == (lookahead == 0)
        ar = Arena(B, G, seed=7)
        res, tr = ar.play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=3000, trace=True,
                          cube=ArenaCube(ra, rb))
        assert ar.eng.error() == 0
        runs.append((res, {k: v.cpu().numpy() for k, v in tr.items()}, ar.games_done.cpu().numpy()))
    res, tr, games_done = runs[0]
    print({k: res[k] for k in ("games", "steps", "unfinished_lanes", "pass_games", "doubles_a", "doubles_b", "passes_a",
                                "passes_b", "cube_log2", "ppg_cubeful_a")})
    out = arena_cube_reference(tr, B, G, ra, rb)
    assert [res[k] for k in CUBE_FIELDS] == out["cube_tally"][:11].tolist()
    assert [res["played_out"][k] for k in FIELDS] == out["tally"][:14].tolist()
    assert np.array_equal(games_done, out["games_done"]) and res["unfinished_lanes"] == out["tally"][13]
    for k in ("cube", "dsel", "offer"):
        assert np.array_equal(tr[k], out[k]), k
    assert np.array_equal(tr["passed"] != 0, out["passed"])
    # the equities are traced where they were used, NaN elsewhere
    assert np.array_equal(np.isnan(tr["eq_offer"]), tr["dsel"] == 0)
    assert np.array_equal(np.isnan(tr["eq_resp"]), tr["offer"] == 0)
    # the run has cube action to compare: doubles of both sides, takes and passes
    assert res["doubles_a"] > 0 and res["doubles_b"] > 0
    assert 0 < res["pass_games"] < res["doubles_a"] + res["doubles_b"]
    assert res == runs[1][0]
    for k in tr:
        assert np.array_equal(tr[k], runs[1][1][k], equal_nan=True), k


def test_cube_none_is_the_plain_path(nets):
    from bgx.arena import Arena, PolicyPlayer
    a = Arena(64, 1, seed=9).play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=300, trace=True)
    b = Arena(64, 1, seed=9).play(PolicyPlayer(nets[0], seed=5), PolicyPlayer(nets[1], seed=6), max_steps=300, trace=True,
                                  cube=None)
    assert a[0] == b[0] and "ppg_stderr" in a[0] and "played_out" not in b[0]
    assert sorted(a[1]) == sorted(b[1]) == ["action", "done", "info", "mover", "n_moves", "owner"]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_lookahead_0_is_value_lanes(nets):
    import bgx
    from bgx.cube import CubeRule
    from bgx.search import ValueHead, value_lanes
    B = 300
    eng = bgx.Engine(batch=B, max_moves=500, seed=4, dice="philox", auto_reset=True)
    eng.reset()
    rng = np.random.RandomState(3)
    for _ in range(9):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    vh = ValueHead(nets[0])
    sel = dev((rng.rand(B) < 0.4).astype(np.uint8))
    rule = CubeRule(vh, lookahead=0)
    assert rule.sync_free and not CubeRule(vh).sync_free
    out = torch.full((B,), -7.0, dtype=torch.float32).cuda()
    got = rule.equity(eng, sel, torch.zeros(B).cuda(), out)
    want = value_lanes(eng, vh, sel=sel, out=torch.full((B,), -7.0, dtype=torch.float32).cuda())
    assert got is out and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool((got[sel == 0] == -7.0).all()) and bool((got[sel != 0] != -7.0).any()) and rule.totals["calls"] == 1
    # lookahead 1, the default, is roll_luck's mean: another number
    one = CubeRule(vh).equity(eng, sel, torch.zeros(B).cuda(), torch.full((B,), -7.0, dtype=torch.float32).cuda())
    assert not torch.equal(one, got) and bool((one[sel == 0] == -7.0).all())


# ----------------------------------------------------------------------- command lines --
def test_command_line(tmp_path, capsys):
    from bgx import arena
    paths = []
    for i, net in enumerate((fresh_net(1), fresh_net(2))):
        paths.append(str(tmp_path / f"net{i}.pt"))
        torch.save(net.state_dict(), paths[-1])
    res = arena.main(["--a", paths[0], "--b", paths[1], "--batch", "128", "--games-per-lane", "1", "--max-steps", "3000",
                      "--seed", "3", "--cube", "--cube-cap", "4", "--jacoby", "--cube-scale-a", "8", "--cube-double-a",
                      "0.3", "--cube-lookahead-a", "0", "--cube-lookahead-b", "0", "--cube-net-b", paths[0]])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert line["cube"] is True and (line["cube_cap"], line["jacoby"]) == (4, True)
    assert (line["cube_double_a"], line["cube_scale_a"], line["cube_lookahead_a"], line["cube_double_b"],
            line["cube_net_b"], line["cube_too_good_b"]) == (0.3, 8.0, 0, 0.4, paths[0], None)
    assert line["games"] + line["unfinished_lanes"] == 128 and line["games"] == line["played_out"]["games"] + line["pass_games"]
    for k in ("ppg_cubeful_a", "ppg_cubeful_stderr", "win_rate_cubeful_a", "pass_share", "doubles_per_game_a",
              "doubles_per_game_b", "take_share_a", "take_share_b", "mean_cube_log2", "games_per_s"):
        assert math.isfinite(line[k]), k
    # a random side has no rule: it never doubles
    res = arena.main(["--a", paths[0], "--b", "random", "--batch", "128", "--games-per-lane", "1", "--max-steps", "3000",
                      "--cube", "--cube-scale-a", "8", "--cube-lookahead-a", "0"])
    capsys.readouterr()
    assert res["doubles_b"] == 0 and res["passes_b"] == 0 and "cube_double_b" not in res


def test_evaluate_with_the_cube_leaves_the_trainer_alone():
    from bgx.train import PPOTrainer, eval_metrics
    tr = PPOTrainer(batch=2048, horizon=8, seed=3)
    tr.iteration()
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in tr.net.parameters()]
    rng, counter, packed = torch.random.get_rng_state(), tr.step_counter, getattr(tr.net, "_packed", None)
    res = tr.evaluate("random", batch=128, games_per_lane=1, max_steps=3000, cube=True)
    torch.cuda.synchronize()
    for p, q in zip(tr.net.parameters(), before):
        assert torch.equal(p, q)
    assert torch.equal(torch.random.get_rng_state(), rng)
    assert tr.step_counter == counter and getattr(tr.net, "_packed", None) is packed
    assert res["games"] == 128 and res["unfinished_lanes"] == 0 and res["doubles_b"] == 0
    m = eval_metrics(res)
    assert m["eval_ppg_cubeful"] == res["ppg_cubeful_a"] and m["eval_pass_share"] == res["pass_share"]
    assert m["eval_games"] == 128 and m["eval_ppg"] == res["played_out"]["ppg_a"]
    plain = eval_metrics(tr.evaluate("random", batch=128, games_per_lane=1, max_steps=3000))
    assert "eval_ppg_cubeful" not in plain and plain["eval_games"] == 128
