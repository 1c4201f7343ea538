"""Match-score rollouts (Rollout.run_lanes / run with match=, the bgx_rollout_match_* kernels and
bgx_match_decision of csrc/bg_match_rollout.h): the kernels alone on the hand-set
state of tests/match_rollout_ref.py against match.match_decision_reference, a captured graph, the
argument checks, traced runs from short race positions against match.rollout_match_reference, the
decision helper and the command line."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import match_rollout_ref as ref
from bgx import match as M

pytestmark = pytest.mark.gpu

F = np.float32
N, P, G = ref.N, ref.P, ref.G


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def same_bits(got, want):
    return np.array_equal(np.asarray(got, F).view(np.uint32), np.asarray(want, F).view(np.uint32))


class Device:
    """The hand-set state on the GPU and the three rollout kernels on it."""

    def __init__(self, s, met, pc):
        from bgx import _lib
        self.L, self.lib, self.length = _lib.load(), _lib, s["L"]
        self.t = {k: dev(s[k]) for k in ("away", "craw", "group", "recs", "starts", "cube", "cube0", "value", "plies",
                                         "games_done", "sel", "done", "info")}
        self.t.update(met=dev(met.reshape(-1)), pc=dev(pc), dsel=torch.full((N,), 9, dtype=torch.uint8).cuda(),
                      mask=torch.full((N,), 9, dtype=torch.uint8).cuda(),
                      hist=torch.zeros(P, 96, dtype=torch.int64).cuda(),
                      active=torch.tensor([int(((s["sel"] != 0) & (s["group"] >= 0) & (s["group"] < P)).sum())]).cuda())
        self.rule = ref.rule_of(self.length).struct()

    def sel(self, st=None):
        t = self.t
        assert self.L.bgx_rollout_match_sel(ptr(t["recs"]), ptr(t["group"]), P, ptr(t["plies"]), ptr(t["sel"]),
                                            ptr(t["cube"]), ptr(t["away"]), ptr(t["craw"]), N, ptr(t["dsel"]),
                                            st) == self.lib.BGX_OK

    def decide(self, st=None):
        t = self.t
        assert self.L.bgx_rollout_match_decide(ptr(t["recs"]), ptr(t["starts"]), ptr(t["group"]), ptr(t["dsel"]),
                                               ptr(t["value"]), N, P, G, self.rule, ptr(t["met"]), ptr(t["pc"]),
                                               self.length, ptr(t["away"]), ptr(t["craw"]), ptr(t["cube0"]),
                                               ptr(t["cube"]), ptr(t["games_done"]), ptr(t["plies"]), ptr(t["sel"]),
                                               ptr(t["hist"]), ptr(t["active"]), ptr(t["mask"]), st) == self.lib.BGX_OK

    def flush(self, st=None):
        t = self.t
        assert self.L.bgx_rollout_match_flush(ptr(t["starts"]), ptr(t["group"]), ptr(t["sel"]), ptr(t["done"]),
                                              ptr(t["info"]), N, P, ptr(t["cube0"]), ptr(t["cube"]), ptr(t["hist"]),
                                              st) == self.lib.BGX_OK

    def get(self, *names):
        return [self.t[k].cpu().numpy() for k in names]


STATE = ("dsel", "mask", "cube", "games_done", "plies", "sel", "hist", "active")


# ------------------------------------------------ kernels against the host reference --
@pytest.mark.parametrize("L", ref.LENGTHS)
def test_kernels_equal_the_reference(L):
    """sel, decide and flush at 300 lanes on the hand-set state, every array against
    match_decision_reference lane by lane; then bgx_match_decision, values and flags bit for bit."""
    met, pc = M.met_table(L)
    s = ref.make_state(L)
    want, seen = ref.expected(s, met, pc)
    assert seen == ref.BRANCHES, ref.BRANCHES - seen
    d = Device(s, met, pc)
    d.sel()
    assert np.array_equal(d.get("dsel")[0], want["dsel"])
    d.decide()
    for name, got in zip(STATE, d.get(*STATE)):
        assert np.array_equal(got.reshape(-1), np.asarray(want[name]).reshape(-1)), name
    d.flush()
    hist, cube = d.get("hist", "cube")
    assert np.array_equal(hist, want["hist_flush"]) and np.array_equal(cube, want["cube_flush"])
    assert (hist[:, 94:] == 0).all() and np.array_equal(hist[:, 88], hist[:, :88].sum(axis=1))
    # the static decision on the same records, cubes and values, with per-lane scores
    from bgx import _lib
    lib = _lib.load()
    values = torch.full((N, 3), 7.0, dtype=torch.float32).cuda()
    flags = torch.full((N,), 0xEE, dtype=torch.uint8).cuda()
    t = d.t
    cube_in = dev(s["cube"])
    assert lib.bgx_match_decision(ptr(t["recs"]), ptr(cube_in), ptr(dev(want["static_away"])), ptr(dev(want["static_craw"])),
                                  ptr(t["value"]), N, d.rule, ptr(t["met"]), ptr(t["pc"]), L, ptr(values), ptr(flags),
                                  None) == _lib.BGX_OK
    assert same_bits(values.cpu().numpy(), want["values"])
    assert np.array_equal(flags.cpu().numpy(), want["flags"])
    # the Python wrapper: the same answer from tensors
    m = M.RolloutMatch(L, ref.rule_of(L))
    v2, f2 = M.static_match_decision(t["recs"], t["value"], m, dev(want["static_away"]), dev(want["static_craw"]), cube_in)
    assert same_bits(v2.cpu().numpy(), want["values"]) and np.array_equal(f2.cpu().numpy(), want["flags"])
    v3, f3 = M.static_match_decision(t["recs"], t["value"], m, (3, 3), 0, None)          # one score, a centred cube
    mv = s["recs"][:, 52].astype(np.int64) & 1
    d3 = M.match_decision_reference(met, pc, L, 3, 3, 0, 0, mv, 1, s["value"], m.rule, over=s["recs"][:, 55] != 0)
    assert same_bits(v3.cpu().numpy(), np.stack([d3["nd"], d3["dt"], d3["dp"]], axis=1))
    assert np.array_equal(f3.cpu().numpy() & 3, d3["access"] * 1 + d3["offer"] * 2)
    torch.cuda.synchronize()


def test_kernels_in_one_graph_equal_eager():
    """sel, decide and flush captured in one linear graph and replayed on the hand-set state equal
    the eager calls."""
    L = 7
    met, pc = M.met_table(L)
    s = ref.make_state(L)
    eager = Device(s, met, pc)
    for step in (eager.sel, eager.decide, eager.flush):
        step()
    want = eager.get(*STATE)
    assert want[STATE.index("mask")].any() and want[STATE.index("hist")][:, 88].all()
    d = Device(s, met, pc)
    start = [d.t[k].clone() for k in STATE]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for step in (d.sel, d.decide, d.flush):
            step(st)
    for name, got, before in zip(STATE, d.get(*STATE), start):
        assert np.array_equal(got, before.cpu().numpy()), name                    # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    for name, got, w in zip(STATE, d.get(*STATE), want):
        assert np.array_equal(got, w), name


def test_argument_checks():
    from bgx import _lib
    lib = _lib.load()
    n = 64
    u8 = [torch.zeros(n * 64, dtype=torch.uint8).cuda() for _ in range(10)]
    i32 = [torch.zeros(n, dtype=torch.int32).cuda() for _ in range(4)]
    f32 = [torch.zeros(1024, dtype=torch.float32).cuda() for _ in range(4)]      # a table to 25 has 676 entries
    hist = torch.zeros(97, dtype=torch.int64).cuda()
    a, b, c, d, e, f, g, h, i, j = (ptr(x) for x in u8)
    grp, plies, gd, info = (ptr(x) for x in i32)
    val, met, pc, out = (ptr(x) for x in f32)
    ok = M.MatchRule(lambda *_: None).struct()

    def bad_rule(**kw):
        r = M.MatchRule(lambda *_: None).struct()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    rules = [bad_rule(scale=math.nan), bad_rule(window=math.nan), bad_rule(window=-0.1), bad_rule(window=1.5),
             bad_rule(win_gammons=math.nan), bad_rule(win_gammons=1.1), bad_rule(loss_gammons=-0.1),
             bad_rule(loss_gammons=math.nan)]

    def check(fn, good, bad):
        assert fn(*good) == _lib.BGX_OK
        for idx, v in bad:
            args = list(good)
            args[idx] = v
            assert fn(*args) == _lib.BGX_EINVAL, (fn.__name__, idx, v)

    check(lib.bgx_rollout_match_sel, [a, grp, 1, plies, b, c, d, e, n, f, None],
          [(k, None) for k in (0, 1, 3, 4, 5, 6, 7, 9)] + [(2, 0), (2, -1), (8, 0), (8, -3)])
    check(lib.bgx_rollout_match_decide,
          [a, b, grp, c, val, n, 1, 1, ok, met, pc, 7, d, e, f, g, gd, plies, h, ptr(hist), ptr(hist[96:]), i, None],
          [(k, None) for k in (0, 1, 2, 3, 4, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)]
          + [(5, 0), (6, 0), (7, -1), (11, 0), (11, 26), (11, -1)] + [(8, r) for r in rules])
    check(lib.bgx_rollout_match_flush, [a, grp, b, c, info, n, 1, d, e, ptr(hist), None],
          [(k, None) for k in (0, 1, 2, 3, 4, 7, 8, 9)] + [(5, 0), (6, 0)])
    check(lib.bgx_match_decision, [a, b, c, d, val, n, ok, met, pc, 7, out, j, None],
          [(k, None) for k in (0, 1, 2, 3, 4, 7, 8, 10, 11)] + [(5, 0), (5, -1), (9, 0), (9, 26)] + [(6, r) for r in rules])
    assert lib.bgx_rollout_match_decide(a, b, grp, c, val, n, 1, 0, bad_rule(scale=math.inf, window=1.0, win_gammons=0.0),
                                        met, pc, 25, d, e, f, g, gd, plies, h, ptr(hist), ptr(hist[96:]), i,
                                        None) == _lib.BGX_OK
    torch.cuda.synchronize()


# ----------------------------------------------- traced runs against the host replay --
B, G2 = 64, 2
AWAY = np.asarray(ref.FORCED_SCORES)
CRAW = np.asarray([0, 0])


def lanes64():
    group = np.repeat(np.arange(2), [30, 31]).astype(np.int32)
    for k in (9, 40, 63):
        group = np.insert(group, k, -1)
    starts = np.where((group == 1)[:, None], ref.GAMMONISH[None], ref.RACE[None]).astype(np.uint8)
    return torch.from_numpy(group), torch.from_numpy(starts)


def by_group(values, group):
    """A rule's callable value that depends on the lane's group alone."""
    v = torch.tensor([values[max(int(g), 0)] for g in group], dtype=torch.float32).cuda().contiguous()

    def value(eng, dsel):
        return v
    value.sync_free = True
    return value


def traced(match, away=AWAY, craw=CRAW, cube0=None, seed=5, player_seed=2):
    """Two traced runs of the same set-up: (the first run's results, its replay)."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    group, starts = lanes64()
    runs = []
    for _ in range(2):
        ro = Rollout(B, seed=seed)
        out = ro.run_lanes(RandomPlayer(player_seed), starts, group, 2, G2, max_steps=400, trace=True, match=match,
                           match_score=(away, craw), cube0=cube0)
        assert ro.eng.error() == 0 and len(out) == 4 and not out[1].any()
        runs.append(out)
    (tally, _, tr, hist), (tally2, _, tr2, hist2) = runs
    assert torch.equal(hist, hist2) and torch.equal(tally, tally2)              # run to run identical
    for k in ("match_cube", "match_dsel", "match_action", "action", "done", "info"):
        assert torch.equal(tr[k], tr2[k]), k
    rp = M.rollout_match_reference(tr, starts, group, 2, G2, match, away, craw, cube0)
    hist, tally = hist.cpu().numpy(), tally.cpu().numpy()
    assert np.array_equal(hist, rp["match_hist"]) and np.array_equal(tally, rp["tally"])
    assert np.array_equal(tr["games_done"].cpu().numpy(), rp["games_done"]) and tr["active"] == rp["active"] == 0
    assert np.array_equal(tr["match_cube"].cpu().numpy(), rp["cube"])
    assert np.array_equal(tr["match_dsel"].cpu().numpy() != 0, rp["dsel"])
    assert np.array_equal(tr["match_action"].cpu().numpy(), rp["action"])
    on = tr["match_dsel"] != 0
    assert torch.isnan(tr["match_value"][~on]).all()
    assert not tr["match_dsel"][:, group.cuda() < 0].any()
    assert (hist[:, 94:] == 0).all() and np.array_equal(hist[:, 88], hist[:, :88].sum(axis=1))
    assert hist[:, 88].sum() == int((group >= 0).sum()) * G2                    # every scheduled game ended
    return hist, tally, tr


def by_kind(hist):
    return hist[:, :88].reshape(-1, 2, 4, 11)


def test_random_player_without_a_rule():
    """No rule: nobody doubles; the played-out bins summed over k are the plain tally's win / gammon /
    backgammon counts, all at the starting cube; the gammon bins fill."""
    from bgx.cube import pack
    group, _ = lanes64()
    cube0 = torch.tensor([pack(1, 1) if g == 1 else 0 for g in group], dtype=torch.uint8)
    hist, tally, tr = traced(M.RolloutMatch(7, None), cube0=cube0)
    b = by_kind(hist)
    assert not hist[:, 89:93].any() and not tr["match_action"].any() and not b[:, :, 0].any()
    assert np.array_equal(b[:, 1, 1:].sum(axis=2), tally[:, 2:5]) and np.array_equal(b[:, 0, 1:].sum(axis=2), tally[:, 5:8])
    assert b[0, :, :, 0].sum() == hist[0, 88] and b[1, :, :, 1].sum() == hist[1, 88]       # all at the start k
    assert np.array_equal(hist[:, 93], hist[:, 88] * [0, 1])
    assert b[1, 1, 2:].sum() > 0                                               # the gammon bins fill: PLAYER2 had none off
    assert tr["match_dsel"][:, group.cuda() == 0].any()                        # there was access, and a NaN decided nothing
    # the summary reads them
    mwc88 = M.outcome_mwc(*M.met_table(7), 7, AWAY[1], 0, 0)
    s = M.summarize_match_rollout(tally[1], hist[1], mwc88, 0, cube_k=1)
    assert s["games"] == hist[1, 88] and 0.0 < s["mwc"] < 1.0 and s["pass_share"] == 0.0 and s["mean_cube_log2"] == 1.0


def test_always_doubled_and_taken_up_to_the_dead_cube():
    m = M.RolloutMatch(7, M.MatchRule(lambda *_: None, window=0.0, win_gammons=0.0, loss_gammons=0.0))
    vals = [ref.forced_value(m, tuple(a), 1)[0] for a in AWAY]
    group, _ = lanes64()
    m = M.RolloutMatch(7, M.MatchRule(by_group(vals, group), window=0.0, win_gammons=0.0, loss_gammons=0.0))
    assert m.sync_free
    hist, tally, tr = traced(m)
    b = by_kind(hist)
    assert not hist[:, 89].any() and not b[:, :, 0].any() and (hist[:, 90] > 0).all() and (hist[:, 91] > 0).all()
    assert np.array_equal(hist[:, 88], tally[:, 0])
    k = tr["match_cube"].cpu().numpy() & 15
    assert k.max() == 3                                                        # 8: dead for sides that need 5, 6 or 7
    assert not tr["match_dsel"].cpu().numpy()[k == 3].any()
    assert b[:, :, :, 1:4].sum() > 0 and b[:, :, :, 4:].sum() == 0             # games ended at doubled cubes, none past 8


def test_always_doubled_and_passed():
    m = M.RolloutMatch(7, M.MatchRule(lambda *_: None, window=0.0, win_gammons=0.0, loss_gammons=0.0))
    vals = [ref.forced_value(m, tuple(a), 2)[0] for a in AWAY]
    group, _ = lanes64()
    m = M.RolloutMatch(7, M.MatchRule(by_group(vals, group), window=0.0, win_gammons=0.0, loss_gammons=0.0))
    hist, tally, tr = traced(m)
    b = by_kind(hist)
    # the first decision of a game is the other side's (no cube action on the first ply): it doubles, the start mover passes
    assert hist[:, 89].sum() > 0 and np.array_equal(hist[:, 89], b[:, :, 0].sum(axis=(1, 2)))
    assert np.array_equal(hist[:, 88], tally[:, 0] + hist[:, 89])
    assert b[:, :, :, 1:].sum() == 0 and not (tr["match_cube"].cpu().numpy() & 15).any()          # no take anywhere
    assert np.array_equal(hist[:, 90] + hist[:, 91], hist[:, 89])              # every double was passed
    assert (tr["match_action"].cpu().numpy() == 2).sum() == hist[:, 89].sum()


@pytest.mark.parametrize("lookahead", [0, 1])
def test_fresh_net_with_its_own_rule(lookahead):
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead
    torch.manual_seed(0)
    vh = ValueHead(PolicyNet(hidden_size=40).cuda())
    m = M.RolloutMatch(7, M.MatchRule(vh, scale=3.0, window=0.3, lookahead=lookahead))
    assert m.sync_free == (lookahead == 0)
    hist, tally, tr = traced(m, away=np.asarray([[3, 5], [2, 4]]))
    on = tr["match_dsel"] != 0
    assert on.any() and torch.isfinite(tr["match_value"][on]).all()
    print("lookahead", lookahead, "value quantiles", np.quantile(tr["match_value"][on].cpu().numpy(), [0, 0.25, 0.5, 0.75, 1]).tolist(),
          "sums", hist[:, 88:94].tolist())


def test_one_away_each_is_the_plain_win_rate():
    """At 1-away / 1-away whoever wins the game wins the match: no double occurs, even by a rule that
    always wants one, and mwc is the plain win rate exactly."""
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    group, _ = lanes64()
    m = M.RolloutMatch(7, M.MatchRule(by_group([0.9, 0.9], group), window=0.0))
    hist, tally, tr = traced(m, away=np.asarray([[1, 1], [1, 1]]))
    assert not hist[:, 89:94].any() and not tr["match_dsel"].any()
    ro = Rollout(B, seed=3)
    res = ro.run(RandomPlayer(4), torch.from_numpy(np.stack([ref.RACE, ref.GAMMONISH])), 64, first_roll="random",
                 max_steps=400, match=m, match_away=(1, 1))
    for r in res:
        p = r["played_out"]
        assert r["games"] == p["games"] == 64 and r["unfinished"] == 0 and r["doubles_start"] == r["doubles_other"] == 0
        assert r["mwc"] == (p["win1"] + p["win2"] + p["win3"]) / p["games"] and r["mwc"] == pytest.approx(p["win"], rel=1e-15)
        assert r["mwc_normalized"] == pytest.approx(2 * r["mwc"] - 1, rel=1e-15)
    assert res[1]["played_out"]["win2"] > 0


# ------------------------------------------------------------------------- other checks --
def test_match_none_is_the_old_tuple():
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    group, starts = lanes64()
    ro = Rollout(B, seed=5)
    out = ro.run_lanes(RandomPlayer(2), starts, group, 2, G2, max_steps=400, trace=True, match=None, match_score=None)
    assert len(out) == 3 and not any(k.startswith("match") for k in out[2])
    ro2 = Rollout(B, seed=5)
    out2 = ro2.run_lanes(RandomPlayer(2), starts, group, 2, G2, max_steps=400, trace=True)
    assert torch.equal(out[0], out2[0]) and torch.equal(out[2]["action"], out2[2]["action"])
    # the games of a run with no rule are those of the plain run
    out3 = Rollout(B, seed=5).run_lanes(RandomPlayer(2), starts, group, 2, G2, max_steps=400, match=M.RolloutMatch(7, None),
                                        match_score=(AWAY, CRAW))
    assert len(out3) == 4 and torch.equal(out3[0], out[0]) and out3[3].shape == (2, 96)
    with pytest.raises(ValueError, match="match_score without match"):
        ro.run_lanes(RandomPlayer(2), starts, group, 2, G2, match_score=(AWAY, CRAW))
    with pytest.raises(ValueError, match="match together with luck"):
        ro.run_lanes(RandomPlayer(2), starts, group, 2, G2, match=M.RolloutMatch(7, None), match_score=(AWAY, CRAW),
                     luck=object())
    with pytest.raises(ValueError, match="match_score"):
        ro.run_lanes(RandomPlayer(2), starts, group, 2, G2, match=M.RolloutMatch(7, None))
    with pytest.raises(ValueError, match="validate_score"):
        ro.run_lanes(RandomPlayer(2), starts, group, 2, G2, match=M.RolloutMatch(7, None),
                     match_score=(np.asarray([[1, 5], [3, 3]]), CRAW))
    torch.cuda.synchronize()


def test_rollout_match_decision():
    from bgx.arena import RandomPlayer
    from bgx.rollout import Rollout
    met, pc = M.met_table(7)
    group = torch.zeros(B, dtype=torch.int32)
    m = M.RolloutMatch(7, M.MatchRule(by_group([-1.0], group), window=0.0))     # nobody doubles again
    ro = Rollout(B, seed=6)
    rec = torch.from_numpy(ref.GAMMONISH)
    d = M.rollout_match_decision(ro, RandomPlayer(1), rec, 64, m, (3, 5), first_roll="random", max_steps=400)
    assert d["double_pass"] == float(met[2, 5]) and d["double_pass_stderr"] == 0.0
    assert [r["games"] for r in d["rollouts"]] == [64, 64] and d["rollouts"][1]["cube_log2"] == 64
    assert d["rollouts"][0]["cube_log2"] == 0 and d["cube"] == [0, 0] and d["away"] == [3, 5] and d["crawford"] == 0
    assert d["double"] == (min(d["double_take"], d["double_pass"]) > d["no_double"]) and d["take"] == (d["double_take"] <= d["double_pass"])
    assert 0.0 < d["no_double"] < 1.0 and d["no_double_stderr"] > 0.0
    # PLAYER2 on roll holding the cube at 2, after the Crawford game: it needs 5, the other 1
    rec2 = rec.clone()
    rec2[52] = 1
    d2 = M.rollout_match_decision(ro, RandomPlayer(1), rec2, 64, m, (1, 5), crawford=2, cube=(1, 2), first_roll="random",
                                  max_steps=400)
    assert d2["double_pass"] == float(pc[3]) and d2["rollouts"][1]["cube_log2"] == 128
    for kw in (dict(away=(1, 5), crawford=1),                    # the Crawford game
               dict(away=(3, 5), cube=(1, 2)),                   # not its cube
               dict(away=(3, 5), cube=(10, 1)),                  # at the cap
               dict(away=(2, 5), cube=(1, 1)),                   # x <= 2^k
               dict(away=(1, 1)),                                # x <= 1
               dict(away=(3, 8)), dict(away=(3, 5), crawford=2)):
        with pytest.raises(ValueError):
            M.rollout_match_decision(ro, RandomPlayer(1), rec, 64, m, **kw)
    torch.cuda.synchronize()


def test_command_line(tmp_path, capsys):
    from bgx import rollout
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    ckpt, table, pos = str(tmp_path / "net.pt"), str(tmp_path / "met.json"), str(tmp_path / "pos.json")
    torch.save(PolicyNet(hidden_size=40).state_dict(), ckpt)
    met, pc = M.met_table(5, gammon=0.2)
    M.save_met(table, 5, met, pc)
    with open(pos, "w") as fh:
        json.dump([{"board": [int(v) for v in r[:52]], "player": int(r[52])} for r in (ref.RACE, ref.GAMMONISH)], fh)
    base = ["--net", ckpt, "--positions", pos, "--trials", "32", "--first-roll", "random", "--batch", "64", "--max-steps",
            "400", "--match", "5", "--match-score", "3,4", "--met", table, "--match-lookahead", "0", "--match-scale", "3",
            "--match-window", "0.3"]
    rollout.main(base)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 3 and [l.get("position") for l in lines[:2]] == [0, 1] and lines[2]["summary"]
    mwc88 = M.outcome_mwc(met, pc, 5, (3, 4), 0, 0)
    for r in lines[:2]:
        assert r["games"] + r["unfinished"] == 32 and r["games"] == r["played_out"]["games"] + r["pass_games"]
        assert r["mwc"] == pytest.approx(float((np.asarray(r["match_hist"][:88]) * mwc88).sum() / r["games"]), rel=1e-13)
        assert 0.0 <= r["mwc"] <= 1.0 and math.isfinite(r["mwc_stderr"]) and math.isfinite(r["mwc_normalized"])
    s = lines[2]
    assert (s["match"], s["match_score"], s["met"], s["match_window"], s["match_rule"]) == (5, [3, 4], table, 0.3, True)
    assert s["games"] == sum(r["games"] for r in lines[:2]) and s["positions"] == 2
    rollout.main(base + ["--match-decision", "--match-net", ckpt])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 3 and lines[0]["match_decision"] is True and lines[2]["match_decision"] is True
    assert lines[0]["double_pass"] == float(met[2, 4]) and len(lines[1]["rollouts"]) == 2
    assert lines[2]["games"] == sum(x["games"] for l in lines[:2] for x in l["rollouts"])
    with pytest.raises(ValueError, match="matches to 5"):
        rollout.main([a if a != "5" else "7" for a in base])
