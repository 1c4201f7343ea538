"""Luck-adjusted arena results on the device: bgx_arena_luck_add against
bgx_roll_luck (mid-game) and against the numpy twin (opening) bit for bit, the flush kernel against
a host replay of hand-set state, graph capture, a traced match against arena.arena_luck_reference, the estimate's
statistics, the opening rule's mean, and the other paths: the search players, the command line and
the trainer's evaluation."""
import ctypes
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
SENT = -12345.0


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
    """Bit for bit, except that a NaN is a NaN."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


@pytest.fixture(scope="module")
def net():
    from bgx.policy import PolicyNet
    torch.manual_seed(0)
    return PolicyNet(hidden_size=40).cuda()


@pytest.fixture(scope="module")
def vh(net):
    from bgx.search import ValueHead
    return ValueHead(net)


# ------------------------------------------------- 1. the entry point against bgx_roll_luck --
def test_luck_add_against_roll_luck_and_the_twin(vh):
    """256 posed and played records (tests/test_gpu_roll_luck.py's).  fresh = 0: luck_out and mean_out
    are bgx_roll_luck's on the same engine bit for bit; fresh = 1: the numpy twin's on the
    bgx_roll_values rows.  Unselected and game-over lanes keep every sentinel."""
    from bgx import _lib
    from bgx.arena import arena_roll_luck_reference
    from bgx.engine import R_OVER
    from bgx.search import roll_luck, roll_values
    RL = _module("test_gpu_roll_luck")
    B, L = RL.B, _lib.load()
    eng = RL.make_engine()
    luck_ref, mean_ref, _ = roll_luck(eng, vh)
    values, _ = roll_values(eng, vh)
    luck_ref, mean_ref, v = luck_ref.cpu().numpy(), mean_ref.cpu().numpy(), values.cpu().numpy()
    rng = np.random.RandomState(4)
    who = rng.randint(0, 3, B)                               # 0 nobody, 1 A, 2 B
    who[:3] = (1, 2, 1)                                      # the posed lanes are played
    over = (rng.rand(B) < 0.1) & (np.arange(B) >= 3)
    rec = eng.records().clone()
    rec[torch.from_numpy(over).cuda(), R_OVER] = 1
    rec_h = rec.cpu().numpy()
    assert (rec_h[:, 53] == rec_h[:, 54]).sum() > 10         # doubles are among the rolls
    on = (who != 0) & ~over
    assert on.sum() > 100 and (~on & (who != 0)).sum() > 5 and (who == 0).sum() > 50
    sel_a, sel_b = dev(who == 1, torch.uint8), dev(who == 2, torch.uint8)
    start = (rng.randn(B) * 3).astype(F)
    for fresh0 in (0, 1):
        lane_luck, fresh = dev(start), torch.full((B,), fresh0, dtype=torch.uint8, device="cuda")
        lo, mo = torch.full((B,), SENT, device="cuda"), torch.full((B,), SENT, device="cuda")
        assert L.bgx_arena_luck_add(ptr(rec), ptr(sel_a), ptr(sel_b), ptr(values), B, ptr(lane_luck), ptr(fresh), ptr(lo),
                                    ptr(mo), None) == _lib.BGX_OK
        torch.cuda.synchronize()
        lo, mo, ll, fr = lo.cpu().numpy(), mo.cpu().numpy(), lane_luck.cpu().numpy(), fresh.cpu().numpy()
        if fresh0 == 0:
            want_l, want_m = luck_ref, mean_ref
        else:
            want_l, want_m = arena_roll_luck_reference(v, rec_h[:, 53], rec_h[:, 54], 1)
            dbl = rec_h[:, 53] == rec_h[:, 54]
            assert (want_l[dbl] == 0).all() and (want_l[on & ~dbl] != 0).any()
            assert not np.array_equal(want_m[on], mean_ref[on])
        assert np.array_equal(bits(lo[on]), bits(want_l[on])) and np.array_equal(bits(mo[on]), bits(want_m[on]))
        signed = np.where(who == 1, want_l, -want_l).astype(F)
        assert np.array_equal(bits(ll[on]), bits((start + signed).astype(F)[on]))
        assert (fr[on] == 0).all()
        # every other lane: untouched
        assert (lo[~on] == SENT).all() and (mo[~on] == SENT).all() and (fr[~on] == fresh0).all()
        assert np.array_equal(bits(ll[~on]), bits(start[~on]))
        # the outputs are optional
        lane2, fresh2 = dev(start), torch.full((B,), fresh0, dtype=torch.uint8, device="cuda")
        assert L.bgx_arena_luck_add(ptr(rec), ptr(sel_a), ptr(sel_b), ptr(values), B, ptr(lane2), ptr(fresh2), None, None,
                                    None) == _lib.BGX_OK
        torch.cuda.synchronize()
        assert torch.equal(lane2, lane_luck) and torch.equal(fresh2, fresh)
    # bgx_arena_luck_begin: the state of a match's start, whatever was there
    tally = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    assert L.bgx_arena_luck_begin(B, ptr(lane_luck), ptr(fresh), ptr(tally), None) == _lib.BGX_OK
    torch.cuda.synchronize()
    assert not lane_luck.any() and bool((fresh == 1).all()) and not tally.any()
    # argument checks
    good = [ptr(rec), ptr(sel_a), ptr(sel_b), ptr(values), B, ptr(lane_luck), ptr(fresh), None, None, None]
    for k, val in ((0, None), (1, None), (2, None), (3, None), (4, 0), (5, None), (6, None)):
        bad = list(good)
        bad[k] = val
        assert L.bgx_arena_luck_add(*bad) == _lib.BGX_EINVAL, k
    assert L.bgx_arena_luck_begin(0, ptr(lane_luck), ptr(fresh), ptr(tally), None) == _lib.BGX_EINVAL
    assert L.bgx_arena_luck_begin(B, None, ptr(fresh), ptr(tally), None) == _lib.BGX_EINVAL
    assert eng.error() == 0


def test_luck_flush_against_host_replay():
    """Hand-set state, n = 700 (three blocks, the last one part full): every kind of lane -- idle,
    retired, active without a done, a done without a winner, counted games of every result and
    seat -- and sums that are huge, tiny, NaN and infinite.  The tally, lane_luck and fresh equal
    the host's."""
    from bgx import _lib
    from bgx.replay import luck_q
    L, n, G = _lib.load(), 700, 3
    rng = np.random.RandomState(13)
    games = rng.randint(0, G + 1, n)                         # G: retired
    who = np.where(games < G, rng.randint(0, 3, n), 0)       # an active lane may still be idle here (who = 0)
    done = (rng.rand(n) < 0.6).astype(np.uint8)
    winner, score = rng.randint(-1, 2, n), rng.randint(0, 5, n)       # scores 0 and 4: no points
    info = ((winner + 1) << 8) | (score << 16) | rng.randint(0, 256, n)
    luck = (rng.randn(n) * 2).astype(F)
    luck[::37], luck[5::41], luck[7::43], luck[9::47] = math.nan, math.inf, 1e30, 3e-6
    luck[11::53] = -40.0
    fresh = rng.randint(0, 2, n).astype(np.uint8)
    d = dict(sel_a=dev(who == 1, torch.uint8), sel_b=dev(who == 2, torch.uint8), done=dev(done),
             info=dev(info, torch.int32), games=dev(games, torch.int32), luck=dev(luck), fresh=dev(fresh),
             tally=torch.zeros(8, dtype=torch.int64, device="cuda"))
    args = [ptr(d["sel_a"]), ptr(d["sel_b"]), ptr(d["done"]), ptr(d["info"]), ptr(d["games"]), n, G, ptr(d["luck"]),
            ptr(d["fresh"]), ptr(d["tally"]), None]
    assert L.bgx_arena_luck_flush(*args) == _lib.BGX_OK
    torch.cuda.synchronize()
    active = (who != 0) & (games < G)
    dn = active & (done != 0)
    fin = dn & (winner >= 0)
    pts = np.where((score >= 1) & (score <= 3), score, 0)
    res = np.where((winner == 0) == (((np.arange(n) + games) & 1) == 0), pts, -pts)
    lq = [int(q) for q in luck_q(luck[fin])]
    want = [sum(lq), sum((q * q) & ((1 << 30) - 1) for q in lq), sum((q * q) >> 30 for q in lq),
            sum(int(x) * q for x, q in zip(res[fin], lq)), int(fin.sum()), 0, 0, 0]
    assert d["tally"].cpu().tolist() == want and want[4] > 50 and (dn & ~fin).sum() > 20 and want[2] > 0
    assert same(d["luck"].cpu().numpy(), np.where(dn, F(0), luck))
    assert np.array_equal(d["fresh"].cpu().numpy(), np.where(dn, 1, fresh))
    for k in (0, 1, 2, 3, 4, 7, 8, 9):
        bad = list(args)
        bad[k] = None
        assert L.bgx_arena_luck_flush(*bad) == _lib.BGX_EINVAL, k
    assert L.bgx_arena_luck_flush(*(args[:5] + [0] + args[6:])) == _lib.BGX_EINVAL
    assert L.bgx_arena_luck_flush(*(args[:6] + [-1] + args[7:])) == _lib.BGX_EINVAL


def test_graph_capture():
    """begin, add and flush captured as one linear chain on one stream: the capture runs nothing, the
    replay gives the eager results."""
    from bgx import _lib
    from bgx.engine import R_OVER, R_ROLL0, R_ROLL1
    L, n, G = _lib.load(), 700, 2
    rng = np.random.RandomState(17)
    rec = np.zeros((n, 64), np.uint8)
    rec[:, R_ROLL0], rec[:, R_ROLL1] = rng.randint(1, 7, n), rng.randint(1, 7, n)
    rec[::29, R_OVER] = 1
    who = rng.randint(0, 3, n)
    info = ((rng.randint(-1, 2, n) + 1) << 8) | (rng.randint(1, 4, n) << 16)
    const = dict(rec=dev(rec), sel_a=dev(who == 1, torch.uint8), sel_b=dev(who == 2, torch.uint8),
                 values=dev(rng.uniform(-1.5, 1.5, (n, 21)).astype(F)), done=dev((rng.rand(n) < 0.5).astype(np.uint8)),
                 info=dev(info, torch.int32), games=dev(rng.randint(0, G + 1, n), torch.int32))

    def state():
        return dict(lane_luck=torch.full((n,), 3.0, device="cuda"), fresh=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                    tally=torch.full((8,), 5, dtype=torch.int64, device="cuda"), luck=torch.full((n,), SENT, device="cuda"))

    def chain(t, st):
        c = const
        assert L.bgx_arena_luck_begin(n, ptr(t["lane_luck"]), ptr(t["fresh"]), ptr(t["tally"]), st) == _lib.BGX_OK
        assert L.bgx_arena_luck_add(ptr(c["rec"]), ptr(c["sel_a"]), ptr(c["sel_b"]), ptr(c["values"]), n, ptr(t["lane_luck"]),
                                    ptr(t["fresh"]), ptr(t["luck"]), None, st) == _lib.BGX_OK
        assert L.bgx_arena_luck_flush(ptr(c["sel_a"]), ptr(c["sel_b"]), ptr(c["done"]), ptr(c["info"]), ptr(c["games"]), n, G,
                                      ptr(t["lane_luck"]), ptr(t["fresh"]), ptr(t["tally"]), st) == _lib.BGX_OK

    eager = state()
    chain(eager, None)
    torch.cuda.synchronize()
    t = state()
    before = {k: v.clone() for k, v in t.items()}
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        chain(t, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, v in before.items():                              # the capture ran nothing
        assert torch.equal(t[k], v), k
    g.replay()
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    assert int(t["tally"][4]) > 50 and int(t["tally"][5:].sum()) == 0 and not torch.equal(t["luck"], before["luck"])


# -------------------------------------------------------------------- 2. a traced match --
def test_traced_match_equals_the_host_replay(net, vh):
    """B = 256, G = 2, policy against random, every lane finished.  The luck tally is the host
    replay's integer for integer, every traced luck and mean the twin's on the traced values bit for
    bit, luck_opening is 1 exactly on each game's first step, the plain tally is that of the same
    match without luck=, and a second run gives the same sums."""
    from bgx.arena import (Arena, FIELDS, LUCK_FIELDS, TRACE_LIMIT, PolicyPlayer, RandomPlayer, arena_luck_reference,
                           arena_roll_luck_reference)
    B, G = 256, 2
    steps = TRACE_LIMIT // (B * 21)

    def play(**kw):
        return Arena(B, G, seed=5).play(PolicyPlayer(net, seed=9), RandomPlayer(4), max_steps=steps, **kw)

    res, tr = play(trace=True, luck=vh)
    print("steps", res["steps"], "of", steps, "unfinished", res["unfinished_lanes"])
    assert res["unfinished_lanes"] == 0 and res["games"] == B * G
    trn = {k: v.cpu().numpy() for k, v in tr.items()}
    ref = arena_luck_reference(tr, B, G)
    assert [res[f] for f in LUCK_FIELDS] == ref["luck_tally"][:5].tolist() and res["luck_games"] == res["games"]
    assert not ref["luck_tally"][5:].any() and ref["luck_tally"][2] >= 0
    on = trn["owner"] != 0
    assert same(trn["luck"], ref["luck"]) and same(trn["luck_mean"], ref["mean"])
    assert np.isnan(trn["luck"][~on]).all() and np.isfinite(trn["luck"][on]).all()
    assert np.isnan(trn["luck_values"][~on]).all() and np.isfinite(trn["luck_values"][on]).all()
    # the twin, straight on the traced values
    l, m = arena_roll_luck_reference(trn["luck_values"][on], trn["luck_roll"][on][:, 0], trn["luck_roll"][on][:, 1],
                                     trn["luck_opening"][on])
    assert np.array_equal(bits(l), bits(trn["luck"][on])) and np.array_equal(bits(m), bits(trn["luck_mean"][on]))
    # a game's first step: step 0, and the step after a done, of a lane that is still playing
    first = np.zeros_like(on)
    first[0] = True
    first[1:] = trn["done"][:-1] != 0
    assert np.array_equal(trn["luck_opening"], (first & on).astype(np.uint8))
    assert np.array_equal(trn["luck_opening"], ref["opening"]) and trn["luck_opening"].sum() == B * G
    assert (trn["luck_roll"][trn["luck_opening"] == 1][:, 0] != trn["luck_roll"][trn["luck_opening"] == 1][:, 1]).all()
    # luck= changes nothing else (but the host reads the active count every step: no steps past the end)
    plain = play()
    assert all(res[k] == v for k, v in plain.items() if k != "steps") and res["steps"] <= plain["steps"]
    again = play(luck=vh)
    assert all(again[k] == res[k] for k in FIELDS + LUCK_FIELDS) and again["ppg_luck_a"] == res["ppg_luck_a"]
    # the trace's size counts luck_values' 21 entries
    with pytest.raises(ValueError, match="x 21"):
        Arena(B, G, seed=5).play(RandomPlayer(1), RandomPlayer(2), max_steps=steps + 1, trace=True, luck=vh)


# ---------------------------------------------------------------- 3. the estimate's statistics --
def test_estimate_is_unbiased_and_no_noisier(net, vh):
    """B = 2,048, G = 2, 1-ply against random: the luck's mean is zero within 5 of its standard
    errors, the fitted adjustment does not raise the variance, and the adjusted estimate agrees with
    the raw one of an independently seeded match within 5 combined standard errors."""
    from bgx.arena import Arena, OnePlyPlayer, RandomPlayer
    res = Arena(2048, 2, seed=31).play(OnePlyPlayer(net), RandomPlayer(6), max_steps=4000, luck=vh)
    other = Arena(2048, 2, seed=77).play(OnePlyPlayer(net), RandomPlayer(8), max_steps=4000)
    print({k: res[k] for k in ("steps", "ppg_a", "ppg_stderr", "ppg_luck_a", "ppg_luck_stderr", "variance_ratio",
                               "luck_scale", "luck_mean", "luck_mean_stderr")}, other["ppg_a"], other["ppg_stderr"])
    assert res["unfinished_lanes"] == 0 and other["unfinished_lanes"] == 0 and res["luck_games"] == 4096
    assert abs(res["luck_mean"]) <= 5 * res["luck_mean_stderr"] and res["luck_mean_stderr"] > 0
    assert res["variance_ratio"] <= 1 + 1e-9
    assert abs(res["ppg_luck_a"] - other["ppg_a"]) <= 5 * math.hypot(res["ppg_luck_stderr"], other["ppg_stderr"])


# ------------------------------------------------------------------- 4. the opening rule --
def test_opening_luck_has_mean_zero(net, vh):
    """The luck of the opening rolls, in the mover's view, of a traced B = 2,048, G = 1 match (97
    steps fit the trace; every lane's first step is its opening): its mean is within 5 of its own
    standard errors of 0.  With the mid-game chain substituted on the host, on these same traced
    values, the mean lies far outside (DESIGN.md §19 has the figures)."""
    from bgx.arena import Arena, TRACE_LIMIT, PolicyPlayer, RandomPlayer
    B = 2048
    res, tr = Arena(B, 1, seed=41).play(PolicyPlayer(net, seed=3), RandomPlayer(5), max_steps=TRACE_LIMIT // (B * 21),
                                        trace=True, luck=vh)
    op = tr["luck_opening"].cpu().numpy() == 1
    assert op[0].all() and op.sum() == B
    x = tr["luck"].cpu().numpy()[op].astype(np.float64)
    mean, se = x.mean(), x.std(ddof=1) / math.sqrt(len(x))
    print("opening luck: mean", mean, "stderr", se, "n", len(x))
    assert se > 0 and abs(mean) <= 5 * se


# ----------------------------------------------------------------------- 5. other paths --
def test_luck_with_cube_is_refused(net, vh):
    from bgx.arena import Arena, ArenaCube, ArenaLuck, RandomPlayer
    ar = Arena(64, 1, seed=2)
    for luck in (vh, ArenaLuck(vh, scale=1.0)):
        with pytest.raises(ValueError, match="cube"):
            ar.play(RandomPlayer(1), RandomPlayer(2), max_steps=10, cube=ArenaCube(), luck=luck)
    with pytest.raises(ValueError, match="ArenaLuck"):
        ar.play(RandomPlayer(1), RandomPlayer(2), max_steps=10, luck=net)


def test_search_players_with_luck(net, vh):
    """1-ply against 2-ply top-k 4 at B = 128 for 60 steps, traced: the luck's search shares the
    engine's workspace with the players' and disturbs neither -- the plain trace is that of the
    match without luck=, and the luck tally the replay's."""
    from bgx.arena import Arena, ArenaLuck, LUCK_FIELDS, OnePlyPlayer, TwoPlyPlayer, arena_luck_reference
    B, G = 128, 1

    def play(**kw):
        return Arena(B, G, seed=8).play(OnePlyPlayer(net), TwoPlyPlayer(net, top_k=4), max_steps=60, trace=True, **kw)

    res, tr = play(luck=vh)
    plain, ptr_ = play()
    assert res["steps"] == plain["steps"] <= 60 and all(res[k] == v for k, v in plain.items())
    assert all(torch.equal(tr[k], v) for k, v in ptr_.items())
    ref = arena_luck_reference(tr, B, G)
    assert [res[f] for f in LUCK_FIELDS] == ref["luck_tally"][:5].tolist()
    assert same(tr["luck"].cpu().numpy(), ref["luck"])
    fixed = Arena(B, G, seed=8).play(OnePlyPlayer(net), TwoPlyPlayer(net, top_k=4), max_steps=60,
                                     luck=ArenaLuck(vh, scale=1.0))
    assert fixed["luck_scale"] == 1.0 and [fixed[f] for f in LUCK_FIELDS] == [res[f] for f in LUCK_FIELDS]


def test_arena_command_line_with_luck(net, tmp_path, capsys):
    from bgx import arena
    path = str(tmp_path / "net.pt")
    torch.save(net.state_dict(), path)
    res = arena.main(["--a", path, "--b", "random", "--batch", "256", "--games-per-lane", "1", "--max-steps", "4000",
                      "--seed", "3", "--luck", "--luck-scale", "1.0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert line["games"] == 256 and line["unfinished_lanes"] == 0 and line["luck"] is True and line["luck_net"] is None
    assert line["luck_scale"] == 1.0 and line["luck_games"] == 256
    for k in ("ppg_luck_a", "ppg_luck_stderr", "variance_ratio", "luck_mean", "luck_mean_stderr"):
        assert math.isfinite(line[k]), k
    assert line["ppg_luck_a"] == pytest.approx(line["ppg_a"] - line["luck_mean"], abs=1e-9)


def test_trainer_evaluate_with_luck():
    """tests/test_gpu_arena.py::test_trainer_undisturbed_by_evaluate with luck=True."""
    from bgx.train import PPOTrainer, eval_metrics
    plain, evald = (PPOTrainer(batch=2048, horizon=8, seed=3) for _ in range(2))
    results = []
    for _ in range(2):
        plain.iteration()
        results.append(evald.evaluate("random", batch=256, games_per_lane=1, max_steps=2000, luck=True))
        evald.iteration()
    torch.cuda.synchronize()
    for p, q in zip(plain.net.parameters(), evald.net.parameters()):
        assert torch.equal(p, q)
    assert plain.step_counter == evald.step_counter
    assert all(r["games"] == 256 == r["luck_games"] and r["unfinished_lanes"] == 0 for r in results)
    assert results[0] != results[1]
    m = eval_metrics(results[1])
    assert m["eval_ppg_luck"] == results[1]["ppg_luck_a"] and m["eval_variance_ratio"] == results[1]["variance_ratio"]
    assert m["eval_ppg_luck_stderr"] == results[1]["ppg_luck_stderr"] > 0
    with pytest.raises(ValueError, match="cube"):
        evald.evaluate("random", batch=256, games_per_lane=1, max_steps=10, luck=True, cube=True)
