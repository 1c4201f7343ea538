"""The head-to-head arena (bgx/arena.py, csrc/bg_engine.hip) and the lane-selected
searches under it (bgx_one_ply_sel / bgx_two_ply_sel): selected lanes get bit for bit
what the unselected call gives, unselected lanes are left alone; the right player moves
in every lane and step; the device tally equals a numpy replay of the traced match."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENT_I, SENT_F = -7, -12345.0


def _net(golden, H):
    from bgx.policy import PolicyNet
    mlp = golden("mlp")
    net = PolicyNet(hidden_size=H).cuda()
    pre = f"h{H}_"
    net.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in mlp.items()
                         if k.startswith(pre) and not k.endswith(("logits", "values"))})
    return net


# ------------------------------------------------ 1. lane-selected search --
# B = 48: not a multiple of the wave; B = 1,100: k_scan walks two lanes per thread
@pytest.fixture(scope="module", params=[(40, 48), (128, 48), (40, 1100)], ids=lambda p: f"H{p[0]}-B{p[1]}")
def position(golden, request):
    """An engine 25 random steps in (as tests/test_gpu_search.py::setup builds it) and the
    unselected searches' outputs over sentinel-filled tensors, computed once."""
    import bgx
    from bgx.search import ValueHead, one_ply, two_ply
    H, B = request.param
    net = _net(golden, H)
    eng = bgx.Engine(batch=B, max_moves=500, dice="mt", auto_reset=True)
    eng.seed(np.arange(500, 500 + B, dtype=np.uint32))
    eng.reset()
    rng = np.random.RandomState(2)
    for _ in range(25):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    vh = ValueHead(net)
    ref1 = one_ply(eng, vh, out=_sentinels(eng))
    ref2 = two_ply(eng, vh, out=_sentinels(eng))
    rec = eng.records().cpu().numpy()
    n = rec[:, 60].astype(np.int64) | (rec[:, 61].astype(np.int64) << 8)
    assert ref2[3]["afterstates"] == int(n.sum()) and eng.error() == 0
    return eng, vh, ref1, ref2, rec[:, 52].copy(), n


def _sentinels(eng):
    kw = dict(device=eng.device)
    return (torch.full((eng.batch,), SENT_I, dtype=torch.int32, **kw),
            torch.full((eng.batch,), SENT_F, dtype=torch.float32, **kw),
            torch.full((eng.batch, eng.max_moves), SENT_F, dtype=torch.float32, **kw))


SELECTIONS = ["ones", "zeros", "alternating", "last", "player2", "random_half"]


def _selection(name, mover):
    B = len(mover)
    if name == "ones":
        return np.ones(B, np.uint8)
    if name == "zeros":
        return np.zeros(B, np.uint8)
    if name == "alternating":
        return (np.arange(B) & 1).astype(np.uint8)
    if name == "last":
        s = np.zeros(B, np.uint8)
        s[-1] = 1
        return s
    if name == "player2":          # the by-mover scan's first group (PLAYER1's rows) is empty
        return (mover == 1).astype(np.uint8)
    return (np.random.RandomState(11).rand(B) < 0.5).astype(np.uint8)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check_selected(got, ref, sel):
    """best, best value and the value rows: selected lanes bitwise equal to the unselected
    call, unselected lanes still the sentinel."""
    s = torch.from_numpy(sel.astype(bool)).cuda()
    for g, r, sent in zip(got[:3], ref[:3], (SENT_I, SENT_F, SENT_F)):
        assert torch.equal(_bits(g)[s], _bits(r)[s])
        assert bool((g[~s] == sent).all())


@pytest.mark.parametrize("name", SELECTIONS)
def test_one_ply_sel(position, name):
    from bgx.search import one_ply
    eng, vh, ref1, _, mover, n = position
    sel = _selection(name, mover)
    got = one_ply(eng, vh, sel=torch.from_numpy(sel).cuda(), out=_sentinels(eng))
    _check_selected(got, ref1, sel)
    assert eng.error() == 0


@pytest.mark.parametrize("name", SELECTIONS)
def test_two_ply_sel(position, name):
    from bgx.search import two_ply
    eng, vh, _, ref2, mover, n = position
    sel = _selection(name, mover)
    got = two_ply(eng, vh, sel=torch.from_numpy(sel).cuda(), out=_sentinels(eng))
    _check_selected(got, ref2, sel)
    rows = int(n[sel != 0].sum())
    assert got[3]["afterstates"] == rows and got[3]["jobs"] == 21 * rows
    if name == "ones":
        assert got[3] == ref2[3]
    if name == "zeros":
        assert got[3] == {"leaves": 0, "jobs": 0, "afterstates": 0}
    assert 0 < got[3]["leaves"] <= ref2[3]["leaves"] or rows == 0
    assert eng.error() == 0


def test_sel_argument_checked(position):
    from bgx.search import one_ply, two_ply
    eng, vh = position[0], position[1]
    for bad in (torch.ones(eng.batch, dtype=torch.int32, device=eng.device),
                torch.ones(eng.batch + 1, dtype=torch.uint8, device=eng.device),
                torch.ones(eng.batch, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            one_ply(eng, vh, sel=bad)
        with pytest.raises(ValueError):
            two_ply(eng, vh, sel=bad)


# ------------------------------------------------------- 2-4. the arena --
class First:
    """Scripted player: always action 0."""
    sync_free = True

    def act(self, eng, sel, step):
        return torch.zeros(eng.batch, dtype=torch.int32, device=eng.device)


class Last:
    """Scripted player: always the last legal action, n_moves - 1 (-1 on a pass, where
    the engine reads no action)."""
    sync_free = True

    def act(self, eng, sel, step):
        return eng.n_moves().to(torch.int32) - 1


def replay(tr, B, G):
    """The tally (16 entries) and the owners [steps, B] recomputed from a trace in numpy."""
    tr = {k: v.cpu().numpy().astype(np.int64) for k, v in tr.items()}
    steps = tr["done"].shape[0]
    lanes = np.arange(B)
    gd = np.zeros(B, np.int64)
    t = np.zeros(16, np.int64)
    owner = np.zeros((steps, B), np.int64)
    for s in range(steps):
        active = gd < G
        a_p1 = ((lanes + gd) & 1) == 0
        a_moves = (tr["mover"][s] == 0) == a_p1
        owner[s] = np.where(active, np.where(a_moves, 1, 2), 0)
        info = tr["info"][s]
        imover, winner, score, kind = info & 0xFF, ((info >> 8) & 0xFF) - 1, (info >> 16) & 0xFF, (info >> 24) & 0xFF
        assert np.array_equal(imover, tr["mover"][s])
        done = tr["done"][s] != 0
        # auto_reset engine: a done is always a win by the mover of that step
        assert np.array_equal(winner[done], imover[done]) and (kind[done] == 0).all() and (winner[~done] == -1).all()
        assert ((score[done] >= 1) & (score[done] <= 3)).all()
        fin = active & done
        a_won, b_won = fin & ((winner == 0) == a_p1), fin & ((winner == 0) != a_p1)
        t[0] += fin.sum()
        t[1] += a_won.sum()
        t[2] += b_won.sum()
        t[3] += score[a_won].sum()
        t[4] += score[b_won].sum()
        t[5] += (score[a_won] == 2).sum()
        t[6] += (score[b_won] == 2).sum()
        t[7] += (score[a_won] == 3).sum()
        t[8] += (score[b_won] == 3).sum()
        t[9] += (fin & a_p1).sum()
        t[10] += (a_won & a_p1).sum()
        t[11] += (fin & (winner == 0)).sum()
        t[12] += active.sum()
        gd += fin
    t[13] = (gd < G).sum()
    return t, owner, tr


def _tally_of(res):
    from bgx.arena import FIELDS
    return np.array([res[k] for k in FIELDS] + [0, 0], np.int64)


@pytest.fixture(scope="module")
def scripted_match():
    from bgx.arena import Arena
    B, G = 64, 2
    ar = Arena(B, G, seed=5)
    res, tr = ar.play(First(), Last(), max_steps=4000, trace=True)
    assert torch.equal(ar.tally.cpu(), torch.from_numpy(_tally_of(res)))      # entries 14, 15 are zero
    return B, G, res, tr


def test_right_player_moves(scripted_match):
    B, G, res, tr = scripted_match
    _, owner, t = replay(tr, B, G)
    assert res["steps"] == t["done"].shape[0] > 0
    assert np.array_equal(t["owner"], owner)                 # the seat rule and the mover
    assert (owner[0] != 0).all() and (owner == 1).any() and (owner == 2).any()
    want = np.where(owner == 2, t["n_moves"] - 1, 0)         # A plays 0, B plays n - 1, nobody: 0
    assert np.array_equal(t["action"], want)
    # owner 0 exactly from the step after the lane's G-th done onwards
    done_before = np.cumsum(t["done"], axis=0) - t["done"]
    assert np.array_equal(owner == 0, done_before >= G)


def test_tally_equals_replay(scripted_match):
    B, G, res, tr = scripted_match
    t, _, _ = replay(tr, B, G)
    got = _tally_of(res)
    assert np.array_equal(got, t), (got, t)
    assert res["unfinished_lanes"] == t[13]
    if res["unfinished_lanes"] == 0:
        assert res["games"] == B * G
        assert res["games_a_p1"] * 2 == res["games"]
    assert res["wins_a"] + res["wins_b"] == res["games"] > 0
    for x in "ab":
        singles = res[f"wins_{x}"] - res[f"gammons_{x}"] - res[f"backgammons_{x}"]
        assert singles >= 0
        assert res[f"points_{x}"] == singles + 2 * res[f"gammons_{x}"] + 3 * res[f"backgammons_{x}"]


def test_step_cap():
    from bgx.arena import Arena
    B, G = 64, 2
    res, tr = Arena(B, G, seed=5).play(First(), Last(), max_steps=40, trace=True)
    assert res["steps"] == 40 and res["unfinished_lanes"] > 0
    t, _, _ = replay(tr, B, G)
    assert tr["done"].shape[0] == 40 and np.array_equal(_tally_of(res), t)
    assert res["plies"] == 40 * B or res["games"] > 0


def test_trace_refused_when_large():
    from bgx.arena import Arena, RandomPlayer, TRACE_LIMIT
    ar = Arena(4096, 1, seed=1)
    with pytest.raises(ValueError):
        ar.play(RandomPlayer(1), RandomPlayer(2), max_steps=TRACE_LIMIT // 4096 + 1, trace=True)


# ----------------------------------------------------- 5. seat symmetry --
def test_seat_symmetry_random_vs_random():
    """Two uniformly random players are equally strong: over B x G = 4,096 games A's wins
    stay within 4.5 sigma = 144 of 2,048 (false-alarm rate 7e-6; the seeds are fixed).
    The step cap is a condition of the test: random games end within a few hundred steps."""
    from bgx.arena import Arena, RandomPlayer
    res = Arena(2048, 2, seed=17).play(RandomPlayer(101), RandomPlayer(202), max_steps=4000)
    assert res["unfinished_lanes"] == 0 and res["games"] == 4096
    assert res["games_a_p1"] == 2048
    assert abs(res["wins_a"] - 2048) <= 144, res


# ------------------------------------------------------ 6. reproducible --
def test_reproducible(golden):
    from bgx.arena import Arena, FIELDS, PolicyPlayer, RandomPlayer
    net = _net(golden, 128)
    runs = [Arena(256, 1, seed=s).play(PolicyPlayer(net, seed=9), RandomPlayer(4), max_steps=4000)
            for s in (3, 3, 4)]
    assert runs[0] == runs[1]
    assert runs[0]["games"] == 256 and runs[0]["unfinished_lanes"] == 0
    assert [runs[0][k] for k in FIELDS] != [runs[2][k] for k in FIELDS]


# --------------------------------------------- 7. search players, a match --
def test_search_players_match(golden):
    """2-ply against 1-ply: each searches only the lanes it is on move in (the 2-ply
    calls' afterstates are those of A's lanes); untrained greedy players may shuffle, so
    the match runs into its step cap."""
    from bgx.arena import Arena, OnePlyPlayer, TwoPlyPlayer
    net = _net(golden, 40)
    B, G = 64, 1
    a, b = TwoPlyPlayer(net), OnePlyPlayer(net)
    ar = Arena(B, G, seed=8)
    res, tr = ar.play(a, b, max_steps=60, trace=True)
    t, owner, trn = replay(tr, B, G)
    assert np.array_equal(_tally_of(res), t)
    assert np.array_equal(trn["owner"], owner)
    assert a.totals["calls"] == res["steps"]
    assert a.totals["afterstates"] == int(trn["n_moves"][owner == 1].sum()) > 0
    assert a.totals["jobs"] == 21 * a.totals["afterstates"]
    assert ((trn["action"] >= 0) & ((trn["action"] < trn["n_moves"]) | (trn["n_moves"] == 0))).all()
    assert ar.eng.error() == 0


# ------------------------------------------------ 8. trainer undisturbed --
def test_trainer_undisturbed_by_evaluate():
    from bgx.train import PPOTrainer
    plain, evald = (PPOTrainer(batch=2048, horizon=8, seed=3) for _ in range(2))
    results = []
    for _ in range(2):
        plain.iteration()
        results.append(evald.evaluate("random", batch=256, games_per_lane=1, max_steps=2000))
        evald.iteration()
    torch.cuda.synchronize()
    for p, q in zip(plain.net.parameters(), evald.net.parameters()):
        assert torch.equal(p, q)
    assert plain.step_counter == evald.step_counter
    assert all(r["games"] == 256 and r["unfinished_lanes"] == 0 for r in results)
    assert results[0] != results[1]                       # each evaluation has seeds of its own


def test_evaluate_against_a_checkpoint(tmp_path):
    """The opponent as a saved state_dict, both sides searching 1-ply; building the
    opponent's net draws nothing from torch's global generator."""
    from bgx.train import PPOTrainer
    tr = PPOTrainer(batch=2048, horizon=8, seed=3)
    path = str(tmp_path / "net.pt")
    tr.save(path)
    before = torch.random.get_rng_state()
    counter, packed = tr.step_counter, getattr(tr.net, "_packed", None)
    res = tr.evaluate(path, player="1ply", opponent_player="greedy", batch=128, games_per_lane=1, max_steps=50)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert tr.step_counter == counter and getattr(tr.net, "_packed", None) is packed
    assert res["steps"] <= 50 and res["plies"] > 0 and res["games"] + res["unfinished_lanes"] == 128
    assert res["wins_a"] + res["wins_b"] == res["games"]


# --------------------------------------------------------- command lines --
def test_arena_command_line(capsys):
    import json
    from bgx import arena
    res = arena.main(["--a", "random", "--b", "random", "--batch", "512", "--games-per-lane", "1", "--max-steps",
                      "2000", "--seed", "3"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert line["games"] == 512 and line["unfinished_lanes"] == 0 and line["player_a"] == "random"
    assert line["win_rate_a"] == line["wins_a"] / 512 and line["games_per_s"] > 0


def test_train_command_line_evaluates(tmp_path, monkeypatch):
    import json
    import sys
    from bgx import train
    metrics = tmp_path / "m.jsonl"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.setattr(sys, "argv", ["bgx.train", "--batch", "2048", "--horizon", "8", "--updates", "2",
                                      "--eval-every", "2", "--eval-games", "1", "--eval-batch", "256", "--metrics",
                                      str(metrics)])
    train.main()
    lines = [json.loads(l) for l in metrics.read_text().splitlines()]
    assert len(lines) == 2 and "eval_win_rate" not in lines[0]
    assert lines[1]["eval_games"] == 256 and lines[1]["eval_unfinished"] == 0
    assert 0.0 <= lines[1]["eval_win_rate"] <= 1.0 and -3.0 <= lines[1]["eval_ppg"] <= 3.0
