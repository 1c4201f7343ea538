"""The env step's apply on the lanes (apply_move_bytes), the root child
lists with one per-lane gen (Gen::nd_both) and the Philox-only instantiations of the split
launch: every golden move applied, pass / invalid / over lanes against the oracle Env, the
root lists of the bar-entry and bear-off rules, and the dispatch order against the generic
kernel."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

CUR, ROLL0, ROLL1, OVER, MATCH, S0 = 52, 53, 54, 55, 56, 57
MAX_MOVES = 500
ENGINE_LANES = 8192


@pytest.fixture(scope="module")
def bgx():
    import bgx as _bgx
    assert torch.cuda.is_available()
    return _bgx


def n_moves_of(rec):
    return rec[:, 60].astype(int) | (rec[:, 61].astype(int) << 8)


def win_of(after, pl):
    """(score, reward) of a board after `pl` moved by the reference's rules
    (backgammon_env.py:156-182): 0 = no win, 1 single, 2 gammon, 3 backgammon."""
    if after[50 + pl] != 15:
        return 0, 0.0
    opp = 1 - pl
    if after[50 + opp] > 0:
        return 1, 1.0
    home = range(18, 24) if pl == 0 else range(6)          # the winner's home board
    if after[48 + opp] > 0 or any(after[opp * 24 + q] > 0 for q in home):
        return 3, 2.0
    return 2, 1.5


@pytest.fixture(scope="module")
def pairs(golden):
    """Every (position, action) pair of the golden move lists' first min(count, 500) moves
    with the oracle's afterstate, the reference rules' outcome and the categories of the
    move, computed once from the decoded golden moves."""
    g = golden("movegen")
    offs = g["offsets"]
    pos, act = [], []
    for i in range(len(g["counts"])):
        k = min(int(g["counts"][i]), MAX_MOVES)
        pos += [i] * k
        act += list(range(k))
    pos, act = np.array(pos), np.array(act, np.int32)
    move = g["moves"][offs[pos] + act]
    n = len(pos)
    after = np.zeros((n, 52), np.int8)
    score = np.zeros(n, int)
    reward = np.zeros(n, np.float32)
    cat = dict.fromkeys(["bar entry", "bear off", "hit", "hit twice", "two on one point", "one checker on",
                         "length 1", "length 4", "player1", "player2", "single", "gammon", "backgammon"], 0)
    for j in range(n):
        b, pl = g["boards"][pos[j]], int(g["players"][pos[j]])
        after[j] = O.apply_move(b, pl, int(move[j]))
        score[j], reward[j] = win_of(after[j], pl)
        subs = O.decode_move(int(move[j]))
        dsts = [d for _, d, _ in subs if d != 25]
        hits = sum(h for _, _, h in subs)
        cat["bar entry"] += any(s == 24 for s, _, _ in subs)
        cat["bear off"] += any(d == 25 for _, d, _ in subs)
        cat["hit"] += hits >= 1
        cat["hit twice"] += hits >= 2
        cat["two on one point"] += len(dsts) != len(set(dsts))
        cat["one checker on"] += any(subs[k][0] == subs[k - 1][1] for k in range(1, len(subs)))
        cat["length 1"] += len(subs) == 1
        cat["length 4"] += len(subs) == 4
        cat["player1" if pl == 0 else "player2"] += 1
        if score[j]:
            cat[["single", "gammon", "backgammon"][score[j] - 1]] += 1
    rec = np.zeros((n, 64), np.uint8)
    rec[:, :52] = g["boards"][pos].view(np.uint8)
    rec[:, CUR] = g["players"][pos]
    rec[:, ROLL0:ROLL1 + 1] = g["rolls"][pos]
    return dict(n=n, pos=pos, act=act, move=move, after=after, score=score, reward=reward, cat=cat, rec=rec,
                player=g["players"][pos].astype(int), count=np.minimum(g["counts"][pos], MAX_MOVES))


def test_golden_pairs_cover_every_category(pairs):
    """The golden set has 42,376 pairs; on the CPU: 1,705 enter from the bar, 2,811 bear
    off, 14,697 hit (5,357 twice or more), 9,432 land two checkers on one point, 12,220 move
    one checker on, 169 of length 1 and 18,103 of length 4, 22,081 / 20,295 per player,
    140 wins (33 single, 103 gammon, 4 backgammon).  None may be empty."""
    print(pairs["n"], pairs["cat"])
    assert pairs["n"] > 40000
    for name, k in pairs["cat"].items():
        assert k > 0, name


def _step_pairs(bgx, pairs, sel, dice):
    """One lane per pair of `sel` in one engine: records from the positions (set_lanes
    regenerates the lists), one step, auto-reset off so winners keep their final board."""
    n = len(sel)
    eng = bgx.Engine(batch=n, max_moves=MAX_MOVES, dice=dice, seed=5, auto_reset=False)
    if dice != "philox":
        eng.seed(np.full(n, 777, np.uint32) if dice == "shared" else np.arange(n, dtype=np.uint32))
    eng.reset(want_obs=False)
    eng.set_lanes(torch.from_numpy(pairs["rec"][sel]))
    rec0, mv0, _ = eng.lanes()
    act = torch.from_numpy(pairs["act"][sel]).cuda()
    own = eng.afterstates()[torch.arange(n, device="cuda"), act.long()].cpu().numpy()
    _, rew, done, info = eng.step(act, want_obs=False, want_info=True)
    rew, done, info = rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy()
    rec = eng.records().cpu().numpy()
    assert eng.error() == 0
    rec0, mv0 = rec0.cpu().numpy(), mv0.cpu().numpy().view(np.uint64)
    # the lists the step chose from are the golden ones
    assert np.array_equal(n_moves_of(rec0), pairs["count"][sel])
    assert np.array_equal(mv0[np.arange(n), pairs["act"][sel]], pairs["move"][sel])
    want, pl, score = pairs["after"][sel], pairs["player"][sel], pairs["score"][sel]
    win = score > 0
    bad = np.where((rec[:, :52].view(np.int8) != want).any(1))[0]
    assert len(bad) == 0, (len(bad), int(sel[bad[0]]), hex(int(pairs["move"][sel[bad[0]]])))
    assert np.array_equal(own, want)
    assert np.array_equal(rec[:, CUR], np.where(win, pl, 1 - pl))
    assert np.array_equal(rec[:, OVER], win.astype(np.uint8))
    assert np.array_equal(rew, pairs["reward"][sel])
    assert np.array_equal(done, win.astype(np.uint8))
    assert np.array_equal(info, pl | (np.where(win, pl + 1, 0) << 8) | (score << 16))    # kind 0: a move
    return int(win.sum())


def test_every_golden_move_applied(bgx, pairs):
    """Bytes 0..51 of each lane's record after one step equal oracle.apply_move and the
    engine's own afterstates row taken before the step; mover, game-over flag, reward,
    done and the info word are the reference rules' for that board.  Philox engines of at
    most 8,192 lanes: the split launch's two Philox-only kernels."""
    wins = 0
    for lo in range(0, pairs["n"], ENGINE_LANES):
        wins += _step_pairs(bgx, pairs, np.arange(lo, min(lo + ENGINE_LANES, pairs["n"])), "philox")
    assert wins == int((pairs["score"] > 0).sum()) > 0


@pytest.mark.parametrize("dice", ["mt", "shared"])
def test_golden_moves_applied_generic_kernels(bgx, pairs, dice):
    """The same on a 512-pair slice (every 85th pair plus the first two wins of each kind)
    with per-lane MT19937 dice (the generic fused kernel) and shared dice (the apply-only and
    advance-only kernels)."""
    sel = np.arange(0, pairs["n"], pairs["n"] // 500 + 1)
    for k in (1, 2, 3):
        sel = np.union1d(sel, np.where(pairs["score"] == k)[0][:2])
    sel = sel[:512]
    assert 500 <= len(sel) <= 512
    assert _step_pairs(bgx, pairs, sel, dice) >= 1


def test_pass_invalid_and_over_lanes_vs_oracle_env(bgx):
    """64 lanes of random play against oracle Envs of the same seeds (per-lane MT19937,
    auto-reset off, matches to 3 points): lanes without a legal move pass, every ninth
    (step + lane) gets one of the actions -1, n, n + 7, -max_moves - 1, and a lane whose
    game is over resets on its next step.  Records, rewards, dones and info words are equal
    after every step.  On the oracle alone these 400 steps hold 1,145 passes, 217 steps of
    finished games and about 710 of each bad action."""
    B, T = 64, 400
    seeds = np.arange(5000, 5000 + B, dtype=np.uint32)
    eng = bgx.Engine(batch=B, max_moves=MAX_MOVES, dice="mt", auto_reset=False, match_length=3)
    eng.seed(seeds)
    envs = [O.Env(seed=int(s), match_length=3) for s in seeds]
    eng.reset(want_obs=False)
    for e in envs:
        e.reset()
    rng = np.random.RandomState(11)
    kinds, bad_given = np.zeros(4, int), np.zeros(4, int)
    for step in range(T):
        acts = np.zeros(B, np.int32)
        for i, e in enumerate(envs):
            nl = int(e.state()[1][3])
            acts[i] = rng.randint(nl) if nl else 0
            if (step + i) % 9 == 0:
                k = ((step + i) // 9) % 4
                acts[i] = [-1, nl, nl + 7, -MAX_MOVES - 1][k]
                bad_given[k] += 1
        _, rew, done, info = eng.step(torch.from_numpy(acts).cuda(), want_obs=False, want_info=True)
        rew, done, info = rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy()
        rec = eng.records().cpu().numpy()
        for i, e in enumerate(envs):
            _, r, d, inf = e.step(int(acts[i]))
            kinds[inf[3]] += 1
            assert (rew[i], bool(done[i])) == (r, d), (step, i)
            assert info[i] == inf[0] | ((inf[1] + 1) << 8) | (inf[2] << 16) | (inf[3] << 24), (step, i)
            b, st = e.state()
            assert np.array_equal(rec[i, :52].view(np.int8), b), (step, i)
            got = [rec[i, CUR], rec[i, ROLL0], rec[i, ROLL1], n_moves_of(rec[i:i + 1])[0], rec[i, OVER], rec[i, MATCH],
                   rec[i, S0], rec[i, S0 + 1]]
            assert got == [st[0], st[1], st[2], st[3], st[5], st[6], st[7], st[8]], (step, i)
    print(kinds, bad_given)
    assert kinds.min() > 0 and bad_given.min() > 0      # moves, passes, invalid actions, finished games
    assert eng.error() == 0


def test_root_child_lists_of_bar_and_bearoff_rules(bgx, golden):
    """The ordered lists of the golden set's 2,160 non-doubles positions (the walk whose
    root lists come from one per-lane gen) equal the golden ones, and those positions
    include, for both players: the mover on the bar with exactly one die's entry point
    blocked, a bear-off by the farthest-checker rule (a die above the farthest checker's
    distance) and a bear-off from the die's exact point.  The golden set alone has all of
    them (106, 241 and 654 positions), so no random boards are added."""
    g = golden("movegen")
    nd = np.where(g["rolls"][:, 0] != g["rolls"][:, 1])[0]
    props = {"bar, one entry blocked": [0, 0], "bear-off, farthest checker": [0, 0], "bear-off, exact point": [0, 0]}
    for i in nd:
        b, pl, roll = g["boards"][i].astype(int), int(g["players"][i]), [int(x) for x in g["rolls"][i]]
        own, opp = b[pl * 24:pl * 24 + 24], b[(1 - pl) * 24:(1 - pl) * 24 + 24]
        if b[48 + pl] > 0:
            blocked = [opp[d - 1 if pl == 0 else 24 - d] >= 2 for d in roll]
            props["bar, one entry blocked"][pl] += sum(blocked) == 1
            continue
        home = list(range(18, 24)) if pl == 0 else list(range(6))
        if own[home].sum() + b[50 + pl] == 15 and b[50 + pl] < 15:
            dist = [24 - q if pl == 0 else q + 1 for q in range(24) if own[q] > 0]
            props["bear-off, farthest checker"][pl] += any(d > max(dist) for d in roll)
            props["bear-off, exact point"][pl] += any(d in dist for d in roll)
    print(len(nd), props)
    assert len(nd) > 2000
    for name, per_player in props.items():
        assert min(per_player) > 0, name
    cap = 2048
    eng = bgx.Engine(batch=len(nd), max_moves=cap, dice="philox")
    nm, nt, mv = eng.movegen(torch.from_numpy(g["boards"][nd]), torch.from_numpy(g["players"][nd]),
                             torch.from_numpy(g["rolls"][nd]), max_moves=cap)
    nm, nt, mv = nm.cpu().numpy(), nt.cpu().numpy(), mv.cpu().numpy().view(np.uint64)
    assert np.array_equal(nt, g["counts"][nd]) and np.array_equal(nm, np.minimum(g["counts"][nd], cap))
    offs = g["offsets"]
    for k, i in enumerate(nd):
        assert np.array_equal(mv[k, :nm[k]], g["moves"][offs[i]:offs[i] + nm[k]]), i
    assert eng.error() == 0


@pytest.mark.parametrize("B", [256, 1024])
def test_order_on_and_off_give_equal_records(bgx, dbg, B):
    """The heavy and light Philox-only kernels of the split launch (dispatch order on)
    against the generic kernel (BGX_ORDER 0: one launch, run-time dice mode): equal
    records, rewards, dones and live move lists after each of 64 steps of random legal
    actions.  The even lanes start two checkers from the end, so games end and reset
    (to the opening) on the way; B = 256 is the plain order's smallest split with a light
    launch, 1,024 the XCD-aware one's."""
    dbg.delenv("BGX_ORDER", raising=False)
    eo = bgx.Engine(batch=B, max_moves=MAX_MOVES, dice="philox", seed=44, auto_reset=True)
    dbg.setenv("BGX_ORDER", "0")
    en = bgx.Engine(batch=B, max_moves=MAX_MOVES, dice="philox", seed=44, auto_reset=True)
    dbg.delenv("BGX_ORDER", raising=False)
    start = np.zeros((B // 2, 64), np.uint8)
    i = np.arange(B // 2)
    start[:, 23], start[:, 24], start[:, 50:52] = 2, 2, 13
    start[:, CUR], start[:, ROLL0], start[:, ROLL1] = i % 2, 1 + i % 6, 1 + (i // 6) % 6
    for e in (eo, en):
        e.reset(want_obs=False)
    rec = eo.records()                                   # openings on the odd lanes
    rec[::2] = torch.from_numpy(start).cuda()
    for e in (eo, en):
        e.set_lanes(rec)
    g = torch.Generator(device="cuda").manual_seed(6)
    idx = torch.arange(MAX_MOVES, device="cuda")[None, :]
    dones = 0
    for step in range(64):
        u = torch.rand(B, device="cuda", generator=g)
        _, ro, do, io = eo.step((u * eo.n_moves().clamp(min=1).float()).to(torch.int32), want_obs=False)
        _, rn, dn, i_n = en.step((u * en.n_moves().clamp(min=1).float()).to(torch.int32), want_obs=False)
        assert torch.equal(ro, rn) and torch.equal(do, dn) and torch.equal(io, i_n), step
        dones += int(do.sum())
        rec_o, mv_o, nt_o = eo.lanes()
        rec_n, mv_n, nt_n = en.lanes()
        assert torch.equal(rec_o, rec_n) and torch.equal(nt_o, nt_n), step
        live = idx < (rec_n[:, 60].long() | (rec_n[:, 61].long() << 8))[:, None]     # entries past n are scratch
        assert torch.equal(torch.where(live, mv_o, 0), torch.where(live, mv_n, 0)), step
    assert dones >= B // 2
    assert eo.error() == 0 and en.error() == 0
    perm, _, _ = eo.order()
    assert np.array_equal(np.sort(perm), np.arange(B))          # the ordered engine did run the split launch
