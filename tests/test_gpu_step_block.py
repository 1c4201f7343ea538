"""The step blocks (k_step_gather): the order's second pass runs at the start
of the next step and lays each lane's index, action, chosen move and counter at its dispatch
position; the split launch's waves start from that block.  Every comparison is against
an engine built with BGX_ORDER 0, which has no order and no blocks and keeps the chained
loads: same seed, same calls, same actions.

Sizes: 64 = one count block, plain order; 128 = XCD-aware order, heavy grid 72, so both
launches run; 200 = padding lanes in the pass; 1,152 = several blocks, XCD-aware."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [64, 128, 200, 1152]
M = 500                                      # max_moves
CUR, ROLL0, ROLL1, OVER = 52, 53, 54, 55
MASK48 = np.uint64((1 << 48) - 1)


@pytest.fixture(scope="module")
def bgx():
    import bgx as _bgx
    assert torch.cuda.is_available()
    return _bgx


def make_pair(bgx, dbg, B, seed, auto_reset=True):
    """(engine with the order and the step blocks, engine with BGX_ORDER 0)."""
    dbg.delenv("BGX_ORDER", raising=False)
    eo = bgx.Engine(batch=B, max_moves=M, dice="philox", seed=seed, auto_reset=auto_reset)
    dbg.setenv("BGX_ORDER", "0")
    en = bgx.Engine(batch=B, max_moves=M, dice="philox", seed=seed, auto_reset=auto_reset)
    dbg.delenv("BGX_ORDER", raising=False)
    with pytest.raises(Exception):
        en.order()                           # no order: the old path
    return eo, en


def bearoff_records(B, left=15):
    """Both sides' last `left` checkers on their own ace points (player 0: point 23, player
    1: point 0), the rest borne off: every roll bears off at least two checkers."""
    rec = np.zeros((B, 64), np.uint8)
    rec[:, 23] = left
    rec[:, 24 + 0] = left
    rec[:, 50:52] = 15 - left
    i = np.arange(B)
    rec[:, CUR] = i % 2
    rec[:, ROLL0] = 1 + i % 6
    rec[:, ROLL1] = 1 + (i // 6) % 6
    return torch.from_numpy(rec).cuda()


def pass_records(n):
    """Player 0 on roll with a checker on the bar against a closed board (player 1 holds
    points 0..5, where player 0 enters): no legal move whatever the roll."""
    rec = np.zeros((n, 64), np.uint8)
    rec[:, 23] = 14
    rec[:, 48] = 1
    rec[:, 24:30] = 2
    rec[:, 24 + 6] = 3
    i = np.arange(n)
    rec[:, CUR] = 0
    rec[:, ROLL0] = 1 + i % 6
    rec[:, ROLL1] = 1 + (i // 6) % 6
    return torch.from_numpy(rec).cuda()


def legal_actions(e, u):
    return (u * e.n_moves().clamp(min=1).float()).to(torch.int32)


def counters(e):
    """The Philox draw counters (low 48 bits; the cache bits belong to the order)."""
    from bgx._lib import check
    ctr = np.empty(e.batch, np.uint64)
    check(e._lib.bgx_engine_order(e._h, None, None, ctr.ctypes.data_as(ctypes.c_void_p), e._stream()),
          "bgx_engine_order")
    return ctr & MASK48


def assert_same_state(eo, en, tag):
    rec_o, mv_o, nt_o = eo.lanes()
    rec_n, mv_n, nt_n = en.lanes()
    assert torch.equal(rec_o, rec_n), tag
    assert torch.equal(nt_o, nt_n), tag
    idx = torch.arange(M, device="cuda")[None, :]
    live = idx < (rec_n[:, 60].long() | (rec_n[:, 61].long() << 8))[:, None]      # entries past n are scratch
    assert torch.equal(torch.where(live, mv_o, 0), torch.where(live, mv_n, 0)), tag
    assert np.array_equal(counters(eo), counters(en)), tag
    assert eo.error() == 0 and en.error() == 0, tag


def step_both(eo, en, ao, an=None, tag=None):
    """One step of both engines; rewards, dones and info words equal.  Returns them."""
    _, ro, do, io = eo.step(ao, want_obs=False)
    _, rn, dn, inn = en.step(ao if an is None else an, want_obs=False)
    assert torch.equal(ro, rn), tag
    assert torch.equal(do, dn), tag
    assert torch.equal(io, inn), tag
    return rn.clone(), dn.clone(), inn.clone()


def midgame(eo, en, g, steps):
    B = eo.batch
    for e in (eo, en):
        e.reset(want_obs=False)
    for t in range(steps):
        u = torch.rand(B, device="cuda", generator=g)
        step_both(eo, en, legal_actions(en, u), tag=("midgame", t))


def check_order(B, perm, cls):
    assert np.array_equal(np.sort(perm), np.arange(B))
    assert cls.max() <= 4
    if B % 128 == 0:                         # XCD-aware: 8 interleaved class-sorted sub-lists
        for x in range(8):
            assert (np.diff(cls[perm[x::8]].astype(int)) >= 0).all(), x
    else:
        assert (np.diff(cls[perm].astype(int)) >= 0).all()


@pytest.mark.parametrize("B", SIZES)
def test_action_edge_cases_through_the_block(bgx, dbg, B):
    """One step from a mid-game population with legal, negative, invalid and extreme actions,
    on playing, passing and finished lanes (auto-reset off): everything the step leaves equals
    the old path's, an invalid action costs -1 and changes nothing, and a second step equals
    as well (nothing stale is left in the blocks)."""
    import oracle as O
    eo, en = make_pair(bgx, dbg, B, 41, auto_reset=False)
    g = torch.Generator(device="cuda").manual_seed(3)
    midgame(eo, en, g, 12)
    # lanes 16..31: two checkers left per side -> their movers win in the next step and the
    # games stay finished; then lanes 0..15: no legal move
    fin = bearoff_records(16, left=2)
    for e in (eo, en):
        e.set_lanes(fin, lane0=16)
    step_both(eo, en, legal_actions(en, torch.rand(B, device="cuda", generator=g)), tag="finish")
    for e in (eo, en):
        e.set_lanes(pass_records(16), lane0=0)
    rec0, mv0, _ = en.lanes()
    rec0, mv0 = rec0.cpu().numpy(), mv0.cpu().numpy()
    n = (rec0[:, 60].astype(np.int64) | (rec0[:, 61].astype(np.int64) << 8))
    over = rec0[:, OVER] != 0
    assert (n[:16] == 0).all() and not over[:16].any()
    assert over[16:32].all()
    i = np.arange(B)
    kind = i % 10
    u = torch.rand(B, device="cuda", generator=g).cpu().numpy()
    legal = np.minimum((u * np.maximum(n, 1)).astype(np.int64), np.maximum(n, 1) - 1)
    a = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7,
                   kind == 8, kind == 9],
                  [legal, legal - M, np.full(B, -1), n, n + 1, np.full(B, M), np.full(B, M + 7),
                   np.full(B, 2**31 - 1), np.full(B, -2**31), np.full(B, -M - 1)]).astype(np.int64)
    acts = torch.from_numpy(a.astype(np.int32)).cuda()
    rew, done, info = step_both(eo, en, acts, tag="edge")
    assert_same_state(eo, en, "edge")
    rew, done, info = rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy()
    rec1 = en.records().cpu().numpy()
    eff = np.where(a < 0, a + M, a)
    play = ~over & (n > 0)
    invalid = play & ((eff < 0) | (eff >= n))
    valid = play & ~invalid
    assert invalid.sum() >= B // 4 and valid.sum() >= B // 16
    assert (kind[valid] <= 2).all() and (valid & (kind == 1)).any()
    assert (rew[invalid] == -1.0).all() and (done[invalid] == 0).all() and ((info[invalid] >> 24) == 2).all()
    assert np.array_equal(rec1[invalid], rec0[invalid])            # a refused action changes nothing
    assert ((info[:16] >> 24) == 1).all() and (rec1[:16, CUR] == 1).all()        # passes: the turn moves on
    assert ((info[over] >> 24) == 3).all() and (done[over] == 1).all()           # finished: the reset step
    # the applied move against the oracle, on the valid lanes of the first 64
    for lane in np.nonzero(valid[:64])[0]:
        mover = int(rec0[lane, CUR])
        want = O.apply_move(rec0[lane, :52].view(np.int8), mover, int(mv0[lane, eff[lane]]) & (2**64 - 1))
        if rec1[lane, OVER] == 0:
            assert rec1[lane, CUR] == 1 - mover
        assert np.array_equal(rec1[lane, :52].view(np.int8), np.asarray(want, np.int8)), lane
    step_both(eo, en, legal_actions(en, torch.rand(B, device="cuda", generator=g)), tag="second")
    assert_same_state(eo, en, "second")


@pytest.mark.parametrize("change", ["set_lanes", "copy_lanes", "masked_reset", "start_table"])
@pytest.mark.parametrize("B", SIZES)
def test_lanes_changed_between_the_order_pass_and_the_step(bgx, dbg, B, change):
    """The gather reads the records, move lists and counters at the start of the step, not
    when the order pass ran: whatever a call between two steps changed is what the step sees."""
    eo, en = make_pair(bgx, dbg, B, 52)
    g = torch.Generator(device="cuda").manual_seed(8)
    midgame(eo, en, g, 10)
    odd = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
    for e in (eo, en):
        if change == "set_lanes":
            e.set_lanes(bearoff_records(8), lane0=B // 2)
        elif change == "copy_lanes":
            e.lanes()
        elif change == "masked_reset":
            e.reset(odd, want_obs=False)
        else:
            start = bearoff_records(B)
            start[:, ROLL0:ROLL1 + 1] = 0          # the roll is drawn at the reset
            e.set_starts(start.cpu())
            e.reset(want_obs=False)
    assert_same_state(eo, en, "changed")
    for t in range(3):
        step_both(eo, en, legal_actions(en, torch.rand(B, device="cuda", generator=g)), tag=(change, t))
        assert_same_state(eo, en, (change, t))


@pytest.mark.parametrize("B", SIZES)
def test_each_step_uses_the_actions_of_its_call(bgx, dbg, B):
    """Two different action tensors on consecutive steps, then one buffer the caller fills on
    the step's stream right before each call."""
    eo, en = make_pair(bgx, dbg, B, 63)
    g = torch.Generator(device="cuda").manual_seed(13)
    midgame(eo, en, g, 10)
    a1 = legal_actions(en, torch.rand(B, device="cuda", generator=g))
    step_both(eo, en, a1.clone(), a1, tag="a1")
    a2 = legal_actions(en, torch.rand(B, device="cuda", generator=g))
    step_both(eo, en, a2.clone(), a2, tag="a2")
    assert_same_state(eo, en, "two tensors")
    buf = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    for t in range(3):
        a = legal_actions(en, torch.rand(B, device="cuda", generator=g))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            buf.copy_(a)                         # queued on s just before the step on s
            _, ro, do, _ = eo.step(buf, want_obs=False)
            buf.zero_()                          # and rewritten right after it
        _, rn, dn, _ = en.step(a, want_obs=False)
        torch.cuda.synchronize()
        assert torch.equal(ro, rn) and torch.equal(do, dn), t
        assert_same_state(eo, en, ("stream", t))


@pytest.mark.parametrize("fork", ["on", "off", "switch"])
@pytest.mark.parametrize("B", [128, 200])
def test_fork_on_off_and_switched_through_game_ends(bgx, dbg, B, fork):
    """40 steps from a bear-off position (every game ends and auto-resets on the way) with the
    light launch and the count pass on the side stream, on the caller's, and switching."""
    eo, en = make_pair(bgx, dbg, B, 74)
    start = bearoff_records(B)
    for e in (eo, en):
        e.set_fork(fork != "off")
        e.reset(want_obs=False)
        e.set_lanes(start)
    g = torch.Generator(device="cuda").manual_seed(17)
    dones = torch.zeros(B, dtype=torch.int64, device="cuda")
    for t in range(40):
        if fork == "switch" and t % 5 == 0:
            eo.set_fork((t // 5) % 2 == 1)
        _, done, _ = step_both(eo, en, legal_actions(en, torch.rand(B, device="cuda", generator=g)), tag=t)
        dones += done.long()
        if t % 8 == 7:
            assert_same_state(eo, en, t)
    assert_same_state(eo, en, "end")
    assert int(dones.min()) >= 1


@pytest.mark.parametrize("B", [128, 200])
def test_graph_replays_with_rewritten_actions(bgx, dbg, B):
    """Two captured steps whose actions come from two buffers rewritten between replays: four
    replays equal eight eager steps of the BGX_ORDER 0 engine."""
    from bgx.graphs import capture
    eo, en = make_pair(bgx, dbg, B, 85)
    g = torch.Generator(device="cuda").manual_seed(19)
    midgame(eo, en, g, 10)
    eo.set_fork(False)
    bufs = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2)]
    rew = [torch.zeros(B, device="cuda") for _ in range(2)]
    done = [torch.zeros(B, dtype=torch.uint8, device="cuda") for _ in range(2)]
    cap = torch.cuda.Stream()
    with torch.cuda.stream(cap):
        eo.join()
    torch.cuda.synchronize()

    def body():
        for k in range(2):
            eo.step(bufs[k], want_obs=False, want_info=False, out=(rew[k], done[k]))
        eo.join()

    graph = capture("test_step_block", body, cap)
    torch.cuda.synchronize()
    for rep in range(4):
        # small indices: legal on most lanes, refused (-1, no change) where the list is shorter
        acts = [torch.randint(0, 6, (B,), device="cuda", generator=g, dtype=torch.int32) for _ in range(2)]
        for k in range(2):
            bufs[k].copy_(acts[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k in range(2):
            _, rn, dn, _ = en.step(acts[k], want_obs=False)
            assert torch.equal(rew[k], rn) and torch.equal(done[k], dn), (rep, k)
        assert_same_state(eo, en, rep)


@pytest.mark.parametrize("B", SIZES)
def test_accessor_returns_the_next_order_and_changes_nothing(bgx, dbg, B):
    """order() straight after a step, after a reset that selects no lane and after the next
    step: each a class-sorted permutation, and the steps compute what they compute without."""
    eo, en = make_pair(bgx, dbg, B, 96)
    g = torch.Generator(device="cuda").manual_seed(23)
    midgame(eo, en, g, 12)
    none = torch.zeros(B, dtype=torch.uint8, device="cuda")
    perm, cls, _ = eo.order()
    check_order(B, perm, cls)
    for e in (eo, en):
        e.reset(none, want_obs=False)
    perm2, cls2, _ = eo.order()
    check_order(B, perm2, cls2)
    assert np.array_equal(perm, perm2) and np.array_equal(cls, cls2)
    for t in range(3):
        step_both(eo, en, legal_actions(en, torch.rand(B, device="cuda", generator=g)), tag=t)
        perm, cls, _ = eo.order()
        check_order(B, perm, cls)
        perm2, _, _ = eo.order()
        assert np.array_equal(perm, perm2)
        assert_same_state(eo, en, t)
