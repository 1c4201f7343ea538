"""The Philox dispatch order with the class resolved in the order pass (k_order_count,
one thread per lane: DESIGN.md §3.4): the dice stream and every result equal the engine
without an order through game ends and resets, the resolved classes are the documented
table's, the order is a valid class-sorted permutation, and the pass is idempotent."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 128: one block on the XCD-aware path; 1000: the plain sort with a padded block;
# 2176 = 17 x 128: several blocks on the XCD-aware path
SIZES = [128, 1000, 2176]
CUR, ROLL0, ROLL1, OVER = 52, 53, 54, 55


@pytest.fixture(scope="module")
def bgx():
    import bgx as _bgx
    assert torch.cuda.is_available()
    return _bgx


def bearoff_records(B):
    """Both sides' 15 checkers on their own ace points (player 0: point 23, player 1:
    point 0): every roll bears off at least two checkers, so a game ends within 16 steps."""
    rec = np.zeros((B, 64), np.uint8)
    rec[:, 23] = 15
    rec[:, 24 + 0] = 15
    i = np.arange(B)
    rec[:, CUR] = i % 2
    rec[:, ROLL0] = 1 + i % 6
    rec[:, ROLL1] = 1 + (i // 6) % 6
    return torch.from_numpy(rec).cuda()


def legal_actions(e, u):
    return (u * e.n_moves().clamp(min=1).float()).to(torch.int32)


def expected_classes(rt, rt1):
    """predict_class's table in numpy: the roll from R_{t+1}, the board and mover from R_t."""
    a, b = rt1[:, ROLL0].astype(int), rt1[:, ROLL1].astype(int)
    nxt = 1 - rt[:, CUR].astype(int)
    B = len(rt)
    pts = np.empty(B, int)
    for i in range(B):
        pts[i] = int((rt[i, nxt[i] * 24:nxt[i] * 24 + 24] > 0).sum()) + (2 if rt[i, 48 + nxt[i]] > 0 else 0)
    c = np.where(pts >= 5, 2, 3)
    c = np.where(((pts >= 8) & (a <= 5)) | (pts >= 10), 1, c)
    c = np.where((pts >= 10) & (a <= 4), 0, c)
    return np.where(a != b, 4, c)


@pytest.mark.parametrize("fork", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_results_equal_no_order_engine_through_game_ends(bgx, dbg, B, fork):
    """An engine without an order (BGX_ORDER 0) never predicts or caches a roll: its dice
    come straight from the counters.  From a bear-off position every lane ends its game,
    auto-resets (the opening roll ignores the cache) and plays on; rewards, dones, records,
    counts and live move lists are equal after every one of 48 steps."""
    dbg.delenv("BGX_ORDER", raising=False)
    eo = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=33, auto_reset=True)
    dbg.setenv("BGX_ORDER", "0")
    en = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=33, auto_reset=True)
    dbg.delenv("BGX_ORDER", raising=False)
    start = bearoff_records(B)
    for e in (eo, en):
        e.set_fork(fork)
        e.reset(want_obs=False)
        e.set_lanes(start)
    g = torch.Generator(device="cuda").manual_seed(5)
    idx = torch.arange(500, device="cuda")[None, :]
    dones = torch.zeros(B, dtype=torch.int64, device="cuda")
    for step in range(48):
        u = torch.rand(B, device="cuda", generator=g)
        _, ro, do, _ = eo.step(legal_actions(eo, u), want_obs=False)
        _, rn, dn, _ = en.step(legal_actions(en, u), want_obs=False)
        assert torch.equal(ro, rn) and torch.equal(do, dn), step
        dones += do.long()
        rec_o, mv_o, nt_o = eo.lanes()
        rec_n, mv_n, nt_n = en.lanes()
        assert torch.equal(rec_o, rec_n) and torch.equal(nt_o, nt_n), step
        live = idx < (rec_n[:, 60].long() | (rec_n[:, 61].long() << 8))[:, None]   # entries past n are scratch
        assert torch.equal(torch.where(live, mv_o, 0), torch.where(live, mv_n, 0)), step
        assert eo.error() == 0 and en.error() == 0
    assert int(dones.min()) >= 1            # the start position ends every game within 16 steps
    # and the ordered engine did cache rolls on the way
    _, cls, ctr = eo.order()
    assert ((ctr >> np.uint64(63)) != 0).mean() > 0.9


def _midgame(bgx, B, auto_reset, fork=True):
    e = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=77, auto_reset=auto_reset)
    e.set_fork(fork)
    e.reset(want_obs=False)
    g = torch.Generator(device="cuda").manual_seed(9)
    if not auto_reset:
        # finished games that stay in the records: the even lanes have two checkers left
        # per side (13 borne off), so their mover wins with any roll in the one step below
        rec = bearoff_records(B)
        rec[::2, 23] = 2
        rec[::2, 24] = 2
        rec[::2, 50:52] = 13
        e.set_lanes(rec)
    for _ in range(40 if auto_reset else 1):
        e.step(legal_actions(e, torch.rand(B, device="cuda", generator=g)), want_obs=False)
    return e, g


def _check_order(B, perm, cls):
    assert np.array_equal(np.sort(perm), np.arange(B))
    assert cls.max() <= 4
    if B % 128 == 0:                         # XCD-aware: 8 interleaved class-sorted sub-lists
        for x in range(8):
            assert (np.diff(cls[perm[x::8]].astype(int)) >= 0).all(), x
    else:
        assert (np.diff(cls[perm].astype(int)) >= 0).all()


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_resolved_classes_and_order(bgx, B, auto_reset):
    """The accessor's classes equal predict_class's table recomputed from the records (the
    roll the lane really draws next, the board it was predicted on), finished games are
    class 4, and perm is a permutation sorted by those classes (per sub-list when
    B % 128 == 0).  auto_reset False leaves finished games in the records."""
    e, g = _midgame(bgx, B, auto_reset)
    rt = e.records().cpu().numpy()
    perm, cls, _ = e.order()
    _check_order(B, perm, cls)
    _, _, done, _ = e.step(legal_actions(e, torch.rand(B, device="cuda", generator=g)), want_obs=False)
    done = done.cpu().numpy() != 0
    rt1 = e.records().cpu().numpy()
    over = rt[:, OVER] != 0
    assert (cls[over] == 4).all()
    if not auto_reset:
        assert over[::2].all() and not over[1::2].any()
    sel = ~over & ~done                      # rolled a normal roll in this step
    assert sel.sum() >= B // 2               # 40 plies from the opening / 2 plies into a 15-checker bear-off
    want = expected_classes(rt, rt1)
    assert np.array_equal(cls[sel], want[sel])
    if auto_reset:
        assert (cls < 4).any()               # not everything in the lightest class
    perm, cls, _ = e.order()
    _check_order(B, perm, cls)
    assert e.error() == 0


@pytest.mark.parametrize("fork", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_order_pass_is_idempotent(bgx, B, fork):
    """The order pass run again with no step between (a reset that selects no lane) finds
    the same counters and pre-class bytes: counters (cache bits included), classes and perm
    stay as they were; likewise after a reset of half the lanes."""
    e, _ = _midgame(bgx, B, True, fork)
    none = torch.zeros(B, dtype=torch.uint8, device="cuda")
    half = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
    a = e.order()
    e.reset(none, want_obs=False)
    b = e.order()
    e.reset(none, want_obs=False)
    c = e.order()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(y, z)
    e.reset(half, want_obs=False)
    d = e.order()
    assert not np.array_equal(d[2], c[2])    # the reset lanes drew their opening rolls
    keep = half.cpu().numpy() == 0
    assert np.array_equal(d[2][keep], c[2][keep])
    e.reset(none, want_obs=False)
    f = e.order()
    for x, y in zip(d, f):
        assert np.array_equal(x, y)
    _check_order(B, f[0], f[1])
    assert e.error() == 0


def _call_sequence(e, B, u, streams):
    """reset, 6 steps, a reset of the odd lanes, set_lanes of 8 bear-off records, 6 steps, a
    movegen of 16 positions, set_fork(False), 4 steps, join: call i on streams[i % len]."""
    odd = (torch.arange(B, device="cuda") % 2).to(torch.uint8)
    pos = bearoff_records(16)
    boards, players = pos[:, :52].contiguous().view(torch.int8), pos[:, CUR].contiguous()
    dice = pos[:, ROLL0:ROLL1 + 1].contiguous()
    start = bearoff_records(8)
    rew = torch.zeros(16, B, dtype=torch.float32, device="cuda")
    done = torch.zeros(16, B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    calls = iter(range(1 << 30))
    out = {}

    def on_next_stream():
        return torch.cuda.stream(streams[next(calls) % len(streams)])

    def steps(t0, n):
        for t in range(t0, t0 + n):
            with on_next_stream():               # the actions on the stream the step runs on
                e.step(legal_actions(e, u[t]), want_obs=False, out=(rew[t], done[t]))

    with on_next_stream():
        e.reset(want_obs=False)
    steps(0, 6)
    with on_next_stream():
        e.reset(odd, want_obs=False)
    with on_next_stream():
        e.set_lanes(start)
    steps(6, 6)
    with on_next_stream():
        out["movegen"] = e.movegen(boards, players, dice)
    with on_next_stream():
        e.set_fork(False)
    steps(12, 4)
    with on_next_stream():
        e.join()
        out["lanes"] = e.lanes()
    torch.cuda.synchronize()
    out["order"] = e.order()
    out["rew"], out["done"] = rew, done
    return out


@pytest.mark.parametrize("B", [256, 200])
def test_calls_on_two_streams_equal_one_stream(bgx, B):
    """The engine orders its own calls (the call guard, the dispatch-order join, the rotating
    overflow counters): the same calls alternating between two non-default streams with no
    host synchronisation between them give what they give on one stream.  256 and 200 are
    the smallest batches whose split dispatch has a light launch on the XCD-aware path
    (heavy 104) and on the plain one (heavy 86)."""
    g = torch.Generator(device="cuda").manual_seed(21)
    u = torch.rand(16, B, device="cuda", generator=g)
    torch.cuda.synchronize()
    ex = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=91, auto_reset=True)
    ey = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=91, auto_reset=True)
    x = _call_sequence(ex, B, u, [torch.cuda.current_stream()])
    y = _call_sequence(ey, B, u, [torch.cuda.Stream(), torch.cuda.Stream()])
    assert torch.equal(x["rew"], y["rew"]) and torch.equal(x["done"], y["done"])
    idx = torch.arange(500, device="cuda")[None, :]
    (rec_x, mv_x, nt_x), (rec_y, mv_y, nt_y) = x["lanes"], y["lanes"]
    assert torch.equal(rec_x, rec_y) and torch.equal(nt_x, nt_y)
    live = idx < (rec_x[:, 60].long() | (rec_x[:, 61].long() << 8))[:, None]       # entries past n are scratch
    assert torch.equal(torch.where(live, mv_x, 0), torch.where(live, mv_y, 0))
    (nm_x, mt_x, mg_x), (nm_y, mt_y, mg_y) = x["movegen"], y["movegen"]
    assert torch.equal(nm_x, nm_y) and torch.equal(mt_x, mt_y)
    live = idx < nm_x.long()[:, None]
    assert torch.equal(torch.where(live, mg_x, 0), torch.where(live, mg_y, 0))
    for a, b in zip(x["order"], y["order"]):
        assert np.array_equal(a, b)
    assert ex.error() == 0 and ey.error() == 0
