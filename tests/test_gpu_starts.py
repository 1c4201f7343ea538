"""Per-lane start positions (bgx_engine_set_starts, Engine.set_starts): every reset path
gives the lane's start record, the dice accounting is exact, an engine without a table is
unchanged.  The starts are small bear-off positions, so games end within a handful of
plies and the lanes reset constantly."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bgx():
    import bgx as _bgx
    assert torch.cuda.is_available()
    return _bgx


def bearoff_starts(B, seed):
    """B start records: 1..3 checkers left per side in the home boards, a random mover; even
    lanes a fixed roll (lane % 4 == 0: doubles), odd lanes roll (0, 0) = drawn at the reset."""
    rng = np.random.RandomState(seed)
    s = np.zeros((B, 64), np.uint8)
    for i in range(B):
        for side, base in ((0, 18), (1, 24)):
            k = rng.randint(1, 4)
            for p in rng.randint(0, 6, size=k):
                s[i, base + p] += 1
            s[i, 50 + side] = 15 - k
        s[i, 52] = rng.randint(2)
        if i % 2 == 0:
            d = rng.randint(1, 7)
            s[i, 53], s[i, 54] = d, d if i % 4 == 0 else rng.randint(1, 7)
        s[i, 55:] = rng.randint(0, 256, size=9)          # ignored by the engine
    return s


def n_of(rec):
    return rec[:, 60].astype(np.int64) | (rec[:, 61].astype(np.int64) << 8)


def host(eng):
    rec, mv, nt = eng.lanes()
    return rec.cpu().numpy(), mv.cpu().numpy().view(np.uint64), nt.cpu().numpy()


def check_movegen(rec, mv, nt, lanes, tag):
    boards = np.ascontiguousarray(rec[lanes, :52]).view(np.int8)
    counts, ref = O.movegen_batch(boards, rec[lanes, 52].copy(), rec[lanes, 53:55].copy(), 500)
    n = n_of(rec)
    for k, i in enumerate(lanes):
        assert nt[i] == counts[k] and n[i] == min(int(counts[k]), 500), (tag, i)
        assert np.array_equal(mv[i, :n[i]], ref[k, :n[i]]), (tag, i)


def test_mt_exact_dice_and_reset(bgx):
    B, T = 64, 40
    starts = bearoff_starts(B, 1)
    fixed = starts[:, 53] != 0
    seeds = np.arange(500, 500 + B, dtype=np.uint32)
    eng = bgx.Engine(batch=B, max_moves=500, dice="mt", auto_reset=True)
    eng.seed(seeds)
    eng.set_starts(torch.from_numpy(starts))
    mts = [O.MT(int(s)) for s in seeds]

    def expect_start(rec, i, tag):
        assert np.array_equal(rec[i, :53], starts[i, :53]) and rec[i, 55] == 0, (tag, i)
        want = tuple(starts[i, 53:55]) if fixed[i] else (mts[i].die(), mts[i].die())
        assert tuple(rec[i, 53:55]) == want, (tag, i, want)

    before = host(eng)[0]
    assert not before.any()                               # set_starts does not touch the lanes
    eng.reset()
    rec, mv, nt = host(eng)
    for i in range(B):
        expect_start(rec, i, "reset")
    check_movegen(rec, mv, nt, np.arange(B), "reset")
    pol = np.random.RandomState(2)
    resets = np.zeros(B, np.int64)
    for t in range(T):
        n = n_of(rec)
        acts = np.array([pol.randint(k) if k else 0 for k in n], np.int32)
        _, _, done, info = eng.step(torch.from_numpy(acts).cuda())
        done, info = done.cpu().numpy(), info.cpu().numpy()
        rec, mv, nt = host(eng)
        for i in range(B):
            if done[i]:
                # the start position again in the step that ended the game
                assert ((info[i] >> 8) & 0xFF) - 1 == (info[i] & 0xFF), (t, i)
                expect_start(rec, i, t)
                resets[i] += 1
            else:
                want = (mts[i].die(), mts[i].die())       # an ordinary roll after a move or a pass
                assert tuple(rec[i, 53:55]) == want, (t, i, want)
        check_movegen(rec, mv, nt, np.arange(B), t)
    assert resets.min() >= 2, resets.min()
    assert (resets[fixed & (starts[:, 53] == starts[:, 54])] >= 2).all()
    assert eng.error() == 0


def test_masked_reset_and_no_auto_reset(bgx):
    """bgx_reset with a mask gives the masked lanes their starts and leaves the others; an
    auto_reset = 0 engine gives the start in its reset step."""
    B = 64
    starts = bearoff_starts(B, 3)
    starts[:, 53:55] = (6, 5)
    eng = bgx.Engine(batch=B, max_moves=500, dice="mt", auto_reset=False)
    eng.seed(np.arange(B, dtype=np.uint32))
    eng.reset()
    opening = host(eng)[0]
    assert all(np.array_equal(opening[i, :52].view(np.int8), O.INITIAL_BOARD52) for i in range(B))
    eng.set_starts(torch.from_numpy(starts))
    mask = torch.zeros(B, dtype=torch.uint8)
    mask[::3] = 1
    eng.reset(lane_mask=mask.cuda())
    rec, mv, nt = host(eng)
    m = mask.numpy().astype(bool)
    assert np.array_equal(rec[m, :55], starts[m, :55]) and np.array_equal(rec[~m], opening[~m])
    check_movegen(rec, mv, nt, np.arange(B), "masked")
    # play the masked lanes' bear-offs out: done, then the reset step returns done again with the start
    pol = np.random.RandomState(4)
    seen = np.zeros(B, bool)
    for t in range(30):
        was_over = rec[:, 55] != 0
        acts = np.array([pol.randint(k) if k else 0 for k in n_of(rec)], np.int32)
        _, _, done, info = eng.step(torch.from_numpy(acts).cuda())
        done, info = done.cpu().numpy(), info.cpu().numpy()
        rec, mv, nt = host(eng)
        for i in np.nonzero(was_over)[0]:
            assert done[i] and (info[i] >> 24) == 3 and np.array_equal(rec[i, :55], starts[i, :55]), (t, i)
            seen[i] = True
        check_movegen(rec, mv, nt, np.nonzero(rec[:, 55] == 0)[0], t)
    assert seen[m].all()
    assert eng.error() == 0


@pytest.mark.parametrize("B", [1024, 1000])
def test_philox_vs_oracle_and_dispatch_variants(bgx, dbg, B):
    """XCD-aware (B % 128 == 0) and plain dispatch order.  Sampled lanes against the oracle
    at every step (move lists of the new record, the applied move, the start position after
    a done); engines without a dispatch order and without the fork give the same records,
    moves and rewards at every step."""
    T = 40
    starts = bearoff_starts(B, 5)
    fixed = starts[:, 53] != 0
    engs = []
    for opt, fork in ((None, True), ("BGX_ORDER", True), (None, False)):
        dbg.delenv("BGX_ORDER", raising=False)
        if opt:
            dbg.setenv(opt, "0")
        e = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=11, auto_reset=True)
        if not fork:
            e.set_fork(False)
        e.set_starts(torch.from_numpy(starts))
        e.reset(want_obs=False)
        engs.append(e)
    dbg.delenv("BGX_ORDER", raising=False)
    eng = engs[0]
    g = torch.Generator(device="cuda").manual_seed(6)
    live_idx = torch.arange(500, device="cuda")[None, :]
    rec, mv, nt = host(eng)
    assert np.array_equal(rec[:, :53], starts[:, :53]) and np.array_equal(rec[fixed, 53:55], starts[fixed, 53:55])
    check_movegen(rec, mv, nt, np.arange(0, B, 3), "reset")
    dbl_resets = 0
    for t in range(T):
        prev, pmv = rec, mv
        u = torch.rand(B, device="cuda", generator=g)
        outs = []
        for e in engs:
            a = (u * e.n_moves().clamp(min=1).float()).to(torch.int32)
            _, r, d, _ = e.step(a, want_obs=False)
            outs.append((a, r.clone(), d.clone()) + e.lanes())
        a0, r0, d0, rec0, mv0, nt0 = outs[0]
        live = live_idx < (rec0[:, 60].long() | (rec0[:, 61].long() << 8))[:, None]
        for a, r, d, rc, m, n in outs[1:]:
            assert torch.equal(a, a0) and torch.equal(r, r0) and torch.equal(d, d0), t
            assert torch.equal(rc, rec0) and torch.equal(n, nt0), t
            assert torch.equal(torch.where(live, m, 0), torch.where(live, mv0, 0)), t
        rec, mv, nt = rec0.cpu().numpy(), mv0.cpu().numpy().view(np.uint64), nt0.cpu().numpy()
        a, done = a0.cpu().numpy(), d0.cpu().numpy()
        sel, n_prev = np.arange(t % 3, B, 3), n_of(prev)
        check_movegen(rec, mv, nt, sel, t)
        assert ((rec[:, 53] >= 1) & (rec[:, 53] <= 6) & (rec[:, 54] >= 1) & (rec[:, 54] <= 6)).all()
        for i in sel:
            if done[i]:
                assert np.array_equal(rec[i, :53], starts[i, :53]) and rec[i, 55] == 0, (t, i)
                if fixed[i]:
                    assert np.array_equal(rec[i, 53:55], starts[i, 53:55]), (t, i)
                dbl_resets += int(rec[i, 53] == rec[i, 54])
            elif n_prev[i] > 0:
                after = O.apply_move(prev[i, :52].view(np.int8), int(prev[i, 52]), int(pmv[i, a[i]]))
                assert np.array_equal(rec[i, :52].view(np.int8), after) and rec[i, 52] == 1 - prev[i, 52], (t, i)
            else:
                assert np.array_equal(rec[i, :52], prev[i, :52]) and rec[i, 52] == 1 - prev[i, 52], (t, i)
    assert dbl_resets >= 30, dbl_resets
    for e in engs:
        assert e.error() == 0


@pytest.mark.parametrize("dice", ["mt", "philox"])
def test_clearing_the_table(bgx, dice):
    """set_starts(None) + reset(): bit for bit a fresh engine with the same seed that never
    had a table.  MT lanes: the table's fixed rolls drew nothing, so no re-seeding; Philox:
    after games from the table, both engines re-seeded.  Those games left match scores in
    the used engine's records (bytes 57, 58), which a reset keeps exactly as the standard
    reset does: they stay as they were and are left out of the Philox comparison."""
    B, T = 256, 20
    starts = bearoff_starts(B, 7)
    seeds = np.arange(40, 40 + B, dtype=np.uint32)
    used = bgx.Engine(batch=B, max_moves=500, dice=dice, seed=5, auto_reset=True)
    fresh = bgx.Engine(batch=B, max_moves=500, dice=dice, seed=5, auto_reset=True)
    g = torch.Generator(device="cuda").manual_seed(8)
    if dice == "mt":
        starts[:, 53:55] = (2, 2)
        used.seed(seeds)
        fresh.seed(seeds)
        used.set_starts(torch.from_numpy(starts))
        used.reset()
        assert np.array_equal(host(used)[0][:, :55], starts[:, :55])
    else:
        used.set_starts(torch.from_numpy(starts))
        used.reset()
        for _ in range(6):
            used.step((torch.rand(B, device="cuda", generator=g) * used.n_moves().clamp(min=1).float()).to(torch.int32))
        keep = used.lanes()[0][:, 56:59].clone()
        keep[keep[:, 0] != 0] = 0                          # a finished match: the reset zeroes its scores
        assert bool((keep[:, 1:] > 0).any())
    used.set_starts(None)
    if dice == "philox":
        used.seed(philox_seed=77)
        fresh.seed(philox_seed=77)
    o1, o2 = used.reset().clone(), fresh.reset().clone()
    assert torch.equal(o1, o2)
    for t in range(T):
        u = torch.rand(B, device="cuda", generator=g)
        res = []
        for e in (used, fresh):
            a = (u * e.n_moves().clamp(min=1).float()).to(torch.int32)
            obs, r, d, info = e.step(a)
            rec, mv, nt = e.lanes()
            if dice == "philox":
                if e is used:
                    assert torch.equal(rec[:, 56:59], keep), t
                rec[:, 56:59] = 0
            live = torch.arange(500, device="cuda")[None, :] < (rec[:, 60].long() | (rec[:, 61].long() << 8))[:, None]
            res.append((obs.clone(), r.clone(), d.clone(), info.clone(), rec, nt, torch.where(live, mv, 0)))
        for x, y in zip(*res):
            assert torch.equal(x, y), t
    assert used.error() == 0 and fresh.error() == 0


def test_refusals(bgx):
    from bgx import _lib
    B = 64
    starts = bearoff_starts(B, 9)
    starts[:, 53:55] = (3, 1)
    L = _lib.load()
    sh = bgx.Engine(batch=B, max_moves=500, dice="shared", auto_reset=True)
    dev = torch.from_numpy(starts).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bgx_engine_set_starts(sh._h, ctypes.c_void_p(dev.data_ptr()), stream) == _lib.BGX_EINVAL
    assert L.bgx_engine_set_starts(sh._h, None, stream) == _lib.BGX_EINVAL
    with pytest.raises(ValueError, match="shared"):
        sh.set_starts(dev)
    eng = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=1, auto_reset=True)
    with pytest.raises(ValueError, match="lane 17"):
        bad = starts.copy()
        bad[17, 50] -= 1
        eng.set_starts(torch.from_numpy(bad))
    with pytest.raises(ValueError):
        eng.set_starts(torch.from_numpy(starts[:32]))
    assert eng.error() == 0
    # one bad record straight through the C ABI: error bit 2, that lane gets the opening
    bad = starts.copy()
    bad[17, 18:24] = 0
    bad[17, 50] = 15                                        # all 15 off: no position to start from
    bdev = torch.from_numpy(bad).cuda()
    assert L.bgx_engine_set_starts(eng._h, ctypes.c_void_p(bdev.data_ptr()), stream) == _lib.BGX_OK
    eng.reset()
    rec, mv, nt = host(eng)
    assert eng.error() == 4
    ok = np.arange(B) != 17
    assert np.array_equal(rec[ok, :55], starts[ok, :55])
    assert np.array_equal(rec[17, :52].view(np.int8), O.INITIAL_BOARD52) and rec[17, 53] != rec[17, 54]
    check_movegen(rec, mv, nt, np.arange(B), "bad record")
