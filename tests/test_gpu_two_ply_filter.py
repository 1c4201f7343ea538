"""bgx_two_ply_topk: the 2-ply search behind a 1-ply move filter (DESIGN.md §5 "Move
filter").  The yardsticks: bgx.search.move_filter_reference (the rule, plain torch on the
CPU; tests/test_move_filter_cpu.py) for WHICH moves are searched, and the full search
(two_ply) for their Q -- a kept move's Q is bit for bit its Q in the full search, so the
comparisons are exact.  Population: that of tests/test_gpu_search.py's setup."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
INF = float("inf")
SENT = -77.0


def _net(golden, H):
    from bgx.policy import PolicyNet
    mlp = golden("mlp")
    net = PolicyNet(hidden_size=H).cuda()
    pre = f"h{H}_"
    net.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in mlp.items()
                         if k.startswith(pre) and not k.endswith(("logits", "values"))})
    return net


@pytest.fixture(scope="module", params=[40, 128])
def setup(golden, request):
    """(engine, value head, n, the full search's (best, bestq, q, stats), the 1-ply
    (best, values)): the references, computed once."""
    import bgx
    from bgx.search import ValueHead, one_ply, two_ply
    net = _net(golden, request.param)
    B = 48
    eng = bgx.Engine(batch=B, max_moves=500, dice="mt", auto_reset=True)
    eng.seed(np.arange(500, 500 + B, dtype=np.uint32))
    eng.reset()
    rng = np.random.RandomState(2)
    for _ in range(25):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    vh = ValueHead(net)
    full = two_ply(eng, vh, want_q=True)
    b1, _, v1 = one_ply(eng, vh, want_values=True)
    return eng, vh, eng.n_moves().to(torch.int64), full, (b1, v1)


def _eq(a, b):
    """Bit equality of float tensors (NaN = never written, equal to itself)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_filtered(eng, n, full, got, v1, top_k, margin, lanes=None):
    """got = two_ply(..., top_k, margin, want_q, want_v1) against the reference mask on v1
    and the full search; `lanes`: bool[B], the lanes that were searched (default all).
    Returns the kept mask."""
    from bgx.search import move_filter_reference
    best, bestq, q, st = got[:4]
    fbest, fbestq, fq, fst = full
    B, M = q.shape
    lanes = torch.ones(B, dtype=torch.bool, device=q.device) if lanes is None else lanes
    legal = (torch.arange(M, device=q.device)[None, :] < n[:, None]) & lanes[:, None]
    keep = move_filter_reference(v1.cpu(), n.cpu(), top_k, margin).to(q.device) & lanes[:, None]
    # the finite entries of q are exactly the kept moves, bit-equal to the full search's
    assert torch.equal(torch.isfinite(q) & legal, keep)
    assert _eq(q[keep], fq[keep])
    assert bool((q[legal & ~keep] == -INF).all())
    assert bool(torch.isnan(q[~legal & lanes[:, None]]).all())             # a >= n: untouched
    # best = the first argmax of the full Q over the kept moves
    qk = torch.where(keep, fq, torch.full_like(fq, -INF))
    # torch's argmax names no tie order: the first index holding the maximum
    want = (qk == qk.max(dim=1, keepdim=True).values).to(torch.int32).argmax(dim=1)
    has = lanes & (n > 0)
    assert torch.equal(best[has].to(torch.int64), want[has])
    assert _eq(bestq[has], fq[has, want[has]])
    kept = int(keep.sum())
    assert st["afterstates"] == kept and st["jobs"] == 21 * kept
    assert st["candidates"] == int(n[lanes].sum())
    return keep


def test_identity_with_everything_kept(setup):
    """top_k = 500, margin = inf: best, bestq and q of two_ply, v1 of one_ply, bit for bit."""
    from bgx.search import two_ply
    eng, vh, n, full, (b1, v1) = setup
    best, bestq, q, st, gv1 = two_ply(eng, vh, want_q=True, top_k=500, margin=INF, want_v1=True)
    assert torch.equal(best, full[0]) and _eq(bestq, full[1]) and _eq(q, full[2])
    assert _eq(gv1, v1)
    assert st["candidates"] == st["afterstates"] == full[3]["afterstates"] == int(n.sum())
    assert {k: st[k] for k in ("leaves", "jobs", "afterstates")} == {k: full[3][k] for k in ("leaves", "jobs", "afterstates")}
    # margin alone: top_k defaults to max_moves
    best2, bestq2, q2, st2 = two_ply(eng, vh, want_q=True, margin=INF)
    assert torch.equal(best2, full[0]) and _eq(bestq2, full[1]) and _eq(q2, full[2]) and st2 == st


def test_filter_rule_and_subset_exactness(setup):
    from bgx.search import move_filter_reference, two_ply
    eng, vh, n, full, (b1, v1) = setup
    # the population must exercise the filter
    assert int((n > 4).sum()) >= 24, n.tolist()
    # margin: the median over lanes (with two moves or more) of V1best - V1(second best)
    legal = torch.arange(v1.shape[1], device=v1.device)[None, :] < n[:, None]
    top2 = torch.where(legal, v1, torch.full_like(v1, -INF)).sort(dim=1, descending=True).values[:, :2]
    gaps = (top2[:, 0] - top2[:, 1])[n >= 2]
    margin = float(gaps.median())
    assert margin > 0.0
    for top_k, mg in ((1, INF), (4, INF), (8, margin)):
        got = two_ply(eng, vh, want_q=True, top_k=top_k, margin=mg, want_v1=True)
        assert _eq(got[4], v1)
        keep = _check_filtered(eng, n, full, got, v1, top_k, mg)
        assert got[3]["leaves"] < full[3]["leaves"]
        if top_k == 1:
            has = n > 0
            assert torch.equal(got[0][has], b1[has])
            assert int(keep.sum()) == int(has.sum())
        if mg != INF:
            # the threshold bites: it drops moves that rank alone would keep
            by_rank = move_filter_reference(v1.cpu(), n.cpu(), top_k, INF).to(keep.device)
            assert int((by_rank & ~keep).sum()) >= 1


def test_lane_selection(setup):
    from bgx.search import two_ply
    eng, vh, n, full, (b1, v1) = setup
    B, M, dev = eng.batch, eng.max_moves, eng.device
    ref = two_ply(eng, vh, want_q=True, top_k=4, want_v1=True)
    sel = (torch.arange(B, device=dev) % 2 == 0).to(torch.uint8)
    on = sel.bool()
    out = (torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), SENT, device=dev),
           torch.full((B, M), SENT, device=dev))
    best, bestq, q, st, gv1 = two_ply(eng, vh, sel=sel, out=out, top_k=4, want_v1=True)
    assert torch.equal(best[on], ref[0][on]) and _eq(bestq[on], ref[1][on])
    legal = torch.arange(M, device=dev)[None, :] < n[:, None]
    assert _eq(q[on][legal[on]], ref[2][on][legal[on]])
    assert bool((q[on][~legal[on]] == SENT).all())
    assert _eq(gv1[on], ref[4][on])
    # unselected lanes: untouched
    assert bool((best[~on] == -7).all()) and bool((bestq[~on] == SENT).all()) and bool((q[~on] == SENT).all())
    assert bool(torch.isnan(gv1[~on]).all())
    keep = torch.isfinite(ref[2]) & legal & on[:, None]
    assert st["afterstates"] == int(keep.sum()) and st["jobs"] == 21 * int(keep.sum())
    assert st["candidates"] == int(n[on].sum())
    _check_filtered(eng, n, full, (best, bestq, torch.where(on[:, None] & legal, q, torch.full_like(q, math.nan)), st),
                    v1, 4, INF, lanes=on)
    # nothing selected: BGX_OK, nothing written, zero stats
    out = (torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), SENT, device=dev),
           torch.full((B, M), SENT, device=dev))
    best, bestq, q, st, gv1 = two_ply(eng, vh, sel=torch.zeros(B, dtype=torch.uint8, device=dev), out=out, top_k=4,
                                      want_v1=True)
    assert st == {"leaves": 0, "jobs": 0, "afterstates": 0, "candidates": 0}
    assert bool((best == -7).all()) and bool((bestq == SENT).all()) and bool((q == SENT).all())
    assert bool(torch.isnan(gv1).all())


@pytest.fixture(scope="module")
def awkward_records(golden):
    """Lane records with awkward legal-move counts: the three G1 golden positions with
    1,654-1,749 moves (500 after truncation: more than 64 x 7), and from a random
    population lanes with 0, 1, 63, 64 and 65 moves."""
    import bgx
    g = golden("movegen")
    big = np.nonzero(g["counts"] >= 1654)[0]
    assert len(big) == 3 and int(g["counts"][big].max()) == 1749, g["counts"][big]
    recs = []
    for i in big:
        r = np.zeros(64, np.uint8)
        r[:52] = g["boards"][i].view(np.uint8)
        r[52] = g["players"][i]
        r[53:55] = g["rolls"][i]
        recs.append(r)
    eng = bgx.Engine(batch=1024, max_moves=500, dice="mt", auto_reset=True)
    eng.seed(np.arange(9000, 9000 + 1024, dtype=np.uint32))
    eng.reset()
    rng = np.random.RandomState(13)
    want = {0: None, 1: None, 63: None, 64: None, 65: None}
    for _ in range(12):
        rec = eng.records().cpu().numpy()
        nm = rec[:, 60].astype(np.int64) | (rec[:, 61].astype(np.int64) << 8)
        for k in want:
            idx = np.nonzero((nm == k) & (rec[:, 55] == 0))[0]
            if want[k] is None and len(idx):
                want[k] = rec[idx[0]].copy()
        if all(v is not None for v in want.values()):
            break
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    assert all(v is not None for v in want.values()), [k for k, v in want.items() if v is None]
    return np.stack(recs + [want[k] for k in sorted(want)]), [500, 500, 500] + sorted(want)


def test_awkward_move_counts(golden, awkward_records):
    """n = 0, 1, 63, 64, 65 and 500 (chunks of 64 moves that are empty, partial, exactly
    full, one over, and eight of them), top_k = 3 at H = 40."""
    import bgx
    from bgx.search import ValueHead, one_ply, two_ply
    R, counts = awkward_records
    vh = ValueHead(_net(golden, 40))
    eng = bgx.Engine(batch=len(R), max_moves=500, dice="mt", auto_reset=True)
    eng.set_lanes(torch.from_numpy(R))
    n = eng.n_moves().to(torch.int64)
    assert n.tolist() == counts
    full = two_ply(eng, vh, want_q=True)
    _, _, v1 = one_ply(eng, vh, want_values=True)
    got = two_ply(eng, vh, want_q=True, top_k=3, want_v1=True)
    assert _eq(got[4], v1)
    keep = _check_filtered(eng, n, full, got, v1, 3, INF)
    assert keep.sum(dim=1).tolist() == [min(c, 3) for c in counts]
    # the lane without a move: what two_ply gives it
    z = counts.index(0)
    assert int(got[0][z]) == int(full[0][z]) and _eq(got[1][z:z + 1], full[1][z:z + 1])
    # a margin of 0 on the same lanes: the moves tied for best, three at most
    got0 = two_ply(eng, vh, want_q=True, top_k=3, margin=0.0, want_v1=True)
    _check_filtered(eng, n, full, got0, v1, 3, 0.0)
    assert eng.error() == 0


@pytest.mark.parametrize("option,value", [("BGX_2PLY_POOL", "32768"), ("BGX_2PLY_LDS_CAP", "6")])
def test_retry_and_overflow_paths(setup, dbg, option, value):
    """top_k = 4 with a leaf pool too small for one pass (retry rounds) and with every reply
    enumeration forced through the overflow tiers: the unforced call's results, bit for bit."""
    from bgx.search import two_ply
    eng, vh, n, full, _ = setup
    best, bestq, q, st = two_ply(eng, vh, want_q=True, top_k=4)
    dbg.setenv(option, value)
    best2, bestq2, q2, st2 = two_ply(eng, vh, want_q=True, top_k=4)
    assert st2 == st
    assert torch.equal(best2, best) and _eq(bestq2, bestq) and _eq(q2, q)
    assert eng.error() == 0


def test_arena_with_filtered_player(golden):
    """TwoPlyPlayer(top_k=2) against the random player: the match finishes, and the player
    searched at most two afterstates per root, fewer than it had candidates."""
    from bgx.arena import Arena, RandomPlayer, TwoPlyPlayer
    a = TwoPlyPlayer(_net(golden, 40), top_k=2)
    roots = []
    act = a.act

    def counting_act(eng, sel, step):
        nm = eng.n_moves()
        roots.append(((sel != 0) & (nm > 0)).sum())
        return act(eng, sel, step)
    a.act = counting_act
    res = Arena(64, 1, seed=3).play(a, RandomPlayer(5), max_steps=6000)
    assert res["unfinished_lanes"] == 0 and res["games"] == 64
    n_roots = int(torch.stack(roots).sum())
    assert 0 < a.totals["afterstates"] <= 2 * n_roots
    assert a.totals["candidates"] > a.totals["afterstates"]
    assert a.totals["jobs"] == 21 * a.totals["afterstates"]


def test_abi_errors(setup):
    """top_k < 1, a negative or NaN margin: BGX_EINVAL, nothing written."""
    from bgx._lib import BgxError
    from bgx.search import two_ply
    eng, vh, n, full, _ = setup
    B, M, dev = eng.batch, eng.max_moves, eng.device
    for top_k, margin in ((0, INF), (-3, INF), (4, -1.0), (4, math.nan)):
        out = (torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B,), SENT, device=dev),
               torch.full((B, M), SENT, device=dev))
        with pytest.raises(BgxError, match="BGX_EINVAL"):
            two_ply(eng, vh, out=out, top_k=top_k, margin=margin)
        torch.cuda.synchronize()
        assert bool((out[0] == -7).all()) and bool((out[1] == SENT).all()) and bool((out[2] == SENT).all())
