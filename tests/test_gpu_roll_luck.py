"""bgx_roll_luck (search.roll_luck) against an oracle made of existing entry points: every
lane's record posed with each of the 21 rolls on a second engine, bgx_one_ply's best value
there (V of the position itself where the mover cannot move, from the net in fp64), and the
mean and luck from those.  Narrow (H = 40) and wide (H = 128) evaluator; tolerance as
tests/test_gpu_search.py's for this evaluator."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]
PROBS = np.array([1 / 36 if a == b else 2 / 36 for a, b in ROLLS], np.float64)
B = 256


def record(p1, p2, mover, roll, bar=(0, 0)):
    r = np.zeros(64, np.uint8)
    for k, v in list(p1.items()) + list(p2.items()):
        r[k] = v
    r[48], r[49] = bar
    r[50] = 15 - r[:24].sum() - r[48]
    r[51] = 15 - r[24:48].sum() - r[49]
    r[52] = mover
    r[53], r[54] = roll
    return r


# PLAYER1 on the bar against a closed board: no roll enters
DANCE = record({18: 5, 19: 5, 21: 4}, {**{24 + i: 2 for i in range(6)}, 24 + 12: 3}, 0, (3, 1), bar=(1, 0))
BEAROFF = record({18: 3, 20: 2, 23: 2}, {24: 2, 26: 3}, 0, (6, 2))
# spread checkers: 394 / 421 legal moves for 1-1 / 3-3 (below the engine's 500-move lists)
SPREAD = record({0: 2, 3: 1, 5: 2, 8: 1, 10: 2, 11: 1, 13: 2, 16: 1, 18: 2, 20: 1},
                {24 + 23: 2, 24 + 12: 5, 24 + 7: 3, 24 + 4: 5}, 0, (2, 2))
POSED = np.stack([DANCE, BEAROFF, SPREAD])


def make_engine():
    """256 lanes after 30 random-action steps, lanes 0..2 posed."""
    import bgx
    eng = bgx.Engine(batch=B, max_moves=500, seed=21, dice="philox", auto_reset=True)
    eng.reset()
    rng = np.random.RandomState(8)
    for _ in range(30):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    eng.set_lanes(torch.from_numpy(POSED).cuda(), lane0=0, regen=True)
    return eng


def oracle_values(net, vh, rec):
    """v[i, r] of the records rec uint8[n, 64] in fp64, and how many (record, roll) pairs had
    a move list cut at the engine's max_moves (their value is not an oracle)."""
    import bgx
    from bgx.engine import encode
    from bgx.search import one_ply
    W1, b1 = net.fc1.weight.detach().double(), net.fc1.bias.detach().double()
    wv, bv = net.value_head.weight.detach().double().reshape(-1), net.value_head.bias.detach().double()
    e2 = bgx.Engine(batch=21 * 64, max_moves=500, seed=1, dice="philox", auto_reset=True)
    e2.reset()
    v = np.zeros((len(rec), 21), np.float64)
    cut = np.zeros((len(rec), 21), bool)
    for c0 in range(0, len(rec), 64):
        chunk = rec[c0:c0 + 64]
        lanes = np.repeat(chunk, 21, axis=0)
        if len(lanes) < 21 * 64:
            lanes = np.concatenate([lanes, np.repeat(chunk[:1], 21 * 64 - len(lanes), axis=0)])
        lanes[:, 53] = np.tile([a for a, _ in ROLLS], 64)
        lanes[:, 54] = np.tile([b for _, b in ROLLS], 64)
        e2.set_lanes(torch.from_numpy(lanes).cuda(), lane0=0, regen=True)
        _, bestv = one_ply(e2, vh)
        n = e2.n_moves().cpu().numpy().astype(np.int64)
        n_total = e2.lanes()[2].cpu().numpy()
        t = torch.from_numpy(lanes).cuda()
        x = encode(t[:, :52].view(torch.int8), t[:, 52]).double()
        v0 = (torch.relu(x @ W1.T + b1) @ wv + bv).cpu().numpy()
        vv = np.where(n > 0, bestv.cpu().numpy().astype(np.float64), v0)
        k = len(chunk) * 21
        v[c0:c0 + 64] = vv[:k].reshape(-1, 21)
        cut[c0:c0 + 64] = (n_total[:k] > 500).reshape(-1, 21)
    return v, cut


@pytest.fixture(scope="module", params=[40, 128])
def setup(golden, request):
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead, roll_luck
    H = request.param
    mlp = golden("mlp")
    net = PolicyNet(hidden_size=H).cuda()
    pre = f"h{H}_"
    net.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in mlp.items()
                         if k.startswith(pre) and not k.endswith(("logits", "values"))})
    vh = ValueHead(net)
    eng = make_engine()
    luck, mean, stats = roll_luck(eng, vh)
    torch.cuda.synchronize()
    return net, vh, eng, luck.clone(), mean.clone(), stats


def test_luck_and_mean_against_one_ply_oracle(setup):
    net, vh, eng, luck, mean, stats = setup
    rec = eng.records().cpu().numpy()
    assert np.array_equal(rec[:3, :55], POSED[:, :55])
    v, cut = oracle_values(net, vh, rec)
    ok = ~cut.any(axis=1)
    assert ok[:3].all() and ok.mean() >= 0.98          # a move list beyond 500 moves is no oracle
    idx = np.array([ROLLS.index((min(a, b), max(a, b))) for a, b in rec[:, 53:55]])
    mean_ref = v @ PROBS
    luck_ref = v[np.arange(B), idx] - mean_ref
    # the same in float32 with the kernel's FMA order (fp64 products and sums rounded per step)
    m32 = np.zeros(B, np.float32)
    for r in range(21):
        m32 = (np.float32(PROBS[r]).astype(np.float64) * v[:, r].astype(np.float32) + m32).astype(np.float32)
    emean = np.abs(mean.cpu().numpy() - mean_ref)[ok].max()
    eluck = np.abs(luck.cpu().numpy() - luck_ref)[ok].max()
    print("max |mean - oracle|", emean, "max |luck - oracle|", eluck, "fp32 order", np.abs(m32 - mean_ref)[ok].max())
    assert emean < TOL and eluck < TOL
    assert np.abs(m32 - mean.cpu().numpy())[ok].max() < TOL
    # nobody enters from the bar: every roll's value is the position's own
    assert abs(float(luck[0])) < TOL
    assert np.abs(v[0] - v[0, 0]).max() == 0.0
    # the posed positions are not degenerate for the others
    assert np.ptp(v[1]) > 0 and np.ptp(v[2]) > 0
    assert stats["rows"] == B and stats["jobs"] == 21 * B and stats["leaves"] >= stats["jobs"]
    assert eng.error() == 0


def test_selection(setup):
    from bgx.search import roll_luck
    net, vh, eng, luck, mean, stats = setup
    rng = np.random.RandomState(3)
    sel = torch.from_numpy((rng.rand(B) < 0.4).astype(np.uint8)).cuda()
    on = sel.bool()
    l2, m2, st = roll_luck(eng, vh, sel=sel)
    assert torch.isnan(l2[~on]).all() and torch.isnan(m2[~on]).all()
    assert torch.equal(l2[on], luck[on]) and torch.equal(m2[on], mean[on])
    assert st["rows"] == int(on.sum()) and st["jobs"] == 21 * st["rows"] and 0 < st["leaves"] < stats["leaves"]
    # the caller's tensors keep the unselected entries; mean is optional
    keep = torch.full((B,), 7.0, device="cuda")
    l3, m3, _ = roll_luck(eng, vh, sel=sel, out=(keep, None))
    assert l3 is keep and m3 is None and bool((keep[~on] == 7.0).all()) and torch.equal(keep[on], luck[on])
    # nothing selected: nothing written, zero stats
    l4, m4, st4 = roll_luck(eng, vh, sel=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    assert torch.isnan(l4).all() and torch.isnan(m4).all() and st4 == {"leaves": 0, "jobs": 0, "rows": 0}
    assert eng.error() == 0


def test_argument_checks(setup):
    from bgx import _lib
    net, vh, eng, luck, mean, stats = setup
    L = _lib.load()
    out = torch.zeros(B, device="cuda")
    good = [eng._h, vh.packed.data_ptr(), vh.hidden, vh.bias, None, out.data_ptr(), None, None, None]
    assert L.bgx_roll_luck(*good) == _lib.BGX_OK
    for idx, val in ((0, None), (1, None), (5, None), (2, 0), (2, 129)):
        bad = list(good)
        bad[idx] = val
        assert L.bgx_roll_luck(*bad) == _lib.BGX_EINVAL, idx
    torch.cuda.synchronize()
    assert torch.equal(out, luck)


@pytest.mark.parametrize("option,value", [("BGX_2PLY_POOL", "16384"), ("BGX_2PLY_LDS_CAP", "6")])
def test_schedule_independence(setup, option, value):
    """Retry rounds (a leaf pool too small for one pass) and the overflow tiers (tiny dedup
    tables): luck and mean bit for bit the default run's."""
    from bgx import _lib
    from bgx.search import roll_luck
    net, vh, eng, luck, mean, stats = setup
    _lib.debug_option(option, value)
    try:
        l2, m2, st = roll_luck(eng, vh)
    finally:
        _lib.debug_option(option, None)
    assert st == stats
    assert torch.equal(l2, luck) and torch.equal(m2, mean)
    assert eng.error() == 0


def test_other_stream_reads_the_stepped_lanes(setup):
    from bgx.search import roll_luck
    net, vh, eng, luck, mean, stats = setup
    eng = make_engine()
    before = eng.records().clone()
    nm = eng.n_moves().cpu().numpy()
    act = torch.from_numpy(np.array([k - 1 if k else 0 for k in nm], np.int32)).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        eng.step(act, want_obs=False)
    with torch.cuda.stream(s2):
        l2, m2, _ = roll_luck(eng, vh)
    torch.cuda.synchronize()
    assert not torch.equal(eng.records()[:, :55], before[:, :55])
    l3, m3, _ = roll_luck(eng, vh)
    assert torch.equal(l2, l3) and torch.equal(m2, m3)
    assert not torch.equal(l2, luck)
