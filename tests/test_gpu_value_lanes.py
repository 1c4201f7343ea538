"""bgx_value_lanes (search.value_lanes): the static value V(enc(X, m)) of lane records, against
the reference network's golden values and bgx_policy_act's value_out, against fp64 at every
evaluator width, under every kind of lane selection, captured into a graph, and against
bgx_roll_luck's mean where the mover cannot move (the definition both lookaheads of a truncated
rollout share)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # BASELINE.json: MLP value outputs within 1e-5 fp32
EPS = 2.0 ** -22                 # tests/test_gpu_widths.py's running-error bound 2^-22 * A(row)
NAN = float("nan")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def records1000():
    """1,000 records of an engine after 25 random-policy steps (both movers, bars, checkers off)."""
    import bgx
    eng = bgx.Engine(batch=1000, max_moves=500, dice="philox", seed=11, auto_reset=True)
    eng.reset()
    rng = np.random.RandomState(4)
    for _ in range(25):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    rec = eng.records().clone()
    r = rec.cpu().numpy()
    assert set(r[:, 52]) == {0, 1} and r[:, 48:50].any() and len({tuple(x[:53]) for x in r}) > 900
    return rec


@pytest.mark.parametrize("H", [128, 40])
def test_golden_values(golden, H):
    from bgx.search import ValueHead, value_lanes
    from test_gpu_policy import _net, _records
    mlp, feat, mg = golden("mlp"), golden("features"), golden("movegen")
    idx = feat["obs_idx"][:600]
    rec = _records(mg["boards"][idx], feat["obs_player"][:600])
    net = _net(mlp, H)
    v = value_lanes(rec, ValueHead(net))
    e_gold = np.abs(v.cpu().numpy() - mlp[f"h{H}_values"][:600]).max()
    val = net.act(rec, seed=1, step=0)[2]
    e_act = float((v - val).abs().max())
    print(f"[value_lanes] golden H={H}: max |v - golden| {e_gold:.3e}, max |v - act's value_out| {e_act:.3e}")
    assert e_gold < TOL and e_act < TOL


def _fp64(net, rec):
    from test_gpu_widths import _w64
    r = rec.cpu().numpy()
    x = O.features_batch(r[:, :52].view(np.int8), r[:, 52]).astype(np.float64)
    x[:, 97] = r[:, 50].astype(np.float64) / 15          # off / 15 exactly, not its fp32 rounding
    x[:, 195] = r[:, 51].astype(np.float64) / 15
    W1, b1, _, _, wv, bv = _w64(net)
    ref = np.maximum(x @ W1.T + b1, 0) @ wv.ravel() + bv[0]
    bound = (x @ np.abs(W1).T + np.abs(b1)) @ np.abs(wv).ravel() + abs(bv[0])
    return ref, bound


def _check_fp64(rec, H, scale):
    from bgx.search import ValueHead, value_lanes
    from test_gpu_widths import _net
    net = _net(H, scale=scale)
    v = value_lanes(rec, ValueHead(net)).cpu().numpy().astype(np.float64)
    ref, bound = _fp64(net, rec)
    err = np.abs(v - ref)
    ratio = err / (EPS * bound)
    print(f"[value_lanes] H={H} {scale}: max err {err.max():.3e}, max err/bound {ratio.max():.3f}")
    assert np.isfinite(v).all() and (ratio <= 1.0).all(), (H, scale, float(ratio.max()))
    if scale == "default":
        assert err.max() < TOL


@pytest.mark.parametrize("H", [7, 24, 48, 64, 65, 96, 100, 127, 128])
def test_every_width_against_fp64(records1000, H):
    """k_value_lanes at every NT = 1..8 (and 128, the full last tile): every record's value
    against the fp64 MLP on the oracle's features, within 2^-22 * A(row) and 1e-5."""
    _check_fp64(records1000, H, "default")


@pytest.mark.parametrize("scale", ["up_down", "down_up"])
@pytest.mark.parametrize("H", [24, 65])
def test_scaled_weights_against_fp64(records1000, H, scale):
    _check_fp64(records1000, H, scale)


@pytest.mark.parametrize("H", [40, 128])
def test_selection(records1000, H):
    """n in {1, 63, 64, 65, 1000} x {all, none, one lane, every 7th lane, a random half}: selected
    entries are bit for bit those of the call without a selection, the others keep their NaN,
    and a second call gives identical bits."""
    from bgx.search import ValueHead, value_lanes
    from test_gpu_widths import _net
    vh = ValueHead(_net(H))
    rng = np.random.RandomState(H)
    for n in (1, 63, 64, 65, 1000):
        rec = records1000[:n].contiguous()
        full = value_lanes(rec, vh)
        assert bool(torch.isfinite(full).all())
        sels = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "one": np.zeros(n, np.uint8),
                "seventh": (np.arange(n) % 7 == 3).astype(np.uint8), "half": (rng.rand(n) < 0.5).astype(np.uint8)}
        sels["one"][n // 2] = 1
        sels["all"][0] = 200                                # any non-zero byte selects
        for name, s in sels.items():
            sel = torch.from_numpy(s).cuda()
            outs = []
            for _ in range(2):
                out = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
                assert value_lanes(rec, vh, sel=sel, out=out) is out
                outs.append(out)
            on = sel != 0
            assert torch.equal(bits(outs[0])[on], bits(full)[on]), (n, name)
            assert bool(torch.isnan(outs[0][~on]).all()), (n, name)
            assert torch.equal(bits(outs[0]), bits(outs[1])), (n, name)


def test_graph_capture(records1000):
    from bgx.search import ValueHead, value_lanes
    from test_gpu_widths import _net
    vh = ValueHead(_net(128))
    n = 1000
    rec = records1000.clone()
    sel = (torch.arange(n, device="cuda") % 3 == 0).to(torch.uint8)
    out = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
    value_lanes(rec, vh, sel=sel, out=out)                 # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        value_lanes(rec, vh, sel=sel, out=out)
    # changed records and a changed selection: the replay reads both anew
    rec.copy_(records1000.flip(0))
    sel.copy_((torch.arange(n, device="cuda") % 5 != 0).to(torch.uint8))
    out.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    eager = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
    value_lanes(rec, vh, sel=sel, out=eager)
    assert torch.equal(bits(out), bits(eager)) and int(torch.isnan(out).sum()) == 200


def test_refusals(records1000):
    from bgx import _lib
    from bgx.search import ValueHead, value_lanes
    from test_gpu_widths import _net
    L = _lib.load()
    vh = ValueHead(_net(40))
    rec, n = records1000, 1000
    out = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
    sel = torch.ones(n, dtype=torch.uint8, device="cuda")
    ok = [ptr(rec), n, ptr(vh.packed), 40, vh.bias, ptr(sel), ptr(out), stream()]
    assert L.bgx_value_lanes(*ok) == _lib.BGX_OK
    # argument index -> bad value: NULL records / pack / out, n, hidden, misaligned records
    for k, v in ((0, None), (1, 0), (1, -5), (2, None), (3, 0), (3, 129), (3, -1), (6, None),
                 (0, ctypes.c_void_p(rec.data_ptr() + 8))):
        a = list(ok)
        a[k] = v
        assert L.bgx_value_lanes(*a) == _lib.BGX_EINVAL, (k, v)
    # a NULL selection is every lane
    out.fill_(NAN)
    a = list(ok)
    a[5] = None
    assert L.bgx_value_lanes(*a) == _lib.BGX_OK and bool(torch.isfinite(out).all())
    # the wrapper's own checks
    for kw in (dict(sel=sel[:10]), dict(sel=sel.float()), dict(out=out.double()), dict(out=out[:5])):
        with pytest.raises(ValueError):
            value_lanes(rec, vh, **kw)
    with pytest.raises(ValueError):
        value_lanes(rec.cpu(), vh)
    with pytest.raises(ValueError):
        value_lanes(rec[:, :52], vh)
    torch.cuda.synchronize()


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


@pytest.mark.parametrize("H", [40, 128])
def test_no_move_lane_ties_the_two_lookaheads(H):
    """The mover on the bar against six closed entry points cannot move with any roll:
    bgx_roll_luck's mean (lookahead 1) is then the position's own value, within 1e-6 of
    bgx_value_lanes (lookahead 0) -- both sides, with and without checkers off."""
    import bgx
    from bgx.policy import PolicyNet
    from bgx.search import ValueHead, roll_luck, value_lanes
    torch.manual_seed(3)
    vh = ValueHead(PolicyNet(hidden_size=H).cuda())
    dance = [record({18: 5, 19: 5, 21: 4}, {**{24 + i: 2 for i in range(6)}, 24 + 12: 3}, 0, (3, 1), bar=(1, 0)),
             record({**{18 + i: 2 for i in range(6)}, 11: 3}, {24 + 5: 5, 24 + 4: 5, 24 + 2: 4}, 1, (6, 6), bar=(0, 1)),
             record({18: 4, 19: 5, 21: 2}, {**{24 + i: 2 for i in range(6)}}, 0, (4, 2), bar=(2, 0)),
             record({**{18 + i: 2 for i in range(6)}}, {24 + 5: 3, 24 + 1: 2}, 1, (2, 5), bar=(0, 3))]
    B = 64
    eng = bgx.Engine(batch=B, max_moves=500, dice="philox", seed=2, auto_reset=True)
    eng.reset()
    eng.set_lanes(torch.from_numpy(np.stack(dance)).cuda(), lane0=0, regen=True)
    assert eng.n_moves()[:4].tolist() == [0, 0, 0, 0]
    sel = torch.zeros(B, dtype=torch.uint8, device="cuda")
    sel[:4] = 1
    _, mean, stats = roll_luck(eng, vh, sel=sel)
    v = value_lanes(eng, vh, sel=sel)
    assert stats["rows"] == 4
    d = (mean[:4] - v[:4]).abs().max().item()
    print(f"[value_lanes] H={H}: max |roll_luck mean - value_lanes| on no-move lanes {d:.3e}")
    assert d < 1e-6 and bool(torch.isnan(v[4:]).all())
    # the engine's lanes read in place equal a copy of them
    assert torch.equal(bits(value_lanes(eng, vh)), bits(value_lanes(eng.records(), vh)))
