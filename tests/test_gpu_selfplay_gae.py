"""Zero-sum GAE(lambda) on the GPU (bgx_selfplay_gae + bgx_normalize_adv, bgx.train.selfplay_gae,
PPOTrainer(returns="selfplay"); DESIGN.md §6 "Self-play returns") against the fp64 recursion,
the existing lane-returns kernel, the torch loop on a real rollout, and through the trainer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SHAPES = [(1, 1), (2, 63), (7, 64), (33, 257), (33, 1000)]


@functools.lru_cache(maxsize=None)
def case(T, B):
    """Random rollout data of one shape (made once, never modified): rewards from the game's
    values and -1 mixed with randn, dones at p = 0.1 with some lanes forced done at t = 0
    and at t = T - 1, movers at p = 0.5 (same-mover transitions occur), randn values."""
    g = torch.Generator(device="cuda").manual_seed(1000 * T + B)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
    table = torch.tensor([0.0, 1.0, 1.5, 2.0, -1.0], device="cuda")
    r = table[(rnd(T, B) * 5).long().clamp(max=4)]
    r = torch.where(rnd(T, B) < 0.5, r, torch.randn(T, B, device="cuda", generator=g))
    d = rnd(T, B) < 0.1
    d[0, ::5] = True
    d[T - 1, 1::3] = True
    rec = (rnd(T, B, 64) * 256).to(torch.uint8)             # the other record bytes: noise
    rec[..., 52] = (rnd(T, B) < 0.5).to(torch.uint8)
    v = torch.randn(T, B, device="cuda", generator=g)
    bv = torch.randn(B, device="cuda", generator=g)
    brec = (rnd(B, 64) * 256).to(torch.uint8)
    brec[:, 52] = (rnd(B) < 0.5).to(torch.uint8)
    return r, d.to(torch.uint8), rec, v, bv, brec


@functools.lru_cache(maxsize=None)
def reference(T, B, boot, lam):
    """The fp64 recursion (with the fp32-rounded g and gl) and the derived error bound per
    lane: 8 T 2^-24 S, S = max_t (|r_t| + |v_t| + |v_{t+1}| + |A_{t+1}| + |A_t|)."""
    from bgx.train import _selfplay_gae_torch
    r, d, rec, v, bv, brec = case(T, B)
    A, ret = _selfplay_gae_torch(r.double(), d, rec, v.double(), bv.double() if boot else None,
                                 brec if boot else None, gamma=GAMMA, lam=lam, normalize=False)
    last_v = bv.double()[None] if boot else torch.zeros(1, B, dtype=torch.float64, device="cuda")
    vn = torch.cat([v.double()[1:], last_v])
    An = torch.cat([A[1:], torch.zeros(1, B, dtype=torch.float64, device="cuda")])
    S = (r.double().abs() + v.double().abs() + vn.abs() + An.abs() + A.abs()).max(0).values
    return A, ret, 8 * T * 2.0 ** -24 * S


def run_kernel(r, d, rec, v, bv, brec, g, gl, want_sums=True):
    """bgx_selfplay_gae through the C ABI: (status, adv, ret, sums)."""
    from bgx import _lib
    L = _lib.load()
    T, B = r.shape
    adv, ret = torch.full_like(r, 7.0), torch.full_like(r, 7.0)
    sums = torch.full((3,), 7.0, dtype=torch.float64, device="cuda") if want_sums else None
    ws = torch.empty(max(int(L.bgx_selfplay_gae_workspace(B)) // 8, 1), dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = L.bgx_selfplay_gae(p(r), p(d), p(rec), p(v), p(bv), p(brec), T, B, g, gl, p(adv), p(ret), p(ws), p(sums),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, adv, ret, sums


@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("boot", [True, False])
@pytest.mark.parametrize("T,B", SHAPES)
def test_kernel_matches_fp64_recursion(T, B, boot, lam):
    from bgx.train import _gae_scalars, selfplay_gae
    r, d, rec, v, bv, brec = case(T, B)
    A64, ret64, bound = reference(T, B, boot, lam)
    adv, ret = selfplay_gae(r, d, rec, v, bv if boot else None, brec if boot else None, gamma=GAMMA, lam=lam,
                            normalize=False)
    ea = (adv.double() - A64).abs()
    er = (ret.double() - ret64).abs()
    print(f"T={T} B={B} boot={boot} lam={lam}: max err adv {float(ea.max()):.3g} ret {float(er.max()):.3g} "
          f"min bound {float(bound.min()):.3g}")
    assert bool((ea <= bound[None]).all()) and bool((er <= bound[None]).all())
    # the sums of the kernel's own A, in fp64, identical from call to call
    g, gl = _gae_scalars(GAMMA, lam)
    rc, adv2, ret2, sums = run_kernel(r, d, rec, v, bv if boot else None, brec if boot else None, g, gl)
    assert rc == 0 and torch.equal(adv2, adv) and torch.equal(ret2, ret)
    a = adv.double().reshape(-1)
    N = T * B
    assert float(sums[2]) == N
    assert abs(float(sums[0]) - float(a.sum())) <= N * 2.0 ** -52 * float(a.abs().sum())
    assert abs(float(sums[1]) - float((a * a).sum())) <= N * 2.0 ** -52 * float((a * a).sum())
    assert torch.equal(run_kernel(r, d, rec, v, bv if boot else None, brec if boot else None, g, gl)[3], sums)


@pytest.mark.parametrize("T,B", [(33, 257), (33, 1000)])
def test_reduces_to_lane_returns_kernel(T, B):
    """Zero values, one mover, lambda = 1, no bootstrap: bit-identical to bgx_lane_returns
    on arbitrary fp32 rewards (both round r + g R as a product and a sum)."""
    from bgx.train import lane_returns, selfplay_gae
    r, d, rec, *_ = case(T, B)
    rec1 = rec.clone()
    rec1[..., 52] = 1
    adv, ret = selfplay_gae(r, d, rec1, torch.zeros_like(r), gamma=GAMMA, lam=1.0, normalize=False)
    want = lane_returns(r, d, GAMMA)
    assert torch.equal(ret, want) and torch.equal(adv, want)


def test_normalize_matches_global_normalize():
    from bgx.ppo import global_normalize
    from bgx.train import selfplay_gae
    r, d, rec, v, bv, brec = case(33, 1000)
    A, ret = selfplay_gae(r, d, rec, v, bv, brec, normalize=False)
    An, ret2 = selfplay_gae(r, d, rec, v, bv, brec)
    assert torch.equal(ret, ret2)
    err = float((An - global_normalize(A.reshape(-1)).view_as(A)).abs().max())
    print("normalised adv: max |err|", err)
    assert err <= 1e-5
    # a misaligned view takes the kernel's scalar path: the same numbers
    from bgx import _lib
    buf = torch.empty(A.numel() + 1, device="cuda")
    buf[1:] = A.reshape(-1)
    sums = torch.stack([A.double().sum(), (A.double() ** 2).sum(),
                        torch.tensor(float(A.numel()), dtype=torch.float64, device="cuda")])
    rc = _lib.load().bgx_normalize_adv(ctypes.c_void_p(buf.data_ptr() + 4), A.numel(), ctypes.c_void_p(sums.data_ptr()),
                                       1e-5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and float((buf[1:] - An.reshape(-1)).abs().max()) <= 1e-6


def test_abi_rejects_bad_arguments():
    """Each BGX_EINVAL case returns BGX_EINVAL and launches nothing (the outputs keep their fill)."""
    from bgx import _lib
    from bgx.train import _gae_scalars
    r, d, rec, v, bv, brec = case(7, 64)
    g, gl = _gae_scalars(GAMMA, 0.95)
    L = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    adv, ret = torch.full_like(r, 7.0), torch.full_like(r, 7.0)
    sums = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(L.bgx_selfplay_gae_workspace(64)) // 8, 1), dtype=torch.float64, device="cuda")
    good = dict(r=r, d=d, rec=rec, v=v, bv=bv, brec=brec, T=7, B=64, adv=adv, ret=ret)
    bad = [dict(T=0), dict(T=-1), dict(B=0), dict(B=-3), dict(r=None), dict(d=None), dict(rec=None), dict(v=None),
           dict(adv=None), dict(ret=None), dict(bv=None), dict(brec=None)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for change in bad:
        a = dict(good, **change)
        rc = L.bgx_selfplay_gae(p(a["r"]), p(a["d"]), p(a["rec"]), p(a["v"]), p(a["bv"]), p(a["brec"]), a["T"], a["B"],
                                g, gl, p(a["adv"]), p(a["ret"]), p(ws), p(sums), s)
        assert rc == _lib.BGX_EINVAL, change
    assert L.bgx_selfplay_gae(p(r), p(d), p(rec), p(v), p(bv), p(brec), 7, 64, g, gl, p(adv), p(ret), None, p(sums),
                              s) == _lib.BGX_EINVAL                        # sums without a workspace
    assert L.bgx_selfplay_gae_workspace(-1) == _lib.BGX_EINVAL
    for n, a_, s_ in ((0, adv, sums), (-1, adv, sums), (8, None, sums), (8, adv, None)):
        assert L.bgx_normalize_adv(p(a_), n, p(s_), 1e-5, s) == _lib.BGX_EINVAL
    torch.cuda.synchronize()
    assert bool((adv == 7.0).all()) and bool((ret == 7.0).all()) and bool((sums == 7.0).all())
    with pytest.raises(ValueError):
        from bgx.train import selfplay_gae
        selfplay_gae(r, d, rec, v, boot_values=bv)


@pytest.fixture(scope="module")
def rolled():
    """A selfplay-mode trainer rolled until its window holds a game end, and how often."""
    from bgx.train import PPOTrainer
    tr = PPOTrainer(batch=4096, horizon=16, seed=2, returns="selfplay")
    n = 0
    for _ in range(12):                  # games last ~60 plies: roll on until some end in the window
        tr.rollout()
        n += 1
        if int(tr.buf["dones"].sum()) > 0:
            break
    assert int(tr.buf["dones"].sum()) > 0
    return tr, n


def test_real_rollout_matches_torch_loop(rolled):
    """On a real rollout (rewards multiples of 1/2 at game ends) the kernel equals the torch
    loop bit for bit; the bootstrap is the value and the mover of the engines' lanes as the
    rollout left them."""
    from bgx.ppo import global_normalize
    from bgx.train import _selfplay_gae_torch, selfplay_gae
    tr, _ = rolled
    b = tr.buf
    args = (b["rewards"], b["dones"], b["records"], b["values"], b["boot_values"], b["boot_records"])
    adv, ret = selfplay_gae(*args, normalize=False)
    adv_t, ret_t = _selfplay_gae_torch(*args, normalize=False)
    assert torch.equal(adv, adv_t) and torch.equal(ret, ret_t)
    _, _, val = tr.net.act(tr.eng, greedy=True)
    assert torch.equal(b["boot_values"], val)
    assert torch.equal(b["boot_records"], tr.eng.records())
    assert torch.equal(b["boot_records"][:, 52], tr.eng.records()[:, 52])
    # the normalised advantages as torch's
    An, _ = selfplay_gae(*args)
    err = float((An - global_normalize(adv.reshape(-1)).view_as(adv)).abs().max())
    print("real rollout, normalised adv: max |err|", err)
    assert err <= 1e-5


def test_bootstrap_pass_leaves_the_rollout_alone(rolled):
    """A returns="lane" trainer with the same seed, rolled as often (the first rollout
    eager, the later ones replayed graphs), holds bitwise-equal rollout buffers."""
    from bgx.train import PPOTrainer
    tr, n = rolled
    ref = PPOTrainer(batch=4096, horizon=16, seed=2, returns="lane")
    for _ in range(n):
        ref.rollout()
    assert "boot_values" not in ref.buf
    assert ref.step_counter == tr.step_counter
    for k in ("records", "actions", "logp", "values", "rewards", "dones"):
        assert torch.equal(ref.buf[k], tr.buf[k]), k


@pytest.mark.parametrize("kw", [dict(batch=256, horizon=8, shards=1), dict(batch=2048, horizon=4, chunk=4096)])
def test_trainer_iterations(kw):
    """Two iterations in selfplay mode: finite loss parts, weights move, and the update's
    graph is captured exactly as in lane mode (the returns are formed before the epochs)."""
    from bgx.train import PPOTrainer
    trs = {mode: PPOTrainer(seed=4, returns=mode, **kw) for mode in ("selfplay", "lane")}
    w0 = [p.detach().clone() for p in trs["selfplay"].net.parameters()]
    for mode, tr in trs.items():
        for _ in range(2):
            m = tr.iteration()
            for k in ("policy_loss", "value_loss", "entropy", "total_loss"):
                assert np.isfinite(m[k]), (mode, k, m)
    sp, ln = trs["selfplay"], trs["lane"]
    assert any(not torch.equal(a, b) for a, b in zip(w0, sp.net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in sp.net.parameters())
    assert sp._ugraph_captures == ln._ugraph_captures
    assert (sp._ugraph is None) == (ln._ugraph is None)
    if kw["batch"] == 2048:
        assert sp._ugraph is not None and sp._ugraph_captures >= 1     # the second update ran the graphed epoch


def test_load_rollout_bootstrap():
    """load_rollout without a bootstrap makes the horizon a cut; with one, update() uses it."""
    from bgx.train import PPOTrainer
    tr = PPOTrainer(batch=256, horizon=8, seed=1, shards=1, returns="selfplay")
    tr.rollout()
    b = {k: v.clone() for k, v in tr.buf.items()}
    six = [b[k] for k in ("records", "actions", "logp", "values", "rewards", "dones")]
    tr.load_rollout(*six)
    assert tr._boot is False
    tr.load_rollout(*six, boot_values=b["boot_values"], boot_records=b["boot_records"])
    assert tr._boot is True and torch.equal(tr.buf["boot_values"], b["boot_values"])
    with pytest.raises(ValueError):
        tr.load_rollout(*six, boot_values=b["boot_values"])
    m = tr.update()
    assert np.isfinite(m["total_loss"])
