"""The fused fp16 output layer + loss head (csrc/bg_ppo_fused.hip: bgx_ppo_rows,
bgx_ppo_gw2): every element against fp64 from the same fp16 operands (the loss head's closed
form head64 of tests/ppo_head_ref.py, pinned to torch autograd by test_ppo_head_ref_cpu.py),
on a real rollout and on synthetic rows that reach every clip and clamp case; and against the
round-2 composition it replaces, on a real rollout: hipBLASLt logits y = h W2h^T + b2h, the
loss-head kernel bgx_ppo_head_ex (checked element by element against the same closed form by
test_gpu_ppo_head.py; test_gpu_train.py compares only the parameter gradients behind it with
torch autograd), dh = ReLU'(h) fp16(dy W2h), gW2 = dy^T h, gb2 = column sums of dy
(ppo_agent.py:268-305 under autocast)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ppo_head_ref import EPS_CLIP, LOG_EPS, U32, head64, ratio_fields, records_of, ulp16

pytestmark = pytest.mark.gpu


def _setup(seed=7, batch=4096, horizon=8):
    from bgx.train import PPOTrainer, lane_returns
    from bgx.ppo import global_normalize
    tr = PPOTrainer(batch=batch, horizon=horizon, seed=seed)
    tr.rollout()
    b = tr.buf
    R = global_normalize(lane_returns(b["rewards"], b["dones"]).reshape(-1)).contiguous()
    adv = (R - b["values"].reshape(-1)).contiguous()
    recs = b["records"].reshape(-1, 64).contiguous()
    acts = b["actions"].reshape(-1).to(torch.int32).contiguous()
    old = b["logp"].reshape(-1).contiguous()
    net = tr.net
    A, Hd = net.action_head.weight.shape
    W2h = torch.zeros(512, Hd, dtype=torch.float16, device="cuda")
    b2h = torch.zeros(512, dtype=torch.float16, device="cuda")
    with torch.no_grad():
        W2h[:A] = net.action_head.weight.half(); W2h[A] = net.value_head.weight[0].half()
        b2h[:A] = net.action_head.bias.half(); b2h[A] = net.value_head.bias[0].half()
        from bgx.engine import encode_records
        h = torch.relu(F.linear(encode_records(recs, torch.float16), net.fc1.weight.half(), net.fc1.bias.half()))
    _setup.net = net
    return recs, acts, old, R, adv, W2h, b2h, h.contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _fused(recs, acts, old, R, adv, W2h, b2h, h, coefs, perm, plan, row_plan, want_dy=True, want_z=False):
    from bgx import _lib
    from bgx._lib import check
    L = _lib.load()
    m = recs.shape[0]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dh = torch.empty(m, 128, dtype=torch.float16, device="cuda")
    stats = torch.empty(m, 4, dtype=torch.float32, device="cuda")
    info = torch.empty(m, dtype=torch.int32, device="cuda")
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    dy = torch.full((m, 512), float("nan"), dtype=torch.float16, device="cuda") if want_dy else None
    z = torch.full((m, 512), float("nan"), dtype=torch.float16, device="cuda") if want_z else None
    eps, cv, ce, gs = coefs
    check(L.bgx_ppo_rows(_p(h), _p(perm), _p(recs), _p(acts), _p(old), _p(R), _p(adv), m, 128, 500, _p(W2h), _p(b2h),
                         eps, cv, ce, gs, _p(dh), _p(stats), _p(info), _p(sums), _p(dy), _p(z), _p(row_plan), 0, s),
          "bgx_ppo_rows")
    gw2 = torch.zeros(512, 128, dtype=torch.float32, device="cuda")
    gb2 = torch.zeros(512, dtype=torch.float32, device="cuda")
    ws = torch.empty(L.bgx_ppo_gw2_workspace(m) // 4, dtype=torch.float32, device="cuda")
    k1 = float(np.float32(gs) * np.float32(ce))
    check(L.bgx_ppo_gw2(_p(h), _p(perm), _p(stats), _p(info), m, 128, 500, _p(W2h), _p(b2h), k1, _p(plan), _p(ws),
                        _p(gw2), _p(gb2), s), "bgx_ppo_gw2")
    torch.cuda.synchronize()
    if want_z:
        return dh, dy, gw2, gb2, sums, z
    return dh, dy, gw2, gb2, sums


def _reference(recs, acts, old, R, adv, W2h, b2h, h, coefs):
    from bgx import _lib
    from bgx._lib import check
    L = _lib.load()
    m = recs.shape[0]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = F.linear(h, W2h, b2h).contiguous()
    vals = y[:, 500].contiguous()
    dy = torch.empty_like(y)
    dval = torch.empty_like(vals)
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    colsum = torch.empty(2048, 512, dtype=torch.float32, device="cuda")
    eps, cv, ce, gs = coefs
    check(L.bgx_ppo_head_ex(_p(y), 1, 512, _p(vals), _p(recs), _p(acts), _p(old), _p(R), _p(adv), m, 500, eps, cv, ce,
                            gs, _p(dy), 512, _p(dval), _p(sums), 1, _p(colsum), s), "bgx_ppo_head_ex")
    dh = (dy @ W2h) * (h > 0)
    gw2 = dy.float().t() @ h.float()
    gb2 = dy.float().sum(0)
    torch.cuda.synchronize()
    return dh, dy, gw2, gb2, sums


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


COEFS = (0.25, 0.5, 0.15, 16.0)      # eps_clip, value coef, entropy coef, per-row gradient scale


def _head64(z, recs, acts, old, R, adv, coefs, wide=False):
    """The loss head's dL/dy in fp64 from the kernel's own fp16 logits z ([c, 512]) in the
    [dlogits | dvalue | 0] layout: head64(drop_masked=True) of tests/ppo_head_ref.py.
    Returns (d64 [c, 512], d_alt, tol [c, 512], row sums (pol, dv^2, ent) [c, 3]).  tol = the
    fp32 rounding budget of the kernel's terms; where a log-prob lies on a clamp bound (within
    the fp32 error of its computation) either side is accepted (`d_alt`)."""
    cnt = recs[:, 60].long() | (recs[:, 61].long() << 8)
    ref = head64(z, z[:, 500], cnt, acts, old, R, adv, coefs, 500, drop_masked=True, wide=wide)
    c = z.shape[0]
    d, d_alt, tol = (torch.zeros(c, 512, dtype=torch.float64, device=z.device) for _ in range(3))
    d[:, :500], d_alt[:, :500], tol[:, :500] = ref.d, ref.d_alt, ref.tol
    d[:, 500] = d_alt[:, 500] = ref.gv
    tol[:, 500] = ref.tol_v
    return d, d_alt, tol, ref.rows


CHUNK = 1 << 17


def _check_fused_vs_fp64(args, coefs, out, wide=False):
    """Every output of bgx_ppo_rows / bgx_ppo_gw2 (`out` = _fused(..., want_z=True)) against
    an fp64 recompute from the same fp16 operands, in chunks of CHUNK rows: z, dy on the
    kernel's own z, dh on the kernel's dy, gW2 / gb2 against fp64 dy^T [h | 1], the loss sums,
    exact zeros on masked columns (the bounds are those of test_fused_head_elementwise_vs_fp64's
    docstring; `wide`: the loss head's budget follows the fp32 resolution of each row's
    log-probs, ppo_head_ref.head64).  Returns the worst error / tolerance per quantity."""
    recs, acts, old, R, adv, W2h, b2h, h = args
    dh, dy, gw2, gb2, sums, z = out
    m = recs.shape[0]
    W = W2h.double()
    sums64 = torch.zeros(3, dtype=torch.float64, device="cuda")
    worst = {}

    def note(name, err, tol):
        r = float((err / tol).max()) if err.numel() else 0.0
        worst[name] = max(worst.get(name, 0.0), r)

    for s0 in range(0, m, CHUNK):
        sl = slice(s0, min(m, s0 + CHUNK))
        zc, dyc, dhc, hc = z[sl], dy[sl], dh[sl], h[sl]
        cnt = recs[sl, 60].long() | (recs[sl, 61].long() << 8)
        lim = torch.where(cnt == 0, torch.full_like(cnt, 500), cnt.clamp(max=500))
        cols = torch.arange(512, device="cuda")[None, :]
        need = (cols < lim[:, None]) | (cols == 500)
        # z: every column a row needs was computed, within one ulp of fp64
        assert not torch.isnan(zc[need]).any()
        z64 = hc.double() @ W.t() + b2h.double()
        zb = hc.double().abs() @ W.abs().t() + b2h.double().abs()
        zt = ulp16(z64) + 130 * U32 * zb
        ez = torch.where(need, (zc.double() - z64).abs(), torch.zeros_like(z64))
        note("z", ez[need], zt[need])
        assert bool((ez <= zt).all()), float((ez / zt).max())
        # dy on the kernel's z
        d64, dalt, dt, rs = _head64(zc, recs[sl], acts[sl], old[sl], R[sl], adv[sl], coefs, wide)
        sums64 += rs.sum(0)
        tol = ulp16(d64) + dt
        e = torch.minimum((dyc.double() - d64).abs(), (dyc.double() - dalt).abs())
        note("dy", e, tol)
        assert bool((e <= tol).all()), float((e / tol).max())
        # dh on the kernel's dy
        dh64 = (dyc.double() @ W) * (hc > 0)
        db = dyc.double().abs() @ W.abs()
        eh = (dhc.double() - dh64).abs()
        th = ulp16(dh64) + 512 * U32 * db
        note("dh", eh, th)
        assert bool((eh <= th).all()), float((eh / th).max())
        assert bool((dhc[hc <= 0] == 0).all())
    # gW2 / gb2: fp64 dy^T [h | 1] on the rows kernel's dy
    g64 = dy.double().t() @ h.double()
    gabs = dy.double().abs().t() @ h.double().abs()
    b64 = dy.double().sum(0)
    babs = dy.double().abs().sum(0)
    eg = (gw2.double() - g64).abs()
    tg = (1024 + 2048 + 64) * U32 * gabs + 1e-30
    note("gW2", eg, tg)
    assert bool((eg <= tg).all()), float((eg / tg).max())
    eb = (gb2.double() - b64).abs()
    assert bool((eb <= (1024 + 2048 + 64) * U32 * babs + 1e-30).all())
    colnorm = g64.norm(dim=1)
    live = colnorm > 0
    colrel = (gw2.double() - g64).norm(dim=1)[live] / colnorm[live]
    worst["gW2_column_rel"] = float(colrel.max())
    assert float(colrel.max()) < 1e-5, float(colrel.max())
    assert bool((gw2[~live] == 0).all())
    # the loss sums (fp32 per lane, fp64 across lanes) against the fp64 per-row recompute
    assert torch.allclose(sums, sums64, rtol=1e-6, atol=1e-6 * m), (sums, sums64)
    # masked columns (past the legal count of a row with legal moves) get exactly 0
    cnt = recs[:, 60].int() | (recs[:, 61].int() << 8)
    cols = torch.arange(500, device="cuda")[None, :]
    masked = (cols >= cnt[:, None]) & (cnt[:, None] > 0)
    assert bool((dy[:, :500][masked] == 0).all())
    assert bool((dy[:, 501:] == 0).all())
    return worst


def test_fused_head_elementwise_vs_fp64():
    """bgx_ppo_rows / bgx_ppo_gw2 at 2^21 rows (a 65,536 x 32 rollout, the production
    launch layout: k_ppo_rows<1/2/4/16> at 2-4 waves per SIMD), every element against
    an fp64 recompute from the same fp16 operands:
      * z (the fp16 logits, test output): within one fp16 ulp of fp64 h W2h^T + b2h
        (+ the fp32 accumulation budget 130 u sum|terms|);
      * dy: within one fp16 ulp of the loss head's dL/dy evaluated in fp64 on the
        kernel's own z (+ the fp32 budget of its terms, _head64);
      * dh: within one fp16 ulp of fp64 (dy W2h) on the kernel's dy (+ 512 u
        sum|dy||W2h|), exactly 0 where h <= 0;
      * gW2 / gb2 (k_ppo_gw2, dz recomputed from the row statistics): every element within
        (1024 + 2048 + 64) u sum_rows |dy||h| of fp64 dy^T [h | 1] -- the kernel's
        summation chain (1,024-row tasks, fixed-order partial sums) -- and every action
        column's (= k_ppo_gw2 lane's) relative error below 1e-5;
      * the loss sums within 1e-6 relative of their fp64 recompute.
    Round 4's evaluator fault (0.01-0.8 % of items wrong by up to 5 %, confined to 16
    lanes) fails every one of these."""
    from bgx.train import ppo_row_plan
    args = _setup(batch=65536, horizon=32)
    recs = args[0]
    m = recs.shape[0]
    assert m == 1 << 21
    perm, plan, row_plan = ppo_row_plan(recs)
    out = _fused(*args, COEFS, perm, plan, row_plan, want_z=True)
    worst = _check_fused_vs_fp64(args, COEFS, out)
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


SYN_COUNTS = (0, 1, 31, 32, 33, 64, 65, 128, 129, 499, 500, 600)   # every row-plan class and its edges
SYN_LOW_COL = 3


def _synthetic(m=4099, seed=11):
    """Epoch 2-4 rows for the fused head, which takes h and W2h, not logits:
      * h = relu(randn) * {0.8, 1.25} per row (fp16), W2h ~ N(0, 0.12^2), b2h ~ N(0, 0.5^2):
        logits of std ~ 0.8-1.2, the most the shortcut's own precondition leaves room for
        beside one bias of -13 (column SYN_LOW_COL), which makes that column's probability
        fall below eps wherever more than a few columns are legal;
      * legal counts from SYN_COUNTS; the action is the row's least likely legal one on a
        quarter of the rows, the most likely on a quarter, uniform on the rest; an eighth of
        the rows with 0 < cnt < 500 take a masked action cnt <= act < 500 instead;
      * advantage and ratio target per row as ppo_head_ref.synthetic_rows; old_logp =
        fp32(la64 - log target) with la64 from the fp64 logits of the fp16 operands.
    Returns (args for _fused, pick [m]: 0 least likely, 1 most likely, 2-3 uniform, 4 masked)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.8, 1.25])[torch.randint(0, 2, (m,), generator=g)]
    h = (torch.relu(torch.randn(m, 128, generator=g)) * scale[:, None]).half()
    W2h = torch.zeros(512, 128)
    W2h[:501] = torch.randn(501, 128, generator=g) * 0.12
    b2h = torch.zeros(512)
    b2h[:501] = torch.randn(501, generator=g) * 0.5
    b2h[SYN_LOW_COL] = -13.0
    W2h, b2h = W2h.half(), b2h.half()
    cnt = torch.tensor(SYN_COUNTS)[torch.randint(0, len(SYN_COUNTS), (m,), generator=g)]
    lim = torch.where(cnt == 0, torch.tensor(500), cnt.clamp(max=500))
    z64 = h.double() @ W2h.double().t() + b2h.double()
    zl = torch.where(torch.arange(512)[None] < lim[:, None], z64, torch.full_like(z64, float("nan")))
    pick = torch.randint(0, 4, (m,), generator=g)
    act = (torch.rand(m, generator=g) * lim).long().clamp(max=499)
    act = torch.where(pick == 0, torch.nan_to_num(zl, nan=float("inf")).argmin(1), act)
    act = torch.where(pick == 1, torch.nan_to_num(zl, nan=float("-inf")).argmax(1), act)
    msk = (torch.randint(0, 8, (m,), generator=g) == 0) & (cnt > 0) & (cnt < 500)
    mact = (cnt + ((500 - cnt).double() * torch.rand(m, generator=g).double()).long()).clamp(max=499)
    act = torch.where(msk, mact, act)
    pick = torch.where(msk, torch.full_like(pick, 4), pick)
    R = torch.randn(m, generator=g)
    adv, tgt = ratio_fields(m, g)
    la = head64(z64, z64[:, 500], cnt, act, torch.zeros(m), R, adv, COEFS, 500, drop_masked=True).la
    old = (la - tgt.log()).float()
    args = (records_of(cnt), act.to(torch.int32), old, R, adv, W2h, b2h, h)
    return tuple(t.cuda().contiguous() for t in args), pick.cuda()


@pytest.mark.parametrize("order", ["plan", "shuffled"])
def test_fused_head_synthetic_rows_vs_fp64(order):
    """bgx_ppo_rows + bgx_ppo_gw2 at m = 4099 on rows as epochs 2-4 of an update see them
    (_synthetic), every element against fp64 as in test_fused_head_elementwise_vs_fp64:
      * ratio targets 0.5 / 2.0 with either sign of the advantage run the clipped branches
        (w1, w2) and put clipped rows into the statistics k_ppo_gw2 rebuilds dy from; 0.9 / 1.1
        the inside branch; 1.0 and advantage 0 the tie s1 == s2;
      * least likely actions: the lower clamp on the action (la = log eps, no policy gradient);
        most likely actions with cnt = 1: the upper clamp;
      * masked actions (cnt <= act < 500, cnt > 0), in a computed tile, in a skipped tile and in
        the value tile: la = log eps, zero policy gradient, no one-hot term, as head64 defines;
      * counts 0 / 1 / 31..33 / 64, 65 / 128, 129 / 499, 500, 600: every k_ppo_rows variant and
        the edges of its tile count; m = 4099 leaves a partial last row tile.
    `plan`: ppo_row_plan's order and plan; `shuffled`: a random order with the plan for it
    (every row tile through the 16-tile variant, every action tile visiting every row), which
    the header allows.  Measured on the MI355X, worst error / tolerance, either order: z 0.49,
    dy 0.50 (the fp16 rounding: no clamp decided the other way), dh 0.48, gW2 0.005, its
    columns' relative error within the 1e-5 bound.  No kernel fault found: a masked chosen
    action already follows head64."""
    from bgx.ppo_epoch import MASK_SHORTCUT_LIMIT
    from bgx.train import ppo_row_plan
    args, pick = _synthetic()
    recs, acts, old, R, adv, W2h, b2h, h = args
    m = recs.shape[0]
    # the shortcut's own precondition (bgx.ppo_epoch._ppo_epoch_amp_fused's guard)
    U = W2h[:500].float().norm(dim=1).max() * h.float().norm(dim=1).max() + b2h[:500].float().abs().max()
    assert 2.0 * float(U) < MASK_SHORTCUT_LIMIT, float(U)
    if order == "plan":
        perm, plan, row_plan = ppo_row_plan(recs)
    else:
        g = torch.Generator().manual_seed(5)
        perm = torch.randperm(m, generator=g).to(torch.int32).cuda()
        ntiles = (m + 31) // 32
        tasks = (ntiles + 31) // 32
        plan = torch.tensor([tasks * i for i in range(17)] + [0] * 16, dtype=torch.int32, device="cuda")
        row_plan = torch.tensor([0, 0, 0, 0, 0, 0, 0, ntiles], dtype=torch.int32, device="cuda")
    out = _fused(*args, COEFS, perm, plan, row_plan, want_z=True)
    dy, z = out[1], out[5]
    # the branches, from the reference on the kernel's own logits
    cnt = recs[:, 60].long() | (recs[:, 61].long() << 8)
    ref = head64(z, z[:, 500], cnt, acts, old, R, adv, COEFS, 500, drop_masked=True)
    assert not bool(ref.near_clip.any())
    rcls = torch.where(ref.rt < 1 - EPS_CLIP, 0, torch.where(ref.rt > 1 + EPS_CLIP, 2, 1))
    cells = torch.bincount(rcls * 3 + torch.sign(adv).long() + 1, minlength=9)
    assert int(cells.min()) >= 20, cells
    legal = acts.long() < ref.lim
    assert int(((pick == 0) & legal & (ref.ua < LOG_EPS)).sum()) >= 20
    assert int((ref.ua > -1.1920930376163597e-07).sum()) >= 20
    masked_act = ~legal
    assert int(masked_act.sum()) >= 20 and bool((pick[masked_act] == 4).all())
    worst = _check_fused_vs_fp64(args, COEFS, out, wide=True)
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})
    # a masked chosen action: no one-hot term (its column is exactly 0), la = log eps in the ratio
    rows = torch.nonzero(masked_act)[:, 0]
    assert bool((dy[rows, acts[rows].long()] == 0).all())
    assert bool((ref.la[masked_act] == LOG_EPS).all())


def test_fused_head_matches_round2_composition():
    """The fused head against the round-2 composition it replaced (hipBLASLt logits +
    bgx_ppo_head_ex + torch GEMMs) on a 4,096 x 8 rollout: the same formulas, so the
    loss sums agree to 1e-5 and the gradients to 2e-3 relative (an fp16 logit may round
    the other way where the two fp32 sums differ; the element-wise gate is
    test_fused_head_elementwise_vs_fp64)."""
    from bgx.train import ppo_row_plan
    args = _setup()
    recs = args[0]
    perm, plan, row_plan = ppo_row_plan(recs)
    dh, dy, gw2, gb2, sums = _fused(*args, COEFS, perm, plan, row_plan)
    rdh, rdy, rgw2, rgb2, rsums = _reference(*args, COEFS)
    m = recs.shape[0]
    assert torch.allclose(sums / m, rsums / m, rtol=1e-5, atol=1e-6), (sums / m, rsums / m)
    assert not torch.isnan(dy).any()
    assert _rel(dy, rdy) < 2e-3
    assert _rel(dh, rdh) < 2e-3
    assert _rel(gw2, rgw2) < 2e-3 and _rel(gb2, rgb2) < 2e-3


def test_fc1_and_gw1_elementwise_vs_fp64():
    """The fused epoch's other two kernels at 2^21 rows (a 65,536 x 32 rollout), every
    element against fp64 from the same fp16 operands:
      * h = bgx_fc1_records_ex (fc1 forward from the records, 8-wave workgroups at
        4 waves/SIMD): within one fp16 ulp of fp64 relu(x W1h^T + b1h), x the G2-pinned
        fp16 features (+ the fp32 accumulation budget 200 u sum|terms|);
      * gW1 / gb1 = bgx_ppo_gw1 on the rows kernel's dh (features generated on chip):
        every element within (4096 + 64) u sum_rows |dh||x| of fp64 dh^T [x | 1] -- the
        kernel's chain (4,096 rows per workgroup, fixed-order partial sums) -- every
        hidden unit's and every feature column's relative error below 1e-5, and the 9
        padding columns exactly 0."""
    from bgx import _lib
    from bgx._lib import check
    from bgx.engine import encode_records
    from bgx.train import ppo_row_plan
    L = _lib.load()
    args = _setup(seed=11, batch=65536, horizon=32)
    recs = args[0]
    net = _setup.net
    m = recs.shape[0]
    assert m == 1 << 21
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    W1h, b1h = net.fc1.weight.detach().half().contiguous(), net.fc1.bias.detach().half().contiguous()
    pk = torch.empty(L.bgx_fc1_packed_size(128), dtype=torch.uint8, device="cuda")
    check(L.bgx_fc1_pack(_p(W1h), 128, _p(pk), s), "bgx_fc1_pack")
    h = torch.full((m, 128), float("nan"), dtype=torch.float16, device="cuda")
    hmax2 = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(L.bgx_fc1_records_ex(_p(recs), m, _p(pk), _p(b1h), 128, _p(h), _p(hmax2), s), "bgx_fc1_records_ex")
    torch.cuda.synchronize()
    W = W1h.double()
    worst = {}
    g64 = torch.zeros(128, 208, dtype=torch.float64, device="cuda")
    gabs = torch.zeros_like(g64)
    for s0 in range(0, m, CHUNK):
        sl = slice(s0, min(m, s0 + CHUNK))
        x = encode_records(recs[sl], torch.float16).double()
        pre = x @ W.t() + b1h.double()
        h64 = pre.clamp(min=0)
        tb = x.abs() @ W.abs().t() + b1h.double().abs()
        e = (h[sl].double() - h64).abs()
        t = ulp16(h64) + 200 * U32 * tb
        worst["h"] = max(worst.get("h", 0.0), float((e / t).max()))
        assert bool((e <= t).all()), float((e / t).max())
    hm = float((h.double() ** 2).sum(1).max())
    assert abs(float(hmax2[0]) - hm) <= 1e-5 * hm
    # dh from the rows kernel on the kernel's h, then gW1
    recs_, acts, old, R, adv, W2h, b2h, _ = args
    perm, plan, row_plan = ppo_row_plan(recs)
    dh = _fused(recs, acts, old, R, adv, W2h, b2h, h, COEFS, perm, plan, row_plan, want_dy=False)[0]
    gw1 = torch.zeros(128, 208, dtype=torch.float32, device="cuda")
    ws = torch.empty(L.bgx_ppo_gw1_workspace(m) // 4, dtype=torch.float32, device="cuda")
    check(L.bgx_ppo_gw1(_p(dh), _p(recs), m, 128, _p(ws), _p(gw1), s), "bgx_ppo_gw1")
    torch.cuda.synchronize()
    for s0 in range(0, m, CHUNK):
        sl = slice(s0, min(m, s0 + CHUNK))
        x = torch.zeros(sl.stop - sl.start, 208, dtype=torch.float64, device="cuda")
        x[:, :198] = encode_records(recs[sl], torch.float16).double()
        x[:, 198] = 1.0
        d = dh[sl].double()
        g64 += d.t() @ x
        gabs += d.abs().t() @ x.abs()
    e = (gw1.double() - g64).abs()
    t = (4096 + 64) * U32 * gabs + 1e-30
    worst["gW1"] = float((e / t).max())
    assert bool((e <= t).all()), float((e / t).max())
    assert bool((gw1[:, 199:] == 0).all())
    for dim, name in ((1, "gW1_unit_rel"), (0, "gW1_column_rel")):
        n = g64.norm(dim=dim)
        live = n > 0
        rel = (gw1.double() - g64).norm(dim=dim)[live] / n[live]
        worst[name] = float(rel.max())
        assert float(rel.max()) < 1e-5, (name, float(rel.max()))
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


def test_fused_head_row_order_invariant():
    """Any row order gives the same dy / dh (per-row work) and the same gW2 up to
    the fp32 summation order: the sort only schedules."""
    from bgx.train import ppo_row_plan
    args = _setup(seed=3, batch=2048, horizon=5)
    recs = args[0]
    m = recs.shape[0]
    perm, plan, row_plan = ppo_row_plan(recs)
    a = _fused(*args, COEFS, perm, plan, row_plan)
    ident = torch.arange(m, dtype=torch.int32, device="cuda")
    ntiles = (m + 31) // 32
    tasks = (ntiles + 31) // 32
    plan2 = torch.tensor([tasks * i for i in range(17)] + [0] * 16, dtype=torch.int32, device="cuda")
    rev = torch.flip(ident, [0]).contiguous()
    # unsorted rows: every row tile through the 16-tile variant
    rp2 = torch.tensor([0, 0, 0, 0, 0, 0, 0, ntiles], dtype=torch.int32, device="cuda")
    for p2 in (ident, rev):
        b = _fused(*args, COEFS, p2, plan2, rp2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert _rel(b[2], a[2]) < 1e-6 and _rel(b[3], a[3]) < 1e-6
        assert torch.allclose(a[4] / m, b[4] / m, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("m", [33, 4096 * 8 - 5, 1 << 18])
def test_gw1_from_records_matches_feature_gemm(m):
    """bgx_ppo_gw1 (gW1 / gb1 = dh^T [x | 1] with x generated on chip from the
    records) against the GEMM it replaces over the encoded fp16 feature rows
    (encode_records, pinned to the reference's features by G2), in fp64: the
    same fp16 operands, so only the fp32 accumulation order differs.  Ragged m
    (partial last row tile), records from a real rollout (every feature type:
    bar, off, one-hot, the ones column)."""
    from bgx import _lib
    from bgx._lib import check
    from bgx.engine import encode_records
    L = _lib.load()
    recs = _setup(seed=5, batch=4096, horizon=8)[0]
    reps = (m + recs.shape[0] - 1) // recs.shape[0]
    recs = recs.repeat(reps, 1)[:m].contiguous()
    g = torch.Generator(device="cuda").manual_seed(m)
    dh = (torch.randn(m, 128, device="cuda", generator=g) * 0.5).half()
    dh[torch.rand(m, 128, device="cuda", generator=g) < 0.4] = 0          # the ReLU mask's zeros
    gw1 = torch.zeros(128, 208, dtype=torch.float32, device="cuda")
    ws = torch.empty(L.bgx_ppo_gw1_workspace(m) // 4, dtype=torch.float32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):                                                   # accumulates (+=)
        check(L.bgx_ppo_gw1(_p(dh), _p(recs), m, 128, _p(ws), _p(gw1), s), "bgx_ppo_gw1")
    x = encode_records(recs, torch.float16, width=208)
    x[:, 198] = 1.0
    ref = 2 * (dh.double().t() @ x.double())
    assert torch.equal(gw1[:, 199:], torch.zeros_like(gw1[:, 199:]))
    err = (gw1.double() - ref).abs()
    assert float(err.max()) <= 1e-5 * float(ref.abs().max()) + 1e-6, float(err.max())
    assert _rel(gw1.double(), ref) < 1e-6
    # deterministic: the same call gives the same bits
    gw1b = torch.zeros_like(gw1)
    for _ in range(2):
        check(L.bgx_ppo_gw1(_p(dh), _p(recs), m, 128, _p(ws), _p(gw1b), s), "bgx_ppo_gw1")
    assert torch.equal(gw1, gw1b)


def test_gather_rollout_matches_torch_indexing():
    """bgx_gather_rollout (the update's rows in plan order, one kernel) == torch
    indexing of the records and the four per-row fields, bit for bit."""
    from bgx.train import gather_rollout
    g = torch.Generator(device="cuda").manual_seed(3)
    m = 100_003
    recs = torch.randint(0, 256, (m, 64), dtype=torch.uint8, device="cuda", generator=g)
    acts = torch.randint(0, 500, (m,), dtype=torch.int32, device="cuda", generator=g)
    old, R, adv = (torch.randn(m, device="cuda", generator=g) for _ in range(3))
    perm = torch.randperm(m, device="cuda", generator=g).to(torch.int32)
    got = gather_rollout(perm, recs, acts, old, R, adv)
    pl = perm.long()
    for a, b in zip(got, (recs[pl], acts[pl], old[pl], R[pl], adv[pl])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("m", [1, 1000, 4097, 3 * 65536 + 77, (1 << 21) + 3])
def test_plan_rows_matches_plan_then_gather(m):
    """bgx_ppo_plan_rows (the rows scattered straight to their plan-order positions) ==
    bgx_ppo_plan + bgx_gather_rollout == the torch plan + torch indexing, bit for bit:
    legal counts 0 (every action) .. 600 (clamped to 500), a ragged last block, and more
    than 64 x 32 counting blocks (the scan's register chunks wrap)."""
    from bgx.train import gather_rollout, plan_rollout, ppo_row_plan, ppo_row_plan_torch
    g = torch.Generator(device="cuda").manual_seed(5)
    recs = torch.randint(0, 256, (m, 64), dtype=torch.uint8, device="cuda", generator=g)
    cnt = torch.randint(0, 601, (m,), device="cuda", generator=g)
    cnt = torch.where(torch.rand(m, device="cuda", generator=g) < 0.7, cnt % 40, cnt)   # mostly class 1-2
    recs[:, 60] = (cnt & 255).to(torch.uint8)
    recs[:, 61] = (cnt >> 8).to(torch.uint8)
    acts = torch.randint(0, 500, (m,), dtype=torch.int32, device="cuda", generator=g)
    old, R, adv = (torch.randn(m, device="cuda", generator=g) for _ in range(3))
    rows, plan, row_plan = plan_rollout(recs, acts, old, R, adv)
    perm, plan2, row_plan2 = ppo_row_plan(recs)
    ref = gather_rollout(perm, recs, acts, old, R, adv)
    permt, plant, row_plant = ppo_row_plan_torch(recs)
    assert torch.equal(perm, permt)
    assert torch.equal(plan, plan2) and torch.equal(plan, plant)
    assert torch.equal(row_plan, row_plan2) and torch.equal(row_plan, row_plant)
    for a, b in zip(rows, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("m", [1, 31, 1024, 4097, 3 * 65536 + 77, (1 << 20) + 5])
def test_device_row_plan_matches_torch(m):
    """bgx_ppo_plan (stable counting sort by action-tile class + the k_ppo_gw2 / rows
    plan from the class totals, no host sync) equals the torch form it replaces
    (argsort stable + bincount + cumsum, ppo_row_plan_torch) exactly: legal counts 0
    (all 16 tiles), 1..500 and above n_actions, at sizes around the 1,024-row blocks."""
    from bgx.train import ppo_row_plan, ppo_row_plan_torch
    g = torch.Generator(device="cpu").manual_seed(m)
    recs = torch.randint(0, 256, (m, 64), dtype=torch.uint8, generator=g)
    kind = torch.randint(0, 10, (m,), generator=g)
    cnt = torch.where(kind == 0, torch.zeros(m, dtype=torch.int64),
                      torch.where(kind == 1, torch.randint(501, 2000, (m,), generator=g),
                                  torch.randint(1, 60, (m,), generator=g)))
    cnt = torch.where(kind == 2, torch.randint(60, 501, (m,), generator=g), cnt)
    recs[:, 60] = (cnt & 255).to(torch.uint8)
    recs[:, 61] = (cnt >> 8).to(torch.uint8)
    recs = recs.cuda()
    p1, pl1, rp1 = ppo_row_plan(recs)
    p2, pl2, rp2 = ppo_row_plan_torch(recs)
    assert torch.equal(p1, p2)
    assert torch.equal(pl1, pl2)
    assert torch.equal(rp1, rp2)


def test_device_row_plan_on_rollout():
    from bgx.train import ppo_row_plan, ppo_row_plan_torch
    recs = _setup(seed=5, batch=2048, horizon=6)[0]
    for a, b in zip(ppo_row_plan(recs), ppo_row_plan_torch(recs)):
        assert torch.equal(a, b)
