"""The PPO loss head (ppo_agent.py:268-296 under the masked softmax of :166) in fp64,
in closed form, with the rounding budget of the HIP kernels that implement it, and a
deterministic set of synthetic rows that reaches every clip and clamp case.  Shared by
test_ppo_head_ref_cpu.py (closed form == torch autograd), test_gpu_ppo_head.py
(bgx_ppo_head / bgx_ppo_head_ex) and test_gpu_ppo_fused.py (bgx_ppo_rows / bgx_ppo_gw2)."""
from types import SimpleNamespace

import numpy as np
import torch

U32 = 2.0 ** -24                     # fp32 unit roundoff
LOG_EPS, LOG_1M_EPS = -15.942384719848633, -1.1920930376163597e-07   # the kernels' fp32 clamp bounds
MASK_LOG = float(np.float32(-103.27892990343185))                   # fp32 log(1e-45), ppo_agent.py:166
LOG2E = 1.4426950408889634

EPS_CLIP = 0.25
COUNTS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 499, 500, 511, 512, 600)
ADVS = (-1.3, 0.0, 0.7)
RATIOS = (0.5, 0.9, 1.0, 1.1, 2.0)   # every target at least 10 % away from 1 -+ EPS_CLIP
KIND_DOMINANT, KIND_TINY, KIND_MASKED = 0, 1, 2     # of 8 equally likely kinds; 3..7 are plain rows


def ulp16(x):
    """fp16 ulp at |x| (fp64 tensor): 2^(e - 10) in the normal range, 2^-24 below it."""
    a = x.abs().clamp(min=2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def ulp32(x):
    """fp32 ulp at |x| (fp64 tensor): 2^(e - 23) in the normal range, 2^-149 below it."""
    a = x.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ulp_of(dtype):
    return ulp16 if dtype == torch.float16 else ulp32


def _logp64(z, cnt, A, drop_masked):
    """(u [n, A] natural log-probs in fp64, play [n, A], lim [n]) of the masked softmax."""
    cnt = cnt.long()
    cols = torch.arange(A, device=z.device)[None, :]
    zd = z[:, :A].double()
    if drop_masked:
        lim = torch.where(cnt == 0, torch.full_like(cnt, A), cnt.clamp(max=A))
        play = cols < lim[:, None]
        zz = torch.where(play, zd, torch.full_like(zd, float("-inf")))
    else:
        lim = torch.full_like(cnt, A)
        play = torch.ones_like(zd, dtype=torch.bool)
        zz = zd + torch.where(cols < cnt[:, None], 0.0, MASK_LOG)
    return zz - torch.logsumexp(zz, dim=1, keepdim=True), play, lim


def head64(z, values, cnt, act, old, R, adv, coefs, A, drop_masked, wide=None):
    """The loss head in fp64 on the logits z[:, :A] and the values as the kernel reads them
    (already rounded to its dtype), per-row gradient scaled by coefs[3] as the kernels scale it.

    drop_masked=True  (bgx_ppo_rows / bgx_ppo_gw2): the columns at or past lim = (cnt or A,
        at most A) are left out of the softmax and get gradient 0; a chosen action at or past
        lim has log-prob -inf, i.e. la = log eps, no policy gradient and no one-hot term.
    drop_masked=False (bgx_ppo_head): every column j < A takes part with
        z_j + (j < cnt ? 0 : fp32 log(1e-45)), as ppo_agent.py:166 forms it.
    wide (default: not drop_masked): the budget follows the fp32 resolution of the row's
        log-probs instead of the constant 1e-6 (see `reach` in the code).

    Returns a namespace of fp64 tensors:
      d [n, A], gv [n]      dL/dlogits and dL/dvalue
      d_alt [n, A]          d with the action's clamp decided the other way on rows `amb`
      rows [n, 3]           per-row (policy loss, (v - R)^2, entropy)
      tol [n, A], tol_v [n] the kernels' fp32 rounding budget per element (the output
                            format's own ulp is added by the caller)
      rowfac [n]            the relative budget per row (also that of the loss sums)
      reach [n]             the absolute fp32 error of a log-prob of the row (the entropy's budget)
      ua, la, rt [n]        the action's log-prob, its clamp, the ratio
      amb_low, amb_high [n] ua within 1e-4 of log eps / `reach` of log(1 - eps)
      near_clip [n]         rt within 1e-3 of 1 -+ eps_clip
      on_bound [n, A]       element log-prob within 1e-4 of log eps / `reach` of log(1 - eps)
      near_low [n, A]       element log-prob within 1e-4 of log eps
      lim [n], plp [n]      columns in play; sum_j p_j |lp_j| (the entropy sum's magnitude)"""
    wide = (not drop_masked) if wide is None else wide
    eps, cv, ce, gs = coefs
    gs32, ce32, cv32 = (float(np.float32(v)) for v in (gs, ce, cv))
    k1 = float(np.float32(gs32) * np.float32(ce32))
    u, play, lim = _logp64(z, cnt, A, drop_masked)
    cols = torch.arange(A, device=z.device)[None, :]
    zero = torch.zeros_like(u)
    p = torch.exp(u)
    lp = u.clamp(LOG_EPS, LOG_1M_EPS)
    q = lp + ((lp == u) & play).double()
    pl = torch.where(play, p, zero)
    ent = -(pl * torch.where(play, lp, zero)).sum(1)
    entq = -(pl * torch.where(play, q, zero)).sum(1)
    a = act.long()
    ua = torch.where(a < lim, u.gather(1, a.clamp(max=A - 1)[:, None])[:, 0], torch.full_like(ent, float("-inf")))
    la = ua.clamp(LOG_EPS, LOG_1M_EPS)
    rt = torch.exp(la - old.double())
    advd = adv.double()
    s1, s2 = rt * advd, rt.clamp(1 - eps, 1 + eps) * advd
    pol = -torch.minimum(s1, s2)
    # torch autograd: min() splits ties, clamp() passes on its inclusive bounds
    w1 = torch.where(s1 < s2, 1.0, torch.where(s1 == s2, 0.5, 0.0)).double()
    w2 = (1 - w1) * ((rt >= 1 - eps) & (rt <= 1 + eps)).double()
    glp_in = -advd * rt * (w1 + w2)                      # g_lp when the action's log-prob is not clamped
    ina = (la == ua).double()
    onehot = ((cols == a[:, None]) & play).double()
    dv = values.double() - R.double()
    gv = gs32 * cv32 * 2.0 * dv

    def dfor(ina_):
        gla = gs32 * glp_in * ina_
        k2 = k1 * entq - gla
        d = pl * (k1 * q + k2[:, None]) + onehot * gla[:, None]
        return torch.where(play, d, zero), gla, k2

    d, gla, k2 = dfor(ina)
    # The kernels form log-probs in the log domain, u_j = (z2_j - lse2) ln 2 with z2 = z log2(e)
    # (+ the mask) and lse2 = max + log2(sum): z2_j, lse2 and the product lse2 ln 2 are each
    # rounded to fp32 at the magnitude Z_row = max_j |z2_j|, half an ulp each, so u_j carries an
    # ABSOLUTE error of up to (1/2 + 1/2) ln 2 + 1/2 < 2 fp32 ulps of Z_row (`reach`), however
    # close to 0 it is.  The loss head has three places where an absolute error in u shows:
    #   (a) a clamp decision (lp == u) within `reach` of a bound may fall on either side;
    #   (b) the entropy sum_j p_j lp_j moves by up to sum_j p_j reach = reach per row;
    #   (c) q_j = lp_j + [unclamped] moves by reach, and with it k2 = k1 entq - gla by k1 reach.
    # `wide` budgets all three from reach; without it (the budget test_fused_head_elementwise_
    # vs_fp64 has always used, on first-epoch rows with |z| < 6 where 2 ulps stay below 1e-6)
    # the reach is the constant 1e-6 and only (a) is allowed for, on the element itself.
    if drop_masked:
        z_abs = torch.where(play, z[:, :A].double().abs(), zero).max(1).values
    else:
        z_abs = z[:, :A].double().abs().max(1).values - MASK_LOG
    z_row = z_abs * LOG2E
    reach = (2 * ulp32(z_row)).clamp(min=1e-6) if wide else torch.full_like(z_row, 1e-6)
    # (a) for the action: the kernel may take either side, d or d_alt.  The synthetic rows never
    # come near the lower bound (test_ppo_head_ref_cpu.py), so on them the allowance acts at the
    # upper bound alone, where the two sides differ by gla (1 - p_a) at the action and gla p_j
    # elsewhere with sum_j p_j = 1 - p_a < eps + reach.
    amb_low = (ua - LOG_EPS).abs() < 1e-4
    amb_high = (ua - LOG_1M_EPS).abs() < reach
    amb = amb_low | amb_high
    d_alt, gla_alt, k2_alt = dfor(1.0 - ina)
    d_alt = torch.where(amb[:, None], d_alt, d)
    # fp32 budget: every p from an fp32 log-sum-exp over lim terms, k2 / gla / entq in fp32
    rowfac = (lim + 16).double() * U32
    qa = torch.where(play, q.abs(), zero)
    if not drop_masked:
        # bgx_ppo_head keeps the masked columns at z - 103.28, so p = exp2(z2 - lse2) and
        # la = za - lse subtract operands of magnitude Z_row = (max_j |z_j| + 103.28) log2(e),
        # each carrying up to one fp32 ulp at that magnitude: two operands, doubled as margin
        rowfac = rowfac + 4 * ulp32(z_row)

    def budget(gla_, k2_):
        g_, k_ = gla_.abs()[:, None], k2_.abs()[:, None]
        return rowfac[:, None] * (pl * (k1 * qa + k_ + g_) + onehot * g_)

    tol = budget(gla, k2)
    if wide:
        # a kernel on the other side of the action's clamp rounds its k2 and gla at that side's
        # magnitudes (they cancel to gla (1 - p_a) only in exact arithmetic)
        tol = torch.where(amb[:, None], torch.maximum(tol, budget(gla_alt, k2_alt)), tol)
    # (a) for an element: its q may take either side.  At the lower bound p < eps and only the
    # element itself moves visibly (p k1).  At the upper bound the element i holds nearly all
    # the mass, and a flip of q_i by 1 moves entq by p_i: d_i by k1 p_i (1 - p_i) and every
    # other d_j by k1 p_j p_i.
    low = ((u - LOG_EPS).abs() < 1e-4) & play
    high = ((u - LOG_1M_EPS).abs() < reach[:, None]) & play
    on_bound = low | high
    if wide:
        p_high = (high.double() * pl).sum(1)[:, None]
        tol = tol + k1 * (low.double() * pl + high.double() * pl * (1 - pl) + (~high).double() * pl * p_high)
        # (c): q_j and entq each within reach
        tol = tol + 2 * k1 * reach[:, None] * pl
    else:
        tol = tol + on_bound.double() * pl * k1
    if not drop_masked:
        # p comes from the hardware exp2 (v_exp_f32), which returns 0 for a result below the
        # smallest normal fp32: an absolute error of up to 2^-126 in p (the masked columns'
        # p ~ 1e-45 p_legal all lie there), times the factor p is multiplied by
        tol = tol + 2.0 ** -126 * (k1 * qa + k2.abs()[:, None])
    return SimpleNamespace(d=d, d_alt=d_alt, gv=gv, tol=tol, tol_v=4 * U32 * gv.abs(),
                           rows=torch.stack([pol, dv * dv, ent], 1), rowfac=rowfac, reach=reach, ua=ua, la=la, rt=rt,
                           amb_low=amb_low, amb_high=amb_high,
                           near_clip=((rt - (1 - eps)).abs() < 1e-3) | ((rt - (1 + eps)).abs() < 1e-3),
                           on_bound=on_bound, near_low=low, lim=lim,
                           plp=(pl * torch.where(play, lp, zero).abs()).sum(1))


def ratio_fields(n, g):
    """(adv, ratio target) per row: every pair of ADVS x RATIOS on a fixed share of the rows."""
    adv = torch.tensor(ADVS)[torch.randint(0, len(ADVS), (n,), generator=g)]
    tgt = torch.tensor(RATIOS, dtype=torch.float64)[torch.randint(0, len(RATIOS), (n,), generator=g)]
    return adv, tgt


def records_of(cnt):
    """64-byte lane records holding only the legal count (bytes 60-61), all the loss head reads."""
    recs = torch.zeros(cnt.shape[0], 64, dtype=torch.uint8, device=cnt.device)
    recs[:, 60] = (cnt & 255).to(torch.uint8)
    recs[:, 61] = (cnt >> 8).to(torch.uint8)
    return recs


def synthetic_rows(n, A, seed, dtype):
    """n deterministic loss-head rows (CPU tensors) for n_actions = A:
      z [n, A], values [n]   in `dtype`: kernel and reference read the same rounded numbers;
                             logits N(0, s^2), s per row from {0.5, 3, 10}
      cnt [n]                legal counts from COUNTS (0 = no legal move; 600 > A)
      act [n]                uniform below min(cnt, A) (below A for cnt = 0); then per `kind`:
                             dominant (chosen logit + 40: p > 1 - eps), tiny (chosen logit =
                             row minimum - 25: p < eps), masked (cnt <= act < A, 0 < cnt < A)
      adv, R, tgt, old [n]   advantage from ADVS, returns N(0, 1), ratio target from RATIOS,
                             old_logp = fp32(la64 - log tgt) with la64 the fp64 reference's
                             clamped log-prob of the action, so the ratio is tgt up to rounding."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.5, 3.0, 10.0])[torch.randint(0, 3, (n,), generator=g)]
    z = torch.randn(n, A, generator=g) * scale[:, None]
    cnt = torch.tensor(COUNTS)[torch.randint(0, len(COUNTS), (n,), generator=g)]
    lim = torch.where(cnt == 0, torch.tensor(A), cnt.clamp(max=A))
    act = (torch.rand(n, generator=g) * lim).long().clamp(max=A - 1)
    kind = torch.randint(0, 8, (n,), generator=g)
    r = torch.arange(n)
    dom = kind == KIND_DOMINANT
    z[r[dom], act[dom]] += 40.0
    tiny = (kind == KIND_TINY) & (lim > 1)
    z[r[tiny], act[tiny]] = z[tiny].min(1).values - 25.0
    msk = (kind == KIND_MASKED) & (cnt > 0) & (cnt < A)
    act[msk] = (cnt[msk] + ((A - cnt[msk]).double() * torch.rand(n, generator=g).double()[msk]).long()).clamp(max=A - 1)
    z = z.to(dtype)
    # a chosen log-prob that lands within 2e-3 of the lower clamp bound by chance is moved off it
    # (half a unit down, exact in fp16 at these magnitudes): no row needs the either-side allowance
    ua = _logp64(z, cnt, A, False)[0].gather(1, act[:, None])[:, 0]
    near = (ua - LOG_EPS).abs() < 2e-3
    z[r[near], act[near]] -= 0.5
    values = torch.randn(n, generator=g).to(dtype)
    R = torch.randn(n, generator=g)
    adv, tgt = ratio_fields(n, g)
    ua = _logp64(z, cnt, A, False)[0].gather(1, act[:, None])[:, 0]
    old = (ua.clamp(LOG_EPS, LOG_1M_EPS) - tgt.log()).float()
    return SimpleNamespace(z=z, values=values, cnt=cnt, act=act, kind=kind, adv=adv, R=R, tgt=tgt, old=old)


def coefs_for(n, scaled):
    """(eps_clip, value coef, entropy coef, per-row gradient scale): 16, or GradScaler's
    65536 / n, which puts fp16 gradients in the subnormal range."""
    return (EPS_CLIP, 0.5, 0.15, 65536.0 / n if scaled else 16.0)


# bgx_ppo_head launch shapes of test_gpu_ppo_head.py: (A, ld_logits, ld_dlogits, pad, base offset)
HEAD_SHAPES = [
    (500, 500, 500, 0, 0),
    (500, 512, 512, 1, 0),
    (500, 504, 504, 1, 0),
    (500, 501, 501, 1, 0),
    (500, 512, 512, 1, 1),
    (512, 512, 512, 0, 0),
    (511, 512, 512, 1, 0),
    (33, 40, 40, 1, 0),
    (17, 17, 17, 0, 0),
    (16, 16, 32, 1, 0),
    (1, 1, 1, 0, 0),
    (1, 8, 8, 1, 0),
]
HEAD_NS = (9, 4099)
HEAD_SMALL_NS = (1, 2, 3, 8)
HEAD_STRIDE_N = 2048 * 8 + 5         # more rows than 32-lane halves in the largest grid
HEAD_DTYPES = (torch.float32, torch.float16)


def head_seed(A, n):
    return 1000 * A + n
