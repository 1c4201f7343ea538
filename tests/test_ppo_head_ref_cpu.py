"""The loss head's fp64 reference (tests/ppo_head_ref.py) against torch autograd of the
literal formulation, and the properties of the synthetic rows that the GPU tests rely on,
asserted from the reference alone."""
import math

import numpy as np
import pytest
import torch

from ppo_head_ref import (EPS_CLIP, HEAD_DTYPES, HEAD_NS, HEAD_SHAPES, HEAD_SMALL_NS, HEAD_STRIDE_N, KIND_MASKED,
                          LOG_1M_EPS, LOG_EPS, coefs_for, head64, head_seed, synthetic_rows)

EPS32 = float(np.finfo(np.float32).eps)
ONE_M_EPS32 = float(np.float32(1) - np.float32(EPS32))


def _autograd(s, coefs, A):
    """ppo_agent.py:268-296 written out in float64: softmax(z + log(mask + 1e-45)),
    Categorical(probs)'s clamp_probs with the fp32 eps written out (in fp64 Categorical would
    clamp at fp64's eps), exp(new - old), torch.min, torch.clamp, MSE, entropy; times gs.
    The coefficients are the fp32 numbers the kernels receive, and the entropy's is their fp32
    product k1 = fp32(gs * ce), which the kernels form once per launch."""
    eps = coefs[0]
    cv, ce, gs = (float(np.float32(c)) for c in coefs[1:])
    k1 = float(np.float32(gs) * np.float32(ce))
    z = s.z.double().clone().requires_grad_(True)
    v = s.values.double().clone().requires_grad_(True)
    mask = (torch.arange(A)[None] < s.cnt[:, None]).float()
    ml = (mask + 1e-45).log().double()                       # fp32 log(1e-45), as the agent forms it
    p = torch.softmax(z + ml, -1)
    lp = torch.log(p.clamp(EPS32, ONE_M_EPS32))
    new = lp.gather(1, s.act[:, None])[:, 0]
    r = torch.exp(new - s.old.double())
    advd = s.adv.double()
    pol = -torch.min(r * advd, torch.clamp(r, 1 - eps, 1 + eps) * advd)
    val = (v - s.R.double()) ** 2
    ent = -(p * lp).sum(1)
    (gs * (pol + cv * val) - k1 * ent).sum().backward()
    return z.grad, v.grad, torch.stack([pol, val, ent], 1).detach(), p.detach()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", HEAD_DTYPES)
@pytest.mark.parametrize("A", [1, 17, 500])
def test_head64_matches_autograd(A, dtype, scaled):
    """head64(drop_masked=False) == autograd of the literal fp64 formulation on the synthetic
    rows, every element within 1e-10 * gs: the closed form's tie splitting (ratio target 1.0
    and advantage 0 give s1 == s2), inclusive clamp and clamp_probs rules are autograd's.
    The per-row loss parts agree as far as the clamp bounds do: the kernels (and head64) clamp
    at the fp32 values of log(eps) and log(1 - eps), fp64 autograd at the fp64 logs of the same
    fp32 eps, 4.3e-7 apart at the lower bound."""
    n = 2051
    s = synthetic_rows(n, A, head_seed(A, n), dtype)
    coefs = coefs_for(n, scaled)
    gs = coefs[3]
    dz, dv, parts, p = _autograd(s, coefs, A)
    ref = head64(s.z, s.values, s.cnt, s.act, s.old, s.R, s.adv, coefs, A, drop_masked=False)
    assert float((dz - ref.d).abs().max()) <= 1e-10 * gs
    assert float((dv - ref.gv).abs().max()) <= 1e-10 * gs
    d_lo, d_hi = abs(math.log(EPS32) - LOG_EPS), abs(math.log(ONE_M_EPS32) - LOG_1M_EPS)
    assert d_lo < 5e-7 and d_hi < 1e-13
    dmax = 2 * max(d_lo, d_hi)
    assert bool(((parts[:, 0] - ref.rows[:, 0]).abs() <= 1e-10 + dmax * (ref.rt * s.adv.double()).abs()).all())
    assert float((parts[:, 1] - ref.rows[:, 1]).abs().max()) <= 1e-10
    assert bool(((parts[:, 2] - ref.rows[:, 2]).abs() <= 1e-10 + dmax).all())
    # the mask the agent forms is the constant the reference adds
    assert float((torch.zeros(1) + 1e-45).log()) == pytest.approx(-103.27892990343185, abs=1e-5)


def _cases():
    out = []
    for A in sorted({sh[0] for sh in HEAD_SHAPES}):
        for dtype in HEAD_DTYPES:
            for n in HEAD_NS + HEAD_SMALL_NS + ((HEAD_STRIDE_N,) if A == 500 else ()):
                out.append((A, dtype, n))
    return out


def _ref(A, dtype, n):
    s = synthetic_rows(n, A, head_seed(A, n), dtype)
    coefs = coefs_for(n, False)
    return s, head64(s.z, s.values, s.cnt, s.act, s.old, s.R, s.adv, coefs, A, drop_masked=False)


@pytest.mark.parametrize("A,dtype,n", _cases())
def test_synthetic_rows_stay_off_the_bounds(A, dtype, n):
    """For every (A, dtype, n) test_gpu_ppo_head.py runs: no row has its action's log-prob
    within 1e-3 of log eps or its ratio within 1e-3 of 1 -+ eps_clip, so the either-side
    allowance is never needed at the lower clamp or at a clip bound; at most 1e-4 of the
    elements lie within 1e-4 of log eps; the inputs are finite and the actions below A."""
    s, ref = _ref(A, dtype, n)
    assert bool(torch.isfinite(s.z.double()).all()) and bool(torch.isfinite(s.old).all())
    assert int(s.act.min()) >= 0 and int(s.act.max()) < A
    assert int(((ref.ua - LOG_EPS).abs() < 1e-3).sum()) == 0
    assert not bool(ref.amb_low.any())
    assert int(((ref.rt - (1 - EPS_CLIP)).abs() < 1e-3).sum()) == 0
    assert int(((ref.rt - (1 + EPS_CLIP)).abs() < 1e-3).sum()) == 0
    assert not bool(ref.near_clip.any())
    assert float(ref.near_low.double().mean()) <= 1e-4


@pytest.mark.parametrize("A,dtype,n", [c for c in _cases() if c[0] >= 16 and c[2] >= 4099])
def test_synthetic_rows_reach_every_branch(A, dtype, n):
    """At A >= 16 and the large row counts each of the 3 x 3 cells {ratio < 1 - eps, inside,
    > 1 + eps} x {adv < 0, = 0, > 0} has at least 20 rows, and so has each special row kind:
    action clamped low, clamped high, masked action, cnt = 0, cnt = 1, cnt > A."""
    s, ref = _ref(A, dtype, n)
    rcls = torch.where(ref.rt < 1 - EPS_CLIP, 0, torch.where(ref.rt > 1 + EPS_CLIP, 2, 1))
    acls = torch.sign(s.adv).long() + 1
    cells = torch.bincount(rcls * 3 + acls, minlength=9)
    assert int(cells.min()) >= 20, cells
    legal = (s.act < s.cnt) | (s.cnt == 0)
    kinds = {"clamped low": (ref.ua < LOG_EPS) & legal, "clamped high": ref.ua > LOG_1M_EPS,
             "masked action": (s.act >= s.cnt) & (s.cnt > 0), "cnt = 0": s.cnt == 0, "cnt = 1": s.cnt == 1,
             "cnt > A": s.cnt > A}
    for name, rows in kinds.items():
        assert int(rows.sum()) >= 20, (name, int(rows.sum()))
    # the masked-action rows are the generator's, and their action is a real column
    m = (s.act >= s.cnt) & (s.cnt > 0)
    assert bool((s.kind[m] == KIND_MASKED).all()) and bool((s.act[m] < A).all())
