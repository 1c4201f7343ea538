"""The loss-head kernel k_ppo_head (csrc/bg_ppo.hip) through bgx_ppo_head / bgx_ppo_head_ex,
every output element against the fp64 closed form head64(drop_masked=False)
(tests/ppo_head_ref.py, pinned to torch autograd by test_ppo_head_ref_cpu.py), on synthetic
rows that reach every clip and clamp case and on every launch shape the ABI accepts.

Row kinds (ppo_head_ref.synthetic_rows; test_ppo_head_ref_cpu.py proves each is present):
  * ratio targets 0.5 / 2.0 with either sign of the advantage: the clipped branches of the
    surrogate (w1 = 0 with w2 = 0, and w1 = 1 beside the clip); 0.9 / 1.1: the inside
    branch; 1.0 and advantage 0: s1 == s2, the tie that min() splits in half;
  * dominant rows: p_a > 1 - eps, the upper clamp of clamp_probs (no policy gradient);
  * tiny rows: p_a < eps, the lower clamp on the action, and clamped elements in the entropy;
  * masked-action rows: cnt <= act < A, the action's logit takes the mask;
  * cnt = 0 (every column masked), cnt = 1 (one legal move), cnt > A.
Launch shapes (ppo_head_ref.HEAD_SHAPES), as (A, ld_logits, ld_dlogits, pad, base offset):
  * (500, 500, 500, 0): the fp32 epoch's layout; fp16 rows 8-byte aligned, the last lane's 16
    columns straddle A (vector load off, scalar store);
  * (500, 512, 512, 1): the fp16 "manual" epoch's layout, value gradient in column 500;
  * (500, 504, 504, 1): vector path with the last lane straddling ld (scalar for that lane);
  * (500, 501, 501, 1): rows unaligned, the scalar load and store path on every lane;
  * (500, 512, 512, 1, offset 1): both base pointers one element off alignment, scalar path;
  * (512, 512, 512, 0): every lane full; (511, 512, 512, 1): the pad column is the last one;
  * (33, 40, 40, 1), (17, 17, 17, 0): lanes 2 / 1 straddle A, the other lanes own no column;
  * (16, 16, 32, 1): pad_value_col with ld_dlogits other than 512 and other than ld_logits;
  * (1, 1, 1, 0), (1, 8, 8, 1): one column.
n = 9 and the small set leave most colsum blocks without a row; an odd n leaves one half-wave
idle in the DPP reductions; n = 2048 * 8 + 5 makes five halves grid-stride to a second row."""
import ctypes
import functools
import math

import pytest
import torch

from ppo_head_ref import (HEAD_DTYPES, HEAD_NS, HEAD_SHAPES, HEAD_SMALL_NS, HEAD_STRIDE_N, U32, coefs_for, head64,
                          head_seed, records_of, synthetic_rows, ulp_of)

pytestmark = pytest.mark.gpu

MARGIN = 64                  # sentinel elements before and after every output buffer
SENTINEL = -7.0
COLSUM_BLOCKS = 2048         # BGX_PPO_COLSUM_BLOCKS


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@functools.lru_cache(maxsize=4)
def _rows(n, A, dtype):
    s = synthetic_rows(n, A, head_seed(A, n), dtype)
    assert int(s.act.min()) >= 0 and int(s.act.max()) < A           # the kernel reads logits[row][act]
    return {k: v.cuda() for k, v in vars(s).items()}


def _framed(n, ld, off, dtype, fill):
    """A flat buffer [MARGIN + off | n x ld | MARGIN] filled with `fill`; returns (buffer, rows view)."""
    buf = torch.full((MARGIN + off + n * ld + MARGIN,), fill, dtype=dtype, device="cuda")
    return buf, buf[MARGIN + off:MARGIN + off + n * ld].view(n, ld)


def _launch(s, A, ldl, ldd, pad, off, dtype, coefs, colsum, plain=False):
    """One call of bgx_ppo_head_ex (bgx_ppo_head with `plain`).  The logits' padding columns
    hold NaN (the kernel may load but never use them); outputs sit in sentinel frames."""
    from bgx import _lib
    from bgx._lib import check
    L = _lib.load()
    n = s["z"].shape[0]
    _, lg = _framed(n, ldl, off, dtype, float("nan"))
    lg[:, :A] = s["z"]
    dbuf, dl = _framed(n, ldd, off, dtype, SENTINEL)
    vbuf, dval = _framed(n, 1, 0, dtype, SENTINEL)
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    cs = torch.full((COLSUM_BLOCKS, 512), float("nan"), dtype=torch.float32, device="cuda") if colsum else None
    recs = records_of(s["cnt"])
    acts = s["act"].to(torch.int32)
    eps, cv, ce, gs = coefs
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (_p(lg), 0 if dtype == torch.float32 else 1, ldl, _p(s["values"]), _p(recs), _p(acts), _p(s["old"]),
            _p(s["R"]), _p(s["adv"]), n, A, eps, cv, ce, gs, _p(dl), ldd, _p(dval), _p(sums))
    if plain:
        check(L.bgx_ppo_head(*head, stream), "bgx_ppo_head")
    else:
        check(L.bgx_ppo_head_ex(*head, pad, _p(cs), stream), "bgx_ppo_head_ex")
    torch.cuda.synchronize()
    return dbuf, dl, vbuf, dval, sums, cs


def _sentinel_only(t):
    return bool((t == SENTINEL).all())


def _check_case(n, A, ldl, ldd, pad, off, dtype, scaled, worst):
    s = _rows(n, A, dtype)
    coefs = coefs_for(n, scaled)
    ref = head64(s["z"], s["values"], s["cnt"], s["act"], s["old"], s["R"], s["adv"], coefs, A, drop_masked=False)
    assert not bool(ref.amb_low.any()) and not bool(ref.near_clip.any())
    ulp = ulp_of(dtype)
    dbuf, dl, vbuf, dval, sums, cs = _launch(s, A, ldl, ldd, pad, off, dtype, coefs, colsum=True)

    def note(name, err, tol):
        worst[name] = max(worst.get(name, 0.0), float((err / tol).max()))

    # dlogits[:, :A] element by element; the either-side allowance acts at the upper clamp alone
    got = dl[:, :A].double()
    tol = ulp(ref.d) + ref.tol
    e = torch.minimum((got - ref.d).abs(), (got - ref.d_alt).abs())
    note("dlogits", e, tol)
    assert bool((e <= tol).all()), ("dlogits", float((e / tol).max()), int((e > tol).sum()))
    # (a kernel that decides a clamp within reach of its bound the other way uses that
    # allowance whole: the rows with no such decision are noted on their own)
    off_bound = ~(ref.amb_high | ref.on_bound.any(1))
    if bool(off_bound.any()):
        note("dlogits_off_bound", e[off_bound], tol[off_bound])
    assert not bool((ref.d_alt != ref.d)[~ref.amb_high].any())
    # dvalues, and with pad the same number in column A, zeros up to ld; without pad the
    # columns past A keep their sentinel
    tv = ulp(ref.gv) + ref.tol_v
    ev = (dval[:, 0].double() - ref.gv).abs()
    note("dvalues", ev, tv)
    assert bool((ev <= tv).all()), ("dvalues", float((ev / tv).max()))
    if pad:
        assert torch.equal(dl[:, A], dval[:, 0])
        assert bool((dl[:, A + 1:] == 0).all())
    else:
        assert _sentinel_only(dl[:, A:])
    # nothing outside [0, n) x [0, ld)
    lo = MARGIN + off
    assert _sentinel_only(dbuf[:lo]) and _sentinel_only(dbuf[lo + n * ldd:])
    assert _sentinel_only(vbuf[:MARGIN]) and _sentinel_only(vbuf[MARGIN + n:])
    # the loss sums: each row's parts carry its relative budget, the entropy also the absolute
    # fp32 error of the row's log-probs (sum_j p_j reach = reach; ppo_head_ref.head64)
    rows = ref.rows
    st = (ref.rowfac[:, None] * torch.stack([rows[:, 0].abs(), rows[:, 1], ref.plp], 1)).sum(0)
    st[2] += ref.reach.sum()
    es = (sums - rows.sum(0)).abs()
    worst["sums"] = max(worst.get("sums", 0.0), float((es / st.clamp(min=1e-300)).max()))
    assert bool((es <= st).all()), ("sums", sums, rows.sum(0), st)
    # column sums of the stored gradient; the blocks without a row wrote their zeros
    assert not bool(torch.isnan(cs).any())
    wid = ldd if pad else A
    stored = dl[:, :wid].double()
    ec = (cs.double().sum(0)[:wid] - stored.sum(0)).abs()
    tc = (math.ceil(n / 16384) + 8) * U32 * stored.abs().sum(0)
    worst["colsum"] = max(worst.get("colsum", 0.0), float((ec / tc.clamp(min=1e-300)).max()))
    assert bool((ec <= tc).all()), ("colsum", float((ec / tc.clamp(min=1e-300)).max()))
    assert bool((cs[:, wid:] == 0).all())
    # the same rows without column sums (the grid follows n): per-row work, so the same bits
    dbuf2, dl2, vbuf2, dval2, sums2, _ = _launch(s, A, ldl, ldd, pad, off, dtype, coefs, colsum=False, plain=not pad)
    assert torch.equal(dbuf2.view(torch.int16 if dtype == torch.float16 else torch.int32),
                       dbuf.view(torch.int16 if dtype == torch.float16 else torch.int32))
    assert torch.equal(vbuf2, vbuf)
    assert bool(((sums2 - rows.sum(0)).abs() <= st).all()), ("sums, no colsum", sums2, rows.sum(0), st)


_IDS = ["A%d-ld%d-%d-pad%d%s" % (a, l, d, p, "-off1" if o else "") for a, l, d, p, o in HEAD_SHAPES]


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_IDS)
@pytest.mark.parametrize("n", HEAD_NS)
@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=["fp32", "fp16"])
def test_head_elementwise_vs_fp64(dtype, n, shape):
    """Every launch shape at n = 9 and 4099, gradient scale 16 and 65536 / n (fp16 gradients
    in the subnormal range).  Measured on the MI355X, worst error / tolerance over all cases:
    dlogits 0.999 in fp32 (a probability just below 2^-126 that the hardware exp2 returns as 0
    uses that allowance whole) and 0.984 in fp16 (so does a clamp decided the other way within
    reach of its bound; 0.50, the fp16 rounding, on the rows without one), dvalues 0.50,
    loss sums 0.026, column sums 0.32.  No kernel fault found."""
    worst = {}
    for scaled in (False, True):
        _check_case(n, *shape, dtype, scaled, worst)
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=_IDS)
@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=["fp32", "fp16"])
def test_head_small_n(dtype, shape):
    """n = 1, 2, 3, 8: a grid of one workgroup (no colsum) with idle halves, and 2,047
    colsum blocks without a row.  Measured: dlogits 0.999 (fp32) / 0.49 (fp16), dvalues 0.50,
    loss sums 0.038, column sums 0.38."""
    worst = {}
    for n in HEAD_SMALL_NS:
        _check_case(n, *shape, dtype, False, worst)
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=["fp32", "fp16"])
def test_head_grid_stride(dtype):
    """n = 2048 * 8 + 5: five halves walk a second row (fp64 partial sums, the column sums
    of two rows in one lane), production layout.  Measured: dlogits 0.999 (fp32) / 0.96 (fp16,
    0.50 off the clamp bounds), dvalues 0.50, loss sums 0.0013, column sums 0.062."""
    worst = {}
    _check_case(HEAD_STRIDE_N, 500, 512, 512, 1, 0, dtype, True, worst)
    print("worst error / tolerance:", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("dtype", HEAD_DTYPES, ids=["fp32", "fp16"])
def test_head_no_rows_with_colsum(dtype):
    """n = 0 with colsum returns OK and every block writes zeros; without colsum nothing is launched."""
    from bgx import _lib
    L = _lib.load()
    cs = torch.full((COLSUM_BLOCKS, 512), float("nan"), dtype=torch.float32, device="cuda")
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = 0 if dtype == torch.float32 else 1
    rc = L.bgx_ppo_head_ex(None, dt, 512, None, None, None, None, None, None, 0, 500, 0.25, 0.5, 0.15, 16.0, None, 512,
                           None, _p(sums), 1, _p(cs), stream)
    torch.cuda.synchronize()
    assert rc == _lib.BGX_OK
    assert bool((cs == 0).all()) and bool((sums == 0).all())
    assert L.bgx_ppo_head_ex(None, dt, 512, None, None, None, None, None, None, 0, 500, 0.25, 0.5, 0.15, 16.0, None,
                             512, None, None, 1, None, stream) == _lib.BGX_OK


def test_head_rejects_bad_arguments():
    """The header's BGX_EINVAL cases: n_actions 0 and 513, dtype 2, pad with ld_dlogits <= A or > 512."""
    from bgx import _lib
    L = _lib.load()
    s = _rows(9, 17, torch.float32)
    n, A = 9, 17
    lg = torch.zeros(n, 520, device="cuda")
    dl = torch.full((n, 520), SENTINEL, device="cuda")
    dval = torch.full((n,), SENTINEL, device="cuda")
    sums = torch.zeros(3, dtype=torch.float64, device="cuda")
    recs = records_of(s["cnt"])
    acts = s["act"].to(torch.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dt, n_actions, ldd, pad):
        return L.bgx_ppo_head_ex(_p(lg), dt, 520, _p(s["values"]), _p(recs), _p(acts), _p(s["old"]), _p(s["R"]),
                                 _p(s["adv"]), n, n_actions, 0.25, 0.5, 0.15, 16.0, _p(dl), ldd, _p(dval), _p(sums),
                                 pad, None, stream)

    for dt, n_actions, ldd, pad in ((0, 0, 520, 0), (0, 513, 520, 0), (2, A, 520, 0), (0, A, A, 1), (0, A, A - 1, 1),
                                    (0, A, 513, 1), (1, A, 520, 1)):
        assert call(dt, n_actions, ldd, pad) == _lib.BGX_EINVAL, (dt, n_actions, ldd, pad)
    torch.cuda.synchronize()
    assert _sentinel_only(dl) and _sentinel_only(dval) and bool((sums == 0).all())
