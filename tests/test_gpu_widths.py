"""Every hidden-width specialisation of the MLP kernels against fp64.

The C ABI takes hidden 1..128 (value search, policy) and hidden % 4 == 0 (fc1 from
records); the kernels compile one instantiation per shape class (NT = ceil(H / 16) for
k_eval / k_rowpart / k_eval_rows, T = ceil(H / 32) for k_policy_act and k_fc1_rec, two
store paths in k_fc1_rec).  The other GPU modules run H = 40 and H = 128 with 500 actions
and torch's default init only; this module walks the widths, the action counts and the
weight scales in between, and compares every output with an fp64 reference built from the
weights' fp32 values.

Networks: PolicyNet(hidden_size=H[, action_size=A]) after torch.manual_seed, then every
bias overwritten with seeded N(0, 0.5) draws, so a dropped or mis-scaled bias is far above
tolerance.

Tolerances.  Default-scale 2-ply leaves: 1e-6 absolute (the bound of
test_gpu_search.test_two_ply_every_leaf_vs_fp64).  Everything else that is
fp32-equivalent: a running-error bound  |got - ref| <= F * 2^-22 * A(row, out),
A = (|x| |W1|^T + |b1|) |W2|^T + |b2|  (for Q the p_r-weighted sum of the chosen leaves'
A; for a log-prob A of the chosen logit plus the row's largest A), with F = 1 unless a
test's docstring says otherwise, plus the project's 1e-5 absolute at default scale.  An
fp32 torch forward reaches 0.45 of that bound and a forward with every operand rounded to
22 bits 0.32, so the reference sits well inside it.  Each test prints its largest
err / bound; the measured maxima are in the docstrings.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
EPS = 2.0 ** -22
ROLLS = [(a, b) for a in range(1, 7) for b in range(a, 7)]
PROBS = np.array([1 / 36 if a == b else 2 / 36 for a, b in ROLLS], np.float64)
SCALES = {"default": (1.0, 1.0), "up_down": (8.0, 1 / 64), "down_up": (1 / 64, 8.0),
          "up_up": (8.0, 8.0), "down_down": (1 / 64, 1 / 64)}


def _net(H, A=500, scale="default", seed=0):
    """PolicyNet(H, A) with seeded weights, N(0, 0.5) biases and fc1.weight / the heads'
    weights multiplied by SCALES[scale] (the biases stay as drawn)."""
    from bgx.policy import PolicyNet
    torch.manual_seed(1000 * seed + H)
    net = PolicyNet(hidden_size=H, action_size=A)
    g = torch.Generator().manual_seed(77 + H + 1000 * A)
    s1, s2 = SCALES[scale]
    with torch.no_grad():
        for b in (net.fc1.bias, net.action_head.bias, net.value_head.bias):
            b.copy_(torch.randn(b.shape, generator=g) * 0.5)
        net.fc1.weight.mul_(s1)
        net.action_head.weight.mul_(s2)
        net.value_head.weight.mul_(s2)
    return net.cuda()


def _w64(net):
    return [t.detach().cpu().double().numpy() for t in (net.fc1.weight, net.fc1.bias, net.action_head.weight,
                                                        net.action_head.bias, net.value_head.weight,
                                                        net.value_head.bias)]


# ---------------------------------------------------------------- 1. value evaluators --

VALUE_WIDTHS = [7, 24, 48, 64, 65, 96, 100, 127]      # NT = 1 .. 8 (see the table in DESIGN.md §5)
N_LEAVES = 153_470                                     # of the 16 roots below (a property of the lanes)


@pytest.fixture(scope="module")
def roots():
    """One engine of 16 roots (MT dice, fixed seeds, 25 random-policy steps) with, from the
    CPU oracle, the leaf count of every (lane, move, roll) job in the evaluator's job order:
    job = (lane_off[lane] + move) * 21 + roll, lane_off = the exclusive scan of the legal
    counts over PLAYER1's lanes first, then PLAYER2's (k_scan, by_mover)."""
    import bgx
    B = 16
    eng = bgx.Engine(batch=B, max_moves=500, dice="mt", auto_reset=True)
    eng.seed(np.arange(1200, 1200 + B, dtype=np.uint32))
    eng.reset()
    rng = np.random.RandomState(2)
    for _ in range(25):
        nm = eng.n_moves().cpu().numpy()
        eng.step(torch.from_numpy(np.array([rng.randint(k) if k else 0 for k in nm], np.int32)).cuda())
    rec, mv, _ = eng.lanes()
    rec, mv = rec.cpu().numpy(), mv.cpu().numpy().view(np.uint64)
    n = eng.n_moves().cpu().numpy().astype(np.int64)
    mover = rec[:, 52].astype(np.int64) & 1
    # both repliers and both enumerators (doubles / non-doubles root rolls) feed the evaluator
    assert set(mover[n > 0]) == {0, 1}
    assert int(((rec[:, 53] == rec[:, 54]) & (n > 0)).sum()) >= 1
    order = np.concatenate([np.nonzero(mover == 0)[0], np.nonzero(mover == 1)[0]])
    lane_off = np.zeros(B, np.int64)
    lane_off[order] = np.concatenate([[0], np.cumsum(n[order])[:-1]])
    rows = int(n.sum())
    job_leaves = np.zeros(rows * 21, np.int64)
    for i in range(B):
        for a in range(int(n[i])):
            _, counts = O.two_ply_leaves(rec[i, :52].view(np.int8), int(mover[i]), int(mv[i, a]))
            job_leaves[(lane_off[i] + a) * 21:(lane_off[i] + a + 1) * 21] = counts
    assert int(job_leaves.sum()) == N_LEAVES and N_LEAVES >= 30_000
    return eng, n, lane_off, job_leaves


def _run_two_ply(eng, net, dbg, tmp_path, unfactored=False, want_q=False):
    """two_ply under BGX_2PLY_DUMP; returns (slot indices of the valid leaves, their jobs,
    V of the kernel, V in fp64, the running-error bound's A per leaf, the call's outputs)."""
    from bgx.search import ValueHead, two_ply
    pre = str(tmp_path / "d")
    dbg.setenv("BGX_2PLY_DUMP", pre)
    if unfactored:
        dbg.setenv("BGX_2PLY_UNFACTORED", "1")
    out = two_ply(eng, ValueHead(net), want_q=want_q)
    dbg.delenv("BGX_2PLY_DUMP")
    keys = np.fromfile(pre + ".keys", np.uint32).reshape(-1, 4)
    tags = np.fromfile(pre + ".tags", np.uint32)
    v = np.fromfile(pre + ".v", np.float32)
    side = np.fromfile(pre + ".side", np.uint32).reshape(-1, 4)
    ml = np.fromfile(pre + ".ml", np.uint8)
    W1, b1, _, _, wv, bv = _w64(net)
    idx, vref = O.leaf_values(W1, b1, wv.ravel(), float(bv[0]), keys, tags, side, ml)
    # the same encoding through |W1|, |b1|, |wv|, |bv|: features are >= 0, so this is A
    idx2, bound = O.leaf_values(np.abs(W1), np.abs(b1), np.abs(wv).ravel(), abs(float(bv[0])), keys, tags, side, ml)
    assert np.array_equal(idx, idx2)
    job = (tags[idx] & 0x1FFFFFFF).astype(np.int64)
    return idx, job, v[idx].astype(np.float64), vref, bound, out


def _check_leaves(H, idx, job, v, vref, bound, out, job_leaves, default_scale, what):
    # no leaf skipped: every job's valid pool slots are exactly the oracle's leaves of it
    assert len(idx) == N_LEAVES == out[3]["leaves"]
    assert np.array_equal(np.bincount(job, minlength=len(job_leaves)), job_leaves)
    err = np.abs(v - vref)
    ratio = err / (EPS * bound)
    print(f"[widths] {what} H={H}: {len(idx)} leaves, max err {err.max():.3e}, max err/bound {ratio.max():.3f}")
    if default_scale:
        bad = err >= 1e-6
    else:
        bad = ratio > 1.0
    assert not bad.any(), (H, int(bad.sum()), float(err.max()), float(ratio.max()), (idx[bad][:16] % 64).tolist())


@pytest.mark.parametrize("unfactored", [False, True])
@pytest.mark.parametrize("H", VALUE_WIDTHS)
def test_two_ply_every_leaf_every_width(roots, dbg, tmp_path, H, unfactored):
    """V of every surviving leaf of the 16 roots (153,470, the same for every H) at every
    NT = 1..8 of k_eval and k_rowpart, factored and full 13-k-block form, against the fp64
    MLP on the leaf's own encoding within 1e-6.  Measured on an MI355X: the largest error
    grows with the width from 3.4e-8 (H = 7) to 2.6e-7 (H = 127), 0.06-0.12 of 2^-22 * A."""
    eng, n, lane_off, job_leaves = roots
    res = _run_two_ply(eng, _net(H), dbg, tmp_path, unfactored)
    _check_leaves(H, *res, job_leaves, True, "2-ply unfactored" if unfactored else "2-ply factored")


@pytest.mark.parametrize("scale", ["up_down", "down_up"])
@pytest.mark.parametrize("unfactored", [False, True])
@pytest.mark.parametrize("H", [24, 65])
def test_two_ply_every_leaf_scaled_weights(roots, dbg, tmp_path, H, unfactored, scale):
    """The every-leaf check with fc1.weight x 8, value_head.weight / 64 and with fc1.weight
    / 64, value_head.weight x 8 (|b1| about 100 x |W1|: the bias rides a constant-1 feature
    inside the split W1, so e1 has to cover it), within 2^-22 * A per leaf.  Measured
    err / bound: at most 0.24 (H = 24, fc1 x 8) and 0.15 (H = 65, fc1 / 64)."""
    eng, n, lane_off, job_leaves = roots
    res = _run_two_ply(eng, _net(H, scale=scale), dbg, tmp_path, unfactored)
    _check_leaves(H, *res, job_leaves, False, f"2-ply {scale} unfactored={unfactored}")


@pytest.mark.parametrize("H", VALUE_WIDTHS)
def test_two_ply_q_and_choice_every_width(roots, dbg, tmp_path, H):
    """Q(a) = sum_r p_r min over the job's leaves of the fp64 V, the segments rebuilt from
    the dumped tags (job = tag & 0x1FFFFFFF, row = job // 21, roll = job % 21; the roots
    fixture checks that map against the oracle's per-job leaf counts), within
    2^-22 * sum_r p_r A(chosen leaf) and 1e-5; best = the first argmax of the returned Q.
    Measured err / bound: at most 0.16 (H = 7), 0.02-0.07 at the other widths."""
    eng, n, lane_off, job_leaves = roots
    idx, job, v, vref, bound, (best, bestq, q, stats) = _run_two_ply(eng, _net(H), dbg, tmp_path, want_q=True)
    assert np.array_equal(np.bincount(job, minlength=len(job_leaves)), job_leaves)
    order = np.lexsort((vref, job))                     # by job, the smallest V first
    starts = np.concatenate([[0], np.cumsum(job_leaves)[:-1]])
    minv, mina = vref[order][starts].reshape(-1, 21), bound[order][starts].reshape(-1, 21)
    qref, qtol = minv @ PROBS, EPS * (mina @ PROBS)
    q, best, bestq = q.cpu().numpy(), best.cpu().numpy(), bestq.cpu().numpy()
    worst = 0.0
    for i in range(eng.batch):
        k, o = int(n[i]), int(lane_off[i])
        assert np.isnan(q[i, k:]).all()
        if k == 0:
            continue
        err = np.abs(q[i, :k].astype(np.float64) - qref[o:o + k])
        worst = max(worst, float((err / qtol[o:o + k]).max()))
        assert (err <= qtol[o:o + k]).all() and err.max() < TOL, (H, i, float(err.max()))
        assert best[i] == int(np.argmax(q[i, :k])) and bestq[i] == q[i, best[i]]
    print(f"[widths] 2-ply Q H={H}: max err/bound {worst:.3f}")


def _one_ply_check(eng, n, net, what, default_scale):
    from bgx.search import ValueHead, one_ply
    best, bestv, vals = one_ply(eng, ValueHead(net), want_values=True)
    x = eng.legal_features().double()
    x[..., 97] = torch.round(x[..., 97] * 15) / 15      # off / 15 exactly, not its fp32 rounding
    x[..., 195] = torch.round(x[..., 195] * 15) / 15
    W1, b1, _, _, wv, bv = [torch.from_numpy(w).cuda() for w in _w64(net)]
    ref = (torch.relu(x @ W1.t() + b1) @ wv.t() + bv).squeeze(-1).cpu().numpy()
    bound = ((x @ W1.abs().t() + b1.abs()) @ wv.abs().t() + bv.abs()).squeeze(-1).cpu().numpy()
    best, bestv, vals = best.cpu().numpy(), bestv.cpu().numpy(), vals.cpu().numpy()
    worst = 0.0
    for i in range(eng.batch):
        k = int(n[i])
        assert np.isnan(vals[i, k:]).all()              # unused columns stay NaN
        if k == 0:
            continue
        err = np.abs(vals[i, :k].astype(np.float64) - ref[i, :k])
        worst = max(worst, float((err / (EPS * bound[i, :k])).max()))
        assert (err <= EPS * bound[i, :k]).all(), (what, i, float(err.max()))
        if default_scale:
            assert err.max() < TOL
        assert best[i] == int(np.argmax(vals[i, :k])) and bestv[i] == vals[i, best[i]]
    print(f"[widths] 1-ply {what}: max err/bound {worst:.3f}")


@pytest.mark.parametrize("H", VALUE_WIDTHS)
def test_one_ply_every_width(roots, H):
    """k_eval_rows at every NT = 1..8: V of every legal afterstate of the 16 lanes against
    fp64 V(legal_features) within 2^-22 * A and 1e-5; best = the first argmax of the
    returned values; columns past the legal count stay NaN.  Measured err / bound: at most
    0.08 (0.21 with the scaled weights of the next test)."""
    eng, n, _, _ = roots
    _one_ply_check(eng, n, _net(H), f"H={H}", True)


@pytest.mark.parametrize("scale", ["up_down", "down_up"])
@pytest.mark.parametrize("H", [24, 65])
def test_one_ply_scaled_weights(roots, H, scale):
    """The 1-ply check with the scaled weights of test_two_ply_every_leaf_scaled_weights,
    within 2^-22 * A.  Measured err / bound: at most 0.21."""
    eng, n, _, _ = roots
    _one_ply_check(eng, n, _net(H, scale=scale), f"H={H} {scale}", False)


# ------------------------------------------------------------------- 2. policy kernel --

def _policy_records(golden, A, tiny_rows=False):
    """600 positions of the movegen / features goldens with the legal counts overwritten:
    rows 0..255 cycle through 0, 1, 31, 32, 33, 64, 65, A - 1, A (more gathered rows than the
    extra workgroups take: they stay on the main waves, unskipped); rows 256..511 hold 44
    count-0 rows and 10 rows with count = A among counts <= 32 (both extra workgroups of the
    window run, at the default heavy bound and at 32); rows 512..599 hold a few of each
    among small counts.  Every count is clipped to A.  tiny_rows: rows 0..15 keep two
    occupied points only (tiny hidden activations next to ordinary positions in their wave)."""
    feat, mg = golden("features"), golden("movegen")
    idx = feat["obs_idx"][:600]
    boards = np.array(mg["boards"][idx], np.int8)
    players = np.asarray(feat["obs_player"][:600])
    if tiny_rows:
        for i in range(16):
            keep = np.nonzero(boards[i])[0][:2]
            b = np.zeros(52, np.int8)
            b[keep] = boards[i, keep]
            boards[i] = b
    pat = np.array([0, 1, 31, 32, 33, 64, 65, A - 1, A])
    rng = np.random.RandomState(A)
    c = np.empty(600, np.int64)
    c[:256] = pat[np.arange(256) % 9]
    c[256:512] = rng.randint(1, 33, 256)
    c[256:512][rng.permutation(256)[:54]] = [0] * 44 + [A] * 10
    c[512:] = rng.randint(1, 31, 88)
    c[512:530] = np.repeat(pat, 2)
    c = np.clip(c, 0, A)
    assert int((c[256:512] == 0).sum()) >= 40 and int((c == A).sum()) >= 10
    r = np.zeros((600, 64), np.uint8)
    r[:, :52] = boards.view(np.uint8)
    r[:, 52] = players
    r[:, 60] = c & 0xFF
    r[:, 61] = c >> 8
    return torch.from_numpy(r).cuda()


def _policy_ref(net, rec):
    """fp64 logits [n, A], values [n], their running-error A's, and the legal counts."""
    from bgx.engine import encode_records
    x = encode_records(rec).double()
    x[:, 97] = rec[:, 50].double() / 15                 # off / 15 exactly, not its fp32 rounding
    x[:, 195] = rec[:, 51].double() / 15
    W1, b1, Wa, ba, wv, bv = [torch.from_numpy(w).cuda() for w in _w64(net)]
    h = torch.relu(x @ W1.t() + b1)
    ha = x @ W1.abs().t() + b1.abs()
    counts = rec[:, 60].long() | (rec[:, 61].long() << 8)
    return (h @ Wa.t() + ba, (h @ wv.t() + bv).squeeze(1), ha @ Wa.abs().t() + ba.abs(),
            (ha @ wv.abs().t() + bv.abs()).squeeze(1), counts)


def _logp_ref(lg, lga, counts, a):
    from bgx.policy import MASK_LOG
    A = lg.shape[1]
    legal = torch.arange(A, device=lg.device)[None] < counts[:, None]
    masked = torch.where(legal, lg, lg + MASK_LOG)
    lsm = torch.log_softmax(masked, -1).gather(1, a.long()[:, None]).squeeze(1)
    # Categorical.log_prob clamps the probability to [eps, 1 - eps] (k_policy_act's epilogue)
    ref = lsm.clamp(-15.942384719848633, -1.1920930376163597e-07)
    bound = EPS * (lga.gather(1, a.long()[:, None]).squeeze(1) + lga.max(1).values)
    return ref, bound + 4 * TOL * (counts == 0), masked


def _check_policy(net, rec, what, default_scale, seed=3, factor=None):
    """Logits, value column, value_out, and the log-prob of the drawn action, through
    MODE -1 (want_logits) and MODE 0 (the sampling call), against fp64, within
    factor[kind] (default 1) times the running-error bound."""
    A = net.action_head.out_features
    lg, v, lga, va, counts = _policy_ref(net, rec)
    a1, lp1, v1, logits = net.act(rec, seed=seed, step=0, want_logits=True)
    a0, lp0, v0 = net.act(rec, seed=seed, step=1)
    assert logits.shape[1] == 32 * ((A + 32) // 32)
    e_l = (logits[:, :A].double() - lg).abs()
    e_v = (logits[:, A].double() - v).abs()
    e_v0 = (v0.double() - v).abs()
    r = {"logits": float((e_l / (EPS * lga)).max()), "value": float((e_v / (EPS * va)).max()),
         "value0": float((e_v0 / (EPS * va)).max())}
    assert torch.equal(v1, logits[:, A])                # value_out == the value column, bit for bit
    for a, lp, k in ((a1, lp1, "logp"), (a0, lp0, "logp0")):
        assert bool(((a >= 0) & (a < A)).all())
        assert bool(((a < counts) | (counts == 0)).all())
        ref, bound, _ = _logp_ref(lg, lga, counts, a)
        r[k] = float(((lp.double() - ref).abs() / bound).max())
    print(f"[widths] policy {what} n={rec.shape[0]}: max err/bound " + " ".join(f"{k}={x:.3f}" for k, x in r.items()))
    over = {k: x for k, x in r.items() if x > (factor or {}).get(k.rstrip("0"), 1.0)}
    assert not over, (what, r)
    if default_scale:
        assert max(float(e_l.max()), float(e_v.max()), float(e_v0.max())) < TOL
    return r


@pytest.mark.parametrize("H", [7, 32, 33, 72, 96, 127])
def test_policy_every_width(golden, H):
    """k_policy_act<T, -1> and <T, 0> at T = 1 ragged and full, 2, 3 ragged and full and 4
    ragged, 500 actions: every logit, the value column and the drawn action's log-prob
    against fp64, on 600 rows and on 583 (a ragged last wave).  Measured err / bound: logits
    at most 0.68, values 0.16, log-probs 0.66."""
    rec = _policy_records(golden, 500)
    net = _net(H)
    _check_policy(net, rec, f"H={H} A=500", True)
    _check_policy(net, rec[:600 - 17].contiguous(), f"H={H} A=500", True)


@pytest.mark.parametrize("A", [31, 32, 33, 100, 511])
@pytest.mark.parametrize("H", [33, 128])
def test_policy_action_counts(golden, dbg, H, A):
    """Action counts with 1, 2, 2, 4 and 16 output tiles: the value column inside the
    actions' tile 0 (31), alone in its tile (32), the very last column (511); the skip's
    o_s < vt test and the extra workgroups' ceil(OT / 4) tile split with fewer tiles than
    waves (waves with an empty tile range merge m = -inf states).  The fp64 checks, then the
    tile skip on against off at the default heavy bound and at 32.  Measured err / bound:
    logits at most 0.57, values 0.34, log-probs 0.49."""
    from test_gpu_policy import _act_both, _assert_same
    rec = _policy_records(golden, A)
    net = _net(H, A)
    _check_policy(net, rec, f"H={H} A={A}", True)
    _check_policy(net, rec[:600 - 17].contiguous(), f"H={H} A={A}", True)
    for heavy in (None, "32"):
        if heavy:
            dbg.setenv("BGX_POLICY_HEAVY", heavy)
        _assert_same(*_act_both(net, rec, 9, 0, dbg), rec)
        _assert_same(*_act_both(net, rec[:600 - 17].contiguous(), 9, 1, dbg), rec[:600 - 17])
        # the skipping call itself against fp64 (the extra workgroups' rows included)
        dbg.setenv("BGX_POLICY_SKIP", "1")
        _check_policy(net, rec, f"H={H} A={A} heavy={heavy}", True, seed=5)


@pytest.mark.parametrize("H,A", [(72, 500), (128, 33)])
def test_policy_greedy_every_row(golden, H, A):
    """greedy=True == argmax of the fp64 masked logits.  A row may differ only where the
    fp64 top-two gap is below the two logits' summed tolerance (on count-0 rows plus two
    fp32 ulps of |z| ~ 110, 2 * 7.63e-6: every logit there carries the -103.28 mask and is
    rounded to that grid before the comparison); fewer than 1 % of rows may use that."""
    rec = _policy_records(golden, A)
    net = _net(H, A)
    lg, v, lga, va, counts = _policy_ref(net, rec)
    g = net.act(rec, greedy=True)[0].long()
    _, _, masked = _logp_ref(lg, lga, counts, g)
    top = masked.topk(2, dim=1)
    tol = EPS * lga.gather(1, top.indices).sum(1) + 2 * 7.63e-6 * (counts == 0)
    near = (top.values[:, 0] - top.values[:, 1]) < tol
    wrong = g != top.indices[:, 0]
    assert not bool((wrong & ~near).any()), (H, A, int((wrong & ~near).sum()))
    # a near-tie row must still have picked one of the two
    assert bool((g[wrong] == top.indices[wrong, 1]).all())
    assert int(near.sum()) < 0.01 * rec.shape[0]
    print(f"[widths] greedy H={H} A={A}: {int(near.sum())} near-tie rows, {int(wrong.sum())} differ")


@pytest.mark.parametrize("scale", ["up_up", "down_down", "up_down", "down_up"])
@pytest.mark.parametrize("H", [72, 128])
def test_policy_scaled_weights(golden, H, scale):
    """The three power-of-two scale paths (e1, e2 at pack time, the per-wave ex of the hidden
    split) away from default-init exponents: fc1 and the heads x 8 or / 64 in the four
    combinations, the biases as drawn; and a batch whose rows 0..15 keep two occupied points
    only and share their 32-row wave with ordinary positions (pins the per-wave ex).

    Measured err / bound with the heads x 8: logits at most 0.58, values 0.21, log-probs 0.16.
    With the heads / 64 the outputs are their biases plus a term 50 x smaller, and the
    kernel is over the bound: logits 3.46 (H = 128) and 2.74 (H = 72), values 1.41,
    log-probs 1.97.  The cause is the accumulation order: k_policy_act starts each output
    tile's fp32 accumulator at b2 * 2^E and adds the 6 T MFMA results of GEMM2 onto it, so
    every one of those additions (24 at H = 128, 18 at H = 72) rounds at the bias's
    magnitude, half an fp32 ulp of |b2| each, where a dot product followed by one bias add
    rounds there once; A is then about |b2| and 2^-22 * A only four such half-ulps.  These
    cases take the factor measured x 2, capped at 4 (2^-20 * A, above which it is a bug):
    logits 4.0, values 2.9, log-probs 3.9."""
    net = _net(H, scale=scale)
    factor = {"logits": 4.0, "value": 2.9, "logp": 3.9} if scale in ("down_down", "up_down") else None
    _check_policy(net, _policy_records(golden, 500), f"H={H} {scale}", False, factor=factor)
    _check_policy(net, _policy_records(golden, 500, tiny_rows=True), f"H={H} {scale} tiny", False, factor=factor)


# ------------------------------------------------------------- 3. PPO-side kernels --

@pytest.fixture(scope="module")
def rollout_records():
    """5,000 records of a short rollout at the default hidden (ragged: no multiple of 256)."""
    from bgx.train import PPOTrainer
    tr = PPOTrainer(batch=2048, horizon=3, seed=5, chunk=8192)
    tr.rollout()
    return tr.buf["records"].reshape(-1, 64)[:5000].clone().contiguous()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("hidden", [4, 32, 36, 72, 96, 100, 124])
def test_fc1_records_every_width(rollout_records, hidden):
    """k_fc1_rec at T = 1, 3 and 4 and on both store paths (36, 100, 124: the 8-byte stores;
    the others the permlane32_swap + 16-byte stores): every output within 1.01 fp16 ulp
    (floor 2^-6) of relu(fp16(x) W1h^T + b1h) in fp32 and in fp64; no store past the last
    row (64 NaN guard halves stay NaN); hmax2 = max_row sum h^2 of the returned h."""
    from bgx import _lib
    from bgx._lib import check
    from bgx.engine import encode_records
    rec = rollout_records
    n = rec.shape[0]
    L = _lib.load()
    torch.manual_seed(1)
    W1h = (torch.randn(hidden, 198, device="cuda") * 0.2).half()
    b1h = (torch.randn(hidden, device="cuda") * 0.1).half()
    pk = torch.empty(L.bgx_fc1_packed_size(hidden), dtype=torch.uint8, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(L.bgx_fc1_pack(_p(W1h), hidden, _p(pk), s), "bgx_fc1_pack")
    buf = torch.full((n * hidden + 64,), float("nan"), dtype=torch.float16, device="cuda")
    hmax2 = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(L.bgx_fc1_records_ex(_p(rec), n, _p(pk), _p(b1h), hidden, _p(buf), _p(hmax2), s), "bgx_fc1_records_ex")
    h = buf[:n * hidden].view(n, hidden)
    assert bool(torch.isnan(buf[n * hidden:]).all())
    assert bool(torch.isfinite(h).all())
    x = encode_records(rec, torch.float16)
    ref32 = torch.relu(x.float() @ W1h.float().t() + b1h.float())
    ref64 = torch.relu(x.double() @ W1h.double().t() + b1h.double())
    for ref in (ref32.double(), ref64):
        ulp = torch.clamp(ref.abs(), min=2.0 ** -6) * 2.0 ** -10
        assert bool(((h.double() - ref).abs() <= ulp * 1.01).all()), hidden
    want = float((h.double() ** 2).sum(1).max())
    assert want > 0 and abs(float(hmax2) - want) <= 1e-5 * want, (float(hmax2), want)


@pytest.mark.parametrize("n", [1, 1000, 4097])
@pytest.mark.parametrize("hidden", [8, 40, 128, 136, 256])
def test_relu_backward_direct(hidden, n):
    """bgx_relu_backward on its own: dh == where(h > 0, dh, 0) bit for bit (h with about
    40 % exact zeros and some -0.0), the summed colsum rows == the fp64 column sums of the
    masked dh within 2^-20 * sum |dh| per column (fp32 partial sums of fp16 values), and
    every colsum row written: zeros for a block that had no row to walk (bgx.h)."""
    from bgx import _lib
    L = _lib.load()
    blocks = 64
    g = torch.Generator(device="cuda").manual_seed(hidden * 10007 + n)
    h = torch.randn(n, hidden, device="cuda", generator=g).half()
    u = torch.rand(n, hidden, device="cuda", generator=g)
    h = torch.where(u < 0.4, torch.zeros_like(h), h)
    h = torch.where(u < 0.05, -torch.zeros_like(h), h)
    assert bool((h.view(torch.int16) == -32768).any()) or n == 1
    dh0 = torch.randn(n, hidden, device="cuda", generator=g).half()
    dh = dh0.clone()
    colsum = torch.full((blocks, hidden), float("nan"), dtype=torch.float32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bgx_relu_backward(_p(dh), _p(h), n, hidden, _p(colsum), blocks, s) == 0
    want = torch.where(h > 0, dh0, torch.zeros_like(dh0))
    assert torch.equal(dh.view(torch.int16), want.view(torch.int16))
    assert bool(torch.isfinite(colsum).all())
    err = (colsum.double().sum(0) - want.double().sum(0)).abs()
    assert bool((err <= 2.0 ** -20 * want.double().abs().sum(0)).all()), float(err.max())
    rows_per_block = 256 // (hidden // 8)                # block b starts at row b * rows_per_block
    idle = torch.arange(blocks, device="cuda") * rows_per_block >= n
    assert bool((colsum[idle] == 0).all())


@pytest.mark.parametrize("hidden", [12, 264])
def test_relu_backward_refuses_bad_width(hidden):
    from bgx import _lib
    L = _lib.load()
    t = torch.zeros(8, 264, dtype=torch.float16, device="cuda")
    cs = torch.zeros(4, 264, dtype=torch.float32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bgx_relu_backward(_p(t), _p(t.clone()), 8, hidden, _p(cs), 4, s) == _lib.BGX_EINVAL
