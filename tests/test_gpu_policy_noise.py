"""The policy kernel's noise guard (bg_mlp.hip, k_policy_act's tile loop): a tile's Gumbel
keys are drawn only where they can beat the best key of the lane's ROW (both lane halves),
not of the lane.  BGX_POLICY_ROWBEST 0 = the lane-level guard, 1 = the row-level guard
(gathered rows of main waves drawing nothing), 2 = that per quarter tile, the default.
Every form is exact: actions, log-probs, values and logits are compared with torch.equal
on small hand-made record batches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# one 32-row wave holds all of these: the half-masked rows (1-4 legal moves: every output
# of lane half 1 is masked from tile 0 on), the group and tile edges, and two gathered
# rows (count 0, more than 64 legal actions)
EDGE = [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 40, 64, 0, 100]
SEEDS_STEPS = [(1, 0), (1, 7), (20, 3), (20, 4), (0xDEADBEEF12, 1), (0xDEADBEEF12, 900)]
FORMS = ("0", "1", "2")


def _records(n, counts, seed=0):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 64), np.uint8)
    r[:, :48] = rng.integers(0, 6, (n, 48))
    r[:, 48:52] = rng.integers(0, 3, (n, 4))
    r[:, 52] = rng.integers(0, 2, n)
    c = np.asarray(counts, np.int64)
    assert len(c) == n
    r[:, 60] = c & 0xFF
    r[:, 61] = c >> 8
    return torch.from_numpy(r).cuda()


def _counts(n, overflow):
    """EDGE in the first wave; then ordinary rows with 1-64 legal moves, a few of them
    half-masked.  n = 300: 40 more gathered rows in the first 256-row window (42 in all:
    both of its extra workgroups run).  `overflow`: rows 32.. hold 68 gathered rows (70 in
    the window, more than kZCap = 64: they stay on the main waves, unskipped)."""
    rng = np.random.default_rng(n)
    c = rng.integers(1, 65, n)
    few = rng.random(n) < 0.15
    c[few] = rng.integers(1, 5, int(few.sum()))
    c[:len(EDGE)] = EDGE
    if n >= 300:
        c[100:140:2] = 0
        c[101:140:2] = 200
        c[270] = 0                                     # the second window's own extra workgroup
        c[271] = 500
    if overflow:
        c[32:100:2] = 0
        c[33:100:2] = 77
    return c


def _net(H):
    from bgx.policy import PolicyNet
    torch.manual_seed(H)
    net = PolicyNet(hidden_size=H).cuda()
    with torch.no_grad():
        net.action_head.weight.mul_(4.0)               # a spread of logits: winners beyond action 0
    net.pack()
    return net


def _act_forms(net, rec, seed, step, dbg, **kw):
    out = []
    for form in FORMS:
        dbg.setenv("BGX_POLICY_ROWBEST", form)
        out.append([t.clone() for t in net.act(rec, seed=seed, step=step, **kw)])
    dbg.delenv("BGX_POLICY_ROWBEST")
    return out


def _assert_forms_equal(outs, A):
    ref = outs[0]
    for o in outs[1:]:
        assert torch.equal(ref[0], o[0])               # actions
        assert torch.equal(ref[1], o[1])               # log-probs
        assert torch.equal(ref[2], o[2])               # values
        if len(ref) > 3:                               # logits: the columns the kernel writes
            assert torch.equal(ref[3][:, :A + 1], o[3][:, :A + 1])


@pytest.mark.parametrize("H", [128, 33])
@pytest.mark.parametrize("n", [32, 33, 100, 300])
def test_noise_guard_forms_equal(dbg, n, H):
    """Lane-level against row-level against quarter-tile guard: one wave (32), ragged (33,
    100), two windows (300); H = 128 and the padded width 33 (T = 2); tile skip on and off;
    the sampling kernel and the logits kernel (sampling and greedy).  n = 100 and 300 also
    with a window of more than kZCap gathered rows (n = 32 and 33 have fewer rows than
    kZCap).  Winners must fall in both lane halves."""
    net = _net(H)
    A = net.action_head.out_features
    halves = set()
    for overflow in ((False, True) if n >= 100 else (False,)):
        rec = _records(n, _counts(n, overflow), seed=n + overflow)
        for skip in ("1", "0"):
            dbg.setenv("BGX_POLICY_SKIP", skip)
            for seed, step in SEEDS_STEPS:
                outs = _act_forms(net, rec, seed, step, dbg)
                _assert_forms_equal(outs, A)
                halves |= set(((outs[0][0] >> 2) & 1).unique().tolist())
                _assert_forms_equal(_act_forms(net, rec, seed, step, dbg, want_logits=True), A)
            _assert_forms_equal(_act_forms(net, rec, 0, 0, dbg, greedy=True, want_logits=True), A)
    assert halves == {0, 1}


@pytest.mark.parametrize("only_value_tile", [False, True])
def test_masked_output_wins(dbg, only_value_tile):
    """Action biases of +200 on masked actions: a few at or above 64 and one in the value
    tile (480-499), or that one alone.  A masked key then beats every legal one and the
    logit bound forbids the tile skip, so no guard may drop those tiles: the sampled action
    is one of the biased masked actions (the value tile's, where it is alone) under every
    form, with the same log-prob."""
    net = _net(128)
    hot = [485] if only_value_tile else [70, 133, 300, 485]
    with torch.no_grad():
        net.action_head.bias[hot] += 200.0
    net.pack()
    n = 100
    c = _counts(n, False)
    c[c > 64] = 64                                     # every hot action is masked (or, count 0, all are)
    rec = _records(n, c, seed=5)
    for skip in ("1", "0"):
        dbg.setenv("BGX_POLICY_SKIP", skip)
        for seed, step in SEEDS_STEPS[:3]:
            outs = _act_forms(net, rec, seed, step, dbg)
            _assert_forms_equal(outs, 500)
            a = outs[0][0].cpu().numpy()
            assert np.isin(a, hot).all(), a
            if not only_value_tile:
                assert len(set(a.tolist())) > 1        # the noise decides among the hot actions


def test_every_row_one_legal_move(dbg):
    """The reset-like extreme: a 32-row wave whose rows all have one legal move, so every
    lane of half 1 is masked from tile 0 on.  Also with a ragged second wave."""
    net = _net(128)
    for n in (32, 45):
        rec = _records(n, np.ones(n, np.int64), seed=9)
        for skip in ("1", "0"):
            dbg.setenv("BGX_POLICY_SKIP", skip)
            for seed, step in SEEDS_STEPS:
                outs = _act_forms(net, rec, seed, step, dbg)
                _assert_forms_equal(outs, 500)
                assert bool((outs[0][0] == 0).all())   # exp(-103) of mass elsewhere
                _assert_forms_equal(_act_forms(net, rec, seed, step, dbg, want_logits=True), 500)
