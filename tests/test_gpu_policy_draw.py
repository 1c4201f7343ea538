"""Which action the device draws, against a host replica (policy_draw_ref.py).

k_policy_act's sampled action is a documented function of (seed, step, row, action): the
argmax of masked logit + Gumbel noise, the noise hashed from those four.  The other policy
modules pin the logits, the log-prob and the greedy argmax against fp64 and compare the
kernel's forms with each other; here every sampled action of every row is compared with
the replica's winner over the fp64 masked logits of test_gpu_widths._policy_ref (computed
from the weights, not by the kernel), so noise shared between rows, steps or seeds, a
dropped winning key or a wrong merge shows as a differing row.

Row rule (the shape of test_gpu_widths.test_policy_greedy_every_row): the drawn action
equals the replica's winner; it may differ only where the replica's top-two key gap is
below the row's band, and is then the runner-up; fewer than 1 % of a case's rows may lie
inside their band.  Band = the two keys' logit tolerances EPS * lga (as the greedy test sums
them) + 2 * 7.63e-6 on count-0 rows (two fp32 ulps of |z| ~ 110 there) + TAU.

TAU, the tolerance for the kernel's fp32 evaluation of the noise (hardware log2, a series
near u = 1), is measured, not assumed: test_noise_tolerance_zero_logits runs a net whose
logits are all exactly 0, where only the noise decides, on 2^17 rows; G is the largest fp64
top-two gap among the rows whose action differs from the replica's, and TAU = 2 G.

bgx_random_act (the arena's baseline opponent) is compared with its replica exactly."""
import ctypes

import numpy as np
import pytest
import torch

import policy_draw_ref as R
from test_gpu_policy_noise import SEEDS_STEPS
from test_gpu_widths import EPS, _logp_ref, _net, _policy_records, _policy_ref

pytestmark = pytest.mark.gpu

# Measured on an MI355X (test_noise_tolerance_zero_logits): no row of the 131,072 differs,
# G = 0, so TAU = 2 G = 0.  u has 23 bits: at the top of 500 keys two noise values are
# either equal (6 rows; the lower action wins, in the kernel and in the replica) or at least
# 1.7e-5 apart there -- typically 6e-5, the spacing of the u grid at u ~ 1 - 1/500 -- while
# a correctly rounded fp32 evaluation is off by 1.4e-6 at most.
TAU = 0.0
G_LIMIT = 16 * 1.4e-6                                  # above this the noise is wrong, not rounded
SEEDS_STEPS_ALL = SEEDS_STEPS + [(2 ** 64 - 1, 2 ** 32 - 1), (-7, 12)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Ref:
    """The fp64 masked logits of one (net, records) pair, computed once, and the row rule
    against them."""

    def __init__(self, net, rec, what):
        self.net, self.rec, self.what = net, rec, what
        self.A = net.action_head.out_features
        lg, _, lga, _, counts = _policy_ref(net, rec)
        _, _, masked = _logp_ref(lg, lga, counts, torch.zeros_like(counts))
        self.masked, self.lga = masked.cpu().numpy(), lga.cpu().numpy()
        self.zero = (counts == 0).cpu().numpy()
        self.n = rec.shape[0]
        self.rows = np.arange(self.n)
        self.draws = {}
        self.calls = self.near = self.differ = self.worst = 0

    def draw(self, seed, step):
        key = (int(seed) & R.M64, int(step) & R.M32)
        if key not in self.draws:
            win, run, gap = R.draw(self.masked, key[0], key[1], self.rows)
            band = EPS * (self.lga[self.rows, win] + self.lga[self.rows, run]) + 2 * 7.63e-6 * self.zero + TAU
            self.draws[key] = (win, run, gap < band)
        return self.draws[key]

    def check(self, a, seed, step, tag=""):
        a = a.cpu().numpy().astype(np.int64)
        win, run, near = self.draw(seed, step)
        assert a.shape == win.shape and a.min() >= 0 and a.max() < self.A, (self.what, tag)
        wrong = a != win
        bad = wrong & ~near
        assert not bad.any(), (self.what, tag, seed, step, int(bad.sum()), np.nonzero(bad)[0][:8].tolist(),
                               a[bad][:8].tolist(), win[bad][:8].tolist())
        assert (a[wrong] == run[wrong]).all(), (self.what, tag, seed, step)
        assert int(near.sum()) < 0.01 * self.n, (self.what, tag, int(near.sum()))
        self.calls += 1
        self.near += int(near.sum())
        self.differ += int(wrong.sum())
        self.worst = max(self.worst, int(near.sum()))

    def report(self):
        print(f"[draw] {self.what} n={self.n}: {self.calls} calls, near-tie rows {self.near} in all "
              f"(at most {self.worst} = {100 * self.worst / self.n:.2f} % in one call), {self.differ} differ")


def _both_modes(ref, seed, step, tag):
    """The MODE 0 call and the MODE -1 call (want_logits) at the same step: both follow the
    row rule and draw the same actions."""
    a0 = ref.net.act(ref.rec, seed=seed, step=step)[0].clone()
    a1 = ref.net.act(ref.rec, seed=seed, step=step, want_logits=True)[0].clone()
    ref.check(a0, seed, step, tag + " mode 0")
    ref.check(a1, seed, step, tag + " mode -1")
    assert torch.equal(a0, a1), (ref.what, tag, seed, step)
    return a0


def _walk(ref, dbg, seeds_steps, heavies=(None, "32"), skips=("1", "0")):
    for heavy in heavies:
        if heavy:
            dbg.setenv("BGX_POLICY_HEAVY", heavy)
        for skip in skips:
            dbg.setenv("BGX_POLICY_SKIP", skip)
            for seed, step in seeds_steps:
                _both_modes(ref, seed, step, f"skip={skip} heavy={heavy}")
    ref.report()


# ------------------------------------------------------------------ the noise tolerance --

def test_noise_tolerance_zero_logits(golden):
    """Action head weight and bias zero: every logit is exactly 0 and the noise alone decides.
    2^17 rows with 500 legal actions.  G = the largest fp64 top-two gap among the rows where
    the kernel's action differs from the replica's; G < 16 x 1.4e-6 (what a correctly
    rounded fp32 evaluation of -log(-log(u)) is off by) and 2 G <= TAU.

    Measured on an MI355X: 0 of 131,072 rows differ, G = 0 (the replica's smallest non-zero
    top-two gap there is 1.74e-5; 6 rows hold an exact tie of their two best keys, which the
    kernel and the replica both give to the lower action)."""
    n = 1 << 17
    net = _net(128)
    with torch.no_grad():
        net.action_head.weight.zero_()
        net.action_head.bias.zero_()
    rec = _policy_records(golden, 500).repeat((n + 599) // 600, 1)[:n].contiguous()
    rec[:, 60], rec[:, 61] = 500 & 0xFF, 500 >> 8
    a, _, _, logits = net.act(rec[:4096].contiguous(), seed=11, step=5, want_logits=True)
    assert bool((logits[:, :500] == 0).all())
    a = net.act(rec, seed=11, step=5)[0]
    assert torch.equal(a[:4096], net.act(rec[:4096].contiguous(), seed=11, step=5)[0])
    a = a.cpu().numpy().astype(np.int64)
    win, run, gap = R.draw(np.zeros((n, 500)), 11, 5, np.arange(n))
    wrong = a != win
    G = float(gap[wrong].max()) if wrong.any() else 0.0
    print(f"[draw] zero logits n={n}: {int(wrong.sum())} rows differ, G = {G:.3e}; exact ties {int((gap == 0).sum())}, "
          f"smallest non-zero gap {gap[gap > 0].min():.3e}")
    assert (a[wrong] == run[wrong]).all()
    assert G < G_LIMIT, G
    assert 2 * G <= TAU, (G, TAU)
    # every action is drawn, about equally often (500 bins of 262 expected)
    f = np.bincount(a, minlength=500)
    assert f.min() > 150 and f.max() < 400


# ------------------------------------------------------------- every path of the tile loop --

@pytest.mark.parametrize("n", [600, 583])
@pytest.mark.parametrize("H", [33, 128])
def test_draw_every_path(golden, dbg, H, n):
    """T = 2 and 4, 500 actions, the count edges 0, 1, 31, 32, 33, 64, 65, 499, 500 in three
    windows (more gathered rows than the extra workgroups take; both extra workgroups
    running), 600 rows and a ragged last wave; eight (seed, step) pairs, 2^64 - 1 /
    2^32 - 1 and a negative seed among them; tile skip on and off; the heavy bound at its
    default and at 32; the sampling kernel and the logits kernel at the same step."""
    rec = _policy_records(golden, 500)[:n].contiguous()
    _walk(_Ref(_net(H), rec, f"paths H={H}"), dbg, SEEDS_STEPS_ALL)


@pytest.mark.parametrize("A", [31, 32, 33, 511])
def test_draw_value_column_and_tile_edges(golden, dbg, A):
    """The value column inside the actions' tile (31), alone in its tile (32), behind one
    action of its tile (33) and the very last column (511), H = 33: the drawn action is never
    A (the replica leaves the value column out) and follows the row rule."""
    ref = _Ref(_net(33, A), _policy_records(golden, A), f"value column A={A}")
    assert ref.masked.shape[1] == A
    _walk(ref, dbg, SEEDS_STEPS_ALL[2:6], heavies=(None,))


# ------------------------------------------------------- peaked and unskippable heads --

@pytest.mark.parametrize("mul", [8.0, 40.0])
def test_draw_peaked_heads(golden, dbg, mul):
    """The action head x 8 (a peaked distribution) and x 40 (the tile skip's logit bound
    fails: the wave reloads the tile it had hoped to skip)."""
    net = _net(128)
    with torch.no_grad():
        net.action_head.weight.mul_(mul)
    _walk(_Ref(net, _policy_records(golden, 500), f"head x{mul:g}"), dbg, SEEDS_STEPS_ALL[:4])


def test_draw_masked_winner(dbg):
    """Biases of +200 on the masked actions 70, 133, 300, 485 (test_gpu_policy_noise.
    test_masked_output_wins): a masked key beats every legal one.  The replica names which of
    the four the kernel drew, row by row."""
    import test_gpu_policy_noise as PN
    net = PN._net(128)
    hot = [70, 133, 300, 485]
    with torch.no_grad():
        net.action_head.bias[hot] += 200.0
    net.pack()
    c = PN._counts(100, False)
    c[c > 64] = 64
    ref = _Ref(net, PN._records(100, c, seed=5), "masked winner")
    for skip in ("1", "0"):
        dbg.setenv("BGX_POLICY_SKIP", skip)
        for seed, step in SEEDS_STEPS_ALL[:4]:
            a = _both_modes(ref, seed, step, f"skip={skip}").cpu().numpy()
            assert np.isin(a, hot).all() and len(set(a.tolist())) > 1
    ref.report()


# ----------------------------------------------------------------------------- the step --

def test_draw_step_counter(golden):
    """The noise's step is step + step_ctr[0] mod 2^32: 2^32 - 3 with a counter of 5 draws
    what step 2 draws, and advance_counter(2^32 - 1) takes the counter back by one."""
    net = _net(128)
    ref = _Ref(net, _policy_records(golden, 500), "step counter")
    ctr = torch.tensor([5], dtype=torch.int32, device="cuda")
    for want_logits in (False, True):
        a = net.act(ref.rec, seed=21, step=2 ** 32 - 3, step_ctr=ctr, want_logits=want_logits)[0]
        ref.check(a, 21, 2, "ctr 5")
        assert torch.equal(a, net.act(ref.rec, seed=21, step=2)[0])
    net.advance_counter(ctr, 2 ** 32 - 1)
    assert int(ctr.item()) == 4
    ref.check(net.act(ref.rec, seed=21, step=0, step_ctr=ctr)[0], 21, 4, "ctr 4")
    ref.check(net.act(ref.rec, seed=21, step=2 ** 32 - 1, step_ctr=ctr)[0], 21, 3, "ctr 4 - 1")
    # steps 2, 3 and 4 are three different draws
    d = [ref.draw(21, t)[0] for t in (2, 3, 4)]
    assert (d[0] != d[1]).mean() > 0.2 and (d[1] != d[2]).mean() > 0.2
    ref.report()


def test_draw_engine_records_in_place():
    """act(engine): the lane records read in place, rows = the lanes, on the game's own
    counts after 30 self-play steps; B = 3,000 leaves a ragged last wave."""
    import bgx
    net = _net(128)
    B = 3000
    eng = bgx.Engine(batch=B, dice="philox", seed=21)
    eng.reset(want_obs=False)
    for t in range(30):
        eng.step(net.act(eng, seed=9, step=t)[0], want_obs=False, want_info=False)
    rec = eng.records().clone()
    counts = rec[:, 60].int() | (rec[:, 61].int() << 8)
    assert int((counts == 0).sum()) > 0 and int(counts.max()) > 64
    ref = _Ref(net, rec, "engine in place")
    for seed, step in ((9, 30), (2 ** 64 - 1, 2 ** 32 - 1)):
        rec_out = torch.empty(B, 64, dtype=torch.uint8, device="cuda")
        a = net.act(eng, seed=seed, step=step, records_out=rec_out)[0].clone()
        assert torch.equal(rec_out, rec)
        ref.check(a, seed, step, "engine")
        assert torch.equal(a, net.act(rec, seed=seed, step=step)[0])
    assert eng.error() == 0
    ref.report()


# ----------------------------------------------------------------------- bgx_random_act --

def _random_act(L, rec, n, seed, step, out):
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return L.bgx_random_act(_p(rec), n, seed, step, _p(out), s)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_random_act_matches_replica(n):
    """k_random_act == the replica exactly: one thread, one block less one, one block, one
    block plus one, twenty blocks; counts cycling through 0, 1, 2, 500, 65535; seeds 0, 17,
    2^64 - 1; steps 0, 1, 2^32 - 1.  No store past the last lane."""
    from bgx import _lib
    L = _lib.load()
    counts = np.array([0, 1, 2, 500, 65535])[np.arange(n) % 5]
    rec = np.random.default_rng(n).integers(0, 256, (n, 64)).astype(np.uint8)
    rec[:, 60], rec[:, 61] = counts & 0xFF, counts >> 8
    rec = torch.from_numpy(rec).cuda()
    seen = set()
    for seed in (0, 17, 2 ** 64 - 1):
        for step in (0, 1, 2 ** 32 - 1):
            out = torch.full((n + 64,), -77, dtype=torch.int32, device="cuda")
            assert _random_act(L, rec, n, seed, step, out) == 0
            got = out.cpu().numpy()
            want = R.random_act(counts, seed, step)
            assert np.array_equal(got[:n], want), (n, seed, step)
            assert (got[n:] == -77).all()
            assert (got[:n] < np.maximum(counts, 1)).all() and (got[:n] >= 0).all()
            seen.add(got[:n].tobytes())
    assert len(seen) == (1 if n == 1 else 9)           # n = 1: count 0, always action 0


def test_random_player_on_engine():
    """RandomPlayer(seed).act(eng, None, step) == the replica on eng.records(), 1,000 lanes
    after 12 random steps (the seed masked to 64 bits, the step to 32)."""
    import bgx
    from bgx.arena import RandomPlayer
    eng = bgx.Engine(batch=1000, dice="philox", seed=3)
    eng.reset(want_obs=False)
    pl = RandomPlayer(5)
    for t in range(12):
        eng.step(pl.act(eng, None, t), want_obs=False, want_info=False)
    rec = eng.records().cpu().numpy()
    counts = rec[:, 60].astype(np.int64) | (rec[:, 61].astype(np.int64) << 8)
    assert counts.max() > 1
    for seed, step in ((5, 12), (-3, 2 ** 32 + 6), (2 ** 64 - 1, 2 ** 32 - 1)):
        a = RandomPlayer(seed).act(eng, None, step).cpu().numpy()
        assert np.array_equal(a, R.random_act(counts, seed, step)), (seed, step)
        assert ((a < counts) | (counts == 0)).all()
    assert eng.error() == 0


def test_random_act_refuses_bad_arguments():
    """Null records, n <= 0 (0 included) and a null output give BGX_EINVAL and launch
    nothing: the output keeps its fill."""
    from bgx import _lib
    L = _lib.load()
    rec = torch.zeros(8, 64, dtype=torch.uint8, device="cuda")
    rec[:, 60] = 9
    out = torch.full((8,), -77, dtype=torch.int32, device="cuda")
    assert _random_act(L, None, 8, 1, 0, out) == _lib.BGX_EINVAL
    assert _random_act(L, rec, 0, 1, 0, out) == _lib.BGX_EINVAL
    assert _random_act(L, rec, -1, 1, 0, out) == _lib.BGX_EINVAL
    assert _random_act(L, rec, 8, 1, 0, None) == _lib.BGX_EINVAL
    torch.cuda.synchronize()
    assert bool((out == -77).all())
    assert _random_act(L, rec, 8, 1, 0, out) == 0
    assert np.array_equal(out.cpu().numpy(), R.random_act(np.full(8, 9), 1, 0))
