"""k_policy_act after the load-latency changes (DESIGN.md §3.6, §8 "Policy load latency"):
bit-equality with the kernel before them.

The changes move loads (the next output tile's bias fragment, GEMM1's bias fragment and the
first W1 ring entries, a main wave's records) ahead of where their values are used and
change no arithmetic, so every output must keep its bits.  The expected arrays in
tests/golden/policy_latency.npz were recorded with the library built from the commit
before the change (tools/record_policy_latency.py, which runs `expected()` below under
BGX_LIB), never from the build under test.

Inputs need no torch RNG: positions of the movegen / features goldens with their legal
counts overwritten, weights from numpy.random.RandomState.  The cases are the smallest at
which the moved loads can go wrong:

* n33: 33 rows (a full wave and a one-row wave whose staging clamps to row n - 1), H = 128,
  500 actions, the action head as drawn (the tile skip holds on both waves: at tile 1 of
  wave 0, at tile 0 of wave 1) and scaled by 2^6 (the logit bound fails the skip ballot: the
  wave reloads the weight and bias fragments of tile o_s).  `test_skip_inputs` checks from
  fp64 logits that the two weight sets are on the side of the ballot they are meant for.
* a31 / a32 / a33 / a511 at H = 33 (T = 2) and 128: the value tile inside the only action
  tile, alone in tile 1, right after the first tile, and the last column of 16 tiles
  (`o_s < vt` false, or the prefetched tile `nx == vt`), with count-0 and heavy rows for the
  extra workgroups.
* win3 / win65: a 256-row window with 3 count-0 rows, one row of 65 and one of 500 legal
  actions among rows of 1..64, then the same window with 65 count-0 rows (more than the
  extra workgroups take: they stay on their main waves, unskipped); 33 more rows follow in a
  second window.  win3 also at H = 32, 64, 96 (T = 1, 2, 3).
* graph: MODE 0 with the step in `step_ctr`, eager and in a replayed HIP graph, against the
  call with the same total step in `step`.
"""
import os

import numpy as np
import pytest

GOLDEN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_latency.npz")
MASK_LOG = -103.27892990343185
SKIP_MARGIN, GUMBEL_MAX, GUMBEL_MIN = 30.0, 17.0, -2.9     # k_policy_act; -log(-log(2^-24)) = -2.81
HEAVY = 64                                                  # kHeavyDefault
SEED, STEP = 11, 12


def _positions(golden, n):
    feat, mg = golden("features"), golden("movegen")
    idx = feat["obs_idx"][:n]
    return np.array(mg["boards"][idx], np.int8), np.asarray(feat["obs_player"][:n])


def _records(golden, counts):
    counts = np.asarray(counts, np.int64)
    boards, players = _positions(golden, len(counts))
    r = np.zeros((len(counts), 64), np.uint8)
    r[:, :52] = boards.view(np.uint8)
    r[:, 52] = players
    r[:, 60] = counts & 0xFF
    r[:, 61] = counts >> 8
    return r


def _weights(H, A, head_scale=1.0, seed=0):
    """fc1, action head, value head in torch's layout (fp32), uniform(+-1/sqrt(fan_in))
    weights and N(0, 0.5) biases; the action head (weight and bias) times head_scale."""
    rs = np.random.RandomState(1000 * seed + 7 * H + A)
    f = np.float32
    return {"fc1.weight": (rs.uniform(-1, 1, (H, 198)) / np.sqrt(198)).astype(f),
            "fc1.bias": (rs.randn(H) * 0.5).astype(f),
            "action_head.weight": (rs.uniform(-1, 1, (A, H)) / np.sqrt(H) * head_scale).astype(f),
            "action_head.bias": (rs.randn(A) * 0.5 * head_scale).astype(f),
            "value_head.weight": (rs.uniform(-1, 1, (1, H)) / np.sqrt(H)).astype(f),
            "value_head.bias": (rs.randn(1) * 0.5).astype(f)}


def _window_counts(n_zero):
    rs = np.random.RandomState(40 + n_zero)
    c = rs.randint(1, 65, 289)
    rows = rs.permutation(256)
    c[rows[:n_zero]] = 0
    c[rows[n_zero]] = 65
    c[rows[n_zero + 1]] = 500
    return c


def cases(golden):
    """name -> (H, A, head_scale, records uint8[n, 64], rows of the MODE -1 logits call)."""
    rs = np.random.RandomState(33)
    c33 = rs.randint(1, 33, 33)
    c33[[3, 17]] = [64, 33]                     # wave 0: two action tiles, then the skip
    c33[32] = 20                                # wave 1 (one row): the skip after tile 0
    out = {"n33": (128, 500, 1.0, _records(golden, c33), 33),
           "n33_x64": (128, 500, 64.0, _records(golden, c33), 33)}
    for A in (31, 32, 33, 511):
        pat = np.clip(np.array([0, 1, 31, 32, 33, 64, 65, A - 1, A]), 0, A)
        for H in (33, 128):
            out[f"a{A}_h{H}"] = (H, A, 1.0, _records(golden, pat[np.arange(70) % 9]), 33)
    out["win3"] = (128, 500, 1.0, _records(golden, _window_counts(3)), 0)
    out["win65"] = (128, 500, 1.0, _records(golden, _window_counts(65)), 0)
    for H in (32, 64, 96):
        out[f"win3_h{H}"] = (H, 500, 1.0, _records(golden, _window_counts(3)), 0)
    return out


def _net(H, A, head_scale):
    import torch
    from bgx.policy import PolicyNet
    net = PolicyNet(hidden_size=H, action_size=A)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _weights(H, A, head_scale).items()})
    net = net.cuda()
    net.pack()
    return net


def run_case(case):
    """The arrays a case is checked on, from the loaded library."""
    import torch
    H, A, scale, rec, lrows = case
    net = _net(H, A, scale)
    r = torch.from_numpy(rec).cuda()
    act, logp, val = net.act(r, seed=SEED, step=STEP)
    res = {"act": act.cpu().numpy(), "log_prob": logp.cpu().numpy(), "value": val.cpu().numpy()}
    if lrows:
        logits = net.act(r[:lrows].contiguous(), seed=SEED, step=STEP, want_logits=True)[3]
        res["logits"] = logits[:, :A + 1].cpu().numpy()
    return res


def expected(golden):
    """Every case's arrays under 'case.array' keys (the recorder saves these)."""
    return {f"{name}.{k}": v for name, case in cases(golden).items() for k, v in run_case(case).items()}


@pytest.fixture(scope="module")
def want():
    return dict(np.load(GOLDEN_NPZ))


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist())


CASE_NAMES = (["n33", "n33_x64"] + [f"a{A}_h{H}" for A in (31, 32, 33, 511) for H in (33, 128)]
              + ["win3", "win65", "win3_h32", "win3_h64", "win3_h96"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_outputs_keep_their_bits(golden, want, name):
    """act, log_prob, value of the sampling call (MODE 0) and, where the case has them, the
    logits and the value column of the logits call (MODE -1): bit for bit the arrays the
    parent commit's library gave."""
    got = run_case(cases(golden)[name])
    assert sorted(f"{name}.{k}" for k in got) == sorted(k for k in want if k.split(".")[0] == name)
    for k, v in got.items():
        _same_bits(v, want[f"{name}.{k}"], f"{name}.{k}")


def test_case_list_is_the_recorded_one(golden, want):
    assert sorted(cases(golden)) == sorted(CASE_NAMES) == sorted({k.split(".")[0] for k in want})


def test_skip_inputs(golden):
    """The n33 inputs are where the docstring says: with the head as drawn the skip ballot
    of both waves holds, by more than the kernel's margins, for every row; with the head
    x 2^6 at least one row of each wave fails the first condition (logit bound against the
    running max), so the wave takes the reload path.  From fp64 logits, with a slack of 1
    for the kernel's fp32 rounding of the bound."""
    from oracle import features
    for name, holds in (("n33", True), ("n33_x64", False)):
        H, A, scale, rec, _ = cases(golden)[name]
        w = {k: v.astype(np.float64) for k, v in _weights(H, A, scale).items()}
        x = np.stack([features(r[:52].view(np.int8), int(r[52])) for r in rec]).astype(np.float64)
        h = np.maximum(x @ w["fc1.weight"].T + w["fc1.bias"], 0.0)
        z = h @ w["action_head.weight"].T + w["action_head.bias"]
        counts = rec[:, 60].astype(np.int64) | (rec[:, 61].astype(np.int64) << 8)
        assert ((counts > 0) & (counts <= HEAVY)).all()          # no row leaves its main wave
        u0 = w["action_head.bias"].max() + np.linalg.norm(w["action_head.weight"], axis=1).max() * (1 + 1 / 1024) \
            * np.linalg.norm(h, axis=1)
        ub = u0 + 1e-3 * np.abs(u0) + 1e-3
        for rows in (np.arange(32), np.array([32])):
            o_s = max((int(counts[rows].max()) + 31) // 32, 1)
            assert o_s < A // 32
            for i in rows:
                legal = z[i, :counts[i]]
                masked = z[i, counts[i]:32 * o_s] + MASK_LOG
                m_row = max(legal.max(), masked.max() if len(masked) else -np.inf)
                b_low = legal.max() + GUMBEL_MIN                 # the best key is at least this
                if holds:
                    assert ub[i] + MASK_LOG + 1 < m_row - SKIP_MARGIN
                    assert ub[i] + MASK_LOG + GUMBEL_MAX + 1 < b_low
            if not holds:
                m_rows = np.array([max(z[i, :counts[i]].max(), (z[i, counts[i]:32 * o_s] + MASK_LOG).max()
                                       if counts[i] < 32 * o_s else -np.inf) for i in rows])
                assert (ub[rows] + MASK_LOG - 1 > m_rows - SKIP_MARGIN).any()


@pytest.mark.gpu
def test_step_counter_and_graph_replay(golden, want):
    """MODE 0 with the noise's step split between `step` and a device counter, eager and in
    a replayed HIP graph: the outputs of the call with the total in `step` (the recorded
    n33 arrays at the counter's first value)."""
    import torch
    H, A, scale, rec, _ = cases(golden)["n33"]
    net = _net(H, A, scale)
    r = torch.from_numpy(rec).cuda()
    n = r.shape[0]
    ref = [net.act(r, seed=SEED, step=STEP + i) for i in range(3)]
    for k, t in zip(("act", "log_prob", "value"), ref[0]):
        _same_bits(t.cpu().numpy(), want[f"n33.{k}"], f"n33.{k} (plain step)")
    ctr = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    got = net.act(r, seed=SEED, step=STEP - 7, step_ctr=ctr)
    for a, b in zip(got, ref[0]):
        assert torch.equal(a, b)
    out = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
           torch.empty(n, dtype=torch.float32, device="cuda"))
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        net.act(r, seed=SEED, step=STEP - 7, step_ctr=ctr, out=out)
        net.advance_counter(ctr, 1)
    torch.cuda.synchronize()
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref[i]):
            assert torch.equal(a, b), i
