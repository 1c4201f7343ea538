"""The 2-ply search's 1-ply move filter (DESIGN.md §5 "Move filter"): its rule in plain
torch, bgx.search.move_filter_reference -- the specification of the k_filter kernel behind
bgx_two_ply_topk and the yardstick of tests/test_gpu_two_ply_filter.py -- on hand-built
rows, and the arena's command-line options for it.  No GPU.

    rank(a) = #{b : V1(b) > V1(a)} + #{b < a : V1(b) == V1(a)}
    keep(a) = rank(a) < top_k and (rank(a) == 0 or V1(a) >= fp32(V1best - margin))
"""
import math

import numpy as np
import pytest
import torch

INF = float("inf")
M = 12            # max_moves of the hand-built rows


def _keep(values, top_k, margin, n=None):
    """Kept move indices of one lane with the given 1-ply values (n = len(values) unless
    given); entries a >= n hold a value larger than every legal one: they must not count."""
    from bgx.search import move_filter_reference
    v = torch.full((1, M), 9.0)
    v[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    n = len(values) if n is None else n
    mask = move_filter_reference(v, torch.tensor([n]), top_k, margin)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, M)
    assert not mask[0, n:].any()
    return mask[0].nonzero().flatten().tolist()


def test_rank_order_and_top_k():
    v = [0.1, 0.7, -0.3, 0.5, 0.6]
    assert _keep(v, 1, INF) == [1]
    assert _keep(v, 2, INF) == [1, 4]
    assert _keep(v, 3, INF) == [1, 3, 4]
    assert _keep(v, 5, INF) == [0, 1, 2, 3, 4]
    assert _keep(v, 500, INF) == [0, 1, 2, 3, 4]        # top_k >= n: every legal move


def test_ties_at_the_cut_keep_the_lower_index():
    v = [0.5, 0.2, 0.5, 0.9, 0.5, 0.2]
    assert _keep(v, 1, INF) == [3]
    assert _keep(v, 2, INF) == [0, 3]                    # three tied for second: index 0
    assert _keep(v, 3, INF) == [0, 2, 3]
    assert _keep(v, 4, INF) == [0, 2, 3, 4]
    assert _keep(v, 5, INF) == [0, 1, 2, 3, 4]           # the tied 0.2s: index 1 before 5


def test_top_k_one_is_the_first_argmax():
    assert _keep([0.3, 0.8, 0.8, 0.1], 1, INF) == [1]
    assert _keep([0.3, 0.8, 0.8, 0.1], 1, 0.0) == [1]
    assert _keep([-2.0, -1.0, -3.0], 1, INF) == [1]


def test_margin_zero_keeps_the_tied_best():
    v = [0.4, 0.8, 0.8, 0.1, 0.8, 0.79999995]
    assert _keep(v, 500, 0.0) == [1, 2, 4]
    assert _keep(v, 2, 0.0) == [1, 2]                    # top_k of them at most
    assert _keep([0.0, -0.0, 0.0], 500, 0.0) == [0, 2]   # the bit order: -0 sorts below +0


def test_margin_cuts_below_top_k():
    v = [0.50, 0.10, 0.45, 0.30, 0.41, 0.39]
    assert _keep(v, 4, INF) == [0, 2, 4, 5]
    assert _keep(v, 4, 0.1) == [0, 2, 4]                 # 0.39 < 0.5 - 0.1
    assert _keep(v, 4, 0.06) == [0, 2]
    assert _keep(v, 4, 1.0) == [0, 2, 4, 5]              # a wide margin: rank alone


def test_threshold_is_fp32_arithmetic():
    """V1best - margin is rounded to fp32 before the comparison: a value equal to the
    rounded difference is kept, the next fp32 below it is not."""
    best, margin = np.float32(0.7), np.float32(0.3)
    thr = np.float32(best - margin)
    below = np.nextafter(thr, np.float32(-1.0))
    assert thr != np.float32(0.4)                        # not the decimal difference
    assert _keep([float(best), float(thr), float(below)], 3, float(margin)) == [0, 1]


def test_no_moves_and_one_move():
    assert _keep([], 3, INF) == []
    assert _keep([], 1, 0.0) == []
    assert _keep([0.2], 1, INF) == [0]
    assert _keep([0.2], 3, 0.0) == [0]
    assert _keep([0.2, 0.9, 0.9], 3, INF, n=1) == [0]    # a >= n never counts, never kept
    assert _keep([-INF], 2, 0.5) == [0]                  # the best move is kept whatever its value


def test_lanes_are_independent():
    from bgx.search import move_filter_reference
    v = torch.tensor([[0.1, 0.9, 0.5, 0.7], [0.3, 0.3, 0.3, 0.3], [5.0, 6.0, 7.0, 8.0], [1.0, 0.0, 2.0, 0.0]])
    n = torch.tensor([4, 3, 0, 2])
    got = move_filter_reference(v, n, 2, INF)
    want = torch.tensor([[0, 1, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]], dtype=torch.bool)
    assert torch.equal(got, want)
    got = move_filter_reference(v, n, 3, 0.25)
    want = torch.tensor([[0, 1, 0, 1], [1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.bool)
    assert torch.equal(got, want)


def test_matches_the_rule_by_counting():
    """The sort-based reference against the rule as written (ranks by counting), random rows
    with many ties."""
    from bgx.search import move_filter_reference
    rng = np.random.RandomState(3)
    B, MM = 40, 70
    v = (rng.randint(-6, 7, size=(B, MM)) / np.float32(8.0)).astype(np.float32)
    n = rng.randint(0, MM + 1, size=B)
    n[:3] = (0, 1, MM)
    for top_k, margin in ((1, INF), (4, INF), (8, 0.25), (70, 0.0), (3, 0.125)):
        got = move_filter_reference(torch.from_numpy(v), torch.from_numpy(n), top_k, margin).numpy()
        for i in range(B):
            x = v[i, :n[i]]
            want = np.zeros(MM, bool)
            for a in range(n[i]):
                rank = int((x > x[a]).sum() + (x[:a] == x[a]).sum())
                want[a] = rank < top_k and (rank == 0 or x[a] >= np.float32(x.max() - np.float32(margin)))
            assert np.array_equal(got[i], want), (top_k, margin, i)


def test_rejects_bad_options():
    from bgx.search import move_filter_reference
    v, n = torch.zeros(1, 4), torch.tensor([4])
    for top_k, margin in ((0, INF), (-1, 0.0), (2, -0.5), (2, math.nan)):
        with pytest.raises(ValueError):
            move_filter_reference(v, n, top_k, margin)


def test_arena_parser_move_filter_flags():
    from bgx.arena import build_parser
    ap = build_parser()
    base = ["--a", "x.pt", "--b", "y.pt", "--max-steps", "900"]
    a = ap.parse_args(base)
    assert (a.top_k_a, a.top_k_b, a.margin_a, a.margin_b) == (None, None, None, None)
    a = ap.parse_args(base + ["--player-a", "2ply", "--top-k-a", "4"])
    assert (a.top_k_a, a.margin_a, a.top_k_b, a.margin_b) == (4, None, None, None)
    a = ap.parse_args(base + ["--player-a", "2ply", "--player-b", "2ply", "--top-k-a", "4", "--margin-a", "0.05",
                              "--top-k-b", "8", "--margin-b", "0"])
    assert (a.top_k_a, a.margin_a, a.top_k_b, a.margin_b) == (4, 0.05, 8, 0.0)
    for bad in (["--top-k-a", "4"],                                           # A is a policy player
                ["--player-a", "1ply", "--top-k-a", "4"],
                ["--player-a", "2ply", "--margin-b", "0.1"],                  # B is a policy player
                ["--player-b", "greedy", "--top-k-b", "2"],
                ["--player-a", "2ply", "--top-k-a", "0"],
                ["--player-a", "2ply", "--margin-a", "-1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)
    with pytest.raises(SystemExit):                                           # the random player has no search
        ap.parse_args(["--a", "random", "--b", "y.pt", "--max-steps", "9", "--player-a", "2ply", "--top-k-a", "2"])


def test_make_player_move_filter_options():
    from bgx.arena import make_player
    for kind, net in (("1ply", object()), ("policy", object()), ("2ply", None), ("2ply", "random")):
        with pytest.raises(ValueError):
            make_player(kind, net, top_k=4)
        with pytest.raises(ValueError):
            make_player(kind, net, margin=0.1)
