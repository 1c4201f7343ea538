"""The layout of the PPO update's host code: bgx.train re-exports what moved to
bgx.returns and bgx.ppo_epoch, Chunk is the one chunk type (plain tuples still accepted),
ScaleHint.advance is GradScaler's finite-step rule.  CPU only."""
import numpy as np
import torch

RETURNS_NAMES = ("lane_returns", "_lane_returns_torch", "reference_returns", "RETURNS_MODES", "check_returns_mode",
                 "_gae_scalars", "selfplay_gae", "_selfplay_gae_torch", "EPISODE_STATS", "episode_stats",
                 "episode_stats_records")
EPOCH_NAMES = ("features_and_masks", "_PPOHead", "ppo_epoch", "ppo_row_plan", "ppo_row_plan_torch", "gather_rollout",
               "plan_rollout", "adam_step", "REF_ROWS", "FEAT_W", "FEAT_BIAS_COL", "PPO_COLSUM_BLOCKS", "RELU_BLOCKS",
               "PPO_GW2_TASK_TILES", "MASK_SHORTCUT_LIMIT")


def test_train_reexports_the_moved_names():
    import bgx.ppo_epoch
    import bgx.returns
    import bgx.train
    for owner, names in ((bgx.returns, RETURNS_NAMES), (bgx.ppo_epoch, EPOCH_NAMES)):
        for n in names:
            assert getattr(bgx.train, n) is getattr(owner, n), n
    for n in ("PPOTrainer", "entropy_coef_after_update", "main"):
        assert getattr(bgx.train, n).__module__ == "bgx.train", n


def test_chunk_from_tuples_and_same_gradients():
    from bgx.policy import PolicyNet
    from bgx.ppo_epoch import Chunk, ppo_epoch
    g = torch.Generator().manual_seed(3)
    n = 256
    legal = torch.rand(n, 500, generator=g) < 0.1
    legal[:, 0] = True
    six = (torch.rand(n, 198, generator=g), legal, torch.randint(0, 1, (n,), generator=g),
           torch.log(torch.rand(n, generator=g) * 0.5 + 0.25), torch.randn(n, generator=g),
           torch.randn(n, generator=g))
    recs = torch.zeros(n, 64, dtype=torch.uint8)
    c6, c7 = Chunk(*six), Chunk(*six, recs)
    assert c6.records is None and c6.plan is None
    assert c7.records is recs and c7.plan is None
    assert all(a is b for a, b in zip(c6[:6], six))
    grads = []
    for as_chunks in (False, True):
        torch.manual_seed(5)
        net = PolicyNet()
        opt = torch.optim.SGD(net.parameters(), lr=1.0)
        halves = [tuple(x[i:i + 128] for x in six) + (recs[i:i + 128],) for i in (0, 128)]
        data = [Chunk(*h) for h in halves] if as_chunks else halves
        ppo_epoch(net, opt, torch.amp.GradScaler(device="cpu"), data, n, 0.15, amp=False, step=False)
        grads.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert any(bool(a.abs().max() > 0) for a in grads[0])


def test_scale_hint_advance_is_the_finite_step_rule():
    from bgx.ppo_epoch import ScaleHint
    sc = torch.amp.GradScaler(device="cpu", growth_interval=3)
    h = ScaleHint(65536.0, 0)
    seen = []
    for _ in range(3):
        h.advance(sc)
        seen.append((h.scale, h.tracker))
    assert seen == [(65536.0, 1), (65536.0, 2), (131072.0, 0)]
    # the grown scale is the fp32 product, as the device computes it
    sc = torch.amp.GradScaler(device="cpu", growth_interval=1, growth_factor=1.5)
    h = ScaleHint(float(np.float32(0.1)), 0)
    h.advance(sc)
    want = float(np.float32(np.float32(0.1) * np.float32(1.5)))
    assert (h.scale, h.tracker) == (want, 0) and h.scale != float(np.float32(0.1)) * 1.5
    # value equality, and a copy that does not alias
    a = ScaleHint(65536.0, 2)
    b = a.copy()
    assert a == b and b is not a and a != ScaleHint(65536.0, 1) and a != ScaleHint(32768.0, 2) and a != None  # noqa: E711
    b.advance(torch.amp.GradScaler(device="cpu", growth_interval=2000))
    assert (a.scale, a.tracker) == (65536.0, 2) and (b.scale, b.tracker) == (65536.0, 3) and a != b
