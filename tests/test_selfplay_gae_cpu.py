"""Zero-sum GAE(lambda) of a self-play rollout (bgx.train._selfplay_gae_torch, the CPU
path and the kernel's reference; DESIGN.md §6 "Self-play returns"): identities that pin
the sign convention, the cuts and the bootstrap, on random data with random movers."""
import numpy as np
import pytest
import torch

T, B, GAMMA, P_DONE = 33, 1000, 0.99, 0.1
G = float(np.float32(GAMMA))


def records_of(movers):
    rec = torch.zeros(*movers.shape, 64, dtype=torch.uint8)
    rec[..., 52] = movers
    return rec


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    r = torch.randn(T, B, generator=g)
    d = (torch.rand(T, B, generator=g) < P_DONE).to(torch.uint8)
    m = (torch.rand(T, B, generator=g) < 0.5).to(torch.uint8)
    v = torch.randn(T, B, generator=g)
    bv = torch.randn(B, generator=g)
    bm = (torch.rand(B, generator=g) < 0.5).to(torch.uint8)
    return r, d, m, v, bv, bm


def test_reduces_to_lane_returns(data):
    """values = 0, one mover, lambda = 1, no bootstrap: the plain discounted return of
    the lane, bit for bit in fp32."""
    from bgx.train import _lane_returns_torch, _selfplay_gae_torch
    r, d = data[0], data[1]
    for mover in (0, 1):
        rec = records_of(torch.full((T, B), mover, dtype=torch.uint8))
        adv, ret = _selfplay_gae_torch(r, d, rec, torch.zeros(T, B), gamma=GAMMA, lam=1.0, normalize=False)
        want = _lane_returns_torch(r, d, GAMMA)
        assert torch.equal(ret, want) and torch.equal(adv, want)


@pytest.mark.parametrize("boot", [True, False])
def test_signed_outcome_lambda_one(data, boot):
    """lambda = 1 in fp64: Ret_t = sum_k s_k g^k r_{t+k} up to the first done, plus
    s g^n v_T when no done intervenes, s_k = the product of the mover-change signs since
    t -- whatever the stored values are.  Each row evaluated directly."""
    from bgx.train import _selfplay_gae_torch
    r, d, m, v, bv, bm = data
    r64, v64, bv64 = r.double(), v.double(), bv.double()
    _, ret = _selfplay_gae_torch(r64, d, records_of(m), v64, bv64 if boot else None,
                                 records_of(bm) if boot else None, gamma=GAMMA, lam=1.0, normalize=False)
    rn, dn, mn, bvn, bmn = r64.numpy(), d.numpy(), m.numpy(), bv64.numpy(), bm.numpy()
    want = np.zeros((T, B))
    for b in range(0, B, 7):                           # every 7th lane: 143 lanes x 33 rows
        for t in range(T):
            acc, s, k = 0.0, 1.0, t
            while True:
                acc += s * G ** (k - t) * rn[k, b]
                if dn[k, b]:
                    break
                if k == T - 1:
                    if boot:
                        s = s if bmn[b] == mn[k, b] else -s
                        acc += s * G ** (T - t) * bvn[b]
                    break
                s = s if mn[k + 1, b] == mn[k, b] else -s
                k += 1
            want[t, b] = acc
    err = np.abs(ret.numpy()[:, ::7] - want[:, ::7]).max()
    print("lambda=1 max |err|", err)
    assert err < 1e-12


def test_seat_symmetry(data):
    """Swapping the two seats everywhere (the bootstrap's mover included) changes nothing."""
    from bgx.train import _selfplay_gae_torch
    r, d, m, v, bv, bm = data
    a = _selfplay_gae_torch(r, d, records_of(m), v, bv, records_of(bm), gamma=GAMMA, lam=0.95)
    b = _selfplay_gae_torch(r, d, records_of(1 - m), v, bv, records_of(1 - bm), gamma=GAMMA, lam=0.95)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_lambda_zero_is_one_step(data):
    """lambda = 0: Ret_t = r_t + g nv exactly (the one-step target)."""
    from bgx.train import _selfplay_gae_torch
    r, d, m, v, bv, bm = (x.double() if x.dtype == torch.float32 else x for x in data)
    adv, ret = _selfplay_gae_torch(r, d, records_of(m), v, bv, records_of(bm), gamma=GAMMA, lam=0.0,
                                   normalize=False)
    vn = torch.cat([v[1:], bv[None]])
    mn = torch.cat([m[1:], bm[None]])
    nv = torch.where(d.bool(), torch.zeros_like(vn), torch.where(mn == m, vn, -vn))
    delta = (r + G * nv) - v
    assert torch.equal(adv, delta)
    assert torch.equal(ret, delta + v)
    assert float((ret - (r + G * nv)).abs().max()) < 1e-14


def test_hand_worked_lane():
    """Four steps of one lane.  t = 0: player 0 moves, no reward.  t = 1: player 1 wins a
    gammon (r = 1.5, done).  t = 2, 3: a new game, player 0 then player 1; the rollout stops
    with player 0 to move in a position worth 0.5 to it.  g = 0.5, lambda = 0.5 (exact)."""
    from bgx.train import _selfplay_gae_torch
    r = torch.tensor([[0.0], [1.5], [0.0], [0.0]], dtype=torch.float64)
    d = torch.tensor([[0], [1], [0], [0]], dtype=torch.uint8)
    m = torch.tensor([[0], [1], [0], [1]], dtype=torch.uint8)
    v = torch.tensor([[0.25], [0.5], [0.125], [-0.25]], dtype=torch.float64)
    bv, bm = torch.tensor([0.5], dtype=torch.float64), torch.tensor([0], dtype=torch.uint8)
    adv, ret = _selfplay_gae_torch(r, d, records_of(m), v, bv, records_of(bm), gamma=0.5, lam=0.5, normalize=False)
    # t = 3: mover 1, next mover 0: nv = -0.5;  delta = 0 + 0.5 * -0.5 + 0.25 = 0;      A = 0
    # t = 2: mover 0, next mover 1: nv = +0.25; delta = 0.125 - 0.125 = 0;  na = -0;    A = 0
    # t = 1: done: nv = na = 0;                 delta = 1.5 - 0.5 = 1;                  A = 1
    # t = 0: mover 0, next mover 1: nv = -0.5;  delta = -0.25 - 0.25 = -0.5; na = -1;   A = -0.5 - 0.25 = -0.75
    assert adv.squeeze(1).tolist() == [-0.75, 1.0, 0.0, 0.0]
    assert ret.squeeze(1).tolist() == [-0.5, 1.5, 0.125, -0.25]
    # without the bootstrap the horizon is a cut: t = 3: delta = 0 - -0.25 = 0.25 = A;
    # t = 2: nv = +0.25, delta = 0, na = -0.25, A = 0.25 * -0.25 = -0.0625
    adv, ret = _selfplay_gae_torch(r, d, records_of(m), v, gamma=0.5, lam=0.5, normalize=False)
    assert adv.squeeze(1).tolist() == [-0.75, 1.0, -0.0625, 0.25]
    assert ret.squeeze(1).tolist() == [-0.5, 1.5, 0.0625, 0.0]
    # the loser's last move before the win gets a negative target: the zero-sum point
    assert float(ret[0]) < 0 < float(ret[1])


def test_normalize_is_global_normalize(data):
    from bgx.ppo import global_normalize
    from bgx.train import _selfplay_gae_torch
    r, d, m, v, bv, bm = data
    a, ret = _selfplay_gae_torch(r, d, records_of(m), v, bv, records_of(bm), normalize=False)
    an, ret2 = _selfplay_gae_torch(r, d, records_of(m), v, bv, records_of(bm))
    assert torch.equal(an, global_normalize(a.reshape(-1)).view_as(a)) and torch.equal(ret, ret2)


def test_boot_pointers_go_together(data):
    from bgx.train import _selfplay_gae_torch, selfplay_gae
    r, d, m, v, bv, bm = data
    for fn in (_selfplay_gae_torch, selfplay_gae):
        with pytest.raises(ValueError):
            fn(r, d, records_of(m), v, boot_values=bv)
        with pytest.raises(ValueError):
            fn(r, d, records_of(m), v, boot_records=records_of(bm))


def test_unknown_returns_mode_is_rejected():
    """Any string but the three modes raises (it used to mean "lane" silently); the check
    runs before the constructor touches a device."""
    from bgx.train import PPOTrainer, RETURNS_MODES, check_returns_mode
    assert RETURNS_MODES == ("lane", "reference", "selfplay")
    for ok in RETURNS_MODES:
        assert check_returns_mode(ok) == ok
    for bad in ("bogus", "", "Lane", "gae"):
        with pytest.raises(ValueError):
            check_returns_mode(bad)
    with pytest.raises(ValueError, match="returns"):
        PPOTrainer(batch=64, horizon=2, device="cpu", returns="bogus")
