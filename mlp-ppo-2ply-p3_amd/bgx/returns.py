"""What is computed from a finished [T, B] rollout: the discounted returns (per lane, or the
reference's flat step-major quirk), the zero-sum GAE(lambda) of self-play (the modes:
bgx/train.py's docstring) and the episode statistics."""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import check
from .engine import _ptr, _stream
from .ppo import GAMMA, global_normalize, _world


def lane_returns(rewards: torch.Tensor, dones: torch.Tensor, gamma: float = GAMMA) -> torch.Tensor:
    """R_t = r_t + gamma * R_{t+1}, reset at done, per lane; [T, B].  On the GPU one HIP
    kernel (bgx_lane_returns, the same fp32 roundings as the torch loop below, which
    stays as the CPU path and the tests' reference)."""
    if rewards.is_cuda and rewards.dtype == torch.float32 and dones.dtype == torch.uint8:
        r, d = rewards.contiguous(), dones.contiguous()
        out = torch.empty_like(r)
        T, B = r.shape[0], r[0].numel()
        check(_lib.load().bgx_lane_returns(_ptr(r), _ptr(d), T, B, float(gamma), _ptr(out), _stream(r.device)),
              "bgx_lane_returns")
        return out
    return _lane_returns_torch(rewards, dones, gamma)


def _lane_returns_torch(rewards: torch.Tensor, dones: torch.Tensor, gamma: float = GAMMA) -> torch.Tensor:
    T = rewards.shape[0]
    out = torch.empty_like(rewards)
    R = torch.zeros_like(rewards[0])
    for t in range(T - 1, -1, -1):
        R = torch.where(dones[t].bool(), torch.zeros_like(R), R)
        R = rewards[t] + gamma * R
        out[t] = R
    return out


def reference_returns(rewards: torch.Tensor, dones: torch.Tensor, gamma: float = GAMMA) -> torch.Tensor:
    """ppo_agent.py:206-216 over the flat step-major memory (envs interleaved)."""
    flat_r = rewards.reshape(-1).double().cpu().numpy()
    flat_d = dones.reshape(-1).cpu().numpy()
    out = [0.0] * len(flat_r)
    R = 0.0
    for k in range(len(flat_r) - 1, -1, -1):
        if flat_d[k]:
            R = 0.0
        R = flat_r[k] + gamma * R
        out[k] = R
    return torch.tensor(out, dtype=torch.float32, device=rewards.device).view_as(rewards)


RETURNS_MODES = ("lane", "reference", "selfplay")


def check_returns_mode(returns: str) -> str:
    if returns not in RETURNS_MODES:
        raise ValueError(f"returns must be one of {RETURNS_MODES}, got {returns!r}")
    return returns


def _gae_scalars(gamma: float, lam: float):
    """g = fp32(gamma), gl = fp32(fp32(gamma) * fp32(lam)) as Python floats."""
    g = np.float32(gamma)
    return float(g), float(np.float32(g * np.float32(lam)))


def selfplay_gae(rewards: torch.Tensor, dones: torch.Tensor, records: torch.Tensor, values: torch.Tensor,
                 boot_values: torch.Tensor | None = None, boot_records: torch.Tensor | None = None,
                 gamma: float = GAMMA, lam: float = 0.95, normalize: bool = True, group=None):
    """Zero-sum GAE(lambda) of a self-play rollout, per game lane (DESIGN.md §6 "Self-play
    returns"): both players move in one lane, `values[t]` is the value of the player on move
    at step t (record byte 52), so the next step's value and advantage change sign where the
    mover changes and are dropped at a done.  boot_values [B] / boot_records [B, 64]: value
    and record of the position the rollout stopped in (both or neither; without them the
    horizon is a cut).  Returns (adv, ret) [T, B]: ret = A + v un-normalised, adv = A
    normalised as global_normalize does over all ranks' rows (normalize=False: A itself).
    On the GPU two HIP calls and no host sync (bgx_selfplay_gae, bgx_normalize_adv; with a
    process group the three sums are all-reduced between them); _selfplay_gae_torch
    elsewhere."""
    if (boot_values is None) != (boot_records is None):
        raise ValueError("selfplay_gae: boot_values and boot_records go together")
    if not (rewards.is_cuda and rewards.dtype == torch.float32 and values.dtype == torch.float32
            and dones.dtype == torch.uint8 and records.dtype == torch.uint8):
        return _selfplay_gae_torch(rewards, dones, records, values, boot_values, boot_records, gamma, lam,
                                   normalize, group)
    T, B = rewards.shape[0], rewards[0].numel()
    if records.numel() != T * B * 64 or values.numel() != T * B or dones.numel() != T * B:
        raise ValueError("selfplay_gae: rewards, dones, values [T, B] and records [T, B, 64] do not agree")
    r, d, rec, v = rewards.contiguous(), dones.contiguous(), records.contiguous(), values.contiguous()
    bv = br = None
    if boot_values is not None:
        bv, br = boot_values.contiguous(), boot_records.contiguous()
        if bv.dtype != torch.float32 or br.dtype != torch.uint8 or bv.numel() != B or br.numel() != B * 64:
            raise ValueError("selfplay_gae: boot_values must be float32 [B], boot_records uint8 [B, 64]")
    g, gl = _gae_scalars(gamma, lam)
    L = _lib.load()
    dev = r.device
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    sums = ws = None
    if normalize:
        sums = torch.empty(3, dtype=torch.float64, device=dev)
        ws = torch.empty(max(int(L.bgx_selfplay_gae_workspace(B)) // 8, 1), dtype=torch.float64, device=dev)
    stream = _stream(dev)
    check(L.bgx_selfplay_gae(_ptr(r), _ptr(d), _ptr(rec), _ptr(v), _ptr(bv), _ptr(br), T, B, g, gl, _ptr(adv),
                             _ptr(ret), _ptr(ws), _ptr(sums), stream), "bgx_selfplay_gae")
    if normalize:
        if _world(group) > 1:
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        check(L.bgx_normalize_adv(_ptr(adv), adv.numel(), _ptr(sums), 1e-5, stream), "bgx_normalize_adv")
    return adv, ret


def _selfplay_gae_torch(rewards: torch.Tensor, dones: torch.Tensor, records: torch.Tensor, values: torch.Tensor,
                        boot_values: torch.Tensor | None = None, boot_records: torch.Tensor | None = None,
                        gamma: float = GAMMA, lam: float = 0.95, normalize: bool = True, group=None):
    """selfplay_gae as a torch loop over the T steps, in the dtype of `rewards` (fp32: the
    kernel's roundings; fp64: the tests' reference).  gamma and gamma * lambda are the
    fp32-rounded scalars in either dtype."""
    if (boot_values is None) != (boot_records is None):
        raise ValueError("selfplay_gae: boot_values and boot_records go together")
    T = rewards.shape[0]
    g, gl = _gae_scalars(gamma, lam)
    values = values.to(rewards.dtype)
    movers = records[..., 52]
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    zero = torch.zeros_like(rewards[0])
    A1 = zero
    if boot_values is not None:
        v1, m1 = boot_values.to(rewards.dtype).reshape(zero.shape), boot_records[..., 52].reshape(zero.shape)
        cut_next = torch.zeros_like(dones[0], dtype=torch.bool)
    else:
        v1, m1 = zero, movers[T - 1]
        cut_next = torch.ones_like(dones[0], dtype=torch.bool)
    for t in range(T - 1, -1, -1):
        cut = dones[t].bool() | cut_next
        same = movers[t] == m1
        nv = torch.where(cut, zero, torch.where(same, v1, -v1))
        na = torch.where(cut, zero, torch.where(same, A1, -A1))
        delta = (rewards[t] + g * nv) - values[t]
        A1 = delta + gl * na
        adv[t] = A1
        ret[t] = A1 + values[t]
        v1, m1 = values[t], movers[t]
        cut_next = torch.zeros_like(cut)
    if normalize:
        adv = global_normalize(adv.reshape(-1), group).view_as(adv)
    return adv, ret


EPISODE_STATS = ("episodes", "episode_reward_sum", "wins", "p1_wins", "gammons", "backgammons")


def episode_stats_records(rewards: torch.Tensor, dones: torch.Tensor, records: torch.Tensor,
                          carry: torch.Tensor) -> torch.Tensor:
    """episode_stats with the movers read from the [T, B, 64] rollout records (byte 52).
    On the GPU one HIP kernel walks each lane's T steps (bgx_episode_stats: the same sums,
    exact in fp64 in any order) instead of ~25 torch launches over [T, B]."""
    if (rewards.is_cuda and rewards.dtype == torch.float32 and dones.dtype == torch.uint8
            and records.dtype == torch.uint8 and carry.dtype == torch.float64 and carry.is_contiguous()
            and rewards.is_contiguous() and dones.is_contiguous() and records.is_contiguous()):
        T, B = rewards.shape
        L = _lib.load()
        ws = torch.empty(max(int(L.bgx_episode_stats_workspace(B)) // 8, 1), dtype=torch.float64, device=rewards.device)
        out = torch.empty(len(EPISODE_STATS), dtype=torch.float64, device=rewards.device)
        check(L.bgx_episode_stats(_ptr(rewards), _ptr(dones), _ptr(records), _ptr(carry), T, B, _ptr(ws), _ptr(out),
                                  _stream(rewards.device)), "bgx_episode_stats")
        return out
    return episode_stats(rewards, dones, records[:, :, 52], carry)


def episode_stats(rewards: torch.Tensor, dones: torch.Tensor, movers: torch.Tensor,
                  carry: torch.Tensor) -> torch.Tensor:
    """The reference loop's per-env episode accounting (train.py:55-99) over a
    [T, B] rollout, on the device without a per-step loop.

    `carry` [B] (fp64) is each lane's reward accumulated in its unfinished
    episode (`episode_rewards`, train.py:58) and is updated in place.  Returns
    the sums named by EPISODE_STATS as one fp64 tensor: finished episodes,
    their summed episode rewards (train.py:73), wins as the reference counts
    them (`info["winner"] == info["current_player"]`, train.py:74-77: the
    mover of a winning step, i.e. a done with a positive reward), wins by
    PLAYER1 (`log_metrics`' "1 if Player1 wins", ppo_agent.py:494), and
    gammon / backgammon wins (rewards 1.5 / 2.0, backgammon_env.py:26-28).
    `movers` [T, B] is the player to move before each step (record byte 52).
    """
    T, B = rewards.shape
    d = dones.bool()
    r = rewards.double()
    seg = torch.cumsum(d, 0, dtype=torch.int64) - d.long()      # episodes finished before step t
    idx = seg + torch.arange(B, device=r.device, dtype=torch.int64) * (T + 1)
    sums = torch.zeros(B * (T + 1), dtype=torch.float64, device=r.device)
    sums.scatter_add_(0, idx.reshape(-1), r.reshape(-1))
    sums = sums.view(B, T + 1)
    sums[:, 0] += carry
    n = d.sum(0, dtype=torch.int64)
    open_ep = sums.gather(1, n[:, None]).squeeze(1)
    finished = sums.sum(1) - open_ep
    carry.copy_(open_ep)
    return torch.stack([n.sum().double(), finished.sum(),
                        (d & (r > 0)).sum().double(), (d & (r > 0) & (movers == 0)).sum().double(),
                        (d & (r == 1.5)).sum().double(), (d & (r == 2.0)).sum().double()])
