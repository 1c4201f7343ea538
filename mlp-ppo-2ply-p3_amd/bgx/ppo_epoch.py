"""One full-batch PPO epoch (ppo_agent.py:268-305) and what it needs: the chunk type, the
choice between its four implementations (epoch_path), the fused head's row plan and
gather, and the one-call Adam step.  PPOTrainer (bgx/train.py) runs NUM_EPOCHS per update."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, replace
from typing import Any, NamedTuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.amp import autocast
from torch.distributions import Categorical

from . import _lib
from ._lib import check
from .engine import encode_records, _ptr, _stream
from .policy import PolicyNet, MASK_LOG
from .ppo import EPS_CLIP, VALUE_LOSS_COEF, allreduce_mean_


class Chunk(NamedTuple):
    """Rows of one gradient-accumulation chunk.  `feats` / `legal` are None where the path
    does not read them (the loss kernels take the legal counts from `records`, the fused
    head its features too).  `plan` = (plan, row_plan) of ppo_row_plan for rows already in
    plan order; None: the fused epoch computes it and reads the rows through its permutation."""
    feats: Any
    legal: Any
    actions: Any
    old_logp: Any
    returns: Any
    adv: Any
    records: Any = None
    plan: Any = None


@dataclass
class ScaleHint:
    """The host's copy of the GradScaler state (PPOTrainer.update), used instead of
    get_scale() (a host sync per epoch that left the GPU idle while the next epoch's
    launches were issued) and advanced as a finite step advances the device state; the
    trainer redoes an update after which a skipped (non-finite) step made the two differ."""
    scale: float
    tracker: int

    def advance(self, scaler) -> None:
        """_amp_update_scale_ without a non-finite gradient."""
        self.tracker += 1
        if self.tracker == scaler._growth_interval:
            self.scale = float(np.float32(self.scale * scaler._growth_factor))
            self.tracker = 0

    def copy(self) -> "ScaleHint":
        return replace(self)


def features_and_masks(records: torch.Tensor, n_actions: int):
    feats = encode_records(records)
    counts = records[:, 60].to(torch.int32) | (records[:, 61].to(torch.int32) << 8)
    legal = torch.arange(n_actions, device=records.device)[None, :] < counts[:, None]
    return feats, legal


def _is_policy_mlp(net) -> bool:
    """The manual fp16 epoch needs exactly relu(fc1) -> {action_head, value_head}."""
    return (isinstance(net, PolicyNet) and type(net).forward is PolicyNet.forward
            and all(getattr(net, k).bias is not None for k in ("fc1", "action_head", "value_head"))
            and net.fc1.out_features % 8 == 0 and net.fc1.out_features <= 256)     # bgx_relu_backward


class EpochPath(NamedTuple):
    kind: str              # "torch" | "head" | "manual" | "fused"
    fast: bool = False     # "fused" only: the one-launch prologue and epilogue


def epoch_path(net, fused: bool | None, amp: bool, fused_head: bool = True) -> EpochPath:
    """Which implementation of the epoch runs: "torch", the autograd reference; "head",
    autograd forward with the loss head as one kernel (bgx_ppo_head); "manual",
    _ppo_epoch_amp_manual; "fused", _ppo_epoch_amp_fused.  fused None: on the GPU."""
    if fused is None:
        fused = next(net.parameters()).device.type == "cuda"
    if not fused:
        return EpochPath("torch")
    if not (amp and _is_policy_mlp(net)):
        return EpochPath("head")
    # the fused output layer + loss head (csrc/bg_ppo_fused.hip) is built for the reference's
    # shape (H = 128, 500 actions); other shapes take the manual epoch
    if not (fused_head and net.fc1.out_features == 128 and net.action_head.out_features == 500):
        return EpochPath("manual")
    # its one-launch prologue / epilogue (bgx_ppo_epoch_prep / _grads): 198 input features
    # and fp32 contiguous parameters
    return EpochPath("fused", net.fc1.in_features == 198 and all(t.dtype == torch.float32 and t.is_contiguous()
                                                                for t in _mlp_params(net)))


def _mlp_params(net):
    return (net.fc1.weight, net.fc1.bias, net.action_head.weight, net.action_head.bias, net.value_head.weight,
            net.value_head.bias)


class _PPOHead(torch.autograd.Function):
    """The loss head of ppo_epoch on the HIP kernel bgx_ppo_head: forward computes
    the per-row losses' sums AND the gradients w.r.t. logits and values (already
    multiplied by `gscale` = GradScaler scale / n_total); backward hands them out.
    Call .backward() on the (zero) output directly: the incoming gradient is
    taken to be 1."""

    @staticmethod
    def forward(ctx, logits, values, records, actions, old_logp, returns, adv, coefs, sums):
        eps, c_v, c_e, gscale = coefs
        if logits.dtype not in (torch.float16, torch.float32) or values.dtype != logits.dtype:
            raise TypeError(f"bgx_ppo_head: logits/values must be fp16 or fp32 alike, got {logits.dtype}/{values.dtype}")
        logits, values = logits.contiguous(), values.contiguous()
        n, A = logits.shape
        dlog = torch.empty_like(logits)
        dval = torch.empty_like(values)
        check(_lib.load().bgx_ppo_head(_ptr(logits), 0 if logits.dtype == torch.float32 else 1, A, _ptr(values),
                                       _ptr(records), _ptr(actions), _ptr(old_logp), _ptr(returns), _ptr(adv), n, A,
                                       eps, c_v, c_e, gscale, _ptr(dlog), A, _ptr(dval), _ptr(sums),
                                       _stream(logits.device)), "bgx_ppo_head")
        ctx.save_for_backward(dlog, dval)
        return logits.new_zeros((), dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        dlog, dval = ctx.saved_tensors
        return dlog, dval, None, None, None, None, None, None, None


def ppo_epoch(net: nn.Module, optimizer, scaler, chunks, n_total: int, entropy_coef: float, group=None,
              amp: bool = True, fused: bool | None = None, step: bool = True, sync: bool = True, guard=None,
              fused_head: bool = True, scale_hint: ScaleHint | None = None, parts=None):
    """One full-batch PPO epoch (ppo_agent.py:268-305) over `chunks` = an iterable of Chunk,
    or of plain (features, legal_mask, actions, old_logp, returns, advantages [, records])
    tuples, with gradient accumulation and one all-reduce.  Returns loss parts (sync=False
    with `parts` given: added on the device to that fp64 [4] tensor, which is returned).
    fused (default: on the GPU): one of the HIP paths of epoch_path instead of the torch
    formulation (_ppo_epoch_torch), which stays as their reference (tests compare them).
    scale_hint: used instead of get_scale(), advanced with the step.  guard: _ppo_epoch_amp_fused."""
    optimizer.zero_grad(set_to_none=True)
    path = epoch_path(net, fused, amp, fused_head)
    chunks = (c if isinstance(c, Chunk) else Chunk(*c) for c in chunks)
    if path.kind == "torch":
        acc = _ppo_epoch_torch(net, scaler, chunks, n_total, entropy_coef, amp)
        if step:
            allreduce_mean_([p.grad for p in net.parameters() if p.grad is not None], group)
            scaler.step(optimizer)
            scaler.update()
        return acc
    dev = next(net.parameters()).device
    if scaler.is_enabled():
        if getattr(scaler, "_scale", None) is None:
            scaler.scale(torch.ones((), device=dev))      # initialises the scale tensor lazily
        scale = scale_hint.scale if scale_hint is not None else scaler.get_scale()
    else:
        scale = 1.0
    coefs = (EPS_CLIP, VALUE_LOSS_COEF, float(entropy_coef), float(scale) / n_total)
    # `parts` (fp64 [4] accumulator, sync=False only): the fast fused epoch adds its loss parts
    # on the device inside its own epilogue launch (and its prologue zeroes the sums)
    in_kernel = parts is not None and not sync and path.fast
    if in_kernel and (parts.device != dev or parts.dtype != torch.float64 or parts.numel() != 4):
        raise ValueError("parts must be a float64 [4] tensor on the parameters' device")
    sums = (torch.empty if in_kernel else torch.zeros)(3, dtype=torch.float64, device=dev)
    if path.kind == "fused":
        _ppo_epoch_amp_fused(net, chunks, n_total, coefs, sums, path.fast, guard, parts if in_kernel else None,
                             entropy_coef)
    elif path.kind == "manual":
        _ppo_epoch_amp_manual(net, chunks, n_total, coefs, sums)
    else:                                   # "head": autograd around the loss-head kernel
        for c in chunks:
            with autocast(device_type=dev.type, enabled=amp):
                logits, values = net(c.feats)
            out = _PPOHead.apply(logits, values, c.records.contiguous(), *_row_fields(c.actions, c.old_logp, c.returns,
                                                                                      c.adv), coefs, sums)
            out.backward()
    if step:
        allreduce_mean_([p.grad for p in net.parameters() if p.grad is not None], group)
        if not adam_step(optimizer, scaler):
            scaler.step(optimizer)
            scaler.update()
        if scale_hint is not None and scaler.is_enabled():
            scale_hint.advance(scaler)
    if in_kernel:
        return parts
    if not sync:        # loss parts stay on the device (fp64, same arithmetic): no host sync per epoch
        m = sums / n_total
        e = torch.cat([m, (m[0] + VALUE_LOSS_COEF * m[1] - entropy_coef * m[2]).reshape(1)])
        if parts is not None:
            parts += e
            return parts
        return e
    pol, val, ent = (sums / n_total).tolist()
    tot = pol + VALUE_LOSS_COEF * val - entropy_coef * ent
    return torch.tensor([pol, val, ent, tot], dtype=torch.float64)


def _ppo_epoch_torch(net, scaler, chunks, n_total, entropy_coef, amp):
    """The epoch's forward, loss and backward as the reference writes them, in torch."""
    acc = torch.zeros(4, dtype=torch.float64)
    dev_type = next(net.parameters()).device.type
    for c in chunks:
        w = c.feats.shape[0] / n_total
        with autocast(device_type=dev_type, enabled=amp):
            logits, values = net(c.feats)
            masked = torch.where(c.legal, logits.float(), logits.float() + MASK_LOG)
            # torch.distributions.Categorical(probs) as ppo_agent.py:273-291: log_prob and
            # entropy on log(clamp(probs, eps, 1 - eps))
            dist_ = Categorical(torch.softmax(masked, dim=-1))
            new_logp = dist_.log_prob(c.actions.long())
            ratios = torch.exp(new_logp - c.old_logp)
            surr1 = ratios * c.adv
            surr2 = torch.clamp(ratios, 1 - EPS_CLIP, 1 + EPS_CLIP) * c.adv
            policy_loss = -torch.min(surr1, surr2).mean()
            value_loss = nn.functional.mse_loss(values.float().squeeze(-1), c.returns)
            entropy = dist_.entropy().mean()
            loss = policy_loss + VALUE_LOSS_COEF * value_loss - entropy_coef * entropy
        scaler.scale(loss * w).backward()
        acc += torch.tensor([policy_loss.item(), value_loss.item(), entropy.item(), loss.item()],
                            dtype=torch.float64) * w
    return acc


PPO_COLSUM_BLOCKS = 2048       # include/bgx.h BGX_PPO_COLSUM_BLOCKS
RELU_BLOCKS = 1024             # bgx_relu_backward's grid (rows of its column-sum partials)


def _wgrad(g: torch.Tensor, x: torch.Tensor, splits: int = 64) -> torch.Tensor:
    """g^T x (fp16 [m, N], [m, K]) -> fp32 [N, K]: the weight gradient of a
    linear layer, a K = m reduction.  hipBLASLt runs this shape (m = 2^20,
    N x K = 512 x 128) at ~70 TFLOP/s; as `splits` batched GEMMs over row slices
    (fp32 partials: no fp16 overflow however many rows a slice sums) plus an
    fp32 sum of the partials it runs 7-10x faster (tools/gemm_probe.py)."""
    m = g.shape[0]
    if m % splits or m < 64 * splits:
        return torch.mm(g.t(), x, out_dtype=torch.float32)
    return torch.bmm(g.view(splits, m // splits, -1).transpose(1, 2), x.view(splits, m // splits, -1),
                     out_dtype=torch.float32).sum(0)


# Rows per update of the reference (T_HORIZON x NUM_ENVS, agent/config.py:4-6).  The
# manual fp16 epoch writes per-row gradients at GradScaler scale / min(n, REF_ROWS):
# the per-row fp16 magnitudes of the reference's own update, whatever the batch
# (scale / n at 4M rows would push them into fp16's subnormal range); the remaining
# factor min(n, REF_ROWS) / n is applied in fp32 to the summed weight gradients.
REF_ROWS = 4096

# Feature row width of the manual fp16 epoch: 208 = 198 features + 10 zero columns,
# so fc1's weight-gradient GEMM reads 16-byte aligned rows (396-byte rows keep
# hipBLASLt off its vector-load kernels; tools/gemm_probe_pad.py).  The zero columns
# meet zero weight columns: every product is unchanged.
FEAT_W = 208

PPO_GW2_TASK_TILES = 32        # include/bgx.h BGX_PPO_GW2_TASK_TILES
FEAT_BIAS_COL = 198            # the ones column of the 208-wide rows: gW1[:, 198] = gb1


def _row_scale(gscale: float, n_total: int):
    """(row_scale, post) of the two fp16 epochs (REF_ROWS above): the kernels' per-row gradient
    scale, and the fp32 factor that takes the summed gradients back to gscale = scale / n_total."""
    return gscale * n_total / min(n_total, REF_ROWS), min(n_total, REF_ROWS) / n_total


def _pack_head_fp16(net, rows: int):
    """[action_head; value_head] in fp16 as ONE weight [rows, H] and bias [rows]: the A
    action rows, the value row, zeros below."""
    Wa, ba, wv, bv = net.action_head.weight, net.action_head.bias, net.value_head.weight, net.value_head.bias
    A, Hd = Wa.shape
    W2h = torch.zeros(rows, Hd, dtype=torch.float16, device=Wa.device)
    b2h = torch.zeros(rows, dtype=torch.float16, device=Wa.device)
    W2h[:A] = Wa.half(); W2h[A] = wv[0].half()
    b2h[:A] = ba.half(); b2h[A] = bv[0].half()
    return W2h, b2h


def _hand_off_grads(net, gW1, gb1, gW2, gb2, post: float):
    """The fp32 sums of an fp16 epoch into W1.grad ... bv.grad, as autograd's would land:
    times `post`; fc1's weight without the padding columns of wider feature rows, its bias
    from the ones column of the 208-wide rows where it has no sum of its own (gb1 None:
    the fused epoch); the packed head's rows back to the action and the value head."""
    if post != 1.0:
        for t in (gW1, gb1, gW2, gb2):
            if t is not None:
                t.mul_(post)
    A = net.action_head.out_features
    F_in = net.fc1.weight.shape[1]
    net.fc1.weight.grad = gW1 if gW1.shape[1] == F_in else gW1[:, :F_in].contiguous()
    net.fc1.bias.grad = gb1 if gb1 is not None else gW1[:, FEAT_BIAS_COL].contiguous()
    net.action_head.weight.grad, net.action_head.bias.grad = gW2[:A].contiguous(), gb2[:A].contiguous()
    net.value_head.weight.grad, net.value_head.bias.grad = gW2[A:A + 1].contiguous(), gb2[A:A + 1].contiguous()


def _ppo_epoch_amp_manual(net, chunks, n_total, coefs, sums):
    """The fp16-autocast epoch's forward and backward written out (the same
    fp16 GEMMs, fp32 accumulation): [action_head; value_head] as ONE GEMM
    padded to 512 outputs (hipBLASLt: 0.35 vs 0.74 ms at 2^20 x 500), the loss
    head kernel reading the logits / writing their gradient in place (row stride
    512), ReLU backward on the stored activations, and split-K weight
    gradients (_wgrad).  Gradients land in p.grad as fp32, as autograd's would."""
    eps, c_v, c_e, gscale = coefs              # gscale = GradScaler scale / n_total
    row_scale, post = _row_scale(gscale, n_total)
    W1, b1 = net.fc1.weight, net.fc1.bias
    A, Hd = net.action_head.weight.shape
    Ap = (A + 1 + 31) // 32 * 32
    dev = W1.device
    with torch.no_grad():
        W1h, b1h = W1.half(), b1.half()
        F_in = W1.shape[1]
        W2h, b2h = _pack_head_fp16(net, Ap)
        gW1 = torch.zeros_like(W1); gb1 = torch.zeros_like(b1)
        gW2 = torch.zeros(Ap, Hd, dtype=torch.float32, device=dev)
        gb2 = torch.zeros(Ap, dtype=torch.float32, device=dev)
        L = _lib.load()
        stream = _stream(dev)
        colsum = torch.empty(PPO_COLSUM_BLOCKS, 512, dtype=torch.float32, device=dev)
        fc1_rec = L.bgx_fc1_packed_size(Hd) > 0        # else the GEMM over the feature rows
        if fc1_rec:                                 # W1h in the record kernel's fragment order
            w1pack = torch.empty(L.bgx_fc1_packed_size(Hd), dtype=torch.uint8, device=dev)
            check(L.bgx_fc1_pack(_ptr(W1h), Hd, _ptr(w1pack), stream), "bgx_fc1_pack")
        hsum = torch.empty(RELU_BLOCKS, Hd, dtype=torch.float32, device=dev)
        for c in chunks:
            x = c.feats.half()
            if x.shape[1] != W1h.shape[1]:          # zero-padded rows: zero weight columns to match
                W1h = torch.nn.functional.pad(W1h, (0, x.shape[1] - F_in))
                gW1 = torch.zeros(W1.shape[0], x.shape[1], dtype=torch.float32, device=dev)
            if fc1_rec:                             # fc1 forward from the 64-byte records (no feature read)
                h = torch.empty(x.shape[0], Hd, dtype=torch.float16, device=dev)
                rec = c.records.contiguous()
                check(L.bgx_fc1_records(_ptr(rec), rec.shape[0], _ptr(w1pack), _ptr(b1h), Hd, _ptr(h), stream),
                      "bgx_fc1_records")
            else:                                   # bias + ReLU in the GEMM epilogue (relu commutes with
                h = torch._addmm_activation(b1h, x, W1h.t())     # the fp16 rounding)
            y = F.linear(h, W2h, b2h)                      # [m, Ap]: logits | value | 0
            m = y.shape[0]
            vals = y[:, A].contiguous()
            dy = torch.empty_like(y)
            dval = torch.empty_like(vals)
            # dy = [dlogits | dvalue | 0] written by the kernel, with its column sums
            check(L.bgx_ppo_head_ex(_ptr(y), 1, Ap, _ptr(vals), _ptr(c.records.contiguous()),
                                    _ptr(c.actions.to(torch.int32).contiguous()),
                                    _ptr(c.old_logp.float().contiguous()), _ptr(c.returns.float().contiguous()),
                                    _ptr(c.adv.float().contiguous()), m, A, eps, c_v, c_e, row_scale, _ptr(dy), Ap,
                                    _ptr(dval), _ptr(sums), 1, _ptr(colsum), stream), "bgx_ppo_head_ex")
            gW2 += _wgrad(dy, h)
            gb2 += colsum.sum(0)[:Ap]
            dh = dy @ W2h
            # relu backward (grad where out > 0) in place + the bias gradient's column sums
            check(L.bgx_relu_backward(_ptr(dh), _ptr(h), m, Hd, _ptr(hsum), RELU_BLOCKS, stream), "bgx_relu_backward")
            gW1 += _wgrad(dh, x)
            gb1 += hsum.sum(0)
    _hand_off_grads(net, gW1, gb1, gW2, gb2, post)


def ppo_row_plan(records: torch.Tensor, n_actions: int = 500):
    """ppo_row_plan_torch on the GPU as three HIP launches (bgx_ppo_plan: a stable
    counting sort by class plus the plan from the class totals), no host sync; the
    torch form on the CPU.  Returns (perm int32[m], plan int32[33], row_plan int32[8])."""
    if not records.is_cuda:
        return ppo_row_plan_torch(records, n_actions)
    m, dev, L = records.shape[0], records.device, _lib.load()
    rec = records.contiguous()
    ws = torch.empty(max(int(L.bgx_ppo_plan_workspace(m)) // 4, 1), dtype=torch.int32, device=dev)
    perm, plan, row_plan = (torch.empty(n, dtype=torch.int32, device=dev) for n in (m, 33, 8))
    check(L.bgx_ppo_plan(_ptr(rec), m, n_actions, _ptr(ws), _ptr(perm), _ptr(plan), _ptr(row_plan), _stream(dev)),
          "bgx_ppo_plan")
    return perm, plan, row_plan


def ppo_row_plan_torch(records: torch.Tensor, n_actions: int = 500):
    """Row order and work plan of bgx_ppo_rows / bgx_ppo_gw2 for one chunk of
    rollout rows (computed once per update; the records do not change across
    epochs).  A row needs the 32-action tiles holding its legal columns
    (ceil(cnt / 32); all 16 when cnt = 0, every action then being masked by the
    same constant); rows are sorted by that count (stable).  plan = the k_ppo_gw2
    task prefix per action tile (17) and the first row tile (in sorted order) that
    reaches each action tile (16); row_plan = the row tiles [lo, hi) of the
    bgx_ppo_rows variants for at most 1, 2, 4 and 16 leading action tiles.  Device
    tensors only: no host sync."""
    m = records.shape[0]
    cnt = records[:, 60].to(torch.int32) | (records[:, 61].to(torch.int32) << 8)
    lim = torch.where(cnt == 0, torch.full_like(cnt, n_actions), cnt.clamp(max=n_actions))
    cls = ((lim + 31) // 32).to(torch.uint8)
    perm = torch.argsort(cls, stable=True).to(torch.int32)
    cum = torch.cumsum(torch.bincount(cls, minlength=17), 0)
    start = torch.div(cum[:16], 32, rounding_mode="floor")
    start[15] = 0                                     # the value column's tile: every row
    ntiles = (m + 31) // 32
    # tasks of tile o: the kTS-aligned row groups that hold a row tile >= start[o]
    tasks = (ntiles + PPO_GW2_TASK_TILES - 1) // PPO_GW2_TASK_TILES - torch.div(start, PPO_GW2_TASK_TILES,
                                                                                rounding_mode="floor")
    pre = torch.cat([torch.zeros(1, dtype=tasks.dtype, device=tasks.device), torch.cumsum(tasks, 0)])
    # row tiles whose last (largest) row needs <= k tiles: cum[k] // 32, all of them at cum[k] == m
    e = torch.where(cum[[1, 2, 4]] >= m, torch.full_like(cum[[1, 2, 4]], ntiles), cum[[1, 2, 4]] // 32)
    z = torch.zeros(1, dtype=e.dtype, device=e.device)
    nt = torch.full_like(z, ntiles)
    row_plan = torch.stack([z[0], e[0], e[0], e[1], e[1], e[2], e[2], nt[0]]).to(torch.int32).contiguous()
    return perm, torch.cat([pre, start]).to(torch.int32).contiguous(), row_plan


def _row_fields(acts, old, R, adv):
    """The four per-row fields in the dtypes the row kernels read."""
    return acts.to(torch.int32).contiguous(), old.float().contiguous(), R.float().contiguous(), adv.float().contiguous()


def gather_rollout(perm, recs, acts, old, R, adv):
    """Rows perm[i] of the records and the four per-row fields, in one HIP kernel on the
    GPU (bgx_gather_rollout; torch's index gathers of the [m, 64] records ran at ~1 TB/s),
    the torch gathers elsewhere.  Returns (records, actions, old_logp, returns, adv)."""
    acts, old, R, adv = _row_fields(acts, old, R, adv)
    recs = recs.contiguous()
    if not recs.is_cuda:
        pl = perm.long()
        return recs[pl].contiguous(), acts[pl], old[pl], R[pl], adv[pl]
    m = perm.shape[0]
    out = tuple(torch.empty_like(t) for t in (recs, acts, old, R, adv))
    check(_lib.load().bgx_gather_rollout(_ptr(perm.to(torch.int32).contiguous()), m, _ptr(recs), _ptr(acts), _ptr(old),
                                         _ptr(R), _ptr(adv), *[_ptr(t) for t in out], _stream(recs.device)),
          "bgx_gather_rollout")
    return out


def plan_rollout(recs, acts, old, R, adv, n_actions: int = 500, out_rows=None, out_plan=None):
    """ppo_row_plan + gather_rollout in one pass on the GPU (bgx_ppo_plan_rows: the rows
    written straight to their plan-order positions).  Returns ((records, actions,
    old_logp, returns, adv) in plan order, plan, row_plan); out_rows / out_plan =
    (plan, row_plan) (the graphed update's persistent buffers) to write into."""
    if not recs.is_cuda:
        perm, plan, row_plan = ppo_row_plan_torch(recs, n_actions)
        return gather_rollout(perm, recs, acts, old, R, adv), plan, row_plan
    acts, old, R, adv = _row_fields(acts, old, R, adv)
    rec = recs.contiguous()
    m, dev = rec.shape[0], rec.device
    L = _lib.load()
    ws = torch.empty(max(int(L.bgx_ppo_plan_workspace(m)) // 4, 1), dtype=torch.int32, device=dev)
    rows = out_rows if out_rows is not None else tuple(torch.empty_like(t) for t in (rec, acts, old, R, adv))
    plan, row_plan = out_plan or (torch.empty(n, dtype=torch.int32, device=dev) for n in (33, 8))
    check(L.bgx_ppo_plan_rows(_ptr(rec), m, n_actions, _ptr(ws), _ptr(acts), _ptr(old), _ptr(R), _ptr(adv),
                              *[_ptr(t) for t in rows], None, _ptr(plan), _ptr(row_plan), _stream(dev)),
          "bgx_ppo_plan_rows")
    return rows, plan, row_plan


# The fused head computes, for a row with cnt >= 1 legal actions, only the action tiles
# holding its legal columns: the masked logits z + log(1e-45) (ppo_agent.py:166) are left
# out of the log-sum-exp and their gradients are 0.  That equals the reference exactly
# while every masked term lies e^-30 below the row's sum, i.e. while 2U + log(1e-45) <
# -30 with U a bound on |z|: U = max_a |Wa_h[a]| max_row |h| + max_a |ba_h[a]|.  The fc1
# kernel reports max_row |h|^2 (bgx_fc1_records_ex); PPOTrainer checks the bound after
# each update and redoes an update that broke it on the exact round-2 epoch.
MASK_SHORTCUT_LIMIT = -MASK_LOG - 30.0


def _ppo_epoch_amp_fused(net, chunks, n_total, coefs, sums, fast, guard=None, parts=None, entropy_coef=0.0):
    """The fp16-autocast epoch with the output layer and loss head fused
    (bgx_ppo_rows + bgx_ppo_gw2): fc1 from the records (bgx_fc1_records), then per
    row the logits, the loss head, dy and dh = ReLU'(h) fp16(dy W2h) on MFMA without
    the [n, 512] logits in HBM; gW2 / gb2 = dy^T [h | 1] from per-row statistics;
    gW1 / gb1 = dh^T [x | 1] with x generated from the records on chip (bgx_ppo_gw1:
    no feature rows in HBM).  Same fp16 operands, fp32 accumulation and per-row
    gradient scaling as _ppo_epoch_amp_manual; gradients land in p.grad as fp32.
    The chunks' feature entries are not read.  `fast` (epoch_path): one launch for the casts,
    the packed fc1 fragments and the zeroed accumulators and one for the gradient hand-off
    (bgx_ppo_epoch_prep / _grads) instead of ~20 small torch kernels per epoch.  `guard` (a
    device bool, optional) is set when the masked-action shortcut's bound (MASK_SHORTCUT_LIMIT)
    does not hold.  `parts` (fp64 [4], fast only): the prologue zeroes `sums` and the epilogue
    adds this epoch's loss parts to `parts` (the torch form's arithmetic): no small torch kernels."""
    eps, c_v, c_e, gscale = coefs
    row_scale, post = _row_scale(gscale, n_total)
    params = _mlp_params(net)
    A, Hd = net.action_head.weight.shape
    dev = params[0].device
    k1 = float(np.float32(row_scale) * np.float32(c_e))      # the kernel's fp32 gscale * c_entropy
    with torch.no_grad():
        L = _lib.load()
        stream = _stream(dev)
        w1pack = torch.empty(L.bgx_fc1_packed_size(Hd), dtype=torch.uint8, device=dev)
        hmax2 = bound = None
        g_shapes = ((Hd, FEAT_W), (512, Hd), (512,))     # gW1 over the 208-wide rows [x | 1 | 0], gW2, gb2
        if fast:
            b1h, W2h, b2h = (torch.empty(*s, dtype=torch.float16, device=dev) for s in ((Hd,), (512, Hd), (512,)))
            gW1, gW2, gb2 = (torch.empty(*s, dtype=torch.float32, device=dev) for s in g_shapes)
            if guard is not None:
                hmax2 = torch.empty(1, dtype=torch.float32, device=dev)
                bound = torch.empty(2, 512, dtype=torch.float32, device=dev)
            check(L.bgx_ppo_epoch_prep(*[_ptr(t) for t in params], Hd, A, _ptr(w1pack), _ptr(b1h), _ptr(W2h), _ptr(b2h),
                                       _ptr(gW1), _ptr(gW2), _ptr(gb2), _ptr(hmax2), _ptr(bound),
                                       _ptr(sums if parts is not None else None), stream), "bgx_ppo_epoch_prep")
        else:
            W1h, b1h = params[0].half(), params[1].half()
            W2h, b2h = _pack_head_fp16(net, 512)
            gW1, gW2, gb2 = (torch.zeros(*s, dtype=torch.float32, device=dev) for s in g_shapes)
            check(L.bgx_fc1_pack(_ptr(W1h), Hd, _ptr(w1pack), stream), "bgx_fc1_pack")
            if guard is not None:
                hmax2 = torch.zeros(1, dtype=torch.float32, device=dev)
        for c in chunks:
            rec = c.records.contiguous()
            m = rec.shape[0]
            perm = None                              # a given plan: the rows are in its order
            if c.plan is not None:
                plan, row_plan = c.plan
            else:
                perm, plan, row_plan = ppo_row_plan(rec, A)
            h = torch.empty(m, Hd, dtype=torch.float16, device=dev)
            check(L.bgx_fc1_records_ex(_ptr(rec), m, _ptr(w1pack), _ptr(b1h), Hd, _ptr(h), _ptr(hmax2), stream),
                  "bgx_fc1_records_ex")
            dh = torch.empty(m, Hd, dtype=torch.float16, device=dev)
            stats = torch.empty(m, 4, dtype=torch.float32, device=dev)
            info = torch.empty(m, dtype=torch.int32, device=dev)
            acts, old, ret, ad = _row_fields(c.actions, c.old_logp, c.returns, c.adv)
            check(L.bgx_ppo_rows(_ptr(h), _ptr(perm), _ptr(rec), _ptr(acts), _ptr(old), _ptr(ret), _ptr(ad), m, Hd, A,
                                 _ptr(W2h), _ptr(b2h), eps, c_v, c_e, row_scale, _ptr(dh), _ptr(stats), _ptr(info),
                                 _ptr(sums), None, None, _ptr(row_plan), 0, stream), "bgx_ppo_rows")
            ws = torch.empty(L.bgx_ppo_gw2_workspace(m) // 4, dtype=torch.float32, device=dev)
            check(L.bgx_ppo_gw2(_ptr(h), _ptr(perm), _ptr(stats), _ptr(info), m, Hd, A, _ptr(W2h), _ptr(b2h), k1,
                                _ptr(plan), _ptr(ws), _ptr(gW2), _ptr(gb2), stream), "bgx_ppo_gw2")
            # dh is in the order of rec (bgx_ppo_rows writes it in the original row order)
            ws1 = torch.empty(L.bgx_ppo_gw1_workspace(m) // 4, dtype=torch.float32, device=dev)
            check(L.bgx_ppo_gw1(_ptr(dh), _ptr(rec), m, Hd, _ptr(ws1), _ptr(gW1), stream), "bgx_ppo_gw1")
        if fast:
            grads = [torch.empty_like(t) for t in params]
            check(L.bgx_ppo_epoch_grads(_ptr(gW1), _ptr(gW2), _ptr(gb2), Hd, A, float(post), *[_ptr(g) for g in grads],
                                        _ptr(bound), _ptr(hmax2), float(MASK_SHORTCUT_LIMIT), _ptr(guard), _ptr(sums),
                                        float(n_total), float(VALUE_LOSS_COEF), float(entropy_coef), _ptr(parts),
                                        stream), "bgx_ppo_epoch_grads")
            for t, g in zip(params, grads):
                t.grad = g
            return
        if guard is not None:
            U = W2h[:A].float().norm(dim=1).max() * hmax2[0].sqrt() + b2h[:A].float().abs().max()
            guard |= 2.0 * U > MASK_SHORTCUT_LIMIT
    _hand_off_grads(net, gW1, None, gW2, gb2, post)


def adam_step(optimizer, scaler) -> bool:
    """`scaler.step(optimizer); scaler.update()` (ppo_agent.py:302-305) for a fused
    torch.optim.Adam as ONE HIP call (bgx_adam_step: the inf check, the Adam step and the
    scale update over every tensor's elements in one flat launch each; torch's fused path
    runs ~4 multi-tensor workgroups over a 90 k-parameter net plus a dozen small ops).
    The optimizer state and the GradScaler state are torch's own tensors, updated as
    torch would (tests/test_gpu_train.py::test_adam_step_matches_torch).  Returns False
    (nothing done) for a configuration it does not restate: the caller then runs torch's."""
    if not isinstance(optimizer, torch.optim.Adam) or len(optimizer.param_groups) != 1:
        return False
    grp = optimizer.param_groups[0]
    if (grp.get("weight_decay", 0) or grp.get("amsgrad") or grp.get("maximize") or grp.get("capturable")
            or grp.get("differentiable") or not grp.get("fused") or torch.is_tensor(grp["lr"])):
        return False
    ps = [p for p in grp["params"] if p.grad is not None]
    if not ps or len(ps) > 8 or any(p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda
                                    or not p.is_contiguous() or not p.grad.is_contiguous() for p in ps):
        return False
    dev = ps[0].device
    for p in ps:                                     # torch's lazy state (fused: fp32 device step)
        st = optimizer.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    found = getattr(optimizer, "_bgx_found", None)
    if found is None or found.device != dev:
        found = optimizer._bgx_found = torch.zeros(1, dtype=torch.int32, device=dev)
    use_scale = scaler is not None and scaler.is_enabled()
    if use_scale and (scaler._scale is None or scaler._growth_tracker is None):
        return False
    n = len(ps)
    arr = lambda ts: ctypes.cast((ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]), ctypes.c_void_p)
    st = [optimizer.state[p] for p in ps]
    numels = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
    b1, b2 = grp["betas"]
    check(_lib.load().bgx_adam_step(
        n, arr(ps), arr([p.grad for p in ps]), arr([s["exp_avg"] for s in st]), arr([s["exp_avg_sq"] for s in st]),
        arr([s["step"] for s in st]), ctypes.cast(numels, ctypes.c_void_p), float(grp["lr"]), float(b1), float(b2),
        float(grp["eps"]), _ptr(scaler._scale if use_scale else None),
        _ptr(scaler._growth_tracker if use_scale else None),
        float(scaler._growth_factor) if use_scale else 2.0, float(scaler._backoff_factor) if use_scale else 0.5,
        int(scaler._growth_interval) if use_scale else 1, _ptr(found), _stream(dev)), "bgx_adam_step")
    return True
