"""GPU-resident PPO self-play trainer (the reference's train.py:30-123 loop,
ppo_agent.py:218-366 update) on the bgx engine.

Rollout: every step the fused policy kernel (bgx_policy_act) samples an
action for all B lanes from their 64-byte lane records, the engine steps them,
and the step's records / actions / log-probs / values / rewards / dones are
kept in device buffers [T, B] (records are int8 boards: 64 B per sample instead
of the reference's 792-byte fp32 observation); optionally mirrored to pinned
host memory on a side stream.

Update: returns, global normalisation, advantages = R_hat - V_old, then
NUM_EPOCHS full-batch epochs exactly like ppo_agent.py:268-305 (autocast +
GradScaler + Adam, clip 0.25, 0.5*MSE, -c_ent*H) but computed in chunks with
gradient accumulation (features re-encoded from the stored records by the HIP
encoder) and ONE all-reduce of the gradients per epoch across ranks.

Entropy coefficient (`entropy_anneal`): the reference's update always calls
update_entropy_coef (ppo_agent.py:193-197), which anneals by
`agent.total_episodes`.  Its vectorised driver train.py never increments that
counter (it counts a module-global `total_episodes`, train.py:74), so under
train.py the coefficient stays at ENTROPY_COEF_START = 0.15 for the whole run;
train_single.py increments `agent.total_episodes` per episode (train_single.py:78)
and the coefficient anneals to 0.01 over 400,000 episodes.  PPOTrainer restates
train.py, so `entropy_anneal="train"` (constant 0.15) is the default;
`"train_single"` anneals by the episodes finished in the rollouts.

Returns: `returns="lane"` (default) discounts within each game lane;
`returns="reference"` reproduces the reference's quirk of discounting over the
flat step-major memory in which the environments are interleaved
(ppo_agent.py:206-216).  Both restate the reference: one unsigned
reward stream runs across both players of a lane, and nothing is bootstrapped at
the horizon.  `returns="selfplay"` treats the lane as the two-player zero-sum game
it is: GAE(lambda) from the mover's point of view, the sign flipped where the turn
passes, cut at each game end, bootstrapped from the value of the position the
rollout stopped in (selfplay_gae, two HIP calls; `gae_lambda`, `gamma`; DESIGN.md §6
"Self-play returns").  The advantages are normalised over all rows, the value
targets are not.

What is computed from a finished rollout is in bgx/returns.py, one PPO epoch in
bgx/ppo_epoch.py; their names are re-exported here.

    python -m bgx.train --batch 65536 --horizon 64 --updates 10 [--metrics m.jsonl]
    torchrun --nproc-per-node 8 -m bgx.train ...            (one process per GPU)
    python -m bgx.train ... --eval-every 5 --eval-opponent random   (a head-to-head match of
        the current weights after every 5th update, bgx.arena; one rank only)
    python -m bgx.train ... --returns selfplay [--gae-lambda 0.95] [--gamma 0.99]
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist
from torch.amp import GradScaler

from .engine import Engine, encode_records
from .graphs import capture
from .hostcopy import HostMirror
from .policy import PolicyNet
from .ppo import (GAMMA, LEARNING_RATE, NUM_EPOCHS, ENTROPY_COEF_START, ENTROPY_COEF_END, ENTROPY_ANNEAL_EPISODES,
                  global_normalize, _world)
from .ppo_epoch import (FEAT_BIAS_COL, FEAT_W, MASK_SHORTCUT_LIMIT, PPO_COLSUM_BLOCKS,  # noqa: F401 (re-exports)
                        PPO_GW2_TASK_TILES, REF_ROWS, RELU_BLOCKS, Chunk, ScaleHint, _PPOHead, adam_step, epoch_path,
                        features_and_masks, gather_rollout, plan_rollout, ppo_epoch, ppo_row_plan, ppo_row_plan_torch)
from .returns import (EPISODE_STATS, RETURNS_MODES, _gae_scalars, _lane_returns_torch,  # noqa: F401 (re-exports)
                      _selfplay_gae_torch, check_returns_mode, episode_stats, episode_stats_records, lane_returns,
                      reference_returns, selfplay_gae)


def entropy_coef_after_update(mode: str, total_episodes: int) -> float:
    """update_entropy_coef (ppo_agent.py:193-197) as each reference driver feeds it:
    train.py leaves agent.total_episodes at 0 (it increments a module global,
    train.py:74), so the coefficient stays at the start value; train_single.py
    counts every episode into it (train_single.py:78)."""
    episodes = total_episodes if mode == "train_single" else 0
    progress = min(1.0, episodes / ENTROPY_ANNEAL_EPISODES)
    return ENTROPY_COEF_START - progress * (ENTROPY_COEF_START - ENTROPY_COEF_END)


class PPOTrainer:
    def __init__(self, batch: int = 65536, horizon: int = 64, hidden: int = 128, n_actions: int = 500,
                 seed: int = 0, device=None, process_group=None, pinned: bool = False, returns: str = "lane",
                 chunk: int = 1 << 21, fused: bool | None = None, amp: bool = True,
                 entropy_anneal: str = "train", shards: int | None = None, graphs: bool | None = None,
                 fork: bool | None = None, streams=None, update_graphs: bool | None = None,
                 gae_lambda: float = 0.95, gamma: float = GAMMA):
        if entropy_anneal not in ("train", "train_single"):
            raise ValueError(f"entropy_anneal must be 'train' or 'train_single', got {entropy_anneal!r}")
        self.entropy_anneal = entropy_anneal
        self.returns_mode = check_returns_mode(returns)
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.group = process_group
        self.rank = dist.get_rank(process_group) if _world(process_group) > 1 else 0
        self.B, self.T, self.A = batch, horizon, n_actions
        # returns="selfplay" only: GAE's lambda and the discount (the other modes discount by GAMMA)
        self.gae_lambda, self.gamma = float(gae_lambda), float(gamma)
        # rows per update chunk (gradient accumulation over chunks): 2^21 = a whole 65,536 x 32
        # rollout in one chunk, the reference's single full batch; 2^20-row chunks cost
        # 8.4 vs 7.8 ms per update (twice the per-call partial sums and launches)
        self.chunk = chunk
        self.fused = (self.dev.type == "cuda") if fused is None else fused
        self.amp = amp            # the reference's autocast (fp16 on the GPU); False = fp32 update
        # the fused output layer + loss head (csrc/bg_ppo_fused.hip) while its exactness bound
        # holds (MASK_SHORTCUT_LIMIT; update() falls back to the exact epoch otherwise)
        self.fused_head = True
        # the B lanes as S engines on S streams (bench.py's C3 layout: one shard's policy
        # kernel runs beside another's env step); shard 0 keeps the 1-shard seeds.  4 shards
        # from 65,536 lanes (one per hardware queue: PPO iteration 133 -> 136 M vs 2)
        if shards is None:
            cuda = self.dev.type == "cuda"
            shards = (4 if cuda and batch >= 65536 and batch % 1024 == 0 else
                      2 if cuda and batch >= 32768 and batch % 256 == 0 else 1)
        if batch % shards:
            raise ValueError(f"batch {batch} is not a multiple of shards {shards}")
        self.S = shards
        self.engs = [Engine(batch=batch // shards, max_moves=n_actions,
                            seed=seed * 1_000_003 + self.rank + 7_919 * k, dice="philox", auto_reset=True,
                            device=self.dev) for k in range(shards)]
        self.eng = self.engs[0]
        # rollout steps replayed as HIP graphs (2 steps per graph, one graph per slot pair
        # and shard), captured at the end of the first rollout: the engines' host state is
        # then a 2-step fixed point (bench.py C3).  Equal to the eager rollout
        # (tests/test_gpu_train.py::test_rollout_graphs_match_eager).  With pinned=True each
        # replayed pair's rows go to the host by one copy launch (bgx.hostcopy) on the
        # shard's copy stream, beside the next pair's steps.
        self.graphs = (self.dev.type == "cuda" and horizon % 2 == 0) if graphs is None else graphs
        self._graphs = None
        self._ctrs = None              # per shard: the graphs' device step counter (_capture)
        # the update's fused-head epoch replayed as a HIP graph (round 5): one eager epoch
        # issues ~50 small torch launches between the big kernels, and the GPU idled 1.4 ms
        # per update waiting for the host (profiles/r5/update_trace_plan.txt).  The graph is
        # captured at the second update (the first initialises the Adam and GradScaler
        # state eagerly) over persistent row buffers, and again when its host-side inputs
        # change: the GradScaler scale (a growth or a skipped step) or the entropy
        # coefficient.  Not with a process group (collectives stay eager).
        self.update_graphs = ((self.dev.type == "cuda" and _world(process_group) == 1
                               and not (dist.is_available() and dist.is_initialized()))
                              if update_graphs is None else bool(update_graphs))
        self._ugraph = None            # (key, graph, loss-parts output)
        self._ugraph_captures = 0
        self._ubufs = None             # (N, persistent per-chunk rows in plan order + plans)
        self._uparts = torch.zeros(4, dtype=torch.float64, device=self.dev)   # the captured epochs' loss parts
        self._updates_done = 0
        # the fused head's bound flag (a captured epoch writes it), the verified scaler state, the snapshot's lists
        self._guard = torch.zeros((), dtype=torch.bool, device=self.dev)
        self._scale_next = None
        self._snap_cache = None
        self._pending_stats = self._pending_eps = None     # a deferred rollout's statistics, then its episodes
        self._evals_done = 0
        # fork (Engine.set_fork): an env step's light launch on the engine's side stream.
        # Off by default with graphs: each shard's graph is then one linear chain on its own
        # hardware queue (forked graphs' internal streams share queues with the other
        # shards' and serialise them: rollout 9.2 -> 6.3 ms at 65,536 x 32)
        self.fork = (not self.graphs) if fork is None else bool(fork)
        for e in self.engs:
            e.set_fork(self.fork)
        torch.manual_seed(seed)
        self.net = PolicyNet(hidden_size=hidden, action_size=n_actions).to(self.dev)
        if _world(process_group) > 1:
            for p in self.net.parameters():
                dist.broadcast(p.data, src=0, group=process_group)
        # ppo_agent.py:83 Adam; on the GPU the fused kernel: GradScaler hands it the scale and
        # the inf flag as device tensors, so an optimizer step needs no host sync
        # (the foreach path's found_inf.item() left ~115 us idle per epoch)
        fused_adam = self.dev.type == "cuda"
        self.opt = torch.optim.Adam(self.net.parameters(), lr=LEARNING_RATE, fused=fused_adam)
        self.scaler = GradScaler(device=self.dev.type)
        self.total_episodes = 0
        self.entropy_coef = ENTROPY_COEF_START
        self.step_counter = 0
        self.seed = seed
        self._alloc_buffers(pinned)
        for e in self.engs:
            e.reset(want_obs=False)
        # `streams`: the S shard streams to use (a process that already runs shards on
        # streams of its own passes them: HIP maps streams onto its 4 hardware queues in
        # creation order, and a fresh set created after many others may land two shards
        # on one queue -- bench.py's PPO leg after the C3/C4/C2 legs: 113 vs 136 M)
        if streams is not None:
            if len(streams) != self.S:
                raise ValueError(f"streams: {len(streams)} given for {self.S} shards")
            self._streams = list(streams)
        else:
            self._streams = ([torch.cuda.current_stream(self.dev)] +
                             [torch.cuda.Stream(self.dev) for _ in range(self.S - 1)]
                             if self.dev.type == "cuda" else [None])
        # per shard: the stream its host copies run on -- with forked steps a copy stream
        # beside the next steps; with linear shards the shard's own stream (one hardware
        # queue per shard; the other shards' steps run beside the copy)
        self._copy_streams = ([torch.cuda.Stream(self.dev) if self.fork else None for _ in range(self.S)]
                              if pinned else None)

    def _alloc_buffers(self, pinned: bool):
        """The [T, B] rollout buffers, their pinned host mirror and the episode carry."""
        T, B = self.T, self.B
        kw = dict(device=self.dev)
        self.buf = {"records": torch.empty(T, B, 64, dtype=torch.uint8, **kw),
                    "actions": torch.empty(T, B, dtype=torch.int32, **kw),
                    "logp": torch.empty(T, B, dtype=torch.float32, **kw),
                    "values": torch.empty(T, B, dtype=torch.float32, **kw),
                    "rewards": torch.empty(T, B, dtype=torch.float32, **kw),
                    "dones": torch.empty(T, B, dtype=torch.uint8, **kw)}
        self.pinned = None
        if pinned:                      # the rollout mirrored into pinned host memory
            if (B // self.S) % 16:
                raise ValueError(f"pinned=True copies each shard's lanes in 16-byte chunks: the shard batch "
                                 f"{B // self.S} must be a multiple of 16")
            self.mirror = HostMirror(dict(self.buf))        # the [T, B] step fields only
            self.pinned = self.mirror.host
        # returns="selfplay": value and record of the position each lane's rollout stopped in
        # (GAE's bootstrap), written by rollout()'s closing value pass or load_rollout
        self._boot = False
        if self.returns_mode == "selfplay":
            self.buf["boot_values"] = torch.empty(B, dtype=torch.float32, **kw)
            self.buf["boot_records"] = torch.empty(B, 64, dtype=torch.uint8, **kw)
            self._boot_scratch = (torch.empty(B, dtype=torch.int32, **kw), torch.empty(B, dtype=torch.float32, **kw))
        self.ep_carry = torch.zeros(B, dtype=torch.float64, **kw)     # train.py:58 episode_rewards
        self.last_episode_stats = None

    def _lanes(self, k: int):
        """Shard k's lane range [lo, hi)."""
        n = self.B // self.S
        return k * n, (k + 1) * n

    def _mirror_slots(self, k: int, t0: int, n: int):
        """Shard k's rows of slots [t0, t0 + n) to the pinned host buffers, on the shard's
        copy stream forked from its step stream (joined at the end of rollout())."""
        cs, cur = self._copy_streams[k], torch.cuda.current_stream(self.dev)
        if cs is not None:
            cs.wait_stream(cur)
        self.mirror.copy(t0, n, *self._lanes(k), stream=cs if cs is not None else cur)    # linear shards: the step stream

    def _slot(self, k: int, t: int):
        """Shard k's views of rollout slot t (contiguous row ranges)."""
        lo, hi = self._lanes(k)
        b = self.buf
        return ((b["actions"][t][lo:hi], b["logp"][t][lo:hi], b["values"][t][lo:hi]), b["records"][t][lo:hi],
                (b["rewards"][t][lo:hi], b["dones"][t][lo:hi]))

    def _act_step(self, k: int, t: int, step: int, step_ctr=None):
        out, rec, env_out = self._slot(k, t)
        self.net.act(self.engs[k], seed=self.seed * 7919 + self.rank + 104_729 * k, step=step, step_ctr=step_ctr,
                     out=out, records_out=rec)
        self.engs[k].step(out[0], want_obs=False, want_info=False, out=env_out)

    def _boot_pass(self, k: int):
        """returns="selfplay": one value pass over shard k's lanes as the rollout left them
        (the packed weights the rollout used), into boot_values / boot_records.  Greedy: no
        noise is drawn, so neither the step counter nor any generator moves; the action and
        log-prob go to scratch.  Eager, after the replayed graphs, on the shard's stream."""
        lo, hi = self._lanes(k)
        a, lp = self._boot_scratch
        self.net.act(self.engs[k], greedy=True, out=(a[lo:hi], lp[lo:hi], self.buf["boot_values"][lo:hi]),
                     records_out=self.buf["boot_records"][lo:hi])

    def _capture(self):
        """One graph per (slot pair, shard): act + step for slots t and t + 1 with the
        noise step read from the shard's device counter (advanced by 2 per replay),
        the engine joined at the end (its side-stream dispatch order).  Thread-local
        capture mode: a communicator's watchdog thread may query events meanwhile.
        A failed capture is terminal (bgx/graphs.py)."""
        self._ctrs = [torch.zeros(1, dtype=torch.int32, device=self.dev) for _ in range(self.S)]
        caps = [torch.cuda.Stream(self.dev) for _ in range(self.S)]
        for k in range(self.S):
            caps[k].wait_stream(self._streams[k])
            with torch.cuda.stream(caps[k]):
                self.engs[k].join()
        torch.cuda.synchronize(self.dev)
        def two_steps(k, t):
            for j in range(2):
                self._act_step(k, t + j, j, self._ctrs[k])
            self.engs[k].join()
            PolicyNet.advance_counter(self._ctrs[k], 2)
        # a failed capture ends the process (bgx/graphs.py: the engines' host state has
        # advanced through steps that never ran)
        graphs = [[capture("trainer", lambda k=k, t=t: two_steps(k, t), caps[k]) for k in range(self.S)]
                  for t in range(0, self.T, 2)]
        torch.cuda.synchronize(self.dev)
        self._graphs = graphs

    def rollout(self, defer_stats: bool = False):
        """T env steps on all B lanes (train.py:46-99 without the Python loops).  Returns
        the episodes finished; with defer_stats the episode statistics stay on the device
        until the next update() reads them with its own final sync (iteration(): no host
        sync, and so no idle GPU, between the rollout and the update) and None is returned."""
        self.net.pack(inplace=True)
        buf = self.buf
        cur = self._streams[0]
        for st in self._streams[1:]:
            st.wait_stream(cur)                  # the packed weights, the previous update
        if self._graphs is not None:
            for k in range(self.S):
                with torch.cuda.stream(self._streams[k]):
                    self._ctrs[k].fill_(self.step_counter)
            for t, row in zip(range(0, self.T, 2), self._graphs):     # the shards' replays side by side
                for k in range(self.S):
                    with torch.cuda.stream(self._streams[k]):
                        row[k].replay()
                        if self.pinned is not None:  # the pair's rows to the host beside the next pair
                            self._mirror_slots(k, t, 2)
            self.step_counter += self.T
        for t in range(self.T if self._graphs is None else 0):
            for k in range(self.S):
                with torch.cuda.stream(self._streams[k]):
                    self._act_step(k, t, self.step_counter)
                    if self.pinned is not None:
                        self._mirror_slots(k, t, 1)
            self.step_counter += 1
        for k, cs in enumerate(self._copy_streams or ()):      # pinned: each shard's stream joins its copies
            if cs is not None:
                self._streams[k].wait_stream(cs)
        if self.returns_mode == "selfplay":
            for k in range(self.S):
                with torch.cuda.stream(self._streams[k]):
                    self._boot_pass(k)
            self._boot = True
        for st in self._streams[1:]:
            cur.wait_stream(st)
        if cur is not None and cur != torch.cuda.current_stream(self.dev):
            torch.cuda.current_stream(self.dev).wait_stream(cur)   # the statistics and update() run there
        if self.graphs and self._graphs is None:
            self._capture()
        st = episode_stats_records(buf["rewards"], buf["dones"], buf["records"], self.ep_carry)
        if _world(self.group) > 1:
            dist.all_reduce(st, group=self.group)
        if defer_stats:
            if self._pending_stats is not None:   # an earlier deferred rollout, no update since
                self._apply_stats(self._pending_stats)
            self._pending_stats = st
            return None
        return self._apply_stats(st)

    def _apply_stats(self, st):
        self.last_episode_stats = dict(zip(EPISODE_STATS, st.tolist()))
        eps = int(self.last_episode_stats["episodes"])
        self.total_episodes += eps
        return eps

    def _fill(self, name: str, v):
        """Copy `v` (any shape with the buffer's element count) into rollout buffer `name`."""
        v = torch.as_tensor(v)
        if v.numel() != self.buf[name].numel():
            raise ValueError(f"load_rollout: {name} has {v.numel()} elements, the buffer {self.buf[name].numel()}")
        self.buf[name].copy_(v.reshape(self.buf[name].shape).to(self.buf[name].dtype))

    def load_rollout(self, records, actions, logp, values, rewards, dones, boot_values=None, boot_records=None):
        """Fill the [T, B] rollout buffers from given data (e.g. a reference
        agent's memory, step-major) instead of running rollout().  boot_values [B] /
        boot_records [B, 64] (returns="selfplay" only): value and record of the position
        after the last step; without them the horizon is a cut."""
        if (boot_values is None) != (boot_records is None):
            raise ValueError("load_rollout: boot_values and boot_records go together")
        if boot_values is not None and self.returns_mode != "selfplay":
            raise ValueError("load_rollout: a bootstrap is used by returns='selfplay' only")
        src = {"records": records, "actions": actions, "logp": logp, "values": values, "rewards": rewards,
               "dones": dones}
        for name, v in src.items():
            self._fill(name, v)
        self._boot = boot_values is not None
        if self._boot:
            self._fill("boot_values", boot_values)
            self._fill("boot_records", boot_records)

    def _path(self):
        """The epoch implementation the update runs (ppo_epoch.epoch_path)."""
        return epoch_path(self.net, self.fused, self.amp, self.fused_head)

    def update(self):
        """ppo_agent.py:218-366 on the device buffers."""
        buf = self.buf
        fused_head = self._path().kind == "fused"
        # the snapshot's host work first: it overlaps the rollout's last kernels instead of
        # idling the GPU between the return computation and the epochs (~0.17 ms)
        snap = self._snapshot() if fused_head else None
        if self.returns_mode == "selfplay":
            adv, R = selfplay_gae(buf["rewards"], buf["dones"], buf["records"], buf["values"],
                                  buf["boot_values"] if self._boot else None,
                                  buf["boot_records"] if self._boot else None, self.gamma, self.gae_lambda,
                                  group=self.group)
            adv, R = adv.reshape(-1), R.reshape(-1)
        else:
            if self.returns_mode == "reference":
                R = reference_returns(buf["rewards"], buf["dones"])
            else:
                R = lane_returns(buf["rewards"], buf["dones"])
            R = global_normalize(R.reshape(-1), self.group)
            adv = R - buf["values"].reshape(-1)
        rows = (buf["records"].reshape(-1, 64), buf["actions"].reshape(-1), buf["logp"].reshape(-1), R, adv)
        if not fused_head:
            parts = self._epochs(*rows)
        else:
            guard = self._guard
            guard.zero_()
            # the scaler's state as the previous update verified it (no host sync here, where
            # it would idle the GPU between the return computation and the epochs), else read
            hint, self._scale_next = self._scale_next or self._scale_state(), None
            parts = self._epochs(*rows, guard, scale_hint=hint)
            if hint is not None and self._scale_state() != hint:
                # a non-finite step was skipped (the scale backed off on the device): the
                # later epochs ran at the host's scale; redo the update with get_scale()
                self._restore(snap)
                guard.zero_()
                parts = self._epochs(*rows, guard)
            elif hint is not None:
                self._scale_next = hint.copy()     # = the device state after this update
            # the bound check of the update that is kept (after any redo above)
            g = guard.to(torch.int32)
            if _world(self.group) > 1:
                dist.all_reduce(g, op=dist.ReduceOp.MAX, group=self.group)
            if bool(g.item()):               # the masked-action shortcut's bound broke: redo exactly
                self._scale_next = None
                print("[bgx] PPO update: logit bound above the fused head's exact range; update redone on the "
                      "exact epoch, later updates too", flush=True)
                self._restore(snap)
                self.fused_head = False
                parts = self._epochs(*rows)
        if self._pending_stats is not None:    # a deferred rollout's statistics
            self._pending_eps = self._apply_stats(self._pending_stats)
            self._pending_stats = None
        self.entropy_coef = entropy_coef_after_update(self.entropy_anneal, self.total_episodes)
        self._updates_done += 1
        p = (parts / NUM_EPOCHS).tolist()
        return {"policy_loss": p[0], "value_loss": p[1], "entropy": p[2], "total_loss": p[3]}

    def _scale_state(self):
        """The GradScaler's (scale, growth tracker) on the host (one sync), or None when
        scaling is off."""
        if not self.scaler.is_enabled():
            return None
        self.scaler.scale(torch.ones((), device=self.dev))     # lazy initialisation
        return ScaleHint(float(self.scaler._scale.item()), int(self.scaler._growth_tracker.item()))

    def _epochs(self, recs, acts, old, R, adv, guard=None, scale_hint=None):
        """The NUM_EPOCHS full-batch epochs of one update on the trainer's path; returns
        the summed loss parts (device, fp64)."""
        N = recs.shape[0]
        path = self._path()
        spans = [(s, min(N, s + self.chunk)) for s in range(0, N, self.chunk)]
        if path.kind == "fused":
            if self.update_graphs and guard is not None and scale_hint is not None and self._updates_done >= 1:
                return self._epochs_graphed(recs, acts, old, R, adv, guard, scale_hint)
            # once per update: each chunk's rows in the order of the fused head's row plan
            # (by the number of action tiles a row needs), gathered so that every kernel
            # of the 4 epochs reads them contiguously.  The fused head generates every
            # feature it needs from the records (fc1 forward, gW1)
            planned = [plan_rollout(recs[s:e], acts[s:e], old[s:e], R[s:e], adv[s:e], self.A) for s, e in spans]
            fixed = [Chunk(None, None, *rows[1:], rows[0], (plan, row_plan)) for rows, plan, row_plan in planned]
        elif self.fused:    # features encoded once for the 4 epochs; the loss kernel reads the legal counts
            fixed = [Chunk(encode_records(recs[s:e], torch.float16 if self.amp else torch.float32,
                                          width=FEAT_W if path.kind == "manual" else 198), None,     # from the records
                           acts[s:e], old[s:e], R[s:e], adv[s:e], recs[s:e]) for s, e in spans]

        def chunks():
            if self.fused:
                return fixed
            return (Chunk(*features_and_masks(recs[s:e], self.A), acts[s:e], old[s:e], R[s:e], adv[s:e], recs[s:e])
                    for s, e in spans)

        parts = torch.zeros(4, dtype=torch.float64, device=self.dev)
        for _ in range(NUM_EPOCHS):
            e = ppo_epoch(self.net, self.opt, self.scaler, chunks(), N, self.entropy_coef, self.group, amp=self.amp,
                          fused=self.fused, sync=False, guard=guard, fused_head=self.fused_head,
                          scale_hint=scale_hint, parts=parts)
            if e is not parts:                 # the torch epoch returns its own (host) parts
                parts += e.to(parts.device)
        return parts

    def _epochs_graphed(self, recs, acts, old, R, adv, guard, hint):
        """_epochs' fused-head epochs as HIP-graph replays: the rows go into persistent
        plan-order buffers (eager), one epoch is captured per (GradScaler scale, entropy
        coefficient) and replayed NUM_EPOCHS times; the host's copy of the scaler state
        advances per replay as ppo_epoch advances it."""
        N = recs.shape[0]
        spans = [(s, min(N, s + self.chunk)) for s in range(0, N, self.chunk)]
        if self._ubufs is None or self._ubufs[0] != N:      # (N, per chunk: (rows, (plan, row_plan)) in plan order)
            self._ubufs, self._ugraph = (N, [(None, None)] * len(spans)), None
        bufs = self._ubufs[1]
        for i, (s, e) in enumerate(spans):      # plan_rollout allocates them the first time, then writes in place
            rows, *plan = plan_rollout(recs[s:e], acts[s:e], old[s:e], R[s:e], adv[s:e], self.A, *bufs[i])
            bufs[i] = (rows, tuple(plan))
        chunks = [Chunk(None, None, *rows[1:], rows[0], plan) for rows, plan in bufs]

        self._uparts.zero_()                   # the captured epochs add their loss parts to it
        cur = torch.cuda.current_stream(self.dev)
        for _ in range(NUM_EPOCHS):
            key = self._ugraph_key(hint.scale, N)
            if self._ugraph is None or self._ugraph[0] != key:
                self._ugraph_captures += 1
                self._ugraph = None
                st = torch.cuda.Stream(self.dev)
                st.wait_stream(cur)
                out = {}

                def body():
                    out["e"] = ppo_epoch(self.net, self.opt, self.scaler, chunks, N, self.entropy_coef, self.group,
                                         amp=self.amp, fused=self.fused, sync=False, guard=guard, fused_head=True,
                                         scale_hint=hint.copy(), parts=self._uparts)
                g = capture("ppo_update", body, st)
                cur.wait_stream(st)
                self._ugraph = (key, g, out["e"])
            self._ugraph[1].replay()
            if self.scaler.is_enabled():
                hint.advance(self.scaler)
        return self._uparts.clone()

    def _snapshot_tensors(self):
        ts = [p for p in self.net.parameters()]
        for p in self.net.parameters():
            ts += [v for _, v in sorted(self.opt.state[p].items()) if torch.is_tensor(v)] if p in self.opt.state else []
        ts += [t for t in (getattr(self.scaler, "_scale", None), getattr(self.scaler, "_growth_tracker", None))
               if torch.is_tensor(t)]
        return ts

    def _snapshot(self):
        """The weights, the Adam state and the GradScaler state (no host sync) as one
        concatenated device copy per dtype, so that an update can be redone.  The tensor
        lists are cached while the same tensors are in place (Adam and the scaler update
        theirs in place), so a snapshot costs one torch.cat per dtype of host time."""
        ts = self._snapshot_tensors()
        sig = tuple(id(t) for t in ts)
        if self._snap_cache is None or self._snap_cache[0] != sig:
            groups = {dt: [t.detach().reshape(-1) for t in ts if t.dtype == dt] for dt in {t.dtype for t in ts}}
            keys = {id(p) for p in self.net.parameters() if p in self.opt.state}
            scal = {k: torch.is_tensor(getattr(self.scaler, k, None)) for k in ("_scale", "_growth_tracker")}
            self._snap_cache = (sig, groups, keys, scal)
        _, groups, keys, scal = self._snap_cache
        flat = {dt: torch.cat(g) for dt, g in groups.items()}
        return flat, set(keys), dict(scal)

    def _restore(self, snap):
        flat, keys, scal = snap
        with torch.no_grad():
            for p in self.net.parameters():
                if id(p) not in keys:                # no Adam state before the update: none after it
                    self.opt.state.pop(p, None)
            for k, had in scal.items():
                if not had:
                    setattr(self.scaler, k, None)    # lazily re-initialised, as before the update
            off = {dt: 0 for dt in flat}
            for t in self._snapshot_tensors():
                n = t.numel()
                t.copy_(flat[t.dtype][off[t.dtype]:off[t.dtype] + n].view_as(t))
                off[t.dtype] += n

    def _ugraph_key(self, scale, N):
        """What the captured update graph bakes in: the GradScaler scale, the entropy
        coefficient and the row count (kernel arguments), Adam's lr / betas / eps (passed by
        value to bgx_adam_step), and the device addresses of every parameter, its Adam state
        and the scaler's tensors (an optimizer or scaler reload replaces them).  Any change
        recaptures."""
        grp = self.opt.param_groups[0]
        ptrs = []
        for p in self.net.parameters():
            ptrs.append(p.data_ptr())
            st = self.opt.state.get(p, {})
            ptrs.extend(st[k].data_ptr() if torch.is_tensor(st.get(k)) else None
                        for k in ("exp_avg", "exp_avg_sq", "step"))
        for k in ("_scale", "_growth_tracker"):
            t = getattr(self.scaler, k, None)
            ptrs.append(t.data_ptr() if torch.is_tensor(t) else None)
        return (scale, float(self.entropy_coef), N, float(grp["lr"]), tuple(float(b) for b in grp["betas"]),
                float(grp["eps"]), id(self.opt), id(self.scaler), tuple(ptrs))

    def iteration(self):
        # rollout and update back to back on the device (the episode statistics are read at
        # the update's final sync); their split is timed with events
        cur = torch.cuda.current_stream(self.dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t0 = time.perf_counter()
        ev[0].record(cur)
        self.rollout(defer_stats=True)
        ev[1].record(cur)
        m = self.update()
        ev[2].record(cur)
        torch.cuda.synchronize(self.dev)
        t2 = time.perf_counter()
        eps = self._pending_eps
        # both phases on the GPU's clock (ev 0 -> 1 -> 2); the wall time covers the host too
        t_roll = ev[0].elapsed_time(ev[1]) * 1e-3
        t_upd = ev[1].elapsed_time(ev[2]) * 1e-3
        ws = _world(self.group)
        e = self.last_episode_stats
        k = max(e["episodes"], 1.0)
        m.update({"avg_episode_reward": e["episode_reward_sum"] / k, "win_rate": e["wins"] / k,
                  "p1_win_rate": e["p1_wins"] / k, "gammon_rate": e["gammons"] / k,
                  "backgammon_rate": e["backgammons"] / k, "total_episodes": self.total_episodes})
        m.update({"episodes": eps, "env_steps": self.B * self.T * ws, "rollout_s": t_roll, "update_s": t_upd,
                  "env_steps_per_s": self.B * self.T * ws / (t2 - t0), "entropy_coef": self.entropy_coef})
        return m

    def save(self, path: str):
        torch.save(self.net.state_dict(), path)

    def evaluate(self, opponent="random", player: str = "policy", batch: int = 4096, games_per_lane: int = 2,
                 max_steps: int = 4000, opponent_player: str = "policy", top_k=None, margin=None, cube=False,
                 luck=False):
        """The current weights as player A of a head-to-head match (bgx.arena) against
        `opponent`: "random", a PolicyNet or the path of a saved state_dict (playing as
        `opponent_player`).  `player`: how A decides ("policy" sample, "greedy" argmax,
        "1ply", "2ply"; `top_k` / `margin`: the 2ply player's move filter, search.two_ply).
        `cube`: True plays money games with the doubling cube, each side by a
        default cube.CubeRule on its own weights' value head (a random opponent has no rule); an
        arena.ArenaCube is used as given.  The result is then arena.summarize_cube's.
        `luck`: True takes every roll's luck from the current weights' value head as a control
        variate; an arena.ArenaLuck is used as given.  The result is then
        arena.summarize_luck's.  Not together with `cube` (ValueError).
        Returns the arena's result dict.  Training is not disturbed: the
        match runs on an engine and seeds of its own (the k-th evaluation of a trainer is
        seeded from (seed, k)), the players pack the weights into buffers of their own, and
        neither the trainer's engines, step counter, packed weights or captured graphs nor
        torch's global generator are touched."""
        if self.group is not None or _world(self.group) > 1:
            raise NotImplementedError("PPOTrainer.evaluate runs on one rank only: multi-rank evaluation is not "
                                      "implemented (evaluate a saved checkpoint with python -m bgx.arena)")
        from . import arena as AR
        if luck and cube:
            raise ValueError("PPOTrainer.evaluate: luck together with cube is not implemented")
        self._evals_done += 1
        base = (self.seed * 1_000_003 + 15_485_863 * self._evals_done) & (2**63 - 1)
        if isinstance(opponent, str) and opponent != "random":
            opponent = AR.load_net(opponent, self.dev)
        a = AR.make_player(player, self.net, seed=base + 1, top_k=top_k, margin=margin)
        b = AR.make_player(opponent_player, opponent, seed=base + 2)
        ar = AR.Arena(batch, games_per_lane, seed=base, dice="philox", max_moves=self.A, device=self.dev)
        if cube is True:
            from .cube import CubeRule
            from .search import ValueHead
            cube = AR.ArenaCube(CubeRule(ValueHead(self.net)),
                                None if opponent is None or isinstance(opponent, str) else CubeRule(ValueHead(opponent)))
        if luck is True:
            from .search import ValueHead
            luck = AR.ArenaLuck(ValueHead(self.net))
        if luck:
            return ar.play(a, b, max_steps=max_steps, luck=luck)
        return ar.play(a, b, max_steps=max_steps, cube=cube or None)


def eval_metrics(ev: dict) -> dict:
    """An evaluation's entries of the metrics line.  With the cube (arena.summarize_cube's result)
    eval_win_rate and eval_ppg are those of the games played to the end, eval_games counts every
    game, and eval_ppg_cubeful and eval_pass_share are added.  With the luck adjustment
    (arena.summarize_luck's result) eval_ppg_luck, eval_ppg_luck_stderr and eval_variance_ratio are."""
    plain = ev.get("played_out", ev)
    m = {"eval_win_rate": plain["win_rate_a"], "eval_ppg": plain["ppg_a"], "eval_games": ev["games"],
         "eval_unfinished": ev["unfinished_lanes"]}
    if "played_out" in ev:
        m.update(eval_ppg_cubeful=ev["ppg_cubeful_a"], eval_pass_share=ev["pass_share"])
    if "ppg_luck_a" in ev:
        m.update(eval_ppg_luck=ev["ppg_luck_a"], eval_ppg_luck_stderr=ev["ppg_luck_stderr"],
                 eval_variance_ratio=ev["variance_ratio"])
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--metrics", default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--returns", default="lane", choices=list(RETURNS_MODES))
    ap.add_argument("--gae-lambda", type=float, default=0.95, help="GAE's lambda (--returns selfplay only)")
    ap.add_argument("--gamma", type=float, default=GAMMA, help="discount (--returns selfplay only)")
    ap.add_argument("--entropy-anneal", default="train", choices=["train", "train_single"])
    # periodic head-to-head evaluation of the current weights (PPOTrainer.evaluate, bgx.arena)
    ap.add_argument("--eval-every", type=int, default=0, help="evaluate after every N-th update (0: never)")
    ap.add_argument("--eval-games", type=int, default=2, help="games per lane of an evaluation")
    ap.add_argument("--eval-batch", type=int, default=4096)
    ap.add_argument("--eval-max-steps", type=int, default=4000)
    ap.add_argument("--eval-opponent", default="random", help="'random' or a saved state_dict")
    ap.add_argument("--eval-player", default="policy", choices=["policy", "greedy", "1ply", "2ply"])
    ap.add_argument("--eval-top-k", type=int, default=None,
                    help="--eval-player 2ply: search only the top-k 1-ply moves (the move filter)")
    ap.add_argument("--eval-margin", type=float, default=None,
                    help="--eval-player 2ply: ... within this 1-ply value of the best move")
    ap.add_argument("--eval-cube", action="store_true",
                    help="evaluate at money play with the doubling cube: adds eval_ppg_cubeful and eval_pass_share")
    ap.add_argument("--eval-luck", action="store_true",
                    help="luck-adjusted evaluation on the current weights' value head: adds eval_ppg_luck, "
                         "eval_ppg_luck_stderr and eval_variance_ratio")
    args = ap.parse_args()
    if args.eval_luck and args.eval_cube:
        ap.error("--eval-luck with --eval-cube is not implemented")
    if (args.eval_top_k is not None or args.eval_margin is not None) and args.eval_player != "2ply":
        ap.error("--eval-top-k / --eval-margin need --eval-player 2ply")
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if ws > 1 and args.eval_every > 0:
        ap.error("--eval-every needs a single rank (multi-rank evaluation is not implemented)")
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if ws > 1:
        backend = os.environ.get("BGX_DIST_BACKEND", "nccl")     # nccl == RCCL over xGMI
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    tr = PPOTrainer(batch=args.batch, horizon=args.horizon, hidden=args.hidden, seed=args.seed,
                    returns=args.returns, entropy_anneal=args.entropy_anneal, gae_lambda=args.gae_lambda,
                    gamma=args.gamma)
    for u in range(args.updates):
        m = tr.iteration()
        m["update"] = u
        if args.eval_every > 0 and (u + 1) % args.eval_every == 0:
            ev = tr.evaluate(args.eval_opponent, player=args.eval_player, batch=args.eval_batch,
                             games_per_lane=args.eval_games, max_steps=args.eval_max_steps,
                             top_k=args.eval_top_k, margin=args.eval_margin, cube=args.eval_cube,
                             **({"luck": True} if args.eval_luck else {}))
            m.update(eval_metrics(ev))
        if tr.rank == 0:
            print(json.dumps(m), flush=True)
            if args.metrics:
                with open(args.metrics, "a") as f:
                    f.write(json.dumps(m) + "\n")
    if args.save and tr.rank == 0:
        tr.save(args.save)
    if ws > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
