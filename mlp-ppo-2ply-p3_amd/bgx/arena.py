"""Head-to-head arena: two players, each with its own weights and decision rule, play
each other on the lanes of one engine until every lane has finished G games
(the device side is the arena kernels of csrc/bg_engine.hip and the
lane-selected searches of csrc/bg_search.hip).  The reference logs self-play statistics
only (train.py:55-99: both seats run the same weights); this answers "is this checkpoint
stronger than that one?".

    python -m bgx.arena --a new.pt --b old.pt --player-a 2ply --player-b 1ply \\
        --batch 4096 --games-per-lane 2 --max-steps 4000 --seed 0

Seat rule: in game g of lane i, A sits as PLAYER1 iff ((i + g) & 1) == 0, so with an even
batch A holds each seat in exactly half of all games.  A lane that has finished its G
games keeps stepping with action 0, belongs to neither player and is not counted: exactly
G games per lane keeps the estimate unbiased (a step budget would favour short games).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math

import torch

from . import _lib
from ._lib import check
from .engine import Engine, R_CUR, R_NM0, R_NM1, _ptr, _stream

# tally int64[16] (include/bgx.h bgx_arena_field); entries 14, 15 stay zero
FIELDS = ("games", "wins_a", "wins_b", "points_a", "points_b", "gammons_a", "gammons_b", "backgammons_a",
          "backgammons_b", "games_a_p1", "wins_a_p1", "wins_p1", "plies", "active_lanes")
ACTIVE = FIELDS.index("active_lanes")
TRACE_LIMIT = 1 << 22           # trace=True: batch x max_steps entries per traced field
SYNC_EVERY = 16                 # sync-free players: steps between host reads of the active-lane count


def summarize(tally, steps: int, unfinished: int) -> dict:
    """The arena result from the 16 tally entries: the fields by name, `steps`,
    `unfinished_lanes`, A's win rate with its binomial standard error and A's points per
    game (points_a - points_b) / games.  No games: the rates are 0."""
    t = [int(v) for v in tally]
    if len(t) < len(FIELDS):
        raise ValueError(f"summarize: the tally has {len(t)} entries, needs {len(FIELDS)}")
    r = dict(zip(FIELDS, t))
    g = r["games"]
    p = r["wins_a"] / g if g > 0 else 0.0
    r.update(steps=int(steps), unfinished_lanes=int(unfinished), win_rate_a=p,
             ppg_a=(r["points_a"] - r["points_b"]) / g if g > 0 else 0.0,
             win_rate_stderr=math.sqrt(max(p * (1.0 - p), 0.0) / g) if g > 0 else 0.0)
    return r


# ------------------------------------------------------------------ players --
# A player is any object with act(eng, sel, step) -> int32[B] on the engine's device; only
# the entries with sel != 0 are read.  `sync_free` (default False): act never waits for the
# device, so the arena reads its active-lane count only every SYNC_EVERY steps.

def _private_pack(net):
    """The net's weights packed for bgx_policy_act into a buffer of the player's own:
    net.pack() would replace the buffer the net itself (and a trainer's captured graphs)
    acts from."""
    prev = getattr(net, "_packed", None)
    try:
        return net.pack()
    finally:
        net._packed = prev


class PolicyPlayer:
    """The policy head: a sample of softmax(masked logits), or its argmax with greedy
    (bgx_policy_act on all lanes: the kernel works 32 rows per wave, so skipping single
    rows would save nothing)."""
    sync_free = True

    def __init__(self, net, greedy: bool = False, seed: int = 0):
        self.net, self.greedy, self.seed = net, bool(greedy), int(seed)
        self.packed = _private_pack(net)
        self.out = None

    def act(self, eng, sel, step):
        if eng.max_moves > self.net.action_head.out_features:
            raise ValueError(f"PolicyPlayer: the engine allows {eng.max_moves} moves, the net has "
                             f"{self.net.action_head.out_features} actions")
        if self.out is None or self.out[0].numel() != eng.batch or self.out[0].device != eng.device:
            self.out = (torch.empty(eng.batch, dtype=torch.int32, device=eng.device),
                        torch.empty(eng.batch, dtype=torch.float32, device=eng.device),
                        torch.empty(eng.batch, dtype=torch.float32, device=eng.device))
        return self.net.act(eng, seed=self.seed, step=step, greedy=self.greedy, packed=self.packed, out=self.out)[0]


class _SearchPlayer:
    def __init__(self, net):
        from .search import ValueHead
        self.vh = ValueHead(net)
        self.out = None

    def _out(self, eng):
        if self.out is None or self.out[0].numel() != eng.batch or self.out[0].device != eng.device:
            self.out = (torch.zeros(eng.batch, dtype=torch.int32, device=eng.device),
                        torch.zeros(eng.batch, dtype=torch.float32, device=eng.device), None)
        return self.out


class OnePlyPlayer(_SearchPlayer):
    """First argmax of V over the afterstates, on the lanes it is on move in only."""
    sync_free = True

    def act(self, eng, sel, step):
        from .search import one_ply
        return one_ply(eng, self.vh, sel=sel, out=self._out(eng))[0]


class TwoPlyPlayer(_SearchPlayer):
    """2-ply expectimax over the 21 rolls, on the lanes it is on move in only; `top_k` /
    `margin`: behind the 1-ply move filter (search.two_ply); `totals` sums the calls' work
    (leaves, jobs, searched afterstates, candidate afterstates)."""
    sync_free = False               # bgx_two_ply_sel sizes its workspace on the host

    def __init__(self, net, top_k=None, margin=None):
        super().__init__(net)
        self.top_k, self.margin = top_k, margin
        self.totals = {"calls": 0, "leaves": 0, "jobs": 0, "afterstates": 0, "candidates": 0}

    def act(self, eng, sel, step):
        from .search import two_ply
        best, _, _, stats = two_ply(eng, self.vh, sel=sel, out=self._out(eng), top_k=self.top_k, margin=self.margin)
        self.totals["calls"] += 1
        for k, v in stats.items():
            self.totals[k] += v
        if "candidates" not in stats:           # no filter: every candidate was searched
            self.totals["candidates"] += stats["afterstates"]
        return best


class RandomPlayer:
    """Uniform over the legal moves, drawn on the device from (seed, step, lane)
    (bgx_random_act)."""
    sync_free = True

    def __init__(self, seed: int = 0):
        self.seed = int(seed)
        self.out = None

    def act(self, eng, sel, step):
        if self.out is None or self.out.numel() != eng.batch or self.out.device != eng.device:
            self.out = torch.empty(eng.batch, dtype=torch.int32, device=eng.device)
        check(_lib.load().bgx_random_act(ctypes.c_void_p(eng.lanes_ptr()), eng.batch, self.seed & (2**64 - 1),
                                         int(step) & 0xFFFFFFFF, _ptr(self.out), _stream(eng.device)),
              "bgx_random_act")
        return self.out


# -------------------------------------------------------------------- arena --
class Arena:
    """`batch` lanes of an engine of its own (auto_reset, so a finished game's lane starts
    its next one in the same step), `games_per_lane` counted games each."""

    def __init__(self, batch: int, games_per_lane: int, seed: int = 0, dice: str = "philox", max_moves: int = 500,
                 device=None):
        if batch <= 0 or games_per_lane < 0:
            raise ValueError(f"Arena: batch {batch} must be positive and games_per_lane {games_per_lane} >= 0")
        self.B, self.G, self.seed = int(batch), int(games_per_lane), int(seed)
        self.eng = Engine(batch=self.B, max_moves=max_moves, seed=self.seed, dice=dice, auto_reset=True, device=device)
        if dice != "philox":
            import numpy as np
            self.eng.seed((np.arange(self.B, dtype=np.uint64) + self.seed) & 0xFFFFFFFF)
        dev = self.eng.device
        self.games_done = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.sel_a = torch.zeros(self.B, dtype=torch.uint8, device=dev)
        self.sel_b = torch.zeros(self.B, dtype=torch.uint8, device=dev)
        self.tally = torch.zeros(16, dtype=torch.int64, device=dev)
        self.actions = torch.zeros(self.B, dtype=torch.int32, device=dev)

    def _act(self, player, sel, step):
        a = player.act(self.eng, sel, step)
        if (not isinstance(a, torch.Tensor) or a.dtype != torch.int32 or a.device != self.eng.device
                or not a.is_contiguous() or a.numel() != self.B):
            raise ValueError("a player's act must return a contiguous int32[B] tensor on the engine's device")
        return a

    def play(self, a, b, max_steps: int, trace: bool = False):
        """begin; then [a.act, b.act, merge, step, advance] until no lane is active or
        `max_steps` env steps ran (weak greedy players can shuffle for thousands of steps:
        the result then reports `unfinished_lanes` instead of hanging).  Returns the
        result dict (summarize); with trace=True also a dict of per-step [steps, B]
        tensors: mover, n_moves, action, owner (0 none, 1 A, 2 B), done, info."""
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError(f"play: max_steps {max_steps} must be >= 0")
        if trace and self.B * max_steps > TRACE_LIMIT:
            raise ValueError(f"play: trace=True holds batch x max_steps = {self.B * max_steps} entries per field; "
                             f"the limit is {TRACE_LIMIT} (it is for tests and small batches)")
        L, eng, dev = _lib.load(), self.eng, self.eng.device
        recs = ctypes.c_void_p(eng.lanes_ptr())
        state = (_ptr(self.games_done), _ptr(self.sel_a), _ptr(self.sel_b), _ptr(self.tally))
        eng.reset(want_obs=False)
        check(L.bgx_arena_begin(recs, self.B, self.G, *state, _stream(dev)), "bgx_arena_begin")
        tr = None
        if trace:
            tr = {k: torch.zeros(max_steps, self.B, dtype=dt, device=dev)
                  for k, dt in (("mover", torch.uint8), ("n_moves", torch.int32), ("action", torch.int32),
                                ("owner", torch.uint8), ("done", torch.uint8), ("info", torch.int32))}
            rec = torch.empty(self.B, 64, dtype=torch.uint8, device=dev)
        every = SYNC_EVERY if getattr(a, "sync_free", False) and getattr(b, "sync_free", False) else 1
        steps = 0
        active = int(self.tally[ACTIVE].item())
        while active > 0 and steps < max_steps:
            act_a = self._act(a, self.sel_a, steps)
            act_b = self._act(b, self.sel_b, steps)
            check(L.bgx_arena_merge(_ptr(self.sel_a), _ptr(self.sel_b), _ptr(act_a), _ptr(act_b), self.B,
                                    _ptr(self.actions), _stream(dev)), "bgx_arena_merge")
            if trace:
                eng.records(out=rec)
                tr["mover"][steps] = rec[:, R_CUR]
                tr["n_moves"][steps] = rec[:, R_NM0].to(torch.int32) | (rec[:, R_NM1].to(torch.int32) << 8)
                tr["action"][steps] = self.actions
                tr["owner"][steps] = self.sel_a + 2 * self.sel_b
            _, _, done, info = eng.step(self.actions, want_obs=False, want_info=True)
            check(L.bgx_arena_advance(recs, _ptr(done), _ptr(info), self.B, self.G, *state, _stream(dev)),
                  "bgx_arena_advance")
            if trace:
                tr["done"][steps] = done
                tr["info"][steps] = info
            steps += 1
            if steps % every == 0 or steps == max_steps:
                active = int(self.tally[ACTIVE].item())
        tally = self.tally.cpu().tolist()
        res = summarize(tally, steps, tally[ACTIVE])
        if trace:
            return res, {k: v[:steps] for k, v in tr.items()}
        return res


# ------------------------------------------------------------- command line --
PLAYER_KINDS = ("policy", "greedy", "1ply", "2ply")


def load_net(path: str, device):
    """A PolicyNet from a state_dict file (PPOTrainer.save); its sizes come from the
    tensors.  Built without drawing from torch's global generator."""
    from .policy import PolicyNet
    sd = torch.load(path, map_location="cpu", weights_only=True)
    with torch.random.fork_rng(devices=[]):
        net = PolicyNet(input_size=sd["fc1.weight"].shape[1], hidden_size=sd["fc1.weight"].shape[0],
                        action_size=sd["action_head.weight"].shape[0])
    net.load_state_dict(sd)
    return net.to(device).eval()


def make_player(kind: str, net, seed: int = 0, top_k=None, margin=None):
    """`net` None or the string "random": the uniformly random player (kind ignored).
    `top_k` / `margin`: the 2ply player's move filter (TwoPlyPlayer), no other kind's."""
    if (top_k is not None or margin is not None) and (kind != "2ply" or net is None or net == "random"):
        raise ValueError("top_k / margin (the move filter) belong to a 2ply player")
    if net is None or (isinstance(net, str) and net == "random"):
        return RandomPlayer(seed)
    if kind == "policy":
        return PolicyPlayer(net, greedy=False, seed=seed)
    if kind == "greedy":
        return PolicyPlayer(net, greedy=True, seed=seed)
    if kind == "1ply":
        return OnePlyPlayer(net)
    if kind == "2ply":
        return TwoPlyPlayer(net, top_k=top_k, margin=margin)
    raise ValueError(f"player kind must be one of {PLAYER_KINDS}, got {kind!r}")


class _Parser(argparse.ArgumentParser):
    """The move-filter options are an error for any player but a 2ply one with weights."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        for side in "ab":
            top_k, margin = getattr(ns, f"top_k_{side}"), getattr(ns, f"margin_{side}")
            if top_k is None and margin is None:
                continue
            if getattr(ns, f"player_{side}") != "2ply" or getattr(ns, side) == "random":
                self.error(f"--top-k-{side} / --margin-{side} need --player-{side} 2ply with weights")
            if top_k is not None and top_k < 1:
                self.error(f"--top-k-{side} must be >= 1")
            if margin is not None and not margin >= 0:
                self.error(f"--margin-{side} must be >= 0")
        for side in "ab":
            k = getattr(ns, f"bearoff_{side}")
            if k is not None and not 1 <= k <= 8:
                self.error(f"--bearoff-{side} takes a number of checkers in 1..8")
            k = getattr(ns, f"bearoff1_{side}")
            if k is not None and not 1 <= k <= 15:
                self.error(f"--bearoff1-{side} takes a number of checkers in 1..15")
        return ns


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(prog="python -m bgx.arena", description="Play two players against each other.")
    ap.add_argument("--a", required=True, help="player A: a state_dict file (PPOTrainer.save) or 'random'")
    ap.add_argument("--b", required=True, help="player B: a state_dict file or 'random'")
    ap.add_argument("--player-a", default="policy", choices=PLAYER_KINDS)
    ap.add_argument("--player-b", default="policy", choices=PLAYER_KINDS)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--games-per-lane", type=int, default=2)
    ap.add_argument("--max-steps", type=int, required=True,
                    help="env steps after which the match stops (unfinished lanes are reported)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dice", default="philox", choices=["philox", "mt", "shared"])
    for side in "ab":
        ap.add_argument(f"--top-k-{side}", type=int, default=None,
                        help=f"player {side.upper()} (2ply only): search only its top-k 1-ply moves")
        ap.add_argument(f"--margin-{side}", type=float, default=None,
                        help=f"player {side.upper()} (2ply only): ... within this 1-ply value of its best move")
        ap.add_argument(f"--bearoff-{side}", type=int, default=None, metavar="K",
                        help=f"player {side.upper()} moves perfectly where the position is in the exact bearoff "
                             "table for K checkers a side (1..8; bgx/bearoff.py)")
        ap.add_argument(f"--bearoff1-{side}", type=int, default=None, metavar="K",
                        help=f"player {side.upper()} moves by the one-sided bearoff table for K checkers a side "
                             f"(1..15) in every pure home-board race; inside --bearoff-{side}'s table that one plays")
    return ap


def main(argv=None):
    import time
    args = build_parser().parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    nets = [None if p == "random" else load_net(p, dev) for p in (args.a, args.b)]
    max_moves = min([n.action_head.out_features for n in nets if n is not None] + [500])
    players = [make_player(k, n, seed=args.seed * 2 + 1 + i, top_k=tk, margin=mg)
               for i, (k, n, tk, mg) in enumerate(zip((args.player_a, args.player_b), nets,
                                                      (args.top_k_a, args.top_k_b), (args.margin_a, args.margin_b)))]
    if args.bearoff1_a is not None or args.bearoff1_b is not None:
        from .bearoff import OneSidedBearoffDB, OneSidedPlayer
        dbs1 = {k: OneSidedBearoffDB(k, device=dev) for k in {args.bearoff1_a, args.bearoff1_b} - {None}}
        players = [p if k is None else OneSidedPlayer(p, dbs1[k])
                   for p, k in zip(players, (args.bearoff1_a, args.bearoff1_b))]
    if args.bearoff_a is not None or args.bearoff_b is not None:
        from .bearoff import BearoffDB, BearoffPlayer
        dbs = {k: BearoffDB(k, device=dev) for k in {args.bearoff_a, args.bearoff_b} - {None}}
        players = [p if k is None else BearoffPlayer(p, dbs[k])
                   for p, k in zip(players, (args.bearoff_a, args.bearoff_b))]
    arena =Arena(args.batch, args.games_per_lane, seed=args.seed, dice=args.dice, max_moves=max_moves, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = arena.play(players[0], players[1], max_steps=args.max_steps)
    dt = time.perf_counter() - t0
    res.update(a=args.a, b=args.b, player_a="random" if nets[0] is None else args.player_a,
               player_b="random" if nets[1] is None else args.player_b, batch=args.batch,
               games_per_lane=args.games_per_lane, max_steps=args.max_steps, seed=args.seed, seconds=dt,
               top_k_a=args.top_k_a, top_k_b=args.top_k_b, margin_a=args.margin_a, margin_b=args.margin_b,
               bearoff_a=args.bearoff_a, bearoff_b=args.bearoff_b,
               **{k: v for k, v in (("bearoff1_a", args.bearoff1_a), ("bearoff1_b", args.bearoff1_b)) if v is not None},
               games_per_s=res["games"] / dt if dt > 0 else 0.0,
               env_steps_per_s=res["steps"] * args.batch / dt if dt > 0 else 0.0)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
