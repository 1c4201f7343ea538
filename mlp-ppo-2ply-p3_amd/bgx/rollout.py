"""Position rollouts: play a position to the end many times with a given player and
average the results (DESIGN.md "Start positions and rollouts"; the device side is the
engine's start table, bgx_engine_set_starts, and the rollout kernels of
csrc/bg_engine.hip).  It answers "what is this position worth?" and, through
rollout_moves, "which of these moves is best when the game is played out?".

    python -m bgx.rollout --net ckpt.pt --player 1ply --positions pos.json --trials 1296 \\
        --batch 4096 --max-steps 4000 --seed 0

Every lane holds one position as its start record: the engine's auto-reset refills the lane
with it in the step that ends a game, so no lane waits for the longest game of a wave.  One
player acts for both sides.  Equity is in points (1 / 2 / 3 per game, cubeless) from the
side of the position's mover.  --luck: the luck-adjusted (variance-reduced) estimate beside the
raw one (summarize_luck; DESIGN.md "Luck adjustment").  --bearoff K: a game that reaches the exact
bearoff table (bgx/bearoff.py) stops there and is scored with its exact win probability
(summarize_bearoff).  --bearoff1 K: the same cut at the one-sided table, which
reaches every pure home-board race but whose win probability is an approximation (DESIGN.md
§12): the `equity_stderr` of cut games then no longer measures the error against the truth.
--cube: money play with the doubling cube (bgx/cube.py): before its roll the side
on roll may double by a threshold rule on a net's value, a passed double ends the game, and the
result is the cubeful equity (cube.summarize_cube); --cube-decision answers "double or not,
take or pass?" per position; --cube-bearoff K cuts the cubeful games at the cubeful exact bearoff
table (bearoff.CubefulBearoffDB), where both the endgame's dice and its cube
action are replaced by the exact cubeful expectation; --cube-truncate N stops the cubeful games
after N plies and scores them with Janowski's cube-life equity from a net's value,
which is what makes --cube-decision affordable with the slow players; --cube-luck: the luck-adjusted
cubeful estimate beside the raw one (cube.summarize_cube_luck), the luck of a roll being
Janowski's equity after it minus its mean over the 21 rolls, times the cube.  --truncate N: a game that
has run N plies stops there and is scored by a net's value head (bgx/truncate.py),
which makes the slow players affordable; with --luck the dice noise of the plies played goes too (summarize_truncated_luck).  The
estimate then carries the net's own error, which no standard error shows.
--match N --match-score A1,A2: the position at a score of a match to N points (bgx/match.py):
single games with cube decisions by one match rule for both sides, the result the mover's match-winning
chance on a match equity table (match.summarize_match_rollout); --match-decision answers "double or not,
take or pass?" per position in that chance.  It goes with no other mode.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .arena import PLAYER_KINDS, SYNC_EVERY, TRACE_LIMIT, _stream, load_net, make_player
from .engine import Engine, R_CUR, R_ROLL0, R_ROLL1, _ptr, validate_starts
from .replay import LaneReplay
from .tally import (CUBE_CUT_FIELDS, CUBE_FIELDS, CUBE_LUCK_FIELDS, CUBE_TRUNC_FIELDS, CUT_FIELDS, CUT_ONE,  # noqa: F401
                    FIELDS, LUCK_CLAMP, LUCK_FIELDS, LUCK_ONE, TRUNC_FIELDS, summarize, summarize_bearoff,
                    summarize_cube, summarize_cube_bearoff, summarize_cube_luck, summarize_cube_truncated,
                    summarize_luck, summarize_truncated, summarize_truncated_luck)
from .truncate import Truncation, truncate_reference  # noqa: F401

ROLLS36 = [(a, b) for a in range(1, 7) for b in range(1, 7)]       # the 36 ordered rolls
FIRST_ROLLS = ("stratified", "random")


def luck_tally_reference(luck, mover, done, info, starts, group, n_groups: int, games_per_lane: int) -> np.ndarray:
    """The luck tally int64[n_groups, 4] of a traced run on the host, with the arithmetic of
    bgx_rollout_luck_add / bgx_rollout_luck_flush (include/bgx.h): per lane the fp32 sum in
    step order of +-luck, left out in a game's first step when the start record fixed the
    roll; at a counted game's end Lq = rint(fp32(sum * 65536)) (round half even) clamped to
    +-2^21, 0 when not finite.  `luck`, `mover`, `done`, `info`: [steps, B] as run_lanes
    traces them; `starts` uint8[B, 64]; `group` int32[B].  A lane is active while its group is
    in [0, n_groups) and it has finished fewer than `games_per_lane` games."""
    luck, mover = np.asarray(luck, np.float32), np.asarray(mover)
    rp = LaneReplay(starts, group, n_groups, games_per_lane)
    rp.tally("luck_tally", LUCK_FIELDS)
    for t in range(luck.shape[0]):
        rp.luck_add(luck[t], mover[t])
        rp.advance(done[t], info[t])
    return rp.tallies["luck_tally"]


def bearoff_cut_reference(records0, records, done, info, starts, group, n_groups: int, games_per_lane: int,
                          configs=None, table=None, max_checkers: int = 0, lookup=None) -> dict:
    """A traced run with the bearoff cut replayed on the host, with the arithmetic of
    bgx_rollout_begin / bgx_rollout_advance / bgx_rollout_bearoff_cut (include/bgx.h): a
    selected lane whose record is in the table (bearoff.lookup_reference) adds
    Pq = rint(fp32(q * 2^20)) clamped to [0, 2^20], q = W for the start mover on roll, else
    fp32(1 - W), counts the game and is masked for the reset.  `records0` uint8[B, 64] = the
    records the cut after begin saw, `records` uint8[steps, B, 64] those after each step (before
    the masked reset), `done` / `info` [steps, B] as run_lanes traces them, `configs` / `table`
    as BearoffDB publishes them.  `lookup` (optional): another table's test and value instead,
    a function records uint8[B, 64] -> (cut bool[B], w f32[B]); for the one-sided table, the
    lanes with bearoff.lookup1_reference's in_db == 1 and its win; configs, table and
    max_checkers are then not read.  Returns dict(tally int64[P, 8], cut_tally int64[P, 4],
    games_done int64[B], active int, cut0 bool[B], cut bool[steps, B])."""
    if lookup is None:
        from .bearoff import lookup_reference

        def lookup(recs):
            return lookup_reference(recs, configs, table, max_checkers)
    records0, records, done = np.asarray(records0), np.asarray(records), np.asarray(done)
    rp = LaneReplay(starts, group, n_groups, games_per_lane)
    rp.tally("cut_tally", CUT_FIELDS)

    def cut(recs):
        in_db, w = lookup(recs)
        m = rp.sel & in_db
        w = np.where(m, w, np.float32(0)).astype(np.float32)
        q = np.where(recs[:, R_CUR] == rp.start_cur, w, (np.float32(1) - w).astype(np.float32))
        pq = np.clip(np.rint((q * np.float32(CUT_ONE)).astype(np.float32)).astype(np.int64), 0, CUT_ONE)
        rp.cut("cut_tally", m, (pq, pq * pq))
        return m

    cut0 = cut(records0)
    cuts = np.zeros(done.shape, bool)
    for t in range(done.shape[0]):
        rp.advance(done[t], info[t])
        cuts[t] = cut(records[t])
    return dict(rp.tallies, games_done=rp.games, active=rp.active, cut0=cut0, cut=cuts)


def layout(n_positions: int, trials: int, first_roll: str = "stratified", batch: int = 4096):
    """How `trials` games of each of `n_positions` positions go onto `batch` lanes.  Returns
    (group int32[passes, batch], roll_of_lane uint8[passes, batch, 2], games_per_lane, passes):
    lane -> position (-1 = idle) and the lane's start roll, per pass.

    A unit is one position ("random": roll bytes (0, 0), drawn at every reset) or one
    (position, ordered roll) pair ("stratified": `trials` is rounded up to a multiple of 36
    and each of the 36 rolls gets trials / 36 games with that first roll).  Every unit gets
    the same number of lanes, side by side, and every lane the same number of games.  More
    games than lanes: several games per lane first; more units than lanes: several passes.
    A unit's games (lanes x games_per_lane) can exceed its share by less than one game per
    lane when the share does not divide; the tallies report what was played."""
    if first_roll not in FIRST_ROLLS:
        raise ValueError(f"first_roll must be one of {FIRST_ROLLS}, got {first_roll!r}")
    if n_positions <= 0 or trials <= 0 or batch <= 0:
        raise ValueError(f"layout: n_positions {n_positions}, trials {trials} and batch {batch} must be positive")
    strat = first_roll == "stratified"
    per_pos = 36 if strat else 1
    share = -(-trials // 36) if strat else trials              # games per unit
    units = n_positions * per_pos
    per_pass = min(units, batch)
    passes = -(-units // per_pass)
    lanes = min(share, batch // per_pass)                        # lanes per unit
    games = -(-share // lanes)
    lanes = -(-share // games)
    group = np.full((passes, batch), -1, np.int32)
    roll = np.zeros((passes, batch, 2), np.uint8)
    for k in range(passes):
        u = np.arange(k * per_pass, min((k + 1) * per_pass, units))
        lane_unit = np.repeat(u, lanes)
        group[k, :lane_unit.size] = lane_unit // per_pos
        if strat:
            roll[k, :lane_unit.size] = np.asarray(ROLLS36, np.uint8)[lane_unit % 36]
    return group, roll, games, passes


def _records(positions) -> torch.Tensor:
    p = torch.as_tensor(positions)
    if p.dim() == 1:
        p = p[None]
    if p.dim() != 2 or p.shape[1] != 64 or p.dtype != torch.uint8 or p.shape[0] == 0:
        raise ValueError(f"positions must be uint8 [P, 64] lane records, got {p.dtype} {tuple(p.shape)}")
    p = p.cpu().clone()
    p[:, R_ROLL0:] = 0
    validate_starts(p)
    return p


def _check_modes(where: str, luck=None, bearoff=None, cube=None, truncate=None, cube_bearoff=None, cube0=None,
                 types: bool = False, cube_truncate=None, match=None, cube_luck=None) -> None:
    """The combinations of modes that Rollout.run and run_lanes refuse, as ValueError(f"{where}: ...")
    for the first one that applies.  `types` (run_lanes): also what only the lanes can tell --
    a cube_bearoff that is no cubeful table, a truncate that is no Truncation, a cube_truncate that
    is no CubeTruncation, a cube_luck that is no CubeLuck, cube0 without cube -- each at its place in
    the order.  `match` goes with no other mode and is asked first.  Nothing here
    touches the engine or the library."""
    if match is not None:
        for name, other in (("luck", luck), ("bearoff", bearoff), ("cube", cube), ("truncate", truncate),
                            ("cube_bearoff", cube_bearoff), ("cube_truncate", cube_truncate), ("cube_luck", cube_luck)):
            if other is not None:
                raise ValueError(f"{where}: match together with {name} is not supported")
        if types:
            from .match import RolloutMatch
            if not isinstance(match, RolloutMatch):
                raise ValueError(f"{where}: match must be a match.RolloutMatch")
    if cube_luck is not None:
        if cube is None:
            raise ValueError(f"{where}: cube_luck without cube")
        for name, other in (("luck", luck), ("bearoff", bearoff), ("truncate", truncate), ("cube_bearoff", cube_bearoff),
                            ("cube_truncate", cube_truncate)):
            if other is not None:
                raise ValueError(f"{where}: cube_luck together with {name} is not supported")
        if types:
            from .cube import CubeLuck
            if not isinstance(cube_luck, CubeLuck):
                raise ValueError(f"{where}: cube_luck must be a cube.CubeLuck")
    if cube_truncate is not None:
        if cube is None:
            raise ValueError(f"{where}: cube_truncate without cube")
        for name, other in (("luck", luck), ("bearoff", bearoff), ("truncate", truncate)):
            if other is not None:
                raise ValueError(f"{where}: cube_truncate together with {name} is not supported")
        if types:
            from .cube import CubeTruncation
            if not isinstance(cube_truncate, CubeTruncation):
                raise ValueError(f"{where}: cube_truncate must be a cube.CubeTruncation")
    if cube_bearoff is not None:
        if cube is None:
            raise ValueError(f"{where}: cube_bearoff without cube")
        for name, other in (("luck", luck), ("bearoff", bearoff), ("truncate", truncate)):
            if other is not None:
                raise ValueError(f"{where}: cube_bearoff together with {name} is not supported")
        if types and getattr(cube_bearoff, "kind", None) != "cubeful":
            raise ValueError(f"{where}: cube_bearoff must be a bearoff.CubefulBearoffDB")
    if truncate is not None and (bearoff is not None or cube is not None):
        raise ValueError(f"{where}: truncate together with {'bearoff' if bearoff is not None else 'cube'} "
                         "is not supported")
    if types and truncate is not None and not isinstance(truncate, Truncation):
        raise ValueError(f"{where}: truncate must be a truncate.Truncation")
    for a, b, x, y in (("bearoff", "luck", bearoff, luck), ("cube", "luck", cube, luck), ("cube", "bearoff", cube, bearoff)):
        if x is not None and y is not None:
            raise ValueError(f"{where}: {a} together with {b} is not supported")
    if types and cube is None and match is None and cube0 is not None:
        raise ValueError(f"{where}: cube0 without cube")


class _Pass:
    """What one run_lanes pass shares with its stages: the library, the engine and its lane
    records, the device copies of starts and group, the sizes, the rollout's own per-lane state
    (`lanes` = games_done, plies, sel as pointers; `active`), and with trace=True the trace
    dicts (`tr` of [max_steps, B] tensors, `tr_end`) and `rec`, a scratch copy of the lane records."""

    def __init__(self, ro, starts, grp, P: int, G: int, max_steps: int, trace: bool):
        self.ro, self.L, self.eng, self.dev = ro, _lib.load(), ro.eng, ro.eng.device
        self.B, self.P, self.G, self.max_steps = ro.B, P, G, max_steps
        self.recs, self.stream = ctypes.c_void_p(ro.eng.lanes_ptr()), _stream(ro.eng.device)
        self.starts, self.grp = starts, grp
        self.lanes, self.active = (_ptr(ro.games_done), _ptr(ro.plies), _ptr(ro.sel)), _ptr(ro.active)
        self.tr, self.tr_end = ({}, {}) if trace else (None, None)      # per step; added once at the end
        self.rec = torch.empty(self.B, 64, dtype=torch.uint8, device=self.dev) if trace else None

    def lane_buffers(self, n: int, dtype, fill=0):
        return [torch.full((self.B,), fill, dtype=dtype, device=self.dev) for _ in range(n)]

    def tally(self, fields):
        return torch.zeros(self.P, len(fields), dtype=torch.int64, device=self.dev)

    def traced(self, *fields):
        """Per-step trace tensors [max_steps, B, ...] for (name, dtype, trailing shape...) fields."""
        if self.tr is not None:
            for name, dtype, *shape in fields:
                self.tr[name] = torch.zeros(self.max_steps, self.B, *shape, dtype=dtype, device=self.dev)

    def reset(self, mask):      # the masked bgx_reset: every masked lane gets its start record again
        self.eng.reset(lane_mask=mask, want_obs=False)


class _Stage:
    """A mode of run_lanes: it owns its buffers, its `tally` (one more result after the trace)
    and its trace fields, and hooks into the step loop where it needs to.  `sync_free`: the
    stage never waits for the device, so the host may read the active-lane count rarely."""
    sync_free = False
    # the hooks, empty unless a stage defines them: after_begin(), before_act(step),
    # after_step(done, info), after_advance(step)
    after_begin = before_act = after_step = after_advance = staticmethod(lambda *args: None)


class _LuckStage(_Stage):
    """`luck` (a search.ValueHead; DESIGN.md "Luck adjustment"): every step first takes the luck
    of the active lanes' rolls under that value head and adds it to their games (before act:
    roll_luck on sel, luck_add; after the step: luck_flush; the host reads the active-lane
    count every step, as roll_luck synchronises anyway).  The games are the same as without it.
    Result: luck_tally int64[n_groups, 4] (LUCK_FIELDS); the trace gains the per-step luck
    f32[steps, B] (NaN on lanes that never were active)."""

    def __init__(self, c: _Pass, head):
        self.c, self.head = c, head
        self.tally = c.tally(LUCK_FIELDS)
        self.buf, = c.lane_buffers(1, torch.float32, float("nan"))
        c.ro.lane_luck.zero_()
        c.traced(("luck", torch.float32))

    def before_act(self, step):
        from .search import roll_luck
        c = self.c
        roll_luck(c.eng, self.head, sel=c.ro.sel, out=(self.buf, None))
        check(c.L.bgx_rollout_luck_add(c.recs, _ptr(c.starts), c.lanes[1], c.lanes[2], _ptr(self.buf), c.B,
                                       _ptr(c.ro.lane_luck), c.stream), "bgx_rollout_luck_add")
        if c.tr is not None:
            c.tr["luck"][step] = self.buf

    def after_step(self, done, info):
        c = self.c
        check(c.L.bgx_rollout_luck_flush(_ptr(c.starts), _ptr(c.grp), c.lanes[2], _ptr(done), _ptr(info), c.B, c.P,
                                         _ptr(c.ro.lane_luck), _ptr(self.tally), c.stream), "bgx_rollout_luck_flush")


class _CubeStage(_Stage):
    """`cube` (a cube.CubeRule): money play with the doubling cube.  `cube0`
    uint8[B] = the cube every game on the lane starts with (cube.pack(k, owner); None: centred
    at 1 everywhere; ValueError names the first lane with an invalid byte).  After begin:
    cube_begin; before act: cube_sel, equity, cube_decide, reset(mask); after the step:
    cube_flush.  Before its roll, but never on a game's first ply, the side on roll may double by
    the rule on its equity (the rule's value head or callable); a passed double ends the game at
    the cube's value and the masked reset gives the lane its start record again.  The host reads
    the active-lane count every step, as the equity synchronises.  Result: cube_tally
    int64[n_groups, 8] (cube.CUBE_FIELDS); the trace gains per step cube uint8 (the state before
    the decision), cube_mover (the side on roll there), cube_dsel (the lanes that may double),
    cube_equity (NaN off cube_dsel) and cube_mask (the passes).  `luck`: the _CubeLuckStage that
    accompanies it, if any, called before the decision, after the masked reset and before cube_flush."""

    def __init__(self, c: _Pass, rule, cube0):
        from .cube import validate_cube0
        self.c, self.rule, self.luck = c, rule, None
        self.c0 = (torch.zeros(c.B, dtype=torch.uint8, device=c.dev) if cube0 is None
                   else torch.as_tensor(cube0).to(c.dev).contiguous())
        if self.c0.shape != (c.B,) or self.c0.dtype != torch.uint8:
            raise ValueError(f"run_lanes: cube0 must be uint8[{c.B}]")
        validate_cube0(self.c0, rule.cap)
        self.struct = rule.struct()
        self.tally = c.tally(CUBE_FIELDS)
        self.state, self.dsel, self.mask = c.lane_buffers(3, torch.uint8)
        self.ebuf, self.escratch = c.lane_buffers(2, torch.float32, float("nan"))
        c.traced(("cube", torch.uint8), ("cube_mover", torch.uint8), ("cube_dsel", torch.uint8),
                 ("cube_equity", torch.float32), ("cube_mask", torch.uint8))

    def after_begin(self):
        c = self.c
        check(c.L.bgx_rollout_cube_begin(_ptr(self.c0), c.B, self.rule.cap, _ptr(self.state), c.stream),
              "bgx_rollout_cube_begin")

    def before_act(self, step):
        c, tr = self.c, self.c.tr
        check(c.L.bgx_rollout_cube_sel(c.recs, _ptr(c.grp), c.P, c.lanes[1], c.lanes[2], _ptr(self.state), c.B,
                                       self.rule.cap, _ptr(self.dsel), c.stream), "bgx_rollout_cube_sel")
        eq = self.rule.equity(c.eng, self.dsel, self.escratch, self.ebuf)
        if tr is not None:
            c.eng.records(out=c.rec)
            tr["cube"][step] = self.state
            tr["cube_mover"][step] = c.rec[:, R_CUR]
            tr["cube_dsel"][step] = self.dsel
            tr["cube_equity"][step] = torch.where(self.dsel != 0, eq, float("nan"))
        if self.luck is not None:
            self.luck.before_decide(eq)
        check(c.L.bgx_rollout_cube_decide(c.recs, _ptr(c.starts), _ptr(c.grp), _ptr(self.dsel), _ptr(eq), c.B, c.P,
                                          c.G, self.struct, _ptr(self.c0), _ptr(self.state), *c.lanes,
                                          _ptr(self.tally), c.active, _ptr(self.mask), c.stream),
              "bgx_rollout_cube_decide")
        if tr is not None:
            tr["cube_mask"][step] = self.mask
        c.reset(self.mask)
        if self.luck is not None:
            self.luck.after_decide(step)

    def after_step(self, done, info):
        c = self.c
        if self.luck is not None:
            self.luck.flush(done, info)
        check(c.L.bgx_rollout_cube_flush(_ptr(c.starts), _ptr(c.grp), c.lanes[2], _ptr(done), _ptr(info), c.B, c.P,
                                         self.struct, _ptr(self.c0), _ptr(self.state), _ptr(self.tally), c.stream),
              "bgx_rollout_cube_flush")


class _MatchStage(_Stage):
    """`match` (a match.RolloutMatch): single games at a fixed match score,
    `match_score` = (away [n_groups, 2], craw [n_groups]) the groups' score and `cube0` uint8[B]
    the cube every game on the lane starts with (cap 10; None: centred at 1).  After begin:
    cube_begin; before act: match_sel, the rule's equity on dsel, match_decide, reset(mask); after
    the step: match_flush.  One rule serves both sides: the side on roll doubles by it, the other
    answers on the same value.  A passed double ends the game and the masked reset gives the lane
    its start record again.  Sync-free when the rule's value is.  Result: match_hist
    int64[n_groups, 96] (match.MATCH_HIST_FIELDS after the 88 bins); the trace gains per step
    match_cube uint8 (the state before the decision), match_mover (the side on roll there),
    match_dsel (the lanes that may double), match_value (NaN off match_dsel) and match_action (0
    none, 1 take, 2 pass)."""

    def __init__(self, c: _Pass, match, score, cube0):
        from .cube import MAX_CAP, validate_cube0
        from .match import MATCH_HIST_ROW, validate_score
        self.c, self.match, self.rule, self.sync_free = c, match, match.rule, match.sync_free
        self.c0 = (torch.zeros(c.B, dtype=torch.uint8, device=c.dev) if cube0 is None
                   else torch.as_tensor(cube0).to(c.dev).contiguous())
        if self.c0.shape != (c.B,) or self.c0.dtype != torch.uint8:
            raise ValueError(f"run_lanes: cube0 must be uint8[{c.B}]")
        validate_cube0(self.c0, MAX_CAP)
        if not isinstance(score, (tuple, list)) or len(score) != 2:
            raise ValueError("run_lanes: match needs match_score = (away [n_groups, 2], craw [n_groups])")
        away, craw = (np.asarray(torch.as_tensor(v).cpu()) for v in score)
        if away.shape != (c.P, 2) or craw.shape != (c.P,):
            raise ValueError(f"run_lanes: match_score must be (away [{c.P}, 2], craw [{c.P}])")
        for a, k in zip(away.tolist(), craw.tolist()):
            validate_score(match.length, a, k)
        self.away = torch.from_numpy(away.astype(np.uint8)).to(c.dev).contiguous()
        self.craw = torch.from_numpy(craw.astype(np.uint8)).to(c.dev).contiguous()
        self.cap, self.struct = MAX_CAP, match.rule.struct()
        self.met, self.pc = match.tables(c.dev)
        self.tally = torch.zeros(c.P, MATCH_HIST_ROW, dtype=torch.int64, device=c.dev)
        self.state, self.dsel, self.mask, self.before = c.lane_buffers(4, torch.uint8)
        self.ebuf, self.escratch = c.lane_buffers(2, torch.float32, float("nan"))
        c.traced(("match_cube", torch.uint8), ("match_mover", torch.uint8), ("match_dsel", torch.uint8),
                 ("match_value", torch.float32), ("match_action", torch.uint8))

    def after_begin(self):
        c = self.c
        check(c.L.bgx_rollout_cube_begin(_ptr(self.c0), c.B, self.cap, _ptr(self.state), c.stream),
              "bgx_rollout_cube_begin")

    def before_act(self, step):
        c, tr = self.c, self.c.tr
        check(c.L.bgx_rollout_match_sel(c.recs, _ptr(c.grp), c.P, c.lanes[1], c.lanes[2], _ptr(self.state),
                                        _ptr(self.away), _ptr(self.craw), c.B, _ptr(self.dsel), c.stream),
              "bgx_rollout_match_sel")
        v = self.rule.equity(c.eng, self.dsel, self.escratch, self.ebuf)
        if tr is not None:
            c.eng.records(out=c.rec)
            self.before.copy_(self.state)
            tr["match_cube"][step] = self.state
            tr["match_mover"][step] = c.rec[:, R_CUR]
            tr["match_dsel"][step] = self.dsel
            tr["match_value"][step] = torch.where(self.dsel != 0, v, float("nan"))
        check(c.L.bgx_rollout_match_decide(c.recs, _ptr(c.starts), _ptr(c.grp), _ptr(self.dsel), _ptr(v), c.B, c.P, c.G,
                                           self.struct, _ptr(self.met), _ptr(self.pc), self.match.length,
                                           _ptr(self.away), _ptr(self.craw), _ptr(self.c0), _ptr(self.state), *c.lanes,
                                           _ptr(self.tally), c.active, _ptr(self.mask), c.stream),
              "bgx_rollout_match_decide")
        if tr is not None:
            # a take is the one decision that raises the cube's k; a pass is the mask
            took = ((self.state & 15) > (self.before & 15)) & (self.mask == 0)
            tr["match_action"][step] = torch.where(self.mask != 0, 2, took.to(torch.uint8)).to(torch.uint8)
        c.reset(self.mask)

    def after_step(self, done, info):
        c = self.c
        check(c.L.bgx_rollout_match_flush(_ptr(c.starts), _ptr(c.grp), c.lanes[2], _ptr(done), _ptr(info), c.B, c.P,
                                          _ptr(self.c0), _ptr(self.state), _ptr(self.tally), c.stream),
              "bgx_rollout_match_flush")


class _CubeLuckStage(_Stage):
    """`cube_luck` (a cube.CubeLuck), with `cube`: the luck of every roll of a cubeful
    game, in points, summed per game and booked against the game's cubeful result.  It has no
    hooks of its own in the loop: the cube stage calls it where the order needs it -- before
    cube_decide: cube_luck_pass (a passed game's luck is booked while its cube still stands); after
    the masked reset: roll_values on sel, cube_roll_luck, cube_luck_add (the cube after the
    decision scales the roll's luck); after the step, before cube_flush: cube_luck_flush.  The
    games are the same as without it.  Result (after cube_tally): cube_luck_tally int64[n_groups, 5]
    (CUBE_LUCK_FIELDS); the trace gains per step cube_luck f32 (in units of the lane's cube, NaN on
    lanes that never were active), cube_luck_state uint8 (the cube after the decision),
    cube_luck_mover (the side on roll there), cube_luck_roll uint8[.., 2] (its roll) and
    cube_luck_values f32[.., 21] (roll_values' rows, NaN on lanes that never were active)."""

    def __init__(self, c: _Pass, cl, cube: _CubeStage):
        self.c, self.cl, self.cube = c, cl, cube
        self.life = cl.life.struct()
        self.tally = c.tally(CUBE_LUCK_FIELDS)
        self.buf, = c.lane_buffers(1, torch.float32, float("nan"))
        self.values = torch.full((c.B, 21), float("nan"), dtype=torch.float32, device=c.dev)
        c.ro.lane_luck.zero_()
        c.traced(("cube_luck", torch.float32), ("cube_luck_state", torch.uint8), ("cube_luck_mover", torch.uint8),
                 ("cube_luck_roll", torch.uint8, 2), ("cube_luck_values", torch.float32, 21))
        cube.luck = self

    def before_decide(self, eq):
        c, cube = self.c, self.cube
        check(c.L.bgx_rollout_cube_luck_pass(c.recs, _ptr(c.starts), _ptr(c.grp), _ptr(cube.dsel), _ptr(eq), c.B, c.P,
                                             cube.struct, _ptr(cube.state), _ptr(c.ro.lane_luck), _ptr(self.tally),
                                             c.stream), "bgx_rollout_cube_luck_pass")

    def after_decide(self, step):
        from .search import roll_values
        c, cube, rule = self.c, self.cube, self.cube.rule
        stats = roll_values(c.eng, self.cl.value, sel=c.ro.sel, out=self.values)[1]
        self.cl.totals["calls"] += 1
        self.cl.totals["rows"] += stats["rows"]
        self.cl.totals["leaves"] += stats["leaves"]
        check(c.L.bgx_cube_roll_luck(c.recs, _ptr(cube.state), _ptr(self.values), c.B, self.cl.scale, self.life,
                                     rule.cap, int(rule.jacoby), c.lanes[2], _ptr(self.buf), None, c.stream),
              "bgx_cube_roll_luck")
        check(c.L.bgx_rollout_cube_luck_add(c.recs, _ptr(c.starts), c.lanes[1], c.lanes[2], _ptr(cube.state),
                                            _ptr(self.buf), c.B, rule.cap, _ptr(c.ro.lane_luck), c.stream),
              "bgx_rollout_cube_luck_add")
        if c.tr is not None:
            c.eng.records(out=c.rec)
            c.tr["cube_luck"][step] = self.buf
            c.tr["cube_luck_state"][step] = cube.state
            c.tr["cube_luck_mover"][step] = c.rec[:, R_CUR]
            c.tr["cube_luck_roll"][step] = c.rec[:, R_ROLL0:R_ROLL1 + 1]
            c.tr["cube_luck_values"][step] = self.values

    def flush(self, done, info):
        c, cube, rule = self.c, self.cube, self.cube.rule
        check(c.L.bgx_rollout_cube_luck_flush(_ptr(c.starts), _ptr(c.grp), c.lanes[2], _ptr(done), _ptr(info), c.B, c.P,
                                              rule.cap, int(rule.jacoby), _ptr(cube.state), _ptr(c.ro.lane_luck),
                                              _ptr(self.tally), c.stream), "bgx_rollout_cube_luck_flush")


class _TableCutStage(_Stage):
    """A game that reaches a bearoff table stops there: one cut and masked reset after begin
    (after cube_begin) and one after every advance (the table's cut kernel, then the masked
    bgx_reset gives every cut lane its start record again).  A start record that is in the table
    itself is cut before a move is made; a lane's later games from it are cut after one ply.
    The trace gains cut uint8[steps, B] (each step's reset mask), cut_records uint8[steps, B, 64]
    (the records that cut saw) and cut0 / cut_records0, the same for the cut after begin.
    `bearoff` (a bearoff.BearoffDB, DESIGN.md §11, or a bearoff.OneSidedBearoffDB, §12, which
    cuts where both sides have a checker off; bgx_rollout_bearoff_cut / bgx_rollout_bearoff1_cut):
    the game is scored with the table's win probability -> cut_tally int64[n_groups, 4] (CUT_FIELDS).
    `cube_bearoff` (a bearoff.CubefulBearoffDB), with `cube`
    (bgx_rollout_cube_bearoff_cut, which also takes the cube stage's cap, cube0 and state): a
    cubeful game is scored with its exact cubeful expectation times its cube, and a lane that
    enters the table is cut before its next cube decision -> after cube_tally, cube_cut_tally
    int64[n_groups, 6] (cube.CUBE_CUT_FIELDS)."""
    sync_free = True

    def __init__(self, c: _Pass, table, cube: _CubeStage = None):
        self.c, self.table = c, table
        if table.kind == "cubeful":
            what, fields, self.entry = "cubeful bearoff table", CUBE_CUT_FIELDS, "bgx_rollout_cube_bearoff_cut"
            self.extra = (cube.rule.cap, _ptr(cube.c0), _ptr(cube.state))
        else:
            what, fields, self.entry, self.extra = "bearoff database", CUT_FIELDS, table.cut_entry, ()
        if table.device != c.dev:
            raise ValueError(f"run_lanes: the {what} is on {table.device}, the engine on {c.dev}")
        self.tally = c.tally(fields)
        self.mask = torch.empty(c.B, dtype=torch.uint8, device=c.dev)
        c.traced(("cut", torch.uint8), ("cut_records", torch.uint8, 64))

    def cut(self, step):
        c = self.c
        if c.tr is not None:
            c.eng.records(out=c.rec)
        check(getattr(c.L, self.entry)(self.table.handle(), c.recs, _ptr(c.starts), _ptr(c.grp), c.B, c.P, c.G,
                                       *c.lanes, _ptr(self.tally), c.active, _ptr(self.mask), *self.extra, c.stream),
              self.entry)
        if c.tr is not None and step is not None:
            c.tr["cut"][step] = self.mask
            c.tr["cut_records"][step] = c.rec
        c.reset(self.mask)

    def after_begin(self):
        self.cut(None)
        if self.c.tr is not None:
            self.c.tr_end.update(cut0=self.mask.clone(), cut_records0=self.c.rec.clone())

    after_advance = cut


class _HorizonStage(_Stage):
    """The two horizon cuts: after advance trunc_sel, value, the stage's cut(tv), reset(mask) -- where
    the bearoff cut sits; the masked reset gives the lane its start record again.  Sync-free when the
    truncation is.  The trace gains per step `prefix` uint8 (the lanes truncated), prefix_value (NaN
    off them), prefix_mover (the side on roll there) and the stage's extra_fields."""
    extra_fields = ()

    def __init__(self, c: _Pass, truncation, fields):
        self.c, self.t, self.sync_free = c, truncation, truncation.sync_free
        self.tally = c.tally(fields)
        self.tsel, self.mask = c.lane_buffers(2, torch.uint8)
        self.buf, self.scratch = c.lane_buffers(2, torch.float32, float("nan"))
        p = self.prefix
        c.traced((p, torch.uint8), (p + "_value", torch.float32), (p + "_mover", torch.uint8), *self.extra_fields)

    def extra_trace(self, step):
        pass

    def after_advance(self, step):
        c, tr, p = self.c, self.c.tr, self.prefix
        check(c.L.bgx_rollout_trunc_sel(c.recs, _ptr(c.grp), c.B, c.P, self.t.plies, c.lanes[1], c.lanes[2],
                                        _ptr(self.tsel), None, c.stream), "bgx_rollout_trunc_sel")
        tv = self.t.equity(c.eng, self.tsel, self.scratch, self.buf)
        if tr is not None:
            c.eng.records(out=c.rec)
            tr[p][step] = self.tsel
            tr[p + "_value"][step] = torch.where(self.tsel != 0, tv, float("nan"))
            tr[p + "_mover"][step] = c.rec[:, R_CUR]
            self.extra_trace(step)
        self.cut(tv)
        c.reset(self.mask)


class _TruncStage(_HorizonStage):
    """`truncate` (a truncate.Truncation): a game that has run truncate.plies plies
    without ending stops there and is scored with the truncation's value of the side on roll
    (trunc_cut).  The cut sits where the truncated game's luck sum is complete (the roll now in the
    record is added only at the next step).  `with_luck`: the luck stage runs too and trunc_cut also
    takes and clears the truncated games' luck sums (summarize_truncated_luck).  Result (after
    luck_tally, if any): trunc_tally int64[n_groups, 7] (TRUNC_FIELDS)."""
    prefix = "trunc"

    def __init__(self, c: _Pass, truncation, with_luck: bool):
        super().__init__(c, truncation, TRUNC_FIELDS)
        self.luck = _ptr(c.ro.lane_luck) if with_luck else None

    def cut(self, tv):
        c = self.c
        check(c.L.bgx_rollout_trunc_cut(c.recs, _ptr(c.starts), _ptr(c.grp), _ptr(self.tsel), _ptr(tv), self.t.scale,
                                        c.B, c.P, c.G, *c.lanes, self.luck, _ptr(self.tally), c.active,
                                        _ptr(self.mask), c.stream), "bgx_rollout_trunc_cut")


class _CubeTruncStage(_HorizonStage):
    """`cube_truncate` (a cube.CubeTruncation), with `cube`: a cubeful game that has
    run cube_truncate.plies plies without ending stops there and is scored with Janowski's
    cube-life equity of the side on roll, times the lane's cube (cube_trunc_cut, which also takes
    the cube stage's cap, Jacoby rule, cube0 and state).  It is the last stage (after the table cut,
    whose lanes have plies 0 and so are not truncated in the same step).  Result (after cube_tally
    and cube_cut_tally, if any): cube_trunc_tally int64[n_groups, 6] (CUBE_TRUNC_FIELDS); the trace
    also gains ctrunc_cube (the cube states before the cut)."""
    prefix = "ctrunc"
    extra_fields = (("ctrunc_cube", torch.uint8),)

    def __init__(self, c: _Pass, truncation, cube: _CubeStage):
        super().__init__(c, truncation, CUBE_TRUNC_FIELDS)
        self.cube, self.life = cube, truncation.life.struct()

    def extra_trace(self, step):
        self.c.tr["ctrunc_cube"][step] = self.cube.state

    def cut(self, tv):
        c, rule = self.c, self.cube.rule
        check(c.L.bgx_rollout_cube_trunc_cut(c.recs, _ptr(c.starts), _ptr(c.grp), _ptr(self.tsel), _ptr(tv),
                                             self.t.scale, self.life, c.B, c.P, c.G, *c.lanes, _ptr(self.tally),
                                             c.active, _ptr(self.mask), rule.cap, int(rule.jacoby), _ptr(self.cube.c0),
                                             _ptr(self.cube.state), c.stream), "bgx_rollout_cube_trunc_cut")


class Rollout:
    """`batch` lanes of an engine of its own (auto_reset, so a finished game's lane starts
    its next one, from its start record, in the same step)."""

    def __init__(self, batch: int, seed: int = 0, dice: str = "philox", max_moves: int = 500, device=None):
        if batch <= 0:
            raise ValueError(f"Rollout: batch {batch} must be positive")
        if dice == "shared":
            raise ValueError("Rollout: a shared-dice engine has no start positions")
        self.B, self.seed = int(batch), int(seed)
        self.eng = Engine(batch=self.B, max_moves=max_moves, seed=self.seed, dice=dice, auto_reset=True, device=device)
        if dice != "philox":
            self.eng.seed((np.arange(self.B, dtype=np.uint64) + self.seed) & 0xFFFFFFFF)
        dev = self.eng.device
        self.games_done = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.plies = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.sel = torch.zeros(self.B, dtype=torch.uint8, device=dev)
        self.active = torch.zeros(1, dtype=torch.int64, device=dev)
        self.actions = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.lane_luck = torch.zeros(self.B, dtype=torch.float32, device=dev)     # luck of the current games
        self.steps = 0                  # steps of every run so far: the players' random streams go on

    def run_lanes(self, player, starts, group, n_groups: int, games_per_lane: int, max_steps: int = 4000,
                  trace: bool = False, luck=None, bearoff=None, cube=None, cube0=None, truncate=None,
                  cube_bearoff=None, cube_truncate=None, cube_luck=None, match=None, match_score=None):
        """One pass on explicit lanes: `starts` uint8[B, 64] start records (a valid one on idle
        lanes too), `group` int32[B] lane -> tally row in [0, n_groups) or -1 (idle),
        `games_per_lane` games on every lane that has a row.  set_starts, reset, begin, then
        [act, merge, step, advance] until no lane is active or `max_steps` env steps ran; the
        host reads the active-lane count every SYNC_EVERY steps when the player and every stage
        are sync-free, else every step.  The engine keeps the table afterwards.  Returns (tally
        int64[n_groups, 8], unfinished int64[n_groups] = scheduled games that did not end, trace)
        followed by one tally per mode, in the stages' order below: trace (None without
        trace=True) holds per-step [steps, B] tensors mover, action, done, info, the modes'
        fields, and the final games_done and active.

        Every mode is a stage (the classes above; their docstrings say what each does per step,
        returns and traces).  The loop calls them in a fixed order -- luck, cube, table cut,
        truncation, cubeful truncation -- after begin, before act, after the step (before advance)
        and after advance:

            begin; cube_begin; cut, reset(mask)
            [ roll_luck, luck_add;  cube_sel, equity, (cube_luck_pass,) cube_decide, reset(mask),
              (roll_values, cube_roll_luck, cube_luck_add);
              act, merge, step;  luck_flush;  (cube_luck_flush,) cube_flush;  advance;
              cut, reset(mask);  trunc_sel, value, trunc_cut or cube_trunc_cut, reset(mask) ]

        `luck` (a search.ValueHead): the luck of every roll, summed per game -> luck_tally.
        `bearoff` (a bearoff.BearoffDB or OneSidedBearoffDB): games stop at the table -> cut_tally.
        `cube` (a cube.CubeRule), `cube0` (uint8[B] start cubes): the doubling cube -> cube_tally.
        `truncate` (a truncate.Truncation): games stop at a horizon, scored by a value -> trunc_tally.
        `cube_bearoff` (a bearoff.CubefulBearoffDB), with `cube`: cubeful games stop at the cubeful
        table -> cube_tally, cube_cut_tally.
        `cube_truncate` (a cube.CubeTruncation), with `cube`: cubeful games stop at a horizon, scored
        by Janowski's cube-life equity -> cube_tally, [cube_cut_tally,] cube_trunc_tally.
        `cube_luck` (a cube.CubeLuck), with `cube` alone: the luck of every roll of the cubeful games
        (the parenthesised calls above, made from inside the cube stage) -> cube_tally,
        cube_luck_tally.
        `match` (a match.RolloutMatch), `match_score` = (away [n_groups, 2], craw [n_groups]), `cube0`:
        single games at a fixed match score (match_sel, the rule's value, match_decide,
        reset(mask) before act and match_flush after the step, where the cube's calls sit) -> match_hist.
        It goes with no other mode.
        Each None: nothing changes; all None: exactly the three results above.

        Together: `truncate` with `luck` IS supported (..., luck_tally, trunc_tally;
        summarize_truncated_luck), `cube_bearoff` and `cube_truncate` need `cube` and go together
        (exact where the table reaches, Janowski elsewhere).  Every other pair raises
        ValueError (_check_modes): `bearoff` with `luck` needs cross sums that are not kept, the
        luck of a cubeful game and cubeful values of the cubeless table do not exist (`cube` with
        `luck` or `bearoff`), nor do other three-way summaries (`truncate`, `cube_bearoff` or
        `cube_truncate` with others; `cube_luck` with anything but `cube`)."""
        _check_modes("run_lanes", luck, bearoff, cube, truncate, cube_bearoff, cube0, types=True,
                     cube_truncate=cube_truncate, cube_luck=cube_luck, match=match)
        if match is None and match_score is not None:
            raise ValueError("run_lanes: match_score without match")
        max_steps, G, P = int(max_steps), int(games_per_lane), int(n_groups)
        if max_steps < 0 or G < 0 or P <= 0:
            raise ValueError(f"run_lanes: max_steps {max_steps}, games_per_lane {G} must be >= 0, n_groups {P} > 0")
        if trace and self.B * max_steps > TRACE_LIMIT:
            raise ValueError(f"run_lanes: trace=True holds batch x max_steps = {self.B * max_steps} entries per "
                             f"field; the limit is {TRACE_LIMIT} (it is for tests and small batches)")
        eng, dev = self.eng, self.eng.device
        starts = torch.as_tensor(starts)
        grp = torch.as_tensor(group).to(device=dev, dtype=torch.int32).contiguous()
        if grp.shape != (self.B,) or bool((grp >= P).any()):
            raise ValueError(f"run_lanes: group must be int32[{self.B}] with entries below n_groups = {P}")
        eng.set_starts(starts)              # validated where the records live (the host, from run())
        # the kernels' copy of starts: the start movers
        c = _Pass(self, starts.to(dev).contiguous(), grp, P, G, max_steps, trace)
        L, tr, rec = c.L, c.tr, c.rec
        tally = torch.zeros(P, 8, dtype=torch.int64, device=dev)
        eng.reset(want_obs=False)
        check(L.bgx_rollout_begin(c.recs, _ptr(c.starts), _ptr(grp), self.B, P, G, *c.lanes, _ptr(tally), c.active,
                                  c.stream), "bgx_rollout_begin")
        c.traced(("mover", torch.uint8), ("action", torch.int32), ("done", torch.uint8), ("info", torch.int32))
        table = bearoff if bearoff is not None else cube_bearoff
        luck_stage = _LuckStage(c, luck) if luck is not None else None
        cube_stage = _CubeStage(c, cube, cube0) if cube is not None else None
        cut_stage = _TableCutStage(c, table, cube_stage) if table is not None else None
        trunc_stage = _TruncStage(c, truncate, luck is not None) if truncate is not None else None
        ctrunc_stage = _CubeTruncStage(c, cube_truncate, cube_stage) if cube_truncate is not None else None
        cluck_stage = _CubeLuckStage(c, cube_luck, cube_stage) if cube_luck is not None else None
        match_stage = _MatchStage(c, match, match_score, cube0) if match is not None else None
        stages = [s for s in (luck_stage, cube_stage, cut_stage, trunc_stage, ctrunc_stage, cluck_stage, match_stage)
                  if s is not None]
        for s in stages:
            s.after_begin()
        every = SYNC_EVERY if getattr(player, "sync_free", False) and all(s.sync_free for s in stages) else 1
        steps = 0
        active = int(self.active.item())
        while active > 0 and steps < max_steps:
            for s in stages:
                s.before_act(steps)
            act = player.act(eng, self.sel, self.steps)
            if (not isinstance(act, torch.Tensor) or act.dtype != torch.int32 or act.device != dev
                    or not act.is_contiguous() or act.numel() != self.B):
                raise ValueError("a player's act must return a contiguous int32[B] tensor on the engine's device")
            # actions = sel ? act : 0 (the arena's merge with one player on both sides)
            check(L.bgx_arena_merge(_ptr(self.sel), _ptr(self.sel), _ptr(act), _ptr(act), self.B,
                                    _ptr(self.actions), c.stream), "bgx_arena_merge")
            if trace:
                eng.records(out=rec)
                tr["mover"][steps] = rec[:, R_CUR]
                tr["action"][steps] = self.actions
            _, _, done, info = eng.step(self.actions, want_obs=False, want_info=True)
            for s in stages:
                s.after_step(done, info)
            check(L.bgx_rollout_advance(c.recs, _ptr(c.starts), _ptr(grp), _ptr(done), _ptr(info), self.B, P, G,
                                        *c.lanes, _ptr(tally), c.active, c.stream), "bgx_rollout_advance")
            if trace:
                tr["done"][steps] = done
                tr["info"][steps] = info
            for s in stages:
                s.after_advance(steps)
            steps += 1
            self.steps += 1
            if steps % every == 0 or steps == max_steps:
                active = int(self.active.item())
        left = torch.where(grp >= 0, G - self.games_done, 0).to(torch.int64)
        unfinished = torch.zeros(P, dtype=torch.int64, device=dev).index_add_(0, grp.clamp(min=0).long(), left)
        if trace:
            tr = {n: v[:steps] for n, v in tr.items()}
            tr.update(c.tr_end, games_done=self.games_done.clone(), active=int(self.active.item()))
        return (tally, unfinished, tr) + tuple(s.tally for s in stages)

    def run(self, player, positions, trials: int, first_roll: str = "stratified", max_steps: int = 4000,
            trace: bool = False, luck=None, luck_scale="fit", bearoff=None, cube=None, cube_start=(0, 0),
            truncate=None, cube_bearoff=None, cube_truncate=None, cube_luck=None, cube_luck_scale="fit", match=None,
            match_away=None, match_crawford=0):
        """Roll out every position (uint8 [P, 64] records: board and mover are read, the roll
        bytes come from the layout) `trials` times with `player` (any arena player object)
        on both sides: run_lanes per pass of the layout, at most `max_steps` env steps each
        (the rest is reported as `unfinished`); standard openings again afterwards.  Returns
        the list of the positions' results (summarize); with trace=True also the last
        pass's trace with its group, starts and games_per_lane.  The modes are run_lanes' (its
        stages; the combinations it refuses raise ValueError here too, before anything runs):
        `luck` (a search.ValueHead): the results are summarize_luck's, with `luck_scale` ("fit" or a
        float) as its scale.  `bearoff` (a bearoff.BearoffDB or bearoff.OneSidedBearoffDB): the
        results are summarize_bearoff's; with the one-sided table they also carry `bearoff_kind` =
        "one-sided": its cut values are approximations, so `equity_stderr` is the sample's spread
        and no longer measures the error against the truth.  `cube` (a cube.CubeRule; DESIGN.md
        §13): every game starts with the cube `cube_start` = (k, owner), owner 0 centred, 1
        PLAYER1, 2 PLAYER2, or one such pair per position; the results are cube.summarize_cube's.
        `truncate` (a truncate.Truncation): the results are summarize_truncated's,
        with `luck` those of summarize_truncated_luck.  `cube_bearoff` (a bearoff.CubefulBearoffDB;
        DESIGN.md §15), with `cube`: the results are cube.summarize_cube_bearoff's and carry
        `bearoff_kind` = "cubeful".  `cube_truncate` (a cube.CubeTruncation), with
        `cube`: the results are cube.summarize_cube_truncated's (with `cube_bearoff` too, its
        cut_row= form).  `cube_luck` (a cube.CubeLuck), with `cube` alone: the results are
        cube.summarize_cube_luck's, with `cube_luck_scale` ("fit" or a float) as its scale.  `match` (a
        match.RolloutMatch), alone: single games at the score `match_away` = (a1, a2),
        the points PLAYER1 and PLAYER2 still need, or one pair per position, with the Crawford state
        `match_crawford` (0 before, 1 the Crawford game, 2 after it; or one per position) and the
        starting cube `cube_start`; the results are match.summarize_match_rollout's, `mwc` the
        match-winning chance of the position's mover."""
        _check_modes("run", luck, bearoff, cube, truncate, cube_bearoff, cube_truncate=cube_truncate,
                     cube_luck=cube_luck, match=match)
        pos = _records(positions)
        P = pos.shape[0]
        score = None
        if match is not None:
            from .match import RolloutMatch, outcome_mwc, summarize_match_rollout, validate_score
            if not isinstance(match, RolloutMatch):
                raise ValueError("run: match must be a match.RolloutMatch")
            if match_away is None:
                raise ValueError("run: match needs match_away = (a1, a2) or one pair per position")
            aw, cr = np.asarray(match_away), np.asarray(match_crawford)
            if aw.shape not in ((2,), (P, 2)) or cr.shape not in ((), (P,)):
                raise ValueError(f"run: match_away must be (a1, a2) or one pair per position and match_crawford one state "
                                 f"or one per position, got shapes {aw.shape} and {cr.shape}")
            checked = [validate_score(match.length, a, c) for a, c in zip(np.broadcast_to(aw, (P, 2)).tolist(),
                                                                          np.broadcast_to(cr, (P,)).tolist())]
            score = (np.asarray([a for a, _ in checked], np.uint8), np.asarray([c for _, c in checked], np.uint8))
        elif match_away is not None:
            raise ValueError("run: match_away without match")
        group, roll, G, passes = layout(P, int(trials), first_roll, self.B)
        totals = tr = None
        if cube is not None or match is not None:
            from .cube import pack
            cs = np.asarray(cube_start, np.int64)
            if cs.shape not in ((2,), (P, 2)):
                raise ValueError(f"run: cube_start must be (k, owner) or one pair per position, got shape {cs.shape}")
            start_byte = torch.tensor([pack(k, o) for k, o in np.broadcast_to(cs, (P, 2))], dtype=torch.uint8)
        for k in range(passes):
            grp = torch.from_numpy(group[k])
            starts = pos[grp.clamp(min=0).long()].clone()          # idle lanes: a valid record, never counted
            starts[:, R_ROLL0:R_ROLL1 + 1] = torch.from_numpy(roll[k])
            tally, unf, tr, *extra = self.run_lanes(
                player, starts, grp, P, G, max_steps=max_steps, trace=trace, luck=luck, bearoff=bearoff, cube=cube,
                cube0=start_byte[grp.clamp(min=0).long()] if cube is not None or match is not None else None,
                truncate=truncate, cube_bearoff=cube_bearoff, cube_truncate=cube_truncate, cube_luck=cube_luck,
                match=match, match_score=score)
            sums = [tally, unf] + extra                            # the modes' tallies in run_lanes' order
            totals = sums if totals is None else [a + b for a, b in zip(totals, sums)]
            if trace:
                tr.update(group=grp, starts=starts, games_per_lane=G)
        self.eng.set_starts(None)
        rows, unf, *extra = (t.cpu().tolist() for t in totals)
        summary = _summary(luck, bearoff, cube, truncate, cube_bearoff, cube_truncate, cube_luck)
        scale = (luck_scale,) if luck is not None else (cube_luck_scale,) if cube_luck is not None else ()
        if match is not None:
            ks = np.broadcast_to(cs, (P, 2))[:, 0]
            res = [summarize_match_rollout(rows[p], extra[0][p],
                                           outcome_mwc(match.met, match.pc, match.length, score[0][p], int(score[1][p]),
                                                       int(pos[p, R_CUR])), unf[p], cube_k=int(ks[p]))
                   for p in range(P)]
            return (res, tr) if trace else res
        res = [summary(rows[p], *(e[p] for e in extra), *scale, unf[p]) for p in range(P)]
        table = bearoff if bearoff is not None else cube_bearoff
        if table is not None and table.kind != "two-sided":
            for r in res:
                r["bearoff_kind"] = table.kind
        return (res, tr) if trace else res


def _summary(luck, bearoff, cube, truncate, cube_bearoff, cube_truncate=None, cube_luck=None):
    """The summary of a position's rows by the modes of the run (after _check_modes): a function
    (tally_row, *the modes' rows in run_lanes' order, [the scale with luck or cube_luck,] unfinished)."""
    if cube is not None:
        if cube_luck is not None:
            return summarize_cube_luck
        if cube_truncate is not None and cube_bearoff is not None:
            return lambda t, c, cut, tr, unf=0: summarize_cube_truncated(t, c, tr, unf, cut_row=cut)
        if cube_truncate is not None:
            return summarize_cube_truncated
        return summarize_cube_bearoff if cube_bearoff is not None else summarize_cube
    if truncate is not None:
        return summarize_truncated_luck if luck is not None else summarize_truncated
    if luck is not None:
        return summarize_luck
    return summarize_bearoff if bearoff is not None else summarize


def exact_score(after52, mover: int) -> int:
    """0 when `mover` has not borne off all 15 checkers in the afterstate (int8[52]); else the
    game's points by the env's rule: 2 when the opponent has none off, 3 when in addition
    the opponent has a checker in the mover's home board or on the bar, else 1."""
    b = np.asarray(after52).astype(np.int64)
    if b[50 + mover] < 15:
        return 0
    opp = 1 - mover
    if b[50 + opp] > 0:
        return 1
    home = 18 if mover == 0 else 0
    return 3 if b[opp * 24 + home:opp * 24 + home + 6].sum() > 0 or b[48 + opp] > 0 else 2


def decode_move(v: int):
    """uint64 move -> [(src, dst, hit), ...] (16 bits per sub-move)."""
    subs = []
    for i in range(4):
        s = (int(v) >> (16 * i)) & 0xFFFF
        if not s & 0x8000:
            break
        subs.append((s & 31, (s >> 5) & 31, (s >> 10) & 1))
    return subs


def rollout_moves(rollout: Rollout, player, record, trials: int, first_roll: str = "stratified",
                  max_steps: int = 4000, luck=None, luck_scale="fit", truncate=None) -> list:
    """A decision: `record` (uint8[64]) holds the board, the mover and the roll to play.  Every
    legal move's afterstate is rolled out with the opponent on roll and the move's equity is
    minus that rollout's; moves that reach the same afterstate share one rollout.  A move
    that ends the game is scored exactly and spends no lanes (`games` 0, `exact` True).
    Returns one dict per move, best first: move (the encoded uint64), submoves, equity,
    equity_stderr, games, exact.  No legal move: one entry with move None (the pass).
    `luck` / `luck_scale` (Rollout.run): luck-adjusted rollouts; every entry also has
    equity_luck, equity_luck_stderr, luck_scale and variance_ratio (an exact move: its score,
    0, 0 and 1), and the order is by equity_luck.  `truncate` (Rollout.run): truncated rollouts;
    every rolled-out entry also has truncated_share (an exact move: 0)."""
    rec = torch.as_tensor(record).reshape(-1)
    if rec.numel() != 64 or rec.dtype != torch.uint8:
        raise ValueError("rollout_moves: record must be 64 bytes (uint8)")
    rec = rec.cpu().clone()
    rec[55:] = 0
    validate_starts(rec[None])
    mover, dice = int(rec[R_CUR]), (int(rec[R_ROLL0]), int(rec[R_ROLL1]))
    if dice[0] == 0:
        raise ValueError("rollout_moves: the record has no roll to play (bytes 53, 54)")
    eng = rollout.eng
    # the legal moves and their afterstates: the position posed on lane 0 (the rollout resets it)
    eng.set_lanes(rec[None], lane0=0)
    lane, mv, _ = eng.lanes(0, 1)
    n = int(lane[0, 60]) | (int(lane[0, 61]) << 8)
    if n == 0:
        moves, afters = [None], rec[None, :52].numpy().view(np.int8)
    else:
        moves = [int(m) for m in mv[0, :n].cpu().numpy().view(np.uint64)]
        afters = eng.afterstates(0, 1)[0, :n].cpu().numpy()
    scores = [exact_score(a, mover) for a in afters]
    open_idx = [i for i, s in enumerate(scores) if s == 0]
    results = {}
    if open_idx:
        uniq, inverse = np.unique(afters[open_idx], axis=0, return_inverse=True)
        pos = np.zeros((len(uniq), 64), np.uint8)
        pos[:, :52] = uniq.view(np.uint8)
        pos[:, R_CUR] = 1 - mover
        res = rollout.run(player, torch.from_numpy(pos), trials, first_roll=first_roll, max_steps=max_steps,
                          luck=luck, luck_scale=luck_scale, truncate=truncate)
        for i, u in zip(open_idx, np.asarray(inverse).reshape(-1)):
            results[i] = res[int(u)]
    out = []
    for i, m in enumerate(moves):
        if scores[i]:
            out.append(dict(move=m, submoves=decode_move(m), equity=float(scores[i]), equity_stderr=0.0, games=0,
                            exact=True, unfinished=0))
            if luck is not None:
                out[-1].update(equity_luck=float(scores[i]), equity_luck_stderr=0.0, luck_scale=0.0,
                               variance_ratio=1.0)
            if truncate is not None:
                out[-1].update(truncated_share=0.0)
        else:
            r = results[i]
            out.append(dict(move=m, submoves=decode_move(m) if m is not None else [], equity=-r["equity"],
                            equity_stderr=r["equity_stderr"], games=r["games"], exact=False,
                            unfinished=r["unfinished"]))
            if luck is not None:
                out[-1].update(equity_luck=-r["equity_luck"], equity_luck_stderr=r["equity_luck_stderr"],
                               luck_scale=r["luck_scale"], variance_ratio=r["variance_ratio"])
            if truncate is not None:
                out[-1].update(truncated_share=r["truncated_share"])
    out.sort(key=lambda d: -d["equity_luck" if luck is not None else "equity"])
    return out


# ------------------------------------------------------------- command line --
def opening_record() -> torch.Tensor:
    """The standard opening position, PLAYER1 on roll."""
    r = torch.zeros(64, dtype=torch.uint8)
    for p, c in ((0, 2), (11, 5), (16, 3), (18, 5), (24 + 23, 2), (24 + 12, 5), (24 + 7, 3), (24 + 5, 5)):
        r[p] = c
    return r


def load_positions(path: str) -> torch.Tensor:
    """"opening", or a JSON file: a list of {"board": [52 ints], "player": 0 | 1}."""
    if path == "opening":
        return opening_record()[None]
    with open(path) as f:
        items = json.load(f)
    if not isinstance(items, list) or not items:
        raise ValueError(f"{path}: expected a non-empty JSON list of positions")
    out = torch.zeros(len(items), 64, dtype=torch.uint8)
    for i, it in enumerate(items):
        board = it["board"]
        if len(board) != 52 or any(not 0 <= int(v) <= 15 for v in board):
            raise ValueError(f"{path}: position {i}: board must be 52 counts in 0..15")
        out[i, :52] = torch.tensor([int(v) for v in board], dtype=torch.uint8)
        out[i, R_CUR] = int(it.get("player", 0))
    return out


def _luck_scale(text: str, option: str = "--luck-scale"):
    if text == "fit":
        return text
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{option} takes 'fit' or a number, got {text!r}")
    if not math.isfinite(v):
        raise argparse.ArgumentTypeError(f"{option} must be finite")
    return v


def _cube_luck_scale(text: str):
    return _luck_scale(text, "--cube-luck-scale")


class _Parser(argparse.ArgumentParser):
    """--top-k is an error for any player but a 2ply one with weights; --luck and --cube need
    weights; --cube goes with neither --luck nor a bearoff cut; --truncate needs a net and goes
    with neither a bearoff cut nor --cube; --cube-truncate and its options need --cube and go with
    none of --luck, --bearoff, --bearoff1 and --truncate; --cube-luck and its options need --cube and
    weights and go with none of --luck, --bearoff, --bearoff1, --truncate, --cube-bearoff and
    --cube-truncate."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.top_k is not None:
            if ns.player != "2ply" or ns.net == "random":
                self.error("--top-k needs --player 2ply with weights")
            if ns.top_k < 1:
                self.error("--top-k must be >= 1")
        if ns.luck and ns.net == "random":
            self.error("--luck needs --net with weights (the luck is measured by the net's value head)")
        if ns.bearoff is not None and ns.luck:
            self.error("--bearoff and --luck cannot be combined")
        if ns.bearoff1 is not None and ns.luck:
            self.error("--bearoff1 and --luck cannot be combined")
        if ns.bearoff is not None and ns.bearoff1 is not None:
            self.error("--bearoff and --bearoff1 cannot be combined (one cut per rollout)")
        for name, top in (("bearoff", 8), ("bearoff_play", 8), ("bearoff1", 15), ("bearoff1_play", 15)):
            k = getattr(ns, name)
            if k is not None and not 1 <= k <= top:
                self.error(f"--{name.replace('_', '-')} takes a number of checkers in 1..{top}")
        if ns.cube_decision and not ns.cube:
            self.error("--cube-decision needs --cube")
        if ns.cube_bearoff is not None:
            if not ns.cube:
                self.error("--cube-bearoff needs --cube")
            if not 1 <= ns.cube_bearoff <= 8:
                self.error("--cube-bearoff takes a number of checkers in 1..8")
        if ns.cube:
            if ns.net == "random" and ns.cube_net is None:
                self.error("--cube needs --net with weights or --cube-net (the decisions are made on a net's "
                           "value head)")
            for name in ("luck", "bearoff", "bearoff1"):
                if getattr(ns, name) not in (None, False):
                    self.error(f"--cube and --{name} cannot be combined")
            if not 0 <= ns.cube_cap <= 10:
                self.error("--cube-cap takes a number in 0..10")
            for name in ("cube_double", "cube_pass", "cube_too_good", "cube_scale"):
                if math.isnan(getattr(ns, name)):
                    self.error(f"--{name.replace('_', '-')} must be a number")
        if ns.truncate is None:
            if ns.truncate_net is not None or ns.truncate_lookahead != 0 or ns.truncate_scale != 1.0:
                self.error("--truncate-net, --truncate-scale and --truncate-lookahead need --truncate")
        else:
            if ns.truncate < 1:
                self.error("--truncate takes a number of plies >= 1")
            if ns.net == "random" and ns.truncate_net is None:
                self.error("--truncate needs --net with weights or --truncate-net (the games are scored by a "
                           "net's value head)")
            for name in ("bearoff", "bearoff1", "cube"):
                if getattr(ns, name) not in (None, False):
                    self.error(f"--truncate and --{name} cannot be combined")
            if math.isnan(ns.truncate_scale):
                self.error("--truncate-scale must be a number")
        if ns.cube_truncate is None:
            if (ns.cube_truncate_net is not None or ns.cube_truncate_lookahead != 0 or ns.cube_truncate_scale != 1.0
                    or ns.cube_life != 0.68 or ns.cube_win_value != 1.0 or ns.cube_loss_value != 1.0):
                self.error("--cube-life, --cube-win-value, --cube-loss-value, --cube-truncate-net, "
                           "--cube-truncate-scale and --cube-truncate-lookahead need --cube-truncate")
        else:
            if not ns.cube:
                self.error("--cube-truncate needs --cube")
            if ns.cube_truncate < 1:
                self.error("--cube-truncate takes a number of plies >= 1")
            for name in ("luck", "bearoff", "bearoff1", "truncate"):
                if getattr(ns, name) not in (None, False):
                    self.error(f"--cube-truncate and --{name} cannot be combined")
            if math.isnan(ns.cube_truncate_scale):
                self.error("--cube-truncate-scale must be a number")
            for name, lo, hi in (("cube_life", 0.0, 1.0), ("cube_win_value", 1.0, 3.0), ("cube_loss_value", 1.0, 3.0)):
                if not lo <= getattr(ns, name) <= hi:
                    self.error(f"--{name.replace('_', '-')} takes a number in [{lo:g}, {hi:g}]")
        if not ns.cube_luck:
            if (ns.cube_luck_net is not None or ns.cube_luck_scale != "fit" or ns.cube_luck_life != 0.68
                    or ns.cube_luck_win_value != 1.0 or ns.cube_luck_loss_value != 1.0 or ns.cube_luck_value_scale != 1.0):
                self.error("--cube-luck-net, --cube-luck-scale, --cube-luck-life, --cube-luck-win-value, "
                           "--cube-luck-loss-value and --cube-luck-value-scale need --cube-luck")
        else:
            if not ns.cube:
                self.error("--cube-luck needs --cube")
            if ns.net == "random" and ns.cube_luck_net is None:
                self.error("--cube-luck needs --net with weights or --cube-luck-net (the luck is measured by a net's "
                           "value head)")
            for name in ("luck", "bearoff", "bearoff1", "truncate", "cube_bearoff", "cube_truncate"):
                if getattr(ns, name) not in (None, False):
                    self.error(f"--cube-luck and --{name.replace('_', '-')} cannot be combined")
            if math.isnan(ns.cube_luck_value_scale):
                self.error("--cube-luck-value-scale must be a number")
            for name, lo, hi in (("cube_luck_life", 0.0, 1.0), ("cube_luck_win_value", 1.0, 3.0),
                                 ("cube_luck_loss_value", 1.0, 3.0)):
                if not lo <= getattr(ns, name) <= hi:
                    self.error(f"--{name.replace('_', '-')} takes a number in [{lo:g}, {hi:g}]")
        self._match_args(ns)
        if ns.trials < 1 or ns.batch < 1:
            self.error("--trials and --batch must be >= 1")
        return ns

    def _match_args(self, ns):
        """--match N needs --match-score and goes with none of --cube, --luck, a bearoff cut and
        --truncate; every other --match-* option and --met need it; the rule's options need weights."""
        rule_opts = ("match_window", "match_gammons", "match_lookahead", "match_net", "match_scale")
        opts = ("match_score", "match_crawford", "met", "match_cube") + rule_opts
        if ns.match is None:
            given = [o for o in opts if getattr(ns, o) is not None] + (["match_decision"] if ns.match_decision else [])
            if given:
                self.error(", ".join("--" + o.replace("_", "-") for o in given) + " need --match")
            return
        if not 1 <= ns.match <= 25:
            self.error("--match takes a match length in 1..25")
        for name in ("cube", "luck", "bearoff", "bearoff1", "truncate", "cube_bearoff", "cube_truncate", "cube_luck"):
            if getattr(ns, name) not in (None, False):
                self.error(f"--match and --{name.replace('_', '-')} cannot be combined")
        if ns.match_score is None:
            self.error("--match needs --match-score A1,A2")
        if ns.net == "random" and ns.match_net is None and any(getattr(ns, o) is not None for o in rule_opts):
            self.error("--match-window, --match-gammons, --match-lookahead and --match-scale need --net with weights or "
                       "--match-net (without either nobody doubles)")
        for name, default in MATCH_DEFAULTS.items():
            if getattr(ns, name) is None:
                setattr(ns, name, default)
        if math.isnan(ns.match_scale):
            self.error("--match-scale is NaN")
        if not 0.0 <= ns.match_window <= 1.0:
            self.error("--match-window takes a number in [0, 1]")
        from .match import validate_score
        try:
            validate_score(ns.match, ns.match_score, ns.match_crawford)
        except ValueError as e:
            self.error(str(e))
        k, owner = ns.match_cube
        if not 0 <= k <= 10 or owner not in (0, 1, 2) or (owner == 0) != (k == 0):
            self.error("--match-cube takes K,OWNER with K in 0..10, OWNER 0 (centred, K = 0), 1 or 2")


MATCH_DEFAULTS = {"match_crawford": 0, "match_cube": (0, 0), "match_window": 0.65, "match_gammons": (0.25, 0.25),
                  "match_lookahead": 1, "match_scale": 1.0}


def _int_pair(option: str):
    def parse(text: str):
        try:
            a, b = (int(v) for v in text.split(","))
        except ValueError:
            raise argparse.ArgumentTypeError(f"{option} takes two whole numbers A,B, got {text!r}")
        return a, b
    return parse


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(prog="python -m bgx.rollout", description="Roll positions out with one player on both sides.")
    ap.add_argument("--net", required=True, help="a state_dict file (PPOTrainer.save) or 'random'")
    ap.add_argument("--player", default="policy", choices=PLAYER_KINDS)
    ap.add_argument("--top-k", type=int, default=None, help="2ply only: search only the top-k 1-ply moves")
    ap.add_argument("--positions", required=True,
                    help="'opening' or a JSON file: a list of {\"board\": [52 ints], \"player\": 0|1}")
    ap.add_argument("--trials", type=int, default=1296, help="games per position (stratified: a multiple of 36)")
    ap.add_argument("--first-roll", default="stratified", choices=FIRST_ROLLS)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--max-steps", type=int, default=4000,
                    help="env steps per pass after which it stops (unfinished games are reported)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--luck", action="store_true",
                    help="luck-adjusted (variance-reduced) rollout with the net's value head; needs weights")
    ap.add_argument("--luck-scale", type=_luck_scale, default="fit",
                    help="'fit' (the control-variate coefficient of the games) or a fixed number")
    ap.add_argument("--bearoff", type=int, default=None, metavar="K",
                    help="stop a game at the exact bearoff table for K checkers a side (1..8) and score it "
                         "with its exact win probability; not with --luck")
    ap.add_argument("--bearoff-play", type=int, nargs="?", const=6, default=None, metavar="K",
                    help="the player moves perfectly where the position is in the bearoff table (K checkers "
                         "a side, default 6)")
    ap.add_argument("--bearoff1", type=int, default=None, metavar="K",
                    help="stop a game at the one-sided bearoff table for K checkers a side (1..15) once both "
                         "sides have a checker off, and score it with the table's approximate win probability; "
                         "not with --luck or --bearoff")
    ap.add_argument("--bearoff1-play", type=int, nargs="?", const=15, default=None, metavar="K",
                    help="the player moves by the one-sided bearoff table in every pure home-board race (K "
                         "checkers a side, default 15); with --bearoff-play the exact table plays where it reaches")
    ap.add_argument("--cube", action="store_true",
                    help="money play with the doubling cube: cubeful equity beside the played-out games' result; "
                         "needs weights; not with --luck, --bearoff or --bearoff1")
    ap.add_argument("--cube-net", default=None, metavar="PATH",
                    help="the state_dict whose value head makes the cube decisions (default: the player's net)")
    ap.add_argument("--cube-double", type=float, default=0.40, help="the mover doubles from this equity on")
    ap.add_argument("--cube-pass", type=float, default=0.50, help="the opponent passes above this equity")
    ap.add_argument("--cube-too-good", type=float, default=math.inf,
                    help="the mover plays on for the gammon above this equity")
    ap.add_argument("--cube-scale", type=float, default=1.0, help="points per unit of the net's value")
    ap.add_argument("--cube-cap", type=int, default=6, help="no double once the cube shows 2^CAP (0..10)")
    ap.add_argument("--jacoby", action="store_true", help="gammons count only after a double")
    ap.add_argument("--truncate", type=int, default=None, metavar="N",
                    help="stop a game after N plies (>= 1) and score it with a net's value head; with --luck the "
                         "luck-adjusted estimate covers the truncated games too; not with --bearoff, --bearoff1 "
                         "or --cube")
    ap.add_argument("--truncate-scale", type=float, default=1.0, help="points per unit of the net's value")
    ap.add_argument("--truncate-lookahead", type=int, default=0, choices=(0, 1),
                    help="0: the value head on the position itself (sync-free); 1: its mean best 1-ply value "
                         "over the 21 rolls")
    ap.add_argument("--truncate-net", default=None, metavar="PATH",
                    help="the state_dict whose value head scores the truncated games (default: the player's net)")
    ap.add_argument("--cube-bearoff", type=int, default=None, metavar="K",
                    help="with --cube: stop a game at the cubeful exact bearoff table for K checkers a side (1..8) "
                         "and score it with its exact cubeful expectation; not with --luck, --bearoff, --bearoff1 "
                         "or --truncate")
    ap.add_argument("--cube-truncate", type=int, default=None, metavar="N",
                    help="with --cube: stop a game after N plies (>= 1) and score it with Janowski's cube-life "
                         "equity from a net's value head; goes with --cube-bearoff; not with --luck, --bearoff, "
                         "--bearoff1 or --truncate")
    ap.add_argument("--cube-life", type=float, default=0.68, metavar="X",
                    help="the cube life in [0, 1]: 0 scores the cubeless equity, 1 the fully live cube's")
    ap.add_argument("--cube-win-value", type=float, default=1.0, metavar="W",
                    help="mean points of a won game in [1, 3] (from a cubeless rollout's gammon rates)")
    ap.add_argument("--cube-loss-value", type=float, default=1.0, metavar="L",
                    help="mean points of a lost game in [1, 3]")
    ap.add_argument("--cube-truncate-scale", type=float, default=1.0, metavar="S",
                    help="points per unit of the net's value")
    ap.add_argument("--cube-truncate-lookahead", type=int, default=0, choices=(0, 1),
                    help="0: the value head on the position itself (sync-free); 1: its mean best 1-ply value "
                         "over the 21 rolls")
    ap.add_argument("--cube-truncate-net", default=None, metavar="PATH",
                    help="the state_dict whose value head scores the truncated games (default: --cube-net if "
                         "given, else the player's net)")
    ap.add_argument("--cube-luck", action="store_true",
                    help="with --cube: the luck-adjusted (variance-reduced) cubeful estimate, the luck of a roll "
                         "being Janowski's cube-life equity after it minus its mean over the 21 rolls; needs weights; "
                         "not with --luck, --bearoff, --bearoff1, --truncate, --cube-bearoff or --cube-truncate")
    ap.add_argument("--cube-luck-net", default=None, metavar="PATH",
                    help="the state_dict whose value head measures the luck (default: --cube-net if given, else "
                         "the player's net)")
    ap.add_argument("--cube-luck-scale", type=_cube_luck_scale, default="fit",
                    help="'fit' (the control-variate coefficient of the games) or a fixed number")
    ap.add_argument("--cube-luck-life", type=float, default=0.68, metavar="X",
                    help="the cube life of the luck's equity in [0, 1]: 0 is the cubeless luck times the cube")
    ap.add_argument("--cube-luck-win-value", type=float, default=1.0, metavar="W",
                    help="mean points of a won game in [1, 3]")
    ap.add_argument("--cube-luck-loss-value", type=float, default=1.0, metavar="L",
                    help="mean points of a lost game in [1, 3]")
    ap.add_argument("--cube-luck-value-scale", type=float, default=1.0, metavar="S",
                    help="points per unit of the net's value")
    ap.add_argument("--cube-decision", action="store_true",
                    help="per position: no double / double, take / double, pass for the side on roll with a "
                         "centred cube, and the verdict")
    from .arena import _gammon_shares
    ap.add_argument("--match", type=int, default=None, metavar="N",
                    help="roll the positions out at a score of a match to N points (1..25): the result is the mover's "
                         "match-winning chance on a match equity table; needs --match-score; not with --cube, --luck, "
                         "a bearoff cut or --truncate")
    ap.add_argument("--match-score", type=_int_pair("--match-score"), default=None, metavar="A1,A2",
                    help="the points PLAYER1 and PLAYER2 still need, each in 1..N")
    ap.add_argument("--match-crawford", type=int, default=None, choices=(0, 1, 2),
                    help="0 before the Crawford game (default), 1 the Crawford game, 2 after it")
    ap.add_argument("--met", default=None, metavar="FILE",
                    help="the match equity table, JSON {length, met, post_crawford} (match.load_met; its length must "
                         "be N; default: match.met_table(N), a cubeless-play table)")
    ap.add_argument("--match-window", type=float, default=None,
                    help="the side on roll doubles from this share of the way between the dead-cube doubling point (0) "
                         "and the cash point (1) on (default 0.65)")
    ap.add_argument("--match-gammons", type=_gammon_shares, default=None, metavar="W,L",
                    help="the share of the side on roll's wins and of its losses that are gammons (default 0.25,0.25)")
    ap.add_argument("--match-lookahead", type=int, default=None, choices=(0, 1),
                    help="0: the value head on the position itself (sync-free); 1 (default): its mean best 1-ply value "
                         "over the 21 rolls")
    ap.add_argument("--match-net", default=None, metavar="PATH",
                    help="the state_dict whose value head makes the cube decisions (default: the player's net)")
    ap.add_argument("--match-scale", type=float, default=None, help="points per unit of the net's value (default 1)")
    ap.add_argument("--match-cube", type=_int_pair("--match-cube"), default=None, metavar="K,OWNER",
                    help="the cube every game starts with: 2^K, OWNER 0 centred, 1 PLAYER1, 2 PLAYER2 (default 0,0)")
    ap.add_argument("--match-decision", action="store_true",
                    help="per position: no double / double, take / double, pass for the side on roll in "
                         "match-winning chance, and the verdict")
    return ap


def match_from_args(args, net, device):
    """The match.RolloutMatch of a parsed command line (None without --match): a MatchRule on
    --match-net, else on the player's net; without either no rule (nobody doubles)."""
    if args.match is None:
        return None
    from .match import MatchRule, RolloutMatch, load_met
    from .search import ValueHead
    met = None
    if args.met is not None:
        length, *met = load_met(args.met)
        if length != args.match:
            raise ValueError(f"--met {args.met} is a table for matches to {length}, --match asks for {args.match}")
    vnet = net if args.match_net is None else load_net(args.match_net, device)
    rule = None
    if vnet is not None:
        w, l = args.match_gammons
        rule = MatchRule(ValueHead(vnet), scale=args.match_scale, window=args.match_window, win_gammons=w,
                         loss_gammons=l, lookahead=args.match_lookahead)
    return RolloutMatch(args.match, rule, met=met)


def main(argv=None):
    import time
    args = build_parser().parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    net = None if args.net == "random" else load_net(args.net, dev)
    max_moves = min(net.action_head.out_features, 500) if net is not None else 500
    player = make_player(args.player, net, seed=args.seed * 2 + 1, top_k=args.top_k)
    positions = load_positions(args.positions)
    ro = Rollout(args.batch, seed=args.seed, max_moves=max_moves, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    vh = None
    if args.luck:
        from .search import ValueHead
        vh = ValueHead(net)
    dbs, dbs1 = {}, {}
    if any(k is not None for k in (args.bearoff, args.bearoff_play, args.bearoff1, args.bearoff1_play)):
        from .bearoff import BearoffDB, BearoffPlayer, OneSidedBearoffDB, OneSidedPlayer
        for k in {args.bearoff, args.bearoff_play} - {None}:
            dbs[k] = BearoffDB(k, device=dev)
        for k in {args.bearoff1, args.bearoff1_play} - {None}:
            dbs1[k] = OneSidedBearoffDB(k, device=dev)
        if args.bearoff1_play is not None:
            player = OneSidedPlayer(player, dbs1[args.bearoff1_play])
        if args.bearoff_play is not None:               # outside: the exact table where it reaches
            player = BearoffPlayer(player, dbs[args.bearoff_play])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()                        # the table's build is not the rollout's time
    rule = None
    if args.cube:
        from .cube import CubeRule, rollout_cube_decision
        from .search import ValueHead
        rule = CubeRule(ValueHead(net if args.cube_net is None else load_net(args.cube_net, dev)),
                        scale=args.cube_scale, double_at=args.cube_double, pass_at=args.cube_pass,
                        too_good_at=args.cube_too_good, cap=args.cube_cap, jacoby=args.jacoby)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    cdb = None
    if args.cube_bearoff is not None:
        from .bearoff import BearoffDB, CubefulBearoffDB
        cdb = CubefulBearoffDB(dbs.get(args.cube_bearoff) or BearoffDB(args.cube_bearoff, device=dev))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()                        # the table's build is not the rollout's time
    trunc = None
    if args.truncate is not None:
        from .search import ValueHead
        trunc = Truncation(ValueHead(net if args.truncate_net is None else load_net(args.truncate_net, dev)),
                           args.truncate, scale=args.truncate_scale, lookahead=args.truncate_lookahead)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    ctrunc = None
    if args.cube_truncate is not None:
        from .cube import CubeLife, CubeTruncation
        from .search import ValueHead
        cnet = args.cube_truncate_net if args.cube_truncate_net is not None else args.cube_net
        ctrunc = CubeTruncation(ValueHead(net if cnet is None else load_net(cnet, dev)), args.cube_truncate,
                                scale=args.cube_truncate_scale, lookahead=args.cube_truncate_lookahead,
                                life=CubeLife(args.cube_life, args.cube_win_value, args.cube_loss_value))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    cluck = None
    if args.cube_luck:
        from .cube import CubeLife, CubeLuck
        from .search import ValueHead
        lnet = args.cube_luck_net if args.cube_luck_net is not None else args.cube_net
        cluck = CubeLuck(ValueHead(net if lnet is None else load_net(lnet, dev)), scale=args.cube_luck_value_scale,
                         life=CubeLife(args.cube_luck_life, args.cube_luck_win_value, args.cube_luck_loss_value))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    match = match_from_args(args, net, dev)
    if match is not None:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    if args.match_decision:
        from .match import rollout_match_decision
        res = []
        for i in range(positions.shape[0]):
            d = rollout_match_decision(ro, player, positions[i], args.trials, match, args.match_score,
                                       crawford=args.match_crawford, cube=args.match_cube, first_roll=args.first_roll,
                                       max_steps=args.max_steps)
            print(json.dumps(dict(position=i, match_decision=True, **d)), flush=True)
            res.extend(d["rollouts"])
    elif match is not None:
        res = ro.run(player, positions, args.trials, first_roll=args.first_roll, max_steps=args.max_steps, match=match,
                     match_away=args.match_score, match_crawford=args.match_crawford, cube_start=args.match_cube)
    elif args.cube_decision:
        # one line per position: the three equities and the verdict; the summary counts both rollouts' games
        res = []
        for i in range(positions.shape[0]):
            d = rollout_cube_decision(ro, player, positions[i], args.trials, rule, first_roll=args.first_roll,
                                      max_steps=args.max_steps, cube_bearoff=cdb, cube_truncate=ctrunc,
                                      cube_luck=cluck, cube_luck_scale=args.cube_luck_scale)
            print(json.dumps(dict(position=i, cube_decision=True, **d)), flush=True)
            res.extend(d["rollouts"])
    else:
        res = ro.run(player, positions, args.trials, first_roll=args.first_roll, max_steps=args.max_steps, luck=vh,
                     luck_scale=args.luck_scale, bearoff=dbs.get(args.bearoff) or dbs1.get(args.bearoff1), cube=rule,
                     truncate=trunc, cube_bearoff=cdb, cube_truncate=ctrunc, cube_luck=cluck,
                     cube_luck_scale=args.cube_luck_scale)
    dt = time.perf_counter() - t0
    for i, r in enumerate(res if not (args.cube_decision or args.match_decision) else ()):
        print(json.dumps(dict(position=i, **r)), flush=True)
    games = sum(r["games"] for r in res)
    summary = dict(summary=True, positions=int(positions.shape[0]), games=games, unfinished=sum(r["unfinished"] for r in res),
                   steps=ro.steps, net=args.net, player="random" if net is None else args.player, top_k=args.top_k,
                   trials=args.trials, first_roll=args.first_roll, batch=args.batch, max_steps=args.max_steps,
                   seed=args.seed, seconds=dt, games_per_s=games / dt if dt > 0 else 0.0,
                   env_steps_per_s=ro.steps * args.batch / dt if dt > 0 else 0.0)
    if args.luck:
        summary.update(luck=True, luck_scale=args.luck_scale)
    if dbs or dbs1:
        cut = sum(r.get("cut_games", 0) for r in res)
        if dbs1:
            summary.update(bearoff1=args.bearoff1, bearoff1_play=args.bearoff1_play)
        summary.update(bearoff=args.bearoff, bearoff_play=args.bearoff_play, cut_games=cut,
                       cut_share=cut / games if games else 0.0,
                       plies_per_game=sum(r["plies_per_game"] * r["games"] for r in res) / games if games else 0.0)
    if args.cube:
        summary.update(cube=True, cube_net=args.cube_net, cube_double=args.cube_double, cube_pass=args.cube_pass,
                       cube_too_good=args.cube_too_good if math.isfinite(args.cube_too_good) else None,
                       cube_scale=args.cube_scale, cube_cap=args.cube_cap, jacoby=args.jacoby,
                       cube_decision=args.cube_decision,
                       pass_share=sum(r["pass_games"] for r in res) / games if games else 0.0,
                       doubles_per_game=sum(r["doubles"] for r in res) / games if games else 0.0,
                       plies_per_game=sum(r["plies_per_game"] * r["games"] for r in res) / games if games else 0.0)
    if cdb is not None:
        cut = sum(r["cut_games"] for r in res)
        summary.update(cube_bearoff=args.cube_bearoff, bearoff_kind=cdb.kind, cut_games=cut,
                       cut_share=cut / games if games else 0.0)
    if trunc is not None:
        tg = sum(r["truncated_games"] for r in res)
        summary.update(truncate=args.truncate, truncate_scale=args.truncate_scale,
                       truncate_lookahead=args.truncate_lookahead, truncate_net=args.truncate_net,
                       truncated_games=tg, truncated_share=tg / games if games else 0.0,
                       plies_per_game=sum(r["plies_per_game"] * r["games"] for r in res) / games if games else 0.0)
    if ctrunc is not None:
        tg = sum(r["truncated_games"] for r in res)
        summary.update(cube_truncate=args.cube_truncate, cube_life=args.cube_life, cube_win_value=args.cube_win_value,
                       cube_loss_value=args.cube_loss_value, cube_truncate_scale=args.cube_truncate_scale,
                       cube_truncate_lookahead=args.cube_truncate_lookahead, cube_truncate_net=args.cube_truncate_net,
                       truncated_games=tg, truncated_share=tg / games if games else 0.0)
    if cluck is not None:
        summary.update(cube_luck=True, cube_luck_net=args.cube_luck_net, cube_luck_scale=args.cube_luck_scale,
                       cube_luck_life=args.cube_luck_life, cube_luck_win_value=args.cube_luck_win_value,
                       cube_luck_loss_value=args.cube_luck_loss_value, cube_luck_value_scale=args.cube_luck_value_scale)
    if match is not None:
        summary.update(match=args.match, match_score=list(args.match_score), match_crawford=args.match_crawford,
                       met=args.met, match_cube=list(args.match_cube), match_decision=args.match_decision,
                       match_rule=match.has_rule, match_net=args.match_net, match_window=args.match_window,
                       match_gammons=list(args.match_gammons), match_lookahead=args.match_lookahead,
                       match_scale=args.match_scale,
                       pass_share=sum(r["pass_games"] for r in res) / games if games else 0.0)
    print(json.dumps(summary), flush=True)
    return res, summary


if __name__ == "__main__":
    main()
