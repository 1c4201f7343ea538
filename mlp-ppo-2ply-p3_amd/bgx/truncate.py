"""Truncated position rollouts (csrc/bg_trunc.h; rollout.run_lanes drives it): a
game that has run `plies` plies without ending stops there and is scored with a value of the
position it reached -- the value head itself (lookahead 0, bgx_value_lanes), the head's mean
best 1-ply value over the 21 rolls (lookahead 1, bgx_roll_luck's mean), or any callable.  A
short horizon makes the slow players affordable; the estimate is then biased by the value's
error, which the standard error does not show.  Together with the luck adjustment the dice
noise of the plies that were played goes as well."""
from __future__ import annotations

import math

import numpy as np
import torch

from .replay import LaneReplay, luck_q
from .tally import (LUCK_FIELDS, TRUNC_CLAMP, TRUNC_FIELDS, TRUNC_ONE, summarize_truncated,  # noqa: F401
                    summarize_truncated_luck)

LOOKAHEADS = (0, 1)


class Truncation:
    """Stop every game after `plies` plies (>= 1) and score it with `value`, the equity of the
    side on roll at the position reached, before its roll: a search.ValueHead -- `lookahead` 0:
    the head's own output for the position (bgx_value_lanes; sync-free), `lookahead` 1: the
    mean over the 21 rolls of the mover's best 1-ply value (bgx_roll_luck's mean, the cube's
    equity; it synchronises) -- or a callable f(eng, tsel) -> contiguous float32[B] on the
    engine's device (entries off tsel are ignored; for tests, or a table as value).  `scale`
    turns the value's unit into points, as CubeRule.scale does; the result is clamped to +-3
    points and a NaN counts 0.  Like the cube's rule it presumes a mover's-view value."""

    def __init__(self, value, plies: int, scale: float = 1.0, lookahead: int = 0):
        from .search import ValueHead
        if not isinstance(value, ValueHead) and not callable(value):
            raise ValueError("Truncation: value must be a search.ValueHead or a callable f(eng, tsel)")
        if isinstance(plies, bool) or int(plies) != plies or int(plies) < 1 or int(plies) > 2 ** 31 - 1:
            raise ValueError(f"Truncation: plies must be an integer >= 1, got {plies!r}")
        if math.isnan(float(scale)):
            raise ValueError("Truncation: scale is NaN")
        if isinstance(lookahead, bool) or lookahead not in LOOKAHEADS:
            raise ValueError(f"Truncation: lookahead must be one of {LOOKAHEADS}, got {lookahead!r}")
        self.value, self.is_head = value, isinstance(value, ValueHead)
        self.plies, self.scale, self.lookahead = int(plies), float(scale), int(lookahead)
        # never waits for the device: the rollout loop may read its active-lane count rarely
        self.sync_free = self.is_head and self.lookahead == 0
        self.totals = {"calls": 0}

    def equity(self, eng, tsel: torch.Tensor, scratch: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The mover's value on the tsel lanes, float32[B] on the engine's device."""
        self.totals["calls"] += 1
        if self.is_head and self.lookahead == 0:
            from .search import value_lanes
            return value_lanes(eng, self.value, sel=tsel, out=out)
        if self.is_head:
            from .search import roll_luck
            roll_luck(eng, self.value, sel=tsel, out=(scratch, out))
            return out
        v = self.value(eng, tsel)
        if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != eng.device
                or not v.is_contiguous() or v.numel() != eng.batch):
            raise ValueError("a truncation's value must return a contiguous float32[B] tensor on the engine's device")
        return v


def value_q(scale: float, value, same) -> np.ndarray:
    """Part 1 of csrc/bg_trunc.h in numpy: e = fp32(scale * v), 0 for a NaN, clamped to +-3;
    y = e where `same` (the side on roll is the start mover) else -e; Vq = rint(fp32(y * 2^16))
    (round half even) as int64."""
    v = np.asarray(value, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (np.float32(scale) * v).astype(np.float32)
    e = np.where(np.isnan(e), np.float32(0), np.minimum(np.maximum(e, np.float32(-TRUNC_CLAMP)), np.float32(TRUNC_CLAMP)))
    y = np.where(np.asarray(same, bool), e, -e).astype(np.float32)
    return np.rint((y * np.float32(TRUNC_ONE)).astype(np.float32)).astype(np.int64)


def truncate_reference(trace, starts, group, n_groups: int, games_per_lane: int, truncation) -> dict:
    """A traced truncated run replayed on the host in numpy, with the arithmetic of
    bgx_rollout_advance, bgx_rollout_trunc_sel / bgx_rollout_trunc_cut and, when the trace has
    `luck`, bgx_rollout_luck_add / bgx_rollout_luck_flush (include/bgx.h).  `trace`: run_lanes'
    trace of a run with truncate= (per step [steps, B]: mover, done, info, trunc_value,
    trunc_mover and, with luck=, luck); `starts` uint8[B, 64]; `group` int32[B]; `truncation`
    gives plies and scale.  Per step: the selected lanes' luck is added, finished games are
    counted (and their luck flushed), then a selected lane whose game has run `plies` plies is
    truncated at value_q(scale, trunc_value, trunc_mover == the start mover).  Returns
    dict(tally int64[P, 8], trunc_tally int64[P, 7], luck_tally int64[P, 4] or None,
    games_done int64[B], active int, trunc bool[steps, B])."""
    def host(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    mover, done, info = host(trace["mover"]), host(trace["done"]), host(trace["info"])
    tval, tmover = host(trace["trunc_value"]).astype(np.float32), host(trace["trunc_mover"])
    luck = host(trace["luck"]).astype(np.float32) if "luck" in trace else None
    rp = LaneReplay(host(starts), host(group), n_groups, games_per_lane)
    rp.tally("trunc_tally", TRUNC_FIELDS)
    if luck is not None:
        rp.tally("luck_tally", LUCK_FIELDS)
    cuts = np.zeros(done.shape, bool)
    for t in range(done.shape[0]):
        if luck is not None:
            rp.luck_add(luck[t], mover[t])
        rp.advance(done[t], info[t])
        cuts[t] = rp.horizon(truncation.plies)
        vq = value_q(truncation.scale, tval[t], tmover[t] == rp.start_cur)
        lq = luck_q(rp.luck) if luck is not None else np.zeros(rp.B, np.int64)
        rp.cut("trunc_tally", cuts[t], (vq, vq * vq, lq, lq * lq, vq * lq))
    return dict(rp.tallies, luck_tally=rp.tallies.get("luck_tally"), games_done=rp.games, active=rp.active, trunc=cuts)
