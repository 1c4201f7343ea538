"""The doubling cube in position rollouts, money play (the device side is
csrc/bg_cube.h, the four bgx_rollout_cube_* entry points of include/bgx.h; bgx/rollout.py runs
them in its loop).  A game is worth its cubeless 1 / 2 / 3 points times the cube, 2^k; the side
on roll may double before it rolls when the cube is centred or its own, the opponent takes
(k + 1, the cube is now the taker's) or passes (the game ends at 2^k).  Both decisions follow one
threshold rule, CubeRule, on the mover's equity before the roll.  Where a game enters the cubeful
exact bearoff table (bearoff.CubefulBearoffDB) it can be cut and scored with its
exact cubeful expectation instead (cube_bearoff=; summarize_cube_bearoff).  A cubeful game can
also stop at a horizon and count Janowski's cube-life equity of the position reached, formed from
a net's cubeless value (cube_truncate= a CubeTruncation; CubeLife; summarize_cube_truncated;
DESIGN.md §17; csrc/bg_cube_trunc.h); static_cube_decision is the same rule per lane with no
rollout, janowski_points its decision points.  The luck adjustment of cubeful games (cube_luck= a
CubeLuck; summarize_cube_luck; csrc/bg_cube_luck.h) takes the dice noise out of the
cubeful estimate: the luck of a roll is Janowski's equity after it minus its mean over the 21 rolls.

    python -m bgx.rollout --net ckpt.pt --player 1ply --positions opening --trials 1296 --cube
    python -m bgx.rollout --net ckpt.pt --player 1ply --positions pos.json --cube --cube-decision
    python -m bgx.rollout --net ckpt.pt --player 2ply --top-k 4 --positions pos.json --cube --cube-decision \\
        --cube-truncate 8 --cube-life 0.68
    python -m bgx.rollout --net ckpt.pt --player 2ply --top-k 4 --positions pos.json --cube --cube-decision --cube-luck
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .replay import R_CUR, LaneReplay, split_sq
from .tally import (CUBE_CUT_FIELDS, CUBE_CUT_ONE, CUBE_CUT_SPLIT, CUBE_FIELDS, CUBE_LUCK_FIELDS,  # noqa: F401
                    CUBE_TRUNC_FIELDS, CUBE_TRUNC_ONE, summarize_cube, summarize_cube_bearoff, summarize_cube_luck,
                    summarize_cube_truncated)
from .truncate import Truncation

MAX_CAP = 10
CENTRED = 0                         # the owner field: 0 centred, 1 PLAYER1, 2 PLAYER2


def pack(k: int, owner: int) -> int:
    """The cube's state byte: k in bits 0-3 (the cube shows 2^k), the owner in bits 4-5."""
    return int(k) | (int(owner) << 4)


def unpack(byte):
    """(k, owner) of state bytes (an int or an array)."""
    b = np.asarray(byte).astype(np.int64)
    return b & 15, (b >> 4) & 3


def sanitise(byte, cap: int):
    """The byte as the kernels read it: k as min(k, cap), owner 3 as 0."""
    k, o = unpack(byte)
    return (np.minimum(k, int(cap)) | (np.where(o == 3, 0, o) << 4)).astype(np.uint8)


def validate_cube0(cube0: torch.Tensor, cap: int) -> None:
    """ValueError naming the first lane whose byte is not a cube state: k <= cap, owner <= 2 and
    owner == 0 exactly when k == 0 (torch ops: the bytes stay where they are)."""
    c = cube0.to(torch.int32)
    k, o = c & 15, c >> 4
    bad = (k > int(cap)) | (o > 2) | ((o == 0) != (k == 0))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0, 0])
        raise ValueError(f"cube0: lane {i} holds {int(c[i])} (k {int(k[i])}, owner {int(o[i])}): need k <= cap = "
                         f"{int(cap)}, owner <= 2 and owner == 0 exactly when k == 0")


class CubeRule:
    """The threshold rule of both cube decisions.  With e = scale * equity, equity the mover's own
    equity before its roll: the mover doubles iff double_at <= e <= too_good_at, the opponent
    passes iff e > pass_at and takes otherwise.  `pass_at` = 0.5 is the dead-cube take point:
    taking at stakes 2 costs 2 e, passing costs 1.  `double_at` is a parameter of the rule, not a
    claim about the best window.  `cap`: no double once the cube shows 2^cap (0..10).  `jacoby`:
    a game that ends with the cube still centred at 1 counts 1 point, gammon or not.

    `value` gives the equity: a search.ValueHead -- equity = roll_luck's mean on the lanes that
    may double, the mover's expected best 1-ply value over the 21 rolls, taken without a look at
    the roll the lane holds -- or a callable f(eng, dsel) -> contiguous float32[B] on the
    engine's device with the mover's equity (entries off dsel are ignored).  `scale` plays the
    part of the luck adjustment's c: it turns the value's unit into points.  The rule presumes a
    mover's-view value (positive = good for the side on roll), which is what `--returns selfplay`
    trains; a net trained on another target gives decisions that mean nothing.

    `lookahead` (a ValueHead's only): 1, the default, is the roll_luck mean above, which
    synchronises the host on every call; 0 is the head's own output for the position, the mover's
    static value (bgx_value_lanes on the selected lanes: sync-free and graph-capturable).
    `sync_free`: the equity never waits for the device -- a head with lookahead 0, or a callable
    that declares it (its own attribute sync_free)."""

    def __init__(self, value, scale: float = 1.0, double_at: float = 0.40, pass_at: float = 0.50,
                 too_good_at: float = math.inf, cap: int = 6, jacoby: bool = False, lookahead: int = 1):
        from .search import ValueHead
        if not isinstance(value, ValueHead) and not callable(value):
            raise ValueError("CubeRule: value must be a search.ValueHead or a callable f(eng, dsel)")
        for name, v in (("scale", scale), ("double_at", double_at), ("pass_at", pass_at), ("too_good_at", too_good_at)):
            if math.isnan(float(v)):
                raise ValueError(f"CubeRule: {name} is NaN")
        if int(cap) != cap or not 0 <= int(cap) <= MAX_CAP:
            raise ValueError(f"CubeRule: cap must be in 0..{MAX_CAP}, got {cap!r}")
        if isinstance(lookahead, bool) or lookahead not in (0, 1):
            raise ValueError(f"CubeRule: lookahead must be 0 or 1, got {lookahead!r}")
        self.value, self.is_head = value, isinstance(value, ValueHead)
        self.lookahead = int(lookahead)
        self.sync_free = self.lookahead == 0 if self.is_head else bool(getattr(value, "sync_free", False))
        self.scale, self.double_at, self.pass_at = float(scale), float(double_at), float(pass_at)
        self.too_good_at, self.cap, self.jacoby = float(too_good_at), int(cap), bool(jacoby)
        # equity calls so far and, with a value head, the lanes they covered (rows) and the leaves
        self.totals = {"calls": 0, "rows": 0, "leaves": 0}

    def struct(self) -> _lib.BgxCubeRule:
        return _lib.BgxCubeRule(self.scale, self.double_at, self.pass_at, self.too_good_at, self.cap, int(self.jacoby))

    def equity(self, eng, dsel: torch.Tensor, scratch: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The mover's equity on the dsel lanes, float32[B] on the engine's device."""
        self.totals["calls"] += 1
        if self.is_head and self.lookahead == 0:
            from .search import value_lanes
            return value_lanes(eng, self.value, sel=dsel, out=out)
        if self.is_head:
            from .search import roll_luck
            stats = roll_luck(eng, self.value, sel=dsel, out=(scratch, out))[2]
            self.totals["rows"] += stats["rows"]
            self.totals["leaves"] += stats["leaves"]
            return out
        e = self.value(eng, dsel)
        if (not isinstance(e, torch.Tensor) or e.dtype != torch.float32 or e.device != eng.device
                or not e.is_contiguous() or e.numel() != eng.batch):
            raise ValueError("a cube rule's value must return a contiguous float32[B] tensor on the engine's device")
        return e


def cube_bearoff_cut_reference(records, cube, plies, games_done, sel, starts, group, n_groups: int,
                               games_per_lane: int, cap: int, cube0, lookup) -> dict:
    """One call of bgx_rollout_cube_bearoff_cut on the host (include/bgx.h), state in, state out.
    `lookup`: records uint8[B, 64], cube uint8[B], cap -> (in_db bool[B], values f32[B, 4], flags),
    e.g. bearoff.cube_lookup_reference on a table.  A selected lane with a valid group whose record
    is in the table adds Yq = bearoff.cube_fixed_reference(nd on its first ply, else e; signed for
    the start mover; k of its cube) to its row, counts the game and gets its starting cube back.
    Returns dict(cut_tally int64[P, 6], mask bool[B], games_done, plies, sel uint8[B], cube
    uint8[B], retired int = the lanes that finished their last game)."""
    rp = LaneReplay(starts, group, n_groups, games_per_lane, cap=cap, c0=sanitise(np.asarray(cube0), cap))
    rp.tally("cut_tally", CUBE_CUT_FIELDS)
    rp.cube = np.asarray(cube).astype(np.uint8).copy()
    rp.plies, rp.games = np.asarray(plies).astype(np.int64).copy(), np.asarray(games_done).astype(np.int64).copy()
    sel = np.asarray(sel).astype(np.uint8).copy()
    m = _table_cut(rp, np.asarray(records), lookup, sel != 0)
    retired = m & (rp.games >= rp.G)
    sel[retired] = 0
    return dict(cut_tally=rp.tallies["cut_tally"], mask=m, games_done=rp.games, plies=rp.plies, sel=sel, cube=rp.cube,
                retired=int(retired.sum()))


def _table_cut(rp: LaneReplay, records, lookup, sel):
    """The cubeful table cut on the replay's state: the `sel` lanes with a valid group whose record
    is in the table are scored, counted and get their starting cube back.  Returns their mask."""
    from .bearoff import cube_fixed_reference
    in_db, values, _ = lookup(records, rp.cube, rp.cap)
    m = sel & rp.valid & np.asarray(in_db, bool)
    k = rp.cube_k()
    v = np.where(rp.plies == 0, values[:, 0], values[:, 2]).astype(np.float32)
    yq = cube_fixed_reference(np.where(m, v, np.float32(0)), records[:, R_CUR] == rp.start_cur, k)
    rp.cut("cut_tally", m, (yq, *split_sq(yq), k), cube=True)
    return m


def decide_reference(cube, mover, equity, rule: CubeRule):
    """cube_decision of csrc/bg_cube.h on arrays: (action int[B]: 0 none, 1 take, 2 pass; next
    uint8[B]; access bool[B] = cube_access), without the lane selection."""
    cube, mover = np.asarray(cube), np.asarray(mover).astype(np.int64) & 1
    cap = rule.cap
    c = sanitise(cube, cap)
    k, o = unpack(c)
    access = (k < cap) & ((o == 0) | (o == mover + 1))
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        e = (f(rule.scale) * np.asarray(equity, f)).astype(f)
        dbl = access & (e >= f(rule.double_at)) & (e <= f(rule.too_good_at))
        pas = dbl & (e > f(rule.pass_at))
    take = dbl & ~pas
    nxt = np.where(take, (k + 1) | ((2 - mover) << 4), c).astype(np.uint8)
    return np.where(pas, 2, np.where(take, 1, 0)), nxt, access


def cube_reference(trace, starts, group, n_groups: int, games_per_lane: int, rule: CubeRule, cube0=None,
                   cut_lookup=None, cube_truncate=None, cube_luck: bool = False) -> dict:
    """A traced cube run replayed on the host with the kernels' arithmetic (include/bgx.h
    bgx_rollout_cube_*).  `trace`: run_lanes' with cube_mover, cube_equity, done and info
    [steps, B]; the lane records are taken as not game_over, which holds between the steps of an
    auto-reset engine.  Returns dict(cube_tally int64[P, 8], tally int64[P, 8], cube uint8[steps,
    B] = the states before each decision, dsel / mask bool[steps, B], games_done int64[B],
    active int).  `cut_lookup` (cube_bearoff_cut_reference's `lookup`): the run was cut at the
    cubeful bearoff table (run_lanes' cube_bearoff=) -- the cut is replayed after begin on the
    trace's cut_records0 and after every step on cut_records[t]; the result gains cut_tally
    int64[P, 6], cut0 bool[B] and cut bool[steps, B].  `cube_truncate`: cube_trunc_reference.
    `cube_luck`: cube_luck_reference."""
    def host(x):
        return np.asarray(torch.as_tensor(x).cpu())
    mover, equity = host(trace["cube_mover"]), host(trace["cube_equity"]).astype(np.float32)
    done, info = host(trace["done"]), host(trace["info"])
    cap = rule.cap
    B = host(group).shape[0]
    c0 = np.zeros(B, np.uint8) if cube0 is None else sanitise(host(cube0), cap)
    rp = LaneReplay(host(starts), host(group), n_groups, games_per_lane, cap=cap, c0=c0, jacoby=rule.jacoby)
    rp.tally("cube_tally", CUBE_FIELDS)
    T = done.shape[0]
    states, dsels, masks = np.zeros((T, B), np.uint8), np.zeros((T, B), bool), np.zeros((T, B), bool)
    if cut_lookup is not None:
        rp.tally("cut_tally", CUBE_CUT_FIELDS)
        cuts = np.zeros((T, B), bool)
        cut0 = _table_cut(rp, host(trace["cut_records0"]), cut_lookup, rp.sel)
    if cube_luck:
        rp.tally("cube_luck_tally", CUBE_LUCK_FIELDS)
        lk, lmover = host(trace["cube_luck"]).astype(np.float32), host(trace["cube_luck_mover"])
        lstates, lsels = np.zeros((T, B), np.uint8), np.zeros((T, B), bool)
    if cube_truncate is not None:
        rp.tally("cube_trunc_tally", CUBE_TRUNC_FIELDS)
        tval, tmover = host(trace["ctrunc_value"]).astype(np.float32), host(trace["ctrunc_mover"])
        tcuts, tstates = np.zeros((T, B), bool), np.zeros((T, B), np.uint8)
    for t in range(T):
        states[t] = rp.cube
        dsels[t], masks[t] = rp.decide(mover[t], *decide_reference(rp.cube, mover[t], equity[t], rule))
        if cube_luck:
            lstates[t], lsels[t] = rp.cube, rp.sel
            rp.cube_luck_add(lk[t], lmover[t])
        rp.advance(done[t], info[t])
        if cut_lookup is not None:
            cuts[t] = _table_cut(rp, host(trace["cut_records"][t]), cut_lookup, rp.sel)
        if cube_truncate is not None:
            # the truncation, after advance and the table cut (whose lanes have plies 0)
            tc, k = rp.horizon(cube_truncate.plies), rp.cube_k()
            tcuts[t], tstates[t] = tc, rp.cube
            values, _ = janowski_reference(np.where(tc, tval[t], np.float32(0)), rp.cube, tmover[t], cube_truncate.scale,
                                           cube_truncate.life, cap, rule.jacoby)
            yq = cube_trunc_fixed_reference(values[:, 2], tmover[t] == rp.start_cur, k)
            rp.cut("cube_trunc_tally", tc, (yq, *split_sq(yq), k), cube=True)
    out = dict(rp.tallies, cube=states, dsel=dsels, mask=masks, games_done=rp.games, active=rp.active)
    if cut_lookup is not None:
        out.update(cut0=cut0, cut=cuts)
    if cube_truncate is not None:
        out.update(ctrunc=tcuts, ctrunc_cube=tstates)
    if cube_luck:
        out.update(cube_luck_state=lstates, cube_luck_sel=lsels, lane_luck=rp.luck)
    return out


def rollout_cube_decision(rollout, player, record, trials: int, rule: CubeRule, cube=(0, CENTRED),
                          first_roll: str = "stratified", max_steps: int = 4000, cube_bearoff=None,
                          cube_truncate=None, cube_luck=None, cube_luck_scale="fit") -> dict:
    """"Double or not, take or pass?" for the side on roll in `record` (uint8[64]: board and
    mover), holding the cube `cube` = (k, owner) with access to it.  The position is rolled out
    twice in one run, as two groups over the same start records: "no double", with the cube as
    given, and "double, take", with k + 1 owned by the opponent.  No cube action happens on a
    game's first ply, so both start after the decision asked about.  Returns `no_double`,
    `double_take` and `double_pass` = +1, the mover's equities in units of the current cube 2^k,
    each with its `_stderr`, the two rollouts' summaries (`rollouts`), and the verdict: `double`
    iff min(double_take, 1) > no_double, `take` iff double_take <= 1.  `cube_bearoff` (a
    bearoff.CubefulBearoffDB): both rollouts are cut at the cubeful table
    (Rollout.run); for a position in the table that is the exact answer, the table's nd and DT at
    the cut's 2^-20 resolution, with standard errors of 0.  `cube_truncate` (a CubeTruncation;
    DESIGN.md §17): both rollouts are truncated at its horizon and scored by Janowski's rule.
    `cube_luck` (a CubeLuck), with `cube_luck_scale` (Rollout.run): both rollouts are
    luck-adjusted; the result gains `no_double_luck` and `double_take_luck` with their `_stderr`,
    from the adjusted equities, and `double_luck` / `take_luck`, the verdict by them.  The
    existing keys keep their meaning: they are the raw estimates of the same games."""
    rec = torch.as_tensor(record).reshape(-1)
    if rec.numel() != 64 or rec.dtype != torch.uint8:
        raise ValueError("rollout_cube_decision: record must be 64 bytes (uint8)")
    k, owner = int(cube[0]), int(cube[1])
    mover = int(rec[52]) & 1
    if not 0 <= k < rule.cap or owner not in (0, mover + 1) or (owner == 0) != (k == 0):
        raise ValueError(f"rollout_cube_decision: cube {(k, owner)} gives the mover (PLAYER{mover + 1}) no double below "
                         f"the cap {rule.cap}")
    pos = torch.stack([rec.cpu(), rec.cpu()])
    res = rollout.run(player, pos, trials, first_roll=first_roll, max_steps=max_steps, cube=rule,
                      cube_start=[(k, owner), (k + 1, 2 - mover)], cube_bearoff=cube_bearoff,
                      cube_truncate=cube_truncate, cube_luck=cube_luck, cube_luck_scale=cube_luck_scale)
    unit = float(1 << k)
    nd, dt = res[0]["equity_cubeful"] / unit, res[1]["equity_cubeful"] / unit
    adjusted = {}
    if cube_luck is not None:
        ndl, dtl = res[0]["equity_cubeful_luck"] / unit, res[1]["equity_cubeful_luck"] / unit
        adjusted = dict(no_double_luck=ndl, no_double_luck_stderr=res[0]["equity_cubeful_luck_stderr"] / unit,
                        double_take_luck=dtl, double_take_luck_stderr=res[1]["equity_cubeful_luck_stderr"] / unit,
                        double_luck=bool(min(dtl, 1.0) > ndl), take_luck=bool(dtl <= 1.0))
    return dict(adjusted, no_double=nd, no_double_stderr=res[0]["equity_cubeful_stderr"] / unit,
                double_take=dt, double_take_stderr=res[1]["equity_cubeful_stderr"] / unit,
                double_pass=1.0, double_pass_stderr=0.0, double=bool(min(dt, 1.0) > nd), take=bool(dt <= 1.0),
                cube=[k, owner], rollouts=res)


# ------------------------------------------------- truncated cubeful rollouts --
class CubeLife:
    """The parameters of Janowski's interpolation (csrc/bg_cube_trunc.h; include/bgx.h
    bgx_cube_life): `x`, the cube life in [0, 1] (0: the cube is dead, the equity is the cubeless
    one; 1: fully live), and `win_value` / `loss_value`, the mean points W / L of a won / lost
    game in [1, 3] (gammon_values gives them from a cubeless rollout).  0.68 is a conventional
    contact value: a parameter, not a claim about the best one."""

    def __init__(self, x: float = 0.68, win_value: float = 1.0, loss_value: float = 1.0):
        for name, v, lo, hi in (("x", x, 0.0, 1.0), ("win_value", win_value, 1.0, 3.0),
                                ("loss_value", loss_value, 1.0, 3.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not lo <= float(v) <= hi:
                raise ValueError(f"CubeLife: {name} must be a number in [{lo:g}, {hi:g}], got {v!r}")
        self.x, self.win_value, self.loss_value = float(x), float(win_value), float(loss_value)

    def struct(self) -> _lib.BgxCubeLife:
        return _lib.BgxCubeLife(self.x, self.win_value, self.loss_value)


class CubeTruncation(Truncation):
    """truncate.Truncation for cubeful rollouts (run_lanes' cube_truncate=, with cube=): a game
    that has run `plies` plies stops there and is scored with Janowski's cube-life equity of the
    position reached, from `value` -- Truncation's value, scale and lookahead, and the same
    equity() -- and `life` (a CubeLife).  The cap and the Jacoby rule are the CubeRule's."""

    def __init__(self, value, plies: int, scale: float = 1.0, lookahead: int = 0, life: CubeLife = None):
        super().__init__(value, plies, scale=scale, lookahead=lookahead)
        life = CubeLife() if life is None else life
        if not isinstance(life, CubeLife):
            raise ValueError("CubeTruncation: life must be a cube.CubeLife")
        self.life = life


class CubeLuck:
    """The luck adjustment of cubeful rollouts (run_lanes' cube_luck=, with cube=; DESIGN.md §18;
    csrc/bg_cube_luck.h).  Every step takes the 21 per-roll values of the active lanes under
    `value` (a search.ValueHead; search.roll_values), turns each into Janowski's cube-life equity
    of the position after the roll -- the opponent on roll with the lane's cube, `scale` points
    per unit of the value, `life` a CubeLife -- and adds the drawn roll's equity minus the mean
    over the 21 rolls, times the cube, to the game's luck.  That luck has mean zero whatever the
    net, the life or the scale, so they only decide how much variance it removes.  The cap and the
    Jacoby rule are the CubeRule's."""

    def __init__(self, value, scale: float = 1.0, life: CubeLife = None):
        from .search import ValueHead
        if not isinstance(value, ValueHead):
            raise ValueError("CubeLuck: value must be a search.ValueHead")
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating, np.integer)) or math.isnan(float(scale)):
            raise ValueError(f"CubeLuck: scale must be a number, got {scale!r}")
        life = CubeLife() if life is None else life
        if not isinstance(life, CubeLife):
            raise ValueError("CubeLuck: life must be a cube.CubeLife")
        self.value, self.scale, self.life = value, float(scale), life
        self.totals = {"calls": 0, "rows": 0, "leaves": 0}      # roll_values calls so far, their lanes and leaves


def gammon_values(summary) -> tuple:
    """(W, L), the mean points of a won and of a lost game, from a cubeless rollout's summary
    (rollout.summarize's win1..3 and loss1..3); 1.0 for a side without a game."""
    def mean(prefix):
        n = [int(summary[f"{prefix}{j}"]) for j in (1, 2, 3)]
        return (n[0] + 2 * n[1] + 3 * n[2]) / sum(n) if sum(n) > 0 else 1.0
    return mean("win"), mean("loss")


def _seg(p, p0, y0, p1, y1):
    return y0 + (p - p0) * ((y1 - y0) / (p1 - p0))


def _live(p, W, L, f):
    """live_cen, live_own, live_opp of include/bgx.h at p, every operation rounded to f once."""
    half, one, zero = f(0.5), f(1), f(0)
    D = f(f(W + L) + half)
    TP, CP = f(f(L - half) / D), f(f(L + one) / D)
    lo, hi = _seg(p, zero, -L, TP, -one), _seg(p, CP, one, one, W)
    cen = np.where(p < TP, lo, np.where(p < CP, _seg(p, TP, -one, CP, one), hi))
    own = np.where(p < CP, _seg(p, zero, -L, CP, one), hi)
    opp = np.where(p < TP, lo, _seg(p, TP, -one, one, W))
    return cen, own, opp


def janowski_equities(p, life: CubeLife, jacoby: bool = False, dtype=np.float64):
    """(c, E_cen, E_own, E_opp) of include/bgx.h at the win probabilities p, with c = p (W + L) - L,
    in `dtype` (fp64: the rule itself, for its properties and janowski_points)."""
    f = dtype
    p = np.asarray(p, f)
    x, W, L, one = f(life.x), f(life.win_value), f(life.loss_value), f(1)
    c = p * f(W + L) - L
    live = _live(p, W, L, f)
    e = [(one - x) * c + x * s for s in live]
    if jacoby:
        e[0] = (one - x) * (f(2) * p - one) + x * _live(p, one, one, f)[0]
    return c, e[0], e[1], e[2]


def janowski_reference(value, cube, mover, scale: float, life: CubeLife, cap: int, jacoby: bool = False):
    """cube_trunc_values of csrc/bg_cube_trunc.h (bgx_cube_janowski without the lane selection)
    on arrays in numpy float32, bit for bit: (values f32[n, 4] = nd, DT, e, c; flags uint8[n])
    for the cubeless values `value`, the cube bytes `cube` (None: centred at 1) and the movers
    `mover` (record byte 52)."""
    f = np.float32
    v = np.asarray(value, f).reshape(-1)
    n = v.shape[0]
    cb = sanitise(np.zeros(n, np.uint8) if cube is None else np.asarray(cube).reshape(-1), cap)
    k, o = unpack(cb)
    m = np.asarray(mover).reshape(-1).astype(np.int64) & 1
    x, W, L, one = f(life.x), f(life.win_value), f(life.loss_value), f(1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (f(scale) * v).astype(f)
    c = np.where(np.isnan(c), f(0), np.minimum(np.maximum(c, -L), W)).astype(f)
    p = ((c + L).astype(f) / f(W + L)).astype(f)
    dead = k >= int(cap)
    access = ~dead & ((o == 0) | (o == m + 1))
    live = _live(p, W, L, f)
    omx = f(one - x)

    def mix(d, s):
        return ((omx * d).astype(f) + (x * s).astype(f)).astype(f)
    e_cen, e_own, e_opp = (mix(c, s.astype(f)) for s in live)
    if jacoby:
        e_cen = mix(((f(2) * p).astype(f) - one).astype(f), _live(p, one, one, f)[0].astype(f))
    nd = np.where(dead, c, np.where(o == 0, e_cen, np.where(access, e_own, e_opp))).astype(f)
    dt = (f(2) * np.where(k + 1 >= int(cap), c, e_opp)).astype(f)
    cash = np.where(dt < one, dt, one).astype(f)
    doubles = access & (cash > nd)
    values = np.stack([nd, dt, np.where(doubles, cash, nd).astype(f), c], axis=1).astype(f)
    flags = (access * 1 + doubles * 2 + (dt <= one) * 4 + dead * 8).astype(np.uint8)
    return values, flags


def cube_trunc_fixed_reference(e, start_mover_on_roll, k):
    """cube_trunc_q of csrc/bg_cube_trunc.h on arrays: Yq = clamp(rint(fp32(+-e 2^16)), +-3 * 2^16) 2^k,
    0 for a NaN (round half even)."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        y = (np.where(start_mover_on_roll, np.asarray(e, f), -np.asarray(e, f)).astype(f) * f(CUBE_TRUNC_ONE)).astype(f)
    y = np.where(np.isnan(y), f(0), np.clip(y, -3.0 * CUBE_TRUNC_ONE, 3.0 * CUBE_TRUNC_ONE))
    return np.rint(y).astype(np.int64) * (np.int64(1) << np.asarray(k).astype(np.int64))


ROLL_P = np.asarray([1 if a == b else 2 for a in range(1, 7) for b in range(a, 7)], np.float32) / np.float32(36)


def roll_index(roll) -> np.ndarray:
    """The index of the rolls (d0, d1) [n, 2] among the 21 rolls (1-1, 1-2, ..., 6-6); -1: no roll."""
    d = np.asarray(roll).astype(np.int64).reshape(-1, 2)
    lo, hi = d.min(axis=1), d.max(axis=1)
    return np.where((lo >= 1) & (hi <= 6), 7 * (lo - 1) - (lo - 1) * lo // 2 + hi - lo, -1)


def fma32(a, b, c) -> np.ndarray:
    """fp32 fma(a, b, c) of finite float32 arrays, rounded once: the product is exact in fp64, the
    sum is formed in fp64 rounded to odd (the error of the fp64 sum, by two-sum, decides the last
    bit), and 53 >= 24 + 2 bits make the final rounding to fp32 that of the exact value."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    nudge = (err != 0) & ((np.ascontiguousarray(s).view(np.int64).reshape(s.shape) & 1) == 0)
    toward = np.where(err > 0, np.inf, -np.inf)
    return np.where(nudge, np.nextafter(s, toward), s).astype(np.float32)


def cube_roll_luck_reference(values21, cube, mover, roll, scale: float, life: CubeLife, cap: int, jacoby: bool = False):
    """cube_roll_luck of csrc/bg_cube_luck.h (bgx_cube_roll_luck without the lane selection) on
    arrays in numpy float32, bit for bit: (luck f32[n], mean f32[n]) for the per-roll values
    `values21` f32[n, 21] of the movers `mover` (record byte 52) holding the rolls `roll` uint8[n, 2]
    (bytes 53, 54) with the cube bytes `cube` (None: centred at 1).  g_r = -e of janowski_reference
    with the opponent on roll and the value -v_r; the mean is the fp32 FMA chain over r = 0..20,
    each step formed exactly and rounded once (fma32); luck = g of the roll - mean, 0 without a roll."""
    f = np.float32
    v = np.asarray(values21, f).reshape(-1, 21)
    n = v.shape[0]
    m = np.asarray(mover).reshape(-1).astype(np.int64) & 1
    g = np.empty((n, 21), f)
    for r in range(21):
        g[:, r] = -janowski_reference(-v[:, r], cube, 1 - m, scale, life, cap, jacoby)[0][:, 2]
    mean = np.zeros(n, f)
    for r in range(21):
        mean = fma32(ROLL_P[r], g[:, r], mean)
    idx = roll_index(roll)
    mine = g[np.arange(n), np.maximum(idx, 0)]
    return np.where(idx >= 0, (mine - mean).astype(f), f(0)).astype(f), mean


def cube_luck_reference(trace, starts, group, n_groups: int, games_per_lane: int, rule: CubeRule, cube0=None) -> dict:
    """A traced luck-adjusted cubeful run (run_lanes' cube= with cube_luck=) replayed on the host:
    cube_reference extended by the three bookkeeping steps of include/bgx.h
    bgx_rollout_cube_luck_*.  A pass books the game's luck before the decision is applied; after
    the decision (and the masked reset) the trace's cube_luck, times the replay's own cube and
    signed by cube_luck_mover, joins the selected lanes' sums; a finished game books its luck
    before the starting cube comes back.  The result gains cube_luck_tally int64[P, 5],
    cube_luck_state uint8[steps, B] (the cubes the luck was scaled with), cube_luck_sel bool[steps,
    B] (the lanes selected there) and lane_luck f32[B] (the sums left at the end)."""
    return cube_reference(trace, starts, group, n_groups, games_per_lane, rule, cube0=cube0, cube_luck=True)


def _root(g, lo=0.0, hi=1.0):
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) < 0.0 else (lo, mid)
    return 0.5 * (lo + hi)


def janowski_points(life: CubeLife) -> dict:
    """The rule's decision points as cubeless equities c = p (W + L) - L of the side on roll, in
    fp64 (no Jacoby rule), from which a CubeRule's thresholds follow for the same cube life:
    `take`, above which the opponent passes (2 E_opp > 1: CubeRule's pass_at); `double_centred`
    and `redouble`, from which doubling beats holding a centred / an own cube (2 E_opp = E_cen /
    E_own: double_at); and, for W > 1, `too_good`, above which playing on with a centred cube
    beats cashing (E_cen > 1: too_good_at).  Each is the root of a continuous piecewise linear
    function on [0, 1], by bisection; `p_take` etc. hold the win probabilities themselves."""
    W, L = life.win_value, life.loss_value

    def eq(p):
        return [float(v) for v in janowski_equities(np.float64(p), life)]
    roots = dict(take=_root(lambda p: 2.0 * eq(p)[3] - 1.0),
                 double_centred=_root(lambda p: 2.0 * eq(p)[3] - eq(p)[1]),
                 redouble=_root(lambda p: 2.0 * eq(p)[3] - eq(p)[2]))
    if W > 1.0:
        roots["too_good"] = _root(lambda p: eq(p)[1] - 1.0)
    out = {name: p * (W + L) - L for name, p in roots.items()}
    out.update({f"p_{name}": p for name, p in roots.items()})
    return out


def cube_trunc_reference(trace, starts, group, n_groups: int, games_per_lane: int, rule: CubeRule, truncation,
                         cube0=None, cut_lookup=None) -> dict:
    """A traced truncated cubeful run (run_lanes' cube= with cube_truncate=) replayed on the host:
    cube_reference extended by the truncation, the way its cut_lookup= extends it by the table
    cut.  After every step's advance (and table cut) a selected lane whose game has run
    truncation.plies plies adds Yq = cube_trunc_fixed_reference(e of janowski_reference on the
    trace's ctrunc_value and ctrunc_mover and the replay's own cube state; signed for the start
    mover; k) to its row, counts the game and gets its starting cube back.  The result gains
    cube_trunc_tally int64[P, 6], ctrunc bool[steps, B] and ctrunc_cube uint8[steps, B] (the
    states the truncation saw)."""
    return cube_reference(trace, starts, group, n_groups, games_per_lane, rule, cube0=cube0, cut_lookup=cut_lookup,
                          cube_truncate=truncation)


def static_cube_decision(eng_or_records, head, cube=None, scale: float = 1.0, life: CubeLife = None, cap: int = 6,
                         jacoby: bool = False, sel=None, value=None, out=None):
    """"Double or not, take or pass?" with no rollout (bgx_cube_janowski): (values f32[n, 4],
    flags uint8[n]) for an Engine's lane records or a contiguous uint8[n, 64] tensor on the GPU,
    shaped like bearoff.CubefulBearoffDB.lookup's -- values = (nd, DT, e, cubeless c) of the
    record's mover holding the cube byte cube[i] (uint8[n], pack(k, owner); None: centred at 1),
    flags bit 0: the mover may double, 1: it doubles, 2: the opponent takes, 3: the cube is dead.
    The cubeless value is `head`'s static value of the records (search.value_lanes), or `value`
    (float32[n] on the records' device) when given.  `sel` (uint8[n]): only those records; a
    record off sel or game_over gets flags 0 and keeps what `out` = (values, flags) held (NaN
    without `out`).  Sync-free."""
    from .arena import _stream
    from .engine import Engine, _ptr
    from .search import value_lanes
    life = CubeLife() if life is None else life
    if not isinstance(life, CubeLife):
        raise ValueError("static_cube_decision: life must be a cube.CubeLife")
    if int(cap) != cap or not 0 <= int(cap) <= MAX_CAP:
        raise ValueError(f"static_cube_decision: cap must be in 0..{MAX_CAP}, got {cap!r}")
    if math.isnan(float(scale)):
        raise ValueError("static_cube_decision: scale is NaN")
    r = eng_or_records
    if isinstance(r, Engine):
        n, dev, rp = r.batch, r.device, ctypes.c_void_p(r.lanes_ptr())
    else:
        if (not isinstance(r, torch.Tensor) or r.dtype != torch.uint8 or r.dim() != 2 or r.shape[1] != 64
                or not r.is_contiguous() or not r.is_cuda):
            raise ValueError("static_cube_decision: records must be an Engine or a contiguous uint8[n, 64] tensor on "
                             "the GPU")
        n, dev, rp = r.shape[0], r.device, _ptr(r)
    for name, t, dt in (("cube", cube, torch.uint8), ("sel", sel, torch.uint8), ("value", value, torch.float32)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.shape != (n,) or t.dtype != dt or t.device != dev
                              or not t.is_contiguous()):
            raise ValueError(f"static_cube_decision: {name} must be a contiguous {dt}[{n}] tensor on {dev}")
    if value is None:
        value = value_lanes(r, head, sel=sel)
    if out is None:
        out = (torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.uint8, device=dev))
    values, flags = out
    check(_lib.load().bgx_cube_janowski(rp, _ptr(cube), _ptr(value), n, float(scale), life.struct(), int(cap),
                                        int(bool(jacoby)), _ptr(sel), _ptr(values), _ptr(flags), _stream(dev)),
          "bgx_cube_janowski")
    return values, flags
