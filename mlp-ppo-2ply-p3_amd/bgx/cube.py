"""The doubling cube in position rollouts, money play (the device side is
csrc/bg_cube.h, the four bgx_rollout_cube_* entry points of include/bgx.h; bgx/rollout.py runs
them in its loop).  A game is worth its cubeless 1 / 2 / 3 points times the cube, 2^k; the side
on roll may double before it rolls when the cube is centred or its own, the opponent takes
(k + 1, the cube is now the taker's) or passes (the game ends at 2^k).  Both decisions follow one
threshold rule, CubeRule, on the mover's equity before the roll.  Where a game enters the cubeful
exact bearoff table (bearoff.CubefulBearoffDB) it can be cut and scored with its
exact cubeful expectation instead (cube_bearoff=; summarize_cube_bearoff).

    python -m bgx.rollout --net ckpt.pt --player 1ply --positions opening --trials 1296 --cube
    python -m bgx.rollout --net ckpt.pt --player 1ply --positions pos.json --cube --cube-decision
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

# cube_tally int64[n_groups][8] (include/bgx.h bgx_rollout_cube_field)
CUBE_FIELDS = ("cube_games", "cube_points", "cube_points2", "cube_log2", "pass_games", "pass_plies", "pass_won",
               "doubles")
MAX_CAP = 10
CENTRED = 0                         # the owner field: 0 centred, 1 PLAYER1, 2 PLAYER2
# cube_cut_tally int64[n_groups][6] (include/bgx.h bgx_rollout_cube_cut_field): the games cut at
# the cubeful bearoff table, fixed point, 2^-20 points
CUBE_CUT_FIELDS = ("cut_games", "cut_plies", "cut_y", "cut_y2_lo", "cut_y2_hi", "cut_log2")
CUBE_CUT_ONE = 1 << 20              # Yq = rint(q * CUBE_CUT_ONE) * 2^k
CUBE_CUT_SPLIT = 30                 # sum Yq^2 = cut_y2_hi * 2^30 + cut_y2_lo


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


def summarize_cube(tally_row, cube_row, unfinished: int = 0) -> dict:
    """One position's cubeful result from its 8 tally entries (the games played to the end) and its
    8 cube sums (CUBE_FIELDS), in fp64 from the integers: `games` (played out + passed),
    `equity_cubeful` = CUBE_POINTS / games in points from the start mover's side,
    `equity_cubeful_stderr` = sqrt((CUBE_POINTS2 - games equity^2) / (games - 1) / games),
    `pass_share` = PASS_GAMES / games, `doubles_per_game`, `mean_cube_log2` (the mean k at the
    game's end), `plies_per_game` over PLIES + PASS_PLIES, the 8 sums under their names, and
    `played_out` = summarize(tally_row): the cubeless result of the subset of games that
    reached the end -- no estimate of the position's cubeless equity, as the passed games are
    missing from it.  No games: the rates are 0; one game: the standard error is 0.  Raises
    ValueError when CUBE_GAMES != GAMES + PASS_GAMES."""
    from .rollout import summarize
    played = summarize(tally_row, unfinished)
    c = [int(v) for v in cube_row]
    if len(c) != len(CUBE_FIELDS):
        raise ValueError(f"summarize_cube: a cube row has {len(CUBE_FIELDS)} entries, got {len(c)}")
    r = dict(zip(CUBE_FIELDS, c))
    n = r["cube_games"]
    if n != played["games"] + r["pass_games"]:
        raise ValueError(f"summarize_cube: the cube row counts {n} games, the tally row {played['games']} and "
                         f"{r['pass_games']} passed")
    def per_game(v):
        return v / n if n > 0 else 0.0

    var_num = max(n * r["cube_points2"] - r["cube_points"] ** 2, 0)        # n^2 (n - 1) x the variance of the mean
    r.update(games=n, equity_cubeful=per_game(r["cube_points"]),
             equity_cubeful_stderr=math.sqrt(var_num / (n * n * (n - 1))) if n > 1 else 0.0,
             pass_share=per_game(r["pass_games"]), doubles_per_game=per_game(r["doubles"]),
             mean_cube_log2=per_game(r["cube_log2"]), plies_per_game=per_game(played["plies"] + r["pass_plies"]),
             unfinished=int(unfinished), played_out=played)
    return r


def summarize_cube_bearoff(tally_row, cube_row, cut_row, unfinished: int = 0) -> dict:
    """summarize_cube(tally_row, cube_row, unfinished) for a run cut at the cubeful bearoff table
    (DESIGN.md §15), with the row's 6 cut sums (CUBE_CUT_FIELDS).  A cut game's result is its
    exact cubeful expectation y = Yq / 2^20 points.  `games` = played out + passed + cut,
    `equity_cubeful` and `equity_cubeful_stderr` over all three kinds together, from Python
    integers: sum y = CUBE_POINTS 2^20 + CUT_Y in units of 2^-20, sum y^2 = CUBE_POINTS2 2^40 +
    CUT_Y2_HI 2^30 + CUT_Y2_LO in units of 2^-40, so equal results give their value exactly and a
    standard error of 0.  `pass_share`, `doubles_per_game`, `mean_cube_log2` (CUBE_LOG2 +
    CUT_LOG2) and `plies_per_game` (PLIES + PASS_PLIES + CUT_PLIES) are over all games; adds
    `cut_share` = CUT_GAMES / games and the 6 sums under their names.  The cut replaces the
    endgame's dice noise and its cube action by the expectation, so the standard error is that of
    the mixed sample.  Raises ValueError when CUBE_GAMES != GAMES + PASS_GAMES (the cut games are
    counted beside them)."""
    r = summarize_cube(tally_row, cube_row, unfinished)
    c = [int(v) for v in cut_row]
    if len(c) != len(CUBE_CUT_FIELDS):
        raise ValueError(f"summarize_cube_bearoff: a cut row has {len(CUBE_CUT_FIELDS)} entries, got {len(c)}")
    cut = dict(zip(CUBE_CUT_FIELDS, c))
    n = r["cube_games"] + cut["cut_games"]
    s1 = r["cube_points"] * CUBE_CUT_ONE + cut["cut_y"]
    s2 = r["cube_points2"] * CUBE_CUT_ONE ** 2 + (cut["cut_y2_hi"] << CUBE_CUT_SPLIT) + cut["cut_y2_lo"]

    def per_game(v):
        return v / n if n > 0 else 0.0

    var_num = max(n * s2 - s1 * s1, 0)                   # n^2 (n - 1) 2^40 x the variance of the mean
    r.update(cut, games=n, cut_share=per_game(cut["cut_games"]),
             equity_cubeful=s1 / (n * CUBE_CUT_ONE) if n > 0 else 0.0,
             equity_cubeful_stderr=math.sqrt(var_num / (n * n * (n - 1))) / CUBE_CUT_ONE if n > 1 else 0.0,
             pass_share=per_game(r["pass_games"]), doubles_per_game=per_game(r["doubles"]),
             mean_cube_log2=per_game(r["cube_log2"] + cut["cut_log2"]),
             plies_per_game=per_game(r["played_out"]["plies"] + r["pass_plies"] + cut["cut_plies"]))
    return r


def cube_bearoff_cut_reference(records, cube, plies, games_done, sel, starts, group, n_groups: int,
                               games_per_lane: int, cap: int, cube0, lookup) -> dict:
    """One call of bgx_rollout_cube_bearoff_cut on the host (include/bgx.h), state in, state out.
    `lookup`: records uint8[B, 64], cube uint8[B], cap -> (in_db bool[B], values f32[B, 4], flags),
    e.g. bearoff.cube_lookup_reference on a table.  A selected lane with a valid group whose record
    is in the table adds Yq = bearoff.cube_fixed_reference(nd on its first ply, else e; signed for
    the start mover; k of its cube) to its row, counts the game and gets its starting cube back.
    Returns dict(cut_tally int64[P, 6], mask bool[B], games_done, plies, sel uint8[B], cube
    uint8[B], retired int = the lanes that finished their last game)."""
    from .bearoff import cube_fixed_reference
    from .rollout import R_CUR
    records, starts = np.asarray(records), np.asarray(starts)
    group = np.asarray(group).astype(np.int64)
    B, P, G = group.shape[0], int(n_groups), int(games_per_lane)
    cube = np.asarray(cube).astype(np.uint8).copy()
    plies, games = np.asarray(plies).astype(np.int64).copy(), np.asarray(games_done).astype(np.int64).copy()
    sel = np.asarray(sel).astype(np.uint8).copy()
    in_db, values, _ = lookup(records, cube, cap)
    m = (sel != 0) & (group >= 0) & (group < P) & np.asarray(in_db, bool)
    k = np.minimum(cube.astype(np.int64) & 15, int(cap))
    v = np.where(plies == 0, values[:, 0], values[:, 2]).astype(np.float32)
    yq = cube_fixed_reference(np.where(m, v, np.float32(0)), records[:, R_CUR] == starts[:, R_CUR], k)
    y2 = yq * yq
    tally = np.zeros((P, len(CUBE_CUT_FIELDS)), np.int64)
    for f, x in enumerate((np.ones(B, np.int64), plies, yq, y2 & ((1 << CUBE_CUT_SPLIT) - 1), y2 >> CUBE_CUT_SPLIT, k)):
        np.add.at(tally[:, f], group[m], x[m])
    games[m] += 1
    plies[m] = 0
    retired = m & (games >= G)
    sel[retired] = 0
    cube[m] = sanitise(np.asarray(cube0), cap)[m]
    return dict(cut_tally=tally, mask=m, games_done=games, plies=plies, sel=sel, cube=cube, retired=int(retired.sum()))


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
                   cut_lookup=None) -> dict:
    """A traced cube run replayed on the host with the kernels' arithmetic (include/bgx.h
    bgx_rollout_cube_*).  `trace`: run_lanes' with cube_mover, cube_equity, done and info
    [steps, B]; the lane records are taken as not game_over, which holds between the steps of an
    auto-reset engine.  Returns dict(cube_tally int64[P, 8], tally int64[P, 8], cube uint8[steps,
    B] = the states before each decision, dsel / mask bool[steps, B], games_done int64[B],
    active int).  `cut_lookup` (cube_bearoff_cut_reference's `lookup`): the run was cut at the
    cubeful bearoff table (run_lanes' cube_bearoff=) -- the cut is replayed after begin on the
    trace's cut_records0 and after every step on cut_records[t]; the result gains cut_tally
    int64[P, 6], cut0 bool[B] and cut bool[steps, B]."""
    from .rollout import FIELDS, R_CUR
    mover = np.asarray(torch.as_tensor(trace["cube_mover"]).cpu()).astype(np.int64)
    equity = np.asarray(torch.as_tensor(trace["cube_equity"]).cpu()).astype(np.float32)
    done = np.asarray(torch.as_tensor(trace["done"]).cpu())
    info = np.asarray(torch.as_tensor(trace["info"]).cpu()).astype(np.int64)
    starts, group = np.asarray(torch.as_tensor(starts).cpu()), np.asarray(torch.as_tensor(group).cpu()).astype(np.int64)
    B, P, G, cap = group.shape[0], int(n_groups), int(games_per_lane), rule.cap
    c0 = np.zeros(B, np.uint8) if cube0 is None else sanitise(np.asarray(torch.as_tensor(cube0).cpu()), cap)
    cube = c0.copy()
    valid = (group >= 0) & (group < P)
    start_m = starts[:, R_CUR].astype(np.int64) & 1
    plies, games = np.zeros(B, np.int64), np.zeros(B, np.int64)
    tally, ct = np.zeros((P, len(FIELDS)), np.int64), np.zeros((P, len(CUBE_FIELDS)), np.int64)
    T = done.shape[0]
    states, dsels, masks = np.zeros((T, B), np.uint8), np.zeros((T, B), bool), np.zeros((T, B), bool)
    cut_tally, cuts = np.zeros((P, len(CUBE_CUT_FIELDS)), np.int64), np.zeros((T, B), bool)

    def cut(recs):
        nonlocal cube, plies, games
        out = cube_bearoff_cut_reference(np.asarray(torch.as_tensor(recs).cpu()), cube, plies, games, valid & (games < G),
                                         starts, group, P, G, cap, c0, cut_lookup)
        cube, plies, games = out["cube"], out["plies"], out["games_done"]
        cut_tally[:] += out["cut_tally"]
        return out["mask"]

    cut0 = cut(trace["cut_records0"]) if cut_lookup is not None else None

    def add(rows, lanes, values):
        for f, v in values.items():
            np.add.at(rows[:, f], group[lanes], np.broadcast_to(v, (B,))[lanes])

    for t in range(T):
        sel = valid & (games < G)
        states[t] = cube
        k, _ = unpack(cube)
        m = mover[t] & 1
        act, nxt, access = decide_reference(cube, m, equity[t], rule)
        dsel = sel & (plies > 0) & access
        dsels[t] = dsel
        act = np.where(dsel, act, 0)
        pas, dbl = act == 2, act > 0
        y = np.where(m == start_m, 1, -1) * (1 << k)
        add(ct, pas, {0: 1, 1: y, 2: y * y, 3: k, 4: 1, 5: plies, 6: (y > 0).astype(np.int64)})
        add(ct, dbl, {7: 1})
        masks[t] = pas
        games += pas
        plies = np.where(pas, 0, plies)
        cube = np.where(pas, c0, np.where(dbl, nxt, cube)).astype(np.uint8)
        # the step, cube_flush and advance
        sel = valid & (games < G)
        plies = plies + sel
        winner = ((info[t] >> 8) & 0xFF) - 1
        score = np.clip((info[t] >> 16) & 0xFF, 1, 3)
        dn = sel & (done[t] != 0)
        fin = dn & (winner >= 0)
        k, _ = unpack(cube)
        won = winner == start_m
        s = np.where(rule.jacoby & (k == 0), 1, score)
        y = np.where(won, 1, -1) * (s << k)
        add(ct, fin, {0: 1, 1: y, 2: y * y, 3: k})
        add(tally, fin, {0: 1, 1: plies})
        np.add.at(tally, (group[fin], (np.where(won, 2, 5) + score - 1)[fin]), 1)
        cube = np.where(dn, c0, cube).astype(np.uint8)
        games += fin
        plies = np.where(fin, 0, plies)
        if cut_lookup is not None:
            cuts[t] = cut(trace["cut_records"][t])
    out = dict(cube_tally=ct, tally=tally, cube=states, dsel=dsels, mask=masks, games_done=games,
               active=int((valid & (games < G)).sum()))
    if cut_lookup is not None:
        out.update(cut_tally=cut_tally, cut0=cut0, cut=cuts)
    return out


def rollout_cube_decision(rollout, player, record, trials: int, rule: CubeRule, cube=(0, CENTRED),
                          first_roll: str = "stratified", max_steps: int = 4000, cube_bearoff=None) -> dict:
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
    the cut's 2^-20 resolution, with standard errors of 0."""
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
                      cube_start=[(k, owner), (k + 1, 2 - mover)], cube_bearoff=cube_bearoff)
    unit = float(1 << k)
    nd, dt = res[0]["equity_cubeful"] / unit, res[1]["equity_cubeful"] / unit
    return dict(no_double=nd, no_double_stderr=res[0]["equity_cubeful_stderr"] / unit,
                double_take=dt, double_take_stderr=res[1]["equity_cubeful_stderr"] / unit,
                double_pass=1.0, double_pass_stderr=0.0, double=bool(min(dt, 1.0) > nd), take=bool(dt <= 1.0),
                cube=[k, owner], rollouts=res)
