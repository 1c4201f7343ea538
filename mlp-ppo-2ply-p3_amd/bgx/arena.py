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

--cube: money play with the doubling cube (csrc/bg_arena_cube.h): every game
starts with the cube centred at 1; before its roll, but never on a game's first ply, the side
on roll may double by its own CubeRule on its own net's equity, and the other side takes or
passes by its own.  The result is A's cubeful points per game beside the played-out games' plain
result.

    python -m bgx.arena --a new.pt --b old.pt --max-steps 4000 --cube --cube-lookahead-a 0 \\
        --cube-lookahead-b 0 --cube-double-a 0.35

--luck: the cubeless result with every roll's luck subtracted as a control variate (DESIGN.md §19;
csrc/bg_arena_luck.h): the mover's best 1-ply value after the roll that came minus its mean over
the rolls it was drawn from -- the 21 rolls, or on a game's first ply the 15 non-doubles of the
opening roll -- summed per game from A's side.  The result gains ppg_luck_a, ppg_luck_stderr,
variance_ratio, luck_scale and luck_mean.

    python -m bgx.arena --a new.pt --b old.pt --player-a 2ply --top-k-a 4 --player-b 2ply --top-k-b 4 \\
        --max-steps 4000 --luck

--match N: matches to N points instead of single games (csrc/bg_match.h; bgx/match.py):
the lanes keep the match score, the Crawford rule holds, each side doubles, takes and passes by its
own MatchRule -- the chance of winning the match on a match equity table -- and --games-per-lane
counts matches.  The result is A's match win rate.

    python -m bgx.arena --a new.pt --b old.pt --max-steps 20000 --match 7 --games-per-lane 1 \\
        --match-lookahead-a 0 --match-lookahead-b 0
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
from .engine import Engine, R_CUR, R_NM0, R_NM1, R_ROLL0, R_ROLL1, _ptr, _stream

# tally int64[16] (include/bgx.h bgx_arena_field); entries 14, 15 stay zero
FIELDS = ("games", "wins_a", "wins_b", "points_a", "points_b", "gammons_a", "gammons_b", "backgammons_a",
          "backgammons_b", "games_a_p1", "wins_a_p1", "wins_p1", "plies", "active_lanes")
ACTIVE = FIELDS.index("active_lanes")
# cube_tally int64[16] (include/bgx.h bgx_arena_cube_field); entries 11..15 stay zero
CUBE_FIELDS = ("cube_games", "cube_points_a", "cube_points2", "cube_wins_a", "cube_log2", "pass_games", "pass_plies",
               "passes_a", "passes_b", "doubles_a", "doubles_b")
# luck_tally int64[8] (include/bgx.h bgx_arena_luck_field): fixed point, 2^-16 points; entries 5..7 stay zero
LUCK_FIELDS = ("luck_sum", "luck2_lo", "luck2_hi", "resluck", "luck_games")
LUCK_ONE = 65536                # Lq = rint(L * LUCK_ONE), clamped to +-2^21 (replay.luck_q)
LUCK_SPLIT = 30                 # sum Lq^2 = luck2_hi * 2^30 + luck2_lo
TRACE_LIMIT = 1 << 22           # trace=True: batch x max_steps entries per traced field
SYNC_EVERY = 16                 # sync-free players: steps between host reads of the active-lane count


def summarize(tally, steps: int, unfinished: int) -> dict:
    """The arena result from the 16 tally entries: the fields by name, `steps`,
    `unfinished_lanes`, A's win rate with its binomial standard error and A's points per
    game (points_a - points_b) / games with its standard error `ppg_stderr`, exact from the
    integers: a game's result is +-1 / 2 / 3, singles = wins - gammons - backgammons, so the sum of
    squares is singles + 4 gammons + 9 backgammons and ppg_stderr = sqrt((sum of squares - games
    ppg^2) / (games - 1) / games).  No games: the rates are 0; one game: ppg_stderr is 0."""
    t = [int(v) for v in tally]
    if len(t) < len(FIELDS):
        raise ValueError(f"summarize: the tally has {len(t)} entries, needs {len(FIELDS)}")
    r = dict(zip(FIELDS, t))
    g = r["games"]
    p = r["wins_a"] / g if g > 0 else 0.0
    s1 = r["points_a"] - r["points_b"]
    s2 = sum(r[f"wins_{x}"] + 3 * r[f"gammons_{x}"] + 8 * r[f"backgammons_{x}"] for x in "ab")
    r.update(ppg_stderr=math.sqrt(max(g * s2 - s1 * s1, 0) / (g * g * (g - 1))) if g > 1 else 0.0)
    r.update(steps=int(steps), unfinished_lanes=int(unfinished), win_rate_a=p,
             ppg_a=(r["points_a"] - r["points_b"]) / g if g > 0 else 0.0,
             win_rate_stderr=math.sqrt(max(p * (1.0 - p), 0.0) / g) if g > 0 else 0.0)
    return r


def summarize_cube(tally, cube_tally, steps: int, unfinished: int) -> dict:
    """The cubeful arena result from the plain tally (the games played to the end) and the 16
    cube sums (CUBE_FIELDS), in fp64 from the integers as cube.summarize_cube does: `games`
    (played out + passed), `ppg_cubeful_a` = CUBE_POINTS_A / games, A's points per game at the
    cube, `ppg_cubeful_stderr` = sqrt((CUBE_POINTS2 - games ppg^2) / (games - 1) / games),
    `win_rate_cubeful_a` = CUBE_WINS_A / games (a pass is a win for the doubler), `pass_share`,
    `doubles_per_game_a` / `_b` (doubles the side offered), `take_share_a` / `_b` (of the doubles
    offered TO the side, the share it took: 1 - PASSES_x / DOUBLES_other; 0 without one),
    `mean_cube_log2` (the mean k at the game's end), the 11 sums under their names, `steps`,
    `unfinished_lanes` and `played_out` = summarize(tally, ...): the plain result of the games
    played to the end -- no estimate of cubeless strength, as the passed games are missing from
    it.  No games: the rates are 0; one game: the standard error is 0.  Raises ValueError when
    CUBE_GAMES != GAMES + PASS_GAMES or PASS_GAMES != PASSES_A + PASSES_B."""
    played = summarize(tally, steps, unfinished)
    c = [int(v) for v in cube_tally]
    if len(c) < len(CUBE_FIELDS):
        raise ValueError(f"summarize_cube: the cube tally has {len(c)} entries, needs {len(CUBE_FIELDS)}")
    r = dict(zip(CUBE_FIELDS, c))
    n = r["cube_games"]
    if n != played["games"] + r["pass_games"]:
        raise ValueError(f"summarize_cube: the cube tally counts {n} games, the plain tally {played['games']} and "
                         f"{r['pass_games']} passed")
    if r["pass_games"] != r["passes_a"] + r["passes_b"]:
        raise ValueError(f"summarize_cube: {r['pass_games']} passed games, but A gave up {r['passes_a']} and B "
                         f"{r['passes_b']}")

    def per_game(v):
        return v / n if n > 0 else 0.0

    def take_share(offered, passed):
        return 1.0 - passed / offered if offered > 0 else 0.0

    var_num = max(n * r["cube_points2"] - r["cube_points_a"] ** 2, 0)      # n^2 (n - 1) x the variance of the mean
    r.update(games=n, ppg_cubeful_a=per_game(r["cube_points_a"]),
             ppg_cubeful_stderr=math.sqrt(var_num / (n * n * (n - 1))) if n > 1 else 0.0,
             win_rate_cubeful_a=per_game(r["cube_wins_a"]), pass_share=per_game(r["pass_games"]),
             doubles_per_game_a=per_game(r["doubles_a"]), doubles_per_game_b=per_game(r["doubles_b"]),
             take_share_a=take_share(r["doubles_b"], r["passes_a"]),
             take_share_b=take_share(r["doubles_a"], r["passes_b"]),
             mean_cube_log2=per_game(r["cube_log2"]), steps=int(steps), unfinished_lanes=int(unfinished),
             played_out=played)
    return r


# --------------------------------------------------------------------- cube --
class _ZeroEquity:
    """The equity of a side without a rule: zeros, never read past the thresholds at +inf."""
    sync_free = True

    def __init__(self):
        self.z = None

    def __call__(self, eng, dsel):
        if self.z is None or self.z.numel() != eng.batch or self.z.device != eng.device:
            self.z = torch.zeros(eng.batch, dtype=torch.float32, device=eng.device)
        return self.z


class ArenaCube:
    """The doubling cube of an arena match: `rule_a` and `rule_b`, A's and B's
    cube.CubeRule, each with its own value and thresholds.  A doubles by rule_a on rule_a's
    equity, B takes or passes by rule_b on rule_b's equity of the same position, and the other
    way round.  Either may be None: that side never doubles and takes every double (a CubeRule
    on a zero callable with double_at = pass_at = +inf, so the kernels need no special case).
    `cap` and `jacoby` belong to the game: both rules must agree on them (ValueError); a None
    side takes the other's, two None sides the CubeRule defaults."""

    def __init__(self, rule_a=None, rule_b=None):
        from .cube import CubeRule
        for r in (rule_a, rule_b):
            if r is not None and not isinstance(r, CubeRule):
                raise ValueError("ArenaCube: a rule must be a cube.CubeRule or None")
        if rule_a is not None and rule_b is not None and (rule_a.cap, rule_a.jacoby) != (rule_b.cap, rule_b.jacoby):
            raise ValueError(f"ArenaCube: cap and jacoby belong to the game, but A's rule has {rule_a.cap}, "
                             f"{rule_a.jacoby} and B's {rule_b.cap}, {rule_b.jacoby}")
        game = {}
        for r in (rule_a, rule_b):
            if r is not None:
                game = dict(cap=r.cap, jacoby=r.jacoby)

        def never():
            return CubeRule(_ZeroEquity(), double_at=math.inf, pass_at=math.inf, **game)

        self.has_a, self.has_b = rule_a is not None, rule_b is not None
        self.rule_a = rule_a if rule_a is not None else never()
        self.rule_b = rule_b if rule_b is not None else never()
        self.cap, self.jacoby = self.rule_a.cap, self.rule_a.jacoby
        self.sync_free = self.rule_a.sync_free and self.rule_b.sync_free


def arena_cube_reference(trace, batch: int, games_per_lane: int, rule_a, rule_b) -> dict:
    """A traced cube match (Arena.play(trace=True, cube=...)) replayed on the host with the
    kernels' fp32 arithmetic (include/bgx.h bgx_arena_cube_*).  Read from the trace, [steps, B]
    each: cube_mover (the side on roll before the decision), eq_offer (the equity the side on roll
    decided on), eq_resp (the doubler's equity as the other side estimated it), done and info; the
    lane records are taken as not game_over, which holds between the steps of an auto-reset
    engine.  `rule_a` / `rule_b`: the CubeRules (None as in ArenaCube).  Returns dict(tally
    int64[16], cube_tally int64[16], games_done int64[B], and [steps, B] each: cube uint8 = the
    states before each decision, dsel / offer uint8 (0 none, 1 A, 2 B), passed bool)."""
    from .cube import sanitise, unpack
    ac = ArenaCube(rule_a, rule_b)
    ra, rb = ac.rule_a, ac.rule_b
    f = np.float32

    def arr(k, dt):
        return np.asarray(torch.as_tensor(trace[k]).cpu()).astype(dt)

    mover, done, info = arr("cube_mover", np.int64), arr("done", np.int64), arr("info", np.int64)
    eq_offer, eq_resp = arr("eq_offer", f), arr("eq_resp", f)
    B, G, cap, T = int(batch), int(games_per_lane), ac.cap, done.shape[0]
    lane = np.arange(B, dtype=np.int64)
    cube, plies, games = np.zeros(B, np.uint8), np.zeros(B, np.int64), np.zeros(B, np.int64)
    tally, ct = np.zeros(16, np.int64), np.zeros(16, np.int64)
    states, dsels, offers = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
    passes = np.zeros((T, B), bool)
    F_, C_ = {k: i for i, k in enumerate(FIELDS)}, {k: i for i, k in enumerate(CUBE_FIELDS)}
    for t in range(T):
        states[t] = cube
        active = games < G
        m = mover[t] & 1
        a_moves = (m == 0) == (((lane + games) & 1) == 0)
        k, o = unpack(sanitise(cube, cap))
        access = (k < cap) & ((o == 0) | (o == m + 1))
        d = active & (plies > 0) & access
        dsel_a, dsel_b = d & a_moves, d & ~a_moves
        dsels[t] = dsel_a + 2 * dsel_b
        with np.errstate(invalid="ignore", over="ignore"):
            ea, eb = (f(ra.scale) * eq_offer[t]).astype(f), (f(rb.scale) * eq_offer[t]).astype(f)
            off_a = dsel_a & (ea >= f(ra.double_at)) & (ea <= f(ra.too_good_at))
            off_b = dsel_b & (eb >= f(rb.double_at)) & (eb <= f(rb.too_good_at))
            # B answers A's double by B's rule, A answers B's by A's
            gives_up = np.where(off_a, (f(rb.scale) * eq_resp[t]).astype(f) > f(rb.pass_at),
                                (f(ra.scale) * eq_resp[t]).astype(f) > f(ra.pass_at))
        offers[t] = off_a + 2 * off_b
        off = off_a | off_b
        pas, take = off & gives_up, off & ~gives_up
        passes[t] = pas
        y = np.where(off_a, 1, -1) * (1 << k)
        ct[C_["doubles_a"]] += off_a.sum()
        ct[C_["doubles_b"]] += off_b.sum()
        for name, v in (("cube_games", 1), ("cube_points_a", y), ("cube_points2", y * y), ("cube_wins_a", y > 0),
                        ("cube_log2", k), ("pass_games", 1), ("pass_plies", plies), ("passes_a", off_b),
                        ("passes_b", off_a)):
            ct[C_[name]] += np.broadcast_to(np.asarray(v, np.int64), (B,))[pas].sum()
        games = games + pas
        plies = np.where(pas, 0, plies)
        cube = np.where(pas, 0, np.where(take, (k + 1) | ((2 - m) << 4), cube)).astype(np.uint8)
        # the step, cube_flush and advance
        active = games < G
        winner, score = ((info[t] >> 8) & 0xFF) - 1, (info[t] >> 16) & 0xFF
        dn = active & (done[t] != 0)
        fin = dn & (winner >= 0)
        a_p1 = ((lane + games) & 1) == 0
        a_won = fin & ((winner == 0) == a_p1)
        b_won = fin & ~a_won
        k = np.minimum(cube.astype(np.int64) & 15, cap)
        s = np.where(ac.jacoby & (k == 0), 1, np.clip(score, 1, 3))
        y = np.where(a_won, 1, -1) * (s << k)
        for name, v in (("cube_games", 1), ("cube_points_a", y), ("cube_points2", y * y), ("cube_wins_a", y > 0),
                        ("cube_log2", k)):
            ct[C_[name]] += np.broadcast_to(np.asarray(v, np.int64), (B,))[fin].sum()
        pts = np.where((score >= 1) & (score <= 3), score, 0)
        for name, v in (("games", fin), ("wins_a", a_won), ("wins_b", b_won), ("points_a", a_won * pts),
                        ("points_b", b_won * pts), ("gammons_a", a_won & (score == 2)),
                        ("gammons_b", b_won & (score == 2)), ("backgammons_a", a_won & (score == 3)),
                        ("backgammons_b", b_won & (score == 3)), ("games_a_p1", fin & a_p1),
                        ("wins_a_p1", a_won & a_p1), ("wins_p1", fin & (winner == 0)), ("plies", active)):
            tally[F_[name]] += int(np.asarray(v, np.int64).sum())
        cube = np.where(dn, 0, cube).astype(np.uint8)
        plies = np.where(dn, 0, plies + active)
        games = games + fin
    tally[ACTIVE] = int((games < G).sum())
    return dict(tally=tally, cube_tally=ct, games_done=games, cube=states, dsel=dsels, offer=offers, passed=passes)


# --------------------------------------------------------------------- luck --
def summarize_luck(tally, luck_tally, steps: int, unfinished: int, scale="fit") -> dict:
    """summarize(tally, steps, unfinished) plus the luck-adjusted estimate from the 5 luck sums
    (LUCK_FIELDS; DESIGN.md §19, with §10's formulas).  A game's adjusted result is res - c L: res
    A's points, L the game's luck from A's side (over its rolls, the value after the roll that came
    minus its expectation under the distribution the roll was drawn from; + on A's rolls, - on
    B's).  E[L] = 0, so any constant c leaves the mean unbiased.  In fp64 from exact Python
    integers, n = games, sum res = points_a - points_b, sum res^2 as summarize forms it,
    sum L = LUCK / 2^16, sum L^2 = (LUCK2_HI 2^30 + LUCK2_LO) / 2^32, sum res L = RESLUCK / 2^16:
        ppg_luck_a = (sum res - c sum L) / n
        var_y = (sum res^2 - 2 c sum res L + c^2 sum L^2 - n ppg_luck_a^2) / (n - 1), >= 0
        ppg_luck_stderr = sqrt(var_y / n)        variance_ratio = var_y / var_res
    (variance_ratio 1.0 when var_res is 0; n < 2: the standard errors are 0).  `scale` = "fit":
    c = cov(res, L) / var(L) of these games, numerator and denominator as exact integers (0 when
    the denominator is 0); fitted on the same games it biases ppg_luck_a by O(1/n).  A float: that
    fixed c (1.0 when the net's values are in points).  Adds ppg_luck_a, ppg_luck_stderr,
    variance_ratio, luck_scale (c), luck_mean = sum L / n with luck_mean_stderr, and the 5 sums
    under their names.  Raises ValueError when LUCK_GAMES != games."""
    r = summarize(tally, steps, unfinished)
    k = [int(v) for v in luck_tally]
    if len(k) < len(LUCK_FIELDS):
        raise ValueError(f"summarize_luck: the luck tally has {len(k)} entries, needs {len(LUCK_FIELDS)}")
    n = r["games"]
    if k[4] != n:
        raise ValueError(f"summarize_luck: the luck tally counts {k[4]} games, the plain tally {n}")
    sr = r["points_a"] - r["points_b"]
    sr2 = sum(r[f"wins_{x}"] + 3 * r[f"gammons_{x}"] + 8 * r[f"backgammons_{x}"] for x in "ab")
    il, il2, irl = k[0], (k[2] << LUCK_SPLIT) + k[1], k[3]                          # 2^-16, 2^-32, 2^-16
    den = n * il2 - il * il                                                          # n^2 var(L), 2^-32
    if scale == "fit":
        c = LUCK_ONE * ((n * irl - sr * il) / den) if den > 0 else 0.0
    else:
        c = float(scale)
    sl, sl2, srl = il / LUCK_ONE, il2 / (LUCK_ONE * LUCK_ONE), irl / LUCK_ONE
    eq = (sr - c * sl) / n if n > 0 else 0.0
    var_y = max(sr2 - 2.0 * c * srl + c * c * sl2 - n * eq * eq, 0.0) / (n - 1) if n > 1 else 0.0
    var_r = max(sr2 - n * r["ppg_a"] ** 2, 0.0) / (n - 1) if n > 1 else 0.0
    r.update(zip(LUCK_FIELDS, k))
    r.update(ppg_luck_a=eq, ppg_luck_stderr=math.sqrt(var_y / n) if n > 0 else 0.0,
             variance_ratio=var_y / var_r if var_r > 0.0 else 1.0, luck_scale=c, luck_mean=sl / n if n > 0 else 0.0,
             luck_mean_stderr=math.sqrt(max(den, 0) / (n * n * (n - 1))) / LUCK_ONE if n > 1 else 0.0)
    return r


class ArenaLuck:
    """The luck adjustment of an arena match: `value`, the search.ValueHead whose
    best 1-ply values of the 21 rolls give each roll's luck (either side's net, or a third one: the
    luck has mean zero whatever the net, a better one removes more variance), and `scale`, "fit" or
    the fixed coefficient c of summarize_luck."""

    def __init__(self, value, scale="fit"):
        from .search import ValueHead
        if not isinstance(value, ValueHead):
            raise ValueError("ArenaLuck: value must be a search.ValueHead")
        if scale != "fit":
            scale = float(scale)
            if math.isnan(scale):
                raise ValueError("ArenaLuck: scale is NaN")
        self.value, self.scale = value, scale


_NOT_DOUBLE = [r for r, (a, b) in enumerate((a, b) for a in range(1, 7) for b in range(a, 7)) if a != b]


def arena_roll_luck_reference(values21, d0, d1, opening):
    """arena_roll_luck of csrc/bg_arena_luck.h (bgx_arena_luck_add's arithmetic) on arrays in numpy
    float32, bit for bit: (luck f32[n], mean f32[n]) for the per-roll values `values21` f32[n, 21]
    of the movers holding the rolls (d0, d1) (record bytes 53, 54).  `opening` == 0: the mean is
    the fp32 FMA chain sum p_r v_r over r = 0..20 with p_r = 1/36 for doubles, else 2/36 (§10's);
    != 0 (the roll was drawn as a game's first, doubles rejected): the chain of 1/15 v_r over the 15
    non-doubles, r ascending -- the doubles' values do not enter it.  Each step is formed exactly
    and rounded once (cube.fma32).  luck = v of the roll - mean; 0 without a roll, and 0 for a
    double at an opening.  NaN and infinite values propagate as in the C++."""
    from .cube import ROLL_P, fma32, roll_index
    f = np.float32
    v = np.asarray(values21, f).reshape(-1, 21)
    n = v.shape[0]
    op = np.broadcast_to(np.asarray(opening).reshape(-1) != 0, (n,))
    idx = roll_index(np.stack([np.broadcast_to(np.asarray(d0).reshape(-1), (n,)),
                               np.broadcast_to(np.asarray(d1).reshape(-1), (n,))], axis=1))
    with np.errstate(all="ignore"):
        mid, opn = np.zeros(n, f), np.zeros(n, f)
        for r in range(21):
            mid = fma32(ROLL_P[r], v[:, r], mid)
        for r in _NOT_DOUBLE:
            opn = fma32(f(1.0) / f(15.0), v[:, r], opn)
        mean = np.where(op, opn, mid).astype(f)
        mine = v[np.arange(n), np.maximum(idx, 0)]
        drawn = (idx >= 0) & ~(op & ~np.isin(idx, _NOT_DOUBLE))
        luck = np.where(drawn, (mine - mean).astype(f), f(0)).astype(f)
    return luck, mean


def arena_luck_reference(trace, batch: int, games_per_lane: int) -> dict:
    """A traced luck-adjusted match (Arena.play(trace=True, luck=...)) replayed on the host with
    the kernels' arithmetic (include/bgx.h bgx_arena_luck_*).  Read from the trace: owner (0 none,
    1 A, 2 B), done, info, luck_values f32[steps, B, 21] and luck_roll uint8[steps, B, 2].  Each
    step, the lanes with an owner get arena_roll_luck_reference of their values, roll and the
    replay's own `fresh`, added to the lane's fp32 sum with A's sign; after the step a counted game
    (an active lane, done, a winner) books replay.luck_q of the sum against A's points, and every
    done of an active lane zeroes the sum and sets fresh.  Returns dict(luck_tally int64[8],
    games_done int64[B], lane_luck f32[B] (the sums left at the end), and [steps, B] each: luck and
    mean f32 (the mover's view, NaN off the selection) and opening uint8)."""
    from .replay import luck_q

    def arr(k, dt):
        return np.asarray(torch.as_tensor(trace[k]).cpu()).astype(dt)

    f = np.float32
    owner, done, info = arr("owner", np.int64), arr("done", np.int64), arr("info", np.int64)
    vals, roll = arr("luck_values", f), arr("luck_roll", np.int64)
    B, G, T = int(batch), int(games_per_lane), done.shape[0]
    lane = np.arange(B, dtype=np.int64)
    games, lane_luck, fresh = np.zeros(B, np.int64), np.zeros(B, f), np.ones(B, bool)
    lt = [0] * 8
    lucks, means = np.full((T, B), np.nan, f), np.full((T, B), np.nan, f)
    opening = np.zeros((T, B), np.uint8)
    for t in range(T):
        sel = owner[t] != 0
        s = np.nonzero(sel)[0]
        if len(s):
            l, m = arena_roll_luck_reference(vals[t, s], roll[t, s, 0], roll[t, s, 1], fresh[s])
            lucks[t, s], means[t, s], opening[t, s] = l, m, fresh[s]
            with np.errstate(all="ignore"):
                lane_luck[s] = (lane_luck[s] + np.where(owner[t, s] == 1, l, -l).astype(f)).astype(f)
            fresh[s] = False
        dn = sel & (games < G) & (done[t] != 0)
        winner, score = ((info[t] >> 8) & 0xFF) - 1, (info[t] >> 16) & 0xFF
        fin = dn & (winner >= 0)
        pts = np.where((score >= 1) & (score <= 3), score, 0)
        res = np.where((winner == 0) == (((lane + games) & 1) == 0), pts, -pts)
        for i in np.nonzero(fin)[0]:
            lq = int(luck_q(lane_luck[i:i + 1])[0])
            lt[0] += lq
            lt[1] += (lq * lq) & ((1 << LUCK_SPLIT) - 1)
            lt[2] += (lq * lq) >> LUCK_SPLIT
            lt[3] += int(res[i]) * lq
            lt[4] += 1
        lane_luck[dn] = 0.0
        fresh[dn] = True
        games = games + fin
    return dict(luck_tally=np.asarray(lt, np.int64), games_done=games, lane_luck=lane_luck, luck=lucks, mean=means,
                opening=opening)


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
        self.cube_state = None          # play(cube=...): the cube stage's arrays, made on first use
        self.luck_state = None          # play(luck=...): the luck stage's arrays, made on first use
        self.match_state = None         # play(match=...): the match stage's arrays, made on first use

    def _act(self, player, sel, step):
        a = player.act(self.eng, sel, step)
        if (not isinstance(a, torch.Tensor) or a.dtype != torch.int32 or a.device != self.eng.device
                or not a.is_contiguous() or a.numel() != self.B):
            raise ValueError("a player's act must return a contiguous int32[B] tensor on the engine's device")
        return a

    def _equity(self, rule, sel, out, scratch=None):
        e = rule.equity(self.eng, sel, self.cube_state["scratch"] if scratch is None else scratch, out)
        if (not isinstance(e, torch.Tensor) or e.dtype != torch.float32 or e.device != self.eng.device
                or not e.is_contiguous() or e.numel() != self.B):
            raise ValueError("a cube rule's equity must be a contiguous float32[B] tensor on the engine's device")
        return e

    def play(self, a, b, max_steps: int, trace: bool = False, cube=None, luck=None, match=None):
        """begin; then [a.act, b.act, merge, step, advance] until no lane is active or
        `max_steps` env steps ran (weak greedy players can shuffle for thousands of steps:
        the result then reports `unfinished_lanes` instead of hanging).  Returns the
        result dict (summarize); with trace=True also a dict of per-step [steps, B]
        tensors: mover, n_moves, action, owner (0 none, 1 A, 2 B), done, info.

        `cube` (an ArenaCube): money play with the doubling cube.  Each step is
        then [cube_sel; A's equity on dsel_a, B's on dsel_b; cube_offer; B's equity on off_a, A's
        on off_b; cube_respond; reset(mask); cube_reseat; a.act, b.act, merge, step; cube_flush;
        advance].  The host reads the active-lane count every SYNC_EVERY steps only when both
        players and both rules are sync-free.  The result is summarize_cube's; the trace gains
        cube (the state before the decision), cube_mover (the side on roll there), dsel and offer
        (0 none, 1 A, 2 B), eq_offer (the equity the side on roll decided on, NaN off dsel),
        eq_resp (the doubler's equity as the other side sees it, NaN off offer) and passed.
        cube=None is exactly the path and result without the argument.

        `luck` (an ArenaLuck, or a bare search.ValueHead for ArenaLuck(value)):
        every roll's luck is taken as a control variate.  Each step is then [roll_values on
        sel_a | sel_b; arena_luck_add; a.act, b.act, merge, step; arena_luck_flush; advance].
        roll_values synchronises, so the active-lane count is read every step.  The result is
        summarize_luck's; the trace gains luck and luck_mean (f32, the mover's view, NaN off the
        selection), luck_opening (uint8: the roll was a game's first and is taken against the
        opening distribution), luck_roll (uint8[steps, B, 2], the roll bytes) and luck_values
        (f32[steps, B, 21], NaN off the selection), whose 21 entries count towards TRACE_LIMIT.
        `luck` together with `cube` raises ValueError: the cubeful arena's luck is not
        implemented.  luck=None is exactly the path and result without the argument.

        `match` (a match.ArenaMatch): matches to match.length points with the
        Crawford rule and cube decisions on the match equity table; `games_per_lane` then counts
        MATCHES per lane.  Each step is [match_sel; A's value on dsel_a, B's on dsel_b; match_offer;
        B's value on off_a, A's on off_b; match_respond; reset(mask); arena_cube_reseat; a.act,
        b.act, merge, step; match_flush; arena_advance; match_retire].  The host reads the
        active-lane count every SYNC_EVERY steps only when both players and both rules are
        sync-free.  The result is match.summarize_match's; the trace gains away (uint8[steps, B, 2],
        the points A and B need), craw, cube, cube_mover, dsel, offer, eq_offer, eq_resp and passed,
        all taken before the decision; the two-wide field counts towards TRACE_LIMIT.  `match`
        together with `cube` or `luck` raises ValueError.  match=None is exactly the path and result
        without the argument."""
        if match is not None:
            if cube is not None or luck is not None:
                raise ValueError("play: match together with cube or luck is not implemented")
            return self._play_match(a, b, max_steps, trace, match)
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError(f"play: max_steps {max_steps} must be >= 0")
        if luck is not None and not isinstance(luck, ArenaLuck):
            from .search import ValueHead
            if not isinstance(luck, ValueHead):
                raise ValueError("play: luck must be an ArenaLuck, a search.ValueHead or None")
            luck = ArenaLuck(luck)
        if luck is not None and cube is not None:
            raise ValueError("play: luck together with cube is not implemented (the cubeful arena's luck)")
        if trace and luck is not None and self.B * max_steps * 21 > TRACE_LIMIT:
            raise ValueError(f"play: trace=True with luck holds batch x max_steps x 21 = {self.B * max_steps * 21} "
                             f"entries in luck_values; the limit is {TRACE_LIMIT} (it is for tests and small batches)")
        if trace and self.B * max_steps > TRACE_LIMIT:
            raise ValueError(f"play: trace=True holds batch x max_steps = {self.B * max_steps} entries per field; "
                             f"the limit is {TRACE_LIMIT} (it is for tests and small batches)")
        L, eng, dev = _lib.load(), self.eng, self.eng.device
        recs = ctypes.c_void_p(eng.lanes_ptr())
        state = (_ptr(self.games_done), _ptr(self.sel_a), _ptr(self.sel_b), _ptr(self.tally))
        if cube is not None and not isinstance(cube, ArenaCube):
            raise ValueError("play: cube must be an ArenaCube or None")
        eng.reset(want_obs=False)
        check(L.bgx_arena_begin(recs, self.B, self.G, *state, _stream(dev)), "bgx_arena_begin")
        tr = None
        if trace:
            tr = {k: torch.zeros(max_steps, self.B, dtype=dt, device=dev)
                  for k, dt in (("mover", torch.uint8), ("n_moves", torch.int32), ("action", torch.int32),
                                ("owner", torch.uint8), ("done", torch.uint8), ("info", torch.int32))}
            rec = torch.empty(self.B, 64, dtype=torch.uint8, device=dev)
        every = SYNC_EVERY if getattr(a, "sync_free", False) and getattr(b, "sync_free", False) else 1
        if cube is not None:
            if not cube.sync_free:
                every = 1
            if self.cube_state is None:
                u8 = lambda: torch.zeros(self.B, dtype=torch.uint8, device=dev)         # noqa: E731
                f32 = lambda: torch.zeros(self.B, dtype=torch.float32, device=dev)      # noqa: E731
                self.cube_state = dict(cube=u8(), plies=torch.zeros(self.B, dtype=torch.int32, device=dev),
                                       tally=torch.zeros(16, dtype=torch.int64, device=dev), dsel_a=u8(), dsel_b=u8(),
                                       off_a=u8(), off_b=u8(), mask=u8(), eq_a=f32(), eq_b=f32(), er_a=f32(),
                                       er_b=f32(), scratch=f32())
            cs = self.cube_state
            ra, rb, st = cube.rule_a.struct(), cube.rule_b.struct(), _stream(dev)
            cstate = (_ptr(cs["cube"]), _ptr(cs["plies"]))
            check(L.bgx_arena_cube_begin(self.B, *cstate, _ptr(cs["tally"]), st), "bgx_arena_cube_begin")
            if trace:
                tr.update({k: torch.zeros(max_steps, self.B, dtype=dt, device=dev)
                           for k, dt in (("cube", torch.uint8), ("cube_mover", torch.uint8), ("dsel", torch.uint8),
                                         ("offer", torch.uint8), ("eq_offer", torch.float32),
                                         ("eq_resp", torch.float32), ("passed", torch.uint8))})
        if luck is not None:
            from .search import roll_values
            every = 1                   # roll_values waits for the device every step
            if self.luck_state is None:
                self.luck_state = dict(lane_luck=torch.zeros(self.B, dtype=torch.float32, device=dev),
                                       fresh=torch.zeros(self.B, dtype=torch.uint8, device=dev),
                                       tally=torch.zeros(8, dtype=torch.int64, device=dev),
                                       sel=torch.zeros(self.B, dtype=torch.uint8, device=dev),
                                       values=torch.zeros(self.B, 21, dtype=torch.float32, device=dev))
            ls = self.luck_state
            lstate = (_ptr(ls["lane_luck"]), _ptr(ls["fresh"]))
            check(L.bgx_arena_luck_begin(self.B, *lstate, _ptr(ls["tally"]), _stream(dev)), "bgx_arena_luck_begin")
            l_out = m_out = None
            if trace:
                tr.update({k: torch.zeros(max_steps, self.B, *shape, dtype=dt, device=dev)
                           for k, dt, shape in (("luck", torch.float32, ()), ("luck_mean", torch.float32, ()),
                                                ("luck_opening", torch.uint8, ()), ("luck_roll", torch.uint8, (2,)),
                                                ("luck_values", torch.float32, (21,)))})
                l_out = torch.empty(self.B, dtype=torch.float32, device=dev)
                m_out = torch.empty(self.B, dtype=torch.float32, device=dev)
        steps = 0
        active = int(self.tally[ACTIVE].item())
        while active > 0 and steps < max_steps:
            if luck is not None:
                torch.bitwise_or(self.sel_a, self.sel_b, out=ls["sel"])
                roll_values(eng, luck.value, sel=ls["sel"], out=ls["values"])
                if trace:
                    nan = float("nan")
                    on = ls["sel"] != 0
                    eng.records(out=rec)
                    tr["luck_opening"][steps] = ls["fresh"] * ls["sel"]
                    tr["luck_roll"][steps] = rec[:, R_ROLL0:R_ROLL1 + 1]
                    tr["luck_values"][steps] = torch.where(on[:, None], ls["values"], nan)
                    l_out.fill_(nan)
                    m_out.fill_(nan)
                check(L.bgx_arena_luck_add(recs, _ptr(self.sel_a), _ptr(self.sel_b), _ptr(ls["values"]), self.B, *lstate,
                                           _ptr(l_out), _ptr(m_out), _stream(dev)), "bgx_arena_luck_add")
                if trace:
                    tr["luck"][steps] = l_out
                    tr["luck_mean"][steps] = m_out
            if cube is not None:
                check(L.bgx_arena_cube_sel(recs, _ptr(self.sel_a), _ptr(self.sel_b), cstate[1], cstate[0], self.B,
                                           cube.cap, _ptr(cs["dsel_a"]), _ptr(cs["dsel_b"]), st), "bgx_arena_cube_sel")
                if trace:
                    eng.records(out=rec)
                    tr["cube"][steps] = cs["cube"]
                    tr["cube_mover"][steps] = rec[:, R_CUR]
                    tr["dsel"][steps] = cs["dsel_a"] + 2 * cs["dsel_b"]
                eq_a = self._equity(cube.rule_a, cs["dsel_a"], cs["eq_a"])
                eq_b = self._equity(cube.rule_b, cs["dsel_b"], cs["eq_b"])
                check(L.bgx_arena_cube_offer(recs, _ptr(cs["dsel_a"]), _ptr(cs["dsel_b"]), _ptr(eq_a), _ptr(eq_b), ra, rb,
                                             cstate[0], self.B, _ptr(cs["off_a"]), _ptr(cs["off_b"]), _ptr(cs["tally"]),
                                             st), "bgx_arena_cube_offer")
                # the doubler's equity as the other side sees it: B's on A's doubles, A's on B's
                er_b = self._equity(cube.rule_b, cs["off_a"], cs["er_b"])
                er_a = self._equity(cube.rule_a, cs["off_b"], cs["er_a"])
                check(L.bgx_arena_cube_respond(recs, _ptr(cs["off_a"]), _ptr(cs["off_b"]), _ptr(er_a), _ptr(er_b), ra, rb,
                                               self.B, self.G, *cstate, *state[:3], _ptr(self.tally), _ptr(cs["tally"]),
                                               _ptr(cs["mask"]), st), "bgx_arena_cube_respond")
                if trace:
                    nan = float("nan")
                    tr["offer"][steps] = cs["off_a"] + 2 * cs["off_b"]
                    tr["eq_offer"][steps] = torch.where(cs["dsel_a"] != 0, eq_a, torch.where(cs["dsel_b"] != 0, eq_b, nan))
                    tr["eq_resp"][steps] = torch.where(cs["off_a"] != 0, er_b, torch.where(cs["off_b"] != 0, er_a, nan))
                    tr["passed"][steps] = cs["mask"]
                eng.reset(lane_mask=cs["mask"], want_obs=False)
                check(L.bgx_arena_cube_reseat(recs, _ptr(cs["mask"]), self.B, self.G, *state[:3], st),
                      "bgx_arena_cube_reseat")
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
            if cube is not None:
                check(L.bgx_arena_cube_flush(_ptr(self.sel_a), _ptr(self.sel_b), _ptr(done), _ptr(info), state[0],
                                             self.B, int(cube.jacoby), cube.cap, *cstate, _ptr(cs["tally"]), st),
                      "bgx_arena_cube_flush")
            if luck is not None:
                check(L.bgx_arena_luck_flush(_ptr(self.sel_a), _ptr(self.sel_b), _ptr(done), _ptr(info), state[0], self.B,
                                             self.G, *lstate, _ptr(ls["tally"]), _stream(dev)), "bgx_arena_luck_flush")
            check(L.bgx_arena_advance(recs, _ptr(done), _ptr(info), self.B, self.G, *state, _stream(dev)),
                  "bgx_arena_advance")
            if trace:
                tr["done"][steps] = done
                tr["info"][steps] = info
            steps += 1
            if steps % every == 0 or steps == max_steps:
                active = int(self.tally[ACTIVE].item())
        tally = self.tally.cpu().tolist()
        if cube is not None:
            res = summarize_cube(tally, cs["tally"].cpu().tolist(), steps, tally[ACTIVE])
        elif luck is not None:
            res = summarize_luck(tally, ls["tally"].cpu().tolist(), steps, tally[ACTIVE], luck.scale)
        else:
            res = summarize(tally, steps, tally[ACTIVE])
        if trace:
            return res, {k: v[:steps] for k, v in tr.items()}
        return res


    def _play_match(self, a, b, max_steps: int, trace: bool, match):
        """play(match=...): the match path, beside the plain one."""
        from .match import ArenaMatch, summarize_match
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError(f"play: max_steps {max_steps} must be >= 0")
        if not isinstance(match, ArenaMatch):
            raise ValueError("play: match must be a match.ArenaMatch or None")
        if trace and self.B * max_steps * 2 > TRACE_LIMIT:
            raise ValueError(f"play: trace=True with match holds batch x max_steps x 2 = {self.B * max_steps * 2} "
                             f"entries in away; the limit is {TRACE_LIMIT} (it is for tests and small batches)")
        L, eng, dev = _lib.load(), self.eng, self.eng.device
        Lm, M, G = match.length, self.G, match.games_quota(self.G)
        recs, st = ctypes.c_void_p(eng.lanes_ptr()), _stream(dev)
        state = (_ptr(self.games_done), _ptr(self.sel_a), _ptr(self.sel_b), _ptr(self.tally))
        if self.match_state is None:
            u8 = lambda *s: torch.zeros(self.B, *s, dtype=torch.uint8, device=dev)      # noqa: E731
            f32 = lambda: torch.zeros(self.B, dtype=torch.float32, device=dev)          # noqa: E731
            i32 = lambda: torch.zeros(self.B, dtype=torch.int32, device=dev)            # noqa: E731
            self.match_state = dict(away=u8(2), craw=u8(), cube=u8(), plies=i32(), matches_done=i32(), seat0=u8(),
                                    retire=u8(), tally=torch.zeros(16, dtype=torch.int64, device=dev), dsel_a=u8(),
                                    dsel_b=u8(), off_a=u8(), off_b=u8(), mask=u8(), eq_a=f32(), eq_b=f32(),
                                    er_a=f32(), er_b=f32(), scratch=f32())
        ms = self.match_state
        met, pc = (_ptr(t) for t in match.tables(dev))
        ra, rb = match.rule_a.struct(), match.rule_b.struct()
        cube_p, plies_p, away_p, craw_p = (_ptr(ms[k]) for k in ("cube", "plies", "away", "craw"))
        lane = (away_p, craw_p, _ptr(ms["matches_done"]), _ptr(ms["seat0"]))
        eng.reset(want_obs=False)
        check(L.bgx_arena_begin(recs, self.B, G, *state, st), "bgx_arena_begin")
        check(L.bgx_arena_match_begin(self.B, Lm, away_p, craw_p, cube_p, plies_p, lane[2], lane[3], _ptr(ms["retire"]),
                                      _ptr(ms["tally"]), st), "bgx_arena_match_begin")
        tr = None
        if trace:
            tr = {k: torch.zeros(max_steps, self.B, *shape, dtype=dt, device=dev)
                  for k, dt, shape in (("mover", torch.uint8, ()), ("n_moves", torch.int32, ()),
                                       ("action", torch.int32, ()), ("owner", torch.uint8, ()),
                                       ("done", torch.uint8, ()), ("info", torch.int32, ()),
                                       ("away", torch.uint8, (2,)), ("craw", torch.uint8, ()),
                                       ("cube", torch.uint8, ()), ("cube_mover", torch.uint8, ()),
                                       ("dsel", torch.uint8, ()), ("offer", torch.uint8, ()),
                                       ("eq_offer", torch.float32, ()), ("eq_resp", torch.float32, ()),
                                       ("passed", torch.uint8, ()))}
            rec = torch.empty(self.B, 64, dtype=torch.uint8, device=dev)
        sync_free = getattr(a, "sync_free", False) and getattr(b, "sync_free", False) and match.sync_free
        every = SYNC_EVERY if sync_free else 1
        steps = 0
        active = int(self.tally[ACTIVE].item())
        while active > 0 and steps < max_steps:
            check(L.bgx_arena_match_sel(recs, state[1], state[2], plies_p, cube_p, away_p, craw_p, self.B,
                                        _ptr(ms["dsel_a"]), _ptr(ms["dsel_b"]), st), "bgx_arena_match_sel")
            if trace:
                eng.records(out=rec)
                tr["away"][steps] = ms["away"]
                tr["craw"][steps] = ms["craw"]
                tr["cube"][steps] = ms["cube"]
                tr["cube_mover"][steps] = rec[:, R_CUR]
                tr["dsel"][steps] = ms["dsel_a"] + 2 * ms["dsel_b"]
            eq_a = self._equity(match.rule_a, ms["dsel_a"], ms["eq_a"], ms["scratch"])
            eq_b = self._equity(match.rule_b, ms["dsel_b"], ms["eq_b"], ms["scratch"])
            check(L.bgx_arena_match_offer(recs, state[1], state[2], _ptr(ms["dsel_a"]), _ptr(ms["dsel_b"]), _ptr(eq_a),
                                          _ptr(eq_b), ra, rb, met, pc, Lm, plies_p, cube_p, away_p, craw_p, self.B,
                                          _ptr(ms["off_a"]), _ptr(ms["off_b"]), _ptr(ms["tally"]), st),
                  "bgx_arena_match_offer")
            # the doubler's value as the other side sees it: B's on A's doubles, A's on B's
            er_b = self._equity(match.rule_b, ms["off_a"], ms["er_b"], ms["scratch"])
            er_a = self._equity(match.rule_a, ms["off_b"], ms["er_a"], ms["scratch"])
            check(L.bgx_arena_match_respond(recs, _ptr(ms["off_a"]), _ptr(ms["off_b"]), _ptr(er_a), _ptr(er_b), ra, rb,
                                            met, pc, Lm, self.B, G, M, cube_p, plies_p, *lane, *state[:3],
                                            _ptr(self.tally), _ptr(ms["tally"]), _ptr(ms["mask"]), st),
                  "bgx_arena_match_respond")
            if trace:
                nan = float("nan")
                tr["offer"][steps] = ms["off_a"] + 2 * ms["off_b"]
                tr["eq_offer"][steps] = torch.where(ms["dsel_a"] != 0, eq_a, torch.where(ms["dsel_b"] != 0, eq_b, nan))
                tr["eq_resp"][steps] = torch.where(ms["off_a"] != 0, er_b, torch.where(ms["off_b"] != 0, er_a, nan))
                tr["passed"][steps] = ms["mask"]
            eng.reset(lane_mask=ms["mask"], want_obs=False)
            check(L.bgx_arena_cube_reseat(recs, _ptr(ms["mask"]), self.B, G, *state[:3], st), "bgx_arena_cube_reseat")
            act_a = self._act(a, self.sel_a, steps)
            act_b = self._act(b, self.sel_b, steps)
            check(L.bgx_arena_merge(state[1], state[2], _ptr(act_a), _ptr(act_b), self.B, _ptr(self.actions), st),
                  "bgx_arena_merge")
            if trace:
                eng.records(out=rec)
                tr["mover"][steps] = rec[:, R_CUR]
                tr["n_moves"][steps] = rec[:, R_NM0].to(torch.int32) | (rec[:, R_NM1].to(torch.int32) << 8)
                tr["action"][steps] = self.actions
                tr["owner"][steps] = self.sel_a + 2 * self.sel_b
            _, _, done, info = eng.step(self.actions, want_obs=False, want_info=True)
            check(L.bgx_arena_match_flush(state[1], state[2], _ptr(done), _ptr(info), state[0], self.B, Lm, M, cube_p,
                                          plies_p, *lane, _ptr(ms["retire"]), _ptr(ms["tally"]), st),
                  "bgx_arena_match_flush")
            check(L.bgx_arena_advance(recs, _ptr(done), _ptr(info), self.B, G, *state, st), "bgx_arena_advance")
            check(L.bgx_arena_match_retire(self.B, G, _ptr(ms["retire"]), *state, st), "bgx_arena_match_retire")
            if trace:
                tr["done"][steps] = done
                tr["info"][steps] = info
            steps += 1
            if steps % every == 0 or steps == max_steps:
                active = int(self.tally[ACTIVE].item())
        tally = self.tally.cpu().tolist()
        res = summarize_match(tally, ms["tally"].cpu().tolist(), steps, tally[ACTIVE])
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


CUBE_SIDE_DEFAULTS = {"cube_double": 0.40, "cube_pass": 0.50, "cube_too_good": math.inf, "cube_scale": 1.0,
                      "cube_net": None, "cube_lookahead": 1}


class _Parser(argparse.ArgumentParser):
    """The move-filter options are an error for any player but a 2ply one with weights; a cube
    option is an error without --cube, a side's cube option for a `random` side (it has no rule);
    --luck is an error with --cube and, without --luck-net, for two `random` sides; --luck-net and
    --luck-scale need --luck."""

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
        for side in "ab":
            given = [k for k in CUBE_SIDE_DEFAULTS if getattr(ns, f"{k}_{side}") is not None]
            flags = ", ".join("--" + k.replace("_", "-") + "-" + side for k in given)
            if given and not ns.cube:
                self.error(f"{flags} need --cube")
            if given and getattr(ns, side) == "random":
                self.error(f"{flags}: a random side has no cube rule")
            for k in ("cube_double", "cube_pass", "cube_scale", "cube_too_good"):
                v = getattr(ns, f"{k}_{side}")
                if v is not None and math.isnan(v):
                    self.error(f"--{k.replace('_', '-')}-{side} is NaN")
            for k, v in CUBE_SIDE_DEFAULTS.items():
                if getattr(ns, f"{k}_{side}") is None:
                    setattr(ns, f"{k}_{side}", v)
        if not ns.cube and (ns.jacoby or ns.cube_cap is not None):
            self.error("--jacoby / --cube-cap need --cube")
        if ns.cube_cap is None:
            ns.cube_cap = 6
        if not 0 <= ns.cube_cap <= 10:
            self.error("--cube-cap takes a number in 0..10")
        if not ns.luck and (ns.luck_net is not None or ns.luck_scale is not None):
            self.error("--luck-net / --luck-scale need --luck")
        if ns.luck and ns.cube:
            self.error("--luck with --cube is not implemented (the cubeful arena's luck)")
        if ns.luck and ns.luck_net is None and ns.a == "random" and ns.b == "random":
            self.error("--luck needs a value head: both sides are random, give --luck-net")
        if ns.luck_scale is None:
            ns.luck_scale = "fit"
        self._match_args(ns)
        return ns

    def _match_args(self, ns):
        """--match N: not with --cube or --luck; a --match-* option needs it, a side's for a side
        with weights."""
        if ns.match is not None and (ns.cube or ns.luck):
            self.error("--match with --cube or --luck is not implemented")
        if ns.match is not None and not 1 <= ns.match <= 25:
            self.error("--match takes a match length in 1..25")
        if ns.met is not None and ns.match is None:
            self.error("--met needs --match")
        for side in "ab":
            given = [k for k in MATCH_SIDE_DEFAULTS if getattr(ns, f"{k}_{side}") is not None]
            flags = ", ".join("--" + k.replace("_", "-") + "-" + side for k in given)
            if given and ns.match is None:
                self.error(f"{flags} need --match")
            if given and getattr(ns, side) == "random":
                self.error(f"{flags}: a random side has no match rule")
            for k, v in MATCH_SIDE_DEFAULTS.items():
                if getattr(ns, f"{k}_{side}") is None:
                    setattr(ns, f"{k}_{side}", v)
            if math.isnan(getattr(ns, f"match_scale_{side}")):
                self.error(f"--match-scale-{side} is NaN")
            if not 0.0 <= getattr(ns, f"match_window_{side}") <= 1.0:
                self.error(f"--match-window-{side} takes a number in [0, 1]")


MATCH_SIDE_DEFAULTS = {"match_window": 0.65, "match_gammons": (0.25, 0.25), "match_lookahead": 1, "match_net": None,
                       "match_scale": 1.0}


def _gammon_shares(text: str):
    try:
        w, l = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--match-gammons takes W,L (two shares in [0, 1]), got {text!r}")
    if not (0.0 <= w <= 1.0 and 0.0 <= l <= 1.0):
        raise argparse.ArgumentTypeError(f"--match-gammons takes two shares in [0, 1], got {text!r}")
    return w, l


def _luck_scale(text: str):
    if text == "fit":
        return text
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--luck-scale takes 'fit' or a number, got {text!r}")
    if math.isnan(v):
        raise argparse.ArgumentTypeError("--luck-scale is NaN")
    return v


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
    ap.add_argument("--cube", action="store_true",
                    help="money play with the doubling cube: each side doubles, takes and passes by its own rule on "
                         "its own net's equity; the result is A's cubeful points per game")
    ap.add_argument("--cube-cap", type=int, default=None, help="no double once the cube shows 2^cap (0..10; default 6)")
    ap.add_argument("--jacoby", action="store_true", help="a game that ends with the cube centred at 1 counts 1 point")
    for side in "ab":
        S = side.upper()
        ap.add_argument(f"--cube-double-{side}", type=float, default=None,
                        help=f"{S} doubles from this equity on (default 0.40)")
        ap.add_argument(f"--cube-pass-{side}", type=float, default=None,
                        help=f"{S} passes a double above this equity of the doubler (default 0.50)")
        ap.add_argument(f"--cube-too-good-{side}", type=float, default=None,
                        help=f"{S} plays on undoubled above this equity (default inf)")
        ap.add_argument(f"--cube-scale-{side}", type=float, default=None,
                        help=f"points per unit of {S}'s value (default 1.0)")
        ap.add_argument(f"--cube-net-{side}", default=None, metavar="PATH",
                        help=f"the net whose value head gives {S}'s equity (default: {S}'s own weights)")
        ap.add_argument(f"--cube-lookahead-{side}", type=int, default=None, choices=[0, 1],
                        help=f"{S}'s equity: 0 the head's static value (sync-free), 1 its mean best 1-ply value over "
                             "the 21 rolls (default)")
    ap.add_argument("--luck", action="store_true",
                    help="luck-adjusted result: every roll's luck is a control variate (adds ppg_luck_a, "
                         "ppg_luck_stderr, variance_ratio, luck_scale, luck_mean); costs one 1-ply search over the 21 "
                         "rolls per step")
    ap.add_argument("--luck-net", default=None, metavar="PATH",
                    help="the net whose value head gives the luck (default: A's weights, else B's)")
    ap.add_argument("--luck-scale", type=_luck_scale, default=None, metavar="fit|FLOAT",
                    help="the control variate's coefficient: 'fit' (default) or a fixed number")
    ap.add_argument("--match", type=int, default=None, metavar="N",
                    help="matches to N points (1..25) with the Crawford rule and cube decisions on a match equity "
                         "table; --games-per-lane then counts matches and the result is A's match win rate")
    ap.add_argument("--met", default=None, metavar="FILE",
                    help="the match equity table, JSON {length, met, post_crawford} (match.load_met; its length must "
                         "be N; default: match.met_table(N), a cubeless-play table)")
    for side in "ab":
        S = side.upper()
        ap.add_argument(f"--match-window-{side}", type=float, default=None,
                        help=f"{S} doubles from this share of the way between the dead-cube doubling point (0) and "
                             "the cash point (1) on (default 0.65)")
        ap.add_argument(f"--match-gammons-{side}", type=_gammon_shares, default=None, metavar="W,L",
                        help=f"the share of {S}'s wins and of its losses that are gammons (default 0.25,0.25)")
        ap.add_argument(f"--match-lookahead-{side}", type=int, default=None, choices=[0, 1],
                        help=f"{S}'s value: 0 the head's static value (sync-free), 1 its mean best 1-ply value over "
                             "the 21 rolls (default)")
        ap.add_argument(f"--match-net-{side}", default=None, metavar="PATH",
                        help=f"the net whose value head gives {S}'s value (default: {S}'s own weights)")
        ap.add_argument(f"--match-scale-{side}", type=float, default=None,
                        help=f"points per unit of {S}'s value (default 1.0)")
    return ap


def match_from_args(args, nets, device):
    """The match.ArenaMatch of a parsed command line (None without --match): a side with weights
    gets a MatchRule on its --match-net-x, else its own net; a random side has no rule."""
    if args.match is None:
        return None
    from .match import ArenaMatch, MatchRule, load_met
    from .search import ValueHead
    met = None
    if args.met is not None:
        length, *met = load_met(args.met)
        if length != args.match:
            raise ValueError(f"--met {args.met} is a table for matches to {length}, --match asks for {args.match}")
    rules = []
    for side, net in zip("ab", nets):
        if net is None:
            rules.append(None)
            continue
        path = getattr(args, f"match_net_{side}")
        w, l = getattr(args, f"match_gammons_{side}")
        rules.append(MatchRule(ValueHead(net if path is None else load_net(path, device)),
                               scale=getattr(args, f"match_scale_{side}"), window=getattr(args, f"match_window_{side}"),
                               win_gammons=w, loss_gammons=l, lookahead=getattr(args, f"match_lookahead_{side}")))
    return ArenaMatch(args.match, *rules, met=met)


def luck_from_args(args, nets, device):
    """The ArenaLuck of a parsed command line (None without --luck): on --luck-net's value head,
    else A's weights, else B's."""
    if not args.luck:
        return None
    from .search import ValueHead
    net = load_net(args.luck_net, device) if args.luck_net is not None else nets[0] if nets[0] is not None else nets[1]
    return ArenaLuck(ValueHead(net), scale=args.luck_scale)


def cube_from_args(args, nets, device):
    """The ArenaCube of a parsed command line (None without --cube): a side with weights gets a
    CubeRule on its --cube-net-x, else its own net; a random side has no rule."""
    if not args.cube:
        return None
    from .cube import CubeRule
    from .search import ValueHead
    rules = []
    for side, net in zip("ab", nets):
        if net is None:
            rules.append(None)
            continue
        path = getattr(args, f"cube_net_{side}")
        vh = ValueHead(net if path is None else load_net(path, device))
        rules.append(CubeRule(vh, scale=getattr(args, f"cube_scale_{side}"), double_at=getattr(args, f"cube_double_{side}"),
                              pass_at=getattr(args, f"cube_pass_{side}"), too_good_at=getattr(args, f"cube_too_good_{side}"),
                              cap=args.cube_cap, jacoby=args.jacoby, lookahead=getattr(args, f"cube_lookahead_{side}")))
    return ArenaCube(*rules)


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
    cube = cube_from_args(args, nets, dev)
    luck = luck_from_args(args, nets, dev)
    match = match_from_args(args, nets, dev)
    res = arena.play(players[0], players[1], max_steps=args.max_steps, cube=cube, **({"luck": luck} if luck else {}),
                     **({"match": match} if match else {}))
    dt = time.perf_counter() - t0
    if luck is not None:
        res.update(luck=True, luck_net=args.luck_net)
    if match is not None:
        res.update(match=args.match, met=args.met, matches_per_s=res["matches"] / dt if dt > 0 else 0.0,
                   **{f"{k}_{side}": getattr(args, f"{k}_{side}")
                      for side, n in zip("ab", nets) if n is not None for k in MATCH_SIDE_DEFAULTS})
    res.update(a=args.a, b=args.b, player_a="random" if nets[0] is None else args.player_a,
               player_b="random" if nets[1] is None else args.player_b, batch=args.batch,
               games_per_lane=args.games_per_lane, max_steps=args.max_steps, seed=args.seed, seconds=dt,
               top_k_a=args.top_k_a, top_k_b=args.top_k_b, margin_a=args.margin_a, margin_b=args.margin_b,
               bearoff_a=args.bearoff_a, bearoff_b=args.bearoff_b,
               **{k: v for k, v in (("bearoff1_a", args.bearoff1_a), ("bearoff1_b", args.bearoff1_b)) if v is not None},
               **({"cube": True, "cube_cap": args.cube_cap, "jacoby": args.jacoby,
                   **{f"{k}_{side}": None if getattr(args, f"{k}_{side}") == math.inf else getattr(args, f"{k}_{side}")
                      for side, n in zip("ab", nets) if n is not None for k in CUBE_SIDE_DEFAULTS}}
                  if args.cube else {}),
               games_per_s=res["games"] / dt if dt > 0 else 0.0,
               env_steps_per_s=res["steps"] * args.batch / dt if dt > 0 else 0.0)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
