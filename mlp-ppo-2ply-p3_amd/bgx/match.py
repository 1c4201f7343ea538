"""Match play in the head-to-head arena (csrc/bg_match.h; include/bgx.h "match
play in the arena"): matches to L points with the Crawford rule, cube decisions that maximise the
chance of winning the match on a match equity table (MET), and a result counted in matches.

    python -m bgx.arena --a new.pt --b old.pt --max-steps 20000 --match 7 --games-per-lane 1

This module holds the table (met_table, load_met, save_met), the rule of a side (MatchRule), the
pair of rules with the table (ArenaMatch), the summary (summarize_match) and the host references
of the kernels: match_decision_reference (part 1 of csrc/bg_match.h on arrays, bit for bit in numpy
float32) and arena_match_reference (the replay of a traced run).  Arena.play(match=...) of
bgx/arena.py drives the device side.
"""
from __future__ import annotations

import json
import math

import numpy as np
import torch

from . import _lib
from .arena import ACTIVE, FIELDS, summarize
from .cube import MAX_CAP, CubeRule

MAX_LENGTH = 25                 # csrc/bg_match.h kMatchMaxLength
# match_tally int64[16] (include/bgx.h bgx_arena_match_field)
MATCH_FIELDS = ("matches", "match_wins_a", "match_games", "pass_games", "match_points_a", "match_points_b",
                "doubles_a", "doubles_b", "passes_a", "passes_b", "cube_log2", "crawford_games",
                "post_crawford_games", "pass_plies", "match_wins_a_seat0", "matches_seat0")
F = np.float32


# -------------------------------------------------------------------- the table --
def _check_length(length, what):
    if isinstance(length, bool) or int(length) != length or not 1 <= int(length) <= MAX_LENGTH:
        raise ValueError(f"{what}: the match length must be in 1..{MAX_LENGTH}, got {length!r}")
    return int(length)


def met_table(length: int, gammon: float = 0.26, backgammon: float = 0.012):
    """(met float32[L + 1, L + 1], pc float32[L + 1]) for matches to `length` = L points: met[i, j]
    is the chance that the side needing i points wins the match against the side needing j at the
    start of a game, rows and columns at 1 the Crawford game's values; pc[j] is the trailer's chance
    after the Crawford game when it needs j and the leader 1.  Row and column 0 are never read
    (met[0, j] = 1, met[i, 0] = 0, pc[0] = 1).

    This is a CUBELESS-PLAY table: each game is won by either side with probability 1/2 and is
    worth 1, 2 or 3 points with r1 = 1 - g - b, r2 = g = `gammon`, r3 = b = `backgammon`; before the
    Crawford game it ignores what the cube is worth (a cubeful MET is out of scope).
    After the Crawford game every game is played at 2, the trailer's free double:
        pc[1] = 0.5,  pc[j] = 0.5 (r1 PC(j - 2) + r2 PC(j - 4) + r3 PC(j - 6)),  PC(<= 0) = 1
    the Crawford game, the leader needing 1 against j >= 2:
        met[1, j] = 0.5 + 0.5 sum_s r_s (1 - PC(j - s)),  met[j, 1] = 1 - met[1, j],  met[1, 1] = 0.5
    and before it, i, j >= 2, with M'(a, b) = 1 for a <= 0 and met[a, b] otherwise (the Crawford
    row where a side reaches 1):
        met[i, j] = 0.5 sum_s r_s M'(i - s, j) + 0.5 sum_s r_s (1 - M'(j - s, i))
    The recurrence runs in fp64 and is rounded to fp32 once."""
    L = _check_length(length, "met_table")
    g, b = float(gammon), float(backgammon)
    if not (0.0 <= g and 0.0 <= b and g + b <= 1.0):
        raise ValueError(f"met_table: gammon {gammon!r} and backgammon {backgammon!r} must be rates with sum <= 1")
    r = (1.0 - g - b, g, b)
    pc = np.ones(L + 1, np.float64)
    PC = lambda j: 1.0 if j <= 0 else pc[j]                                     # noqa: E731
    if L >= 1:
        pc[1] = 0.5
    for j in range(2, L + 1):
        pc[j] = 0.5 * sum(r[s - 1] * PC(j - 2 * s) for s in (1, 2, 3))
    M = np.zeros((L + 1, L + 1), np.float64)
    M[0, :] = 1.0
    M[0, 0] = 0.5
    M[1, 1] = 0.5
    for j in range(2, L + 1):
        M[1, j] = 0.5 + 0.5 * sum(r[s - 1] * (1.0 - PC(j - s)) for s in (1, 2, 3))
        M[j, 1] = 1.0 - M[1, j]
    Mp = lambda a, c: 1.0 if a <= 0 else M[a, c]                                # noqa: E731
    for n in range(4, 2 * L + 1):
        for i in range(max(2, n - L), min(L, n - 2) + 1):
            j = n - i
            M[i, j] = (0.5 * sum(r[s - 1] * Mp(i - s, j) for s in (1, 2, 3))
                       + 0.5 * sum(r[s - 1] * (1.0 - Mp(j - s, i)) for s in (1, 2, 3)))
    return M.astype(F), pc.astype(F)


def check_met(length: int, met, pc):
    """Validates a table for matches to `length`: met [L + 1, L + 1] and pc [L + 1] (row, column and
    entry 0 are not read and not checked), finite values in [0, 1], met[i, j] + met[j, i] = 1
    within 1e-6 and pc[1] = 0.5 within 1e-6.  Returns (met, pc) as contiguous float32 arrays."""
    L = _check_length(length, "check_met")
    try:
        m, p = np.asarray(met, np.float64), np.asarray(pc, np.float64)
    except (TypeError, ValueError):
        raise ValueError("check_met: the table is not a rectangular array of numbers")
    if m.shape != (L + 1, L + 1) or p.shape != (L + 1,):
        raise ValueError(f"check_met: a match to {L} needs met [{L + 1}, {L + 1}] and post_crawford [{L + 1}], got "
                         f"{m.shape} and {p.shape}")
    mi, pi = m[1:, 1:], p[1:]
    if not (np.isfinite(mi).all() and np.isfinite(pi).all() and (mi >= 0).all() and (mi <= 1).all()
            and (pi >= 0).all() and (pi <= 1).all()):
        raise ValueError("check_met: every value must be a probability in [0, 1]")
    if np.abs(mi + mi.T - 1.0).max() > 1e-6:
        raise ValueError("check_met: met[i][j] + met[j][i] must be 1 within 1e-6")
    if abs(pi[0] - 0.5) > 1e-6:
        raise ValueError("check_met: post_crawford[1] must be 0.5")
    return np.ascontiguousarray(m, F), np.ascontiguousarray(p, F)


def load_met(path: str):
    """(length, met, pc) from a JSON file {"length": L, "met": [[...]], "post_crawford": [...]} with
    met [L + 1][L + 1] and post_crawford [L + 1] indexed by points still needed (index 0 unused),
    validated by check_met."""
    with open(path) as fh:
        d = json.load(fh)
    if not isinstance(d, dict) or not {"length", "met", "post_crawford"} <= set(d):
        raise ValueError(f"load_met: {path} needs the keys length, met and post_crawford")
    L = _check_length(d["length"], "load_met")
    met, pc = check_met(L, d["met"], d["post_crawford"])
    return L, met, pc


def save_met(path: str, length: int, met, pc):
    """Writes load_met's file (fp32 values print exactly as Python floats)."""
    met, pc = check_met(length, met, pc)
    with open(path, "w") as fh:
        json.dump({"length": int(length), "met": [[float(v) for v in row] for row in met],
                   "post_crawford": [float(v) for v in pc]}, fh)


# ---------------------------------------------------------------------- the rule --
class MatchRule(CubeRule):
    """The match cube rule of one side (csrc/bg_match.h part 1).  `value` and `lookahead` are
    CubeRule's, with its equity() and sync_free: the value of the side on roll, a search.ValueHead
    or a callable.  `scale` turns the value's unit into points.  From c = scale * value the side
    takes the win probability p = (c + 1 + gl) / (2 + gw + gl), c clamped to [-(1 + gl), 1 + gw],
    with gw = `win_gammons` and gl = `loss_gammons` the share of its wins and of its losses that
    are gammons (swapped when it answers a double: it then evaluates the doubler's chances).  With
    ND, DT and DP the match-winning chances of the side on roll at no double, double/take and
    double/pass, it doubles iff ND <= DP and DT - ND >= `window` (DP - ND) -- window 0 is the
    dead-cube doubling point, 1 the cash point -- or the double is free; it passes iff DT > DP.
    The defaults are parameters of the rule, not claims about the best ones."""

    def __init__(self, value, scale: float = 1.0, window: float = 0.65, win_gammons: float = 0.25,
                 loss_gammons: float = 0.25, lookahead: int = 1):
        super().__init__(value, scale=scale, lookahead=lookahead)
        for name, v in (("window", window), ("win_gammons", win_gammons), ("loss_gammons", loss_gammons)):
            if not 0.0 <= float(v) <= 1.0:                  # a NaN fails it
                raise ValueError(f"MatchRule: {name} must be in [0, 1], got {v!r}")
        self.window, self.win_gammons, self.loss_gammons = float(window), float(win_gammons), float(loss_gammons)

    def struct(self) -> _lib.BgxMatchRule:
        return _lib.BgxMatchRule(self.scale, self.window, self.win_gammons, self.loss_gammons)


class _NanValue:
    """The value of a side without a rule: NaN, which never offers and never passes."""
    sync_free = True

    def __init__(self):
        self.v = None

    def __call__(self, eng, dsel):
        if self.v is None or self.v.numel() != eng.batch or self.v.device != eng.device:
            self.v = torch.full((eng.batch,), float("nan"), dtype=torch.float32, device=eng.device)
        return self.v


class ArenaMatch:
    """Match play of an arena run: matches to `length` points, `rule_a` and
    `rule_b` A's and B's MatchRule, `met` = (met, pc) as met_table returns them, or None for
    met_table(length).  Either rule may be None: that side never doubles and takes every double (a
    MatchRule on a constant callable whose value is NaN, which cannot offer or pass, so the kernels
    need no special case).  With two None sides the cube stays at 1 and the match is plain points
    up to `length` with the Crawford rule idle."""

    def __init__(self, length: int, rule_a=None, rule_b=None, met=None):
        self.length = _check_length(length, "ArenaMatch")
        for r in (rule_a, rule_b):
            if r is not None and not isinstance(r, MatchRule):
                raise ValueError("ArenaMatch: a rule must be a match.MatchRule or None")
        if met is None:
            met = met_table(self.length)
        if not isinstance(met, (tuple, list)) or len(met) != 2:
            raise ValueError("ArenaMatch: met must be (met, pc) or None")
        self.met, self.pc = check_met(self.length, *met)
        self.has_a, self.has_b = rule_a is not None, rule_b is not None
        self.rule_a = rule_a if rule_a is not None else MatchRule(_NanValue())
        self.rule_b = rule_b if rule_b is not None else MatchRule(_NanValue())
        self.sync_free = self.rule_a.sync_free and self.rule_b.sync_free
        self._dev = None

    def games_quota(self, matches_per_lane: int) -> int:
        """G of the arena's game-counting kernels: matches_per_lane (2 L - 1), which no lane reaches
        by playing since every game gives somebody a point."""
        g = int(matches_per_lane) * (2 * self.length - 1)
        if g >= 2 ** 31:
            raise ValueError(f"ArenaMatch: {matches_per_lane} matches to {self.length} per lane do not fit the int32 "
                             "game count")
        return g

    def tables(self, device):
        """(met, pc) as float32 tensors on `device`, made once."""
        if self._dev is None or self._dev[0].device != device:
            self._dev = (torch.from_numpy(self.met.reshape(-1).copy()).to(device),
                         torch.from_numpy(self.pc.copy()).to(device))
        return self._dev


# ------------------------------------------------------------------- the summary --
def summarize_match(tally, match_tally, steps: int, unfinished: int) -> dict:
    """The match result from the plain tally (the games played to the end) and the 16 match sums
    (MATCH_FIELDS), from the integers: `matches`, `match_wins_a`, `match_win_rate_a` = w,
    `match_win_rate_stderr` = sqrt(w (1 - w) / n) (None below 2 matches), `games` (played out +
    passed, those of unfinished matches included), `games_per_match`, `doubles_per_game_a` / `_b`,
    `take_share_a` / `_b` (of the doubles offered TO the side, the share it took),  `pass_share`,
    `mean_cube_log2`, `crawford_share` and `post_crawford_share` (of the games),
    `match_win_rate_a_first_seat` (A's win rate in the matches whose first game it played as
    PLAYER1), the 16 sums under their names, `steps`, `unfinished_lanes` and `played_out` =
    summarize(tally, ...).  Without matches or games the rates are 0.  Raises ValueError on broken
    invariants: wins > matches (also within the first-seat matches), passes > the other side's
    doubles, PASS_GAMES != PASSES_A + PASSES_B or GAMES != the plain tally's games + PASS_GAMES."""
    played = summarize(tally, steps, unfinished)
    m = [int(v) for v in match_tally]
    if len(m) < len(MATCH_FIELDS):
        raise ValueError(f"summarize_match: the match tally has {len(m)} entries, needs {len(MATCH_FIELDS)}")
    r = dict(zip(MATCH_FIELDS, m))
    n, g = r["matches"], r["match_games"]
    if r["match_wins_a"] > n or r["matches_seat0"] > n or r["match_wins_a_seat0"] > min(r["matches_seat0"],
                                                                                       r["match_wins_a"]):
        raise ValueError(f"summarize_match: {r['match_wins_a']} wins ({r['match_wins_a_seat0']} of "
                         f"{r['matches_seat0']} from the first seat) in {n} matches")
    if r["passes_a"] > r["doubles_b"] or r["passes_b"] > r["doubles_a"]:
        raise ValueError(f"summarize_match: A gave up {r['passes_a']} of B's {r['doubles_b']} doubles, B "
                         f"{r['passes_b']} of A's {r['doubles_a']}")
    if r["pass_games"] != r["passes_a"] + r["passes_b"]:
        raise ValueError(f"summarize_match: {r['pass_games']} passed games, but A gave up {r['passes_a']} and B "
                         f"{r['passes_b']}")
    if g != played["games"] + r["pass_games"]:
        raise ValueError(f"summarize_match: the match tally counts {g} games, the plain tally {played['games']} and "
                         f"{r['pass_games']} passed")

    def ratio(a, b):
        return a / b if b > 0 else 0.0

    w = ratio(r["match_wins_a"], n)
    r.update(games=g, match_win_rate_a=w,
             match_win_rate_stderr=math.sqrt(max(w * (1.0 - w), 0.0) / n) if n >= 2 else None,
             games_per_match=ratio(g, n), doubles_per_game_a=ratio(r["doubles_a"], g),
             doubles_per_game_b=ratio(r["doubles_b"], g),
             take_share_a=1.0 - r["passes_a"] / r["doubles_b"] if r["doubles_b"] > 0 else 0.0,
             take_share_b=1.0 - r["passes_b"] / r["doubles_a"] if r["doubles_a"] > 0 else 0.0,
             pass_share=ratio(r["pass_games"], g), mean_cube_log2=ratio(r["cube_log2"], g),
             crawford_share=ratio(r["crawford_games"], g), post_crawford_share=ratio(r["post_crawford_games"], g),
             match_win_rate_a_first_seat=ratio(r["match_wins_a_seat0"], r["matches_seat0"]), steps=int(steps),
             unfinished_lanes=int(unfinished), played_out=played)
    return r


# ---------------------------------------------------------------- host references --
def _met_after(met2, pc, L, me, opp, craw):
    """met_after of csrc/bg_match.h on int64 arrays."""
    mc, oc = np.clip(me, 1, L), np.clip(opp, 1, L)
    post = np.where(mc == 1, (F(1.0) - pc[oc]).astype(F), pc[mc]).astype(F)
    r = np.where(craw != 0, post, met2[mc, oc]).astype(F)
    r = np.where(opp <= 0, F(0.0), r)
    return np.where(me <= 0, F(1.0), r).astype(F)


def _match_p(scale, v, gw, gl):
    W, L_ = F(1.0) + F(gw), F(1.0) + F(gl)
    c = (F(scale) * v).astype(F)
    c = np.where(c < -L_, -L_, np.where(c > W, W, c)).astype(F)         # comparisons: a NaN stays a NaN
    return ((c + L_).astype(F) / (W + L_)).astype(F)


def _match_values(met2, pc, L, x, y, craw, k, p, gw, gl):
    gw, gl = F(gw), F(gl)
    ma = lambda me, opp: _met_after(met2, pc, L, me, opp, craw)         # noqa: E731

    def win(n):
        return ((F(1.0) - gw) * ma(x - n, y) + gw * ma(x - 2 * n, y)).astype(F)

    def loss(n):
        return ((F(1.0) - gl) * (F(1.0) - ma(y - n, x)).astype(F) + gl * (F(1.0) - ma(y - 2 * n, x)).astype(F)).astype(F)

    v = np.int64(1) << k
    w1, l1, w2, l2 = win(v), loss(v), win(2 * v), loss(2 * v)
    nd = (l1 + (p * (w1 - l1).astype(F)).astype(F)).astype(F)
    dt = (l2 + (p * (w2 - l2).astype(F)).astype(F)).astype(F)
    return nd, dt, ma(x - v, y)


def match_decision_reference(met, pc, length: int, x, y, craw, cube, mover, plies, value_offer, rule_offer,
                             value_resp=None, rule_resp=None, over=False, active=True) -> dict:
    """Part 1 of csrc/bg_match.h on arrays, bit for bit in numpy float32 (each product, sum and
    difference a float32 operation of its own).  The side on roll needs `x`, the other `y`; `craw`
    the game's Crawford state, `cube` the cube byte, `mover` the record's mover byte, `plies` the
    game's steps so far, `over` / `active` the record's game_over and the lane's activity.
    `value_offer` is the value the side on roll decides on by `rule_offer`, `value_resp` the doubler's
    value as the other side sees it, answered by `rule_resp` (both default to the offer's).  A rule
    is anything with scale, window, win_gammons and loss_gammons.  Returns dict of arrays: p, nd,
    dt, dp (the side on roll's, by rule_offer), access, offer (access and the rule says double),
    p_resp, dt_resp, dp_resp, passes (the answer to a double, whether or not one is offered) and
    passed (offer and passes)."""
    L = _check_length(length, "match_decision_reference")
    met2, pc = np.asarray(met, F).reshape(L + 1, L + 1), np.asarray(pc, F).reshape(L + 1)
    x, y, craw, cube, mover, plies, over, active, vo, vr = np.broadcast_arrays(
        *(np.asarray(a) for a in (x, y, craw, cube, mover, plies, over, active, value_offer,
                                  value_offer if value_resp is None else value_resp)))
    x, y, craw, plies = x.astype(np.int64), y.astype(np.int64), craw.astype(np.int64), plies.astype(np.int64)
    cube, mover, vo, vr = cube.astype(np.int64), mover.astype(np.int64) & 1, vo.astype(F), vr.astype(F)
    rr = rule_offer if rule_resp is None else rule_resp
    k = np.minimum(cube & 15, MAX_CAP)
    o = (cube >> 4) & 3
    o = np.where(o == 3, 0, o)
    v = np.int64(1) << k
    access = ((plies > 0) & ~over.astype(bool) & active.astype(bool) & (craw != 1) & (k < MAX_CAP)
              & ((o == 0) | (o == mover + 1)) & (x > v))
    with np.errstate(invalid="ignore", over="ignore"):
        p = _match_p(rule_offer.scale, vo, rule_offer.win_gammons, rule_offer.loss_gammons)
        nd, dt, dp = _match_values(met2, pc, L, x, y, craw, k, p, rule_offer.win_gammons, rule_offer.loss_gammons)
        window = (dt - nd).astype(F) >= (F(rule_offer.window) * (dp - nd).astype(F)).astype(F)
        offer = access & (nd <= dp) & (window | ((y <= v) & (dt > nd)))
        pr = _match_p(rr.scale, vr, rr.loss_gammons, rr.win_gammons)
        _, dtr, dpr = _match_values(met2, pc, L, x, y, craw, k, pr, rr.loss_gammons, rr.win_gammons)
        passes = dtr > dpr
    return dict(p=p, nd=nd, dt=dt, dp=dp, access=access, offer=offer, p_resp=pr, dt_resp=dtr, dp_resp=dpr,
                passes=passes, passed=offer & passes)


def end_game_reference(away, craw, length: int, winner: int, points: int):
    """match_end_game of csrc/bg_match.h on one lane: (away (A, B), craw, match over) after a game
    worth `points` to side `winner` (0 A, 1 B)."""
    a = [int(away[0]), int(away[1])]
    left = a[winner] - int(points)
    if left <= 0:
        return (int(length), int(length)), 0, True
    a[winner] = left
    c = int(craw)
    if c == 0 and left == 1:
        c = 1
    elif c == 1:
        c = 2
    return (a[0], a[1]), c, False


def arena_match_reference(trace, batch: int, matches_per_lane: int, match: ArenaMatch) -> dict:
    """A traced match run (Arena.play(trace=True, match=...)) replayed on the host with the
    kernels' arithmetic (include/bgx.h bgx_arena_match_*).  Read from the trace, [steps, B] each:
    cube_mover (the side on roll before the decision), eq_offer (the value the side on roll
    decided on), eq_resp (the doubler's value as the other side estimated it), done and info; the
    lane records are taken as not game_over, which holds between the steps of an auto-reset engine.
    Returns dict(tally int64[16], match_tally int64[16], games_done int64[B] (G = matches_per_lane
    (2 L - 1) on a retired lane), matches_done int64[B], and per step the states before each
    decision: away uint8[steps, B, 2], craw and cube uint8[steps, B]; dsel / offer uint8 (0 none, 1
    A, 2 B) and passed bool)."""
    def arr(key, dt):
        return np.asarray(torch.as_tensor(trace[key]).cpu()).astype(dt)

    mover, done, info = arr("cube_mover", np.int64), arr("done", np.int64), arr("info", np.int64)
    eq_offer, eq_resp = arr("eq_offer", F), arr("eq_resp", F)
    B, M, L, T = int(batch), int(matches_per_lane), match.length, done.shape[0]
    G = match.games_quota(M)
    ra, rb = match.rule_a, match.rule_b
    lane = np.arange(B, dtype=np.int64)
    away, craw, cube = np.full((B, 2), L, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    plies, games, matches = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    seat0 = ((lane & 1) == 0)
    tally, mt = np.zeros(16, np.int64), np.zeros(16, np.int64)
    if M <= 0:
        games[:] = G
    s_away, s_craw, s_cube = np.zeros((T, B, 2), np.uint8), np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
    dsels, offers, passes = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8), np.zeros((T, B), bool)
    F_, M_ = {k: i for i, k in enumerate(FIELDS)}, {k: i for i, k in enumerate(MATCH_FIELDS)}

    def score(i, a_won, points, k, passed_by=None, pl=0):
        """the end of a game on lane i; True when the lane's last match ended"""
        mt[M_["match_games"]] += 1
        mt[M_["match_points_a" if a_won else "match_points_b"]] += points
        mt[M_["cube_log2"]] += k
        mt[M_["crawford_games"]] += craw[i] == 1
        mt[M_["post_crawford_games"]] += craw[i] == 2
        if passed_by is not None:
            mt[M_["pass_games"]] += 1
            mt[M_["passes_" + passed_by]] += 1
            mt[M_["pass_plies"]] += pl
        aw, cr, over = end_game_reference(away[i], craw[i], L, 0 if a_won else 1, points)
        away[i], craw[i] = aw, cr
        if not over:
            return False
        mt[M_["matches"]] += 1
        mt[M_["match_wins_a"]] += a_won
        mt[M_["matches_seat0"]] += seat0[i]
        mt[M_["match_wins_a_seat0"]] += a_won and seat0[i]
        seat0[i] = ((i + games[i] + 1) & 1) == 0
        matches[i] += 1
        return matches[i] >= M

    for t in range(T):
        s_away[t], s_craw[t], s_cube[t] = away, craw, cube
        active = games < G
        m = mover[t] & 1
        a_moves = (m == 0) == (((lane + games) & 1) == 0)
        x, y = np.where(a_moves, away[:, 0], away[:, 1]), np.where(a_moves, away[:, 1], away[:, 0])
        da = match_decision_reference(match.met, match.pc, L, x, y, craw, cube, m, plies, eq_offer[t], ra,
                                      eq_resp[t], rb, active=active)           # A on roll, B answers
        db = match_decision_reference(match.met, match.pc, L, x, y, craw, cube, m, plies, eq_offer[t], rb,
                                      eq_resp[t], ra, active=active)
        dsel_a, dsel_b = da["access"] & a_moves, db["access"] & ~a_moves
        off_a, off_b = da["offer"] & a_moves, db["offer"] & ~a_moves
        pas = (off_a & da["passes"]) | (off_b & db["passes"])
        take = (off_a | off_b) & ~pas
        dsels[t], offers[t], passes[t] = dsel_a + 2 * dsel_b, off_a + 2 * off_b, pas
        mt[M_["doubles_a"]] += off_a.sum()
        mt[M_["doubles_b"]] += off_b.sum()
        k = np.minimum(cube & 15, MAX_CAP)
        for i in np.nonzero(pas)[0]:
            last = score(i, bool(off_a[i]), 1 << int(k[i]), int(k[i]), "b" if off_a[i] else "a", int(plies[i]))
            games[i] = G if last else games[i] + 1
        plies = np.where(pas, 0, plies)
        cube = np.where(pas, 0, np.where(take, (k + 1) | ((2 - m) << 4), cube))
        # the step, match_flush, advance and match_retire
        active = games < G
        winner, sc = ((info[t] >> 8) & 0xFF) - 1, (info[t] >> 16) & 0xFF
        dn = active & (done[t] != 0)
        fin = dn & (winner >= 0)
        a_p1 = ((lane + games) & 1) == 0
        a_won = fin & ((winner == 0) == a_p1)
        b_won = fin & ~a_won
        pts = np.where((sc >= 1) & (sc <= 3), sc, 0)
        for name, v in (("games", fin), ("wins_a", a_won), ("wins_b", b_won), ("points_a", a_won * pts),
                        ("points_b", b_won * pts), ("gammons_a", a_won & (sc == 2)), ("gammons_b", b_won & (sc == 2)),
                        ("backgammons_a", a_won & (sc == 3)), ("backgammons_b", b_won & (sc == 3)),
                        ("games_a_p1", fin & a_p1), ("wins_a_p1", a_won & a_p1), ("wins_p1", fin & (winner == 0)),
                        ("plies", active)):
            tally[F_[name]] += int(np.asarray(v, np.int64).sum())
        k = np.minimum(cube & 15, MAX_CAP)
        retire = []
        for i in np.nonzero(fin)[0]:
            if score(i, bool(a_won[i]), int(np.clip(sc[i], 1, 3)) << int(k[i]), int(k[i])):
                retire.append(i)
        cube = np.where(dn, 0, cube)
        plies = np.where(dn, 0, plies + active)
        games = games + fin
        games[retire] = G
    tally[ACTIVE] = int((games < G).sum())
    return dict(tally=tally, match_tally=mt, games_done=games, matches_done=matches, away=s_away, craw=s_craw,
                cube=s_cube.astype(np.uint8), dsel=dsels, offer=offers, passed=passes)
