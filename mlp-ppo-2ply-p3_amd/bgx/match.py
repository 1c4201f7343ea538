"""Match play in the head-to-head arena (csrc/bg_match.h; include/bgx.h "match
play in the arena"): matches to L points with the Crawford rule, cube decisions that maximise the
chance of winning the match on a match equity table (MET), and a result counted in matches.

    python -m bgx.arena --a new.pt --b old.pt --max-steps 20000 --match 7 --games-per-lane 1

This module holds the table (met_table, load_met, save_met), the rule of a side (MatchRule), the
pair of rules with the table (ArenaMatch), the summary (summarize_match) and the host references
of the kernels: match_decision_reference (part 1 of csrc/bg_match.h on arrays, bit for bit in numpy
float32) and arena_match_reference (the replay of a traced run).  Arena.play(match=...) of
bgx/arena.py drives the device side.

Match-score rollouts (csrc/bg_match_rollout.h; include/bgx.h "match-score
rollouts"; Rollout.run(match=...) of bgx/rollout.py drives the device side): RolloutMatch,
validate_score, outcome_mwc, summarize_match_rollout, rollout_match_reference (the replay of a traced
run), static_match_decision and rollout_match_decision.

    python -m bgx.rollout --net ckpt.pt --player 1ply --positions pos.json --match 7 --match-score 3,5
    python -m bgx.rollout --net ckpt.pt --player 1ply --positions pos.json --match 7 --match-score 3,5 --match-decision
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


# ------------------------------------------------- match-score rollouts --
# match_hist int64[n_groups, 96] (include/bgx.h bgx_rollout_match_field): bins 0..87, index
# won * 44 + kind * 11 + k, then the six sums below at 88..93; 94 and 95 stay zero
MATCH_BINS, MATCH_HIST_ROW = 88, 96
MATCH_HIST_FIELDS = ("games", "pass_games", "doubles_start", "doubles_other", "pass_plies", "cube_log2")


def match_bin(won, kind, k):
    """match_bin of csrc/bg_match_rollout.h on ints or arrays."""
    return np.asarray(won).astype(np.int64) * 44 + np.clip(kind, 0, 3) * 11 + np.clip(k, 0, MAX_CAP)


class RolloutMatch:
    """Match play of a rollout: single games at a fixed score of a match to
    `length` points, the cube decisions of both sides by one `rule` (a MatchRule, or None for the
    NaN rule: nobody doubles), `met` = (met, pc) as met_table returns them, or None for
    met_table(length)."""

    def __init__(self, length: int, rule, met=None):
        self.length = _check_length(length, "RolloutMatch")
        if rule is not None and not isinstance(rule, MatchRule):
            raise ValueError("RolloutMatch: rule must be a match.MatchRule or None")
        if met is None:
            met = met_table(self.length)
        if not isinstance(met, (tuple, list)) or len(met) != 2:
            raise ValueError("RolloutMatch: met must be (met, pc) or None")
        self.met, self.pc = check_met(self.length, *met)
        self.has_rule = rule is not None
        self.rule = rule if rule is not None else MatchRule(_NanValue())
        self.sync_free = self.rule.sync_free
        self._dev = None

    tables = ArenaMatch.tables


def validate_score(length: int, away, crawford=0):
    """((a1, a2), crawford) as ints for a score of a match to `length`: PLAYER1 needs a1, PLAYER2
    a2.  ValueError for an away outside 1..L, `crawford` outside 0..2, `crawford` 1 or 2 with no
    side at 1, and `crawford` 0 with a side at 1 unless both are (1-away / 1-away is reached only
    through a Crawford game, but its value does not depend on the state, so 0 is allowed there)."""
    L = _check_length(length, "validate_score")
    try:
        a = [int(v) for v in away]
        ok = len(a) == 2 and all(int(v) == v and not isinstance(v, bool) for v in away)
    except (TypeError, ValueError):
        ok = False
    if not ok or not all(1 <= v <= L for v in a):
        raise ValueError(f"validate_score: away must be two numbers of points in 1..{L}, got {away!r}")
    if isinstance(crawford, bool) or crawford not in (0, 1, 2):
        raise ValueError(f"validate_score: crawford must be 0, 1 or 2, got {crawford!r}")
    c = int(crawford)
    if c != 0 and 1 not in a:
        raise ValueError(f"validate_score: crawford {c} at {a[0]}-away / {a[1]}-away, where no side needs 1 point")
    if c == 0 and 1 in a and a != [1, 1]:
        raise ValueError(f"validate_score: {a[0]}-away / {a[1]}-away is the Crawford game or a later one: crawford "
                         "must be 1 or 2")
    return (a[0], a[1]), c


def met_after64(met, pc, length: int, me, opp, craw):
    """met_after of csrc/bg_match.h on ints or arrays, the fp32 table values promoted to fp64."""
    L = int(length)
    m2, p = np.asarray(met, F).reshape(L + 1, L + 1).astype(np.float64), np.asarray(pc, F).reshape(L + 1).astype(np.float64)
    me, opp = np.asarray(me, np.int64), np.asarray(opp, np.int64)
    mc, oc = np.clip(me, 1, L), np.clip(opp, 1, L)
    r = np.where(np.asarray(craw) != 0, np.where(mc == 1, 1.0 - p[oc], p[mc]), m2[mc, oc])
    return np.where(me <= 0, 1.0, np.where(opp <= 0, 0.0, r))


def outcome_mwc(met, pc, length: int, away, crawford: int, start_mover: int) -> np.ndarray:
    """float64[88]: the start mover's match-winning chance after each bin's outcome at the score
    `away` = (a1, a2), `crawford`.  With x_s the start mover's away and y_s the other's, points =
    max(kind, 1) << k: a win gives met_after(x_s - points, y_s, crawford), a loss 1 -
    met_after(y_s - points, x_s, crawford)."""
    s = int(start_mover) & 1
    xs, ys = int(away[s]), int(away[1 - s])
    kind, k = np.divmod(np.arange(44), 11)
    points = np.maximum(kind, 1) << k
    win = met_after64(met, pc, length, xs - points, ys, crawford)
    loss = 1.0 - met_after64(met, pc, length, ys - points, xs, crawford)
    return np.concatenate([loss, win])


def summarize_match_rollout(tally_row, hist_row, mwc88, unfinished: int = 0, cube_k: int = 0) -> dict:
    """One position's match-score result from its plain tally row (the games played to the end),
    its 96 histogram entries and outcome_mwc's 88 values, all from the integers: `games`; `mwc` =
    sum(bin * mwc88) / games, the start mover's match-winning chance, with `mwc_stderr` = sqrt(sum(bin
    (mwc88 - mwc)^2) / (games - 1) / games) (None below 2 games); `mwc_normalized` = (2 mwc - (W + L))
    / (W - L) with W and L the chance after winning / losing a plain game at the starting cube
    2^`cube_k` (None when they are equal): +-1 is winning / losing one current cube; `pass_share`,
    `doubles_per_game_start` / `_other`, `mean_cube_log2`, the six sums under their names
    (MATCH_HIST_FIELDS), `match_hist` (the 96 entries), `unfinished` and `played_out` =
    summarize(tally_row, unfinished).  Without games the rates are 0.  Raises ValueError when a bin
    is negative, GAMES != the sum of the bins or != the plain tally's games + PASS_GAMES, PASS_GAMES
    != the sum of the pass bins, or the played-out bins summed over k differ from the plain tally's
    win / gammon / backgammon counts."""
    from .tally import summarize
    played = summarize(tally_row, unfinished)
    h = [int(v) for v in hist_row]
    m = np.asarray(mwc88, np.float64).reshape(-1)
    if len(h) != MATCH_HIST_ROW or m.shape[0] != MATCH_BINS:
        raise ValueError(f"summarize_match_rollout: need {MATCH_HIST_ROW} histogram entries and {MATCH_BINS} values, "
                         f"got {len(h)} and {m.shape[0]}")
    bins = np.asarray(h[:MATCH_BINS], np.int64)
    r = dict(zip(MATCH_HIST_FIELDS, h[MATCH_BINS:]))
    n = r["games"]
    if (bins < 0).any():
        raise ValueError("summarize_match_rollout: a bin count is negative")
    if n != int(bins.sum()):
        raise ValueError(f"summarize_match_rollout: GAMES is {n}, the bins hold {int(bins.sum())}")
    if n != played["games"] + r["pass_games"]:
        raise ValueError(f"summarize_match_rollout: the histogram counts {n} games, the plain tally {played['games']} "
                         f"and {r['pass_games']} passed")
    by = bins.reshape(2, 4, 11).sum(axis=2)                 # [won, kind]
    if int(by[:, 0].sum()) != r["pass_games"]:
        raise ValueError(f"summarize_match_rollout: PASS_GAMES is {r['pass_games']}, the pass bins hold {int(by[:, 0].sum())}")
    want = [played[f"{w}{s}"] for w in ("loss", "win") for s in (1, 2, 3)]
    if [int(v) for v in by[:, 1:].reshape(-1)] != want:
        raise ValueError(f"summarize_match_rollout: the played-out bins hold {by[:, 1:].tolist()} (losses, wins by "
                         f"score), the plain tally {want}")

    def ratio(a, b):
        return a / b if b > 0 else 0.0

    mwc = float((bins * m).sum() / n) if n > 0 else 0.0
    se = math.sqrt(float((bins * (m - mwc) ** 2).sum()) / (n - 1) / n) if n >= 2 else None
    k0 = min(max(int(cube_k), 0), MAX_CAP)
    W, L_ = float(m[44 + 11 + k0]), float(m[11 + k0])
    r.update(mwc=mwc, mwc_stderr=se, mwc_normalized=(2.0 * mwc - (W + L_)) / (W - L_) if W != L_ else None,
             pass_share=ratio(r["pass_games"], n), doubles_per_game_start=ratio(r["doubles_start"], n),
             doubles_per_game_other=ratio(r["doubles_other"], n), mean_cube_log2=ratio(r["cube_log2"], n),
             match_hist=h, unfinished=int(unfinished), played_out=played)
    return r


def rollout_match_reference(trace, starts, group, n_groups: int, games_per_lane: int, match: RolloutMatch, away, craw,
                            cube0=None) -> dict:
    """A traced match-score run (run_lanes(trace=True, match=...)) replayed on the host with the
    kernels' arithmetic (include/bgx.h bgx_rollout_match_*), through replay.LaneReplay and
    match_decision_reference.  Read from the trace, [steps, B] each: match_mover (the side on roll
    before the decision), match_value (the rule's value there), done and info; the lane records are
    taken as not game_over, which holds between the steps of an auto-reset engine.  `away`
    [n_groups, 2] and `craw` [n_groups] the groups' score, `cube0` uint8[B] the lanes' starting
    cubes (None: centred at 1).  Returns dict(match_hist int64[P, 96], tally int64[P, 8], cube
    uint8[steps, B] = the states before each decision, dsel bool[steps, B], action uint8[steps, B]
    (0 none, 1 take, 2 pass), mask bool[steps, B], games_done int64[B], active int)."""
    from .cube import sanitise
    from .replay import LaneReplay, result_of

    def host(x):
        return np.asarray(torch.as_tensor(x).cpu())
    mover, value = host(trace["match_mover"]).astype(np.int64), host(trace["match_value"]).astype(F)
    done, info = host(trace["done"]), host(trace["info"])
    P, L = int(n_groups), match.length
    rp = LaneReplay(host(starts), host(group), P, games_per_lane)
    B, T = rp.B, done.shape[0]
    c0 = np.zeros(B, np.uint8) if cube0 is None else sanitise(host(cube0), MAX_CAP)
    cube = c0.copy()
    away, craw = np.asarray(away, np.int64).reshape(P, 2), np.asarray(craw, np.int64).reshape(P)
    gi = np.clip(rp.group, 0, P - 1)
    start = rp.start_cur.astype(np.int64) & 1
    hist = np.zeros((P, MATCH_HIST_ROW), np.int64)
    fld = {name: MATCH_BINS + i for i, name in enumerate(MATCH_HIST_FIELDS)}
    states, dsels = np.zeros((T, B), np.uint8), np.zeros((T, B), bool)
    actions, masks = np.zeros((T, B), np.uint8), np.zeros((T, B), bool)

    def add(lanes, col, v=1):
        np.add.at(hist, (gi[lanes], np.broadcast_to(col, (B,))[lanes]), np.broadcast_to(v, (B,))[lanes])

    for t in range(T):
        states[t] = cube
        m = mover[t] & 1
        k = np.minimum(cube.astype(np.int64) & 15, MAX_CAP)
        d = match_decision_reference(match.met, match.pc, L, away[gi, m], away[gi, 1 - m], craw[gi], cube, m, rp.plies,
                                     value[t], match.rule, active=rp.sel)
        offer = d["offer"]
        pas = offer & d["passes"]
        take = offer & ~pas
        dsels[t], masks[t], actions[t] = d["access"], pas, np.where(pas, 2, np.where(take, 1, 0))
        mine = m == start
        add(pas, match_bin(mine, 0, k))
        for name, v in (("games", 1), ("pass_games", 1), ("pass_plies", rp.plies), ("cube_log2", k)):
            add(pas, fld[name], v)
        add(offer & mine, fld["doubles_start"])
        add(offer & ~mine, fld["doubles_other"])
        cube = np.where(pas, c0, np.where(take, (k + 1) | ((2 - m) << 4), cube)).astype(np.uint8)
        rp.end(pas)
        # the step, match_flush and advance
        winner, score = result_of(info[t])
        dn = done[t] != 0
        fin = rp.sel & dn & (winner >= 0)
        k = np.minimum(cube.astype(np.int64) & 15, MAX_CAP)
        add(fin, match_bin(winner == start, score, k))
        add(fin, fld["games"])
        add(fin, fld["cube_log2"], k)
        cube = np.where(dn, c0, cube).astype(np.uint8)
        rp.advance(done[t], info[t])
    return dict(match_hist=hist, tally=rp.tallies["tally"], cube=states, dsel=dsels, action=actions, mask=masks,
                games_done=rp.games, active=rp.active)


def _lane_bytes(name, v, n, dev, width=None):
    """`v` as a contiguous uint8 tensor [n] or [n, width] on `dev`: a tensor of that shape, or one
    entry (an int, or `width` ints) for every lane."""
    shape = (n,) if width is None else (n, width)
    if isinstance(v, torch.Tensor):
        if v.shape != shape or v.dtype != torch.uint8 or v.device != dev or not v.is_contiguous():
            raise ValueError(f"static_match_decision: {name} must be a contiguous uint8{list(shape)} tensor on {dev}")
        return v
    a = np.asarray(v, np.int64)
    if a.shape != shape[1:] or (a < 0).any() or (a > 255).any():
        raise ValueError(f"static_match_decision: {name} must be a uint8{list(shape)} tensor or one entry for all lanes")
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a.astype(np.uint8), shape))).to(dev)


def static_match_decision(eng_or_records, head_or_values, match: RolloutMatch, away, crawford=0, cube=None):
    """"Double or not, take or pass?" at a match score with no rollout (bgx_match_decision):
    (values f32[n, 3], flags uint8[n]) for an Engine's lane records or a contiguous uint8[n, 64]
    tensor on the GPU.  values = ND, DT, DP, the match-winning chances of the record's mover by
    `match`'s rule and tables; flags bit 0: the mover has access (without the first-ply term), 1:
    it doubles, 2: the other side passes a double, 3: too good (ND > DP).  `head_or_values`: a
    search.ValueHead (its static value of the records, search.value_lanes) or float32[n] values of
    the side on roll on the records' device.  `away` uint8[n, 2] by player or one pair for all,
    `crawford` uint8[n] or one state, `cube` uint8[n] cube bytes, one (k, owner) pair or None
    (centred at 1).  Sync-free."""
    from .arena import _stream
    from .cube import pack
    from .engine import Engine, _ptr
    from .search import value_lanes
    import ctypes
    if not isinstance(match, RolloutMatch):
        raise ValueError("static_match_decision: match must be a match.RolloutMatch")
    r = eng_or_records
    if isinstance(r, Engine):
        n, dev, rp = r.batch, r.device, ctypes.c_void_p(r.lanes_ptr())
    else:
        if (not isinstance(r, torch.Tensor) or r.dtype != torch.uint8 or r.dim() != 2 or r.shape[1] != 64
                or not r.is_contiguous() or not r.is_cuda):
            raise ValueError("static_match_decision: records must be an Engine or a contiguous uint8[n, 64] tensor on "
                             "the GPU")
        n, dev, rp = r.shape[0], r.device, _ptr(r)
    if isinstance(head_or_values, torch.Tensor):
        value = head_or_values
        if value.shape != (n,) or value.dtype != torch.float32 or value.device != dev or not value.is_contiguous():
            raise ValueError(f"static_match_decision: values must be a contiguous float32[{n}] tensor on {dev}")
    else:
        value = value_lanes(r, head_or_values)
    if cube is None:
        cube = 0
    elif not isinstance(cube, torch.Tensor):
        cube = pack(*cube)
    aw, cr, cb = _lane_bytes("away", away, n, dev, 2), _lane_bytes("crawford", crawford, n, dev), _lane_bytes("cube", cube, n, dev)
    met, pc = match.tables(dev)
    values = torch.empty(n, 3, dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().bgx_match_decision(rp, _ptr(cb), _ptr(aw), _ptr(cr), _ptr(value), n, match.rule.struct(),
                                              _ptr(met), _ptr(pc), match.length, _ptr(values), _ptr(flags), _stream(dev)),
               "bgx_match_decision")
    return values, flags


def rollout_match_decision(rollout, player, record, trials: int, match: RolloutMatch, away, crawford: int = 0,
                           cube=(0, 0), first_roll: str = "stratified", max_steps: int = 4000) -> dict:
    """"Double or not, take or pass?" at a match score for the side on roll in `record` (uint8[64]:
    board and mover) at `away` = (PLAYER1's, PLAYER2's points to go), `crawford`, holding the cube
    `cube` = (k, owner).  The position is rolled out twice in one run, as two groups over the same
    start records: "no double", with the cube as given, and "double, take", with k + 1 owned by
    the opponent.  No cube action happens on a game's first ply, so both start after the decision
    asked about.  Returns `no_double` and `double_take`, the match-winning chances of the side on
    roll, each with its `_stderr`; `double_pass` = met_after(x - 2^k, y, crawford) with stderr 0;
    the verdict: `double` iff min(double_take, double_pass) > no_double, `take` iff double_take <=
    double_pass; `cube`, `away`, `crawford` and the two summaries (`rollouts`).  ValueError when
    the side on roll has no access at that score: the Crawford game, a cube that is not its own
    or at the cap, or x <= 2^k (winning this game wins the match)."""
    if not isinstance(match, RolloutMatch):
        raise ValueError("rollout_match_decision: match must be a match.RolloutMatch")
    rec = torch.as_tensor(record).reshape(-1)
    if rec.numel() != 64 or rec.dtype != torch.uint8:
        raise ValueError("rollout_match_decision: record must be 64 bytes (uint8)")
    (a1, a2), cr = validate_score(match.length, away, crawford)
    k, owner = int(cube[0]), int(cube[1])
    mover = int(rec[52]) & 1
    x, y = ((a1, a2), (a2, a1))[mover]
    if cr == 1:
        raise ValueError("rollout_match_decision: no double in the Crawford game")
    if not 0 <= k < MAX_CAP or owner not in (0, mover + 1) or (owner == 0) != (k == 0):
        raise ValueError(f"rollout_match_decision: cube {(k, owner)} gives the mover (PLAYER{mover + 1}) no double")
    if x <= (1 << k):
        raise ValueError(f"rollout_match_decision: the side on roll needs {x} with the cube at {1 << k}: the cube is "
                         "dead, winning this game wins the match")
    pos = torch.stack([rec.cpu(), rec.cpu()])
    res = rollout.run(player, pos, trials, first_roll=first_roll, max_steps=max_steps, match=match,
                      match_away=(a1, a2), match_crawford=cr, cube_start=[(k, owner), (k + 1, 2 - mover)])
    nd, dt = res[0]["mwc"], res[1]["mwc"]
    dp = float(met_after64(match.met, match.pc, match.length, x - (1 << k), y, cr))
    return dict(no_double=nd, no_double_stderr=res[0]["mwc_stderr"], double_take=dt, double_take_stderr=res[1]["mwc_stderr"],
                double_pass=dp, double_pass_stderr=0.0, double=bool(min(dt, dp) > nd), take=bool(dt <= dp),
                cube=[k, owner], away=[a1, a2], crawford=cr, rollouts=res)
