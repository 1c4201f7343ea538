"""The host replay of a rollout's bookkeeping: what the accounting kernels (csrc/bg_rollout.h,
bg_cube.h, the cut kernels) do to the per-lane state and the tallies, in numpy on a step's lanes at
once.  The *_reference functions of rollout.py, truncate.py and cube.py are short drivers of it:
each feeds a trace through the methods in run_lanes' order and scores its own cut, as a kernel does.
An independent oracle: numpy and tally.py's constants only, no library, no torch, no device code."""
from __future__ import annotations

import numpy as np

from .tally import (CUBE_CUT_SPLIT, CUBE_FIELDS, CUBE_LUCK_CLAMP, CUBE_LUCK_ONE, FIELDS, LUCK_CLAMP, LUCK_FIELDS,
                    LUCK_ONE)

R_CUR, R_ROLL0 = 52, 53             # the lane record's mover and first roll byte (engine.R_CUR, engine.R_ROLL0)


def result_of(info):
    """(winner, score) of a step's info words: the winner (-1 = none) and the game's points, 1..3."""
    info = np.asarray(info).astype(np.int64)
    return ((info >> 8) & 0xFF) - 1, np.clip((info >> 16) & 0xFF, 1, 3)


def luck_q(luck) -> np.ndarray:
    """A game's fp32 luck sum in 2^-16 fixed point: Lq = rint(fp32(sum * 65536)) (round half even)
    clamped to +-2^21, 0 when not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (luck * np.float32(LUCK_ONE)).astype(np.float32)
    x = np.where(np.isfinite(x), np.clip(x, -float(LUCK_CLAMP), float(LUCK_CLAMP)), 0.0)
    return np.rint(x).astype(np.int64)


def cube_luck_q(luck) -> np.ndarray:
    """A cubeful game's fp32 luck sum in points as Lq = rint(fp32(sum * 65536)) (round half even)
    clamped to +-2^31, 0 when not finite (cube_luck_q of csrc/bg_cube_luck.h)."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.asarray(luck, np.float32) * np.float32(CUBE_LUCK_ONE)).astype(np.float32)
    x = np.where(np.isfinite(x), np.clip(x, -float(CUBE_LUCK_CLAMP), float(CUBE_LUCK_CLAMP)), 0.0)
    return np.rint(x).astype(np.int64)


def split_sq(y):
    """(y^2 & (2^30 - 1), y^2 >> 30): the two sums of a cubeful result's square."""
    y2 = y * y
    return y2 & ((1 << CUBE_CUT_SPLIT) - 1), y2 >> CUBE_CUT_SPLIT


class LaneReplay:
    """The per-lane state of a rollout and its tallies.  `starts` uint8[B, 64], `group` int[B]
    (a lane counts while its group is in [0, n_groups) and it has finished fewer than
    `games_per_lane` games: `sel`).  State: `plies`, `games` int64[B], `luck` f32[B] (the current
    games' luck sums), with `cap` the cube bytes `cube` uint8[B] and `c0` (every game's starting
    cube, sanitised by the caller).  `tallies`: name -> int64[n_groups, fields], made by tally()."""

    def __init__(self, starts, group, n_groups: int, games_per_lane: int, cap=None, c0=None, jacoby=False):
        self.starts, self.group = np.asarray(starts), np.asarray(group).astype(np.int64)
        self.B, self.P, self.G = self.group.shape[0], int(n_groups), int(games_per_lane)
        self.valid = (self.group >= 0) & (self.group < self.P)
        self.start_cur = self.starts[:, R_CUR]
        self.fixed = self.starts[:, R_ROLL0] != 0
        self.plies, self.games = np.zeros(self.B, np.int64), np.zeros(self.B, np.int64)
        self.luck = np.zeros(self.B, np.float32)
        self.cap, self.c0, self.jacoby = cap, c0, jacoby
        self.cube = None if c0 is None else c0.copy()
        self.tallies = {}
        self.tally("tally", FIELDS)

    def tally(self, name, fields):
        self.tallies[name] = np.zeros((self.P, len(fields)), np.int64)

    @property
    def sel(self):
        return self.valid & (self.games < self.G)

    @property
    def active(self) -> int:
        return int(self.sel.sum())

    def cube_k(self):
        return np.minimum(self.cube.astype(np.int64) & 15, int(self.cap))

    def add(self, name, lanes, values, first: int = 0):
        """tallies[name][group, first + j] += values[j] over `lanes` (a value may be a scalar)."""
        for f, v in enumerate(values, first):
            np.add.at(self.tallies[name][:, f], self.group[lanes], np.broadcast_to(v, (self.B,))[lanes])

    def end(self, lanes, cube: bool = False):
        """end_game on `lanes`: the game is counted, the next one starts at 0 plies and 0 luck
        and, where the caller says so, with the lane's starting cube."""
        self.games = self.games + lanes
        self.plies = np.where(lanes, 0, self.plies)
        self.luck = np.where(lanes, np.float32(0), self.luck)
        if cube:
            self.cube = np.where(lanes, self.c0, self.cube).astype(np.uint8)

    def luck_add(self, luck, mover):
        """bgx_rollout_luck_add: +-luck (signed for the start mover) joins the selected lanes' fp32
        sums in step order, left out in a game's first step when the start record fixed the roll."""
        add = self.sel & ~((self.plies == 0) & self.fixed)
        signed = np.where(mover == self.start_cur, luck, -luck).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            self.luck = np.where(add, (self.luck + np.where(add, signed, np.float32(0))).astype(np.float32), self.luck)

    def cube_luck_add(self, luck, mover):
        """bgx_rollout_cube_luck_add: luck_add with the roll's luck in units of the lane's cube as it
        stands (after the step's decision): +-ldexp(luck, k) joins the selected lanes' sums."""
        with np.errstate(invalid="ignore", over="ignore"):
            self.luck_add(np.ldexp(np.asarray(luck, np.float32), self.cube_k().astype(np.int32)).astype(np.float32), mover)

    def cube_luck_book(self, lanes, y):
        """The booking of bgx_rollout_cube_luck_pass / _flush (where the replay has that tally):
        the `lanes`' luck sums as Lq against their games' results y in points."""
        if "cube_luck_tally" in self.tallies:
            lq = cube_luck_q(self.luck)
            self.add("cube_luck_tally", lanes, (lq, *split_sq(lq), y * lq, 1))

    def decide(self, mover, act, nxt, access):
        """bgx_rollout_cube_sel + bgx_rollout_cube_decide with cube.decide_reference's (act, nxt,
        access) of the current cubes: a pass ends the game at the cube's value, a take turns the
        cube.  Returns (dsel, passed)."""
        k, m = self.cube_k(), np.asarray(mover).astype(np.int64) & 1
        dsel = self.sel & (self.plies > 0) & access
        act = np.where(dsel, act, 0)
        pas, dbl = act == 2, act > 0
        y = np.where(m == (self.start_cur.astype(np.int64) & 1), 1, -1) * (1 << k)
        self.cube_luck_book(pas, y)             # bgx_rollout_cube_luck_pass runs before the decision is applied
        self.add("cube_tally", pas, (1, y, y * y, k, 1, self.plies, (y > 0).astype(np.int64)))
        self.add("cube_tally", dbl, (1,), first=CUBE_FIELDS.index("doubles"))
        self.cube = np.where(dbl, nxt, self.cube).astype(np.uint8)
        self.end(pas, cube=True)
        return dsel, pas

    def advance(self, done, info):
        """The step's end on the selected lanes: bgx_rollout_luck_flush, bgx_rollout_cube_luck_flush and
        bgx_rollout_cube_flush (where the replay has those tallies), then bgx_rollout_advance.  A done with a winner is
        a finished game; any done clears the lane's luck and puts its starting cube back."""
        sel = self.sel
        winner, score = result_of(info)
        dn = sel & (np.asarray(done) != 0)
        fin = dn & (winner >= 0)
        won = winner == (self.start_cur & 1)
        if "luck_tally" in self.tallies:
            lq = luck_q(self.luck)
            self.add("luck_tally", fin, (lq, lq * lq, np.where(won, score, -score) * lq, 1))
        if self.cube is not None:
            k = self.cube_k()
            y = np.where(won, 1, -1) * (np.where(self.jacoby & (k == 0), 1, score) << k)
            self.cube_luck_book(fin, y)         # bgx_rollout_cube_luck_flush, before the sums are cleared
        self.luck = np.where(dn, np.float32(0), self.luck)
        if self.cube is not None:
            self.add("cube_tally", fin, (1, y, y * y, k))
            self.cube = np.where(dn, self.c0, self.cube).astype(np.uint8)
        self.plies = self.plies + sel
        self.add("tally", fin, (1, self.plies))
        np.add.at(self.tallies["tally"], (self.group[fin], (np.where(won, 2, 5) + score - 1)[fin]), 1)
        self.end(fin)

    def horizon(self, plies: int):
        """bgx_rollout_trunc_sel: the selected lanes whose game has run `plies` plies."""
        return self.sel & (self.plies >= int(plies))

    def cut(self, name, lanes, own, cube: bool = False):
        """A cut kernel's tail (cut_finish of csrc/bg_rollout.h): tallies[name] gains GAMES, PLIES
        and the mode's `own` fields of `lanes`, whose games end."""
        self.add(name, lanes, (1, self.plies) + tuple(own))
        self.end(lanes, cube)
