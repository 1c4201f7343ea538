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

from .engine import R_CUR, R_ROLL0

# trunc_tally int64[n_groups][7] (include/bgx.h bgx_rollout_trunc_field): fixed point, 2^-16 points
TRUNC_FIELDS = ("trunc_games", "trunc_plies", "trunc_v", "trunc_v2", "trunc_luck", "trunc_luck2", "trunc_vluck")
TRUNC_ONE = 65536                   # Vq = rint(y * TRUNC_ONE)
TRUNC_CLAMP = 3.0                   # |y| <= TRUNC_CLAMP points
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


def _row(row, fields, what):
    t = [int(v) for v in row]
    if len(t) != len(fields):
        raise ValueError(f"{what}: a row has {len(fields)} entries, got {len(t)}")
    return t


def summarize_truncated(tally_row, trunc_row, unfinished: int = 0) -> dict:
    """One position's result from its 8 tally entries (the games played to the end) and its 7
    truncation sums (TRUNC_FIELDS: the games stopped at the horizon; a truncated game's result is
    y = Vq / 2^16 points from the start mover's side).  On summarize's fields: `games` = natural
    + truncated, `equity` = (sum res + sum y) / games and `equity_stderr` from sum res^2 +
    sum y^2 as summarize forms it, both from exact integers (sum res 2^16 + sum Vq, and the
    squares), so equal values give their value exactly and a standard error of 0;
    `plies_per_game` over both kinds.  The win, gammon and backgammon rates (`win`, `loss`,
    `win_gammon`, ...) are those of the NATURAL games alone, over `natural_games`: the value has
    one output and says nothing about how a truncated game would have ended.  Adds
    `natural_games`, `truncated_games`, `truncated_share` = truncated_games / games and
    `truncated_equity`, the mean of the truncated games' values.  The standard error is the
    sample's spread: it does not contain the value's own error."""
    from .rollout import summarize
    r = summarize(tally_row, unfinished)
    c = _row(trunc_row, TRUNC_FIELDS, "summarize_truncated")
    n_t, t_plies, sv, sv2 = c[:4]
    w, l = [r[f"win{j}"] for j in (1, 2, 3)], [r[f"loss{j}"] for j in (1, 2, 3)]
    n_nat = r["games"]
    n = n_nat + n_t
    # sum of results in 2^-16 points, sum of squares in 2^-32: exact integers
    s1 = sum((k + 1) * (w[k] - l[k]) for k in range(3)) * TRUNC_ONE + sv
    s2 = sum((k + 1) ** 2 * (w[k] + l[k]) for k in range(3)) * TRUNC_ONE ** 2 + sv2
    inv = 1.0 / n if n > 0 else 0.0
    var_num = max(n * s2 - s1 * s1, 0)                       # n^2 (n - 1) 2^32 x the variance of the mean
    r.update(games=n, natural_games=n_nat, truncated_games=n_t, truncated_share=n_t * inv,
             truncated_equity=sv / (n_t * TRUNC_ONE) if n_t > 0 else 0.0,
             plies_per_game=(r["plies"] + t_plies) * inv,
             equity=s1 / (n * TRUNC_ONE) if n > 0 else 0.0,
             equity_stderr=math.sqrt(var_num / (n * n * (n - 1))) / TRUNC_ONE if n > 1 else 0.0)
    r.update(zip(TRUNC_FIELDS, c))
    return r


def summarize_truncated_luck(tally_row, luck_row, trunc_row, scale="fit", unfinished: int = 0) -> dict:
    """summarize_truncated plus the luck-adjusted estimate over all games, with summarize_luck's
    formulas: a game's adjusted result is y - c L, y the natural result or Vq / 2^16 of a
    truncated game, L the luck of the rolls it played.  From the integer sums
        sum L = (LUCK + TRUNC_LUCK) / 2^16      sum L^2 = (LUCK2 + TRUNC_LUCK2) / 2^32
        sum y L = RESLUCK / 2^16 + TRUNC_VLUCK / 2^32
    `scale` = "fit": c = cov(y, L) / var(L) of these games, numerator and denominator as exact
    integers (0 when var(L) is 0); a float: that c.  Adds luck_scale, luck_mean, equity_luck,
    equity_luck_stderr and variance_ratio.  Without truncated games it is summarize_luck.  Raises
    ValueError when the luck row counts other games than the tally row."""
    from .rollout import LUCK_FIELDS
    r = summarize_truncated(tally_row, trunc_row, unfinished)
    k = _row(luck_row, LUCK_FIELDS, "summarize_truncated_luck")
    c7 = [r[f] for f in TRUNC_FIELDS]
    if k[3] != r["natural_games"]:
        raise ValueError(f"summarize_truncated_luck: the luck row counts {k[3]} games, the tally row "
                         f"{r['natural_games']}")
    n, one = r["games"], TRUNC_ONE
    w, l = [r[f"win{j}"] for j in (1, 2, 3)], [r[f"loss{j}"] for j in (1, 2, 3)]
    y1 = sum((j + 1) * (w[j] - l[j]) for j in range(3)) * one + c7[2]                 # 2^-16
    y2 = sum((j + 1) ** 2 * (w[j] + l[j]) for j in range(3)) * one * one + c7[3]      # 2^-32
    il, il2, iyl = k[0] + c7[4], k[1] + c7[5], k[2] * one + c7[6]                     # 2^-16, 2^-32, 2^-32
    sl, sl2, srl = il / one, il2 / (one * one), iyl / (one * one)
    sr, sr2 = y1 / one, y2 / (one * one)
    if scale == "fit":
        num, den = n * iyl - y1 * il, n * il2 - il * il          # both in 2^-32: a constant result gives 0
        c = num / den if den > 0 else 0.0
    else:
        c = float(scale)
    inv = 1.0 / n if n > 0 else 0.0
    eq = (sr - c * sl) * inv
    var_y = max(sr2 - 2.0 * c * srl + c * c * sl2 - n * eq * eq, 0.0) / (n - 1) if n > 1 else 0.0
    var_r = max(sr2 - n * r["equity"] ** 2, 0.0) / (n - 1) if n > 1 else 0.0
    r.update(luck_scale=c, luck_mean=sl * inv, equity_luck=eq, equity_luck_stderr=math.sqrt(var_y * inv),
             variance_ratio=var_y / var_r if var_r > 0.0 else 1.0)
    return r


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
    from .rollout import FIELDS, LUCK_CLAMP, LUCK_FIELDS, LUCK_ONE

    def host(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    mover, done, info = host(trace["mover"]), host(trace["done"]), host(trace["info"]).astype(np.int64)
    tval, tmover = host(trace["trunc_value"]).astype(np.float32), host(trace["trunc_mover"])
    luck = host(trace["luck"]).astype(np.float32) if "luck" in trace else None
    starts, group = host(starts), host(group).astype(np.int64)
    B, P, G, H = group.shape[0], int(n_groups), int(games_per_lane), int(truncation.plies)
    valid = (group >= 0) & (group < P)
    fixed = starts[:, R_ROLL0] != 0
    start_mover = starts[:, R_CUR]
    lane = np.zeros(B, np.float32)
    plies, games = np.zeros(B, np.int64), np.zeros(B, np.int64)
    tally, ttally = np.zeros((P, len(FIELDS)), np.int64), np.zeros((P, len(TRUNC_FIELDS)), np.int64)
    ltally = np.zeros((P, len(LUCK_FIELDS)), np.int64) if luck is not None else None
    cuts = np.zeros(done.shape, bool)
    ones = np.ones(B, np.int64)

    def luck_q():
        with np.errstate(invalid="ignore", over="ignore"):
            x = (lane * np.float32(LUCK_ONE)).astype(np.float32)
        x = np.where(np.isfinite(x), np.clip(x, -float(LUCK_CLAMP), float(LUCK_CLAMP)), 0.0)
        return np.rint(x).astype(np.int64)

    for t in range(done.shape[0]):
        sel = valid & (games < G)
        if luck is not None:
            add = sel & ~((plies == 0) & fixed)
            signed = np.where(mover[t] == start_mover, luck[t], -luck[t]).astype(np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                lane = np.where(add, (lane + np.where(add, signed, np.float32(0))).astype(np.float32), lane)
        winner = ((info[t] >> 8) & 0xFF) - 1
        score = np.clip((info[t] >> 16) & 0xFF, 1, 3)
        dn = sel & (done[t] != 0)
        fin = dn & (winner >= 0)
        won = winner == (start_mover & 1)
        if luck is not None:
            lq = luck_q()
            res = np.where(won, score, -score)
            for f, v in enumerate((lq, lq * lq, res * lq, ones)):
                np.add.at(ltally[:, f], group[fin], v[fin])
            lane = np.where(dn, np.float32(0), lane)
        plies = np.where(sel, plies + 1, plies)
        field = np.where(won, 2, 5) + score - 1
        np.add.at(tally[:, 0], group[fin], 1)
        np.add.at(tally[:, 1], group[fin], plies[fin])
        np.add.at(tally, (group[fin], field[fin]), 1)
        games[fin] += 1
        plies[fin] = 0
        # the truncation, after advance
        cut = valid & (games < G) & (plies >= H)
        vq = value_q(truncation.scale, tval[t], tmover[t] == start_mover)
        lq = luck_q() if luck is not None else np.zeros(B, np.int64)
        for f, v in enumerate((ones, plies, vq, vq * vq, lq, lq * lq, vq * lq)):
            np.add.at(ttally[:, f], group[cut], v[cut])
        lane = np.where(cut, np.float32(0), lane)
        games[cut] += 1
        plies[cut] = 0
        cuts[t] = cut
    return dict(tally=tally, trunc_tally=ttally, luck_tally=ltally, games_done=games,
                active=int((valid & (games < G)).sum()), trunc=cuts)
