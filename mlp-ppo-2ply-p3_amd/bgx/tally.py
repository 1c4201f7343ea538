"""The tallies of position rollouts: the field names and fixed-point units of every tally run_lanes
returns (include/bgx.h bgx_rollout_*_field) and the summaries that turn a position's rows into its
result.  Plain Python, no other module of the package: rollout.py, truncate.py, cube.py and
replay.py import it and re-export its names.  The sums of results and of squares are Python
integers, so equal results give their value exactly and a standard error of 0."""
from __future__ import annotations

import math

# tally int64[n_groups][8] (bgx_rollout_field)
FIELDS = ("games", "plies", "win1", "win2", "win3", "loss1", "loss2", "loss3")
# luck_tally int64[n_groups][4] (bgx_rollout_luck_field): fixed point, 2^-16 points
LUCK_FIELDS = ("luck", "luck2", "resluck", "luck_games")
LUCK_ONE = 65536                    # Lq = rint(L * LUCK_ONE)
LUCK_CLAMP = 1 << 21                # |Lq| <= LUCK_CLAMP
# cut_tally int64[n_groups][4] (bgx_rollout_cut_field): fixed point, 2^-20
CUT_FIELDS = ("cut_games", "cut_plies", "cut_p", "cut_p2")
CUT_ONE = 1 << 20                   # Pq = rint(q * CUT_ONE), q the start mover's exact win probability
# trunc_tally int64[n_groups][7] (bgx_rollout_trunc_field): fixed point, 2^-16 points
TRUNC_FIELDS = ("trunc_games", "trunc_plies", "trunc_v", "trunc_v2", "trunc_luck", "trunc_luck2", "trunc_vluck")
TRUNC_ONE = 65536                   # Vq = rint(y * TRUNC_ONE)
TRUNC_CLAMP = 3.0                   # |y| <= TRUNC_CLAMP points
# cube_tally int64[n_groups][8] (bgx_rollout_cube_field)
CUBE_FIELDS = ("cube_games", "cube_points", "cube_points2", "cube_log2", "pass_games", "pass_plies", "pass_won",
               "doubles")
# cube_cut_tally int64[n_groups][6] (bgx_rollout_cube_cut_field): the games cut at the cubeful
# bearoff table, fixed point, 2^-20 points
CUBE_CUT_FIELDS = ("cut_games", "cut_plies", "cut_y", "cut_y2_lo", "cut_y2_hi", "cut_log2")
CUBE_CUT_ONE = 1 << 20              # Yq = rint(q * CUBE_CUT_ONE) * 2^k
CUBE_CUT_SPLIT = 30                 # sum Yq^2 = cut_y2_hi * 2^30 + cut_y2_lo
# cube_trunc_tally int64[n_groups][6] (bgx_rollout_cube_trunc_field): the cubeful games truncated
# at the horizon, fixed point, 2^-16 points (TRUNC_ONE)
CUBE_TRUNC_FIELDS = ("cube_trunc_games", "cube_trunc_plies", "cube_trunc_y", "cube_trunc_y2_lo", "cube_trunc_y2_hi",
                     "cube_trunc_log2")
CUBE_TRUNC_ONE = 1 << 16            # Yq = rint(q * CUBE_TRUNC_ONE) * 2^k, |q| <= 3
# cube_luck_tally int64[n_groups][5] (bgx_rollout_cube_luck_field): the luck of cubeful games
# (DESIGN.md §18), fixed point, 2^-16 points; the squares split as the cut tallies' (CUBE_CUT_SPLIT)
CUBE_LUCK_FIELDS = ("cube_luck", "cube_luck2_lo", "cube_luck2_hi", "cube_yluck", "cube_luck_games")
CUBE_LUCK_ONE = 65536               # Lq = rint(L * CUBE_LUCK_ONE), L in points
CUBE_LUCK_CLAMP = 1 << 31           # |Lq| <= CUBE_LUCK_CLAMP


# ------------------------------------------------------------------ what the summaries share --
def _row(row, fields, what):
    """The row as Python ints; ValueError(f"{what} has ...") unless it has one entry per field."""
    t = [int(v) for v in row]
    if len(t) != len(fields):
        raise ValueError(f"{what} has {len(fields)} entries, got {len(t)}")
    return t


def _natural_sums(r):
    """(sum of the results, sum of their squares) in points of the games played to the end, from
    summarize's dict: integers."""
    w, l = [r[f"win{j}"] for j in (1, 2, 3)], [r[f"loss{j}"] for j in (1, 2, 3)]
    return (sum((k + 1) * (w[k] - l[k]) for k in range(3)), sum((k + 1) ** 2 * (w[k] + l[k]) for k in range(3)))


def _mean_stderr(n, s1, s2, one):
    """(mean, standard error of the mean) in points of n results with the integer sums s1 (in
    1 / one points) and s2 (squares, in 1 / one^2); n = 0: mean 0.0; n < 2: standard error 0.0."""
    var_num = max(n * s2 - s1 * s1, 0)                       # n^2 (n - 1) one^2 x the variance of the mean
    return (s1 / (n * one) if n > 0 else 0.0,
            math.sqrt(var_num / (n * n * (n - 1))) / one if n > 1 else 0.0)


def _per_game(v, n):
    return v / n if n > 0 else 0.0


def _luck_adjusted(r, n, c, sr, sr2, sl, sl2, srl):
    """summarize_luck's formulas with the coefficient c on the sums in points: sr, sr2 of the
    results, sl, sl2 of the luck, srl of their products; r["equity"] is the raw mean."""
    inv = 1.0 / n if n > 0 else 0.0
    eq = (sr - c * sl) * inv
    var_y = max(sr2 - 2.0 * c * srl + c * c * sl2 - n * eq * eq, 0.0) / (n - 1) if n > 1 else 0.0
    var_r = max(sr2 - n * r["equity"] ** 2, 0.0) / (n - 1) if n > 1 else 0.0
    r.update(luck_scale=c, luck_mean=sl * inv, equity_luck=eq, equity_luck_stderr=math.sqrt(var_y * inv),
             variance_ratio=var_y / var_r if var_r > 0.0 else 1.0)
    return r


# --------------------------------------------------------------------------- cubeless play --
def summarize(tally_row, unfinished: int = 0) -> dict:
    """One position's result from its 8 tally entries: `games`, `plies_per_game`, the
    cumulative rates of each side (`win` = any win, `win_gammon` = gammon or backgammon,
    `win_backgammon`; `loss*` likewise), `equity` = sum_k k (WINk - LOSSk) / games in points,
    `equity_stderr` = sqrt((sum_k k^2 (WINk + LOSSk) - games equity^2) / (games - 1) / games),
    the standard error of a mean of independent games, and `unfinished` (scheduled games that
    did not end).  With stratified first rolls the games are not independent draws -- each
    first roll occurs exactly equally often, which removes that part of the variance -- so
    the standard error is a conservative bound there.  No games: the rates are 0; one game:
    the standard error is 0."""
    t = _row(tally_row, FIELDS, "summarize: a tally row")
    r = dict(zip(FIELDS, t))
    g = r["games"]
    w, l = t[2:5], t[5:8]
    inv = 1.0 / g if g > 0 else 0.0
    s1, sq = _natural_sums(r)
    eq = s1 * inv
    var = max(sq - g * eq * eq, 0.0) / (g - 1) / g if g > 1 else 0.0
    r.update(plies_per_game=r["plies"] * inv,
             win=sum(w) * inv, win_gammon=(w[1] + w[2]) * inv, win_backgammon=w[2] * inv,
             loss=sum(l) * inv, loss_gammon=(l[1] + l[2]) * inv, loss_backgammon=l[2] * inv,
             equity=eq, equity_stderr=math.sqrt(var), unfinished=int(unfinished))
    return r


def summarize_luck(tally_row, luck_row, scale="fit", unfinished: int = 0) -> dict:
    """summarize(tally_row, unfinished) plus the luck-adjusted estimate from the row's 4 luck
    sums (LUCK_FIELDS; DESIGN.md "Luck adjustment").  A game's adjusted result is
    y = res - c L with L its luck (the sum over its rolls of the value after the roll that came
    minus the mean over all 21 rolls, signed for the start mover).  E[L] = 0, so any constant
    c leaves the mean unbiased.  In fp64 from the integer sums, n = games, sum L = LUCK / 2^16,
    sum L^2 = LUCK2 / 2^32, sum res L = RESLUCK / 2^16:
        equity_luck = (sum res - c sum L) / n
        var_y = (sum res^2 - 2 c sum res L + c^2 sum L^2 - n equity_luck^2) / (n - 1), >= 0
        equity_luck_stderr = sqrt(var_y / n)        variance_ratio = var_y / var_res
    (variance_ratio 1.0 when var_res is 0; n < 2: the stderr is 0).  `scale` = "fit": the
    control-variate coefficient c = cov(res, L) / var(L) of these games (0 when var(L) is 0),
    which absorbs the unit difference between the net's reward scale and points and never
    raises the variance in the limit; fitted on the same games, it biases equity_luck by
    O(1/n).  A float: that fixed c (1.0 when the net's values are in points).  Adds luck_scale
    (c), luck_mean (sum L / n), equity_luck, equity_luck_stderr and variance_ratio.  Raises
    ValueError when the luck row counts other games than the tally row."""
    r = summarize(tally_row, unfinished)
    k = _row(luck_row, LUCK_FIELDS, "summarize_luck: a luck row")
    n = r["games"]
    if k[3] != n:
        raise ValueError(f"summarize_luck: the luck row counts {k[3]} games, the tally row {n}")
    sl, sl2, srl = k[0] / LUCK_ONE, k[1] / (LUCK_ONE * LUCK_ONE), k[2] / LUCK_ONE
    sr, sr2 = _natural_sums(r)
    if scale == "fit":
        # numerator and denominator times n, as exact integers: a constant result gives 0
        num, den = n * k[2] - sr * k[0], n * k[1] - k[0] * k[0]
        c = LUCK_ONE * (num / den) if den > 0 else 0.0
    else:
        c = float(scale)
    return _luck_adjusted(r, n, c, sr, float(sr2), sl, sl2, srl)


def summarize_bearoff(tally_row, cut_row, unfinished: int = 0) -> dict:
    """One position's result from its 8 tally entries (the games played to the end) and its 4
    cut sums (CUT_FIELDS: the games that reached the bearoff table and were scored with the
    start mover's exact win probability P).  A cut game's result is y = 2 P - 1
    points (a single game: both sides have checkers off).  With n_c cut games,
    sum P = CUT_P / 2^20 and sum P^2 = CUT_P2 / 2^40: sum y = 2 sum P - n_c and
    sum y^2 = 4 sum P^2 - 4 sum P + n_c.  On summarize's fields: `games` = natural + cut,
    `equity` = (sum res + sum y) / games, `equity_stderr` from sum res^2 + sum y^2 as summarize
    forms it, `win` = (wins + sum P) / games and `loss` likewise, the gammon and backgammon
    rates count natural games only (over all games), `plies_per_game` over both kinds; adds
    `natural_games`, `cut_games` and `cut_share` = cut_games / games.  The sums are combined as
    integers, so equal cut values give their value exactly and a standard error of 0.  The
    cut removes the endgame's dice noise, so equity_stderr is that of the mixed sample."""
    r = summarize(tally_row, unfinished)
    n_c, cut_plies, sp, sp2 = _row(cut_row, CUT_FIELDS, "summarize_bearoff: a cut row")
    w, l = [r[f"win{j}"] for j in (1, 2, 3)], [r[f"loss{j}"] for j in (1, 2, 3)]
    n_nat = r["games"]
    n = n_nat + n_c
    # sum of results in 2^-20 points, sum of squares in 2^-40: exact integers
    r1, r2 = _natural_sums(r)
    s1 = r1 * CUT_ONE + 2 * sp - n_c * CUT_ONE
    s2 = r2 * CUT_ONE ** 2 + 4 * sp2 - 4 * sp * CUT_ONE + n_c * CUT_ONE ** 2
    inv = 1.0 / n if n > 0 else 0.0
    equity, stderr = _mean_stderr(n, s1, s2, CUT_ONE)
    r.update(games=n, natural_games=n_nat, cut_games=n_c, cut_share=n_c * inv,
             plies_per_game=(r["plies"] + cut_plies) * inv,
             win=(sum(w) * CUT_ONE + sp) / (n * CUT_ONE) if n > 0 else 0.0,
             loss=(sum(l) * CUT_ONE + n_c * CUT_ONE - sp) / (n * CUT_ONE) if n > 0 else 0.0,
             win_gammon=(w[1] + w[2]) * inv, win_backgammon=w[2] * inv,
             loss_gammon=(l[1] + l[2]) * inv, loss_backgammon=l[2] * inv,
             equity=equity, equity_stderr=stderr)
    return r


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
    r = summarize(tally_row, unfinished)
    c = _row(trunc_row, TRUNC_FIELDS, "summarize_truncated: a row")
    n_t, t_plies, sv, sv2 = c[:4]
    n_nat = r["games"]
    n = n_nat + n_t
    # sum of results in 2^-16 points, sum of squares in 2^-32: exact integers
    r1, r2 = _natural_sums(r)
    equity, stderr = _mean_stderr(n, r1 * TRUNC_ONE + sv, r2 * TRUNC_ONE ** 2 + sv2, TRUNC_ONE)
    inv = 1.0 / n if n > 0 else 0.0
    r.update(games=n, natural_games=n_nat, truncated_games=n_t, truncated_share=n_t * inv,
             truncated_equity=sv / (n_t * TRUNC_ONE) if n_t > 0 else 0.0,
             plies_per_game=(r["plies"] + t_plies) * inv, equity=equity, equity_stderr=stderr)
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
    r = summarize_truncated(tally_row, trunc_row, unfinished)
    k = _row(luck_row, LUCK_FIELDS, "summarize_truncated_luck: a row")
    c7 = [r[f] for f in TRUNC_FIELDS]
    if k[3] != r["natural_games"]:
        raise ValueError(f"summarize_truncated_luck: the luck row counts {k[3]} games, the tally row "
                         f"{r['natural_games']}")
    n, one = r["games"], TRUNC_ONE
    r1, r2 = _natural_sums(r)
    y1, y2 = r1 * one + c7[2], r2 * one * one + c7[3]                                 # 2^-16, 2^-32
    il, il2, iyl = k[0] + c7[4], k[1] + c7[5], k[2] * one + c7[6]                     # 2^-16, 2^-32, 2^-32
    sl, sl2, srl = il / one, il2 / (one * one), iyl / (one * one)
    if scale == "fit":
        num, den = n * iyl - y1 * il, n * il2 - il * il          # both in 2^-32: a constant result gives 0
        c = num / den if den > 0 else 0.0
    else:
        c = float(scale)
    return _luck_adjusted(r, n, c, y1 / one, y2 / (one * one), sl, sl2, srl)


# ---------------------------------------------------------------------------- cubeful play --
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
    played = summarize(tally_row, unfinished)
    r = dict(zip(CUBE_FIELDS, _row(cube_row, CUBE_FIELDS, "summarize_cube: a cube row")))
    n = r["cube_games"]
    if n != played["games"] + r["pass_games"]:
        raise ValueError(f"summarize_cube: the cube row counts {n} games, the tally row {played['games']} and "
                         f"{r['pass_games']} passed")
    var_num = max(n * r["cube_points2"] - r["cube_points"] ** 2, 0)        # n^2 (n - 1) x the variance of the mean
    r.update(games=n, equity_cubeful=_per_game(r["cube_points"], n),
             equity_cubeful_stderr=math.sqrt(var_num / (n * n * (n - 1))) if n > 1 else 0.0,
             unfinished=int(unfinished), played_out=played)
    return _cube_rates(r, n)


def summarize_cube_luck(tally_row, cube_row, luck_row, scale="fit", unfinished: int = 0) -> dict:
    """summarize_cube(tally_row, cube_row, unfinished) plus the luck-adjusted cubeful estimate from
    the row's 5 luck sums (CUBE_LUCK_FIELDS), with summarize_luck's formulas on y, a
    game's cubeful result in points (played out and passed games alike), and L, its luck in
    points (the sum over its rolls of 2^k times the cubeful luck of the roll, signed for the start
    mover).  E[L] = 0, so any constant c leaves the mean unbiased.  From the integer sums, n =
    games, sum y = CUBE_POINTS, sum y^2 = CUBE_POINTS2, sum L = LUCK / 2^16, sum L^2 =
    (LUCK2_HI 2^30 + LUCK2_LO) / 2^32, sum y L = YLUCK / 2^16:
        equity_cubeful_luck = (sum y - c sum L) / n
        var_a = (sum y^2 - 2 c sum y L + c^2 sum L^2 - n equity_cubeful_luck^2) / (n - 1), >= 0
        equity_cubeful_luck_stderr = sqrt(var_a / n)        variance_ratio = var_a / var_y
    (variance_ratio 1.0 when var_y is 0; n < 2: the stderr is 0).  `scale` = "fit": c = cov(y, L) /
    var(L) of these games, numerator and denominator as exact integers (0 when var(L) is 0); a
    float: that fixed c.  Adds luck_scale (c), luck_mean (sum L / n), equity_cubeful_luck,
    equity_cubeful_luck_stderr, variance_ratio and the 5 sums under their names.  Raises ValueError
    when the luck row counts other games than the cube row."""
    r = summarize_cube(tally_row, cube_row, unfinished)
    k = _row(luck_row, CUBE_LUCK_FIELDS, "summarize_cube_luck: a luck row")
    n, one = r["games"], CUBE_LUCK_ONE
    if k[4] != n:
        raise ValueError(f"summarize_cube_luck: the luck row counts {k[4]} games, the cube row {n}")
    sy, sy2 = r["cube_points"], r["cube_points2"]
    il, il2, iyl = k[0], (k[2] << CUBE_CUT_SPLIT) + k[1], k[3]                        # 2^-16, 2^-32, 2^-16
    if scale == "fit":
        # numerator (2^-16) and denominator (2^-32) times n, as exact integers: a constant result gives 0
        num, den = n * iyl - sy * il, n * il2 - il * il
        c = one * (num / den) if den > 0 else 0.0
    else:
        c = float(scale)
    sl, sl2, syl = il / one, il2 / (one * one), iyl / one
    inv = 1.0 / n if n > 0 else 0.0
    eq = (sy - c * sl) * inv
    raw = r["equity_cubeful"]
    var_a = max(sy2 - 2.0 * c * syl + c * c * sl2 - n * eq * eq, 0.0) / (n - 1) if n > 1 else 0.0
    var_y = max(sy2 - n * raw * raw, 0.0) / (n - 1) if n > 1 else 0.0
    r.update(zip(CUBE_LUCK_FIELDS, k))
    r.update(luck_scale=c, luck_mean=sl * inv, equity_cubeful_luck=eq, equity_cubeful_luck_stderr=math.sqrt(var_a * inv),
             variance_ratio=var_a / var_y if var_y > 0.0 else 1.0)
    return r


def _cube_rates(r, n, log2: int = 0, plies: int = 0):
    """The per-game rates of a cubeful summary over its n games, with the cut and truncated games'
    `log2` and `plies` beside the cube row's and the played-out games' own."""
    r.update(pass_share=_per_game(r["pass_games"], n), doubles_per_game=_per_game(r["doubles"], n),
             mean_cube_log2=_per_game(r["cube_log2"] + log2, n),
             plies_per_game=_per_game(r["played_out"]["plies"] + r["pass_plies"] + plies, n))
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
    cut = dict(zip(CUBE_CUT_FIELDS, _row(cut_row, CUBE_CUT_FIELDS, "summarize_cube_bearoff: a cut row")))
    n = r["cube_games"] + cut["cut_games"]
    s1 = r["cube_points"] * CUBE_CUT_ONE + cut["cut_y"]
    s2 = r["cube_points2"] * CUBE_CUT_ONE ** 2 + (cut["cut_y2_hi"] << CUBE_CUT_SPLIT) + cut["cut_y2_lo"]
    equity, stderr = _mean_stderr(n, s1, s2, CUBE_CUT_ONE)
    r.update(cut, games=n, cut_share=_per_game(cut["cut_games"], n), equity_cubeful=equity, equity_cubeful_stderr=stderr)
    return _cube_rates(r, n, cut["cut_log2"], cut["cut_plies"])


def summarize_cube_truncated(tally_row, cube_row, trunc_row, unfinished: int = 0, cut_row=None) -> dict:
    """summarize_cube(tally_row, cube_row, unfinished) for a truncated cubeful run,
    with the row's 6 truncation sums (CUBE_TRUNC_FIELDS) and, when the run was also cut at the
    cubeful bearoff table, its 6 cut sums `cut_row` (CUBE_CUT_FIELDS).  A truncated game's result
    is y = Yq / 2^16 points, Janowski's estimate times the cube.  `games` = played out + passed +
    truncated (+ cut); `equity_cubeful` and `equity_cubeful_stderr` over all kinds together from
    Python integers, in units of 2^-16 (2^-20 with cut_row: the truncation's sums are rescaled
    by 2^4 and 2^8), so equal results give their value exactly and a standard error of 0.
    `pass_share`, `doubles_per_game`, `mean_cube_log2` and `plies_per_game` are over all games;
    adds `truncated_games`, `truncated_share`, `truncated_equity_cubeful` (the truncated games'
    mean result in points), with cut_row `cut_share`, and the sums under their names.  The
    standard error is the sample's spread: it contains neither the net's error nor the rule's.
    Raises ValueError when CUBE_GAMES != GAMES + PASS_GAMES."""
    r = summarize_cube(tally_row, cube_row, unfinished)
    tr = dict(zip(CUBE_TRUNC_FIELDS, _row(trunc_row, CUBE_TRUNC_FIELDS, "summarize_cube_truncated: a truncation row")))
    ty, ty2 = tr["cube_trunc_y"], (tr["cube_trunc_y2_hi"] << CUBE_CUT_SPLIT) + tr["cube_trunc_y2_lo"]
    cut = None
    if cut_row is not None:
        cut = dict(zip(CUBE_CUT_FIELDS, _row(cut_row, CUBE_CUT_FIELDS, "summarize_cube_truncated: a cut row")))
    one = CUBE_TRUNC_ONE if cut is None else CUBE_CUT_ONE
    up = one // CUBE_TRUNC_ONE
    n_t = tr["cube_trunc_games"]
    n = r["cube_games"] + n_t + (cut["cut_games"] if cut else 0)
    s1 = r["cube_points"] * one + ty * up + (cut["cut_y"] if cut else 0)
    s2 = (r["cube_points2"] * one * one + ty2 * up * up +
          ((cut["cut_y2_hi"] << CUBE_CUT_SPLIT) + cut["cut_y2_lo"] if cut else 0))
    equity, stderr = _mean_stderr(n, s1, s2, one)
    r.update(tr)
    if cut:
        r.update(cut, cut_share=_per_game(cut["cut_games"], n))
    r.update(games=n, truncated_games=n_t, truncated_share=_per_game(n_t, n),
             truncated_equity_cubeful=ty / (n_t * CUBE_TRUNC_ONE) if n_t > 0 else 0.0,
             equity_cubeful=equity, equity_cubeful_stderr=stderr)
    return _cube_rates(r, n, tr["cube_trunc_log2"] + (cut["cut_log2"] if cut else 0),
                       tr["cube_trunc_plies"] + (cut["cut_plies"] if cut else 0))
