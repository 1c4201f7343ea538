"""The arena's match kernels (csrc/bg_match.h; include/bgx.h bgx_arena_match_*) written out in
scalar Python, one lane at a time in numpy float32 scalars, and a hand-set state for them:
tests/test_gpu_match.py runs the kernels on the state and compares every array;
tests/test_match_cpu.py checks that the state reaches every branch (BRANCHES) and every counted
field without a GPU, and that the scalar rule agrees with match.match_decision_reference."""
import numpy as np

F = np.float32
R_CUR, R_OVER = 52, 55
N, M, CAP = 300, 2, 10                      # two 256-thread blocks, a partial last wave; 2 matches per lane
LENGTHS = (5, 7)
# (scale, window, win_gammons, loss_gammons)
RULE_A = (1.0, 0.65, 0.25, 0.25)
RULE_B = (2.0, 0.0, 0.4, 0.1)
MATCH_FIELDS = ("matches", "match_wins_a", "match_games", "pass_games", "match_points_a", "match_points_b",
                "doubles_a", "doubles_b", "passes_a", "passes_b", "cube_log2", "crawford_games",
                "post_crawford_games", "pass_plies", "match_wins_a_seat0", "matches_seat0")
MF = {k: i for i, k in enumerate(MATCH_FIELDS)}
BRANCHES = {"retired", "first_ply", "game_over", "crawford_game", "dead_cube", "owner_mismatch", "invalid_byte",
            "may_double_a", "may_double_b", "nan_offer", "too_good", "window", "free_double", "no_double", "offer_a",
            "offer_b", "foreign_dsel", "take_by_a", "take_by_b", "nan_takes", "pass_by_a", "pass_by_b",
            "pass_match_goes_on", "pass_to_crawford", "reseat_a", "reseat_b", "win_a", "win_b", "gammon_at_the_cube",
            "overshoot", "played_ends_match", "played_ends_last_match", "played_match_goes_on", "to_crawford",
            "crawford_to_post", "post_crawford_game", "done_without_winner", "ply", "done_of_a_retired_lane",
            "a_is_player1", "a_is_player2", "retire_flag_of_a_retired_lane"}
# With access the doubler needs more than the cube shows, so a pass leaves it short of the match:
# respond's "the match ends" and "the lane's last match" paths exist but no state reaches them.
UNREACHABLE = {"pass_ends_match", "pass_ends_last_match", "reseat_retired"}


def games_quota(L):
    return M * (2 * L - 1)


def cube_k(c):
    return min(int(c) & 15, CAP)


def cube_owner(c):
    o = (int(c) >> 4) & 3
    return 0 if o == 3 else o


def a_p1(i, g):
    return ((i + g) & 1) == 0


# ------------------------------------------------------------- part 1, scalar --
def met_after(t, me, opp, craw):
    met, pc, L = t
    if me <= 0:
        return F(1.0)
    if opp <= 0:
        return F(0.0)
    me, opp = min(me, L), min(opp, L)
    if craw != 0:
        return F(1.0) - pc[opp] if me == 1 else pc[me]
    return met[me, opp]


def match_p(scale, v, gw, gl):
    W, L_ = F(1.0) + F(gw), F(1.0) + F(gl)
    with np.errstate(all="ignore"):
        c = F(scale) * F(v)
        c = -L_ if c < -L_ else W if c > W else c
        return (c + L_) / (W + L_)


def match_values(t, x, y, craw, k, p, gw, gl):
    gw, gl, v = F(gw), F(gl), 1 << k
    win = lambda n: (F(1.0) - gw) * met_after(t, x - n, y, craw) + gw * met_after(t, x - 2 * n, y, craw)    # noqa: E731
    loss = lambda n: ((F(1.0) - gl) * (F(1.0) - met_after(t, y - n, x, craw))                                # noqa: E731
                      + gl * (F(1.0) - met_after(t, y - 2 * n, x, craw)))
    with np.errstate(all="ignore"):
        w1, l1, w2, l2 = win(v), loss(v), win(2 * v), loss(2 * v)
        return l1 + p * (w1 - l1), l2 + p * (w2 - l2), met_after(t, x - v, y, craw)


def access(c, mover, plies, over, active, craw, x):
    return bool(plies > 0 and not over and active and craw != 1 and cube_k(c) < CAP
                and cube_owner(c) in (0, (mover & 1) + 1) and x > (1 << cube_k(c)))


def offers(t, x, y, craw, k, rule, value, seen=None):
    scale, window, wg, lg = rule
    p = match_p(scale, value, wg, lg)
    nd, dt, dp = match_values(t, x, y, craw, k, p, wg, lg)
    with np.errstate(all="ignore"):
        if not nd <= dp:
            why, yes = ("nan_offer" if np.isnan(nd) else "too_good"), False
        elif dt - nd >= F(window) * (dp - nd):
            why, yes = "window", True
        elif y <= (1 << k) and dt > nd:
            why, yes = "free_double", True
        else:
            why, yes = "no_double", False
    if seen is not None:
        seen.add(why)
    return yes


def passes(t, x, y, craw, k, rule, value):
    scale, _, wg, lg = rule
    p = match_p(scale, value, lg, wg)                      # the doubler's chances: the shares swapped
    _, dt, dp = match_values(t, x, y, craw, k, p, lg, wg)
    return bool(dt > dp)


def end_game(away, craw, L, w, points):
    """-> (away, craw, match over)"""
    a = [int(away[0]), int(away[1])]
    left = a[w] - points
    if left <= 0:
        return [L, L], 0, True
    a[w] = left
    return a, (1 if craw == 0 and left == 1 else 2 if craw == 1 else craw), False


# ------------------------------------------------------------- the hand-set state --
def make_state(L, seed=35):
    """Every Crawford state, away 1..L on both sides, cube bytes that are no cube states and dead
    cubes, retired lanes, game_over records, both seats, synthetic values with NaN and the
    infinities, lanes in their last match with little to go."""
    from bgx.match import met_table
    rng = np.random.RandomState(seed + L)
    G = games_quota(L)
    recs = rng.randint(0, 4, (N, 64)).astype(np.uint8)
    recs[:, R_CUR] = rng.randint(0, 2, N)
    recs[:, R_OVER] = rng.rand(N) < 0.05
    matches = rng.choice([0, 1, 2], N, p=[0.35, 0.53, 0.12]).astype(np.int32)
    games = np.where(matches >= M, G, rng.randint(0, 4, N)).astype(np.int32)
    active = games < G
    a_moves = (recs[:, R_CUR] == 0) == (((np.arange(N) + games) & 1) == 0)
    away = rng.randint(1, L + 1, (N, 2)).astype(np.uint8)
    near = rng.rand(N) < 0.35                               # close to the end: matches end in this step
    away[near] = rng.randint(1, 3, (int(near.sum()), 2))
    craw = rng.choice([0, 1, 2], N, p=[0.6, 0.15, 0.25]).astype(np.uint8)
    k = rng.choice([0, 1, 2, 3], N, p=[0.55, 0.3, 0.1, 0.05])
    owner = np.where(k == 0, 0, rng.randint(1, 3, N))
    cube = (k | (owner << 4)).astype(np.uint8)
    odd = rng.rand(N) < 0.1
    n_odd = int(odd.sum())                                  # any high bits and owner 3, k small or past the cap
    cube[odd] = (rng.randint(0, 4, n_odd) << 6) | (rng.randint(0, 4, n_odd) << 4) | rng.choice([0, 1, 2, 12, 15], n_odd)
    values = np.array([-3, -1, -.5, -.2, 0, .1, .2, .3, .4, .5, .6, .7, .8, .9, 1, 1.2, 3, np.nan, np.inf, -np.inf], F)
    done = rng.rand(N) < 0.35
    winner = np.where(rng.rand(N) < 0.12, -1, rng.randint(0, 2, N))
    info = np.where(done, ((winner + 1) << 8) | (rng.randint(1, 4, N) << 16), 0).astype(np.int32)
    foreign = np.zeros(N, bool)
    foreign[rng.choice(N, 40, replace=False)] = True
    stale = ~active & (rng.rand(N) < 0.3)                   # a retire flag on a lane that is retired already
    met, pc = met_table(L)
    return dict(recs=recs, games_done=games, matches_done=matches, sel_a=(active & a_moves).astype(np.uint8),
                sel_b=(active & ~a_moves).astype(np.uint8), away=away, craw=craw, cube=cube,
                plies=rng.randint(0, 4, N).astype(np.int32), seat0=rng.randint(0, 2, N).astype(np.uint8),
                retire=stale.astype(np.uint8), eq_a=rng.choice(values, N), eq_b=rng.choice(values, N),
                er_a=rng.choice(values, N), er_b=rng.choice(values, N), new_mover=rng.randint(0, 2, N).astype(np.uint8),
                done=done.astype(np.uint8), info=info, foreign=foreign, met=met, pc=pc)


def lane_access(s, i, a_on_roll, active):
    r = s["recs"][i]
    return access(s["cube"][i], int(r[R_CUR]), int(s["plies"][i]), r[R_OVER] != 0, active, int(s["craw"][i]),
                  int(s["away"][i, 0 if a_on_roll else 1]))


def sides(s, i):
    sa = s["sel_a"][i] != 0
    return sa, (not sa) and s["sel_b"][i] != 0


def ref_sel(s, seen):
    da, db = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        sa, sb = sides(s, i)
        d = lane_access(s, i, sa, sa or sb)
        da[i], db[i] = d and sa, d and sb
        c, m = s["cube"][i], int(s["recs"][i, R_CUR])
        if not (sa or sb):
            seen.add("retired")
        elif s["plies"][i] == 0:
            seen.add("first_ply")
        elif s["recs"][i, R_OVER]:
            seen.add("game_over")
        elif s["craw"][i] == 1:
            seen.add("crawford_game")
        elif cube_owner(c) not in (0, m + 1):
            seen.add("owner_mismatch")
        elif not d:
            seen.add("dead_cube")
        else:
            seen.add("may_double_a" if sa else "may_double_b")
            seen.add("a_is_player1" if (m == 0) == bool(sa) else "a_is_player2")
            if (int(c) & 15) > CAP or (int(c) >> 4) & 3 == 3 or int(c) > 63:
                seen.add("invalid_byte")
    return da, db


def xyk(s, i, sa):
    return (int(s["away"][i, 0 if sa else 1]), int(s["away"][i, 1 if sa else 0]), int(s["craw"][i]), cube_k(s["cube"][i]))


def ref_offer(s, t, dsel_a, dsel_b, mt, seen):
    oa, ob = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        sa, sb = sides(s, i)
        da, db = sa and dsel_a[i] != 0, sb and dsel_b[i] != 0
        if not (da or db):
            continue
        if not lane_access(s, i, sa, True):
            seen.add("foreign_dsel")
            continue
        o = offers(t, *xyk(s, i, sa), RULE_A if sa else RULE_B, s["eq_a"][i] if sa else s["eq_b"][i], seen)
        oa[i], ob[i] = o and sa, o and sb
        if o:
            seen.add("offer_a" if sa else "offer_b")
            mt[MF["doubles_a" if sa else "doubles_b"]] += 1
    return oa, ob


def score(s, i, L, a_won, points, k, g_next, mt, seen, how, passed_by=None):
    """The end of a game on lane i, in place; True when the lane's last match ended."""
    cr = int(s["craw"][i])
    mt[MF["match_games"]] += 1
    mt[MF["match_points_a" if a_won else "match_points_b"]] += points
    mt[MF["cube_log2"]] += k
    mt[MF["crawford_games"]] += cr == 1
    mt[MF["post_crawford_games"]] += cr == 2
    if passed_by:
        mt[MF["pass_games"]] += 1
        mt[MF["passes_" + passed_by]] += 1
        mt[MF["pass_plies"]] += int(s["plies"][i])
    if cr == 2:
        seen.add("post_crawford_game")
    need = int(s["away"][i, 0 if a_won else 1])
    away, cr2, over = end_game(s["away"][i], cr, L, 0 if a_won else 1, points)
    s["away"][i], s["craw"][i] = away, cr2
    if not over:
        seen.add(f"{how}_match_goes_on")
        if cr == 0 and cr2 == 1:
            seen.add("pass_to_crawford" if passed_by else "to_crawford")
        if cr == 1:
            seen.add("crawford_to_post")
        return False
    if points > need:
        seen.add("overshoot")
    mt[MF["matches"]] += 1
    mt[MF["match_wins_a"]] += a_won
    mt[MF["matches_seat0"]] += int(s["seat0"][i] != 0)
    mt[MF["match_wins_a_seat0"]] += int(a_won and s["seat0"][i] != 0)
    s["seat0"][i] = a_p1(i, g_next)
    s["matches_done"][i] += 1
    last = s["matches_done"][i] >= M
    seen.add(f"{how}_ends_last_match" if last else f"{how}_ends_match")
    return bool(last)


def ref_respond(s, t, L, off_a, off_b, tally, mt, seen):
    """In place on s.  Returns the reset mask."""
    G, mask = games_quota(L), np.zeros(N, np.uint8)
    for i in range(N):
        sa, sb = sides(s, i)
        oa, ob = sa and off_a[i] != 0, sb and off_b[i] != 0
        g = int(s["games_done"][i])
        if not (oa or ob) or g >= G or not lane_access(s, i, sa, True):
            continue
        x, y, cr, k = xyk(s, i, sa)
        eq = s["er_b"][i] if oa else s["er_a"][i]             # the other side's estimate, by its rule
        if passes(t, x, y, cr, k, RULE_B if oa else RULE_A, eq):
            last = score(s, i, L, bool(oa), 1 << k, k, g + 1, mt, seen, "pass", "b" if oa else "a")
            s["plies"][i], s["cube"][i] = 0, 0
            s["games_done"][i] = G if last else g + 1
            s["sel_a"][i] = s["sel_b"][i] = 0
            mask[i] = 1
            tally[13] -= last
            seen.add("pass_by_a" if ob else "pass_by_b")
        else:
            s["cube"][i] = (k + 1) | ((2 - (int(s["recs"][i, R_CUR]) & 1)) << 4)
            seen.add("take_by_a" if ob else "take_by_b")
            if np.isnan(eq):
                seen.add("nan_takes")
    return mask


def ref_reseat(s, L, mask, seen):
    """bgx_arena_cube_reseat, after the masked lanes got their new records (new_mover)."""
    G = games_quota(L)
    for i in range(N):
        if not mask[i]:
            continue
        g = int(s["games_done"][i])
        if g >= G:
            seen.add("reseat_retired")
            continue
        a_moves = (int(s["recs"][i, R_CUR]) & 1 == 0) == a_p1(i, g)
        s["sel_a"][i], s["sel_b"][i] = a_moves, not a_moves
        seen.add("reseat_a" if a_moves else "reseat_b")


def ref_flush(s, L, mt, seen):
    for i in range(N):
        on = s["sel_a"][i] or s["sel_b"][i]
        if not on:
            if s["done"][i]:
                seen.add("done_of_a_retired_lane")
            continue
        dn = s["done"][i] != 0
        info = int(s["info"][i])
        winner, sc = ((info >> 8) & 0xFF) - 1, min(max((info >> 16) & 0xFF, 1), 3)
        if dn and winner >= 0:
            g, k = int(s["games_done"][i]), cube_k(s["cube"][i])
            a_won = (winner == 0) == a_p1(i, g)
            if score(s, i, L, a_won, sc << k, k, g + 1, mt, seen, "played"):
                s["retire"][i] = 1
            seen.add("win_a" if a_won else "win_b")
            if k > 0 and sc > 1:
                seen.add("gammon_at_the_cube")
        elif dn:
            seen.add("done_without_winner")
        if dn:
            s["cube"][i], s["plies"][i] = 0, 0
        else:
            s["plies"][i] += 1
            seen.add("ply")


def ref_retire(s, L, tally, seen):
    G = games_quota(L)
    for i in range(N):
        if s["retire"][i]:
            s["retire"][i] = 0
            if s["games_done"][i] < G:
                tally[13] -= 1
            else:
                seen.add("retire_flag_of_a_retired_lane")
            s["games_done"][i] = G
            s["sel_a"][i] = s["sel_b"][i] = 0


LANE = ("cube", "plies", "away", "craw", "matches_done", "seat0", "games_done", "sel_a", "sel_b", "retire")


def run_reference(L, seed=35):
    """All six stages on make_state(L, seed): the state after each (copies), both tallies, the seen set."""
    s = make_state(L, seed)
    t = (s["met"], s["pc"], L)
    seen, tally, mt = set(), np.zeros(16, np.int64), np.zeros(16, np.int64)
    tally[13] = int((s["games_done"] < games_quota(L)).sum())
    out = {"state0": {k: v.copy() for k, v in s.items()}}
    dsel_a, dsel_b = ref_sel(s, seen)
    out["dsel"] = (dsel_a.copy(), dsel_b.copy())
    # a dsel of another origin: access is tested again in the offer
    dsel_a, dsel_b = dsel_a | (s["foreign"] & (s["sel_a"] != 0)), dsel_b | (s["foreign"] & (s["sel_b"] != 0))
    out["dsel_forced"] = (dsel_a.astype(np.uint8), dsel_b.astype(np.uint8))
    out["off"] = ref_offer(s, t, dsel_a, dsel_b, mt, seen)
    out["mt_offer"] = mt.copy()
    out["mask"] = ref_respond(s, t, L, *out["off"], tally, mt, seen)
    out["after_respond"] = {k: s[k].copy() for k in LANE}
    out["mt_respond"], out["tally_respond"] = mt.copy(), tally.copy()
    s["recs"][out["mask"] != 0, R_CUR] = s["new_mover"][out["mask"] != 0]          # the masked reset
    out["recs_reset"] = s["recs"].copy()
    ref_reseat(s, L, out["mask"], seen)
    out["after_reseat"] = {k: s[k].copy() for k in ("sel_a", "sel_b")}
    ref_flush(s, L, mt, seen)
    out["after_flush"] = {k: s[k].copy() for k in LANE}
    out["mt_flush"] = mt.copy()
    ref_retire(s, L, tally, seen)
    out["after_retire"] = {k: s[k].copy() for k in LANE}
    out["tally"] = tally.copy()
    return out, seen
