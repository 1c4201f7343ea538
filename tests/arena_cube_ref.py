"""The arena's cube kernels (csrc/bg_arena_cube.h; include/bgx.h bgx_arena_cube_*) written out in
scalar Python, one lane at a time, and a hand-set state for them: tests/test_gpu_arena_cube.py
runs the kernels on the state and compares every array; tests/test_arena_cube_cpu.py checks that
the state reaches every branch (BRANCHES) and every counted field without a GPU."""
import numpy as np

F = np.float32
R_CUR, R_OVER = 52, 55
N, G, CAP, JACOBY = 300, 2, 3, 1            # two 256-thread blocks, a partial last wave
# (scale, double_at, pass_at, too_good_at)
RULE_A = (1.0, 0.4, 0.5, 0.8)
RULE_B = (2.0, 0.3, 0.6, float("inf"))
CUBE_FIELDS = ("cube_games", "cube_points_a", "cube_points2", "cube_wins_a", "cube_log2", "pass_games", "pass_plies",
               "passes_a", "passes_b", "doubles_a", "doubles_b")
BRANCHES = {"retired", "first_ply", "game_over", "cap", "owner_mismatch", "invalid_byte", "may_double_a", "may_double_b",
            "nan_offer", "too_good", "below_double", "offer_a", "offer_b", "foreign_dsel", "take_by_a", "take_by_b",
            "nan_takes", "pass_by_a", "pass_by_b", "pass_last_game", "pass_with_games_left", "reseat_a", "reseat_b",
            "reseat_retired", "win_a", "win_b", "jacoby", "gammon_at_the_cube", "done_without_winner", "ply",
            "done_of_a_retired_lane", "a_is_player1", "a_is_player2"}


def cube_k(c, cap):
    return min(int(c) & 15, cap)


def cube_owner(c):
    o = (int(c) >> 4) & 3
    return 0 if o == 3 else o


def access(c, cap, m):
    return cube_k(c, cap) < cap and cube_owner(c) in (0, (m & 1) + 1)


def a_p1(i, g):
    return ((i + g) & 1) == 0


def make_state(seed=20):
    """Retired lanes, game_over records, bytes that are no cube states, both seats, synthetic
    equities on, beside and far from the thresholds."""
    rng = np.random.RandomState(seed)
    recs = rng.randint(0, 4, (N, 64)).astype(np.uint8)
    recs[:, R_CUR] = rng.randint(0, 2, N)
    recs[:, R_OVER] = rng.rand(N) < 0.05
    games = rng.choice([0, 1, 2], N, p=[0.45, 0.45, 0.10]).astype(np.int32)
    active = games < G
    a_moves = (recs[:, R_CUR] == 0) == (((np.arange(N) + games) & 1) == 0)
    k = rng.randint(0, CAP + 1, N)
    owner = np.where(k == 0, 0, rng.randint(1, 3, N))
    cube = (k | (owner << 4)).astype(np.uint8)
    odd = rng.rand(N) < 0.12
    cube[odd] = rng.randint(0, 256, int(odd.sum()))
    offers = np.array([-1, 0, .1, .15, .2, F(.4), .45, .6, .7, .9, np.nan, np.inf], F)
    answers = np.array([.1, .25, F(.3), .31, .5, .55, .9, np.nan, -np.inf], F)
    done = rng.rand(N) < 0.3
    winner = np.where(rng.rand(N) < 0.15, -1, rng.randint(0, 2, N))
    info = np.where(done, ((winner + 1) << 8) | (rng.randint(1, 4, N) << 16), 0).astype(np.int32)
    foreign = np.zeros(N, bool)
    foreign[rng.choice(N, 24, replace=False)] = True
    return dict(recs=recs, games_done=games, sel_a=(active & a_moves).astype(np.uint8),
                sel_b=(active & ~a_moves).astype(np.uint8), cube=cube, plies=rng.randint(0, 4, N).astype(np.int32),
                eq_a=rng.choice(offers, N), eq_b=rng.choice(offers, N), er_a=rng.choice(answers, N),
                er_b=rng.choice(answers, N), new_mover=rng.randint(0, 2, N).astype(np.uint8), done=done.astype(np.uint8),
                info=info, foreign=foreign)


def ref_sel(s, seen):
    da, db = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        m, c = int(s["recs"][i, R_CUR]), s["cube"][i]
        on = s["sel_a"][i] or s["sel_b"][i]
        d = s["plies"][i] > 0 and s["recs"][i, R_OVER] == 0 and access(c, CAP, m)
        da[i], db[i] = d and s["sel_a"][i] != 0, d and s["sel_b"][i] != 0
        if not on:
            seen.add("retired")
        elif s["plies"][i] == 0:
            seen.add("first_ply")
        elif s["recs"][i, R_OVER]:
            seen.add("game_over")
        elif cube_k(c, CAP) >= CAP:
            seen.add("cap")
        elif not d:
            seen.add("owner_mismatch")
        else:
            seen.add("may_double_a" if da[i] else "may_double_b")
            seen.add("a_is_player1" if (m == 0) == bool(da[i]) else "a_is_player2")
            if (int(c) & 15) > CAP or (int(c) >> 4) & 3 == 3 or int(c) > 63:
                seen.add("invalid_byte")
    return da, db


def offers(c, m, rule, eq, seen=None):
    scale, double_at, _, too_good = rule
    if not access(c, CAP, m):
        if seen is not None:
            seen.add("foreign_dsel")
        return False
    with np.errstate(invalid="ignore", over="ignore"):
        e = F(scale) * F(eq)                                  # one fp32 product
    yes = bool(e >= F(double_at) and e <= F(too_good))
    if seen is not None:
        seen.add("nan_offer" if np.isnan(e) else "too_good" if e > F(too_good) else "below_double" if e < F(double_at)
                 else "offered")
    return yes


def passes(rule, eq):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(F(rule[0]) * F(eq) > F(rule[2]))


def ref_offer(s, dsel_a, dsel_b, ct, seen):
    oa, ob = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for i in range(N):
        m, c = int(s["recs"][i, R_CUR]), s["cube"][i]
        oa[i] = dsel_a[i] != 0 and offers(c, m, RULE_A, s["eq_a"][i], seen)
        ob[i] = dsel_b[i] != 0 and offers(c, m, RULE_B, s["eq_b"][i], seen)
        if oa[i]:
            seen.add("offer_a")
        if ob[i]:
            seen.add("offer_b")
        ct[9] += oa[i]
        ct[10] += ob[i]
    seen.discard("offered")
    return oa, ob


def ref_respond(s, off_a, off_b, tally, ct, seen):
    """In place on s: cube, plies, games_done, sel_a, sel_b.  Returns the reset mask."""
    mask = np.zeros(N, np.uint8)
    for i in range(N):
        oa = off_a[i] != 0
        ob = not oa and off_b[i] != 0
        m, c, g = int(s["recs"][i, R_CUR]), s["cube"][i], int(s["games_done"][i])
        if not (oa or ob) or g >= G or not access(c, CAP, m):
            continue
        eq = s["er_b"][i] if oa else s["er_a"][i]             # the other side's estimate
        if passes(RULE_B if oa else RULE_A, eq):
            k = cube_k(c, CAP)
            y = (1 << k) if oa else -(1 << k)
            for f, v in enumerate((1, y, y * y, y > 0, k, 1, s["plies"][i], ob, oa)):
                ct[f] += int(v)
            s["plies"][i], s["cube"][i], s["games_done"][i] = 0, 0, g + 1
            s["sel_a"][i] = s["sel_b"][i] = 0
            mask[i] = 1
            if g + 1 >= G:
                tally[13] -= 1
            seen.add("pass_by_a" if ob else "pass_by_b")
            seen.add("pass_last_game" if g + 1 >= G else "pass_with_games_left")
        else:
            s["cube"][i] = (cube_k(c, CAP) + 1) | ((2 - (m & 1)) << 4)
            seen.add("take_by_a" if ob else "take_by_b")
            if np.isnan(eq):
                seen.add("nan_takes")
    return mask


def ref_reseat(s, mask, seen):
    """After the masked lanes got their new records (new_mover)."""
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


def ref_flush(s, ct, seen):
    for i in range(N):
        on = s["sel_a"][i] or s["sel_b"][i]
        dn = on and s["done"][i] != 0
        if not on:
            if s["done"][i]:
                seen.add("done_of_a_retired_lane")
            continue
        info = int(s["info"][i])
        winner, score = ((info >> 8) & 0xFF) - 1, min(max((info >> 16) & 0xFF, 1), 3)
        if dn and winner >= 0:
            k = cube_k(s["cube"][i], CAP)
            sc = 1 if JACOBY and k == 0 else score
            y = (sc << k) if (winner == 0) == a_p1(i, int(s["games_done"][i])) else -(sc << k)
            for f, v in enumerate((1, y, y * y, y > 0, k)):
                ct[f] += int(v)
            seen.add("win_a" if y > 0 else "win_b")
            if k == 0 and score > 1:
                seen.add("jacoby")
            if k > 0 and score > 1:
                seen.add("gammon_at_the_cube")
        elif dn:
            seen.add("done_without_winner")
        if dn:
            s["cube"][i], s["plies"][i] = 0, 0
        else:
            s["plies"][i] += 1
            seen.add("ply")


def run_reference(seed=20):
    """All five stages on make_state(seed): the state after each (copies), both tallies, the seen set."""
    s = make_state(seed)
    seen, tally, ct = set(), np.zeros(16, np.int64), np.zeros(16, np.int64)
    tally[13] = int((s["games_done"] < G).sum())
    out = {"state0": {k: v.copy() for k, v in s.items()}}
    dsel_a, dsel_b = ref_sel(s, seen)
    out["dsel"] = (dsel_a.copy(), dsel_b.copy())
    # a dsel of another origin: access is tested again in the offer
    dsel_a, dsel_b = dsel_a | (s["foreign"] & (s["sel_a"] != 0)), dsel_b | (s["foreign"] & (s["sel_b"] != 0))
    out["dsel_forced"] = (dsel_a.astype(np.uint8), dsel_b.astype(np.uint8))
    out["off"] = ref_offer(s, dsel_a, dsel_b, ct, seen)
    out["ct_offer"] = ct.copy()
    out["mask"] = ref_respond(s, *out["off"], tally, ct, seen)
    out["after_respond"] = {k: s[k].copy() for k in ("cube", "plies", "games_done", "sel_a", "sel_b")}
    out["ct_respond"], out["tally"] = ct.copy(), tally.copy()
    s["recs"][out["mask"] != 0, R_CUR] = s["new_mover"][out["mask"] != 0]          # the masked reset
    out["recs_reset"] = s["recs"].copy()
    ref_reseat(s, out["mask"], seen)
    out["after_reseat"] = {k: s[k].copy() for k in ("sel_a", "sel_b")}
    ref_flush(s, ct, seen)
    out["after_flush"] = {k: s[k].copy() for k in ("cube", "plies")}
    out["ct_flush"] = ct.copy()
    return out, seen
