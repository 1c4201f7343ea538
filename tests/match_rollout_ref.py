"""A hand-set state for the match-rollout kernels (csrc/bg_match_rollout.h; include/bgx.h
bgx_rollout_match_*, bgx_match_decision) and what they must make of it, by
match.match_decision_reference lane by lane: tests/test_gpu_match_rollout.py runs the kernels on
the state and compares every array; tests/test_match_rollout_cpu.py checks without a GPU that the
state reaches every branch (BRANCHES).  Also the short race positions of the traced runs and the
values that force a rule's decision at a score."""
import numpy as np

from bgx import match as M
from bgx.cube import pack

F = np.float32
R_CUR, R_OVER = 52, 55
N, P, G = 300, 6, 2                         # two 256-thread blocks, a partial last wave; six groups
LENGTHS = (5, 7)
RULES = {5: dict(scale=1.0, window=0.65, win_gammons=0.25, loss_gammons=0.25),
         7: dict(scale=1.5, window=0.7, win_gammons=0.4, loss_gammons=0.1)}
BRANCHES = {"unselected", "idle_group", "invalid_group", "first_ply", "game_over", "crawford_game", "owner_mismatch",
            "cap", "dead_cube", "invalid_byte", "nan", "too_good", "window", "free_double", "no_double", "take", "pass",
            "last_game", "pass_by_start", "pass_by_other", "done_with_winner", "done_without_winner", "done_unselected",
            "gammon_at_the_cube"}


def rule_of(L):
    return M.MatchRule(lambda eng, dsel: None, **RULES[L])


def make_state(L, seed=11):
    rng = np.random.RandomState(seed + L)
    # the groups' scores: before the Crawford game, the Crawford game, after it, far and near
    away = np.asarray([[L, L], [2, 3], [1, 4], [4, 1], [3, 2], [L - 1, 2]], np.uint8)
    craw = np.asarray([0, 0, 1, 2, 0, 0], np.uint8)
    group = rng.randint(0, P, size=N).astype(np.int32)
    group[rng.choice(N, 12, replace=False)] = -1
    group[[7, 130, 290]] = [P, 99, -5]                               # not a group: idle lanes too
    valid = (group >= 0) & (group < P)
    recs, starts = np.zeros((N, 64), np.uint8), np.zeros((N, 64), np.uint8)
    recs[:, R_CUR], starts[:, R_CUR] = rng.randint(2, size=N), rng.randint(2, size=N)
    recs[rng.choice(N, 10, replace=False), R_OVER] = 1
    states = [0, 0, 0, pack(1, 1), pack(1, 2), pack(2, 1), pack(2, 2), pack(3, 1), pack(10, 1), pack(10, 2)]
    cube = np.asarray(states, np.uint8)[rng.randint(len(states), size=N)]
    cube[[5, 77, 150]] = [0x0F, 0x31, 0x4B]                          # not cube states: read as (10, 0), (1, 0), (10, 0)
    cube0 = np.asarray(states, np.uint8)[rng.randint(len(states), size=N)]
    palette = np.asarray([-1.0, -0.3, 0.0, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.0, 3.0, np.nan, np.inf], F)
    value = palette[rng.randint(len(palette), size=N)]
    plies = rng.randint(0, 4, size=N).astype(np.int32)
    games_done = rng.randint(0, G, size=N).astype(np.int32)
    sel = (valid & (rng.rand(N) < 0.85)).astype(np.uint8)
    games_done[(sel == 0) & valid] = G
    done = (rng.rand(N) < 0.6).astype(np.uint8)
    winner, score = rng.randint(-1, 2, size=N), rng.randint(1, 4, size=N)
    info = (((winner + 1) << 8) | (score << 16)).astype(np.int32)
    return dict(L=L, away=away, craw=craw, group=group, recs=recs, starts=starts, cube=cube, cube0=cube0, value=value,
                plies=plies, games_done=games_done, sel=sel, done=done, info=info)


def expected(s, met, pc):
    """What sel, decide and flush (in that order) and bgx_match_decision make of the state, and the
    branches it reaches."""
    L, rule = s["L"], rule_of(s["L"])
    group = s["group"]
    valid = (group >= 0) & (group < P)
    gi = np.clip(group, 0, P - 1)
    m = s["recs"][:, R_CUR].astype(np.int64) & 1
    x, y, craw = s["away"][gi, m].astype(np.int64), s["away"][gi, 1 - m].astype(np.int64), s["craw"][gi].astype(np.int64)
    over, sel = s["recs"][:, R_OVER] != 0, (s["sel"] != 0) & valid
    d = M.match_decision_reference(met, pc, L, x, y, craw, s["cube"], m, s["plies"], s["value"], rule, over=over, active=sel)
    k = np.minimum(s["cube"].astype(np.int64) & 15, 10)
    o = (s["cube"].astype(np.int64) >> 4) & 3
    o = np.where(o == 3, 0, o)
    dsel, offer, pas = d["access"], d["offer"], d["passed"]
    take = offer & ~pas
    mine = m == (s["starts"][:, R_CUR].astype(np.int64) & 1)
    hist = np.zeros((P, 96), np.int64)

    def add(lanes, col, v=1):
        np.add.at(hist, (gi[lanes], np.broadcast_to(col, (N,))[lanes]), np.broadcast_to(v, (N,))[lanes])

    add(pas, M.match_bin(mine, 0, k))
    for col, v in ((88, 1), (89, 1), (92, s["plies"]), (93, k)):
        add(pas, col, v)
    add(offer & mine, 90)
    add(offer & ~mine, 91)
    c0 = (np.minimum(s["cube0"] & 15, 10) | (np.where(s["cube0"] >> 4 == 3, 0, s["cube0"] >> 4) << 4)).astype(np.uint8)
    cube = np.where(pas, c0, np.where(take, (k + 1) | ((2 - m) << 4), s["cube"])).astype(np.uint8)
    games = s["games_done"] + pas
    retired = pas & (games >= G)
    sel2 = sel & ~retired
    out = dict(dsel=dsel.astype(np.uint8), mask=pas.astype(np.uint8), cube=cube, games_done=games.astype(np.int32),
               plies=np.where(pas, 0, s["plies"]).astype(np.int32), sel=np.where(retired, 0, s["sel"]).astype(np.uint8),
               hist=hist.copy(), active=int(sel.sum()) - int(retired.sum()))
    # flush on the state decide left
    winner, score = ((s["info"] >> 8) & 0xFF) - 1, np.clip((s["info"] >> 16) & 0xFF, 1, 3)
    dn = s["done"] != 0
    fin = dn & sel2 & (winner >= 0)
    k2 = np.minimum(cube.astype(np.int64) & 15, 10)
    add(fin, M.match_bin(winner == (s["starts"][:, R_CUR] & 1), score, k2))
    add(fin, 88)
    add(fin, 93, k2)
    out.update(hist_flush=hist, cube_flush=np.where(dn, c0, cube).astype(np.uint8))
    # the static decision: per-lane scores, no plies term, every lane active
    aw = np.where(valid[:, None], s["away"][gi], np.asarray([[3, 3]], np.uint8)).astype(np.uint8)
    cr = np.where(valid, s["craw"][gi], 0).astype(np.uint8)
    xs, ys = aw[np.arange(N), m].astype(np.int64), aw[np.arange(N), 1 - m].astype(np.int64)
    ds = M.match_decision_reference(met, pc, L, xs, ys, cr, s["cube"], m, 1, s["value"], rule, over=over)
    with np.errstate(invalid="ignore"):
        flags = (ds["access"] * 1 + ds["offer"] * 2 + ds["passes"] * 4 + (ds["nd"] > ds["dp"]) * 8).astype(np.uint8)
    out.update(static_away=aw, static_craw=cr, values=np.stack([ds["nd"], ds["dt"], ds["dp"]], axis=1).astype(F), flags=flags)
    # the branches
    live = sel & (s["plies"] > 0) & ~over
    with np.errstate(invalid="ignore"):
        window = dsel & (d["nd"] <= d["dp"]) & ((d["dt"] - d["nd"]).astype(F) >= (F(rule.window) * (d["dp"] - d["nd"]).astype(F)).astype(F))
        too_good = dsel & (d["nd"] > d["dp"])
    seen = {name for name, hit in (
        ("unselected", valid & (s["sel"] == 0)), ("idle_group", group == -1), ("invalid_group", ~valid & (group != -1)),
        ("first_ply", sel & (s["plies"] == 0)), ("game_over", sel & over), ("crawford_game", live & (craw == 1)),
        ("owner_mismatch", live & (craw != 1) & (k < 10) & (o != 0) & (o != m + 1)), ("cap", live & (craw != 1) & (k >= 10)),
        ("dead_cube", live & (craw != 1) & (k < 10) & ((o == 0) | (o == m + 1)) & (x <= (1 << k))),
        ("invalid_byte", np.isin(s["cube"], (0x0F, 0x31, 0x4B))), ("nan", dsel & np.isnan(s["value"])),
        ("too_good", too_good), ("window", offer & window), ("free_double", offer & ~window),
        ("no_double", dsel & ~offer & ~too_good & ~np.isnan(s["value"])), ("take", take), ("pass", pas),
        ("last_game", retired), ("pass_by_start", pas & mine), ("pass_by_other", pas & ~mine),
        ("done_with_winner", fin), ("done_without_winner", dn & sel2 & (winner < 0)), ("done_unselected", dn & ~sel2),
        ("gammon_at_the_cube", fin & (score > 1) & (k2 > 0))) if hit.any()}
    return out, seen


# ------------------------------------------------------- positions of the traced runs --
def record(p1, p2, mover):
    r = np.zeros(64, np.uint8)
    for pt, v in p1.items():
        r[pt] = v
    for pt, v in p2.items():
        r[24 + pt] = v
    r[50], r[51] = 15 - r[:24].sum(), 15 - r[24:48].sum()
    r[R_CUR] = mover
    return r


# both sides have borne off most checkers: plain wins within a few plies
RACE = record({23: 2, 21: 1, 19: 1}, {0: 2, 2: 1, 4: 1}, 0)
# PLAYER2 still has all 15 checkers on the board, two of them outside its home board: PLAYER1, with
# five left, wins a gammon when it rolls a double in time
GAMMONISH = record({23: 2, 22: 2, 21: 1}, {6: 2, 5: 13}, 0)


# the scores of the forced runs: at both, one value is a double and a take at every cube with access
FORCED_SCORES = ((5, 6), (6, 7))


def forced_value(match, away, want, start_cubes=(0,)):
    """A value on which the rule's decision is `want` (1 take, 2 pass) at every state with access
    that a game at the score `away` = (a1, a2) can reach from the cubes `start_cubes`."""
    todo, states = list(start_cubes), set()
    while todo:
        c = todo.pop()
        for mover in (0, 1):
            x, y = away[mover], away[1 - mover]
            d = M.match_decision_reference(match.met, match.pc, match.length, x, y, 0, c, mover, 1, F(0), match.rule)
            if bool(d["access"]) and (c, mover) not in states:
                states.add((c, mover))
                todo.append(pack((c & 15) + 1, 2 - mover))
    for v in np.linspace(0.0, 1.0, 101):
        acts = []
        for c, mover in states:
            d = M.match_decision_reference(match.met, match.pc, match.length, away[mover], away[1 - mover], 0, c, mover, 1,
                                           F(v), match.rule)
            acts.append(2 if d["passed"] else 1 if d["offer"] else 0)
        if states and all(a == want for a in acts):
            return float(F(v)), max(c & 15 for c, _ in states)
    raise AssertionError(f"no value forces {want} at {away}")
