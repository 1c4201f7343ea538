// bg_match.h — match play in the head-to-head arena: matches to L points with the Crawford rule
// and cube decisions on a match equity table (include/bgx.h "match play in the
// arena"; bgx/match.py and bgx/arena.py drive it).  Included by bg_returns.hip only, after
// bg_arena_cube.h, for the reason bg_cube.h gives: kernels added to bg_engine.hip move its step
// kernels in the code object.
//
// Part 1 (plain C++, host and device) is the specification: the table lookup, the win probability
// of a value, the three match-winning chances of the side on roll, access, offer, answer and the
// end of a game.  Every fp32 product, sum and difference goes through ct_mul / ct_add / ct_sub of
// bg_cube_trunc.h, so each is rounded once and none is contracted; the one quotient is a single
// division.
// Part 2 (device): the six kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, count, wave_sum, result_of).  No LDS, no scratch.
// BGX_MATCH_PART1_ONLY (the host test program tools/match_host.cpp, any C++ compiler) takes part
// 1 alone, of this header and of the ones it includes.
#pragma once
#if defined(BGX_MATCH_PART1_ONLY)
#if !defined(BGX_CUBE_TRUNC_PART1_ONLY)
#define BGX_CUBE_TRUNC_PART1_ONLY
#endif
#if !defined(BGX_CUBE_PART1_ONLY)
#define BGX_CUBE_PART1_ONLY
#endif
#endif
#include "bg_cube_trunc.h"
#include "bg_arena_cube.h"

namespace bg {

constexpr int kMatchMaxLength = 25;

// The rule of one side (include/bgx.h bgx_match_rule, restated for the host program): scale turns
// the value's unit into points, window in [0, 1] places the doubling point between the dead-cube
// doubling point (0) and the cash point (1), win_gammons / loss_gammons in [0, 1] are the share of
// the owner's wins / losses that are gammons.  Backgammons are not modelled.
struct match_rule {
    float scale, window, win_gammons, loss_gammons;
};

// The tables: met float32[(L + 1)^2], met[i * (L + 1) + j] the chance that the side needing i wins
// the match against the side needing j at the start of a game (rows and columns at 1: the
// Crawford game); pc float32[L + 1], pc[j] the trailer's chance after the Crawford game when it
// needs j and the leader 1.  Row and column 0 are never read.
struct match_tables {
    const float* met;
    const float* pc;
    int L;
};

CUBE_HD int match_clamp(int i, int L) { return i < 1 ? 1 : i > L ? L : i; }

// The value of the next game to the side that then needs `me` against `opp`, with this game's
// points taken off already.  craw_now is this game's Crawford state: != 0 (the Crawford game or a
// later one) and the next game is post-Crawford; 0 and the table's row / column at 1 is the
// Crawford game itself.  Total: indices past L read L, so a hand-set state stays inside the tables.
CUBE_HD float met_after(const match_tables& t, int me, int opp, int craw_now) {
    if (me <= 0) return 1.0f;
    if (opp <= 0) return 0.0f;
    me = match_clamp(me, t.L);
    opp = match_clamp(opp, t.L);
    if (craw_now != 0) return me == 1 ? ct_sub(1.0f, t.pc[opp]) : t.pc[me];
    return t.met[me * (t.L + 1) + opp];
}

// The win probability of the side on roll from a value v of its position: c = scale * v clamped
// to [-(1 + gl), 1 + gw] by comparisons (a NaN stays a NaN), p = (c + 1 + gl) / (2 + gw + gl).
CUBE_HD float match_p(float scale, float v, float gw, float gl) {
    const float W = ct_add(1.0f, gw), L_ = ct_add(1.0f, gl);
    float c = ct_mul(scale, v);
    c = c < -L_ ? -L_ : c > W ? W : c;
    return ct_add(c, L_) / ct_add(W, L_);
}

// the match-winning chance of the side on roll (needs x, the other y) after winning / losing a
// game at stake n.  The loser's side is the opponent's own lookup, one minus it.
CUBE_HD float match_win(const match_tables& t, int x, int y, int craw, int n, float gw) {
    return ct_add(ct_mul(ct_sub(1.0f, gw), met_after(t, x - n, y, craw)), ct_mul(gw, met_after(t, x - 2 * n, y, craw)));
}
CUBE_HD float match_loss(const match_tables& t, int x, int y, int craw, int n, float gl) {
    return ct_add(ct_mul(ct_sub(1.0f, gl), ct_sub(1.0f, met_after(t, y - n, x, craw))),
                  ct_mul(gl, ct_sub(1.0f, met_after(t, y - 2 * n, x, craw))));
}

// values[0..2] = ND, DT, DP of the side on roll at win probability p with the cube at 2^k:
//   ND = loss(v) + p (win(v) - loss(v)), DT = loss(2v) + p (win(2v) - loss(2v)), DP = met_after(x - v, y)
CUBE_HD void match_values(const match_tables& t, int x, int y, int craw, int k, float p, float gw, float gl,
                          float values[3]) {
    const int v = 1 << k;
    const float w1 = match_win(t, x, y, craw, v, gw), l1 = match_loss(t, x, y, craw, v, gl);
    const float w2 = match_win(t, x, y, craw, 2 * v, gw), l2 = match_loss(t, x, y, craw, 2 * v, gl);
    values[0] = ct_add(l1, ct_mul(p, ct_sub(w1, l1)));
    values[1] = ct_add(l2, ct_mul(p, ct_sub(w2, l2)));
    values[2] = met_after(t, x - v, y, craw);
}

// The side on roll (record mover byte `mover`, needing x) may double: past the game's first ply,
// in a game that is not over on an active lane, not in the Crawford game, the cube below the cap
// and centred or its own, and x > 2^k (else the cube is dead: winning this game wins the match).
CUBE_HD bool match_access(uint8_t c, int mover, int plies, bool over, bool active, int craw, int x) {
    return plies > 0 && !over && active && craw != 1 && cube_access(c, kCubeMaxCap, mover) &&
           x > (1 << cube_k(c, kCubeMaxCap));
}

// With access: the side on roll doubles iff it is not too good (ND <= DP) and either the window
// is reached, DT - ND >= window (DP - ND), or the double is free (y <= v: losing this game loses
// the match at any cube) and gains, DT > ND.  A NaN compares false: never.
CUBE_HD bool match_offers(const match_tables& t, int x, int y, int craw, int k, const match_rule& r, float value) {
    const float p = match_p(r.scale, value, r.win_gammons, r.loss_gammons);
    float m[3];
    match_values(t, x, y, craw, k, p, r.win_gammons, r.loss_gammons, m);
    if (!(m[0] <= m[2])) return false;
    if (ct_sub(m[1], m[0]) >= ct_mul(r.window, ct_sub(m[2], m[0]))) return true;
    return y <= (1 << k) && m[1] > m[0];
}

// The other side answers by its own rule r on `value`, its own estimate of the doubler's value:
// the doubler's chances with the shares swapped (the doubler's wins are its losses).  It passes
// iff DT' > DP'; a tie or a NaN takes.
CUBE_HD bool match_passes(const match_tables& t, int x, int y, int craw, int k, const match_rule& r, float value) {
    const float p = match_p(r.scale, value, r.loss_gammons, r.win_gammons);
    float m[3];
    match_values(t, x, y, craw, k, p, r.loss_gammons, r.win_gammons, m);
    return m[1] > m[2];
}

// The end of a game worth `points` (s 2^k, or 2^k after a pass) to side w (0 A, 1 B) of a match to
// L: true when the match is over (away back to (L, L), craw to 0), else the Crawford state moves
// on: 0 -> 1 when the winner now needs 1, 1 -> 2.
CUBE_HD bool match_end_game(uint8_t away[2], uint8_t* craw, int L, int w, long long points) {
    const long long left = (long long)away[w] - points;
    if (left <= 0) {
        away[0] = away[1] = (uint8_t)L;
        *craw = 0;
        return true;
    }
    away[w] = (uint8_t)left;
    if (*craw == 0 && left == 1) *craw = 1;
    else if (*craw == 1) *craw = 2;
    return false;
}

CUBE_HD bool match_rule_ok(const match_rule& r) {
    return r.scale == r.scale && r.window >= 0.0f && r.window <= 1.0f && r.win_gammons >= 0.0f &&
           r.win_gammons <= 1.0f && r.loss_gammons >= 0.0f && r.loss_gammons <= 1.0f;
}

}  // namespace bg

#ifndef BGX_MATCH_PART1_ONLY
// ======================================================================== part 2 ==
// The lane's quota is matches, the arena kernels of bg_engine.hip count games: they are called
// with G = matches_per_lane (2 L - 1), which no lane reaches by playing (every game gives somebody
// a point), and a lane that finishes its last match is retired here by games_done = G, sel_a =
// sel_b = 0 and tally[BGX_ARENA_ACTIVE] -= 1: at once on a pass (respond), and after
// bgx_arena_advance has counted the game on a played-out one (flush leaves a flag, retire acts).

namespace {

using namespace bg;

__device__ __forceinline__ match_rule match_rule_of(const bgx_match_rule& r) {
    return match_rule{r.scale, r.window, r.win_gammons, r.loss_gammons};
}

__global__ __launch_bounds__(256) void k_arena_match_begin(int n, int L, uint8_t* away, uint8_t* craw, uint8_t* cube,
                                                           int32_t* plies, int32_t* matches_done, uint8_t* seat0,
                                                           uint8_t* retire, int64_t* match_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        away[2 * i] = away[2 * i + 1] = (uint8_t)L;
        craw[i] = 0;
        cube[i] = 0;
        plies[i] = 0;
        matches_done[i] = 0;
        seat0[i] = arena_a_p1(i, 0) ? 1 : 0;
        retire[i] = 0;
    }
    if (i < 16) match_tally[i] = 0;
}

// the lane's access with A (a_moves) or B on roll: x the side on roll's away
__device__ __forceinline__ bool lane_access(const uint8_t* recs, int i, bool a_moves, bool active, const int32_t* plies,
                                            const uint8_t* cube, const uint8_t* away, const uint8_t* craw) {
    const uint8_t* r = recs + (size_t)i * 64;
    return match_access(cube[i], r[R_CUR], plies[i], r[R_OVER] != 0, active, craw[i], away[2 * i + (a_moves ? 0 : 1)]);
}

__global__ __launch_bounds__(256) void k_arena_match_sel(const uint8_t* __restrict__ recs,
                                                         const uint8_t* __restrict__ sel_a,
                                                         const uint8_t* __restrict__ sel_b,
                                                         const int32_t* __restrict__ plies,
                                                         const uint8_t* __restrict__ cube,
                                                         const uint8_t* __restrict__ away,
                                                         const uint8_t* __restrict__ craw, int n, uint8_t* dsel_a,
                                                         uint8_t* dsel_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool sa = sel_a[i] != 0, sb = !sa && sel_b[i] != 0;
    const bool d = lane_access(recs, i, sa, sa || sb, plies, cube, away, craw);
    dsel_a[i] = d && sa ? 1 : 0;
    dsel_b[i] = d && sb ? 1 : 0;
}

// The offers: each side by its own rule on its own value.  Access is tested again, so a dsel of
// another origin cannot double in a Crawford game, past the cap or with a dead cube.
__global__ __launch_bounds__(256) void k_arena_match_offer(
    const uint8_t* __restrict__ recs, const uint8_t* __restrict__ sel_a, const uint8_t* __restrict__ sel_b,
    const uint8_t* __restrict__ dsel_a, const uint8_t* __restrict__ dsel_b, const float* __restrict__ eq_a,
    const float* __restrict__ eq_b, bgx_match_rule ra, bgx_match_rule rb, const float* __restrict__ met,
    const float* __restrict__ pc, int L, const int32_t* __restrict__ plies, const uint8_t* __restrict__ cube,
    const uint8_t* __restrict__ away, const uint8_t* __restrict__ craw, int n, uint8_t* off_a, uint8_t* off_b,
    int64_t* match_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool oa = false, ob = false;
    if (i < n) {
        const bool sa = sel_a[i] != 0, sb = !sa && sel_b[i] != 0;
        const bool da = sa && dsel_a[i] != 0, db = sb && dsel_b[i] != 0;
        if ((da || db) && lane_access(recs, i, sa, true, plies, cube, away, craw)) {
            const match_tables t{met, pc, L};
            const int x = away[2 * i + (sa ? 0 : 1)], y = away[2 * i + (sa ? 1 : 0)];
            const int k = cube_k(cube[i], kCubeMaxCap);
            const bool o = match_offers(t, x, y, craw[i], k, match_rule_of(sa ? ra : rb), sa ? eq_a[i] : eq_b[i]);
            oa = o && sa;
            ob = o && sb;
        }
        off_a[i] = oa ? 1 : 0;
        off_b[i] = ob ? 1 : 0;
    }
    // every thread of the wave reaches the ballots (no early return above)
    tally_add(match_tally, BGX_ARENA_MATCH_DOUBLES_A, count(oa));
    tally_add(match_tally, BGX_ARENA_MATCH_DOUBLES_B, count(ob));
}

// what the end of a game adds to the match tally, summed over the wave by match_count
struct match_game {
    bool fin = false, pass = false, pass_by_a = false, over = false, a_won = false, first = false, crawford = false,
         post = false;
    long long pts_a = 0, pts_b = 0, kk = 0, pl = 0;
};

// scores a game worth `points` to A (a_won) or B on lane i's match state; true: the lane's last
// match ended
__device__ __forceinline__ bool match_score(int i, int L, int M, bool a_won, long long points, int g_next,
                                            uint8_t* away, uint8_t* craw, int32_t* matches_done, uint8_t* seat0,
                                            match_game* mg) {
    uint8_t aw[2] = {away[2 * i], away[2 * i + 1]}, cr = craw[i];
    mg->fin = true;
    mg->a_won = a_won;
    mg->crawford = cr == 1;
    mg->post = cr == 2;
    (a_won ? mg->pts_a : mg->pts_b) = points;
    mg->over = match_end_game(aw, &cr, L, a_won ? 0 : 1, points);
    away[2 * i] = aw[0];
    away[2 * i + 1] = aw[1];
    craw[i] = cr;
    if (!mg->over) return false;
    mg->first = seat0[i] != 0;
    seat0[i] = arena_a_p1(i, g_next) ? 1 : 0;
    const int m = matches_done[i] + 1;
    matches_done[i] = m;
    return m >= M;
}

__device__ __forceinline__ void match_count(int64_t* mt, const match_game& g) {
    tally_add(mt, BGX_ARENA_MATCH_MATCHES, count(g.over));
    tally_add(mt, BGX_ARENA_MATCH_WINS_A, count(g.over && g.a_won));
    tally_add(mt, BGX_ARENA_MATCH_GAMES, count(g.fin));
    tally_add(mt, BGX_ARENA_MATCH_PASS_GAMES, count(g.pass));
    tally_add(mt, BGX_ARENA_MATCH_POINTS_A, wave_sum(g.pts_a));
    tally_add(mt, BGX_ARENA_MATCH_POINTS_B, wave_sum(g.pts_b));
    tally_add(mt, BGX_ARENA_MATCH_PASSES_A, count(g.pass && g.pass_by_a));
    tally_add(mt, BGX_ARENA_MATCH_PASSES_B, count(g.pass && !g.pass_by_a));
    tally_add(mt, BGX_ARENA_MATCH_LOG2, wave_sum(g.kk));
    tally_add(mt, BGX_ARENA_MATCH_CRAWFORD_GAMES, count(g.crawford));
    tally_add(mt, BGX_ARENA_MATCH_POST_CRAWFORD_GAMES, count(g.post));
    tally_add(mt, BGX_ARENA_MATCH_PASS_PLIES, wave_sum(g.pl));
    tally_add(mt, BGX_ARENA_MATCH_WINS_A_SEAT0, count(g.over && g.a_won && g.first));
    tally_add(mt, BGX_ARENA_MATCH_MATCHES_SEAT0, count(g.over && g.first));
}

// The answers: on an off_a lane B answers by B's rule on eq_b, on an off_b lane A by A's on eq_a.
// A take turns the cube; a pass gives the doubler 2^k points, ends the game, may end the match
// and the lane's quota, and masks the lane for the reset.  Active lanes with access only.  (Access
// asks x > 2^k, so today the doubler is still short of the match after a pass; the game's end is
// scored by the same match_score as flush's all the same, and a looser access rule stays correct.)
__global__ __launch_bounds__(256) void k_arena_match_respond(
    const uint8_t* __restrict__ recs, const uint8_t* __restrict__ off_a, const uint8_t* __restrict__ off_b,
    const float* __restrict__ eq_a, const float* __restrict__ eq_b, bgx_match_rule ra, bgx_match_rule rb,
    const float* __restrict__ met, const float* __restrict__ pc, int L, int n, int G, int M, uint8_t* cube,
    int32_t* plies, uint8_t* away, uint8_t* craw, int32_t* matches_done, uint8_t* seat0, int32_t* games_done,
    uint8_t* sel_a, uint8_t* sel_b, int64_t* tally, int64_t* match_tally, uint8_t* mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    match_game mg;
    bool retired = false;
    if (i < n) {
        const bool sa = sel_a[i] != 0, sb = !sa && sel_b[i] != 0;
        const bool oa = sa && off_a[i] != 0, ob = sb && off_b[i] != 0;
        const int g = games_done[i];
        if ((oa || ob) && g < G && lane_access(recs, i, sa, true, plies, cube, away, craw)) {
            const match_tables t{met, pc, L};
            const int x = away[2 * i + (sa ? 0 : 1)], y = away[2 * i + (sa ? 1 : 0)];
            const uint8_t c = cube[i];
            const int k = cube_k(c, kCubeMaxCap);
            // the doubler's value as the other side sees it, by the other side's rule
            mg.pass = match_passes(t, x, y, craw[i], k, match_rule_of(oa ? rb : ra), oa ? eq_b[i] : eq_a[i]);
            if (mg.pass) {
                mg.pass_by_a = ob;                          // B doubled: A gave up
                mg.kk = k;
                mg.pl = plies[i];
                plies[i] = 0;
                cube[i] = 0;
                retired = match_score(i, L, M, oa, 1ll << k, g + 1, away, craw, matches_done, seat0, &mg);
                games_done[i] = retired ? G : g + 1;
                sel_a[i] = 0;                               // until bgx_arena_cube_reseat
                sel_b[i] = 0;
            } else {
                cube[i] = cube_taken(c, kCubeMaxCap, recs[(size_t)i * 64 + R_CUR] & 1);
            }
        }
        mask[i] = mg.pass ? 1 : 0;
    }
    match_count(match_tally, mg);
    tally_add(tally, BGX_ARENA_ACTIVE, -count(retired));
}

// After the step, before bgx_arena_advance (games_done is still the finished game's g, sel_a /
// sel_b still the step's): a game that advance will count is scored at the cube's value on the
// match; the lane's last match leaves retire[i] = 1 for bgx_arena_match_retire.
__global__ __launch_bounds__(256) void k_arena_match_flush(const uint8_t* __restrict__ sel_a,
                                                           const uint8_t* __restrict__ sel_b,
                                                           const uint8_t* __restrict__ done,
                                                           const int32_t* __restrict__ info,
                                                           const int32_t* __restrict__ games_done, int n, int L, int M,
                                                           uint8_t* cube, int32_t* plies, uint8_t* away, uint8_t* craw,
                                                           int32_t* matches_done, uint8_t* seat0, uint8_t* retire,
                                                           int64_t* match_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && (sel_a[i] != 0 || sel_b[i] != 0);
    const bool dn = on && done[i] != 0;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    match_game mg;
    if (dn && winner >= 0) {
        const int g = games_done[i];
        mg.kk = cube_k(cube[i], kCubeMaxCap);
        const bool a_won = (winner == 0) == arena_a_p1(i, g);
        if (match_score(i, L, M, a_won, (long long)score << mg.kk, g + 1, away, craw, matches_done, seat0, &mg))
            retire[i] = 1;
    }
    if (dn) {
        cube[i] = 0;
        plies[i] = 0;
    } else if (on) {
        plies[i] += 1;
    }
    match_count(match_tally, mg);
}

// After bgx_arena_advance: a flagged lane has played its last match.
__global__ __launch_bounds__(256) void k_arena_match_retire(int n, int G, uint8_t* retire, int32_t* games_done,
                                                            uint8_t* sel_a, uint8_t* sel_b, int64_t* tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool r = false;
    if (i < n && retire[i] != 0) {
        retire[i] = 0;
        r = games_done[i] < G;
        games_done[i] = G;
        sel_a[i] = 0;
        sel_b[i] = 0;
    }
    tally_add(tally, BGX_ARENA_ACTIVE, -count(r));
}

bool match_rules_ok(const bgx_match_rule& a, const bgx_match_rule& b) {
    return match_rule_ok(match_rule{a.scale, a.window, a.win_gammons, a.loss_gammons}) &&
           match_rule_ok(match_rule{b.scale, b.window, b.win_gammons, b.loss_gammons});
}
bool match_length_ok(int L) { return L >= 1 && L <= kMatchMaxLength; }
// G = M (2 L - 1) as the caller must pass it: it fits int32 and M >= 0
bool match_quota_ok(int L, int G, int M) { return M >= 0 && (long long)M * (2 * L - 1) == (long long)G; }

}  // namespace

extern "C" {

int bgx_arena_match_begin(int32_t n, int32_t length, uint8_t* away_dev, uint8_t* craw_dev, uint8_t* cube_dev,
                          int32_t* plies_dev, int32_t* matches_done_dev, uint8_t* seat0_dev, uint8_t* retire_dev,
                          int64_t* match_tally_dev, void* stream) {
    if (n <= 0 || !match_length_ok(length) || !away_dev || !craw_dev || !cube_dev || !plies_dev ||
        !matches_done_dev || !seat0_dev || !retire_dev || !match_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_begin, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, length,
                       away_dev, craw_dev, cube_dev, plies_dev, matches_done_dev, seat0_dev, retire_dev,
                       match_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_match_sel(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                        const int32_t* plies_dev, const uint8_t* cube_dev, const uint8_t* away_dev,
                        const uint8_t* craw_dev, int32_t n, uint8_t* dsel_a_out, uint8_t* dsel_b_out, void* stream) {
    if (!records_dev || !sel_a_dev || !sel_b_dev || !plies_dev || !cube_dev || !away_dev || !craw_dev || n <= 0 ||
        !dsel_a_out || !dsel_b_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_sel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       sel_a_dev, sel_b_dev, plies_dev, cube_dev, away_dev, craw_dev, n, dsel_a_out, dsel_b_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_match_offer(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                          const uint8_t* dsel_a_dev, const uint8_t* dsel_b_dev, const float* eq_a_dev,
                          const float* eq_b_dev, bgx_match_rule rule_a, bgx_match_rule rule_b, const float* met_dev,
                          const float* pc_dev, int32_t length, const int32_t* plies_dev, const uint8_t* cube_dev,
                          const uint8_t* away_dev, const uint8_t* craw_dev, int32_t n, uint8_t* off_a_out,
                          uint8_t* off_b_out, int64_t* match_tally_dev, void* stream) {
    if (!records_dev || !sel_a_dev || !sel_b_dev || !dsel_a_dev || !dsel_b_dev || !eq_a_dev || !eq_b_dev ||
        !match_rules_ok(rule_a, rule_b) || !met_dev || !pc_dev || !match_length_ok(length) || !plies_dev ||
        !cube_dev || !away_dev || !craw_dev || n <= 0 || !off_a_out || !off_b_out || !match_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_offer, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       sel_a_dev, sel_b_dev, dsel_a_dev, dsel_b_dev, eq_a_dev, eq_b_dev, rule_a, rule_b, met_dev, pc_dev,
                       length, plies_dev, cube_dev, away_dev, craw_dev, n, off_a_out, off_b_out, match_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_match_respond(const uint8_t* records_dev, const uint8_t* off_a_dev, const uint8_t* off_b_dev,
                            const float* eq_a_dev, const float* eq_b_dev, bgx_match_rule rule_a, bgx_match_rule rule_b,
                            const float* met_dev, const float* pc_dev, int32_t length, int32_t n,
                            int32_t games_per_lane, int32_t matches_per_lane, uint8_t* cube_dev, int32_t* plies_dev,
                            uint8_t* away_dev, uint8_t* craw_dev, int32_t* matches_done_dev, uint8_t* seat0_dev,
                            int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev,
                            int64_t* match_tally_dev, uint8_t* reset_mask_out, void* stream) {
    if (!records_dev || !off_a_dev || !off_b_dev || !eq_a_dev || !eq_b_dev || !match_rules_ok(rule_a, rule_b) ||
        !met_dev || !pc_dev || !match_length_ok(length) || n <= 0 ||
        !match_quota_ok(length, games_per_lane, matches_per_lane) || !cube_dev || !plies_dev || !away_dev ||
        !craw_dev || !matches_done_dev || !seat0_dev || !games_done_dev || !sel_a_dev || !sel_b_dev || !tally_dev ||
        !match_tally_dev || !reset_mask_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_respond, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       off_a_dev, off_b_dev, eq_a_dev, eq_b_dev, rule_a, rule_b, met_dev, pc_dev, length, n,
                       games_per_lane, matches_per_lane, cube_dev, plies_dev, away_dev, craw_dev, matches_done_dev,
                       seat0_dev, games_done_dev, sel_a_dev, sel_b_dev, tally_dev, match_tally_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_match_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                          const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t length,
                          int32_t matches_per_lane, uint8_t* cube_dev, int32_t* plies_dev, uint8_t* away_dev,
                          uint8_t* craw_dev, int32_t* matches_done_dev, uint8_t* seat0_dev, uint8_t* retire_dev,
                          int64_t* match_tally_dev, void* stream) {
    if (!sel_a_dev || !sel_b_dev || !done_dev || !info_dev || !games_done_dev || n <= 0 || !match_length_ok(length) ||
        matches_per_lane < 0 || !cube_dev || !plies_dev || !away_dev || !craw_dev || !matches_done_dev || !seat0_dev ||
        !retire_dev || !match_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sel_a_dev,
                       sel_b_dev, done_dev, info_dev, games_done_dev, n, length, matches_per_lane, cube_dev, plies_dev,
                       away_dev, craw_dev, matches_done_dev, seat0_dev, retire_dev, match_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_match_retire(int32_t n, int32_t games_per_lane, uint8_t* retire_dev, int32_t* games_done_dev,
                           uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev, void* stream) {
    if (n <= 0 || games_per_lane < 0 || !retire_dev || !games_done_dev || !sel_a_dev || !sel_b_dev || !tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_match_retire, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n,
                       games_per_lane, retire_dev, games_done_dev, sel_a_dev, sel_b_dev, tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
