// Device helpers of the accounting kernels of the arena and of position rollouts: the per-wave
// integer sums, the group loop, a game's end, the cut skeleton.  Device-only: bg_engine.hip and
// part 2 of bg_bearoff.h, bg_bearoff1.h, bg_cube.h, bg_trunc.h, bg_cube_trunc.h and
// bg_bearoff_cube.h include it; part 1 of those headers and the host-only builds never see it.
#pragma once
#include "bg_engine.h"

namespace bg {

// The tally fields are integer sums, so the order of the additions does not matter: each
// wave counts its lanes with ballots and adds once per field (64-bit atomic add from lane 0).
__device__ __forceinline__ void tally_add(int64_t* tally, int field, long long v) {
    if (v != 0 && lane_id() == 0) atomicAdd((unsigned long long*)tally + field, (unsigned long long)v);
}
__device__ __forceinline__ long long count(bool p) { return (long long)__popcll(__ballot(p)); }
__device__ __forceinline__ long long wave_sum(long long v) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- position rollouts (DESIGN.md "Start positions and rollouts"; bgx/rollout.py drives it) ----
// Bookkeeping of rollouts on an engine whose start table holds the positions: lane i plays
// G games of position group[i] (one player acts for both sides), every game from the
// lane's start record again (the engine's auto-reset refills it in the step that ends the
// game).  State, plain arrays of the caller:
//   group int32[n]        position of the lane in [0, n_groups); anything else = idle lane
//   games_done int32[n]   finished, counted games of the lane (active while < G)
//   plies int32[n]        steps of the lane's current game
//   sel uint8[n]          the lane is active (lane selection of bgx_one_ply_sel / bgx_two_ply_sel)
//   tally int64[n_groups][8]  bgx_rollout_field; win = won by the start record's mover
//   active int64[1]       active lanes remaining
// PLIES is added at the game's end with the game, so the atomics are per finished game.
// Lanes of one group are usually neighbours: a wave adds once per (group, field) it holds
// finishers of.  Integer adds commute: the tallies are the same from run to run.
__device__ __forceinline__ int rollout_group(const int32_t* group, int i, int n_groups) {
    const int g = group[i];
    return g >= 0 && g < n_groups ? g : -1;
}

// The wave's lanes with p, one group at a time: add(gl, mine, m) once per group gl the wave
// holds such lanes of, with mine = this lane is one of them and m their ballot.  EVERY thread
// of the wave calls it, outside any divergent branch (no early return before it): the
// ballots and shuffles here, and those of count / wave_sum inside `add`, need the whole wave,
// and `rest` is wave-uniform, so the wave leaves the loop together.
template <class F>
__device__ __forceinline__ void for_each_group(bool p, int g, F add) {
    uint64_t rest = __ballot(p);
    while (rest) {
        const int lead = __ffsll((unsigned long long)rest) - 1;
        const int gl = __shfl(g, lead, 64);
        const bool mine = p && g == gl;
        const uint64_t m = __ballot(mine);
        add(gl, mine, m);
        rest &= ~m;
    }
}

// Lane i's current game ends and is counted: its plies so far go to *plies_before, the lane
// starts its next game at 0 plies; true when that was its last game (the lane leaves sel; the
// caller takes it off `active` with tally_add(active, 0, -count(retired))).
__device__ __forceinline__ bool end_game(int i, int G, int32_t* games_done, int32_t* plies, uint8_t* sel,
                                         long long* plies_before) {
    *plies_before = plies[i];
    plies[i] = 0;
    const int gd = games_done[i] + 1;
    games_done[i] = gd;
    const bool retired = gd >= G;
    if (retired) sel[i] = 0;
    return retired;
}

// ---- the cut skeleton of the kernels that end a game early (the table cuts k_bo_cut, k_b1_cut,
// k_boc_cut, the horizon cuts k_trunc_cut, k_cube_trunc_cut): cut_group, the kernel's own scoring
// of the lane with end_game, cut_finish ----
// Thread i's group when flag[i] (the table cuts' sel, the horizon cuts' tsel) marks a lane with a valid one, else -1.
__device__ __forceinline__ int cut_group(const uint8_t* flag, const int32_t* group, int i, int n, int n_groups) {
    const bool on = i < n && flag[i] != 0;
    return on ? rollout_group(group, i, n_groups) : -1;
}

// The tail: mask[i] = cut; per group of the wave's cut lanes GAMES += their number,
// PLIES += their `pl` (end_game's plies_before) and field 2 + k += their own[k], on a tally of
// 2 + N fields a row (every cut tally of include/bgx.h has GAMES = 0 and PLIES = 1; the
// kernels assert the places of their own fields); the retired lanes leave `active`.  EVERY
// thread of the wave calls it, outside any divergent branch: for_each_group's rule.
template <int N>
__device__ __forceinline__ void cut_finish(int i, int n, bool cut, bool retired, int g, long long pl,
                                           const long long (&own)[N], int64_t* tally, int64_t* active, uint8_t* mask) {
    static_assert(BGX_ROLLOUT_CUT_GAMES == 0 && BGX_ROLLOUT_TRUNC_GAMES == 0 && BGX_ROLLOUT_CUBE_CUT_GAMES == 0 &&
                  BGX_ROLLOUT_CUBE_TRUNC_GAMES == 0 && BGX_ROLLOUT_CUT_PLIES == 1 && BGX_ROLLOUT_TRUNC_PLIES == 1 &&
                  BGX_ROLLOUT_CUBE_CUT_PLIES == 1 && BGX_ROLLOUT_CUBE_TRUNC_PLIES == 1, "cut tallies: GAMES, PLIES");
    if (i < n) mask[i] = cut ? 1 : 0;
    for_each_group(cut, g, [&](int gl, bool mine, uint64_t m) {
        int64_t* row = tally + (size_t)gl * (2 + N);
        tally_add(row, 0, (long long)__popcll(m));
        tally_add(row, 1, wave_sum(mine ? pl : 0));
        #pragma unroll
        for (int k = 0; k < N; ++k) tally_add(row, 2 + k, wave_sum(mine ? own[k] : 0));
    });
    tally_add(active, 0, -count(retired));
}

// y^2 of a cubeful result as the two sums that cannot overflow int64: y^2 & (2^30 - 1), y^2 >> 30
__device__ __forceinline__ void square_split(long long y, long long* lo, long long* hi) {
    const long long y2 = y * y;
    *lo = y2 & ((1ll << 30) - 1);
    *hi = y2 >> 30;
}

// A table cut (k_bo_cut, k_b1_cut): a selected lane with a valid group whose record is in the
// table ends its game here: its start mover's win probability in 2^-20 fixed point goes to its
// group's row, the lane counts the game and is marked for the caller's masked reset.
// win(i, &cur, &w): the table's test on record i and, when it holds, the record's mover byte
// and the win probability of the side on roll.
template <class Win>
__device__ __forceinline__ void table_cut(const uint8_t* __restrict__ starts, const int32_t* __restrict__ group,
                                          int n_rec, int n_groups, int G, int32_t* games_done, int32_t* plies,
                                          uint8_t* sel, int64_t* cut_tally, int64_t* active, uint8_t* mask, Win win) {
    static_assert(BGX_ROLLOUT_CUT_P == 2 && BGX_ROLLOUT_CUT_P2 == 3, "cut_tally: P, P2 follow PLIES");
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = cut_group(sel, group, i, n_rec, n_groups);
    bool cut = false, retired = false;
    long long pq = 0, pl = 0;
    int cur;
    float w;
    if (g >= 0 && win(i, &cur, &w)) {
        cut = true;
        const float q = cur == (int)starts[(size_t)i * 64 + R_CUR] ? w : __fsub_rn(1.0f, w);
        pq = min(max(llrintf(__fmul_rn(q, 1048576.0f)), 0ll), 1048576ll);
        retired = end_game(i, G, games_done, plies, sel, &pl);
    }
    const long long own[2] = {pq, pq * pq};
    cut_finish(i, n_rec, cut, retired, g, pl, own, cut_tally, active, mask);
}

// a step's info word: the winner (-1 = none) and the game's points, 1..3
__device__ __forceinline__ void result_of(int info, int* winner, int* score) {
    *winner = ((info >> 8) & 0xFF) - 1;
    *score = min(max((info >> 16) & 0xFF, 1), 3);
}

// a game's fp32 luck sum in 2^-16 fixed point: round half even, clamped to +-2^21, 0 when not finite
__device__ __forceinline__ long long luck_q(float luck) {
    float x = luck * 65536.0f;
    x = isfinite(x) ? fminf(fmaxf(x, -2097152.0f), 2097152.0f) : 0.0f;
    return llrintf(x);
}

}  // namespace bg
