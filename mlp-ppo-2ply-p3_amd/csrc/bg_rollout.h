// Device helpers of the accounting kernels of the arena and of position rollouts: the per-wave
// integer sums, the group loop, a game's end.  Device-only: bg_engine.hip and part 2 of
// bg_bearoff.h, bg_bearoff1.h, bg_cube.h, bg_trunc.h and bg_bearoff_cube.h include it; part 1 of
// those headers and the host-only builds never see it.
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
