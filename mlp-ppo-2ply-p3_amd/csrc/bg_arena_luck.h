// bg_arena_luck.h — luck-adjusted arena results (include/bgx.h "luck of the arena";
// bgx/arena.py drives it): the cubeless luck of a roll from the 21 per-roll values of
// bgx_roll_values, against the mid-game distribution of the 21 rolls or, on a game's first ply,
// against the opening roll's (the engine's standard reset draws it with doubles rejected: 15 rolls
// at 1/15 each), and its bookkeeping per game beside the arena's own (bg_engine.hip).  Included by
// bg_returns.hip only, after bg_cube_luck.h, whose part 1 it builds on.
//
// Part 1 (plain C++, host and device): arena_roll_luck, the FMA chain of the mean under either
// distribution and the luck.  It adds no arithmetic of its own: the roll's index and the mid-game
// weights are bg_cube_luck.h's (cube_luck_roll, cube_luck_p), the difference is bg_cube_trunc.h's
// ct_sub.
// Part 2 (device): the three kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, wave_sum, count, square_split, luck_q).  No LDS, no scratch.
// BGX_ARENA_LUCK_PART1_ONLY (the host test program tools/arena_luck_host.cpp, any C++ compiler,
// -ffp-contract=off) takes part 1 alone.
//
// Ranges of the tally: Lq = luck_q(L), |Lq| <= 2^21 (32 points), so Lq^2 <= 2^42 goes through
// square_split and LUCK2_LO grows by less than 2^30 a game; |res| <= 3, so |res Lq| < 2^23: the
// tally holds 2^33 games at the clamp before a sum could pass 2^63.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(BGX_ARENA_LUCK_PART1_ONLY) && !defined(BGX_CUBE_LUCK_PART1_ONLY)
#define BGX_CUBE_LUCK_PART1_ONLY
#endif
#include "bg_cube_luck.h"

namespace bg {

// roll r of the 21 is a double (cube_luck_p's list)
CUBE_HD bool arena_luck_double(int r) { return r == 0 || r == 6 || r == 11 || r == 15 || r == 18 || r == 20; }

// The luck of the roll (d0, d1) given the mover's value v_r after each of the 21 rolls.
// opening == 0: mean = fma(p_20, v_20, ... fma(p_0, v_0, 0)), p_r = cube_luck_p(r): bgx_roll_luck's
// chain bit for bit.  opening != 0: mean = fma(1/15, v_r, mean) over the 15 non-doubles, r
// ascending; the doubles are skipped, so their values are never read into the chain.
// luck = v of the roll - mean; 0 when the bytes hold no roll, and 0 for a double at an opening
// (it cannot have been drawn).
CUBE_HD float arena_roll_luck(const float v[21], int d0, int d1, int opening, float* mean_out) {
    const int mine = cube_luck_roll(d0, d1);
    float mean = 0.0f, vmine = 0.0f;
    for (int r = 0; r < 21; ++r) {
        if (opening != 0 && arena_luck_double(r)) continue;
        const float x = v[r];
        mean = fmaf(opening != 0 ? 1.0f / 15.0f : cube_luck_p(r), x, mean);
        if (r == mine) vmine = x;
    }
    *mean_out = mean;
    return mine >= 0 && !(opening != 0 && arena_luck_double(mine)) ? ct_sub(vmine, mean) : 0.0f;
}

}  // namespace bg

#ifndef BGX_ARENA_LUCK_PART1_ONLY
// ======================================================================== part 2 ==
#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

namespace {

using namespace bg;

// every lane starts its first game: no luck yet, the record holds an opening roll; the tally is 0
__global__ __launch_bounds__(256) void k_arena_luck_begin(int n, float* lane_luck, uint8_t* fresh, int64_t* luck_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 8) luck_tally[i] = 0;
    if (i >= n) return;
    lane_luck[i] = 0.0f;
    fresh[i] = 1;
}

// Before the players act: the luck of the roll each lane on move holds joins the lane's sum, A's view.
__global__ __launch_bounds__(256) void k_arena_luck_add(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ sel_a,
                                                        const uint8_t* __restrict__ sel_b,
                                                        const float* __restrict__ values21, int n, float* lane_luck,
                                                        uint8_t* fresh, float* luck_out, float* mean_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool a = sel_a[i] != 0;
    const uint8_t* r = recs + (size_t)i * 64;
    if ((!a && sel_b[i] == 0) || r[R_OVER] != 0) return;
    float mean;                                      // the 21 values are read where the chain uses them: no array
    const float l = arena_roll_luck(values21 + (size_t)i * 21, r[R_ROLL0], r[R_ROLL1], fresh[i], &mean);
    lane_luck[i] += a ? l : -l;
    fresh[i] = 0;
    if (luck_out) luck_out[i] = l;
    if (mean_out) mean_out[i] = mean;
}

// After the step, before k_arena_advance (games_done and the selections are still the step's): a
// game that advance will count books A's result against its luck; any done of an active lane
// zeroes the lane's sum, and the record now holds the next game's opening roll.
__global__ __launch_bounds__(256) void k_arena_luck_flush(const uint8_t* __restrict__ sel_a, const uint8_t* __restrict__ sel_b,
                                                          const uint8_t* __restrict__ done,
                                                          const int32_t* __restrict__ info,
                                                          const int32_t* __restrict__ games_done, int n, int G,
                                                          float* lane_luck, uint8_t* fresh, int64_t* luck_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int g = in ? games_done[i] : G;
    const bool active = in && g < G && (sel_a[i] != 0 || sel_b[i] != 0);
    const bool dn = active && done[i] != 0;
    const int inf = dn ? info[i] : 0;
    const int winner = ((inf >> 8) & 0xFF) - 1, score = (inf >> 16) & 0xFF;
    const bool fin = dn && winner >= 0;
    long long res = 0, lq = 0, lo = 0, hi = 0;
    if (fin) {
        const bool a_p1 = ((i + g) & 1) == 0;
        const long long pts = score >= 1 && score <= 3 ? score : 0;          // k_arena_advance's POINTS
        res = (winner == 0) == a_p1 ? pts : -pts;
        lq = luck_q(lane_luck[i]);
        square_split(lq, &lo, &hi);
    }
    if (dn) {
        lane_luck[i] = 0.0f;
        fresh[i] = 1;
    }
    // every thread of the wave reaches the ballot (no early return above); a wave without a
    // finished game, the common case, leaves together before the shuffles
    if (__ballot(fin) == 0) return;
    tally_add(luck_tally, BGX_ARENA_LUCK, wave_sum(lq));
    tally_add(luck_tally, BGX_ARENA_LUCK2_LO, wave_sum(lo));
    tally_add(luck_tally, BGX_ARENA_LUCK2_HI, wave_sum(hi));
    tally_add(luck_tally, BGX_ARENA_RESLUCK, wave_sum(res * lq));
    tally_add(luck_tally, BGX_ARENA_LUCK_GAMES, count(fin));
}

}  // namespace

extern "C" {

int bgx_arena_luck_begin(int32_t n, float* lane_luck_dev, uint8_t* fresh_dev, int64_t* luck_tally_dev, void* stream) {
    if (n <= 0 || !lane_luck_dev || !fresh_dev || !luck_tally_dev) return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_luck_begin, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, lane_luck_dev,
                       fresh_dev, luck_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_luck_add(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                       const float* values21_dev, int32_t n, float* lane_luck_dev, uint8_t* fresh_dev,
                       float* luck_out_or_null, float* mean_out_or_null, void* stream) {
    if (!records_dev || !sel_a_dev || !sel_b_dev || !values21_dev || n <= 0 || !lane_luck_dev || !fresh_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_luck_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, sel_a_dev,
                       sel_b_dev, values21_dev, n, lane_luck_dev, fresh_dev, luck_out_or_null, mean_out_or_null);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_luck_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                         const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t games_per_lane,
                         float* lane_luck_dev, uint8_t* fresh_dev, int64_t* luck_tally_dev, void* stream) {
    if (!sel_a_dev || !sel_b_dev || !done_dev || !info_dev || !games_done_dev || n <= 0 || games_per_lane < 0 ||
        !lane_luck_dev || !fresh_dev || !luck_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_luck_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sel_a_dev, sel_b_dev,
                       done_dev, info_dev, games_done_dev, n, games_per_lane, lane_luck_dev, fresh_dev, luck_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
