// bg_cube_luck.h — luck-adjusted cubeful rollouts (include/bgx.h "luck of cubeful
// rollouts"; bgx/cube.py and bgx/rollout.py drive it): the luck of a roll with a cube on the
// position, from the 21 per-roll values of bgx_roll_values and Janowski's cube-life equity
// (bg_cube_trunc.h's cube_trunc_values, called with the opponent as the side on roll), and its
// bookkeeping per game beside bg_cube.h's.  Included by bg_returns.hip only, after
// bg_cube_trunc.h, for bg_cube.h's reasons.
//
// Part 1 (plain C++, host and device): the roll's index, the cubeful value g_r of one roll, the
// FMA chain of the mean and the luck, and a game's luck in fixed point.
// Part 2 (device): the four kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, wave_sum, for_each_group, square_split, result_of).  No LDS,
// no scratch.  BGX_CUBE_LUCK_PART1_ONLY (the host test program tools/cube_luck_host.cpp, any C++
// compiler, -ffp-contract=off) takes part 1 alone.
//
// Ranges of the tally: Lq = rint(L 2^16) clamped to +-2^31 (|L| <= 32768 points: the cube's 2^10
// times the cubeless clamp of 32), so Lq^2 <= 2^62 goes through square_split; |y| <= 3 * 2^10,
// so |y Lq| < 2^43: a row holds 2^20 games at the clamp before YLUCK could pass 2^63.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(BGX_CUBE_LUCK_PART1_ONLY) && !defined(BGX_CUBE_TRUNC_PART1_ONLY)
#define BGX_CUBE_TRUNC_PART1_ONLY
#endif
#include "bg_cube_trunc.h"

namespace bg {

constexpr float kClOne = 65536.0f;               // 2^16: the luck's fixed point, luck_q's
constexpr float kClClamp = 2147483648.0f;        // 2^31 = 32768 points

// the index of the roll (d0, d1) among the 21 rolls in kRoll0 / kRoll1 order; -1: no roll
CUBE_HD int cube_luck_roll(int d0, int d1) {
    const int lo = d0 < d1 ? d0 : d1, hi = d0 < d1 ? d1 : d0;
    return lo >= 1 && hi <= 6 ? 7 * (lo - 1) - (lo - 1) * lo / 2 + hi - lo : -1;
}
// p_r: 1/36 for the doubles (rolls 0, 6, 11, 15, 18, 20), else 2/36 (k_luck_reduce's constants)
CUBE_HD float cube_luck_p(int r) {
    return r == 0 || r == 6 || r == 11 || r == 15 || r == 18 || r == 20 ? 1.0f / 36.0f : 2.0f / 36.0f;
}

// g_r: after `mover` has played a roll to a position it values v (its own view, cubeless), its
// opponent is on roll with the same cube c, before its own cube decision: minus the opponent's e.
CUBE_HD float cube_luck_g(uint8_t c, int cap, int mover, float scale, float v, float x, float W, float L, int jacoby) {
    float values[4];
    cube_trunc_values(c, cap, 1 - (mover & 1), scale, -v, x, W, L, jacoby, values);
    return -values[2];
}

// mean = fma(p_20, g_20, ... fma(p_0, g_0, 0)), luck = g of the roll (d0, d1) - mean (0: no roll)
CUBE_HD float cube_roll_luck(const float v[21], uint8_t c, int cap, int mover, int d0, int d1, float scale, float x,
                             float W, float L, int jacoby, float* mean_out) {
    const int mine = cube_luck_roll(d0, d1);
    float mean = 0.0f, gmine = 0.0f;
    for (int r = 0; r < 21; ++r) {
        const float g = cube_luck_g(c, cap, mover, scale, v[r], x, W, L, jacoby);
        mean = fmaf(cube_luck_p(r), g, mean);
        if (r == mine) gmine = g;
    }
    *mean_out = mean;
    return mine >= 0 ? ct_sub(gmine, mean) : 0.0f;
}

// a game's fp32 luck sum in points as Lq: round half even, clamped to +-2^31, 0 when not finite
CUBE_HD long long cube_luck_q(float luck) {
    const float y = ct_mul(luck, kClOne);
    if (!(y == y) || y == INFINITY || y == -INFINITY) return 0;
    return (long long)llrintf(y > kClClamp ? kClClamp : y < -kClClamp ? -kClClamp : y);
}

}  // namespace bg

#ifndef BGX_CUBE_LUCK_PART1_ONLY
// ======================================================================== part 2 ==
#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

namespace {

using namespace bg;

// The cubeful luck of the roll each selected lane record holds, when it is not game_over.
__global__ __launch_bounds__(256) void k_cube_roll_luck(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ cube,
                                                        const float* __restrict__ values21, int n, float scale,
                                                        bgx_cube_life life, int cap, int jacoby,
                                                        const uint8_t* __restrict__ sel, float* luck, float* mean_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = recs + (size_t)i * 64;
    if ((sel != nullptr && sel[i] == 0) || r[R_OVER] != 0) return;
    float mean;                                      // the 21 values are read where the chain uses them: no array
    const float l = cube_roll_luck(values21 + (size_t)i * 21, cube ? cube[i] : (uint8_t)0, cap, r[R_CUR], r[R_ROLL0],
                                   r[R_ROLL1], scale, life.cube_life, life.win_value, life.loss_value, jacoby, &mean);
    luck[i] = l;
    if (mean_out) mean_out[i] = mean;
}

// k_rollout_luck_add with the roll's luck in units of the lane's cube (after the step's decision)
__global__ __launch_bounds__(256) void k_cube_luck_add(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                       const int32_t* __restrict__ plies, const uint8_t* __restrict__ sel,
                                                       const uint8_t* __restrict__ cube, const float* __restrict__ luck,
                                                       int n, int cap, float* lane_luck) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !sel[i]) return;
    if (plies[i] == 0 && starts[(size_t)i * 64 + R_ROLL0] != 0) return;
    const float l = ldexpf(luck[i], cube_k(cube[i], cap));
    lane_luck[i] += recs[(size_t)i * 64 + R_CUR] == starts[(size_t)i * 64 + R_CUR] ? l : -l;
}

// per group of the wave's `fin` lanes: the game's luck lq against its result y
__device__ __forceinline__ void cube_luck_book(bool fin, int g, long long lq, long long y, int64_t* tally) {
    long long lo, hi;
    square_split(lq, &lo, &hi);
    for_each_group(fin, g, [&](int gl, bool mine, uint64_t m) {
        int64_t* row = tally + (size_t)gl * 5;
        tally_add(row, BGX_ROLLOUT_CUBE_LUCK, wave_sum(mine ? lq : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_LUCK2_LO, wave_sum(mine ? lo : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_LUCK2_HI, wave_sum(mine ? hi : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_YLUCK, wave_sum(mine ? y * lq : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_LUCK_GAMES, (long long)__popcll(m));
    });
}

// Before k_cube_decide, with its inputs: where it will find a pass, the game's luck is booked
// against the pass's result and the lane's sum zeroed.
__global__ __launch_bounds__(256) void k_cube_luck_pass(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                        const int32_t* __restrict__ group,
                                                        const uint8_t* __restrict__ dsel, const float* __restrict__ equity,
                                                        int n, int n_groups, bgx_cube_rule rule,
                                                        const uint8_t* __restrict__ cube, float* lane_luck,
                                                        int64_t* tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && dsel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    bool pass = false;
    long long y = 0, lq = 0;
    if (g >= 0) {
        const int m = recs[(size_t)i * 64 + R_CUR] & 1;
        const uint8_t c = cube[i];
        uint8_t next;
        pass = cube_decision(c, rule.cap, m, rule.scale, equity[i], rule.double_at, rule.pass_at, rule.too_good_at,
                             &next) == kCubePass;
        if (pass) {
            const int kk = cube_k(c, rule.cap);
            y = m == (int)(starts[(size_t)i * 64 + R_CUR] & 1) ? (1ll << kk) : -(1ll << kk);
            lq = cube_luck_q(lane_luck[i]);
            lane_luck[i] = 0.0f;
        }
    }
    cube_luck_book(pass, g, lq, y, tally);
}

// After the step, before k_cube_flush (the cube is still the finished game's): k_cube_flush's
// result of a counted game against its luck; any done of a selected lane zeroes the lane's sum.
__global__ __launch_bounds__(256) void k_cube_luck_flush(const uint8_t* __restrict__ starts, const int32_t* __restrict__ group,
                                                         const uint8_t* __restrict__ sel, const uint8_t* __restrict__ done,
                                                         const int32_t* __restrict__ info, int n, int n_groups, int cap,
                                                         int jacoby, const uint8_t* __restrict__ cube, float* lane_luck,
                                                         int64_t* tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && sel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    const bool dn = on && done[i] != 0;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    const bool fin = dn && g >= 0 && winner >= 0;
    long long y = 0, lq = 0;
    if (fin) {
        const long long kk = cube_k(cube[i], cap);
        const long long s = jacoby && kk == 0 ? 1 : score;
        y = winner == (int)(starts[(size_t)i * 64 + R_CUR] & 1) ? (s << kk) : -(s << kk);
        lq = cube_luck_q(lane_luck[i]);
    }
    if (dn) lane_luck[i] = 0.0f;
    cube_luck_book(fin, g, lq, y, tally);
}

}  // namespace

extern "C" {

int bgx_cube_roll_luck(const uint8_t* records_dev, const uint8_t* cube_dev_or_null, const float* values21_dev, int32_t n,
                       float scale, bgx_cube_life life, int32_t cap, int32_t jacoby, const uint8_t* sel_or_null,
                       float* luck_out, float* mean_out_or_null, void* stream) {
    if (!records_dev || !values21_dev || !luck_out || n <= 0 || scale != scale || !cube_life_struct_ok(life) ||
        cap < 0 || cap > kCubeMaxCap)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_roll_luck, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       cube_dev_or_null, values21_dev, n, scale, life, cap, jacoby, sel_or_null, luck_out,
                       mean_out_or_null);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_luck_add(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* plies_dev,
                              const uint8_t* sel_dev, const uint8_t* cube_dev, const float* luck_dev, int32_t n,
                              int32_t cap, float* lane_luck_dev, void* stream) {
    if (!records_dev || !starts_dev || !plies_dev || !sel_dev || !cube_dev || !luck_dev || n <= 0 || cap < 0 ||
        cap > kCubeMaxCap || !lane_luck_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_luck_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       starts_dev, plies_dev, sel_dev, cube_dev, luck_dev, n, cap, lane_luck_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_luck_pass(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                               const uint8_t* dsel_dev, const float* equity_dev, int32_t n, int32_t n_groups,
                               bgx_cube_rule rule, const uint8_t* cube_dev, float* lane_luck_dev,
                               int64_t* cube_luck_tally_dev, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !dsel_dev || !equity_dev || n <= 0 || n_groups <= 0 ||
        !cube_rule_ok(rule) || !cube_dev || !lane_luck_dev || !cube_luck_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_luck_pass, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       starts_dev, group_dev, dsel_dev, equity_dev, n, n_groups, rule, cube_dev, lane_luck_dev,
                       cube_luck_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_luck_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                                const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                                int32_t cap, int32_t jacoby, const uint8_t* cube_dev, float* lane_luck_dev,
                                int64_t* cube_luck_tally_dev, void* stream) {
    if (!starts_dev || !group_dev || !sel_dev || !done_dev || !info_dev || n <= 0 || n_groups <= 0 || cap < 0 ||
        cap > kCubeMaxCap || !cube_dev || !lane_luck_dev || !cube_luck_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_luck_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts_dev,
                       group_dev, sel_dev, done_dev, info_dev, n, n_groups, cap, jacoby, cube_dev, lane_luck_dev,
                       cube_luck_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
