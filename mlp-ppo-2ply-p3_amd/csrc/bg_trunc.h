// bg_trunc.h — truncated position rollouts: a game that reaches its horizon stops there and is
// scored by a value (include/bgx.h "truncated rollouts"; bgx/rollout.py drives
// it).  Included by bg_returns.hip only, after bg_cube.h, for bg_cube.h's reasons.
//
// Part 1 (plain C++, host and device): the one function that turns a value into the game's
// fixed-point result.
// Part 2 (device): the two kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, count, and the cut skeleton: cut_group, end_game, cut_finish).  No LDS, no
// scratch.  BGX_TRUNC_PART1_ONLY (the host test program tools/trunc_host.cpp, any C++ compiler)
// takes part 1 alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(BGX_TRUNC_PART1_ONLY)
#define TRUNC_HD __host__ __device__ __forceinline__
#else
#define TRUNC_HD inline
#endif

namespace bg {

constexpr long long kTruncOne = 65536;          // Vq = rint(y * kTruncOne)
constexpr float kTruncClamp = 3.0f;             // a game is worth at most 3 points

// The result of a game truncated with `v` the value of the side on roll there, from the start
// mover's side in 2^-16 points: e = scale * v (one fp32 product, rounded once: nothing follows
// it that could fuse), 0 for a NaN, clamped to +-3 (an infinity too); negated when the side on
// roll is not the start record's mover (`same` false); rounded half to even.  |Vq| <= 196608.
TRUNC_HD long long trunc_value_q(float scale, float v, bool same) {
    float e = scale * v;
    e = e != e ? 0.0f : fminf(fmaxf(e, -kTruncClamp), kTruncClamp);
    const float y = same ? e : -e;
    return llrintf(y * 65536.0f);
}

}  // namespace bg

#ifndef BGX_TRUNC_PART1_ONLY
// ======================================================================== part 2 ==
#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

namespace {

using namespace bg;

// tsel: the lanes whose game stops at the horizon now (the value's lane selection).  After
// bgx_rollout_advance: a game that ended in this step has plies 0 and a fresh record.
__global__ __launch_bounds__(256) void k_trunc_sel(const uint8_t* __restrict__ recs, const int32_t* __restrict__ group,
                                                   int n, int n_groups, int horizon,
                                                   const int32_t* __restrict__ plies, const uint8_t* __restrict__ sel,
                                                   uint8_t* tsel, int64_t* cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool t = i < n && sel[i] != 0 && rollout_group(group, i, n_groups) >= 0 &&
                   recs[(size_t)i * 64 + R_OVER] == 0 && plies[i] >= horizon;
    if (i < n) tsel[i] = t ? 1 : 0;
    // every thread of the wave reaches the ballot
    const long long c = count(t);
    if (cnt) tally_add(cnt, 0, c);
}

// The truncation on the tsel lanes: the game is counted at its value (end_game) together with
// the luck it gathered, and the lane is masked for the reset.
__global__ __launch_bounds__(256) void k_trunc_cut(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                   const int32_t* __restrict__ group,
                                                   const uint8_t* __restrict__ tsel, const float* __restrict__ value,
                                                   float scale, int n, int n_groups, int G, int32_t* games_done,
                                                   int32_t* plies, uint8_t* sel, float* lane_luck, int64_t* trunc_tally,
                                                   int64_t* active, uint8_t* mask) {
    static_assert(BGX_ROLLOUT_TRUNC_V == 2 && BGX_ROLLOUT_TRUNC_V2 == 3 && BGX_ROLLOUT_TRUNC_LUCK == 4 &&
                  BGX_ROLLOUT_TRUNC_LUCK2 == 5 && BGX_ROLLOUT_TRUNC_VLUCK == 6, "trunc_tally: `own` in field order");
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = cut_group(tsel, group, i, n, n_groups);
    const bool cut = g >= 0;
    bool retired = false;
    long long vq = 0, lq = 0, pl = 0;
    if (cut) {
        const bool same = recs[(size_t)i * 64 + R_CUR] == starts[(size_t)i * 64 + R_CUR];
        vq = trunc_value_q(scale, value[i], same);
        if (lane_luck) {
            lq = luck_q(lane_luck[i]);                             // bgx_rollout_luck_flush's Lq
            lane_luck[i] = 0.0f;
        }
        retired = end_game(i, G, games_done, plies, sel, &pl);
    }
    const long long own[5] = {vq, vq * vq, lq, lq * lq, vq * lq};
    cut_finish(i, n, cut, retired, g, pl, own, trunc_tally, active, mask);
}

}  // namespace

extern "C" {

int bgx_rollout_trunc_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n, int32_t n_groups,
                          int32_t horizon, const int32_t* plies_dev, const uint8_t* sel_dev, uint8_t* tsel_out,
                          int64_t* count_inout_or_null, void* stream) {
    if (!records_dev || !group_dev || n <= 0 || n_groups <= 0 || horizon < 1 || !plies_dev || !sel_dev || !tsel_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_trunc_sel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, group_dev, n,
                       n_groups, horizon, plies_dev, sel_dev, tsel_out, count_inout_or_null);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_trunc_cut(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                          const uint8_t* tsel_dev, const float* value_dev, float scale, int32_t n,
                          int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev,
                          uint8_t* sel_dev, float* lane_luck_or_null, int64_t* trunc_tally_dev,
                          int64_t* active_dev, uint8_t* reset_mask_out, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !tsel_dev || !value_dev || scale != scale || n <= 0 ||
        n_groups <= 0 || games_per_lane < 0 || !games_done_dev || !plies_dev || !sel_dev || !trunc_tally_dev ||
        !active_dev || !reset_mask_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_trunc_cut, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, starts_dev,
                       group_dev, tsel_dev, value_dev, scale, n, n_groups, games_per_lane, games_done_dev, plies_dev,
                       sel_dev, lane_luck_or_null, trunc_tally_dev, active_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
