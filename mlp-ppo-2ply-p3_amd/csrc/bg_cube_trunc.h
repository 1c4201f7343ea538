// bg_cube_trunc.h — truncated cubeful rollouts and the static cube evaluator (DESIGN.md §17;
// include/bgx.h "truncated cubeful rollouts"; bgx/cube.py and bgx/rollout.py drive it): the value
// of a position with a cube on it from one cubeless value, by Janowski's interpolation between
// the dead-cube and the live-cube equity.  Included by bg_returns.hip only, after bg_trunc.h,
// for bg_cube.h's reasons.
//
// Part 1 (plain C++, host and device): the whole rule in one function -- the four values and the
// flags of bgx_bearoff_cube_lookup from (cube byte, mover, value) -- and the fixed-point result
// of a game cut there.  Every fp32 operation is rounded once: the products and sums go through
// ct_mul / ct_add / ct_sub, which carry no contraction flag (bg_returns.hip's mul_rn / add_rn /
// sub_rn for host and device); a compiler without the pragma takes -ffp-contract=off.
// Part 2 (device): the two kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's cut skeleton (cut_group, end_game, square_split, cut_finish).  No LDS, no
// scratch.  BGX_CUBE_TRUNC_PART1_ONLY (the host test program tools/cube_trunc_host.cpp, any C++
// compiler) takes part 1 alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(BGX_CUBE_TRUNC_PART1_ONLY) && !defined(BGX_CUBE_PART1_ONLY)
#define BGX_CUBE_PART1_ONLY
#endif
#include "bg_cube.h"

namespace bg {

constexpr float kCtOne = 65536.0f;               // 2^16: the cut's fixed point, bg_trunc.h's
constexpr float kCtClamp = 196608.0f;            // 3 points

CUBE_HD float ct_mul(float a, float b) {
#if defined(__clang__)
    #pragma clang fp contract(off)
#endif
    return a * b;
}
CUBE_HD float ct_add(float a, float b) {
#if defined(__clang__)
    #pragma clang fp contract(off)
#endif
    return a + b;
}
CUBE_HD float ct_sub(float a, float b) {
#if defined(__clang__)
    #pragma clang fp contract(off)
#endif
    return a - b;
}

// the line through (p0, y0) and (p1, y1) at p
CUBE_HD float ct_seg(float p, float p0, float y0, float p1, float y1) {
    return ct_add(y0, ct_mul(ct_sub(p, p0), ct_sub(y1, y0) / ct_sub(p1, p0)));
}

// The live-cube equity at win probability p with W / L the points of a won / lost game:
// live[0..2] for the cube centred, owned by the side on roll, owned by its opponent.
CUBE_HD void ct_live(float p, float W, float L, float live[3]) {
    const float D = ct_add(ct_add(W, L), 0.5f);
    const float TP = ct_sub(L, 0.5f) / D, CP = ct_add(L, 1.0f) / D;      // take point, cash point
    const float lo = ct_seg(p, 0.0f, -L, TP, -1.0f), hi = ct_seg(p, CP, 1.0f, 1.0f, W);
    live[0] = p < TP ? lo : p < CP ? ct_seg(p, TP, -1.0f, CP, 1.0f) : hi;
    live[1] = p < CP ? ct_seg(p, 0.0f, -L, CP, 1.0f) : hi;
    live[2] = p < TP ? lo : ct_seg(p, TP, -1.0f, 1.0f, W);
}

// E = (1 - x) dead + x live
CUBE_HD float ct_mix(float x, float dead, float live) {
    return ct_add(ct_mul(ct_sub(1.0f, x), dead), ct_mul(x, live));
}

// The rule.  The side on roll, `mover` (record byte 52), holds the cube byte c (read as every
// cube kernel reads it) and v is its cubeless value; x = the cube life in [0, 1], W / L = the
// mean points of a won / lost game in [1, 3].  values: nd, DT, e, the cubeless equity, in units
// of the current cube; returns the flags.
CUBE_HD uint8_t cube_trunc_values(uint8_t c, int cap, int mover, float scale, float v, float x, float W, float L,
                                  int jacoby, float values[4]) {
    float cl = ct_mul(scale, v);
    cl = cl != cl ? 0.0f : fminf(fmaxf(cl, -L), W);
    const float p = ct_add(cl, L) / ct_add(W, L);
    const int k = cube_k(c, cap), o = cube_owner(c);
    const bool dead = k >= cap, access = !dead && (o == 0 || o == (mover & 1) + 1);
    float live[3];
    ct_live(p, W, L, live);
    float nd = cl;
    if (!dead) {
        if (o == 0 && jacoby) {                      // no gammons while the cube is centred
            float l1[3];
            ct_live(p, 1.0f, 1.0f, l1);
            nd = ct_mix(x, ct_sub(ct_mul(2.0f, p), 1.0f), l1[0]);
        } else {
            nd = ct_mix(x, cl, live[o == 0 ? 0 : access ? 1 : 2]);
        }
    }
    const float dt = ct_mul(2.0f, k + 1 >= cap ? cl : ct_mix(x, cl, live[2]));
    const float cash = dt < 1.0f ? dt : 1.0f;
    const bool doubles = access && cash > nd;        // strict: a tie is no double
    values[0] = nd;
    values[1] = dt;
    values[2] = doubles ? cash : nd;
    values[3] = cl;
    return (uint8_t)((access ? kBocMayDouble : 0) | (doubles ? kBocDoubles : 0) | (dt <= 1.0f ? kBocTakes : 0) |
                     (dead ? kBocIsDead : 0));
}

// A cut game's result in 2^-16 units of one point: e = the equity of the record's mover in units
// of the cube 2^k, signed for the start mover.  Qq = rint(q 2^16) clamped to +-3 * 2^16 (0 for a
// NaN), Yq = Qq 2^k.
CUBE_HD long long cube_trunc_q(float e, bool start_mover_on_roll, int k) {
    float y = ct_mul(start_mover_on_roll ? e : -e, kCtOne);
    if (!(y == y)) return 0;
    y = y > kCtClamp ? kCtClamp : y < -kCtClamp ? -kCtClamp : y;
    return (long long)llrintf(y) * (1ll << k);
}

// cube life, W and L in their ranges (a NaN fails every comparison)
CUBE_HD bool cube_life_ok(float x, float W, float L) {
    return x >= 0.0f && x <= 1.0f && W >= 1.0f && W <= 3.0f && L >= 1.0f && L <= 3.0f;
}

}  // namespace bg

#ifndef BGX_CUBE_TRUNC_PART1_ONLY
// ======================================================================== part 2 ==
#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

namespace {

using namespace bg;

// The static cube evaluator: the rule on every selected lane record that is not game_over.
__global__ __launch_bounds__(256) void k_cube_janowski(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ cube,
                                                       const float* __restrict__ value, int n, float scale,
                                                       bgx_cube_life life, int cap, int jacoby,
                                                       const uint8_t* __restrict__ sel, float* values, uint8_t* flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = recs + (size_t)i * 64;
    uint8_t fl = 0;
    if ((sel == nullptr || sel[i] != 0) && r[R_OVER] == 0) {
        float v[4];
        fl = cube_trunc_values(cube ? cube[i] : (uint8_t)0, cap, r[R_CUR], scale, value[i], life.cube_life,
                               life.win_value, life.loss_value, jacoby, v);
        if (values) ((float4*)values)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (flags) flags[i] = fl;
}

// The truncation of a cubeful game on the tsel lanes (bg_rollout.h's cut skeleton with the rule's e,
// scaled by the lane's cube, as the game's result; k_boc_cut's six sums in bg_trunc.h's unit).
__global__ __launch_bounds__(256) void k_cube_trunc_cut(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                        const int32_t* __restrict__ group,
                                                        const uint8_t* __restrict__ tsel, const float* __restrict__ value,
                                                        float scale, bgx_cube_life life, int n, int n_groups, int G,
                                                        int32_t* games_done, int32_t* plies, uint8_t* sel,
                                                        int64_t* tally, int64_t* active, uint8_t* mask, int cap, int jacoby,
                                                        const uint8_t* __restrict__ cube0, uint8_t* cube) {
    static_assert(BGX_ROLLOUT_CUBE_TRUNC_Y == 2 && BGX_ROLLOUT_CUBE_TRUNC_Y2_LO == 3 &&
                  BGX_ROLLOUT_CUBE_TRUNC_Y2_HI == 4 && BGX_ROLLOUT_CUBE_TRUNC_LOG2 == 5, "cube_trunc_tally: `own`");
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = cut_group(tsel, group, i, n, n_groups);
    const bool cut = g >= 0;
    bool retired = false;
    long long yq = 0, pl = 0, kk = 0;
    if (cut) {
        const int m = recs[(size_t)i * 64 + R_CUR];
        const uint8_t c = cube[i];
        float v[4];
        cube_trunc_values(c, cap, m, scale, value[i], life.cube_life, life.win_value, life.loss_value, jacoby, v);
        kk = cube_k(c, cap);
        yq = cube_trunc_q(v[2], m == (int)starts[(size_t)i * 64 + R_CUR], (int)kk);
        retired = end_game(i, G, games_done, plies, sel, &pl);
        cube[i] = cube_sanitise(cube0[i], cap);
    }
    long long own[4] = {yq, 0, 0, kk};
    square_split(yq, &own[1], &own[2]);
    cut_finish(i, n, cut, retired, g, pl, own, tally, active, mask);
}

bool cube_life_struct_ok(const bgx_cube_life& l) { return cube_life_ok(l.cube_life, l.win_value, l.loss_value); }

}  // namespace

extern "C" {

int bgx_cube_janowski(const uint8_t* records_dev, const uint8_t* cube_dev_or_null, const float* value_dev, int32_t n,
                      float scale, bgx_cube_life life, int32_t cap, int32_t jacoby, const uint8_t* sel_or_null,
                      float* values_out, uint8_t* flags_out, void* stream) {
    if (!records_dev || !value_dev || n <= 0 || scale != scale || !cube_life_struct_ok(life) || cap < 0 ||
        cap > kCubeMaxCap || ((uintptr_t)values_out & 15))
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_janowski, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       cube_dev_or_null, value_dev, n, scale, life, cap, jacoby, sel_or_null, values_out, flags_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_trunc_cut(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                               const uint8_t* tsel_dev, const float* value_dev, float scale, bgx_cube_life life,
                               int32_t n, int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev,
                               int32_t* plies_dev, uint8_t* sel_dev, int64_t* cube_trunc_tally_dev, int64_t* active_dev,
                               uint8_t* reset_mask_out, int32_t cap, int32_t jacoby, const uint8_t* cube0_dev,
                               uint8_t* cube_dev, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !tsel_dev || !value_dev || scale != scale ||
        !cube_life_struct_ok(life) || n <= 0 || n_groups <= 0 || games_per_lane < 0 || !games_done_dev || !plies_dev ||
        !sel_dev || !cube_trunc_tally_dev || !active_dev || !reset_mask_out || cap < 0 || cap > kCubeMaxCap ||
        !cube0_dev || !cube_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_trunc_cut, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       starts_dev, group_dev, tsel_dev, value_dev, scale, life, n, n_groups, games_per_lane,
                       games_done_dev, plies_dev, sel_dev, cube_trunc_tally_dev, active_dev, reset_mask_out, cap, jacoby,
                       cube0_dev, cube_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
