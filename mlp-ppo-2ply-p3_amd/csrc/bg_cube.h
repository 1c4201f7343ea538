// bg_cube.h — the doubling cube of position rollouts, money play (include/bgx.h
// "doubling cube"; bgx/cube.py and bgx/rollout.py drive it).  Included by bg_returns.hip only,
// after bg_bearoff1.h: kernels added to bg_engine.hip move its step kernels in the code object
//  and the library keeps one code object per HIP source.
//
// Part 1 (plain C++, host and device): the state byte's pack and unpack and the whole decision
// rule in one function.  A state byte holds k in bits 0-3 (the cube shows 2^k) and the owner in
// bits 4-5 (0 centred, 1 PLAYER1 = mover byte 0, 2 PLAYER2).  So that every kernel is defined on
// any byte, k reads as min(k, cap) and owner 3 as 0.
// Part 2 (device): the four kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, count, wave_sum, for_each_group, end_game).  No LDS, no
// scratch.  BGX_CUBE_PART1_ONLY (the host test program tools/cube_host.cpp, any C++ compiler)
// takes part 1 alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) && !defined(BGX_CUBE_PART1_ONLY)
#define CUBE_HD __host__ __device__ __forceinline__
#else
#define CUBE_HD inline
#endif

namespace bg {

constexpr int kCubeMaxCap = 10;
enum CubeAction { kCubeNone = 0, kCubeTake = 1, kCubePass = 2 };
// the flags of bgx_bearoff_cube_lookup and bgx_cube_janowski (bg_bearoff_cube.h, bg_cube_trunc.h)
enum BocFlag { kBocMayDouble = 1, kBocDoubles = 2, kBocTakes = 4, kBocIsDead = 8 };

CUBE_HD int cube_k(uint8_t c, int cap) {
    const int k = c & 15;
    return k < cap ? k : cap;
}
CUBE_HD int cube_owner(uint8_t c) {
    const int o = (c >> 4) & 3;
    return o == 3 ? 0 : o;
}
CUBE_HD uint8_t cube_pack(int k, int owner) { return (uint8_t)(k | (owner << 4)); }
CUBE_HD uint8_t cube_sanitise(uint8_t c, int cap) { return cube_pack(cube_k(c, cap), cube_owner(c)); }
// the mover (record byte 52: 0 or 1) may double: below the cap, and the cube centred or its own
CUBE_HD bool cube_access(uint8_t c, int cap, int mover) {
    const int o = cube_owner(c);
    return cube_k(c, cap) < cap && (o == 0 || o == (mover & 1) + 1);
}

// The decision of the side on roll, `mover`, before it rolls, with `equity` its own equity there
// and e = scale * equity (one fp32 product, rounded once: nothing follows it that could fuse).
// Without access: kCubeNone.  The mover doubles iff double_at <= e <= too_good_at (a NaN
// compares false: it never doubles); the opponent passes iff e > pass_at, else it takes and
// *next = k + 1 owned by the other side.  *next is the byte as it stood (sanitised) otherwise;
// after a pass the caller puts the game's starting cube back.
CUBE_HD int cube_decision(uint8_t c, int cap, int mover, float scale, float equity, float double_at, float pass_at,
                          float too_good_at, uint8_t* next) {
    *next = cube_sanitise(c, cap);
    if (!cube_access(c, cap, mover)) return kCubeNone;
    const float e = scale * equity;
    if (!(e >= double_at && e <= too_good_at)) return kCubeNone;
    if (e > pass_at) return kCubePass;
    *next = cube_pack(cube_k(c, cap) + 1, 2 - (mover & 1));
    return kCubeTake;
}

}  // namespace bg

#ifndef BGX_CUBE_PART1_ONLY
// ======================================================================== part 2 ==
#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

namespace {

using namespace bg;

__global__ __launch_bounds__(256) void k_cube_begin(const uint8_t* __restrict__ cube0, int n, int cap, uint8_t* cube) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cube[i] = cube_sanitise(cube0[i], cap);
}

// dsel: the lanes on which the side on roll may double now (bgx_roll_luck's lane selection).
// Never on a game's first ply (plies == 0).
__global__ __launch_bounds__(256) void k_cube_sel(const uint8_t* __restrict__ recs, const int32_t* __restrict__ group,
                                                  int n_groups, const int32_t* __restrict__ plies,
                                                  const uint8_t* __restrict__ sel, const uint8_t* __restrict__ cube, int n,
                                                  int cap, uint8_t* dsel) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool d = sel[i] != 0 && rollout_group(group, i, n_groups) >= 0 && plies[i] > 0;
    if (d) {
        const uint8_t* r = recs + (size_t)i * 64;
        d = r[R_OVER] == 0 && cube_access(cube[i], cap, r[R_CUR]);
    }
    dsel[i] = d ? 1 : 0;
}

// The decision on the dsel lanes: a pass ends the game at the cube's value (end_game: the game
// is counted; the lane is masked for the reset), a take turns the cube.
__global__ __launch_bounds__(256) void k_cube_decide(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                     const int32_t* __restrict__ group,
                                                     const uint8_t* __restrict__ dsel, const float* __restrict__ equity,
                                                     int n, int n_groups, int G, bgx_cube_rule rule,
                                                     const uint8_t* __restrict__ cube0, uint8_t* cube,
                                                     int32_t* games_done, int32_t* plies, uint8_t* sel,
                                                     int64_t* cube_tally, int64_t* active, uint8_t* mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && dsel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    bool dbl = false, pass = false, retired = false;
    long long y = 0, kk = 0, pl = 0;
    if (g >= 0) {
        const int m = recs[(size_t)i * 64 + R_CUR] & 1;
        const uint8_t c = cube[i];
        uint8_t next;
        const int act = cube_decision(c, rule.cap, m, rule.scale, equity[i], rule.double_at, rule.pass_at,
                                      rule.too_good_at, &next);
        dbl = act != kCubeNone;
        pass = act == kCubePass;
        if (pass) {
            kk = cube_k(c, rule.cap);
            y = m == (int)(starts[(size_t)i * 64 + R_CUR] & 1) ? (1ll << kk) : -(1ll << kk);
            retired = end_game(i, G, games_done, plies, sel, &pl);
            cube[i] = cube_sanitise(cube0[i], rule.cap);
        } else if (dbl) {
            cube[i] = next;
        }
    }
    if (i < n) mask[i] = pass ? 1 : 0;
    for_each_group(dbl, g, [&](int gl, bool mine, uint64_t md) {
        const bool pm = mine && pass;
        const long long np = count(pm), v = pm ? y : 0;
        int64_t* row = cube_tally + (size_t)gl * 8;
        tally_add(row, BGX_ROLLOUT_CUBE_GAMES, np);
        tally_add(row, BGX_ROLLOUT_CUBE_POINTS, wave_sum(v));
        tally_add(row, BGX_ROLLOUT_CUBE_POINTS2, wave_sum(v * v));
        tally_add(row, BGX_ROLLOUT_CUBE_LOG2, wave_sum(pm ? kk : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_PASS_GAMES, np);
        tally_add(row, BGX_ROLLOUT_CUBE_PASS_PLIES, wave_sum(pm ? pl : 0));
        tally_add(row, BGX_ROLLOUT_CUBE_PASS_WON, count(pm && y > 0));
        tally_add(row, BGX_ROLLOUT_CUBE_DOUBLES, (long long)__popcll(md));
    });
    tally_add(active, 0, -count(retired));
}

// After the step, before bgx_rollout_advance (sel is still the step's selection): a game that
// advance will count is scored at the cube's value; any done of a selected lane puts the lane's
// starting cube back.
__global__ __launch_bounds__(256) void k_cube_flush(const uint8_t* __restrict__ starts, const int32_t* __restrict__ group,
                                                    const uint8_t* __restrict__ sel, const uint8_t* __restrict__ done,
                                                    const int32_t* __restrict__ info, int n, int n_groups,
                                                    bgx_cube_rule rule, const uint8_t* __restrict__ cube0, uint8_t* cube,
                                                    int64_t* cube_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && sel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    const bool dn = on && done[i] != 0;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    const bool fin = dn && g >= 0 && winner >= 0;
    long long y = 0, kk = 0;
    if (fin) {
        kk = cube_k(cube[i], rule.cap);
        const long long s = rule.jacoby && kk == 0 ? 1 : score;
        y = winner == (int)(starts[(size_t)i * 64 + R_CUR] & 1) ? (s << kk) : -(s << kk);
    }
    if (dn) cube[i] = cube_sanitise(cube0[i], rule.cap);
    for_each_group(fin, g, [&](int gl, bool mine, uint64_t m) {
        const long long v = mine ? y : 0;
        int64_t* row = cube_tally + (size_t)gl * 8;
        tally_add(row, BGX_ROLLOUT_CUBE_GAMES, (long long)__popcll(m));
        tally_add(row, BGX_ROLLOUT_CUBE_POINTS, wave_sum(v));
        tally_add(row, BGX_ROLLOUT_CUBE_POINTS2, wave_sum(v * v));
        tally_add(row, BGX_ROLLOUT_CUBE_LOG2, wave_sum(mine ? kk : 0));
    });
}

bool cube_rule_ok(const bgx_cube_rule& r) {
    return r.scale == r.scale && r.double_at == r.double_at && r.pass_at == r.pass_at && r.cap >= 0 &&
           r.cap <= kCubeMaxCap;
}

}  // namespace

extern "C" {

int bgx_rollout_cube_begin(const uint8_t* cube0_dev, int32_t n, int32_t cap, uint8_t* cube_dev, void* stream) {
    if (!cube0_dev || !cube_dev || n <= 0 || cap < 0 || cap > kCubeMaxCap) return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_begin, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, cube0_dev, n, cap,
                       cube_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n_groups,
                         const int32_t* plies_dev, const uint8_t* sel_dev, const uint8_t* cube_dev, int32_t n,
                         int32_t cap, uint8_t* dsel_out, void* stream) {
    if (!records_dev || !group_dev || n_groups <= 0 || !plies_dev || !sel_dev || !cube_dev || n <= 0 || cap < 0 ||
        cap > kCubeMaxCap || !dsel_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_sel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, group_dev,
                       n_groups, plies_dev, sel_dev, cube_dev, n, cap, dsel_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_decide(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                            const uint8_t* dsel_dev, const float* equity_dev, int32_t n, int32_t n_groups,
                            int32_t games_per_lane, bgx_cube_rule rule, const uint8_t* cube0_dev, uint8_t* cube_dev,
                            int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cube_tally_dev,
                            int64_t* active_dev, uint8_t* reset_mask_out, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !dsel_dev || !equity_dev || n <= 0 || n_groups <= 0 ||
        games_per_lane < 0 || !cube_rule_ok(rule) || !cube0_dev || !cube_dev || !games_done_dev || !plies_dev ||
        !sel_dev || !cube_tally_dev || !active_dev || !reset_mask_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_decide, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, starts_dev,
                       group_dev, dsel_dev, equity_dev, n, n_groups, games_per_lane, rule, cube0_dev, cube_dev,
                       games_done_dev, plies_dev, sel_dev, cube_tally_dev, active_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                           const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                           bgx_cube_rule rule, const uint8_t* cube0_dev, uint8_t* cube_dev, int64_t* cube_tally_dev,
                           void* stream) {
    if (!starts_dev || !group_dev || !sel_dev || !done_dev || !info_dev || n <= 0 || n_groups <= 0 ||
        !cube_rule_ok(rule) || !cube0_dev || !cube_dev || !cube_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_cube_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts_dev, group_dev,
                       sel_dev, done_dev, info_dev, n, n_groups, rule, cube0_dev, cube_dev, cube_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
