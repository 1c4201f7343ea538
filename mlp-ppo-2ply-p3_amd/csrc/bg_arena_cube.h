// bg_arena_cube.h — the doubling cube of the head-to-head arena, money play (DESIGN.md §16;
// include/bgx.h "doubling cube in the arena"; bgx/arena.py drives it).  Included by
// bg_returns.hip only, after bg_cube.h, for the reason bg_cube.h gives: kernels added to
// bg_engine.hip move its step kernels in the code object.
//
// Part 1 (plain C++, host and device): cube_decision of bg_cube.h in its two halves, so that a
// different party can take each.  In a rollout one rule and one value decide for both sides; in
// the arena the side on roll offers by its own rule on its own equity and the other side answers
// by its own rule on its own estimate of the doubler's equity.
// Part 2 (device): the five kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (tally_add, count, wave_sum, result_of).  No LDS, no scratch.
// BGX_CUBE_PART1_ONLY (the host test program tools/arena_cube_host.cpp, any C++ compiler) takes
// part 1 alone, of this header and of bg_cube.h.
#pragma once
#include "bg_cube.h"

namespace bg {

// The side on roll, `mover`, offers a double: it has access to the cube and, with e = scale *
// equity (one fp32 product), double_at <= e <= too_good_at.  A NaN compares false: never.
CUBE_HD bool cube_offers(uint8_t c, int cap, int mover, float scale, float equity, float double_at,
                         float too_good_at) {
    if (!cube_access(c, cap, mover)) return false;
    const float e = scale * equity;
    return e >= double_at && e <= too_good_at;
}

// The side that was offered the double gives up: `equity` is the doubler's equity, the mover's
// view, as the responder estimates it.  A NaN compares false: it takes.
CUBE_HD bool cube_passes(float scale, float equity, float pass_at) { return scale * equity > pass_at; }

// the cube after a take: k + 1, owned by the side that is not on roll
CUBE_HD uint8_t cube_taken(uint8_t c, int cap, int mover) { return cube_pack(cube_k(c, cap) + 1, 2 - (mover & 1)); }

}  // namespace bg

#ifndef BGX_CUBE_PART1_ONLY
// ======================================================================== part 2 ==

namespace {

using namespace bg;

// the seat rule, restated from bg_engine.hip's select_lane: in game g of lane i, A is PLAYER1
// (mover byte 0) iff ((i + g) & 1) == 0
__device__ __forceinline__ bool arena_a_p1(int i, int g) { return ((i + g) & 1) == 0; }

__global__ __launch_bounds__(256) void k_arena_cube_begin(int n, uint8_t* cube, int32_t* plies, int64_t* cube_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        cube[i] = 0;
        plies[i] = 0;
    }
    if (i < 16) cube_tally[i] = 0;
}

// dsel_a / dsel_b: the lanes on which A / B is on roll and may double now.  Never on a game's
// first ply (plies == 0).
__global__ __launch_bounds__(256) void k_arena_cube_sel(const uint8_t* __restrict__ recs,
                                                        const uint8_t* __restrict__ sel_a,
                                                        const uint8_t* __restrict__ sel_b,
                                                        const int32_t* __restrict__ plies,
                                                        const uint8_t* __restrict__ cube, int n, int cap,
                                                        uint8_t* dsel_a, uint8_t* dsel_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = recs + (size_t)i * 64;
    const bool d = plies[i] > 0 && r[R_OVER] == 0 && cube_access(cube[i], cap, r[R_CUR]);
    dsel_a[i] = d && sel_a[i] != 0 ? 1 : 0;
    dsel_b[i] = d && sel_b[i] != 0 ? 1 : 0;
}

// The offers: each side by its own rule on its own equity.  Access is tested again inside
// cube_offers, so a dsel of another origin cannot take the cube past the cap.
__global__ __launch_bounds__(256) void k_arena_cube_offer(const uint8_t* __restrict__ recs,
                                                          const uint8_t* __restrict__ dsel_a,
                                                          const uint8_t* __restrict__ dsel_b,
                                                          const float* __restrict__ eq_a,
                                                          const float* __restrict__ eq_b, bgx_cube_rule ra,
                                                          bgx_cube_rule rb, const uint8_t* __restrict__ cube, int n,
                                                          uint8_t* off_a, uint8_t* off_b, int64_t* cube_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool oa = false, ob = false;
    if (i < n) {
        const int m = recs[(size_t)i * 64 + R_CUR] & 1;
        const uint8_t c = cube[i];
        oa = dsel_a[i] != 0 && cube_offers(c, ra.cap, m, ra.scale, eq_a[i], ra.double_at, ra.too_good_at);
        ob = dsel_b[i] != 0 && cube_offers(c, rb.cap, m, rb.scale, eq_b[i], rb.double_at, rb.too_good_at);
        off_a[i] = oa ? 1 : 0;
        off_b[i] = ob ? 1 : 0;
    }
    // every thread of the wave reaches the ballots (no early return above)
    tally_add(cube_tally, BGX_ARENA_CUBE_DOUBLES_A, count(oa));
    tally_add(cube_tally, BGX_ARENA_CUBE_DOUBLES_B, count(ob));
}

// The answers: on an off_a lane B answers by B's rule on eq_b, on an off_b lane (off_a first,
// should a foreign pair name both) A answers by A's on eq_a.  A take turns the cube; a pass ends
// the game at the cube's value and masks the lane for the reset.  The lane must be active and
// the cube open to the side on roll (tested once more: off arrays of another origin can neither
// pass the cap nor count a game of a lane that has played its G).
__global__ __launch_bounds__(256) void k_arena_cube_respond(const uint8_t* __restrict__ recs,
                                                            const uint8_t* __restrict__ off_a,
                                                            const uint8_t* __restrict__ off_b,
                                                            const float* __restrict__ eq_a,
                                                            const float* __restrict__ eq_b, bgx_cube_rule ra,
                                                            bgx_cube_rule rb, int n, int G, uint8_t* cube,
                                                            int32_t* plies, int32_t* games_done, uint8_t* sel_a,
                                                            uint8_t* sel_b, int64_t* tally, int64_t* cube_tally,
                                                            uint8_t* mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool pass = false, by_a = false, retired = false;
    long long y = 0, kk = 0, pl = 0;
    if (i < n) {
        const bool oa = off_a[i] != 0, ob = !oa && off_b[i] != 0;
        const int m = recs[(size_t)i * 64 + R_CUR] & 1;
        const uint8_t c = cube[i];
        const int g = games_done[i];
        if ((oa || ob) && g < G && cube_access(c, ra.cap, m)) {
            // the doubler's equity as the other side sees it
            pass = oa ? cube_passes(rb.scale, eq_b[i], rb.pass_at) : cube_passes(ra.scale, eq_a[i], ra.pass_at);
            if (pass) {
                by_a = ob;                                  // B doubled: A gave up
                kk = cube_k(c, ra.cap);
                y = oa ? (1ll << kk) : -(1ll << kk);
                pl = plies[i];
                plies[i] = 0;
                cube[i] = 0;
                games_done[i] = g + 1;
                retired = g + 1 >= G;
                sel_a[i] = 0;                               // until bgx_arena_cube_reseat
                sel_b[i] = 0;
            } else {
                cube[i] = cube_taken(c, ra.cap, m);
            }
        }
        mask[i] = pass ? 1 : 0;
    }
    const long long np = count(pass);
    tally_add(cube_tally, BGX_ARENA_CUBE_GAMES, np);
    tally_add(cube_tally, BGX_ARENA_CUBE_POINTS_A, wave_sum(y));
    tally_add(cube_tally, BGX_ARENA_CUBE_POINTS2, wave_sum(y * y));
    tally_add(cube_tally, BGX_ARENA_CUBE_WINS_A, count(pass && y > 0));
    tally_add(cube_tally, BGX_ARENA_CUBE_LOG2, wave_sum(kk));
    tally_add(cube_tally, BGX_ARENA_CUBE_PASS_GAMES, np);
    tally_add(cube_tally, BGX_ARENA_CUBE_PASS_PLIES, wave_sum(pl));
    tally_add(cube_tally, BGX_ARENA_CUBE_PASSES_A, count(pass && by_a));
    tally_add(cube_tally, BGX_ARENA_CUBE_PASSES_B, count(pass && !by_a));
    tally_add(tally, BGX_ARENA_ACTIVE, -count(retired));
}

// After the masked bgx_reset: a masked lane that has games left is seated for the first
// position of its next game, by the new record's mover and the new g.
__global__ __launch_bounds__(256) void k_arena_cube_reseat(const uint8_t* __restrict__ recs,
                                                           const uint8_t* __restrict__ mask, int n, int G,
                                                           const int32_t* __restrict__ games_done, uint8_t* sel_a,
                                                           uint8_t* sel_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || mask[i] == 0) return;
    const int g = games_done[i];
    if (g >= G) return;
    const bool a_moves = ((recs[(size_t)i * 64 + R_CUR] & 1) == 0) == arena_a_p1(i, g);
    sel_a[i] = a_moves ? 1 : 0;
    sel_b[i] = a_moves ? 0 : 1;
}

// After the step, before bgx_arena_advance (games_done is still the finished game's g, sel_a /
// sel_b still the step's): a game that advance will count is scored at the cube's value.
__global__ __launch_bounds__(256) void k_arena_cube_flush(const uint8_t* __restrict__ sel_a,
                                                          const uint8_t* __restrict__ sel_b,
                                                          const uint8_t* __restrict__ done,
                                                          const int32_t* __restrict__ info,
                                                          const int32_t* __restrict__ games_done, int n, int jacoby,
                                                          int cap, uint8_t* cube, int32_t* plies, int64_t* cube_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && (sel_a[i] != 0 || sel_b[i] != 0);
    const bool dn = on && done[i] != 0;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    const bool fin = dn && winner >= 0;
    long long y = 0, kk = 0;
    if (fin) {
        kk = cube_k(cube[i], cap);
        const long long s = jacoby && kk == 0 ? 1 : score;
        y = (winner == 0) == arena_a_p1(i, games_done[i]) ? (s << kk) : -(s << kk);
    }
    if (dn) {
        cube[i] = 0;
        plies[i] = 0;
    } else if (on) {
        plies[i] += 1;
    }
    tally_add(cube_tally, BGX_ARENA_CUBE_GAMES, count(fin));
    tally_add(cube_tally, BGX_ARENA_CUBE_POINTS_A, wave_sum(y));
    tally_add(cube_tally, BGX_ARENA_CUBE_POINTS2, wave_sum(y * y));
    tally_add(cube_tally, BGX_ARENA_CUBE_WINS_A, count(fin && y > 0));
    tally_add(cube_tally, BGX_ARENA_CUBE_LOG2, wave_sum(kk));
}

// both sides' rules are rules (bg_cube.h's cube_rule_ok) of one game: the same cap and Jacoby
bool arena_rules_ok(const bgx_cube_rule& a, const bgx_cube_rule& b) {
    return cube_rule_ok(a) && cube_rule_ok(b) && a.cap == b.cap && (a.jacoby != 0) == (b.jacoby != 0);
}

}  // namespace

extern "C" {

int bgx_arena_cube_begin(int32_t n, uint8_t* cube_dev, int32_t* plies_dev, int64_t* cube_tally_dev, void* stream) {
    if (n <= 0 || !cube_dev || !plies_dev || !cube_tally_dev) return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_begin, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, cube_dev,
                       plies_dev, cube_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_cube_sel(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                       const int32_t* plies_dev, const uint8_t* cube_dev, int32_t n, int32_t cap, uint8_t* dsel_a_out,
                       uint8_t* dsel_b_out, void* stream) {
    if (!records_dev || !sel_a_dev || !sel_b_dev || !plies_dev || !cube_dev || n <= 0 || cap < 0 ||
        cap > kCubeMaxCap || !dsel_a_out || !dsel_b_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_sel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       sel_a_dev, sel_b_dev, plies_dev, cube_dev, n, cap, dsel_a_out, dsel_b_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_cube_offer(const uint8_t* records_dev, const uint8_t* dsel_a_dev, const uint8_t* dsel_b_dev,
                         const float* eq_a_dev, const float* eq_b_dev, bgx_cube_rule rule_a, bgx_cube_rule rule_b,
                         const uint8_t* cube_dev, int32_t n, uint8_t* off_a_out, uint8_t* off_b_out,
                         int64_t* cube_tally_dev, void* stream) {
    if (!records_dev || !dsel_a_dev || !dsel_b_dev || !eq_a_dev || !eq_b_dev || !arena_rules_ok(rule_a, rule_b) ||
        !cube_dev || n <= 0 || !off_a_out || !off_b_out || !cube_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_offer, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       dsel_a_dev, dsel_b_dev, eq_a_dev, eq_b_dev, rule_a, rule_b, cube_dev, n, off_a_out, off_b_out,
                       cube_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_cube_respond(const uint8_t* records_dev, const uint8_t* off_a_dev, const uint8_t* off_b_dev,
                           const float* eq_a_dev, const float* eq_b_dev, bgx_cube_rule rule_a, bgx_cube_rule rule_b,
                           int32_t n, int32_t games_per_lane, uint8_t* cube_dev, int32_t* plies_dev,
                           int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev,
                           int64_t* cube_tally_dev, uint8_t* reset_mask_out, void* stream) {
    if (!records_dev || !off_a_dev || !off_b_dev || !eq_a_dev || !eq_b_dev || !arena_rules_ok(rule_a, rule_b) ||
        n <= 0 || games_per_lane < 0 || !cube_dev || !plies_dev || !games_done_dev || !sel_a_dev || !sel_b_dev ||
        !tally_dev || !cube_tally_dev || !reset_mask_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_respond, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       off_a_dev, off_b_dev, eq_a_dev, eq_b_dev, rule_a, rule_b, n, games_per_lane, cube_dev, plies_dev,
                       games_done_dev, sel_a_dev, sel_b_dev, tally_dev, cube_tally_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_cube_reseat(const uint8_t* records_dev, const uint8_t* reset_mask_dev, int32_t n, int32_t games_per_lane,
                          const int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, void* stream) {
    if (!records_dev || !reset_mask_dev || n <= 0 || games_per_lane < 0 || !games_done_dev || !sel_a_dev || !sel_b_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_reseat, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       reset_mask_dev, n, games_per_lane, games_done_dev, sel_a_dev, sel_b_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_cube_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                         const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t jacoby, int32_t cap,
                         uint8_t* cube_dev, int32_t* plies_dev, int64_t* cube_tally_dev, void* stream) {
    if (!sel_a_dev || !sel_b_dev || !done_dev || !info_dev || !games_done_dev || n <= 0 || cap < 0 ||
        cap > kCubeMaxCap || !cube_dev || !plies_dev || !cube_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_cube_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sel_a_dev,
                       sel_b_dev, done_dev, info_dev, games_done_dev, n, jacoby, cap, cube_dev, plies_dev,
                       cube_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
