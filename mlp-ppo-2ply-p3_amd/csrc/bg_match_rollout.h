// bg_match_rollout.h — position rollouts at a match score: single games from a start position at
// a fixed score, cube decisions by the arena's match rule, and a histogram of the games' outcomes from
// which the host takes the match-winning chance (include/bgx.h "match-score
// rollouts"; bgx/match.py and bgx/rollout.py drive it).  Included by bg_returns.hip only, after the
// arena's match header, for the reason bg_cube.h gives: kernels added to
// bg_engine.hip move its step kernels in the code object.  It includes nothing
// itself: whoever includes it has included the match header first, whose part 1 it builds on.
//
// Part 1 (plain C++, host and device): the bin index of an outcome, the fused decision of a step
// (none / take / pass and the next cube byte), built from the match header's match_access,
// match_offers and match_passes, and the argument checks of the entry points.
// Part 2 (device): the four kernels, one thread per lane, and their C entry points.  They use
// bg_rollout.h's helpers (rollout_group, end_game, for_each_group, tally_add, count, wave_sum,
// result_of).  No LDS, no scratch.  BGX_MATCH_ROLLOUT_PART1_ONLY (the host test program
// tools/match_rollout_host.cpp, any C++ compiler, after the match header's own part 1) takes part
// 1 alone.
#pragma once

namespace bg {

// match_hist int64[n_groups][96] (include/bgx.h bgx_rollout_match_field): 88 outcome bins, then
// six sums, then two entries that stay zero.
constexpr int kMatchKinds = 4;                              // 0 a pass, 1 / 2 / 3 the played-out score
constexpr int kMatchBinsPerKind = kCubeMaxCap + 1;          // k in 0..10
constexpr int kMatchBins = 2 * kMatchKinds * kMatchBinsPerKind;      // 88
constexpr int kMatchHistRow = 96;

// The bin of a game's outcome: won * 44 + kind * 11 + k, with won = the start record's mover won
// the game, kind 0 a pass and 1 / 2 / 3 the played-out score, k the cube at the end (before the
// double for a pass).  Total: kind reads as clamped to 0..3, k to 0..10, so the index stays in 0..87.
CUBE_HD int match_bin(bool won, int kind, int k) {
    kind = kind < 0 ? 0 : kind > kMatchKinds - 1 ? kMatchKinds - 1 : kind;
    k = k < 0 ? 0 : k > kCubeMaxCap ? kCubeMaxCap : k;
    return (won ? kMatchKinds * kMatchBinsPerKind : 0) + kind * kMatchBinsPerKind + k;
}

// The decision of a step on one lane.  The side on roll (record mover byte `mover`, needing x, the
// other y) holds the cube byte c (read with cap 10).  Without access (match_access): kCubeNone.
// With access it doubles iff match_offers on `value`; the other side answers by the same rule on
// the same value: kCubePass iff match_passes, else kCubeTake and *next = k + 1 owned by the taker.
// *next is the byte as it stood (sanitised) otherwise; after a pass the caller puts the game's
// starting cube back.  A NaN value neither offers nor passes.
CUBE_HD int match_rollout_decision(const match_tables& t, uint8_t c, int mover, int plies, bool over, bool active,
                                   int craw, int x, int y, const match_rule& r, float value, uint8_t* next) {
    *next = cube_sanitise(c, kCubeMaxCap);
    if (!match_access(c, mover, plies, over, active, craw, x)) return kCubeNone;
    const int k = cube_k(c, kCubeMaxCap);
    if (!match_offers(t, x, y, craw, k, r, value)) return kCubeNone;
    if (match_passes(t, x, y, craw, k, r, value)) return kCubePass;
    *next = cube_taken(c, kCubeMaxCap, mover);
    return kCubeTake;
}

// the argument checks of the entry points (pointers apart)
CUBE_HD bool match_rollout_length_ok(int L) { return L >= 1 && L <= kMatchMaxLength; }
CUBE_HD bool match_rollout_sizes_ok(int n, int n_groups) { return n > 0 && n_groups > 0; }
CUBE_HD bool match_rollout_rule_ok(const match_rule& r, int L) { return match_rollout_length_ok(L) && match_rule_ok(r); }

}  // namespace bg

#ifndef BGX_MATCH_ROLLOUT_PART1_ONLY
// ======================================================================== part 2 ==

namespace {

using namespace bg;

static_assert(BGX_ROLLOUT_MATCH_BINS == kMatchBins && BGX_ROLLOUT_MATCH_ROW == kMatchHistRow &&
              BGX_ROLLOUT_MATCH_GAMES == 88 && BGX_ROLLOUT_MATCH_LOG2 == 93, "match_hist: 88 bins, six sums");

// one finished game joins its bin: few lanes finish in a step, so a 64-bit atomic per lane
__device__ __forceinline__ void match_bin_add(int64_t* hist, int g, int bin) {
    atomicAdd((unsigned long long*)hist + (size_t)g * kMatchHistRow + bin, 1ull);
}

// the lane's access from its record, plies, cube and its group's score; g is valid
__device__ __forceinline__ bool match_lane_access(const uint8_t* recs, int i, int g, bool active, const int32_t* plies,
                                                  const uint8_t* cube, const uint8_t* away, const uint8_t* craw) {
    const uint8_t* r = recs + (size_t)i * 64;
    return match_access(cube[i], r[R_CUR], plies[i], r[R_OVER] != 0, active, craw[g], away[2 * g + (r[R_CUR] & 1)]);
}

__global__ __launch_bounds__(256) void k_match_ro_sel(const uint8_t* __restrict__ recs, const int32_t* __restrict__ group,
                                                      int n_groups, const int32_t* __restrict__ plies,
                                                      const uint8_t* __restrict__ sel, const uint8_t* __restrict__ cube,
                                                      const uint8_t* __restrict__ away, const uint8_t* __restrict__ craw,
                                                      int n, uint8_t* dsel) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int g = sel[i] != 0 ? rollout_group(group, i, n_groups) : -1;
    dsel[i] = g >= 0 && match_lane_access(recs, i, g, true, plies, cube, away, craw) ? 1 : 0;
}

// The decision on the dsel lanes, access tested again: a pass is binned at the cube before the
// double and ends the game (end_game: the game is counted; the lane is masked for the reset and
// gets its starting cube back), a take turns the cube.
__global__ __launch_bounds__(256) void k_match_ro_decide(
    const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts, const int32_t* __restrict__ group,
    const uint8_t* __restrict__ dsel, const float* __restrict__ value, int n, int n_groups, int G, bgx_match_rule rule,
    const float* __restrict__ met, const float* __restrict__ pc, int L, const uint8_t* __restrict__ away,
    const uint8_t* __restrict__ craw, const uint8_t* __restrict__ cube0, uint8_t* cube, int32_t* games_done,
    int32_t* plies, uint8_t* sel, int64_t* hist, int64_t* active, uint8_t* mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && dsel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    bool dbl = false, pass = false, retired = false, mine_start = false;
    long long kk = 0, pl = 0;
    if (g >= 0) {
        const uint8_t* r = recs + (size_t)i * 64;
        const int m = r[R_CUR] & 1;
        const uint8_t c = cube[i];
        const match_tables t{met, pc, L};
        uint8_t next;
        const int act = match_rollout_decision(t, c, m, plies[i], r[R_OVER] != 0, sel[i] != 0, craw[g], away[2 * g + m],
                                               away[2 * g + 1 - m],
                                               match_rule{rule.scale, rule.window, rule.win_gammons, rule.loss_gammons},
                                               value[i], &next);
        dbl = act != kCubeNone;
        pass = act == kCubePass;
        mine_start = m == (int)(starts[(size_t)i * 64 + R_CUR] & 1);
        if (pass) {
            kk = cube_k(c, kCubeMaxCap);
            match_bin_add(hist, g, match_bin(mine_start, 0, (int)kk));
            retired = end_game(i, G, games_done, plies, sel, &pl);
            cube[i] = cube_sanitise(cube0[i], kCubeMaxCap);
        } else if (dbl) {
            cube[i] = next;
        }
    }
    if (i < n) mask[i] = pass ? 1 : 0;
    // every thread of the wave reaches the ballots (no early return above)
    for_each_group(dbl, g, [&](int gl, bool mine, uint64_t) {
        const bool pm = mine && pass;
        const long long np = count(pm);
        int64_t* row = hist + (size_t)gl * kMatchHistRow;
        tally_add(row, BGX_ROLLOUT_MATCH_GAMES, np);
        tally_add(row, BGX_ROLLOUT_MATCH_PASS_GAMES, np);
        tally_add(row, BGX_ROLLOUT_MATCH_DOUBLES_START, count(mine && mine_start));
        tally_add(row, BGX_ROLLOUT_MATCH_DOUBLES_OTHER, count(mine && !mine_start));
        tally_add(row, BGX_ROLLOUT_MATCH_PASS_PLIES, wave_sum(pm ? pl : 0));
        tally_add(row, BGX_ROLLOUT_MATCH_LOG2, wave_sum(pm ? kk : 0));
    });
    tally_add(active, 0, -count(retired));
}

// After the step, before bgx_rollout_advance (sel is still the step's selection): a game that
// advance will count is binned at the cube's k; any done puts the lane's starting cube back.
__global__ __launch_bounds__(256) void k_match_ro_flush(const uint8_t* __restrict__ starts,
                                                        const int32_t* __restrict__ group,
                                                        const uint8_t* __restrict__ sel, const uint8_t* __restrict__ done,
                                                        const int32_t* __restrict__ info, int n, int n_groups,
                                                        const uint8_t* __restrict__ cube0, uint8_t* cube, int64_t* hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool dn = i < n && done[i] != 0;
    const int g = dn && sel[i] != 0 ? rollout_group(group, i, n_groups) : -1;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    const bool fin = g >= 0 && winner >= 0;
    long long kk = 0;
    if (fin) {
        kk = cube_k(cube[i], kCubeMaxCap);
        match_bin_add(hist, g, match_bin(winner == (int)(starts[(size_t)i * 64 + R_CUR] & 1), score, (int)kk));
    }
    if (dn) cube[i] = cube_sanitise(cube0[i], kCubeMaxCap);
    for_each_group(fin, g, [&](int gl, bool mine, uint64_t m) {
        int64_t* row = hist + (size_t)gl * kMatchHistRow;
        tally_add(row, BGX_ROLLOUT_MATCH_GAMES, (long long)__popcll(m));
        tally_add(row, BGX_ROLLOUT_MATCH_LOG2, wave_sum(mine ? kk : 0));
    });
}

// The static answer per lane: ND, DT, DP of the side on roll and the flags, from a value tensor.
__global__ __launch_bounds__(256) void k_match_decision(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ cube,
                                                        const uint8_t* __restrict__ away, const uint8_t* __restrict__ craw,
                                                        const float* __restrict__ value, int n, bgx_match_rule rule,
                                                        const float* __restrict__ met, const float* __restrict__ pc, int L,
                                                        float* values, uint8_t* flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = recs + (size_t)i * 64;
    const int m = r[R_CUR] & 1, x = away[2 * i + m], y = away[2 * i + 1 - m], cr = craw[i];
    const uint8_t c = cube[i];
    const int k = cube_k(c, kCubeMaxCap);
    const match_tables t{met, pc, L};
    const match_rule mr{rule.scale, rule.window, rule.win_gammons, rule.loss_gammons};
    const float v = value[i];
    float nd[3];
    match_values(t, x, y, cr, k, match_p(mr.scale, v, mr.win_gammons, mr.loss_gammons), mr.win_gammons, mr.loss_gammons, nd);
    const bool access = match_access(c, m, 1, r[R_OVER] != 0, true, cr, x);
    const bool offers = access && match_offers(t, x, y, cr, k, mr, v);
    const bool passes = match_passes(t, x, y, cr, k, mr, v);
    values[3 * (size_t)i] = nd[0];
    values[3 * (size_t)i + 1] = nd[1];
    values[3 * (size_t)i + 2] = nd[2];
    flags[i] = (uint8_t)((access ? 1 : 0) | (offers ? 2 : 0) | (passes ? 4 : 0) | (nd[0] > nd[2] ? 8 : 0));
}

bool match_ro_rule_ok(const bgx_match_rule& r, int L) {
    return match_rollout_rule_ok(match_rule{r.scale, r.window, r.win_gammons, r.loss_gammons}, L);
}

}  // namespace

extern "C" {

int bgx_rollout_match_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n_groups,
                          const int32_t* plies_dev, const uint8_t* sel_dev, const uint8_t* cube_dev,
                          const uint8_t* away_dev, const uint8_t* craw_dev, int32_t n, uint8_t* dsel_out, void* stream) {
    if (!records_dev || !group_dev || !plies_dev || !sel_dev || !cube_dev || !away_dev || !craw_dev || !dsel_out ||
        !match_rollout_sizes_ok(n, n_groups))
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_match_ro_sel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, group_dev,
                       n_groups, plies_dev, sel_dev, cube_dev, away_dev, craw_dev, n, dsel_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_match_decide(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                             const uint8_t* dsel_dev, const float* value_dev, int32_t n, int32_t n_groups,
                             int32_t games_per_lane, bgx_match_rule rule, const float* met_dev, const float* pc_dev,
                             int32_t length, const uint8_t* away_dev, const uint8_t* craw_dev, const uint8_t* cube0_dev,
                             uint8_t* cube_dev, int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                             int64_t* match_hist_dev, int64_t* active_dev, uint8_t* reset_mask_out, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !dsel_dev || !value_dev || !match_rollout_sizes_ok(n, n_groups) ||
        games_per_lane < 0 || !match_ro_rule_ok(rule, length) || !met_dev || !pc_dev || !away_dev || !craw_dev ||
        !cube0_dev || !cube_dev || !games_done_dev || !plies_dev || !sel_dev || !match_hist_dev || !active_dev ||
        !reset_mask_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_match_ro_decide, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       starts_dev, group_dev, dsel_dev, value_dev, n, n_groups, games_per_lane, rule, met_dev, pc_dev,
                       length, away_dev, craw_dev, cube0_dev, cube_dev, games_done_dev, plies_dev, sel_dev,
                       match_hist_dev, active_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_match_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                            const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                            const uint8_t* cube0_dev, uint8_t* cube_dev, int64_t* match_hist_dev, void* stream) {
    if (!starts_dev || !group_dev || !sel_dev || !done_dev || !info_dev || !match_rollout_sizes_ok(n, n_groups) ||
        !cube0_dev || !cube_dev || !match_hist_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_match_ro_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts_dev, group_dev,
                       sel_dev, done_dev, info_dev, n, n_groups, cube0_dev, cube_dev, match_hist_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_match_decision(const uint8_t* records_dev, const uint8_t* cube_dev, const uint8_t* away_dev,
                       const uint8_t* craw_dev, const float* value_dev, int32_t n, bgx_match_rule rule,
                       const float* met_dev, const float* pc_dev, int32_t length, float* values_out, uint8_t* flags_out,
                       void* stream) {
    if (!records_dev || !cube_dev || !away_dev || !craw_dev || !value_dev || n <= 0 || !match_ro_rule_ok(rule, length) ||
        !met_dev || !pc_dev || !values_out || !flags_out)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_match_decision, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, cube_dev,
                       away_dev, craw_dev, value_dev, n, rule, met_dev, pc_dev, length, values_out, flags_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
