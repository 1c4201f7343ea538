// bg_bearoff_cube.h — the cubeful exact bearoff table (include/bgx.h "cubeful
// bearoff table"; bgx/bearoff.py, bgx/cube.py and bgx/rollout.py drive it): for every pair of
// configurations of the two-sided table (bg_bearoff.h) the money-play equity of the side on roll
// in units of the current cube, for the three cube states cen / own / opp as that side sees them,
// and the equity when it does not double now.  Built from an existing bgx_bearoff through
// bgx_bearoff_buffers_get alone, so it needs nothing of bg_bearoff.h's part 2.  Included by
// bg_returns.hip only, after bg_cube.h: kernels added to bg_engine.hip move its step kernels in
// the code object, and no launch of the benchmark reads this one.
//
// Part 1 (plain C++, host and device): the cube state of a record's mover from the cube byte,
// the choice of the four values and the flags from the planes' entries, and the fixed-point
// value of a cut game.
// Part 2 (device): the build -- one launch per total pip count, one thread per (a, b) that walks
// a's successor lists once for all three states -- then the lookup and the cubeful rollout cut,
// one thread per lane record, and their C entry points.  It reuses bg_cube.h's byte decoding,
// bg_bearoff1.h's B1Rec, bg_rollout.h's helpers and bg_returns.hip's mul_rn / add_rn / sub_rn.
// BGX_CUBE_PART1_ONLY (the host test program tools/cube_bearoff_host.cpp, any C++ compiler) takes
// part 1 alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "bg_cube.h"

namespace bg {

// the cube as the record's mover sees it; dead: the cube shows 2^cap, nobody doubles any more
enum BocState { kBocCen = 0, kBocOwn = 1, kBocOpp = 2, kBocDead = 3 };
constexpr float kBocOne = 1048576.0f;              // 2^20: the cut's fixed point

CUBE_HD int boc_state(uint8_t c, int cap, int mover) {
    if (cube_k(c, cap) >= cap) return kBocDead;
    const int o = cube_owner(c);
    return o == 0 ? kBocCen : o == (mover & 1) + 1 ? kBocOwn : kBocOpp;
}

// One (a, b) of the table as the lookup and the cut read it: nd_s = ND_s[a][b] for s = cen or
// own (not read otherwise), e_opp = E_opp[a][b], w = W[a][b].  values: nd, DT, e, cubeless.
// Without access e = nd; dead: nd = e = the cubeless value.  Every operation is exact but the
// cubeless 2 w - 1, and that is one rounding whether or not it is contracted (2 w is exact).
CUBE_HD uint8_t boc_values(int state, float nd_s, float e_opp, float w, float values[4]) {
    const float dt = 2.0f * e_opp, cl = 2.0f * w - 1.0f;
    const bool access = state == kBocCen || state == kBocOwn;
    const float nd = access ? nd_s : state == kBocOpp ? e_opp : cl;
    const float cash = dt < 1.0f ? dt : 1.0f;
    const bool doubles = access && cash > nd;      // strict: a tie is no double
    values[0] = nd;
    values[1] = dt;
    values[2] = doubles ? cash : nd;
    values[3] = cl;
    return (uint8_t)((access ? kBocMayDouble : 0) | (doubles ? kBocDoubles : 0) | (dt <= 1.0f ? kBocTakes : 0) |
                     (state == kBocDead ? kBocIsDead : 0));
}

// A cut game's result in 2^-20 units of one point: v = the equity of the record's mover in units
// of the cube 2^k (nd on a game's first ply, where the decision lies behind, else e), signed for
// the start mover.  Qq = rint(q 2^20) clamped to +-2^20 (0 for a NaN), Yq = Qq 2^k.
CUBE_HD long long boc_fixed(float v, bool start_mover_on_roll, int k) {
    float x = (start_mover_on_roll ? v : -v) * kBocOne;
    if (!(x == x)) return 0;
    x = x > kBocOne ? kBocOne : x < -kBocOne ? -kBocOne : x;
    return (long long)llrintf(x) * (1ll << k);
}

}  // namespace bg

#ifndef BGX_CUBE_PART1_ONLY
// ======================================================================== part 2 ==
#include <vector>

#include "bg_debug.h"
#include "bg_rollout.h"

// The object behind the C ABI's opaque bgx_bearoff_cube*: device buffers, fixed after creation.
// W, succ_off and succ stay the cubeless database's, which must outlive this object.
struct bgx_bearoff_cube {
    int device{0};
    int K{0}, n{0};
    float* equity{nullptr};        // [3][n][n] E_cen, E_own, E_opp
    float* nd{nullptr};            // [2][n][n] ND_cen, ND_own
    int16_t* rank_of{nullptr};     // [9^6] key -> index, -1 = more than K checkers
    int32_t* level{nullptr};       // [6 K + 2] first index of each pip count; then n pip counts
    const float* W{nullptr};
    const int8_t* configs{nullptr};
};

namespace {

using namespace bg;

// boundary rows of every plane and of the transposed working copies (tr, may be NULL):
// [a][empty] = -1 (the opponent has already won), [empty][b] = +1 for b != empty
__global__ __launch_bounds__(256) void k_boc_init(float* E, float* ND, float* tr, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t nn = (size_t)n * n;
    for (int s = 0; s < 3; ++s) {
        E[s * nn + (size_t)i * n] = -1.0f;
        if (i > 0) E[s * nn + i] = 1.0f;
        if (tr) {
            tr[s * nn + i] = -1.0f;
            if (i > 0) tr[s * nn + (size_t)i * n] = 1.0f;
        }
        if (s < 2) {
            ND[s * nn + (size_t)i * n] = -1.0f;
            if (i > 0) ND[s * nn + i] = 1.0f;
        }
    }
}

// One level: every state (a, b) of total pip count t, laid out as k_bo_level (block y =
// configuration a0 + y, threads over the b of pip count t - pa).  The child values E_c[b][a'] have
// a smaller total, so an earlier launch wrote them.  TR: they are read from the transposed
// working copy tr_c[a'][b], where the wave's lanes (consecutive b) read consecutive floats; else
// from the planes themselves, a stride of n floats between lanes.  The child of cen is cen, of
// own opp, of opp own.  Each product and sum is rounded once, the rolls in order from 0.
template <bool TR>
__global__ __launch_bounds__(128) void k_boc_level(float* E, float* ND, float* tr, const int32_t* __restrict__ succ_off,
                                                   const int32_t* __restrict__ succ, const int32_t* __restrict__ level,
                                                   int n, int max_pip, int t, int a0) {
    const int a = a0 + (int)blockIdx.y;
    if (a >= n) return;
    const int pb = t - level[max_pip + 2 + a];
    if (pb < 1 || pb > max_pip) return;
    const int b = level[pb] + (int)blockIdx.x * 128 + (int)threadIdx.x;
    if (b >= level[pb + 1]) return;
    const size_t nn = (size_t)n * n, step = TR ? (size_t)n : 1;
    const float* base = TR ? tr + b : E + (size_t)b * n;
    const float *c_cen = base, *c_own = base + nn, *c_opp = base + 2 * nn;
    const int32_t* off = succ_off + (size_t)a * kBoRolls;
    float acc_cen = 0.0f, acc_own = 0.0f, acc_opp = 0.0f;
    int r = 0;
    for (int r0 = 1; r0 <= 6; ++r0) {
        for (int r1 = r0; r1 <= 6; ++r1, ++r) {
            float w_cen = -3.0f, w_own = -3.0f, w_opp = -3.0f;      // below every equity: a set is never empty
            for (int j = off[r]; j < off[r + 1]; ++j) {
                const int ap = succ[j];
                const size_t at = (size_t)ap * step;
                w_cen = fmaxf(w_cen, ap == 0 ? 1.0f : -c_cen[at]);
                w_own = fmaxf(w_own, ap == 0 ? 1.0f : -c_opp[at]);
                w_opp = fmaxf(w_opp, ap == 0 ? 1.0f : -c_own[at]);
            }
            const float p = r0 == r1 ? 1.0f / 36.0f : 2.0f / 36.0f;
            acc_cen = add_rn(acc_cen, mul_rn(p, w_cen));
            acc_own = add_rn(acc_own, mul_rn(p, w_own));
            acc_opp = add_rn(acc_opp, mul_rn(p, w_opp));
        }
    }
    const float cash = fminf(mul_rn(2.0f, acc_opp), 1.0f);
    const float e_cen = fmaxf(acc_cen, cash), e_own = fmaxf(acc_own, cash);
    const size_t ab = (size_t)a * n + b;
    E[ab] = e_cen;
    E[nn + ab] = e_own;
    E[2 * nn + ab] = acc_opp;
    ND[ab] = acc_cen;
    ND[nn + ab] = acc_own;
    if (TR) {
        const size_t ba = (size_t)b * n + a;
        tr[ba] = e_cen;
        tr[nn + ba] = e_own;
        tr[2 * nn + ba] = acc_opp;
    }
}

// bgx_bearoff_lookup's record test (bo_in_table of bg_bearoff.h) on a B1Rec
__device__ __forceinline__ bool boc_in_table(const B1Rec& rec, int K, const int16_t* __restrict__ rank_of, int idx[2]) {
    int out0 = 0, out1 = 0, home0 = 0, home1 = 0;
    #pragma unroll
    for (int p = 0; p < 18; ++p) { out0 += rec.at(p); out1 += rec.at(24 + 6 + p); }
    #pragma unroll
    for (int d = 1; d <= 6; ++d) { home0 += rec.at(24 - d); home1 += rec.at(24 + d - 1); }
    const bool in = rec.at(R_OVER) == 0 && rec.at(48) == 0 && rec.at(49) == 0 && out0 == 0 && out1 == 0 &&
                    home0 >= 1 && home0 <= K && home1 >= 1 && home1 <= K && home0 + rec.at(50) == 15 &&
                    home1 + rec.at(51) == 15;
    if (!in) return false;                     // only now are the keys known to be below 9^6
    idx[0] = (int)rank_of[bo_key(rec.pack(0))];
    idx[1] = (int)rank_of[bo_key(rec.pack(1))];
    return idx[0] > 0 && idx[1] > 0;
}

// the four values and the flags of the mover m (configuration idx[m]) holding the cube byte c
__device__ __forceinline__ uint8_t boc_read(const float* __restrict__ E, const float* __restrict__ ND,
                                            const float* __restrict__ W, int n, const int idx[2], int m, uint8_t c, int cap,
                                            float values[4]) {
    const size_t nn = (size_t)n * n, ab = (size_t)idx[m] * n + idx[1 - m];
    const int state = boc_state(c, cap, m);
    const float nd_s = state == kBocCen ? ND[ab] : state == kBocOwn ? ND[nn + ab] : 0.0f;
    return boc_values(state, nd_s, E[2 * nn + ab], W[ab], values);
}

__global__ __launch_bounds__(256) void k_boc_lookup(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ cube,
                                                    int n_rec, int cap, int K, int n, const int16_t* __restrict__ rank_of,
                                                    const float* __restrict__ E, const float* __restrict__ ND,
                                                    const float* __restrict__ W, uint8_t* in_db, float* values,
                                                    uint8_t* flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rec) return;
    B1Rec rec;
    rec.load(recs, i);
    int idx[2];
    const bool in = boc_in_table(rec, K, rank_of, idx);
    in_db[i] = in ? 1 : 0;
    uint8_t fl = 0;
    if (in) {
        float v[4];
        fl = boc_read(E, ND, W, n, idx, rec.at(R_CUR) & 1, cube ? cube[i] : (uint8_t)0, cap, v);
        if (values) ((float4*)values)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (flags) flags[i] = fl;
}

// ---- the cubeful rollout cut (bgx_rollout_cube_bearoff_cut), after bgx_rollout_begin +
// bgx_rollout_cube_begin and after every bgx_rollout_advance: bg_rollout.h's cut skeleton (cut_group,
// end_game, cut_finish) with the cubeful expectation, scaled by the lane's cube, as the game's result ----
__global__ __launch_bounds__(256) void k_boc_cut(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                 const int32_t* __restrict__ group, int n_rec, int n_groups, int G,
                                                 int cap, int K, int n, const int16_t* __restrict__ rank_of,
                                                 const float* __restrict__ E, const float* __restrict__ ND,
                                                 const float* __restrict__ W, const uint8_t* __restrict__ cube0,
                                                 uint8_t* cube, int32_t* games_done, int32_t* plies, uint8_t* sel,
                                                 int64_t* cut_tally, int64_t* active, uint8_t* mask) {
    static_assert(BGX_ROLLOUT_CUBE_CUT_Y == 2 && BGX_ROLLOUT_CUBE_CUT_Y2_LO == 3 && BGX_ROLLOUT_CUBE_CUT_Y2_HI == 4 &&
                  BGX_ROLLOUT_CUBE_CUT_LOG2 == 5, "cube_cut_tally: `own` in field order");
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = cut_group(sel, group, i, n_rec, n_groups);
    bool cut = false, retired = false;
    long long yq = 0, pl = 0, kk = 0;
    if (g >= 0) {
        B1Rec rec;
        rec.load(recs, i);
        int idx[2];
        if (boc_in_table(rec, K, rank_of, idx)) {
            cut = true;
            const uint8_t c = cube[i];
            float v[4];
            boc_read(E, ND, W, n, idx, rec.at(R_CUR) & 1, c, cap, v);
            retired = end_game(i, G, games_done, plies, sel, &pl);
            kk = cube_k(c, cap);
            yq = boc_fixed(pl == 0 ? v[0] : v[2], rec.at(R_CUR) == (int)starts[(size_t)i * 64 + R_CUR], (int)kk);
            cube[i] = cube_sanitise(cube0[i], cap);
        }
    }
    long long own[4] = {yq, 0, 0, kk};
    square_split(yq, &own[1], &own[2]);
    cut_finish(i, n_rec, cut, retired, g, pl, own, cut_tally, active, mask);
}

}  // namespace

extern "C" {

int bgx_bearoff_cube_destroy(bgx_bearoff_cube* cdb) {
    if (!cdb) return BGX_EINVAL;
    (void)hipSetDevice(cdb->device);
    (void)hipDeviceSynchronize();                     // nothing in flight reads the buffers
    for (void* p : {(void*)cdb->equity, (void*)cdb->nd, (void*)cdb->rank_of, (void*)cdb->level})
        if (p) (void)hipFree(p);
    delete cdb;
    return BGX_OK;
}

int bgx_bearoff_cube_create(bgx_bearoff* db, void* stream, bgx_bearoff_cube** out) {
    if (!db || !out) return BGX_EINVAL;
    bgx_bearoff_buffers src;
    if (bgx_bearoff_buffers_get(db, &src) != BGX_OK || !src.table || src.n < 2 || src.max_checkers < 1 ||
        src.max_checkers > kBoMaxK)
        return BGX_EINVAL;
    hipPointerAttribute_t attr;
    BGX_CK(hipPointerGetAttributes(&attr, src.table));
    BGX_CK(hipSetDevice(attr.device));
    hipStream_t s = (hipStream_t)stream;
    const int K = src.max_checkers, n = src.n, max_pip = 6 * K;
    const size_t nn = (size_t)n * n;
    // the index order is the database's: rank_of and the level bounds follow from its configs
    std::vector<int8_t> configs((size_t)n * 6);
    BGX_CK(hipMemcpyAsync(configs.data(), src.configs, configs.size(), hipMemcpyDeviceToHost, s));
    BGX_CK(hipStreamSynchronize(s));
    std::vector<int16_t> rank((size_t)kBoKeys, (int16_t)-1);
    std::vector<int32_t> level((size_t)max_pip + 2 + n, n);      // level[p] = first index of pip count p
    int last = 0;
    for (int i = n - 1; i >= 0; --i) {
        int pip = 0, key = 0, sum = 0;
        for (int d = 6; d >= 1; --d) {
            const int c = configs[(size_t)i * 6 + d - 1];
            if (c < 0 || c > K) { bgx_set_error("bearoff_cube: a configuration's count is out of range"); return BGX_EINVAL; }
            pip += d * c; key = key * 9 + c; sum += c;
        }
        if (sum > K || (i < n - 1 && pip > last)) { bgx_set_error("bearoff_cube: configurations out of order"); return BGX_EINVAL; }
        last = pip;
        rank[key] = (int16_t)i;
        level[pip] = i;
        level[max_pip + 2 + i] = pip;
    }
    int widest = 1;
    for (int p = max_pip; p >= 0; --p) widest = std::max(widest, level[p + 1] - level[p]);
    // BGX_BOC_DIRECT (bgx_debug_option; tools/cube_bearoff_profile.py): build without the
    // transposed working copies -- the same bits, strided child reads
    const bool transposed = bgx_dbg("BGX_BOC_DIRECT").empty();

    bgx_bearoff_cube* cdb = new bgx_bearoff_cube();
    cdb->device = attr.device; cdb->K = K; cdb->n = n; cdb->W = src.table; cdb->configs = src.configs;
    float* tr = nullptr;
    hipError_t err = hipSuccess;
    const struct { void** p; size_t bytes; } bufs[] = {
        {(void**)&cdb->equity, 3 * nn * 4}, {(void**)&cdb->nd, 2 * nn * 4}, {(void**)&cdb->rank_of, rank.size() * 2},
        {(void**)&cdb->level, level.size() * 4}, {(void**)&tr, transposed ? 3 * nn * 4 : 0}};
    for (const auto& b : bufs) if (err == hipSuccess && b.bytes) err = hipMalloc(b.p, b.bytes);
    if (err != hipSuccess) {
        if (tr) (void)hipFree(tr);
        bgx_bearoff_cube_destroy(cdb);
        return bgx_internal_fail(err, BGX_ENOMEM);
    }
    // a failure below frees everything again (after the stream has drained)
    auto build = [&]() -> int {
        BGX_CK(hipMemcpyAsync(cdb->rank_of, rank.data(), rank.size() * 2, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemcpyAsync(cdb->level, level.data(), level.size() * 4, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemsetAsync(cdb->equity, 0, 3 * nn * 4, s));
        BGX_CK(hipMemsetAsync(cdb->nd, 0, 2 * nn * 4, s));
        if (tr) BGX_CK(hipMemsetAsync(tr, 0, 3 * nn * 4, s));
        hipLaunchKernelGGL(k_boc_init, dim3((n + 255) / 256), dim3(256), 0, s, cdb->equity, cdb->nd, tr, n);
        for (int t = 2; t <= 2 * max_pip; ++t) {
            const int p_lo = std::max(1, t - max_pip), p_hi = std::min(max_pip, t - 1);
            const int a0 = level[p_lo], a1 = level[p_hi + 1];
            if (a1 <= a0) continue;
            const dim3 grid((widest + 127) / 128, a1 - a0);
            if (transposed)
                hipLaunchKernelGGL(k_boc_level<true>, grid, dim3(128), 0, s, cdb->equity, cdb->nd, tr, src.succ_off,
                                   src.succ, cdb->level, n, max_pip, t, a0);
            else
                hipLaunchKernelGGL(k_boc_level<false>, grid, dim3(128), 0, s, cdb->equity, cdb->nd, tr, src.succ_off,
                                   src.succ, cdb->level, n, max_pip, t, a0);
        }
        BGX_CK_LAUNCH();
        BGX_CK(hipStreamSynchronize(s));
        return BGX_OK;
    };
    const int rc = build();
    if (rc != BGX_OK) (void)hipStreamSynchronize(s);
    if (tr) (void)hipFree(tr);
    if (rc != BGX_OK) { bgx_bearoff_cube_destroy(cdb); return rc; }
    *out = cdb;
    return BGX_OK;
}

int bgx_bearoff_cube_buffers_get(bgx_bearoff_cube* cdb, bgx_bearoff_cube_buffers* out) {
    if (!cdb || !out) return BGX_EINVAL;
    out->equity = cdb->equity; out->nd = cdb->nd; out->configs = cdb->configs;
    out->n = cdb->n; out->max_checkers = cdb->K;
    return BGX_OK;
}

int bgx_bearoff_cube_lookup(const bgx_bearoff_cube* cdb, const uint8_t* records_dev, const uint8_t* cube_dev, int32_t n,
                            int32_t cap, uint8_t* in_db_out, float* values_out, uint8_t* flags_out, void* stream) {
    if (!cdb || n < 0 || cap < 0 || cap > kCubeMaxCap || (n > 0 && (!records_dev || !in_db_out)) ||
        ((uintptr_t)records_dev & 15) || ((uintptr_t)values_out & 15))
        return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipLaunchKernelGGL(k_boc_lookup, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, cube_dev, n,
                       cap, cdb->K, cdb->n, cdb->rank_of, cdb->equity, cdb->nd, cdb->W, in_db_out, values_out, flags_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_cube_bearoff_cut(const bgx_bearoff_cube* cdb, const uint8_t* records_dev, const uint8_t* starts_dev,
                                 const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                                 int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                                 int64_t* cube_cut_tally_dev, int64_t* active_dev, uint8_t* reset_mask_out, int32_t cap,
                                 const uint8_t* cube0_dev, uint8_t* cube_dev, void* stream) {
    if (!cdb || !records_dev || !starts_dev || !group_dev || n <= 0 || n_groups <= 0 || games_per_lane < 0 ||
        !games_done_dev || !plies_dev || !sel_dev || !cube_cut_tally_dev || !active_dev || !reset_mask_out ||
        ((uintptr_t)records_dev & 15) || cap < 0 || cap > kCubeMaxCap || !cube0_dev || !cube_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_boc_cut, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, starts_dev,
                       group_dev, n, n_groups, games_per_lane, cap, cdb->K, cdb->n, cdb->rank_of, cdb->equity, cdb->nd,
                       cdb->W, cube0_dev, cube_dev, games_done_dev, plies_dev, sel_dev, cube_cut_tally_dev, active_dev,
                       reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
