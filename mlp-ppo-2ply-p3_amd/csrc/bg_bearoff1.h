// bg_bearoff1.h — the one-sided bearoff database (include/bgx.h "one-sided
// bearoff database"; bgx/bearoff.py drives it): for every configuration of one side's home board
// with at most K <= 15 checkers, the distribution of the number of rolls it needs to bear
// everything off when it plays to minimise their mean.  The win probability of a race between
// two home boards follows from two rows.  Included by bg_returns.hip only: kernels added to
// bg_engine.hip move its step kernels in the code object, the library keeps one
// code object per HIP source, and bg_returns.hip has the fp32 helpers this table's arithmetic
// needs (mul_rn / add_rn / sub_rn: no contraction to fma).
//
// Part 1 (plain C++ on top of part 1 of bg_bearoff.h, host and device): the configuration rank
// and the play visitor.  A configuration is a `pack` as in bg_bearoff.h (count d in nibble
// d - 1), now with a sum of up to 15; the pack is the base-16 key of the index order.  A
// successor set at K = 15 holds up to 108 configurations, more than a BoSet has room for, and
// the table needs none: the argmin over (mean, index) is the same with duplicates.  So the
// plays are walked, not stored.
// Part 2 (device): the build -- one pair of launches per pip count (a play always lowers it),
// k_b1_choice then k_b1_dist -- then lookup, play and the rollout cut, one thread per lane
// record, as in bg_bearoff.h, and their C entry points.  BGX_BEAROFF_HOST_ONLY (the host test
// program tools/bearoff1_host.cpp, any C++ compiler) takes part 1 alone.
#pragma once
#ifndef BGX_BEAROFF_HOST_ONLY
#define BGX_BEAROFF_PART1_ONLY
#endif
#include "bg_bearoff.h"

namespace bg {

constexpr int kB1MaxK = 15;
constexpr int kB1T = 32;                   // entries per row: t = 0..31 rolls

// C(a, B) for B <= a <= 21 as a product in registers (21 * 20 * ... * 16 < 2^32)
template <int B> BO_HD int b1_binom(int a) {
    uint32_t p = 1, f = 1;
    for (int i = 0; i < B; ++i) { p *= (uint32_t)(a - i); f *= (uint32_t)(i + 1); }
    return (int)(p / f);
}

// The rank of a configuration of at most K checkers among all of them, lexicographic on
// (c6, ..., c1): in [0, C(K + 6, 6)).  At position j with `rem` checkers still free and B = 6 - j
// positions left including this one, the tuples with a smaller count here number
// C(rem + B, B) - C(rem - c + B, B) (hockey stick).  The caller has checked the sum.
BO_HD int b1_rank(uint32_t pack, int K) {
    int rem = K, rank = 0, c;
    c = bo_at(pack, 6); rank += b1_binom<6>(rem + 6) - b1_binom<6>(rem - c + 6); rem -= c;
    c = bo_at(pack, 5); rank += b1_binom<5>(rem + 5) - b1_binom<5>(rem - c + 5); rem -= c;
    c = bo_at(pack, 4); rank += b1_binom<4>(rem + 4) - b1_binom<4>(rem - c + 4); rem -= c;
    c = bo_at(pack, 3); rank += b1_binom<3>(rem + 3) - b1_binom<3>(rem - c + 3); rem -= c;
    c = bo_at(pack, 2); rank += b1_binom<2>(rem + 2) - b1_binom<2>(rem - c + 2);
    return rank + bo_at(pack, 1);
}
BO_HD int b1_sum(uint32_t pack) {
    int s = 0;
    for (int d = 1; d <= 6; ++d) s += bo_at(pack, d);
    return s;
}

// bo_pass as a walk: v(configuration, sub-moves) for every play of d1 then d2, in bo_pass's
// order.  Returns bo_successors' test after its first pass: the plays gave one distinct
// configuration, by one sub-move.
template <class V> BO_HD bool bo_visit_pass(uint32_t pack, int d1, int d2, V& v) {
    uint32_t first[8], second[8];
    const int n1 = bo_moves(pack, d1, first);
    bool exists = false;
    for (int i = 0; i < n1 && !exists; ++i) exists = bo_moves(first[i], d2, second) > 0;
    bool single = n1 > 0 && !exists;
    for (int i = 0; i < n1; ++i) {
        if (!exists) { v(first[i], 1); single = single && first[i] == first[0]; continue; }
        const int n2 = bo_moves(first[i], d2, second);
        for (int j = 0; j < n2; ++j) v(second[j], 2);
    }
    return single;
}

// bo_doubles as a walk
template <class V> BO_HD void bo_visit_doubles(uint32_t pack, int d, V& v) {
    uint32_t l1[8], l2[8], l3[8], l4[8];
    bool got4 = false;
    const int n1 = bo_moves(pack, d, l1);
    for (int i = 0; i < n1; ++i) {
        const int n2 = bo_moves(l1[i], d, l2);
        if (n2 == 0 && !got4) v(l1[i], 1);
        for (int j = 0; j < n2; ++j) {
            const int n3 = bo_moves(l2[j], d, l3);
            if (n3 == 0 && !got4) v(l2[j], 2);
            for (int k = 0; k < n3; ++k) {
                const int n4 = bo_moves(l3[k], d, l4);
                if (n4 == 0 && !got4) v(l3[k], 3);
                for (int m = 0; m < n4; ++m) { v(l4[m], 4); got4 = true; }
            }
        }
    }
}

// Every play of (r0, r1) from `pack`, duplicates included: v(configuration, sub-moves).  The
// successor set of bo_successors is the distinct configurations visited with the largest
// number of sub-moves; the visitor keeps that filter (B1Argmin does: a longer play discards
// what shorter ones gave).  Nothing is visited from the empty configuration.
template <class V> BO_HD void bo_visit(uint32_t pack, int r0, int r1, V& v) {
    if (r0 != r1) {
        const int hi = r0 > r1 ? r0 : r1, lo = r0 > r1 ? r1 : r0;
        if (!bo_visit_pass(pack, hi, lo, v)) bo_visit_pass(pack, lo, hi, v);
    } else {
        bo_visit_doubles(pack, r0, v);
    }
}

// The visitor of the table's build: among the plays of the largest length, the configuration
// with the smallest (mean, index).  index_of maps b1_rank to the configuration's index.
struct B1Argmin {
    const float* mean;
    const int32_t* index_of;
    int K;
    int len, arg;
    float best;
    BO_HD void operator()(uint32_t pack, int l) {
        if (l < len) return;
        const int idx = index_of[b1_rank(pack, K)];
        const float m = mean[idx];
        if (l > len || m < best || (m == best && idx < arg)) { len = l; best = m; arg = idx; }
    }
};

}  // namespace bg

#ifndef BGX_BEAROFF_HOST_ONLY
// ======================================================================== part 2 ==
#include <algorithm>
#include <vector>

#include "bg_engine.h"
#include "bg_host.h"
#include "bg_rollout.h"

// The object behind the C ABI's opaque bgx_bearoff1*: device buffers, fixed after creation.
struct bgx_bearoff1 {
    int device{0};
    int K{0}, n{0};
    float* dist{nullptr};          // [n][32] D
    float* surv{nullptr};          // [n][32] S
    float* mean{nullptr};          // [n]
    int32_t* choice{nullptr};      // [n][21]
    int8_t* configs{nullptr};      // [n][6]
    int32_t* index_of{nullptr};    // [n] b1_rank -> index
    int32_t* err{nullptr};         // build errors: 1 = a non-zero D[a][31], 2 = a configuration without a play
};

namespace {

using namespace bg;

constexpr int kErrTail = 1, kErrPlay = 2;

// ---- build ----
// k_b1_choice: one thread per (configuration of the level, roll); blockIdx.y is the roll's
// slot, doubles first (1-1 .. 6-6, then the 15 others).  A doubles walk visits up to 7^4
// plays, another roll's at most 2 * 49: with the roll per block, a wave's lanes walk trees of
// one die pair, and the long walks are dispatched first.  A level has at most a few thousand
// configurations, so a block is one wave: the level spreads over as many CUs as it has waves.
__global__ __launch_bounds__(64) void k_b1_choice(const int8_t* __restrict__ configs,
                                                  const int32_t* __restrict__ index_of,
                                                  const float* __restrict__ mean, int K, int a0, int cnt,
                                                  int32_t* __restrict__ choice, int32_t* err) {
    const int slot = (int)blockIdx.y;
    int r = 0, r0 = 1, r1 = 1;
    for (int seen = 0; r < kBoRolls; ++r) {              // the slot's roll (the same in the whole block)
        bo_roll(r, r0, r1);
        if ((r0 == r1) != (slot < 6)) continue;
        if (seen == (slot < 6 ? slot : slot - 6)) break;
        ++seen;
    }
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= cnt) return;
    const int a = a0 + i;
    uint32_t pack = 0;
    #pragma unroll
    for (int d = 1; d <= 6; ++d) pack |= (uint32_t)(configs[(size_t)a * 6 + d - 1] & 15) << (4 * (d - 1));
    B1Argmin pick{mean, index_of, K, 0, 0, 0.0f};
    bo_visit(pack, r0, r1, pick);
    if (pick.len == 0) atomicOr(err, kErrPlay);
    choice[(size_t)a * kBoRolls + r] = pick.arg;
}

// k_b1_dist: 8 configurations a block, 32 threads each over t.  D[a][t] from the chosen
// successors' rows (written by earlier launches), then thread t = 0 runs the two sums that go
// in order of t: the mean and S.  Every product, sum and difference is rounded once.
__global__ __launch_bounds__(256) void k_b1_dist(const int32_t* __restrict__ choice, int a0, int cnt, float* dist,
                                                 float* __restrict__ surv, float* __restrict__ mean, int32_t* err) {
    __shared__ float sd[8][kB1T], ss[8][kB1T];
    const int c = (int)threadIdx.x >> 5, t = (int)threadIdx.x & 31;
    const int i = (int)blockIdx.x * 8 + c;
    const bool on = i < cnt;
    const int a = a0 + (on ? i : 0);
    float acc = 0.0f;
    if (on && t > 0) {
        const int32_t* ch = choice + (size_t)a * kBoRolls;
        int r = 0;
        for (int r0 = 1; r0 <= 6; ++r0)
            for (int r1 = r0; r1 <= 6; ++r1, ++r)
                acc = add_rn(acc, mul_rn(r0 == r1 ? 1.0f / 36.0f : 2.0f / 36.0f,
                                               dist[(size_t)ch[r] * kB1T + t - 1]));
    }
    sd[c][t] = acc;
    __syncthreads();
    if (on && t == 0) {
        float m = 0.0f, s = 1.0f;
        ss[c][0] = 1.0f;
        for (int u = 1; u < kB1T; ++u) {
            m = add_rn(m, mul_rn((float)u, sd[c][u]));
            ss[c][u] = s;
            s = sub_rn(s, sd[c][u]);
        }
        mean[a] = m;
        if (sd[c][kB1T - 1] != 0.0f) atomicOr(err, kErrTail);
    }
    __syncthreads();
    if (on) {
        dist[(size_t)a * kB1T + t] = acc;
        surv[(size_t)a * kB1T + t] = ss[c][t];
    }
}

// ---- records ----
// One 64-byte record in registers (constant indices only), as bg_bearoff.h's BoRec.
struct B1Rec {
    uint4 q[4];
    __device__ __forceinline__ void load(const uint8_t* recs, int i) {
        #pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = ((const uint4*)recs)[(size_t)i * 4 + k];
    }
    __device__ __forceinline__ int at(int j) const { return (int)((const uint8_t*)q)[j]; }
    // the mover's (side 0 = PLAYER1) home board as a pack; counts above 15 are cut (the table
    // test refuses such a record before the pack is used)
    __device__ __forceinline__ uint32_t pack(int side) const {
        uint32_t p = 0;
        #pragma unroll
        for (int d = 1; d <= 6; ++d)
            p |= (uint32_t)((side == 0 ? at(24 - d) : at(24 + d - 1)) & 15) << (4 * (d - 1));
        return p;
    }
};

// bgx_bearoff1_lookup's test: 0 = not in the table, 1 = in it and both sides have a checker
// off, 2 = in it with 15 checkers of a side on the board.  Gives the two sides' indices.
__device__ __forceinline__ int b1_in_table(const B1Rec& rec, int K, const int32_t* __restrict__ index_of, int idx[2]) {
    int out0 = 0, out1 = 0, home0 = 0, home1 = 0;
    #pragma unroll
    for (int p = 0; p < 18; ++p) { out0 += rec.at(p); out1 += rec.at(24 + 6 + p); }
    #pragma unroll
    for (int d = 1; d <= 6; ++d) { home0 += rec.at(24 - d); home1 += rec.at(24 + d - 1); }
    const bool in = rec.at(R_OVER) == 0 && rec.at(48) == 0 && rec.at(49) == 0 && out0 == 0 && out1 == 0 &&
                    home0 >= 1 && home0 <= K && home1 >= 1 && home1 <= K && home0 + rec.at(50) == 15 &&
                    home1 + rec.at(51) == 15;
    if (!in) return 0;                         // only now do the counts fit their nibbles
    idx[0] = index_of[b1_rank(rec.pack(0), K)];
    idx[1] = index_of[b1_rank(rec.pack(1), K)];
    return home0 < 15 && home1 < 15 ? 1 : 2;
}

// win1(x on roll, y) = sum_t D[x][t] S[y][t], t = 1..31 in order from 0.0f
__device__ __forceinline__ float b1_win(const float* __restrict__ dx, const float* __restrict__ sy) {
    float acc = 0.0f;
    #pragma unroll
    for (int t = 1; t < kB1T; ++t) acc = add_rn(acc, mul_rn(dx[t], sy[t]));
    return acc;
}

__global__ __launch_bounds__(256) void k_b1_lookup(const uint8_t* __restrict__ recs, int n_rec, int K,
                                                   const int32_t* __restrict__ index_of, const float* __restrict__ dist,
                                                   const float* __restrict__ surv, uint8_t* in_db, float* win) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rec) return;
    B1Rec rec;
    rec.load(recs, i);
    int idx[2];
    const int in = b1_in_table(rec, K, index_of, idx);
    in_db[i] = (uint8_t)in;
    if (in && win) {
        const int m = rec.at(R_CUR) & 1;
        win[i] = b1_win(dist + (size_t)idx[m] * kB1T, surv + (size_t)idx[1 - m] * kB1T);
    }
}

// ---- play: one thread per lane over the engine's own move list (k_bo_act's walk) ----
__global__ __launch_bounds__(256) void k_b1_act(const uint8_t* __restrict__ recs, const uint64_t* __restrict__ moves,
                                                int B, int max_moves, const uint8_t* __restrict__ sel, int K,
                                                const int32_t* __restrict__ index_of, const float* __restrict__ dist,
                                                const float* __restrict__ surv, int32_t* act, uint8_t* in_db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if (sel && sel[i] == 0) {
        if (in_db) in_db[i] = 0;
        return;
    }
    B1Rec rec;
    rec.load(recs, i);
    int idx[2];
    const int in = b1_in_table(rec, K, index_of, idx);
    if (in_db) in_db[i] = (uint8_t)in;
    const int nm = min(rec.at(R_NM0) | (rec.at(R_NM1) << 8), max_moves);
    if (!in || nm <= 0) return;
    const int mover = rec.at(R_CUR) & 1;
    const uint32_t own = rec.pack(mover);
    float dopp[kB1T];                                  // the opponent's row, read once
    #pragma unroll
    for (int t = 0; t < kB1T; ++t) dopp[t] = dist[(size_t)idx[1 - mover] * kB1T + t];
    float best = -2.0f;
    int arg = 0;
    for (int m = 0; m < nm; ++m) {
        const uint64_t mv = moves[(size_t)i * max_moves + m];
        uint32_t pack = own;
        bool ok = true;
        for (int s = 0; s < 4 && ok; ++s) {
            const uint32_t e = (uint32_t)(mv >> (16 * s)) & 0xFFFFu;
            if (!(e & 0x8000u)) break;
            const int src = (int)(e & 31u), dst = (int)((e >> 5) & 31u);
            const int ds = mover == 0 ? 24 - src : src + 1, dd = mover == 0 ? 24 - dst : dst + 1;
            ok = ds >= 1 && ds <= 6 && bo_at(pack, ds) > 0 && (dst == kOff || (dd >= 1 && dd <= 6));
            if (!ok) break;
            pack -= bo_one(ds);
            if (dst != kOff) pack += bo_one(dd);
        }
        float v = -1.0f;                                // a move that leaves the home board: never chosen
        if (ok) {
            if (pack == 0u) {
                v = 1.0f;
            } else {
                const float* sy = surv + (size_t)index_of[b1_rank(pack, K)] * kB1T;
                float acc = 0.0f;
                #pragma unroll
                for (int t = 1; t < kB1T; ++t) acc = add_rn(acc, mul_rn(dopp[t], sy[t]));
                v = sub_rn(1.0f, acc);
            }
        }
        if (v > best) { best = v; arg = m; }
    }
    act[i] = arg;
}

// ---- rollout cut (bgx_rollout_bearoff1_cut): bg_rollout.h's table_cut on this table, where the
// record is in it with checkers of both sides off (the test's value 1: a single game) ----
__global__ __launch_bounds__(256) void k_b1_cut(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                const int32_t* __restrict__ group, int n_rec, int n_groups, int G,
                                                int K, const int32_t* __restrict__ index_of,
                                                const float* __restrict__ dist, const float* __restrict__ surv,
                                                int32_t* games_done, int32_t* plies, uint8_t* sel, int64_t* cut_tally,
                                                int64_t* active, uint8_t* mask) {
    table_cut(starts, group, n_rec, n_groups, G, games_done, plies, sel, cut_tally, active, mask,
              [&](int i, int* cur, float* w) {
        B1Rec rec;
        rec.load(recs, i);
        int idx[2];
        if (b1_in_table(rec, K, index_of, idx) != 1) return false;
        *cur = rec.at(R_CUR);
        const int m = *cur & 1;
        *w = b1_win(dist + (size_t)idx[m] * kB1T, surv + (size_t)idx[1 - m] * kB1T);
        return true;
    });
}

// the host's list of configurations: (pip count, pack) ascending
struct B1Config { int pip; uint32_t pack; };

}  // namespace

extern "C" {

int bgx_bearoff1_destroy(bgx_bearoff1* db) {
    if (!db) return BGX_EINVAL;
    (void)hipSetDevice(db->device);
    (void)hipDeviceSynchronize();                     // nothing in flight reads the buffers
    for (void* p : {(void*)db->dist, (void*)db->surv, (void*)db->mean, (void*)db->choice, (void*)db->configs,
                    (void*)db->index_of, (void*)db->err})
        if (p) (void)hipFree(p);
    delete db;
    return BGX_OK;
}

int bgx_bearoff1_create(int device, int32_t max_checkers, void* stream, bgx_bearoff1** out) {
    if (!out || max_checkers < 1 || max_checkers > kB1MaxK) return BGX_EINVAL;
    BGX_CK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int K = max_checkers, max_pip = 6 * K;
    std::vector<B1Config> cfg;
    int c[6];
    for (c[0] = 0; c[0] <= K; ++c[0]) for (c[1] = 0; c[0] + c[1] <= K; ++c[1])
    for (c[2] = 0; c[0] + c[1] + c[2] <= K; ++c[2]) for (c[3] = 0; c[0] + c[1] + c[2] + c[3] <= K; ++c[3])
    for (c[4] = 0; c[0] + c[1] + c[2] + c[3] + c[4] <= K; ++c[4])
    for (c[5] = 0; c[0] + c[1] + c[2] + c[3] + c[4] + c[5] <= K; ++c[5]) {
        B1Config x{0, 0u};
        for (int d = 1; d <= 6; ++d) { x.pip += d * c[d - 1]; x.pack |= (uint32_t)c[d - 1] << (4 * (d - 1)); }
        cfg.push_back(x);
    }
    std::sort(cfg.begin(), cfg.end(), [](const B1Config& a, const B1Config& b) {
        return a.pip != b.pip ? a.pip < b.pip : a.pack < b.pack;
    });
    const int n = (int)cfg.size();
    std::vector<int8_t> configs((size_t)n * 6);
    std::vector<int32_t> index_of((size_t)n, -1), level((size_t)max_pip + 2, n);    // level[p] = first index of pip count p
    for (int i = n - 1; i >= 0; --i) {
        for (int d = 1; d <= 6; ++d) configs[(size_t)i * 6 + d - 1] = (int8_t)bo_at(cfg[i].pack, d);
        index_of[b1_rank(cfg[i].pack, K)] = i;
        level[cfg[i].pip] = i;
    }
    for (int v : index_of) if (v < 0) { bgx_set_error("bearoff1: the configuration rank is not a bijection"); return BGX_EINVAL; }

    bgx_bearoff1* db = new bgx_bearoff1();
    db->device = device; db->K = K; db->n = n;
    hipError_t err = hipSuccess;
    const size_t row = (size_t)n * kB1T * 4;
    const struct { void** p; size_t bytes; } bufs[] = {
        {(void**)&db->dist, row}, {(void**)&db->surv, row}, {(void**)&db->mean, (size_t)n * 4},
        {(void**)&db->choice, (size_t)n * kBoRolls * 4}, {(void**)&db->configs, configs.size()},
        {(void**)&db->index_of, (size_t)n * 4}, {(void**)&db->err, 16}};
    for (const auto& b : bufs) if (err == hipSuccess) err = hipMalloc(b.p, b.bytes);
    if (err != hipSuccess) { bgx_bearoff1_destroy(db); return bgx_internal_fail(err, BGX_ENOMEM); }
    int32_t berr = 0;
    const float one = 1.0f;
    // a failure below frees everything again (after the stream has drained)
    auto build = [&]() -> int {
        BGX_CK(hipMemcpyAsync(db->configs, configs.data(), configs.size(), hipMemcpyHostToDevice, s));
        BGX_CK(hipMemcpyAsync(db->index_of, index_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemsetAsync(db->err, 0, 16, s));
        // the empty configuration: D = S = (1, 0, ...), mean 0, every choice itself
        BGX_CK(hipMemsetAsync(db->dist, 0, row, s));
        BGX_CK(hipMemsetAsync(db->surv, 0, row, s));
        BGX_CK(hipMemsetAsync(db->mean, 0, (size_t)n * 4, s));
        BGX_CK(hipMemsetAsync(db->choice, 0, (size_t)n * kBoRolls * 4, s));
        BGX_CK(hipMemcpyAsync(db->dist, &one, 4, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemcpyAsync(db->surv, &one, 4, hipMemcpyHostToDevice, s));
        for (int p = 1; p <= max_pip; ++p) {
            const int a0 = level[p], cnt = level[p + 1] - a0;       // every pip count occurs
            if (cnt <= 0) continue;
            hipLaunchKernelGGL(k_b1_choice, dim3((cnt + 63) / 64, kBoRolls), dim3(64), 0, s, db->configs, db->index_of,
                               db->mean, K, a0, cnt, db->choice, db->err);
            hipLaunchKernelGGL(k_b1_dist, dim3((cnt + 7) / 8), dim3(256), 0, s, db->choice, a0, cnt, db->dist, db->surv,
                               db->mean, db->err);
        }
        BGX_CK_LAUNCH();
        BGX_CK(hipMemcpyAsync(&berr, db->err, 4, hipMemcpyDeviceToHost, s));
        BGX_CK(hipStreamSynchronize(s));
        if (berr) {
            bgx_set_error(berr & kErrPlay ? "bearoff1: a configuration without a play"
                                          : "bearoff1: a distribution does not end within its 32 entries");
            return BGX_EOVERFLOW;
        }
        return BGX_OK;
    };
    const int rc = build();
    if (rc != BGX_OK) { (void)hipStreamSynchronize(s); bgx_bearoff1_destroy(db); return rc; }
    *out = db;
    return BGX_OK;
}

int bgx_bearoff1_buffers_get(bgx_bearoff1* db, bgx_bearoff1_buffers* out) {
    if (!db || !out) return BGX_EINVAL;
    out->dist = db->dist; out->surv = db->surv; out->mean = db->mean; out->choice = db->choice;
    out->configs = db->configs; out->n = db->n; out->max_checkers = db->K;
    return BGX_OK;
}

int bgx_bearoff1_lookup(const bgx_bearoff1* db, const uint8_t* records_dev, int32_t n, uint8_t* in_db_out,
                        float* win_out, void* stream) {
    if (!db || n < 0 || (n > 0 && (!records_dev || !in_db_out)) || ((uintptr_t)records_dev & 15)) return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipLaunchKernelGGL(k_b1_lookup, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, n, db->K,
                       db->index_of, db->dist, db->surv, in_db_out, win_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_bearoff1_act(bgx_engine* e, const bgx_bearoff1* db, const uint8_t* lane_sel_dev, int32_t* act_inout,
                     uint8_t* in_db_out, void* stream) {
    if (!e || !db || !act_inout || e->device != db->device) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    EngineCall call(e, s);
    BGX_CK(call.err);
    hipLaunchKernelGGL(k_b1_act, dim3((e->a.B + 255) / 256), dim3(256), 0, s, e->a.lanes, e->a.moves, e->a.B,
                       e->a.max_moves, lane_sel_dev, db->K, db->index_of, db->dist, db->surv, act_inout, in_db_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_bearoff1_cut(const bgx_bearoff1* db, const uint8_t* records_dev, const uint8_t* starts_dev,
                             const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                             int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cut_tally_dev,
                             int64_t* active_dev, uint8_t* reset_mask_out, void* stream) {
    if (!db || !records_dev || !starts_dev || !group_dev || n <= 0 || n_groups <= 0 || games_per_lane < 0 ||
        !games_done_dev || !plies_dev || !sel_dev || !cut_tally_dev || !active_dev || !reset_mask_out ||
        ((uintptr_t)records_dev & 15))
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_b1_cut, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, starts_dev,
                       group_dev, n, n_groups, games_per_lane, db->K, db->index_of, db->dist, db->surv, games_done_dev,
                       plies_dev, sel_dev, cut_tally_dev, active_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"

#endif  // part 2
