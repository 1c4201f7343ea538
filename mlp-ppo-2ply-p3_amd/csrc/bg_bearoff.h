// bg_bearoff.h — the exact two-sided bearoff database (include/bgx.h
// "bearoff database"; bgx/bearoff.py drives it).  Included by bg_engine.hip only.
//
// A configuration is one side's six counts c[d-1], d = 1..6 = checkers at distance d from
// bearing off (PLAYER1: point 24 - d; PLAYER2: point d - 1), sum <= K <= 8.  In the code it is
// a `pack`: count d in nibble d - 1 of a uint32.  The n = C(K+6, 6) configurations are indexed
// by (pip count, base-9 key) ascending, so index 0 is the empty one and every pip count is a
// contiguous range; rank_of int16[9^6] maps the base-9 key sum_d c[d-1] 9^(d-1) to the index.
//
// Part 1 (plain C++, host and device): the one-die plays and the successor sets, following the
// reference's enumeration order for order (handle_moves.py:109-310 + the max-length filter,
// get_all_moves.py:9-94) on a pure bearoff board, where the opponent never blocks or is hit.
// Part 2 (device): the build, lookup, perfect-play and rollout-cut kernels and their C entry
// points.  BGX_BEAROFF_HOST_ONLY (a host test program, any C++ compiler) takes part 1 alone;
// BGX_BEAROFF_PART1_ONLY does so in a device translation unit (bg_bearoff1.h).
#pragma once
#include <stdint.h>

#ifdef BGX_BEAROFF_HOST_ONLY
#define BO_HD inline
#else
#define BO_HD __host__ __device__ __forceinline__
#endif

namespace bg {

constexpr int kBoMaxK = 8;
constexpr int kBoKeys = 531441;            // 9^6
constexpr int kBoRolls = 21;
constexpr int kBoSetCap = 64;              // a successor set's room (largest measured: 55 at K = 8)

BO_HD uint32_t bo_one(int d) { return 1u << (4 * (d - 1)); }
BO_HD int bo_at(uint32_t pack, int d) { return (int)((pack >> (4 * (d - 1))) & 15u); }
BO_HD int bo_key(uint32_t pack) {
    int key = 0;
    for (int d = 6; d >= 1; --d) key = key * 9 + bo_at(pack, d);
    return key;
}
// roll r of the 21 in bgx_two_ply's order: (1,1), (1,2), ..., (1,6), (2,2), ..., (6,6)
BO_HD void bo_roll(int r, int& r0, int& r1) {
    int a = 1;
    while (r >= 7 - a) { r -= 7 - a; ++a; }
    r0 = a; r1 = a + r;
}

// get_moves_bear_off (move_logic.py:140-255) with die d: the configurations after one
// sub-move, at most 7 (5 moves inside the home board, 2 bear-offs).  None from the empty one.
BO_HD int bo_moves(uint32_t pack, int d, uint32_t* out) {
    int n = 0;
    if (pack == 0u) return 0;
    int far = 0;
    for (int s = 1; s <= 6; ++s) {
        if (bo_at(pack, s) == 0) continue;
        far = s;
        if (s > d) out[n++] = pack - bo_one(s) + bo_one(s - d);
    }
    if (far <= d) out[n++] = pack - bo_one(far);                            // the farthest checker
    else if (bo_at(pack, d) > 0) out[n++] = pack - bo_one(d);               // the die's own point
    return n;
}

// A set of (configuration, sub-move count) in insertion order, first insertion kept
// (add_unique_board).  ovf: it outgrew kBoSetCap.
struct BoSet {
    uint32_t pack[kBoSetCap];
    uint8_t len[kBoSetCap];
    int n;
    bool ovf;
};
BO_HD void bo_add(BoSet& s, uint32_t pack, int len) {
    for (int i = 0; i < s.n; ++i) if (s.pack[i] == pack) return;
    if (s.n == kBoSetCap) { s.ovf = true; return; }
    s.pack[s.n] = pack; s.len[s.n] = (uint8_t)len; ++s.n;
}

// handle_non_doubles with dice (d1, d2) in that order
BO_HD void bo_pass(BoSet& s, uint32_t pack, int d1, int d2) {
    uint32_t first[8], second[8];
    const int n1 = bo_moves(pack, d1, first);
    bool exists = false;
    for (int i = 0; i < n1 && !exists; ++i) exists = bo_moves(first[i], d2, second) > 0;
    for (int i = 0; i < n1; ++i) {
        if (!exists) { bo_add(s, first[i], 1); continue; }
        const int n2 = bo_moves(first[i], d2, second);
        for (int j = 0; j < n2; ++j) bo_add(s, second[j], 2);
    }
}

// handle_doubles
BO_HD void bo_doubles(BoSet& s, uint32_t pack, int d) {
    uint32_t l1[8], l2[8], l3[8], l4[8];
    bool got4 = false;
    const int n1 = bo_moves(pack, d, l1);
    for (int i = 0; i < n1; ++i) {
        const int n2 = bo_moves(l1[i], d, l2);
        if (n2 == 0 && !got4) bo_add(s, l1[i], 1);
        for (int j = 0; j < n2; ++j) {
            const int n3 = bo_moves(l2[j], d, l3);
            if (n3 == 0 && !got4) bo_add(s, l2[j], 2);
            for (int k = 0; k < n3; ++k) {
                const int n4 = bo_moves(l3[k], d, l4);
                if (n4 == 0 && !got4) bo_add(s, l3[k], 3);
                for (int m = 0; m < n4; ++m) { bo_add(s, l4[m], 4); got4 = true; }
            }
        }
    }
}

// The distinct configurations `pack` can reach with a legal play of (r0, r1), compacted to
// s.pack[0 .. return): get_all_possible_moves and the max-length filter.  A roll that cannot
// be played (only the empty configuration has one) gives the configuration itself.
BO_HD int bo_successors(uint32_t pack, int r0, int r1, BoSet& s) {
    s.n = 0; s.ovf = false;
    if (r0 != r1) {
        const int hi = r0 > r1 ? r0 : r1, lo = r0 > r1 ? r1 : r0;
        bo_pass(s, pack, hi, lo);
        if (!(s.n == 1 && s.len[0] == 1)) bo_pass(s, pack, lo, hi);
    } else {
        bo_doubles(s, pack, r0);
    }
    int maxn = 0, m = 0;
    for (int i = 0; i < s.n; ++i) maxn = s.len[i] > maxn ? s.len[i] : maxn;
    for (int i = 0; i < s.n; ++i) if (s.len[i] == maxn) s.pack[m++] = s.pack[i];
    if (m == 0) s.pack[m++] = pack;
    return m;
}

}  // namespace bg

#if !defined(BGX_BEAROFF_HOST_ONLY) && !defined(BGX_BEAROFF_PART1_ONLY)
// ======================================================================== part 2 ==
#include "bg_rollout.h"

// The object behind the C ABI's opaque bgx_bearoff*: device buffers, fixed after creation.
struct bgx_bearoff {
    int device{0};
    int K{0}, n{0};
    float* table{nullptr};         // [n][n] W
    int8_t* configs{nullptr};      // [n][6]
    int32_t* succ_off{nullptr};    // [n * 21 + 1]
    int32_t* succ{nullptr};        // [succ_off[n * 21]] configuration indices, ascending per set
    int16_t* rank_of{nullptr};     // [9^6] key -> index, -1 = more than K checkers
    int32_t* level{nullptr};       // [6 K + 2] first index of each pip count; then n pip counts
    int32_t* err{nullptr};         // build errors: 1 = a successor set outgrew kBoSetCap, 2 = an unknown key
};

namespace {

using namespace bg;

__device__ __forceinline__ uint32_t bo_pack_of(const int8_t* c) {
    uint32_t p = 0;
    #pragma unroll
    for (int d = 1; d <= 6; ++d) p |= (uint32_t)(c[d - 1] & 15) << (4 * (d - 1));
    return p;
}

// ---- build: count, scan, fill (one thread per (configuration, roll)), then the levels ----
// FILL 0: succ_off[i + 1] = the set's size.  FILL 1: the set's indices, ascending, at succ_off[i].
template <int FILL>
__global__ __launch_bounds__(128) void k_bo_succ(const int8_t* __restrict__ configs, const int16_t* __restrict__ rank_of,
                                                  int n, int32_t* succ_off, int32_t* succ, int32_t* err) {
    const int i = blockIdx.x * 128 + threadIdx.x;
    if (i >= n * kBoRolls) return;
    const int c = i / kBoRolls, r = i - c * kBoRolls;
    int r0, r1;
    bo_roll(r, r0, r1);
    BoSet s;
    const int m = bo_successors(bo_pack_of(configs + (size_t)c * 6), r0, r1, s);
    if (s.ovf) atomicOr(err, 1);
    if (FILL == 0) {
        if (i == 0) succ_off[0] = 0;
        succ_off[i + 1] = m;
        return;
    }
    int32_t* out = succ + succ_off[i];
    if (succ_off[i + 1] - succ_off[i] != m) { atomicOr(err, 4); return; }
    for (int j = 0; j < m; ++j) {                       // insertion sort into the set's own segment
        int v = (int)rank_of[bo_key(s.pack[j])];
        if (v < 0) { atomicOr(err, 2); v = 0; }
        int k = j;
        for (; k > 0 && out[k - 1] > v; --k) out[k] = out[k - 1];
        out[k] = v;
    }
}

// inclusive scan of a[1 .. m] in place (a[0] = 0 stays): one block, each thread a run of
// consecutive entries, the runs' sums scanned in LDS
__global__ __launch_bounds__(1024) void k_bo_scan(int32_t* a, int m) {
    __shared__ int sums[1024];
    const int t = threadIdx.x, per = (m + 1023) / 1024;
    const int lo = 1 + t * per, hi = min(lo + per, m + 1);
    int s = 0;
    for (int j = lo; j < hi; ++j) s += a[j];
    sums[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? sums[t - o] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int run = sums[t] - s;
    for (int j = lo; j < hi; ++j) { run += a[j]; a[j] = run; }
}

// boundary rows: W[a][empty] = 0 (the opponent has already won), W[empty][b] = 1 for b != empty
__global__ __launch_bounds__(256) void k_bo_init(float* W, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    W[(size_t)i * n] = 0.0f;
    if (i > 0) W[i] = 1.0f;
}

// One level: every state (a, b) of total pip count t.  Block y = configuration a0 + y (pip
// count pa in [1, t - 1]), threads over the b of pip count t - pa.  W[b][a'] has a smaller
// total, so it was written by an earlier launch.  Each product and sum is rounded once, the
// rolls in order from 0: a numpy float32 loop gives the same bits.
__global__ __launch_bounds__(128) void k_bo_level(float* W, const int32_t* __restrict__ succ_off,
                                                   const int32_t* __restrict__ succ, const int32_t* __restrict__ level,
                                                   int n, int max_pip, int t, int a0) {
    const int a = a0 + (int)blockIdx.y;
    if (a >= n) return;
    const int pb = t - level[max_pip + 2 + a];
    if (pb < 1 || pb > max_pip) return;
    const int b = level[pb] + (int)blockIdx.x * 128 + (int)threadIdx.x;
    if (b >= level[pb + 1]) return;
    const float* Wb = W + (size_t)b * n;
    const int32_t* off = succ_off + (size_t)a * kBoRolls;
    float acc = 0.0f;
    int r = 0;
    for (int r0 = 1; r0 <= 6; ++r0) {
        for (int r1 = r0; r1 <= 6; ++r1, ++r) {
            float w = -1.0f;
            for (int j = off[r]; j < off[r + 1]; ++j) {
                const int ap = succ[j];
                w = fmaxf(w, ap == 0 ? 1.0f : __fsub_rn(1.0f, Wb[ap]));
            }
            acc = __fadd_rn(acc, __fmul_rn(r0 == r1 ? 1.0f / 36.0f : 2.0f / 36.0f, w));
        }
    }
    W[(size_t)a * n + b] = acc;
}

// ---- lookup ----
// The table test on one 64-byte record (held in registers: constant indices only).  In the
// table: game not over, both bars empty, each side 1..K checkers, all on its own home points,
// points + off == 15.  Gives the two sides' configuration indices.
struct BoRec {
    uint4 q[4];
    __device__ __forceinline__ void load(const uint8_t* recs, int i) {
        #pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = ((const uint4*)recs)[(size_t)i * 4 + k];
    }
    __device__ __forceinline__ int at(int j) const { return (int)((const uint8_t*)q)[j]; }
};

__device__ __forceinline__ bool bo_in_table(const BoRec& rec, int K, const int16_t* __restrict__ rank_of, int idx[2]) {
    int out0 = 0, out1 = 0, home0 = 0, home1 = 0, key0 = 0, key1 = 0;
    #pragma unroll
    for (int p = 0; p < 18; ++p) { out0 += rec.at(p); out1 += rec.at(24 + 6 + p); }
    #pragma unroll
    for (int d = 6; d >= 1; --d) {
        home0 += rec.at(24 - d); home1 += rec.at(24 + d - 1);
        key0 = key0 * 9 + rec.at(24 - d); key1 = key1 * 9 + rec.at(24 + d - 1);
    }
    const bool in = rec.at(R_OVER) == 0 && rec.at(48) == 0 && rec.at(49) == 0 && out0 == 0 && out1 == 0 &&
                    home0 >= 1 && home0 <= K && home1 >= 1 && home1 <= K && home0 + rec.at(50) == 15 &&
                    home1 + rec.at(51) == 15;
    if (!in) return false;                     // only now are the keys known to be below 9^6
    idx[0] = (int)rank_of[key0];
    idx[1] = (int)rank_of[key1];
    return idx[0] > 0 && idx[1] > 0;
}

__global__ __launch_bounds__(256) void k_bo_lookup(const uint8_t* __restrict__ recs, int n_rec, int K, int n,
                                                    const int16_t* __restrict__ rank_of, const float* __restrict__ W,
                                                    uint8_t* in_db, float* win) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rec) return;
    BoRec rec;
    rec.load(recs, i);
    int idx[2];
    const bool in = bo_in_table(rec, K, rank_of, idx);
    in_db[i] = in ? 1 : 0;
    if (in && win) {
        const int m = rec.at(R_CUR) & 1;
        win[i] = W[(size_t)idx[m] * n + idx[1 - m]];
    }
}

// ---- perfect play: one thread per lane over the engine's own move list ----
__global__ __launch_bounds__(256) void k_bo_act(const uint8_t* __restrict__ recs, const uint64_t* __restrict__ moves,
                                                 int B, int max_moves, const uint8_t* __restrict__ sel, int K, int n,
                                                 const int16_t* __restrict__ rank_of, const float* __restrict__ W,
                                                 int32_t* act, uint8_t* in_db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if (sel && sel[i] == 0) {
        if (in_db) in_db[i] = 0;
        return;
    }
    BoRec rec;
    rec.load(recs, i);
    int idx[2];
    const bool in = bo_in_table(rec, K, rank_of, idx);
    if (in_db) in_db[i] = in ? 1 : 0;
    const int nm = min(rec.at(R_NM0) | (rec.at(R_NM1) << 8), max_moves);
    if (!in || nm <= 0) return;
    const int mover = rec.at(R_CUR) & 1;
    uint32_t own = 0;
    #pragma unroll
    for (int d = 1; d <= 6; ++d) own |= (uint32_t)(mover == 0 ? rec.at(24 - d) : rec.at(24 + d - 1)) << (4 * (d - 1));
    const float* Wopp = W + (size_t)idx[1 - mover] * n;
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
            const int ap = pack == 0u ? 0 : (int)rank_of[bo_key(pack)];
            if (ap == 0) v = 1.0f;
            else if (ap > 0) v = __fsub_rn(1.0f, Wopp[ap]);
        }
        if (v > best) { best = v; arg = m; }
    }
    act[i] = arg;
}

// ---- rollout cut (bgx_rollout_bearoff_cut), after k_rollout_begin / k_rollout_advance ----
// bg_rollout.h's table_cut with this table's test and its exact win probability.  Per wave one
// add per (group, field) it holds cut lanes of; integer adds commute.
__global__ __launch_bounds__(256) void k_bo_cut(const uint8_t* __restrict__ recs, const uint8_t* __restrict__ starts,
                                                 const int32_t* __restrict__ group, int n_rec, int n_groups, int G,
                                                 int K, int n, const int16_t* __restrict__ rank_of,
                                                 const float* __restrict__ W, int32_t* games_done, int32_t* plies,
                                                 uint8_t* sel, int64_t* cut_tally, int64_t* active, uint8_t* mask) {
    table_cut(starts, group, n_rec, n_groups, G, games_done, plies, sel, cut_tally, active, mask,
              [&](int i, int* cur, float* w) {
        BoRec rec;
        rec.load(recs, i);
        int idx[2];
        if (!bo_in_table(rec, K, rank_of, idx)) return false;
        *cur = rec.at(R_CUR);
        const int m = *cur & 1;
        *w = W[(size_t)idx[m] * n + idx[1 - m]];
        return true;
    });
}

// the host's list of configurations: (pip count, base-9 key) ascending
struct BoConfig { int pip, key; int8_t c[6]; };

}  // namespace

extern "C" {

int bgx_bearoff_destroy(bgx_bearoff* db) {
    if (!db) return BGX_EINVAL;
    (void)hipSetDevice(db->device);
    (void)hipDeviceSynchronize();                     // nothing in flight reads the buffers
    for (void* p : {(void*)db->table, (void*)db->configs, (void*)db->succ_off, (void*)db->succ, (void*)db->rank_of,
                    (void*)db->level, (void*)db->err})
        if (p) (void)hipFree(p);
    delete db;
    return BGX_OK;
}

int bgx_bearoff_create(int device, int32_t max_checkers, void* stream, bgx_bearoff** out) {
    if (!out || max_checkers < 1 || max_checkers > kBoMaxK) return BGX_EINVAL;
    BGX_CK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    const int K = max_checkers, max_pip = 6 * K;
    std::vector<BoConfig> cfg;
    int c[6];
    for (c[0] = 0; c[0] <= K; ++c[0]) for (c[1] = 0; c[0] + c[1] <= K; ++c[1])
    for (c[2] = 0; c[0] + c[1] + c[2] <= K; ++c[2]) for (c[3] = 0; c[0] + c[1] + c[2] + c[3] <= K; ++c[3])
    for (c[4] = 0; c[0] + c[1] + c[2] + c[3] + c[4] <= K; ++c[4])
    for (c[5] = 0; c[0] + c[1] + c[2] + c[3] + c[4] + c[5] <= K; ++c[5]) {
        BoConfig x{0, 0, {}};
        for (int d = 6; d >= 1; --d) { x.pip += d * c[d - 1]; x.key = x.key * 9 + c[d - 1]; x.c[d - 1] = (int8_t)c[d - 1]; }
        cfg.push_back(x);
    }
    std::sort(cfg.begin(), cfg.end(), [](const BoConfig& a, const BoConfig& b) {
        return a.pip != b.pip ? a.pip < b.pip : a.key < b.key;
    });
    const int n = (int)cfg.size(), m = n * kBoRolls;
    std::vector<int8_t> configs((size_t)n * 6);
    std::vector<int16_t> rank((size_t)kBoKeys, (int16_t)-1);
    std::vector<int32_t> level((size_t)max_pip + 2 + n, n);      // level[p] = first index of pip count p
    int widest = 1;
    for (int i = n - 1; i >= 0; --i) {
        for (int d = 0; d < 6; ++d) configs[(size_t)i * 6 + d] = cfg[i].c[d];
        rank[cfg[i].key] = (int16_t)i;
        level[cfg[i].pip] = i;
        level[max_pip + 2 + i] = cfg[i].pip;
    }
    for (int p = max_pip; p >= 0; --p) widest = std::max(widest, level[p + 1] - level[p]);   // every pip count occurs

    bgx_bearoff* db = new bgx_bearoff();
    db->device = device; db->K = K; db->n = n;
    hipError_t err = hipSuccess;
    const struct { void** p; size_t bytes; } bufs[] = {
        {(void**)&db->table, (size_t)n * n * 4}, {(void**)&db->configs, configs.size()},
        {(void**)&db->succ_off, ((size_t)m + 1) * 4}, {(void**)&db->rank_of, rank.size() * 2},
        {(void**)&db->level, level.size() * 4}, {(void**)&db->err, 16}};
    for (const auto& b : bufs) if (err == hipSuccess) err = hipMalloc(b.p, b.bytes);
    if (err != hipSuccess) { bgx_bearoff_destroy(db); return bgx_internal_fail(err, BGX_ENOMEM); }
    int rc = BGX_OK;
    int32_t total = 0, berr = 0;
    // a failure below frees everything again (after the stream has drained)
    auto build = [&]() -> int {
        BGX_CK(hipMemcpyAsync(db->configs, configs.data(), configs.size(), hipMemcpyHostToDevice, s));
        BGX_CK(hipMemcpyAsync(db->rank_of, rank.data(), rank.size() * 2, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemcpyAsync(db->level, level.data(), level.size() * 4, hipMemcpyHostToDevice, s));
        BGX_CK(hipMemsetAsync(db->err, 0, 16, s));
        BGX_CK(hipMemsetAsync(db->table, 0, (size_t)n * n * 4, s));
        hipLaunchKernelGGL(k_bo_succ<0>, dim3((m + 127) / 128), dim3(128), 0, s, db->configs, db->rank_of, n,
                           db->succ_off, (int32_t*)nullptr, db->err);
        hipLaunchKernelGGL(k_bo_scan, dim3(1), dim3(1024), 0, s, db->succ_off, m);
        BGX_CK_LAUNCH();
        BGX_CK(hipMemcpyAsync(&total, db->succ_off + m, 4, hipMemcpyDeviceToHost, s));
        BGX_CK(hipStreamSynchronize(s));                  // the successor table's size
        if (total < m) { bgx_set_error("bearoff: successor count"); return BGX_EDEVICE; }
        if (hipMalloc((void**)&db->succ, (size_t)total * 4) != hipSuccess) return bgx_internal_fail(hipGetLastError(), BGX_ENOMEM);
        hipLaunchKernelGGL(k_bo_succ<1>, dim3((m + 127) / 128), dim3(128), 0, s, db->configs, db->rank_of, n,
                           db->succ_off, db->succ, db->err);
        hipLaunchKernelGGL(k_bo_init, dim3((n + 255) / 256), dim3(256), 0, s, db->table, n);
        for (int t = 2; t <= 2 * max_pip; ++t) {
            const int p_lo = std::max(1, t - max_pip), p_hi = std::min(max_pip, t - 1);
            const int a0 = level[p_lo], a1 = level[p_hi + 1];
            if (a1 <= a0) continue;
            hipLaunchKernelGGL(k_bo_level, dim3((widest + 127) / 128, a1 - a0), dim3(128), 0, s, db->table,
                               db->succ_off, db->succ, db->level, n, max_pip, t, a0);
        }
        BGX_CK_LAUNCH();
        BGX_CK(hipMemcpyAsync(&berr, db->err, 4, hipMemcpyDeviceToHost, s));
        BGX_CK(hipStreamSynchronize(s));
        if (berr) { bgx_set_error("bearoff: a successor set outgrew its room or left the table"); return BGX_EOVERFLOW; }
        return BGX_OK;
    };
    rc = build();
    if (rc != BGX_OK) { (void)hipStreamSynchronize(s); bgx_bearoff_destroy(db); return rc; }
    *out = db;
    return BGX_OK;
}

int bgx_bearoff_buffers_get(bgx_bearoff* db, bgx_bearoff_buffers* out) {
    if (!db || !out) return BGX_EINVAL;
    out->table = db->table; out->configs = db->configs; out->succ_off = db->succ_off; out->succ = db->succ;
    out->n = db->n; out->max_checkers = db->K;
    return BGX_OK;
}

int bgx_bearoff_lookup(const bgx_bearoff* db, const uint8_t* records_dev, int32_t n, uint8_t* in_db_out,
                       float* win_out, void* stream) {
    if (!db || n < 0 || (n > 0 && (!records_dev || !in_db_out)) || ((uintptr_t)records_dev & 15)) return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipLaunchKernelGGL(k_bo_lookup, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, n, db->K,
                       db->n, db->rank_of, db->table, in_db_out, win_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_bearoff_act(bgx_engine* e, const bgx_bearoff* db, const uint8_t* lane_sel_dev, int32_t* act_inout,
                    uint8_t* in_db_out, void* stream) {
    if (!e || !db || !act_inout || e->device != db->device) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    EngineCall call(e, s);
    BGX_CK(call.err);
    hipLaunchKernelGGL(k_bo_act, dim3((e->a.B + 255) / 256), dim3(256), 0, s, e->a.lanes, e->a.moves, e->a.B,
                       e->a.max_moves, lane_sel_dev, db->K, db->n, db->rank_of, db->table, act_inout, in_db_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_bearoff_cut(const bgx_bearoff* db, const uint8_t* records_dev, const uint8_t* starts_dev,
                            const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                            int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cut_tally_dev,
                            int64_t* active_dev, uint8_t* reset_mask_out, void* stream) {
    if (!db || !records_dev || !starts_dev || !group_dev || n <= 0 || n_groups <= 0 || games_per_lane < 0 ||
        !games_done_dev || !plies_dev || !sel_dev || !cut_tally_dev || !active_dev || !reset_mask_out ||
        ((uintptr_t)records_dev & 15))
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_bo_cut, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, starts_dev,
                       group_dev, n, n_groups, games_per_lane, db->K, db->n, db->rank_of, db->table, games_done_dev,
                       plies_dev, sel_dev, cut_tally_dev, active_dev, reset_mask_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

}  // extern "C"
#endif  // part 2
