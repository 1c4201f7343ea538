// bg_engine.hip — MI355X (gfx950) self-play engine: lane records in HBM, one
// wavefront per game, move enumeration + board apply + dice + encoder as HIP
// kernels, exported through the C ABI declared in include/bgx.h.
//
// Data layout in HBM (per engine, batch B, max_moves M):
//   lanes   [B][64]  u8   board52 | cur | roll[2] | game_over | match_over |
//                         score[2] | need | n_moves(i16) | flags | pad
//   moves   [B][M]   u64  current legal-move list (first M of the filtered list)
//   n_total [B]      i32  untruncated count
//   mt      [B][640] u32  per-lane numpy-legacy MT19937 state (+ index at [624])
//   ctr     [B]      u64  per-lane Philox draw counters
//   starts  [B][64]  u8   start table (bgx_engine_set_starts): the record a lane resets to
//                         instead of the opening while a table is set; byte 63 = record valid
// Kernels are launched one 64-thread workgroup (= one wave) per game.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "bg_engine.h"
#include "bg_rollout.h"
#include "bg_debug.h"
#include "bg_host.h"
#include <map>

using namespace bg;

namespace {

constexpr int kMaxRegions = BGX_MAX_COPY_REGIONS;
using namespace bg;

// -------------------------------------------------------------- kernels --
// PHASE 0: apply + advance fused (per-lane dice); 1: apply only; 2: advance only.
// One lane's step: apply (PHASE 0/1), roll + movegen (PHASE 0/2), record, the
// next dispatch class's pre-class byte (the order pass resolves it).
// DICE: the dice mode as a compile-time constant, or -1 = A.dice_mode (roll_lane).
// BLK (the split launch of a step with a dispatch order): `at` is the wave's dispatch
// position, and the lane, its action, the chosen move and the counter are in the step block
// k_step_gather laid there, addressed by blockIdx alone; the record follows from the lane:
// two levels of loads.  Otherwise `at` is the lane and the chain is (perm ->) lane ->
// record, action, counter -> move: three.  Every store goes to the lane's own arrays.
template <int PHASE, int LOG, int MEMO, bool NO_DOUBLES = false, int DICE = -1, bool BLK = false>
__device__ __forceinline__ void step_lane(const Args& A, int at, uint4* tab, uint4* memo, const int32_t* actions,
                                          float* obs, float* reward, uint8_t* done, int32_t* info) {
    const uint64_t t0 = A.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    int gi = at, bv, act;
    uint64_t ctr, chosen = 0;
    if (BLK) {
        const uint8_t* b = A.blk + (size_t)at * kBlkBytes;
        // the header through the constant address space (no kernel of the launch writes the
        // blocks): wave-uniform, so its six words are scalar loads
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const uintptr_t hp = (uintptr_t)b;
        const u32x4 h = *(const __attribute__((address_space(4))) u32x4*)hp;
        const u32x2 c = *(const __attribute__((address_space(4))) u32x2*)(hp + 16);
        // the lane in a register of its own: it lives to the wave's end, and left in the
        // loaded four-register tuple it cost the heavy kernel 26 more SGPR spills (measured
        // with the record in the block as well, profiles/step_block)
        asm volatile("s_mov_b32 %0, %1" : "=s"(gi) : "s"(h.x));
        bv = load_rec(A, gi);
        act = (int)h.y;
        chosen = (uint64_t)h.z | ((uint64_t)h.w << 32);
        ctr = (uint64_t)c.x | ((uint64_t)c.y << 32);
    } else {
        // issue the independent loads together (record, action, dice counter)
        bv = load_rec(A, gi);
        act = PHASE != 2 ? (int)ufl((uint32_t)actions[gi]) : 0;
        ctr = (DICE >= 0 ? DICE : A.dice_mode) == BGX_DICE_PHILOX ? A.ctr[gi] : 0;
    }
    if (PHASE != 2) bv = apply_lane<BLK>(bv, gi, act, A, reward, done, info, chosen);
    if (PHASE != 1) {
        bv = advance_lane<LOG, MEMO == 2 ? 2 : 0, NO_DOUBLES, DICE>(bv, gi, A, tab, memo, &ctr);
        if (obs) write_obs(bv, obs + (size_t)gi * 198);
    }
    store_rec(A, gi, bv);
    if (PHASE == 0 && A.pre) {
        const int p = pre_class(bv);
        if (lane_id() == 0) A.pre[gi] = (uint8_t)p;
    }
    if (A.stamps && lane_id() == 0) {
        A.stamps[2 * gi] = t0;
        A.stamps[2 * gi + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// `base` offsets blockIdx into the dispatch order.  MEMO: 0 = no revisit memo,
// 1 = separate memo tables (10 KB of LDS), 2 = memo inside the dedup table.
// NO_DOUBLES: doubles rolls are deferred to the overflow tiers (light launch).
// DICE: BGX_DICE_PHILOX for the split launch of a Philox engine (no MT19937 or shared-dice
// code in the two kernels where the step's time goes), -1 = every mode (Args::dice_mode).
// BLK: the wave starts from the step block of its dispatch position (A.blk, step_lane).
template <int PHASE, int LOG, int MEMO = 1, bool NO_DOUBLES = false, int WPE = 1, int DICE = -1, bool BLK = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE))) void k_step(Args A, const int32_t* actions, float* obs, float* reward, uint8_t* done,
                                             int32_t* info, int base) {
    __shared__ uint4 tab[1 << LOG];
    __shared__ uint4 memo_[MEMO == 1 ? kMemoSlots : 1];
    uint4* memo = MEMO == 1 ? memo_ : MEMO == 2 ? tab : nullptr;
    const int bi = (int)blockIdx.x + base;
    const int at = BLK ? bi : A.perm ? (int)ufl((uint32_t)A.perm[bi]) : lane_of_block(A, bi);
    step_lane<PHASE, LOG, MEMO, NO_DOUBLES, DICE, BLK>(A, at, tab, memo, actions, obs, reward, done, info);
}

template <int LOG>
__global__ __launch_bounds__(64) void k_reset(Args A, const uint8_t* lane_mask, float* obs, int mark_only) {
    __shared__ uint4 tab[1 << LOG];
    __shared__ uint4 memo[kMemoSlots];
    const int gi = blockIdx.x;
    int bv = load_rec(A, gi);
    uint64_t ctr = A.dice_mode == BGX_DICE_PHILOX ? A.ctr[gi] : 0;
    const bool sel = lane_mask == nullptr || ufl(lane_mask[gi]) != 0u;
    if (sel) bv = wr(bv, R_NEED, NEED_RESET);
    if (!mark_only) {
        bv = advance_lane<LOG>(bv, gi, A, tab, memo, &ctr);
        if (obs) write_obs(bv, obs + (size_t)gi * 198);
        if (A.pre) {
            const int p = pre_class(bv);
            if (lane_id() == 0) A.pre[gi] = (uint8_t)p;
        }
    }
    store_rec(A, gi, bv);
}

// Next dispatch order = lanes grouped by predicted class (class 0 first), in
// lane order within a class: a two-pass counting sort (pass 1 also resolves the
// classes; it counts blocks of 256 lanes, pass 2 places blocks of 1024).  perm
// is a full permutation of 0..B-1 whatever pre and the counters hold.
//
// XCD-aware form (B % 128 == 0): the lanes are split into 8 sub-lists by
// x = (lane >> 4) & 7 (runs of 16 lanes), each sub-list is class-sorted on its
// own, and position 8k + x holds the k-th lane of sub-list x.  Blocks b and
// b + 8 of a launch run on one XCD (round-robin placement; the launch bases are
// multiples of 8), so every 16-lane run -- one 64-B line of the reward / action
// / n_total arrays, one 128-B line of the Philox counters, 8 lane records -- is
// stepped by ONE XCD per launch and its partial-line loads and stores meet in
// that XCD's L2 instead of crossing all eight.  The 8 sub-lists have nearly the
// same class mix, so the interleave keeps the heaviest-first order.
constexpr int kXcd = 8, kRun = 16;
__device__ __forceinline__ int order_class(const uint8_t* cls, int i, int B) {
    return i < B ? min((int)cls[i], kClasses - 1) : kClasses;     // kClasses = padding, never written
}

// pass 1: thread i resolves lane i's class from the step's pre-class byte and the
// lane's next roll (predict_class: the Philox block as VALU work for 64 lanes per
// instruction, where the step's waves would each run it on their CU's scalar unit),
// leaves the roll in the counter's cache bits for the next roll_lane, and counts:
// cnt[b][x][c] = lanes of class c in sub-list x of block b (x = 0 when !xcd).
// Blocks of kCountThreads lanes, a quarter of pass 2's: the Philox block is a chain of
// dependent multiplies, so the pass is latency-bound and spreads over 4x the CUs.
// Run again with no step between, it finds the same counter (low 48 bits) and
// pre-class byte and writes the same cache word and class.
constexpr int kCountThreads = 256;
__global__ __launch_bounds__(kCountThreads) void k_order_count(const uint8_t* pre, uint8_t* cls, uint64_t* ctr, uint32_t key0,
                                                      uint32_t key1, int32_t* cnt, int B, int32_t* zero_next,
                                                      int xcd) {
    __shared__ int sc[kXcd][kClasses];
    const int t = threadIdx.x, i = blockIdx.x * kCountThreads + t, w = t >> 6;
    if (blockIdx.x == 0 && t < 4) zero_next[t] = 0;     // the next step's overflow counters
    if (t < kXcd * kClasses) sc[t / kClasses][t % kClasses] = 0;
    __syncthreads();
    int c = kClasses;                                   // padding past B: no Philox, never written
    if (i < B) {
        const int p = (int)pre[i];
        const uint64_t cv = (p & kPreOver) ? 0ull : ctr[i];
        uint32_t cache;
        c = predict_class(p, cv, key0, key1, (uint32_t)i, cache);
        if (cache) ctr[i] = (cv & kCtrMask) | ((uint64_t)cache << 48);
        cls[i] = (uint8_t)c;
    }
    #pragma unroll
    for (int k = 0; k < kClasses; ++k) {
        const uint64_t m = __ballot(c == k);
        if (xcd) {
            // the wave's four 16-lane runs belong to sub-lists (4w + s) & 7
            if ((t & 63) < 4) {
                const int s = t & 3;
                const int n = __popcll(m & (0xFFFFull << (16 * s)));
                if (n) atomicAdd(&sc[(4 * w + s) & 7][k], n);
            }
        } else if ((t & 63) == 0 && m) {
            atomicAdd(&sc[0][k], __popcll(m));
        }
    }
    __syncthreads();
    if (t < kXcd * kClasses) cnt[blockIdx.x * kXcd * kClasses + t] = sc[t / kClasses][t % kClasses];
}

// pass 2, at the start of the next step (bgx_step, which knows the actions by then):
// position (within the lane's sub-list) = (lanes of lower classes) + (class-c lanes of
// earlier blocks) + (class-c lanes earlier in this block), written to perm; and with
// BLOCKS the lane's step block (kBlkBytes: lane, action, chosen move, counter) laid at that
// position, so the step wave of dispatch position p starts from blk[p] where it would chase
// perm[p] -> action / counter of the lane -> the move.  Here those levels are in flight for
// a whole block of lanes at once.  Without BLOCKS (the accessor bgx_engine_order between
// two steps) only perm is written.  A block of kGatherThreads lanes (pass 1's block: one
// count row each); thread t resolves lane b * kGatherThreads + t and writes its block with
// two 16-byte stores.
constexpr int kGatherThreads = kCountThreads;
template <bool BLOCKS>
__global__ __launch_bounds__(kGatherThreads) void k_step_gather(const uint8_t* cls, const int32_t* cnt, int32_t* perm,
                                                                int B, int ncnt, int xcd, const uint64_t* moves,
                                                                const uint64_t* ctr, const int32_t* actions,
                                                                int max_moves, uint8_t* blk) {
    constexpr int T = kGatherThreads, NC = kXcd * kClasses, STRIPES = T / NC, PER = T / kCountThreads;
    __shared__ int tot[NC], pre[NC], wsum[T / 64][4][kClasses];
    const int t = threadIdx.x, b = blockIdx.x, w = t >> 6, l = t & 63;
    const int i = b * T + t;
    // the loads nothing here orders: the lane's action and counter, then the move the
    // action names -- read only inside the lane's own list
    int act = 0;
    uint64_t cv = 0, mv = 0;
    if (BLOCKS && i < B) {
        act = actions[i];
        cv = ctr[i];
        const int a = act < 0 ? act + max_moves : act;
        if (a >= 0 && a < max_moves) mv = moves[(size_t)i * max_moves + a];
    }
    if (t < NC) { tot[t] = 0; pre[t] = 0; }
    __syncthreads();
    // the 40 counters summed over pass 1's ncnt blocks (PER of them per block of this
    // pass), in STRIPES strided partial sums per counter
    if (t < NC * STRIPES) {
        const int k = t % NC;
        int a_tot = 0, a_pre = 0;
        for (int j = t / NC; j < ncnt; j += STRIPES) {
            const int v = cnt[j * NC + k];
            a_tot += v;
            a_pre += j < b * PER ? v : 0;
        }
        if (a_tot) atomicAdd(&tot[k], a_tot);
        if (a_pre) atomicAdd(&pre[k], a_pre);
    }
    const int c = order_class(cls, i, B);
    const int s = xcd ? (l >> 4) : 0;                 // the lane's 16-lane run within the wave
    const uint64_t seg = xcd ? (0xFFFFull << (16 * s)) : ~0ull;
    int rank = 0;
    #pragma unroll
    for (int k = 0; k < kClasses; ++k) {
        const uint64_t m = __ballot(c == k);
        if (c == k) rank = __popcll(m & seg & ((1ull << l) - 1ull));
        if (l < 4) wsum[w][l][k] = __popcll(m & (xcd ? (0xFFFFull << (16 * l)) : (l == 0 ? ~0ull : 0ull)));
    }
    __syncthreads();
    if (c < kClasses) {                                   // (padding past B: no position, no block)
        const int x = xcd ? ((4 * w + s) & 7) : 0;
        int pos = pre[x * kClasses + c] + rank;
        for (int k = 0; k < c; ++k) pos += tot[x * kClasses + k];
        // earlier waves of this block holding runs of the same sub-list: w' = w (mod 2)
        for (int v = xcd ? (w & 1) : 0; v < w; v += xcd ? 2 : 1) pos += wsum[v][s][c];
        const int p = xcd ? pos * kXcd + x : pos;
        perm[p] = i;
        if (BLOCKS) {
            uint4* o = (uint4*)(blk + (size_t)p * kBlkBytes);
            o[0] = make_uint4((uint32_t)i, (uint32_t)act, (uint32_t)mv, (uint32_t)(mv >> 32));
            o[1] = make_uint4((uint32_t)cv, (uint32_t)(cv >> 32), 0u, 0u);
        }
    }
}

// SHARED dice: one wave draws every lane's dice from ONE MT stream in lane order
// (VectorizedBackgammonEnv: all envs call np.random.randint on the global state).
__global__ __launch_bounds__(64) void k_shared_dice(Args A) {
    __shared__ uint32_t sh[640];
    Rng rng;
    rng.init_mt(A.mt, sh);
    for (int base = 0; base < A.B; base += 64) {
        const int j = base + lane_id();
        const int needv = j < A.B ? (int)A.lanes[(size_t)j * 64 + R_NEED] : 0;
        const int cnt = A.B - base < 64 ? A.B - base : 64;
        for (int t = 0; t < cnt; ++t) {
            const int need = __builtin_amdgcn_readlane(needv, t);
            if (need == NEED_NONE) continue;
            int r0, r1, starter = 0;
            if (need == NEED_RESET) {
                int a, b;
                do { a = rng.die(); b = rng.die(); } while (a == b);
                starter = a < b ? 1 : 0;
                do { r0 = rng.die(); r1 = rng.die(); } while (r0 == r1);
            } else {
                r0 = rng.die(); r1 = rng.die();
            }
            if (lane_id() == 0) {
                uint8_t* sr = A.shared_rolls + (size_t)(base + t) * 4;
                sr[0] = (uint8_t)r0; sr[1] = (uint8_t)r1; sr[2] = (uint8_t)starter;
            }
        }
    }
    rng.finish(nullptr);
}

// Standalone get_all_possible_moves on arbitrary boards.
template <int LOG>
__global__ __launch_bounds__(64) void k_movegen(const int8_t* boards, const uint8_t* players, const uint8_t* dice,
                                                int n, int cap, int16_t* nmoves, int32_t* ntotal, uint64_t* moves,
                                                int32_t* ovf_count, int32_t* ovf_queue, int cap_unique) {
    __shared__ uint4 tab[1 << LOG];
    __shared__ uint4 memo[kMemoSlots];
    const int gi = blockIdx.x;
    const int l = lane_id();
    const int bv = l < 52 ? (int)boards[(size_t)gi * 52 + l] : 0;
    const int pl = (int)ufl(players[gi]);
    const int r0 = (int)ufl(dice[2 * gi]), r1 = (int)ufl(dice[2 * gi + 1]);
    int total;
    bool ovf;
    int nm = run_movegen<LOG>(bv, pl, r0, r1, moves + (size_t)gi * cap, cap, tab, cap_unique, &total, &ovf, memo);
    if (ovf) {
        if (l == 0) { const int q = atomicAdd(ovf_count, 1); ovf_queue[q] = gi; }
        nm = 0; total = 0;
    }
    if (l == 0) { nmoves[gi] = (int16_t)nm; if (ntotal) ntotal[gi] = total; }
}

// Overflow tiers for positions whose dedup set outgrew the main LDS table
// (cap 7/8 of 2^LOG slots), fed by the overflow queue.  Tier 1: the same code with a
// 4,096-slot (64 KiB) LDS table; a position with more distinct afterstates (> 3,584)
// runs again in the same wave on tier 2, a 131,072-slot table in HBM that is the
// workgroup's own (grid = kSlowWaves tables).  Every position stays exact.  Round 6:
// one launch of kSlowWaves workgroups for both tiers (was 256 tier-1 workgroups, then a
// tier-2 launch fed by a second queue): the queue is empty or short on almost every
// step, so the launch is mostly its own cost.  SRC 0 = engine lanes, 1 = standalone arrays.
constexpr int kLogMid = 12;

template <int SRC>
__global__ __launch_bounds__(64) void k_movegen_over(Args A, const int8_t* boards, const uint8_t* players,
                                                     const uint8_t* dice, int cap, int16_t* nmoves, int32_t* ntotal,
                                                     uint64_t* moves, uint4* tables) {
    __shared__ uint4 memo[kMemoSlots];
    __shared__ uint4 lds_tab[1 << kLogMid];
    uint4* slow = tables + ((size_t)blockIdx.x << kLogSlotsSlow);
    const int count = (int)ufl((uint32_t)A.ovf_count[0]);
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int gi = (int)ufl((uint32_t)A.ovf_queue[q]);
        const int l = lane_id();
        int bv, pl, r0, r1;
        if (SRC == 0) {
            bv = load_rec(A, gi); pl = rd(bv, R_CUR); r0 = rd(bv, R_ROLL0); r1 = rd(bv, R_ROLL1);
        } else {
            bv = l < 52 ? (int)boards[(size_t)gi * 52 + l] : 0;
            pl = (int)ufl(players[gi]); r0 = (int)ufl(dice[2 * gi]); r1 = (int)ufl(dice[2 * gi + 1]);
        }
        uint64_t* out = SRC == 0 ? A.moves + (size_t)gi * A.max_moves : moves + (size_t)gi * cap;
        const int c = SRC == 0 ? A.max_moves : cap;
        int total;
        bool ovf;
        int nm = run_movegen<kLogMid>(bv, pl, r0, r1, out, c, lds_tab, A.cap_mid, &total, &ovf, memo);
        if (ovf) nm = run_movegen<kLogSlotsSlow>(bv, pl, r0, r1, out, c, slow, kCapSlow, &total, &ovf, memo);
        if (ovf) {
            if (l == 0) atomicOr(A.err, 1);
            nm = 0; total = 0;
        }
        if (SRC == 0) {
            bv = wr(bv, R_NM0, nm & 0xFF);
            bv = wr(bv, R_NM1, (nm >> 8) & 0xFF);
            bv = wr(bv, R_FLAGS, rd(bv, R_FLAGS) & ~1);
            store_rec(A, gi, bv);
            if (l == 0) A.n_total[gi] = total;
        } else if (l == 0) {
            nmoves[gi] = (int16_t)nm;
            if (ntotal) ntotal[gi] = total;
        }
    }
}

__global__ __launch_bounds__(64) void k_encode(const int8_t* boards, const uint8_t* players, int n, float* out) {
    const int gi = blockIdx.x;
    const int l = lane_id();
    const int bv = l < 52 ? (int)boards[(size_t)gi * 52 + l] : 0;
    const int cur = (int)ufl(players[gi]);
    float* row = out + (size_t)gi * 198;
    #pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int f = l + 64 * t;
        const float v = feature_at(bv, f < 198 ? f : 197, cur);
        if (f < 198) row[f] = v;
    }
}

// The 198 features of n 64-byte lane records (the rollout's stored records), as
// T = float or _Float16 (fp16: the rounding of the fp32 features that autocast's
// cast applies, ppo_agent.py:274), feature_at's encoding (immutable_board.py:171-212).
// A 256-thread block encodes 64 consecutive records into an LDS image of their
// contiguous output (64 x 198 T): one wave per record, lane l < 48 holding byte
// l = the count of point l % 24 of player l / 24 (its 4 units at 98 (l / 24) +
// 4 (l % 24)), lanes 48 / 49 (bar, off) of P1 / P2, lane 50 the one-hot; then the
// block copies the image out with 16-byte stores (coalesced, whole lines).
template <typename T>
__device__ __forceinline__ void lds_pair(T* o, float a, float b) {
    if (sizeof(T) == 2) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        h2 v; v[0] = (_Float16)a; v[1] = (_Float16)b;
        *(h2*)o = v;
    } else {
        *(float2*)o = make_float2(a, b);
    }
}

template <typename T, int W>
__global__ __launch_bounds__(256) void k_encode_rec(const uint8_t* __restrict__ records, int n, T* __restrict__ out) {
    static_assert(W >= 198 && W % 2 == 0 && (W - 198) / 2 <= 13, "row width: 198 features + up to 26 zero columns");
    constexpr int kRows = 64, kImg = kRows * W * (int)sizeof(T);          // bytes
    __shared__ __attribute__((aligned(16))) uint8_t img[kImg];
    T* im = (T*)img;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l2 = l == 48 ? 50 : (l == 49 ? 51 : 52);      // off1 / off2 / mover byte
    for (int r0 = blockIdx.x * kRows; r0 < n; r0 += gridDim.x * kRows) {
        const int nr = min(kRows, n - r0);
        int b[16], b2[16];
        #pragma unroll
        for (int k = 0; k < 16; ++k) {                      // this wave's 16 records, loads in flight
            const int r = r0 + w + 4 * k;
            b[k] = r < n ? records[(size_t)r * 64 + l] : 0;
            b2[k] = r < n ? records[(size_t)r * 64 + l2] : 0;
        }
        __syncthreads();                                    // the previous image is copied out
        #pragma unroll
        for (int k = 0; k < 16; ++k) {
            T* o = im + (w + 4 * k) * W;
            const int v = b[k], v2 = b2[k];
            if (l < 48) {
                const int P = l >= 24 ? 1 : 0, f = 98 * P + 4 * (l - 24 * P);
                lds_pair(o + f, v >= 1 ? 1.0f : 0.0f, v >= 2 ? 1.0f : 0.0f);
                lds_pair(o + f + 2, v >= 3 ? 1.0f : 0.0f, v >= 3 ? (float)(v - 3) * 0.5f : 0.0f);
            } else if (l < 50) {
                lds_pair(o + (l == 48 ? 96 : 194), (float)v * 0.5f, kOff15[v2 & 15]);
            } else if (l == 50) {
                lds_pair(o + 196, v2 == 0 ? 1.0f : 0.0f, v2 == 0 ? 0.0f : 1.0f);
            } else if (l < 51 + (W - 198) / 2) {            // zero padding columns (GEMM-aligned rows)
                lds_pair(o + 198 + 2 * (l - 51), 0.0f, 0.0f);
            }
        }
        __syncthreads();
        const int nbytes = nr * W * (int)sizeof(T);
        uint8_t* dst = (uint8_t*)(out + (size_t)r0 * W);
        if (((uintptr_t)dst & 15) == 0) {
            for (int q = threadIdx.x; q < nbytes / 16; q += blockDim.x) ((uint4*)dst)[q] = ((const uint4*)img)[q];
            for (int q = (nbytes & ~15) + threadIdx.x; q < nbytes; q += blockDim.x) dst[q] = img[q];
        } else {                                            // rows not 16-byte aligned: 4-byte copies
            for (int q = threadIdx.x; q < nbytes / 4; q += blockDim.x) ((uint32_t*)dst)[q] = ((const uint32_t*)img)[q];
        }
    }
}

// Afterstates / afterstate features of every legal move of a lane.
// MODE 0: int8 boards [M][52]; MODE 1: float features [M][198] (mover one-hot).
template <int MODE>
__global__ __launch_bounds__(64) void k_legal(Args A, int lane0, void* out) {
    const int gi = lane0 + blockIdx.x;
    const int l = lane_id();
    const int bv = load_rec(A, gi);
    const int cur = rd(bv, R_CUR);
    const int n = rd(bv, R_NM0) | (rd(bv, R_NM1) << 8);
    uint32_t blocked;
    const Node s0 = node_from_bytes(bv, cur, blocked);
    for (int m = 0; m < A.max_moves; ++m) {
        int nb = 0;
        if (m < n) {
            const uint64_t mv = A.moves[(size_t)gi * A.max_moves + m];
            const uint32_t mlo = ufl((uint32_t)mv), mhi = ufl((uint32_t)(mv >> 32));
            const uint64_t mm = (uint64_t)mlo | ((uint64_t)mhi << 32);
            Node s = s0;
            for (int i = 0; i < 4; ++i) {
                const uint32_t e = (uint32_t)(mm >> (16 * i)) & 0xFFFFu;
                if (!(e & 0x8000u)) break;
                Sub sm; sm.src = (int)(e & 31u); sm.dst = (int)((e >> 5) & 31u); sm.hit = (int)((e >> 10) & 1u);
                sm.enc = e;
                s = apply(s, sm, cur);
            }
            nb = bytes_from_node(bv, s, cur);
        }
        const size_t row = (size_t)blockIdx.x * A.max_moves + m;
        if (MODE == 0) {
            if (l < 52) ((int8_t*)out)[row * 52 + l] = (int8_t)(m < n ? nb : 0);
        } else {
            float* o = (float*)out + row * 198;
            #pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int f = l + 64 * t;
                const float v = m < n ? feature_at(nb, f < 198 ? f : 197, cur) : 0.0f;
                if (f < 198) o[f] = v;
            }
        }
    }
}

__global__ void k_action_masks(Args A, int16_t* counts, float* masks) {
    const int gi = blockIdx.x;
    const uint8_t* r = A.lanes + (size_t)gi * 64;
    const int n = (int)r[R_NM0] | ((int)r[R_NM1] << 8);
    if (counts && threadIdx.x == 0) counts[gi] = (int16_t)n;
    if (masks)
        for (int m = threadIdx.x; m < A.max_moves; m += blockDim.x) masks[(size_t)gi * A.max_moves + m] = m < n ? 1.0f : 0.0f;
}

// Re-enumerate the legal moves of caller-posed lanes (bgx_set_lanes).
template <int LOG>
__global__ __launch_bounds__(64) void k_regen(Args A, int lane0) {
    __shared__ uint4 tab[1 << LOG];
    __shared__ uint4 memo[kMemoSlots];
    const int gi = lane0 + blockIdx.x;
    int bv = load_rec(A, gi);
    const int cur = rd(bv, R_CUR), r0 = rd(bv, R_ROLL0), r1 = rd(bv, R_ROLL1);
    int total;
    bool ovf;
    int n = run_movegen<LOG>(bv, cur, r0, r1, A.moves + (size_t)gi * A.max_moves, A.max_moves, tab, cap_fast<LOG>(),
                             &total, &ovf, memo);
    int flags = rd(bv, R_FLAGS) & ~1;
    if (ovf) {
        if (lane_id() == 0) { const int q = atomicAdd(A.ovf_count, 1); A.ovf_queue[q] = gi; }
        n = 0; total = 0; flags |= 1;
    }
    if (lane_id() == 0) A.n_total[gi] = total;
    bv = wr(bv, R_NM0, n & 0xFF);
    bv = wr(bv, R_NM1, (n >> 8) & 0xFF);
    bv = wr(bv, R_FLAGS, flags);
    bv = wr(bv, R_NEED, NEED_NONE);
    store_rec(A, gi, bv);
}

// numpy legacy seeding (_legacy_seeding -> init_genrand): mt[0]=s,
// mt[i] = 1812433253*(mt[i-1]^(mt[i-1]>>30)) + i; index = 624.
__global__ void k_mt_seed(uint32_t* mt, const uint32_t* seeds, int B) {
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= B) return;
    uint32_t* s = mt + (size_t)gi * kMtWords;
    uint32_t x = seeds[gi];
    s[0] = x;
    for (int i = 1; i < 624; ++i) { x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i; s[i] = x; }
    s[624] = 624u;
}


// ---- rollout rows to pinned host memory (bgx_copy_regions): up to 8 strided 2-D
// copies in one launch, 16 bytes per thread-step, non-temporal stores (the
// destination is host memory across PCIe; nothing on the device reads it back).
struct CopyRegions {
    const uint8_t* src[kMaxRegions];
    uint8_t* dst[kMaxRegions];
    int64_t wchunks[kMaxRegions], spitch[kMaxRegions], dpitch[kMaxRegions];
    int64_t pre[kMaxRegions + 1];               // chunk prefix over the regions
    int n;
};

__global__ __launch_bounds__(256) void k_copy_regions(CopyRegions R) {
    const int64_t total = R.pre[R.n];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int r = 0;
        #pragma unroll
        for (int k = 1; k < kMaxRegions; ++k) r += (k < R.n && i >= R.pre[k]) ? 1 : 0;
        const int64_t j = i - R.pre[r], row = j / R.wchunks[r], col = j - row * R.wchunks[r];
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = *(const u32x4*)(R.src[r] + row * R.spitch[r] + 16 * col);
        __builtin_nontemporal_store(v, (u32x4*)(R.dst[r] + row * R.dpitch[r] + 16 * col));
    }
}

// ---- head-to-head arena (bgx/arena.py drives it) ----
// Bookkeeping of a match between two players A and B on the engine's lanes: each has its
// own weights and decision rule, every lane plays exactly G games, and the whole
// accounting stays on the device in arrays the caller owns:
//   games_done int32[B]   finished, counted games of the lane (active while < G)
//   sel_a, sel_b uint8[B] the lanes on which A / B is on move in the current position
//                         (the lane selection of bgx_one_ply_sel / bgx_two_ply_sel)
//   tally int64[16]       the result (BGX_ARENA_* indices, bgx.h)
// Seat rule: in game g of lane i, A sits as PLAYER1 (mover 0) iff ((i + g) & 1) == 0, so
// with B even A holds each seat in exactly half of all games.  A lane that has finished
// its G games keeps stepping (the engine steps every lane) with action 0, belongs to
// neither player and is not counted: counting exactly G games per lane keeps the result
// unbiased, where a fixed step budget would over-represent short games.
// The tally fields are integer sums, so the order of the additions does not matter: each
// wave counts its lanes with ballots and adds once per field (tally_add, count: bg_rollout.h).

// sel_a / sel_b of lane i for its current position: the mover's seat in the lane's game g
__device__ __forceinline__ void select_lane(const uint8_t* recs, int i, int g, bool active, uint8_t* sel_a,
                                            uint8_t* sel_b) {
    const int mover = recs[(size_t)i * 64 + R_CUR] & 1;
    const bool a_p1 = ((i + g) & 1) == 0;
    const bool a_moves = (mover == 0) == a_p1;
    sel_a[i] = (uint8_t)(active && a_moves);
    sel_b[i] = (uint8_t)(active && !a_moves);
}

// tally is zero already (the entry point's memset, ordered before this kernel)
__global__ __launch_bounds__(256) void k_arena_begin(const uint8_t* recs, int n, int G, int32_t* games_done,
                                                     uint8_t* sel_a, uint8_t* sel_b, int64_t* tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n, active = in && G > 0;
    if (in) {
        games_done[i] = 0;
        select_lane(recs, i, 0, active, sel_a, sel_b);
    }
    tally_add(tally, BGX_ARENA_ACTIVE, count(active));
}

__global__ __launch_bounds__(256) void k_arena_merge(const uint8_t* sel_a, const uint8_t* sel_b, const int32_t* act_a,
                                                     const int32_t* act_b, int n, int32_t* actions) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) actions[i] = sel_a[i] ? act_a[i] : (sel_b[i] ? act_b[i] : 0);
}

// After bgx_step, with that step's done / info.  The engine runs with auto_reset = 1: a
// lane never sits in a finished game when a step begins, so done == 1 is always a win by
// the mover of that step (info's winner field == its mover field, kind 0: apply_lane) and
// the record read here is already the first position of the lane's next game.  A pass
// (kind 1) or a refused action (kind 2) is a ply without a result; a done without a winner
// (kind 3, the auto_reset = 0 engine's reset step) would be no result either.
__global__ __launch_bounds__(256) void k_arena_advance(const uint8_t* recs, const uint8_t* done, const int32_t* info,
                                                       int n, int G, int32_t* games_done, uint8_t* sel_a,
                                                       uint8_t* sel_b, int64_t* tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    int g = in ? games_done[i] : G;
    const bool active = in && g < G;
    const int inf = active ? info[i] : 0;
    const int winner = ((inf >> 8) & 0xFF) - 1, score = (inf >> 16) & 0xFF;
    const bool fin = active && done[i] != 0 && winner >= 0;
    const bool a_p1 = ((i + g) & 1) == 0;
    const bool a_won = fin && ((winner == 0) == a_p1), b_won = fin && !a_won;
    bool retired = false;
    if (active) {
        if (fin) {
            games_done[i] = ++g;
            retired = g >= G;
        }
        select_lane(recs, i, g, !retired, sel_a, sel_b);
    }
    // every thread of the wave reaches the ballots (no early return above)
    tally_add(tally, BGX_ARENA_GAMES, count(fin));
    tally_add(tally, BGX_ARENA_WINS_A, count(a_won));
    tally_add(tally, BGX_ARENA_WINS_B, count(b_won));
    tally_add(tally, BGX_ARENA_POINTS_A, count(a_won && score == 1) + 2 * count(a_won && score == 2) +
                                             3 * count(a_won && score == 3));
    tally_add(tally, BGX_ARENA_POINTS_B, count(b_won && score == 1) + 2 * count(b_won && score == 2) +
                                             3 * count(b_won && score == 3));
    tally_add(tally, BGX_ARENA_GAMMONS_A, count(a_won && score == 2));
    tally_add(tally, BGX_ARENA_GAMMONS_B, count(b_won && score == 2));
    tally_add(tally, BGX_ARENA_BACKGAMMONS_A, count(a_won && score == 3));
    tally_add(tally, BGX_ARENA_BACKGAMMONS_B, count(b_won && score == 3));
    tally_add(tally, BGX_ARENA_GAMES_A_P1, count(fin && a_p1));
    tally_add(tally, BGX_ARENA_WINS_A_P1, count(a_won && a_p1));
    tally_add(tally, BGX_ARENA_WINS_P1, count(fin && winner == 0));
    tally_add(tally, BGX_ARENA_PLIES, count(active));
    tally_add(tally, BGX_ARENA_ACTIVE, -count(retired));
}

// ---- start table (bgx_engine_set_starts) ----
// One thread per record: copy it into the engine's table and mark it in byte kStartOk as
// valid (1) or not (0; error bit 2, the lane keeps the standard opening).  Valid: each
// side's points + bar + off == 15, no point held by both sides, both off counts < 15, mover
// 0 or 1, roll (0, 0) or both dice in 1..6.
__global__ __launch_bounds__(256) void k_check_starts(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int B,
                                                      int32_t* err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    uint4 q[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = ((const uint4*)src)[(size_t)i * 4 + k];
    uint8_t* r = (uint8_t*)q;
    int sum0 = r[48] + r[50], sum1 = r[49] + r[51];
    bool shared = false;
    #pragma unroll
    for (int p = 0; p < 24; ++p) {
        sum0 += r[p];
        sum1 += r[24 + p];
        shared |= r[p] != 0 && r[24 + p] != 0;
    }
    const int d0 = r[R_ROLL0], d1 = r[R_ROLL1];
    const bool roll_ok = (d0 == 0 && d1 == 0) || (d0 >= 1 && d0 <= 6 && d1 >= 1 && d1 <= 6);
    const bool ok = sum0 == 15 && sum1 == 15 && !shared && r[50] < 15 && r[51] < 15 && r[R_CUR] <= 1 && roll_ok;
    r[kStartOk] = ok ? 1 : 0;
    #pragma unroll
    for (int k = 0; k < 4; ++k) ((uint4*)dst)[(size_t)i * 4 + k] = q[k];
    if (!ok) atomicOr(err, 4);
}

// ---- position rollouts: the accounting arrays and the helpers are bg_rollout.h's ----
// tally and active are zero already (the entry point's memsets, ordered before this kernel)
__global__ __launch_bounds__(256) void k_rollout_begin(const int32_t* group, int n, int n_groups, int G,
                                                       int32_t* games_done, int32_t* plies, uint8_t* sel,
                                                       int64_t* active) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const bool on = in && G > 0 && rollout_group(group, i, n_groups) >= 0;
    if (in) {
        games_done[i] = 0;
        plies[i] = 0;
        sel[i] = (uint8_t)on;
    }
    tally_add(active, 0, count(on));
}

__global__ __launch_bounds__(256) void k_rollout_advance(const uint8_t* starts, const int32_t* group,
                                                         const uint8_t* done, const int32_t* info, int n, int n_groups,
                                                         int G, int32_t* games_done, int32_t* plies, uint8_t* sel,
                                                         int64_t* tally, int64_t* active) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const int g = in ? rollout_group(group, i, n_groups) : -1;
    const bool on = g >= 0 && games_done[i] < G;
    int winner, score;
    result_of(on ? info[i] : 0, &winner, &score);
    const bool fin = on && done[i] != 0 && winner >= 0;
    long long p = 0;
    int field = 0;
    bool retired = false;
    if (on) plies[i] += 1;                              // the step's own ply counts for the game it ends
    if (fin) {
        const bool won = winner == (int)(starts[(size_t)i * 64 + R_CUR] & 1);
        field = (won ? BGX_ROLLOUT_WIN1 : BGX_ROLLOUT_LOSS1) + score - 1;
        retired = end_game(i, G, games_done, plies, sel, &p);
    }
    for_each_group(fin, g, [&](int gl, bool mine, uint64_t m) {
        int64_t* row = tally + (size_t)gl * 8;
        tally_add(row, BGX_ROLLOUT_GAMES, (long long)__popcll(m));
        tally_add(row, BGX_ROLLOUT_PLIES, wave_sum(mine ? p : 0));
        #pragma unroll
        for (int f = BGX_ROLLOUT_WIN1; f <= BGX_ROLLOUT_LOSS3; ++f) tally_add(row, f, count(mine && field == f));
    });
    tally_add(active, 0, -count(retired));
}

// ---- luck-adjusted rollouts (DESIGN.md "Luck adjustment"; bgx_roll_luck gives luck[i]) ----
// lane_luck float[n] holds the running fp32 sum of s * luck over the steps of the lane's
// current game, s = +1 when the step's mover is the start record's mover, else -1.  The roll
// of a game's first step is left out when the start record fixed it (it was not drawn).
__global__ __launch_bounds__(256) void k_rollout_luck_add(const uint8_t* recs, const uint8_t* starts,
                                                          const int32_t* plies, const uint8_t* sel, const float* luck,
                                                          int n, float* lane_luck) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !sel[i]) return;
    if (plies[i] == 0 && starts[(size_t)i * 64 + R_ROLL0] != 0) return;
    const float l = luck[i];
    lane_luck[i] += recs[(size_t)i * 64 + R_CUR] == starts[(size_t)i * 64 + R_CUR] ? l : -l;
}

// After the step, before k_rollout_advance (sel is still the step's selection): a counted
// game (k_rollout_advance's rule) adds its luck in 2^-16 fixed point to its group's row and
// zeroes the lane's sum; any other done of a selected lane only zeroes it.  Per wave, one
// add per (group, field) it holds finishers of; integer adds commute.
__global__ __launch_bounds__(256) void k_rollout_luck_flush(const uint8_t* starts, const int32_t* group,
                                                            const uint8_t* sel, const uint8_t* done,
                                                            const int32_t* info, int n, int n_groups,
                                                            float* lane_luck, int64_t* luck_tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && sel[i] != 0;
    const int g = on ? rollout_group(group, i, n_groups) : -1;
    const bool dn = on && done[i] != 0;
    int winner, score;
    result_of(dn ? info[i] : 0, &winner, &score);
    const bool fin = dn && g >= 0 && winner >= 0;
    long long lq = 0, res = 0;
    if (fin) {
        lq = luck_q(lane_luck[i]);
        res = winner == (int)(starts[(size_t)i * 64 + R_CUR] & 1) ? score : -score;
    }
    if (dn) lane_luck[i] = 0.0f;
    for_each_group(fin, g, [&](int gl, bool mine, uint64_t m) {
        const long long v = mine ? lq : 0;
        int64_t* row = luck_tally + (size_t)gl * 4;
        tally_add(row, BGX_ROLLOUT_LUCK, wave_sum(v));
        tally_add(row, BGX_ROLLOUT_LUCK2, wave_sum(v * v));
        tally_add(row, BGX_ROLLOUT_RESLUCK, wave_sum(mine ? res * lq : 0));
        tally_add(row, BGX_ROLLOUT_LUCK_GAMES, (long long)__popcll(m));
    });
}

// murmur3's 64-bit finalizer
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// a uniformly random legal action per record: floor(u * count), u in [0, 1) from (seed, step, i)
__global__ __launch_bounds__(256) void k_random_act(const uint8_t* recs, int n, uint64_t seed, uint32_t step,
                                                    int32_t* act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = (uint32_t)recs[(size_t)i * 64 + R_NM0] | ((uint32_t)recs[(size_t)i * 64 + R_NM1] << 8);
    const uint64_t h = mix64(mix64(seed ^ 0x9E3779B97F4A7C15ull) + (((uint64_t)step << 32) | (uint32_t)i));
    act[i] = (int32_t)(((h >> 32) * (uint64_t)cnt) >> 32);      // 0 when the lane has no legal move
}

thread_local std::string g_err;      // bgx_last_error()

}  // namespace

// the error hooks of every translation unit (bg_host.h)
int bgx_internal_fail(hipError_t e, int code) {
    g_err = hipGetErrorString(e);
    return code;
}
void bgx_set_error(const char* msg) { g_err = msg; }
// the explicit debug options (bg_debug.h, bgx_debug_option)
static std::mutex g_dbg_mu;
static std::map<std::string, std::string> g_dbg;
std::string bgx_dbg(const char* name) {
    std::lock_guard<std::mutex> g(g_dbg_mu);
    const auto it = g_dbg.find(name);
    return it == g_dbg.end() ? std::string() : it->second;
}
long long bgx_dbg_int(const char* name, long long dflt) {
    const std::string v = bgx_dbg(name);
    return v.empty() ? dflt : strtoll(v.c_str(), nullptr, 10);
}

// the per-position kernels (reset, standalone movegen, regeneration) with the
// 512-slot dedup table
#define LAUNCH_LOG(K, grid, s, ...) hipLaunchKernelGGL(K<9>, grid, dim3(64), 0, s, __VA_ARGS__)

// The order's first pass, at the end of a step or reset: classes, roll cache, block counts.
// Its second pass (launch_gather) is due from here until the next bgx_step runs it.
static void launch_count(bgx_engine* e, hipStream_t s) {
    const int ncnt = (e->a.B + kCountThreads - 1) / kCountThreads;
    hipLaunchKernelGGL(k_order_count, dim3(ncnt), dim3(kCountThreads), 0, s, e->a.pre, e->a.cls, e->a.ctr, e->a.key0, e->a.key1,
                       e->order_cnt, e->a.B, e->ovf_base + 4 * (e->ovf_parity ^ 1), e->a.xcd);
    e->ovf_next_zeroed = true;
    e->gather_due = true;
}

// The order's second pass on stream s, which has joined the count pass: perm, and with
// `actions` (bgx_step) the step blocks of the step that follows on s.
static void launch_gather(bgx_engine* e, hipStream_t s, const int32_t* actions) {
    const Args& A = e->a;
    const int nblk = (A.B + kGatherThreads - 1) / kGatherThreads, ncnt = (A.B + kCountThreads - 1) / kCountThreads;
    if (actions)
        hipLaunchKernelGGL(k_step_gather<true>, dim3(nblk), dim3(kGatherThreads), 0, s, A.cls, e->order_cnt, e->perm, A.B,
                           ncnt, A.xcd, A.moves, A.ctr, actions, A.max_moves, e->blk);
    else
        hipLaunchKernelGGL(k_step_gather<false>, dim3(nblk), dim3(kGatherThreads), 0, s, A.cls, e->order_cnt, e->perm, A.B,
                           ncnt, A.xcd, nullptr, nullptr, nullptr, 0, nullptr);
}

// bgx_step's device arguments
struct StepIo {
    const int32_t* actions;
    float *obs, *reward;
    uint8_t* done;
    int32_t* info;
};

// The first `grid` positions of the dispatch order (every lane when there is no order).
static void launch_heavy(hipStream_t s, const Args& a, int grid, const StepIo& io) {
    if (grid <= 0) return;
    // the split's doubles prefix: a 512-slot table and no revisit memo (8 KB of LDS):
    // the doubles walks that cannot bear off use no table at all, so occupancy
    // (VGPR-bound, 4 waves/SIMD) beats a bigger table (C3: 1,024 slots + memo 242 M/s,
    // 512 slots + memo inside 284 M/s, no memo 288 M/s; measured round 2)
    // (MT_LANE engines have no order and step every lane here, with the generic kernel)
    if (a.blk)                                    // with a dispatch order: from the step blocks
        hipLaunchKernelGGL((k_step<0, 9, 0, false, 1, BGX_DICE_PHILOX, true>), dim3(grid), dim3(64), 0, s, a, io.actions,
                           io.obs, io.reward, io.done, io.info, 0);
    else if (a.dice_mode == BGX_DICE_PHILOX)
        hipLaunchKernelGGL((k_step<0, 9, 0, false, 1, BGX_DICE_PHILOX>), dim3(grid), dim3(64), 0, s, a, io.actions,
                           io.obs, io.reward, io.done, io.info, 0);
    else
        hipLaunchKernelGGL((k_step<0, 9, 0>), dim3(grid), dim3(64), 0, s, a, io.actions, io.obs, io.reward, io.done,
                           io.info, 0);
}

// The order's positions from `heavy` on: a 256-slot table, no memo, no doubles code (4 KB,
// 49 VGPRs: the hardware wave limit, ~5x the resident waves; doubles go to the overflow tiers).
static void launch_light(hipStream_t s, const Args& a, int heavy, const StepIo& io) {
    // (reached only with a dispatch order, which only a Philox engine has: from the step blocks)
    hipLaunchKernelGGL((k_step<0, 8, 0, true, 1, BGX_DICE_PHILOX, true>), dim3(a.B - heavy), dim3(64), 0, s, a, io.actions,
                       io.obs, io.reward, io.done, io.info, heavy);
}

// Doubles share of the dispatch order (Philox mode): the expected doubles
// fraction 1/6 plus 4 sigma.  Lanes past it run in the light launch whatever
// their class (exact either way; an unpredicted doubles lane is only slower).
// With the XCD-aware order the count is a multiple of 8, so the light launch's
// blocks keep the order's position -> XCD residue.
static int heavy_grid(int B, bool xcd) {
    const double g = B / 6.0 + 4.0 * std::sqrt(B * 5.0 / 36.0) + 32.0;
    int h = g >= B ? B : (int)g;
    if (xcd) h = (h + 7) & ~7;
    return h > B ? B : h;
}

static int slow_path(bgx_engine* e, hipStream_t s, int src, const int8_t* boards, const uint8_t* players,
                     const uint8_t* dice, int cap, int16_t* nm, int32_t* nt, uint64_t* moves) {
    if (src == 0)
        hipLaunchKernelGGL(k_movegen_over<0>, dim3(e->slow_waves), dim3(64), 0, s, e->a, boards, players, dice, cap,
                           nm, nt, moves, e->slow_tables);
    else
        hipLaunchKernelGGL(k_movegen_over<1>, dim3(e->slow_waves), dim3(64), 0, s, e->a, boards, players, dice, cap,
                           nm, nt, moves, e->slow_tables);
    return bgx_launch_status();
}

// The engine's fixed device buffers: bgx_engine_create allocates them in this order (bytes
// 0: not in this configuration) and zeroes the marked ones, bgx_engine_destroy frees them.
struct EngineBuf {
    void** p;
    size_t bytes;
    bool zero;
};
static std::vector<EngineBuf> engine_bufs(bgx_engine* e, bool stamps, bool order) {
    Args& A = e->a;
    const size_t B = (size_t)A.B;
    const bool shared = A.dice_mode == BGX_DICE_MT_SHARED;
    return {
        {(void**)&A.lanes, B * 64, true},
        {(void**)&A.moves, B * (size_t)A.max_moves * 8, false},
        {(void**)&A.n_total, B * 4, true},
        {(void**)&A.mt, (A.dice_mode == BGX_DICE_MT_LANE ? B : 1) * kMtWords * 4, false},
        {(void**)&A.ctr, B * 8, true},
        {(void**)&A.shared_rolls, B * 4, false},
        {(void**)&e->ovf_base, 32, true},
        {(void**)&A.ovf_queue, B * 4, false},
        {(void**)&A.err, 16, true},
        {(void**)&e->starts, shared ? 0 : B * 64, false},                   // bgx_engine_set_starts
        {(void**)&e->slow_tables, (size_t)kSlowWaves * ((size_t)16 << kLogSlotsSlow), false},
        {(void**)&A.stamps, stamps ? B * 16 : 0, false},
        {(void**)&e->perm, order ? B * 4 : 0, false},
        {(void**)&e->blk, order ? B * kBlkBytes : 0, false},
        {(void**)&A.cls, order ? B : 0, true},
        {(void**)&A.pre, order ? B : 0, true},
        {(void**)&e->order_cnt, order ? (B / kCountThreads + 1) * kXcd * kClasses * 4 : 0, false},
    };
}

// This call's overflow counters (Args::ovf_count), zero on stream s before its launches.
// With `rotate` (bgx_reset, bgx_step: the calls an order pass follows) the set that the
// last order pass zeroed is taken when there is one; every other case zeroes the current set.
static hipError_t fresh_ovf_counters(bgx_engine* e, hipStream_t s, bool rotate) {
    if (rotate && e->ovf_next_zeroed) {
        e->ovf_parity ^= 1;
        e->a.ovf_count = e->ovf_base + 4 * e->ovf_parity;
        e->ovf_next_zeroed = false;
        return hipSuccess;
    }
    return hipMemsetAsync(e->a.ovf_count, 0, 16, s);
}

// SHARED dice: apply, the one stream's dice for every lane that needs a roll, advance.
static void step_shared_dice(const Args& A, const StepIo& io, hipStream_t s) {
    hipLaunchKernelGGL((k_step<1, 9>), dim3(A.B), dim3(64), 0, s, A, io.actions, io.obs, io.reward, io.done, io.info, 0);
    hipLaunchKernelGGL(k_shared_dice, dim3(1), dim3(64), 0, s, A);
    hipLaunchKernelGGL((k_step<2, 9>), dim3(A.B), dim3(64), 0, s, A, io.actions, io.obs, io.reward, io.done, io.info, 0);
}

// The next dispatch order on the side stream once both launches of a forked step have
// written their pre-class bytes and counters: it runs beside stream s's overflow tiers and
// the caller's next policy kernel instead of before them (neither touches pre, cls, perm or
// the counters); the order pass writes the counters' roll cache, so the next bgx_step and
// every other call that reads or rewrites counters joins it (join_order) before its own
// launches.
static int order_on_side(bgx_engine* e, hipStream_t s) {
    BGX_CK(hipEventRecord(e->step_ev[2], s));
    BGX_CK(hipStreamWaitEvent(e->step_side, e->step_ev[2], 0));
    launch_count(e, e->step_side);
    BGX_CK(hipEventRecord(e->step_ev[3], e->step_side));
    e->order_pending = true;
    return BGX_OK;
}

// Per-lane dice.  Split dispatch (Philox mode, once there is a dispatch order): the
// predicted-doubles prefix of the order in the heavy launch, the rest in the light one,
// then the next order.  Forked (bgx_engine_set_fork), the light launch and the order pass
// run on the side stream beside the heavy launch (filling the CUs its tail leaves idle),
// fork-join on events; linear, everything is in plain stream order -- no cross-stream wait
// that a serializing tool (profiler) or a shared hardware queue could deadlock.
static int step_lane_dice(bgx_engine* e, const StepIo& io, hipStream_t s) {
    Args a = e->a;
    // the order's second pass, due since the last step's or reset's count pass (which the
    // caller's EngineCall has joined): perm and this step's blocks, from the actions of
    // this call and the records, move lists and counters as they stand now on s
    if (a.cls && e->gather_due) {
        launch_gather(e, s, io.actions);
        e->gather_due = false;
        a.perm = e->perm;
        a.blk = e->blk;
    }
    const int heavy = a.perm ? heavy_grid(a.B, a.xcd != 0) : a.B;
    if (heavy < a.B && e->step_fork) {
        if (!e->step_side) {
            BGX_CK(hipStreamCreateWithFlags(&e->step_side, hipStreamNonBlocking));
            for (hipEvent_t& ev : e->step_ev) BGX_CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        BGX_CK(hipEventRecord(e->step_ev[0], s));
        BGX_CK(hipStreamWaitEvent(e->step_side, e->step_ev[0], 0));
        launch_heavy(s, a, heavy, io);
        launch_light(e->step_side, a, heavy, io);
        BGX_CK(hipEventRecord(e->step_ev[1], e->step_side));
        if (a.cls) {
            const int rc = order_on_side(e, s);
            if (rc != BGX_OK) return rc;
        }
        BGX_CK(hipStreamWaitEvent(s, e->step_ev[1], 0));
    } else {
        launch_heavy(s, a, heavy, io);
        if (heavy < a.B) launch_light(s, a, heavy, io);
        if (a.cls) launch_count(e, s);
    }
    return BGX_OK;
}

// BGX_STEP_DEBUG: the overflow-tier queue size of this step and its first lanes, to stderr.
static int step_debug_dump(bgx_engine* e, hipStream_t s) {
    const Args& A = e->a;
    int32_t q[2] = {0, 0};
    BGX_CK(hipMemcpyAsync(q, A.ovf_count, 8, hipMemcpyDeviceToHost, s));
    BGX_CK(hipStreamSynchronize(s));
    fprintf(stderr, "[bgx step] overflow queue %d of %d lanes\n", q[0], A.B);
    for (int i = 0; i < q[0] && i < 4; ++i) {
        int32_t gi = 0;
        uint8_t rec[64];
        BGX_CK(hipMemcpy(&gi, A.ovf_queue + i, 4, hipMemcpyDeviceToHost));
        BGX_CK(hipMemcpy(rec, A.lanes + (size_t)gi * 64, 64, hipMemcpyDeviceToHost));
        int own = 0, outside = 0;
        const int pl = rec[52];
        for (int p = 0; p < 24; ++p) {
            own += rec[pl * 24 + p] > 0;
            if (!(pl == 0 ? p >= 18 : p < 6)) outside += rec[pl * 24 + p];
        }
        fprintf(stderr, "   lane %d pl %d roll %d-%d points %d outside %d bar %d off %d n %d\n", gi, pl, rec[53],
                rec[54], own, outside, rec[48 + pl], rec[50 + pl], rec[60] | (rec[61] << 8));
    }
    return BGX_OK;
}

// the bearoff database: its kernels and entry points (they use bg_rollout.h's helpers)
#include "bg_bearoff.h"

extern "C" {

int bgx_engine_create(int device, int32_t batch, int32_t max_moves, uint64_t seed, int32_t dice_mode,
                      int32_t auto_reset, int32_t match_length, bgx_engine** out) {
    if (!out || batch <= 0 || max_moves <= 0 || max_moves > 32767 || dice_mode < 0 || dice_mode > 2)
        return BGX_EINVAL;
    BGX_CK(hipSetDevice(device));
    bgx_engine* e = new bgx_engine();
    e->device = device;
    e->seed = seed;
    Args& A = e->a;
    A.B = batch; A.max_moves = max_moves; A.dice_mode = dice_mode; A.auto_reset = auto_reset ? 1 : 0;
    A.match_length = match_length;
    A.key0 = (uint32_t)seed; A.key1 = (uint32_t)(seed >> 32);
    A.xcd = batch % 128 == 0 && bgx_dbg_int("BGX_XCD", 1) != 0 ? 1 : 0;
    e->step_debug = !bgx_dbg("BGX_STEP_DEBUG").empty();
    // the overflow tiers' caps (tests force positions through tier 1 and tier 2 with small ones)
    A.cap_mid = (int)std::min<long long>(std::max<long long>(bgx_dbg_int("BGX_TIER1_CAP", cap_fast<kLogMid>()), 1),
                                         cap_fast<kLogMid>());
    A.cap_main = (int)std::min<long long>(std::max<long long>(bgx_dbg_int("BGX_MOVEGEN_CAP", cap_fast<9>()), 1),
                                          cap_fast<9>());
    const bool stamps = !bgx_dbg("BGX_STAMPS").empty();
    const bool order = dice_mode == BGX_DICE_PHILOX && bgx_dbg_int("BGX_ORDER", 1) != 0;
    hipError_t err = hipSuccess;
    for (const EngineBuf& b : engine_bufs(e, stamps, order))
        if (err == hipSuccess && b.bytes) err = hipMalloc(b.p, b.bytes);
    A.ovf_count = e->ovf_base;
    if (err != hipSuccess) { bgx_engine_destroy(e); return bgx_internal_fail(err, BGX_ENOMEM); }
    for (const EngineBuf& b : engine_bufs(e, stamps, order)) {
        if (b.zero && b.bytes && hipMemset(*b.p, 0, b.bytes) != hipSuccess) {
            bgx_engine_destroy(e);
            return bgx_internal_fail(hipGetLastError());
        }
    }
    // default seeds: lane i -> seed + i
    std::vector<uint32_t> seeds((size_t)batch);
    for (size_t i = 0; i < seeds.size(); ++i) seeds[i] = (uint32_t)(seed + i);
    int rc = bgx_engine_seed(e, seeds.data(), seed);
    if (rc != BGX_OK) { bgx_engine_destroy(e); return rc; }
    *out = e;
    return BGX_OK;
}

int bgx_engine_join(bgx_engine* e, void* stream) {
    if (!e) return BGX_EINVAL;
    EngineCall call(e, (hipStream_t)stream, true);   // the next step's dispatch order, on the side stream
    BGX_CK(call.err);
    return BGX_OK;
}

int bgx_engine_order(bgx_engine* e, int32_t* perm_host, uint8_t* cls_host, uint64_t* ctr_host, void* stream) {
    if (!e) return BGX_EINVAL;
    // no dispatch order (not Philox, or BGX_ORDER 0), or none built yet (before the first reset / step)
    if ((perm_host || cls_host) && (!e->a.cls || !e->gather_due)) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)e->a.B;
    {
        EngineCall call(e, s, true);         // the last step's count pass, on the side stream
        BGX_CK(call.err);
        // the second pass is due (the next step runs it with its actions): the same kernel
        // in its perm-only form gives the order that step will use, and leaves it due
        if (perm_host) {
            launch_gather(e, s, nullptr);
            BGX_CK_LAUNCH();
        }
        if (perm_host) BGX_CK(hipMemcpyAsync(perm_host, e->perm, B * 4, hipMemcpyDeviceToHost, s));
        if (cls_host) BGX_CK(hipMemcpyAsync(cls_host, e->a.cls, B, hipMemcpyDeviceToHost, s));
        if (ctr_host) BGX_CK(hipMemcpyAsync(ctr_host, e->a.ctr, B * 8, hipMemcpyDeviceToHost, s));
    }
    BGX_CK(hipStreamSynchronize(s));
    return BGX_OK;
}

int bgx_engine_set_fork(bgx_engine* e, int32_t fork, void* stream) {
    if (!e) return BGX_EINVAL;
    EngineCall call(e, (hipStream_t)stream, !fork);  // going linear: a pending dispatch order joins `stream` first
    BGX_CK(call.err);
    e->step_fork = fork != 0;
    return BGX_OK;
}

int bgx_engine_destroy(bgx_engine* e) {
    if (!e) return BGX_EINVAL;
    (void)hipSetDevice(e->device);
    if (e->use_valid) (void)hipEventSynchronize(e->use_ev);   // the last call's work is done
    if (e->use_ev) (void)hipEventDestroy(e->use_ev);
    for (const EngineBuf& b : engine_bufs(e, true, true)) if (*b.p) (void)hipFree(*b.p);
    for (const DeviceBuf* b : {&e->search_ws, &e->search_pool, &e->oneply_ws}) if (b->p) (void)hipFree(b->p);
    for (hipEvent_t ev : e->search_ev) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->step_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->step_side) (void)hipStreamDestroy(e->step_side);
    if (e->search_side) (void)hipStreamDestroy(e->search_side);
    delete e;
    return BGX_OK;
}

int bgx_engine_seed(bgx_engine* e, const uint32_t* seeds_host, uint64_t philox_seed) {
    if (!e || !seeds_host) return BGX_EINVAL;
    BGX_CK(hipSetDevice(e->device));
    Args& A = e->a;
    // device-wide order (bgx.h "Stream ordering"): every earlier call on any stream has
    // finished before the dice state changes, and the new state is in place on return
    BGX_CK(hipDeviceSynchronize());
    A.key0 = (uint32_t)philox_seed; A.key1 = (uint32_t)(philox_seed >> 32);
    BGX_CK(hipMemset(A.ctr, 0, (size_t)A.B * 8));
    if (A.dice_mode == BGX_DICE_PHILOX) {
        BGX_CK(hipDeviceSynchronize());
        return BGX_OK;
    }
    const int n = A.dice_mode == BGX_DICE_MT_LANE ? A.B : 1;
    uint32_t* dseeds = nullptr;
    BGX_CK(hipMalloc(&dseeds, (size_t)n * 4));
    hipError_t err = hipMemcpy(dseeds, seeds_host, (size_t)n * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_mt_seed, dim3((n + 255) / 256), dim3(256), 0, 0, A.mt, dseeds, n);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    (void)hipFree(dseeds);
    BGX_CK(err);
    return BGX_OK;
}

int bgx_engine_mt_state(bgx_engine* e, int32_t lane, uint32_t* state_host, int32_t set) {
    if (!e || !state_host) return BGX_EINVAL;
    Args& A = e->a;
    if (A.dice_mode == BGX_DICE_PHILOX) return BGX_EINVAL;
    if (A.dice_mode == BGX_DICE_MT_SHARED) lane = 0;
    if (lane < 0 || lane >= A.B) return BGX_EINVAL;
    BGX_CK(hipSetDevice(e->device));
    BGX_CK(hipDeviceSynchronize());
    uint32_t* dev = A.mt + (size_t)lane * kMtWords;
    if (set) BGX_CK(hipMemcpy(dev, state_host, 625 * 4, hipMemcpyHostToDevice));
    else BGX_CK(hipMemcpy(state_host, dev, 625 * 4, hipMemcpyDeviceToHost));
    return BGX_OK;
}

#ifdef BGX_COUNTERS
extern "C" int bgx_debug_counters(unsigned long long* out16) {
    BGX_CK(hipDeviceSynchronize());
    constexpr size_t n = 16 * (size_t)bg::kCntSlots;
    std::vector<unsigned long long> h(n), z(n, 0ull);
    BGX_CK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(bg::g_cnt), n * 8));
    for (int i = 0; i < 16; ++i) {
        out16[i] = 0;
        for (int k = 0; k < bg::kCntSlots; ++k) out16[i] += h[(size_t)i * bg::kCntSlots + k];
    }
    BGX_CK(hipMemcpyToSymbol(HIP_SYMBOL(bg::g_cnt), z.data(), n * 8));
    return BGX_OK;
}
#endif

// diagnostics: copy the per-lane [start, end] s_memrealtime stamps of the last step
extern "C" int bgx_debug_stamps(bgx_engine* e, uint64_t* host_out) {
    if (!e || !host_out || !e->a.stamps) return BGX_EINVAL;
    BGX_CK(hipDeviceSynchronize());
    BGX_CK(hipMemcpy(host_out, e->a.stamps, (size_t)e->a.B * 16, hipMemcpyDeviceToHost));
    return BGX_OK;
}

int bgx_engine_buffers(bgx_engine* e, bgx_buffers* out) {
    if (!e || !out) return BGX_EINVAL;
    out->lanes = e->a.lanes; out->moves = e->a.moves; out->n_total = e->a.n_total;
    out->batch = e->a.B; out->max_moves = e->a.max_moves;
    return BGX_OK;
}

int bgx_reset(bgx_engine* e, const uint8_t* lane_mask_dev, float* obs_dev, void* stream) {
    if (!e) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Args& A = e->a;
    EngineCall call(e, s, true);             // joins a step's dispatch order still on the side stream
    BGX_CK(call.err);
    BGX_CK(fresh_ovf_counters(e, s, true));
    if (A.dice_mode == BGX_DICE_MT_SHARED) {
        LAUNCH_LOG(k_reset, dim3(A.B), s, A, lane_mask_dev, obs_dev, 1);
        hipLaunchKernelGGL(k_shared_dice, dim3(1), dim3(64), 0, s, A);
        LAUNCH_LOG(k_reset, dim3(A.B), s, A, nullptr, obs_dev, 0);
    } else {
        LAUNCH_LOG(k_reset, dim3(A.B), s, A, lane_mask_dev, obs_dev, 0);
    }
    BGX_CK_LAUNCH();
    if (A.cls) launch_count(e, s);
    return slow_path(e, s, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
}

int bgx_step(bgx_engine* e, const int32_t* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
             int32_t* info_dev, void* stream) {
    if (!e || !actions_dev || !reward_dev || !done_dev) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const StepIo io{actions_dev, obs_dev, reward_dev, done_dev, info_dev};
    // joins the previous step's dispatch order (side stream).  A pending order has zeroed
    // the other counter set, so fresh_ovf_counters below then rotates and issues no memset:
    // the wait is this call's first operation on s either way.
    EngineCall call(e, s, true);
    BGX_CK(call.err);
    BGX_CK(fresh_ovf_counters(e, s, true));
    if (e->a.dice_mode == BGX_DICE_MT_SHARED) {
        step_shared_dice(e->a, io, s);
    } else {
        const int rc = step_lane_dice(e, io, s);
        if (rc != BGX_OK) return rc;
    }
    BGX_CK_LAUNCH();
    const int rc = slow_path(e, s, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
    if (e->step_debug) {
        const int drc = step_debug_dump(e, s);
        if (drc != BGX_OK) return drc;
    }
    return rc;
}

int bgx_movegen(bgx_engine* e, const int8_t* boards52_dev, const uint8_t* players_dev, const uint8_t* dice_dev,
                int32_t n, int32_t max_moves, int16_t* n_moves_dev, int32_t* n_total_dev, uint64_t* moves_dev,
                void* stream) {
    if (!e || n < 0 || max_moves <= 0 || !boards52_dev || !players_dev || !dice_dev || !n_moves_dev || !moves_dev)
        return BGX_EINVAL;
    if (n > e->a.B) return BGX_EINVAL;   // overflow queue is sized by the engine batch
    if (n == 0) return BGX_OK;
    hipStream_t s = (hipStream_t)stream;
    EngineCall call(e, s);
    BGX_CK(call.err);
    BGX_CK(fresh_ovf_counters(e, s, false));
    LAUNCH_LOG(k_movegen, dim3(n), s, boards52_dev, players_dev, dice_dev, n, max_moves, n_moves_dev, n_total_dev,
               moves_dev, e->a.ovf_count, e->a.ovf_queue, e->a.cap_main);
    BGX_CK_LAUNCH();
    return slow_path(e, s, 1, boards52_dev, players_dev, dice_dev, max_moves, n_moves_dev, n_total_dev, moves_dev);
}

int bgx_encode(const int8_t* boards52_dev, const uint8_t* players_dev, int32_t n, float* out_dev, void* stream) {
    if (n < 0 || (n > 0 && (!boards52_dev || !players_dev || !out_dev))) return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipLaunchKernelGGL(k_encode, dim3(n), dim3(64), 0, (hipStream_t)stream, boards52_dev, players_dev, n, out_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_encode_records_ex(const uint8_t* records_dev, int32_t n, int32_t dtype, int32_t width, void* out_dev,
                          void* stream) {
    if (n < 0 || (dtype != 0 && dtype != 1) || (width != 198 && width != 208) || (n > 0 && (!records_dev || !out_dev)))
        return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    const int blocks = (n + 63) / 64 < 4096 ? (n + 63) / 64 : 4096;
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == 0 && width == 198)
        hipLaunchKernelGGL((k_encode_rec<float, 198>), dim3(blocks), dim3(256), 0, s, records_dev, n, (float*)out_dev);
    else if (dtype == 0)
        hipLaunchKernelGGL((k_encode_rec<float, 208>), dim3(blocks), dim3(256), 0, s, records_dev, n, (float*)out_dev);
    else if (width == 198)
        hipLaunchKernelGGL((k_encode_rec<_Float16, 198>), dim3(blocks), dim3(256), 0, s, records_dev, n,
                           (_Float16*)out_dev);
    else
        hipLaunchKernelGGL((k_encode_rec<_Float16, 208>), dim3(blocks), dim3(256), 0, s, records_dev, n,
                           (_Float16*)out_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_encode_records(const uint8_t* records_dev, int32_t n, int32_t dtype, void* out_dev, void* stream) {
    return bgx_encode_records_ex(records_dev, n, dtype, 198, out_dev, stream);
}

int bgx_afterstates(bgx_engine* e, int32_t lane0, int32_t nlanes, int8_t* boards52_dev, void* stream) {
    if (!e || !boards52_dev || lane0 < 0 || nlanes < 0 || lane0 + nlanes > e->a.B) return BGX_EINVAL;
    if (nlanes == 0) return BGX_OK;
    EngineCall call(e, (hipStream_t)stream);
    BGX_CK(call.err);
    hipLaunchKernelGGL(k_legal<0>, dim3(nlanes), dim3(64), 0, (hipStream_t)stream, e->a, lane0, (void*)boards52_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_legal_features(bgx_engine* e, int32_t lane0, int32_t nlanes, float* out_dev, void* stream) {
    if (!e || !out_dev || lane0 < 0 || nlanes < 0 || lane0 + nlanes > e->a.B) return BGX_EINVAL;
    if (nlanes == 0) return BGX_OK;
    EngineCall call(e, (hipStream_t)stream);
    BGX_CK(call.err);
    hipLaunchKernelGGL(k_legal<1>, dim3(nlanes), dim3(64), 0, (hipStream_t)stream, e->a, lane0, (void*)out_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_action_masks(bgx_engine* e, int16_t* counts_dev, float* masks_dev, void* stream) {
    if (!e) return BGX_EINVAL;
    if (!counts_dev && !masks_dev) return BGX_OK;
    EngineCall call(e, (hipStream_t)stream);
    BGX_CK(call.err);
    hipLaunchKernelGGL(k_action_masks, dim3(e->a.B), dim3(masks_dev ? 256 : 64), 0, (hipStream_t)stream, e->a,
                       counts_dev, masks_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_copy_lanes(bgx_engine* e, int32_t lane0, int32_t n, uint8_t* lanes_dst, uint64_t* moves_dst,
                   int32_t* n_total_dst, void* stream) {
    if (!e || lane0 < 0 || n < 0 || lane0 + n > e->a.B) return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipStream_t s = (hipStream_t)stream;
    const Args& A = e->a;
    EngineCall call(e, s);
    BGX_CK(call.err);
    if (lanes_dst) BGX_CK(hipMemcpyAsync(lanes_dst, A.lanes + (size_t)lane0 * 64, (size_t)n * 64, hipMemcpyDeviceToDevice, s));
    if (moves_dst)
        BGX_CK(hipMemcpyAsync(moves_dst, A.moves + (size_t)lane0 * A.max_moves, (size_t)n * A.max_moves * 8,
                          hipMemcpyDeviceToDevice, s));
    if (n_total_dst) BGX_CK(hipMemcpyAsync(n_total_dst, A.n_total + lane0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return BGX_OK;
}

int bgx_set_lanes(bgx_engine* e, int32_t lane0, int32_t n, const uint8_t* lanes_src, void* stream) {
    return bgx_set_lanes_ex(e, lane0, n, lanes_src, 1, stream);
}

int bgx_set_lanes_ex(bgx_engine* e, int32_t lane0, int32_t n, const uint8_t* lanes_src, int32_t regen, void* stream) {
    if (!e || !lanes_src || lane0 < 0 || n < 0 || lane0 + n > e->a.B) return BGX_EINVAL;
    if (n == 0) return BGX_OK;
    hipStream_t s = (hipStream_t)stream;
    Args& A = e->a;
    EngineCall call(e, s);
    BGX_CK(call.err);
    BGX_CK(hipMemcpyAsync(A.lanes + (size_t)lane0 * 64, lanes_src, (size_t)n * 64, hipMemcpyDeviceToDevice, s));
    if (!regen) return BGX_OK;
    BGX_CK(fresh_ovf_counters(e, s, false));
    LAUNCH_LOG(k_regen, dim3(n), s, A, lane0);
    BGX_CK_LAUNCH();
    return slow_path(e, s, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
}

int bgx_engine_error(bgx_engine* e, int32_t* err_out) {
    if (!e || !err_out) return BGX_EINVAL;
    BGX_CK(hipSetDevice(e->device));
    BGX_CK(hipDeviceSynchronize());
    BGX_CK(hipMemcpy(err_out, e->a.err, 4, hipMemcpyDeviceToHost));
    return BGX_OK;
}

int bgx_host_device_ptr(void* host_ptr, void** dev_ptr_out) {
    if (!host_ptr || !dev_ptr_out) return BGX_EINVAL;
    BGX_CK(hipHostGetDevicePointer(dev_ptr_out, host_ptr, 0));
    return BGX_OK;
}

int bgx_copy_regions(const bgx_region* regions, int32_t n, int32_t workgroups, void* stream) {
    if (!regions || n < 0 || n > kMaxRegions) return BGX_EINVAL;
    CopyRegions R;
    memset(&R, 0, sizeof R);
    R.n = n;
    int64_t acc = 0;
    for (int i = 0; i < n; ++i) {
        const bgx_region& g = regions[i];
        if (!g.src || !g.dst || g.width < 0 || g.rows < 0 || g.width % 16 || g.spitch % 16 || g.dpitch % 16 ||
            (uintptr_t)g.src % 16 || (uintptr_t)g.dst % 16 || (g.rows > 1 && (g.spitch < g.width || g.dpitch < g.width)))
            return BGX_EINVAL;
        R.src[i] = (const uint8_t*)g.src; R.dst[i] = (uint8_t*)g.dst;
        R.wchunks[i] = g.width / 16 > 0 ? g.width / 16 : 1;
        R.spitch[i] = g.spitch; R.dpitch[i] = g.dpitch;
        R.pre[i] = acc;
        acc += g.width / 16 * g.rows;
    }
    for (int i = n; i <= kMaxRegions; ++i) R.pre[i] = acc;
    if (acc == 0) return BGX_OK;
    const int64_t need = (acc + 255) / 256;
    const int wg = (int)(workgroups > 0 && workgroups < need ? workgroups : (need < 64 ? need : 64));
    hipLaunchKernelGGL(k_copy_regions, dim3(wg), dim3(256), 0, (hipStream_t)stream, R);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_begin(const uint8_t* records_dev, int32_t n, int32_t games_per_lane, int32_t* games_done_dev,
                    uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev, void* stream) {
    if (!records_dev || n <= 0 || games_per_lane < 0 || !games_done_dev || !sel_a_dev || !sel_b_dev || !tally_dev)
        return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    BGX_CK(hipMemsetAsync(tally_dev, 0, 16 * sizeof(int64_t), s));
    hipLaunchKernelGGL(k_arena_begin, dim3((n + 255) / 256), dim3(256), 0, s, records_dev, n, games_per_lane,
                       games_done_dev, sel_a_dev, sel_b_dev, tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_merge(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const int32_t* act_a_dev,
                    const int32_t* act_b_dev, int32_t n, int32_t* actions_dev, void* stream) {
    if (!sel_a_dev || !sel_b_dev || !act_a_dev || !act_b_dev || n <= 0 || !actions_dev) return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_merge, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sel_a_dev, sel_b_dev,
                       act_a_dev, act_b_dev, n, actions_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_arena_advance(const uint8_t* records_dev, const uint8_t* done_dev, const int32_t* info_dev, int32_t n,
                      int32_t games_per_lane, int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev,
                      int64_t* tally_dev, void* stream) {
    if (!records_dev || !done_dev || !info_dev || n <= 0 || games_per_lane < 0 || !games_done_dev || !sel_a_dev ||
        !sel_b_dev || !tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_arena_advance, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       done_dev, info_dev, n, games_per_lane, games_done_dev, sel_a_dev, sel_b_dev, tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_engine_set_starts(bgx_engine* e, const uint8_t* starts_dev, void* stream) {
    if (!e || e->a.dice_mode == BGX_DICE_MT_SHARED || ((uintptr_t)starts_dev & 15)) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Args& A = e->a;
    EngineCall call(e, s);
    BGX_CK(call.err);
    if (!starts_dev) {
        A.starts = nullptr;
        return BGX_OK;
    }
    hipLaunchKernelGGL(k_check_starts, dim3((A.B + 255) / 256), dim3(256), 0, s, starts_dev, e->starts, A.B, A.err);
    BGX_CK_LAUNCH();
    A.starts = e->starts;
    return BGX_OK;
}

int bgx_rollout_begin(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev, int32_t n,
                      int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev,
                      uint8_t* sel_dev, int64_t* tally_dev, int64_t* active_dev, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || n <= 0 || n_groups <= 0 || games_per_lane < 0 ||
        !games_done_dev || !plies_dev || !sel_dev || !tally_dev || !active_dev)
        return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    BGX_CK(hipMemsetAsync(tally_dev, 0, (size_t)n_groups * 8 * sizeof(int64_t), s));
    BGX_CK(hipMemsetAsync(active_dev, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(k_rollout_begin, dim3((n + 255) / 256), dim3(256), 0, s, group_dev, n, n_groups, games_per_lane,
                       games_done_dev, plies_dev, sel_dev, active_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_advance(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                        const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                        int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                        int64_t* tally_dev, int64_t* active_dev, void* stream) {
    if (!records_dev || !starts_dev || !group_dev || !done_dev || !info_dev || n <= 0 || n_groups <= 0 ||
        games_per_lane < 0 || !games_done_dev || !plies_dev || !sel_dev || !tally_dev || !active_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_rollout_advance, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts_dev,
                       group_dev, done_dev, info_dev, n, n_groups, games_per_lane, games_done_dev, plies_dev, sel_dev,
                       tally_dev, active_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_luck_add(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* plies_dev,
                         const uint8_t* sel_dev, const float* luck_dev, int32_t n, float* lane_luck_dev, void* stream) {
    if (!records_dev || !starts_dev || !plies_dev || !sel_dev || !luck_dev || n <= 0 || !lane_luck_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_rollout_luck_add, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev,
                       starts_dev, plies_dev, sel_dev, luck_dev, n, lane_luck_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_rollout_luck_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                           const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                           float* lane_luck_dev, int64_t* luck_tally_dev, void* stream) {
    if (!starts_dev || !group_dev || !sel_dev || !done_dev || !info_dev || n <= 0 || n_groups <= 0 ||
        !lane_luck_dev || !luck_tally_dev)
        return BGX_EINVAL;
    hipLaunchKernelGGL(k_rollout_luck_flush, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, starts_dev,
                       group_dev, sel_dev, done_dev, info_dev, n, n_groups, lane_luck_dev, luck_tally_dev);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

int bgx_random_act(const uint8_t* records_dev, int32_t n, uint64_t seed, uint32_t step, int32_t* act_out,
                   void* stream) {
    if (!records_dev || n <= 0 || !act_out) return BGX_EINVAL;
    hipLaunchKernelGGL(k_random_act, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, records_dev, n, seed,
                       step, act_out);
    BGX_CK_LAUNCH();
    return BGX_OK;
}

const char* bgx_last_error(void) { return g_err.c_str(); }

int bgx_debug_option(const char* name, const char* value) {
    if (!name || !name[0]) return BGX_EINVAL;
    std::lock_guard<std::mutex> g(g_dbg_mu);
    if (value) g_dbg[name] = value; else g_dbg.erase(name);
    return BGX_OK;
}

#ifndef BGX_BUILD_ID
#define BGX_BUILD_ID "unknown"
#endif
// the tag lets build() read the id from the file without loading it
__attribute__((used)) static const char kBuildId[] = "bgx-build-id:" BGX_BUILD_ID;
const char* bgx_build_id(void) { return kBuildId + 13; }

}  // extern "C"
