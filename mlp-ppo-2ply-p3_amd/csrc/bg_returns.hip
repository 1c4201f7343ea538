// bg_returns.hip — what bgx/returns.py calls after a rollout, each a walk over the
// [T][B] rollout with one thread per game lane: discounted lane returns
// (bgx_lane_returns), zero-sum GAE(lambda) for self-play (bgx_selfplay_gae), the
// episode statistics (bgx_episode_stats) and the advantage normalisation from sums
// kept on the device (bgx_normalize_adv).  The fp32 arithmetic repeats the torch
// forms' roundings one by one (mul_rn / add_rn / sub_rn: no contraction to fma).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "bg_host.h"

namespace {

// One fp32 product / sum / difference, rounded on its own.  hipcc contracts a * b + c to an
// fma by default, also through __fmul_rn / __fadd_rn (inline a * b and a + b of a header
// compiled with contraction allowed); these carry no contraction flag, so they never fuse.
__device__ __forceinline__ float mul_rn(float a, float b) {
    #pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
    #pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
    #pragma clang fp contract(off)
    return a - b;
}

// ---- discounted returns per game lane (bgx.train.lane_returns; ppo_agent.py:206-216
// restated per lane): R_t = r_t + gamma R_{t+1}, R reset at done -- one thread per lane
// walking its T steps backwards, the same two fp32 roundings as the torch ops (no fma)
__global__ __launch_bounds__(256) void k_lane_returns(const float* __restrict__ r, const uint8_t* __restrict__ d,
                                                      int T, int B, float gamma, float* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float R = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * B + b;
        if (d[i]) R = 0.0f;
        R = add_rn(r[i], mul_rn(gamma, R));
        out[i] = R;
    }
}

// ---- the rollout's episode accounting per game lane (bgx_episode_stats;
// bgx.train.episode_stats restated, train.py:55-99): one thread per lane walks its T
// steps, accumulating the unfinished episode's reward from the carry, closing it at each
// done; per-block sums of the six statistics (fp64: the rewards are multiples of 1/2, so
// every sum is exact in any order), then one block adds the block sums in order.  The
// mover byte (record byte 52) is read only at winning steps.
constexpr int kEpStats = 6;
__global__ __launch_bounds__(256) void k_episode_partials(const float* __restrict__ r, const uint8_t* __restrict__ d,
                                                          const uint8_t* __restrict__ rec, double* __restrict__ carry,
                                                          int T, int B, double* __restrict__ part) {
    __shared__ double red[4][kEpStats];
    const int b = blockIdx.x * 256 + threadIdx.x;
    double v[kEpStats] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (b < B) {
        double acc = carry[b];
        for (int t = 0; t < T; ++t) {
            const size_t i = (size_t)t * B + b;
            const double rw = (double)r[i];
            acc += rw;
            if (d[i]) {
                v[0] += 1.0;                               // finished episodes
                v[1] += acc;                               // their rewards (carry included)
                acc = 0.0;
                if (rw > 0.0) {
                    v[2] += 1.0;                           // wins (the mover of a winning step)
                    v[3] += rec[i * 64 + 52] == 0 ? 1.0 : 0.0;     // by PLAYER1
                }
                v[4] += rw == 1.5 ? 1.0 : 0.0;             // gammon wins
                v[5] += rw == 2.0 ? 1.0 : 0.0;             // backgammon wins
            }
        }
        carry[b] = acc;
    }
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int k = 0; k < kEpStats; ++k) {
        double x = v[k];
        #pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
        if (l == 0) red[w][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kEpStats)
        part[(size_t)blockIdx.x * kEpStats + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
__global__ __launch_bounds__(64) void k_episode_sum(const double* __restrict__ part, int nb, double* __restrict__ out) {
    if (threadIdx.x >= kEpStats) return;
    double s = 0.0;
    for (int k = 0; k < nb; ++k) s += part[(size_t)k * kEpStats + threadIdx.x];
    out[threadIdx.x] = s;
}

// ---- zero-sum GAE(lambda) per game lane (bgx_selfplay_gae; bgx.train._selfplay_gae_torch
// restated, DESIGN.md §6 "Self-play returns"): one thread per lane walks its T steps
// backwards carrying (A, v, mover) of step t + 1, sign-flipped where the mover changes and
// dropped at a done; five fp32 roundings per step in the torch loop's order (no fma).
// A step's four loads (reward, done, value, mover byte) do not depend on the recurrence:
// they are issued kGaeU steps at a time, the next group's before the current group's
// arithmetic, so 2 x 4 x kGaeU loads per lane are in flight (a 65,536-lane launch is one
// wave per SIMD: the loads in flight per wave are all the memory parallelism there is).
// The mover is one byte load per record: the lanes of a wave touch 64 different 64-byte
// records either way, and a wider load would move bytes nobody reads.
constexpr int kGaeU = 8;                     // steps per load group
struct GaeGroup { float r[kGaeU], v[kGaeU]; int d[kGaeU], m[kGaeU]; };

// steps top, top - 1, ..., top - kGaeU + 1; a step below 0 (the last group of a T that is
// no multiple of kGaeU) loads step 0 again and is not used: no branch between the loads
__device__ __forceinline__ void gae_load(GaeGroup& s, const float* __restrict__ r, const uint8_t* __restrict__ d,
                                         const uint8_t* __restrict__ rec, const float* __restrict__ v, int top, int B,
                                         int b) {
    #pragma unroll
    for (int j = 0; j < kGaeU; ++j) {
        const int t = top - j > 0 ? top - j : 0;
        const size_t i = (size_t)t * B + b;
        s.r[j] = r[i];
        s.v[j] = v[i];
        s.d[j] = d[i];
        s.m[j] = rec[i * 64 + 52];
    }
}

__global__ __launch_bounds__(256) void k_selfplay_gae(const float* __restrict__ r, const uint8_t* __restrict__ d,
                                                      const uint8_t* __restrict__ rec, const float* __restrict__ v,
                                                      const float* __restrict__ boot_v,
                                                      const uint8_t* __restrict__ boot_rec, int T, int B, float g,
                                                      float gl, float* __restrict__ adv, float* __restrict__ ret,
                                                      double* __restrict__ part) {
    __shared__ double red[4][2];
    const int b = blockIdx.x * 256 + threadIdx.x;
    double sa = 0.0, sq = 0.0;
    if (b < B) {
        GaeGroup cur, nxt;
        gae_load(cur, r, d, rec, v, T - 1, B, b);
        // step T: the position the rollout stopped in, or nothing (the horizon is a cut)
        const bool boot = boot_v != nullptr;
        float v1 = boot ? boot_v[b] : 0.0f;
        int m1 = boot ? (int)boot_rec[(size_t)b * 64 + 52] : 0;
        float a1 = 0.0f;
        bool cut_next = !boot;
        for (int top = T - 1; top >= 0; top -= kGaeU) {
            if (top >= kGaeU) gae_load(nxt, r, d, rec, v, top - kGaeU, B, b);
            #pragma unroll
            for (int j = 0; j < kGaeU; ++j) {
                const int t = top - j;
                if (t >= 0) {
                    const float rv = cur.v[j];
                    const bool cut = cur.d[j] != 0 || cut_next;
                    const bool same = cur.m[j] == m1;
                    const float nv = cut ? 0.0f : (same ? v1 : -v1);
                    const float na = cut ? 0.0f : (same ? a1 : -a1);
                    const float delta = sub_rn(add_rn(cur.r[j], mul_rn(g, nv)), rv);
                    const float a = add_rn(delta, mul_rn(gl, na));
                    const size_t i = (size_t)t * B + b;
                    adv[i] = a;
                    ret[i] = add_rn(a, rv);
                    sa += (double)a;
                    sq += (double)a * (double)a;
                    a1 = a; v1 = rv; m1 = cur.m[j];
                    cut_next = false;
                }
            }
            cur = nxt;
        }
    }
    if (part == nullptr) return;                             // uniform: no sums asked for
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    #pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sa += __shfl_xor(sa, o);
        sq += __shfl_xor(sq, o);
    }
    if (l == 0) { red[w][0] = sa; red[w][1] = sq; }
    __syncthreads();
    if (threadIdx.x < 2)
        part[(size_t)blockIdx.x * 2 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// the block partials in a fixed order: lane l adds blocks l, l + 64, ..., then a xor tree
__global__ __launch_bounds__(64) void k_selfplay_gae_sum(const double* __restrict__ part, int nb, double n,
                                                         double* __restrict__ sums) {
    double sa = 0.0, sq = 0.0;
    for (int k = threadIdx.x; k < nb; k += 64) {
        sa += part[(size_t)k * 2];
        sq += part[(size_t)k * 2 + 1];
    }
    #pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sa += __shfl_xor(sa, o);
        sq += __shfl_xor(sq, o);
    }
    if (threadIdx.x == 0) { sums[0] = sa; sums[1] = sq; sums[2] = n; }
}

// ---- advantage normalisation from the three sums on the device (bgx_normalize_adv;
// bgx.ppo.global_normalize's multi-rank branch): mean and unbiased variance in fp64, var
// clamped at 0, then (a - fp32(mean)) / (fp32(std) + eps) in fp32, in place
__device__ __forceinline__ void normalize_consts(const double* __restrict__ sums, float eps, float& mean, float& den) {
    const double n = sums[2];
    const double mu = sums[0] / n;
    double var = (sums[1] - n * mu * mu) / (n - 1.0);
    var = var > 0.0 ? var : (var == var ? 0.0 : var);       // clamp(min=0); NaN (n = 1) stays NaN
    mean = (float)mu;
    den = add_rn((float)sqrt(var), eps);
}
__global__ __launch_bounds__(256) void k_normalize_adv(float* __restrict__ a, int64_t n, int64_t n4,
                                                       const double* __restrict__ sums, float eps) {
    float mean, den;
    normalize_consts(sums, eps, mean, den);
    const int64_t stride = (int64_t)gridDim.x * 256;
    float4* a4 = reinterpret_cast<float4*>(a);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 x = a4[i];
        x.x = __fdiv_rn(sub_rn(x.x, mean), den);
        x.y = __fdiv_rn(sub_rn(x.y, mean), den);
        x.z = __fdiv_rn(sub_rn(x.z, mean), den);
        x.w = __fdiv_rn(sub_rn(x.w, mean), den);
        a4[i] = x;
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        a[i] = __fdiv_rn(sub_rn(a[i], mean), den);
}

}  // namespace

extern "C" int64_t bgx_episode_stats_workspace(int32_t B) {
    if (B < 0) return BGX_EINVAL;
    return (int64_t)((B + 255) / 256) * kEpStats * (int64_t)sizeof(double);
}

extern "C" int bgx_episode_stats(const float* rewards, const uint8_t* dones, const uint8_t* records, double* carry,
                                 int32_t T, int32_t B, double* workspace, double* out, void* stream) {
    if (T < 0 || B < 0 || !out || (B > 0 && (!carry || !workspace)) ||
        (T > 0 && B > 0 && (!rewards || !dones || !records)))
        return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nb = (B + 255) / 256;
    if (nb > 0)
        hipLaunchKernelGGL(k_episode_partials, dim3(nb), dim3(256), 0, s, rewards, dones, records, carry, T, B,
                           workspace);
    hipLaunchKernelGGL(k_episode_sum, dim3(1), dim3(64), 0, s, workspace, nb, out);
    return bgx_launch_status();
}

extern "C" int bgx_lane_returns(const float* rewards, const uint8_t* dones, int32_t T, int32_t B, float gamma,
                                float* out, void* stream) {
    if (T < 0 || B < 0 || (T > 0 && B > 0 && (!rewards || !dones || !out))) return BGX_EINVAL;
    if (T == 0 || B == 0) return BGX_OK;
    hipLaunchKernelGGL(k_lane_returns, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, dones, T, B,
                       gamma, out);
    return bgx_launch_status();
}

extern "C" int64_t bgx_selfplay_gae_workspace(int32_t B) {
    if (B < 0) return BGX_EINVAL;
    return (int64_t)((B + 255) / 256) * 2 * (int64_t)sizeof(double);
}

extern "C" int bgx_selfplay_gae(const float* rewards, const uint8_t* dones, const uint8_t* records, const float* values,
                                const float* boot_values, const uint8_t* boot_records, int32_t T, int32_t B, float g,
                                float gl, float* adv, float* ret, double* workspace, double* sums, void* stream) {
    if (T <= 0 || B <= 0 || !rewards || !dones || !records || !values || !adv || !ret) return BGX_EINVAL;
    if ((boot_values == nullptr) != (boot_records == nullptr)) return BGX_EINVAL;
    if (sums && !workspace) return BGX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nb = (B + 255) / 256;
    hipLaunchKernelGGL(k_selfplay_gae, dim3(nb), dim3(256), 0, s, rewards, dones, records, values, boot_values,
                       boot_records, T, B, g, gl, adv, ret, sums ? workspace : (double*)nullptr);
    if (sums)
        hipLaunchKernelGGL(k_selfplay_gae_sum, dim3(1), dim3(64), 0, s, workspace, nb, (double)T * (double)B, sums);
    return bgx_launch_status();
}

extern "C" int bgx_normalize_adv(float* adv, int64_t n, const double* sums, float eps, void* stream) {
    if (n <= 0 || !adv || !sums) return BGX_EINVAL;
    const int64_t n4 = ((uintptr_t)adv & 15) == 0 ? n / 4 : 0;
    const int64_t work = n4 > 0 ? n4 + 3 : n;                 // threads that find an element
    const int nb = (int)((work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_normalize_adv, dim3(nb), dim3(256), 0, (hipStream_t)stream, adv, n, n4, sums, eps);
    return bgx_launch_status();
}

// the one-sided bearoff database: its kernels use mul_rn / add_rn / sub_rn above
#include "bg_bearoff1.h"

// the doubling cube of position rollouts: its kernels reuse bg_bearoff1.h's tally helpers
#include "bg_cube.h"

// truncated position rollouts: the same helpers again
#include "bg_trunc.h"

// truncated cubeful rollouts and the static cube evaluator: bg_cube.h's byte decoding, the helpers
#include "bg_cube_trunc.h"

// luck-adjusted cubeful rollouts: bg_cube_trunc.h's rule per roll, bg_cube.h's decision, the helpers
#include "bg_cube_luck.h"

// the cubeful exact bearoff table: bg_cube.h's byte decoding, bg_bearoff1.h's records and helpers
#include "bg_bearoff_cube.h"

// the doubling cube of the head-to-head arena: bg_cube.h's rule in two halves, the same helpers
#include "bg_arena_cube.h"

// luck-adjusted arena results: bg_cube_luck.h's roll index, weights and rounding, the helpers
#include "bg_arena_luck.h"

// match play in the arena: bg_arena_cube.h's seat rule and take, bg_cube_trunc.h's ct_ arithmetic
#include "bg_match.h"

// match-score rollouts: bg_match.h's rule fused into one decision, bg_cube.h's bytes, the helpers
#include "bg_match_rollout.h"
