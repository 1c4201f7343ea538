// bg_adam.hip — the PPO update's optimizer step (bgx_adam_step): fused Adam over every
// parameter tensor with the GradScaler's non-finite check, unscale and scale update.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "bg_host.h"

namespace {

// ---- the optimizer step (bgx_adam_step): torch.optim.Adam(fused=True) driven by
// GradScaler.step + update, as three launches over the flat element range of every
// tensor instead of torch's per-tensor multi-tensor chunks (a 90 k-parameter net ran
// as ~4 workgroups each walking 65,536 elements: 69 us for the Adam kernel alone, plus
// the inf check, the step increments and the scale update as separate launches)
constexpr int kAdamMax = 8;
struct AdamArgs {
    float* p[kAdamMax];
    float* g[kAdamMax];
    float* m[kAdamMax];
    float* v[kAdamMax];
    float* step[kAdamMax];
    int64_t end[kAdamMax];            // exclusive prefix sums of the element counts
    int n;
    int64_t total;
    double lr, beta1, beta2, eps;     // torch passes them as doubles
    const float* scale;               // GradScaler scale (null: no scaler)
    int32_t* found;                   // non-finite flag (0 between calls)
};

__device__ __forceinline__ int adam_tensor(const AdamArgs& a, int64_t i) {
    int t = 0;
    #pragma unroll
    for (int k = 0; k < kAdamMax - 1; ++k)
        t += (k < a.n - 1 && i >= a.end[k]) ? 1 : 0;
    return t;
}

// GradScaler._check_inf_per_device: any non-finite scaled gradient
__global__ __launch_bounds__(256) void k_adam_check(AdamArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < a.total) {
        const int t = adam_tensor(a, i);
        const float g = a.g[t][i - (t ? a.end[t - 1] : 0)];
        bad = !isfinite(g);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(a.found, 1);
}

// _fused_adam_ (ADAM_MODE::ORIGINAL, no weight decay / amsgrad / maximize): the
// gradient unscaled by the GradScaler scale (and stored back, as torch does), then the
// moments and the parameter at step s + 1; nothing when the check found a non-finite.
// The mixed fp32 / fp64 arithmetic follows torch's adam_math (fp32 state, double
// hyper-parameters: the moment updates and the unscale round from fp64, the bias
// corrections are fp64 rounded to fp32, the parameter update is fp32)
__global__ __launch_bounds__(256) void k_adam_apply(AdamArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total || (a.scale && *a.found)) return;
    const int t = adam_tensor(a, i);
    const int64_t j = i - (t ? a.end[t - 1] : 0);
    float g = a.g[t][j];
    if (a.scale) {
        g = (float)((double)g / (double)*a.scale);
        a.g[t][j] = g;
    }
    const double s = (double)(*a.step[t] + 1.0f);
    float m = a.m[t][j], v = a.v[t][j];
    m = (float)(a.beta1 * (double)m + (1.0 - a.beta1) * (double)g);
    v = (float)(a.beta2 * (double)v + (1.0 - a.beta2) * (double)g * (double)g);
    const float bc1 = (float)(1.0 - pow(a.beta1, s));
    const float bc2s = (float)sqrt(1.0 - pow(a.beta2, s));
    const float step_size = (float)(a.lr / (double)bc1);
    const float denom = (float)((double)(sqrtf(v) / bc2s) + a.eps);
    a.p[t][j] -= step_size * m / denom;
    a.m[t][j] = m;
    a.v[t][j] = v;
}

// the step counters (+1 unless skipped) and _amp_update_scale_; the flag back to 0
__global__ void k_adam_finish(AdamArgs a, float* scale, int32_t* tracker, float growth, float backoff, int interval) {
    const int l = threadIdx.x;
    const int found = (a.scale && *a.found) ? 1 : 0;
    if (l < a.n && !found) *a.step[l] += 1.0f;
    if (l == 0 && scale) {
        if (found) {
            *scale = (float)((double)*scale * (double)backoff);
            *tracker = 0;
        } else {
            const int succ = *tracker + 1;
            if (succ == interval) {
                const float ns = (float)((double)*scale * (double)growth);
                if (isfinite(ns)) *scale = ns;
                *tracker = 0;
            } else {
                *tracker = succ;
            }
        }
        *a.found = 0;
    }
}

}  // namespace

extern "C" int bgx_adam_step(int32_t n, float* const* params, float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, float* const* steps, const int64_t* numels, double lr,
                             double beta1, double beta2, double eps, float* scale, int32_t* growth_tracker,
                             float growth_factor, float backoff_factor, int32_t growth_interval, int32_t* found,
                             void* stream) {
    if (n <= 0 || n > kAdamMax || !params || !grads || !exp_avg || !exp_avg_sq || !steps || !numels || !found)
        return BGX_EINVAL;
    if (scale && !growth_tracker) return BGX_EINVAL;
    AdamArgs a{};
    int64_t tot = 0;
    for (int t = 0; t < n; ++t) {
        if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || !steps[t] || numels[t] < 0) return BGX_EINVAL;
        a.p[t] = params[t]; a.g[t] = grads[t]; a.m[t] = exp_avg[t]; a.v[t] = exp_avg_sq[t]; a.step[t] = steps[t];
        tot += numels[t];
        a.end[t] = tot;
    }
    for (int t = n; t < kAdamMax; ++t) a.end[t] = tot;
    a.n = n; a.total = tot;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.scale = scale; a.found = found;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    if (tot > 0) {
        if (scale) hipLaunchKernelGGL(k_adam_check, dim3(blocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_adam_apply, dim3(blocks), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_adam_finish, dim3(1), dim3(64), 0, s, a, scale, growth_tracker, growth_factor, backoff_factor,
                       growth_interval);
    return bgx_launch_status();
}
