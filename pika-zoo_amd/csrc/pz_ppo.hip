// libpikazoo_ppo.so (include/pikazoo_ppo.h): the PPO update loss -- loss, logging statistics and the gradients with respect to
// the logits and the values from one pass over the logit rows -- and the moments of the advantage normalisation.
//
// The loss kernel is pz_policy's backward_kernel with a few float operations and a reduction added: one lane per row,
// blockIdx.y = agent, one wave (64 consecutive rows) per workgroup, the wave's span staged into its transposed LDS image,
// the gradient row written into the same image and stored transposed back.  Everything that reads and judges a logit row
// is pz_policy_rows.hpp, the text pz_policy.hip runs: the log-prob and the entropy of a row are the bits
// pz_action_log_probs returns.  The loss is a scalar, so d loss / d logits needs nothing the forward does not already
// hold: g_lp / M and -ent_coef / M are the upstream gradients of the backward formula.
//
// The reductions use no floating-point atomic (two calls must return the same bits).  A wave adds its rows' five terms
// (pg, vl, H, kl, cf) as a butterfly over the lane index -- a fixed order -- and lane 0 writes the five sums to
// partials[(side * 5 + term) * waves + wave] with plain stores.  The finishing launch (one workgroup per agent) sums the
// partials in float64: thread t takes indices t, t + 256, ... in order, and the 256 sums fold in a fixed tree.  The kernel
// boundary publishes the partials: no fence, no counter, nothing to reset, and no workgroup waits for another.
// One wave per workgroup is kept: the image and the transposed stores are per wave, with one wave a barrier is a wait for
// the LDS only, and the finisher's share is 5 floats per 64 rows (1/15 of the bytes the loss launch reads at A = 18).
//
// The logit format is the compile-time instantiation (3 loss kernels); the value formats are run-time switches.  The
// moments kernel accumulates in float64 about x[0] (pikazoo_ppo.h says why), 4096 rows per workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_policy.h"
#include "pikazoo_ppo.h"
#include "pz_policy_rows.hpp"

namespace pz_ppo {

using namespace pz_policy;

constexpr int kTerms = 5;              // pg, vl, H, kl, cf
constexpr int kFinishThreads = 256;    // of either finishing kernel
constexpr int kMomentThreads = 256;
constexpr int kMomentRows = 4096;      // rows per workgroup of the moments kernel: 16 per thread
constexpr int64_t kMaxRows = (int64_t)1 << 30;

struct LossArgs {
    Common c;  // (logp and ent are not used)
    const float* old_logp[2];
    const float* adv[2];
    const float* ret[2];
    const void* values[2];
    const void* old_values[2];
    const float* adv_norm;
    void* grad_logits[2];
    void* grad_values[2];
    float* partials;
    int64_t value_pitch, grad_pitch, grad_value_pitch, waves;
    int32_t value_format, old_value_format;
    float clip, value_clip, vf_coef, ent_coef;
};

struct FinishArgs {
    const float* partials;
    float* stats;
    int64_t n, waves;
    float vf_coef, ent_coef;
};

struct MomentArgs {
    const float* x[2];
    double* partials;  // [side][2][blocks]
    float* out;
    int64_t n, blocks;
    float eps;
};

// an element of a run-time format (the logit formats' values) as float32, and back
__device__ __forceinline__ float load_as_float(const void* p, int format, int64_t i)
{
    if (format == PZ_POLICY_LOGIT_FLOAT32) return ((const float*)p)[i];
    const uint16_t bits = ((const uint16_t*)p)[i];
    return format == PZ_POLICY_LOGIT_FLOAT16 ? to_float<PZ_POLICY_LOGIT_FLOAT16>(bits) : to_float<PZ_POLICY_LOGIT_BFLOAT16>(bits);
}

__device__ __forceinline__ void store_from_float(void* p, int format, int64_t i, float x)
{
    if (format == PZ_POLICY_LOGIT_FLOAT32)
        ((float*)p)[i] = x;
    else if (format == PZ_POLICY_LOGIT_FLOAT16)
        ((uint16_t*)p)[i] = from_float<PZ_POLICY_LOGIT_FLOAT16>(x);
    else
        ((uint16_t*)p)[i] = from_float<PZ_POLICY_LOGIT_BFLOAT16>(x);
}

// the sum over the wave's 64 lanes, the same value in every lane: a butterfly, whose order is a function of the lane index
template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int off = kLanes / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, kLanes);
    return x;
}

template <int LF>
__global__ void __launch_bounds__(kLanes) loss_kernel(const LossArgs a)
{
    __shared__ float image[kLanes * kMaxStride];
    using R = typename Raw<LF>::type;
    const Common& c = a.c;
    const int lane = threadIdx.x, side = blockIdx.y;
    const int64_t g0 = (int64_t)blockIdx.x * kLanes;
    const int rows = (int)min((int64_t)kLanes, c.n - g0);
    const int A = c.A, stride = A | 1;
    load_image<LF>(c, side, g0, rows, stride, image, lane);
    float pg = 0.0f, vl = 0.0f, H = 0.0f, kl = 0.0f, cf = 0.0f;  // (a lane without a row adds +0)
    if (lane < rows) {
        const int64_t g = g0 + lane;
        float* row = image + lane * stride;
        const RowStats s = row_stats(row, A);
        const int act = load_action(c.act[side], c.action_format, g);
        const float nan = __uint_as_float(0x7FC00000u);
        const float M = (float)c.n;
        // the log-prob and the entropy: pikazoo_policy.h's step 5, the expression pz_action_log_probs stores
        const bool in_range = (unsigned)act < (unsigned)A;
        const bool nan_row = s.bad || !in_range;
        const float la = row[in_range ? act : 0];
        const float lp = nan_row ? nan : (la - s.m) - s.logS;
        H = s.bad ? nan : s.H;
        // the policy term
        const float d = lp - a.old_logp[side][g];
        const float r = expf(d);
        float Ahat = a.adv[side][g];
        if (a.adv_norm) Ahat = (Ahat - a.adv_norm[2 * side]) * a.adv_norm[2 * side + 1];
        const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
        const float unclipped = -Ahat * r;
        const float clipped = -Ahat * fminf(fmaxf(r, lo), hi);
        pg = clipped > unclipped ? clipped : unclipped;  // (a NaN in `unclipped` stays)
        const bool flat = (r > hi && Ahat > 0.0f) || (r < lo && Ahat < 0.0f);
        const float g_lp = flat ? 0.0f : unclipped;
        kl = (r - 1.0f) - d;
        cf = r != r ? nan : (fabsf(r - 1.0f) > a.clip ? 1.0f : 0.0f);
        // the value term
        const float v = load_as_float(a.values[side], a.value_format, g * a.value_pitch);
        const float ret = a.ret[side][g];
        const float e = v - ret;
        float g_v = e;
        vl = 0.5f * e * e;
        if (a.value_clip > 0.0f) {
            const float old_v = load_as_float(a.old_values[side], a.old_value_format, g);
            const float dv = v - old_v;
            const float ec = (old_v + fminf(fmaxf(dv, -a.value_clip), a.value_clip)) - ret;
            if (ec * ec > e * e) {
                vl = 0.5f * ec * ec;
                g_v = fabsf(dv) <= a.value_clip ? ec : 0.0f;
            }
        }
        if (a.grad_values[side]) store_from_float(a.grad_values[side], a.value_format, g * a.grad_value_pitch, a.vf_coef * g_v / M);
        // the gradient row: pikazoo_policy.h's backward formula with glogp = g_lp / M, gent = -ent_coef / M
        if (a.grad_logits[side]) {
            const float glogp = g_lp / M, gent = -a.ent_coef / M;
            for (int i = 0; i < A; ++i) {
                const float di = row[i] - s.m;
                const float ei = expf(di);
                const float p = ei / s.S;
                float grad = glogp * ((i == act ? 1.0f : 0.0f) - p);
                if (ei > 0.0f) grad += gent * (-p * ((di - s.logS) + s.H));
                row[i] = nan_row ? nan : grad;
            }
        }
    }
    // the wave's partial sums
    pg = wave_sum(pg), vl = wave_sum(vl), H = wave_sum(H), kl = wave_sum(kl), cf = wave_sum(cf);
    if (lane == 0) {
        float* out = a.partials + (int64_t)side * kTerms * a.waves + blockIdx.x;
        out[0 * a.waves] = pg;
        out[1 * a.waves] = vl;
        out[2 * a.waves] = H;
        out[3 * a.waves] = kl;
        out[4 * a.waves] = cf;
    }
    if (!a.grad_logits[side]) return;
    __syncthreads();
    R* span = (R*)a.grad_logits[side] + g0 * a.grad_pitch;
    if (a.grad_pitch == A) {
        store_dense<LF>(span, rows * A, A, c.a_magic, stride, image, lane);
    } else {
        const int count = rows * A;
        for (int e = lane; e < count; e += kLanes) {
            const int row = (int)(((uint32_t)e * c.a_magic) >> kDivShift), col = e - row * A;
            span[row * a.grad_pitch + col] = from_float<LF>(image[row * stride + col]);
        }
    }
}

// sum of count float64 values per thread slot, folded in a fixed tree; the total in thread 0
__device__ __forceinline__ double block_fold(double x, double* fold, int t)
{
    __syncthreads();  // (the previous fold has been read)
    fold[t] = x;
    __syncthreads();
    for (int half = kFinishThreads / 2; half > 0; half >>= 1) {
        if (t < half) fold[t] += fold[t + half];
        __syncthreads();
    }
    return fold[0];
}

__global__ void __launch_bounds__(kFinishThreads) loss_finish_kernel(const FinishArgs a)
{
    __shared__ double fold[kFinishThreads];
    const int t = threadIdx.x, side = blockIdx.y;
    double mean[kTerms];
    for (int q = 0; q < kTerms; ++q) {
        const float* part = a.partials + ((int64_t)side * kTerms + q) * a.waves;
        double sum = 0.0;
        for (int64_t i = t; i < a.waves; i += kFinishThreads) sum += (double)part[i];
        mean[q] = block_fold(sum, fold, t) / (double)a.n;
    }
    if (t == 0) {
        float* out = a.stats + 8 * side;
        out[0] = (float)(mean[0] + (double)a.vf_coef * mean[1] - (double)a.ent_coef * mean[2]);
        for (int q = 0; q < kTerms; ++q) out[1 + q] = (float)mean[q];
        out[6] = 0.0f;
        out[7] = 0.0f;
    }
}

__global__ void __launch_bounds__(kMomentThreads) moments_kernel(const MomentArgs a)
{
    __shared__ double s1w[kMomentThreads / kLanes], s2w[kMomentThreads / kLanes];
    const int t = threadIdx.x, side = blockIdx.y;
    const float* x = a.x[side];
    const double K = (double)x[0];
    const int64_t base = (int64_t)blockIdx.x * kMomentRows;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int k = 0; k < kMomentRows / kMomentThreads; ++k) {
        const int64_t i = base + k * kMomentThreads + t;
        if (i < a.n) {
            const double d = (double)x[i] - K;  // exact
            s1 += d;
            s2 = fma(d, d, s2);
        }
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    if ((t & (kLanes - 1)) == 0) s1w[t / kLanes] = s1, s2w[t / kLanes] = s2;
    __syncthreads();
    if (t == 0) {
        double* out = a.partials + (int64_t)side * 2 * a.blocks + blockIdx.x;
        out[0] = ((s1w[0] + s1w[1]) + s1w[2]) + s1w[3];
        out[a.blocks] = ((s2w[0] + s2w[1]) + s2w[2]) + s2w[3];
    }
}

__global__ void __launch_bounds__(kFinishThreads) moments_finish_kernel(const MomentArgs a)
{
    __shared__ double fold[kFinishThreads];
    const int t = threadIdx.x, side = blockIdx.y;
    double total[2];
    for (int q = 0; q < 2; ++q) {
        const double* part = a.partials + ((int64_t)side * 2 + q) * a.blocks;
        double sum = 0.0;
        for (int64_t i = t; i < a.blocks; i += kFinishThreads) sum += part[i];
        total[q] = block_fold(sum, fold, t);
    }
    if (t == 0) {
        const double n = (double)a.n, K = (double)a.x[side][0];
        const double v = total[1] - total[0] * total[0] / n;
        const double var = (v < 0.0 ? 0.0 : v) / (n - 1.0);  // (a NaN stays one)
        a.out[2 * side] = (float)(K + total[0] / n);
        a.out[2 * side + 1] = (float)(1.0 / (sqrt(var) + (double)a.eps));
    }
}

static int64_t waves_of(int64_t n) { return (n + kLanes - 1) / kLanes; }
static int64_t moment_blocks_of(int64_t n) { return (n + kMomentRows - 1) / kMomentRows; }

static bool bad_vector_pitch(int64_t n, int64_t pitch) { return pitch < 1 || (n > 0 && pitch > (INT64_MAX / 4) / n); }

static bool finite_at_least_zero(float x) { return x >= 0.0f && x < INFINITY; }

}  // namespace pz_ppo

using namespace pz_ppo;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kPpoBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_ppo_build_id(void) { return kPpoBuildIdRecord + 12; }

int pz_ppo_abi_version(void) { return PZ_PPO_ABI_VERSION; }

int64_t pz_ppo_workspace_bytes(int64_t n)
{
    if (n <= 0 || n > kMaxRows) return 0;
    const int64_t loss = 2 * kTerms * waves_of(n) * (int64_t)sizeof(float);
    const int64_t moments = 2 * 2 * moment_blocks_of(n) * (int64_t)sizeof(double);
    return ((loss > moments ? loss : moments) + 15) & ~(int64_t)15;
}

int pz_ppo_moments(const float* x_p1, const float* x_p2, int64_t n, float eps, float* out, void* workspace, void* stream)
{
    if (!x_p1 || !out || !workspace) return PZ_E_NULL;
    if (n < 0 || n == 1 || n > kMaxRows) return PZ_E_SIZE;
    if (!finite_at_least_zero(eps)) return PZ_E_CONFIG;
    if (misaligned(x_p1, 4) || misaligned(x_p2, 4) || misaligned(out, 4) || misaligned(workspace, 16)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const int64_t blocks = moment_blocks_of(n);
    const MomentArgs a{{x_p1, x_p2}, (double*)workspace, out, n, blocks, eps};
    const unsigned sides = x_p2 ? 2 : 1;
    hipLaunchKernelGGL(moments_kernel, dim3((unsigned)blocks, sides), dim3(kMomentThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1, sides), dim3(kFinishThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int pz_ppo_loss(const void* logits_p1, const void* logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                int64_t logit_pitch, int32_t action_format, const void* act_p1, const void* act_p2, const float* old_logp_p1,
                const float* old_logp_p2, const float* adv_p1, const float* adv_p2, const float* ret_p1, const float* ret_p2,
                const void* values_p1, const void* values_p2, int32_t value_format, int64_t value_pitch, const void* old_values_p1,
                const void* old_values_p2, int32_t old_value_format, const float* adv_norm, float clip, float value_clip, float vf_coef,
                float ent_coef, void* grad_logits_p1, void* grad_logits_p2, int64_t grad_pitch, void* grad_values_p1,
                void* grad_values_p2, int64_t grad_value_pitch, float* stats, void* workspace, void* stream)
{
    if (!logits_p1 || !act_p1 || !old_logp_p1 || !adv_p1 || !ret_p1 || !values_p1 || !stats || !workspace) return PZ_E_NULL;
    if (value_clip > 0.0f && !old_values_p1) return PZ_E_NULL;
    const bool both = logits_p2 != nullptr;
    if (!paired(act_p1, act_p2, both) || !paired(old_logp_p1, old_logp_p2, both) || !paired(adv_p1, adv_p2, both) ||
        !paired(ret_p1, ret_p2, both) || !paired(values_p1, values_p2, both) || !paired(old_values_p1, old_values_p2, both) ||
        !paired(grad_logits_p1, grad_logits_p2, both) || !paired(grad_values_p1, grad_values_p2, both))
        return PZ_E_NULL;
    if (bad_sizes(num_actions, n, logit_pitch) || (grad_logits_p1 && bad_sizes(num_actions, n, grad_pitch)) ||
        bad_vector_pitch(n, value_pitch) || (grad_values_p1 && bad_vector_pitch(n, grad_value_pitch)))
        return PZ_E_SIZE;
    if (!known_logit_format(logit_format) || !known_action_format(action_format) || !known_logit_format(value_format) ||
        (old_values_p1 && !known_logit_format(old_value_format)))
        return PZ_E_CONFIG;
    if (!(clip > 0.0f && clip < 1.0f) || !finite_at_least_zero(value_clip) || !finite_at_least_zero(vf_coef) ||
        !finite_at_least_zero(ent_coef))
        return PZ_E_CONFIG;
    const uintptr_t lb = logit_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2, ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    const uintptr_t vb = value_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2, ob = old_value_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2;
    if (misaligned(logits_p1, lb) || misaligned(logits_p2, lb) || misaligned(act_p1, ab) || misaligned(act_p2, ab) ||
        misaligned(old_logp_p1, 4) || misaligned(old_logp_p2, 4) || misaligned(adv_p1, 4) || misaligned(adv_p2, 4) ||
        misaligned(ret_p1, 4) || misaligned(ret_p2, 4) || misaligned(values_p1, vb) || misaligned(values_p2, vb) ||
        misaligned(old_values_p1, ob) || misaligned(old_values_p2, ob) || misaligned(adv_norm, 4) || misaligned(grad_logits_p1, lb) ||
        misaligned(grad_logits_p2, lb) || misaligned(grad_values_p1, vb) || misaligned(grad_values_p2, vb) || misaligned(stats, 4) ||
        misaligned(workspace, 16))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const int64_t waves = waves_of(n);
    const LossArgs a{Common{{logits_p1, logits_p2}, {act_p1, act_p2}, {nullptr, nullptr}, {nullptr, nullptr}, n, logit_pitch,
                            num_actions, action_format, logit_pitch <= kMaxStagedPitch ? magic_of(logit_pitch) : 0u,
                            magic_of(num_actions)},
                     {old_logp_p1, old_logp_p2}, {adv_p1, adv_p2}, {ret_p1, ret_p2}, {values_p1, values_p2},
                     {old_values_p1, old_values_p2}, adv_norm, {grad_logits_p1, grad_logits_p2}, {grad_values_p1, grad_values_p2},
                     (float*)workspace, value_pitch, grad_pitch, grad_value_pitch, waves, value_format, old_value_format, clip,
                     value_clip, vf_coef, ent_coef};
    const dim3 grid((unsigned)waves, both ? 2 : 1);
    switch (logit_format) {
        case PZ_POLICY_LOGIT_FLOAT32:
            hipLaunchKernelGGL((loss_kernel<PZ_POLICY_LOGIT_FLOAT32>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        case PZ_POLICY_LOGIT_FLOAT16:
            hipLaunchKernelGGL((loss_kernel<PZ_POLICY_LOGIT_FLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        default:
            hipLaunchKernelGGL((loss_kernel<PZ_POLICY_LOGIT_BFLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
    }
    const FinishArgs f{(const float*)workspace, stats, n, waves, vf_coef, ent_coef};
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1, both ? 2 : 1), dim3(kFinishThreads), 0, (hipStream_t)stream, f);
    return (int)hipGetLastError();
}

}  // extern "C"
