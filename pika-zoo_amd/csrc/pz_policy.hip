// libpikazoo_policy.so (include/pikazoo_policy.h): the categorical policy head over [n, A] logits -- sample + log-prob +
// entropy in one launch, log-prob + entropy of given actions, and the backward of that pair.
//
// One lane owns one game's row and does the serial work over it; blockIdx.y = agent; one wave (64 consecutive games) per
// workgroup.  A wave's 64 rows are one contiguous span of (rows - 1) * pitch + A elements, and 64 lanes each walking a
// 72-byte row would be 64 strided segments per load instruction.  So the span is read in 16-byte pieces, lane after lane
// (stage_span), and transposed through LDS: every element lands as a float32 at [row * stride + column] of the wave's
// image, where its lane then finds its row.  The image's row stride is A | 1 dwords: an odd stride puts the 32 lanes of a
// ds_read_b32 group on 32 different banks (A = 18 as it stands would put lanes l and l + 16 on one bank, 2-way).
//   * A span that starts or ends off 16-byte alignment (an odd pitch in a 2-byte format, a base pointer one element into
//     a buffer) keeps the wide loads for its aligned middle: only the elements in front of the first and behind the last
//     whole 16-byte piece are loaded one by one, by one lane each.  Nothing outside the span is read.
//   * The wide loads are issued a group at a time with no condition around any of them (a lane whose piece lies behind
//     the span re-reads the last whole piece and drops it), so that they are all in flight together.
//   * A pitch above kMaxStagedPitch (a view into a much wider tensor) would mostly load pad columns: there the A live
//     columns are gathered element by element, 64 consecutive (row, column) pairs per instruction.
// The passes over the row re-read the image (A is a runtime value: a register array indexed by it would live in scratch).
// The backward writes its row into the same image and the wave stores it transposed back: whole 16-byte pieces where the
// gradient rows are dense (grad_pitch == A), element by element where pad columns, which are not written, lie between.
//
// The logit format is a compile-time instantiation (3 formats x 3 launches = 9 kernels); A, the pitches and the action
// format are runtime values.  Contraction may stay on -- nothing here is pinned against a host restatement -- but the one
// product-sum whose bits two kernels must share (the entropy's) is an explicit fmaf, and the row statistics of all three
// kernels are the same function.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_policy.h"
// the formats, the staged image, row_stats, load_action and store_dense: shared with pz_ppo.hip, which runs the same text
#include "pz_policy_rows.hpp"

namespace pz_policy {

struct SampleArgs {
    Common c;
    const uint64_t* step_dev;
    uint64_t step;
    int64_t first_game;
    uint32_t key0, key1;
};

struct BackwardArgs {
    Common c;
    const float* glogp[2];
    const float* gent[2];
    void* grad[2];
    int64_t grad_pitch;
};

// step 5's log-prob, and the stores of one game
__device__ __forceinline__ void finish(const Common& c, int side, int64_t g, const float* row, const RowStats& s, int a)
{
    const bool in_range = (unsigned)a < (unsigned)c.A;
    const float la = row[in_range ? a : 0];
    const float nan = __uint_as_float(0x7FC00000u);
    const float logp = (la - s.m) - s.logS;
    if (c.logp[side]) c.logp[side][g] = (s.bad || !in_range) ? nan : logp;
    if (c.ent[side]) c.ent[side][g] = s.bad ? nan : s.H;
}

// (philox4x32_10: pz_policy_rows.hpp, shared with pz_act.hip)
template <int LF>
__global__ void __launch_bounds__(kLanes) sample_kernel(const SampleArgs a)
{
    __shared__ float image[kLanes * kMaxStride];
    const Common& c = a.c;
    const int lane = threadIdx.x, side = blockIdx.y;
    const int64_t g0 = (int64_t)blockIdx.x * kLanes;
    const int rows = (int)min((int64_t)kLanes, c.n - g0);
    const int stride = c.A | 1;
    load_image<LF>(c, side, g0, rows, stride, image, lane);
    if (lane >= rows) return;
    const int64_t g = g0 + lane;
    const float* row = image + lane * stride;
    const RowStats s = row_stats(row, c.A);
    // step 3: the draw (pz_policy_rows.hpp)
    const uint64_t T = a.step + (a.step_dev ? *a.step_dev : 0);
    const float u = draw_uniform((uint64_t)(a.first_game + g), T, a.key0, a.key1, side);
    // step 4: the same sums again (the same expf of the same arguments: the same c_i), counted against the threshold
    const float thr = u * s.S;
    float cum = 0.0f;
    int act = 0;
    for (int i = 0; i < c.A - 1; ++i) {
        cum += expf(row[i] - s.m);
        act += cum <= thr;
    }
    act = s.bad ? 0 : min(act, s.last);
    if (c.action_format == PZ_POLICY_ACTION_INT32)
        ((int32_t*)c.act[side])[g] = act;
    else
        ((int64_t*)c.act[side])[g] = act;
    finish(c, side, g, row, s, act);
}

template <int LF>
__global__ void __launch_bounds__(kLanes) log_probs_kernel(const Common c)
{
    __shared__ float image[kLanes * kMaxStride];
    const int lane = threadIdx.x, side = blockIdx.y;
    const int64_t g0 = (int64_t)blockIdx.x * kLanes;
    const int rows = (int)min((int64_t)kLanes, c.n - g0);
    const int stride = c.A | 1;
    load_image<LF>(c, side, g0, rows, stride, image, lane);
    if (lane >= rows) return;
    const int64_t g = g0 + lane;
    const float* row = image + lane * stride;
    const RowStats s = row_stats(row, c.A);
    finish(c, side, g, row, s, load_action(c.act[side], c.action_format, g));
}


template <int LF>
__global__ void __launch_bounds__(kLanes) backward_kernel(const BackwardArgs a)
{
    __shared__ float image[kLanes * kMaxStride];
    using R = typename Raw<LF>::type;
    const Common& c = a.c;
    const int lane = threadIdx.x, side = blockIdx.y;
    const int64_t g0 = (int64_t)blockIdx.x * kLanes;
    const int rows = (int)min((int64_t)kLanes, c.n - g0);
    const int A = c.A, stride = A | 1;
    load_image<LF>(c, side, g0, rows, stride, image, lane);
    if (lane < rows) {
        const int64_t g = g0 + lane;
        float* row = image + lane * stride;
        const RowStats s = row_stats(row, A);
        const int act = load_action(c.act[side], c.action_format, g);
        const float glogp = a.glogp[side] ? a.glogp[side][g] : 0.0f;
        const float gent = a.gent[side] ? a.gent[side][g] : 0.0f;
        const float nan = __uint_as_float(0x7FC00000u);
        for (int i = 0; i < A; ++i) {
            const float d = row[i] - s.m;
            const float e = expf(d);
            const float p = e / s.S;
            float grad = glogp * ((i == act ? 1.0f : 0.0f) - p);
            if (e > 0.0f) grad += gent * (-p * ((d - s.logS) + s.H));
            row[i] = s.bad ? nan : grad;
        }
    }
    __syncthreads();
    R* span = (R*)a.grad[side] + g0 * a.grad_pitch;
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

static dim3 grid_of(int64_t n, bool both) { return dim3((unsigned)((n + kLanes - 1) / kLanes), both ? 2 : 1); }

static Common common_of(const void* l1, const void* l2, int32_t A, int64_t n, int64_t pitch, int32_t action_format, const void* a1,
                        const void* a2, float* lp1, float* lp2, float* e1, float* e2)
{
    return Common{{l1, l2}, {a1, a2}, {lp1, lp2}, {e1, e2}, n, pitch, A, action_format, pitch <= kMaxStagedPitch ? magic_of(pitch) : 0u,
                  magic_of(A)};
}

}  // namespace pz_policy

using namespace pz_policy;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kPolicyBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_policy_build_id(void) { return kPolicyBuildIdRecord + 12; }

int pz_policy_abi_version(void) { return PZ_POLICY_ABI_VERSION; }

int pz_sample_actions(const void* logits_p1, const void* logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                      int64_t logit_pitch, uint64_t seed, int64_t first_game, uint64_t step, const uint64_t* step_dev,
                      int32_t action_format, void* act_p1, void* act_p2, float* logp_p1, float* logp_p2, float* ent_p1, float* ent_p2,
                      void* stream)
{
    if (!logits_p1 || !act_p1) return PZ_E_NULL;
    const bool both = logits_p2 != nullptr;
    if (!paired(act_p1, act_p2, both) || !paired(logp_p1, logp_p2, both) || !paired(ent_p1, ent_p2, both)) return PZ_E_NULL;
    if (bad_sizes(num_actions, n, logit_pitch)) return PZ_E_SIZE;
    if (first_game < 0 || step >= ((uint64_t)1 << 62)) return PZ_E_SIZE;
    if (!known_logit_format(logit_format) || !known_action_format(action_format)) return PZ_E_CONFIG;
    const uintptr_t lb = logit_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2, ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    if (misaligned(logits_p1, lb) || misaligned(logits_p2, lb) || misaligned(act_p1, ab) || misaligned(act_p2, ab) ||
        misaligned(logp_p1, 4) || misaligned(logp_p2, 4) || misaligned(ent_p1, 4) || misaligned(ent_p2, 4) || misaligned(step_dev, 8))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const SampleArgs a{common_of(logits_p1, logits_p2, num_actions, n, logit_pitch, action_format, act_p1, act_p2, logp_p1, logp_p2,
                                 ent_p1, ent_p2),
                       step_dev, step, first_game, (uint32_t)seed, (uint32_t)(seed >> 32)};
    const dim3 grid = grid_of(n, both);
    switch (logit_format) {
        case PZ_POLICY_LOGIT_FLOAT32:
            hipLaunchKernelGGL((sample_kernel<PZ_POLICY_LOGIT_FLOAT32>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        case PZ_POLICY_LOGIT_FLOAT16:
            hipLaunchKernelGGL((sample_kernel<PZ_POLICY_LOGIT_FLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        default:
            hipLaunchKernelGGL((sample_kernel<PZ_POLICY_LOGIT_BFLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
    }
    return (int)hipGetLastError();
}

int pz_action_log_probs(const void* logits_p1, const void* logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                        int64_t logit_pitch, int32_t action_format, const void* act_p1, const void* act_p2, float* logp_p1,
                        float* logp_p2, float* ent_p1, float* ent_p2, void* stream)
{
    if (!logits_p1 || !act_p1) return PZ_E_NULL;
    const bool both = logits_p2 != nullptr;
    if (!paired(act_p1, act_p2, both) || !paired(logp_p1, logp_p2, both) || !paired(ent_p1, ent_p2, both)) return PZ_E_NULL;
    if (bad_sizes(num_actions, n, logit_pitch)) return PZ_E_SIZE;
    if (!known_logit_format(logit_format) || !known_action_format(action_format)) return PZ_E_CONFIG;
    const uintptr_t lb = logit_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2, ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    if (misaligned(logits_p1, lb) || misaligned(logits_p2, lb) || misaligned(act_p1, ab) || misaligned(act_p2, ab) ||
        misaligned(logp_p1, 4) || misaligned(logp_p2, 4) || misaligned(ent_p1, 4) || misaligned(ent_p2, 4))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const Common c = common_of(logits_p1, logits_p2, num_actions, n, logit_pitch, action_format, act_p1, act_p2, logp_p1, logp_p2,
                               ent_p1, ent_p2);
    const dim3 grid = grid_of(n, both);
    switch (logit_format) {
        case PZ_POLICY_LOGIT_FLOAT32:
            hipLaunchKernelGGL((log_probs_kernel<PZ_POLICY_LOGIT_FLOAT32>), grid, dim3(kLanes), 0, (hipStream_t)stream, c);
            break;
        case PZ_POLICY_LOGIT_FLOAT16:
            hipLaunchKernelGGL((log_probs_kernel<PZ_POLICY_LOGIT_FLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, c);
            break;
        default:
            hipLaunchKernelGGL((log_probs_kernel<PZ_POLICY_LOGIT_BFLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, c);
            break;
    }
    return (int)hipGetLastError();
}

int pz_action_log_probs_backward(const void* logits_p1, const void* logits_p2, int32_t logit_format, int32_t num_actions, int64_t n,
                                 int64_t logit_pitch, int32_t action_format, const void* act_p1, const void* act_p2,
                                 const float* glogp_p1, const float* glogp_p2, const float* gent_p1, const float* gent_p2, void* grad_p1,
                                 void* grad_p2, int64_t grad_pitch, void* stream)
{
    if (!logits_p1 || !act_p1 || !grad_p1 || (!glogp_p1 && !gent_p1)) return PZ_E_NULL;
    const bool both = logits_p2 != nullptr;
    if (!paired(act_p1, act_p2, both) || !paired(glogp_p1, glogp_p2, both) || !paired(gent_p1, gent_p2, both) ||
        !paired(grad_p1, grad_p2, both))
        return PZ_E_NULL;
    if (bad_sizes(num_actions, n, logit_pitch) || bad_sizes(num_actions, n, grad_pitch)) return PZ_E_SIZE;
    if (!known_logit_format(logit_format) || !known_action_format(action_format)) return PZ_E_CONFIG;
    const uintptr_t lb = logit_format == PZ_POLICY_LOGIT_FLOAT32 ? 4 : 2, ab = action_format == PZ_POLICY_ACTION_INT32 ? 4 : 8;
    if (misaligned(logits_p1, lb) || misaligned(logits_p2, lb) || misaligned(act_p1, ab) || misaligned(act_p2, ab) ||
        misaligned(glogp_p1, 4) || misaligned(glogp_p2, 4) || misaligned(gent_p1, 4) || misaligned(gent_p2, 4) ||
        misaligned(grad_p1, lb) || misaligned(grad_p2, lb))
        return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    const BackwardArgs a{common_of(logits_p1, logits_p2, num_actions, n, logit_pitch, action_format, act_p1, act_p2, nullptr, nullptr,
                                   nullptr, nullptr),
                         {glogp_p1, glogp_p2}, {gent_p1, gent_p2}, {grad_p1, grad_p2}, grad_pitch};
    const dim3 grid = grid_of(n, both);
    switch (logit_format) {
        case PZ_POLICY_LOGIT_FLOAT32:
            hipLaunchKernelGGL((backward_kernel<PZ_POLICY_LOGIT_FLOAT32>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        case PZ_POLICY_LOGIT_FLOAT16:
            hipLaunchKernelGGL((backward_kernel<PZ_POLICY_LOGIT_FLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
        default:
            hipLaunchKernelGGL((backward_kernel<PZ_POLICY_LOGIT_BFLOAT16>), grid, dim3(kLanes), 0, (hipStream_t)stream, a);
            break;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
