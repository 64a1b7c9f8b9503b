// libpikazoo_optim.so: the optimizer step -- the global gradient norm, the clip and the Adam / AdamW update of one or two
// nets' parameters in ONE launch (C ABI and the definition: include/pikazoo_optim.h; the shape and its reasons: DESIGN.md 4.19).
//
// One workgroup of 1024 threads per group.  The groups arrive BY VALUE in the kernel's arguments; sixteen threads turn their
// group's tensor list into a table in LDS (pointers, the first element and the first chunk of every tensor), and both phases
// walk the CONCATENATION of the tensors through that table, so that a thread's loads of one round trip come from whichever
// tensors its indices fall into: six small tensors cost one memory round trip, not six.
//   phase 1: thread j squares elements j, j + 1024, ... of the concatenated gradients into a float64 partial; a fixed tree of
//            wave shuffles and LDS gives every thread the same sum (the header's order).
//   phase 2: a CHUNK is four consecutive elements of one tensor behind a scalar head of 0..3 elements that brings the
//            parameter to a 16-byte boundary; thread j takes chunks j, j + 1024, ...  A full chunk of a tensor whose four bases
//            share their offset within 16 bytes moves as 16-byte accesses, anything else as 4-byte accesses.
// Thread 0 stores t, skipped and the statistics at the end with ordinary stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pikazoo_hip.h"
#include "pikazoo_optim.h"

namespace pz_optim {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kNormUnroll = 8;   // gradient loads in flight per thread in phase 1
constexpr int kChunkUnroll = 2;  // chunks (4 x 4 loads of 16 bytes) in flight per thread in phase 2

// the configuration as the kernel takes it: the float64 hyperparameters that meet t or a device lr in float64, and the
// float32 constants of the header's definition, each rounded from float64 once on the host
struct Consts {
    double lr, beta1, beta2, weight_decay;
    float omb1, omb2, beta2_f, eps_f, wd_f, max_norm_f;
    int32_t decoupled, skip_nonfinite;
};

struct Args {
    pz_optim_group group[PZ_OPTIM_MAX_GROUPS];
    Consts cfg;
};

// the tensors are global memory: a pointer that comes back from the LDS table says so again (global, not flat, accesses)
using gfloat = __attribute__((address_space(1))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using gfloat4 = __attribute__((address_space(1))) f32x4;
__device__ __forceinline__ gfloat* as_global(const float* p) { return (gfloat*)p; }

struct Scalars {  // the per-call constants of the header's definition
    float coef, step_size, omb1, omb2, beta2, bc2, eps, wd, decay;
    bool coupled, decoupled;
};

// one element, the header's lines in their order; nothing is contracted
__device__ __forceinline__ void adam_element(const Scalars& s, float& p, float g, float& m, float& v)
{
#pragma clang fp contract(off)
    float g1 = s.coef * g;
    if (s.coupled) g1 = __builtin_fmaf(s.wd, p, g1);
    if (s.decoupled) p = p * s.decay;
    const float d = g1 - m;
    m = __builtin_fmaf(s.omb1, d, m);
    const float a = s.beta2 * v;
    const float gg = g1 * g1;
    v = __builtin_fmaf(s.omb2, gg, a);
    const float r = __fsqrt_rn(v);
    const float q = __fdiv_rn(r, s.bc2);
    const float den = q + s.eps;
    const float u = __fdiv_rn(m, den);
    p = __builtin_fmaf(-s.step_size, u, p);
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const Args args)
{
    __shared__ float* s_p[PZ_OPTIM_MAX_TENSORS];
    __shared__ const float* s_g[PZ_OPTIM_MAX_TENSORS];
    __shared__ float* s_m[PZ_OPTIM_MAX_TENSORS];
    __shared__ float* s_v[PZ_OPTIM_MAX_TENSORS];
    __shared__ int32_t s_elem[PZ_OPTIM_MAX_TENSORS + 1];   // first concatenated element of tensor k; [count..16] = the total
    __shared__ int32_t s_chunk[PZ_OPTIM_MAX_TENSORS + 1];  // first chunk of tensor k; [count..16] = the total
    __shared__ int32_t s_head[PZ_OPTIM_MAX_TENSORS];       // elements in front of the first 4-element chunk (0..3)
    __shared__ int32_t s_vector[PZ_OPTIM_MAX_TENSORS];     // 1: the four bases share their offset within 16 bytes
    __shared__ double s_wave[kWaves];
    __shared__ float s_bc[2];

    const pz_optim_group& grp = args.group[blockIdx.x];
    const Consts& cfg = args.cfg;
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int count = grp.count;

    // ---- the table: thread k <= 16 sums the tensors in front of tensor k (k == 16, and every k >= count: the totals)
    if (tid <= PZ_OPTIM_MAX_TENSORS) {
        int32_t elems = 0, chunks = 0, my_numel = 0, my_head = 0, my_vector = 0;
#pragma unroll
        for (int i = 0; i < PZ_OPTIM_MAX_TENSORS; ++i) {
            if (i < count) {
                const pz_optim_tensor t = grp.tensors[i];
                const int32_t numel = (int32_t)t.numel;
                const uintptr_t off = (uintptr_t)t.param & 15;
                const bool same = ((uintptr_t)t.grad & 15) == off && ((uintptr_t)t.exp_avg & 15) == off && ((uintptr_t)t.exp_avg_sq & 15) == off;
                int32_t head = same ? (int32_t)(((16 - off) & 15) >> 2) : 0;
                head = head < numel ? head : numel;
                if (i == tid) {
                    s_p[i] = t.param;
                    s_g[i] = t.grad;
                    s_m[i] = t.exp_avg;
                    s_v[i] = t.exp_avg_sq;
                    my_numel = numel;
                    my_head = head;
                    my_vector = same ? 1 : 0;
                }
                if (i < tid) {
                    elems += numel;
                    chunks += (head > 0 ? 1 : 0) + ((numel - head + 3) >> 2);
                }
            }
        }
        s_elem[tid] = elems;
        s_chunk[tid] = chunks;
        if (tid < PZ_OPTIM_MAX_TENSORS) {
            s_head[tid] = my_head;
            s_vector[tid] = my_vector;
        }
        (void)my_numel;
    }
    const int64_t t_old = grp.step[0];
    const int64_t skipped_old = grp.step[1];
    const double lr = grp.lr_device != nullptr ? (double)*grp.lr_device : cfg.lr;
    __syncthreads();

    // ---- phase 1: the float64 sum of squares, in the header's order
    const int total = s_elem[PZ_OPTIM_MAX_TENSORS];
    double acc = 0.0;
    {
        int k = 0;
        for (int e0 = tid; e0 < total; e0 += kThreads * kNormUnroll) {
            float gv[kNormUnroll];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int e = e0 + u * kThreads;
                gv[u] = 0.0f;
                if (e < total) {
                    while (e >= s_elem[k + 1]) ++k;  // (s_elem[count] == total > e: k stays below count)
                    gv[u] = as_global(s_g[k])[e - s_elem[k]];
                }
            }
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) acc += (double)gv[u] * (double)gv[u];  // (+0 for an index beyond the end)
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) s_wave[wave] = acc;
    // the last wave has the least to square: its first two lanes take the bias corrections from t in float64 meanwhile
    // (lane 0: step_size = lr / (1 - beta1^t), lane 1: bc2 = sqrt(1 - beta2^t), each rounded to float32 once)
    if (wave == kWaves - 1 && lane < 2) {
        const double c = 1.0 - pow(lane == 0 ? cfg.beta1 : cfg.beta2, (double)(t_old + 1));
        s_bc[lane] = (float)(lane == 0 ? lr / c : sqrt(c));
    }
    __syncthreads();
    double S = s_wave[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) S += s_wave[w];
    const float norm = (float)sqrt(S);
    const bool clipping = cfg.max_norm_f > 0.0f && cfg.max_norm_f < INFINITY;
    Scalars s;
    {
#pragma clang fp contract(off)
        s.coef = 1.0f;
        if (clipping) {
            const float c = __fdiv_rn(cfg.max_norm_f, norm + 1e-6f);
            s.coef = c > 1.0f ? 1.0f : c;
        }
        s.step_size = s_bc[0];
        s.bc2 = s_bc[1];
        s.omb1 = cfg.omb1;
        s.omb2 = cfg.omb2;
        s.beta2 = cfg.beta2_f;
        s.eps = cfg.eps_f;
        s.wd = cfg.wd_f;
        s.decay = (float)(1.0 - lr * cfg.weight_decay);
        s.coupled = cfg.weight_decay != 0.0 && cfg.decoupled == 0;
        s.decoupled = cfg.weight_decay != 0.0 && cfg.decoupled != 0;
    }
    const bool skip = cfg.skip_nonfinite != 0 && !isfinite(norm);
    if (tid == 0) {
        if (skip)
            grp.step[1] = skipped_old + 1;
        else
            grp.step[0] = t_old + 1;
        if (grp.stats != nullptr) {
            grp.stats[0] = norm;
            grp.stats[1] = s.coef;
        }
    }
    if (skip) return;

    // ---- phase 2: every thread updates its chunks
    const int chunks = s_chunk[PZ_OPTIM_MAX_TENSORS];
    int k = 0;
    for (int c0 = tid; c0 < chunks; c0 += kThreads * kChunkUnroll) {
        float p[kChunkUnroll][4], g[kChunkUnroll][4], m[kChunkUnroll][4], v[kChunkUnroll][4];
        gfloat *pp[kChunkUnroll], *pm[kChunkUnroll], *pv[kChunkUnroll];
        int len[kChunkUnroll];
        bool vec[kChunkUnroll];
#pragma unroll
        for (int u = 0; u < kChunkUnroll; ++u) {
            const int c = c0 + u * kThreads;
            len[u] = 0;
            vec[u] = false;
            pp[u] = pm[u] = pv[u] = nullptr;
#pragma unroll
            for (int e = 0; e < 4; ++e) p[u][e] = g[u][e] = m[u][e] = v[u][e] = 0.0f;
            if (c < chunks) {
                while (c >= s_chunk[k + 1]) ++k;  // (s_chunk[count] == chunks > c: k stays below count)
                const int numel = s_elem[k + 1] - s_elem[k];
                const int head = s_head[k];
                const int i = c - s_chunk[k];  // the chunk's index within its tensor
                int start, n;
                if (head > 0 && i == 0) {
                    start = 0;
                    n = head;
                } else {
                    start = head + 4 * (i - (head > 0 ? 1 : 0));
                    n = numel - start < 4 ? numel - start : 4;
                }
                len[u] = n;
                vec[u] = s_vector[k] != 0 && n == 4 && start >= head;
                pp[u] = as_global(s_p[k]) + start;
                pm[u] = as_global(s_m[k]) + start;
                pv[u] = as_global(s_v[k]) + start;
                const gfloat* pg = as_global(s_g[k]) + start;
                if (vec[u]) {
                    const f32x4 P = *(const gfloat4*)pp[u], G = *(const gfloat4*)pg, M = *(const gfloat4*)pm[u], V = *(const gfloat4*)pv[u];
                    p[u][0] = P.x, p[u][1] = P.y, p[u][2] = P.z, p[u][3] = P.w;
                    g[u][0] = G.x, g[u][1] = G.y, g[u][2] = G.z, g[u][3] = G.w;
                    m[u][0] = M.x, m[u][1] = M.y, m[u][2] = M.z, m[u][3] = M.w;
                    v[u][0] = V.x, v[u][1] = V.y, v[u][2] = V.z, v[u][3] = V.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (e < n) {
                            p[u][e] = pp[u][e];
                            g[u][e] = pg[e];
                            m[u][e] = pm[u][e];
                            v[u][e] = pv[u][e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kChunkUnroll; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) adam_element(s, p[u][e], g[u][e], m[u][e], v[u][e]);  // (an unused slot computes on zeros)
            if (vec[u]) {
                *(gfloat4*)pp[u] = f32x4{p[u][0], p[u][1], p[u][2], p[u][3]};
                *(gfloat4*)pm[u] = f32x4{m[u][0], m[u][1], m[u][2], m[u][3]};
                *(gfloat4*)pv[u] = f32x4{v[u][0], v[u][1], v[u][2], v[u][3]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (e < len[u]) {
                        pp[u][e] = p[u][e];
                        pm[u][e] = m[u][e];
                        pv[u][e] = v[u][e];
                    }
                }
            }
        }
    }
}

}  // namespace pz_optim

using namespace pz_optim;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kOptimBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_optim_build_id(void) { return kOptimBuildIdRecord + 12; }

int pz_optim_abi_version(void) { return PZ_OPTIM_ABI_VERSION; }

int pz_adam_step(const pz_optim_group* groups, int32_t n_groups, const pz_adam_config* cfg, void* stream)
{
    if (groups == nullptr || cfg == nullptr) return PZ_E_NULL;
    const int32_t seen = n_groups < 0 ? 0 : (n_groups > PZ_OPTIM_MAX_GROUPS ? PZ_OPTIM_MAX_GROUPS : n_groups);
    auto tensors_of = [](const pz_optim_group& g) { return g.count < 0 ? 0 : (g.count > PZ_OPTIM_MAX_TENSORS ? PZ_OPTIM_MAX_TENSORS : g.count); };
    for (int32_t a = 0; a < seen; ++a) {
        const pz_optim_group& g = groups[a];
        if (g.step == nullptr) return PZ_E_NULL;
        for (int32_t k = 0; k < tensors_of(g); ++k) {
            const pz_optim_tensor& t = g.tensors[k];
            if (t.param == nullptr || t.grad == nullptr || t.exp_avg == nullptr || t.exp_avg_sq == nullptr) return PZ_E_NULL;
        }
    }
    if (n_groups < 1 || n_groups > PZ_OPTIM_MAX_GROUPS) return PZ_E_SIZE;
    for (int32_t a = 0; a < n_groups; ++a) {
        const pz_optim_group& g = groups[a];
        if (g.count < 1 || g.count > PZ_OPTIM_MAX_TENSORS) return PZ_E_SIZE;
        int64_t total = 0;
        for (int32_t k = 0; k < g.count; ++k) {
            if (g.tensors[k].numel < 1 || g.tensors[k].numel > PZ_OPTIM_MAX_ELEMENTS) return PZ_E_SIZE;
            total += g.tensors[k].numel;
        }
        if (total > PZ_OPTIM_MAX_ELEMENTS) return PZ_E_SIZE;
    }
    // (every comparison is false for a NaN: the conditions are written so that a NaN fails them)
    if (!(cfg->lr >= 0.0) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) ||
        !(cfg->eps >= 0.0) || !(cfg->weight_decay >= 0.0) || (cfg->decoupled != 0 && cfg->decoupled != 1) ||
        (cfg->skip_nonfinite != 0 && cfg->skip_nonfinite != 1))
        return PZ_E_CONFIG;
    for (int32_t a = 0; a < n_groups; ++a) {
        const pz_optim_group& g = groups[a];
        if (((uintptr_t)g.step & 7) || ((uintptr_t)g.stats & 3) || ((uintptr_t)g.lr_device & 3)) return PZ_E_ALIGN;
        for (int32_t k = 0; k < g.count; ++k) {
            const pz_optim_tensor& t = g.tensors[k];
            if (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 3) return PZ_E_ALIGN;
        }
    }
    Args args;
    for (int32_t a = 0; a < PZ_OPTIM_MAX_GROUPS; ++a) {
        args.group[a] = groups[a < n_groups ? a : 0];
        for (int32_t k = args.group[a].count; k < PZ_OPTIM_MAX_TENSORS; ++k) args.group[a].tensors[k] = pz_optim_tensor{0, nullptr, nullptr, nullptr, nullptr};
    }
    args.cfg = Consts{cfg->lr, cfg->beta1, cfg->beta2, cfg->weight_decay, (float)(1.0 - cfg->beta1), (float)(1.0 - cfg->beta2),
                      (float)cfg->beta2, (float)cfg->eps, (float)cfg->weight_decay, (float)cfg->max_grad_norm, cfg->decoupled,
                      cfg->skip_nonfinite};
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0, (hipStream_t)stream, args);
    return (int)hipGetLastError();
}

}  // extern "C"
