// gae_variants.hip -- pz_gae's shipped form against a variant that was measured and not shipped (diagnostic)
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -Ipika-zoo_amd/csrc tools/gae_variants.hip -o tools/bin/gae_variants
//   tools/bin/gae_variants [rounds]
//
// Compiles the library's own translation unit (csrc/pz_learn.hip is included as text: the same Lane and row arithmetic the
// product runs, under the same schedule of csrc/pz_traj_scan.hpp) and beside it
//   pair      both agents in ONE thread: the flags loaded once, two independent chains per lane, half the waves;
// float32 rewards and values, both agents.  Per cell (games x rows) the forms are launched interleaved, each sample a
// batch of launches between two HIP events; medians and spread (max - min) over the rounds.  Before a form is timed its
// outputs must equal the shipped form's bit for bit (which the GPU tests hold to the judge).
#include "pz_learn.hip"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

namespace variants {
using namespace pz_learn;

constexpr int RF = PZ_GAE_REWARD_FLOAT32, VF = PZ_GAE_VALUE_FLOAT32;

// both agents' lanes as one lane state of the shared schedule (pz_traj_scan.hpp: scan_rows): the flags loaded once
struct Pair {
    struct Chunk {
        uint32_t r1[kChunk], r2[kChunk], v1[kChunk], v2[kChunk];
        uint8_t d[kChunk];
    };
    Lane<RF, VF> s1, s2;  // (the pitches and the flags are s1's)

    __device__ __forceinline__ void scan_row(int64_t t)
    {
        const uint8_t d = s1.term[t * s1.term_pitch];
        s1.scan(t, s1.rew[t * s1.rew_pitch], s1.val[t * s1.val_pitch], d);
        s2.scan(t, s2.rew[t * s1.rew_pitch], s2.val[t * s1.val_pitch], d);
    }

    __device__ __forceinline__ void load_chunk(int64_t t0, Chunk& c) const
    {
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            c.r1[i] = s1.rew[(t0 + i) * s1.rew_pitch];
            c.r2[i] = s2.rew[(t0 + i) * s1.rew_pitch];
            c.v1[i] = s1.val[(t0 + i) * s1.val_pitch];
            c.v2[i] = s2.val[(t0 + i) * s1.val_pitch];
            c.d[i] = s1.term[(t0 + i) * s1.term_pitch];
        }
    }

    __device__ __forceinline__ void scan_chunk(int64_t t0, const Chunk& c)
    {
#pragma unroll
        for (int i = kChunk - 1; i >= 0; --i) {
            s1.scan(t0 + i, c.r1[i], c.v1[i], c.d[i]);
            s2.scan(t0 + i, c.r2[i], c.v2[i], c.d[i]);
        }
    }
};

// the shipped kernel's set-up (pz_learn.hip: gae_kernel), two chains per lane
__global__ void __launch_bounds__(kLanes) gae_pair_kernel(const GaeArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (g >= a.n) return;
    Pair p;
    Lane<RF, VF>&s1 = p.s1, &s2 = p.s2;
    s1.rew = (const uint32_t*)a.rew_p1 + g, s2.rew = (const uint32_t*)a.rew_p2 + g;
    s1.val = (const uint32_t*)a.val_p1 + g, s2.val = (const uint32_t*)a.val_p2 + g;
    s1.term = s2.term = a.term + g;
    s1.adv = a.adv_p1 + g, s2.adv = a.adv_p2 + g;
    s1.ret = a.ret_p1 + g, s2.ret = a.ret_p2 + g;
    s1.rew_pitch = s2.rew_pitch = a.rew_pitch, s1.term_pitch = s2.term_pitch = a.term_pitch;
    s1.val_pitch = s2.val_pitch = a.val_pitch, s1.out_pitch = s2.out_pitch = a.out_pitch;
    s1.gamma = s2.gamma = a.gamma, s1.gl = s2.gl = a.gl;
    s1.v_next = value_of<VF>(s1.val[a.k * a.val_pitch]), s2.v_next = value_of<VF>(s2.val[a.k * a.val_pitch]);
    s1.a_next = s2.a_next = 0.0f;
    scan_rows(p, a.k);
}

}  // namespace variants

struct Cell {
    int64_t n;
    int k;
};

static float median(std::vector<float> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 7;
    const Cell cells[] = {{65536, 32}, {65536, 128}, {524288, 32}, {4096, 128}, {65536, 33}};
    const float gamma = 0.99f, lam = 0.95f;
    hipStream_t stream;
    CHECK(hipStreamCreate(&stream));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (const Cell& c : cells) {
        const int64_t n = c.n, rows = c.k, cells_in = rows * n, cells_val = (rows + 1) * n;
        std::vector<float> h_r(2 * cells_in), h_v(2 * cells_val);
        std::vector<uint8_t> h_d(cells_in);
        uint32_t x = 12345u + (uint32_t)n + (uint32_t)rows;
        auto next = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        for (auto& r : h_r) r = (float)((int)(next() % 3) - 1) + 0.01f * (float)(next() % 3);
        for (auto& v : h_v) v = ((float)(next() % 60001) - 30000.0f) / 10000.0f;
        for (auto& d : h_d) d = next() % 50 == 0;
        float *rew, *val, *out_a, *out_b;
        uint8_t* term;
        CHECK(hipMalloc(&rew, h_r.size() * 4));
        CHECK(hipMalloc(&val, h_v.size() * 4));
        CHECK(hipMalloc(&term, h_d.size()));
        CHECK(hipMalloc(&out_a, 4 * cells_in * 4));
        CHECK(hipMalloc(&out_b, 4 * cells_in * 4));
        CHECK(hipMemcpy(rew, h_r.data(), h_r.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(val, h_v.data(), h_v.size() * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(term, h_d.data(), h_d.size(), hipMemcpyHostToDevice));
        CHECK(hipMemset(out_a, 0xFF, 4 * cells_in * 4));
        CHECK(hipMemset(out_b, 0xEE, 4 * cells_in * 4));
        auto shipped = [&](float* o) {
            const int rc = pz_gae(rew, rew + cells_in, 1, term, val, val + cells_val, 0, (int32_t)rows, n, n, n, n, n, gamma, lam, o,
                                  o + cells_in, o + 2 * cells_in, o + 3 * cells_in, stream);
            if (rc != 0) {
                fprintf(stderr, "pz_gae: %d\n", rc);
                exit(1);
            }
        };
        auto pair = [&](float* o) {
            const pz_learn::GaeArgs a{rew, rew + cells_in, term, val, val + cells_val, o, o + cells_in, o + 2 * cells_in,
                                      o + 3 * cells_in, n, n, n, n, n, (int32_t)rows, gamma, gamma * lam};
            hipLaunchKernelGGL(variants::gae_pair_kernel, dim3((unsigned)((n + pz_learn::kLanes - 1) / pz_learn::kLanes)),
                               dim3(pz_learn::kLanes), 0, stream, a);
            CHECK(hipGetLastError());
        };
        shipped(out_a);
        pair(out_b);
        CHECK(hipStreamSynchronize(stream));
        std::vector<uint32_t> got_a(4 * cells_in), got_b(4 * cells_in);
        CHECK(hipMemcpy(got_a.data(), out_a, got_a.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(got_b.data(), out_b, got_b.size() * 4, hipMemcpyDeviceToHost));
        if (memcmp(got_a.data(), got_b.data(), got_a.size() * 4) != 0) {
            fprintf(stderr, "pair differs from the shipped form at %lld x %d\n", (long long)n, c.k);
            return 1;
        }
        const double bytes = 2.0 * (cells_in * 4.0 + cells_val * 4.0 + 2.0 * cells_in * 4.0) + cells_in;
        const int reps = (int)std::max<int64_t>(20, std::min<int64_t>(2000, (int64_t)(4.0e9 / bytes * 25)));
        std::vector<float> t_ship, t_pair;
        for (int r = 0; r < rounds; ++r) {
            for (int which = 0; which < 2; ++which) {
                const bool first = (which == 0) == (r % 2 == 0);
                if (first) shipped(out_a); else pair(out_b);  // untimed lead-in
                CHECK(hipEventRecord(e0, stream));
                for (int i = 0; i < reps; ++i) {
                    if (first) shipped(out_a); else pair(out_b);
                }
                CHECK(hipEventRecord(e1, stream));
                CHECK(hipEventSynchronize(e1));
                float ms;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                (first ? t_ship : t_pair).push_back(ms * 1e3f / reps);
            }
        }
        auto spread = [](const std::vector<float>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
        printf("%7lld games x %3d rows (%d launches per sample, %d rounds, bits equal): shipped %8.2f us (spread %.2f)  pair %8.2f us "
               "(spread %.2f)  pair / shipped %.3f\n", (long long)n, c.k, reps, rounds, median(t_ship), spread(t_ship), median(t_pair),
               spread(t_pair), median(t_pair) / median(t_ship));
        fflush(stdout);
        CHECK(hipFree(rew));
        CHECK(hipFree(val));
        CHECK(hipFree(term));
        CHECK(hipFree(out_a));
        CHECK(hipFree(out_b));
    }
    return 0;
}
