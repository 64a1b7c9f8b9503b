// libpikazoo_batch.so: the data movement of a PPO iteration -- one policy step's records into the rollout buffers
// (pz_batch_copy) and every tensor of a shuffled minibatch out of them (pz_batch_gather), each in ONE launch (C ABI and the
// definition: include/pikazoo_batch.h; the shape and its reasons: DESIGN.md 4.20).
//
// One workgroup of 256 threads moves a TILE of 256 output rows of every column.
//   step 1 (gather only): thread i finds the source row of output row j0 + i ONCE -- the Feistel permutation with its cycle
//            walk, or the caller's index -- checks it, writes it to index_out and leaves (r / n, r % n) in LDS.  No column
//            recomputes it.
//   step 2: per column, the tile's output is walked in WORDS of the column's access width (the widest of 16, 8, 4, 2, 1 bytes
//            that divides both bases, the pitches and the row): thread i takes words i, i + 256, ... of the tile, so the 64
//            lanes of a wave store 64 consecutive words of the (dense) destination, and each lane reads its word's row from
//            LDS.  A word's row is word / words_per_row by a multiplication with a reciprocal from the host; a column whose
//            every offset fits 32 bits (the host knows) is addressed with 32-bit offsets from a uniform base.
// The column descriptors arrive BY VALUE in the kernel's arguments.  Nothing is written by a scalar unit and there are no
// atomics: `errors` is set by the lanes that meet a bad index, with the same ordinary store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pikazoo_batch.h"
#include "pikazoo_hip.h"

namespace pz_batch {

constexpr int kThreads = 256;
constexpr int kRows = 256;   // output rows per workgroup
constexpr int kUnroll = 4;   // words in flight per thread
constexpr uint32_t kBadRow = 0xFFFFFFFFu;
enum Mode { kCopy = 0, kPerm = 1, kIndex = 2 };

struct Column {
    const char* src;
    char* dst;
    int64_t step_pitch, game_pitch, dst_pitch;
    uint32_t words;   // words per row: row_bytes / width
    uint32_t magic;   // floor(2^32 / words) + 1: word / words == umulhi(word, magic) for word < 2^17 (words == 1: unused)
    uint32_t width;   // bytes per word: 16, 8, 4, 2 or 1
    uint32_t narrow;  // 1: every offset of this column from its bases fits uint32
};

struct Args {
    Column col[PZ_BATCH_MAX_COLUMNS];
    int32_t ncols;
    uint32_t n, M, B;  // games per step, flat rows, output rows (each <= 2^31)
    uint32_t minibatches, hb;
    uint32_t key0, key1;
    uint64_t counter;
    const uint64_t* counter_dev;
    const int64_t* index_in;
    int64_t* index_out;
    uint32_t* errors;
};

using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;

// Philox4x32-10 (Salmon et al., SC'11), the whole block
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        c0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        c1 = (uint32_t)p1;
        c2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
}

__device__ __forceinline__ uint32_t mix(uint32_t v)
{
    v *= 0x9E3779B1u;
    v ^= v >> 15;
    v *= 0x85EBCA77u;
    v ^= v >> 13;
    v *= 0xC2B2AE3Du;
    v ^= v >> 16;
    return v;
}

// the header's perm(p): six Feistel rounds on two halves of hb bits, walked until the value falls below M
__device__ __forceinline__ uint32_t perm(uint32_t p, const uint32_t (&K)[6], uint32_t hb, uint32_t M)
{
    const uint32_t mask = (1u << hb) - 1u, down = 32u - hb;
    uint32_t x = p;
    do {
        uint32_t L = x >> hb, R = x & mask;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const uint32_t next = L ^ (mix(R ^ K[r]) >> down);
            L = R;
            R = next;
        }
        x = (L << hb) | R;
    } while (x >= M);
    return x;
}

// One column of one tile.  OFF is the type of a byte offset from the column's (wave-uniform) bases: uint32_t where the host
// found that every offset fits (the column's `narrow`), uint64_t otherwise.
template <int MODE, typename T, typename OFF>
__device__ __forceinline__ void move_column(const Column& c, uint32_t j0, uint32_t rows, uint32_t tid, const u32x2* s_row)
{
    const uint32_t words = c.words, magic = c.magic;
    const uint32_t total = rows * words;  // <= 256 * 512
    const OFF step_pitch = (OFF)c.step_pitch, game_pitch = (OFF)c.game_pitch, dst_pitch = (OFF)c.dst_pitch;
    const global_ptr<char> dst = (global_ptr<char>)(c.dst + (int64_t)j0 * c.dst_pitch);
    // (a copy's source row is the output row: the tile's base takes the 64-bit part)
    const global_ptr<const char> src = (global_ptr<const char>)(MODE == kCopy ? c.src + (int64_t)j0 * c.game_pitch : c.src);
    for (uint32_t w0 = tid; w0 < total; w0 += kThreads * kUnroll) {
        T v[kUnroll];
        OFF to[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint32_t w = w0 + u * kThreads;
            v[u] = T{};
            to[u] = 0;
            if (w < total) {
                const uint32_t row = words == 1 ? w : __umulhi(w, magic);
                const uint32_t at = (w - row * words) * (uint32_t)sizeof(T);
                to[u] = (OFF)row * dst_pitch + at;
                if (MODE == kCopy) {
                    v[u] = *(global_ptr<const T>)(src + ((OFF)row * game_pitch + at));
                } else {
                    const u32x2 tg = s_row[row];
                    if (tg.y != kBadRow) v[u] = *(global_ptr<const T>)(src + ((OFF)tg.x * step_pitch + (OFF)tg.y * game_pitch + at));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (w0 + u * kThreads < total) *(global_ptr<T>)(dst + to[u]) = v[u];
    }
}

template <int MODE, typename T>
__device__ __forceinline__ void move_column(const Column& c, uint32_t j0, uint32_t rows, uint32_t tid, const u32x2* s_row)
{
    if (c.narrow)
        move_column<MODE, T, uint32_t>(c, j0, rows, tid, s_row);
    else
        move_column<MODE, T, uint64_t>(c, j0, rows, tid, s_row);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void batch_kernel(const Args a)
{
    __shared__ u32x2 s_row[kRows];  // (r / n, r % n) of the tile's rows; .y == kBadRow: an index outside [0, M)
    const uint32_t tid = threadIdx.x;
    const uint32_t j0 = blockIdx.x * (uint32_t)kRows;
    const uint32_t rows = a.B - j0 < (uint32_t)kRows ? a.B - j0 : (uint32_t)kRows;

    if (MODE != kCopy) {
        if (tid < rows) {
            const uint32_t j = j0 + tid;
            int64_t r64;
            if (MODE == kIndex) {
                r64 = a.index_in[j];
            } else {
                const uint64_t C = a.counter + (a.counter_dev != nullptr ? *a.counter_dev : 0);
                const uint64_t E = C / a.minibatches;
                const uint32_t m = (uint32_t)(C - E * a.minibatches);
                uint32_t b0[4], b1[4];
                philox4x32_10((uint32_t)E, (uint32_t)(E >> 32), 0u, 0u, a.key0, a.key1, b0);
                philox4x32_10((uint32_t)E, (uint32_t)(E >> 32), 1u, 0u, a.key0, a.key1, b1);
                const uint32_t K[6] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1]};
                r64 = (int64_t)perm(m * a.B + j, K, a.hb, a.M);  // (m * B + j < M <= 2^31)
            }
            if (a.index_out != nullptr) a.index_out[j] = r64;
            u32x2 tg = {0u, kBadRow};
            if ((uint64_t)r64 < (uint64_t)a.M) {
                const uint32_t r = (uint32_t)r64;
                const uint32_t t = r / a.n;
                tg = u32x2{t, r - t * a.n};
            } else if (a.errors != nullptr) {
                *a.errors = 1u;
            }
            s_row[tid] = tg;
        }
        __syncthreads();
    }
    for (int i = 0; i < a.ncols; ++i) {
        const Column& c = a.col[i];
        switch (c.width) {
        case 16: move_column<MODE, u32x4>(c, j0, rows, tid, s_row); break;
        case 8: move_column<MODE, u32x2>(c, j0, rows, tid, s_row); break;
        case 4: move_column<MODE, uint32_t>(c, j0, rows, tid, s_row); break;
        case 2: move_column<MODE, uint16_t>(c, j0, rows, tid, s_row); break;
        default: move_column<MODE, uint8_t>(c, j0, rows, tid, s_row); break;
        }
    }
}

constexpr int64_t kMaxRows = (int64_t)1 << 31;

// (count - 1) * pitch, added onto `sum`; false when it leaves int64
static bool add_span(int64_t count, int64_t pitch, int64_t& sum)
{
    int64_t span;
    return !__builtin_mul_overflow(count - 1, pitch, &span) && !__builtin_add_overflow(sum, span, &sum);
}

// The checks of both entry points that concern the columns, in the header's order, behind the caller's own NULL and size
// checks (`early`: PZ_OK or the caller's size error, which stands behind the columns' NULL check and before their size
// check).  `k` == 0 marks pz_batch_copy: src_step_pitch is ignored.  On PZ_OK `out` holds the device descriptors.
static int plan_columns(const pz_batch_column* cols, int32_t ncols, int early, int64_t k, int64_t n, int64_t B, int late, Column* out)
{
    const bool gather = k > 0;
    const int32_t seen = ncols < 0 ? 0 : (ncols > PZ_BATCH_MAX_COLUMNS ? PZ_BATCH_MAX_COLUMNS : ncols);
    if (ncols > 0 && cols == nullptr) return PZ_E_NULL;
    for (int32_t i = 0; i < seen; ++i)
        if (cols[i].src == nullptr || cols[i].dst == nullptr) return PZ_E_NULL;
    if (ncols < 0 || ncols > PZ_BATCH_MAX_COLUMNS) return PZ_E_SIZE;
    if (early != PZ_OK) return early;
    for (int32_t i = 0; i < ncols; ++i) {
        const pz_batch_column& c = cols[i];
        if (c.row_bytes < 1 || c.row_bytes > PZ_BATCH_MAX_ROW_BYTES) return PZ_E_SIZE;
        if (c.src_game_pitch < c.row_bytes || c.dst_pitch < c.row_bytes || (gather && c.src_step_pitch < c.row_bytes)) return PZ_E_SIZE;
        int64_t src_extent = c.row_bytes, dst_extent = c.row_bytes;
        if (n > 0 && !add_span(n, c.src_game_pitch, src_extent)) return PZ_E_SIZE;
        if (gather && !add_span(k, c.src_step_pitch, src_extent)) return PZ_E_SIZE;
        if (B > 0 && !add_span(B, c.dst_pitch, dst_extent)) return PZ_E_SIZE;
    }
    for (int32_t i = 0; i < ncols; ++i)
        if (cols[i].elem_bytes != 1 && cols[i].elem_bytes != 2 && cols[i].elem_bytes != 4 && cols[i].elem_bytes != 8) return PZ_E_CONFIG;
    for (int32_t i = 0; i < ncols; ++i) {
        const pz_batch_column& c = cols[i];
        const uint64_t bits = (uint64_t)(uintptr_t)c.src | (uint64_t)(uintptr_t)c.dst | (uint64_t)c.src_game_pitch | (uint64_t)c.dst_pitch |
                              (uint64_t)c.row_bytes | (gather ? (uint64_t)c.src_step_pitch : 0);
        if (bits & (uint64_t)(c.elem_bytes - 1)) return PZ_E_ALIGN;
    }
    if (late != PZ_OK) return late;
    for (int32_t i = 0; i < ncols; ++i) {
        const pz_batch_column& c = cols[i];
        const uint64_t bits = (uint64_t)(uintptr_t)c.src | (uint64_t)(uintptr_t)c.dst | (uint64_t)c.src_game_pitch | (uint64_t)c.dst_pitch |
                              (uint64_t)c.row_bytes | (gather ? (uint64_t)c.src_step_pitch : 0);
        uint32_t width = 16;
        while (width > 1 && (bits & (width - 1))) width >>= 1;
        Column& d = out[i];
        d.src = (const char*)c.src;
        d.dst = (char*)c.dst;
        d.step_pitch = gather ? c.src_step_pitch : 0;
        d.game_pitch = c.src_game_pitch;
        d.dst_pitch = c.dst_pitch;
        d.width = width;
        d.words = (uint32_t)c.row_bytes / width;
        d.magic = d.words > 1 ? (uint32_t)(((uint64_t)1 << 32) / d.words) + 1u : 0u;
        // 32-bit offsets: the destination's and a copy's source's from the tile's base (at most 256 rows), a gather's source's
        // from the column's base (the whole extent)
        const int64_t limit = (int64_t)1 << 32;
        int64_t src_reach = gather ? (int64_t)c.row_bytes : 0;
        bool narrow = c.dst_pitch < limit / kRows && c.src_game_pitch < limit / kRows;
        if (gather) narrow = narrow && add_span(n, c.src_game_pitch, src_reach) && add_span(k, c.src_step_pitch, src_reach) && src_reach < limit;
        d.narrow = narrow ? 1u : 0u;
    }
    for (int32_t i = ncols; i < PZ_BATCH_MAX_COLUMNS; ++i) out[i] = Column{nullptr, nullptr, 0, 0, 0, 1, 0, 1, 1};
    return PZ_OK;
}

}  // namespace pz_batch

using namespace pz_batch;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kBatchBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_batch_build_id(void) { return kBatchBuildIdRecord + 12; }

int pz_batch_abi_version(void) { return PZ_BATCH_ABI_VERSION; }

int pz_batch_copy(const pz_batch_column* cols, int32_t ncols, int64_t n, void* stream)
{
    if (ncols == 0) return PZ_E_NULL;
    const int early = (n < 0 || n > kMaxRows) ? PZ_E_SIZE : PZ_OK;
    Args args;
    const int rc = plan_columns(cols, ncols, early, 0, n < 0 ? 0 : n, n < 0 ? 0 : n, PZ_OK, args.col);
    if (rc != PZ_OK) return rc;
    if (n == 0) return PZ_OK;
    args.ncols = ncols;
    args.n = args.M = args.B = (uint32_t)n;
    args.minibatches = 1, args.hb = 1, args.key0 = args.key1 = 0, args.counter = 0;
    args.counter_dev = nullptr, args.index_in = nullptr, args.index_out = nullptr, args.errors = nullptr;
    hipLaunchKernelGGL(batch_kernel<kCopy>, dim3((unsigned)((n + kRows - 1) / kRows)), dim3(kThreads), 0, (hipStream_t)stream, args);
    return (int)hipGetLastError();
}

int pz_batch_gather(const pz_batch_column* cols, int32_t ncols, int64_t k, int64_t n, int64_t minibatches, uint64_t seed, uint64_t counter,
                    const uint64_t* counter_dev, const int64_t* index_in, int64_t* index_out, uint32_t* errors, void* stream)
{
    if (ncols == 0 && index_out == nullptr) return PZ_E_NULL;
    // the sizes of the call itself: they stand behind the columns' NULL check and in front of the columns' own sizes
    int early = PZ_OK;
    int64_t M = 0, B = 0;
    if (k < 1 || n < 0 || n > kMaxRows || k > kMaxRows || k * n > kMaxRows) {
        early = PZ_E_SIZE;
    } else {
        M = k * n;
        if (index_in != nullptr) {
            if (minibatches < 0 || minibatches > kMaxRows) early = PZ_E_SIZE;
            B = minibatches;
        } else if (M > 0) {
            if (minibatches < 1 || minibatches > M || counter >= ((uint64_t)1 << 62)) early = PZ_E_SIZE;
            else B = M / minibatches;
        }
    }
    const int late = (((uintptr_t)counter_dev | (uintptr_t)index_in | (uintptr_t)index_out) & 7) || ((uintptr_t)errors & 3) ? PZ_E_ALIGN : PZ_OK;
    Args args;
    const int rc = plan_columns(cols, ncols, early, k < 1 ? 1 : k, early == PZ_OK ? n : 0, early == PZ_OK ? B : 0, late, args.col);
    if (rc != PZ_OK) return rc;
    if (n == 0 || B == 0) return PZ_OK;
    uint32_t b = 0;
    while (b < 32 && ((uint64_t)(M - 1) >> b) != 0) ++b;  // bit_length(M - 1)
    if (b < 2) b = 2;
    args.ncols = ncols;
    args.n = (uint32_t)n, args.M = (uint32_t)M, args.B = (uint32_t)B;
    args.minibatches = index_in != nullptr ? 1u : (uint32_t)minibatches;
    args.hb = (b + 1) / 2;
    args.key0 = (uint32_t)seed ^ 0x53485546u, args.key1 = (uint32_t)(seed >> 32) ^ 0x42415443u;
    args.counter = counter, args.counter_dev = index_in != nullptr ? nullptr : counter_dev;
    args.index_in = index_in, args.index_out = index_out, args.errors = errors;
    const dim3 grid((unsigned)((B + kRows - 1) / kRows));
    if (index_in != nullptr)
        hipLaunchKernelGGL(batch_kernel<kIndex>, grid, dim3(kThreads), 0, (hipStream_t)stream, args);
    else
        hipLaunchKernelGGL(batch_kernel<kPerm>, grid, dim3(kThreads), 0, (hipStream_t)stream, args);
    return (int)hipGetLastError();
}

}  // extern "C"
