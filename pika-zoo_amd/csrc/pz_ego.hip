// libpikazoo_ego.so: the egocentric view of observation rows -- eight of a row's 35 columns mirrored about the court's centre
// line, the other 27 copied (pz_ego_rows) -- and the matching involution of the 18 absolute actions (pz_ego_actions), each in
// ONE launch (C ABI and the definitions: include/pikazoo_ego.h; the shape and its reasons: DESIGN.md 4.25).
//
// ROWS.  The launch streams: it moves every byte once in and once out and does one subtraction on 8 elements of 35, so its
// floor is the bytes moved.  Rows that lie back to back (both pitches 35) whose two bases share their offset within 16 bytes
// go as ONE flat array: a thread takes 16 bytes (4 or 8 elements) per trip of a grid-stride loop, the column of its first
// element is `index mod 35` computed ONCE per thread and advanced by a constant with one conditional subtraction per trip; the
// elements in front of the first 16-byte boundary and behind the last one are taken one by one by the grid's first threads.
// Every other layout (a pitch above 35, bases of different phase) goes element by element: (row, column) from one division
// per thread, advanced the same way.  Every element is read and written by the same thread, so in == out needs no care.
// No LDS, no scratch; the grid is capped and strides, so one form serves a step's [n, 35] and a trajectory's [k, n, 35].
// ACTIONS.  One element per thread and trip; pi swaps six pairs of neighbours, which two 18-bit masks say without a table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "pikazoo_ego.h"
#include "pikazoo_hip.h"

namespace pz_ego {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 workgroups; the rest is the stride
constexpr int kDim = PZ_OBS_DIM;
static_assert(kDim == 35, "the column masks below are those of a 35-element row");

constexpr uint64_t bit(int c) { return (uint64_t)1 << c; }
// both players' x, the ball's x, previous x and previous-previous x: M = 432 (normalised: c = 1, but c_26 = 392 / 412)
constexpr uint64_t kCourtCols = bit(0) | bit(13) | bit(26) | bit(28) | bit(30);
// both diving directions, the ball's x velocity: M = 0 (normalised: c = 1)
constexpr uint64_t kSignCols = bit(3) | bit(16) | bit(32);
constexpr uint64_t kMirrorCols = kCourtCols | kSignCols;
constexpr float kBallX = 0x1.e72548p-1f;  // the float32 nearest to (432 - 2 * 20) / (432 - 20)

template <int F> struct Format;
template <> struct Format<PZ_OBS_I32> { using Elem = uint32_t; static constexpr bool kFloat = false, kNorm = false; };
template <> struct Format<PZ_OBS_F32_NORM> { using Elem = uint32_t; static constexpr bool kFloat = true, kNorm = true; };
template <> struct Format<PZ_OBS_I16> { using Elem = uint16_t; static constexpr bool kFloat = false, kNorm = false; };
template <> struct Format<PZ_OBS_F16> { using Elem = uint16_t; static constexpr bool kFloat = true, kNorm = false; };
template <> struct Format<PZ_OBS_BF16> { using Elem = uint16_t; static constexpr bool kFloat = true, kNorm = false; };
template <> struct Format<PZ_OBS_F16_NORM> { using Elem = uint16_t; static constexpr bool kFloat = true, kNorm = true; };
template <> struct Format<PZ_OBS_BF16_NORM> { using Elem = uint16_t; static constexpr bool kFloat = true, kNorm = true; };

// the stored element widened to float32 (exact in all three float formats)
template <int F> __device__ __forceinline__ float widen(uint32_t bits)
{
    if constexpr (F == PZ_OBS_F32_NORM) {
        return __uint_as_float(bits);
    } else if constexpr (F == PZ_OBS_F16 || F == PZ_OBS_F16_NORM) {
        const uint16_t h = (uint16_t)bits;
        _Float16 v;
        memcpy(&v, &h, 2);
        return (float)v;
    } else {
        return __uint_as_float(bits << 16);
    }
}

// float32 rounded to nearest even into the row's format
template <int F> __device__ __forceinline__ uint32_t narrow(float r)
{
    if constexpr (F == PZ_OBS_F32_NORM) {
        return __float_as_uint(r);
    } else if constexpr (F == PZ_OBS_F16 || F == PZ_OBS_F16_NORM) {
        const _Float16 v = (_Float16)r;
        uint16_t h;
        memcpy(&h, &v, 2);
        return h;
    } else {
        const uint32_t u = __float_as_uint(r);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;  // a NaN stays one
        return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    }
}

// one element of column `col` (0..34), as its bits in the low end of a word
template <int F> __device__ __forceinline__ uint32_t mirror(uint32_t bits, int col)
{
    if (!((kMirrorCols >> col) & 1)) return bits;
    const bool court = (kCourtCols >> col) & 1;
    if constexpr (!Format<F>::kFloat) {
        const int32_t v = F == PZ_OBS_I32 ? (int32_t)bits : (int32_t)(int16_t)(uint16_t)bits;
        const uint32_t r = (uint32_t)((court ? PZ_EGO_COURT_WIDTH : 0) - v);
        return F == PZ_OBS_I32 ? r : (r & 0xFFFFu);
    } else {
        const float m = Format<F>::kNorm ? (col == 26 ? kBallX : 1.0f) : (court ? (float)PZ_EGO_COURT_WIDTH : 0.0f);
        return narrow<F>(m - widen<F>(bits));
    }
}

__device__ __forceinline__ int wrap(int col) { return col >= kDim ? col - kDim : col; }

// rows back to back, `in` and `out` of one phase within 16 bytes: `head` elements in front of the first 16-byte boundary,
// then `vectors` pieces of 16 bytes, then the rest up to `total`
template <int F>
__global__ __launch_bounds__(kThreads) void rows_flat_kernel(const typename Format<F>::Elem* in, typename Format<F>::Elem* out, int64_t head,
                                                             int64_t vectors, int64_t total)
{
    using Elem = typename Format<F>::Elem;
    constexpr int V = 16 / (int)sizeof(Elem);
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t body_end = head + vectors * V;
    // the edges: at most V - 1 elements on either side, one thread each
    if (gid < head + (total - body_end)) {
        const int64_t e = gid < head ? gid : body_end + (gid - head);
        out[e] = (Elem)mirror<F>(in[e], (int)(e % kDim));
    }
    if (gid >= vectors) return;
    const uint4* vin = (const uint4*)(in + head);
    uint4* vout = (uint4*)(out + head);
    int col = (int)((head + gid * V) % kDim);            // the one division of this thread
    const int step = (int)((stride * V) % kDim);         // (uniform)
    for (int64_t v = gid; v < vectors; v += stride) {
        const uint4 w = vin[v];
        uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (sizeof(Elem) == 4) {
                x[i] = mirror<F>(x[i], wrap(col + i));
            } else {
                const uint32_t lo = mirror<F>(x[i] & 0xFFFFu, wrap(col + 2 * i));
                const uint32_t hi = mirror<F>(x[i] >> 16, wrap(col + 2 * i + 1));
                x[i] = lo | (hi << 16);
            }
        }
        vout[v] = make_uint4(x[0], x[1], x[2], x[3]);
        col = wrap(col + step);
    }
}

// any pitches, any element-aligned bases: element by element
template <int F>
__global__ __launch_bounds__(kThreads) void rows_pitched_kernel(const typename Format<F>::Elem* in, typename Format<F>::Elem* out, int64_t rows,
                                                                int64_t in_pitch, int64_t out_pitch)
{
    using Elem = typename Format<F>::Elem;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    int64_t row = gid / kDim;                            // the one division of this thread
    int col = (int)(gid - row * kDim);
    const int64_t row_step = stride / kDim;              // (uniform)
    const int col_step = (int)(stride - row_step * kDim);
    while (row < rows) {
        out[row * out_pitch + col] = (Elem)mirror<F>(in[row * in_pitch + col], col);
        row += row_step;
        col += col_step;
        if (col >= kDim) {
            col -= kDim;
            ++row;
        }
    }
}

// pi swaps (3 4) (6 7) (8 9) (11 12) (14 15) (16 17): the lower of a pair goes up by one, the upper down
constexpr uint32_t kPairLow = (1u << 3) | (1u << 6) | (1u << 8) | (1u << 11) | (1u << 14) | (1u << 16);
constexpr uint32_t kPairHigh = kPairLow << 1;

template <typename T> __global__ __launch_bounds__(kThreads) void actions_kernel(const T* in, T* out, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        T a = in[i];
        if ((uint64_t)(int64_t)a < 18u) {  // (on the full value: an int64 of 2^32 + 3 is no action)
            const uint32_t v = (uint32_t)a;
            a = (T)(v + ((kPairLow >> v) & 1u) - ((kPairHigh >> v) & 1u));
        }
        out[i] = a;
    }
}

static unsigned blocks_for(int64_t threads)
{
    const int64_t blocks = (threads + kThreads - 1) / kThreads;
    return (unsigned)(blocks < 1 ? 1 : blocks > kMaxBlocks ? kMaxBlocks : blocks);
}

static bool overlap(uintptr_t a, int64_t a_bytes, uintptr_t b, int64_t b_bytes) { return a < b + (uintptr_t)b_bytes && b < a + (uintptr_t)a_bytes; }

template <int F> static int launch_rows(const void* in, void* out, int64_t rows, int64_t in_pitch, int64_t out_pitch, hipStream_t stream)
{
    using Elem = typename Format<F>::Elem;
    constexpr int V = 16 / (int)sizeof(Elem);
    const int64_t total = rows * kDim;
    if (in_pitch == kDim && out_pitch == kDim && (((uintptr_t)in ^ (uintptr_t)out) & 15) == 0) {
        int64_t head = (int64_t)((16 - ((uintptr_t)in & 15)) & 15) / (int64_t)sizeof(Elem);
        if (head > total) head = total;
        const int64_t vectors = (total - head) / V;
        const int64_t threads = vectors > 2 * V ? vectors : 2 * V;  // (the edges need at most 2 (V - 1) threads)
        hipLaunchKernelGGL(rows_flat_kernel<F>, dim3(blocks_for(threads)), dim3(kThreads), 0, stream, (const Elem*)in, (Elem*)out, head, vectors, total);
    } else {
        hipLaunchKernelGGL(rows_pitched_kernel<F>, dim3(blocks_for(total)), dim3(kThreads), 0, stream, (const Elem*)in, (Elem*)out, rows, in_pitch,
                           out_pitch);
    }
    return (int)hipGetLastError();
}

template <typename T> static int launch_actions(const void* in, void* out, int64_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(actions_kernel<T>, dim3(blocks_for(n)), dim3(kThreads), 0, stream, (const T*)in, (T*)out, n);
    return (int)hipGetLastError();
}

}  // namespace pz_ego

using namespace pz_ego;

extern "C" {

#ifndef PZ_BUILD_ID
#define PZ_BUILD_ID "unknown"
#endif
// (the same record the product library carries: build.py reads it from the file's bytes)
static const char kEgoBuildIdRecord[] = "pz_build_id:" PZ_BUILD_ID;
const char* pz_ego_build_id(void) { return kEgoBuildIdRecord + 12; }

int pz_ego_abi_version(void) { return PZ_EGO_ABI_VERSION; }

const char* pz_ego_error_string(int code)
{
    switch (code) {
    case PZ_OK: return nullptr;
    case PZ_E_NULL: return "a required pointer is NULL";
    case PZ_E_SIZE: return "a count below 0, a pitch below 35 or an extent beyond int64 bytes";
    case PZ_E_CONFIG: return "an unknown row or action format";
    case PZ_E_ALIGN: return "a pointer not aligned to its element";
    case PZ_E_EGO_OVERLAP: return "the input and output ranges overlap without being the same rows";
    default: return code > 0 ? "HIP error" : "unknown error";
    }
}

int pz_ego_rows(const void* in, void* out, int32_t format, int64_t rows, int64_t in_pitch, int64_t out_pitch, void* stream)
{
    if (rows > 0 && (in == nullptr || out == nullptr)) return PZ_E_NULL;
    if (rows < 0 || in_pitch < kDim || out_pitch < kDim) return PZ_E_SIZE;
    int64_t in_bytes, out_bytes;  // (an element has at most 4 bytes)
    if (__builtin_mul_overflow(rows, in_pitch, &in_bytes) || __builtin_mul_overflow(in_bytes, (int64_t)4, &in_bytes) ||
        __builtin_mul_overflow(rows, out_pitch, &out_bytes) || __builtin_mul_overflow(out_bytes, (int64_t)4, &out_bytes))
        return PZ_E_SIZE;
    if (format < PZ_OBS_I32 || format > PZ_OBS_BF16_NORM) return PZ_E_CONFIG;
    const int64_t eb = (format == PZ_OBS_I32 || format == PZ_OBS_F32_NORM) ? 4 : 2;
    if (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(eb - 1)) return PZ_E_ALIGN;
    if (rows == 0) return PZ_OK;
    in_bytes = ((rows - 1) * in_pitch + kDim) * eb;
    out_bytes = ((rows - 1) * out_pitch + kDim) * eb;
    if (!(in == out && in_pitch == out_pitch) && overlap((uintptr_t)in, in_bytes, (uintptr_t)out, out_bytes)) return PZ_E_EGO_OVERLAP;
    const hipStream_t s = (hipStream_t)stream;
    switch (format) {
    case PZ_OBS_I32: return launch_rows<PZ_OBS_I32>(in, out, rows, in_pitch, out_pitch, s);
    case PZ_OBS_F32_NORM: return launch_rows<PZ_OBS_F32_NORM>(in, out, rows, in_pitch, out_pitch, s);
    case PZ_OBS_I16: return launch_rows<PZ_OBS_I16>(in, out, rows, in_pitch, out_pitch, s);
    case PZ_OBS_F16: return launch_rows<PZ_OBS_F16>(in, out, rows, in_pitch, out_pitch, s);
    case PZ_OBS_BF16: return launch_rows<PZ_OBS_BF16>(in, out, rows, in_pitch, out_pitch, s);
    case PZ_OBS_F16_NORM: return launch_rows<PZ_OBS_F16_NORM>(in, out, rows, in_pitch, out_pitch, s);
    default: return launch_rows<PZ_OBS_BF16_NORM>(in, out, rows, in_pitch, out_pitch, s);
    }
}

int pz_ego_actions(const void* in, void* out, int32_t action_format, int64_t n, void* stream)
{
    if (n > 0 && (in == nullptr || out == nullptr)) return PZ_E_NULL;
    if (n < 0 || n > INT64_MAX / 8) return PZ_E_SIZE;
    if (action_format < PZ_ACT_I32 || action_format > PZ_ACT_I16) return PZ_E_CONFIG;
    const int64_t eb = action_format == PZ_ACT_I32 ? 4 : action_format == PZ_ACT_I64 ? 8 : action_format == PZ_ACT_U8 ? 1 : 2;
    if (((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(eb - 1)) return PZ_E_ALIGN;
    if (n == 0) return PZ_OK;
    if (in != out && overlap((uintptr_t)in, n * eb, (uintptr_t)out, n * eb)) return PZ_E_EGO_OVERLAP;
    const hipStream_t s = (hipStream_t)stream;
    switch (action_format) {
    case PZ_ACT_I32: return launch_actions<int32_t>(in, out, n, s);
    case PZ_ACT_I64: return launch_actions<int64_t>(in, out, n, s);
    case PZ_ACT_U8: return launch_actions<uint8_t>(in, out, n, s);
    default: return launch_actions<int16_t>(in, out, n, s);
    }
}

}  // extern "C"
