// Shared host/device helpers for the gfx950 kernels.  Wave = 64 lanes everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/sleekit_amd.h"

namespace slk {

void set_error(const char *fmt, ...);

#define SLK_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            slk::set_error(__VA_ARGS__); \
            return SLK_E_ARG;           \
        }                               \
    } while (0)

#define SLK_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            slk::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SLK_E_HIP;                                                          \
        }                                                                              \
    } while (0)

#define SLK_LAUNCH_CHECK() SLK_HIP(hipGetLastError())

// Optional per-launch timing (slk_profile_*): when enabled every kernel launch is bracketed
// by a pair of HIP events on its own stream, tagged with its name and ALGORITHMIC flops and
// bytes (the roofline numerators of DESIGN.md).  Disabled: one predictable branch.
struct ProfScope {
    int slot;
    hipStream_t stream;
    ProfScope(const char *name, double flops, double bytes, hipStream_t s);
    ~ProfScope();
};

// Workgroups of the NEXT profiled launch, for launches that cannot fill the chip (a latency chain on
// one workgroup is not "dominant" because it is long): the report weighs a launch's time by
// min(1, workgroups / 256).  0 = not stated, taken as chip-wide.
void prof_next_width(long workgroups);

// SLK_RUN("kernel name", flops, bytes, stream, kernel<<<grid, block, smem, stream>>>(args...));
#define SLK_RUN(name, flops, bytes, stream, ...)                 \
    do {                                                         \
        {                                                        \
            slk::ProfScope prof_scope_(name, flops, bytes, stream); \
            __VA_ARGS__;                                         \
        }                                                        \
        SLK_LAUNCH_CHECK();                                      \
    } while (0)

// SLK_RUN for a launch of `wgs` workgroups (see prof_next_width)
#define SLK_RUN_W(name, flops, bytes, wgs, stream, ...) \
    do {                                                \
        slk::prof_next_width((long)(wgs));              \
        SLK_RUN(name, flops, bytes, stream, __VA_ARGS__); \
    } while (0)

// Run-time switches (slk_set_option / slk_get_option; initial values read ONCE from the environment, SLK_<NAME>).
// They select between code paths that give the same results (tests hold them to that) or shape measurements.
enum Opt {
    OPT_NO_FAST_LEAF,          // leaves: true divides instead of the exact-division fma sequence
    OPT_NO_DEFER,              // window kernel: no deferred helper updates
    OPT_NO_WINDOW2,            // general window kernel for every window
    OPT_WIN_DBG,               // window kernels: measurement bits (8: cycle counters of workgroup 0, 16: U blocks from global)
    OPT_NO_REGULAR_SEARCH,     // scale search: staged row sums for every row length
    OPT_NO_FAST_SEARCH_DIV,    // scale search: true divides
    OPT_NO_ERROR_SPLITK,       // layer error: never cut K into chunks
    OPT_ERROR_CB,              // layer error: force this K-chunk count
    OPT_NO_SYM_ERROR,          // layer error: ignore the symmetry of H
    OPT_NO_BF16_ERROR,         // layer error: float32 MFMA kernel
    OPT_NO_BF16_DMA,           // bfloat16 x 3 GEMMs: stage operands through registers
    OPT_NO_BF16_HESSIAN,       // Hessian accumulation: float32 MFMA kernel
    OPT_ERROR_F32_BELOW,       // layer error of a batch: float32 kernel when a layer has fewer rows than this (0: never, the default)
    OPT_NO_BF16_ASYM,          // layer error: an H that is not symmetric goes to the float32 kernel
    OPT_NO_SYM_AVERAGE,        // layer error: an H that is not symmetric is NOT averaged with its transpose (planes of H^T, every k, instead)
    OPT_NO_WAVE_SEARCH,        // local search: the workgroup-per-row kernel for every row length
    OPT_LOOKAHEAD,             // factorisation: the bulk of an outer syrk on a helper stream, beside the next block's panels
    OPT_WINDOW_ROWS,           // window kernel: rows per workgroup forced to 16 or 32 (0: 32, or 16 where the caller asks for latency)
    OPT_PANEL_SPLIT,           // factorisation: 0 / 3: an outer block's panels as a chain of workgroups in one launch; 1 / 2: the panel kernel, two launches / one per panel
    OPT_ROWS_BELOW_WIDE,       // factorisation: the rows below a diagonal block 64 rows per workgroup (1) or 16 (2) whatever the batch (0: 64 from 1024 strips per launch up)
    OPT_NO_LOOP_ERROR,         // layer error: sleekit_amd's callers never take the error the loop carries (slk_gptq_quantize_batch_error); the product instead
    OPT_CHAIN_CARRIES_BELOW,   // factorisation: the rows below a diagonal block in the chain's own launch wherever the cap on waiting workgroups allows (1), never (2), by the rule (0)
    OPT_COUNT
};
int opt(Opt o);

// A helper stream beside the caller's (one per (device, caller stream), created at first use, with a pool of events):
// the factorisation forks the bulk of an outer syrk onto it and joins again before it returns, so the caller still sees
// one stream.  Fork and join are event record / wait pairs, which a hipGraph capture of the caller's stream follows.
struct Helper {
    hipStream_t stream;
    hipStream_t stream2;  // a second one: what the look-ahead runs beside the rest of an outer update (nodes of the inverse)
    hipEvent_t *events;   // room for HELPER_EVENTS; the first `need` of helper_for exist
};
constexpr int HELPER_EVENTS = 512;
// the helper of (current device, main) with at least `need` events (created as they are first asked for; on failure
// nothing made by the call is kept).  slk_release_helpers() destroys them all.
hipError_t helper_for(hipStream_t main, int need, Helper *out);

// Opt a kernel in to `bytes` of dynamic LDS (above the 64 KB default) on the CURRENT device; remembered per
// (kernel, device), safe to call from several threads.  Returns a hipError_t.
hipError_t lds_opt_in(const void *kernel, size_t bytes);
#define SLK_LDS_OPT_IN(kernel, bytes) SLK_HIP(slk::lds_opt_in(reinterpret_cast<const void *>(kernel), (bytes)))

// The float32 inputs of a batch of layers (caller-owned tensors: no common base), passed by value to the kernels
// that read them; blockIdx.z is the layer in every batched launch.
struct PtrTable {
    const float *p[64];
};

// What the column loop READS of every layer of a batch -- W, the row scales (all nullptr: none), the column order (all
// nullptr: the identity, one layer) and the factor U -- as per-layer base pointers, passed by value to the loop's kernels: a
// workgroup picks its layer's with the uniform r0 / rpl it computes anyway (one scalar load).  The layers of
// slk_gptq_quantize_layers are caller-owned tensors anywhere in memory, at most LOOP_LAYERS of them.  A batch stacked by rows
// in ONE allocation (the batch entries, up to 64 layers) is the same table: entry i is layer i's base, and layer b >=
// LOOP_LAYERS lies (b - b % LOOP_LAYERS) layer strides behind entry b % LOOP_LAYERS (layer_base; the strides follow from
// rpl and n).  The loop's workspace and its outputs are one stack either way, indexed by the stacked row.
constexpr int LOOP_LAYERS = 16;
struct LayerTable {
    const float *W[LOOP_LAYERS], *scale[LOOP_LAYERS];
    const long long *order[LOOP_LAYERS];
    const double *U[LOOP_LAYERS];
};
// layer b's base from one column of the table, `stride` elements a layer in a stack
template <class T>
__device__ __forceinline__ const T *layer_base(const T *const (&column)[LOOP_LAYERS], int b, size_t stride) {
    return column[b % LOOP_LAYERS] + (size_t)(b - b % LOOP_LAYERS) * stride;
}

// the layer error of a stack of `batch` layers (rows [b rpl, (b + 1) rpl) against Hs[b]) WITH the products G = (Q - W) H
// the local search starts from (sgemm.hip; the public entries are slk_row_errors / slk_row_errors_batch)
int row_errors_products(const float *W, const float *Q, const float *const *Hs, int batch, int rpl, int n, const int *sym_known,
                        float *row_err, float *G, void *workspace, size_t ws_bytes, slk_stream_t stream);

// mean(diag Hs[b]) in float32, NumPy's order, at out[64 b] for b < batch: the means slk_hessian_prepare damps with, by the
// kernels it forms them with (prepare.hip); what the loop's carried error takes its damping term from
int loop_error_means(const float *const *Hs, int batch, int n, float *out, hipStream_t s);

static inline hipStream_t as_stream(slk_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller's workspace.
struct Arena {
    char *base;
    size_t size, used;
    Arena(void *p, size_t bytes) : base(static_cast<char *>(p)), size(bytes), used(0) {}
    template <class T>
    T *take(size_t count) {
        size_t off = align_up(used, 256);
        size_t end = off + count * sizeof(T);
        if (end > size || base == nullptr) return nullptr;
        used = end;
        return reinterpret_cast<T *>(base + off);
    }
};

// Codebook in float32.  Uniform (table == nullptr): formed exactly like the reference
// (sleekit/codebook.py:35-41 under NEP 50: the Python-float step is cast to float32).  General
// (sleekit/codebook.py:98-190): `table` points to n sorted values followed by the n - 1 bin limits;
// a value's index is np.digitize(x, limits) = the number of limits <= x.
struct Grid {
    float zero, step, top;  // top = levels - 1
    const float *table;
    int n;
};

static inline Grid make_grid(int levels, double lo, double hi, const float *table = nullptr) {
    Grid g;
    g.zero = (float)lo;
    g.step = (float)((hi - lo) / (double)(levels - 1));
    g.top = (float)(levels - 1);
    g.table = table;
    g.n = levels;
    return g;
}

// t = clip(rint((x - zero) / step + shift), first, last): codebook.py:47-49, 71-74, 83-86.
// No contraction: the library is built with -ffp-contract=off.
__device__ __forceinline__ float grid_pos(float x, const Grid g, float shift, float first, float last) {
    float t = (x - g.zero) / g.step;
    t = t + shift;  // exact no-op for shift == 0
    t = rintf(t);
    return fminf(fmaxf(t, first), last);
}
__device__ __forceinline__ float grid_val(float t, const Grid g) { return t * g.step + g.zero; }
__device__ __forceinline__ float grid_value(float x, const Grid g) {
    return grid_val(grid_pos(x, g, 0.0f, 0.0f, g.top), g);
}

// np.digitize(x, limits) for increasing limits: how many of them are <= x (binary search).
__device__ __forceinline__ int table_index(float x, const Grid g) {
    const float *lim = g.table + g.n;
    int lo = 0, hi = g.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lim[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The four maps of either kind of codebook (codebook.py:43-95 and 150-190).
__device__ __forceinline__ float cb_value(float x, const Grid g) { return g.table ? g.table[table_index(x, g)] : grid_value(x, g); }
__device__ __forceinline__ int cb_index(float x, const Grid g) {
    return g.table ? table_index(x, g) : (int)grid_pos(x, g, 0.0f, 0.0f, g.top);
}
__device__ __forceinline__ float cb_up(float x, const Grid g) {
    return g.table ? g.table[min(table_index(x, g) + 1, g.n - 1)] : grid_val(grid_pos(x, g, 1.0f, 1.0f, g.top), g);
}
__device__ __forceinline__ float cb_down(float x, const Grid g) {
    return g.table ? g.table[max(table_index(x, g) - 1, 0)] : grid_val(grid_pos(x, g, -1.0f, 0.0f, g.top - 1.0f), g);
}
// the value of codebook entry k (codebook.py:58-63: k * step + zero in float32, or the table's)
__device__ __forceinline__ float cb_entry(int k, const Grid g) { return g.table ? g.table[k] : grid_val((float)k, g); }

// The group quantizer of one element (sleekit_amd/groups.py): its group's scale s, rs = RN(1 / s) and, OFFSET, offset o.
//   value   codebook(x / s) / rs             OFFSET: codebook((x - o) / s) / rs + o
//   index   cb_index(x / s)                  OFFSET: cb_index((x - o) / s)
// Float32 IEEE divides in this order are what make the indices the reference's bit for bit.  The symmetric form is not
// the asymmetric one with o = 0: -0.0f + 0.0f is +0.0f, and the leaf chain would pay an instruction for it.
template <bool OFFSET>
struct GroupQ {
    float s, rs, o;  // (o: OFFSET only)
    __device__ __forceinline__ static GroupQ of(float s, float o = 0.0f) { return {s, 1.0f / s, o}; }
    // group k of the scales S (and offsets O) in memory
    __device__ __forceinline__ static GroupQ at(const float *S, const float *O, size_t k) {
        GroupQ e = of(S[k]);
        if constexpr (OFFSET) e.o = O[k];
        return e;
    }
    // x in codebook units, and back: the dequantised value of codebook value v
    __device__ __forceinline__ float scaled(float x) const {
        if constexpr (OFFSET) return (x - o) / s;
        else return x / s;
    }
    __device__ __forceinline__ float dequant(float v) const {
        if constexpr (OFFSET) return v / rs + o;
        else return v / rs;
    }
    __device__ __forceinline__ float value(float x, const Grid g) const { return dequant(cb_value(scaled(x), g)); }
    __device__ __forceinline__ int index(float x, const Grid g) const { return cb_index(scaled(x), g); }
    __device__ __forceinline__ float up(float x, const Grid g) const { return dequant(cb_up(scaled(x), g)); }
    __device__ __forceinline__ float down(float x, const Grid g) const { return dequant(cb_down(scaled(x), g)); }
};

// Cross-lane steps on the vector ALU (DPP) instead of the LDS crossbar (__shfl_xor compiles to ds_bpermute_b32: ~150 cycles
// each, six dependent levels per reduction, three reductions per move -- a third of a move's time).  A butterfly level only
// needs SOME lane of the partner group once the earlier levels have made the groups uniform:
//   xor 1, xor 2: quad_perm;  xor 4: row_half_mirror (lane i <-> 7 - i of each 8);  xor 8: row_mirror (i <-> 15 - i of each 16);
//   across the four 16-lane rows: v_readlane of lanes 0, 16, 32, 48.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

// Output element types of the de-quantizers (pack.hip, mx.hip): float32, or that value rounded to nearest even.
enum { PK_F32 = 0, PK_BF16 = 1, PK_F16 = 2 };

__device__ __forceinline__ unsigned short pk_bf16(float f) {  // round to nearest even, quiet NaN (torch's conversion)
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int OUT>
struct PkOut;
template <>
struct PkOut<PK_F32> {
    static constexpr int OUT = PK_F32;
    typedef float T;
    typedef float V __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float cvt(float v) { return v; }
};
template <>
struct PkOut<PK_BF16> {
    static constexpr int OUT = PK_BF16;
    typedef unsigned short T;
    typedef unsigned short V __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ unsigned short cvt(float v) { return pk_bf16(v); }
};
template <>
struct PkOut<PK_F16> {
    static constexpr int OUT = PK_F16;
    typedef _Float16 T;
    typedef _Float16 V __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ _Float16 cvt(float v) { return (_Float16)v; }
};

// The entries' checks of a 16-bit or float32 `dtype` argument and of a pointer the kernels move 16 bytes at a time through
static inline bool known_dtype(int d) { return d == SLK_DTYPE_F32 || d == SLK_DTYPE_BF16 || d == SLK_DTYPE_F16; }
static inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

// f(PkOut<..>()) for a known_dtype: the one place a SLK_DTYPE_* becomes a type.
//   return with_dtype(x_dtype, [&](auto t) -> int { typedef typename decltype(t)::T T; SLK_RUN(..., kernel<T><<<...>>>(...)); return SLK_OK; });
template <class F>
static inline int with_dtype(int dtype, F &&f) {
    if (dtype == SLK_DTYPE_BF16) return f(PkOut<PK_BF16>());
    if (dtype == SLK_DTYPE_F16) return f(PkOut<PK_F16>());
    return f(PkOut<PK_F32>());
}

// f(std::true_type()) or f(std::false_type()): the one place OPT_NO_BF16_DMA becomes a type -- true: the bfloat16 x 3
// GEMMs bring their operands to LDS by global_load_lds (mfma_bf16x3.h), false: staged through registers.
//   return with_bf16_staging([&](auto dma) -> int { SLK_RUN(..., kernel<dma.value><<<...>>>(...)); return SLK_OK; });
template <class F>
static inline int with_bf16_staging(F &&f) {
    if (opt(OPT_NO_BF16_DMA)) return f(std::false_type());
    return f(std::true_type());
}

// Entry `lin` of the lower triangle listed row by row, (0, 0), (1, 0), (1, 1), (2, 0), ... -> (bi, bj <= bi): the float32
// guess of the row, corrected either way.
__device__ __forceinline__ void lower_tile(int lin, int &bi, int &bj) {
    bi = (int)((sqrtf(8.0f * (float)lin + 1.0f) - 1.0f) * 0.5f);
    while (bi * (bi + 1) / 2 > lin) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= lin) ++bi;
    bj = lin - bi * (bi + 1) / 2;
}

// Broadcast lane `src` (wave-uniform index) of a double to the whole wave through SGPRs.
__device__ __forceinline__ double readlane_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffLL), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Zero-fill and copy as plain kernels rather than hipMemsetAsync / hipMemcpyAsync: inside a captured hipGraph the
// runtime's memset node did not take effect on replay (ROCm 7.2: a counting sort's rank buffer kept the previous
// replay's counts and the order it produced indexed out of bounds); kernel nodes replay faithfully.
__global__ __launch_bounds__(256) static void k_zero_words(unsigned *__restrict__ p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}
__global__ __launch_bounds__(256) static void k_copy_words(unsigned *__restrict__ dst, const unsigned *__restrict__ src, size_t words) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// (sizes are multiples of 4 bytes everywhere they are used)
static inline void zero_async(void *p, size_t bytes, hipStream_t s) {
    const size_t words = bytes / 4;
    const int blocks = (int)((words + 1023) / 1024 < 2048 ? (words + 1023) / 1024 : 2048);
    if (words) k_zero_words<<<blocks ? blocks : 1, 256, 0, s>>>(static_cast<unsigned *>(p), words);
}
static inline void copy_async(void *dst, const void *src, size_t bytes, hipStream_t s) {
    const size_t words = bytes / 4;
    const int blocks = (int)((words + 1023) / 1024 < 2048 ? (words + 1023) / 1024 : 2048);
    if (words) k_copy_words<<<blocks ? blocks : 1, 256, 0, s>>>(static_cast<unsigned *>(dst), static_cast<const unsigned *>(src), words);
}

}  // namespace slk
