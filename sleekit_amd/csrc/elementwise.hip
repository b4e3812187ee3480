// Element-wise stages of the path: codebook maps, row scaling, Hessian fix-ups,
// column statistics.  All HBM-bound streaming kernels: 16-byte loads where the
// layout allows, grid-stride over at most 2048 blocks (guide: Guideline 11/13).
#include <stdarg.h>

#include "npsum.h"

namespace slk {

static thread_local char g_error[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

static inline int stream_blocks(size_t work_items, int per_block) {
    size_t b = (work_items + per_block - 1) / per_block;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

// ---------------------------------------------------------------- codebook maps
template <int WHAT>
__global__ __launch_bounds__(256) void k_codebook(const float *__restrict__ x, size_t count, Grid g,
                                                  void *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const float v = x[i];
        if (WHAT == SLK_CB_VALUE) {
            static_cast<float *>(out)[i] = cb_value(v, g);
        } else if (WHAT == SLK_CB_INDEX) {
            static_cast<uint8_t *>(out)[i] = (uint8_t)cb_index(v, g);
        } else if (WHAT == SLK_CB_INDEX16) {
            static_cast<uint16_t *>(out)[i] = (uint16_t)cb_index(v, g);
        } else if (WHAT == SLK_CB_INDEX32) {
            static_cast<uint32_t *>(out)[i] = (uint32_t)cb_index(v, g);
        } else if (WHAT == SLK_CB_UP) {
            static_cast<float *>(out)[i] = cb_up(v, g);
        } else {
            static_cast<float *>(out)[i] = cb_down(v, g);
        }
    }
}

// ---------------------------------------------------------------- row scaling
__global__ __launch_bounds__(256) void k_rows_divide(const float *__restrict__ x,
                                                     const float *__restrict__ scale, int R, int n,
                                                     int invert, float *__restrict__ out) {
    // one block walks rows; threads walk columns (coalesced)
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        float s = scale[r];
        if (invert) s = 1.0f / s;
        const float *xr = x + (size_t)r * n;
        float *orow = out + (size_t)r * n;
        for (int j = threadIdx.x; j < n; j += blockDim.x) orow[j] = xr[j] / s;
    }
}

// ---------------------------------------------------------------- stacking row shards
// dst[b][r][:] = src_b[r][:] for r < rows, `fill` for the padding rows up to rows_padded; blockIdx.z = layer
__global__ __launch_bounds__(256) void k_stack_rows(PtrTable srcs, int rows, int rows_padded, int cols, float fill,
                                                    float *__restrict__ dst) {
    const float *__restrict__ src = srcs.p[blockIdx.z];
    float *__restrict__ out = dst + (size_t)blockIdx.z * rows_padded * cols;
    const size_t live = (size_t)rows * cols, all = (size_t)rows_padded * cols;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < all; i += (size_t)gridDim.x * 256) out[i] = i < live ? src[i] : fill;
}

// ---------------------------------------------------------------- H - m m^T
__global__ __launch_bounds__(256) void k_strip_mean(const float *__restrict__ H,
                                                    const float *__restrict__ mean, int n,
                                                    float *__restrict__ out) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const float mi = mean[i];
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const float p = mi * mean[j];  // np.outer in float32, then one subtraction
            out[(size_t)i * n + j] = H[(size_t)i * n + j] - p;
        }
    }
}

// ---------------------------------------------------------------- dead columns
__global__ __launch_bounds__(256) void k_patch_dead(float *__restrict__ H, float *__restrict__ W,
                                                    int R, int n, const float *__restrict__ fill,
                                                    uint8_t *__restrict__ dead) {
    // pass 1 (block 0 .. ): flag dead columns and patch the diagonal
    const float f = fill[0];
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const bool d = H[(size_t)j * n + j] == 0.0f;
        dead[j] = d;
        if (d) H[(size_t)j * n + j] = f;
    }
}

__global__ __launch_bounds__(256) void k_zero_dead(float *__restrict__ W, int R, int n,
                                                   const uint8_t *__restrict__ dead) {
    for (int r = blockIdx.x; r < R; r += gridDim.x)
        for (int j = threadIdx.x; j < n; j += blockDim.x)
            if (dead[j]) W[(size_t)r * n + j] = 0.0f;
}

// ---------------------------------------------------------------- column miss
// miss[j] = sum_r f(q(W[r][j]) - W[r][j]), accumulated in row order in float32
// (NumPy's axis-0 reduction adds row after row, and the sort that follows sees every bit of it).
// One workgroup per 32 columns.  The order of the ADDS is fixed, everything else is not: all 256 threads evaluate
// the terms of a 256-row chunk (coalesced 128-byte row segments, the next chunk's loads already in flight) into
// LDS, then one thread per column adds its 256 terms top to bottom.  (One thread per column doing everything
// took 1.4 ms for a 4096 x 4096 layer: 4096 dependent trips to memory.)
typedef float float4v_t __attribute__((ext_vector_type(4)));
constexpr int CM_COLS = 32, CM_ROWS = 256;
// GROUPED: q = codebook(w / s) / rs with the element's group scale s = S[r][j / gsize], rs = RN(1 / s) (slk_column_miss_grouped)
// OFFSET (with GROUPED): q = codebook((w - o) / s) / rs + o, o = O[r][j / gsize] (slk_column_miss_grouped_asym)
template <bool GROUPED, bool OFFSET = false>
__global__ __launch_bounds__(256) void k_column_miss(const float *__restrict__ W, int R, int n, Grid g,
                                                     int squared, float *__restrict__ miss, int vec_ok,
                                                     const float *__restrict__ S, int gsize, const float *__restrict__ O) {
    __shared__ float term[CM_ROWS][CM_COLS + 1];
    const int t = threadIdx.x;
    const int j0 = blockIdx.x * CM_COLS;
    const int lr = t >> 3, c4 = (t & 7) * 4;  // this thread's row inside a pass of 32 rows, its four columns
    float4v_t cur[8], nxt[8];
    auto fetch = [&](int base, float4v_t(&v)[8]) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int r = min(base + p * 32 + lr, R - 1);  // clamped: rows beyond R are never added
            const float *src = W + (size_t)r * n + j0 + c4;
            if (vec_ok && j0 + c4 + 3 < n) {
                v[p] = *reinterpret_cast<const float4v_t *>(src);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[p][e] = (j0 + c4 + e < n) ? src[e] : 0.0f;
            }
        }
    };
    float acc = 0.0f;
    if (R > 0) fetch(0, cur);
    for (int base = 0; base < R; base += CM_ROWS) {
        if (base + CM_ROWS < R) fetch(base + CM_ROWS, nxt);
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = cur[p][e];
                float qv;
                if constexpr (GROUPED) {
                    // (clamped like the loads: a row beyond R or a column beyond n is never added)
                    const size_t k = (size_t)min(base + p * 32 + lr, R - 1) * (n / gsize) + min(j0 + c4 + e, n - 1) / gsize;
                    qv = GroupQ<OFFSET>::at(S, O, k).value(w, g);
                } else {
                    qv = cb_value(w, g);
                }
                const float d = qv - w;
                term[p * 32 + lr][c4 + e] = squared ? d * d : fabsf(d);
            }
        __syncthreads();
        if (t < CM_COLS) {
            const int rows = min(CM_ROWS, R - base);
            for (int r = 0; r < rows; ++r) acc = acc + term[r][t];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 8; ++p) cur[p] = nxt[p];
    }
    if (t < CM_COLS && j0 + t < n) miss[j0 + t] = acc;
}
// n == 1: the one column is a contiguous vector, and NumPy reduces an (R, 1) array along axis 0 as that vector -- its
// pairwise sum of R elements (npsum.h), not the row-after-row order of wider matrices.  One workgroup.  (Nothing sorts by the
// key of a lone column; the value is held to the reference all the same.)
template <bool GROUPED, bool OFFSET = false>
__global__ __launch_bounds__(256) void k_column_miss_single(const float *__restrict__ W, int R, Grid g, int squared,
                                                            float *__restrict__ miss, const float *__restrict__ S,
                                                            const float *__restrict__ O) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    SumTree *trees = reinterpret_cast<SumTree *>(smem_raw);
    float *terms = reinterpret_cast<float *>(smem_raw + 2 * sizeof(SumTree));
    prepare_trees(trees, R);
    const float total = row_sum_numpy(trees, terms, R, [&](int r) {
        const float w = W[r];
        float qv;
        if constexpr (GROUPED) {
            qv = GroupQ<OFFSET>::at(S, O, (size_t)r).value(w, g);
        } else {
            qv = cb_value(w, g);
        }
        const float d = qv - w;
        return squared ? d * d : fabsf(d);
    });
    if (threadIdx.x == 0) miss[0] = total;
}
static size_t single_smem(int R) { return 2 * sizeof(SumTree) + sizeof(float) * (size_t)(R < NP_CHUNK ? R : NP_CHUNK); }

// Q[r][c] = value(idx[r][c]) / RN(1 / S[r][c / gsize]): the grouped loop's result rebuilt from its compact form.  The value
// of index t is formed like the quantizer's (t * step + zero in float32, codebook.py:58-63) or read from the table.
// OFFSET: Q[r][c] = value / RN(1 / s) + o, o = O[r][c / gsize] (slk_dequantize_grouped_asym).
template <bool OFFSET = false>
__global__ __launch_bounds__(256) void k_dequantize_grouped(const uint8_t *__restrict__ idx, const float *__restrict__ S, int gsize,
                                                            int R, int n, Grid g, float *__restrict__ Q, const float *__restrict__ O) {
    const size_t total = (size_t)R * n;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / n, c = e % n;
        const float v = cb_entry(min((int)idx[e], g.n - 1), g);
        Q[e] = GroupQ<OFFSET>::at(S, O, r * (n / gsize) + c / gsize).dequant(v);
    }
}

// ---------------------------------------------------------------- group offsets
// MIDPOINTS: O[r][k] = 0.5f * (min + max) of group k of row r (float32, as NumPy forms it), then, Wc given, the centred
// weights Wc = W - O by element (what the scale search of an asymmetric layer reads).  !MIDPOINTS: O is given, Wc only.
// One workgroup per row: the row is read from memory once for O and again, from the cache, for Wc.  Groups of at least
// 64 columns take a wave each (lanes stride the group, then a butterfly), smaller ones a thread each.
template <bool MIDPOINTS>
__global__ __launch_bounds__(256) void k_group_offsets(const float *__restrict__ W, int R, int n, int gsize, float *__restrict__ O,
                                                       float *__restrict__ Wc) {
    const int G = n / gsize, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const float *w = W + (size_t)r * n;
        if constexpr (MIDPOINTS) {
            if (gsize >= 64) {
                for (int k = wave; k < G; k += 4) {
                    float mn = w[(size_t)k * gsize], mx = mn;
                    for (int c = lane; c < gsize; c += 64) {
                        const float v = w[(size_t)k * gsize + c];
                        mn = fminf(mn, v);
                        mx = fmaxf(mx, v);
                    }
                    for (int off = 32; off > 0; off >>= 1) {
                        mn = fminf(mn, __shfl_xor(mn, off));
                        mx = fmaxf(mx, __shfl_xor(mx, off));
                    }
                    if (lane == 0) O[(size_t)r * G + k] = 0.5f * (mn + mx);
                }
            } else {
                for (int k = t; k < G; k += 256) {
                    float mn = w[(size_t)k * gsize], mx = mn;
                    for (int c = 1; c < gsize; ++c) {
                        const float v = w[(size_t)k * gsize + c];
                        mn = fminf(mn, v);
                        mx = fmaxf(mx, v);
                    }
                    O[(size_t)r * G + k] = 0.5f * (mn + mx);
                }
            }
            __syncthreads();  // (global writes of this workgroup, read back below)
        }
        if (Wc)
            for (int c = t; c < n; c += 256) Wc[(size_t)r * n + c] = w[c] - O[(size_t)r * G + c / gsize];
        if constexpr (MIDPOINTS) __syncthreads();
    }
}

// slk_column_miss_grouped[_asym] and slk_dequantize_grouped[_asym]: goffset == nullptr is the symmetric quantizer
static int column_miss_grouped(const float *W, const float *gscale, const float *goffset, int group_size, int R, int n, int levels,
                               double lo, double hi, const float *table, int squared, float *miss, slk_stream_t stream) {
    SLK_REQUIRE(levels >= 2 && (table || lo < hi), "codebook needs levels >= 2 and lo < hi");
    SLK_REQUIRE(R > 0 && n > 0 && W && gscale && miss, "bad arguments");
    SLK_REQUIRE(group_size >= 1 && n % group_size == 0, "group_size must be >= 1 and divide n");
    hipStream_t s = as_stream(stream);
    const Grid g = make_grid(levels, lo, hi, table);
    const int blocks = (n + CM_COLS - 1) / CM_COLS, vec_ok = n % 4 == 0 && (uintptr_t)W % 16 == 0;
    if (n == 1) {
        if (goffset)
            SLK_RUN("column_miss_grouped_asym", 0, 4.0 * R, s,
                    k_column_miss_single<true, true><<<1, 256, single_smem(R), s>>>(W, R, g, squared, miss, gscale, goffset));
        else
            SLK_RUN("column_miss_grouped", 0, 4.0 * R, s,
                    k_column_miss_single<true><<<1, 256, single_smem(R), s>>>(W, R, g, squared, miss, gscale, nullptr));
        return SLK_OK;
    }
    if (goffset)
        SLK_RUN("column_miss_grouped_asym", 0, 4.0 * R * n, s,
                k_column_miss<true, true><<<blocks, 256, 0, s>>>(W, R, n, g, squared, miss, vec_ok, gscale, group_size, goffset));
    else
        SLK_RUN("column_miss_grouped", 0, 4.0 * R * n, s,
                k_column_miss<true><<<blocks, 256, 0, s>>>(W, R, n, g, squared, miss, vec_ok, gscale, group_size, nullptr));
    return SLK_OK;
}

static int dequantize_grouped(const uint8_t *idx, const float *gscale, const float *goffset, int group_size, int R, int n, int levels,
                              double lo, double hi, const float *table, float *Q, slk_stream_t stream) {
    SLK_REQUIRE(levels >= 2 && levels <= 256 && (table || lo < hi), "codebook needs 2 <= levels <= 256 and lo < hi");
    SLK_REQUIRE(R > 0 && n > 0 && idx && gscale && Q, "bad arguments");
    SLK_REQUIRE(group_size >= 1 && n % group_size == 0, "group_size must be >= 1 and divide n");
    hipStream_t s = as_stream(stream);
    const Grid g = make_grid(levels, lo, hi, table);
    const int blocks = stream_blocks((size_t)R * n, 256 * 4);
    if (goffset)
        SLK_RUN("dequantize_grouped_asym", 0, 13.0 * R * n, s,
                k_dequantize_grouped<true><<<blocks, 256, 0, s>>>(idx, gscale, group_size, R, n, g, Q, goffset));
    else
        SLK_RUN("dequantize_grouped", 0, 9.0 * R * n, s,
                k_dequantize_grouped<<<blocks, 256, 0, s>>>(idx, gscale, group_size, R, n, g, Q, nullptr));
    return SLK_OK;
}

}  // namespace slk

using namespace slk;

extern "C" {

int slk_abi_version(void) { return 8; }

const char *slk_last_error(void) { return g_error; }

int slk_codebook_apply(const float *x, size_t count, int levels, double lo, double hi, const float *table, int what,
                       void *out, slk_stream_t stream) {
    SLK_REQUIRE(levels >= 2 && (table || lo < hi), "codebook needs levels >= 2 and lo < hi");
    SLK_REQUIRE(what >= 0 && what <= 5, "unknown codebook map %d", what);
    SLK_REQUIRE(what != SLK_CB_INDEX || levels <= 256, "uint8 indices need levels <= 256");
    SLK_REQUIRE(what != SLK_CB_INDEX16 || levels <= 65536, "uint16 indices need levels <= 65536");
    SLK_REQUIRE(table == nullptr || levels <= 256, "general codebooks hold at most 256 entries");
    if (count == 0) return SLK_OK;
    SLK_REQUIRE(x && out, "null pointer");
    const Grid g = make_grid(levels, lo, hi, table);
    const int blocks = stream_blocks(count, 256 * 4);
    hipStream_t s = as_stream(stream);
    const double bytes = (double)count * (what == SLK_CB_INDEX ? 5.0 : 8.0);
    switch (what) {
        case SLK_CB_VALUE: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_VALUE><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
        case SLK_CB_INDEX: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_INDEX><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
        case SLK_CB_UP: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_UP><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
        case SLK_CB_INDEX16: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_INDEX16><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
        case SLK_CB_INDEX32: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_INDEX32><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
        default: SLK_RUN("codebook_apply", 0, bytes, s, k_codebook<SLK_CB_DOWN><<<blocks, 256, 0, s>>>(x, count, g, out)); break;
    }
    return SLK_OK;
}

int slk_rows_divide(const float *x, const float *scale, int R, int n, int invert, float *out,
                    slk_stream_t stream) {
    SLK_REQUIRE(R >= 0 && n >= 0, "negative shape");
    if (R == 0 || n == 0) return SLK_OK;
    SLK_REQUIRE(x && scale && out, "null pointer");
    hipStream_t s = as_stream(stream);
    SLK_RUN("rows_divide", 0, 8.0 * R * n, s, k_rows_divide<<<stream_blocks(R, 1), 256, 0, s>>>(x, scale, R, n, invert, out));
    return SLK_OK;
}

int slk_stack_rows(const float *const *src, int batch, int rows, int rows_padded, int cols, float fill, float *dst,
                   slk_stream_t stream) {
    SLK_REQUIRE(batch >= 0 && rows >= 0 && rows_padded >= rows && cols >= 0, "bad shape");
    if (batch == 0 || rows_padded == 0 || cols == 0) return SLK_OK;
    SLK_REQUIRE(src && dst, "null pointer");
    hipStream_t s = as_stream(stream);
    const size_t per = (size_t)rows_padded * cols;
    for (int b0 = 0; b0 < batch; b0 += 64) {  // (a table of 64 pointers travels by value with each launch)
        const int nb = batch - b0 < 64 ? batch - b0 : 64;
        PtrTable t;
        for (int b = 0; b < 64; ++b) t.p[b] = b < nb ? src[b0 + b] : nullptr;
        for (int b = 0; b < nb; ++b) SLK_REQUIRE(t.p[b] || rows == 0, "null source in the batch");
        const int bx = (int)std::min<size_t>((per + 1023) / 1024, 1024);
        SLK_RUN("stack_rows", 0, 8.0 * per * nb, s, k_stack_rows<<<dim3(bx, 1, nb), 256, 0, s>>>(t, rows, rows_padded, cols, fill, dst + (size_t)b0 * per));
    }
    return SLK_OK;
}

int slk_hessian_strip_mean(const float *H, const float *mean, int n, float *out, slk_stream_t stream) {
    SLK_REQUIRE(n >= 0, "negative shape");
    if (n == 0) return SLK_OK;
    SLK_REQUIRE(H && mean && out, "null pointer");
    hipStream_t s = as_stream(stream);
    SLK_RUN("hessian_strip_mean", 0, 8.0 * n * n, s, k_strip_mean<<<stream_blocks(n, 1), 256, 0, s>>>(H, mean, n, out));
    return SLK_OK;
}

int slk_hessian_patch_dead(float *H, float *W, int R, int n, void *workspace, size_t ws_bytes,
                           slk_stream_t stream) {
    SLK_REQUIRE(n > 0 && R >= 0 && H, "bad arguments");
    Arena ws(workspace, ws_bytes);
    float *fill = ws.take<float>(64);
    uint8_t *dead = ws.take<uint8_t>((size_t)n);
    if (!fill || !dead) {
        set_error("workspace too small");
        return SLK_E_WS;
    }
    size_t used = ws.used;
    int rc = slk_diag_mean(H, n, fill, static_cast<char *>(workspace) + align_up(used, 256),
                           ws_bytes - align_up(used, 256), stream);
    if (rc != SLK_OK) return rc;
    hipStream_t s = as_stream(stream);
    SLK_RUN("patch_dead", 0, 8.0 * n, s, k_patch_dead<<<stream_blocks(n, 256), 256, 0, s>>>(H, W, R, n, fill, dead));
    if (W && R > 0) SLK_RUN("zero_dead", 0, 1.0 * n, s, k_zero_dead<<<stream_blocks(R, 1), 256, 0, s>>>(W, R, n, dead));
    return SLK_OK;
}

int slk_column_miss(const float *W, int R, int n, int levels, double lo, double hi, const float *table, int squared,
                    float *miss, slk_stream_t stream) {
    SLK_REQUIRE(levels >= 2 && (table || lo < hi), "codebook needs levels >= 2 and lo < hi");
    SLK_REQUIRE(R >= 0 && n > 0 && W && miss, "bad arguments");
    hipStream_t s = as_stream(stream);
    if (n == 1 && R > 0) {
        SLK_RUN("column_miss", 0, 4.0 * R, s,
                k_column_miss_single<false><<<1, 256, single_smem(R), s>>>(W, R, make_grid(levels, lo, hi, table), squared, miss,
                                                                             nullptr, nullptr));
        return SLK_OK;
    }
    SLK_RUN("column_miss", 0, 4.0 * R * n, s,
            k_column_miss<false><<<(n + CM_COLS - 1) / CM_COLS, 256, 0, s>>>(W, R, n, make_grid(levels, lo, hi, table), squared, miss,
                                                                             n % 4 == 0 && (uintptr_t)W % 16 == 0, nullptr, 1, nullptr));
    return SLK_OK;
}

int slk_column_miss_grouped(const float *W, const float *gscale, int group_size, int R, int n, int levels, double lo, double hi,
                            const float *table, int squared, float *miss, slk_stream_t stream) {
    return column_miss_grouped(W, gscale, nullptr, group_size, R, n, levels, lo, hi, table, squared, miss, stream);
}

int slk_dequantize_grouped(const uint8_t *idx, const float *gscale, int group_size, int R, int n, int levels, double lo, double hi,
                           const float *table, float *Q, slk_stream_t stream) {
    return dequantize_grouped(idx, gscale, nullptr, group_size, R, n, levels, lo, hi, table, Q, stream);
}

int slk_column_miss_grouped_asym(const float *W, const float *gscale, const float *goffset, int group_size, int R, int n, int levels,
                                 double lo, double hi, const float *table, int squared, float *miss, slk_stream_t stream) {
    SLK_REQUIRE(goffset, "bad arguments");
    return column_miss_grouped(W, gscale, goffset, group_size, R, n, levels, lo, hi, table, squared, miss, stream);
}

int slk_dequantize_grouped_asym(const uint8_t *idx, const float *gscale, const float *goffset, int group_size, int R, int n, int levels,
                                double lo, double hi, const float *table, float *Q, slk_stream_t stream) {
    SLK_REQUIRE(goffset, "bad arguments");
    return dequantize_grouped(idx, gscale, goffset, group_size, R, n, levels, lo, hi, table, Q, stream);
}

int slk_group_midpoints(const float *W, int group_size, int R, int n, float *goffset, float *Wc, slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && W && goffset, "bad arguments");
    SLK_REQUIRE(group_size >= 1 && n % group_size == 0, "group_size must be >= 1 and divide n");
    hipStream_t s = as_stream(stream);
    SLK_RUN("group_midpoints", 0, (Wc ? 8.0 : 4.0) * R * n, s,
            k_group_offsets<true><<<R < 4096 ? R : 4096, 256, 0, s>>>(W, R, n, group_size, goffset, Wc));
    return SLK_OK;
}

int slk_group_center(const float *W, const float *goffset, int group_size, int R, int n, float *Wc, slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && W && goffset && Wc, "bad arguments");
    SLK_REQUIRE(group_size >= 1 && n % group_size == 0, "group_size must be >= 1 and divide n");
    hipStream_t s = as_stream(stream);
    SLK_RUN("group_center", 0, 8.0 * R * n, s,
            k_group_offsets<false><<<R < 4096 ? R : 4096, 256, 0, s>>>(W, R, n, group_size, const_cast<float *>(goffset), Wc));
    return SLK_OK;
}

}  // extern "C"
