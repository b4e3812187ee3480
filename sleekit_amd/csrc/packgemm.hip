// A linear layer computed from bit-packed codebook indices (slk_packed_gemm; the format is pack.hip's, pinned in
// include/sleekit_amd.h and INTEGRATION.md): the words are de-quantized inside a bfloat16 / float16 MFMA GEMM, nothing
// de-quantized reaches global memory and there is no workspace.
//
// v_mfma_f32_16x16x32_{bf16,f16} as gemm16.h states it (the instruction, the activations' fragment and the result's store
// are there, shared with mxgemm_a16.hip).  One MFMA step is K = 32: one chunk of the format, `bits`
// words of a weight row, of which the lane of quarter q needs bits [8 q b, 8 q b + 8 b) -- a FRAGMENT: 8 consecutive k of
// one row.  K % 8 == 0 and g % 8 == 0 put a fragment wholly inside or outside the row and under one scale and offset.
//
// A weight is value(min(index, levels - 1)) / (1 / s) [+ o] in float32, true divides in this order, rounded once to the
// compute type: slk_dequantize_packed's element.  It is formed either DIRECTLY, per element, or -- where a (row, group)
// has few distinct values against its length -- once per distinct value into a TABLE of compute-type values in LDS, built
// with the same arithmetic and then indexed (pg_table_mode).
#include "common.h"
#include "gemm16.h"

namespace slk {

enum { PG_NONE = 0, PG_ROW = 1, PG_GROUP = 2, PG_GROUP_OFF = 3 };

constexpr int PG_ROWS_MAX_M = 16;     // up to here the few-rows kernel
constexpr int PG_SK = 8;              // its waves, which share K
constexpr int PG_UNIT = 4;            // chunks a wave takes at a time: 128 columns
constexpr int PG_TABLE_LEVELS = 64;   // the largest codebook a table is built for
constexpr int PG_TAB_LD = PG_TABLE_LEVELS + 4;  // a table row's stride: 34 dwords, so that the short tables of 16 rows (8
                                                // entries are 4 dwords) lie in 16 different sets of banks, not in two
constexpr int PG_BM = 64, PG_BN = 64, PG_BK = 64;  // the tile kernel's workgroup tile; a wave holds 32 x 32
constexpr int PG_LD = PG_BK + 8;      // LDS row stride in elements: 144 bytes, so that 16-byte row reads spread over the banks

// The weights of a layer, by value.
struct PgW {
    const unsigned *words;
    const float *scale;   // PG_ROW: (N); PG_GROUP*: (N, G)
    const float *goffset;
    Grid grid;
    int bits, kind, gsize, G, wpr;  // wpr: words a row
    int table;                      // the table form (pg_table_mode)
};

// the tile kernel's workgroups for an M x N result
static inline long long pg_tiles(int M, int N) { return (((long long)M + PG_BM - 1) / PG_BM) * (((long long)N + PG_BN - 1) / PG_BN); }

// The table form pays `levels` de-quantized values per (row, group) for `g` direct ones; it needs a chunk (few rows) or
// a K-step (tiles) to lie in one group.  Without group scales the table is per row and serves all of K.
static inline int pg_table_mode(int levels, int kind, int g, int span) {
    if (levels > PG_TABLE_LEVELS) return 0;
    return kind < PG_GROUP || (g % span == 0 && 2 * levels <= g);
}

// ---------------------------------------------------------------- weights
// The words that hold bits [8 q b, 8 q b + 8 b) of the chunk whose b words start at `w`: one to three dword loads, all
// inside the chunk (its last bit is below 32 b).  A row of words starts on a 4-byte boundary only, so nothing wider.
struct WRaw {
    unsigned a, b, c;
};
__device__ __forceinline__ WRaw pg_load_w(const unsigned *__restrict__ w, int q, int b, bool ok) {
    WRaw r = {0u, 0u, 0u};
    const int bit = 8 * q * b, w0 = bit >> 5, end = (bit & 31) + 8 * b;
    if (ok) {
        r.a = w[w0];
        if (end > 32) r.b = w[w0 + 1];
        if (end > 64) r.c = w[w0 + 2];
    }
    return r;
}
// ... as one integer: index j of the fragment is its bits [j b, j b + b)
__device__ __forceinline__ unsigned long long pg_frag_bits(const WRaw r, int q, int b) {
    const int sh = (8 * q * b) & 31;
    unsigned long long x = ((unsigned long long)r.b << 32 | r.a) >> sh;
    if (sh + 8 * b > 64) x |= (unsigned long long)r.c << (64 - sh);  // (then sh > 0)
    return x;
}

// value / (1 / s) [+ o]: the group quantizer's own de-scale (GroupQ::dequant of common.h, which slk_dequantize_packed's
// element is), picked by the kind of scales; rs = 1 / s
__device__ __forceinline__ float pg_descale(float v, int kind, float rs, float o) {
    if (kind == PG_GROUP_OFF) return GroupQ<true>{0.0f, rs, o}.dequant(v);
    if (kind >= PG_ROW) return GroupQ<false>{0.0f, rs, 0.0f}.dequant(v);
    return v;
}

// A fragment's eight weights in compute type: from the row's table `tab`, or directly with the codebook values `lut`.
template <int C16>
__device__ __forceinline__ v4i pg_w_frag(unsigned long long x, int b, int top, const unsigned short *tab, const float *lut, int kind,
                                         float rs, float o) {
    const unsigned mask = (1u << b) - 1u;
    unsigned e[8];
    if (tab) {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = tab[min((int)((unsigned)(x >> (j * b)) & mask), top)];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = pg_cvt<C16>(pg_descale(lut[min((int)((unsigned)(x >> (j * b)) & mask), top)], kind, rs, o));
    }
    return (v4i){(int)(e[0] | e[1] << 16), (int)(e[2] | e[3] << 16), (int)(e[4] | e[5] << 16), (int)(e[6] | e[7] << 16)};
}

// Entries k = first, first + stride, ... of one row's table under (rs, o).
template <int C16>
__device__ __forceinline__ void pg_build_row(unsigned short *tab, const float *lut, int levels, int first, int stride, int kind, float rs,
                                             float o) {
    for (int k = first; k < levels; k += stride) tab[k] = pg_cvt<C16>(pg_descale(lut[k], kind, rs, o));
}

// LDS traffic inside ONE wave (a wave's own table): its LDS instructions run in order, so only the compiler is held.
__device__ __forceinline__ void pg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------- few rows
// M <= PG_ROWS_MAX_M: the layer is read once and the time is its bytes, so a workgroup is one 16-column tile of Y and
// its PG_SK waves share K: wave w takes the units (PG_UNIT chunks, 128 columns) w, w + PG_SK, ... in this order, with the
// next unit's loads in flight while it works on one, and wave 0 adds the partial tiles in wave order.  Both orders are
// fixed.  A row past N reads row N - 1 and a row of x past M reads row M - 1 (their results are not stored); a fragment
// past K is zeros on both sides by predicate, and loads nothing.
// The loads of CH consecutive chunks from chunk `first` on, for the lane of quarter q: its words, its 8 elements of x and
// its fragment's scale and offset.
template <class TX, int CH>
struct PgLoads {
    WRaw w[CH];
    XRaw<TX> x[CH];
    float s[CH], o[CH];
};
template <class TX, int CH>
__device__ __forceinline__ PgLoads<TX, CH> pg_load(const TX *__restrict__ xrow, const PgW &w, size_t wrow, int first, int q, int K) {
    PgLoads<TX, CH> u;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        const int c = first + j, k0 = 32 * c + 8 * q;
        const bool ok = k0 < K;
        u.w[j] = pg_load_w(w.words + wrow * w.wpr + (size_t)w.bits * c, q, w.bits, ok);
        u.x[j] = pg_load_x<TX>(xrow + k0, ok);
        u.s[j] = 1.0f;
        u.o[j] = 0.0f;
        if (ok && w.kind >= PG_GROUP) {
            const size_t at = wrow * w.G + k0 / w.gsize;
            u.s[j] = w.scale[at];
            if (w.kind == PG_GROUP_OFF) u.o[j] = w.goffset[at];
        }
    }
    return u;
}

template <class TX, int C16>
__global__ __launch_bounds__(64 * PG_SK) void k_packed_gemm_rows(const TX *__restrict__ X, const PgW w, const float *__restrict__ bias, int M,
                                                                int N, int K, int out_dtype, void *__restrict__ Y) {
    __shared__ v4f part[PG_SK - 1][64];
    __shared__ float lut[256];
    __shared__ unsigned short tab[PG_SK][16][PG_TAB_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int levels = w.grid.n, top = levels - 1;
    const size_t wrow = (size_t)min((int)blockIdx.x * 16 + i, N - 1);
    const TX *xrow = X + (size_t)min(i, M - 1) * K;
    for (int k = threadIdx.x; k < levels; k += blockDim.x) lut[k] = cb_entry(k, w.grid);
    __syncthreads();
    float rs = 1.0f;
    if (w.kind == PG_ROW) rs = 1.0f / w.scale[wrow];
    const bool shared_table = w.table && w.kind < PG_GROUP, wave_table = w.table && w.kind >= PG_GROUP;
    if (shared_table) {  // one table a row for all of K: lane (i, q) of wave v writes entries 4 v + q, + 32, ...
        pg_build_row<C16>(tab[0][i], lut, levels, 4 * wave + q, 4 * PG_SK, w.kind, rs, 0.0f);
        __syncthreads();
    }
    const unsigned short *mytab = w.table ? tab[shared_table ? 0 : wave][i] : nullptr;
    const int chunks = (K + 31) / 32, units = (chunks + PG_UNIT - 1) / PG_UNIT;
    int built = -1;
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    PgLoads<TX, PG_UNIT> cur = pg_load<TX, PG_UNIT>(xrow, w, wrow, PG_UNIT * wave, q, K);  // (a unit past the end loads nothing and is zeros)
    for (int u = wave; u < units; u += PG_SK) {
        const PgLoads<TX, PG_UNIT> next = pg_load<TX, PG_UNIT>(xrow, w, wrow, PG_UNIT * (u + PG_SK), q, K);
#pragma unroll
        for (int j = 0; j < PG_UNIT; ++j) {
            const int c = PG_UNIT * u + j, k0 = 32 * c + 8 * q;
            if (wave_table && 32 * c < K && 32 * c / w.gsize != built) {  // (wave-uniform; g % 32 == 0: the chunk is in one group)
                built = 32 * c / w.gsize;
                pg_wave_sync();
                pg_build_row<C16>(tab[wave][i], lut, levels, q, 4, w.kind, 1.0f / cur.s[j], cur.o[j]);
                pg_wave_sync();
            }
            v4i b = {0, 0, 0, 0};
            if (k0 < K) {
                const float frs = w.kind >= PG_GROUP ? 1.0f / cur.s[j] : rs;
                b = pg_w_frag<C16>(pg_frag_bits(cur.w[j], q, w.bits), w.bits, top, mytab, lut, w.kind, frs, cur.o[j]);
            }
            acc = pg_mfma<C16>(pg_x_frag<TX, C16>(cur.x[j]), b, acc);
        }
        cur = next;
    }
    if (wave) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int v = 0; v < PG_SK - 1; ++v) acc += part[v][lane];
    pg_store_tile(acc, bias, 4 * q, blockIdx.x * 16 + i, M, N, out_dtype, Y);
}

// ---------------------------------------------------------------- many rows
// A workgroup of four waves owns a 64 x 64 tile of Y and walks K in steps of 64 (two chunks).  Thread t = 4 r + q loads
// fragment q of row r of both chunks of the step, for X and for W (rows past M or N read the last row), one step ahead
// of the MFMAs; it de-quantizes its two weight fragments ONCE for the 64 rows of the tile and writes both operands into
// LDS in compute type, rows padded to 144 bytes.  Each wave then holds 32 x 32 of Y as 2 x 2 MFMA tiles: four 16-byte LDS
// reads feed four MFMAs per chunk.  No split of K across workgroups: one fixed order of sums.
template <class TX, int C16>
__global__ __launch_bounds__(256) void k_packed_gemm_tile(const TX *__restrict__ X, const PgW w, const float *__restrict__ bias, int M, int N,
                                                          int K, int out_dtype, void *__restrict__ Y) {
    __shared__ __attribute__((aligned(16))) unsigned short xs[PG_BM][PG_LD];
    __shared__ __attribute__((aligned(16))) unsigned short ws[PG_BN][PG_LD];
    __shared__ unsigned short tab[PG_BN][PG_TAB_LD];
    __shared__ float lut[256];
    const int t = threadIdx.x, r = t >> 2, q = t & 3, lane = t & 63, wave = t >> 6;
    const int tiles_n = (N + PG_BN - 1) / PG_BN;  // (the tiles of Y are folded into grid.x, N fastest)
    const int m0 = (int)(blockIdx.x / tiles_n) * PG_BM, n0 = (int)(blockIdx.x % tiles_n) * PG_BN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int levels = w.grid.n, top = levels - 1;
    const size_t wrow = (size_t)min(n0 + r, N - 1);
    const TX *xrow = X + (size_t)min(m0 + r, M - 1) * K;
    for (int k = t; k < levels; k += 256) lut[k] = cb_entry(k, w.grid);
    __syncthreads();
    float rs = 1.0f;
    if (w.kind == PG_ROW) rs = 1.0f / w.scale[wrow];
    const bool step_table = w.table && w.kind >= PG_GROUP;
    if (w.table && w.kind < PG_GROUP) {
        pg_build_row<C16>(tab[r], lut, levels, q, 4, w.kind, rs, 0.0f);
        __syncthreads();
    }
    const unsigned short *mytab = w.table ? tab[r] : nullptr;
    const int steps = (K + PG_BK - 1) / PG_BK;
    int built = -1;
    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    PgLoads<TX, 2> cur = pg_load<TX, 2>(xrow, w, wrow, 0, q, K);
    for (int s = 0; s < steps; ++s) {
        const PgLoads<TX, 2> next = pg_load<TX, 2>(xrow, w, wrow, 2 * (s + 1), q, K);  // (past the end: nothing loaded)
        if (step_table && PG_BK * s / w.gsize != built) {  // (uniform; g % 64 == 0: the step is in one group; the last
            built = PG_BK * s / w.gsize;                    //  reads of the old table lie before the barrier that ended step s - 1)
            pg_build_row<C16>(tab[r], lut, levels, q, 4, w.kind, 1.0f / cur.s[0], cur.o[0]);
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k0 = PG_BK * s + 32 * j + 8 * q;
            v4i b = {0, 0, 0, 0};
            if (k0 < K) {
                const float frs = w.kind >= PG_GROUP ? 1.0f / cur.s[j] : rs;
                b = pg_w_frag<C16>(pg_frag_bits(cur.w[j], q, w.bits), w.bits, top, mytab, lut, w.kind, frs, cur.o[j]);
            }
            *reinterpret_cast<v4i *>(&ws[r][32 * j + 8 * q]) = b;
            *reinterpret_cast<v4i *>(&xs[r][32 * j + 8 * q]) = pg_x_frag<TX, C16>(cur.x[j]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            v4i a[2], b[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[e] = *reinterpret_cast<const v4i *>(&xs[wm + 16 * e + (lane & 15)][32 * j + 8 * (lane >> 4)]);
                b[e] = *reinterpret_cast<const v4i *>(&ws[wn + 16 * e + (lane & 15)][32 * j + 8 * (lane >> 4)]);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int f = 0; f < 2; ++f) acc[e][f] = pg_mfma<C16>(a[e], b[f], acc[e][f]);
        }
        __syncthreads();
        cur = next;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
            pg_store_tile(acc[e][f], bias, m0 + wm + 16 * e + 4 * (lane >> 4), n0 + wn + 16 * f + (lane & 15), M, N, out_dtype, Y);
}

template <class TX, int C16>
static int packed_gemm_launch(const void *X, PgW w, const float *bias, int M, int N, int K, int out_dtype, void *out, double bytes,
                              hipStream_t s) {
    const double flops = 2.0 * M * N * K;
    const TX *x = static_cast<const TX *>(X);
    if (M <= PG_ROWS_MAX_M) {
        w.table = pg_table_mode(w.grid.n, w.kind, w.gsize, 32);
        SLK_RUN("packed_gemm", flops, bytes, s,
                k_packed_gemm_rows<TX, C16><<<(N + 15) / 16, 64 * PG_SK, 0, s>>>(x, w, bias, M, N, K, out_dtype, out));
    } else {
        w.table = pg_table_mode(w.grid.n, w.kind, w.gsize, PG_BK);
        const unsigned grid = (unsigned)(pg_tiles(M, N));
        SLK_RUN("packed_gemm", flops, bytes, s, k_packed_gemm_tile<TX, C16><<<grid, 256, 0, s>>>(x, w, bias, M, N, K, out_dtype, out));
    }
    return SLK_OK;
}

template <int C16>
static int packed_gemm_x(int x_dtype, const void *X, const PgW &w, const float *bias, int M, int N, int K, int out_dtype, void *out,
                         double bytes, hipStream_t s) {
    if (x_dtype == SLK_DTYPE_BF16) return packed_gemm_launch<unsigned short, C16>(X, w, bias, M, N, K, out_dtype, out, bytes, s);
    if (x_dtype == SLK_DTYPE_F16) return packed_gemm_launch<_Float16, C16>(X, w, bias, M, N, K, out_dtype, out, bytes, s);
    return packed_gemm_launch<float, C16>(X, w, bias, M, N, K, out_dtype, out, bytes, s);
}

}  // namespace slk

using namespace slk;

static inline bool pg_known_dtype(int d) { return d == SLK_DTYPE_F32 || d == SLK_DTYPE_BF16 || d == SLK_DTYPE_F16; }

extern "C" {

int slk_packed_gemm(const void *X, int x_dtype, const uint32_t *words, int bits, int levels, double lo, double hi, const float *table,
                    const float *scale, const float *gscale, const float *goffset, int group_size, const float *bias, int M, int N, int K,
                    int compute_dtype, int out_dtype, void *out, slk_stream_t stream) {
    SLK_REQUIRE(M >= 1 && N >= 1, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 8 && K % 8 == 0,
                "K must be a positive multiple of 8 (K = %d): de-quantize such a layer with slk_dequantize_packed (dequantize_packed)", K);
    SLK_REQUIRE(bits >= 1 && bits <= 8, "bits must be in 1..8 (got %d)", bits);
    SLK_REQUIRE(levels >= 2 && levels <= (1 << bits), "levels must be in 2..2^bits (levels = %d, bits = %d)", levels, bits);
    SLK_REQUIRE(table || lo < hi, "a uniform codebook needs lo < hi");
    SLK_REQUIRE(!(scale && gscale), "scale and gscale are mutually exclusive");
    SLK_REQUIRE(!goffset || gscale, "goffset needs gscale");
    SLK_REQUIRE(!gscale || (group_size >= 8 && group_size % 8 == 0 && K % group_size == 0),
                "group_size must be a multiple of 8 that divides K (group_size = %d, K = %d): de-quantize such a layer with "
                "slk_dequantize_packed (dequantize_packed)", group_size, K);
    SLK_REQUIRE(X && words && out, "null pointer (X, words and out are required)");
    SLK_REQUIRE(pg_known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(pg_known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(compute_dtype == SLK_DTYPE_BF16 || compute_dtype == SLK_DTYPE_F16, "compute_dtype must be SLK_DTYPE_BF16 or SLK_DTYPE_F16 (got %d)",
                compute_dtype);
    SLK_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)out % 16 == 0, "X and out must be aligned to 16 bytes");
    SLK_REQUIRE((uintptr_t)words % 4 == 0, "words must be aligned to 4 bytes");
    SLK_REQUIRE(M <= PG_ROWS_MAX_M || pg_tiles(M, N) <= 0x7fffffffLL, "M x N is above the 2^31 - 1 tiles of 64 x 64 of one launch (M = %d, N = %d)",
                M, N);
    hipStream_t s = as_stream(stream);
    PgW w;
    w.words = words;
    w.scale = gscale ? gscale : scale;
    w.goffset = goffset;
    w.grid = make_grid(levels, lo, hi, table);
    w.bits = bits;
    w.kind = goffset ? PG_GROUP_OFF : (gscale ? PG_GROUP : (scale ? PG_ROW : PG_NONE));
    w.gsize = gscale ? group_size : K;
    w.G = K / w.gsize;
    w.wpr = bits * ((K + 31) / 32);
    w.table = 0;
    const double side = gscale ? (goffset ? 8.0 : 4.0) * ((double)N * w.G) : (scale ? 4.0 * N : 0.0);
    const double bytes = 4.0 * N * w.wpr + side + (double)M * K * (x_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0) +
                         (double)M * N * (out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0);
    if (compute_dtype == SLK_DTYPE_BF16) return packed_gemm_x<PK_BF16>(x_dtype, X, w, bias, M, N, K, out_dtype, out, bytes, s);
    return packed_gemm_x<PK_F16>(x_dtype, X, w, bias, M, N, K, out_dtype, out, bytes, s);
}

}  // extern "C"
