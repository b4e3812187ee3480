// A stored MX layer against 16-bit activations, weight-only (W4A16, W6A16): slk_mx_gemm_a16 and, over the experts of a
// mixture-of-experts layer, slk_mx_gemm_experts_a16 (the contract is pinned in include/sleekit_amd.h and INTEGRATION.md).
// The layer stays as slk_mx_pack / slk_mx_pack6 left it -- E2M1 codes, 16 bytes a block of 32 columns, or E2M3 codes, 24 --
// and is de-quantized inside a bfloat16 / float16 MFMA GEMM (gemm16.h: the instruction, the activations' fragment, the
// store): nothing de-quantized reaches global memory, and the dense call has no workspace.
//
// A weight is the de-quantizer's own element (mx.hip, k_mx_dequantize): value(code) 2^(b - 127) in float32, rounded once
// to the compute type by the conversion that kernel uses.  Here the float32 product is formed without a multiply: the
// code's magnitude bits, moved to the top of a float32's mantissa and the bottom of its exponent, ARE value 2^-126 (the
// code's own subnormals become float32 subnormals), and v_ldexp_f32 by b - 1 is the exact product, rounded as the multiply
// rounds it where it underflows (scale byte 0 is 2^-127 on both routes) and infinite where it overflows.  Scale byte 255
// makes the whole block NaN, as the de-quantizer's multiply by NaN does.  One thing is not the de-quantizer's bit: the E2M1
// code 0x8, which it reads as +0, is -0 here -- a sum that starts from +0 cannot tell.
// So Wc is the de-quantizer's for EVERY scale byte; the operand contract is promised where every non-zero Wc is a normal
// number (bytes 10 .. 245 in bfloat16, 116 .. 140 in float16), and outside it a subnormal Wc meets whatever the MFMA does
// with subnormal operands, which nothing here examines.
//
// The map (the identity test of tests/test_gpu_mx_a16.py holds it).  a16_load_w brings lane (i, q) one whole block of weight row
// i: 16 or 24 bytes and the scale byte.  The order of k inside one 16x16x32 step is free as long as both operands agree,
// so the block's 32 weights feed FOUR MFMAs as four fragments of 8 consecutive k, and fragment t meets
// x[row i][32 block + 8 t + 0 .. 7]: weight loads stay whole blocks, x loads stay 16 bytes (bf16 / f16) or two of them.
#include "common.h"
#include "gemm16.h"
#include "mxexperts.h"
#include "mxquant.h"

namespace slk {

// ---------------------------------------------------------------- weights
// One block as stored: 4 (E2M1) or 6 (E2M3) words and the scale byte; zeros under the scale 1 where `ok` is false (past the end of K).
template <int WF>
struct WBlock {
    unsigned w[mxa_bits<WF>()];
    unsigned sb;
};
template <int WF>
__device__ __forceinline__ WBlock<WF> a16_load_w(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t row, int kb, int bpr,
                                                 bool ok) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    WBlock<WF> r;
#pragma unroll
    for (int k = 0; k < mxa_bits<WF>(); ++k) r.w[k] = 0u;
    r.sb = 127u;
    if (ok) {
        const size_t blk = row * bpr + kb;
        if constexpr (WF == MXA_E2M1) {
            const v4i v = *reinterpret_cast<const v4i *>(codes + 16 * blk);
#pragma unroll
            for (int k = 0; k < 4; ++k) r.w[k] = (unsigned)v[k];
        } else {  // a row starts on 8 bytes and a block every 24: three 8-byte loads, nothing past the layer
            const v2i *p = reinterpret_cast<const v2i *>(codes + 24 * blk);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const v2i v = p[k];
                r.w[2 * k] = (unsigned)v.x, r.w[2 * k + 1] = (unsigned)v.y;
            }
        }
        r.sb = E[blk];
    }
    return r;
}
// value(code) 2^-126 as float32 bits: E2M1 is sign, two exponent bits, one mantissa bit; E2M3 sign, two and three
template <int WF>
__device__ __forceinline__ unsigned a16_tiny(unsigned c) {
    if constexpr (WF == MXA_E2M1) return ((c & 7u) << 22) | ((c & 8u) << 28);
    else return ((c & 31u) << 20) | ((c & 32u) << 26);
}
// The block's 32 weights in the compute type, as the four B fragments of its four MFMAs.  To bfloat16 the conversion is a
// cut: a code has at most four significant bits and bfloat16 has float32's exponents, so the float32 product -- normal,
// subnormal (down to 2^-130 >= 2^-133), infinite or NaN -- is a bfloat16 already, and rounding to
// nearest even, which is what the de-quantizer does to it, has nothing to round.  To float16 it is the de-quantizer's own cast.
template <int WF, int C16>
__device__ __forceinline__ void a16_decode(const WBlock<WF> &b, v4i (&frag)[4]) {
    const unsigned nan = b.sb == 255u ? 0x7fc00000u : 0u;
    const int ex = (int)b.sb - 1;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float f[2];
#pragma unroll
            for (int e = 0; e < 2; ++e)
                f[e] = __builtin_ldexpf(__uint_as_float(a16_tiny<WF>(mxa_code_at<WF>(b.w, 8 * t + 2 * p + e)) | nan), ex);
            if constexpr (C16 == PK_BF16) frag[t][p] = (int)((__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xffff0000u));
            else frag[t][p] = (int)((unsigned)pg_cvt<C16>(f[0]) | ((unsigned)pg_cvt<C16>(f[1]) << 16));
        }
}

// One lane's loads of one block step: its block of the layer and the 32 elements of x that meet it.  CHECK: the block may
// lie past K, and then nothing is loaded and both sides are zeros.  Without it every load is unconditional, which is what
// lets the compiler count the loads in flight and wait for one step's while the next one's are still under way (behind a
// predicate it waits for all of them: vmcnt(0) after every step).
template <class TX, int WF>
struct A16Loads {
    WBlock<WF> w;
    XRaw<TX> x[4];
};
template <class TX, int WF, bool CHECK>
__device__ __forceinline__ A16Loads<TX, WF> a16_load(const TX *__restrict__ xrow, const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                     size_t wrow, int kb, int bpr) {
    const bool ok = !CHECK || kb < bpr;
    A16Loads<TX, WF> u;
    u.w = a16_load_w<WF>(Wc, Ws, wrow, kb, bpr, ok);
#pragma unroll
    for (int t = 0; t < 4; ++t) u.x[t] = pg_load_x<TX>(xrow + 32 * (size_t)kb + 8 * t, ok);
    return u;
}

// ---------------------------------------------------------------- few rows
// Up to MXG_SPLIT_MAX_M rows: the layer is read once per 16 rows and the time is its bytes, so a workgroup is one 16 x 16
// tile of Y and its MXG_SK waves share K: wave w takes the steps of four blocks w, w + SK, ... in this order, the next
// step's loads in flight while it works on one, and wave 0 adds the partial tiles in wave order.  Both orders are fixed.
// The whole steps (K / 128 of them) load without a predicate (the last one's look-ahead reads that step again); the step
// that K % 128 leaves is the last of the wave whose turn it is, with blocks past K zeros on both sides.
// A row past N reads row N - 1 and a row of x past `rows` reads row rows - 1 (their results are not stored).
// (row0 / rows: the tile's first row and the row bound of the matrix -- or of the expert --, n0 the tile's first column.)
template <class TX, int C16, int WF>
__device__ __forceinline__ v4f a16_step(const A16Loads<TX, WF> &u, v4f acc) {
    v4i b[4];
    a16_decode<WF, C16>(u.w, b);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = pg_mfma<C16>(pg_x_frag<TX, C16>(u.x[t]), b[t], acc);
    return acc;
}
template <class TX, int C16, int WF>
__device__ __forceinline__ void mx_a16_splitk_tile(const TX *__restrict__ X, const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                   const float *__restrict__ bias, int row0, int rows, int n0, int N, int K, int out_dtype,
                                                   void *__restrict__ Y) {
    __shared__ v4f part[MXG_SK - 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int bpr = K / 32, whole = bpr / 4;
    const size_t wrow = (size_t)min(n0 + i, N - 1);
    const TX *xrow = X + (size_t)min(row0 + i, rows - 1) * K;
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wave < whole) {
        A16Loads<TX, WF> cur = a16_load<TX, WF, false>(xrow, Wc, Ws, wrow, 4 * wave + q, bpr);
        for (int s = wave; s < whole; s += MXG_SK) {
            const A16Loads<TX, WF> next = a16_load<TX, WF, false>(xrow, Wc, Ws, wrow, 4 * min(s + MXG_SK, whole - 1) + q, bpr);
            acc = a16_step<TX, C16, WF>(cur, acc);
            cur = next;
        }
    }
    if (bpr % 4 && wave == whole % MXG_SK) acc = a16_step<TX, C16, WF>(a16_load<TX, WF, true>(xrow, Wc, Ws, wrow, 4 * whole + q, bpr), acc);
    if (wave) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int v = 0; v < MXG_SK - 1; ++v) acc += part[v][lane];
    pg_store_tile(acc, bias, row0 + 4 * q, n0 + i, rows, N, out_dtype, Y);
}
template <class TX, int C16, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_a16_splitk(const TX *__restrict__ X, const uint8_t *__restrict__ Wc,
                                                               const uint8_t *__restrict__ Ws, const float *__restrict__ bias, int M, int N,
                                                               int K, int out_dtype, void *__restrict__ Y) {
    mx_a16_splitk_tile<TX, C16, WF>(X, Wc, Ws, bias, blockIdx.y * 16, M, blockIdx.x * 16, N, K, out_dtype, Y);
}

// ---------------------------------------------------------------- many rows
// A workgroup of four waves owns a 64 x 64 tile of Y and walks K in steps of 128 (four blocks).  Thread t = 4 r + q loads
// block q of the step of row r, for W and for X (rows past N or `rows` read the last row), one step ahead of the MFMAs; it
// de-quantizes its block ONCE for the 64 rows of the tile and writes both operands into LDS in compute type, rows padded
// to A16_LD elements (272 bytes: 16 rows of 16-byte reads start 4 banks apart, as packgemm.hip's PG_LD has them).  Each
// wave then holds 32 x 32 of Y as 2 x 2 MFMA tiles: four 16-byte LDS reads feed four MFMAs per 32 columns.  No split of K
// across workgroups: one fixed order of sums.  Whole steps and the one K % 128 leaves as in the few-rows form.
constexpr int A16_BK = 128, A16_LD = A16_BK + 8;
template <class TX, int C16, int WF>
struct A16Tile {
    unsigned short (*xs)[A16_LD], (*ws)[A16_LD];
    int r, q, lane, wm, wn;
    v4f acc[2][2];
    // one step: this thread's block of both operands to LDS, then the wave's 2 x 2 MFMA tiles over the step's 128 columns
    __device__ __forceinline__ void step(const A16Loads<TX, WF> &u) {
        v4i wf[4];
        a16_decode<WF, C16>(u.w, wf);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<v4i *>(&ws[r][32 * q + 8 * j]) = wf[j];
            *reinterpret_cast<v4i *>(&xs[r][32 * q + 8 * j]) = pg_x_frag<TX, C16>(u.x[j]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
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
    }
};
template <class TX, int C16, int WF>
__device__ __forceinline__ void mx_a16_tiled_tile(const TX *__restrict__ X, const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                  const float *__restrict__ bias, int row0, int rows, int col0, int N, int K, int out_dtype,
                                                  void *__restrict__ Y) {
    __shared__ __attribute__((aligned(16))) unsigned short xs[64][A16_LD];
    __shared__ __attribute__((aligned(16))) unsigned short ws[64][A16_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    A16Tile<TX, C16, WF> tile = {xs, ws, t >> 2, t & 3, lane, (wave >> 1) * 32, (wave & 1) * 32, {}};
    const int bpr = K / 32, whole = bpr / 4;
    const size_t wrow = (size_t)min(col0 + tile.r, N - 1);
    const TX *xrow = X + (size_t)min(row0 + tile.r, rows - 1) * K;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) tile.acc[a][b] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    if (whole) {
        A16Loads<TX, WF> cur = a16_load<TX, WF, false>(xrow, Wc, Ws, wrow, tile.q, bpr);
        for (int s = 0; s < whole; ++s) {
            const A16Loads<TX, WF> next = a16_load<TX, WF, false>(xrow, Wc, Ws, wrow, 4 * min(s + 1, whole - 1) + tile.q, bpr);
            tile.step(cur);
            cur = next;
        }
    }
    if (bpr % 4) tile.step(a16_load<TX, WF, true>(xrow, Wc, Ws, wrow, 4 * whole + tile.q, bpr));
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f)
            pg_store_tile(tile.acc[e][f], bias, row0 + tile.wm + 16 * e + 4 * (lane >> 4), col0 + tile.wn + 16 * f + (lane & 15), rows, N,
                          out_dtype, Y);
}
template <class TX, int C16, int WF>
__global__ __launch_bounds__(256) void k_mx_a16_tiled(const TX *__restrict__ X, const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                      const float *__restrict__ bias, int M, int N, int K, int out_dtype,
                                                      void *__restrict__ Y) {
    mx_a16_tiled_tile<TX, C16, WF>(X, Wc, Ws, bias, blockIdx.y * 64, M, blockIdx.x * 64, N, K, out_dtype, Y);
}

// ---------------------------------------------------------------- a mixture-of-experts layer in one call
// The tile bodies above behind an ExpertTile, over the two tables k_mx_expert_tiles makes of the offsets (mxgemm.hip): each
// expert's rows take the form the dense call would choose for them alone, so they are that call's bit for bit.
template <class TX, int C16, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_a16_experts_splitk(const TX *__restrict__ X, const uint8_t *__restrict__ Wc,
                                                                       const uint8_t *__restrict__ Ws, const float *__restrict__ bias,
                                                                       const int *__restrict__ count, const int *__restrict__ table, int N,
                                                                       int K, int out_dtype, void *__restrict__ Y) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, N, K);
    mx_a16_splitk_tile<TX, C16, WF>(X, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 16, N, K, out_dtype, Y);
}
template <class TX, int C16, int WF>
__global__ __launch_bounds__(256) void k_mx_a16_experts_tiled(const TX *__restrict__ X, const uint8_t *__restrict__ Wc,
                                                              const uint8_t *__restrict__ Ws, const float *__restrict__ bias,
                                                              const int *__restrict__ count, const int *__restrict__ table, int N, int K,
                                                              int out_dtype, void *__restrict__ Y) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, N, K);
    mx_a16_tiled_tile<TX, C16, WF>(X, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 64, N, K, out_dtype, Y);
}

}  // namespace slk

using namespace slk;

// ---------------------------------------------------------------- the entries
// What both entries require, in slk_mx_gemm's order and words where it has them
static int a16_check(const void *X, int x_dtype, const void *w_codes, const void *w_scales, int w_fmt, int M, int N, int K, int compute_dtype,
                     int out_dtype, const void *out) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(X && w_codes && w_scales && out, "null pointer");
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(compute_dtype == SLK_DTYPE_BF16 || compute_dtype == SLK_DTYPE_F16, "compute_dtype must be SLK_DTYPE_BF16 or SLK_DTYPE_F16 (got %d)",
                compute_dtype);
    SLK_REQUIRE(w_fmt == SLK_MX_W_FP4 || w_fmt == SLK_MX_W_FP6, "unknown w_fmt %d", w_fmt);
    SLK_REQUIRE(aligned16(X) && aligned16(w_codes) && aligned16(out), "X, w_codes and out must be aligned to 16 bytes");
    return SLK_OK;
}

// f(x's element type, PkOut of the compute type, the weights' format as a constant): the one place the three become types
template <int W>
struct A16Fmt {
    static constexpr int WF = W;
};
template <class F>
static int a16_dispatch(int x_dtype, int compute_dtype, int w_fmt, F &&f) {
    return with_dtype(x_dtype, [&](auto tx) -> int {
        const auto with_fmt = [&](auto tc) -> int {
            if (w_fmt == SLK_MX_W_FP6) return f(tx, tc, A16Fmt<MXA_E2M3>());
            return f(tx, tc, A16Fmt<MXA_E2M1>());
        };
        return compute_dtype == SLK_DTYPE_BF16 ? with_fmt(PkOut<PK_BF16>()) : with_fmt(PkOut<PK_F16>());
    });
}
static inline double a16_bytes(int x_dtype, int w_fmt, int out_dtype, double layers, int M, int N, int K) {
    return layers * N * (w_fmt == SLK_MX_W_FP6 ? 25.0 : 17.0) * (K / 32) + (double)M * K * (x_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0) +
           (double)M * N * (out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0);
}

extern "C" {

int slk_mx_gemm_a16(const void *X, int x_dtype, const uint8_t *w_codes, const uint8_t *w_scales, int w_fmt, const float *bias, int M, int N,
                    int K, int compute_dtype, int out_dtype, void *out, slk_stream_t stream) {
    if (const int rc = a16_check(X, x_dtype, w_codes, w_scales, w_fmt, M, N, K, compute_dtype, out_dtype, out)) return rc;
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    hipStream_t s = as_stream(stream);
    const double flops = 2.0 * M * N * K, bytes = a16_bytes(x_dtype, w_fmt, out_dtype, 1.0, M, N, K);
    const char *name = w_fmt == SLK_MX_W_FP6 ? "mx_gemm_a16_w6" : "mx_gemm_a16";
    return a16_dispatch(x_dtype, compute_dtype, w_fmt, [&](auto tx, auto tc, auto wf) -> int {
        typedef typename decltype(tx)::T TX;
        constexpr int C16 = decltype(tc)::OUT, WF = decltype(wf)::WF;
        const TX *x = static_cast<const TX *>(X);
        if (M <= MXG_SPLIT_MAX_M) {
            const dim3 grid((N + 15) / 16, (M + 15) / 16);
            SLK_RUN(name, flops, bytes, s, (k_mx_a16_splitk<TX, C16, WF><<<grid, 64 * MXG_SK, 0, s>>>(x, w_codes, w_scales, bias, M, N, K, out_dtype, out)));
        } else {
            const dim3 grid((N + 63) / 64, (M + 63) / 64);
            SLK_RUN(name, flops, bytes, s, (k_mx_a16_tiled<TX, C16, WF><<<grid, 256, 0, s>>>(x, w_codes, w_scales, bias, M, N, K, out_dtype, out)));
        }
        return SLK_OK;
    });
}

// The prologue, the split-K product over the 16-row table and, where an expert can have more than MXG_SPLIT_MAX_M rows at
// all, the tiled product over the 64-row table; in order on the stream (slk_mx_gemm_experts' three launches)
int slk_mx_gemm_experts_a16(const void *X, int x_dtype, const uint8_t *w_codes, const uint8_t *w_scales, int w_fmt, const float *bias,
                            const int *offsets, int E, int M, int N, int K, int compute_dtype, int out_dtype, void *out, int *flag,
                            void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(E >= 1 && E <= SLK_MX_MAX_EXPERTS, "E must be 1 .. %d experts (E = %d)", SLK_MX_MAX_EXPERTS, E);
    if (const int rc = a16_check(X, x_dtype, w_codes, w_scales, w_fmt, M, N, K, compute_dtype, out_dtype, out)) return rc;
    SLK_REQUIRE(flag, "null flag");
    if (const int rc = mx_check_experts(E, M, offsets, workspace, ws_bytes)) return rc;
    hipStream_t s = as_stream(stream);
    int *ws = static_cast<int *>(workspace);
    ExpertGrid g;
    if (const int rc = mx_expert_prologue(offsets, E, M, ws, flag, s, g)) return rc;
    const double flops = 2.0 * M * N * K, bytes = a16_bytes(x_dtype, w_fmt, out_dtype, (double)E, M, N, K);
    const char *name = w_fmt == SLK_MX_W_FP6 ? "mx_gemm_experts_a16_w6" : "mx_gemm_experts_a16";
    return a16_dispatch(x_dtype, compute_dtype, w_fmt, [&](auto tx, auto tc, auto wf) -> int {
        typedef typename decltype(tx)::T TX;
        constexpr int C16 = decltype(tc)::OUT, WF = decltype(wf)::WF;
        const TX *x = static_cast<const TX *>(X);
        const dim3 grid16((N + 15) / 16, g.rows16), grid64((N + 63) / 64, g.rows64);
        SLK_RUN(name, flops, bytes, s,
                (k_mx_a16_experts_splitk<TX, C16, WF><<<grid16, 64 * MXG_SK, 0, s>>>(x, w_codes, w_scales, bias, ws, g.t16, N, K, out_dtype, out)));
        if (M > MXG_SPLIT_MAX_M)
            SLK_RUN(name, 0, 0, s,
                    (k_mx_a16_experts_tiled<TX, C16, WF><<<grid64, 256, 0, s>>>(x, w_codes, w_scales, bias, ws + 1, g.t64, N, K, out_dtype, out)));
        return SLK_OK;
    });
}

}  // extern "C"
