// The product of a linear layer in a packed MX form on the block-scaled MFMA, and that product over the experts of a
// mixture-of-experts layer (slk_mx_gemm, _a4, _a6, _w6, slk_mx_gemm_experts; the formats are pinned in include/sleekit_amd.h
// and INTEGRATION.md).  Nothing here converts: the kernels that write and read back these forms are mx.hip's.  The one
// exception is the fused gate/up product of a gated MLP (slk_mx_gemm_glu, _experts), whose epilogue ends in the plain
// quantizer's own block encoder (mxq_encode, mxquant.h) and writes the next layer's activations.
// The entries at the end share one dispatcher from (a_fmt, w_fmt) to a pair of template arguments (with_pair), one list of
// what a product requires of its operands (mx_check_operands; the gated and the expert-grouped entries add theirs) and one
// prologue for the two expert-grouped products (mx_expert_prologue).
//
// Weights stay as slk_mx_pack left them: FP4 E2M1 codes, two a byte, and one E8M0 byte per block of 32 columns -- or, for
// an MXFP6 layer (slk_mx_gemm_w6), as slk_mx_pack6 left them: E2M3 codes, 24 bytes a block.
// Activations come as slk_mx_quantize_act left them, MXFP8: E4M3 codes, one a byte, under the same kind of block scale -- or
// as MXFP4 (_act4), in the weights' own form, or as MXFP6 (_act6: E2M3, 24 bytes a block).
//
// v_mfma_scale_f32_16x16x128_f8f6f4, as found on the hardware and held by the one-hot test of
// tests/test_gpu_mx_gemm.py.  Lane l = i + 16 q carries row (A) or column (B) i.
//   B, E2M1 (4 VGPRs): the 32 consecutive k of block q, 16 bytes, the even k in the low nibble.
//   A, E4M3 (8 VGPRs): VGPRs 0-3 hold k = 16 q + 0 .. 15, VGPRs 4-7 hold k = 64 + 16 q + 0 .. 15, in k order -- the
//      instruction runs as two halves of 64 -- so a lane's bytes are two 16-byte pieces of its row, from two blocks.
//   scales: the byte of lane i + 16 b's scale VGPR that op_sel names is the E8M0 scale of (row or column i, block b) for
//      both operands, whichever lanes carry that block's elements.
//   A, E2M1 (4 VGPRs; slk_mx_gemm_a4, MXFP4 activations): as B -- the 32 consecutive k of block q, the even k low.
//   A, E2M3 (6 VGPRs; slk_mx_gemm_a6, MXFP6 activations): the 32 consecutive k of block q as one little-endian stream of
//      192 bits, element j of the block at bits 6 j .. 6 j + 5 of VGPRs 0-5 -- not cut in halves, the stored form as it is
//      (held by the one-hot test of tests/test_gpu_mx_act6.py).
//   B, E2M3 (6 VGPRs, blgp = 2; slk_mx_gemm_w6, MXFP6 layers): that map mirrored -- lane i + 16 q carries column i and the 32
//      consecutive k of block q as the stored stream in VGPRs 0-5 (held by the one-hot test of tests/test_gpu_mx6.py).
// The stored forms feed the instruction with plain loads (16 bytes a piece; three of 8 for E2M3): no shuffle, no pre-swizzle, no LDS.
// D: lane l holds column l & 15, rows 4 (l >> 4) + 0 .. 3.
#include "common.h"
#include "hadamard.h"
#include "mxexperts.h"
#include "mxglu.h"
#include "mxquant.h"

#include <math.h>

namespace slk {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- the product
// One lane's share of a 16 x 128 operand step (the map above), or zeros (and the scale 1) past the rows or past the
// blocks, so nothing outside a buffer of exactly its stated size is read.
template <int AF>
struct FragA {
    int v[mxa_bits<AF>()];  // 8, 4 or 6 VGPRs
    int sc;
};
template <int WF = MXA_E2M1>
struct FragB;
template <>
struct FragB<MXA_E2M1> {
    v4i v;
    int sc;
};
template <>
struct FragB<MXA_E2M3> {
    int v[6];
    int sc;
};
template <int AF>
__device__ __forceinline__ FragA<AF> load_a_block(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int kb,
                                                  int bpr);
// The B fragment: the lane's block of the layer, 16 bytes of E2M1 in one load, or 24 bytes of E2M3 as three 8-byte loads
// (load_a_block below: exactly 24 bytes, so the last block of the last row reads nothing past the layer's 3 N K / 4 bytes).
template <int WF = MXA_E2M1>
__device__ __forceinline__ FragB<WF> load_b(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int kb,
                                            int bpr) {
    if constexpr (WF == MXA_E2M1) {
        FragB<WF> f;
        f.v = (v4i){0, 0, 0, 0};
        f.sc = 127;
        if (row < rows && kb < bpr) {
            const size_t blk = (size_t)row * bpr + kb;
            f.v = *reinterpret_cast<const v4i *>(codes + 16 * blk);
            f.sc = E[blk];
        }
        return f;
    } else {
        const FragA<WF> a = load_a_block<WF>(codes, E, row, rows, kb, bpr);
        return {{a.v[0], a.v[1], a.v[2], a.v[3], a.v[4], a.v[5]}, a.sc};
    }
}
// The A fragment of each activation format (load_a).  E4M3: two 16-byte pieces of the row, from two blocks (the two halves
// of the map above).  E2M1 activations are stored like the weights and map like them (held by the one-hot test of
// tests/test_gpu_mx_act4.py): lane i + 16 q carries the 32 consecutive k of block q of row i under that block's scale, so
// the fragment is B's, one 16-byte load.  E2M3 activations (tests/test_gpu_mx_act6.py) map the same way -- the 32
// consecutive k of block q in VGPRs 0-5, in the stored bit order -- so a lane's fragment is the 24 bytes of its block
// (load_a_block).  A row starts on 8 bytes and a block every 24, so these are three 8-byte loads: 24 bytes exactly, and the
// last block of the last row reads nothing past the buffer's 3 M K / 4 bytes, which a 16-byte pair of loads would.
// (load_a_block would serve E2M1 too, as two 8-byte loads; it keeps load_b's one, and the kernels the code they had:
// DESIGN.md section 21.)
template <int AF>
__device__ __forceinline__ FragA<AF> load_a_block(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int kb,
                                                  int bpr) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    constexpr int WORDS = mxa_bits<AF>();
    FragA<AF> f;
#pragma unroll
    for (int i = 0; i < WORDS; ++i) f.v[i] = 0;
    f.sc = 127;
    if (row < rows && kb < bpr) {
        const size_t blk = (size_t)row * bpr + kb;
        const v2i *p = reinterpret_cast<const v2i *>(codes + 4 * WORDS * blk);
#pragma unroll
        for (int i = 0; i < WORDS / 2; ++i) {
            const v2i w = p[i];
            f.v[2 * i] = w.x, f.v[2 * i + 1] = w.y;
        }
        f.sc = E[blk];
    }
    return f;
}
template <int AF>
__device__ __forceinline__ FragA<AF> load_a(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int step,
                                            int q, int bpr) {
    if constexpr (AF == MXA_E4M3) {
        FragA<AF> f;
        f.sc = 127;
        v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (row < rows) {
            const uint8_t *p = codes + 32 * ((size_t)row * bpr + 4 * step) + 16 * q;  // k = 128 step + 16 q
            if (4 * step + (q >> 1) < bpr) lo = *reinterpret_cast<const v4i *>(p);
            if (4 * step + 2 + (q >> 1) < bpr) hi = *reinterpret_cast<const v4i *>(p + 64);
            if (4 * step + q < bpr) f.sc = E[(size_t)row * bpr + 4 * step + q];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) f.v[i] = i < 4 ? lo[i] : hi[i - 4];
        return f;
    } else if constexpr (AF == MXA_E2M1) {
        const FragB<> b = load_b(codes, E, row, rows, 4 * step + q, bpr);
        return {{b.v.x, b.v.y, b.v.z, b.v.w}, b.sc};
    } else {
        return load_a_block<AF>(codes, E, row, rows, 4 * step + q, bpr);
    }
}
// acc += A (16 x 128) B^T (E2M1 or E2M3, 16 x 128), each lane's block under its own scale.  The instruction takes eight VGPRs a
// side and reads as many of them as the format has; with A in E2M1 or E2M3 it runs at twice the E4M3 rate.
template <int AF>
__host__ __device__ constexpr int mx_cbsz() { return AF == MXA_E2M1 ? 4 : AF == MXA_E2M3 ? 2 : 0; }
template <int AF, int WF = MXA_E2M1>
__device__ __forceinline__ v4f mx_mfma(const FragA<AF> a, const FragB<WF> b, v4f acc) {
    v8i av = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < mxa_bits<AF>(); ++i) av[i] = a.v[i];
    v8i bv = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < mxa_bits<WF>(); ++i) bv[i] = b.v[i];
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, mx_cbsz<AF>(), mx_cbsz<WF>() /* blgp: B's format */, 0, a.sc, 0, b.sc);
}

template <int OUT>
__device__ __forceinline__ void store_tile(v4f acc, const float *__restrict__ bias, int m0, int n, int M, int N,
                                           typename PkOut<OUT>::T *__restrict__ Y) {
    if (n >= N) return;
    const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + r;
        if (m < M) Y[(size_t)m * N + n] = PkOut<OUT>::cvt(bias ? acc[r] + bv : acc[r]);
    }
}

// Few rows (M <= MXG_SPLIT_MAX_M): the weights are read once and the time is their bandwidth, so a workgroup is one
// 16 x 16 tile of Y and its SK waves share K: wave w takes the 128-steps w, w + SK, ..., in this order, and wave 0 adds
// the SK partial tiles in wave order.  Both orders are fixed, so a result does not depend on timing.
// (MXG_SK and MXG_SPLIT_MAX_M are mxexperts.h's: mxgemm_a16.hip switches forms where this file does.  The body is shared
// with the expert-grouped kernel below: row0 / rows are the tile's first row and the row bound of the matrix -- or of the
// expert --, n0 the tile's first column.)
template <int OUT, int AF, int WF>
__device__ __forceinline__ void mx_gemm_splitk_tile(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                    const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                    const float *__restrict__ bias, int row0, int rows, int n0, int N, int K,
                                                    typename PkOut<OUT>::T *__restrict__ Y) {
    __shared__ v4f part[MXG_SK - 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m = row0 + (lane & 15), n = n0 + (lane & 15), q = lane >> 4;
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = wave; s < steps; s += 2 * MXG_SK) {  // two steps' loads in flight; a step past the end loads zeros
        const FragA<AF> a0 = load_a<AF>(Ac, As, m, rows, s, q, bpr), a1 = load_a<AF>(Ac, As, m, rows, s + MXG_SK, q, bpr);
        const FragB<WF> b0 = load_b<WF>(Wc, Ws, n, N, 4 * s + q, bpr), b1 = load_b<WF>(Wc, Ws, n, N, 4 * (s + MXG_SK) + q, bpr);
        acc = mx_mfma<AF, WF>(a0, b0, acc);
        acc = mx_mfma<AF, WF>(a1, b1, acc);
    }
    if (wave) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < MXG_SK - 1; ++w) acc += part[w][lane];
    store_tile<OUT>(acc, bias, row0 + 4 * q, n, rows, N, Y);
}
template <int OUT, int AF = MXA_E4M3, int WF = MXA_E2M1>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                const float *__restrict__ bias, int M, int N, int K,
                                                                typename PkOut<OUT>::T *__restrict__ Y) {
    mx_gemm_splitk_tile<OUT, AF, WF>(Ac, As, Wc, Ws, bias, blockIdx.y * 16, M, blockIdx.x * 16, N, K, Y);
}

// Many rows: a wave holds a 32 x 32 tile of Y as 2 x 2 MFMA tiles, so each fragment it loads feeds two MFMAs, and the four
// waves of a workgroup cover 64 x 64; the fragments two waves share come to the second of them from the cache.
template <int OUT, int AF, int WF>
__device__ __forceinline__ void mx_gemm_tiled_tile(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                   const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                   const float *__restrict__ bias, int row0, int rows, int col0, int N, int K,
                                                   typename PkOut<OUT>::T *__restrict__ Y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m0 = row0 + (wave >> 1) * 32, n0 = col0 + (wave & 1) * 32, q = lane >> 4;
    v4f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < steps; ++s) {
        FragA<AF> a[2];
        FragB<WF> b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = load_a<AF>(Ac, As, m0 + 16 * i + (lane & 15), rows, s, q, bpr);
            b[i] = load_b<WF>(Wc, Ws, n0 + 16 * i + (lane & 15), N, 4 * s + q, bpr);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mx_mfma<AF, WF>(a[i], b[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) store_tile<OUT>(acc[i][j], bias, m0 + 16 * i + 4 * q, n0 + 16 * j + (lane & 15), rows, N, Y);
}
template <int OUT, int AF = MXA_E4M3, int WF = MXA_E2M1>
__global__ __launch_bounds__(256) void k_mx_gemm_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                       const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                       const float *__restrict__ bias, int M, int N, int K,
                                                       typename PkOut<OUT>::T *__restrict__ Y) {
    mx_gemm_tiled_tile<OUT, AF, WF>(Ac, As, Wc, Ws, bias, blockIdx.y * 64, M, blockIdx.x * 64, N, K, Y);
}

// ---------------------------------------------------------------- the fused gate/up product of a gated MLP
// slk_mx_gemm_glu: A against a layer of 2 N rows, gate and up, and instead of Y (M, 2 N) the next layer's activations:
// h = mx_glu(gate + bias, up + bias) (mxglu.h), quantized per (row, block of 32 hidden columns) to A's own format exactly as
// the plain quantizer of mx.hip would have done it -- mxq_encode (mxquant.h), which both call, then mxa_store and the
// scale byte.  Every accumulator keeps the order over K of the kernels above (the split-K
// form: wave w the steps w, w + SK, ..., two in flight, wave 0 adds in wave order; the tiled form: the steps in order), so the
// gate and up sums are slk_mx_gemm's float32 values bit for bit, and the codes are those of the three-step route
// slk_mx_gemm to float32, slk_mx_glu to float32, slk_mx_quantize_act*.
//
// A block of h must lie inside one workgroup.  The accumulator layout (lane l: column l & 15, rows 4 (l >> 4) + 0 .. 3) is
// not the packer's (contiguous elements a lane), so the float32 tile of h goes through LDS: rows of GLU_LD = 36 floats (the
// pad keeps a row on 16 bytes for the re-read in 16-byte pieces; a 32-lane group's dword stores fall on 32 distinct banks:
// lanes of q = 0 on 0 .. 15, of q = 1 on 4 * 36 % 32 + 0 .. 15), re-read in the quantizer's lane shape, mxq_lanes lanes a block.
//
// The rotating form (slk_mx_gemm_glu_rot, _experts_rot): the down layer sits behind a block Hadamard rotation of at most 32
// hidden columns, which then lies inside the staged block of its row.  Between the re-read and the encoder a lane runs steps
// 1 to 3 of slk_hadamard_rows' contract on its EPL elements -- v = s h, the butterflies (hadamard.h: strides below EPL in
// registers, the rest lane distances 1 and 2 inside a quad, DPP), y = v c -- in k_hadamard_quantize's operations, so the codes
// are those of slk_mx_rotate_quantize_act* on the float32 h.  ROT is a template argument: the plain form compiles as before.
constexpr int GLU_LD = 36;
struct GluRot {
    const float *signs;  // N of +-1 on 16 bytes, or null: all +1
    int lb;              // the block is 2^lb, 1 .. 5
    float c;             // 1 / sqrt(block), rounded once from double
};

// One MFMA tile of gate and up sums -> h in the staged tile: rows r0 .. r0 + 3, column c.
__device__ __forceinline__ void glu_stage(float *__restrict__ tile, v4f g, v4f u, const float *__restrict__ bias, int gate, int up, int r0,
                                          int c, const GluParams p) {
    const float bg = bias ? bias[gate] : 0.0f, bu = bias ? bias[up] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(r0 + r) * GLU_LD + c] = mx_glu(bias ? g[r] + bg : g[r], bias ? u[r] + bu : u[r], p);
}
// The staged ROWS x 32 tile -> codes and scale bytes of hidden block `blk` of rows row0 .. (below `rows`), by one wave:
// k_mx_quantize_act's lane shape around the same mxq_encode.  Returns whether a live block holds a NaN or an infinity.
// ROT: the block is rotated first; the signs of a lane's columns are the same in every row.  The stages between lanes run
// with every lane of the wave active, outside `staged` and `live`: a lane that stages nothing carries zeros through them.
template <int AF, int ROWS, bool ROT>
__device__ __forceinline__ bool glu_quantize_tile(const float *__restrict__ tile, int lane, int row0, int rows, int N, int blk, bool blk_live,
                                                  uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, const GluRot rot) {
    constexpr int LPB = mxq_lanes<AF>(), EPL = 32 / LPB, BYTES = EPL * mxa_bits<AF>() / 8;
    bool bad = false;
    float s[EPL];
    if constexpr (ROT) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) s[e] = 1.0f;
        if (rot.signs && blk_live) {  // (a block past the end has no signs; uniform over the wave)
            const v4f *sp = reinterpret_cast<const v4f *>(rot.signs + (size_t)32 * blk + (lane % LPB) * EPL);
#pragma unroll
            for (int p = 0; p < EPL / 4; ++p) {
                const v4f four = sp[p];
#pragma unroll
                for (int e = 0; e < 4; ++e) s[4 * p + e] = four[e];
            }
        }
    }
#pragma unroll
    for (int i0 = 0; i0 < ROWS * LPB; i0 += 64) {  // (every lane of a block takes the round: 64 is a multiple of LPB)
        const int i = i0 + lane, r = i / LPB, piece = i % LPB, m = row0 + r;
        const bool staged = r < ROWS, live = staged && blk_live && m < rows;
        float x[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) x[e] = staged ? tile[r * GLU_LD + piece * EPL + e] : 0.0f;
        if constexpr (ROT) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) x[e] = s[e] * x[e];
            hd_quad_butterfly(x, rot.lb, lane);
#pragma unroll
            for (int e = 0; e < EPL; ++e) x[e] = x[e] * rot.c;
        }
        unsigned eb, w[BYTES / 4];
        const int top = mxq_encode<AF>(x, eb, w);
        bad |= live && top >= 0x7f800000;
        if (live) {
            mxa_store<AF, EPL>(Hc + (size_t)m * mxa_byte_of<AF>((size_t)N) + (size_t)blk * (4 * mxa_bits<AF>()) + piece * BYTES, w);
            if (piece == 0) Hs[(size_t)m * (N / 32) + blk] = (uint8_t)eb;
        }
    }
    return bad;
}

// Few rows: a workgroup is 16 rows x one block of 32 hidden columns -- four accumulators a wave, gate and up times two
// 16-column tiles -- and each A fragment meets four B fragments.  (row0 / rows as in mx_gemm_splitk_tile; blk the block.)
template <int AF, int WF, bool ROT = false>
__device__ __forceinline__ void mx_gemm_glu_splitk_tile(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                        const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                        const float *__restrict__ bias, int row0, int rows, int blk, int N, int K,
                                                        const GluParams p, uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs,
                                                        int *__restrict__ flag, const GluRot rot = GluRot()) {
    __shared__ v4f part[MXG_SK - 1][4][64];
    __shared__ float tile[16 * GLU_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m = row0 + (lane & 15), q = lane >> 4;
    int wrow[4];  // the layer's rows of this lane's column: gate and up of tile 0, gate and up of tile 1
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = 32 * blk + 16 * t + (lane & 15);  // (N % 32 == 0: every hidden column of the block exists)
        wrow[2 * t] = glu_gate_of(j, N, p.interleaved), wrow[2 * t + 1] = glu_up_of(j, N, p.interleaved);
    }
    v4f acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = wave; s < steps; s += 2 * MXG_SK) {  // two steps' loads in flight; a step past the end loads zeros
        const FragA<AF> a0 = load_a<AF>(Ac, As, m, rows, s, q, bpr), a1 = load_a<AF>(Ac, As, m, rows, s + MXG_SK, q, bpr);
        FragB<WF> b0[4], b1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            b0[c] = load_b<WF>(Wc, Ws, wrow[c], 2 * N, 4 * s + q, bpr);
            b1[c] = load_b<WF>(Wc, Ws, wrow[c], 2 * N, 4 * (s + MXG_SK) + q, bpr);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = mx_mfma<AF, WF>(a0, b0[c], acc[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = mx_mfma<AF, WF>(a1, b1[c], acc[c]);
    }
    if (wave) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[wave - 1][c][lane] = acc[c];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int w = 0; w < MXG_SK - 1; ++w) acc[c] += part[w][c][lane];
#pragma unroll
        for (int t = 0; t < 2; ++t) glu_stage(tile, acc[2 * t], acc[2 * t + 1], bias, wrow[2 * t], wrow[2 * t + 1], 4 * q, 16 * t + (lane & 15), p);
    }
    __syncthreads();
    if (wave == 0 && glu_quantize_tile<AF, 16, ROT>(tile, lane, row0, rows, N, blk, true, Hc, Hs, rot)) *flag = 1;
}
template <int AF, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_glu_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                    const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                    const float *__restrict__ bias, int M, int N, int K, const GluParams p,
                                                                    uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag) {
    mx_gemm_glu_splitk_tile<AF, WF>(Ac, As, Wc, Ws, bias, blockIdx.y * 16, M, blockIdx.x, N, K, p, Hc, Hs, flag);
}
template <int AF, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_glu_rot_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                        const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                        const float *__restrict__ bias, int M, int N, int K, const GluParams p,
                                                                        uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag,
                                                                        const GluRot rot) {
    mx_gemm_glu_splitk_tile<AF, WF, true>(Ac, As, Wc, Ws, bias, blockIdx.y * 16, M, blockIdx.x, N, K, p, Hc, Hs, flag, rot);
}

// Many rows: a wave keeps its 32 x 32 tile of h, one block a row, as eight accumulators -- gate and up times 2 x 2 -- and the
// four waves of a workgroup cover 64 x 64.  N % 32 == 0, so a wave's block is whole or past the end; a wave past the end
// loads zeros, stores nothing and keeps the barrier.
template <int AF, int WF, bool ROT = false>
__device__ __forceinline__ void mx_gemm_glu_tiled_tile(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                       const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                       const float *__restrict__ bias, int row0, int rows, int col0, int N, int K,
                                                       const GluParams p, uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs,
                                                       int *__restrict__ flag, const GluRot rot = GluRot()) {
    __shared__ float tile[4][32 * GLU_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m0 = row0 + (wave >> 1) * 32, n0 = col0 + (wave & 1) * 32, q = lane >> 4;
    const bool blk_live = n0 < N;
    int wrow[2][2];  // [gate, up][column tile]: the layer's row, or 2 N (no row: zeros) past the end
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + 16 * j + (lane & 15);
        wrow[0][j] = blk_live ? glu_gate_of(col, N, p.interleaved) : 2 * N;
        wrow[1][j] = blk_live ? glu_up_of(col, N, p.interleaved) : 2 * N;
    }
    v4f acc[2][2][2];  // [gate, up][row tile][column tile]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[h][i][j] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < steps; ++s) {
        FragA<AF> a[2];
        FragB<WF> b[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = load_a<AF>(Ac, As, m0 + 16 * i + (lane & 15), rows, s, q, bpr);
#pragma unroll
            for (int h = 0; h < 2; ++h) b[h][i] = load_b<WF>(Wc, Ws, wrow[h][i], 2 * N, 4 * s + q, bpr);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[h][i][j] = mx_mfma<AF, WF>(a[i], b[h][j], acc[h][i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            glu_stage(tile[wave], acc[0][i][j], acc[1][i][j], blk_live ? bias : nullptr, wrow[0][j], wrow[1][j], 16 * i + 4 * q, 16 * j + (lane & 15), p);
    __syncthreads();
    if (glu_quantize_tile<AF, 32, ROT>(tile[wave], lane, m0, rows, N, n0 / 32, blk_live, Hc, Hs, rot)) *flag = 1;
}
template <int AF, int WF>
__global__ __launch_bounds__(256) void k_mx_gemm_glu_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                           const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                           const float *__restrict__ bias, int M, int N, int K, const GluParams p,
                                                           uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag) {
    mx_gemm_glu_tiled_tile<AF, WF>(Ac, As, Wc, Ws, bias, blockIdx.y * 64, M, blockIdx.x * 64, N, K, p, Hc, Hs, flag);
}
template <int AF, int WF>
__global__ __launch_bounds__(256) void k_mx_gemm_glu_rot_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                               const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                               const float *__restrict__ bias, int M, int N, int K, const GluParams p,
                                                               uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag,
                                                               const GluRot rot) {
    mx_gemm_glu_tiled_tile<AF, WF, true>(Ac, As, Wc, Ws, bias, blockIdx.y * 64, M, blockIdx.x * 64, N, K, p, Hc, Hs, flag, rot);
}

// ---------------------------------------------------------------- a mixture-of-experts layer in one call
// slk_mx_gemm_experts: the rows of A are sorted by expert and `offsets` (device memory, E + 1 ints) says where each expert's
// rows begin.  The host never reads it.  k_mx_expert_tiles, one workgroup, checks the offsets and turns them into two
// tables of row tiles in the workspace: 16-row tiles of the experts with 1 .. MXG_SPLIT_MAX_M rows, for the split-K form, and
// 64-row tiles of the others, for the 2 x 2 tiled form -- the form mx_gemm would choose for that expert's rows alone, so the
// result is that call's bit for bit.  The two products are launched over host-computable upper bounds of the tile counts;
// a workgroup at or past its table's count returns at once.  Invalid offsets raise the flag and leave both counts 0: no
// address is ever made from an offset that was not checked.
//
// The workspace, as ints: [0] the number of 16-row tiles, [1] of 64-row tiles, [2], [3] unused; from [4] the 16-row table,
// M / 16 + E entries of (expert, first row, row bound); after it the 64-row table, M / 64 + E entries of the same.
// An expert of m rows has at most m / 16 + 1 (m / 64 + 1) tiles, so the tables cannot overflow when the offsets are valid.
constexpr int MXE_MAX_EXPERTS = SLK_MX_MAX_EXPERTS;
constexpr int MXE_HEAD = 4;
static inline size_t mxe_cap16(int E, int M) { return (size_t)M / 16 + E; }
static inline size_t mxe_cap64(int E, int M) { return (size_t)M / 64 + E; }

__global__ __launch_bounds__(256) void k_mx_expert_tiles(const int *__restrict__ offsets, int E, int M, int *__restrict__ ws,
                                                         int cap16, int *__restrict__ flag) {
    __shared__ int scan16[256], scan64[256];
    __shared__ int base[2];
    const int t = threadIdx.x;
    // 1. the rule: offsets[0] == 0, non-decreasing, offsets[E] == M (so every offset lies in 0 .. M)
    int bad = 0;
    for (int e = t; e < E; e += 256) {
        const int o0 = offsets[e], o1 = offsets[e + 1];
        bad |= o1 < o0 || (e == 0 && o0 != 0) || (e == E - 1 && o1 != M);
    }
    bad = __syncthreads_or(bad);
    if (t == 0) flag[0] = bad ? 1 : 0;
    if (bad) {
        if (t < 2) ws[t] = 0;
        return;
    }
    // 2. the tables, in expert order: 256 experts a round, each thread its expert's tiles behind an exclusive scan
    if (t < 2) base[t] = 0;
    int *const t16 = ws + MXE_HEAD, *const t64 = ws + MXE_HEAD + 3 * (size_t)cap16;
    for (int e0 = 0; e0 < E; e0 += 256) {
        const int e = e0 + t;
        const int o0 = e < E ? offsets[e] : 0, o1 = e < E ? offsets[e + 1] : 0, m = o1 - o0;
        const int n16 = m >= 1 && m <= MXG_SPLIT_MAX_M ? (m + 15) / 16 : 0, n64 = m > MXG_SPLIT_MAX_M ? (m + 63) / 64 : 0;
        scan16[t] = n16, scan64[t] = n64;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // (inclusive, Hillis-Steele)
            const int a = t >= d ? scan16[t - d] : 0, b = t >= d ? scan64[t - d] : 0;
            __syncthreads();
            scan16[t] += a, scan64[t] += b;
            __syncthreads();
        }
        int at16 = base[0] + scan16[t] - n16, at64 = base[1] + scan64[t] - n64;
        for (int i = 0; i < n16; ++i, ++at16) t16[3 * at16] = e, t16[3 * at16 + 1] = o0 + 16 * i, t16[3 * at16 + 2] = o1;
        for (int i = 0; i < n64; ++i, ++at64) t64[3 * at64] = e, t64[3 * at64 + 1] = o0 + 64 * i, t64[3 * at64 + 2] = o1;
        __syncthreads();
        if (t == 255) base[0] += scan16[255], base[1] += scan64[255];
        __syncthreads();
    }
    if (t < 2) ws[t] = base[t];
}

// One row tile of one expert is an ExpertTile (mxexperts.h): the dense kernels' bodies on that expert's layer, bias and
// row bound.
template <int OUT, int AF, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_experts_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                        const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                        const float *__restrict__ bias, const int *__restrict__ count,
                                                                        const int *__restrict__ table, int N, int K,
                                                                        typename PkOut<OUT>::T *__restrict__ Y) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, N, K);
    mx_gemm_splitk_tile<OUT, AF, WF>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 16, N, K, Y);
}
template <int OUT, int AF, int WF>
__global__ __launch_bounds__(256) void k_mx_gemm_experts_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                               const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                               const float *__restrict__ bias, const int *__restrict__ count,
                                                               const int *__restrict__ table, int N, int K,
                                                               typename PkOut<OUT>::T *__restrict__ Y) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, N, K);
    mx_gemm_tiled_tile<OUT, AF, WF>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 64, N, K, Y);
}

// ... and of the fused gate/up product: the layers have 2 N rows and the biases 2 N entries an expert
template <int AF, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_glu_experts_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                            const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                            const float *__restrict__ bias, const int *__restrict__ count,
                                                                            const int *__restrict__ table, int N, int K, const GluParams p,
                                                                            uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs,
                                                                            int *__restrict__ flag) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, 2 * N, K);
    mx_gemm_glu_splitk_tile<AF, WF>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x, N, K, p, Hc, Hs, flag);
}
template <int AF, int WF>
__global__ __launch_bounds__(256) void k_mx_gemm_glu_experts_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                   const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                   const float *__restrict__ bias, const int *__restrict__ count,
                                                                   const int *__restrict__ table, int N, int K, const GluParams p,
                                                                   uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, 2 * N, K);
    mx_gemm_glu_tiled_tile<AF, WF>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 64, N, K, p, Hc, Hs, flag);
}
// ... and of its rotating form: one rotation of the N hidden columns, shared by all experts
template <int AF, int WF>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_glu_rot_experts_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                                const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                                const float *__restrict__ bias, const int *__restrict__ count,
                                                                                const int *__restrict__ table, int N, int K, const GluParams p,
                                                                                uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs,
                                                                                int *__restrict__ flag, const GluRot rot) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, 2 * N, K);
    mx_gemm_glu_splitk_tile<AF, WF, true>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x, N, K, p, Hc, Hs, flag, rot);
}
template <int AF, int WF>
__global__ __launch_bounds__(256) void k_mx_gemm_glu_rot_experts_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                       const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                       const float *__restrict__ bias, const int *__restrict__ count,
                                                                       const int *__restrict__ table, int N, int K, const GluParams p,
                                                                       uint8_t *__restrict__ Hc, uint8_t *__restrict__ Hs, int *__restrict__ flag,
                                                                       const GluRot rot) {
    if ((int)blockIdx.y >= *count) return;
    const ExpertTile<WF> x(table, Wc, Ws, bias, 2 * N, K);
    mx_gemm_glu_tiled_tile<AF, WF, true>(Ac, As, x.Wc, x.Ws, x.bias, x.row0, x.rows, blockIdx.x * 64, N, K, p, Hc, Hs, flag, rot);
}

}  // namespace slk

using namespace slk;

// ---------------------------------------------------------------- the entries
// f(MxPair<..>()) for an (a_fmt, w_fmt) that mx_check_pair has passed: the one place the two constants become template
// arguments, in the manner of with_dtype.  INDEX is the pair's place in an entry's names: none, _a4, _a6, _w6, _w6a6.
// (Every name SLK_RUN records is a literal: ProfScope may keep the pointer, and profiles/README.md reads them.)
template <int A, int W, int I>
struct MxPair {
    static constexpr int AF = A, WF = W, INDEX = I;
};
template <class F>
static int with_pair(int a_fmt, int w_fmt, F &&f) {
    if (w_fmt == SLK_MX_W_FP6) return a_fmt == SLK_MX_ACT_FP6 ? f(MxPair<MXA_E2M3, MXA_E2M3, 4>()) : f(MxPair<MXA_E4M3, MXA_E2M3, 3>());
    if (a_fmt == SLK_MX_ACT_FP4) return f(MxPair<MXA_E2M1, MXA_E2M1, 1>());
    if (a_fmt == SLK_MX_ACT_FP6) return f(MxPair<MXA_E2M3, MXA_E2M1, 2>());
    return f(MxPair<MXA_E4M3, MXA_E2M1, 0>());
}
static const char MX_W6_TAKES[] = "an MXFP6 layer takes MXFP8 (SLK_MX_ACT_FP8) or MXFP6 (SLK_MX_ACT_FP6) activations (a_fmt = %d)";
static int mx_check_pair(int a_fmt, int w_fmt) {
    SLK_REQUIRE(a_fmt == SLK_MX_ACT_FP8 || a_fmt == SLK_MX_ACT_FP4 || a_fmt == SLK_MX_ACT_FP6, "unknown a_fmt %d", a_fmt);
    SLK_REQUIRE(w_fmt == SLK_MX_W_FP4 || w_fmt == SLK_MX_W_FP6, "unknown w_fmt %d", w_fmt);
    SLK_REQUIRE(!(w_fmt == SLK_MX_W_FP6 && a_fmt == SLK_MX_ACT_FP4), MX_W6_TAKES, a_fmt);
    return SLK_OK;
}

// What every product requires of its operands; `out` is Y or h_codes, and `out_name` says which in the text.  (The lists
// below are functions because SLK_REQUIRE returns from the one it stands in: an entry returns what they return when it is not 0.)
static int mx_check_operands(const void *a_codes, const void *a_scales, const void *w_codes, const void *w_scales, const void *out,
                             const char *out_name, int M, int N, int K) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(a_codes && a_scales && w_codes && w_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(w_codes) && aligned16(out), "a_codes, w_codes and %s must be aligned to 16 bytes", out_name);
    return SLK_OK;
}
// ... what the fused gate/up products require on top, ahead of it: their rule for N has its own text and covers M ...
static int mx_check_gated(int M, int N, const void *h_scales, const int *flag, float alpha, float limit, float shift, int interleaved) {
    SLK_REQUIRE(M > 0 && N >= 32 && N % 32 == 0, "a block of h is 32 hidden columns: N must be a positive multiple of 32 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(N <= 0x3fffffff, "the layer has 2 N rows: N must be below 2^30 (N = %d)", N);
    SLK_REQUIRE(h_scales, "null pointer");
    SLK_REQUIRE(flag, "null flag");
    SLK_REQUIRE(limit > 0.0f, "limit must be above 0, +inf meaning no clamp (limit = %g)", (double)limit);
    SLK_REQUIRE(glu_finite(alpha) && glu_finite(shift), "alpha and shift must be finite (alpha = %g, shift = %g)", (double)alpha, (double)shift);
    SLK_REQUIRE(interleaved == 0 || interleaved == 1, "interleaved must be 0 or 1 (got %d)", interleaved);
    return SLK_OK;
}
// ... and the expert-grouped ones, behind it (M is positive by then; mxexperts.h: mxgemm_a16.hip's entry asks the same)
int slk::mx_check_experts(int E, int M, const int *offsets, const void *workspace, size_t ws_bytes) {
    SLK_REQUIRE(offsets, "null offsets");
    SLK_REQUIRE(workspace && (uintptr_t)workspace % sizeof(int) == 0, "the workspace must be non-null and aligned to 4 bytes");
    SLK_REQUIRE(ws_bytes >= slk_mx_experts_workspace_bytes(E, M), "the workspace is too small: %zu bytes, slk_mx_experts_workspace_bytes(%d, %d) = %zu",
                ws_bytes, E, M, slk_mx_experts_workspace_bytes(E, M));
    SLK_REQUIRE(mxe_cap64(E, M) <= 65535, "M / 64 + E is above the 65535 row tiles of one launch (M = %d, E = %d)", M, E);
    return SLK_OK;
}

// The prologue of both expert-grouped products: k_mx_expert_tiles on the stream, and what the two launches behind it need --
// host-computable upper bounds of the tile counts as grid rows, and the two tables (their counts are ws[0] and ws[1]).
int slk::mx_expert_prologue(const int *offsets, int E, int M, int *ws, int *flag, hipStream_t s, ExpertGrid &g) {
    const int cap16 = (int)mxe_cap16(E, M), cap64 = (int)mxe_cap64(E, M);
    // an expert of the split-K form has at most MXG_SPLIT_MAX_M / 16 tiles, so 4 E bounds the first launch as well
    g = {cap16 < 4 * E ? cap16 : 4 * E, cap64, ws + MXE_HEAD, ws + MXE_HEAD + 3 * (size_t)cap16};
    SLK_RUN("mx_expert_tiles", 0, 4.0 * (E + 1), s, (k_mx_expert_tiles<<<1, 256, 0, s>>>(offsets, E, M, ws, cap16, flag)));
    return SLK_OK;
}

// slk_mx_gemm (P::AF MXA_E4M3), _a4 (MXA_E2M1) and _a6 (MXA_E2M3) against an MXFP4 layer; _w6 (P::WF MXA_E2M3) against an MXFP6 one
template <class P>
static int mx_gemm(P, const char *name, const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                   const float *bias, int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    if (const int rc = mx_check_operands(a_codes, a_scales, w_codes, w_scales, out, "out", M, N, K)) return rc;
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    hipStream_t s = as_stream(stream);
    return with_dtype(out_dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T T;
        constexpr int OUT = decltype(t)::OUT;
        T *Y = static_cast<T *>(out);
        const double flops = 2.0 * M * N * K;
        const double bytes = ((double)M * mxa_block_bytes<P::AF>() + (double)N * mxa_block_bytes<P::WF>()) * K / 32.0 + (double)M * N * sizeof(T);
        if (M <= MXG_SPLIT_MAX_M) {
            const dim3 grid((N + 15) / 16, (M + 15) / 16);
            SLK_RUN(name, flops, bytes, s,
                    (k_mx_gemm_splitk<OUT, P::AF, P::WF><<<grid, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, Y)));
        } else {
            const dim3 grid((N + 63) / 64, (M + 63) / 64);
            SLK_RUN(name, flops, bytes, s,
                    (k_mx_gemm_tiled<OUT, P::AF, P::WF><<<grid, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, Y)));
        }
        return SLK_OK;
    });
}

// ... and the rotating ones, last: the block of the rotation and its signs (N % 32 == 0 by then, so the block divides N)
static int mx_check_rot(int block, const float *signs, GluRot &rot) {
    SLK_REQUIRE(block >= 2 && block <= 32 && (block & (block - 1)) == 0,
                "block must be a power of two in 2..32: a Hadamard block of h lies inside one MX block (got %d)", block);
    SLK_REQUIRE(aligned16(signs), "signs must be aligned to 16 bytes");
    int lb = 0;
    while ((1 << lb) < block) ++lb;
    rot = {signs, lb, (float)(1.0 / sqrt((double)block))};
    return SLK_OK;
}

// slk_mx_gemm_glu (ROT false; block and signs unused) and slk_mx_gemm_glu_rot
template <bool ROT>
static int mx_gemm_glu(const char *const (&names)[5], const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                       const float *bias, int M, int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift, int interleaved,
                       uint8_t *h_codes, uint8_t *h_scales, int *flag, int block, const float *signs, slk_stream_t stream) {
    if (const int rc = mx_check_gated(M, N, h_scales, flag, alpha, limit, shift, interleaved)) return rc;
    if (const int rc = mx_check_operands(a_codes, a_scales, w_codes, w_scales, h_codes, "h_codes", M, N, K)) return rc;
    if (const int rc = mx_check_pair(a_fmt, w_fmt)) return rc;
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    SLK_REQUIRE(N / 32 <= 0x7fffffff / 64, "N is above the column tiles of one launch (N = %d)", N);
    GluRot rot = {};
    if constexpr (ROT) {
        if (const int rc = mx_check_rot(block, signs, rot)) return rc;
    }
    hipStream_t s = as_stream(stream);
    const GluParams p = {alpha, limit, shift, interleaved};
    return with_pair(a_fmt, w_fmt, [&](auto pair) -> int {
        typedef decltype(pair) P;
        const double flops = 4.0 * M * N * K;
        const double bytes = ((double)M * mxa_block_bytes<P::AF>() + 2.0 * N * mxa_block_bytes<P::WF>()) * K / 32.0 + (double)M * mxa_block_bytes<P::AF>() * N / 32.0;
        if (M <= MXG_SPLIT_MAX_M) {
            const dim3 grid(N / 32, (M + 15) / 16);
            if constexpr (ROT)
                SLK_RUN(names[P::INDEX], flops, bytes, s,
                        (k_mx_gemm_glu_rot_splitk<P::AF, P::WF><<<grid, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, p, h_codes, h_scales, flag, rot)));
            else
                SLK_RUN(names[P::INDEX], flops, bytes, s,
                        (k_mx_gemm_glu_splitk<P::AF, P::WF><<<grid, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, p, h_codes, h_scales, flag)));
        } else {
            const dim3 grid((N + 63) / 64, (M + 63) / 64);
            if constexpr (ROT)
                SLK_RUN(names[P::INDEX], flops, bytes, s,
                        (k_mx_gemm_glu_rot_tiled<P::AF, P::WF><<<grid, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, p, h_codes, h_scales, flag, rot)));
            else
                SLK_RUN(names[P::INDEX], flops, bytes, s,
                        (k_mx_gemm_glu_tiled<P::AF, P::WF><<<grid, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, p, h_codes, h_scales, flag)));
        }
        return SLK_OK;
    });
}

// slk_mx_gemm_experts' three launches with the fused tile bodies; flag[0] is the prologue's, flag[1] the non-finite rule's.
// slk_mx_gemm_glu_experts (ROT false) and slk_mx_gemm_glu_experts_rot
template <bool ROT>
static int mx_gemm_glu_experts(const char *const (&names)[5], const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes,
                               const uint8_t *w_scales, const float *bias, const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt,
                               float alpha, float limit, float shift, int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag,
                               void *workspace, size_t ws_bytes, int block, const float *signs, slk_stream_t stream) {
    SLK_REQUIRE(E >= 1 && E <= MXE_MAX_EXPERTS, "E must be 1 .. %d experts (E = %d)", MXE_MAX_EXPERTS, E);
    if (const int rc = mx_check_gated(M, N, h_scales, flag, alpha, limit, shift, interleaved)) return rc;
    if (const int rc = mx_check_operands(a_codes, a_scales, w_codes, w_scales, h_codes, "h_codes", M, N, K)) return rc;
    if (const int rc = mx_check_pair(a_fmt, w_fmt)) return rc;
    if (const int rc = mx_check_experts(E, M, offsets, workspace, ws_bytes)) return rc;
    GluRot rot = {};
    if constexpr (ROT) {
        if (const int rc = mx_check_rot(block, signs, rot)) return rc;
    }
    hipStream_t s = as_stream(stream);
    int *ws = static_cast<int *>(workspace);
    const GluParams p = {alpha, limit, shift, interleaved};
    ExpertGrid g;
    if (const int rc = mx_expert_prologue(offsets, E, M, ws, flag, s, g)) return rc;
    return with_pair(a_fmt, w_fmt, [&](auto pair) -> int {
        typedef decltype(pair) P;
        const double flops = 4.0 * M * N * K;
        const double bytes = ((double)M * mxa_block_bytes<P::AF>() + 2.0 * E * N * mxa_block_bytes<P::WF>()) * K / 32.0 + (double)M * mxa_block_bytes<P::AF>() * N / 32.0;
        const dim3 grid16(N / 32, g.rows16), grid64((N + 63) / 64, g.rows64);
        if constexpr (ROT)
            SLK_RUN(names[P::INDEX], flops, bytes, s,
                    (k_mx_gemm_glu_rot_experts_splitk<P::AF, P::WF><<<grid16, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws, g.t16, N, K,
                                                                                                  p, h_codes, h_scales, flag + 1, rot)));
        else
            SLK_RUN(names[P::INDEX], flops, bytes, s,
                    (k_mx_gemm_glu_experts_splitk<P::AF, P::WF><<<grid16, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws, g.t16, N, K, p,
                                                                                              h_codes, h_scales, flag + 1)));
        if (M > MXG_SPLIT_MAX_M) {
            if constexpr (ROT)
                SLK_RUN(names[P::INDEX], 0, 0, s,
                        (k_mx_gemm_glu_rot_experts_tiled<P::AF, P::WF><<<grid64, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws + 1, g.t64, N, K,
                                                                                             p, h_codes, h_scales, flag + 1, rot)));
            else
                SLK_RUN(names[P::INDEX], 0, 0, s,
                        (k_mx_gemm_glu_experts_tiled<P::AF, P::WF><<<grid64, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws + 1, g.t64, N, K, p,
                                                                                         h_codes, h_scales, flag + 1)));
        }
        return SLK_OK;
    });
}

extern "C" {

int slk_mx_gemm_glu(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias, int M,
                    int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift, int interleaved, uint8_t *h_codes,
                    uint8_t *h_scales, int *flag, slk_stream_t stream) {
    static const char *const names[5] = {"mx_gemm_glu", "mx_gemm_glu_a4", "mx_gemm_glu_a6", "mx_gemm_glu_w6", "mx_gemm_glu_w6a6"};
    return mx_gemm_glu<false>(names, a_codes, a_scales, w_codes, w_scales, bias, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h_codes,
                              h_scales, flag, 0, nullptr, stream);
}

int slk_mx_gemm_glu_rot(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias, int M,
                        int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift, int interleaved, uint8_t *h_codes,
                        uint8_t *h_scales, int *flag, int block, const float *signs, slk_stream_t stream) {
    static const char *const names[5] = {"mx_gemm_glu_rot", "mx_gemm_glu_rot_a4", "mx_gemm_glu_rot_a6", "mx_gemm_glu_rot_w6", "mx_gemm_glu_rot_w6a6"};
    return mx_gemm_glu<true>(names, a_codes, a_scales, w_codes, w_scales, bias, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h_codes,
                             h_scales, flag, block, signs, stream);
}

int slk_mx_gemm_glu_experts(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                            const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift,
                            int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag, void *workspace, size_t ws_bytes,
                            slk_stream_t stream) {
    static const char *const names[5] = {"mx_gemm_glu_experts", "mx_gemm_glu_experts_a4", "mx_gemm_glu_experts_a6", "mx_gemm_glu_experts_w6",
                                         "mx_gemm_glu_experts_w6a6"};
    return mx_gemm_glu_experts<false>(names, a_codes, a_scales, w_codes, w_scales, bias, offsets, E, M, N, K, a_fmt, w_fmt, alpha, limit, shift,
                                      interleaved, h_codes, h_scales, flag, workspace, ws_bytes, 0, nullptr, stream);
}

int slk_mx_gemm_glu_experts_rot(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                                const float *bias, const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, float alpha, float limit,
                                float shift, int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag, void *workspace, size_t ws_bytes,
                                int block, const float *signs, slk_stream_t stream) {
    static const char *const names[5] = {"mx_gemm_glu_experts_rot", "mx_gemm_glu_experts_rot_a4", "mx_gemm_glu_experts_rot_a6",
                                         "mx_gemm_glu_experts_rot_w6", "mx_gemm_glu_experts_rot_w6a6"};
    return mx_gemm_glu_experts<true>(names, a_codes, a_scales, w_codes, w_scales, bias, offsets, E, M, N, K, a_fmt, w_fmt, alpha, limit, shift,
                                     interleaved, h_codes, h_scales, flag, workspace, ws_bytes, block, signs, stream);
}

size_t slk_mx_experts_workspace_bytes(int E, int M) {
    if (E < 1 || M < 1) return 0;
    return sizeof(int) * (MXE_HEAD + 3 * (mxe_cap16(E, M) + mxe_cap64(E, M)));
}

// The prologue, the split-K product over the 16-row table and, where an expert can have more than MXG_SPLIT_MAX_M rows at
// all, the tiled product over the 64-row table; in order on the stream
int slk_mx_gemm_experts(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                        const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, int out_dtype, void *out, int *flag,
                        void *workspace, size_t ws_bytes, slk_stream_t stream) {
    static const char *const names[5] = {"mx_gemm_experts", "mx_gemm_experts_a4", "mx_gemm_experts_a6", "mx_gemm_experts_w6", "mx_gemm_experts_w6a6"};
    SLK_REQUIRE(E >= 1 && E <= MXE_MAX_EXPERTS, "E must be 1 .. %d experts (E = %d)", MXE_MAX_EXPERTS, E);
    if (const int rc = mx_check_operands(a_codes, a_scales, w_codes, w_scales, out, "out", M, N, K)) return rc;
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    if (const int rc = mx_check_pair(a_fmt, w_fmt)) return rc;
    SLK_REQUIRE(flag, "null flag");
    if (const int rc = mx_check_experts(E, M, offsets, workspace, ws_bytes)) return rc;
    hipStream_t s = as_stream(stream);
    int *ws = static_cast<int *>(workspace);
    ExpertGrid g;
    if (const int rc = mx_expert_prologue(offsets, E, M, ws, flag, s, g)) return rc;
    return with_pair(a_fmt, w_fmt, [&](auto pair) -> int {
        typedef decltype(pair) P;
        return with_dtype(out_dtype, [&](auto t) -> int {
            typedef typename decltype(t)::T T;
            constexpr int OUT = decltype(t)::OUT;
            T *Y = static_cast<T *>(out);
            const double flops = 2.0 * M * N * K;
            const double bytes = ((double)M * mxa_block_bytes<P::AF>() + (double)E * N * mxa_block_bytes<P::WF>()) * K / 32.0 + (double)M * N * sizeof(T);
            const dim3 grid16((N + 15) / 16, g.rows16), grid64((N + 63) / 64, g.rows64);
            SLK_RUN(names[P::INDEX], flops, bytes, s,
                    (k_mx_gemm_experts_splitk<OUT, P::AF, P::WF><<<grid16, 64 * MXG_SK, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws, g.t16, N, K, Y)));
            if (M > MXG_SPLIT_MAX_M)
                SLK_RUN(names[P::INDEX], 0, 0, s,
                        (k_mx_gemm_experts_tiled<OUT, P::AF, P::WF><<<grid64, 256, 0, s>>>(a_codes, a_scales, w_codes, w_scales, bias, ws + 1, g.t64, N, K, Y)));
            return SLK_OK;
        });
    });
}

int slk_mx_gemm(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    return mx_gemm(MxPair<MXA_E4M3, MXA_E2M1, 0>(), "mx_gemm", a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out_dtype, out, stream);
}

int slk_mx_gemm_a4(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                   int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    return mx_gemm(MxPair<MXA_E2M1, MXA_E2M1, 1>(), "mx_gemm_a4", a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out_dtype, out, stream);
}

int slk_mx_gemm_a6(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                   int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    return mx_gemm(MxPair<MXA_E2M3, MXA_E2M1, 2>(), "mx_gemm_a6", a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out_dtype, out, stream);
}

int slk_mx_gemm_w6(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                   int M, int N, int K, int a_fmt, int out_dtype, void *out, slk_stream_t stream) {
    SLK_REQUIRE(a_fmt == SLK_MX_ACT_FP8 || a_fmt == SLK_MX_ACT_FP6, MX_W6_TAKES, a_fmt);  // (this entry's text for an unknown a_fmt as well)
    return with_pair(a_fmt, SLK_MX_W_FP6, [&](auto pair) -> int {
        const char *name = decltype(pair)::INDEX == 4 ? "mx_gemm_w6a6" : "mx_gemm_w6";
        return mx_gemm(pair, name, a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out_dtype, out, stream);
    });
}

}  // extern "C"
