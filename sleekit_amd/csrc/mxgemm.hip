// A linear layer computed from the packed MXFP4 form on the block-scaled MFMA (slk_mx_quantize_act, _act4, _act6,
// slk_mx_dequantize_act, _act6, slk_mx_gemm, _a4, _a6; the formats are pinned in include/sleekit_amd.h and INTEGRATION.md).
//
// Weights stay as slk_mx_pack left them: FP4 E2M1 codes, two a byte, and one E8M0 byte per block of 32 columns.
// Activations are quantized on the fly to MXFP8: E4M3 codes, one a byte, under the same kind of block scale -- or to
// MXFP4, in the weights' own form, or to MXFP6 (E2M3, 24 bytes a block).
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
// The stored forms feed the instruction with plain loads (16 bytes a piece; 16 + 8 for E2M3): no shuffle, no pre-swizzle, no LDS.
// D: lane l holds column l & 15, rows 4 (l >> 4) + 0 .. 3.
#include <type_traits>

#include "common.h"
#include "mxquant.h"

namespace slk {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

// 2^(b - 127) for a scale byte (0: the denormal 2^-127; 255 is E8M0's NaN)
__device__ __forceinline__ float mxg_e8m0(unsigned b) {
    return __uint_as_float(b == 0u ? 0x00400000u : (b == 255u ? 0x7fc00000u : b << 23));
}

// the float32 value of a code; 0x7f / 0xff are NaN
__device__ __forceinline__ float e4m3_value(unsigned c) {
    const unsigned e = (c >> 3) & 15u, m = c & 7u;
    const float mag = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
    const float v = (c & 0x7fu) == 0x7fu ? __uint_as_float(0x7fc00000u) : mag;
    return (c & 0x80u) ? -v : v;
}

template <class T>
__device__ __forceinline__ float act_f32(T x);
template <>
__device__ __forceinline__ float act_f32<float>(float x) { return x; }
template <>
__device__ __forceinline__ float act_f32<unsigned short>(unsigned short x) { return __uint_as_float((unsigned)x << 16); }
template <>
__device__ __forceinline__ float act_f32<_Float16>(_Float16 x) { return (float)x; }

// Four lanes a block, eight elements a lane: the block's largest |x| over a quad on DPP, the scale byte from lane 0 of
// the quad, eight codes from every lane -- 8 bytes of E4M3 (MXFP8), or one 32-bit word of E2M1 nibbles, the even k in the
// low ones, which is the weights' own layout (MXFP4).  A NaN or an infinity has the largest magnitude bits of its block,
// so the integer maximum finds it and raises the flag.
template <class T, int FMT>
__global__ __launch_bounds__(256) void k_mx_quantize_act(const T *__restrict__ X, size_t blocks, uint8_t *__restrict__ codes,
                                                         uint8_t *__restrict__ E, int *__restrict__ flag) {
    static_assert(FMT == MXA_E4M3 || FMT == MXA_E2M1, "E2M3 has its own shape: k_mx_quantize_act6");
    typedef T V __attribute__((ext_vector_type(8)));
    constexpr int BITS = FMT == MXA_E2M1 ? 4 : 8, PER = 32 / BITS, WORDS = 8 / PER;  // codes a word, words a lane
    typedef typename std::conditional<WORDS == 1, unsigned, u2v>::type C;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t units = 4 * blocks, rounds = (units + threads - 1) / threads;
    const V *src = reinterpret_cast<const V *>(X);
    C *dst = reinterpret_cast<C *>(codes);
    bool bad = false;
    for (size_t r = 0; r < rounds; ++r) {  // (every lane of a quad takes every round: units is a multiple of 4, and so is threads)
        const size_t i = r * threads + gid;
        const bool live = i < units;
        float x[8];
        if (live) {
            const V v = src[i];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = act_f32<T>(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = 0.0f;
        }
        int top = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) top = max(top, (int)(__float_as_uint(x[e]) & 0x7fffffffu));
        top = max(top, dpp_i<DPP_XOR1>(top));
        top = max(top, dpp_i<DPP_XOR2>(top));
        bad |= top >= 0x7f800000;
        const unsigned eb = mxa_scale_byte<FMT>(top);
        const float inv = mxa_inverse(eb);
        unsigned w[WORDS];
#pragma unroll
        for (int k = 0; k < WORDS; ++k) w[k] = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e / PER] |= mxa_code<FMT>(x[e], inv) << (BITS * (e % PER));
        if (live) {
            if constexpr (WORDS == 1) dst[i] = w[0];
            else dst[i] = (u2v){w[0], w[1]};
            if ((i & 3) == 0) E[i >> 2] = (uint8_t)eb;
        }
    }
    if (bad) *flag = 1;
}

// MXFP6 (E2M3): eight 6-bit codes are 6 bytes, which no lane can store as whole dwords at a 6-byte stride.  So LPB = 2
// lanes a block, sixteen elements a lane: the block's largest |x| over the pair on one DPP step, the scale byte from the
// even lane, and each lane's 16 codes as 96 bits of the row's little-endian bit stream -- three whole dwords at a 12-byte
// stride, every one of them aligned (a row is 24 bytes a block).  LPB = 1 (a lane a block: 32 elements, six dwords, no
// DPP) is the other shape that was measured; DESIGN.md section 20 has both.
constexpr int MXQ6_LPB = 2;
template <int WORDS>
struct alignas(4) CodeWords {
    unsigned w[WORDS];
};
typedef CodeWords<3> Codes12;
template <class T, int LPB>
__global__ __launch_bounds__(256) void k_mx_quantize_act6(const T *__restrict__ X, size_t blocks, uint8_t *__restrict__ codes,
                                                          uint8_t *__restrict__ E, int *__restrict__ flag) {
    static_assert(LPB == 1 || LPB == 2, "one or two lanes a block");
    constexpr int EPL = 32 / LPB, WORDS = 6 / LPB;                // elements and code words a lane
    constexpr int PER = 16 / (int)sizeof(T), PIECES = EPL / PER;  // elements a 16-byte piece, pieces a lane
    typedef T V __attribute__((ext_vector_type(PER)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t units = LPB * blocks, rounds = (units + threads - 1) / threads;
    const V *src = reinterpret_cast<const V *>(X);
    CodeWords<WORDS> *dst = reinterpret_cast<CodeWords<WORDS> *>(codes);
    bool bad = false;
    for (size_t r = 0; r < rounds; ++r) {  // (both lanes of a pair take every round: units is a multiple of LPB, and so is threads)
        const size_t i = r * threads + gid;
        const bool live = i < units;
        float x[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) x[e] = 0.0f;
        if (live) {
#pragma unroll
            for (int p = 0; p < PIECES; ++p) {
                const V v = src[PIECES * i + p];
#pragma unroll
                for (int e = 0; e < PER; ++e) x[p * PER + e] = act_f32<T>(v[e]);
            }
        }
        int top = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) top = max(top, (int)(__float_as_uint(x[e]) & 0x7fffffffu));
        if constexpr (LPB == 2) top = max(top, dpp_i<DPP_XOR1>(top));
        bad |= top >= 0x7f800000;
        const unsigned eb = mxa_scale_byte<MXA_E2M3>(top);
        CodeWords<WORDS> c;
        mxa_pack<MXA_E2M3>(x, mxa_inverse(eb), c.w);
        if (live) {
            dst[i] = c;
            if (i % LPB == 0) E[i / LPB] = (uint8_t)eb;
        }
    }
    if (bad) *flag = 1;
}

// the float32 value of an E2M3 code (bias 1, subnormals m / 8, no NaN)
__device__ __forceinline__ float e2m3_value(unsigned c) {
    const unsigned e = (c >> 3) & 3u, m = c & 7u;
    const float mag = e ? __uint_as_float(((e + 126u) << 23) | (m << 20)) : (float)m * 0.125f;
    return (c & 0x20u) ? -mag : mag;
}

// ... and back: a lane reads the 12 bytes of sixteen codes and stores sixteen values (64 or 32 bytes, 16 at a time).
template <int OUT>
__global__ __launch_bounds__(256) void k_mx_dequantize_act6(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E,
                                                            size_t blocks, typename PkOut<OUT>::T *__restrict__ out,
                                                            int *__restrict__ flag) {
    typedef typename PkOut<OUT>::T T;
    constexpr int PER = 16 / (int)sizeof(T), PIECES = 16 / PER;
    typedef T V __attribute__((ext_vector_type(PER)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const Codes12 *src = reinterpret_cast<const Codes12 *>(codes);
    V *dst = reinterpret_cast<V *>(out);
    const size_t units = 2 * blocks;
    bool bad = false;
    for (size_t i = gid; i < units; i += threads) {
        const Codes12 c = src[i];
        const unsigned b = E[i >> 1];
        bad |= b == 255u;
        const float sc = mxg_e8m0(b);
#pragma unroll
        for (int p = 0; p < PIECES; ++p) {
            V v;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const int at = 6 * (p * PER + e), word = at >> 5, shift = at & 31;
                unsigned code = c.w[word] >> shift;
                if (shift > 26) code |= c.w[word + 1] << (32 - shift);
                v[e] = PkOut<OUT>::cvt(e2m3_value(code & 0x3fu) * sc);
            }
            dst[PIECES * i + p] = v;
        }
    }
    if (bad && flag) *flag = 1;
}

// A unit is the 16 bytes a lane stores: 4 float32 values from 4 codes, or 8 16-bit values from 8 codes.
template <int OUT>
__global__ __launch_bounds__(256) void k_mx_dequantize_act(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E,
                                                           size_t blocks, typename PkOut<OUT>::T *__restrict__ out,
                                                           int *__restrict__ flag) {
    typedef typename PkOut<OUT>::T T;
    constexpr int EPL = 16 / (int)sizeof(T), UPB = 32 / EPL;  // elements a unit, units a block
    typedef T V __attribute__((ext_vector_type(EPL)));
    typedef typename std::conditional<EPL == 4, unsigned, u2v>::type C;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const C *src = reinterpret_cast<const C *>(codes);
    V *dst = reinterpret_cast<V *>(out);
    const size_t units = UPB * blocks;
    bool bad = false;
    for (size_t i = gid; i < units; i += threads) {
        const C c = src[i];
        const unsigned b = E[i / UPB];
        bad |= b == 255u;
        const float sc = mxg_e8m0(b);
        V v;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            unsigned word;
            if constexpr (EPL == 4) word = c;
            else word = c[e >> 2];
            v[e] = PkOut<OUT>::cvt(e4m3_value((word >> (8 * (e & 3))) & 0xffu) * sc);
        }
        dst[i] = v;
    }
    if (bad && flag) *flag = 1;
}

// ---------------------------------------------------------------- the product
// One lane's share of a 16 x 128 operand step (the map above), or zeros (and the scale 1) past the rows or past the
// blocks, so nothing outside a buffer of exactly its stated size is read.
struct FragA {
    v8i v;
    int sc;
};
struct FragB {
    v4i v;
    int sc;
};
__device__ __forceinline__ FragA load_a(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int step,
                                        int q, int bpr) {
    FragA f;
    f.sc = 127;
    v4i lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (row < rows) {
        const uint8_t *p = codes + 32 * ((size_t)row * bpr + 4 * step) + 16 * q;  // k = 128 step + 16 q
        if (4 * step + (q >> 1) < bpr) lo = *reinterpret_cast<const v4i *>(p);
        if (4 * step + 2 + (q >> 1) < bpr) hi = *reinterpret_cast<const v4i *>(p + 64);
        if (4 * step + q < bpr) f.sc = E[(size_t)row * bpr + 4 * step + q];
    }
    f.v = (v8i){lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return f;
}
__device__ __forceinline__ FragB load_b(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int kb,
                                        int bpr) {
    FragB f;
    f.v = (v4i){0, 0, 0, 0};
    f.sc = 127;
    if (row < rows && kb < bpr) {
        const size_t blk = (size_t)row * bpr + kb;
        f.v = *reinterpret_cast<const v4i *>(codes + 16 * blk);
        f.sc = E[blk];
    }
    return f;
}
// The A fragment of each activation format.  E2M1 activations are stored like the weights and map like them (held by
// the one-hot test of tests/test_gpu_mx_act4.py): lane i + 16 q carries the 32 consecutive k of block q of row i, one
// 16-byte load, under that block's scale.  E2M3 activations (tests/test_gpu_mx_act6.py) map the same way -- the 32
// consecutive k of block q in VGPRs 0-5, in the stored bit order -- so a lane's fragment is the 24 bytes of its block.
// A row starts on 8 bytes and a block every 24, so the fragment is three 8-byte loads: 24 bytes exactly, and the last
// block of the last row reads nothing past the buffer's 3 M K / 4 bytes, which a 16-byte pair of loads would.
struct FragA6 {
    int v[6];
    int sc;
};
__device__ __forceinline__ FragA6 load_a6(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row, int rows, int kb,
                                          int bpr) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    FragA6 f;
#pragma unroll
    for (int i = 0; i < 6; ++i) f.v[i] = 0;
    f.sc = 127;
    if (row < rows && kb < bpr) {
        const size_t blk = (size_t)row * bpr + kb;
        const v2i *p = reinterpret_cast<const v2i *>(codes + 24 * blk);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const v2i w = p[i];
            f.v[2 * i] = w.x, f.v[2 * i + 1] = w.y;
        }
        f.sc = E[blk];
    }
    return f;
}
template <int AF>
struct FragOfA {
    typedef FragA T;
};
template <>
struct FragOfA<MXA_E2M1> {
    typedef FragB T;
};
template <>
struct FragOfA<MXA_E2M3> {
    typedef FragA6 T;
};
template <int AF>
__device__ __forceinline__ typename FragOfA<AF>::T load_a_fmt(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, int row,
                                                              int rows, int step, int q, int bpr) {
    if constexpr (AF == MXA_E2M1) return load_b(codes, E, row, rows, 4 * step + q, bpr);
    else if constexpr (AF == MXA_E2M3) return load_a6(codes, E, row, rows, 4 * step + q, bpr);
    else return load_a(codes, E, row, rows, step, q, bpr);
}
// acc += A (E4M3, 16 x 128) B^T (E2M1, 16 x 128), each lane's block under its own scale
__device__ __forceinline__ v4f mx_mfma(const FragA a, const FragB b, v4f acc) {
    const v8i bv = {b.v.x, b.v.y, b.v.z, b.v.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.v, bv, acc, 0 /* A: E4M3 */, 4 /* B: E2M1 */, 0, a.sc, 0, b.sc);
}

// ... and with A in E2M1 as well (cbsz = 4): four VGPRs a side, the instruction at twice the E4M3 rate
__device__ __forceinline__ v4f mx_mfma(const FragB a, const FragB b, v4f acc) {
    const v8i av = {a.v.x, a.v.y, a.v.z, a.v.w, 0, 0, 0, 0};
    const v8i bv = {b.v.x, b.v.y, b.v.z, b.v.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 4 /* A: E2M1 */, 4 /* B: E2M1 */, 0, a.sc, 0, b.sc);
}

// ... and with A in E2M3 (cbsz = 2): six VGPRs of A, the instruction at the E2M1 rate
__device__ __forceinline__ v4f mx_mfma(const FragA6 a, const FragB b, v4f acc) {
    const v8i av = {a.v[0], a.v[1], a.v[2], a.v[3], a.v[4], a.v[5], 0, 0};
    const v8i bv = {b.v.x, b.v.y, b.v.z, b.v.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 2 /* A: E2M3 */, 4 /* B: E2M1 */, 0, a.sc, 0, b.sc);
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
constexpr int MXG_SK = 8;
constexpr int MXG_SPLIT_MAX_M = 64;
template <int OUT, int AF = MXA_E4M3>
__global__ __launch_bounds__(64 * MXG_SK) void k_mx_gemm_splitk(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                                const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                                const float *__restrict__ bias, int M, int N, int K,
                                                                typename PkOut<OUT>::T *__restrict__ Y) {
    __shared__ v4f part[MXG_SK - 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m = blockIdx.y * 16 + (lane & 15), n = blockIdx.x * 16 + (lane & 15), q = lane >> 4;
    v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = wave; s < steps; s += 2 * MXG_SK) {  // two steps' loads in flight; a step past the end loads zeros
        const typename FragOfA<AF>::T a0 = load_a_fmt<AF>(Ac, As, m, M, s, q, bpr), a1 = load_a_fmt<AF>(Ac, As, m, M, s + MXG_SK, q, bpr);
        const FragB b0 = load_b(Wc, Ws, n, N, 4 * s + q, bpr), b1 = load_b(Wc, Ws, n, N, 4 * (s + MXG_SK) + q, bpr);
        acc = mx_mfma(a0, b0, acc);
        acc = mx_mfma(a1, b1, acc);
    }
    if (wave) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < MXG_SK - 1; ++w) acc += part[w][lane];
    store_tile<OUT>(acc, bias, blockIdx.y * 16 + 4 * q, n, M, N, Y);
}

// Many rows: a wave holds a 32 x 32 tile of Y as 2 x 2 MFMA tiles, so each fragment it loads feeds two MFMAs, and the four
// waves of a workgroup cover 64 x 64; the fragments two waves share come to the second of them from the cache.
template <int OUT, int AF = MXA_E4M3>
__global__ __launch_bounds__(256) void k_mx_gemm_tiled(const uint8_t *__restrict__ Ac, const uint8_t *__restrict__ As,
                                                       const uint8_t *__restrict__ Wc, const uint8_t *__restrict__ Ws,
                                                       const float *__restrict__ bias, int M, int N, int K,
                                                       typename PkOut<OUT>::T *__restrict__ Y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpr = K / 32, steps = (bpr + 3) / 4;
    const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.x * 64 + (wave & 1) * 32, q = lane >> 4;
    v4f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < steps; ++s) {
        typename FragOfA<AF>::T a[2];
        FragB b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = load_a_fmt<AF>(Ac, As, m0 + 16 * i + (lane & 15), M, s, q, bpr);
            b[i] = load_b(Wc, Ws, n0 + 16 * i + (lane & 15), N, 4 * s + q, bpr);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = mx_mfma(a[i], b[j], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) store_tile<OUT>(acc[i][j], bias, m0 + 16 * i + 4 * q, n0 + 16 * j + (lane & 15), M, N, Y);
}

static inline int mxg_grid(size_t units) {
    size_t b = (units + 255) / 256;
    if (b > 4096) b = 4096;  // 16 workgroups a CU, grid-stride beyond
    return b < 1 ? 1 : (int)b;
}

template <int OUT, int AF = MXA_E4M3>
static int mx_gemm_launch(const uint8_t *Ac, const uint8_t *As, const uint8_t *Wc, const uint8_t *Ws, const float *bias, int M, int N,
                          int K, void *out, hipStream_t s) {
    typedef typename PkOut<OUT>::T T;
    const double flops = 2.0 * M * N * K;
    const double bytes = (double)M * K * (1.0 + 4.0 * mxa_bits<AF>()) / 32.0 + (double)N * K * 17.0 / 32.0 + (double)M * N * sizeof(T);
    const char *name = AF == MXA_E2M1 ? "mx_gemm_a4" : AF == MXA_E2M3 ? "mx_gemm_a6" : "mx_gemm";
    if (M <= MXG_SPLIT_MAX_M) {
        const dim3 grid((N + 15) / 16, (M + 15) / 16);
        SLK_RUN(name, flops, bytes, s,
                (k_mx_gemm_splitk<OUT, AF><<<grid, 64 * MXG_SK, 0, s>>>(Ac, As, Wc, Ws, bias, M, N, K, static_cast<T *>(out))));
    } else {
        const dim3 grid((N + 63) / 64, (M + 63) / 64);
        SLK_RUN(name, flops, bytes, s, (k_mx_gemm_tiled<OUT, AF><<<grid, 256, 0, s>>>(Ac, As, Wc, Ws, bias, M, N, K, static_cast<T *>(out))));
    }
    return SLK_OK;
}

}  // namespace slk

using namespace slk;

static inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }
static inline bool known_dtype(int d) { return d == SLK_DTYPE_F32 || d == SLK_DTYPE_BF16 || d == SLK_DTYPE_F16; }

// slk_mx_quantize_act (FMT MXA_E4M3) and slk_mx_quantize_act4 (MXA_E2M1)
template <int FMT>
static int mx_quantize_act(const char *name, const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag,
                           slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (M = %d, K = %d)", M, K);
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(X && a_codes && a_scales && flag, "null pointer");
    SLK_REQUIRE(aligned16(X) && aligned16(a_codes), "X and a_codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)M * (K / 32);
    zero_async(flag, sizeof(int), s);
    const double bytes = ((FMT == MXA_E2M1 ? 17.0 : 33.0) + 32.0 * (x_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0)) * blocks;
    const int grid = mxg_grid(4 * blocks);
    if (x_dtype == SLK_DTYPE_BF16)
        SLK_RUN(name, 0, bytes, s,
                (k_mx_quantize_act<unsigned short, FMT><<<grid, 256, 0, s>>>(static_cast<const unsigned short *>(X), blocks, a_codes, a_scales, flag)));
    else if (x_dtype == SLK_DTYPE_F16)
        SLK_RUN(name, 0, bytes, s,
                (k_mx_quantize_act<_Float16, FMT><<<grid, 256, 0, s>>>(static_cast<const _Float16 *>(X), blocks, a_codes, a_scales, flag)));
    else
        SLK_RUN(name, 0, bytes, s,
                (k_mx_quantize_act<float, FMT><<<grid, 256, 0, s>>>(static_cast<const float *>(X), blocks, a_codes, a_scales, flag)));
    return SLK_OK;
}

extern "C" {

int slk_mx_quantize_act(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_quantize_act<MXA_E4M3>("mx_quantize_act", X, x_dtype, M, K, a_codes, a_scales, flag, stream);
}

int slk_mx_quantize_act4(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_quantize_act<MXA_E2M1>("mx_quantize_act4", X, x_dtype, M, K, a_codes, a_scales, flag, stream);
}

int slk_mx_dequantize_act(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                          slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (M = %d, K = %d)", M, K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(a_codes && a_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(out), "a_codes and out must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)M * (K / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (33.0 + 32.0 * (out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0)) * blocks;
    if (out_dtype == SLK_DTYPE_BF16)
        SLK_RUN("mx_dequantize_act", 0, bytes, s,
                k_mx_dequantize_act<PK_BF16><<<mxg_grid(4 * blocks), 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<unsigned short *>(out), flag));
    else if (out_dtype == SLK_DTYPE_F16)
        SLK_RUN("mx_dequantize_act", 0, bytes, s,
                k_mx_dequantize_act<PK_F16><<<mxg_grid(4 * blocks), 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<_Float16 *>(out), flag));
    else
        SLK_RUN("mx_dequantize_act", 0, bytes, s,
                k_mx_dequantize_act<PK_F32><<<mxg_grid(8 * blocks), 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<float *>(out), flag));
    return SLK_OK;
}

int slk_mx_gemm(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(a_codes && a_scales && w_codes && w_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(w_codes) && aligned16(out), "a_codes, w_codes and out must be aligned to 16 bytes");
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    hipStream_t s = as_stream(stream);
    if (out_dtype == SLK_DTYPE_BF16) return mx_gemm_launch<PK_BF16>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    if (out_dtype == SLK_DTYPE_F16) return mx_gemm_launch<PK_F16>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    return mx_gemm_launch<PK_F32>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
}

int slk_mx_gemm_a4(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                   int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(a_codes && a_scales && w_codes && w_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(w_codes) && aligned16(out), "a_codes, w_codes and out must be aligned to 16 bytes");
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    hipStream_t s = as_stream(stream);
    if (out_dtype == SLK_DTYPE_BF16) return mx_gemm_launch<PK_BF16, MXA_E2M1>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    if (out_dtype == SLK_DTYPE_F16) return mx_gemm_launch<PK_F16, MXA_E2M1>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    return mx_gemm_launch<PK_F32, MXA_E2M1>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
}

int slk_mx_quantize_act6(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (M = %d, K = %d)", M, K);
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(X && a_codes && a_scales && flag, "null pointer");
    SLK_REQUIRE(aligned16(X) && aligned16(a_codes), "X and a_codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)M * (K / 32);
    zero_async(flag, sizeof(int), s);
    const double bytes = (25.0 + 32.0 * (x_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0)) * blocks;
    const int grid = mxg_grid(MXQ6_LPB * blocks);
    if (x_dtype == SLK_DTYPE_BF16)
        SLK_RUN("mx_quantize_act6", 0, bytes, s,
                (k_mx_quantize_act6<unsigned short, MXQ6_LPB><<<grid, 256, 0, s>>>(static_cast<const unsigned short *>(X), blocks, a_codes, a_scales, flag)));
    else if (x_dtype == SLK_DTYPE_F16)
        SLK_RUN("mx_quantize_act6", 0, bytes, s,
                (k_mx_quantize_act6<_Float16, MXQ6_LPB><<<grid, 256, 0, s>>>(static_cast<const _Float16 *>(X), blocks, a_codes, a_scales, flag)));
    else
        SLK_RUN("mx_quantize_act6", 0, bytes, s,
                (k_mx_quantize_act6<float, MXQ6_LPB><<<grid, 256, 0, s>>>(static_cast<const float *>(X), blocks, a_codes, a_scales, flag)));
    return SLK_OK;
}

int slk_mx_dequantize_act6(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                           slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (M = %d, K = %d)", M, K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(a_codes && a_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(out), "a_codes and out must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)M * (K / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (25.0 + 32.0 * (out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0)) * blocks;
    const int grid = mxg_grid(2 * blocks);
    if (out_dtype == SLK_DTYPE_BF16)
        SLK_RUN("mx_dequantize_act6", 0, bytes, s,
                k_mx_dequantize_act6<PK_BF16><<<grid, 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<unsigned short *>(out), flag));
    else if (out_dtype == SLK_DTYPE_F16)
        SLK_RUN("mx_dequantize_act6", 0, bytes, s,
                k_mx_dequantize_act6<PK_F16><<<grid, 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<_Float16 *>(out), flag));
    else
        SLK_RUN("mx_dequantize_act6", 0, bytes, s,
                k_mx_dequantize_act6<PK_F32><<<grid, 256, 0, s>>>(a_codes, a_scales, blocks, static_cast<float *>(out), flag));
    return SLK_OK;
}

int slk_mx_gemm_a6(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales, const float *bias,
                   int M, int N, int K, int out_dtype, void *out, slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(a_codes && a_scales && w_codes && w_scales && out, "null pointer");
    SLK_REQUIRE(aligned16(a_codes) && aligned16(w_codes) && aligned16(out), "a_codes, w_codes and out must be aligned to 16 bytes");
    SLK_REQUIRE((M + 63) / 64 <= 65535, "M is above the 65535 row tiles of one launch (M = %d)", M);
    hipStream_t s = as_stream(stream);
    if (out_dtype == SLK_DTYPE_BF16) return mx_gemm_launch<PK_BF16, MXA_E2M3>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    if (out_dtype == SLK_DTYPE_F16) return mx_gemm_launch<PK_F16, MXA_E2M3>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
    return mx_gemm_launch<PK_F32, MXA_E2M3>(a_codes, a_scales, w_codes, w_scales, bias, M, N, K, out, s);
}

}  // extern "C"
