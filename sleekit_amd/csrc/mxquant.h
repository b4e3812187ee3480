// What a kernel knows of an MX activation format (include/sleekit_amd.h): the element encoders and decoders, the block
// scale, and how one lane's codes are packed, stored and read back.  Shared by the plain quantizer and the de-quantizer
// of mxgemm.hip and by the rotation's quantizing epilogue in hadamard.hip, so that all of them write and read the same bits.
#pragma once

#include <type_traits>

#include "common.h"

namespace slk {

// ---------------------------------------------------------------- E4M3
// |y| as float32 bits -> the OCP E4M3 code of its nearest value, ties to even, clamped at 448 (0x7e).  From 2^-6 up
// the grid is the floats of three mantissa bits: add half of the last kept bit (less one, plus that bit: to even), cut
// 20 bits, and the exponent and mantissa fields are the code's after the bias moves from 127 to 7.  Below 2^-6 the
// grid is k 2^-9, k = 0 .. 8, and k = 8 is code 0x08, the first normal.
__device__ __forceinline__ unsigned e4m3_code(unsigned a) {
    const unsigned normal = min(((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3), 0x7eu);
    const unsigned sub = (unsigned)rintf(__uint_as_float(a) * 512.0f);
    return a >= 0x3c800000u ? normal : sub;
}

// the float32 value of a code; 0x7f / 0xff are NaN
__device__ __forceinline__ float e4m3_value(unsigned c) {
    const unsigned e = (c >> 3) & 15u, m = c & 7u;
    const float mag = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
    const float v = (c & 0x7fu) == 0x7fu ? __uint_as_float(0x7fc00000u) : mag;
    return (c & 0x80u) ? -v : v;
}

// ---------------------------------------------------------------- E2M1
// |y| as float32 bits -> the magnitude index 0 .. 7 of its nearest value on 0, .5, 1, 1.5, 2, 3, 4, 6, ties to the even
// index, clamped at 6.  From 1 up the grid is the floats of one mantissa bit: add half of the last kept bit (less one,
// plus that bit: to even), cut 22 bits, and the fields are the index after the bias moves from 127 to 1.  Below 1 the
// grid is k / 2, k = 0 .. 2, and k = 2 is index 2, the first normal.
__device__ __forceinline__ unsigned e2m1_code(unsigned a) {
    const unsigned normal = min(((a + 0x1fffffu + ((a >> 22) & 1u)) >> 22) - (126u << 1), 7u);
    const unsigned sub = (unsigned)rintf(__uint_as_float(a) * 2.0f);
    return a >= 0x3f800000u ? normal : sub;
}

// ---------------------------------------------------------------- E2M3
// |y| as float32 bits -> the OCP E2M3 code 0 .. 31 of its nearest value on 0, 0.125 .. 1.875 (steps of 0.125), 2 .. 3.75
// (0.25), 4 .. 7.5 (0.5), ties to the even code, clamped at 7.5 (0x1f).  From 1 up the grid is the floats of three mantissa
// bits: add half of the last kept bit (less one, plus that bit: to even), cut 20 bits, and the fields are the code after
// the bias moves from 127 to 1.  Below 1 the grid is k / 8, k = 0 .. 8, and k = 8 is code 0x08, the first normal.
__device__ __forceinline__ unsigned e2m3_code(unsigned a) {
    const unsigned normal = min(((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (126u << 3), 0x1fu);
    const unsigned sub = (unsigned)rintf(__uint_as_float(a) * 8.0f);
    return a >= 0x3f800000u ? normal : sub;
}

// the float32 value of a code (bias 1, subnormals m / 8, no NaN)
__device__ __forceinline__ float e2m3_value(unsigned c) {
    const unsigned e = (c >> 3) & 3u, m = c & 7u;
    const float mag = e ? __uint_as_float(((e + 126u) << 23) | (m << 20)) : (float)m * 0.125f;
    return (c & 0x20u) ? -mag : mag;
}

// ---------------------------------------------------------------- E8M0
// 2^(b - 127) for a scale byte (0: the denormal 2^-127; 255 is E8M0's NaN)
__device__ __forceinline__ float e8m0_value(unsigned b) {
    return __uint_as_float(b == 0u ? 0x00400000u : (b == 255u ? 0x7fc00000u : b << 23));
}

// The formats of an activation block: the largest magnitude of its element grid divides the block's largest |x|.
enum { MXA_E4M3 = 0, MXA_E2M1 = 1, MXA_E2M3 = 2 };

template <int FMT>
__device__ __forceinline__ constexpr float mxa_largest() { return FMT == MXA_E2M1 ? 6.0f : FMT == MXA_E2M3 ? 7.5f : 448.0f; }
// bits a code
template <int FMT>
__host__ __device__ constexpr int mxa_bits() { return FMT == MXA_E2M1 ? 4 : FMT == MXA_E2M3 ? 6 : 8; }
// bytes a block in memory: 32 codes and the scale byte
template <int FMT>
__host__ __device__ constexpr int mxa_block_bytes() { return 4 * mxa_bits<FMT>() + 1; }

// `top`: the largest magnitude bits of a block (an integer maximum: a NaN or an infinity is the largest).  The exponent
// field of the smallest power of two >= max(amax / LARGEST, 1e-16): 74 (the floor) .. 247 for 448, .. 253 for 6 and 7.5.
template <int FMT>
__device__ __forceinline__ unsigned mxa_scale_byte(int top) {
    const float b0 = fmaxf(__uint_as_float((unsigned)min(top, 0x7f7fffff)) / mxa_largest<FMT>(), 1.0e-16f);
    return ((__float_as_uint(b0) + 0x7fffffu) >> 23) & 0xffu;
}
// 1 / scale of a scale byte: x * inv is the exact quotient
__device__ __forceinline__ float mxa_inverse(unsigned eb) { return __uint_as_float((254u - eb) << 23); }

// The code of x * inv: sign and magnitude, a zero magnitude as 0 (never -0).
template <int FMT>
__device__ __forceinline__ unsigned mxa_code(float x, float inv) {
    const unsigned u = __float_as_uint(x * inv);
    if constexpr (FMT == MXA_E2M1) {
        const unsigned c = e2m1_code(u & 0x7fffffffu);
        return c ? c | ((u >> 28) & 0x8u) : 0u;
    } else if constexpr (FMT == MXA_E2M3) {
        const unsigned c = e2m3_code(u & 0x7fffffffu);
        return c ? c | ((u >> 26) & 0x20u) : 0u;
    } else {
        const unsigned c = e4m3_code(u & 0x7fffffffu);
        return c ? c | ((u >> 24) & 0x80u) : 0u;
    }
}

// ... and the value of a code (E2M1 is the weights' format: its decoder is mx.hip's)
template <int FMT>
__device__ __forceinline__ float mxa_value(unsigned c) {
    static_assert(FMT == MXA_E4M3 || FMT == MXA_E2M3, "no decoder for this format here");
    if constexpr (FMT == MXA_E2M3) return e2m3_value(c);
    else return e4m3_value(c);
}

// N codes of BITS bits as a little-endian bit stream in N BITS / 32 words: code e at bits BITS e .. BITS e + BITS - 1.
// For 4 and 8 bits a code lies inside one word; a 6-bit code may straddle two (every index here is a constant once
// the loop is unrolled, so a lane's words are built with shifts and ors alone).
template <int FMT, int N>
__device__ __forceinline__ void mxa_pack(const float (&x)[N], float inv, unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
    constexpr int BITS = mxa_bits<FMT>();
#pragma unroll
    for (int k = 0; k < N * BITS / 32; ++k) w[k] = 0u;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const unsigned c = mxa_code<FMT>(x[e], inv);
        const int at = BITS * e, word = at >> 5, shift = at & 31;
        w[word] |= c << shift;
        if (shift + BITS > 32) w[word + 1] |= c >> (32 - shift);
    }
}

// One lane's words in memory: one, two or four of them move as one aligned vector, three (16 E2M3 codes: 12 bytes of a
// row whose blocks are 24) as Codes12, three dwords, every one of them aligned.
struct alignas(4) Codes12 {
    unsigned w[3];
};

// The byte of a row-major matrix's bit stream at which element e starts, for an e whose codes before it are whole bytes
// (a multiple of 8 / gcd(BITS, 8): 1, 2 or 4 elements -- the gcd is BITS' lowest set bit).
template <int FMT>
__host__ __device__ constexpr size_t mxa_byte_of(size_t e) {
    constexpr int BITS = mxa_bits<FMT>(), G = BITS & -BITS;
    return e / (8 / G) * (BITS / G);
}

// mxa_pack's words to `at` in one store, and back in one load.
template <int FMT, int N>
__device__ __forceinline__ void mxa_store(uint8_t *at, const unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
    constexpr int WORDS = N * mxa_bits<FMT>() / 32;
    static_assert(N * mxa_bits<FMT>() % 32 == 0 && WORDS >= 1 && WORDS <= 4, "a lane stores one to four whole dwords");
    if constexpr (WORDS == 3) {
        *reinterpret_cast<Codes12 *>(at) = (Codes12){{w[0], w[1], w[2]}};
    } else {
        typedef unsigned V __attribute__((ext_vector_type(WORDS)));
        V v;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) v[k] = w[k];
        *reinterpret_cast<V *>(at) = v;
    }
}
template <int FMT, int N>
__device__ __forceinline__ void mxa_load(const uint8_t *at, unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
    constexpr int WORDS = N * mxa_bits<FMT>() / 32;
    static_assert(N * mxa_bits<FMT>() % 32 == 0 && WORDS >= 1 && WORDS <= 4, "a lane loads one to four whole dwords");
    typedef unsigned V __attribute__((ext_vector_type(WORDS)));
    typedef typename std::conditional<WORDS == 3, Codes12, V>::type C;
    const C c = *reinterpret_cast<const C *>(at);
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
        if constexpr (WORDS == 3) w[k] = c.w[k];
        else w[k] = c[k];
    }
}

// Code e of mxa_pack's words (e a constant once the caller's loop is unrolled).
template <int FMT, int WORDS>
__device__ __forceinline__ unsigned mxa_code_at(const unsigned (&w)[WORDS], int e) {
    constexpr int BITS = mxa_bits<FMT>();
    const int at = BITS * e, word = at >> 5, shift = at & 31;
    unsigned c = w[word] >> shift;
    if (shift + BITS > 32) c |= w[word + 1] << (32 - shift);
    return c & ((1u << BITS) - 1u);
}

}  // namespace slk
