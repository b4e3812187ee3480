// The element encoders and the block scale of the MX activation formats (include/sleekit_amd.h): shared by the plain
// quantizers of mxgemm.hip and by the rotation's quantizing epilogue in hadamard.hip, so that both write the same bits.
#pragma once

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

// The formats of an activation block: the largest magnitude of its element grid divides the block's largest |x|.
enum { MXA_E4M3 = 0, MXA_E2M1 = 1, MXA_E2M3 = 2 };

template <int FMT>
__device__ __forceinline__ constexpr float mxa_largest() { return FMT == MXA_E2M1 ? 6.0f : FMT == MXA_E2M3 ? 7.5f : 448.0f; }
// bits a code (a block of 32 codes is four times as many bytes)
template <int FMT>
__host__ __device__ constexpr int mxa_bits() { return FMT == MXA_E2M1 ? 4 : FMT == MXA_E2M3 ? 6 : 8; }

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

}  // namespace slk
