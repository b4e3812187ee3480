// What a kernel knows of an MX element format (include/sleekit_amd.h), whichever side of the product it is on: the element
// encoders, roundings and decoders, the block scale, how one lane's codes are placed in words, stored and read back, how 32
// floats become a scale byte and those words (mxq_encode, the one block encoder of every quantizing kernel), and how
// a layer's table indices map to codes.  Shared by the converters and the scale search of mx.hip, the product's fragments in
// mxgemm.hip and the rotation's quantizing epilogue in hadamard.hip, so that all of them write and read the same bits.
// Two roundings live here: *_code sends a tie to the even code and is the activations' rule (quantized on the fly, as the
// OCP text does it); *_round sends a tie upward and is the weights' rule (np.digitize over the codebook's midpoints).
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

// The codebook's midpoints send a tie upward (np.digitize counts the limits <= x): |x| on a limit rounds away from
// zero for x > 0 and towards zero for x < 0.  On the bits of |x| as an integer that is one rule for both signs: a
// negative x is moved one float down first (|x| > L  <=>  the float below |x| is >= L; -0.0 becomes -1, below every
// limit).  `a`: those bits, `neg` (0 or 1) already taken off.  Returns the bits of the magnitude |x| rounds to:
// from 1 up the grid is the floats of one mantissa bit, so adding half of that bit and cutting the rest rounds with ties
// up (6 is the top); below 1 it is 0, 0.5, 1 with the limits 0.25 and 0.75.
__device__ __forceinline__ unsigned e2m1_round(int a) {
    a = min(a, 0x40c00000);  // 6
    const unsigned high = ((unsigned)a + 0x00200000u) & 0xffc00000u;
    const unsigned low = a >= 0x3f400000 ? 0x3f800000u : (a >= 0x3e800000 ? 0x3f000000u : 0u);
    return a >= 0x3f800000 ? high : low;
}
// the float32 bits of magnitude m: 0, 0.5, then (1 + (m & 1) / 2) 2^((m >> 1) - 1)
__device__ __forceinline__ unsigned e2m1_bits(int m) {
    const unsigned normal = ((126u + (unsigned)(m >> 1)) << 23) | ((unsigned)(m & 1) << 22);
    return m >= 2 ? normal : (m ? 0x3f000000u : 0u);
}
// the value of code c (sign << 3 | m) times `sc`; code 0x8 reads as +0
__device__ __forceinline__ float e2m1_value(unsigned c, float sc) {
    const int m = (int)(c & 7u);
    const unsigned sign = m ? (c & 8u) << 28 : 0u;
    return __uint_as_float(e2m1_bits(m) | sign) * sc;
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

// e2m1_round's rule on the 32 magnitudes of E2M3: `a` as there, the bits of the magnitude |x| rounds to with a tie upward.
// The grid is the floats of 3 mantissa bits from 1 up (spacing 2^(e - 3) in binade e) and k / 8 below, which in the binades
// 1/2, 1/4 and 1/8 is the floats of 2, 1 and 0 mantissa bits, and in the binade of 1/16 the one limit 1/16 = its lowest
// float, above which everything goes to 1/8: 24 bits cut, the exponent's own lowest bit among them (123 + 1 = 124 is even).
// So one rule serves all binades -- add half of the last kept bit and cut `cut` = 20 .. 24 bits -- and integer
// arithmetic alone decides every limit; below 1/16 (-1, a negative zero, included) the answer is 0.  7.5 is the top.
__device__ __forceinline__ unsigned e2m3_round(int a) {
    a = min(a, 0x40f00000);  // 7.5
    const int cut = min(max(147 - (a >> 23), 20), 24);
    const unsigned r = (((unsigned)a + (1u << (cut - 1))) >> cut) << cut;
    return a >= 0x3d800000 ? r : 0u;
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

// The formats of a block's elements: the largest magnitude of the element grid divides the block's largest |x|.
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

// ... the value of a code (its low bits; the rest of c is ignored) ...
template <int FMT>
__device__ __forceinline__ float mxa_value(unsigned c) {
    if constexpr (FMT == MXA_E2M1) return e2m1_value(c, 1.0f);
    else if constexpr (FMT == MXA_E2M3) return e2m3_value(c);
    else return e4m3_value(c);
}
// ... and the weights' rounding of a magnitude onto the grid, as the scale search sees it (e2m1_round's `a`)
template <int WF>
__device__ __forceinline__ unsigned mxw_round(int a) {
    if constexpr (WF == MXA_E2M3) return e2m3_round(a);
    else return e2m1_round(a);
}

// N codes of BITS bits as a little-endian bit stream in N BITS / 32 words: code e at bits BITS e .. BITS e + BITS - 1.
// For 4 and 8 bits a code lies inside one word; a 6-bit code may straddle two (every index here is a constant once
// the loop is unrolled, so a lane's words are built with shifts and ors alone).
// The placing half of a packer: code c becomes element e of the words w, which start as zeros.
template <int FMT, int WORDS>
__device__ __forceinline__ void mxa_put(unsigned (&w)[WORDS], int e, unsigned c) {
    constexpr int BITS = mxa_bits<FMT>();
    const int at = BITS * e, word = at >> 5, shift = at & 31;
    w[word] |= c << shift;
    if (shift + BITS > 32) w[word + 1] |= c >> (32 - shift);
}
// ... of codes that exist already (a layer's, from its indices) ...
template <int FMT, int N>
__device__ __forceinline__ void mxa_place(const unsigned (&c)[N], unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
#pragma unroll
    for (int k = 0; k < N * mxa_bits<FMT>() / 32; ++k) w[k] = 0u;
#pragma unroll
    for (int e = 0; e < N; ++e) mxa_put<FMT>(w, e, c[e]);
}
// ... and of the values x * inv: encode (mxa_code), then place, an element at a time
template <int FMT, int N>
__device__ __forceinline__ void mxa_pack(const float (&x)[N], float inv, unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
#pragma unroll
    for (int k = 0; k < N * mxa_bits<FMT>() / 32; ++k) w[k] = 0u;
#pragma unroll
    for (int e = 0; e < N; ++e) mxa_put<FMT>(w, e, mxa_code<FMT>(x[e], inv));
}

// Lanes a block in a quantizer: each lane's codes must be whole dwords, so 8 elements a lane for E4M3 and E2M1 and 16 for E2M3
// (mx.hip, k_mx_quantize_act).
template <int FMT>
__host__ __device__ constexpr int mxq_lanes() { return FMT == MXA_E2M3 ? 2 : 4; }

// The block encoder, once: 32 floats -> one scale byte and each lane's code words.  x: this lane's N contiguous elements
// of the block, whose 32 / N lanes are neighbours (N = 8: four lanes, two DPP steps; N = 16: two lanes, one).  eb: the
// block's scale byte, the same in all of its lanes; w: this lane's words of the row's bit stream (mxa_pack under
// mxa_inverse(eb)).  Returns the block's largest magnitude bits: a caller's non-finite rule is `>= 0x7f800000`, under its
// own guard, as are its loads and stores.  Every lane of a block must call it.  The plain quantizer (mx.hip), the
// rotation's epilogue (hadamard.hip) and the fused gate/up product's (mxgemm.hip) write the same bits because this is
// the one place that makes them.
template <int FMT, int N>
__device__ __forceinline__ int mxq_encode(const float (&x)[N], unsigned &eb, unsigned (&w)[N * mxa_bits<FMT>() / 32]) {
    static_assert(N == 8 || N == 16, "the maximum takes one or two DPP steps: two or four lanes a block");
    static_assert(N * mxa_bits<FMT>() % 32 == 0, "a lane stores whole dwords: fewer lanes a block for this format");
    int top = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) top = max(top, (int)(__float_as_uint(x[e]) & 0x7fffffffu));
    top = max(top, dpp_i<DPP_XOR1>(top));
    if constexpr (N == 8) top = max(top, dpp_i<DPP_XOR2>(top));
    eb = mxa_scale_byte<FMT>(top);
    mxa_pack<FMT>(x, mxa_inverse(eb), w);
    return top;
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

// mxa_pack's words to `at` in one store, and back in one load.  The load also takes half a word (four E2M1 codes, the
// float32 de-quantizer's unit: DESIGN.md section 24), into the low half of w[0].
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
__device__ __forceinline__ void mxa_load(const uint8_t *at, unsigned (&w)[(N * mxa_bits<FMT>() + 31) / 32]) {
    constexpr int WORDS = (N * mxa_bits<FMT>() + 31) / 32;
    static_assert((N * mxa_bits<FMT>() % 32 == 0 && WORDS <= 4) || N * mxa_bits<FMT>() == 16, "a lane loads one to four whole dwords, or half of one");
    if constexpr (N * mxa_bits<FMT>() == 16) {
        w[0] = *reinterpret_cast<const unsigned short *>(at);
    } else {
        typedef unsigned V __attribute__((ext_vector_type(WORDS)));
        typedef typename std::conditional<WORDS == 3, Codes12, V>::type C;
        const C c = *reinterpret_cast<const C *>(at);
#pragma unroll
        for (int k = 0; k < WORDS; ++k) {
            if constexpr (WORDS == 3) w[k] = c.w[k];
            else w[k] = c[k];
        }
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

// ---------------------------------------------------------------- a layer's table
// A layer keeps indices into its format's table of values in rising order: 2 L + 1 of them with L = 2^(BITS - 1) - 1 (15 for
// E2M1, 63 for E2M3), entry L the zero.  Index i, clamped to 2 L, is the code sign | (L - i) below L and i - L from it; back, a
// set sign bit is L - magnitude (-0 reads as L) and anything else code + L.
template <int WF>
__device__ __forceinline__ unsigned mxw_code_of(unsigned i) {
    constexpr unsigned SIGN = 1u << (mxa_bits<WF>() - 1), L = SIGN - 1u;
    i = min(i, 2u * L);
    return i < L ? SIGN | (L - i) : i - L;
}
template <int WF>
__device__ __forceinline__ unsigned mxw_index_of(unsigned c) {
    constexpr unsigned SIGN = 1u << (mxa_bits<WF>() - 1), L = SIGN - 1u;
    return (c & SIGN) ? L - (c & L) : c + L;
}

// Sixteen index bytes (a 16-byte piece of the layer) <-> their codes as mxa_place's words.  E2M1 does four bytes of a word at
// once: min(i, 14), then i < 7 -> 15 - i (= 8 | (7 - i)), else i - 7, no byte carrying into the next; their four nibbles as
// 16 bits, the first index lowest; and back, code >= 8 -> 15 - code (0x8 -> 7), else code + 7.
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned e2m1_codes_of(unsigned x) {
    const unsigned over = (((x & 0x7f7f7f7fu) + 0x71717171u) | x) & 0x80808080u;  // bytes >= 15
    const unsigned om = (over >> 7) * 0xffu;
    x = (x & ~om) | (0x0e0e0e0eu & om);
    const unsigned gm = (((x + 0x79797979u) >> 7) & 0x01010101u) * 0xffu;  // bytes >= 7
    const unsigned c = (gm & ((x + 0x09090909u) & 0x0f0f0f0fu)) | (~gm & (x ^ 0x0f0f0f0fu)), y = c | (c >> 4);
    return (y & 0xffu) | ((y >> 8) & 0xff00u);
}
__device__ __forceinline__ unsigned e2m1_indices_of(unsigned h) {
    unsigned x = (h & 0xffu) | ((h & 0xff00u) << 8);
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    const unsigned m = ((x >> 3) & 0x01010101u) * 0xffu;
    return (m & (x ^ 0x0f0f0f0fu)) | (~m & (x + 0x07070707u));
}

template <int WF>
__device__ __forceinline__ void mxw_words_of(const uint4v idx, unsigned (&w)[mxa_bits<WF>() / 2]) {
    if constexpr (WF == MXA_E2M1) {
        w[0] = e2m1_codes_of(idx.x) | (e2m1_codes_of(idx.y) << 16);
        w[1] = e2m1_codes_of(idx.z) | (e2m1_codes_of(idx.w) << 16);
    } else {
        unsigned c[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) c[e] = mxw_code_of<WF>((idx[e >> 2] >> (8 * (e & 3))) & 0xffu);
        mxa_place<WF, 16>(c, w);
    }
}
template <int WF>
__device__ __forceinline__ uint4v mxw_indices_of(const unsigned (&w)[mxa_bits<WF>() / 2]) {
    if constexpr (WF == MXA_E2M1) {
        return (uint4v){e2m1_indices_of(w[0] & 0xffffu), e2m1_indices_of(w[0] >> 16), e2m1_indices_of(w[1] & 0xffffu),
                        e2m1_indices_of(w[1] >> 16)};
    } else {
        uint4v o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e >> 2] |= mxw_index_of<WF>(mxa_code_at<WF>(w, e)) << (8 * (e & 3));
        return o;
    }
}

}  // namespace slk
