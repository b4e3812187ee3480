// What the GEMMs that de-quantize a layer inside a bfloat16 / float16 MFMA share (packgemm.hip: packed codebook indices;
// mxgemm_a16.hip: MX layers against 16-bit activations): the instruction, the activations' fragment and the result's store.
//
// v_mfma_f32_16x16x32_{bf16,f16} (the identity tests of tests/test_gpu_packed_gemm.py and
// tests/test_gpu_mx_a16.py hold the map): lane l = i + 16 q carries A[row i][k = 8 q + j] and B[k = 8 q + j][col i],
// j = 0 .. 7, as 16 bytes; D: lane l holds column l & 15, rows 4 (l >> 4) + 0 .. 3.  A is X, B is W^T.
#pragma once

#include <type_traits>

#include "common.h"

namespace slk {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

template <int C16>
__device__ __forceinline__ unsigned short pg_cvt(float v) {
    if constexpr (C16 == PK_BF16) return pk_bf16(v);
    else return __builtin_bit_cast(unsigned short, (_Float16)v);
}

template <int C16>
__device__ __forceinline__ v4f pg_mfma(v4i a, v4i b, v4f c) {
    if constexpr (C16 == PK_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

// ---------------------------------------------------------------- activations
// Eight consecutive elements of x as loaded, and as the lane's A fragment: each rounded to nearest even to the compute
// type through float32 (the identity where x has that type already).
template <class TX>
struct XRaw {
    v4i v;
};
template <>
struct XRaw<float> {
    v4f a, b;
};
template <class TX>
__device__ __forceinline__ XRaw<TX> pg_load_x(const TX *__restrict__ p, bool ok) {
    XRaw<TX> r;
    if constexpr (std::is_same<TX, float>::value) {
        r.a = r.b = (v4f){0.0f, 0.0f, 0.0f, 0.0f};
        if (ok) {
            r.a = *reinterpret_cast<const v4f *>(p);
            r.b = *reinterpret_cast<const v4f *>(p + 4);
        }
    } else {
        r.v = (v4i){0, 0, 0, 0};
        if (ok) r.v = *reinterpret_cast<const v4i *>(p);
    }
    return r;
}
template <class TX, int C16>
__device__ __forceinline__ v4i pg_x_frag(const XRaw<TX> r) {
    if constexpr (std::is_same<TX, typename PkOut<C16>::T>::value) {
        return r.v;
    } else {
        float f[8];
        if constexpr (std::is_same<TX, float>::value) {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = r.a[e], f[4 + e] = r.b[e];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned short h = (unsigned short)((unsigned)r.v[e >> 1] >> (16 * (e & 1)));
                if constexpr (std::is_same<TX, _Float16>::value) f[e] = (float)__builtin_bit_cast(_Float16, h);
                else f[e] = __uint_as_float((unsigned)h << 16);
            }
        }
        v4i o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (int)((unsigned)pg_cvt<C16>(f[2 * e]) | ((unsigned)pg_cvt<C16>(f[2 * e + 1]) << 16));
        return o;
    }
}

// ---------------------------------------------------------------- results
__device__ __forceinline__ void pg_store(void *__restrict__ Y, size_t at, float v, int out_dtype) {
    if (out_dtype == SLK_DTYPE_F32) static_cast<float *>(Y)[at] = v;
    else if (out_dtype == SLK_DTYPE_BF16) static_cast<unsigned short *>(Y)[at] = pk_bf16(v);
    else static_cast<_Float16 *>(Y)[at] = (_Float16)v;
}
// a lane's four results of one MFMA tile: column n, rows m0 + 0 .. 3
__device__ __forceinline__ void pg_store_tile(v4f acc, const float *__restrict__ bias, int m0, int n, int M, int N, int out_dtype,
                                              void *__restrict__ Y) {
    if (n >= N) return;
    const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + r;
        if (m < M) pg_store(Y, (size_t)m * N + n, bias ? acc[r] + bv : acc[r], out_dtype);
    }
}

}  // namespace slk
