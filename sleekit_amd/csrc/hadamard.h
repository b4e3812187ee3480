// The butterflies of the block Hadamard rotation (step 2 of slk_hadamard_rows' contract, include/sleekit_amd.h) for a lane
// that holds N contiguous elements of a row: the stages inside a lane's registers and the stages between the lanes of one
// wave.  Shared by the transform and its quantizing form (hadamard.hip, N = 16) and by the rotating epilogue of the fused
// gate/up product (mxgemm.hip, N = 8 or 16), so that every kernel that rotates adds the same two values in the same
// operation, whichever of them are registers and whichever lanes: the butterfly fixes which two values meet in each addition,
// and the lower element always takes lower + upper, the upper one lower - upper.
#pragma once

#include "common.h"

namespace slk {

// the value lane (l ^ D) holds, for a 32-bit word
template <int D>
__device__ __forceinline__ int hd_xor_word(int x, int lane) {
    if constexpr (D == 1) return dpp_i<DPP_XOR1>(x);
    else if constexpr (D == 2) return dpp_i<DPP_XOR2>(x);
    else if constexpr (D == 4) return dpp_i<0x1B>(dpp_i<DPP_HALF_MIRROR>(x));  // (i ^ 7) ^ 3
    else if constexpr (D == 8) return dpp_i<0x128>(x);                          // row_ror:8 of a row of 16
    else if constexpr (D == 16) {
        // rows 1 and 3 of the first operand change places with rows 0 and 2 of the second: [0] = rows 0 0 2 2, [1] = 1 1 3 3
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((lane & 16) ? r[0] : r[1]);
    } else {
        // the upper half of the first operand changes places with the lower half of the second: [0] = lower lower, [1] = upper upper
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((lane & 32) ? r[0] : r[1]);
    }
}
template <int D>
__device__ __forceinline__ float hd_xor(float x, int lane) { return __int_as_float(hd_xor_word<D>(__float_as_int(x), lane)); }
template <int D>
__device__ __forceinline__ double hd_xor(double x, int lane) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)hd_xor_word<D>((int)(b & 0xffffffffLL), lane);
    const unsigned hi = (unsigned)hd_xor_word<D>((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one stage between lanes: the lower element takes lower + upper, the upper one lower - upper.  Every lane of the wave must
// be active: the exchange reads a lane that is not as zero.  (Written as p + (-v) under a per-lane sign mask instead of the
// select, an earlier form of the transform took 162 to 210 registers instead of 64 to 113 and ran 8 to 14 % slower at 4096
// rows: DESIGN.md section 16.)
template <int D, class C, int N>
__device__ __forceinline__ void hd_lane_stage(C (&v)[N], int lane) {
    const bool upper = lane & D;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const C p = hd_xor<D>(v[e], lane);
        v[e] = upper ? p - v[e] : v[e] + p;
    }
}

// the stages inside a lane, strides 1 .. N / 2 in that order, of a block of 2^lb (blocks below N: a lane holds N >> lb whole blocks)
template <class C, int N>
__device__ __forceinline__ void hd_register_stages(C (&v)[N], int lb) {
    static_assert(N >= 2 && (N & (N - 1)) == 0, "a lane holds a power of two of elements");
#pragma unroll
    for (int k = 0; (1 << k) < N; ++k) {
        if (lb > k) {
            const int h = 1 << k;
#pragma unroll
            for (int i = 0; i < N; ++i)
                if ((i & h) == 0) {
                    const C a = v[i], b = v[i + h];
                    v[i] = a + b;
                    v[i + h] = a - b;
                }
        }
    }
}

// A block of at most 4 N elements whose lanes share a quad (N = 8: 32 / 8 = 4 lanes, N = 16: 2): the registers, then lane
// distances 1 and 2, both quad_perm.  lb is uniform, and so is every branch here.
template <class C, int N>
__device__ __forceinline__ void hd_quad_butterfly(C (&v)[N], int lb, int lane) {
    constexpr int LN = N == 16 ? 4 : N == 8 ? 3 : N == 4 ? 2 : 1;
    static_assert(1 << LN == N, "2, 4, 8 or 16 elements a lane");
    hd_register_stages(v, lb);
    if (lb > LN) hd_lane_stage<1>(v, lane);
    if (lb > LN + 1) hd_lane_stage<2>(v, lane);
}

}  // namespace slk
