// MXFP4: blocks of 32 consecutive columns of a row share one power-of-two scale (an E8M0 byte), the elements are FP4
// E2M1 codes, two a byte (slk_mx_scale_search, slk_mx_pack, slk_mx_unpack, slk_mx_dequantize; the format is pinned in
// include/sleekit_amd.h and INTEGRATION.md).  MXFP6 layers keep E2M3 codes instead, a row as a stream of 6-bit codes
// (slk_mx_scale_search6, slk_mx_pack6, slk_mx_unpack6; slk_mx_dequantize_act6 of mxgemm.hip reads that stream back).
//
// n % 32 == 0, so block k of the (R, n) layer is elements [32 k, 32 k + 32) of the flat array whatever the row: every
// kernel here runs over the R n / 32 blocks (64-bit counts) and only the diagonal of H needs a block's place in its row.
//
// A power-of-two scale s = 2^(b - 127) makes every step of the group quantizer exact: x / s = x * 2^(127 - b) and
// v / (1 / s) = v * s are the IEEE quotients (one rounding of the same real number), so no kernel here divides by a
// scale, and the value of a code is put together from its bits and the scale byte.
#include <type_traits>

#include "common.h"
#include "mxquant.h"

namespace slk {

static constexpr int MX_UNROLL = 4;  // units per thread and step, a whole grid apart: enough loads in flight

static inline int mx_grid(size_t units) {
    size_t b = (units + 256 * MX_UNROLL - 1) / (256 * MX_UNROLL);
    if (b > 4096) b = 4096;  // 16 workgroups a CU, grid-stride beyond
    return b < 1 ? 1 : (int)b;
}

// ---------------------------------------------------------------- E2M1
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

// ---------------------------------------------------------------- E2M3 (MXFP6 layers)
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

// The element format of a layer as the scale search sees it: the largest magnitude, and the rounding onto the grid.
template <int WF>
__device__ __forceinline__ unsigned mxw_round(int a) {
    if constexpr (WF == MXA_E2M3) return e2m3_round(a);
    else return e2m1_round(a);
}

// ---------------------------------------------------------------- scale selection
// 8 lanes a block, 8 blocks a wave: lane a of a block keeps elements a, 8 + a, 16 + a, 24 + a (and their diagonal
// entries) in registers for all four candidates, which is NumPy's running sum r[a] of a 32-element row; the xor steps
// 1, 2, 4 on DPP combine them as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).  Nothing goes through LDS.
// MODE 0: max (the power of two at or above the non-saturating scale), 1: mse, 2: diag (terms weighed by diag(H)).
// WF: the elements, MXA_E2M1 (largest magnitude 6) or MXA_E2M3 (7.5).
template <int MODE, int WF = MXA_E2M1>
__global__ __launch_bounds__(256) void k_mx_scale_search(const float *__restrict__ W, const float *__restrict__ hdiag, size_t blocks,
                                                         int bpr, uint8_t *__restrict__ E, float *__restrict__ S) {
    const int lane = threadIdx.x & 63, q = lane >> 3, a = lane & 7;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (size_t)gridDim.x * 4;
    for (size_t k0 = wave * 8; k0 < blocks; k0 += waves * 8) {
        const size_t k = min(k0 + q, blocks - 1);  // (a wave's last blocks may repeat the final one: every lane stays active)
        const float *w = W + 32 * k + a;
        float x[4], h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = w[8 * i];
        if constexpr (MODE == 2) {
            const float *hd = hdiag + 32 * ((unsigned)k % (unsigned)bpr) + a;  // (blocks < 2^31, checked by the entry)
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = hd[8 * i];
        }
        float mn = fminf(fminf(x[0], x[1]), fminf(x[2], x[3])), mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        mn = fminf(mn, dpp_f<DPP_XOR1>(mn));
        mx = fmaxf(mx, dpp_f<DPP_XOR1>(mx));
        mn = fminf(mn, dpp_f<DPP_XOR2>(mn));
        mx = fmaxf(mx, dpp_f<DPP_XOR2>(mx));
        mn = fminf(mn, dpp_f<DPP_HALF_MIRROR>(mn));
        mx = fmaxf(mx, dpp_f<DPP_HALF_MIRROR>(mx));
        // scaling.py:53-54 with codes +-6: max(max / 6, min / -6) = max(max, -min) / 6 (a division by 6 is monotonic and odd)
        const float b0 = fmaxf(fmaxf(mx, -mn) / mxa_largest<WF>(), 1.0e-16f);
        // the smallest power of two >= b0, as its exponent field: 74 (the floor) .. 253 for finite weights
        unsigned eb = min(((__float_as_uint(b0) + 0x7fffffu) >> 23) & 0xffu, 253u);
        if constexpr (MODE != 0) {
            float ax[4];
            int neg[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ax[i] = fabsf(x[i]);
                neg[i] = (int)(__float_as_uint(x[i]) >> 31);
            }
            float best = __builtin_huge_valf();
            int bf = 3;  // (errors that all overflow leave the non-saturating scale)
#pragma unroll
            for (int f = 0; f < 4; ++f) {  // factors 0.125, 0.25, 0.5, 1
                const unsigned es = eb - 3u + (unsigned)f;
                const float s = __uint_as_float(es << 23), inv = __uint_as_float((254u - es) << 23);
                float acc = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // |x| / s, its magnitude on the grid, |v| / (1 / s) - |x|: the error but for its sign, which the square drops
                    const float v = __uint_as_float(mxw_round<WF>((int)__float_as_uint(ax[i] * inv) - neg[i]));
                    const float e = v * s - ax[i];
                    const float e2 = e * e;
                    const float term = MODE == 2 ? h[i] * e2 : e2;
                    acc = i == 0 ? term : acc + term;
                }
                acc = acc + dpp_f<DPP_XOR1>(acc);
                acc = acc + dpp_f<DPP_XOR2>(acc);
                acc = acc + dpp_f<DPP_HALF_MIRROR>(acc);
                if (acc < best) {  // strict: the first minimum is kept (scaling.py:131-133)
                    best = acc;
                    bf = f;
                }
            }
            eb = eb - 3u + (unsigned)bf;
        }
        if (a == 0 && k0 + q < blocks) {
            if (E) E[k] = (uint8_t)eb;
            if (S) S[k] = __uint_as_float(eb << 23);
        }
    }
}

// ---------------------------------------------------------------- pack / unpack
// Four index bytes in a word: min(i, 14), then i < 7 -> 15 - i (= 8 | (7 - i)), else i - 7; no byte carries into the next.
__device__ __forceinline__ unsigned mx_codes_of(unsigned x) {
    const unsigned over = (((x & 0x7f7f7f7fu) + 0x71717171u) | x) & 0x80808080u;  // bytes >= 15
    const unsigned om = (over >> 7) * 0xffu;
    x = (x & ~om) | (0x0e0e0e0eu & om);
    const unsigned gm = (((x + 0x79797979u) >> 7) & 0x01010101u) * 0xffu;  // bytes >= 7
    return (gm & ((x + 0x09090909u) & 0x0f0f0f0fu)) | (~gm & (x ^ 0x0f0f0f0fu));
}
// ... their four nibbles as 16 bits, the first index lowest
__device__ __forceinline__ unsigned mx_nibbles(unsigned c) {
    const unsigned y = c | (c >> 4);
    return (y & 0xffu) | ((y >> 8) & 0xff00u);
}
// 16 bits of codes -> four index bytes: code >= 8 -> 15 - code (0x8 -> 7), else code + 7
__device__ __forceinline__ unsigned mx_indices_of(unsigned h) {
    unsigned x = (h & 0xffu) | ((h & 0xff00u) << 8);
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    const unsigned m = ((x >> 3) & 0x01010101u) * 0xffu;
    return (m & (x ^ 0x0f0f0f0fu)) | (~m & (x + 0x07070707u));
}

typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef unsigned uint2v __attribute__((ext_vector_type(2)));

// float32 scales -> E8M0 bytes, and back: a block a thread, the same for every element format.
__device__ __forceinline__ void mx_pack_scales(const float *__restrict__ S, size_t blocks, size_t gid, size_t threads,
                                               uint8_t *__restrict__ E, int *__restrict__ flag) {
    bool bad = false;
    for (size_t k = gid; k < blocks; k += threads) {
        const unsigned u = __float_as_uint(S[k]), b = u >> 23;  // a positive normal power of two: its exponent field
        bad |= (u & 0x807fffffu) != 0u || b == 0u || b == 255u;
        E[k] = (uint8_t)min(b & 0xffu, 254u);
    }
    if (bad && flag) *flag = 1;
}
__device__ __forceinline__ void mx_unpack_scales(const uint8_t *__restrict__ E, size_t blocks, size_t gid, size_t threads,
                                                 float *__restrict__ S, int *__restrict__ flag) {
    bool bad = false;
    for (size_t k = gid; k < blocks; k += threads) {
        const unsigned b = E[k];
        bad |= b == 255u;
        S[k] = e8m0_value(b);
    }
    if (bad && flag) *flag = 1;
}

// A unit is 16 indices <-> 8 bytes of codes (two lanes a block): one 16-byte and one 8-byte access a lane, contiguous
// over the wave.  The scales take a loop of their own, a block a thread.
__global__ __launch_bounds__(256) void k_mx_pack(const uint8_t *__restrict__ idx, const float *__restrict__ S, size_t blocks,
                                                 uint8_t *__restrict__ codes, uint8_t *__restrict__ E, int *__restrict__ flag) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    if (S) mx_pack_scales(S, blocks, gid, threads, E, flag);
    if (!idx) return;
    const uint4v *src = reinterpret_cast<const uint4v *>(idx);
    uint2v *dst = reinterpret_cast<uint2v *>(codes);
    const size_t units = 2 * blocks;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        uint4v v[MX_UNROLL];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            uint2v o;
            o.x = mx_nibbles(mx_codes_of(v[u].x)) | (mx_nibbles(mx_codes_of(v[u].y)) << 16);
            o.y = mx_nibbles(mx_codes_of(v[u].z)) | (mx_nibbles(mx_codes_of(v[u].w)) << 16);
            dst[i] = o;
        }
    }
}

__global__ __launch_bounds__(256) void k_mx_unpack(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t blocks,
                                                   uint8_t *__restrict__ idx, float *__restrict__ S, int *__restrict__ flag) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    if (S) mx_unpack_scales(E, blocks, gid, threads, S, flag);
    if (!idx) return;
    const uint2v *src = reinterpret_cast<const uint2v *>(codes);
    uint4v *dst = reinterpret_cast<uint4v *>(idx);
    const size_t units = 2 * blocks;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        uint2v v[MX_UNROLL];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            uint4v o;
            o.x = mx_indices_of(v[u].x & 0xffffu);
            o.y = mx_indices_of(v[u].x >> 16);
            o.z = mx_indices_of(v[u].y & 0xffffu);
            o.w = mx_indices_of(v[u].y >> 16);
            dst[i] = o;
        }
    }
}

// MXFP6.  Index i of the 63-entry table -> E2M3 code: min(i, 62), then i < 31 -> 0x20 | (31 - i), else i - 31; and back:
// a set sign bit -> 31 - magnitude code (0x20, -0, -> 31), else code + 31.
__device__ __forceinline__ unsigned mx6_code_of(unsigned i) {
    i = min(i, 62u);
    return i < 31u ? 0x20u | (31u - i) : i - 31u;
}
__device__ __forceinline__ unsigned mx6_index_of(unsigned c) { return (c & 0x20u) ? 31u - (c & 31u) : c + 31u; }

// A unit is 16 indices <-> 12 bytes of the row's stream of 6-bit codes (two lanes a block, as above): one 16-byte access
// and three aligned dwords a lane (mxquant.h: the activation quantizer's own packer, store and load).
__global__ __launch_bounds__(256) void k_mx_pack6(const uint8_t *__restrict__ idx, const float *__restrict__ S, size_t blocks,
                                                  uint8_t *__restrict__ codes, uint8_t *__restrict__ E, int *__restrict__ flag) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    if (S) mx_pack_scales(S, blocks, gid, threads, E, flag);
    if (!idx) return;
    const uint4v *src = reinterpret_cast<const uint4v *>(idx);
    const size_t units = 2 * blocks;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        uint4v v[MX_UNROLL];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            float x[16];  // the codes' values: the quantizer's packer turns them, under the scale 1, back into their codes
            unsigned w[3];
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = e2m3_value(mx6_code_of((v[u][e >> 2] >> (8 * (e & 3))) & 0xffu));
            mxa_pack<MXA_E2M3, 16>(x, 1.0f, w);
            mxa_store<MXA_E2M3, 16>(codes + 12 * i, w);
        }
    }
}

__global__ __launch_bounds__(256) void k_mx_unpack6(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t blocks,
                                                    uint8_t *__restrict__ idx, float *__restrict__ S, int *__restrict__ flag) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    if (S) mx_unpack_scales(E, blocks, gid, threads, S, flag);
    if (!idx) return;
    uint4v *dst = reinterpret_cast<uint4v *>(idx);
    const size_t units = 2 * blocks;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        unsigned w[MX_UNROLL][3];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) mxa_load<MXA_E2M3, 16>(codes + 12 * i, w[u]);
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            uint4v o = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 16; ++e) o[e >> 2] |= mx6_index_of(mxa_code_at<MXA_E2M3>(w[u], e)) << (8 * (e & 3));
            dst[i] = o;
        }
    }
}

// ---------------------------------------------------------------- de-quantize
// A unit is the 16 bytes a lane stores: 4 float32 values from 2 bytes of codes, or 8 16-bit values from 4 bytes.  OUT as
// in pack.hip: the 16-bit results are the float32 value rounded to nearest even.
template <int OUT>
__global__ __launch_bounds__(256) void k_mx_dequantize(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t blocks,
                                                       typename PkOut<OUT>::T *__restrict__ out, int *__restrict__ flag) {
    typedef typename PkOut<OUT>::T T;
    constexpr int EPL = 16 / (int)sizeof(T), UPB = 32 / EPL;  // elements a unit, units a block
    typedef T V __attribute__((ext_vector_type(EPL)));
    typedef typename std::conditional<EPL == 4, unsigned short, unsigned>::type C;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const C *src = reinterpret_cast<const C *>(codes);
    V *dst = reinterpret_cast<V *>(out);
    const size_t units = UPB * blocks;
    bool bad = false;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        unsigned c[MX_UNROLL], b[MX_UNROLL];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) {
                c[u] = src[i];
                b[u] = E[i / UPB];
            }
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            bad |= b[u] == 255u;
            const float sc = e8m0_value(b[u]);
            V v;
#pragma unroll
            for (int e = 0; e < EPL; ++e) v[e] = PkOut<OUT>::cvt(e2m1_value(c[u] >> (4 * e), sc));
            dst[i] = v;
        }
    }
    if (bad && flag) *flag = 1;
}

}  // namespace slk

using namespace slk;

// slk_mx_scale_search (WF MXA_E2M1) and slk_mx_scale_search6 (MXA_E2M3)
template <int WF>
static int mx_scale_search(const char *name, const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S,
                           slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE(mode >= SLK_MX_MAX && mode <= SLK_MX_DIAG, "unknown scale mode %d", mode);
    SLK_REQUIRE(W && (scales || S), "null pointer");
    SLK_REQUIRE((mode == SLK_MX_DIAG) == (hdiag != nullptr), "hdiag goes with the diag mode and with no other");
    hipStream_t s = as_stream(stream);
    const int bpr = n / 32;
    const size_t blocks = (size_t)R * bpr;
    SLK_REQUIRE(blocks <= 0x7fffffffULL, "too many blocks");
    const size_t wgs = (blocks + 31) / 32;  // 8 blocks a wave, 4 waves a workgroup
    const int grid = (int)(wgs < 8192 ? wgs : 8192);
    const double bytes = 4.0 * R * n + 5.0 * blocks;
    if (mode == SLK_MX_MAX)
        SLK_RUN(name, 0, bytes, s, (k_mx_scale_search<0, WF><<<grid, 256, 0, s>>>(W, hdiag, blocks, bpr, scales, S)));
    else if (mode == SLK_MX_MSE)
        SLK_RUN(name, 0, bytes, s, (k_mx_scale_search<1, WF><<<grid, 256, 0, s>>>(W, hdiag, blocks, bpr, scales, S)));
    else
        SLK_RUN(name, 0, bytes, s, (k_mx_scale_search<2, WF><<<grid, 256, 0, s>>>(W, hdiag, blocks, bpr, scales, S)));
    return SLK_OK;
}

// slk_mx_pack, slk_mx_unpack (BITS 4) and slk_mx_pack6, slk_mx_unpack6 (6): one contract
template <int BITS>
static int mx_pack(const char *name, const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag,
                   slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE((idx != nullptr) == (codes != nullptr) && (S != nullptr) == (scales != nullptr) && (idx || S),
                "null pointer: idx goes with codes, S with scales, and one pair is needed");
    SLK_REQUIRE(aligned16(idx) && aligned16(codes), "idx and codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)R * (n / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (idx ? 32.0 + 4.0 * BITS : 0.0) * blocks + (S ? 5.0 : 0.0) * blocks;
    if constexpr (BITS == 6) SLK_RUN(name, 0, bytes, s, k_mx_pack6<<<mx_grid(2 * blocks), 256, 0, s>>>(idx, S, blocks, codes, scales, flag));
    else SLK_RUN(name, 0, bytes, s, k_mx_pack<<<mx_grid(2 * blocks), 256, 0, s>>>(idx, S, blocks, codes, scales, flag));
    return SLK_OK;
}

template <int BITS>
static int mx_unpack(const char *name, const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag,
                     slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE((idx != nullptr) == (codes != nullptr) && (S != nullptr) == (scales != nullptr) && (idx || S),
                "null pointer: codes go with idx, scales with S, and one pair is needed");
    SLK_REQUIRE(aligned16(idx) && aligned16(codes), "idx and codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)R * (n / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (idx ? 32.0 + 4.0 * BITS : 0.0) * blocks + (S ? 5.0 : 0.0) * blocks;
    if constexpr (BITS == 6) SLK_RUN(name, 0, bytes, s, k_mx_unpack6<<<mx_grid(2 * blocks), 256, 0, s>>>(codes, scales, blocks, idx, S, flag));
    else SLK_RUN(name, 0, bytes, s, k_mx_unpack<<<mx_grid(2 * blocks), 256, 0, s>>>(codes, scales, blocks, idx, S, flag));
    return SLK_OK;
}

extern "C" {

int slk_mx_scale_search(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S, slk_stream_t stream) {
    return mx_scale_search<MXA_E2M1>("mx_scale_search", W, hdiag, mode, R, n, scales, S, stream);
}

int slk_mx_scale_search6(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S, slk_stream_t stream) {
    return mx_scale_search<MXA_E2M3>("mx_scale_search6", W, hdiag, mode, R, n, scales, S, stream);
}

int slk_mx_pack(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag, slk_stream_t stream) {
    return mx_pack<4>("mx_pack", idx, S, R, n, codes, scales, flag, stream);
}

int slk_mx_pack6(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag, slk_stream_t stream) {
    return mx_pack<6>("mx_pack6", idx, S, R, n, codes, scales, flag, stream);
}

int slk_mx_unpack(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag, slk_stream_t stream) {
    return mx_unpack<4>("mx_unpack", codes, scales, R, n, idx, S, flag, stream);
}

int slk_mx_unpack6(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag, slk_stream_t stream) {
    return mx_unpack<6>("mx_unpack6", codes, scales, R, n, idx, S, flag, stream);
}

int slk_mx_dequantize(const uint8_t *codes, const uint8_t *scales, int R, int n, int out_dtype, void *out, int *flag,
                      slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE(codes && scales && out, "null pointer");
    SLK_REQUIRE(out_dtype == SLK_DTYPE_F32 || out_dtype == SLK_DTYPE_BF16 || out_dtype == SLK_DTYPE_F16, "unknown out_dtype %d",
                out_dtype);
    SLK_REQUIRE(aligned16(codes) && aligned16(out), "codes and out must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)R * (n / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (17.0 + 32.0 * (out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0)) * blocks;
    if (out_dtype == SLK_DTYPE_BF16)
        SLK_RUN("mx_dequantize", 0, bytes, s,
                k_mx_dequantize<PK_BF16><<<mx_grid(4 * blocks), 256, 0, s>>>(codes, scales, blocks, static_cast<unsigned short *>(out), flag));
    else if (out_dtype == SLK_DTYPE_F16)
        SLK_RUN("mx_dequantize", 0, bytes, s,
                k_mx_dequantize<PK_F16><<<mx_grid(4 * blocks), 256, 0, s>>>(codes, scales, blocks, static_cast<_Float16 *>(out), flag));
    else
        SLK_RUN("mx_dequantize", 0, bytes, s,
                k_mx_dequantize<PK_F32><<<mx_grid(8 * blocks), 256, 0, s>>>(codes, scales, blocks, static_cast<float *>(out), flag));
    return SLK_OK;
}

}  // extern "C"
