// Every kernel that turns a matrix into an MX form or back (the forms are pinned in include/sleekit_amd.h and
// INTEGRATION.md; what a kernel knows of an element format is mxquant.h's).  Blocks of 32 consecutive columns of a row
// share one power-of-two scale (an E8M0 byte); the elements are E2M1 codes, two a byte (MXFP4), E2M3 codes, a row as a
// stream of 6-bit codes (MXFP6), or E4M3 codes, one a byte (MXFP8).
//   a layer:      slk_mx_scale_search, slk_mx_pack, slk_mx_unpack (E2M1); slk_mx_scale_search6, _pack6, _unpack6 (E2M3)
//   activations:  slk_mx_quantize_act (E4M3), _act4 (E2M1), _act6 (E2M3); slk_mx_quantize_act_rows: the three behind a row map
//   either, back: slk_mx_dequantize (E2M1), slk_mx_dequantize_act (E4M3), _act6 (E2M3): one kernel, whatever wrote the codes
//   between two layers of a gated MLP: slk_mx_glu, the gate (mxglu.h) over a (M, 2 N) matrix, elementwise
//
// n % 32 == 0, so block k of the (R, n) layer is elements [32 k, 32 k + 32) of the flat array whatever the row: every
// kernel here runs over the R n / 32 blocks (64-bit counts) and only the diagonal of H needs a block's place in its row.
//
// A power-of-two scale s = 2^(b - 127) makes every step of the group quantizer exact: x / s = x * 2^(127 - b) and
// v / (1 / s) = v * s are the IEEE quotients (one rounding of the same real number), so no kernel here divides by a
// scale, and the value of a code is put together from its bits and the scale byte.
#include <type_traits>

#include "common.h"
#include "mxglu.h"
#include "mxquant.h"

namespace slk {

static constexpr int MX_UNROLL = 4;  // units per thread and step, a whole grid apart: enough loads in flight

// workgroups of 256 lanes for `units` of work, `per` of them a thread and step
static inline int mx_grid(size_t units, int per) {
    size_t b = (units + 256 * per - 1) / (256 * per);
    if (b > 4096) b = 4096;  // 16 workgroups a CU, grid-stride beyond
    return b < 1 ? 1 : (int)b;
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

// A unit is 16 indices <-> their codes, 8 bytes of E2M1 or 12 of E2M3 (two lanes a block): one 16-byte access and two or
// three aligned dwords a lane (mxquant.h: the quantizer's own placing, store and load), contiguous over the wave.  The
// scales take a loop of their own, a block a thread.
template <int WF>
__global__ __launch_bounds__(256) void k_mx_pack(const uint8_t *__restrict__ idx, const float *__restrict__ S, size_t blocks,
                                                 uint8_t *__restrict__ codes, uint8_t *__restrict__ E, int *__restrict__ flag) {
    constexpr int WORDS = mxa_bits<WF>() / 2;
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
            unsigned w[WORDS];
            mxw_words_of<WF>(v[u], w);
            mxa_store<WF, 16>(codes + 4 * WORDS * i, w);
        }
    }
}

template <int WF>
__global__ __launch_bounds__(256) void k_mx_unpack(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t blocks,
                                                   uint8_t *__restrict__ idx, float *__restrict__ S, int *__restrict__ flag) {
    constexpr int WORDS = mxa_bits<WF>() / 2;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    if (S) mx_unpack_scales(E, blocks, gid, threads, S, flag);
    if (!idx) return;
    uint4v *dst = reinterpret_cast<uint4v *>(idx);
    const size_t units = 2 * blocks;
    for (size_t i0 = gid; i0 < units; i0 += threads * MX_UNROLL) {
        unsigned w[MX_UNROLL][WORDS];
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) mxa_load<WF, 16>(codes + 4 * WORDS * i, w[u]);
        }
#pragma unroll
        for (int u = 0; u < MX_UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) dst[i] = mxw_indices_of<WF>(w[u]);
        }
    }
}

// ---------------------------------------------------------------- quantize activations
template <class T>
__device__ __forceinline__ float act_f32(T x);
template <>
__device__ __forceinline__ float act_f32<float>(float x) { return x; }
template <>
__device__ __forceinline__ float act_f32<unsigned short>(unsigned short x) { return __uint_as_float((unsigned)x << 16); }
template <>
__device__ __forceinline__ float act_f32<_Float16>(_Float16 x) { return (float)x; }

// The plain quantizer.  LPB lanes a block, 32 / LPB elements a lane, read in 16-byte pieces; mxq_encode (mxquant.h) turns
// them into the block's scale byte, stored by the block's first lane, and every lane's codes as whole dwords of the row's
// little-endian bit stream (mxa_store).  E4M3 and E2M1 take four lanes a block: 8 bytes a lane, or one dword of
// nibbles, the even k in the low ones, which is the weights' own layout.  Eight 6-bit codes are 6 bytes, which no lane can
// store as whole dwords at a 6-byte stride, so E2M3 takes two: 12 bytes a lane, three dwords at a 12-byte stride, every one
// of them aligned (a row is 24 bytes a block; DESIGN.md section 20 has this shape measured against a lane a block).
// A NaN or an infinity has the largest magnitude bits of its block, so the integer maximum finds it and raises the flag.
// (mxq_lanes, the lanes a block of each format, is mxquant.h's: the fused product's epilogue stages its tile for mxq_encode
// in the same lane shape.)
template <class T, int FMT, int LPB>
__global__ __launch_bounds__(256) void k_mx_quantize_act(const T *__restrict__ X, size_t blocks, uint8_t *__restrict__ codes,
                                                         uint8_t *__restrict__ E, int *__restrict__ flag) {
    constexpr int EPL = 32 / LPB, BYTES = EPL * mxa_bits<FMT>() / 8;  // elements and bytes of codes a lane
    constexpr int PER = 16 / (int)sizeof(T), PIECES = EPL / PER;      // elements a 16-byte piece, pieces a lane
    typedef T V __attribute__((ext_vector_type(PER)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t units = LPB * blocks, rounds = (units + threads - 1) / threads;
    const V *src = reinterpret_cast<const V *>(X);
    bool bad = false;
    for (size_t r = 0; r < rounds; ++r) {  // (every lane of a block takes every round: units is a multiple of LPB, and so is threads)
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
        unsigned eb, w[BYTES / 4];
        bad |= mxq_encode<FMT>(x, eb, w) >= 0x7f800000;
        if (live) {
            mxa_store<FMT, EPL>(codes + BYTES * i, w);
            if (i % LPB == 0) E[i / LPB] = (uint8_t)eb;
        }
    }
    if (bad) *flag = 1;
}

// The plain quantizer behind a row map: row m of the output is the quantization of row rows[m] / div of X (tokens x K), so a
// mixture-of-experts layer quantizes its routed rows straight from x and the gathered matrix is never in memory.  The lane
// shape, the encoder and the stores are k_mx_quantize_act's, so the bits are those of that kernel on the gathered matrix.
// The map is read from device memory: a source row outside 0 .. tokens - 1 raises flag[1], loads nothing and is encoded as
// a block of zeros; flag[0] is the non-finite flag, as above.
template <class T, int FMT, int LPB>
__global__ __launch_bounds__(256) void k_mx_quantize_act_rows(const T *__restrict__ X, int tokens, int bpr, const int *__restrict__ rows,
                                                              int div, size_t blocks, uint8_t *__restrict__ codes, uint8_t *__restrict__ E,
                                                              int *__restrict__ flag) {
    constexpr int EPL = 32 / LPB, BYTES = EPL * mxa_bits<FMT>() / 8;
    constexpr int PER = 16 / (int)sizeof(T), PIECES = EPL / PER;
    typedef T V __attribute__((ext_vector_type(PER)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t units = LPB * blocks, rounds = (units + threads - 1) / threads;
    const V *src = reinterpret_cast<const V *>(X);
    bool bad = false, off = false;
    for (size_t r = 0; r < rounds; ++r) {
        const size_t i = r * threads + gid;
        const bool live = i < units;
        float x[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) x[e] = 0.0f;
        if (live) {
            const size_t b = i / LPB, m = b / (size_t)bpr, kb = b - m * (size_t)bpr;
            const int row = rows[m];
            const unsigned from = (unsigned)max(row, 0) / (unsigned)div;
            if (row < 0 || from >= (unsigned)tokens) {
                off = true;
            } else {
                const size_t at = (((size_t)from * bpr + kb) * LPB + i % LPB) * PIECES;
#pragma unroll
                for (int p = 0; p < PIECES; ++p) {
                    const V v = src[at + p];
#pragma unroll
                    for (int e = 0; e < PER; ++e) x[p * PER + e] = act_f32<T>(v[e]);
                }
            }
        }
        unsigned eb, w[BYTES / 4];
        bad |= mxq_encode<FMT>(x, eb, w) >= 0x7f800000;
        if (live) {
            mxa_store<FMT, EPL>(codes + BYTES * i, w);
            if (i % LPB == 0) E[i / LPB] = (uint8_t)eb;
        }
    }
    if (bad) flag[0] = 1;
    if (off) flag[1] = 1;
}

// ---------------------------------------------------------------- the gate, elementwise
// H (M, N) = mx_glu(gate, up) of Y (M, 2 N): VEC hidden columns a thread (4 where N % 4 == 0, so that every piece is one
// aligned vector: 16 bytes of float32, 8 of a 16-bit type), a unit a step, a whole grid apart.  Not interleaved, a thread reads
// VEC gates at column j and VEC ups at N + j; interleaved, the 2 VEC consecutive elements from column 2 j, gate first.
template <class T, int OUT, int VEC>
__global__ __launch_bounds__(256) void k_mx_glu(const T *__restrict__ Y, size_t units, int N, const GluParams p,
                                                typename PkOut<OUT>::T *__restrict__ H) {
    typedef typename PkOut<OUT>::T O;
    typedef T VI __attribute__((ext_vector_type(VEC)));
    typedef O VO __attribute__((ext_vector_type(VEC)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t per_row = (size_t)N / VEC;
    for (size_t i = gid; i < units; i += threads) {
        const size_t m = i / per_row, j = (i - m * per_row) * VEC;
        const T *row = Y + m * 2 * (size_t)N;
        float g[VEC], u[VEC];
        if (p.interleaved) {
            const VI v0 = *reinterpret_cast<const VI *>(row + 2 * j), v1 = *reinterpret_cast<const VI *>(row + 2 * j + VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T a = 2 * e < VEC ? v0[(2 * e) % VEC] : v1[(2 * e) % VEC];
                const T b = 2 * e + 1 < VEC ? v0[(2 * e + 1) % VEC] : v1[(2 * e + 1) % VEC];
                g[e] = act_f32<T>(a), u[e] = act_f32<T>(b);
            }
        } else {
            const VI vg = *reinterpret_cast<const VI *>(row + j), vu = *reinterpret_cast<const VI *>(row + N + j);
#pragma unroll
            for (int e = 0; e < VEC; ++e) g[e] = act_f32<T>(vg[e]), u[e] = act_f32<T>(vu[e]);
        }
        VO o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = PkOut<OUT>::cvt(mx_glu(g[e], u[e], p));
        *reinterpret_cast<VO *>(H + m * (size_t)N + j) = o;
    }
}

// ---------------------------------------------------------------- de-quantize
// value(code) 2^(b - 127) of any format's codes, whoever wrote them.  A lane stores 16 bytes of E4M3's or E2M1's values (4
// float32 values from 4 codes, 8 16-bit ones from 8: for E2M1 half a dword of codes, or one), or the sixteen values of the 12
// bytes an E2M3 lane wrote (64 or 32 bytes, 16 at a time).  E2M1's lanes keep MX_UNROLL units in flight, a whole grid
// apart, as the layer's other kernels do; the others take a unit a step (DESIGN.md section 24 has both measured).  OUT as
// in pack.hip: the 16-bit results are the float32 value rounded to nearest even.
template <int FMT, class T>
__host__ __device__ constexpr int mxd_elements() { return FMT == MXA_E2M3 ? 16 : 16 / (int)sizeof(T); }
template <int FMT>
__host__ __device__ constexpr int mxd_unroll() { return FMT == MXA_E2M1 ? MX_UNROLL : 1; }

template <int OUT, int FMT>
__global__ __launch_bounds__(256) void k_mx_dequantize(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ E, size_t blocks,
                                                       typename PkOut<OUT>::T *__restrict__ out, int *__restrict__ flag) {
    typedef typename PkOut<OUT>::T T;
    constexpr int EPL = mxd_elements<FMT, T>(), LPB = 32 / EPL, BYTES = EPL * mxa_bits<FMT>() / 8, UNROLL = mxd_unroll<FMT>();
    constexpr int PER = 16 / (int)sizeof(T), PIECES = EPL / PER;
    typedef T V __attribute__((ext_vector_type(PER)));
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    V *dst = reinterpret_cast<V *>(out);
    const size_t units = LPB * blocks;
    bool bad = false;
    for (size_t i0 = gid; i0 < units; i0 += threads * UNROLL) {
        unsigned w[UNROLL][(BYTES + 3) / 4], b[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i < units) {
                mxa_load<FMT, EPL>(codes + BYTES * i, w[u]);
                b[u] = E[i / LPB];
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const size_t i = i0 + u * threads;
            if (i >= units) continue;
            bad |= b[u] == 255u;
            const float sc = e8m0_value(b[u]);
#pragma unroll
            for (int p = 0; p < PIECES; ++p) {
                V v;
#pragma unroll
                for (int e = 0; e < PER; ++e) v[e] = PkOut<OUT>::cvt(mxa_value<FMT>(mxa_code_at<FMT>(w[u], p * PER + e)) * sc);
                dst[PIECES * i + p] = v;
            }
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

// slk_mx_pack, slk_mx_unpack (WF MXA_E2M1) and slk_mx_pack6, slk_mx_unpack6 (MXA_E2M3): one contract
template <int WF>
static int mx_pack(const char *name, const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag,
                   slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE((idx != nullptr) == (codes != nullptr) && (S != nullptr) == (scales != nullptr) && (idx || S),
                "null pointer: idx goes with codes, S with scales, and one pair is needed");
    SLK_REQUIRE(aligned16(idx) && aligned16(codes), "idx and codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)R * (n / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (idx ? 32.0 + 4.0 * mxa_bits<WF>() : 0.0) * blocks + (S ? 5.0 : 0.0) * blocks;
    SLK_RUN(name, 0, bytes, s, k_mx_pack<WF><<<mx_grid(2 * blocks, MX_UNROLL), 256, 0, s>>>(idx, S, blocks, codes, scales, flag));
    return SLK_OK;
}

template <int WF>
static int mx_unpack(const char *name, const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag,
                     slk_stream_t stream) {
    SLK_REQUIRE(R > 0 && n > 0 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (R = %d, n = %d)", R, n);
    SLK_REQUIRE((idx != nullptr) == (codes != nullptr) && (S != nullptr) == (scales != nullptr) && (idx || S),
                "null pointer: codes go with idx, scales with S, and one pair is needed");
    SLK_REQUIRE(aligned16(idx) && aligned16(codes), "idx and codes must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)R * (n / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    const double bytes = (idx ? 32.0 + 4.0 * mxa_bits<WF>() : 0.0) * blocks + (S ? 5.0 : 0.0) * blocks;
    SLK_RUN(name, 0, bytes, s, k_mx_unpack<WF><<<mx_grid(2 * blocks, MX_UNROLL), 256, 0, s>>>(codes, scales, blocks, idx, S, flag));
    return SLK_OK;
}

// slk_mx_quantize_act (MXA_E4M3), _act4 (MXA_E2M1) and _act6 (MXA_E2M3)
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
    constexpr int LPB = mxq_lanes<FMT>();
    const int grid = mx_grid(LPB * blocks, 1);
    return with_dtype(x_dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T T;
        const double bytes = (mxa_block_bytes<FMT>() + 32.0 * sizeof(T)) * blocks;
        SLK_RUN(name, 0, bytes, s, (k_mx_quantize_act<T, FMT, LPB><<<grid, 256, 0, s>>>(static_cast<const T *>(X), blocks, a_codes, a_scales, flag)));
        return SLK_OK;
    });
}

// slk_mx_quantize_act_rows in one element format (the checks are the entry's)
template <int FMT>
static int mx_quantize_act_rows(const void *X, int x_dtype, int T, int K, const int *rows, int div, int M, uint8_t *a_codes, uint8_t *a_scales,
                                int *flag, hipStream_t s) {
    const size_t blocks = (size_t)M * (K / 32);
    zero_async(flag, 2 * sizeof(int), s);
    constexpr int LPB = mxq_lanes<FMT>();
    const int grid = mx_grid(LPB * blocks, 1);
    return with_dtype(x_dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T Tx;
        const double bytes = (mxa_block_bytes<FMT>() + 32.0 * sizeof(Tx)) * blocks + 4.0 * M;
        SLK_RUN("mx_quantize_act_rows", 0, bytes, s,
                (k_mx_quantize_act_rows<Tx, FMT, LPB><<<grid, 256, 0, s>>>(static_cast<const Tx *>(X), T, K / 32, rows, div, blocks, a_codes, a_scales, flag)));
        return SLK_OK;
    });
}

// slk_mx_dequantize (MXA_E2M1), slk_mx_dequantize_act (MXA_E4M3) and _act6 (MXA_E2M3)
template <int FMT>
static int mx_dequantize(const char *name, const uint8_t *codes, const uint8_t *scales, int M, int K, int out_dtype, void *out, int *flag,
                         slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (M = %d, K = %d)", M, K);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(codes && scales && out, "null pointer");
    SLK_REQUIRE(aligned16(codes) && aligned16(out), "codes and out must be aligned to 16 bytes");
    hipStream_t s = as_stream(stream);
    const size_t blocks = (size_t)M * (K / 32);
    if (flag) zero_async(flag, sizeof(int), s);
    return with_dtype(out_dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T T;
        const double bytes = (mxa_block_bytes<FMT>() + 32.0 * sizeof(T)) * blocks;
        const int grid = mx_grid(32 / mxd_elements<FMT, T>() * blocks, mxd_unroll<FMT>());
        SLK_RUN(name, 0, bytes, s, (k_mx_dequantize<decltype(t)::OUT, FMT><<<grid, 256, 0, s>>>(codes, scales, blocks, static_cast<T *>(out), flag)));
        return SLK_OK;
    });
}

extern "C" {

int slk_mx_glu(const void *Y, int x_dtype, int M, int N, float alpha, float limit, float shift, int interleaved, int out_dtype, void *H,
               slk_stream_t stream) {
    SLK_REQUIRE(M > 0 && N > 0, "M and N must be at least 1 (M = %d, N = %d)", M, N);
    SLK_REQUIRE(N <= 0x3fffffff, "Y has 2 N columns: N must be below 2^30 (N = %d)", N);
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(known_dtype(out_dtype), "unknown out_dtype %d", out_dtype);
    SLK_REQUIRE(Y && H, "null pointer");
    SLK_REQUIRE(aligned16(Y) && aligned16(H), "Y and H must be aligned to 16 bytes");
    SLK_REQUIRE(limit > 0.0f, "limit must be above 0, +inf meaning no clamp (limit = %g)", (double)limit);
    SLK_REQUIRE(glu_finite(alpha) && glu_finite(shift), "alpha and shift must be finite (alpha = %g, shift = %g)", (double)alpha, (double)shift);
    SLK_REQUIRE(interleaved == 0 || interleaved == 1, "interleaved must be 0 or 1 (got %d)", interleaved);
    hipStream_t s = as_stream(stream);
    const GluParams p = {alpha, limit, shift, interleaved};
    return with_dtype(x_dtype, [&](auto ti) -> int {
        typedef typename decltype(ti)::T T;
        return with_dtype(out_dtype, [&](auto to) -> int {
            typedef typename decltype(to)::T O;
            constexpr int OUT = decltype(to)::OUT;
            const double bytes = (double)M * N * (2.0 * sizeof(T) + sizeof(O));
            if (N % 4 == 0) {
                const size_t units = (size_t)M * N / 4;
                SLK_RUN("mx_glu", 0, bytes, s, (k_mx_glu<T, OUT, 4><<<mx_grid(units, 1), 256, 0, s>>>(static_cast<const T *>(Y), units, N, p, static_cast<O *>(H))));
            } else {
                const size_t units = (size_t)M * N;
                SLK_RUN("mx_glu", 0, bytes, s, (k_mx_glu<T, OUT, 1><<<mx_grid(units, 1), 256, 0, s>>>(static_cast<const T *>(Y), units, N, p, static_cast<O *>(H))));
            }
            return SLK_OK;
        });
    });
}

int slk_mx_scale_search(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S, slk_stream_t stream) {
    return mx_scale_search<MXA_E2M1>("mx_scale_search", W, hdiag, mode, R, n, scales, S, stream);
}

int slk_mx_scale_search6(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S, slk_stream_t stream) {
    return mx_scale_search<MXA_E2M3>("mx_scale_search6", W, hdiag, mode, R, n, scales, S, stream);
}

int slk_mx_pack(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag, slk_stream_t stream) {
    return mx_pack<MXA_E2M1>("mx_pack", idx, S, R, n, codes, scales, flag, stream);
}

int slk_mx_pack6(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag, slk_stream_t stream) {
    return mx_pack<MXA_E2M3>("mx_pack6", idx, S, R, n, codes, scales, flag, stream);
}

int slk_mx_unpack(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag, slk_stream_t stream) {
    return mx_unpack<MXA_E2M1>("mx_unpack", codes, scales, R, n, idx, S, flag, stream);
}

int slk_mx_unpack6(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag, slk_stream_t stream) {
    return mx_unpack<MXA_E2M3>("mx_unpack6", codes, scales, R, n, idx, S, flag, stream);
}

int slk_mx_quantize_act(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_quantize_act<MXA_E4M3>("mx_quantize_act", X, x_dtype, M, K, a_codes, a_scales, flag, stream);
}

int slk_mx_quantize_act4(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_quantize_act<MXA_E2M1>("mx_quantize_act4", X, x_dtype, M, K, a_codes, a_scales, flag, stream);
}

int slk_mx_quantize_act6(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_quantize_act<MXA_E2M3>("mx_quantize_act6", X, x_dtype, M, K, a_codes, a_scales, flag, stream);
}

int slk_mx_quantize_act_rows(const void *X, int x_dtype, int T, int K, const int *rows, int div, int M, int a_fmt, uint8_t *a_codes,
                             uint8_t *a_scales, int *flag, slk_stream_t stream) {
    SLK_REQUIRE(T > 0 && M > 0, "T and M must be at least 1 (T = %d, M = %d)", T, M);
    SLK_REQUIRE(M <= 1 << 24, "M is above the 2^24 routed rows of one call (got %d)", M);
    SLK_REQUIRE(K >= 32 && K % 32 == 0, "MX blocks are 32 columns: K must be a positive multiple of 32 (K = %d)", K);
    SLK_REQUIRE(div >= 1, "div must be at least 1 (got %d)", div);
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(a_fmt == SLK_MX_ACT_FP8 || a_fmt == SLK_MX_ACT_FP4 || a_fmt == SLK_MX_ACT_FP6, "unknown a_fmt %d", a_fmt);
    SLK_REQUIRE(X && rows && a_codes && a_scales && flag, "null pointer");
    SLK_REQUIRE(aligned16(X) && aligned16(a_codes), "X and a_codes must be aligned to 16 bytes");
    SLK_REQUIRE((uintptr_t)rows % 4 == 0 && (uintptr_t)flag % 4 == 0, "rows and flag must be aligned to 4 bytes");
    hipStream_t s = as_stream(stream);
    if (a_fmt == SLK_MX_ACT_FP4) return mx_quantize_act_rows<MXA_E2M1>(X, x_dtype, T, K, rows, div, M, a_codes, a_scales, flag, s);
    if (a_fmt == SLK_MX_ACT_FP6) return mx_quantize_act_rows<MXA_E2M3>(X, x_dtype, T, K, rows, div, M, a_codes, a_scales, flag, s);
    return mx_quantize_act_rows<MXA_E4M3>(X, x_dtype, T, K, rows, div, M, a_codes, a_scales, flag, s);
}

int slk_mx_dequantize(const uint8_t *codes, const uint8_t *scales, int R, int n, int out_dtype, void *out, int *flag,
                      slk_stream_t stream) {
    return mx_dequantize<MXA_E2M1>("mx_dequantize", codes, scales, R, n, out_dtype, out, flag, stream);
}

int slk_mx_dequantize_act(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                          slk_stream_t stream) {
    return mx_dequantize<MXA_E4M3>("mx_dequantize_act", a_codes, a_scales, M, K, out_dtype, out, flag, stream);
}

int slk_mx_dequantize_act6(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                           slk_stream_t stream) {
    return mx_dequantize<MXA_E2M3>("mx_dequantize_act6", a_codes, a_scales, M, K, out_dtype, out, flag, stream);
}

}  // extern "C"
