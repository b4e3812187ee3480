// Bit-packed codebook indices: pack, unpack and de-quantize straight from the packed words (slk_pack_indices,
// slk_unpack_indices, slk_dequantize_packed; the format is pinned in include/sleekit_amd.h and INTEGRATION.md).
//
// Layout: a row of n indices is cut into C = ceil(n / 32) chunks of 32; chunk k of row r is the b words
// [b k, b k + b) of that row (W = b C words a row), read as one little-endian integer whose bits [i b, i b + b) hold
// index 32 k + i.  A chunk is 4 b bytes of words for 32 bytes of indices, so eight chunks -- one SEGMENT, 256
// indices -- map onto a wave: lane l owns indices 4 l .. 4 l + 3 of the segment (lanes 8 q .. 8 q + 7 are chunk q),
// which are 4 b consecutive bits of the chunk, starting at bit 4 (l % 8) b.
//
// All three kernels are memory-bound streams: every wave instruction touches contiguous bytes (256 B of indices,
// 8 b words, 1 KB of float32 out), each wave takes PK_UNROLL segments per step to keep enough loads in flight, and
// every element offset is 64-bit (a stack of layers can pass 2^31 indices).
#include "common.h"

namespace slk {

static constexpr int PK_UNROLL = 4;  // segments per wave and step

static inline int pk_blocks(size_t segments) {
    const size_t waves = (segments + PK_UNROLL - 1) / PK_UNROLL;
    size_t b = (waves + 3) / 4;  // 4 waves a workgroup
    if (b > 4096) b = 4096;      // 16 workgroups a CU, grid-stride beyond
    return b < 1 ? 1 : (int)b;
}

// Bits [4 l b, 4 l b + 4 b) of the chunk whose b words start at `w` (lane-in-chunk l): one or two word loads.
__device__ __forceinline__ unsigned chunk_piece(const unsigned *__restrict__ w, int l, int b) {
    const int bit = 4 * l * b, w0 = bit >> 5, sh = bit & 31;
    unsigned long long x = w[w0];
    if (sh + 4 * b > 32) x |= (unsigned long long)w[w0 + 1] << 32;  // (then w0 + 1 < b: the piece ends inside the chunk)
    return (unsigned)(x >> sh);
}

// ---------------------------------------------------------------- pack
// ALIGNED: n % 4 == 0 and a 4-byte aligned base, so a lane's four indices are one 4-byte load; otherwise byte loads.
// Word j of a chunk is ORed together by lane j of the chunk from the pieces of the (at most 9) lanes it overlaps,
// fetched with cross-lane reads; lanes j < b store, so a wave stores 8 b contiguous words.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_pack_indices(const uint8_t *__restrict__ idx, int R, int n, int b,
                                                      unsigned *__restrict__ out) {
    const int lane = threadIdx.x & 63, q = lane >> 3, l = lane & 7;
    const int C = (n + 31) >> 5, spr = (C + 7) >> 3;  // chunks and segments a row
    const size_t W = (size_t)b * C, segs = (size_t)R * spr;
    const unsigned mask = (1u << b) - 1u;
    const size_t wave = (size_t)__builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const size_t waves = (size_t)gridDim.x * 4;
    for (size_t t = wave * PK_UNROLL; t < segs; t += waves * PK_UNROLL) {
        unsigned piece[PK_UNROLL];
        int col[PK_UNROLL];
        size_t row[PK_UNROLL];
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            const size_t seg = t + u;
            row[u] = seg / spr;
            col[u] = (int)(seg % spr) * 256 + 4 * lane;
            unsigned x = 0;
            if (seg < segs) {
                const uint8_t *src = idx + row[u] * n;
                if (ALIGNED && col[u] + 3 < n) {
                    x = *reinterpret_cast<const unsigned *>(src + col[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col[u] + e < n) x |= (unsigned)src[col[u] + e] << (8 * e);
                }
            }
            piece[u] = x;
        }
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            unsigned p = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) p |= ((piece[u] >> (8 * e)) & mask) << (e * b);  // 4 b <= 32 bits
            // word l of this chunk: bits [32 l, 32 l + 32) gather the pieces of lanes l0 .. l0 + 8 (those below 8)
            const int l0 = (8 * l) / b;
            unsigned word = 0;
#pragma unroll
            for (int s = 0; s < 9; ++s) {
                const int src = l0 + s;
                const unsigned v = __shfl(p, 8 * q + (src < 8 ? src : 7));
                const int sh = 4 * src * b - 32 * l;
                if (src < 8 && sh < 32) word |= sh >= 0 ? v << sh : (sh > -32 ? v >> -sh : 0u);
            }
            const int k = (col[u] >> 5);  // this lane's chunk in the row (the chunk's first column is 32 k)
            if (t + u < segs && l < b && k < C) out[row[u] * W + (size_t)b * k + l] = word;
        }
    }
}

// ---------------------------------------------------------------- unpack
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_unpack_indices(const unsigned *__restrict__ words, int R, int n, int b,
                                                        uint8_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63, l = lane & 7;
    const int C = (n + 31) >> 5, spr = (C + 7) >> 3;
    const size_t W = (size_t)b * C, segs = (size_t)R * spr;
    const unsigned mask = (1u << b) - 1u;
    const size_t wave = (size_t)__builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const size_t waves = (size_t)gridDim.x * 4;
    for (size_t t = wave * PK_UNROLL; t < segs; t += waves * PK_UNROLL) {
        unsigned piece[PK_UNROLL];
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            const size_t seg = t + u, r = seg / spr;
            const int col = (int)(seg % spr) * 256 + 4 * lane;
            piece[u] = (seg < segs && col < n) ? chunk_piece(words + r * W + (size_t)b * (col >> 5), l, b) : 0u;
        }
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            const size_t seg = t + u, r = seg / spr;
            const int col = (int)(seg % spr) * 256 + 4 * lane;
            if (seg >= segs || col >= n) continue;
            unsigned x = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) x |= ((piece[u] >> (e * b)) & mask) << (8 * e);
            uint8_t *dst = idx + r * n;
            if (ALIGNED && col + 3 < n) {
                *reinterpret_cast<unsigned *>(dst + col) = x;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < n) dst[col + e] = (uint8_t)(x >> (8 * e));
            }
        }
    }
}

// ---------------------------------------------------------------- de-quantize
// SCALE: 0 none, 1 per row (value / (1 / scale[r]), the loop's de-scale), 2 per group (value / (1 / S[r][c / g]), as
// k_dequantize_grouped), 3 per group with offsets (+ O[r][c / g]).  OUT: 0 float32, 1 bfloat16, 2 float16 (the float32
// value rounded to nearest even).  The codebook's values sit in LDS: index k reads value min(k, levels - 1), formed like
// the quantizer's (k * step + zero in float32) or read from the table.  ALIGNED: n % 4 == 0 and an output base aligned
// to 4 elements, so a lane's four values are one vector store.
template <int SCALE, int OUT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_dequantize_packed(const unsigned *__restrict__ words, int R, int n, int b, Grid g,
                                                           const float *__restrict__ scale, int gsize, const float *__restrict__ O,
                                                           typename PkOut<OUT>::T *__restrict__ out) {
    typedef typename PkOut<OUT>::T T;
    typedef typename PkOut<OUT>::V V;
    __shared__ float lut[256];
    for (int k = threadIdx.x; k < g.n; k += blockDim.x) lut[k] = cb_entry(k, g);
    __syncthreads();
    const int lane = threadIdx.x & 63, l = lane & 7, top = g.n - 1;
    const int C = (n + 31) >> 5, spr = (C + 7) >> 3, G = SCALE >= 2 ? n / gsize : 1;
    const bool quad = SCALE >= 2 && gsize % 4 == 0;  // a lane's four columns share one group
    const size_t W = (size_t)b * C, segs = (size_t)R * spr;
    const unsigned mask = (1u << b) - 1u;
    const size_t wave = (size_t)__builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const size_t waves = (size_t)gridDim.x * 4;
    for (size_t t = wave * PK_UNROLL; t < segs; t += waves * PK_UNROLL) {
        unsigned piece[PK_UNROLL];
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            const size_t seg = t + u, r = seg / spr;
            const int col = (int)(seg % spr) * 256 + 4 * lane;
            piece[u] = (seg < segs && col < n) ? chunk_piece(words + r * W + (size_t)b * (col >> 5), l, b) : 0u;
        }
#pragma unroll
        for (int u = 0; u < PK_UNROLL; ++u) {
            const size_t seg = t + u, r = seg / spr;
            const int col = (int)(seg % spr) * 256 + 4 * lane;
            if (seg >= segs || col >= n) continue;
            float inv = 1.0f;
            if constexpr (SCALE == 1) inv = 1.0f / scale[r];  // scaling.py:80: a division by the reciprocal
            V v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = min((int)((piece[u] >> (e * b)) & mask), top);
                float x = lut[k];
                if constexpr (SCALE == 1) x = x / inv;
                if constexpr (SCALE >= 2) {
                    const int c = min(col + (quad ? 0 : e), n - 1);
                    x = GroupQ<SCALE == 3>::at(scale, O, r * G + c / gsize).dequant(x);
                }
                v[e] = PkOut<OUT>::cvt(x);
            }
            T *dst = out + r * n;
            if (ALIGNED && col + 3 < n) {
                *reinterpret_cast<V *>(dst + col) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < n) dst[col + e] = v[e];
            }
        }
    }
}

template <int SCALE, int OUT>
static void launch_dequantize(const unsigned *words, int R, int n, int b, Grid g, const float *scale, int gsize, const float *O,
                              void *out, hipStream_t s) {
    typedef typename PkOut<OUT>::T T;
    const size_t segs = (size_t)R * (((n + 31) / 32 + 7) / 8);
    const bool aligned = n % 4 == 0 && (uintptr_t)out % (4 * sizeof(T)) == 0;
    if (aligned)
        k_dequantize_packed<SCALE, OUT, true><<<pk_blocks(segs), 256, 0, s>>>(words, R, n, b, g, scale, gsize, O, static_cast<T *>(out));
    else
        k_dequantize_packed<SCALE, OUT, false><<<pk_blocks(segs), 256, 0, s>>>(words, R, n, b, g, scale, gsize, O, static_cast<T *>(out));
}

template <int SCALE>
static void launch_dequantize_out(int out_dtype, const unsigned *words, int R, int n, int b, Grid g, const float *scale, int gsize,
                                  const float *O, void *out, hipStream_t s) {
    if (out_dtype == SLK_DTYPE_BF16)
        launch_dequantize<SCALE, PK_BF16>(words, R, n, b, g, scale, gsize, O, out, s);
    else if (out_dtype == SLK_DTYPE_F16)
        launch_dequantize<SCALE, PK_F16>(words, R, n, b, g, scale, gsize, O, out, s);
    else
        launch_dequantize<SCALE, PK_F32>(words, R, n, b, g, scale, gsize, O, out, s);
}

}  // namespace slk

using namespace slk;

static inline size_t packed_words(int R, int n, int bits) { return (size_t)R * bits * ((n + 31) / 32); }

extern "C" {

int slk_pack_indices(const uint8_t *idx, int R, int n, int bits, uint32_t *words, slk_stream_t stream) {
    SLK_REQUIRE(bits >= 1 && bits <= 8, "bits must be in 1..8 (got %d)", bits);
    SLK_REQUIRE(R > 0 && n > 0, "bad shape (R = %d, n = %d)", R, n);
    SLK_REQUIRE(idx && words, "null pointer");
    hipStream_t s = as_stream(stream);
    const size_t segs = (size_t)R * (((n + 31) / 32 + 7) / 8);
    const double bytes = (double)R * n + 4.0 * packed_words(R, n, bits);
    if (n % 4 == 0 && (uintptr_t)idx % 4 == 0)
        SLK_RUN("pack_indices", 0, bytes, s, k_pack_indices<true><<<pk_blocks(segs), 256, 0, s>>>(idx, R, n, bits, words));
    else
        SLK_RUN("pack_indices", 0, bytes, s, k_pack_indices<false><<<pk_blocks(segs), 256, 0, s>>>(idx, R, n, bits, words));
    return SLK_OK;
}

int slk_unpack_indices(const uint32_t *words, int R, int n, int bits, uint8_t *idx, slk_stream_t stream) {
    SLK_REQUIRE(bits >= 1 && bits <= 8, "bits must be in 1..8 (got %d)", bits);
    SLK_REQUIRE(R > 0 && n > 0, "bad shape (R = %d, n = %d)", R, n);
    SLK_REQUIRE(idx && words, "null pointer");
    hipStream_t s = as_stream(stream);
    const size_t segs = (size_t)R * (((n + 31) / 32 + 7) / 8);
    const double bytes = (double)R * n + 4.0 * packed_words(R, n, bits);
    if (n % 4 == 0 && (uintptr_t)idx % 4 == 0)
        SLK_RUN("unpack_indices", 0, bytes, s, k_unpack_indices<true><<<pk_blocks(segs), 256, 0, s>>>(words, R, n, bits, idx));
    else
        SLK_RUN("unpack_indices", 0, bytes, s, k_unpack_indices<false><<<pk_blocks(segs), 256, 0, s>>>(words, R, n, bits, idx));
    return SLK_OK;
}

int slk_dequantize_packed(const uint32_t *words, int R, int n, int bits, int levels, double lo, double hi, const float *table,
                          const float *scale, const float *gscale, const float *goffset, int group_size, int out_dtype, void *out,
                          slk_stream_t stream) {
    SLK_REQUIRE(bits >= 1 && bits <= 8, "bits must be in 1..8 (got %d)", bits);
    SLK_REQUIRE(R > 0 && n > 0, "bad shape (R = %d, n = %d)", R, n);
    SLK_REQUIRE(words && out, "null pointer");
    SLK_REQUIRE(levels >= 2 && levels <= 256 && (table || lo < hi), "codebook needs 2 <= levels <= 256 and lo < hi");
    SLK_REQUIRE(!(scale && gscale), "scale and gscale are mutually exclusive");
    SLK_REQUIRE(!goffset || gscale, "goffset needs gscale");
    SLK_REQUIRE(!gscale || (group_size >= 1 && n % group_size == 0), "group_size must be >= 1 and divide n");
    SLK_REQUIRE(out_dtype == SLK_DTYPE_F32 || out_dtype == SLK_DTYPE_BF16 || out_dtype == SLK_DTYPE_F16, "unknown out_dtype %d",
                out_dtype);
    hipStream_t s = as_stream(stream);
    const Grid g = make_grid(levels, lo, hi, table);
    const double osz = out_dtype == SLK_DTYPE_F32 ? 4.0 : 2.0;
    const double side = gscale ? (goffset ? 8.0 : 4.0) * ((double)R * (n / group_size)) : (scale ? 4.0 * R : 0.0);
    const double bytes = 4.0 * packed_words(R, n, bits) + osz * R * n + side;
    if (goffset)
        SLK_RUN("dequantize_packed", 0, bytes, s, launch_dequantize_out<3>(out_dtype, words, R, n, bits, g, gscale, group_size, goffset, out, s));
    else if (gscale)
        SLK_RUN("dequantize_packed", 0, bytes, s, launch_dequantize_out<2>(out_dtype, words, R, n, bits, g, gscale, group_size, nullptr, out, s));
    else if (scale)
        SLK_RUN("dequantize_packed", 0, bytes, s, launch_dequantize_out<1>(out_dtype, words, R, n, bits, g, scale, 1, nullptr, out, s));
    else
        SLK_RUN("dequantize_packed", 0, bytes, s, launch_dequantize_out<0>(out_dtype, words, R, n, bits, g, nullptr, 1, nullptr, out, s));
    return SLK_OK;
}

}  // extern "C"
