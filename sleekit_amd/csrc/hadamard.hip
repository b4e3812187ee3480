// slk_hadamard_rows (and slk_mx_rotate_quantize_act / _act6, the same butterflies ending in the MX quantizer): Y = X R or X R^T, R = diag(s) blockdiag(H_block) / sqrt(block) (the contract: include/sleekit_amd.h).
//
// The map.  A row is cut into CHUNKS of 16 consecutive columns and a lane owns one chunk, so inside a block of `block`
// columns element i sits in lane i / 16 (counted from the block's first lane) at register i % 16:
//   strides 1, 2, 4, 8           registers of one lane (blocks below 16: a lane holds 16 / block whole blocks)
//   strides 16, 32, 64, 128      lane distances 1, 2, 4, 8: DPP on the vector ALU (quad_perm; half-mirror then reversed quads;
//                                row_ror:8)
//   strides 256, 512             lane distances 16 and 32: v_permlane16_swap / v_permlane32_swap (gfx950), VALU as well
//   strides 1024, 2048           the 2 or 4 waves of a block, through LDS: one exchange in which a lane reads the chunks of its
//                                one or three partner lanes and repeats their first stage itself (the same two operands in the
//                                same operation: the same bits)
// Chunks are numbered through the whole matrix (row * chunks-per-row + chunk), a workgroup of 256 lanes takes 256
// consecutive ones, in a grid that covers them all: a block's lanes are consecutive and aligned to their count because
// chunks-per-row is a multiple of block / 16, whatever the row.  The butterfly fixes which two values meet in each addition,
// so none of this shows in the result.
#include "common.h"
#include "hadamard.h"
#include "mxquant.h"

#include <math.h>

namespace slk {

constexpr int HD_CHUNK = 16;     // elements a lane
constexpr int HD_THREADS = 256;  // four waves: a block of 4096

// element types in memory: T is what the kernel holds them as
template <int D> struct HdType;
template <> struct HdType<SLK_DTYPE_F32> { typedef float T; };
template <> struct HdType<SLK_DTYPE_BF16> { typedef unsigned short T; };
template <> struct HdType<SLK_DTYPE_F16> { typedef _Float16 T; };
template <> struct HdType<SLK_DTYPE_F64> { typedef double T; };

__device__ __forceinline__ void hd_get(float &v, float x) { v = x; }
__device__ __forceinline__ void hd_get(float &v, unsigned short x) { v = __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ void hd_get(float &v, _Float16 x) { v = (float)x; }
__device__ __forceinline__ void hd_get(double &v, double x) { v = x; }
__device__ __forceinline__ void hd_put(float &y, float v) { y = v; }
__device__ __forceinline__ void hd_put(unsigned short &y, float v) { y = pk_bf16(v); }
__device__ __forceinline__ void hd_put(_Float16 &y, float v) { y = (_Float16)v; }
__device__ __forceinline__ void hd_put(double &y, double v) { y = v; }

// 16 elements as 16-byte pieces
template <class T>
struct alignas(16) HdPiece {
    T e[16 / sizeof(T)];
};

// Where a lane's chunk lies: chunks are numbered through the whole matrix, one trip, the grid covers every chunk.
struct HdChunk {
    size_t row;
    int col, count;  // first column, and how many of the 16 lie inside the row (0: a lane past the last chunk)
    bool live;
};
__device__ __forceinline__ HdChunk hd_chunk(size_t rows, int n, int t) {
    const int cpr = (n + HD_CHUNK - 1) / HD_CHUNK;
    const size_t total = rows * (size_t)cpr;
    const size_t g = (size_t)blockIdx.x * HD_THREADS + t;
    HdChunk k;
    k.live = g < total;
    k.row = k.live ? g / cpr : 0;
    k.col = k.live ? (int)(g - k.row * cpr) * HD_CHUNK : 0;
    k.count = k.live ? min(HD_CHUNK, n - k.col) : 0;
    return k;
}

// A lane's 16 elements and their signs (zeros and ones past the matrix).
// VEC: X and the signs start on 16 bytes and n is a multiple of 16, so every chunk is whole and moves in 16-byte pieces;
// otherwise element by element, the last chunk of a row cut at n (blocks below 16 only: a larger block makes n a multiple of 16).
template <class C, class XT, bool VEC>
__device__ __forceinline__ void hd_load(const XT *X, const float *__restrict__ signs, int n, const HdChunk k, C (&v)[HD_CHUNK],
                                        C (&s)[HD_CHUNK]) {
#pragma unroll
    for (int e = 0; e < HD_CHUNK; ++e) v[e] = (C)0, s[e] = (C)1;
    if constexpr (VEC) {
        if (k.live) {
            constexpr int PER = 16 / sizeof(XT);
            const HdPiece<XT> *src = reinterpret_cast<const HdPiece<XT> *>(X + k.row * n + k.col);
#pragma unroll
            for (int p = 0; p < HD_CHUNK / PER; ++p) {
                const HdPiece<XT> piece = src[p];
#pragma unroll
                for (int e = 0; e < PER; ++e) hd_get(v[p * PER + e], piece.e[e]);
            }
            if (signs) {
                const HdPiece<float> *sp = reinterpret_cast<const HdPiece<float> *>(signs + k.col);
#pragma unroll
                for (int p = 0; p < HD_CHUNK / 4; ++p) {
                    const HdPiece<float> piece = sp[p];
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[p * 4 + e] = (C)piece.e[e];
                }
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < HD_CHUNK; ++e)
            if (e < k.count) {
                hd_get(v[e], X[k.row * n + k.col + e]);
                if (signs) s[e] = (C)signs[k.col + e];
            }
    }
}

// The butterflies of a block of 2^lb over the lanes' chunks (step 2 of the contract), for every kernel that rotates.
// xch: (register, lane), so that a register's 256 values lie in consecutive banks; read for blocks above 1024 only.
template <class C>
__device__ __forceinline__ void hd_butterfly(C (&v)[HD_CHUNK], int lb, int t, C (*xch)[HD_THREADS]) {
    const int lane = t & 63;
    // strides 1 .. 8
    hd_register_stages(v, lb);
    // strides 16 .. 512: lanes of one wave (lb is uniform, and so is every branch here)
    if (lb > 4) hd_lane_stage<1>(v, lane);
    if (lb > 5) hd_lane_stage<2>(v, lane);
    if (lb > 6) hd_lane_stage<4>(v, lane);
    if (lb > 7) hd_lane_stage<8>(v, lane);
    if (lb > 8) hd_lane_stage<16>(v, lane);
    if (lb > 9) hd_lane_stage<32>(v, lane);
    // strides 1024 and 2048: waves of one workgroup
    if (lb > 10) {
#pragma unroll
        for (int e = 0; e < HD_CHUNK; ++e) xch[e][t] = v[e];
        __syncthreads();
        const bool up1 = t & 64, up2 = t & 128;
#pragma unroll
        for (int e = 0; e < HD_CHUNK; ++e) {
            const C p = xch[e][t ^ 64];
            const C mine = up1 ? p - v[e] : v[e] + p;
            if (lb > 11) {
                // the partner two waves away went through the same first stage with ITS neighbour
                const C q = xch[e][t ^ 128], r = xch[e][t ^ 192];
                const C theirs = up1 ? r - q : q + r;
                v[e] = up2 ? theirs - mine : mine + theirs;
            } else {
                v[e] = mine;
            }
        }
    }
}

// VEC: as in hd_load, and Y starts on 16 bytes too.
template <class C, class XT, class YT, bool VEC>
__global__ __launch_bounds__(HD_THREADS) static void k_hadamard_rows(const XT *X, YT *Y, size_t rows, int n,
                                                                      int lb, const float *__restrict__ signs, int transposed, C c) {
    // Dynamic: blocks up to 1024 get none.
    extern __shared__ __align__(16) unsigned char hd_lds[];
    C(*xch)[HD_THREADS] = reinterpret_cast<C(*)[HD_THREADS]>(hd_lds);
    const int t = threadIdx.x;
    const HdChunk k = hd_chunk(rows, n, t);
    C v[HD_CHUNK], s[HD_CHUNK];
    hd_load<C, XT, VEC>(X, signs, n, k, v, s);
    if (!transposed) {
#pragma unroll
        for (int e = 0; e < HD_CHUNK; ++e) v[e] = s[e] * v[e];
    }
    hd_butterfly(v, lb, t, xch);
#pragma unroll
    for (int e = 0; e < HD_CHUNK; ++e) {
        v[e] = v[e] * c;
        if (transposed) v[e] = s[e] * v[e];
    }
    if constexpr (VEC) {
        if (k.live) {
            constexpr int PER = 16 / sizeof(YT);
            HdPiece<YT> *dst = reinterpret_cast<HdPiece<YT> *>(Y + k.row * n + k.col);
#pragma unroll
            for (int p = 0; p < HD_CHUNK / PER; ++p) {
                HdPiece<YT> piece;
#pragma unroll
                for (int e = 0; e < PER; ++e) hd_put(piece.e[e], v[p * PER + e]);
                dst[p] = piece;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < HD_CHUNK; ++e)
            if (e < k.count) hd_put(Y[k.row * n + k.col + e], v[e]);
    }
}

// slk_mx_rotate_quantize_act: steps 1 to 3 of the transform (transposed == 0) with the MX activation quantizer as the
// epilogue, applied to the float32 value -- the bits of slk_hadamard_rows to float32 followed by slk_mx_quantize_act /
// _act4, without the float32 matrix in between.  n % 32 == 0, so a block of 32 is the chunks of an even lane and its right
// neighbour in one row: mxq_encode (mxquant.h) with 16 elements a lane, the even lane stores the scale byte, and each lane its 16 codes
// (16 bytes of E4M3, 8 of E2M1; 12 of E2M3, three aligned dwords of the row's bit stream: slk_mx_rotate_quantize_act6).
// Lanes past the matrix come in pairs too (rows * n / 16 is even) and carry zeros.
template <class XT, int FMT>
__global__ __launch_bounds__(HD_THREADS) static void k_hadamard_quantize(const XT *X, size_t rows, int n, int lb,
                                                                          const float *__restrict__ signs, float c,
                                                                          uint8_t *__restrict__ codes, uint8_t *__restrict__ E,
                                                                          int *__restrict__ flag) {
    extern __shared__ __align__(16) unsigned char hd_lds[];
    float(*xch)[HD_THREADS] = reinterpret_cast<float(*)[HD_THREADS]>(hd_lds);
    const int t = threadIdx.x;
    const HdChunk k = hd_chunk(rows, n, t);
    float v[HD_CHUNK], s[HD_CHUNK];
    hd_load<float, XT, true>(X, signs, n, k, v, s);
#pragma unroll
    for (int e = 0; e < HD_CHUNK; ++e) v[e] = s[e] * v[e];
    hd_butterfly(v, lb, t, xch);
#pragma unroll
    for (int e = 0; e < HD_CHUNK; ++e) v[e] = v[e] * c;
    unsigned eb, w[HD_CHUNK * mxa_bits<FMT>() / 32];
    const int top = mxq_encode<FMT>(v, eb, w);
    if (k.live) {
        const size_t at = k.row * n + k.col;  // a multiple of 16
        mxa_store<FMT, HD_CHUNK>(codes + mxa_byte_of<FMT>(at), w);
        if ((k.col & 16) == 0) E[at / 32] = (uint8_t)eb;
        if (top >= 0x7f800000) *flag = 1;
    }
}

template <class C, int XD, int YD>
static void launch_hadamard(const void *X, void *Y, long long rows, int n, int lb, const float *signs, int transposed, hipStream_t s) {
    typedef typename HdType<XD>::T XT;
    typedef typename HdType<YD>::T YT;
    const C c = (C)(1.0 / sqrt((double)(1 << lb)));
    const size_t total = (size_t)rows * (size_t)((n + HD_CHUNK - 1) / HD_CHUNK);
    const size_t need = (total + HD_THREADS - 1) / HD_THREADS;
    const unsigned grid = (unsigned)need;  // (the entry point refuses what does not fit one grid)
    const size_t lds = lb > 10 ? sizeof(C) * HD_CHUNK * HD_THREADS : 0;
    const bool vec = n % HD_CHUNK == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)signs % 16 == 0;
    if (vec)
        k_hadamard_rows<C, XT, YT, true><<<grid, HD_THREADS, lds, s>>>(static_cast<const XT *>(X), static_cast<YT *>(Y), (size_t)rows, n, lb,
                                                                     signs, transposed, c);
    else
        k_hadamard_rows<C, XT, YT, false><<<grid, HD_THREADS, lds, s>>>(static_cast<const XT *>(X), static_cast<YT *>(Y), (size_t)rows, n, lb,
                                                                      signs, transposed, c);
}

template <int XD>
static void launch_hadamard_out(int y_dtype, const void *X, void *Y, long long rows, int n, int lb, const float *signs, int transposed,
                                hipStream_t s) {
    if (y_dtype == SLK_DTYPE_BF16)
        launch_hadamard<float, XD, SLK_DTYPE_BF16>(X, Y, rows, n, lb, signs, transposed, s);
    else if (y_dtype == SLK_DTYPE_F16)
        launch_hadamard<float, XD, SLK_DTYPE_F16>(X, Y, rows, n, lb, signs, transposed, s);
    else
        launch_hadamard<float, XD, SLK_DTYPE_F32>(X, Y, rows, n, lb, signs, transposed, s);
}

static inline double hd_bytes(int dtype) { return dtype == SLK_DTYPE_F64 ? 8.0 : dtype == SLK_DTYPE_F32 ? 4.0 : 2.0; }

}  // namespace slk

using namespace slk;

// slk_mx_rotate_quantize_act (FMT MXA_E4M3, MXA_E2M1) and slk_mx_rotate_quantize_act6 (MXA_E2M3)
template <int FMT>
static int mx_rotate_quantize(const char *name, const void *X, int x_dtype, long long rows, int n, int block, const float *signs,
                              uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    SLK_REQUIRE(block >= 2 && block <= 4096 && (block & (block - 1)) == 0, "block must be a power of two in 2..4096 (got %d)", block);
    SLK_REQUIRE(rows > 0 && n >= 32 && n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (rows = %lld, n = %d)", rows, n);
    SLK_REQUIRE(n % block == 0, "block %d does not divide n = %d", block, n);
    SLK_REQUIRE(known_dtype(x_dtype), "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(X && a_codes && a_scales && flag, "null pointer");
    SLK_REQUIRE(aligned16(X) && aligned16(a_codes) && aligned16(signs), "X, signs and a_codes must be aligned to 16 bytes");
    SLK_REQUIRE(rows <= (long long)((~(size_t)0 >> 1) / (size_t)n / 8), "rows * n * 8 must fit the address space (rows = %lld, n = %d)", rows, n);
    SLK_REQUIRE((unsigned long long)rows * (unsigned long long)(n / HD_CHUNK) <= 0x7fffffffULL * HD_THREADS,
                "rows * n / 16 must not pass 2^31 - 1 workgroups of 256 chunks (rows = %lld, n = %d)", rows, n);
    hipStream_t s = as_stream(stream);
    int lb = 0;
    while ((1 << lb) < block) ++lb;
    zero_async(flag, sizeof(int), s);
    const float c = (float)(1.0 / sqrt((double)(1 << lb)));
    const size_t total = (size_t)rows * (size_t)(n / HD_CHUNK);
    const unsigned grid = (unsigned)((total + HD_THREADS - 1) / HD_THREADS);  // (what does not fit one grid is refused above)
    const size_t lds = lb > 10 ? sizeof(float) * HD_CHUNK * HD_THREADS : 0;
    const double elems = (double)rows * n;
    const double flops = elems * (lb + 1), bytes = elems * (hd_bytes(x_dtype) + mxa_block_bytes<FMT>() / 32.0);
    return with_dtype(x_dtype, [&](auto t) -> int {
        typedef typename decltype(t)::T XT;
        SLK_RUN(name, flops, bytes, s,
                (k_hadamard_quantize<XT, FMT><<<grid, HD_THREADS, lds, s>>>(static_cast<const XT *>(X), (size_t)rows, n, lb, signs, c, a_codes, a_scales, flag)));
        return SLK_OK;
    });
}

extern "C" {

int slk_hadamard_rows(const void *X, int x_dtype, void *Y, int y_dtype, long long rows, int n, int block, const float *signs,
                      int transposed, slk_stream_t stream) {
    SLK_REQUIRE(block >= 2 && block <= 4096 && (block & (block - 1)) == 0, "block must be a power of two in 2..4096 (got %d)", block);
    SLK_REQUIRE(rows > 0 && n > 0, "bad shape (rows = %lld, n = %d)", rows, n);
    SLK_REQUIRE(n % block == 0, "block %d does not divide n = %d", block, n);
    SLK_REQUIRE(X && Y, "null pointer");
    SLK_REQUIRE(x_dtype >= SLK_DTYPE_F32 && x_dtype <= SLK_DTYPE_F64, "unknown x_dtype %d", x_dtype);
    SLK_REQUIRE(y_dtype >= SLK_DTYPE_F32 && y_dtype <= SLK_DTYPE_F64, "unknown y_dtype %d", y_dtype);
    SLK_REQUIRE((x_dtype == SLK_DTYPE_F64) == (y_dtype == SLK_DTYPE_F64), "float64 goes to float64 and nothing else does (x_dtype %d, y_dtype %d)",
                x_dtype, y_dtype);
    SLK_REQUIRE(rows <= (long long)((~(size_t)0 >> 1) / (size_t)n / 8), "rows * n * 8 must fit the address space (rows = %lld, n = %d)", rows, n);
    SLK_REQUIRE((unsigned long long)rows * (unsigned long long)((n + HD_CHUNK - 1) / HD_CHUNK) <= 0x7fffffffULL * HD_THREADS,
                "rows * ceil(n / 16) must not pass 2^31 - 1 workgroups of 256 chunks (rows = %lld, n = %d)", rows, n);
    hipStream_t s = as_stream(stream);
    int lb = 0;
    while ((1 << lb) < block) ++lb;
    const double elems = (double)rows * n;
    const double flops = elems * (lb + 1), bytes = elems * (hd_bytes(x_dtype) + hd_bytes(y_dtype));
    if (x_dtype == SLK_DTYPE_F64)
        SLK_RUN("hadamard_rows", flops, bytes, s, (launch_hadamard<double, SLK_DTYPE_F64, SLK_DTYPE_F64>(X, Y, rows, n, lb, signs, transposed, s)));
    else if (x_dtype == SLK_DTYPE_BF16)
        SLK_RUN("hadamard_rows", flops, bytes, s, launch_hadamard_out<SLK_DTYPE_BF16>(y_dtype, X, Y, rows, n, lb, signs, transposed, s));
    else if (x_dtype == SLK_DTYPE_F16)
        SLK_RUN("hadamard_rows", flops, bytes, s, launch_hadamard_out<SLK_DTYPE_F16>(y_dtype, X, Y, rows, n, lb, signs, transposed, s));
    else
        SLK_RUN("hadamard_rows", flops, bytes, s, launch_hadamard_out<SLK_DTYPE_F32>(y_dtype, X, Y, rows, n, lb, signs, transposed, s));
    return SLK_OK;
}

int slk_mx_rotate_quantize_act(const void *X, int x_dtype, long long rows, int n, int block, const float *signs, int fmt,
                               uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream) {
    SLK_REQUIRE(fmt == SLK_MX_ACT_FP8 || fmt == SLK_MX_ACT_FP4, "unknown fmt %d", fmt);
    const auto body = fmt == SLK_MX_ACT_FP4 ? mx_rotate_quantize<MXA_E2M1> : mx_rotate_quantize<MXA_E4M3>;
    return body("mx_rotate_quantize_act", X, x_dtype, rows, n, block, signs, a_codes, a_scales, flag, stream);
}

int slk_mx_rotate_quantize_act6(const void *X, int x_dtype, long long rows, int n, int block, const float *signs, uint8_t *a_codes,
                                uint8_t *a_scales, int *flag, slk_stream_t stream) {
    return mx_rotate_quantize<MXA_E2M3>("mx_rotate_quantize_act6", X, x_dtype, rows, n, block, signs, a_codes, a_scales, flag, stream);
}

}  // extern "C"
