// float32 MFMA products on the path:
//   a11  channelwise_error (sleekit/obq.py:89-95): row_err = rowsum(((W-Q) @ H) * (W-Q))
//   a1   Sleekit.add_batch (sleekit/statistics.py:76-87): H = H f + X^T X / c'
//        and, for the E experts of a mixture in one call, slk_hessian_accumulate_experts (float rows) and
//        slk_hessian_accumulate_experts_mx (MX-coded rows: one bfloat16 MFMA pass over the decoded codes)
// Both are dense contractions on v_mfma_f32_32x32x2_f32 through mfma32.h.
#include <stdlib.h>

#include <algorithm>

#include "mfma32.h"
#include "mfma_bf16x3.h"
#include "mxquant.h"

namespace slk {

// ------------------------------------------------------------------ row errors
// Tile (rows r0.., cols j0..) of G = D @ H with D = W - Q formed on load.  The epilogue
// multiplies by D again and reduces each row over the tile's 128 columns in a fixed
// order (lane tree, then the two column waves); partial[r][tile] goes to scratch and a
// second kernel adds the tiles left to right, so results are run-to-run identical.
using HPtrs = PtrTable;  // the Hessians of a batch of layers stacked by rows

// The epilogue of both error kernels, for the tile at (r0, j0): rowpart[wc][row] = the sum over column wave wc's 64 columns
// of acc * (W - Q); G, when given, receives acc.  The order of additions per row is fixed: 0 + acc d for column block 0,
// then block 1, then the lane tree xor 16 ... xor 1 (and row_sums_store adds the two column waves).  GUARD: the columns at
// or past n count for nothing (n % 128 != 0).
// The 32 differences W - Q of a half of the sub-tile are fetched TOGETHER -- rows beyond R (GUARD: columns beyond n) read the
// last one and count for nothing --, then the sixteen row sums go down the lane tree side by side.  Row by row -- four loads,
// a wait, five dependent shuffles each -- the tail of a tile was 32 trips to memory one behind the other.
template <bool GUARD>
__device__ __forceinline__ void row_sums(const Acc128 &acc, const float *__restrict__ W, const float *__restrict__ Q,
                                         float *__restrict__ G, int R, int n, int r0, int j0, float (&rowpart)[2][T32]) {
    const int wc = (threadIdx.x >> 6) & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float dd[16][2], sv[16];
        // (plain loops over tile128_row: handed out through a lambda that captures W, Q and G, the compiler no longer
        // proves the store to G apart from the loads behind it and waits for every pair of loads on its own)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile128_row(i, r);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = j0 + tile128_col(j);
                const bool live = r0 + row < R && (!GUARD || col < n);
                const size_t o = (size_t)min(r0 + row, R - 1) * n + (GUARD ? min(col, n - 1) : col);
                dd[r][j] = W[o] - Q[o];
                if (G && live) G[o] = acc.c[i][j][r];
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float sacc = 0.0f;
            if (r0 + tile128_row(i, r) < R) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (!GUARD || j0 + tile128_col(j) < n) sacc = sacc + acc.c[i][j][r] * dd[r][j];
            }
            sv[r] = sacc;
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1)
#pragma unroll
            for (int r = 0; r < 16; ++r) sv[r] = sv[r] + __shfl_xor(sv[r], m, 64);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if ((threadIdx.x & 31) == 0) rowpart[wc][tile128_row(i, r)] = sv[r];
    }
}
// ... and the tile's row sums to their slot of the scratch
__device__ __forceinline__ void row_sums_store(const float (&rowpart)[2][T32], float *__restrict__ partial, int R, int r0, int p_stride,
                                               int slot) {
    __syncthreads();
    if (threadIdx.x < T32 && r0 + threadIdx.x < R)
        partial[(size_t)(r0 + threadIdx.x) * p_stride + slot] = rowpart[0][threadIdx.x] + rowpart[1][threadIdx.x];
}

__global__ __launch_bounds__(256) void k_error_tiles(const float *__restrict__ W, const float *__restrict__ Q,
                                                     const HPtrs hs, int R, int n,
                                                     float *__restrict__ G, float *__restrict__ partial,
                                                     int n_tiles, int vec_ok, const int *__restrict__ sym_flag,
                                                     int bf16_takes_sym, int p_stride, int rpl) {
    __shared__ Tile128Smem sm;
    __shared__ float rowpart[2][T32];
    // Column tiles are rotated by the row-tile index: with the symmetric shortcut below a tile's
    // depth grows with its column, and blocks id, id + 256, ... (same CU) must not all be deep.
    // XCD-aware tile order.  Workgroup i runs on XCD i % 8; each XCD has its own L2.  XCD x takes a
    // contiguous run of the row-major tile list (for a square 4096 layer: four row tiles by all
    // 32 column tiles = its 128 resident workgroups), so its L2 holds 4 row panels of W - Q and one
    // sweep of H instead of every XCD streaming every panel (2.8 GB past the L2 per launch before).
    // Within a row the column is rotated with the row and mirrored on odd rows: with the symmetric
    // shortcut below a tile's depth grows with its column, and the workgroups that share a CU
    // (i, i + 256, ...) must not all be deep.
    const int n_rt = (R + T32 - 1) / T32, n_all = n_tiles * n_rt;
    const int per_xcd = (n_all + 7) / 8;
    const int lin = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (lin >= n_all) return;
    const int tile_y = lin / n_tiles, in_row = lin - tile_y * n_tiles;
    const int rot = (in_row + tile_y * max(1, n_tiles / 4)) % n_tiles;
    const int tile_x = (tile_y & 1) ? n_tiles - 1 - rot : rot;
    const int r0 = tile_y * T32, j0 = tile_x * T32;
    const int layer = r0 / rpl;  // rows [b rpl, (b + 1) rpl) belong to layer b (rpl a multiple of the tile when there are several)
    const float *__restrict__ H = hs.p[layer];
    if (sym_flag) sym_flag += layer;
    const int t = threadIdx.x;
    Acc128 acc;
    acc.zero();
    const int kfull = (n + K32 - 1) / K32 * K32;
    // H symmetric (checked bit-wise on the device) and G not wanted:
    //   sum_k D_k H_kj over all k  ==  2 * sum_{k < j0} + the 128-wide diagonal band, after the
    //   final multiplication by D_j and the sum over j.  Halves the flops of the layer error.
    const bool sym = sym_flag != nullptr && sym_flag[0] > 0;  // (a negative verdict = unknown: the general route)
    if (sym && bf16_takes_sym) return;  // (that layer's rows are the bfloat16 kernel's)
    const int kend = sym ? min(j0 + T32, kfull) : kfull;
    const int ksplit = sym ? j0 : 0;  // [0, ksplit) counted twice
    const int a_row = r0 + (t >> 1), a_k = (t & 1) * 8;  // A: D = W - Q, K contiguous
    const int b_k = t >> 4, b_col = j0 + (t & 15) * 8;   // B: H, columns contiguous
    // the rows under the band, twice, then the band -- over whichever pair of loaders applies
    auto product = [&](auto la, auto lb) {
        if (ksplit > 0) {
            tile128_mac<true, true>(acc, sm, 0, ksplit, la, lb);
            acc.scale(2.0f);
            __syncthreads();
        }
        tile128_mac<true, true>(acc, sm, ksplit, kend, la, lb);
    };
    if (vec_ok && r0 + T32 <= R && j0 + T32 <= n && kfull == n) {
        // interior tile: unconditional 16-byte loads
        const float *pw = W + (size_t)a_row * n + a_k, *pq = Q + (size_t)a_row * n + a_k;
        const float *ph = H + (size_t)b_k * n + b_col;
        auto la = [&](int k0, float(&v)[8]) {
            float w[8], q[8];
            load8<true>(pw + k0, w);
            load8<true>(pq + k0, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w[e] - q[e];
        };
        auto lb = [&](int k0, float(&v)[8]) { load8<true>(ph + (size_t)k0 * n, v); };
        product(la, lb);
    } else {
        const bool row_ok = a_row < R;
        const size_t arow = (size_t)min(a_row, R - 1) * n;
        auto la = [&](int k0, float(&v)[8]) {
            const int k = min(k0 + a_k, n - 1), last = n - 1 - (k0 + a_k);
            float w[8], q[8];
            load8_guarded(W + arow + k, last, row_ok, w);
            load8_guarded(Q + arow + k, last, row_ok, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = w[e] - q[e];
        };
        auto lb = [&](int k0, float(&v)[8]) {
            const int k = k0 + b_k;
            load8_guarded(H + (size_t)min(k, n - 1) * n + min(b_col, n - 1), n - 1 - b_col, k < n, v);
        };
        product(la, lb);
    }
    row_sums<true>(acc, W, Q, G, R, n, r0, j0, rowpart);
    row_sums_store(rowpart, partial, R, r0, p_stride, tile_x);
}

// x (or x - y when y is given), rows x n row-major -> its three bfloat16 pieces in the GEMM's own order:
// plane p at out + p * plane, and inside a plane the slab (128-row block rb, 32-deep k step ks) is one
// contiguous 8 KB run, [row in block][32 k] -- what a workgroup of k_error_tiles_bf16 loads per round, so
// its 16-byte loads walk memory linearly (row-major planes gave 64 contiguous bytes per row and round).
// Rows beyond `rows` in the last block repeat the last row (never stored by the GEMM).  n % 32 == 0.
// One pass at HBM speed; it takes all the splitting arithmetic out of the GEMM, where every element
// would otherwise be split once per tile that uses it (32 times at n = 4096).
// blockIdx.y: the layer of a stack (its own x, flag and planes: out + blockIdx.y * 3 * plane); one launch for a round's
// Hessians -- eight 4 MB matrices split one by one are eight launches of 17 us each, bound by nothing but their number.
// swz: the 16-byte chunks of a row swizzled for global_load_lds (tile128_mac_bf16<true>).
__global__ __launch_bounds__(256) void k_split3(PtrTable xs, const float *__restrict__ y, int rows, int n,
                                                unsigned short *__restrict__ out, size_t plane,
                                                const int *__restrict__ sym_flag, int swz, int band_only, int average) {
    const float *__restrict__ x = xs.p[blockIdx.y];
    out += (size_t)blockIdx.y * 3 * plane;
    // `average`: a square matrix that is NOT symmetric is split as (x + x^T) / 2 -- the quadratic form d x d^T, which is all
    // the layer error wants of it, is the same for both, and the symmetric half-product route then serves every Hessian
    // (the second read is a column gather: twice the time of this pass, a tenth of the products it saves)
    const bool avg = average && sym_flag && sym_flag[blockIdx.y] <= 0;
    if (sym_flag && sym_flag[blockIdx.y] <= 0 && !avg) return;
    const int ksteps = n / 32;
    const size_t quads = plane / 4;  // groups of four consecutive k
    for (size_t qd = (size_t)blockIdx.x * blockDim.x + threadIdx.x; qd < quads; qd += (size_t)gridDim.x * blockDim.x) {
        const size_t e = qd * 4;                      // position in the plane
        const size_t slab = e >> 12;                  // rb * ksteps + ks
        const int k4 = (int)(e & 31), r = (int)((e >> 5) & 127);
        const int ks = (int)(slab % ksteps), rb = (int)(slab / ksteps);
        // (a symmetric H whose error alone is wanted: tile column rb of the GEMM reads the k steps up to its diagonal
        // band only, k < 128 (rb + 1) -- the other half of the plane is never looked at)
        if (band_only && ks >= 4 * (rb + 1)) continue;
        const int row = min(rb * 128 + r, rows - 1);
        const int kcol = ks * 32 + k4;
        const size_t src = (size_t)row * n + kcol;
        float4_t v = *reinterpret_cast<const float4_t *>(x + src);
        if (avg) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = 0.5f * (v[c] + x[(size_t)(kcol + c) * n + row]);
        }
        if (y) {
            const float4_t u = *reinterpret_cast<const float4_t *>(y + src);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = v[c] - u[c];
        }
        unsigned w[3][2];
        split3_pair(v[0], v[1], w[0][0], w[1][0], w[2][0]);
        split3_pair(v[2], v[3], w[0][1], w[1][1], w[2][1]);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            // (swz: the 16-byte chunk moves inside its row, see swizzled_chunk)
            const size_t eo = swz ? (e & ~(size_t)31) + (size_t)(swizzled_chunk(r, k4 >> 3) * 8 + (k4 & 7)) : e;
            unsigned *o = reinterpret_cast<unsigned *>(out + (size_t)p * plane + eo);
            o[0] = w[p][0];
            o[1] = w[p][1];
        }
    }
}

// The symmetric case on the bfloat16 MFMA (mfma_bf16x3.h): same tile order, same epilogue, the product
// emulated to float32 grade with six bfloat16 terms from operands split by k_split3.  Runs only when the
// device-side flag says H is symmetric (its rows then serve as the K-contiguous B operand) -- the float32
// kernel above takes the other case; each returns at once when the flag is not its own.  n % 128 == 0.
template <bool DMA>
__global__ __launch_bounds__(256) void k_error_tiles_bf16(const float *__restrict__ W, const float *__restrict__ Q,
                                                          const unsigned short *__restrict__ Dp,
                                                          const unsigned short *__restrict__ Hp, int R, int n,
                                                          float *__restrict__ partial, int n_tiles,
                                                          const int *__restrict__ sym_flag, int p_stride, int cb, int rpl,
                                                          float *__restrict__ G, int asym_mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];  // TileBf16<DMA>
    __shared__ float rowpart[2][T32];
    // XCD-aware tile order, column-major inside the XCD.  Workgroup i runs on XCD i % 8 (own L2).  XCD x takes
    // the row tiles [x rpx, (x + 1) rpx) (rpx = 4 for a 4096-row layer) and walks the column tiles in the order
    // `rank`; its slot s = rank * rpx + row, so the workgroups resident together (two per CU, 64 per XCD) are
    // ALL the band's rows times 16 column tiles: an H slab is fetched once and serves every row of the band, the
    // band's own D slabs stay in L2.  (Row-major slots left only two of the four rows resident at a time and
    // cost 1.9 GB past the L2 per launch.)  The column ranks go up and down the depths in groups of 8 so that
    // the tiles a CU gets over time (slots s, s + 32, ...) add up to the same depth.
    //
    // Few rows (a row shard of a multi-GPU run): the tiles alone do not fill the chip and the deepest one is the
    // whole critical path, so K is cut into chunks of `cb` 128-blocks (cb > 0) and a tile of depth d = tile_x + 1
    // blocks becomes ceil(d / cb) workgroups, each with its own slot of partial sums.  Workgroup order: the row
    // tiles of one (column tile, chunk) are neighbours, so the H slabs they share are fetched once.
    const int n_rt = (R + T32 - 1) / T32;
    int tile_x, tile_y, p_slot, blk_lo, blk_hi;  // blocks [blk_lo, blk_hi) of K; block tile_x is the diagonal band
    if (cb > 0) {
        tile_y = blockIdx.x % n_rt;
        int sl = blockIdx.x / n_rt;
        p_slot = sl;
        tile_x = 0;
        while (tile_x < n_tiles && sl >= (tile_x + cb) / cb) {
            sl -= (tile_x + cb) / cb;
            ++tile_x;
        }
        if (tile_x >= n_tiles) return;
        blk_lo = sl * cb;
        blk_hi = min(blk_lo + cb, tile_x + 1);
    } else {
        const int rpx = (n_rt + 7) / 8, per_xcd = rpx * n_tiles;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        if (slot >= per_xcd) return;
        const int rank = slot / rpx;
        tile_y = xcd * rpx + (slot - rank * rpx);
        if (tile_y >= n_rt) return;
        const int grp = rank >> 3, in_grp = rank & 7;
        const int g_lo = grp * 8, g_hi = min(n_tiles, g_lo + 8) - 1;
        tile_x = (grp & 1) ? g_hi - in_grp : g_lo + in_grp;
        if (tile_x < g_lo || tile_x > g_hi) return;  // a last group shorter than 8
        p_slot = tile_x;
        blk_lo = 0;
        blk_hi = tile_x + 1;
    }
    const int r0 = tile_y * T32, j0 = tile_x * T32;
    // a batch of layers stacked by rows (rpl rows each, a multiple of the tile): layer b has its own flag and planes of H
    const int layer = r0 / rpl;
    // H not symmetric (or not known to be): its planes then hold H^T (k_split3_transposed), every k is multiplied and
    // nothing counted twice -- when the caller asked for that (asym_mode); otherwise those rows are the float32 kernel's
    const bool full_k = G != nullptr || (sym_flag[layer] <= 0 && asym_mode != 2);  // (2: the planes hold (H + H^T) / 2)
    if (sym_flag[layer] <= 0 && !asym_mode) return;
    Hp += (size_t)layer * 3 * n * n;
    Acc128 acc;
    acc.zero();
    const int ksteps = n / 32;
    const size_t d_plane = (size_t)n_rt * T32 * n, h_plane = (size_t)n * n;
    const unsigned short *a_slabs = Dp + (size_t)tile_y * ksteps * 4096, *b_slabs = Hp + (size_t)tile_x * ksteps * 4096;
    auto product = [&](int k_begin, int k_end) { tile128_mac_bf16<DMA>(acc, smem_raw, k_begin, k_end, a_slabs, d_plane, b_slabs, h_plane); };
    // sum_k D_k H_kj over all k == 2 * sum_{k < j0} + the 128-wide diagonal band (see k_error_tiles)
    const int k_lo = blk_lo * T32, k_below = min(blk_hi * T32, j0);  // [k_lo, k_below) lies under the band: twice
    if (full_k) {
        // the product itself is wanted (local search: G = (W - Q) H, obq.py:231), or H is not symmetric: every k, nothing
        // counted twice
        product(0, n);
    } else if (k_below > k_lo) {
        product(k_lo, k_below);
        acc.scale(2.0f);
        __syncthreads();
    }
    if (!full_k && blk_hi == tile_x + 1) product(j0, j0 + T32);
    row_sums<false>(acc, W, Q, G, R, n, r0, j0, rowpart);
    row_sums_store(rowpart, partial, R, r0, p_stride, p_slot);
}

// H[i][j .. j + 3] of an n x n matrix, zeros beyond it; vec: one 16-byte load where all four are inside
__device__ __forceinline__ float4_t load4_inside(const float *__restrict__ H, int n, bool vec, int i, int j) {
    float4_t v = (float4_t){0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) {
        if (vec && j + 3 < n) {
            v = *reinterpret_cast<const float4_t *>(H + (size_t)i * n + j);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < n) v[e] = H[(size_t)i * n + j + e];
        }
    }
    return v;
}

// flag[0] = 1 iff H is bit-wise symmetric (flag must be preset to 1).  One workgroup per pair of mirrored
// 64 x 64 tiles (a triangular list of pairs): tile (bi, bj) goes to LDS through coalesced 16-byte loads, tile
// (bj, bi) is read the same way and compared with the transpose out of LDS -- every element is read once.
__global__ __launch_bounds__(256) void k_symmetry_flag(PtrTable hs, int n, int *__restrict__ flag) {
    __shared__ float tile[64][65];
    const float *__restrict__ H = hs.p[blockIdx.y];  // blockIdx.y: the layer of a stack, with a flag of its own
    flag += blockIdx.y;
    int bi, bj;  // pair index -> (bi >= bj)
    lower_tile(blockIdx.x, bi, bj);
    const int t = threadIdx.x, c4 = (t & 15) * 4, r_first = t >> 4;  // 16 threads x 16 bytes per row, 16 rows per pass
    const bool vec = n % 4 == 0 && (uintptr_t)H % 16 == 0;
    bool ok = true;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = r_first + 16 * p;
        const float4_t v = load4_inside(H, n, vec, bi * 64 + r, bj * 64 + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r][c4 + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = r_first + 16 * p, i = bj * 64 + r, j = bi * 64 + c4;  // the mirrored tile, read row-wise
        if (i >= n) continue;
        const float4_t v = load4_inside(H, n, vec, i, j);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < n) ok = ok && (__float_as_int(v[e]) == __float_as_int(tile[c4 + e][r]));
    }
    if (!ok) flag[0] = 0;
}

__global__ void k_set_flag(int *flag, int v, int count) {
    if ((int)threadIdx.x < count) flag[threadIdx.x] = v;
}

__global__ __launch_bounds__(256) void k_error_reduce(const float *__restrict__ partial, int R, int n_tiles,
                                                      float *__restrict__ row_err) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float s = 0.0f;
    for (int t = 0; t < n_tiles; ++t) s = s + partial[(size_t)r * n_tiles + t];
    row_err[r] = s;
}

// ------------------------------------------------------------------ Hessian accumulation
// The bodies of the four kernels are functions of (operand, row count, tile, factor, count): the single-layer kernels call
// them with their arguments, the expert-grouped ones (further down) with an expert's slice and the factor and count the
// prologue formed for it -- the same steps in the same order, so an expert's statistics are the single call's bit for bit.
//
// One entry of the running update, mirrored: H[i][j] = H[j][i] = fl(fl(H[i][j] f) + fl(v / cnt)).
__device__ __forceinline__ void hessian_store(float *__restrict__ H, int n, int i, int j, float v, float factor, float count) {
    const float h = H[(size_t)i * n + j] * factor + v / count;
    H[(size_t)i * n + j] = h;
    if (i != j) H[(size_t)j * n + i] = h;
}
// ... and the lower tile (bi, bj) of them from its accumulators: inside the matrix, and on a diagonal tile at or under the
// diagonal only (the mirror writes the rest).
// (The 64 read-modify-writes of a thread come out as 64 load -> wait -> store round trips one behind the other; fetching
// the old values first was measured on the bfloat16 kernel: 310 against 300 us per 2048 tokens -- 256 VGPRs, and two
// workgroups per CU hide the tail as it is.)
__device__ __forceinline__ void hessian_store_tile(const Acc128 &acc, float *__restrict__ H, int n, int bi, int bj, float factor,
                                                   float count) {
    tile128_foreach(acc, [&](int r, int c, float v) {
        const int i = bi * T32 + r, j = bj * T32 + c;
        if (i < n && j < n && (bi != bj || j <= i)) hessian_store(H, n, i, j, v, factor, count);
    });
}

// Lower tile (bi, bj) of X^T X, mirrored on store so H stays exactly symmetric.
__device__ __forceinline__ void hessian_tile_f32(Tile128Smem &sm, float *__restrict__ H, const float *__restrict__ X, int n, int T,
                                                 int bi, int bj, float factor, float count, int vec_ok) {
    const int i0 = bi * T32, j0 = bj * T32;
    const int t = threadIdx.x;
    Acc128 acc;
    acc.zero();
    const int kend = (T + K32 - 1) / K32 * K32;
    // both operands are rows of X (tokens x features): A[r][k] = X[k][i0 + r], B[k][c] = X[k][j0 + c]
    const int x_k = t >> 4, a_col = i0 + (t & 15) * 8, b_col = j0 + (t & 15) * 8;
    if (vec_ok && i0 + T32 <= n && kend == T) {  // j0 <= i0, so the B tile is interior too
        const float *pa = X + (size_t)x_k * n + a_col, *pb = X + (size_t)x_k * n + b_col;
        tile128_mac<false, true>(
            acc, sm, 0, kend, [&](int k0, float(&v)[8]) { load8<true>(pa + (size_t)k0 * n, v); },
            [&](int k0, float(&v)[8]) { load8<true>(pb + (size_t)k0 * n, v); });
    } else {
        tile128_mac<false, true>(
            acc, sm, 0, kend,
            [&](int k0, float(&v)[8]) {
                const int k = k0 + x_k;
                load8_guarded(X + (size_t)min(k, T - 1) * n + min(a_col, n - 1), n - 1 - a_col, k < T, v);
            },
            [&](int k0, float(&v)[8]) {
                const int k = k0 + x_k;
                load8_guarded(X + (size_t)min(k, T - 1) * n + min(b_col, n - 1), n - 1 - b_col, k < T, v);
            });
    }
    // (hessian_store_tile written out: through the shared function k_hessian_tiles_experts compiled to another epilogue and
    // was measured 1.8 % slower where an expert has a hundred rows -- DESIGN.md section 29)
    tile128_foreach(acc, [&](int r, int c, float v) {
        const int i = i0 + r, j = j0 + c;
        if (i < n && j < n && (bi != bj || j <= i)) hessian_store(H, n, i, j, v, factor, count);
    });
}
__global__ __launch_bounds__(256) void k_hessian_tiles(float *__restrict__ H, const float *__restrict__ X, int n, int T,
                                                       float factor, float count, int vec_ok) {
    __shared__ Tile128Smem sm;
    if (blockIdx.x > blockIdx.y) return;
    hessian_tile_f32(sm, H, X, n, T, blockIdx.y, blockIdx.x, factor, count, vec_ok);
}

// X (T x n, tokens x features) -> the three bfloat16 pieces of its TRANSPOSE in the GEMM's slab order: slab
// (128-feature block ib, 32-token step ks) is [feature in block][32 tokens], contiguous; tokens beyond T are
// zero.  One workgroup per slab: 32 coalesced rows of 128 floats in, through LDS, 8 KB per plane out.
typedef float Split3Tile[32][T32 + 1];
// slab (ib, ks) of X's planes, `ksteps` slabs a feature block
__device__ __forceinline__ void split3_transposed_slab(Split3Tile &tile, const float *__restrict__ X, int n, int T, int t_first, int t_count,
                                                       unsigned short *__restrict__ out, size_t plane, int swz, int ib, int ks, int ksteps) {
    const int t = threadIdx.x;
    for (int e = t; e < 32 * T32; e += 256) {
        const int tt = e >> 7, ii = e & 127;
        const int tok = t_first + ks * 32 + tt;
        tile[tt][ii] = (ks * 32 + tt < t_count && tok < T) ? X[(size_t)tok * n + ib * T32 + ii] : 0.0f;
    }
    __syncthreads();
    const int ii = t >> 1, half = (t & 1) * 16;
    unsigned w[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) split3_pair(tile[half + 2 * e][ii], tile[half + 2 * e + 1][ii], w[0][e], w[1][e], w[2][e]);
    const size_t slab = ((size_t)ib * ksteps + ks) * 4096 + (size_t)ii * 32;
    const int c0 = (t & 1) * 2;  // this thread's two 16-byte chunks of the row
    const int p0 = swz ? swizzled_chunk(ii, c0) : c0, p1 = swz ? swizzled_chunk(ii, c0 + 1) : c0 + 1;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        unsigned short *o = out + p * plane + slab;
        *reinterpret_cast<uint4v_t *>(o + p0 * 8) = (uint4v_t){w[p][0], w[p][1], w[p][2], w[p][3]};
        *reinterpret_cast<uint4v_t *>(o + p1 * 8) = (uint4v_t){w[p][4], w[p][5], w[p][6], w[p][7]};
    }
}
__global__ __launch_bounds__(256) void k_split3_transposed(PtrTable xs, int n, int T, int t_first, int t_count,
                                                           unsigned short *__restrict__ out, size_t plane, int swz,
                                                           const int *__restrict__ skip_if_symmetric) {
    __shared__ Split3Tile tile;
    // blockIdx.z: the layer of a stack (its own X, flag and planes)
    if (skip_if_symmetric && skip_if_symmetric[blockIdx.z] > 0) return;  // (the layer error: a symmetric H is split as it stands)
    split3_transposed_slab(tile, xs.p[blockIdx.z], n, T, t_first, t_count, out + (size_t)blockIdx.z * 3 * plane, plane, swz, blockIdx.x, blockIdx.y,
                           gridDim.y);
}

// Lower tiles of X^T X on the bfloat16 MFMA (mfma_bf16x3.h), from the planes of k_split3_transposed; same
// epilogue as k_hessian_tiles.  Tiles of the lower triangle in an XCD-aware order (see k_syrk_triangle): `block` of the
// launch's 8 * ceil(total / 8) workgroups.
template <bool DMA>
__device__ __forceinline__ void hessian_tile_bf16(unsigned char *smem_raw, float *__restrict__ H, const unsigned short *__restrict__ Xp, int n,
                                                  int ksteps, size_t plane, int block, float factor, float count) {
    const int m = n / T32, total = m * (m + 1) / 2, per_xcd = (total + 7) / 8;
    const int lin = (block & 7) * per_xcd + (block >> 3);
    if (lin >= total) return;
    int bi, bj;
    lower_tile(lin, bi, bj);
    Acc128 acc;
    acc.zero();
    tile128_mac_bf16<DMA>(acc, smem_raw, 0, ksteps * 32, Xp + (size_t)bi * ksteps * 4096, plane, Xp + (size_t)bj * ksteps * 4096, plane);
    hessian_store_tile(acc, H, n, bi, bj, factor, count);
}
template <bool DMA>
__global__ __launch_bounds__(256) void k_hessian_tiles_bf16(float *__restrict__ H, const unsigned short *__restrict__ Xp, int n,
                                                            int ksteps, size_t plane, float factor, float count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    hessian_tile_bf16<DMA>(smem_raw, H, Xp, n, ksteps, plane, blockIdx.x, factor, count);
}

// mean[j] = mean[j] * factor + (sum over the T tokens of X[t][j]) / count  (statistics.py:76-87).
// One workgroup per 32 features: 8 token groups x 32 features, each thread walks its tokens t = g, g + 8, ... with four
// running sums (128-byte row segments, loads independent of one another), then a fixed-order reduction through LDS.
// (One thread per feature walking all T tokens, the first version, took 470 us for 2048 x 4096: longer than the
// Hessian update itself.)
// x(t, j): element j of token t -- a float row's, or a coded row's value (the expert-grouped statistics over MX codes)
typedef float MeanPart[8][33];
template <class LoadX>
__device__ __forceinline__ void mean_update_block(MeanPart &part, float *__restrict__ mean, int n, int T, int block, float factor, float count,
                                                  LoadX x) {
    const int f = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int j = block * 32 + f;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (j < n) {
        int t = g;
        for (; t + 24 < T; t += 32) {
            s0 = s0 + x(t, j);
            s1 = s1 + x(t + 8, j);
            s2 = s2 + x(t + 16, j);
            s3 = s3 + x(t + 24, j);
        }
        for (; t < T; t += 8) s0 = s0 + x(t, j);
    }
    part[g][f] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && j < n) {
        float s = part[0][f];
#pragma unroll
        for (int q = 1; q < 8; ++q) s = s + part[q][f];
        mean[j] = mean[j] * factor + s / count;
    }
}
__global__ __launch_bounds__(256) void k_mean_update(float *__restrict__ mean, const float *__restrict__ X, int n, int T,
                                                     float factor, float count) {
    __shared__ MeanPart part;
    mean_update_block(part, mean, n, T, blockIdx.x, factor, count, [&](int t, int j) { return X[(size_t)t * n + j]; });
}

// ------------------------------------------------------------------ expert-grouped Hessian accumulation
// slk_hessian_accumulate_experts / _experts_mx: E running statistics, rows sorted by expert, `offsets` and `counts` in device
// memory.  k_expert_stats, one workgroup, runs first on the stream: it checks the offsets rule of slk_mx_gemm_experts before
// any address is made from an offset, sets flag[0], advances counts[e] of the experts that have rows (no other entry of
// counts is touched) and, given a workspace, writes one entry an expert.  The kernels behind it are the single-layer bodies
// above over grids with an expert axis; a workgroup of an expert without rows returns at once.
//
// The workspace, as ints: [0] the 32-token slabs of all experts' planes, [1] .. [7] unused; from [8] E entries of 8 ints
// (first row, rows, first slab, f's bits, cnt's bits, 3 unused).  Without a workspace the kernels form the same five values
// from flag[0], offsets and the advanced counts: c' = counts[e], c = c' - rows.
constexpr int XS_HEAD = 8, XS_ENTRY = 8;
struct ExpertRows {
    int first, rows, slab;  // rows == 0: nothing to do (no rows, or offsets that break the rule)
    float f, cnt;
};
// `rows` tokens on top of `before`: H = H f + X^T X / cnt (slk_hessian_accumulate on the host, the prologue on the device)
__host__ __device__ __forceinline__ void expert_factor(long long before, int rows, float &f, float &cnt) {
    const long long after = before + rows;
    f = (float)((double)before / (double)after);
    cnt = (float)after;
}
__device__ __forceinline__ ExpertRows expert_rows(const int *__restrict__ table, const int *__restrict__ offsets,
                                                  const long long *__restrict__ counts, const int *__restrict__ flag, int e) {
    ExpertRows x = {0, 0, 0, 0.0f, 0.0f};
    if (table) {
        const int *entry = table + XS_HEAD + XS_ENTRY * (size_t)e;
        x.first = entry[0], x.rows = entry[1], x.slab = entry[2], x.f = __int_as_float(entry[3]), x.cnt = __int_as_float(entry[4]);
    } else if (flag[0] == 0) {  // (the prologue has checked the rule: the offsets are addresses now)
        x.first = offsets[e], x.rows = offsets[e + 1] - x.first;
        if (x.rows > 0) expert_factor(counts[e] - x.rows, x.rows, x.f, x.cnt);
    }
    return x;
}

__global__ __launch_bounds__(256) void k_expert_stats(const int *__restrict__ offsets, int E, int M, long long *__restrict__ counts,
                                                      int *__restrict__ table, int *__restrict__ flag, int flags) {
    __shared__ int scan[256];
    __shared__ int base;
    const int t = threadIdx.x;
    int bad = 0;
    for (int e = t; e < E; e += 256) {
        const int o0 = offsets[e], o1 = offsets[e + 1];
        bad |= o1 < o0 || (e == 0 && o0 != 0) || (e == E - 1 && o1 != M);
    }
    bad = __syncthreads_or(bad);
    if (t < flags) flag[t] = t == 0 && bad ? 1 : 0;
    if (t == 0) base = 0;
    for (int e0 = 0; e0 < E; e0 += 256) {  // 256 experts a round, each thread its expert's slabs behind an exclusive scan
        const int e = e0 + t;
        const int o0 = !bad && e < E ? offsets[e] : 0, rows = !bad && e < E ? offsets[e + 1] - o0 : 0, slabs = (rows + 31) / 32;
        scan[t] = slabs;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // (inclusive, Hillis-Steele)
            const int a = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += a;
            __syncthreads();
        }
        float f = 0.0f, cnt = 0.0f;
        if (rows > 0) {
            const long long before = counts[e];
            expert_factor(before, rows, f, cnt);
            counts[e] = before + rows;
        }
        if (table && e < E) {
            int *entry = table + XS_HEAD + XS_ENTRY * (size_t)e;
            entry[0] = o0, entry[1] = rows, entry[2] = base + scan[t] - slabs, entry[3] = __float_as_int(f), entry[4] = __float_as_int(cnt);
        }
        __syncthreads();
        if (t == 255) base += scan[255];
        __syncthreads();
    }
    if (table && t == 0) table[0] = base;
}

#define SLK_EXPERT_ARGS const int *__restrict__ table, const int *__restrict__ offsets, const long long *__restrict__ counts, const int *__restrict__ flag

// grid (feature blocks of 32, experts)
__global__ __launch_bounds__(256) void k_mean_update_experts(float *__restrict__ mean, const float *__restrict__ X, int n, SLK_EXPERT_ARGS) {
    __shared__ MeanPart part;
    const ExpertRows x = expert_rows(table, offsets, counts, flag, blockIdx.y);
    if (x.rows == 0) return;
    const float *__restrict__ Xe = X + (size_t)x.first * n;
    mean_update_block(part, mean + (size_t)blockIdx.y * n, n, x.rows, blockIdx.x, x.f, x.cnt, [&](int t, int j) { return Xe[(size_t)t * n + j]; });
}
// grid (tile columns, tile rows, experts)
__global__ __launch_bounds__(256, 4) void k_hessian_tiles_experts(float *__restrict__ H, const float *__restrict__ X, int n, SLK_EXPERT_ARGS) {
    __shared__ Tile128Smem sm;
    if (blockIdx.x > blockIdx.y) return;
    const ExpertRows x = expert_rows(table, offsets, counts, flag, blockIdx.z);
    if (x.rows == 0) return;
    const float *__restrict__ Xe = X + (size_t)x.first * n;
    hessian_tile_f32(sm, H + (size_t)blockIdx.z * n * n, Xe, n, x.rows, blockIdx.y, blockIdx.x, x.f, x.cnt, n % 4 == 0 && (uintptr_t)Xe % 16 == 0);
}
// The bfloat16 x 3 path (a table is there): expert e's planes are 3 x (n / 128) x its slabs x 4096 values from its first slab
// on, as the single call lays out one chunk that holds all its tokens.
__device__ __forceinline__ int expert_of_slab(const int *__restrict__ table, int E, int slab) {
    int lo = 0, hi = E - 1;  // the last expert whose first slab is <= slab (those without rows share their successor's)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[XS_HEAD + XS_ENTRY * (size_t)mid + 2] <= slab) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// grid (feature blocks of 128, an upper bound of the slabs)
__global__ __launch_bounds__(256) void k_split3_transposed_experts(const float *__restrict__ X, int n, int E, const int *__restrict__ table,
                                                                   unsigned short *__restrict__ planes, int swz) {
    __shared__ Split3Tile tile;
    if ((int)blockIdx.y >= table[0]) return;
    const ExpertRows x = expert_rows(table, nullptr, nullptr, nullptr, expert_of_slab(table, E, blockIdx.y));
    const int ksteps = (x.rows + 31) / 32, m = n / T32;
    split3_transposed_slab(tile, X + (size_t)x.first * n, n, x.rows, 0, x.rows, planes + (size_t)3 * m * 4096 * x.slab, (size_t)n * ksteps * 32, swz,
                           blockIdx.x, blockIdx.y - x.slab, ksteps);
}
// grid (8 * ceil(lower tiles / 8), experts)
template <bool DMA>
__global__ __launch_bounds__(256) void k_hessian_tiles_bf16_experts(float *__restrict__ H, const unsigned short *__restrict__ planes, int n,
                                                                    const int *__restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const ExpertRows x = expert_rows(table, nullptr, nullptr, nullptr, blockIdx.y);
    if (x.rows == 0) return;
    const int ksteps = (x.rows + 31) / 32;
    hessian_tile_bf16<DMA>(smem_raw, H + (size_t)blockIdx.y * n * n, planes + (size_t)3 * (n / T32) * 4096 * x.slab, n, ksteps,
                           (size_t)n * ksteps * 32, blockIdx.x, x.f, x.cnt);
}

// ... and over MX-coded rows (a_codes / a_scales as the activation quantizers write them): x = value(code) 2^(b - 127) has
// at most 4 significant bits, so it is a bfloat16 exactly (scale bytes 10 .. 245 keep every E4M3 value normal, 2^-9 2^(b - 127)
// .. 448 2^(b - 127); results are promised exact inside that range only) and X^T X is ONE bfloat16 MFMA pass with exact
// products and float32 sums.  The block scales lie along the features, not along the summed tokens, so the block-scaled
// MFMA is no use; v_mfma_f32_32x32x16_bf16 is.  A workgroup decodes 32 tokens x 128 features of each operand into a
// [token][feature] image in LDS, and both operands are COLUMN reads of it: ds_read_b64_tr_b16.  No software pipelining yet.
//
// Byte offset of 16-byte chunk ch (8 features) of token row `row` in an image of 256-byte rows; the XOR keeps the
// transposed reads off one another's banks (stores and reads go through it alike).
__device__ __forceinline__ int mxs_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

typedef short bf16x4_t __attribute__((ext_vector_type(4)));
// the 32x32x16 operand of 32 features from feature f0 of the image, tokens k0 .. k0 + 15: lane l holds feature f0 + (l & 31),
// tokens k0 + 8 (l >> 5) + 0 .. 7.  Every lane of the wave must call it (the gather crosses lanes).
__device__ __forceinline__ bf16x8_t mxs_operand(const unsigned char *img, int f0, int k0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int ch = (f0 + 16 * (g & 1)) / 8 + (p >> 1), row = k0 + 8 * (g >> 1) + q;
    typedef __attribute__((address_space(3))) bf16x4_t *lds_ptr;
    const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + mxs_off(row, ch) + 8 * (p & 1)));
    const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + mxs_off(row + 4, ch) + 8 * (p & 1)));
    union {
        bf16x4_t h[2];
        bf16x8_t v;
    } u;
    u.h[0] = lo, u.h[1] = hi;
    return u.v;
}
// One coded element: its code's unit of whole dwords, then the code
template <int FMT>
__device__ __forceinline__ float mxs_value(const uint8_t *__restrict__ codes, const uint8_t *__restrict__ scales, int n, size_t row, int j, bool &bad) {
    constexpr int UNIT = FMT == MXA_E2M3 ? 16 : FMT == MXA_E2M1 ? 8 : 4;
    unsigned w[UNIT * mxa_bits<FMT>() / 32];
    mxa_load<FMT, UNIT>(codes + mxa_byte_of<FMT>(row * n + (j & ~(UNIT - 1))), w);
    unsigned c = 0u;
#pragma unroll
    for (int e = 0; e < UNIT; ++e)
        if ((j & (UNIT - 1)) == e) c = mxa_code_at<FMT>(w, e);
    const unsigned b = scales[row * (n / 32) + j / 32];
    bad |= b == 255u;
    return mxa_value<FMT>(c) * e8m0_value(b);
}
// grid (feature blocks of 32, experts)
template <int FMT>
__global__ __launch_bounds__(256) void k_mean_update_experts_mx(float *__restrict__ mean, const uint8_t *__restrict__ codes,
                                                                const uint8_t *__restrict__ scales, int n, SLK_EXPERT_ARGS, int *__restrict__ nan_flag) {
    __shared__ MeanPart part;
    const ExpertRows x = expert_rows(table, offsets, counts, flag, blockIdx.y);
    if (x.rows == 0) return;
    bool bad = false;
    mean_update_block(part, mean + (size_t)blockIdx.y * n, n, x.rows, blockIdx.x, x.f, x.cnt,
                      [&](int t, int j) { return mxs_value<FMT>(codes, scales, n, (size_t)x.first + t, j, bad); });
    if (bad) *nan_flag = 1;
}
// grid (tile columns, tile rows, experts); 4 waves, each 64 x 64 of the 128 x 128 tile
template <int FMT>
__global__ __launch_bounds__(256) void k_hessian_tiles_experts_mx(float *__restrict__ H, const uint8_t *__restrict__ codes,
                                                                  const uint8_t *__restrict__ scales, int n, SLK_EXPERT_ARGS) {
    __shared__ __attribute__((aligned(16))) unsigned char img[2][32 * 256];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const ExpertRows x = expert_rows(table, offsets, counts, flag, blockIdx.z);
    if (x.rows == 0) return;
    H += (size_t)blockIdx.z * n * n;
    const int t = threadIdx.x, wave = t >> 6;
    const int i0 = bi * T32, j0 = bj * T32, wi = 64 * (wave >> 1), wj = 64 * (wave & 1);
    Acc128 acc;
    acc.zero();
    const int tok = t >> 3, fc = (t & 7) * 16;  // this thread stages 16 features (half a block) of one token, per operand
    for (int k0 = 0; k0 < x.rows; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int feature = (side ? j0 : i0) + fc;
            unsigned short v[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = 0;
            if (k0 + tok < x.rows && feature < n) {  // (n is a multiple of 32: 16 features are inside or outside together)
                const size_t row = (size_t)x.first + k0 + tok;
                unsigned w[(16 * mxa_bits<FMT>() + 31) / 32];
                mxa_load<FMT, 16>(codes + mxa_byte_of<FMT>(row * n + feature), w);
                const float sc = e8m0_value(scales[row * (n / 32) + feature / 32]);  // (byte 255: NaNs; the mean's kernel raises the flag)
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = pk_bf16(mxa_value<FMT>(mxa_code_at<FMT>(w, e)) * sc);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                uint4v_t pack;
#pragma unroll
                for (int e = 0; e < 4; ++e) pack[e] = (unsigned)v[8 * c + 2 * e] | ((unsigned)v[8 * c + 2 * e + 1] << 16);
                *reinterpret_cast<uint4v_t *>(img[side] + mxs_off(tok, fc / 8 + c)) = pack;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 32; ks += 16) {
            bf16x8_t a[2], b[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) a[s] = mxs_operand(img[0], wi + 32 * s, ks), b[s] = mxs_operand(img[1], wj + 32 * s, ks);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc.c[s][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b[u], acc.c[s][u], 0, 0, 0);
        }
    }
    hessian_store_tile(acc, H, n, bi, bj, x.f, x.cnt);
}

}  // namespace slk

using namespace slk;

extern "C" {

static PtrTable ptr_table(const float *const *ps, int count) {
    PtrTable t;
    for (int b = 0; b < 64; ++b) t.p[b] = b < count ? ps[b] : nullptr;
    return t;
}
static PtrTable one_ptr(const float *p) { return ptr_table(&p, 1); }

// flag[b] = 1 iff the n x n matrix hs.p[b] is bit-wise symmetric, b < batch
static int symmetry_flags(const PtrTable &hs, int batch, int n, int *flag, hipStream_t s) {
    const int t64 = (n + 63) / 64;
    SLK_RUN("set_flag", 0, 4, s, k_set_flag<<<1, 64, 0, s>>>(flag, 1, batch));
    SLK_RUN("symmetry_check", 0, 4.0 * n * n * batch, s, k_symmetry_flag<<<dim3(t64 * (t64 + 1) / 2, batch), 256, 0, s>>>(hs, n, flag));
    return SLK_OK;
}

static int row_errors_impl(const float *W, const float *Q, const float *const *Hs, int batch, int rpl, int n, float *row_err,
                           float *G, void *workspace, size_t ws_bytes, slk_stream_t stream, const int *sym_known = nullptr) {
    const int R = batch * rpl;
    const int n_tiles = (n + T32 - 1) / T32;
    Arena ws(workspace, ws_bytes);
    // K split of the bfloat16 kernel for few rows (see the kernel): the largest chunk that still gives >= 512 workgroups
    const int n_rt = (R + T32 - 1) / T32;
    int cb = 0, n_slots = n_tiles;
    if (G == nullptr && n_rt * n_tiles < 512 && !opt(OPT_NO_ERROR_SPLITK)) {
        const int force = opt(OPT_ERROR_CB);
        for (int c = force ? force : 16; c >= 2; c >>= 1) {
            int slots = 0;
            for (int x = 0; x < n_tiles; ++x) slots += (x + c) / c;
            if (slots > 4 * n_tiles) break;
            cb = c;
            n_slots = slots;
            if (n_rt * slots >= 512 || force) break;
        }
    }
    float *partial = ws.take<float>((size_t)R * n_slots);
    int *sym = ws.take<int>(64);
    if (!partial || !sym) {
        set_error("workspace too small");
        return SLK_E_WS;
    }
    hipStream_t s = as_stream(stream);
    if (cb > 0) zero_async(partial, (size_t)R * n_slots * sizeof(float), s);  // the float32 kernel fills n_tiles slots only
    dim3 grid(8 * ((n_tiles * n_rt + 7) / 8));  // a multiple of the 8 XCDs: see the tile order in the kernel
    bool aligned = ((uintptr_t)W | (uintptr_t)Q) % 16 == 0;
    const HPtrs hp = ptr_table(Hs, batch);
    for (int b = 0; b < batch; ++b) aligned = aligned && (uintptr_t)Hs[b] % 16 == 0;
    const int vec_ok = n % 4 == 0 && aligned;
    const bool try_sym = !opt(OPT_NO_SYM_ERROR);  // (with G too: the bfloat16 kernel needs H symmetric)
    if (try_sym && sym_known) {
        sym = const_cast<int *>(sym_known);  // verdicts computed elsewhere (slk_symmetry_flag), read only from here on
    } else if (try_sym) {
        if (const int rc = symmetry_flags(hp, batch, n, sym, s)) return rc;
    }
    // the bfloat16 x 3 kernel when the shape allows (16-byte loads, whole tiles of columns).  Its operands are split into
    // planes first, 10 bytes of traffic per element of H and layer; until the end of round 2 a batch with fewer than 1024
    // rows per layer (the row shards of a round on 8 ranks: 512 rows each) took the float32 kernel instead (H as it
    // stands).  Measured again after the non-symmetric route and the banded splits: the bfloat16 kernel wins at every
    // shard size by now (a rank of 8: 4.31 -> 4.14 ms per round; OPT-125M ... BLOOM-560M shards 0.5-1.5 %), so the
    // threshold is a switch that is off by default ("error_f32_below" = rows).
    const int f32_below = opt(OPT_ERROR_F32_BELOW) > 0 ? opt(OPT_ERROR_F32_BELOW) : 0;
    const bool few_rows = G == nullptr && batch > 1 && rpl < f32_below;
    const size_t d_plane = (size_t)n_rt * T32 * n;  // rows padded to whole tiles
    unsigned short *Dp = ws.take<unsigned short>(3 * d_plane), *Hp = ws.take<unsigned short>(3 * (size_t)n * n * batch);
    const int bf16_ok = try_sym && vec_ok && n % T32 == 0 && Dp && Hp && !opt(OPT_NO_BF16_ERROR) && !few_rows;
    // a Hessian that is NOT symmetric stays on the bfloat16 kernel too (planes of H^T, every k) unless K is cut into chunks
    // ... or, when only the error is wanted (no G), is AVERAGED with its transpose on the way into the planes (asym_mode 2):
    // d H d^T = d ((H + H^T) / 2) d^T, so every Hessian takes the symmetric half-product route
    const int asym_mode = !bf16_ok ? 0 : (G == nullptr && !opt(OPT_NO_SYM_AVERAGE)) ? 2 : (cb == 0 && !opt(OPT_NO_BF16_ASYM)) ? 1 : 0;
    if (batch > 1 && !few_rows && !(Dp && Hp)) {
        set_error("workspace too small for the operand planes of %d layers (slk_workspace_bytes_batch)", batch);
        return SLK_E_WS;
    }
    // every layer's rows through the float32 kernel in one launch (those whose flag says "symmetric" are skipped when
    // the bfloat16 kernel has taken them)
    auto f32_all = [&](const int *flags, int bf16_takes_sym) {
        k_error_tiles<<<grid, 256, 0, s>>>(W, Q, hp, R, n, G, partial, n_tiles, vec_ok, flags, bf16_takes_sym, n_slots, rpl);
    };
    // algorithmic flops: the definition (2 R n^2) whichever way they are obtained
    if (bf16_ok) {
        const int dma = !opt(OPT_NO_BF16_DMA);  // operands to LDS by global_load_lds: swizzled planes
        SLK_RUN("error_split", 0, 14.0 * R * n, s,
                k_split3<<<2048, 256, 0, s>>>(one_ptr(W), Q, R, n, Dp, d_plane, batch == 1 && !asym_mode ? sym : nullptr, dma, 0, 0));
        {
            // every layer's H in one launch each (blockIdx.y / z = layer)
            const int split_blocks = (int)std::min<size_t>(2048, ((size_t)n * n / 4 + 255) / 256);
            SLK_RUN("error_split", 0, 10.0 * n * n * batch, s,
                    k_split3<<<dim3(split_blocks, batch), 256, 0, s>>>(hp, nullptr, n, n, Hp, (size_t)n * n, sym, dma, G == nullptr,
                                                                       asym_mode == 2));
            if (asym_mode == 1)  // (a layer's blocks return at once when its flag says symmetric)
                SLK_RUN("error_split_t", 0, 0, s,
                        k_split3_transposed<<<dim3(n / T32, n / 32, batch), 256, 0, s>>>(hp, n, n, 0, n, Hp, (size_t)n * n, dma, sym));
        }
        // flops as executed: six bfloat16 products per float32 product, over k <= j only (the definition of the
        // layer error, SURVEY.md 8d, counts 2 R n^2 float32 flops: a third of this, twice over)
        const int wgs = cb > 0 ? n_rt * n_slots : 8 * ((n_rt + 7) / 8) * ((n_tiles + 7) / 8 * 8);  // see the tile order in the kernel
        const int rc = with_bf16_staging([&](auto staging) -> int {
            constexpr bool DMA = decltype(staging)::value;
            SLK_LDS_OPT_IN(k_error_tiles_bf16<DMA>, sizeof(TileBf16<DMA>));
            SLK_RUN_W("error_gemm_bf16", 6.0 * R * n * (n + (double)T32), 6.0 * R * n + 3.0 * n * n * batch, cb > 0 ? wgs : n_rt * n_tiles, s,
                      k_error_tiles_bf16<DMA><<<wgs, 256, sizeof(TileBf16<DMA>), s>>>(W, Q, Dp, Hp, R, n, partial, n_tiles, sym, n_slots, cb,
                                                                                      rpl, G, asym_mode));
            return SLK_OK;
        });
        if (rc) return rc;
        if (!asym_mode) SLK_RUN("error_gemm_f32", 0, 0, s, f32_all(sym, 1));
    } else {
        SLK_RUN("error_gemm", 2.0 * R * n * n, 8.0 * R * n + 4.0 * n * n * batch + (G ? 4.0 * R * n : 0.0), s,
                f32_all(try_sym && G == nullptr ? sym : nullptr, 0));  // (its symmetric shortcut does not produce G)
    }
    SLK_RUN("error_reduce", 0, 4.0 * R * n_slots, s, k_error_reduce<<<(R + 255) / 256, 256, 0, s>>>(partial, R, n_slots, row_err));
    return SLK_OK;
}

int slk_row_errors(const float *W, const float *Q, const float *H, int R, int n, float *row_err, float *G,
                   void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(W && Q && H && row_err && R > 0 && n > 0, "bad arguments");
    return row_errors_impl(W, Q, &H, 1, R, n, row_err, G, workspace, ws_bytes, stream);
}

int slk_row_errors_batch(const float *W, const float *Q, const float *const *H, int batch, int rows_per_layer, int n,
                         const int *symmetric, float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(W && Q && H && row_err && rows_per_layer > 0 && n > 0, "bad arguments");
    SLK_REQUIRE(batch >= 1 && batch <= 64, "batch must be 1..64");
    SLK_REQUIRE(batch == 1 || rows_per_layer % T32 == 0, "a batch needs rows_per_layer to be a multiple of 128");
    for (int b = 0; b < batch; ++b) SLK_REQUIRE(H[b], "null Hessian in the batch");
    return row_errors_impl(W, Q, H, batch, rows_per_layer, n, row_err, nullptr, workspace, ws_bytes, stream, symmetric);
}

int slk_symmetry_flag(const float *H, int n, int *flag, slk_stream_t stream) {
    SLK_REQUIRE(H && flag && n > 0, "bad arguments");
    return symmetry_flags(one_ptr(H), 1, n, flag, as_stream(stream));
}

int slk_hessian_accumulate(float *H, float *mean, const float *X, int n, int T, long long count_before,
                           void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(H && mean && X && n > 0 && T > 0 && count_before >= 0, "bad arguments");
    float factor, count;
    expert_factor(count_before, T, factor, count);
    hipStream_t s = as_stream(stream);
    const int nt = (n + T32 - 1) / T32;
    SLK_RUN("mean_update", 0, 4.0 * T * n, s, k_mean_update<<<(n + 31) / 32, 256, 0, s>>>(mean, X, n, T, factor, count));
    // bfloat16 x 3 path: whole tiles of features, and room for the planes of at least 32 tokens
    Arena ws(workspace, ws_bytes);
    const size_t room = workspace && ws_bytes > 4096 ? (ws_bytes - 4096) / ((size_t)6 * n) / 32 * 32 : 0;  // tokens per chunk
    if (n % T32 == 0 && room >= 32 && !opt(OPT_NO_BF16_HESSIAN)) {
        const int dma = !opt(OPT_NO_BF16_DMA);
        const int chunk = (int)(room < (size_t)((T + 31) / 32 * 32) ? room : (size_t)((T + 31) / 32 * 32));
        unsigned short *Xp = ws.take<unsigned short>((size_t)3 * n * chunk);
        const int m = n / T32, total = m * (m + 1) / 2;
        for (int t0 = 0; t0 < T; t0 += chunk) {
            const int cnt = T - t0 < chunk ? T - t0 : chunk, ksteps = (cnt + 31) / 32;
            const size_t plane = (size_t)n * ksteps * 32;
            SLK_RUN("hessian_split", 0, 10.0 * cnt * n, s,
                    k_split3_transposed<<<dim3(m, ksteps), 256, 0, s>>>(one_ptr(X), n, T, t0, cnt, Xp, plane, dma, nullptr));
            // the running-mean factor applies once per batch: later chunks add to what the first one scaled
            const int rc = with_bf16_staging([&](auto staging) -> int {
                constexpr bool DMA = decltype(staging)::value;
                SLK_LDS_OPT_IN(k_hessian_tiles_bf16<DMA>, sizeof(TileBf16<DMA>));
                SLK_RUN("hessian_syrk_bf16", 6.0 * cnt * n * (n + (double)T32), 6.0 * cnt * n + 8.0 * n * n, s,
                        k_hessian_tiles_bf16<DMA><<<8 * ((total + 7) / 8), 256, sizeof(TileBf16<DMA>), s>>>(
                            H, Xp, n, ksteps, plane, t0 == 0 ? factor : 1.0f, count));
                return SLK_OK;
            });
            if (rc) return rc;
        }
        return SLK_OK;
    }
    dim3 grid(nt, nt);
    SLK_RUN("hessian_syrk", (double)T * n * (n + 1), 4.0 * T * n + 8.0 * n * n, s,
            k_hessian_tiles<<<grid, 256, 0, s>>>(H, X, n, T, factor, count, n % 4 == 0 && (uintptr_t)X % 16 == 0));
    return SLK_OK;
}

// Bytes of the table, and the 32-token slabs the planes of all experts can take: every expert with rows pads to 32
static inline size_t xs_table_bytes(int E) { return sizeof(int) * (XS_HEAD + (size_t)XS_ENTRY * E); }
static inline size_t xs_slab_cap(int E, int M) { return (size_t)M / 32 + (size_t)(E < M ? E : M); }

size_t slk_hessian_experts_workspace_bytes(int E, int n, int M) {
    if (E < 1 || n < 1 || M < 1) return 0;
    return align_up(xs_table_bytes(E), 256) + (n % T32 == 0 ? (size_t)6 * n * 32 * xs_slab_cap(E, M) : 0);
}

static int xs_check(int E, int n, int M, const void *H, const void *mean, const void *offsets, const void *counts, const void *flag,
                    const void *workspace, size_t ws_bytes) {
    SLK_REQUIRE(E >= 1 && E <= SLK_MX_MAX_EXPERTS, "E must be 1 .. %d experts (E = %d)", SLK_MX_MAX_EXPERTS, E);
    SLK_REQUIRE(n >= 1 && M >= 1, "n and M must be at least 1 (n = %d, M = %d)", n, M);
    SLK_REQUIRE(H && mean, "null H or mean");
    SLK_REQUIRE(offsets, "null offsets");
    SLK_REQUIRE(counts, "null counts");
    SLK_REQUIRE(flag, "null flag");
    SLK_REQUIRE((uintptr_t)workspace % 16 == 0, "the workspace must be aligned to 16 bytes");
    SLK_REQUIRE(!workspace || ws_bytes >= xs_table_bytes(E), "the workspace is too small for the table of %d experts: %zu bytes, at least %zu",
                E, ws_bytes, xs_table_bytes(E));
    SLK_REQUIRE((n + T32 - 1) / T32 <= 65535, "n is above the 65535 tile rows of one launch (n = %d)", n);
    return SLK_OK;
}

int slk_hessian_accumulate_experts(float *H, float *mean, const float *X, const int *offsets, int E, int n, int M, long long *counts,
                                   int *flag, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    if (const int rc = xs_check(E, n, M, H, mean, offsets, counts, flag, workspace, ws_bytes)) return rc;
    SLK_REQUIRE(X, "null X");
    hipStream_t s = as_stream(stream);
    int *table = static_cast<int *>(workspace);
    const int nt = (n + T32 - 1) / T32;
    SLK_RUN("expert_stats", 0, 4.0 * (E + 1) + 16.0 * E, s, k_expert_stats<<<1, 256, 0, s>>>(offsets, E, M, counts, table, flag, 1));
    SLK_RUN("mean_update_experts", 0, 4.0 * M * n, s,
            k_mean_update_experts<<<dim3((n + 31) / 32, E), 256, 0, s>>>(mean, X, n, table, offsets, counts, flag));
    // bfloat16 x 3 path: whole tiles of features, and room for the planes of every expert's tokens padded to 32; no chunks
    Arena ws(workspace, ws_bytes);
    ws.take<int>(XS_HEAD + (size_t)XS_ENTRY * E);
    const size_t slabs = xs_slab_cap(E, M);
    // (its split is one launch over the slabs: past 65535 of them, 2 M tokens, the float32 chain as well)
    unsigned short *planes =
        n % T32 == 0 && slabs <= 65535 && !opt(OPT_NO_BF16_HESSIAN) ? ws.take<unsigned short>((size_t)3 * n * 32 * slabs) : nullptr;
    if (planes) {
        const int dma = !opt(OPT_NO_BF16_DMA);
        const int m = n / T32, total = m * (m + 1) / 2;
        SLK_RUN("hessian_split_experts", 0, 10.0 * M * n, s,
                k_split3_transposed_experts<<<dim3(m, (unsigned)slabs), 256, 0, s>>>(X, n, E, table, planes, dma));
        return with_bf16_staging([&](auto staging) -> int {
            constexpr bool DMA = decltype(staging)::value;
            SLK_LDS_OPT_IN(k_hessian_tiles_bf16_experts<DMA>, sizeof(TileBf16<DMA>));
            SLK_RUN("hessian_syrk_bf16_experts", 6.0 * M * n * (n + (double)T32), 6.0 * M * n + 8.0 * n * n * E, s,
                    k_hessian_tiles_bf16_experts<DMA><<<dim3(8 * ((total + 7) / 8), E), 256, sizeof(TileBf16<DMA>), s>>>(H, planes, n, table));
            return SLK_OK;
        });
    }
    SLK_RUN("hessian_syrk_experts", (double)M * n * (n + 1), 4.0 * M * n + 8.0 * n * n * E, s,
            k_hessian_tiles_experts<<<dim3(nt, nt, E), 256, 0, s>>>(H, X, n, table, offsets, counts, flag));
    return SLK_OK;
}

}  // extern "C"

template <int FMT>
static int hessian_experts_mx(float *H, float *mean, const uint8_t *a_codes, const uint8_t *a_scales, const int *offsets, int E, int n, int M,
                              long long *counts, int *flag, int *table, hipStream_t s) {
    const int nt = (n + T32 - 1) / T32;
    const double coded = (double)M * n / 32.0 * mxa_block_bytes<FMT>();
    SLK_RUN("expert_stats", 0, 4.0 * (E + 1) + 16.0 * E, s, k_expert_stats<<<1, 256, 0, s>>>(offsets, E, M, counts, table, flag, 2));
    SLK_RUN("mean_update_experts_mx", 0, coded, s,
            k_mean_update_experts_mx<FMT><<<dim3(n / 32, E), 256, 0, s>>>(mean, a_codes, a_scales, n, table, offsets, counts, flag, flag + 1));
    SLK_RUN("hessian_syrk_experts_mx", (double)M * n * (n + 1), coded * nt + 8.0 * n * n * E, s,
            k_hessian_tiles_experts_mx<FMT><<<dim3(nt, nt, E), 256, 0, s>>>(H, a_codes, a_scales, n, table, offsets, counts, flag));
    return SLK_OK;
}

extern "C" {

int slk_hessian_accumulate_experts_mx(float *H, float *mean, const uint8_t *a_codes, const uint8_t *a_scales, int a_fmt, const int *offsets,
                                      int E, int n, int M, long long *counts, int *flag, void *workspace, size_t ws_bytes,
                                      slk_stream_t stream) {
    if (const int rc = xs_check(E, n, M, H, mean, offsets, counts, flag, workspace, ws_bytes)) return rc;
    SLK_REQUIRE(n % 32 == 0, "MX blocks are 32 columns: n must be a positive multiple of 32 (n = %d)", n);
    SLK_REQUIRE(a_codes && a_scales, "null a_codes or a_scales");
    SLK_REQUIRE(aligned16(a_codes), "a_codes must be aligned to 16 bytes");
    SLK_REQUIRE(a_fmt == SLK_MX_ACT_FP8 || a_fmt == SLK_MX_ACT_FP4 || a_fmt == SLK_MX_ACT_FP6, "unknown a_fmt %d", a_fmt);
    hipStream_t s = as_stream(stream);
    int *table = static_cast<int *>(workspace);
    if (a_fmt == SLK_MX_ACT_FP4) return hessian_experts_mx<MXA_E2M1>(H, mean, a_codes, a_scales, offsets, E, n, M, counts, flag, table, s);
    if (a_fmt == SLK_MX_ACT_FP6) return hessian_experts_mx<MXA_E2M3>(H, mean, a_codes, a_scales, offsets, E, n, M, counts, flag, table, s);
    return hessian_experts_mx<MXA_E4M3>(H, mean, a_codes, a_scales, offsets, E, n, M, counts, flag, table, s);
}

}  // extern "C"

namespace slk {
int row_errors_products(const float *W, const float *Q, const float *const *Hs, int batch, int rpl, int n, const int *sym_known,
                        float *row_err, float *G, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    return row_errors_impl(W, Q, Hs, batch, rpl, n, row_err, G, workspace, ws_bytes, stream, sym_known);
}
}  // namespace slk

