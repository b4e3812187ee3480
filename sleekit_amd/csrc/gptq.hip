// a5 + a8 + a9 + a10: the column-sequential quantize / error-propagation loop
// (sleekit/obq.py:106-137, 202-213) with the reference's recursion and rounding points.
//
// Host side flattens the recursion of _quantize_opt_block into
//   LEAF(a, b)        quantize columns a..b-1 one at a time           (obq.py:106-118)
//   UPDATE(a, b, c)   Q[:, b:c] -= E[:, a:b] @ U[a:b, b:c]            (obq.py:137)
// and cuts it into WINDOWS: maximal sub-trees at most 512 columns wide.  A window runs in
// one kernel, a 16-row tile per workgroup with its Q and E columns resident in LDS; the
// updates that reach beyond a window run as chip-wide float64 MFMA GEMMs.
//
// Numerics follow the reference exactly: float32 quantizer (true divide, rint, separate
// multiply/add), err = float64(w - q) / U[i][i], rank-1 and block updates in float64
// (product rounded, then subtraction rounded), one rounding to float32 per update.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "window2.h"

namespace slk {

constexpr int OP_LEAF = 0, OP_UPDATE = 1;
constexpr int MAX_OPS = 60;   // ops per window kernel (kernel-argument table)

struct Op {
    int kind, a, b, c;
    int m;   // UPDATE: columns [b, m) are needed at once, [m, c) may trail behind the next leaves
    int nl;  // UPDATE: number of leaves before [m, c) is touched again
};
struct OpTable {
    int count;
    Op op[MAX_OPS];
};

// ------------------------------------------------------------------ permute in / out
// Both are row gathers by a fixed column permutation.  A row goes through LDS: coalesced 16-byte loads in,
// the gather reads LDS (random 4-byte reads there cost a few cycles; straight from global every one of them
// was its own L1/L2 request: 2 TB/s), coalesced 16-byte stores out.  Rows longer than PERM_MAX floats take
// the plain kernels.
constexpr int PERM_MAX = 16384;

// One body for both forms of a row gather.  LDS: the source row is read from its copy in LDS (rowbuf), four elements an iteration,
// 16-byte stores; otherwise straight from global memory, one element an iteration.
template <bool LDS>
__device__ __forceinline__ void stage_row(float *rowbuf, const float *src, int n) {
    if constexpr (LDS) {
        __syncthreads();  // the previous row's gathers are done
        for (int c = threadIdx.x; c < (n >> 2); c += 256) reinterpret_cast<float4v_t *>(rowbuf)[c] = reinterpret_cast<const float4v_t *>(src)[c];
        __syncthreads();
    }
}
template <int V>
__device__ __forceinline__ void load_elems(const float *p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4v_t x = *reinterpret_cast<const float4v_t *>(p);
        v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_elems(float *p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4v_t *>(p) = (float4v_t){v[0], v[1], v[2], v[3]};
    else *p = v[0];
}

// Qp[r][c] = W[r][order[c]] (/ scale[r]);  E is cleared by the window kernels as they go.  No orders in the table (never with
// LDS): the identity.
template <bool LDS>
__global__ __launch_bounds__(256) void k_permute_in(LayerTable lt, int R, int n, float *__restrict__ Qp,
                                                    int *__restrict__ inv_order, int rpl) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];  // (LDS only)
    constexpr int V = LDS ? 4 : 1;
    const int t = threadIdx.x;
    const bool scale = lt.scale[0] != nullptr, order = lt.order[0] != nullptr;
    // (a batch of layers: stacked rows [b rpl, (b + 1) rpl) are layer b's, and follow order[b], inv_order[b])
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const int b = r / rpl, rl = r - b * rpl;
        const float *__restrict__ src = layer_base(lt.W, b, (size_t)rpl * n) + (size_t)rl * n;
        const long long *__restrict__ ord = (LDS || order) ? layer_base(lt.order, b, n) : nullptr;
        stage_row<LDS>(rowbuf, src, n);
        const float s = scale ? layer_base(lt.scale, b, rpl)[rl] : 1.0f;
        for (int c = V * t; c < n; c += V * 256) {
            long long from[V];  // all of an iteration's order entries first: wide loads, in flight together
            float v[V];
#pragma unroll
            for (int e = 0; e < V; ++e) from[e] = (LDS || ord) ? ord[c + e] : c + e;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float x = LDS ? rowbuf[from[e]] : src[from[e]];
                v[e] = scale ? x / s : x;
            }
            store_elems<V>(Qp + (size_t)r * n + c, v);
        }
    }
    for (int b = blockIdx.x; b < (R + rpl - 1) / rpl; b += gridDim.x) {
        const long long *__restrict__ ord = order ? layer_base(lt.order, b, n) : nullptr;
        for (int c = t; c < n; c += 256) inv_order[(size_t)b * n + (ord ? ord[c] : c)] = c;
    }
}

// Q[r][j] = Qp[r][inv[j]];  idx[r][j] = grid index of that value (codebook.py:43-54).
// ERR (slk_gptq_quantize_batch_error): the workgroup that writes row r of Q also reads row r of W and of the loop's scaled
// errors E and leaves the row's error (W - Qw) H (W - Qw)^T, carried by the loop instead of a product of its own:
//     row_err[r] = float32(scale_r^2 * sum_j E[r][j]^2 - lambda_b * sum_j (W[r][j] - Qw[r][j])^2)
// with Qw the value STORED to Q, float32 differences, float64 squares and sums, lambda_b = damp * mean(diag H_b) the float32
// damping term the factor was made with (hmean[64 b]: loop_error_means).  E is in processing order, W and Q in the
// original one: the sums do not care.  One fixed-order workgroup reduction and one store per row: the same bits every run.
struct RowErrArgs {
    const float *E, *hmean;  // (W and the scales: the layers' own, from the table)
    float damp;
    float *row_err;
};
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // lane 0 holds the sum
}
// the row's two sums over the workgroup's 256 threads, then the store (red: 8 doubles of LDS; scale: the row's, 1 without)
__device__ __forceinline__ void row_error_store(double se, double sd, double *red, const RowErrArgs &a, int r, int rpl, float scale) {
    se = wave_sum_f64(se);
    sd = wave_sum_f64(sd);
    const int t = threadIdx.x;
    if ((t & 63) == 0) {
        red[t >> 6] = se;
        red[4 + (t >> 6)] = sd;
    }
    __syncthreads();
    if (t == 0) {
        const double SE = ((red[0] + red[1]) + red[2]) + red[3], SD = ((red[4] + red[5]) + red[6]) + red[7];
        const double s = (double)scale;
        const float lambda = a.damp * a.hmean[64 * (r / rpl)];  // float32 product, as k_diag_prepare forms it
        a.row_err[r] = (float)((s * s) * SE - (double)lambda * SD);
    }
    __syncthreads();  // red is free again
}

template <bool LDS, bool ERR>
__global__ __launch_bounds__(256) void k_permute_out(const float *__restrict__ Qp, const int *__restrict__ inv_order,
                                                     int R, int n, Grid g, int unscale, float *__restrict__ Q,
                                                     uint8_t *__restrict__ idx, int rpl, RowErrArgs ea, LayerTable lt) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];  // (LDS only)
    __shared__ double red[ERR ? 8 : 1];
    constexpr int V = LDS ? 4 : 1;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const float *src = Qp + (size_t)r * n;
        const int b = r / rpl, rl = r - b * rpl;
        const int *inv_o = inv_order + (size_t)b * n;
        stage_row<LDS>(rowbuf, src, n);
        const float scale = unscale ? layer_base(lt.scale, b, rpl)[rl] : 1.0f;
        const float inv = unscale ? 1.0f / scale : 1.0f;  // scaling.py:80: a division by the reciprocal
        const float *__restrict__ wrow = ERR ? layer_base(lt.W, b, (size_t)rpl * n) + (size_t)rl * n : nullptr;
        double se = 0.0, sd = 0.0;
        for (int j = V * threadIdx.x; j < n; j += V * 256) {
            float qw[V];
            unsigned packed = 0;  // the elements' indices, one byte each
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float v = LDS ? rowbuf[inv_o[j + e]] : src[inv_o[j + e]];
                if (idx) packed |= (unsigned)(cb_index(v, g) & 255) << (8 * e);
                qw[e] = unscale ? v / inv : v;
            }
            store_elems<V>(Q + (size_t)r * n + j, qw);
            if (idx) {
                if constexpr (LDS) *reinterpret_cast<unsigned *>(idx + (size_t)r * n + j) = packed;
                else idx[(size_t)r * n + j] = (uint8_t)packed;
            }
            if constexpr (ERR) {
                float w[V], ev[V];
                load_elems<V>(wrow + j, w);
                load_elems<V>(ea.E + (size_t)r * n + j, ev);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float d = w[e] - qw[e];
                    sd += (double)d * (double)d;
                    se += (double)ev[e] * (double)ev[e];
                }
            }
        }
        if constexpr (ERR) row_error_store(se, sd, red, ea, r, rpl, scale);
    }
}
// one launch of either permute kernel: the LDS form stages a row of n floats
template <class K, class... A>
static int launch_permute(const char *name, double flops, double bytes, K kernel, bool lds, int R, int n, hipStream_t s, A... args) {
    if (lds) SLK_LDS_OPT_IN(kernel, PERM_MAX * 4);
    SLK_RUN(name, flops, bytes, s, kernel<<<R < 2048 ? R : 2048, 256, lds ? (size_t)n * 4 : 0, s>>>(args...));
    return SLK_OK;
}

// ------------------------------------------------------------------ group scales (slk_gptq_quantize_grouped_batch)
// S (R x G, G = n / gsize) holds one scale per row and per group of gsize ORIGINAL columns; the loop runs on the
// unscaled weights and only its leaves scale (see leaf_chain16 and LeafTile).  pg[b n + c] = group of processing column c
// of layer b (a batch of layers stacked by rows, `batch` rows of order; no order: batch 1, the identity).
__global__ __launch_bounds__(256) void k_group_of_column(const long long *__restrict__ order, int batch, int n, int gsize,
                                                         int *__restrict__ pg) {
    const size_t total = (size_t)batch * n;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
        pg[e] = (int)((order ? order[e] : (long long)e) / gsize);
}

// Q[r][j] = Qp[r][inv[j]] (already de-scaled by the leaves);  idx[r][j] = codebook index of Q[r][j] / S[r][j / gsize].
// Q = value / rs with rs = RN(1 / s), so Q / s is the codebook value to within a few ulps: far closer than half a step
// (uniform) or than the nearest bin limit (table), and the index comes back exactly (dequantize_grouped checks it).
// OFFSET (slk_gptq_quantize_grouped_asym): Q = value / rs + o, o = O[r][j / gsize], and the index is that of (Q - o) / s,
// checked to rebuild Q bit for bit; where `+ o` has absorbed part of the codebook term (|o| / s large, s at its floor)
// that index may not, and the codebook is searched for one that does (the leaf's own always does).
template <bool OFFSET = false>
__global__ __launch_bounds__(256) void k_permute_out_grouped(const float *__restrict__ Qp, const int *__restrict__ inv_order,
                                                             int R, int n, Grid g, const float *__restrict__ S, int gsize,
                                                             float *__restrict__ Q, uint8_t *__restrict__ idx, int rpl,
                                                             const float *__restrict__ O) {
    const int G = n / gsize;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const float *src = Qp + (size_t)r * n;
        const int *inv_o = inv_order + (size_t)(r / rpl) * n;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const float v = src[inv_o[j]];
            Q[(size_t)r * n + j] = v;
            if (idx) {
                const GroupQ<OFFSET> gq = GroupQ<OFFSET>::at(S, O, (size_t)r * G + j / gsize);
                int k = gq.index(v, g);
                if constexpr (OFFSET) {
                    auto back = [&](int t) { return __float_as_uint(gq.dequant(cb_entry(t, g))); };
                    if (back(k) != __float_as_uint(v))
                        for (int t = 0; t < g.n; ++t)
                            if (back(t) == __float_as_uint(v)) {
                                k = t;
                                break;
                            }
                }
                idx[(size_t)r * n + j] = (uint8_t)k;
            }
        }
    }
}

// ------------------------------------------------------------------ window kernel
struct WindowSmem {
    // leaf tables first: their offsets fit the 16-bit immediate of ds_read, so the unrolled leaf
    // needs one address register instead of one per step.  Two copies: the helper waves fill the
    // tables of the next leaf while the chain waves read those of the current one.
    LeafTables lt[2];
    int odd[2][4];  // per helper wave: a diagonal entry of that block defeats the exact-division shortcut
    float q[RB][WPITCH];
    float e[RB][WPITCH];
    float cbt[512];  // a general codebook's values and limits (<= 256 entries), copied here for the leaves
};
// the update's view of it (TileUpdate): one tile, E beside Q, column for column
struct WindowTile {
    WindowSmem &sm;
    int w0;
    __device__ __forceinline__ float *q(int, int row, int col) const { return &sm.q[row][col - w0]; }
    __device__ __forceinline__ const float *e(int, int row, int k) const { return &sm.e[row][k - w0]; }
    __device__ __forceinline__ static bool straight(int) { return true; }
};

// the group quantizers: q = codebook(x / s) / rs (two true divides; the codebook step keeps the exact-division sequence),
// OFFSET codebook((x - o) / s) / rs + o
template <bool OFFSET>
__device__ __forceinline__ float leaf_group_q(float x, const GroupQ<OFFSET> e, const Grid g, float inv_step) {
    return e.dequant(grid_value_fast(e.scaled(x), g, inv_step));
}

// The window's scales in the grouped loop, beside WindowSmem: s[r][c] = S[row][group of column c], rs = RN(1 / s).
// The pitch leaves room for the steps a leaf runs past its width (up to 31 columns beyond the window), which read 1.0.
constexpr int GPITCH = WMAX + 32;
struct GroupTile {
    float s[RB][GPITCH];
    float rs[RB][GPITCH];
};
// the symmetric group quantizer with s, rs of every (row, column) from the GroupTile
struct LeafTile {
    const GroupTile &gt;
    typedef GroupQ<false> Step;
    __device__ __forceinline__ Step at(int row, int a, int k) const { return {(&gt.s[row][a])[k], (&gt.rs[row][a])[k]}; }
    template <bool FAST>
    __device__ __forceinline__ static float q(float x, Step e, const Grid g, float inv_step) { return leaf_group_q(x, e, g, inv_step); }
};

// The asymmetric grouped loop (OFFSET) needs a third value per step, the offset o.  A third per-column plane beside the
// GroupTile does not fit in LDS, so this tile holds s, rs and o per ROW AND GROUP instead -- all G groups of the tile's
// rows when G <= GSLOTS -- and a column -> group map of the window (its padding points at slot GSLOTS: s = 1, o = 0).
// Beyond GSLOTS groups the leaves read S and O from memory (the generic leaf).
constexpr int GSLOTS = 384;
struct GroupSlots {
    float s[RB][GSLOTS + 1];
    float rs[RB][GSLOTS + 1];
    float o[RB][GSLOTS + 1];
    int slot[GPITCH];
};
static_assert(sizeof(WindowSmem) + sizeof(GroupSlots) <= 160 * 1024, "the asymmetric window's LDS exceeds a CU's 160 KiB");
// the asymmetric group quantizer: the map entry of column a + k, then that group's s, rs and o
struct LeafSlots {
    const GroupSlots &gs;
    typedef GroupQ<true> Step;
    __device__ __forceinline__ Step at(int row, int a, int k) const {
        const int slot = gs.slot[a + k];
        return {gs.s[row][slot], gs.rs[row][slot], gs.o[row][slot]};
    }
    template <bool FAST>
    __device__ __forceinline__ static float q(float x, Step e, const Grid g, float inv_step) { return leaf_group_q(x, e, g, inv_step); }
};

// A fast leaf of k_gptq_window's tile, columns [a_rel, a_rel + w) of the window, by chain wave `wave`: x out of sm.q, q and e into
// sm.q and sm.e.
template <class P>
__device__ __forceinline__ void leaf_tile16(WindowSmem &sm, const P &pol, const LeafTables &lt, int wave, int lane, int a_rel, int w,
                                            const Grid g, float inv_step) {
    const int c16 = lane & 15, row = 4 * wave + (lane >> 4);
    const bool m0 = c16 < w, m1 = c16 + 16 < w;
    const float x0 = m0 ? sm.q[row][a_rel + c16] : 0.0f, x1 = m1 ? sm.q[row][a_rel + 16 + c16] : 0.0f;
    float q0 = 0.0f, q1 = 0.0f, e0 = 0.0f, e1 = 0.0f;
    if (w <= 16) leaf_chain16<16, true>(lt, pol, row, a_rel, c16, x0, x1, q0, q1, e0, e1, g, inv_step);
    else leaf_chain16<32, true>(lt, pol, row, a_rel, c16, x0, x1, q0, q1, e0, e1, g, inv_step);
    if (m0) {
        sm.q[row][a_rel + c16] = q0;
        sm.e[row][a_rel + c16] = e0;
    }
    if (m1) {
        sm.q[row][a_rel + 16 + c16] = q1;
        sm.e[row][a_rel + 16 + c16] = e1;
    }
}

// The generic leaves' quantizer (true divides): the codebook alone, or through the group's scale (and offset)
template <bool GROUPED, bool OFFSET>
__device__ __forceinline__ float generic_q(float x, const GroupQ<OFFSET> gq, const Grid g) {
    if constexpr (GROUPED) return gq.value(x, g);
    else return cb_value(x, g);
}

// One workgroup = 512 threads = 8 waves = RB rows, Q and E of the window resident in LDS.
//
// LEAF (fast path): waves 0-3, the CHAIN waves, run the column chain, four rows each.  Waves 4-7,
// the HELPERS, meanwhile (a) write the U tables of the next leaf into the other LDS buffer and
// fetch those of the one after, (b) run a share of the DEFERRED part of the last update on the MFMA
// pipe: UPDATE(a, b, c) is split at m, the end of the sub-tree that follows it -- columns [b, m) are
// needed at once (urgent, all eight waves, the chain waits for them), columns [m, c) are not touched
// again before the next update with the same c and are folded in behind the chain's back, spread
// over the `nl` leaves in between.  Every column still sees the same updates in the same order,
// each rounded to float32 once, so the result is the reference's bit for bit.
// UPDATE: the target columns are cut in 16-wide MFMA blocks (M = the 16 rows of the tile), dealt
// round-robin to the participating waves, K in chunks of 64.
// GROUPED: the leaves quantize with the group scales S (R x G) of the unscaled weights, pg[c] =
// group of processing column c; in LDS the window's scales sit in a GroupTile behind WindowSmem.  Everything else --
// updates, deferral, staging -- is the same code.
// OFFSET (with GROUPED): the asymmetric group quantizer, offsets O (R x G) beside S; in LDS a GroupSlots behind WindowSmem
// when G <= GSLOTS, otherwise every leaf is the generic one and reads S and O from memory.
// (A window wider than WMAX is a single leaf: k_gptq_wide_leaf.)
template <bool GROUPED, bool OFFSET = false>
__global__ __launch_bounds__(512) void k_gptq_window(float *__restrict__ Qp, float *__restrict__ Eg,
                                                     LayerTable lt, int R, int n, int w0, int w1,
                                                     Grid g, float inv_step, int fast_ok, int dbg, OpTable tab, int rpl,
                                                     const float *__restrict__ Sg, const int *__restrict__ pg, int G,
                                                     const float *__restrict__ Og) {
    static_assert(GROUPED || !OFFSET, "offsets come with group scales");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    WindowSmem &sm = *reinterpret_cast<WindowSmem *>(smem_raw);
    GroupTile &gt = *reinterpret_cast<GroupTile *>(smem_raw + sizeof(WindowSmem));  // (GROUPED only)
    GroupSlots &gs = *reinterpret_cast<GroupSlots *>(smem_raw + sizeof(WindowSmem));  // (OFFSET only)
    const bool slots = OFFSET && G <= GSLOTS;  // the leaves' s, rs, o in LDS
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool helper = wave >= 4;
    const int ht = t - 256;  // helper thread index
    const int r0 = blockIdx.x * RB;
    const double *__restrict__ U = layer_base(lt.U, r0 / rpl, (size_t)n * n);  // a batch of layers: rows [b rpl, (b + 1) rpl) use factor b
    if constexpr (GROUPED) pg += (size_t)(r0 / rpl) * n;  // ... and group table b (a tile never straddles two layers)
    if (g.table) {  // the leaves search the codebook once per column: keep it next to them
        for (int i = t; i < 2 * g.n - 1; i += 512) sm.cbt[i] = g.table[i];
        g.table = sm.cbt;  // visible after the first barrier below
    }
    const int width = w1 - w0;
    Laps laps(dbg);  // cycle accounting (debug)
    auto lap = [&](int slot, int w) { laps.lap(slot, wave == w); };
    // Plain accesses to the tile: every producer/consumer pair below is separated by a __syncthreads().
    const bool vec4 = tile_vec4(Qp, n, w0);
    auto load_cols = [&](int c_lo, int c_hi, int tid, int nth) { load_tile_cols<RB>(sm.q, Qp, r0, R, n, w0, vec4, c_lo, c_hi, tid, nth); };

    // ---- staging pipeline of the leaf tables (helpers only): registers <- U two staged leaves
    // ahead, LDS buffer <- registers one leaf ahead.
    double pu[4] = {0.0, 0.0, 0.0, 0.0};
    int fetch_w = 0;     // width of the block held in pu, 0 = none
    int next_fetch = 0;  // op from which to look for the next staged leaf
    auto fetch_block = [&]() {
        fetch_w = 0;
        for (; next_fetch < tab.count; ++next_fetch) {
            const Op nx = tab.op[next_fetch];
            const int w = nx.b - nx.a;
            if (nx.kind != OP_LEAF || w > ULEAF) continue;
            fetch_leaf_block(U, n, nx.a, w, ht, pu);
            fetch_w = w;
            ++next_fetch;
            return;
        }
    };
    auto write_block = [&](int buf) {
        const bool any = write_leaf_tables(sm.lt[buf], pu, fetch_w, ht);
        if (lane == 0) sm.odd[buf][wave - 4] = any ? 1 : 0;
    };

    if constexpr (OFFSET) {  // every group of the tile's rows (s = 1, o = 0 beyond G and R), read after the barrier below
        if (slots) {
            for (int e = t; e < RB * (GSLOTS + 1); e += 512) {
                const int r = e / (GSLOTS + 1), k = e % (GSLOTS + 1);
                const bool in = k < G && r0 + r < R;
                const float sv = in ? Sg[(size_t)(r0 + r) * G + k] : 1.0f;
                gs.s[r][k] = sv;
                gs.rs[r][k] = 1.0f / sv;
                gs.o[r][k] = in ? Og[(size_t)(r0 + r) * G + k] : 0.0f;
            }
            for (int c = t; c < GPITCH; c += 512) gs.slot[c] = c < width ? pg[w0 + c] : GSLOTS;
        }
    }
    if constexpr (GROUPED && !OFFSET) {  // the window's scales (1.0 on the padding and on rows beyond R), read after the barrier below
        for (int e = t; e < RB * GPITCH; e += 512) {
            const int r = e / GPITCH, c = e % GPITCH;
            const float sv = (c < width && r0 + r < R) ? Sg[(size_t)(r0 + r) * G + pg[w0 + c]] : 1.0f;
            gt.s[r][c] = sv;
            gt.rs[r][c] = 1.0f / sv;
        }
    }

    // Warm this XCD's L2 with the window's block of U (workgroup i runs on XCD i % 8; the
    // workgroups of an XCD share the lines, one 4-byte touch per 128-byte line).
    float warm = 0.0f;
    if (!(dbg & 16)) {
        const int per_xcd = max(1, min(32, (int)gridDim.x >> 3));
        const int slice = (blockIdx.x >> 3) % per_xcd;
        const int lpr = (width + 15) >> 4, total = width * lpr;
        const int per_slice = (total + per_xcd - 1) / per_xcd;
        for (int id = slice * per_slice + t; id < min(total, (slice + 1) * per_slice); id += 512) {
            const int row = id / lpr, c0 = (id % lpr) << 4;
            if (c0 + 15 >= row) warm += reinterpret_cast<const float *>(U + (size_t)(w0 + row) * n + w0 + min(c0, width - 1))[0];
        }
    }

    // Prologue: only the first leaf's columns are needed before the first barrier; the rest of the
    // tile is loaded by the helpers during that leaf.
    if (helper) fetch_block();
    const int first_end = (tab.op[0].kind == OP_LEAF && !(dbg & 32)) ? tab.op[0].b : w1;
    load_cols(w0, first_end, t, 512);
    int rest_from = first_end;  // columns [rest_from, w1) of the tile still to be loaded
    if (helper) {
        if (fetch_w) write_block(0);
        fetch_block();
    }
    __syncthreads();
    lap(7, 0);

    // ---- UPDATE: Q[:, lo:hi] -= E[:, a:b] @ U[a:b, lo:hi] on the 16 rows of this tile (TileUpdate); the chain waves issue
    // round 0 of the urgent part BEFORE their leaf.  Layers wider than 16384 columns come here too: 64-bit offsets then.
    TileUpdate<1, WindowTile, false> upd{{sm, w0}, U, n, n <= 16384, lane & 15, lane >> 4};
    bool primed = false;
    // generic leaf (any width, true divides): the whole workgroup in lockstep, 32 lanes per row,
    // one barrier per column.  Rare (width > 32, or a diagonal hitting the exact-division
    // exception), so simplicity wins.
    auto generic_leaf = [&](int a, int b, bool staged, int buf) {
        const LeafTables &lt = sm.lt[buf];
        const int myrow = 2 * wave + (lane >> 5), l = lane & 31;
        float *qrow = sm.q[myrow], *erow = sm.e[myrow];  // of window columns
        for (int i = a; i < b; ++i) {
            GroupQ<OFFSET> gq = {1.0f, 1.0f, 0.0f};  // (the tile's padding rows (x = 0) past R: nothing of S or O to read)
            if constexpr (OFFSET) {
                if (slots) {
                    const int k = gs.slot[i - w0];
                    gq = {gs.s[myrow][k], gs.rs[myrow][k], gs.o[myrow][k]};
                } else if (r0 + myrow < R) {
                    gq = GroupQ<true>::at(Sg, Og, (size_t)(r0 + myrow) * G + pg[i]);
                }
            } else if constexpr (GROUPED) {
                gq = {gt.s[myrow][i - w0], gt.rs[myrow][i - w0], 0.0f};
            }
            const float x = qrow[i - w0], q = generic_q<GROUPED>(x, gq, g);
            const double uii = staged ? lt.udr[i - a][0] : U[(size_t)i * n + i];
            const double err = (double)(x - q) / uii;
            __syncthreads();  // everyone has read column i before lane 0 overwrites it
            for (int j = i + 1 + l; j < b; j += 32) {
                const double uij = staged ? lt.u[i - a][j - a] : U[(size_t)i * n + j];
                const double p = err * uij;
                qrow[j - w0] = (float)((double)qrow[j - w0] - p);
            }
            if (l == 0) {
                erow[i - w0] = (float)err;
                qrow[i - w0] = q;
            }
            __syncthreads();
        }
    };

    // deferred part of the last update: Q[:, pm:pc] -= E[:, pa:pb] @ U[pa:pb, pm:pc], of which the
    // first pdone 16-column blocks are done and the rest is due within pleaves more leaves
    int pa = 0, pb = 0, pm = 0, pc = 0, pdone = 0, pleaves = 1;
#ifdef SLK_WINDOW_EXPERIMENTS  // measurement builds only: these bits switch parts of the work OFF (wrong values)
    const bool no_updates = dbg & 2, no_leaves = dbg & 1, no_leaf_regs = dbg & 4;
#else
    constexpr bool no_updates = false, no_leaves = false, no_leaf_regs = false;
#endif
    int sbuf = 0;  // LDS buffer holding the tables of the next staged leaf

    // One pass per op plus a final pass that folds in whatever is still pending.  Each pass: at most
    // one update job per wave (ONE call site of upd.run: it is big), then the leaf, then a barrier.
    for (int oi = 0; oi <= tab.count; ++oi) {
        const bool fin = oi == tab.count;
        const Op op = tab.op[fin ? 0 : oi];
        const bool is_leaf = !fin && op.kind == OP_LEAF;
        if (!fin && (is_leaf ? no_leaves : no_updates)) continue;
        const int prem = (pc - pm + 15) / 16 - pdone;  // pending blocks
        const int plo = pm + 16 * pdone;
        // the update job of this wave in this pass: Q[:, ulo:uhi] -= E[:, ua:ub] @ U[ua:ub, ulo:uhi]
        int ua = 0, ub = 0, ulo = 0, uhi = 0, uwid = wave, unw = 8;
        bool uready = false, redo = false, use_fast = false, staged = false;
        if (is_leaf) {
            const int w = op.b - op.a;
            staged = w <= ULEAF;
            use_fast = staged && fast_ok;
            if (use_fast) use_fast = (sm.odd[sbuf][0] | sm.odd[sbuf][1] | sm.odd[sbuf][2] | sm.odd[sbuf][3]) == 0;
            if constexpr (OFFSET) use_fast = use_fast && slots;
            lap(1, 0);
        }
        // the rest of the tile goes in during the first leaf, behind a fast one by the helpers, otherwise by everyone (or here
        // at the end where no leaf ran: debug modes).  ONE call site: the loader is big too.
        const bool rest = (is_leaf || fin) && rest_from < w1;
        if (rest && (helper || !use_fast)) load_cols(rest_from, w1, use_fast ? ht : t, use_fast ? 256 : 512);
        if (rest) rest_from = w1;
        if (is_leaf) {
            if (use_fast) {
                // this leaf's share of the pending blocks, in whole turns of the four helpers
                const int take = prem > 0 ? min(prem, ((prem + pleaves - 1) / pleaves + 3) & ~3) : 0;
                if (helper) {
                    if (fetch_w) write_block(sbuf ^ 1);
                    fetch_block();
                    ua = pa, ub = pb, ulo = plo, uhi = min(pc, plo + 16 * take), uwid = wave - 4, unw = 4;
                } else if (oi + 1 < tab.count && tab.op[oi + 1].kind == OP_UPDATE && !no_updates) {
                    const Op nx = tab.op[oi + 1];
                    upd.load_round(nx.a, nx.b, nx.b, nx.m, wave, 0, upd.cur);
                    primed = true;
                }
                pdone += take;
                pleaves = max(1, pleaves - 1);
            } else {
                if (helper && staged) {
                    if (fetch_w) write_block(sbuf ^ 1);
                    fetch_block();
                }
                ua = pa, ub = pb, ulo = plo, uhi = pc;  // everything pending, all eight waves
                pdone += prem;
            }
        } else if (fin) {
            if (prem <= 0 && !rest) break;
            ua = pa, ub = pb, ulo = plo, uhi = pc;
            pdone += prem;
        } else if (prem > 0 && ((op.c > plo && op.b < pc) || op.m < op.c)) {
            // an update that meets columns still pending, or has a deferred part of its own while the
            // older one is unfinished (never under the host's leaf counts, unless leaves were
            // skipped): fold the pending columns in first, then come back
            ua = pa, ub = pb, ulo = plo, uhi = pc;
            pdone += prem;
            redo = true;
        } else {
            ua = op.a, ub = op.b, ulo = op.b, uhi = op.m, uready = primed;
            primed = false;
            // an update without a deferred part (a small one between two leaves) leaves the older
            // deferral alone: that one keeps trailing behind the following leaves
            if (op.m < op.c) pa = op.a, pb = op.b, pm = op.m, pc = op.c, pdone = 0, pleaves = max(1, op.nl);
        }
        if (!is_leaf) lap(10, 0);
        if (ulo < uhi) upd.run(ua, ub, ulo, uhi, uwid, unw, uready);
        if (is_leaf) {
            if (use_fast) {
                if (!helper && !no_leaf_regs) {
                    const int w = op.b - op.a;
                    if constexpr (OFFSET) leaf_tile16(sm, LeafSlots{gs}, sm.lt[sbuf], wave, lane, op.a - w0, w, g, inv_step);
                    else if constexpr (GROUPED) leaf_tile16(sm, LeafTile{gt}, sm.lt[sbuf], wave, lane, op.a - w0, w, g, inv_step);
                    else leaf_tile16(sm, LeafRows{}, sm.lt[sbuf], wave, lane, op.a - w0, w, g, inv_step);
                }
                lap(0, 0);
                lap(5, 4);
            } else {
                __syncthreads();
                generic_leaf(op.a, op.b, staged, sbuf);
            }
            if (staged) sbuf ^= 1;
        } else {
            lap(3, 0);
        }
        __syncthreads();
        if (is_leaf) {
            lap(2, 0);
            lap(6, 4);
        } else {
            lap(4, 0);
        }
        if (redo) --oi;
    }

    store_tile<RB>(sm.q, Qp, r0, R, n, w0, width, vec4, t);
    store_tile<RB>(sm.e, Eg, r0, R, n, w0, width, tile_vec4(Eg, n, w0), t);
    if (warm == 1.2345e-30f) g_win_cycles[15] = 1;  // keeps the touches alive
    lap(8, 0);
    laps.flush(lane, wave);
}

// A window wider than WMAX is one LEAF (plan() cuts anything else down to WMAX): the generic leaf on global memory, the
// whole workgroup in lockstep, 16 rows per workgroup and 32 lanes per row, S, O and the codebook read where they are.
template <bool GROUPED, bool OFFSET = false>
__global__ __launch_bounds__(512) void k_gptq_wide_leaf(float *__restrict__ Qp, float *__restrict__ Eg, LayerTable lt,
                                                        int R, int n, int a, int b, Grid g, int rpl, const float *__restrict__ Sg,
                                                        const int *__restrict__ pg, int G, const float *__restrict__ Og) {
    static_assert(GROUPED || !OFFSET, "offsets come with group scales");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 31;
    const int r0 = blockIdx.x * RB, row = r0 + 2 * wave + (lane >> 5);
    const bool live = row < R;
    const double *__restrict__ U = layer_base(lt.U, r0 / rpl, (size_t)n * n);  // a batch of layers, as in k_gptq_window
    if constexpr (GROUPED) pg += (size_t)(r0 / rpl) * n;
    float *qrow = Qp + (size_t)min(row, R - 1) * n, *erow = Eg + (size_t)min(row, R - 1) * n;  // (touched where live)
    for (int i = a; i < b; ++i) {
        float q = 0.0f;
        double err = 0.0;
        if (live) {
            GroupQ<OFFSET> gq = {1.0f, 1.0f, 0.0f};
            if constexpr (GROUPED) gq = GroupQ<OFFSET>::at(Sg, Og, (size_t)row * G + pg[i]);
            const float x = qrow[i];
            q = generic_q<GROUPED>(x, gq, g);
            err = (double)(x - q) / U[(size_t)i * n + i];
        }
        __syncthreads();  // everyone has read column i before lane 0 overwrites it
        if (live) {
            for (int j = i + 1 + l; j < b; j += 32) {
                const double p = err * U[(size_t)i * n + j];
                qrow[j] = (float)((double)qrow[j] - p);
            }
            if (l == 0) {
                erow[i] = (float)err;
                qrow[i] = q;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ trailing update
// Qp[:, ja:jb] = float32(float64(Qp[:, ja:jb]) - E[:, ka:kb] @ U[ka:kb, ja:jb]), 64 x 64 tiles.
__global__ __launch_bounds__(256) void k_gptq_trailing(float *__restrict__ Qp, const float *__restrict__ Eg,
                                                       LayerTable lt, int R, int n, int ka, int kb,
                                                       int ja, int jb, int vec_ok, int rpl) {
#ifdef SLK_TRAILING_F64_IMAGE
    __shared__ __attribute__((aligned(16))) Tile64Smem sm;
#else
    __shared__ __attribute__((aligned(16))) Tile64SmemAf sm;  // E stays float32 in LDS (mfma64.h)
#endif
    const int r0 = blockIdx.y * TILE, j0 = ja + blockIdx.x * TILE;
    const double *__restrict__ U = layer_base(lt.U, r0 / rpl, (size_t)n * n);  // a batch of layers (rpl a multiple of the tile)
    const int t = threadIdx.x;
    Acc64 acc;
    acc.zero();
    const int kend = ka + (kb - ka + KSTEP - 1) / KSTEP * KSTEP;
    const int a_row = r0 + (t >> 2), a_k = (t & 3) * 8;  // A = E (float32), K contiguous
    const int b_k = t >> 3, b_c2 = (t & 7) * 2;          // B = U (float64), columns contiguous: pieces at 16 h + b_c2
    // interior tiles take the unguarded loaders over the whole K-steps; a ragged last step (K = 172 at n = 11008)
    // and the edge tiles take the guarded ones
    int k_fast = ka;
    if (vec_ok && r0 + TILE <= R && j0 + TILE <= jb) {
        k_fast = ka + (kb - ka) / KSTEP * KSTEP;
        const float *pe = Eg + (size_t)a_row * n + a_k;
        const double *pu = U + (size_t)b_k * n + j0 + b_c2;
        tile64_mac<true, float>(
            acc, sm, ka, k_fast, [&](int k0, float(&v)[8]) { load8f<true>(pe + k0, v); },
            [&](int k0, double(&v)[8]) { load8d_cols(pu + (size_t)k0 * n, v); });
    }
    if (k_fast < kend) {
        const bool row_ok = a_row < R;
        const float *pe = Eg + (size_t)min(a_row, R - 1) * n;
        tile64_mac<true, float>(
            acc, sm, k_fast, kend,
            [&](int k0, float(&v)[8]) {
                const int k = k0 + a_k;
                load8f_guarded(pe + min(k, kb - 1), kb - 1 - k, row_ok, v);
            },
            [&](int k0, double(&v)[8]) {
                const int k = k0 + b_k;
                load8d_cols_guarded(U + (size_t)min(k, kb - 1) * n + j0, b_c2, jb - 1 - j0, k < kb, v);
            });
    }
    if (r0 + TILE <= R && j0 + TILE <= jb) {
        // interior tile: ALL sixteen old values of a thread first, then the sixteen stores.  Element by element (below) every
        // guarded `*p = *p - v` is a load -> s_waitcnt vmcnt(0) -> store round trip of its own, sixteen in a row at the end of
        // every tile: the compiler cannot tell the addresses apart.
        float *q0 = Qp + (size_t)r0 * n + j0;
        float oldq[16];
        int e = 0;
        tile64_foreach(acc, [&](int r, int c, double) { oldq[e++] = q0[(size_t)r * n + c]; });
        e = 0;
        tile64_foreach(acc, [&](int r, int c, double v) { q0[(size_t)r * n + c] = (float)((double)oldq[e++] - v); });
        return;
    }
    tile64_foreach(acc, [&](int r, int c, double v) {
        if (r0 + r < R && j0 + c < jb) {
            float *p = Qp + (size_t)(r0 + r) * n + j0 + c;
            *p = (float)((double)*p - v);
        }
    });
}

// ------------------------------------------------------------------ host planning
static void flatten(int a, int b, int mb, int nb, std::vector<Op> &ops) {
    const int size = b - a;
    if (size <= mb) {
        ops.push_back({OP_LEAF, a, b, 0, 0, 0});
        return;
    }
    int step = (size + nb - 1) / nb;
    if (step < mb) step = mb;
    for (int s = a; s < b; s += step) {
        const int e = s + step < b ? s + step : b;
        flatten(s, e, mb, nb, ops);
        if (e < b) ops.push_back({OP_UPDATE, s, e, b, b, 1});
    }
}

struct Plan {
    // kind 0: window [a, b) with ops; kind 1: chip-wide update (a, b, c)
    struct Step {
        int kind, a, b, c;
        std::vector<Op> ops;
    };
    std::vector<Step> steps;
};

static void plan(int a, int b, int mb, int nb, Plan &p) {
    const int size = b - a;
    std::vector<Op> ops;
    flatten(a, b, mb, nb, ops);
    if (size <= mb || (size <= WMAX && (int)ops.size() <= MAX_OPS)) {
        p.steps.push_back({0, a, b, 0, ops});
        return;
    }
    int step = (size + nb - 1) / nb;
    if (step < mb) step = mb;
    for (int s = a; s < b; s += step) {
        const int e = s + step < b ? s + step : b;
        plan(s, e, mb, nb, p);
        if (e < b) p.steps.push_back({1, s, e, b, {}});
    }
}

// A window's ops as periods (window2.h), or false when the window is not of the standard shape.
static bool as_periods(const std::vector<Op> &ops, int wa, int wb, PeriodTable &pt) {
    pt.count = 0;
    size_t i = 0;
    while (i < ops.size()) {
        if (pt.count == MAXP || ops[i].kind != OP_LEAF) return false;
        Period P = {ops[i].a, ops[i].b - ops[i].a, 0, 0};
        ++i;
        if (i + 1 < ops.size() && ops[i].kind == OP_UPDATE && ops[i].a == P.s && ops[i].b == P.s + P.w1 &&
            ops[i + 1].kind == OP_LEAF && ops[i + 1].a == P.s + P.w1 && ops[i].c == ops[i + 1].b) {
            P.w2 = ops[i + 1].b - ops[i + 1].a;
            i += 2;
        }
        const int K = P.w1 + P.w2;
        if (i < ops.size()) {
            if (ops[i].kind != OP_UPDATE || ops[i].a != P.s || ops[i].b != P.s + K || ops[i].c != wb) return false;
            ++i;
        } else if (P.s + K != wb) {
            return false;
        }
        if (P.w1 > ULEAF || P.w2 > ULEAF || (P.s & 1) || (P.w1 & 1) || (P.w2 & 1) || P.w1 < 2) return false;
        pt.p[pt.count++] = P;
    }
    if (pt.count == 0 || pt.p[0].s != wa) return false;
    for (int k = 0; k + 1 < pt.count; ++k) {
        if (pt.p[k + 1].s != pt.p[k].s + pt.p[k].w1 + pt.p[k].w2) return false;
        pt.p[k].nw = pt.p[k + 1].w1 + pt.p[k + 1].w2;
    }
    return true;
}

}  // namespace slk

using namespace slk;

namespace slk {
// the leaf chain alone: `iters` leaves of 32 columns on the tables of a made-up block; out[0] = cycles
// of wave 0, out[1] = checksum.  blockDim = 256 (one wave per SIMD) or 512 (two).
__global__ void k_probe_leaf(double *out, int iters, int mode, Grid g, float inv_step) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    WindowSmem &sm = *reinterpret_cast<WindowSmem *>(smem_raw);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int e = t; e < 32 * 32; e += blockDim.x) {
        const int i = e >> 5, j = e & 31;
        sm.lt[0].u[i][j] = j > i ? 0.01 * ((i * 7 + j * 3) % 11 - 5) : 0.0;
        if (i == j) sm.lt[0].udr[i][0] = 1.0 + 0.01 * i, sm.lt[0].udr[i][1] = 1.0 / (1.0 + 0.01 * i);
    }
    for (int e = t; e < RB * 64; e += blockDim.x) sm.q[e >> 6][e & 63] = 0.37f * ((e * 13) % 17 - 8);
    __syncthreads();
    const long long t0 = (long long)__builtin_readcyclecounter();
    double4_t macc = {0, 0, 0, 0};
    double vacc = 1.0;
    // modes 1-3: leaf waves 0-3, companions 4-7 (same SIMDs if waves go round the SIMDs);
    // mode 4: leaf waves 0, 1, 4, 5 and MFMA companions 2, 3, 6, 7 (other SIMDs under that mapping)
    const bool leafer = mode == 4 ? (wave & 2) == 0 : (wave < 4 || mode == 0);
    if (mode == 4) mode = leafer ? 0 : 1;
    if (t == 0) out[2] = (double)__builtin_amdgcn_s_getreg((4 << 11) | (0 << 6) | 4);  // HW_ID, 32 bits... low 16 here
    if (leafer || mode == 0) {
        // (with more than two leaf waves per SIMD several waves run the same four rows: garbage values, honest timing)
        for (int it = 0; it < iters; ++it) leaf_tile16(sm, LeafRows{}, sm.lt[0], ((wave & 1) + ((wave >> 2) << 1)) & 3, lane, (it & 1) * 32, 32, g, inv_step);
    } else if (mode == 5) {
        // companion wave on the same SIMD: back-to-back bfloat16 MFMAs (what the layer-error kernel issues)
        typedef __bf16 probe_bf16x8_t __attribute__((ext_vector_type(8)));
        typedef float probe_f32x16_t __attribute__((ext_vector_type(16)));
        probe_bf16x8_t av, bv;
        for (int k = 0; k < 8; ++k) av[k] = (__bf16)(1.0f + lane), bv[k] = (__bf16)2.0f;
        probe_f32x16_t c16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int it = 0; it < iters * 64; ++it) c16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, c16, 0, 0, 0);
        vacc = c16[0];
    } else if (mode == 1) {
        // companion wave on the same SIMD: back-to-back 16x16x4 MFMAs for about as long
        for (int it = 0; it < iters * 64; ++it) macc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0 + lane, 2.0, macc, 0, 0, 0);
    } else if (mode == 2) {
        // companion wave: a dependent float64 fma chain
        for (int it = 0; it < iters * 400; ++it) vacc = __builtin_fma(vacc, 1.0000001, 1e-9);
    } else {
        // companion wave: LDS reads
        for (int it = 0; it < iters * 100; ++it) vacc += sm.lt[1].u[(it + lane) & 31][lane & 31];
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    __shared__ long long leaf_cycles[16];
    if (lane == 0) leaf_cycles[wave] = leafer || mode == 0 ? t1 - t0 : 0;
    __syncthreads();
    if (t == 0) {
        out[0] = (double)(t1 - t0);
        out[1] = sm.q[3][5] + sm.e[2][7];
        long long slowest = 0;  // the oldest wave of a SIMD issues first: wave 0 alone says nothing about the others
        for (int w = 0; w < (int)blockDim.x / 64; ++w) slowest = leaf_cycles[w] > slowest ? leaf_cycles[w] : slowest;
        out[3] = (double)slowest;
    }
    if (macc[0] + vacc == 1.2345e-30) out[1] = macc[0];
}
}  // namespace slk

extern "C" int slk_probe_leaf_chain(double *out, int iters, int waves_per_simd, slk_stream_t stream) {
    // waves_per_simd: 1, 2, 3, 4 (all leaf waves), or 2 + 10 * mode for companions (1 float64 MFMA, 2 fma chain, 3 LDS reads,
    // 5 bfloat16 MFMA)
    const int mode = waves_per_simd / 10;
    waves_per_simd %= 10;
    SLK_REQUIRE(out && iters > 0 && waves_per_simd >= 1 && waves_per_simd <= 4 && mode >= 0 && mode <= 5, "bad arguments");
    hipStream_t s = as_stream(stream);
    const Grid g = make_grid(8, -1.0, 1.0);
    SLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe_leaf), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sizeof(WindowSmem)));
    SLK_RUN("probe_leaf", 0, 0, s, k_probe_leaf<<<1, 256 * waves_per_simd, sizeof(WindowSmem), s>>>(out, iters, mode, g, 1.0f / g.step));
    return SLK_OK;
}

extern "C" int slk_probe_window_cycles(long long *host_out, int reset) {
    SLK_REQUIRE(host_out, "null pointer");
    SLK_HIP(hipDeviceSynchronize());
    SLK_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_win_cycles), sizeof(long long) * 16));
    SLK_HIP(hipMemcpyFromSymbol(host_out + 16, HIP_SYMBOL(g_win_trace), sizeof(long long) * 64));
    if (reset) {
        long long zero[64] = {0};
        SLK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_win_cycles), zero, sizeof(long long) * 16));
        SLK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_win_trace), zero, sizeof(zero)));
    }
    return SLK_OK;
}

extern "C" int slk_gptq_quantize(const float *W, const float *scale, const long long *order, const double *U,
                                 int R, int n, int levels, double lo, double hi, const float *table, int min_block, int num_blocks,
                                 int flags, float *Q, uint8_t *idx, float *E_out, void *workspace, size_t ws_bytes,
                                 slk_stream_t stream) {
    return slk_gptq_quantize_batch(W, scale, order, U, 1, R, n, levels, lo, hi, table, min_block, num_blocks, flags, Q, idx,
                                   E_out, workspace, ws_bytes, stream);
}

// The general window kernel's LDS: the tile, then the group quantizer's tables behind it.
template <bool GROUPED, bool OFFSET>
constexpr size_t window_lds() {
    return sizeof(WindowSmem) + (OFFSET ? sizeof(GroupSlots) : GROUPED ? sizeof(GroupTile) : 0);
}
// One launch of it, or of the wide leaf for a window beyond WMAX (one LEAF op): the kernel, the LDS size and the profile name
// follow from the template arguments and the width (gptq_loop has opted in to the LDS).
template <bool GROUPED, bool OFFSET>
static int launch_window(double flops, double bytes, int row_tiles, hipStream_t s, float *Qp, float *Eg, const LayerTable &lt, int R,
                         int n, int w0, int w1, Grid g, float inv_step, int fast_ok, int dbg, const OpTable &tab, int rpl, const float *Sg,
                         const int *pg, int G, const float *Og) {
    if (w1 - w0 > WMAX) {
        SLK_REQUIRE(tab.count == 1 && tab.op[0].kind == OP_LEAF, "a window of %d columns that is not one leaf", w1 - w0);
        SLK_RUN(OFFSET ? "gptq_window_wide_grouped_asym" : GROUPED ? "gptq_window_wide_grouped" : "gptq_window_wide", flops, bytes, s,
                k_gptq_wide_leaf<GROUPED, OFFSET><<<row_tiles, 512, 0, s>>>(Qp, Eg, lt, R, n, w0, w1, g, rpl, Sg, pg, G, Og));
        return SLK_OK;
    }
    SLK_RUN(OFFSET ? "gptq_window_grouped_asym" : GROUPED ? "gptq_window_grouped" : "gptq_window", flops, bytes, s,
            k_gptq_window<GROUPED, OFFSET><<<row_tiles, 512, window_lds<GROUPED, OFFSET>(), s>>>(Qp, Eg, lt, R, n, w0, w1, g, inv_step, fast_ok, dbg,
                                                                                               tab, rpl, Sg, pg, G, Og));
    return SLK_OK;
}

// The table of a batch stacked by rows in one allocation: W, scale (batch rows_per_layer) (x n), order batch x n, U batch x n x n.
static LayerTable stacked_layers(const float *W, const float *scale, const long long *order, const double *U, int batch,
                                 int rows_per_layer, int n) {
    LayerTable lt{};
    for (int b = 0; b < batch && b < LOOP_LAYERS; ++b) {
        lt.W[b] = W + (size_t)b * rows_per_layer * n;
        lt.scale[b] = scale ? scale + (size_t)b * rows_per_layer : nullptr;
        lt.order[b] = order ? order + (size_t)b * n : nullptr;
        lt.U[b] = U + (size_t)b * n * n;
    }
    return lt;
}

// `batch` layers of one shape, their rows stacked in the workspace and in the outputs: every launch of the loop covers all
// of them, each row tile reading its own layer's factor.  What a row shard of a multi-GPU run needs: R / G rows alone leave
// most of the chip idle (the window kernel runs one workgroup per 16 rows), G layers' shards together fill it; and what two
// full-height layers need to fill the chip with 32-row window workgroups without another stream's help.
// lt: where every layer's W, scale, order and U lie (stacked_layers, or the caller's own pointers: slk_gptq_quantize_layers).
// gscale != nullptr: the grouped loop (slk_gptq_quantize_grouped_batch), no row scale.  Arena: Qp and Eg (R n floats
// each), the inverse orders (batch n ints) and, grouped, the group tables (batch n ints): four 256-byte-aligned takes.
// row_err != nullptr (slk_gptq_quantize_batch_error; Hs: host array of the layers' Hessians): the last kernel also leaves the
// rows' errors (k_permute_out<true>), from the diagonal means of a fifth take (64 floats per layer).
static int gptq_loop(const LayerTable &lt, int batch, int rows_per_layer, int n, int levels, double lo, double hi, const float *table,
                     int min_block, int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out, void *workspace, size_t ws_bytes, slk_stream_t stream,
                     const float *gscale, int group_size, const float *goffset, const float *const *Hs = nullptr, float damp = 0.0f,
                     float *row_err = nullptr) {
    const bool grouped = gscale != nullptr, asym = goffset != nullptr;
    const int unscale = flags & SLK_LOOP_UNSCALE;
    const bool scale = lt.scale[0] != nullptr, order = lt.order[0] != nullptr;
    SLK_REQUIRE(!unscale || scale, "unscale needs the row scales");
    SLK_REQUIRE(rows_per_layer > 0 && n > 0, "empty layer");
    SLK_REQUIRE(batch >= 1 && batch <= 64, "batch must be 1..64");
    SLK_REQUIRE(batch == 1 || rows_per_layer % TILE == 0, "a batch needs rows_per_layer to be a multiple of 64");
    SLK_REQUIRE(batch == 1 || order, "a batch needs the column orders");
    // what the 16-byte forms ask of the inputs holds for every layer or for none (the layers of a stack beyond the table
    // follow its entries by whole strides, which the forms' conditions on n keep aligned)
    uintptr_t W_bits = 0, U_bits = 0;
    for (int b = 0; b < batch && b < LOOP_LAYERS; ++b) W_bits |= (uintptr_t)lt.W[b], U_bits |= (uintptr_t)lt.U[b];
    SLK_REQUIRE((long long)batch * rows_per_layer <= 0x7fffffffLL, "too many rows");
    const int R = batch * rows_per_layer, rpl = rows_per_layer;
    SLK_REQUIRE(levels >= 2 && (table || lo < hi), "codebook needs levels >= 2 and lo < hi");
    SLK_REQUIRE(table == nullptr || levels <= 256, "general codebooks hold at most 256 entries");
    SLK_REQUIRE(idx == nullptr || levels <= 256, "uint8 indices need levels <= 256");
    SLK_REQUIRE(min_block >= 1 && num_blocks >= 1, "min_block_size and num_blocks must be >= 1");
    Arena ws(workspace, ws_bytes);
    float *Qp = ws.take<float>((size_t)R * n);
    float *Eg = ws.take<float>((size_t)R * n);
    int *inv_order = ws.take<int>((size_t)batch * n);
    int *pg = grouped ? ws.take<int>((size_t)batch * n) : nullptr;  // group of every processing column, per layer
    float *hmean = row_err ? ws.take<float>(64 * (size_t)batch) : nullptr;  // mean(diag H_b) at [64 b]
    if (!Qp || !Eg || !inv_order || (grouped && !pg) || (row_err && !hmean)) {
        set_error("workspace too small for a %d x %d layer", R, n);
        return SLK_E_WS;
    }
    hipStream_t s = as_stream(stream);
    const Grid g = make_grid(levels, lo, hi, table);
    // exact-division shortcut of the leaf: needs a sane step whose significand is not all ones
    const float inv_step = 1.0f / g.step;
    unsigned step_bits;
    memcpy(&step_bits, &g.step, 4);
    const int fast_ok = table == nullptr && (step_bits & 0x7FFFFFu) != 0x7FFFFFu && g.step > 9.0e-13f && g.step < 1.0e12f &&
                        !opt(OPT_NO_FAST_LEAF);
#ifdef SLK_WINDOW_EXPERIMENTS
    const int dbg = opt(OPT_WIN_DBG);
#else
    const int dbg = opt(OPT_WIN_DBG) & (8 | 16 | 32 | 64 | 128);  // cycle counters, no L2 warm-up, whole tile loaded up front: same results
#endif
    const bool no_defer = opt(OPT_NO_DEFER) != 0;
    if (asym) SLK_LDS_OPT_IN((k_gptq_window<true, true>), (window_lds<true, true>()));
    else if (grouped) SLK_LDS_OPT_IN((k_gptq_window<true, false>), (window_lds<true, false>()));
    else SLK_LDS_OPT_IN((k_gptq_window<false, false>), (window_lds<false, false>()));
    SLK_LDS_OPT_IN(k_gptq_window2<1>, sizeof(Window2SmemT<1>));
    SLK_LDS_OPT_IN(k_gptq_window2<2>, sizeof(Window2SmemT<2>));
    // 32 rows per workgroup (eight rows per chain wave, ONE quantizer instruction stream for them: leaf_chain8) halve the CUs
    // a window launch occupies for 1.45 times the duration (96 against 66 us at 4096 rows): less chip time per row, which is
    // what counts when other streams' kernels fill the CUs it leaves (round 3, every BASELINE stream on one MI355X: headline
    // 5040 -> 5180 Mweights/s, OPT-125M 5350 -> 5700, OPT-350M 4430 -> 4650, BLOOM-560M 3620 -> 3860) -- the default.  16
    // rows (four per chain wave) are faster for ONE layer alone: callers ask with SLK_LOOP_LATENCY (the single-layer API
    // does).  slk_set_option("window_rows", 16 | 32) forces either.
    // (fewer than 2048 rows -- the row shards of small layers on several ranks -- leave most CUs idle either way: what
    // counts then is the length of the launch chain, 16 rows again: one rank of 8 on OPT-125M 14.0 -> 12.6 ms per step)
    const int window_rows = opt(OPT_WINDOW_ROWS) == 16 || opt(OPT_WINDOW_ROWS) == 32 ? opt(OPT_WINDOW_ROWS)
                                                                                     : (((flags & SLK_LOOP_LATENCY) || R < 2048) ? 16 : 32);
    // the grouped loop runs on k_gptq_window alone (16 rows per workgroup whatever window_rows / SLK_LOOP_LATENCY ask)
    const bool periods_ok = !grouped && n % 2 == 0 && n <= 16384 && U_bits % 16 == 0 && !opt(OPT_NO_WINDOW2) && (dbg & ~(24 | 64 | 128)) == 0;

    // rows staged through LDS when they fit and 16-byte accesses line up
    const bool perm_lds = order && n % 4 == 0 && n <= PERM_MAX && (W_bits | (uintptr_t)Q | (uintptr_t)workspace) % 16 == 0 &&
                          (idx == nullptr || (uintptr_t)idx % 4 == 0);
    {
        const int rc = launch_permute("permute_in", 0, 8.0 * R * n, perm_lds ? k_permute_in<true> : k_permute_in<false>, perm_lds, R, n, s, lt, R,
                                      n, Qp, inv_order, rpl);
        if (rc != SLK_OK) return rc;
    }

    const int G = grouped ? n / group_size : 0;
    if (grouped)
        SLK_RUN("group_of_column", 0, 12.0 * batch * n, s,
                k_group_of_column<<<(batch * n + 255) / 256, 256, 0, s>>>(lt.order[0], batch, n, group_size, pg));

    Plan p;
    plan(0, n, min_block, num_blocks, p);
    const int row_tiles = (R + RB - 1) / RB;
    for (const Plan::Step &st : p.steps) {
        if (st.kind == 0) {
            // plan() cuts a window until its ops fit the table (a single leaf, however wide, is one op)
            SLK_REQUIRE(st.ops.size() <= (size_t)MAX_OPS, "a window of %d ops (the table holds %d)", (int)st.ops.size(), MAX_OPS);
            OpTable tab;
            tab.count = (int)st.ops.size();
            double fl = 0, ub = 0;  // float64 flops per row; bytes of U the window touches
            for (int i = 0; i < tab.count; ++i) {
                const Op &q = tab.op[i] = st.ops[i];
                if (q.kind == OP_LEAF) {
                    const double w = q.b - q.a;
                    fl += w * (w - 1);
                    ub += 4.0 * w * (w + 1);
                } else {
                    fl += 2.0 * (q.b - q.a) * (q.c - q.b);
                    ub += 8.0 * (q.b - q.a) * (q.c - q.b);
                }
            }
            // split every update at the end of the sibling sub-tree that follows it: the columns
            // beyond are not touched again before that sibling's own update (same c, a == this b)
            for (int i = 0; i < tab.count; ++i) {
                Op &q = tab.op[i];
                if (q.kind != OP_UPDATE) continue;
                q.m = q.c;
                q.nl = 1;
                if (no_defer) continue;
                int leaves = 0;
                for (int j = i + 1; j < tab.count; ++j) {
                    const Op &x = tab.op[j];
                    if (x.kind == OP_LEAF) ++leaves;
                    if (x.kind == OP_UPDATE && x.c == q.c && x.a == q.b) {
                        q.m = x.b;
                        q.nl = leaves > 0 ? leaves : 1;
                        break;
                    }
                }
            }
            const double wbytes = 12.0 * R * (st.b - st.a) + ub;  // Q in/out + E out, U once
            PeriodTable pt;
            if (st.b - st.a <= WMAX && periods_ok && as_periods(st.ops, st.a, st.b, pt)) {
                if (window_rows == 32)
                    SLK_RUN_W("gptq_window", fl * R, wbytes, (R + 2 * RB - 1) / (2 * RB), s,
                              k_gptq_window2<2><<<(R + 2 * RB - 1) / (2 * RB), 512, sizeof(Window2SmemT<2>), s>>>(
                                  Qp, Eg, lt, R, n, st.a, st.b, g, inv_step, fast_ok, dbg & (24 | 64 | 128), pt, rpl));
                else
                    SLK_RUN_W("gptq_window", fl * R, wbytes, row_tiles, s,
                              k_gptq_window2<1><<<row_tiles, 512, sizeof(Window2SmemT<1>), s>>>(Qp, Eg, lt, R, n, st.a, st.b, g, inv_step,
                                                                                             fast_ok, dbg & 24, pt, rpl));
            }
            else {
                const auto launch = asym ? launch_window<true, true> : grouped ? launch_window<true, false> : launch_window<false, false>;
                const int rc = launch(fl * R, wbytes, row_tiles, s, Qp, Eg, lt, R, n, st.a, st.b, g, inv_step, fast_ok, dbg, tab, rpl, gscale, pg, G,
                                      goffset);
                if (rc != SLK_OK) return rc;
            }
        } else {
            const double K = st.b - st.a, N = st.c - st.b;
            const int vec_ok = n % 4 == 0 && st.a % 4 == 0 && st.b % 2 == 0 && U_bits % 16 == 0;
            {
                dim3 grid((st.c - st.b + TILE - 1) / TILE, (R + TILE - 1) / TILE);
                SLK_RUN("gptq_trailing", 2.0 * R * K * N, 4.0 * R * K + 8.0 * K * N + 8.0 * R * N, s,
                        k_gptq_trailing<<<grid, 256, 0, s>>>(Qp, Eg, lt, R, n, st.a, st.b, st.b, st.c, vec_ok, rpl));
            }
        }
    }
    if (asym)
        SLK_RUN("permute_out_grouped_asym", 0, (idx ? 17.0 : 8.0) * R * n, s,
                k_permute_out_grouped<true><<<R < 2048 ? R : 2048, 256, 0, s>>>(Qp, inv_order, R, n, g, gscale, group_size, Q, idx, rpl,
                                                                               goffset));
    else if (grouped)
        SLK_RUN("permute_out_grouped", 0, (idx ? 13.0 : 8.0) * R * n, s,
                k_permute_out_grouped<<<R < 2048 ? R : 2048, 256, 0, s>>>(Qp, inv_order, R, n, g, gscale, group_size, Q, idx, rpl,
                                                                         nullptr));
    else {
        // the rows' errors ride on the last kernel: 8 R n bytes more (the rows of W and E) instead of a product of its own
        RowErrArgs ea{};
        if (row_err) {
            const int rc = loop_error_means(Hs, batch, n, hmean, s);
            if (rc != SLK_OK) return rc;
            ea = RowErrArgs{Eg, hmean, damp, row_err};
        }
        const auto kernel = row_err ? (perm_lds ? k_permute_out<true, true> : k_permute_out<false, true>)
                                    : (perm_lds ? k_permute_out<true, false> : k_permute_out<false, false>);
        const int rc = launch_permute(row_err ? "permute_out_error" : "permute_out", row_err ? 4.0 * R * n : 0,
                                      (row_err ? (idx ? 17.0 : 16.0) : (idx ? 9.0 : 8.0)) * R * n, kernel, perm_lds, R, n, s, Qp, inv_order, R, n, g,
                                      unscale, Q, idx, rpl, ea, lt);
        if (rc != SLK_OK) return rc;
    }
    if (E_out) copy_async(E_out, Eg, sizeof(float) * (size_t)R * n, s);
    return SLK_OK;
}

extern "C" int slk_gptq_quantize_batch(const float *W, const float *scale, const long long *order, const double *U,
                                       int batch, int rows_per_layer, int n, int levels, double lo, double hi,
                                       const float *table, int min_block, int num_blocks, int flags, float *Q, uint8_t *idx,
                                       float *E_out, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(W && U && Q, "null pointer");
    SLK_REQUIRE((flags & ~(SLK_LOOP_UNSCALE | SLK_LOOP_LATENCY)) == 0, "unknown flags");
    return gptq_loop(stacked_layers(W, scale, order, U, batch, rows_per_layer, n), batch, rows_per_layer, n, levels, lo, hi, table,
                     min_block, num_blocks, flags, Q, idx, E_out, workspace, ws_bytes, stream, nullptr, 0, nullptr);
}

// slk_gptq_quantize_batch that also leaves the rows' errors (W - Qw) H (W - Qw)^T, carried by the loop (k_permute_out<true>).
extern "C" int slk_gptq_quantize_batch_error(const float *W, const float *scale, const long long *order, const double *U,
                                             const float *const *H, float damp, int batch, int rows_per_layer, int n, int levels,
                                             double lo, double hi, const float *table, int min_block, int num_blocks, int flags,
                                             float *Q, uint8_t *idx, float *E_out, float *row_err, void *workspace, size_t ws_bytes,
                                             slk_stream_t stream) {
    SLK_REQUIRE(W && U && Q && H && row_err, "null pointer");
    SLK_REQUIRE((flags & ~(SLK_LOOP_UNSCALE | SLK_LOOP_LATENCY)) == 0, "unknown flags");
    SLK_REQUIRE(batch >= 1 && batch <= 64, "batch must be 1..64");
    for (int b = 0; b < batch; ++b) SLK_REQUIRE(H[b] != nullptr, "null Hessian (layer %d)", b);
    SLK_REQUIRE(scale == nullptr || (flags & SLK_LOOP_UNSCALE),
                "the carried error is that of the de-scaled Q: row scales need SLK_LOOP_UNSCALE");
    return gptq_loop(stacked_layers(W, scale, order, U, batch, rows_per_layer, n), batch, rows_per_layer, n, levels, lo, hi, table,
                     min_block, num_blocks, flags, Q, idx, E_out, workspace, ws_bytes, stream, nullptr, 0, nullptr, H, damp, row_err);
}

// The same loop over `batch` layers that lie anywhere in memory: HOST arrays of the layers' device pointers instead of stacks
// (scale may be nullptr: no scales; H and row_err both given: the error-carrying form).  Q, idx, E_out and row_err are
// written here and stay one stack.  Group scales stay with the stacked entries.
extern "C" int slk_gptq_quantize_layers(const float *const *W, const float *const *scale, const long long *const *order,
                                        const double *const *U, const float *const *H, float damp, const float *const *gscale,
                                        int group_size, int batch, int rows_per_layer, int n, int levels, double lo, double hi,
                                        const float *table, int min_block, int num_blocks, int flags, float *Q, uint8_t *idx,
                                        float *E_out, float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    SLK_REQUIRE(W && order && U && Q, "null pointer");
    SLK_REQUIRE(gscale == nullptr && group_size == 0,
                "group scales are not taken per layer: stack the layers (slk_gptq_quantize_grouped_batch)");
    SLK_REQUIRE((flags & ~(SLK_LOOP_UNSCALE | SLK_LOOP_LATENCY)) == 0, "unknown flags");
    SLK_REQUIRE(batch >= 1 && batch <= LOOP_LAYERS, "the layer table holds 1..%d layers (batch %d)", LOOP_LAYERS, batch);
    SLK_REQUIRE((H == nullptr) == (row_err == nullptr), "the carried error needs both the Hessians and row_err");
    SLK_REQUIRE(!H || scale == nullptr || (flags & SLK_LOOP_UNSCALE),
                "the carried error is that of the de-scaled Q: row scales need SLK_LOOP_UNSCALE");
    LayerTable lt{};
    for (int b = 0; b < batch; ++b) {
        SLK_REQUIRE(W[b] && order[b] && U[b] && (!scale || scale[b]) && (!H || H[b]), "null pointer (layer %d)", b);
        lt.W[b] = W[b], lt.scale[b] = scale ? scale[b] : nullptr, lt.order[b] = order[b], lt.U[b] = U[b];
    }
    return gptq_loop(lt, batch, rows_per_layer, n, levels, lo, hi, table, min_block, num_blocks, flags, Q, idx, E_out, workspace,
                     ws_bytes, stream, nullptr, 0, nullptr, H, damp, row_err);
}

// what both grouped entries ask of their arguments (`tables`: gscale, and goffset where there is one)
static int check_grouped(bool tables, const float *W, const double *U, const float *Q, int flags, int rows_per_layer, int n, int group_size) {
    SLK_REQUIRE(W && tables && U && Q, "null pointer");
    SLK_REQUIRE((flags & ~SLK_LOOP_LATENCY) == 0, "the grouped loop takes SLK_LOOP_LATENCY only");
    SLK_REQUIRE(rows_per_layer > 0 && n > 0, "empty layer");
    SLK_REQUIRE(group_size >= 1 && n % group_size == 0, "group_size must be >= 1 and divide n (%d columns, group_size %d)", n,
                group_size);
    return SLK_OK;
}

// `batch` layers with one scale per row and per group of `group_size` original columns (gscale: (batch rows_per_layer) x
// n / group_size, positive), stacked by rows like slk_gptq_quantize_batch.
extern "C" int slk_gptq_quantize_grouped_batch(const float *W, const float *gscale, int group_size, const long long *order,
                                               const double *U, int batch, int rows_per_layer, int n, int levels, double lo,
                                               double hi, const float *table, int min_block, int num_blocks, int flags, float *Q,
                                               uint8_t *idx, float *E_out, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    if (const int rc = check_grouped(gscale != nullptr, W, U, Q, flags, rows_per_layer, n, group_size)) return rc;
    return gptq_loop(stacked_layers(W, nullptr, order, U, batch, rows_per_layer, n), batch, rows_per_layer, n, levels, lo, hi, table,
                     min_block, num_blocks, flags, Q, idx, E_out, workspace, ws_bytes, stream, gscale, group_size, nullptr);
}

// One layer with group scales: the batch of one.
extern "C" int slk_gptq_quantize_grouped(const float *W, const float *gscale, int group_size, const long long *order, const double *U,
                                         int R, int n, int levels, double lo, double hi, const float *table, int min_block,
                                         int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out, void *workspace,
                                         size_t ws_bytes, slk_stream_t stream) {
    return slk_gptq_quantize_grouped_batch(W, gscale, group_size, order, U, 1, R, n, levels, lo, hi, table, min_block, num_blocks,
                                           flags, Q, idx, E_out, workspace, ws_bytes, stream);
}

// The asymmetric group quantizer: goffset (batch rows_per_layer) x n / group_size beside gscale, stacked by rows like
// slk_gptq_quantize_grouped_batch.
extern "C" int slk_gptq_quantize_grouped_asym_batch(const float *W, const float *gscale, const float *goffset, int group_size,
                                                    const long long *order, const double *U, int batch, int rows_per_layer, int n,
                                                    int levels, double lo, double hi, const float *table, int min_block,
                                                    int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out, void *workspace,
                                                    size_t ws_bytes, slk_stream_t stream) {
    if (const int rc = check_grouped(gscale && goffset, W, U, Q, flags, rows_per_layer, n, group_size)) return rc;
    return gptq_loop(stacked_layers(W, nullptr, order, U, batch, rows_per_layer, n), batch, rows_per_layer, n, levels, lo, hi, table,
                     min_block, num_blocks, flags, Q, idx, E_out, workspace, ws_bytes, stream, gscale, group_size, goffset);
}

// One layer with group scales and offsets: the batch of one.
extern "C" int slk_gptq_quantize_grouped_asym(const float *W, const float *gscale, const float *goffset, int group_size,
                                              const long long *order, const double *U, int R, int n, int levels, double lo, double hi,
                                              const float *table, int min_block, int num_blocks, int flags, float *Q, uint8_t *idx,
                                              float *E_out, void *workspace, size_t ws_bytes, slk_stream_t stream) {
    return slk_gptq_quantize_grouped_asym_batch(W, gscale, goffset, group_size, order, U, 1, R, n, levels, lo, hi, table, min_block,
                                                num_blocks, flags, Q, idx, E_out, workspace, ws_bytes, stream);
}
