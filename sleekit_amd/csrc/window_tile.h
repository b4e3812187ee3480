// What the two window kernels (k_gptq_window in gptq.hip, k_gptq_window2 in window2.h) are both made of: the shape of a
// tile, the register leaf chain and the staging of its tables, the tile's load and write-back, the lap counters and the
// 16-row MFMA update.
#pragma once

#include <stdint.h>

#include <type_traits>

#include "mfma64.h"

namespace slk {

constexpr int WMAX = 512;     // widest window held in LDS
constexpr int WPITCH = WMAX + 4;
constexpr int RB = 16;        // rows per window workgroup
constexpr int ULEAF = 32;     // leaves up to this width stage their U block in LDS

struct LeafTables {
    double u[ULEAF][ULEAF + 1];  // leaf block of U, STRICTLY upper part (zero on/below the diagonal and beyond the width)
    double udr[ULEAF][2];        // its diagonal (1 beyond the width) and 1 / diagonal by true division
    __device__ __forceinline__ static int col(int j) { return j; }  // where column j of a row of u sits
};

// codebook.py:56-65 with the divide replaced by Markstein's sequence: with y = RN(1/step),
//   q0 = RN(t0 y);  r = t0 - step q0 (exact in one fma);  t = RN(q0 + r y) == RN(t0 / step)
// for every t0 whose quotient neither overflows nor underflows (rint of an underflowing
// quotient is 0 either way).  Saves ~40 dependent cycles per column on the leaf's critical
// path.  tests/test_gpu_parity.py::test_fast_quantizer_matches_true_divide sweeps it against
// the true-divide kernel.  The clamp is one v_med3 (the leaf chain counts instructions).
__device__ __forceinline__ float grid_value_fast(float x, const Grid g, float inv_step) {
    const float t0 = x - g.zero;
    const float q0 = t0 * inv_step;
    const float r = __builtin_fmaf(-g.step, q0, t0);
    float t = __builtin_fmaf(r, inv_step, q0);
    t = rintf(t);
    t = __builtin_amdgcn_fmed3f(t, 0.0f, g.top);
    return t * g.step + g.zero;
}

// A column's error float64(x - q) / uii (obq.py:112).  FAST: the exact-division fma sequence with rii = RN(1 / uii) taken
// once per leaf by a true division (exact unless uii's significand is all ones, which the caller has excluded).
template <bool FAST>
__device__ __forceinline__ double chain_err(float x, float q, double uii, double rii) {
    const double d = (double)(x - q);
    if constexpr (FAST) {
        const double qq = d * rii;
        const double rem = __builtin_fma(-uii, qq, d);
        return __builtin_fma(rem, rii, qq);
    } else {
        return d / uii;
    }
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// lane L of every 16-lane row, to all lanes of that row (DPP row_newbcast, gfx90a and later)
template <int L>
__device__ __forceinline__ float row_bcast(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + L, 0xf, 0xf, true));
}

// the per-row quantizer: nothing to read per step
struct LeafRows {
    struct Step {};
    __device__ __forceinline__ Step at(int, int, int) const { return {}; }
    template <bool FAST>
    __device__ __forceinline__ static float q(float x, Step, const Grid g, float inv_step) {
        return FAST ? grid_value_fast(x, g, inv_step) : cb_value(x, g);
    }
};

// LEAF, register path (width <= 32, tables in LDS): a chain wave owns FOUR rows, 16 lanes per row; lane c16 keeps
// columns c16 and 16 + c16 of its row's leaf in x0 and x1.  Step i: column i's value is broadcast inside its
// 16-lane DPP row, every lane recomputes q_i and err_i for its own row (no second broadcast), then
// updates its two columns:  x_c <- float32(float64(x_c) - err_i * U[i][c])   (obq.py:114-118)
// FAST: Markstein divisions (chain_err, grid_value_fast); otherwise true divides / table look-ups.
// The loop is issue-bound (~35 instructions a step with the per-step selection this chain no longer has), which is why
// four rows share a wave and, in k_gptq_window, the other four waves of the workgroup stay parked at the barrier: two
// waves per SIMD would just take turns (measured 430 -> ~230 cycles/step).
// Steps beyond the width run on the padding (x = 0, U row = 0, diagonal = 1; the group tables
// read 1.0 / slot GSLOTS there: a finite error that meets a zero U row) and change nothing: no per-step branch,
// so the whole leaf is one basic block and the LDS reads of step i + 1 (U row, diagonal,
// reciprocal, the policy's step) are issued before the arithmetic of step i.
// The policy P is the quantizer: P::Step is what a step reads from LDS besides U (read one step
// ahead, like the U row), pol.at(row, a, k) reads it for column a + k of tile row `row`, and P::q<FAST>(x, step, g, inv_step)
// forms q.  (The tile's reads take a and k apart: one base address for s and rs, k in the offsets.)
// On return q0, e0 (q1, e1) are the quantized value and scaled error of columns c16 (16 + c16); loading x and storing
// q and e is the caller's.
template <int NSTEP, bool FAST, class P>
__device__ __forceinline__ void leaf_chain16(const LeafTables &lt, const P &pol, int row, int a, int c16, float x0, float x1, float &q0,
                                             float &q1, float &e0, float &e1, const Grid g, float inv_step) {
    static_assert(FAST || std::is_same<P, LeafRows>::value, "the group quantizers' slow path is the generic leaf");
    double u0n = lt.u[0][c16], u1n = lt.u[0][c16 + 16], uiin = lt.udr[0][0], riin = lt.udr[0][1];
    typename P::Step sn = pol.at(row, a, 0);
    static_for<0, NSTEP>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const double u0 = u0n, u1 = u1n, uii = uiin, rii = riin;
        const typename P::Step sc = sn;
        if constexpr (i + 1 < NSTEP) {
            u0n = lt.u[i + 1][c16];
            u1n = lt.u[i + 1][c16 + 16];
            uiin = lt.udr[i + 1][0];
            riin = lt.udr[i + 1][1];
            sn = pol.at(row, a, i + 1);
        }
        // the chain values pass through this point: the reads above are issued before step i starts
        asm volatile("" : "+v"(x0), "+v"(x1)::"memory");
        // column i of each of the wave's rows, broadcast inside its 16-lane DPP row; every lane recomputes the
        // column's error for its own row.  The chain is bound by the ISSUE of these instructions: nothing is kept
        // per step (the column's own q and e come after the loop, below)
        const float xi = row_bcast<(i & 15)>(i < 16 ? x0 : x1);
        const double err = chain_err<FAST>(xi, P::template q<FAST>(xi, sc, g, inv_step), uii, rii);
        // the staged block is zero on and below the diagonal: only later columns move
        if (i < 15) x0 = (float)((double)x0 - err * u0);
        if (NSTEP > 16) x1 = (float)((double)x1 - err * u1);
    });
    // A lane's own columns are final once their step has passed: the block of U is zero on and below the diagonal, so
    // the later steps subtract err * 0 (at most the sign of a zero changes, which no result can see).  Their q and e
    // are the same expressions on the same value as in the step that broadcast it: computed once here instead of being
    // selected into place in every step (two v_cndmask and a conversion per step less on the chain).  The policy's step
    // of a lane's own column is a run-time k into the same tables.
    q0 = P::template q<FAST>(x0, pol.at(row, a, c16), g, inv_step);
    e0 = (float)chain_err<FAST>(x0, q0, lt.udr[c16][0], lt.udr[c16][1]);
    if constexpr (NSTEP > 16) {
        q1 = P::template q<FAST>(x1, pol.at(row, a, c16 + 16), g, inv_step);
        e1 = (float)chain_err<FAST>(x1, q1, lt.udr[c16 + 16][0], lt.udr[c16 + 16][1]);
    }
}

// ---- staging of a leaf's tables by the 256 helper threads (ht = 0 ... 255): thread ht carries the slots e = ht + 256 h,
// h < 4, of the 32 x 32 block, slot e = (row e >> 5, column e & 31).
// registers <- U[a : a + w, a : a + w], w >= 1 (clamped, selected when written)
__device__ __forceinline__ void fetch_leaf_block(const double *__restrict__ U, int n, int a, int w, int ht, double (&pu)[4]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int e = ht + 256 * h, i = min(e >> 5, w - 1), j = min(e & 31, w - 1);
        pu[h] = U[(size_t)(a + i) * n + a + j];
    }
}
// table <- registers, all 32 x 32 slots (w = 0: an empty leaf).  Returns whether a diagonal entry met by this WAVE defeats
// the exact-division shortcut: a significand that is all ones.
template <class Tables>
__device__ __forceinline__ bool write_leaf_tables(Tables &lt, const double (&pu)[4], int w, int ht) {
    // a thread meets at most one diagonal slot (e = 33 i): one division, not four
    double dgv = 1.0;
    int di = -1;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int e = ht + 256 * h, i = e >> 5, j = e & 31;
        const bool in = i < w && j < w;
        lt.u[i][Tables::col(j)] = (in && j > i) ? pu[h] : 0.0;
        if (i == j) {
            dgv = in ? pu[h] : 1.0;
            di = i;
        }
    }
    bool odd = false;
    if (di >= 0) {
        lt.udr[di][0] = dgv;
        lt.udr[di][1] = 1.0 / dgv;
        odd = (__double_as_longlong(dgv) & 0xFFFFFFFFFFFFFLL) == 0xFFFFFFFFFFFFFLL;
    }
    return __builtin_amdgcn_ballot_w64(odd) != 0;
}

// ---- the tile between global memory and LDS: ROWS rows from row r0 of the R x n arrays, columns from w0 at q[.][0]
// 16-byte accesses need rows and the window's first column to line up
__device__ __forceinline__ bool tile_vec4(const float *base, int n, int w0) {
    return n % 4 == 0 && (w0 & 3) == 0 && ((uintptr_t)base & 15) == 0;
}
// columns [c_lo, c_hi) of the Q tile, global -> LDS (zero beyond row R), by `nth` threads of which this is number `tid`:
// 16-byte loads when the layout allows (vec4: tile_vec4 of Qp), eight (four) loads in flight per thread either way
// (a load-wait-store loop pays the full latency per element)
template <int ROWS>
__device__ __forceinline__ void load_tile_cols(float (*q)[WPITCH], const float *__restrict__ Qp, int r0, int R, int n, int w0, bool vec4,
                                               int c_lo, int c_hi, int tid, int nth) {
    const int cw = c_hi - c_lo;
    if (vec4 && (c_lo & 3) == 0 && (cw & 3) == 0) {
        const int cw4 = cw >> 2, total = ROWS * cw4;
        for (int e0 = tid; e0 < total; e0 += 4 * nth) {
            float4v_t v[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int e = min(e0 + h * nth, total - 1);
                const int r = e / cw4, c = c_lo + 4 * (e % cw4);
                v[h] = *reinterpret_cast<const float4v_t *>(Qp + (size_t)min(r0 + r, R - 1) * n + c);
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int e = e0 + h * nth;
                const int r = e / cw4, c = c_lo + 4 * (e % cw4);
                if (e < total) *reinterpret_cast<float4v_t *>(&q[r][c - w0]) = (r0 + r < R) ? v[h] : (float4v_t){0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        return;
    }
    const int total = ROWS * cw;
    for (int e0 = tid; e0 < total; e0 += 8 * nth) {
        float v[8];
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int e = min(e0 + h * nth, total - 1);
            const int r = e / cw, c = c_lo + e % cw;
            v[h] = Qp[(size_t)min(r0 + r, R - 1) * n + c];
        }
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int e = e0 + h * nth;
            const int r = e / cw, c = c_lo + e % cw;
            if (e < total) q[r][c - w0] = (r0 + r < R) ? v[h] : 0.0f;
        }
    }
}
// the first `width` columns of a tile, LDS -> global, by all 512 threads (vec4: tile_vec4 of dst)
template <int ROWS>
__device__ __forceinline__ void store_tile(const float (*q)[WPITCH], float *__restrict__ dst, int r0, int R, int n, int w0, int width,
                                           bool vec4, int t) {
    if (vec4 && (width & 3) == 0) {
        const int cw4 = width >> 2;
        for (int e = t; e < ROWS * cw4; e += 512) {
            const int r = e / cw4, c = 4 * (e % cw4);
            if (r0 + r < R) *reinterpret_cast<float4v_t *>(dst + (size_t)(r0 + r) * n + w0 + c) = *reinterpret_cast<const float4v_t *>(&q[r][c]);
        }
    } else {
        for (int e = t; e < ROWS * width; e += 512) {
            const int r = e / width, c = e % width;
            if (r0 + r < R) dst[(size_t)(r0 + r) * n + w0 + c] = q[r][c];
        }
    }
}

// cycle counters of workgroup 0 (SLK_WIN_DBG bit 3), read back by slk_probe_window_cycles
__device__ long long g_win_cycles[16];
__device__ long long g_win_trace[64];  // window2: busy cycles per period, chain wave 0 / helper wave 2 (+32)

// Cycle accounting (debug): wave-uniform accumulators of workgroup 0, added to g_win_cycles once at the end by waves 0 and 4
// (slot 9: wave 0's whole run).
struct Laps {
    bool on;
    long long mark, start;
    long long acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ explicit Laps(int dbg) : on((dbg & 8) && blockIdx.x == 0) {
        mark = start = on ? (long long)__builtin_readcyclecounter() : 0;
    }
    // adds the cycles since the last mark to counter `slot` (where `mine`) and moves the mark
    __device__ __forceinline__ void lap(int slot, bool mine = true) {
        if (on) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (mine) acc[slot] += now - mark;
            mark = now;
        }
    }
    __device__ __forceinline__ void flush(int lane, int wave) {
        if (on && lane == 0 && (wave == 0 || wave == 4)) {
            if (wave == 0) acc[9] += (long long)__builtin_readcyclecounter() - start;
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (acc[k]) g_win_cycles[k] += acc[k];
        }
    }
};

// ---- the 16-row MFMA update: Q[:, lo:hi] -= E[:, a:b] @ U[a:b, lo:hi] on SETS tiles of 16 rows, Q and E in LDS.
// A ROUND is (16-column block, 64-deep K chunk).  Operands of U come straight from global memory (every workgroup streams the
// same panel out of L2), so the loads of the rounds after are in flight during the MFMAs of a round; the round of U in
// registers serves every one of the SETS tiles.
// Tile is the kernel's view of its LDS: q(st, row, col) and e(st, row, k) point at Q[row][col] and E[row][k] of tile st
// (window columns), straight(k) says whether the 32 columns of E from k on lie side by side there.
// off32: the layer is at most 16384 columns wide, so that byte offsets into U fit 32 bits ((n^2 - 1) * 8 < 2^32 up to
// n = 23170).
// EAGER: see run().
template <int SETS, class Tile, bool EAGER>
struct TileUpdate {
    const Tile tile;
    const double *U;
    const int n;
    const bool off32;
    const int lr, lk;  // lane & 15, lane >> 4
    double cur[16];    // the round a run starts with

    __device__ __forceinline__ void load_round(int a, int b, int lo, int hi, int blk, int kc, double (&bv)[16]) const {
        // Clamped addresses, no masking: rows beyond b meet a zero E operand, columns beyond hi are
        // never stored -- and any arithmetic on the loaded value here would make the wave wait for
        // the load at once instead of after the MFMAs of the round before.
        // (Scalar per-row-group bases with one vector offset were tried to take the address arithmetic
        // off the vector ALU, which the float64 MFMA shares: the SALU chain it needs is slower, 36 vs 31 us.)
        // The waves that run this share their SIMDs' issue slots with the chain waves, so the address arithmetic counts: a
        // full chunk of 64 rows (the common case) is read at a uniform base + a 32-bit byte offset that advances by a
        // constant (one v_add_u32 per load; the clamped form below costs an add, a min, a 64-bit multiply-add and a 64-bit
        // shift-add each).
        const int cc = min(lo + blk * 16 + lr, hi - 1);
        const int kbase = a + 64 * kc;
        if (off32 && kbase + 64 <= b) {
            const char *Ubytes = reinterpret_cast<const char *>(U);
            const unsigned row4 = 32u * (unsigned)n;  // bytes from row k to row k + 4
            unsigned off = ((unsigned)(kbase + lk) * (unsigned)n + (unsigned)cc) * 8u;
#pragma unroll
            for (int s4 = 0; s4 < 16; ++s4) {
                bv[s4] = *reinterpret_cast<const double *>(Ubytes + off);
                off += row4;
            }
            return;
        }
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) {
            const int k = kbase + 4 * s4 + lk;
            bv[s4] = U[(size_t)min(k, b - 1) * n + cc];
        }
    }
    // one round of MFMAs: acc += E[:, chunk kc of a:b] @ bv.  Full and half chunks (K = 64, 32: all
    // the reference's default schedules) take straight-line code: 16 (8) LDS reads, then the MFMAs.
    __device__ __forceinline__ void mac_round(int a, int b, int kc, const double (&bv)[16], double4_t (&acc)[SETS]) const {
        const int kbase = a + 64 * kc, kcount = min(64, b - kbase);
        if ((kcount == 64 || kcount == 32) && tile.straight(kbase)) {
#pragma unroll
            for (int st = 0; st < SETS; ++st) {
                const float *ep = tile.e(st, lr, kbase) + lk;
                float av[16];
#pragma unroll
                for (int s4 = 0; s4 < 8; ++s4) av[s4] = ep[4 * s4];
                if (kcount == 64) {
#pragma unroll
                    for (int s4 = 8; s4 < 16; ++s4) av[s4] = ep[4 * s4];
                }
#pragma unroll
                for (int s4 = 0; s4 < 8; ++s4) acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[s4], bv[s4], acc[st], 0, 0, 0);
                if (kcount == 64) {
#pragma unroll
                    for (int s4 = 8; s4 < 16; ++s4) acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[s4], bv[s4], acc[st], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int s4 = 0; s4 < 16; ++s4) {
                const int k = kbase + 4 * s4 + lk;
#pragma unroll
                for (int st = 0; st < SETS; ++st) {
                    const float ev = *tile.e(st, lr, min(k, b - 1));  // clamped: the load is unconditional, the value is selected
                    const double av = k < b ? (double)ev : 0.0;
                    if (4 * s4 < kcount) acc[st] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[s4], acc[st], 0, 0, 0);
                }
            }
        }
    }
    __device__ __forceinline__ void store_block(int lo, int hi, int blk, double4_t (&acc)[SETS]) const {  // and clear the accumulators
        const int col = lo + blk * 16 + lr;
#pragma unroll
        for (int st = 0; st < SETS; ++st) {
            if (col < hi) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float *qp = tile.q(st, lk + 4 * r, col);
                    *qp = (float)((double)*qp - acc[st][r]);
                }
            }
            acc[st] = (double4_t){0.0, 0.0, 0.0, 0.0};
        }
    }
    // Blocks wid, wid + nw, ... of [lo, hi); `ready`: cur already holds (block wid, chunk 0).
    // Rounds in pairs on two register buffers.  EAGER: the loads of the round after next are issued
    // UNCONDITIONALLY (clamped to the last round when there is none): with a fixed number of loads
    // between a buffer's fill and its use the compiler can wait with vmcnt(16); a conditional
    // load in the loop makes it fall back to vmcnt(0), which serialises load and MFMA.  That pays where a run is long
    // (k_gptq_window2's helpers: the rest of the window).  The general kernel's runs are mostly one or two rounds a wave
    // (a 32- or 64-column urgent part over eight waves), where two rounds of loads that nobody uses triple the traffic:
    // not EAGER there (measured).
    __device__ __forceinline__ void run(int a, int b, int lo, int hi, int wid, int nw, bool ready) {
        const int nblk = (hi - lo + 15) / 16, nchunk = (b - a + 63) / 64;
        if (wid >= nblk) return;
        const int nr = (nblk - wid + nw - 1) / nw * nchunk;
        const int last_blk = wid + ((nblk - wid - 1) / nw) * nw;
        double other[16];
        if (!ready) load_round(a, b, lo, hi, wid, 0, cur);
        double4_t acc[SETS];
#pragma unroll
        for (int st = 0; st < SETS; ++st) acc[st] = (double4_t){0.0, 0.0, 0.0, 0.0};
        int blk = wid, kc = 0;
        for (int r = 0; r < nr; r += 2) {
            int blk1 = blk, kc1 = kc + 1;
            if (kc1 == nchunk) kc1 = 0, blk1 += nw;
            const bool has1 = r + 1 < nr;
            if (EAGER || has1) load_round(a, b, lo, hi, has1 ? blk1 : last_blk, has1 ? kc1 : nchunk - 1, other);
            mac_round(a, b, kc, cur, acc);
            if (kc + 1 == nchunk) store_block(lo, hi, blk, acc);
            int blk2 = blk1, kc2 = kc1 + 1;
            if (kc2 == nchunk) kc2 = 0, blk2 += nw;
            const bool has2 = r + 2 < nr;
            if (EAGER || has2) load_round(a, b, lo, hi, has2 ? blk2 : last_blk, has2 ? kc2 : nchunk - 1, cur);
            if (has1) {
                mac_round(a, b, kc1, other, acc);
                if (kc1 + 1 == nchunk) store_block(lo, hi, blk1, acc);
            }
            blk = blk2, kc = kc2;
        }
    }
};

}  // namespace slk
