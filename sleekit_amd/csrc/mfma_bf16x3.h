// float32-grade products on the bfloat16 MFMA: each float32 operand is split into three bfloat16 pieces
// (a = a1 + a2 + a3 exactly, to 24 bits) and the product takes the six piece products above 2^-24,
//     a b ~ a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1),
// every one exact in float32, accumulated in float32 by v_mfma_f32_32x32x16_bf16 (smallest terms first).
// Measured (tools/scratch/mfma_bf16.hip): error / sum|a b| = 9e-8 ... 1.7e-7 for K = 512 ... 4096, the same as a
// sequential float32 fma chain (1.3e-7).  The bfloat16 MFMA does 16x the float32 MFMA's flops per cycle, so six
// terms cost 3/8 of the float32 instruction stream.
//
// One 256-thread workgroup accumulates a 128 x 128 tile; wave w owns the 64 x 64 sub-tile (w >> 1, w & 1) as
// 2 x 2 blocks of 32 x 32.  BOTH operands are given K-contiguous: A[row][k] and Bt[col][k] (the callers' B is
// symmetric, so B[k][col] = B[col][k] and its rows serve), already split into three bfloat16 planes in the
// slab order of k_split3 (splitting in the loop was measured: 656 us against 550, the vector ALU work of
// 7.5 instructions per element and tile).  K goes in steps of 32 through LDS: three planes per operand,
// [row][32 k] bfloat16 with a pitch of 80 bytes, which makes the 16-byte operand reads (lane l: row l & 31,
// k group l >> 5) conflict-free over ds_read_b128's 16-lane groups.
//
// Operand maps of v_mfma_f32_32x32x16_bf16 (checked by the scratch program above):
//   A: lane l holds A[row = l & 31][k = 8 (l >> 5) .. + 7]    B: lane l holds B[k = 8 (l >> 5) .. + 7][col = l & 31]
//   D: as v_mfma_f32_32x32x2_f32 (mfma32.h)
#pragma once

#include <type_traits>

#include "mfma32.h"

namespace slk {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned uint4v_t __attribute__((ext_vector_type(4)));

constexpr int KB16 = 32;          // K depth per LDS round
constexpr int PITCH_B16 = 80;     // bytes per staged row of one plane (64 of data)

struct TileBf16Smem {
    unsigned char a[3][T32 * PITCH_B16];
    unsigned char b[3][T32 * PITCH_B16];
};

// Two floats -> three words holding their bfloat16 pieces pairwise (round to nearest even at each level:
// v_cvt_pk_bf16_f32, gfx950's hardware conversion; the residuals x - piece are exact in float32).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3_pair(float x, float y, unsigned &w1, unsigned &w2, unsigned &w3) {
    const __bf16 x1 = (__bf16)x, y1 = (__bf16)y;
    const float rx = x - (float)x1, ry = y - (float)y1;
    const __bf16 x2 = (__bf16)rx, y2 = (__bf16)ry;
    const float sx = rx - (float)x2, sy = ry - (float)y2;
    const __bf16 x3 = (__bf16)sx, y3 = (__bf16)sy;
    w1 = __builtin_bit_cast(unsigned, (bf16x2_t){x1, y1});
    w2 = __builtin_bit_cast(unsigned, (bf16x2_t){x2, y2});
    w3 = __builtin_bit_cast(unsigned, (bf16x2_t){x3, y3});
}

// The six piece products of one 32 x 32 block over 16 k, smallest terms first (pieces 3·1, 2·2, 1·3, 2·1, 1·2, 1·1):
// both stagings below issue exactly this on the same accumulators in the same K order, so they agree bit for bit.
__device__ __forceinline__ void mfma_bf16x3(float16_t &acc, const bf16x8_t (&a)[3], const bf16x8_t (&b)[3]) {
    float16_t c = acc;
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    acc = c;
}

// acc += A(128 x K) * Bt(128 x K)^T from operands split beforehand (k_split3 in sgemm.hip): plane p of A is a
// bfloat16 image A_p[row][k] in slabs, likewise Bt_p[col][k].  Both stagings take the operands the same way:
// a_slabs / b_slabs: this tile's slab of K-step 0 in plane 0 -- 128 rows x 32 k, 4096 elements; consecutive K-steps are
// 4096 elements apart, the planes a_plane / b_plane.
//
// Staged through registers.  The loop has no vector arithmetic at all: six 16-byte loads per operand and round,
// twelve LDS writes, the reads and the MFMAs.
__device__ __forceinline__ void tile128_mac_bf16_staged(Acc128 &acc, TileBf16Smem &sm, int k_begin, int k_end,
                                                        const unsigned short *__restrict__ a_slabs, size_t a_plane,
                                                        const unsigned short *__restrict__ b_slabs, size_t b_plane) {
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // v[p][h] = 16 bytes h of plane p of this thread's row (t >> 1) of the slab, k = k0 + 16 (t & 1) + 8 h ...
    auto load = [&](const unsigned short *slabs, size_t plane, int k0, uint4v_t(&v)[3][2]) {
        const unsigned short *q = slabs + (size_t)(k0 >> 5) * 4096 + (size_t)t * 16;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h) v[p][h] = *reinterpret_cast<const uint4v_t *>(q + p * plane + 8 * h);
    };
    auto la = [&](int k0, uint4v_t(&v)[3][2]) { load(a_slabs, a_plane, k0, v); };
    auto lb = [&](int k0, uint4v_t(&v)[3][2]) { load(b_slabs, b_plane, k0, v); };
    // A round's MFMAs last ~0.7 us, less than a trip to memory: the loads run TWO rounds ahead, in two register
    // sets used in turn.  Rounds go in pairs and every load is issued unconditionally (clamped to the last
    // round), so that the compiler can count what is in flight (s_waitcnt vmcnt(12), not 0).
    uint4v_t ra0[3][2], rb0[3][2], ra1[3][2], rb1[3][2];
    const int s_off = (t >> 1) * PITCH_B16 + (t & 1) * 32;
    if (k_begin >= k_end) return;
    const int k_last = k_end - KB16;
    la(k_begin, ra0);
    lb(k_begin, rb0);
    la(min(k_begin + KB16, k_last), ra1);
    lb(min(k_begin + KB16, k_last), rb1);
    const int r_off = (lane & 31) * PITCH_B16 + (lane >> 5) * 16;
    auto stash = [&](const uint4v_t(&va)[3][2], const uint4v_t(&vb)[3][2]) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                *reinterpret_cast<uint4v_t *>(sm.a[p] + s_off + 16 * h) = va[p][h];
                *reinterpret_cast<uint4v_t *>(sm.b[p] + s_off + 16 * h) = vb[p][h];
            }
    };
    auto mac = [&]() {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8_t a[2][3], b[2][3];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    a[i][p] = *reinterpret_cast<const bf16x8_t *>(sm.a[p] + (wr * 64 + i * 32) * PITCH_B16 + r_off + s * 32);
                    b[i][p] = *reinterpret_cast<const bf16x8_t *>(sm.b[p] + (wc * 64 + i * 32) * PITCH_B16 + r_off + s * 32);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mfma_bf16x3(acc.c[i][j], a[i], b[j]);
        }
    };
    // pairs of rounds, then the single round an odd count leaves
    int k0 = k_begin;
    for (; k0 + 2 * KB16 <= k_end; k0 += 2 * KB16) {
        __syncthreads();
        stash(ra0, rb0);
        __syncthreads();
        la(min(k0 + 2 * KB16, k_last), ra0);
        lb(min(k0 + 2 * KB16, k_last), rb0);
        mac();
        __syncthreads();
        stash(ra1, rb1);
        __syncthreads();
        la(min(k0 + 3 * KB16, k_last), ra1);
        lb(min(k0 + 3 * KB16, k_last), rb1);
        mac();
    }
    if (k0 < k_end) {  // one round left: its operands are in set 0
        __syncthreads();
        stash(ra0, rb0);
        __syncthreads();
        mac();
    }
}

// ---- the same product with the operands brought to LDS by the memory pipeline itself (global_load_lds_dwordx4).
// LDS writes are slow (80 bytes a cycle against 256 for reads, profiles/r01_lds_access_microbench.txt): staged through
// registers a round costs 48 ds_write_b128 a workgroup -- more LDS time than all its operand reads -- and 96 VGPRs
// of staging (230 -> 122 VGPRs here).  Measured: error GEMM 520 -> 493 us, Hessian accumulation 0.786 -> 0.771 ms; no
// more, because at 128 x 128 tiles the kernel moves 48 KB from L2 per 6.3 Mflop round -- it runs at the rate the
// CUs can pull operands out of L2 (32 bytes a cycle and CU), not at the LDS's or the MFMA's.  A slab of k_split3 (128 rows x 32 k of one plane, 8 KB contiguous) is instead copied
// verbatim, eight 1 KB wave instructions; no padding is possible in such an image, so the planes are stored
// SWIZZLED: the 16-byte chunk c (of 4) of row r sits at chunk c ^ ((r >> 2) & 3), which makes the operand reads
// (lane l: row l & 31, chunk (l >> 5) + 2 s) conflict-free -- the eight quads of a half-wave split into two sets of
// four with disjoint banks.
struct TileBf16DmaSmem {
    unsigned char a[3][8192];
    unsigned char b[3][8192];
};
__device__ __forceinline__ int swizzled_chunk(int row, int c) { return c ^ ((row >> 2) & 3); }

// SLK_BF16_COPY_AFTER_HALF = 1 (round 4): every operand read of a round is issued up front (a scheduling barrier keeps hipcc from
// sinking the second k-half's reads to their MFMAs), the MFMAs of the first k-half run while the second half's reads land,
// and only then comes the barrier behind which the next round's copy is issued.  Same MFMAs in the same order.  Layer error
// of a 4096 x 4096 layer, alternating on one box: 449 / 474 / 457 us -> 443 / 409 / 423.  (0: wait for all reads, barrier, copy,
// then the round's MFMAs.)
#ifndef SLK_BF16_COPY_AFTER_HALF
#define SLK_BF16_COPY_AFTER_HALF 1
#endif
__device__ __forceinline__ void tile128_mac_bf16_dma(Acc128 &acc, TileBf16DmaSmem &sm, int k_begin, int k_end,
                                                    const unsigned short *__restrict__ a_slabs, size_t a_plane,
                                                    const unsigned short *__restrict__ b_slabs, size_t b_plane) {
    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    if (k_begin >= k_end) return;
    // this wave's quarter of a slab: 2 KB = two instructions of 64 lanes x 16 bytes
    const unsigned short *ga = a_slabs + (size_t)(k_begin >> 5) * 4096 + wave * 1024 + lane * 8;
    const unsigned short *gb = b_slabs + (size_t)(k_begin >> 5) * 4096 + wave * 1024 + lane * 8;
    const int sw = ((lane & 31) >> 2) & 3;
    const int r_off0 = (lane & 31) * 64 + (((lane >> 5) ^ sw) * 16), r_off1 = (lane & 31) * 64 + ((((lane >> 5) + 2) ^ sw) * 16);
    // One LDS buffer, but the copy of round r + 1 is in flight while the MFMAs of round r run: the operands of a round are
    // read into registers first (barrier: every wave has them), THEN the next round's copy is issued, then the MFMAs.
    // (Measured against issuing the copy at the top of the round and waiting for it there: 0.441 against 0.445 ms for the
    // layer error of a 4096 x 4096 layer -- the three workgroups of a CU already overlap one another's copies; what bounds
    // the kernel is the rate at which a CU pulls operands out of L2, 48 KB per 6.3 Mflop round.)
    auto copy_round = [&](const unsigned short *pa, const unsigned short *pb) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_global_load_lds(pa + p * a_plane + i * 512, sm.a[p] + wave * 2048 + i * 1024, 16, 0, 0);
                __builtin_amdgcn_global_load_lds(pb + p * b_plane + i * 512, sm.b[p] + wave * 2048 + i * 1024, 16, 0, 0);
            }
    };
    __syncthreads();  // whatever used this LDS before is done
    copy_round(ga, gb);
    for (int k0 = k_begin; k0 < k_end; k0 += KB16) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's copies have landed before it passes the barrier
        __syncthreads();
        bf16x8_t a[2][2][3], b[2][2][3];  // [s][i][plane]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    a[s][i][p] = *reinterpret_cast<const bf16x8_t *>(sm.a[p] + (wr * 64 + i * 32) * 64 + (s ? r_off1 : r_off0));
                    b[s][i][p] = *reinterpret_cast<const bf16x8_t *>(sm.b[p] + (wc * 64 + i * 32) * 64 + (s ? r_off1 : r_off0));
                }
        ga += 4096, gb += 4096;
        if (SLK_BF16_COPY_AFTER_HALF) __builtin_amdgcn_sched_barrier(0);  // every read of the round is issued before its first MFMA
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s == SLK_BF16_COPY_AFTER_HALF && k0 + KB16 < k_end) {
                // (the reads above must have completed in EVERY wave before the copy overwrites the buffer)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();
                copy_round(ga, gb);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mfma_bf16x3(acc.c[i][j], a[s][i], b[s][j]);
        }
    }
}

// The one entry: DMA chooses the staging, smem_raw is the workgroup's sizeof(TileBf16<DMA>) bytes of LDS (16-byte aligned).
template <bool DMA>
using TileBf16 = std::conditional_t<DMA, TileBf16DmaSmem, TileBf16Smem>;
template <bool DMA>
__device__ __forceinline__ void tile128_mac_bf16(Acc128 &acc, unsigned char *smem_raw, int k_begin, int k_end,
                                                 const unsigned short *__restrict__ a_slabs, size_t a_plane,
                                                 const unsigned short *__restrict__ b_slabs, size_t b_plane) {
    TileBf16<DMA> &sm = *reinterpret_cast<TileBf16<DMA> *>(smem_raw);
    if constexpr (DMA) tile128_mac_bf16_dma(acc, sm, k_begin, k_end, a_slabs, a_plane, b_slabs, b_plane);
    else tile128_mac_bf16_staged(acc, sm, k_begin, k_end, a_slabs, a_plane, b_slabs, b_plane);
}

}  // namespace slk
