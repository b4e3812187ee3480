// What the products over an MX layer share across files (mxgemm.hip: coded activations on the block-scaled MFMA;
// mxgemm_a16.hip: 16-bit activations on the bf16 / f16 MFMA): where the few-rows form ends, and the expert-grouped forms'
// row tiles -- the checks, the prologue that turns offsets into the two tables (k_mx_expert_tiles, mxgemm.hip) and one
// table entry as a tile body's arguments.
#pragma once

#include "common.h"
#include "mxquant.h"

namespace slk {

constexpr int MXG_SK = 8;             // the waves of a split-K workgroup, which share K
constexpr int MXG_SPLIT_MAX_M = 64;   // up to here the split-K form over 16 rows, above it the 64 x 64 tile

// What the expert-grouped entries require on top of the dense ones (M is positive by then)
int mx_check_experts(int E, int M, const int *offsets, const void *workspace, size_t ws_bytes);

// The prologue of every expert-grouped product: k_mx_expert_tiles on the stream, and what the two launches behind it need --
// host-computable upper bounds of the tile counts as grid rows, and the two tables (their counts are ws[0] and ws[1]).
struct ExpertGrid {
    int rows16, rows64;
    const int *t16, *t64;
};
int mx_expert_prologue(const int *offsets, int E, int M, int *ws, int *flag, hipStream_t s, ExpertGrid &g);

// One row tile of one expert: the dense kernels' bodies on that expert's layer, bias and row bound.
template <int WF>
struct ExpertTile {
    const uint8_t *Wc, *Ws;
    const float *bias;
    int row0, rows;
    __device__ __forceinline__ ExpertTile(const int *__restrict__ table, const uint8_t *__restrict__ w_codes,
                                          const uint8_t *__restrict__ w_scales, const float *__restrict__ b, int N, int K) {
        const int *entry = table + 3 * (size_t)blockIdx.y;
        const size_t e = (size_t)entry[0], blocks = (size_t)N * (K / 32);
        Wc = w_codes + e * blocks * (4 * mxa_bits<WF>()), Ws = w_scales + e * blocks;  // 16 or 24 bytes of codes a block
        bias = b ? b + e * N : nullptr;
        row0 = entry[1], rows = entry[2];
    }
};

}  // namespace slk
