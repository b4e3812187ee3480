// The gate of a gated MLP, down(act(gate(x)) * up(x)), as one float32 function: every kernel that gates -- the streaming
// slk_mx_glu of mx.hip and the epilogues of slk_mx_gemm_glu / _experts in mxgemm.hip -- calls mx_glu and nothing else, so the
// fused product and its three-step route give the same bits.
//
//   g' = g > limit ? limit : g                          (a NaN passes through; limit = +inf: no clamp)
//   u' = u > limit ? limit : (u < -limit ? -limit : u)
//   s  = 1 / (1 + exp(-(alpha g')))
//   h  = (u' + shift) (g' s)
//
// alpha = 1, limit = +inf, shift = 0 is SwiGLU (silu(g) u); alpha = 1.702, limit = 7, shift = 1 is the gpt-oss form.
// Every operation is rounded once, in this order: no multiply is contracted with an add (the pragma below, whatever the
// file's flags), the division is the IEEE one, and exp is expf at every site (alpha = 0: exp(-0) = 1 and s = 0.5 exactly).
#pragma once

#include "common.h"

namespace slk {

struct GluParams {
    float alpha, limit, shift;
    int interleaved;  // 0: hidden column j takes gate j and up N + j of the 2 N; 1: gate 2 j and up 2 j + 1
};

__device__ __forceinline__ float mx_glu(float g, float u, const GluParams p) {
#pragma clang fp contract(off)
    const float gc = g > p.limit ? p.limit : g;
    const float uc = u > p.limit ? p.limit : (u < -p.limit ? -p.limit : u);
    const float t = p.alpha * gc;
    const float s = 1.0f / (1.0f + expf(-t));
    const float a = uc + p.shift;
    const float b = gc * s;
    return a * b;
}

// (the entries' check of alpha and shift: x - x is 0 for a finite x and NaN for the rest)
static inline bool glu_finite(float x) { return x - x == 0.0f; }

// the gate and up rows (or columns) of hidden column j among the 2 N
__device__ __forceinline__ int glu_gate_of(int j, int N, int interleaved) { return interleaved ? 2 * j : j; }
__device__ __forceinline__ int glu_up_of(int j, int N, int interleaved) { return interleaved ? 2 * j + 1 : N + j; }

}  // namespace slk
