"""NumPy model of the gated MLP's middle (sleekit_amd.mx: glu, matmul_mx_glu; slk_mx_glu, slk_mx_gemm_glu), from the rules alone.

The gate, in the stated operation order, every operation rounded once:
    g' = g > limit ? limit : g                          (a NaN passes through; limit None: no clamp)
    u' = u > limit ? limit : (u < -limit ? -limit : u)
    s  = 1 / (1 + exp(-(alpha g')))
    h  = (u' + shift) (g' s)
gate_f32 runs it in float32 (NumPy's float32 exp is not the GPU's: bit for bit only where exp is exact, alpha = 0), gate_f64 in
float64 on the same float32 inputs and the float32 values of alpha, limit and shift (the bound's reference).

Layouts: hidden column j of N takes gate = column j and up = column N + j of the 2 N, or, interleaved, 2 j and 2 j + 1.

The fused product is three existing pieces: the matmul of mx_experts_model (one expert: the dense models of every format pair),
the gate in float32, and the quantizer model of the activations' format.  It is exact -- the only right answer -- where the
sums are exact in float32 and exp is (tests/test_gpu_mx_glu.py, check 1).
"""

import numpy as np

import mx_act4_model
import mx_act6_model
import mx_experts_model
import mx_gemm_model

SWIGLU = dict(alpha=1.0, limit=None, shift=0.0)
GPT_OSS = dict(alpha=1.702, limit=7.0, shift=1.0)
QUANTIZE = {"mxfp8": mx_gemm_model.quantize_act_model, "mxfp4": mx_act4_model.quantize_act4_model,
            "mxfp6_e2m3": mx_act6_model.quantize_act6_model}


def _gate(g, u, alpha, limit, shift, T):
    g, u = np.asarray(g, np.float32).astype(T), np.asarray(u, np.float32).astype(T)
    alpha, shift = T(np.float32(alpha)), T(np.float32(shift))
    lim = T(np.float32(np.inf if limit is None else limit))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        gc = np.where(g > lim, lim, g)
        uc = np.where(u > lim, lim, np.where(u < -lim, -lim, u))
        t = alpha * gc
        s = T(1) / (T(1) + np.exp(-t))
        a = uc + shift
        b = gc * s
        h = a * b
    assert h.dtype == T
    return h


def gate_f32(g, u, alpha=1.0, limit=None, shift=0.0):
    return _gate(g, u, alpha, limit, shift, np.float32)


def gate_f64(g, u, alpha=1.0, limit=None, shift=0.0):
    return _gate(g, u, alpha, limit, shift, np.float64)


def columns(N, interleaved):
    """(gate columns, up columns) of the N hidden columns among 2 N."""
    j = np.arange(N)
    return (2 * j, 2 * j + 1) if interleaved else (j, N + j)


def split(Y, interleaved=False):
    """(gate, up), each (..., N), of Y (..., 2 N)."""
    assert Y.shape[-1] % 2 == 0
    gc, uc = columns(Y.shape[-1] // 2, interleaved)
    return Y[..., gc], Y[..., uc]


def glu_f32(Y, alpha=1.0, limit=None, shift=0.0, interleaved=False):
    return gate_f32(*split(Y, interleaved), alpha, limit, shift)


def glu_f64(Y, alpha=1.0, limit=None, shift=0.0, interleaved=False):
    return gate_f64(*split(Y, interleaved), alpha, limit, shift)


def sums_model(a_codes, a_scales, codes, scales, activations="mxfp8", weights="mxfp4"):
    """The 2 N gate and up sums without bias, float64 (M, 2 N): mx_experts_model's matmul with one expert."""
    M = a_codes.shape[0]
    return mx_experts_model.matmul_model(a_codes, a_scales, codes[None], scales[None], np.array([0, M], np.int32), None, activations, weights)[0]


def hidden_model(sums, bias, activations, alpha=1.0, limit=None, shift=0.0, interleaved=False):
    """(h_codes, h_scales) of float64 sums that float32 holds exactly: + bias (float32 addition), the gate in float32, the
    quantizer model of the activations' format."""
    Y = sums.astype(np.float32)
    assert (Y.astype(np.float64) == sums).all(), "the model takes sums that are exact in float32"
    if bias is not None:
        Y = Y + np.asarray(bias, np.float32)[None, :]
    return QUANTIZE[activations](glu_f32(Y, alpha, limit, shift, interleaved))


def matmul_glu_model(a_codes, a_scales, codes, scales, bias=None, activations="mxfp8", weights="mxfp4", alpha=1.0, limit=None, shift=0.0,
                     interleaved=False):
    return hidden_model(sums_model(a_codes, a_scales, codes, scales, activations, weights), bias, activations, alpha, limit, shift, interleaved)
