"""NumPy model of the fused gate/up product in front of a rotated down layer (sleekit_amd.mx: matmul_mx_glu(rotation=);
slk_mx_gemm_glu_rot), composed of the models that exist: the float32 hidden activations as mx_glu_model.hidden_model makes
them (the exact sums, + bias in float32, the gate in float32), rotation_model.transform on them (steps 1 to 3 of
slk_hadamard_rows in float32, no rounding after them), and the quantizer model of the activations' format.  Nothing here is
a reference of its own."""

import numpy as np

import mx_glu_model
import rotation_model


def hidden_f32(sums, bias, alpha=1.0, limit=None, shift=0.0, interleaved=False):
    """The float32 h that mx_glu_model.hidden_model quantizes: its own three lines up to the quantizer."""
    Y = sums.astype(np.float32)
    assert (Y.astype(np.float64) == sums).all(), "the model takes sums that are exact in float32"
    if bias is not None:
        Y = Y + np.asarray(bias, np.float32)[None, :]
    return mx_glu_model.glu_f32(Y, alpha, limit, shift, interleaved)


def hidden_rot_model(sums, bias, activations, block, signs=None, alpha=1.0, limit=None, shift=0.0, interleaved=False):
    """(h_codes, h_scales) of float64 sums that float32 holds exactly, behind the rotation (block, signs of the N hidden columns)."""
    h = hidden_f32(sums, bias, alpha, limit, shift, interleaved)
    return mx_glu_model.QUANTIZE[activations](rotation_model.transform(h, block, signs))
