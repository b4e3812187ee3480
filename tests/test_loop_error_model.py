"""The contract of the layer error the loop carries, pinned on the CPU independently of any kernel: the kernel's formula
in NumPy (loop_error_model.carried_row_errors) from the oracle's Q and E, against the float64 product.

Bounds: 1e-5 per row and 1e-6 on the layer mean, relative to float64 -- the bounds the GPU tests hold the layer error to.
Measured when this was written, on the cases below: worst row 9.7e-7, layer mean at most 4e-8 (the reference's own
float32 product is 2e-7 ... 1e-6 off float64 on such rows); decaying spectrum 1.6e-5 against the reference's 8.4e-4;
rank-deficient 2.1e-6.
"""

import numpy as np
import pytest

from sleekit_amd import synth

import loop_error_model as model
from oracle import obq_ref

# (R, n, seed, levels, strip the input mean)
CASES = [
    (256, 192, 4101, 8, False), (100, 320, 4102, 8, False), (48, 172, 4103, 8, False), (128, 1100, 4104, 8, False),
    (64, 2048, 4105, 8, False), (256, 768, 4106, 8, False),
    (256, 1024, 4107, 3, True),
    (128, 1024, 4108, 16, False), (128, 1024, 4108, 2, False),
    (64, 4096, 4109, 8, False), (64, 4096, 4109, 4, False),
    (16, 11008, 4110, 4, False),
]


@pytest.mark.parametrize("R,n,seed,levels,strip", CASES, ids=lambda v: str(v))
def test_carried_error_is_the_float64_product(R, n, seed, levels, strip):
    lay = synth.make_layer(R, n, seed)
    H = lay["H"]
    if strip:
        H = obq_ref.strip_input_mean(H, lay["mean"]).astype(np.float32)
        H = np.ascontiguousarray((H + H.T) / 2)  # (float32 H - m m^T is symmetric already; this keeps it so by construction)
    Qw, E = model.quantize(lay["W"], H, model.uniform(levels), lay["scale"])
    exact = model.product_row_errors(lay["W"], Qw, H)
    carried = model.carried_row_errors(lay["W"], Qw, E, H, 0.01, lay["scale"]).astype(np.float64)
    rows = np.abs(carried - exact) / exact
    mean = abs(carried.mean() - exact.mean()) / exact.mean()
    print(f"{R}x{n} levels {levels}: worst row {rows.max():.3g}, layer mean {mean:.3g}")
    assert rows.max() <= 1e-5
    assert mean <= 1e-6


def test_decaying_spectrum_no_farther_than_the_reference_float32():
    """A hard case: where the float32 product itself is far off float64, the carried error is held to being no farther from
    float64, on EVERY row, than the reference's own float32 row_errors is on its worst row."""
    n, R = 1024, 64
    H = model.decaying_hessian(n)
    assert np.array_equal(H, H.T)
    W = synth.make_weights(R, n, 4111)
    scale = synth.make_scale(W)
    Qw, E = model.quantize(W, H, model.uniform(8), scale)
    exact = model.product_row_errors(W, Qw, H)
    carried = model.carried_row_errors(W, Qw, E, H, 0.01, scale).astype(np.float64)
    reference = obq_ref.row_errors(W, Qw, H).astype(np.float64)  # float32 throughout, as obq.py:89-95 on float32 inputs
    rows = np.abs(carried - exact) / exact
    ref_rows = np.abs(reference - exact) / exact
    print(f"decaying spectrum: carried worst row {rows.max():.3g} (mean {rows.mean():.3g}); reference float32 worst row {ref_rows.max():.3g}")
    assert rows.max() <= ref_rows.max()


def test_rank_deficient_hessian():
    """n / 4 samples: H is singular, the damping term alone makes the factor; the identity still holds."""
    R, n = 64, 512
    lay = synth.make_layer(R, n, 4112, T=n // 4)
    Qw, E = model.quantize(lay["W"], lay["H"], model.uniform(8), lay["scale"])
    exact = model.product_row_errors(lay["W"], Qw, lay["H"])
    carried = model.carried_row_errors(lay["W"], Qw, E, lay["H"], 0.01, lay["scale"]).astype(np.float64)
    rows = np.abs(carried - exact) / exact
    print(f"rank-deficient: worst row {rows.max():.3g}")
    assert rows.max() <= 1e-5


def test_float32_sums_would_not_do():
    """Why the kernel sums in float64: the same formula with float32 sums is several times farther off."""
    lay = synth.make_layer(64, 2048, 4105)
    Qw, E = model.quantize(lay["W"], lay["H"], model.uniform(8), lay["scale"])
    exact = model.product_row_errors(lay["W"], Qw, lay["H"])
    carried = model.carried_row_errors(lay["W"], Qw, E, lay["H"], 0.01, lay["scale"]).astype(np.float64)
    lam = model.damping_term(lay["H"], 0.01)
    d = lay["W"] - Qw
    f32 = lay["scale"] * lay["scale"] * np.square(E).sum(axis=1, dtype=np.float32) - lam * np.square(d).sum(axis=1, dtype=np.float32)
    assert (np.abs(carried - exact) / exact).max() < (np.abs(f32.astype(np.float64) - exact) / exact).max()
