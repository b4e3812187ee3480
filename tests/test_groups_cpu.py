"""CPU checks of group-wise scales (sleekit_amd.groups): the module, the C ABI's argument checks, the absence of a CPU
path, and a NumPy model built from oracle.obq_ref pieces that reproduces the reference's grouped results in
tests/golden/groups.npz bit for bit (which pins the model the GPU tests reason with to the reference itself)."""

import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from groups_model import model_grouped, oracle_grid, rebuild

GROUPED = ("slk_gptq_quantize_grouped", "slk_column_miss_grouped", "slk_scale_search_grouped", "slk_dequantize_grouped")


def load_groups():
    data = np.load(os.path.join(GOLDEN, "groups.npz"))
    return data, json.loads(str(data["meta"]))


def test_module_and_symbols_exist():
    from sleekit_amd import _lib, groups

    for name in ("compute_group_scaling", "quantize_grouped", "dequantize_grouped"):
        assert callable(getattr(groups, name)), name
    for name in GROUPED:
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES, name
    assert _lib.lib.slk_abi_version() == 8
    import inspect

    import sleekit_amd

    sig = inspect.signature(sleekit_amd.Sleekit.quantize)
    assert list(sig.parameters)[-1] == "group_size" and sig.parameters["group_size"].default is None
    assert inspect.signature(groups.quantize_grouped).parameters["return_indices"].default is False


def test_argument_errors_come_back_before_any_launch():
    """SLK_E_ARG on the host: the (made-up, never dereferenced) addresses are not touched."""
    from sleekit_amd import _lib

    L = _lib.lib
    A = 4096  # a non-null address; every call below is refused before it could be used
    q = lambda W, S, g, n, flags=0, Q=A: L.slk_gptq_quantize_grouped(W, S, g, None, A, 64, n, 8, -1.0, 1.0, None, 32, 8, flags, Q,
                                                                      None, None, A, 1 << 30, None)
    assert q(None, A, 32, 128) == _lib.E_ARG
    assert q(A, None, 32, 128) == _lib.E_ARG
    assert q(A, A, 32, 128, Q=None) == _lib.E_ARG
    assert q(A, A, 0, 128) == _lib.E_ARG and b"group_size" in L.slk_last_error()
    assert q(A, A, -4, 128) == _lib.E_ARG
    assert q(A, A, 48, 128) == _lib.E_ARG and b"divide" in L.slk_last_error()
    assert q(A, A, 32, 128, flags=1) == _lib.E_ARG  # SLK_LOOP_UNSCALE: not a grouped flag
    assert L.slk_column_miss_grouped(A, A, 48, 64, 128, 8, -1.0, 1.0, None, 0, A, None) == _lib.E_ARG
    assert L.slk_column_miss_grouped(A, None, 32, 64, 128, 8, -1.0, 1.0, None, 0, A, None) == _lib.E_ARG
    assert L.slk_scale_search_grouped(A, A, A, 100, None, 0, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_scale_search_grouped(A, A, A, 100, None, 3, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_scale_search_grouped(None, A, A, 100, None, 32, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_dequantize_grouped(A, A, 0, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_dequantize_grouped(A, A, 32, 64, 128, 512, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_dequantize_grouped(None, A, 32, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG


def test_grouped_calls_have_no_cpu_path():
    import torch

    from sleekit_amd import codebook, groups

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cb = codebook.UniformCodebook(8, -1, 1)
    W = np.zeros((4, 8), np.float32)
    S = np.ones((4, 2), np.float32)
    H = np.eye(8, dtype=np.float32)
    for call in (
        lambda: groups.compute_group_scaling(W, cb, 4),
        lambda: groups.quantize_grouped(W, S, cb, H, 4),
        lambda: groups.dequantize_grouped(np.zeros((4, 8), np.uint8), S, cb, 4),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_numpy_model_reproduces_the_reference_fixtures():
    """Every case's Q to the reference's SHA-256; where the fixture keeps the indices, Q rebuilt from them as well."""
    from sleekit_amd import synth

    data, meta = load_groups()
    assert len(meta["cases"]) >= 30
    kept = 0
    for i, c in enumerate(meta["cases"]):
        L = synth.make_layer(c["R"], c["n"], c["seed"])
        S = data[f"S_{i}"]
        assert S.shape == (c["R"], c["n"] // c["g"]) and S.dtype == np.float32 and (S > 0).all()
        Q = model_grouped(L["W"], S, oracle_grid(c["codebook"]), L["H"], c["g"], c["act_order"], c["damp"], c["min_block_size"],
                          c["num_blocks"])
        assert Q.dtype == np.float32 and sha(Q) == c["sha256_Q"], f"case {i}: {c}"
        if f"idx_{i}" in data.files:
            kept += 1
            back = rebuild(data[f"idx_{i}"], S, c["codebook"], c["g"])
            assert np.array_equal(back.view(np.uint32), Q.view(np.uint32)), f"case {i}: indices"
    assert kept >= 8


def load_edges():
    data = np.load(os.path.join(GOLDEN, "groups_edges.npz"))
    return data, json.loads(str(data["meta"]))


def edge_layer(c):
    """The layer of an edge case: the synthetic generator's, with one group of weights zeroed where the case says so."""
    from sleekit_amd import synth

    L = synth.make_layer(c["R"], c["n"], c["seed"])
    if c["zero_group"] is not None:
        k, g = c["zero_group"], c["g"]
        L["W"][:, k * g:(k + 1) * g] = 0
    return L


def test_numpy_model_reproduces_the_edge_fixtures():
    """groups_edges.npz (ragged rows, odd and tiny groups, widths off a multiple of 4, leaves of 1 to 550 columns, every
    order, 2 to 256 levels and nf4, zero groups): the model's Q to the reference's SHA-256, its indices to the reference's
    where kept, and the per-group pick_scale to the reference's S bit for bit."""
    from groups_model import group_scales_model, indices

    data, meta = load_edges()
    cases = meta["cases"]
    assert len(cases) >= 16
    assert {c["act_order"] for c in cases} >= {"none", "diag", "err", "sqerr", "pivot", "inv_diag", "combined_diag"}
    assert {c["codebook"] for c in cases} >= {"2", "3", "16", "256", "nf4"}
    assert sum(c["zero_group"] is not None for c in cases) >= 2
    kept = 0
    for i, c in enumerate(cases):
        L = edge_layer(c)
        grd = oracle_grid(c["codebook"])
        S = data[f"S_{i}"]
        assert S.shape == (c["R"], c["n"] // c["g"]) and S.dtype == np.float32 and (S > 0).all()
        if c["zero_group"] is not None:  # the floor of the scale search: 1e-16, times the smallest factor after a search
            floor = np.float32(1e-16) if c["mode"] == "max" else np.float32(1e-16) * np.float32(0.05)
            assert (S[:, c["zero_group"]] == floor).all(), f"case {i}"
        want_S = group_scales_model(L["W"], grd, L["H"], c["g"], c["mode"])
        assert np.array_equal(want_S.view(np.uint32), S.view(np.uint32)), f"case {i}: scales"
        Q = model_grouped(L["W"], S, grd, L["H"], c["g"], c["act_order"], c["damp"], c["min_block_size"], c["num_blocks"])
        assert sha(Q) == c["sha256_Q"], f"case {i}: {c}"
        # no exact key ties: the stable-tie order (the device's) gives the same Q
        Qs = model_grouped(L["W"], S, grd, L["H"], c["g"], c["act_order"], c["damp"], c["min_block_size"], c["num_blocks"],
                           ties="stable")
        assert sha(Qs) == c["sha256_Q"], f"case {i}: stable ties"
        if f"idx_{i}" in data.files:
            kept += 1
            assert np.array_equal(indices(Q, S, grd, c["g"]), data[f"idx_{i}"]), f"case {i}: indices"
            back = rebuild(data[f"idx_{i}"], S, c["codebook"], c["g"])
            assert np.array_equal(back.view(np.uint32), Q.view(np.uint32)), f"case {i}: rebuild"
    assert kept >= 10
