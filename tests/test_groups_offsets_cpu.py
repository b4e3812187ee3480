"""CPU checks of asymmetric group quantization (an offset per row and group beside the scale): the module and the C ABI's
argument checks, the stream's refusal of `goffset`, and a NumPy model built from oracle pieces that reproduces the
reference's results in tests/golden/groups_offsets.npz bit for bit (which pins the model the GPU tests reason with)."""

import hashlib
import inspect
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from groups_offsets_model import offsets_model, rebuild, shaped_layer

ASYM = ("slk_gptq_quantize_grouped_asym", "slk_gptq_quantize_grouped_asym_batch", "slk_column_miss_grouped_asym",
        "slk_dequantize_grouped_asym", "slk_group_midpoints", "slk_group_center")


def load():
    data = np.load(os.path.join(GOLDEN, "groups_offsets.npz"))
    return data, json.loads(str(data["meta"]))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_keywords_and_symbols_exist():
    import sleekit_amd
    from sleekit_amd import _lib, groups

    assert callable(groups.compute_group_offsets)
    for fn in (groups.compute_group_scaling, groups.quantize_layer_grouped, groups.run_loop_batch_grouped, groups.dequantize_grouped):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "offsets" and params["offsets"].default is None, fn.__name__
    # quantize_grouped keeps its parameter list; its offset form is a sibling.  Sleekit.quantize keeps group_size last.
    assert "offsets" not in inspect.signature(groups.quantize_grouped).parameters
    assert list(inspect.signature(groups.quantize_grouped_asym).parameters)[:3] == ["W", "S", "O"]
    params = inspect.signature(sleekit_amd.Sleekit.quantize).parameters
    assert list(params)[-2:] == ["offsets", "group_size"] and params["offsets"].default is None
    for name in ASYM:
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES, name
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_come_back_before_any_launch():
    """SLK_E_ARG on the host: the (made-up, never dereferenced) addresses are not touched."""
    from sleekit_amd import _lib

    L = _lib.lib
    A = 4096
    q = lambda W, S, O, g, n, flags=0, Q=A: L.slk_gptq_quantize_grouped_asym(W, S, O, g, None, A, 64, n, 8, -1.0, 1.0, None, 32, 8,
                                                                             flags, Q, None, None, A, 1 << 30, None)
    assert q(None, A, A, 32, 128) == _lib.E_ARG
    assert q(A, None, A, 32, 128) == _lib.E_ARG
    assert q(A, A, None, 32, 128) == _lib.E_ARG and b"null" in L.slk_last_error()
    assert q(A, A, A, 32, 128, Q=None) == _lib.E_ARG
    assert q(A, A, A, 0, 128) == _lib.E_ARG and b"group_size" in L.slk_last_error()
    assert q(A, A, A, 48, 128) == _lib.E_ARG and b"divide" in L.slk_last_error()
    assert q(A, A, A, 32, 128, flags=1) == _lib.E_ARG
    b = lambda batch, rpl, order=A: L.slk_gptq_quantize_grouped_asym_batch(A, A, A, 32, order, A, batch, rpl, 128, 8, -1.0, 1.0, None,
                                                                          32, 8, 0, A, None, None, A, 1 << 30, None)
    assert b(0, 64) == _lib.E_ARG and b"batch" in L.slk_last_error()
    assert b(65, 64) == _lib.E_ARG
    assert b(2, 48) == _lib.E_ARG and b"multiple of 64" in L.slk_last_error()
    assert b(2, 64, order=None) == _lib.E_ARG and b"orders" in L.slk_last_error()
    cm = L.slk_column_miss_grouped_asym
    assert cm(A, A, None, 32, 64, 128, 8, -1.0, 1.0, None, 0, A, None) == _lib.E_ARG
    assert cm(A, A, A, 48, 64, 128, 8, -1.0, 1.0, None, 0, A, None) == _lib.E_ARG
    assert cm(A, A, A, 32, 64, 128, 1, -1.0, 1.0, None, 0, A, None) == _lib.E_ARG and b"levels" in L.slk_last_error()
    dq = L.slk_dequantize_grouped_asym
    assert dq(A, A, None, 32, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert dq(A, A, A, 0, 64, 128, 8, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert dq(A, A, A, 32, 64, 128, 512, -1.0, 1.0, None, A, None) == _lib.E_ARG
    assert L.slk_group_midpoints(None, 32, 64, 128, A, None, None) == _lib.E_ARG
    assert L.slk_group_midpoints(A, 32, 64, 128, None, None, None) == _lib.E_ARG
    assert L.slk_group_midpoints(A, 48, 64, 128, A, None, None) == _lib.E_ARG and b"divide" in L.slk_last_error()
    assert L.slk_group_midpoints(A, 32, 0, 128, A, None, None) == _lib.E_ARG
    assert L.slk_group_center(A, A, 32, 64, 128, None, None) == _lib.E_ARG
    assert L.slk_group_center(A, None, 32, 64, 128, A, None) == _lib.E_ARG
    assert L.slk_group_center(A, A, 0, 64, 128, A, None) == _lib.E_ARG


def test_stream_refuses_group_offsets():
    """check_layers runs before anything: a layer carrying `goffset` is refused alike on every rank."""
    import torch

    from sleekit_amd import dist

    W = torch.zeros((4, 8))
    lay = dict(W=W, gscale=torch.ones((4, 2)), group_size=4, goffset=torch.zeros((4, 2)))
    with pytest.raises(NotImplementedError, match="goffset"):
        dist.check_layers([dict(W=W), lay])
    with pytest.raises(NotImplementedError, match="goffset"):
        dist.check_layers([dict(W=W, goffset=torch.zeros((4, 2)))])
    dist.check_layers([dict(W=W, gscale=torch.ones((4, 2)), group_size=4)])  # without it: as before


def test_fixture_cases_cover_the_issue():
    data, meta = load()
    cases = meta["cases"]
    assert {c["act_order"] for c in cases} >= {"none", "diag", "err", "sqerr", "inv_diag", "pivot"}
    assert {c["codebook"] for c in cases} >= {"2", "3", "8", "16", "256", "nf4"}
    assert {c["mode"] for c in cases} >= {"max", "mse", "diag", "hessian"}
    assert {c["variant"] for c in cases} >= {"pos", "const", "huge"}
    assert any(c["R"] % 16 for c in cases) and any(c["g"] == 1 for c in cases) and any(c["g"] == c["n"] for c in cases)
    for i, c in enumerate(cases):
        if c["variant"] == "huge":  # the absorbed group: |o| / s >= 2^20
            O, S = data[f"O_{i}"], data[f"S_{i}"]
            assert (np.abs(O[:, 1]) / S[:, 1]).min() >= 2**20
        if c["variant"] == "const":
            assert (data[f"S_{i}"][:, 1] <= 1e-15).all()
    assert meta["large"] is not None and meta["large"]["n"] == 4096


def test_model_reproduces_the_reference():
    data, meta = load()
    for i, c in enumerate(meta["cases"]):
        L = shaped_layer(c["R"], c["n"], c["g"], c["seed"], c["variant"])
        O, S, Q = offsets_model(L["W"], L["H"], c["codebook"], c["g"], c["act_order"], c["mode"], c["damp"], c["min_block_size"],
                                c["num_blocks"])
        assert np.array_equal(bits(O), bits(data[f"O_{i}"])), f"case {i}: O"
        assert np.array_equal(bits(S), bits(data[f"S_{i}"])), f"case {i}: S"
        assert sha(Q) == c["sha256_Q"], f"case {i}: {c}"
        if f"idx_{i}" in data:
            back = rebuild(data[f"idx_{i}"], S, O, c["codebook"], c["g"])
            assert np.array_equal(bits(back), bits(Q)), f"case {i}: the stored indices do not rebuild Q"
