"""MXFP4 without a GPU: the NumPy model (tests/mx_model.py) against the reference's own results (tests/golden/mx.npz,
tests/golden/make_golden_mx.py) -- every scale byte, the indices after the loop and after the moves, the packed codes --
the format's known answers, the C entry points' argument checks and the Python layer's refusals.  The device kernels are
held to the fixtures and to the model in tests/test_gpu_mx.py."""

import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mx_model  # noqa: E402
from groups_ls_model import local_search_grouped, trace_of  # noqa: E402
from groups_model import model_grouped  # noqa: E402
from ls_evidence import explain_rows  # noqa: E402

FIX = np.load(os.path.join(HERE, "golden", "mx.npz"))
META = json.loads(str(FIX["meta"]))
CASES = META["cases"]
ROOT = os.path.dirname(HERE)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def row_hashes(idx):
    return np.array([int.from_bytes(hashlib.sha256(np.ascontiguousarray(r).tobytes()).digest()[:8], "little") for r in idx],
                    dtype=np.uint64)


def case_inputs(i):
    """W, H (float32) and the reference's scales S of fixture case i."""
    L = mx_model.case_layer(CASES[i])
    return L["W"].astype(np.float32), L["H"].astype(np.float32), mx_model.decode_model(FIX[f"E_{i}"])


def near(i):
    return {k: FIX[f"near_{i}/{k}"] for k in ("rows", "choice", "runner", "ratio")}


def check_indices(i, idx, trace=None):
    """idx: the final indices of case i; trace: the moves taken (search cases).  Bit for bit the reference's, except rows
    one of whose decisions was a proven near-tie (tests/ls_evidence.py).  Returns the rows that differ."""
    c = CASES[i]
    bad = np.flatnonzero(row_hashes(idx) != FIX[f"row_hash_{i}"])
    if f"idx_{i}" in FIX:
        assert np.array_equal(np.flatnonzero((idx != FIX[f"idx_{i}"]).any(axis=1)), bad)
    if c["moves"] == 0:
        assert len(bad) == 0 and sha(idx) == c["sha256_idx"], f"case {i}: {c}"
    else:
        explain_rows(bad, trace, near(i))
    return bad


def check_codes(i, codes, bad):
    """The packed codes against the reference's (where every row is the reference's)."""
    if len(bad) == 0:
        assert sha(codes) == CASES[i]["sha256_codes"], f"case {i}: codes"


def test_fixture_cover():
    assert len(CASES) >= 20
    assert {c["act_order"] for c in CASES} >= {"none", "diag", "err", "sqerr", "pivot", "inv_diag", "combined_diag"}
    assert {c["mode"] for c in CASES} == {"max", "mse", "diag"}
    assert {c["moves"] for c in CASES} >= {0, 10, 100}
    assert {c["n"] for c in CASES if c["moves"]} >= {768, 1024, 3072, 96}
    assert min(c["R"] for c in CASES) == 1 and min(c["n"] for c in CASES) == 32 and max(c["n"] for c in CASES) == 4096
    assert {(c["special"] or [None])[0] for c in CASES} >= {"zero", "negative", "outlier"}
    assert all(v > 0 for v in META["factors_chosen"].values()) and len(META["factors_chosen"]) == 4
    assert any(f"idx_{i}" not in FIX for i in range(len(CASES)))
    assert os.path.getsize(os.path.join(HERE, "golden", "mx.npz")) <= 150 * 1024


def test_known_answers():
    from sleekit_amd import mx

    assert mx.BLOCK == 32 and len(mx.E2M1) == 15
    assert mx.E2M1.values.tolist() == mx_model.VALUES
    assert mx.E2M1.thresholds.tolist() == [-5, -3.5, -2.5, -1.75, -1.25, -0.75, -0.25, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5]
    assert "".join(f"{c:x}" for c in mx_model.codes_of(np.arange(15))) == "fedcba901234567"
    assert mx_model.indices_of(np.arange(16)).tolist() == [7, 8, 9, 10, 11, 12, 13, 14, 7, 6, 5, 4, 3, 2, 1, 0]
    assert mx_model.codes_of(np.array([15, 200])).tolist() == [7, 7]
    idx = np.full((1, 32), 7, np.uint8)
    idx[0, :4] = mx_model.indices_of(np.array([1, 2, 0xF, 0]))
    codes, scales = mx_model.pack_model(idx, np.array([[0.0078125]], np.float32))
    assert codes[0, :2].tolist() == [0x21, 0x0F] and not codes[0, 2:].any() and scales.tolist() == [[120]]
    assert mx_model.decode_model(np.array([[120, 71, 253, 127]], np.uint8)).tolist() == [[2.0 ** -7, 2.0 ** -56, 2.0 ** 126, 1.0]]
    for bad in (3.0, 0.0, -1.0, np.inf, 2.0 ** -127):
        with pytest.raises(ValueError):
            mx_model.encode_model(np.array([[bad]], np.float32))
    # a tie goes upward: 0.25 is index 8 (0.5), -0.25 is index 7 (0); code 0x8 reads as +0
    g = mx_model.e2m1_grid()
    assert g.index(np.array([0.25, -0.25, 5.0, -5.0, -0.0], np.float32)).tolist() == [8, 7, 14, 1, 7]
    back = mx_model.dequantize_model(np.array([[0x08] + [0] * 15], np.uint8), np.array([[127]], np.uint8))
    assert not back.view(np.uint32).any()
    # the header and the integration notes state the format with these answers
    for name in (os.path.join("include", "sleekit_amd.h"), "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        for needle in ("f e d c b a 9 0 1 2 3 4 5 6 7", "0x21", "0.0078125", "120", "E8M0", "E2M1"):
            assert needle in text, (name, needle)


def test_scale_floor_and_all_negative_blocks():
    for i, c in enumerate(CASES):
        E = FIX[f"E_{i}"]
        assert E.dtype == np.uint8 and E.shape == (c["R"], c["n"] // 32) and E.min() >= 71 and E.max() <= 253
        if c["special"] and c["special"][0] == "zero":
            assert (E[:, c["special"][1]] == (74 if c["mode"] == "max" else 71)).all()
        if c["special"] and c["special"][0] == "negative":
            W = case_inputs(i)[0]
            assert (W[:, :32] < 0).all()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_model_reproduces_the_reference(i):
    """The reference's scale bytes, its indices after the loop (SHA-256), after the moves (row by row) and its codes."""
    c = CASES[i]
    W, H, S = case_inputs(i)
    Sm, Em = mx_model.scales_model(W, H, c["mode"])
    assert np.array_equal(Em, FIX[f"E_{i}"]) and np.array_equal(Sm.view(np.uint32), S.view(np.uint32)), f"case {i}: scales"
    L = mx_model.case_layer(c)
    grd = mx_model.e2m1_grid()
    Q0 = model_grouped(L["W"], S, grd, L["H"], 32, c["act_order"], c["damp"], c["min_block_size"], c["num_blocks"])
    s = np.repeat(S, 32, axis=1)
    assert sha(grd.index(Q0 / s).astype(np.uint8)) == c["sha256_idx0"], f"case {i}: loop"
    records = []
    Q = local_search_grouped(W, Q0, S, grd, H, 32, c["moves"], records)
    idx = grd.index(Q / s).astype(np.uint8)
    bad = check_indices(i, idx, trace_of(records) if records else None)
    assert c["moves"] == 0 or len(bad) <= len(near(i)["rows"])
    codes, E = mx_model.pack_model(idx, S)
    check_codes(i, codes, bad)
    # Q is +-magnitude * 2^(b - 127) bit for bit, and the packed form gives the indices and the scales back
    assert np.array_equal(mx_model.dequantize_model(codes, E).view(np.uint32), Q.view(np.uint32))
    back_idx, back_S = mx_model.unpack_model(codes, E)
    assert np.array_equal(back_idx, idx) and np.array_equal(back_S, S)
    if f"idx_{i}" in FIX:
        assert sha(mx_model.pack_model(FIX[f"idx_{i}"], S)[0]) == c["sha256_codes"]


def test_codes_are_the_four_bit_packing_of_the_codes():
    from packing_model import pack_model as pack_bits

    rng = np.random.default_rng(4)
    idx = rng.integers(0, 15, (5, 96)).astype(np.uint8)
    codes, _ = mx_model.pack_model(idx, np.ones((5, 3), np.float32))
    assert np.array_equal(codes, pack_bits(mx_model.codes_of(idx), 4).view(np.uint8).reshape(5, -1))


def test_module_and_symbols_exist():
    import inspect

    import sleekit_amd
    from sleekit_amd import _lib, mx

    for name in ("slk_mx_scale_search", "slk_mx_pack", "slk_mx_unpack", "slk_mx_dequantize"):
        assert hasattr(_lib.lib, name) and name in _lib.PROTOTYPES, name
    assert _lib.lib.slk_abi_version() == 8
    for name in ("compute_mx_scales", "quantize_mxfp4", "pack_mxfp4", "unpack_mxfp4", "dequantize_mxfp4", "encode_scales",
                 "decode_scales"):
        assert callable(getattr(mx, name)), name
    assert sleekit_amd.mx is mx and mx.MXResult._fields == ("Q", "idx", "S", "codes", "scales")
    sig = inspect.signature(mx.quantize_mxfp4)
    assert list(sig.parameters) == ["W", "H", "act_order", "damp", "scale_mode", "nb_ls_moves", "scales", "min_block_size", "num_blocks"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:]] == ["diag", 0.01, "mse", 0, None, 32, 8]
    sig = inspect.signature(sleekit_amd.Sleekit.quantize_mxfp4)
    assert list(sig.parameters) == ["self", "scale_mode", "order_mode", "bias_correction", "damp", "nb_ls_moves"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[1:]] == ["mse", "diag", False, 0.01, 0]


def test_argument_errors_do_not_touch_the_gpu():
    """Bad arguments are rejected on the host before any launch (safe without a GPU)."""
    from sleekit_amd import _lib

    L, A = _lib.lib, 4096  # (a non-null, 16-byte aligned address that is never dereferenced: each call fails its checks first)
    for R, n in ((4, 48), (4, 0), (0, 32), (-1, 32), (4, 31)):
        assert L.slk_mx_scale_search(A, None, _lib.MX_MSE, R, n, A, A, None) == _lib.E_ARG
        assert L.slk_mx_pack(A, A, R, n, A, A, None, None) == _lib.E_ARG
        assert L.slk_mx_unpack(A, A, R, n, A, A, None, None) == _lib.E_ARG
        assert L.slk_mx_dequantize(A, A, R, n, 0, A, None, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, None, _lib.MX_MSE, 4, 48, A, A, None) == _lib.E_ARG and b"32" in L.slk_last_error()
    assert L.slk_mx_scale_search(None, None, _lib.MX_MSE, 4, 64, A, A, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, None, _lib.MX_MSE, 4, 64, None, None, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, None, 3, 4, 64, A, A, None) == _lib.E_ARG and b"mode" in L.slk_last_error()
    assert L.slk_mx_scale_search(A, None, -1, 4, 64, A, A, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, None, _lib.MX_DIAG, 4, 64, A, A, None) == _lib.E_ARG and b"hdiag" in L.slk_last_error()
    assert L.slk_mx_scale_search(A, A, _lib.MX_MSE, 4, 64, A, A, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, A, _lib.MX_MAX, 4, 64, A, A, None) == _lib.E_ARG
    assert L.slk_mx_scale_search(A, None, _lib.MX_MSE, 1 << 30, 1 << 20, A, A, None) == _lib.E_ARG  # 2^45 blocks
    for fn in (L.slk_mx_pack, L.slk_mx_unpack):
        assert fn(None, None, 4, 64, None, None, None, None) == _lib.E_ARG
        assert fn(A, A, 4, 64, None, A, None, None) == _lib.E_ARG   # one half of a pair
        assert fn(None, A, 4, 64, A, A, None, None) == _lib.E_ARG
        assert fn(A, None, 4, 64, A, A, None, None) == _lib.E_ARG
        assert fn(A, A, 4, 64, A, None, None, None) == _lib.E_ARG
        assert fn(A + 4, A, 4, 64, A, A, None, None) == _lib.E_ARG and b"aligned" in L.slk_last_error()
        assert fn(A, A, 4, 64, A + 8, A, None, None) == _lib.E_ARG
    dq = L.slk_mx_dequantize
    assert dq(None, A, 4, 64, 0, A, None, None) == _lib.E_ARG
    assert dq(A, None, 4, 64, 0, A, None, None) == _lib.E_ARG
    assert dq(A, A, 4, 64, 0, None, None, None) == _lib.E_ARG
    assert dq(A, A, 4, 64, 3, A, None, None) == _lib.E_ARG and b"out_dtype" in L.slk_last_error()
    assert dq(A + 2, A, 4, 64, 0, A, None, None) == _lib.E_ARG and b"aligned" in L.slk_last_error()
    assert dq(A, A, 4, 64, 1, A + 8, None, None) == _lib.E_ARG


def test_python_refusals():
    import torch

    from sleekit_amd import mx

    W = np.zeros((4, 64), np.float32)
    H = np.eye(64, dtype=np.float32)
    idx = np.zeros((4, 64), np.uint8)
    S = np.ones((4, 2), np.float32)
    codes = np.zeros((4, 32), np.uint8)
    E = np.full((4, 2), 127, np.uint8)
    for call in (
        lambda: mx.compute_mx_scales(np.zeros((4, 48), np.float32)),
        lambda: mx.compute_mx_scales(W, mode="hessian"),
        lambda: mx.compute_mx_scales(W, mode="norm"),
        lambda: mx.compute_mx_scales(W, mode="diag"),                    # diag without H
        lambda: mx.compute_mx_scales(W[0], H),
        lambda: mx.compute_mx_scales(W.astype(np.float64)),
        lambda: mx.quantize_mxfp4(np.zeros((4, 48), np.float32), np.eye(48, dtype=np.float32)),
        lambda: mx.quantize_mxfp4(W, H, scale_mode="obq"),
        lambda: mx.quantize_mxfp4(W, np.eye(32, dtype=np.float32)),
        lambda: mx.pack_mxfp4(np.zeros((4, 48), np.uint8), np.ones((4, 1), np.float32)),
        lambda: mx.pack_mxfp4(idx, np.ones((4, 3), np.float32)),
        lambda: mx.pack_mxfp4(idx.astype(np.int32), S),
        lambda: mx.pack_mxfp4(idx, S.astype(np.float64)),
        lambda: mx.unpack_mxfp4(np.zeros((4, 24), np.uint8), E),
        lambda: mx.unpack_mxfp4(codes, np.full((4, 3), 127, np.uint8)),
        lambda: mx.unpack_mxfp4(codes, S),
        lambda: mx.dequantize_mxfp4(codes, E, dtype=torch.float64),
        lambda: mx.dequantize_mxfp4(codes, E, dtype=torch.bfloat16),      # NumPy has no bfloat16
        lambda: mx.dequantize_mxfp4(np.zeros((4, 24), np.uint8), E),
        lambda: mx.encode_scales(np.ones(4, np.float32)),
        lambda: mx.decode_scales(S),
    ):
        with pytest.raises(ValueError):
            call()


def test_numpy_calls_have_no_cpu_path(monkeypatch):
    """With no GPU visible, NumPy input raises rather than falling back to a CPU computation."""
    import torch

    from sleekit_amd import _device, mx

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_device, "_gpu_seen", False)
    W = np.zeros((4, 64), np.float32)
    H = np.eye(64, dtype=np.float32)
    idx = np.zeros((4, 64), np.uint8)
    S = np.ones((4, 2), np.float32)
    codes = np.zeros((4, 32), np.uint8)
    E = np.full((4, 2), 127, np.uint8)
    for call in (
        lambda: mx.compute_mx_scales(W),
        lambda: mx.compute_mx_scales(W, H, "diag"),
        lambda: mx.quantize_mxfp4(W, H),
        lambda: mx.pack_mxfp4(idx, S),
        lambda: mx.unpack_mxfp4(codes, E),
        lambda: mx.dequantize_mxfp4(codes, E),
        lambda: mx.encode_scales(S),
        lambda: mx.decode_scales(E),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
