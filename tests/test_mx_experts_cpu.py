"""The expert-grouped MX product without a GPU: the two entries are declared and bound, slk_mx_gemm_experts refuses bad
arguments on the host with the cause named, the tile-table model (tests/mx_experts_model.py) on hand-written offsets, the
Python surface's refusals that need no device, and MXExperts' state dict.  The kernels are held to the model and to the
dense product in tests/test_gpu_mx_experts.py."""

import inspect
import os

import numpy as np
import pytest
import torch

import mx_experts_model as model
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sleekit_amd.h")


def test_header_declares_the_entries():
    from sleekit_amd import _lib

    header = open(HEADER).read()
    assert "size_t slk_mx_experts_workspace_bytes(int E, int M);" in header and "int slk_mx_gemm_experts(" in header
    assert _lib.PROTOTYPES["slk_mx_experts_workspace_bytes"][1] == [_lib.c_int, _lib.c_int]
    assert len(_lib.PROTOTYPES["slk_mx_gemm_experts"][1]) == 18
    assert f"#define SLK_MX_W_FP4 {_lib.MX_W_FP4}" in header and f"#define SLK_MX_W_FP6 {_lib.MX_W_FP6}" in header
    assert f"#define SLK_MX_MAX_EXPERTS {_lib.MX_MAX_EXPERTS}" in header and _lib.MX_MAX_EXPERTS >= 256
    assert _lib.MX_W_FP4 != _lib.MX_W_FP6 and _lib.lib.slk_abi_version() == 8
    for needle in ("offsets[0] == 0", "offsets[E] == M", "BIT FOR BIT"):
        assert needle in header, needle


def test_workspace_bytes():
    from sleekit_amd import _lib

    ws = _lib.lib.slk_mx_experts_workspace_bytes
    for E, M in ((1, 1), (5, 83), (2, 129), (128, 64), (32, 32768), (1024, 1 << 20)):
        assert ws(E, M) == 4 * (4 + 3 * (M // 16 + E) + 3 * (M // 64 + E)), (E, M)
    assert ws(0, 5) == 0 and ws(3, 0) == 0


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    L, A = _lib.lib, 4096  # (a non-null, 16-byte aligned address that is never dereferenced: each call fails its checks first)
    g = L.slk_mx_gemm_experts
    F8, F4, F6, W4, W6 = _lib.MX_ACT_FP8, _lib.MX_ACT_FP4, _lib.MX_ACT_FP6, _lib.MX_W_FP4, _lib.MX_W_FP6
    big = 1 << 20

    def refused(needle, *args):
        assert g(*args) == _lib.E_ARG
        assert needle in L.slk_last_error(), (needle, L.slk_last_error())

    # the issue's six: E = 0, K = 48, FP4 activations with FP6 weights, null offsets, a short workspace, a misaligned out
    refused(b"E must be", A, A, A, A, None, A, 0, 8, 8, 64, F8, W4, 0, A, A, A, big, None)
    refused(b"multiple of 32", A, A, A, A, None, A, 2, 8, 8, 48, F8, W4, 0, A, A, A, big, None)
    refused(b"MXFP6 layer", A, A, A, A, None, A, 2, 8, 8, 64, F4, W6, 0, A, A, A, big, None)
    refused(b"null offsets", A, A, A, A, None, None, 2, 8, 8, 64, F8, W4, 0, A, A, A, big, None)
    need = L.slk_mx_experts_workspace_bytes(2, 8)
    refused(b"workspace is too small", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, A, A, A, need - 1, None)
    refused(b"aligned to 16", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, A + 8, A, A, big, None)
    # and the rest of the header's list
    refused(b"E must be", A, A, A, A, None, A, _lib.MX_MAX_EXPERTS + 1, 8, 8, 64, F8, W4, 0, A, A, A, 1 << 30, None)
    refused(b"at least 1", A, A, A, A, None, A, 2, 0, 8, 64, F8, W4, 0, A, A, A, big, None)
    refused(b"at least 1", A, A, A, A, None, A, 2, 8, 0, 64, F8, W4, 0, A, A, A, big, None)
    refused(b"multiple of 32", A, A, A, A, None, A, 2, 8, 8, 0, F8, W4, 0, A, A, A, big, None)
    refused(b"out_dtype", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 3, A, A, A, big, None)
    refused(b"a_fmt", A, A, A, A, None, A, 2, 8, 8, 64, 3, W4, 0, A, A, A, big, None)
    refused(b"w_fmt", A, A, A, A, None, A, 2, 8, 8, 64, F8, 2, 0, A, A, A, big, None)
    refused(b"null pointer", A, A, None, A, None, A, 2, 8, 8, 64, F8, W4, 0, A, A, A, big, None)
    refused(b"null pointer", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, None, A, A, big, None)
    refused(b"null flag", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, A, None, A, big, None)
    refused(b"aligned to 16", A + 8, A, A, A, None, A, 2, 8, 8, 64, F6, W4, 0, A, A, A, big, None)
    refused(b"aligned to 16", A, A, A + 8, A, None, A, 2, 8, 8, 64, F6, W6, 0, A, A, A, big, None)
    refused(b"workspace must be", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, A, A, None, big, None)
    refused(b"workspace must be", A, A, A, A, None, A, 2, 8, 8, 64, F8, W4, 0, A, A, A + 2, big, None)
    refused(b"row tiles", A, A, A, A, None, A, 2, 64 * 65535, 8, 64, F8, W4, 0, A, A, A, 1 << 30, None)


# ---------------------------------------------------------------------------------------------------------------- the model
def test_tile_tables_of_hand_written_offsets():
    valid, t16, t64 = model.tile_tables([0, 0, 1, 18, 83, 83], 83)
    assert valid
    # expert 1: one row; expert 2: 17 rows, two tiles; expert 3: 65 rows, the other form, two tiles; experts 0 and 4: none
    assert t16.tolist() == [[1, 0, 1], [2, 1, 18], [2, 17, 18]]
    assert t64.tolist() == [[3, 18, 83], [3, 82, 83]]
    valid, t16, t64 = model.tile_tables([0, 64, 129], 129)
    assert valid
    assert t16.tolist() == [[0, 0, 64], [0, 16, 64], [0, 32, 64], [0, 48, 64]]   # 64 rows: still the few-rows form
    assert t64.tolist() == [[1, 64, 129], [1, 128, 129]]
    valid, t16, t64 = model.tile_tables([0, 0, 0], 0)
    assert valid and t16.shape == (0, 3) and t64.shape == (0, 3)
    assert t16.dtype == np.int32 and t64.dtype == np.int32


INVALID = {"descending": ([0, 5, 3, 9], 9), "wrong last": ([0, 3, 8], 9), "non-zero first": ([1, 3, 9], 9)}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_model_rejects_invalid_offsets(name):
    offsets, M = INVALID[name]
    valid, t16, t64 = model.tile_tables(offsets, M)
    assert not valid and len(t16) == 0 and len(t64) == 0 and not model.offsets_valid(offsets, M)


def test_tables_fit_the_workspace_and_the_grids():
    """Random valid offsets: the tables never pass the M / 16 + E and M / 64 + E entries the workspace holds, the 16-row
    table never passes 4 E (the first launch's other bound), and the tiles cover every row exactly once."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        E = int(rng.integers(1, 12))
        counts = rng.choice([0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 200], E)
        M = int(counts.sum())
        if M == 0:
            continue
        offsets = model.offsets_of(counts)
        valid, t16, t64 = model.tile_tables(offsets, M)
        assert valid and len(t16) <= min(M // 16 + E, 4 * E) and len(t64) <= M // 64 + E
        seen = np.zeros(M, np.int64)
        for table, rows in ((t16, 16), (t64, 64)):
            for e, lo, hi in table:
                assert offsets[e] <= lo < hi == offsets[e + 1]
                seen[lo:min(lo + rows, hi)] += 1
        assert (seen == 1).all()


# ---------------------------------------------------------------------------------------------------------------- surface
def test_surface_exists():
    import sleekit_amd
    from sleekit_amd import mx

    assert sleekit_amd.MXExperts is mx.MXExperts
    sig = inspect.signature(mx.matmul_mx_experts).parameters
    assert list(sig) == ["a_codes", "a_scales", "codes", "scales", "offsets", "bias", "dtype", "activations", "weights"]
    assert (sig["dtype"].default, sig["activations"].default, sig["weights"].default) == (torch.float32, "mxfp8", "mxfp4")
    sig = inspect.signature(mx.linear_mx_experts).parameters
    assert list(sig) == ["x", "codes", "scales", "offsets", "bias", "dtype", "activations", "weights", "rotation"]
    assert list(inspect.signature(mx.sort_by_expert).parameters) == ["expert_ids", "E"]
    sig = inspect.signature(mx.quantize_experts).parameters
    assert list(sig) == ["Ws", "Hs", "weights", "act_order", "damp", "scale_mode"] and "nb_ls_moves" not in sig
    assert (sig["weights"].default, sig["act_order"].default, sig["damp"].default, sig["scale_mode"].default) == ("mxfp4", "diag", 0.01, "mse")
    assert list(inspect.signature(mx.MXExperts.forward_tokens).parameters) == ["self", "x", "expert_ids", "gates", "rotation"]
    assert "index_add" not in inspect.getsource(mx.MXExperts.forward_tokens).replace("no index_add_", "")


def test_python_refusals_come_before_the_device():
    from sleekit_amd import mx

    E, N, K, M = 3, 8, 64, 5
    a8, aE = np.zeros((M, K), np.uint8), np.full((M, K // 32), 127, np.uint8)
    codes, scales = np.zeros((E, N, K // 2), np.uint8), np.full((E, N, K // 32), 127, np.uint8)
    codes6 = np.zeros((E, N, 3 * K // 4), np.uint8)
    offsets = np.array([0, 2, 2, 5], np.int32)
    x = np.zeros((M, K), np.float32)
    for call in (
        lambda: mx.matmul_mx_experts(a8, aE, codes[0], scales[0], offsets),                     # wrong ranks
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales[0], offsets),
        lambda: mx.matmul_mx_experts(a8[0], aE, codes, scales, offsets),
        lambda: mx.matmul_mx_experts(a8, aE, codes.astype(np.int32), scales, offsets),          # dtypes
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales.astype(np.float32), offsets),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets.astype(np.int64)),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, dtype=torch.float64),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, dtype=torch.bfloat16),     # NumPy has no bfloat16
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets[:3]),                       # shapes
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales[:, :, :1], offsets),
        lambda: mx.matmul_mx_experts(a8, aE, codes[:, :, :24], scales, offsets),
        lambda: mx.matmul_mx_experts(a8, aE, np.zeros((E, N, K), np.uint8), np.full((E, N, K // 16), 127, np.uint8), offsets),  # other K
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, bias=np.zeros(N, np.float32)),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, bias=np.zeros((E, N + 1), np.float32)),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, activations="mxfp6"),
        lambda: mx.matmul_mx_experts(a8, aE, codes, scales, offsets, weights="mxfp6"),
        lambda: mx.matmul_mx_experts(np.zeros((M, K // 2), np.uint8), aE, codes6, scales, offsets, activations="mxfp4", weights="mxfp6_e2m3"),
        lambda: mx.linear_mx_experts(x[0], codes, scales, offsets),
        lambda: mx.linear_mx_experts(x.astype(np.float64), codes, scales, offsets),
        lambda: mx.linear_mx_experts(np.zeros((M, 96), np.float32), codes, scales, offsets),
        lambda: mx.linear_mx_experts(x, codes, scales, offsets, bias=np.zeros((E, 1), np.float32)),
        lambda: mx.linear_mx_experts(x, codes, scales, offsets, rotation="hadamard"),
        lambda: mx.linear_mx_experts(x, codes6, scales, offsets, activations="mxfp4", weights="mxfp6_e2m3"),
        lambda: mx.sort_by_expert(np.zeros(4, np.float32), 3),
        lambda: mx.sort_by_expert(np.zeros(4, np.int64), 0),
        lambda: mx.sort_by_expert(np.zeros(0, np.int64), 3),
        lambda: mx.MXExperts(0, 64, 8),
        lambda: mx.MXExperts(2, 48, 8),
        lambda: mx.MXExperts(2, 64, 8, activations="mxfp4", weights="mxfp6_e2m3"),
        lambda: mx.MXExperts.from_results([]),
        lambda: mx.quantize_experts([np.zeros((4, 64), np.float32)], []),
        lambda: mx.quantize_experts([np.zeros((4, 48), np.float32)], [np.eye(48, dtype=np.float32)]),
        lambda: mx.quantize_experts([np.zeros((4, 64), np.float32)] * 2, [np.eye(64, dtype=np.float32), np.eye(32, dtype=np.float32)]),
        lambda: mx.quantize_experts([np.zeros((4, 64), np.float32)], [np.eye(64, dtype=np.float32)], scale_mode="obq"),
        lambda: mx.quantize_experts([np.zeros((4, 64), np.float32)], [np.eye(64, dtype=np.float32)], weights="mxfp6"),
    ):
        with pytest.raises(ValueError):
            call()


def test_numpy_calls_have_no_cpu_path(monkeypatch):
    from sleekit_amd import _device, mx

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_device, "_gpu_seen", False)
    codes, scales = np.zeros((2, 8, 32), np.uint8), np.full((2, 8, 2), 127, np.uint8)
    offsets = np.array([0, 1, 3], np.int32)
    for call in (
        lambda: mx.matmul_mx_experts(np.zeros((3, 64), np.uint8), np.full((3, 2), 127, np.uint8), codes, scales, offsets),
        lambda: mx.linear_mx_experts(np.zeros((3, 64), np.float32), codes, scales, offsets),
        lambda: mx.sort_by_expert(np.array([1, 0, 1]), 2),
        lambda: mx.quantize_experts([np.zeros((4, 64), np.float32)], [np.eye(64, dtype=np.float32)]),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_module_state_round_trips():
    import collections

    from sleekit_amd import mx

    W6 = "mxfp6_e2m3"
    mod = mx.MXExperts(3, 64, 8)
    assert mod.codes.shape == (3, 8, 32) and mod.scales.shape == (3, 8, 2) and mod.bias.shape == (3, 8)
    assert sorted(mod.state_dict()) == ["bias", "codes", "scales"] and "num_experts=3" in repr(mod)
    w6 = mx.MXExperts(3, 64, 8, bias=False, activations=W6, weights=W6)
    assert w6.codes.shape == (3, 8, 48) and w6.bias is None
    assert w6.state_dict()["_extra_state"] == {"activations": W6, "weights": W6}
    copy = mx.MXExperts(3, 64, 8, bias=False, weights=W6)
    copy.load_state_dict(w6.state_dict())
    assert copy.activations == W6 and copy.weights == W6
    with pytest.raises(RuntimeError, match="weights|size mismatch"):
        mod.load_state_dict(w6.state_dict())
    Result = collections.namedtuple("Result", "codes scales")
    E8 = torch.full((8, 2), 127, dtype=torch.uint8)
    results = [Result(torch.full((8, 32), e, dtype=torch.uint8), E8) for e in range(3)]
    made = mx.MXExperts.from_results(results, biases=np.arange(24, dtype=np.float32).reshape(3, 8), activations="mxfp4", device="cpu")
    assert (made.weights, made.activations, made.num_experts, made.in_features, made.out_features) == ("mxfp4", "mxfp4", 3, 64, 8)
    assert made.codes[2, 5, 7] == 2 and made.bias[1, 0] == 8.0
    other = mx.MXExperts(3, 64, 8)
    other.load_state_dict(made.state_dict())
    assert other.activations == "mxfp4" and torch.equal(other.codes, made.codes) and torch.equal(other.bias, made.bias)
    six = mx.MXExperts.from_results([Result(torch.zeros((8, 48), dtype=torch.uint8), E8)] * 2, device="cpu")
    assert six.weights == W6 and six.bias is None
    for bad in ([Result(torch.zeros((8, 40), dtype=torch.uint8), E8)],
                [results[0], Result(torch.zeros((4, 32), dtype=torch.uint8), E8[:4])]):
        with pytest.raises(ValueError):
            mx.MXExperts.from_results(bad, device="cpu")
    with pytest.raises(ValueError):
        mx.MXExperts.from_results(results, biases=np.zeros((2, 8), np.float32), device="cpu")
