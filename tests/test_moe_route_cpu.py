"""The MoE route without a GPU: the entries are declared and bound, every one of them refuses bad arguments on the host
with the cause named, slk_moe_sort_workspace_bytes follows its formula, the model (tests/moe_route_model.py) gives the
hand-written answers -- ties and -inf masks included --, and the Python surface exists and refuses what needs no device.
The kernels are held to the model and to torch in tests/test_gpu_moe_route.py."""

import inspect
import os

import numpy as np
import pytest
import torch

import moe_route_model as model
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sleekit_amd.h")
ENTRIES = ("slk_moe_topk", "slk_moe_sort_workspace_bytes", "slk_moe_sort", "slk_mx_quantize_act_rows", "slk_moe_combine")


def test_header_declares_the_entries_and_the_constants():
    from sleekit_amd import _lib

    header = open(HEADER).read()
    for name in ENTRIES:
        assert f" {name}(" in header and name in _lib.PROTOTYPES, name
    assert "size_t slk_moe_sort_workspace_bytes(int n, int E);" in header
    assert f"#define SLK_MOE_GATE_SELECTED {_lib.MOE_GATE_SELECTED}" in header and f"#define SLK_MOE_GATE_ALL {_lib.MOE_GATE_ALL}" in header
    assert (_lib.MOE_GATE_SELECTED, _lib.MOE_GATE_ALL) == (0, 1)
    assert f"#define SLK_MOE_MAX_K {_lib.MOE_MAX_K}" in header and _lib.MOE_MAX_K == 16
    assert [len(_lib.PROTOTYPES[name][1]) for name in ENTRIES] == [10, 2, 10, 12, 11]
    assert _lib.PROTOTYPES["slk_moe_sort_workspace_bytes"][0] is _lib.c_size_t
    assert _lib.lib.slk_abi_version() == 8
    for needle in ("v[a] == v[b] and a < b", "pos[order[p]] == p", "BIT FOR BIT what that entry writes", "no workgroup waits for another"):
        assert needle in header, needle


def test_sort_workspace_bytes():
    from sleekit_amd import _lib

    ws = _lib.lib.slk_moe_sort_workspace_bytes

    def chunks(n):
        per = -(-n // 1024)
        chunk = 2048 if per <= 2048 else -(-per // 64) * 64
        return -(-n // chunk)

    for n, E in ((1, 1), (1024, 1024), (1025, 1), (2048, 7), (2049, 128), (8193, 128), (40000, 128), (1 << 21, 32), ((1 << 21) + 1, 32),
                 (1 << 24, 1024)):
        assert ws(n, E) == (0 if n <= 1024 else 4 * E * chunks(n)), (n, E)
    assert chunks(1 << 24) == 1024 and chunks(2049) == 2
    assert ws(0, 4) == 0 and ws(5000, 0) == 0 and ws(5000, 1025) == 0 and ws((1 << 24) + 1, 4) == 0


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    L, A = _lib.lib, 4096  # (a non-null, 16-byte aligned address that is never dereferenced: each call fails its checks first)
    big = 1 << 30

    def refused(entry, needle, *args):
        assert entry(*args) == _lib.E_ARG
        assert needle in L.slk_last_error(), (needle, L.slk_last_error())

    t = L.slk_moe_topk  # (logits, dtype, T, E, k, gating, expert_ids, gates, flag, stream)
    refused(t, b"null pointer", None, 0, 4, 8, 2, 0, A, A, A, None)
    refused(t, b"null pointer", A, 0, 4, 8, 2, 0, None, A, A, None)
    refused(t, b"null pointer", A, 0, 4, 8, 2, 0, A, None, A, None)
    refused(t, b"null pointer", A, 0, 4, 8, 2, 0, A, A, None, None)
    refused(t, b"aligned", A + 2, 0, 4, 8, 2, 0, A, A, A, None)
    refused(t, b"aligned", A + 1, 1, 4, 8, 2, 0, A, A, A, None)
    refused(t, b"aligned", A, 0, 4, 8, 2, 0, A + 2, A, A, None)
    refused(t, b"E must be", A, 0, 4, 0, 1, 0, A, A, A, None)
    refused(t, b"E must be", A, 0, 4, _lib.MX_MAX_EXPERTS + 1, 1, 0, A, A, A, None)
    refused(t, b"k must be", A, 0, 4, 8, 0, 0, A, A, A, None)
    refused(t, b"k must be", A, 0, 4, 8, 9, 0, A, A, A, None)
    refused(t, b"k must be", A, 0, 4, 64, 17, 0, A, A, A, None)
    refused(t, b"unknown dtype", A, 3, 4, 8, 2, 0, A, A, A, None)
    refused(t, b"unknown gating", A, 0, 4, 8, 2, 2, A, A, A, None)
    refused(t, b"T must be", A, 0, 0, 8, 2, 0, A, A, A, None)
    refused(t, b"2^24", A, 0, (1 << 24) // 2 + 1, 8, 2, 0, A, A, A, None)

    s = L.slk_moe_sort  # (expert_ids, n, E, order, pos, offsets, flag, workspace, ws_bytes, stream)
    for hole in range(5):
        args = [A, 5000, 8, A, A, A, A, A, big, None]
        args[(0, 3, 4, 5, 6)[hole]] = None
        refused(s, b"null pointer", *args)
    refused(s, b"aligned to 4", A + 2, 5000, 8, A, A, A, A, A, big, None)
    refused(s, b"aligned to 4", A, 5000, 8, A, A + 1, A, A, A, big, None)
    refused(s, b"E must be", A, 5000, 0, A, A, A, A, A, big, None)
    refused(s, b"E must be", A, 5000, _lib.MX_MAX_EXPERTS + 1, A, A, A, A, A, big, None)
    refused(s, b"at least 1", A, 0, 8, A, A, A, A, A, big, None)
    refused(s, b"2^24", A, (1 << 24) + 1, 8, A, A, A, A, A, big, None)
    refused(s, b"workspace is too small", A, 5000, 8, A, A, A, A, A, L.slk_moe_sort_workspace_bytes(5000, 8) - 1, None)
    refused(s, b"workspace must be", A, 5000, 8, A, A, A, A, None, big, None)
    refused(s, b"workspace must be", A, 5000, 8, A, A, A, A, A + 2, big, None)

    q = L.slk_mx_quantize_act_rows  # (X, x_dtype, T, K, rows, div, M, a_fmt, a_codes, a_scales, flag, stream)
    for hole in (0, 4, 8, 9, 10):
        args = [A, 0, 4, 64, A, 2, 8, 0, A, A, A, None]
        args[hole] = None
        refused(q, b"null pointer", *args)
    refused(q, b"aligned to 16", A + 8, 0, 4, 64, A, 2, 8, 0, A, A, A, None)
    refused(q, b"aligned to 16", A, 0, 4, 64, A, 2, 8, 0, A + 8, A, A, None)
    refused(q, b"aligned to 4", A, 0, 4, 64, A + 2, 2, 8, 0, A, A, A, None)
    refused(q, b"unknown x_dtype", A, 3, 4, 64, A, 2, 8, 0, A, A, A, None)
    refused(q, b"unknown a_fmt", A, 0, 4, 64, A, 2, 8, 3, A, A, A, None)
    refused(q, b"multiple of 32", A, 0, 4, 48, A, 2, 8, 0, A, A, A, None)
    refused(q, b"div must be", A, 0, 4, 64, A, 0, 8, 0, A, A, A, None)
    refused(q, b"at least 1", A, 0, 0, 64, A, 2, 8, 0, A, A, A, None)
    refused(q, b"at least 1", A, 0, 4, 64, A, 2, 0, 0, A, A, A, None)
    refused(q, b"2^24", A, 0, 4, 64, A, 2, (1 << 24) + 1, 0, A, A, A, None)

    c = L.slk_moe_combine  # (Y, y_dtype, pos, gates, T, k, N, out, out_dtype, flag, stream)
    for hole in (0, 2, 7, 9):
        args = [A, 0, A, None, 4, 2, 8, A, 0, A, None]
        args[hole] = None
        refused(c, b"null pointer", *args)
    refused(c, b"aligned to 16", A + 8, 0, A, A, 4, 2, 8, A, 0, A, None)
    refused(c, b"aligned to 16", A, 0, A, A, 4, 2, 8, A + 8, 0, A, None)
    refused(c, b"aligned to 4", A, 0, A, A + 2, 4, 2, 8, A, 0, A, None)
    refused(c, b"unknown y_dtype", A, 3, A, A, 4, 2, 8, A, 0, A, None)
    refused(c, b"unknown out_dtype", A, 0, A, A, 4, 2, 8, A, 3, A, None)
    refused(c, b"at least 1", A, 0, A, A, 0, 2, 8, A, 0, A, None)
    refused(c, b"at least 1", A, 0, A, A, 4, 2, 0, A, 0, A, None)
    refused(c, b"k must be", A, 0, A, A, 4, 0, 8, A, 0, A, None)
    refused(c, b"2^24", A, 0, A, A, 1 << 23, 3, 8, A, 0, A, None)


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_selection_on_hand_written_rows():
    inf = np.inf
    rows = np.array([[1.0, 3.0, 2.0, 3.0, -1.0],        # a tie: the lower index first
                     [0.0, -0.0, -0.0, 0.0, -1.0],      # +0 and -0 tie
                     [-inf, 5.0, -inf, 4.0, -inf],      # masks: the unmasked first, then the masked by index
                     [7.0, 7.0, 7.0, 7.0, 7.0]], np.float32)
    assert model.topk_ids(rows, 3).tolist() == [[1, 3, 2], [0, 1, 2], [1, 3, 0], [0, 1, 2]]
    assert [model.row_flagged(r, 3) for r in rows] == [False, False, True, False]
    assert [model.row_flagged(r, 2) for r in rows] == [False] * 4
    assert model.row_flagged([1.0, np.nan], 1) and model.row_flagged([1.0, inf], 1) and not model.row_flagged([1.0, -inf], 1)


def test_model_gates_on_hand_written_rows():
    inf = np.inf
    rows = np.array([[2.0, 2.0, 2.0, 2.0], [-inf, 1.0, 1.0, -inf], [0.0, np.log(3.0), -inf, -inf]], np.float32)
    for gates in (model.gates_f32, model.gates_f64):
        g = gates(rows, 2, "selected")
        assert g[0].tolist() == [0.5, 0.5] and g[1].tolist() == [0.5, 0.5]
        np.testing.assert_allclose(g[2], [0.75, 0.25], rtol=1e-6)
        g = gates(rows, 2, "all")
        assert g[0].tolist() == [0.25, 0.25] and g[1].tolist() == [0.5, 0.5]   # the masked experts weigh nothing
    assert model.gates_f32(rows, 2).dtype == np.float32 and model.gates_f64(rows, 2).dtype == np.float64
    # 1 / k and 1 / E exactly, in float32, whatever the order of the sum
    for k in (1, 3, 7, 16):
        assert (model.gates_f32(np.full((1, 200), -3.5, np.float32), k) == np.float32(1) / np.float32(k)).all()
    assert (model.gates_f32(np.full((1, 1000), 0.25, np.float32), 4, "all") == np.float32(1) / np.float32(1000)).all()
    assert (model.gates_f32([[np.nan, 1.0, 2.0]], 2) == 0).all() and (model.gates_f64([[-inf, -inf, 2.0]], 2) == 0).all()
    # float32 against float64 on an ordinary row: inside the GPU test's bound
    row = np.random.default_rng(3).standard_normal((4, 130)).astype(np.float32) * 4
    for gating in ("selected", "all"):
        assert np.abs(model.gates_f32(row, 8, gating) - model.gates_f64(row, 8, gating)).max() < 2.0 ** -18


def test_model_sort_and_combine():
    order, pos, offsets, bad = model.sort_model([2, 0, 2, 1, 0, 2], 4)
    assert order.tolist() == [1, 4, 3, 0, 2, 5] and pos.tolist() == [3, 0, 4, 2, 1, 5] and offsets.tolist() == [0, 2, 3, 6, 6] and not bad
    assert all(a.dtype == np.int32 for a in (order, pos, offsets))
    order, pos, offsets, bad = model.sort_model([[5, -1], [1, 0]], 3)     # clamped: 2, 0, 1, 0
    assert bad and order.tolist() == [1, 3, 2, 0] and offsets.tolist() == [0, 2, 3, 4]
    Y = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], np.float32)
    out = model.combine_model(Y, [3, 0, 1, 2], None, 2, 2)
    assert out.tolist() == [[9.0, 90.0], [6.0, 60.0]] and out.dtype == np.float32
    out = model.combine_model(Y, [3, 0, 1, 2], np.array([[0.5, 2.0], [1.0, 0.25]], np.float32), 2, 2)
    assert out.tolist() == [[6.0, 60.0], [3.0, 30.0]]
    # the order of the sum is j = 0, 1, 2: (1 + 2^-24) + 2^-24 loses both halves of an ulp, the other order keeps one
    Y = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert model.combine_model(Y, [0, 1, 2], None, 1, 3)[0, 0] == 1.0 and model.combine_model(Y, [1, 2, 0], None, 1, 3)[0, 0] > 1.0


def test_model_mapped_quantizer_is_the_plain_one_on_the_gathered_rows():
    rng = np.random.default_rng(11)
    X = rng.standard_normal((5, 64)).astype(np.float32)
    rows = np.array([7, 0, 19, 8, 3, 20, -1], np.int32)      # 20 // 4 = 5 and -1 are outside X: zeros
    for name, plain in model.QUANTIZERS.items():
        codes, scales = model.quantize_rows_model(X, rows, 4, name)
        want = np.concatenate([X[[1, 0, 4, 2, 0]], np.zeros((2, 64), np.float32)])
        for got, ref in zip((codes, scales), plain(want)):
            assert np.array_equal(got, ref), name


# ---------------------------------------------------------------------------------------------------------------- surface
def test_surface_exists():
    import sleekit_amd
    from sleekit_amd import mx, routing

    assert sleekit_amd.routing is routing and sleekit_amd.route_topk is routing.route_topk and sleekit_amd.sort_experts is routing.sort_experts
    assert routing.Routing._fields == ("expert_ids", "gates", "order", "pos", "offsets")
    sig = inspect.signature(routing.route_topk).parameters
    assert list(sig) == ["logits", "k", "gating"] and sig["gating"].default == "selected"
    assert list(inspect.signature(routing.sort_experts).parameters) == ["expert_ids", "E"]
    sig = inspect.signature(mx.MXExperts.forward_logits).parameters
    assert list(sig) == ["self", "x", "logits", "k", "gating", "rotation"] and sig["gating"].default == "selected" and sig["rotation"].default is None
    sig = inspect.signature(mx.MXExpertsMLP.forward_logits).parameters
    assert list(sig) == ["self", "x", "logits", "k", "gating", "rotation", "fused", "down_rotation"]
    assert (sig["fused"].default, sig["down_rotation"].default) == (True, None)
    # the signatures this feature leaves alone
    assert list(inspect.signature(mx.sort_by_expert).parameters) == ["expert_ids", "E"]
    assert list(inspect.signature(mx.MXExperts.forward_tokens).parameters) == ["self", "x", "expert_ids", "gates", "rotation"]
    for method in (mx.MXExperts.forward_logits, mx.MXExpertsMLP.forward_logits, mx._route_logits):
        assert "index_add" not in inspect.getsource(method)


def test_python_refusals_come_before_the_device():
    from sleekit_amd import mx, routing

    L = np.zeros((4, 8), np.float32)
    experts = mx.MXExperts(8, 64, 32)
    mlp = mx.MXExpertsMLP(mx.MXExperts(8, 64, 128), mx.MXExperts(8, 64, 32))
    x = np.zeros((4, 64), np.float32)
    for call in (
        lambda: routing.route_topk(L[0], 2),                          # ranks and dtypes
        lambda: routing.route_topk(L.astype(np.float64), 2),
        lambda: routing.route_topk(L.astype(np.int32), 2),
        lambda: routing.route_topk([[1.0, 2.0]], 1),
        lambda: routing.route_topk(np.zeros((0, 8), np.float32), 2),
        lambda: routing.route_topk(np.zeros((2, 1025), np.float32), 2),
        lambda: routing.route_topk(L, 0),                             # k
        lambda: routing.route_topk(L, 9),
        lambda: routing.route_topk(np.zeros((2, 64), np.float32), 17),
        lambda: routing.route_topk(L, 2.0),
        lambda: routing.route_topk(L, True),
        lambda: routing.route_topk(L, 2, gating="sigmoid"),           # gating
        lambda: routing.route_topk(L, 2, gating=None),
        lambda: routing.sort_experts(np.zeros(4, np.float32), 3),
        lambda: routing.sort_experts(np.zeros(4, np.int64), 0),
        lambda: routing.sort_experts(np.zeros(4, np.int32), 1025),
        lambda: routing.sort_experts(np.zeros(0, np.int64), 3),
        lambda: experts.forward_logits(x, L[:3], 2),                  # one row of logits a token
        lambda: experts.forward_logits(x, np.zeros((4, 7), np.float32), 2),   # one column an expert
        lambda: experts.forward_logits(x, L, 9),
        lambda: experts.forward_logits(x, L, 2, gating="softmax"),
        lambda: experts.forward_logits(x[0], L, 2),
        lambda: experts.forward_logits(x.astype(np.float64), L, 2),
        lambda: mlp.forward_logits(x, L[:, :5], 2),
        lambda: mlp.forward_logits(x, L, 0),
    ):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match=r"logits must be \(4, 8\)"):
        experts.forward_logits(x, L[:3], 2)


def test_numpy_calls_have_no_cpu_path(monkeypatch):
    from sleekit_amd import _device, mx, routing

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_device, "_gpu_seen", False)
    L = np.zeros((4, 8), np.float32)
    for call in (
        lambda: routing.route_topk(L, 2),
        lambda: routing.sort_experts(np.array([1, 0, 1]), 2),
        lambda: mx.MXExperts(8, 64, 32).forward_logits(np.zeros((4, 64), np.float32), L, 2),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
