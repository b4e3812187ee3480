"""MXFP6 (E2M3) layers without a GPU: the NumPy model (tests/mx6_model.py) against the reference's own results
(tests/golden/mx6.npz, tests/golden/make_golden_mx6.py) -- every scale byte, the indices after the loop and after the moves,
the packed stream --, the format's known answers as the header states them, the index <-> code map, a NumPy emulation of the
scale-search kernel's integer arithmetic (sleekit_amd/csrc/mx.hip: e2m3_round, the scale byte) against np.digitize, the new
entry points' argument checks and the Python layer's refusals, and the output-error table of DESIGN.md section 22 (W6A8 and
W6A6 beside W4A8 and W4A6).  The device kernels are held to the fixtures and to the model in tests/test_gpu_mx6.py."""

import json
import os

import numpy as np
import pytest
import torch

import mx6_model as model
import mx_act4_model
import mx_act6_model
import mx_gemm_model
import rotation_model
from conftest import ROOT
from groups_ls_model import local_search_grouped, trace_of
from groups_model import model_grouped
from ls_evidence import explain_rows
from test_mx_act6_cpu import SEEDS
from test_mx_cpu import row_hashes, sha

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "mx6.npz"))
META = json.loads(str(FIX["meta"]))
CASES = META["cases"]
W6 = "mxfp6_e2m3"
ENTRIES = (("slk_mx_scale_search6", 8), ("slk_mx_pack6", 8), ("slk_mx_unpack6", 8), ("slk_mx_gemm_w6", 12))


def case_inputs(i):
    """W, H (float32) and the reference's scales S of fixture case i."""
    L = model.case_layer(CASES[i])
    return L["W"].astype(np.float32), L["H"].astype(np.float32), model.decode_model(FIX[f"E_{i}"])


def near(i):
    return {k: FIX[f"near_{i}/{k}"] for k in ("rows", "choice", "runner", "ratio")}


def check_indices(i, idx, trace=None):
    """test_mx_cpu.check_indices on this fixture: bit for bit the reference's, except rows one of whose decisions was a proven
    near-tie (tests/ls_evidence.py).  Returns the rows that differ."""
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
    if len(bad) == 0:
        assert sha(codes) == CASES[i]["sha256_codes"], f"case {i}: codes"


# ---------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_cover():
    assert 8 <= len(CASES) <= 12
    assert {c["act_order"] for c in CASES} == {"none", "diag", "err", "sqerr", "pivot", "inv_diag", "combined_diag"}
    assert {c["mode"] for c in CASES} == {"max", "mse", "diag"}
    assert {c["n"] for c in CASES} >= {32, 96, 288, 1056}
    assert sorted(c["n"] for c in CASES if c["moves"]) == [96, 768] and all(c["moves"] == 10 for c in CASES if c["moves"])
    assert {(c["special"] or [None])[0] for c in CASES} >= {"zero", "negative", "small_diag"}
    assert all(v > 0 for v in META["factors_chosen"].values()) and len(META["factors_chosen"]) == 4
    assert any(f"idx_{i}" not in FIX for i in range(len(CASES))) and any(f"idx_{i}" in FIX for i in range(len(CASES)))
    assert os.path.getsize(os.path.join(HERE, "golden", "mx6.npz")) <= os.path.getsize(os.path.join(HERE, "golden", "mx.npz"))


def test_special_cases_are_what_they_say():
    for i, c in enumerate(CASES):
        E = FIX[f"E_{i}"]
        assert E.dtype == np.uint8 and E.shape == (c["R"], c["n"] // 32) and E.min() >= 71 and E.max() <= 253
        kind = (c["special"] or [None])[0]
        if kind == "zero":
            assert (E[:, c["special"][1]] == (74 if c["mode"] == "max" else 71)).all()
        if kind == "negative":
            assert (case_inputs(i)[0][:, :32] < 0).all()
        if kind == "small_diag":
            W, H, S = case_inputs(i)
            j = c["special"][1]
            d = H.diagonal()
            # 1e-4 of what they were (the generator's diagonals spread over 0.6 .. 200): far below every other entry
            assert d[j::32].max() < 2e-3 * np.delete(d, np.arange(j, c["n"], 32)).min()
            assert np.linalg.eigvalsh(H.astype(np.float64)).min() > 0
            base = model.scales_model(W, None, "max")[1].astype(np.int32)
            assert set(np.unique(E.astype(np.int32) - base)) == {-3, -2, -1, 0}  # every factor, in this one case


@pytest.mark.parametrize("i", range(len(CASES)))
def test_model_reproduces_the_reference(i):
    """The reference's scale bytes, its indices after the loop (SHA-256), after the moves (row by row) and its codes."""
    c = CASES[i]
    W, H, S = case_inputs(i)
    Sm, Em = model.scales_model(W, H, c["mode"])
    assert np.array_equal(Em, FIX[f"E_{i}"]) and np.array_equal(Sm.view(np.uint32), S.view(np.uint32)), f"case {i}: scales"
    L = model.case_layer(c)
    grd = model.e2m3_grid()
    Q0 = model_grouped(L["W"], S, grd, L["H"], 32, c["act_order"], c["damp"], c["min_block_size"], c["num_blocks"])
    s = np.repeat(S, 32, axis=1)
    assert sha(grd.index(Q0 / s).astype(np.uint8)) == c["sha256_idx0"], f"case {i}: loop"
    records = []
    Q = local_search_grouped(W, Q0, S, grd, H, 32, c["moves"], records)
    idx = grd.index(Q / s).astype(np.uint8)
    bad = check_indices(i, idx, trace_of(records) if records else None)
    assert c["moves"] == 0 or len(bad) <= len(near(i)["rows"])
    codes, E = model.pack_model(idx, S)
    assert codes.shape == (c["R"], 3 * c["n"] // 4)
    check_codes(i, codes, bad)
    # Q is +-magnitude * 2^(b - 127) bit for bit, and the packed form gives the indices and the scales back
    assert np.array_equal(model.dequantize_model(codes, E).view(np.uint32), Q.view(np.uint32))
    assert np.array_equal(mx_act6_model.dequantize_act6_model(codes, E, np.float32).view(np.uint32), Q.view(np.uint32))
    back_idx, back_S = model.unpack_model(codes, E)
    assert np.array_equal(back_idx, idx) and np.array_equal(back_S, S)
    if f"idx_{i}" in FIX:
        assert sha(model.pack_model(FIX[f"idx_{i}"], S)[0]) == c["sha256_codes"]


# ---------------------------------------------------------------------------------------------------------------- format
def test_known_answers():
    from sleekit_amd import mx

    assert len(mx.E2M3) == 63 and mx.E2M3.values.tolist() == model.VALUES and model.VALUES[31] == 0 and model.VALUES[62] == 7.5
    assert model.VALUES == sorted(model.VALUES) and model.VALUES == [-v for v in reversed(model.VALUES)]
    mids = (np.array(model.VALUES[:-1]) + np.array(model.VALUES[1:])) / 2
    assert mx.E2M3.thresholds.tolist() == mids.tolist()
    assert " ".join(f"{c:02x}" for c in model.codes_of(np.array([0, 1, 30, 31, 32, 61, 62]))) == "3f 3e 21 00 01 1e 1f"
    idx = np.full((1, 32), 31, np.uint8)
    idx[0, :4] = model.indices_of(np.array([0x01, 0x02, 0x3f, 0x00]))
    codes, scales = model.pack_model(idx, np.array([[0.0078125]], np.float32))
    assert codes.shape == (1, 24) and codes[0, :3].tolist() == [0x81, 0xf0, 0x03] and not codes[0, 3:].any() and scales.tolist() == [[120]]
    idx[0, :4] = [0, 62, 31, 32]
    assert model.pack_model(idx, np.ones((1, 1), np.float32))[0][0, :3].tolist() == [0xff, 0x07, 0x04]
    # a tie goes upward: 0.0625 is index 32 (0.125), -0.0625 is index 31 (0); -0.0 is index 31
    g = model.e2m3_grid()
    assert g.index(np.array([0.0625, -0.0625, 7.25, -7.25, -0.0, 100.0, -100.0], np.float32)).tolist() == [32, 31, 62, 1, 31, 62, 0]
    # the header and the integration notes state the format with these answers
    for name in (os.path.join("include", "sleekit_amd.h"), "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        for needle in ("3f 3e 21 00 01 1e 1f", "[81, f0, 03]", "[ff, 07, 04]", "0x20 | (31 - i)", "0x1f", "slk_mx_gemm_w6", "SLK_MX_ACT_FP6"):
            assert needle in text, (name, needle)


def test_index_code_map():
    i = np.arange(63)
    c = model.codes_of(i)
    assert sorted(c.tolist()) == [x for x in range(64) if x != 0x20] and np.array_equal(model.indices_of(c), i)
    # the code's value is the table's
    assert np.array_equal(mx_act6_model.e2m3_decode(c), np.array(model.VALUES))
    assert (c[:31] == (0x20 | (31 - i[:31]))).all() and (c[31:] == i[31:] - 31).all()
    assert model.indices_of(np.array([0x20])).tolist() == [31]                 # -0 reads back as the zero entry
    assert model.codes_of(np.array([63, 64, 200, 255])).tolist() == [0x1f] * 4   # a caller error is stored as 7.5
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 63, (5, 96)).astype(np.uint8)
    codes, _ = model.pack_model(idx, np.ones((5, 3), np.float32))
    assert np.array_equal(mx_act6_model.unpack_codes(codes), model.codes_of(idx))
    from packing_model import pack_model as pack_bits

    assert np.array_equal(codes, pack_bits(model.codes_of(idx), 6).view(np.uint8).reshape(5, -1)[:, :72])


# ---------------------------------------------------------------------------------------------------------------- kernel arithmetic
def e2m3_round(a):
    """sleekit_amd/csrc/mx.hip: e2m3_round, operation for operation on int64 arrays holding the kernel's 32-bit integers."""
    a = np.minimum(a, 0x40f00000)
    cut = np.minimum(np.maximum(147 - (a >> 23), 20), 24)          # (an arithmetic shift, as the kernel's on an int)
    r = ((((a & 0xffffffff) + (1 << (cut - 1))) & 0xffffffff) >> cut) << cut
    return np.where(a >= 0x3d800000, r, 0).astype(np.uint32)


def kernel_quantized_magnitude(x, eb):
    """What k_mx_scale_search<., MXA_E2M3> takes |x / s| to, for float32 x and the scale byte eb."""
    x = np.asarray(x, np.float32)
    inv = np.array((254 - eb) << 23, np.uint32).view(np.float32)
    ax = np.abs(x)
    neg = (x.view(np.uint32) >> 31).astype(np.int64)
    a = (ax * inv).astype(np.float32).view(np.uint32).astype(np.int64) - neg
    return e2m3_round(a).view(np.float32)


def kernel_scale_byte(block):
    """The byte of the smallest power of two >= max(max / 7.5, min / -7.5, 1e-16), the kernel's integer form."""
    block = np.asarray(block, np.float32)
    b0 = np.maximum(np.maximum(block.max(axis=-1), -block.min(axis=-1)) / np.float32(7.5), np.float32(1e-16)).astype(np.float32)
    return np.minimum(((b0.view(np.uint32).astype(np.int64) + 0x7fffff) >> 23) & 0xff, 253)


def digitized_magnitude(x, eb):
    s = np.ldexp(np.float32(1), int(eb) - 127)
    g = model.e2m3_grid()
    return np.abs(g.value((np.asarray(x, np.float32) / s).astype(np.float32))).astype(np.float32)


def test_e2m3_round_equals_digitize_on_every_limit():
    limits = ((np.array(model.VALUES[31:-1]) + np.array(model.VALUES[32:])) / 2).astype(np.float32)  # the 31 non-negative limits
    assert len(limits) == 31 and limits[0] == 0.0625 and limits[-1] == 7.25
    pts = np.concatenate([limits, np.array(model.VALUES[31:], np.float32), np.float32([7.5, 7.75, 8, 100, 3e38, 1e-30, 1e-45])])
    for eb in (71, 74, 100, 126, 127, 128, 150, 253):
        s = np.ldexp(np.float32(1), eb - 127)
        y = np.concatenate([pts, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))]).astype(np.float32)
        with np.errstate(over="ignore", under="ignore"):
            x = (y * s).astype(np.float32)
        x = x[np.isfinite(x)]
        x = np.concatenate([x, -x, np.float32([0.0, -0.0])])
        got, want = kernel_quantized_magnitude(x, eb), digitized_magnitude(x, eb)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (eb, x[got != want][:4], got[got != want][:4], want[got != want][:4])
    # the tie rule by sign, spelled out: +limit goes up, -limit goes towards zero
    assert kernel_quantized_magnitude(np.float32([0.0625, -0.0625, 0.9375, -0.9375, 7.25, -7.25, 1.0625, -1.0625]), 127).tolist() == \
        [0.125, 0.0, 1.0, 0.875, 7.5, 7.0, 1.125, 1.0]


def test_e2m3_round_equals_digitize_on_random_values():
    rng = np.random.default_rng(61)
    for eb in (90, 120, 127, 131):
        s = np.ldexp(np.float32(1), eb - 127)
        x = np.concatenate([rng.standard_normal(20000) * 3, rng.uniform(-8, 8, 10000), rng.uniform(-1, 1, 10000),
                            (rng.integers(-124, 125, 5000) / 16.0)]).astype(np.float32) * s   # (the last: exact limits and grid points)
        got, want = kernel_quantized_magnitude(x, eb), digitized_magnitude(x, eb)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), eb
    # 4 x 45 000 values; and the scale byte on random blocks of many magnitudes, amax exactly 7.5 * 2^e among them
    blocks = (rng.standard_normal((4000, 32)) * np.exp2(rng.integers(-60, 60, (4000, 1)))).astype(np.float32)
    blocks[::7, 3] = np.float32(7.5) * np.exp2(rng.integers(-40, 40, len(blocks[::7]))).astype(np.float32)
    blocks[::7] = np.clip(blocks[::7], -np.abs(blocks[::7, 3:4]), np.abs(blocks[::7, 3:4]))
    blocks[5] = 0
    blocks[6] = -np.abs(blocks[6])
    want = model.encode_model(model.pow2_at_or_above(model.scaling_ref.no_clip_scale(blocks, model.e2m3_grid(), 0)))
    assert np.array_equal(kernel_scale_byte(blocks), want) and want[5] == 74


def test_the_emulated_search_equals_the_model():
    """The whole choice -- scale byte, four candidates, float32 sums in NumPy's pairwise order of 32, first minimum -- on the
    fixture's small-diagonal case, where every factor wins somewhere."""
    i = next(k for k, c in enumerate(CASES) if (c["special"] or [None])[0] == "small_diag")
    W, H, _ = case_inputs(i)
    hd = H.diagonal()
    E = np.zeros(FIX[f"E_{i}"].shape, np.uint8)
    for k in range(W.shape[1] // 32):
        blk, h = W[:, 32 * k:32 * k + 32], hd[32 * k:32 * k + 32]
        eb = kernel_scale_byte(blk)
        best, bf = np.full(len(blk), np.inf, np.float32), np.full(len(blk), 3)
        for f in range(4):
            es = eb - 3 + f
            err = np.zeros(len(blk), np.float32)
            for r in range(len(blk)):
                v = kernel_quantized_magnitude(blk[r], int(es[r]))
                e = (v * np.ldexp(np.float32(1), int(es[r]) - 127) - np.abs(blk[r])).astype(np.float32)
                err[r] = (h * (e * e)).sum(dtype=np.float32)
            better = err < best
            best[better], bf[better] = err[better], f
        E[:, k] = eb - 3 + bf
    assert np.array_equal(E, FIX[f"E_{i}"])


# ---------------------------------------------------------------------------------------------------------------- surface
def test_module_and_symbols_exist():
    import inspect

    import sleekit_amd
    from sleekit_amd import _lib, mx

    header = open(os.path.join(ROOT, "include", "sleekit_amd.h")).read()
    for name, nargs in ENTRIES:
        assert hasattr(_lib.lib, name) and len(_lib.PROTOTYPES[name][1]) == nargs and f"int {name}(" in header, name
    assert _lib.lib.slk_abi_version() == 8 and _lib.MX_ACT_FP6 == 2 and "#define SLK_MX_ACT_FP6 2" in header
    for name in ("pack_mxfp6", "unpack_mxfp6", "dequantize_mxfp6", "quantize_layer_mxfp6", "quantize_mxfp6", "linear_mxfp6"):
        assert callable(getattr(mx, name)), name
    for a, b in ((mx.quantize_mxfp6, mx.quantize_mxfp4), (mx.quantize_layer_mxfp6, mx.quantize_layer_mxfp4),
                 (mx.linear_mxfp6, mx.linear_mxfp4), (sleekit_amd.Sleekit.quantize_mxfp6, sleekit_amd.Sleekit.quantize_mxfp4)):
        assert str(inspect.signature(a)) == str(inspect.signature(b))
    for fn in (mx.compute_mx_scales, mx.matmul_mx, mx.MXLinear.__init__):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "weights" and p["weights"].default == "mxfp4"
    assert mx.MXResult._fields == ("Q", "idx", "S", "codes", "scales")


def test_argument_errors_do_not_touch_the_gpu():
    from sleekit_amd import _lib

    L, A = _lib.lib, 4096  # (a non-null, 16-byte aligned address that is never dereferenced: each call fails its checks first)
    for R, n in ((4, 48), (4, 0), (0, 32), (-1, 32), (4, 31)):
        assert L.slk_mx_scale_search6(A, None, _lib.MX_MSE, R, n, A, A, None) == _lib.E_ARG
        assert L.slk_mx_pack6(A, A, R, n, A, A, None, None) == _lib.E_ARG
        assert L.slk_mx_unpack6(A, A, R, n, A, A, None, None) == _lib.E_ARG
    assert L.slk_mx_scale_search6(A, None, 3, 4, 64, A, A, None) == _lib.E_ARG and b"mode" in L.slk_last_error()
    assert L.slk_mx_scale_search6(A, None, _lib.MX_DIAG, 4, 64, A, A, None) == _lib.E_ARG and b"hdiag" in L.slk_last_error()
    assert L.slk_mx_scale_search6(A, A, _lib.MX_MSE, 4, 64, A, A, None) == _lib.E_ARG
    assert L.slk_mx_scale_search6(A, None, _lib.MX_MSE, 4, 64, None, None, None) == _lib.E_ARG
    for fn in (L.slk_mx_pack6, L.slk_mx_unpack6):
        assert fn(None, None, 4, 64, None, None, None, None) == _lib.E_ARG
        assert fn(A, A, 4, 64, None, A, None, None) == _lib.E_ARG   # one half of a pair
        assert fn(A, None, 4, 64, A, A, None, None) == _lib.E_ARG
        assert fn(A + 4, A, 4, 64, A, A, None, None) == _lib.E_ARG and b"aligned" in L.slk_last_error()
        assert fn(A, A, 4, 64, A + 8, A, None, None) == _lib.E_ARG
    g = L.slk_mx_gemm_w6
    assert g(A, A, A, A, None, 4, 8, 64, _lib.MX_ACT_FP4, 0, A, None) == _lib.E_ARG and b"a_fmt" in L.slk_last_error()
    assert g(A, A, A, A, None, 4, 8, 64, 3, 0, A, None) == _lib.E_ARG
    for a_fmt in (_lib.MX_ACT_FP8, _lib.MX_ACT_FP6):
        assert g(A, A, A, A, None, 4, 8, 48, a_fmt, 0, A, None) == _lib.E_ARG and b"32" in L.slk_last_error()
        assert g(A, A, A, A, None, 0, 8, 64, a_fmt, 0, A, None) == _lib.E_ARG
        assert g(A, A, A, A, None, 4, 0, 64, a_fmt, 0, A, None) == _lib.E_ARG
        assert g(A, A, None, A, None, 4, 8, 64, a_fmt, 0, A, None) == _lib.E_ARG
        assert g(A, A, A, A, None, 4, 8, 64, a_fmt, 3, A, None) == _lib.E_ARG and b"out_dtype" in L.slk_last_error()
        assert g(A, A, A + 8, A, None, 4, 8, 64, a_fmt, 0, A, None) == _lib.E_ARG and b"aligned" in L.slk_last_error()


def test_python_refusals_come_before_the_device():
    from sleekit_amd import mx

    W = np.zeros((4, 64), np.float32)
    H = np.eye(64, dtype=np.float32)
    idx = np.zeros((4, 64), np.uint8)
    S = np.ones((4, 2), np.float32)
    codes = np.zeros((4, 48), np.uint8)
    E = np.full((4, 2), 127, np.uint8)
    a8, a6, a4 = np.zeros((3, 64), np.uint8), np.zeros((3, 48), np.uint8), np.zeros((3, 32), np.uint8)
    aE = np.full((3, 2), 127, np.uint8)
    x = np.zeros((3, 64), np.float32)
    for call in (
        lambda: mx.compute_mx_scales(W, weights="mxfp6"),
        lambda: mx.compute_mx_scales(W, weights="mxfp6_e3m2"),
        lambda: mx.compute_mx_scales(W, weights=None),
        lambda: mx.compute_mx_scales(np.zeros((4, 48), np.float32), weights=W6),
        lambda: mx.compute_mx_scales(W, mode="diag", weights=W6),               # diag without H
        lambda: mx.quantize_mxfp6(np.zeros((4, 48), np.float32), np.eye(48, dtype=np.float32)),
        lambda: mx.quantize_mxfp6(W, H, scale_mode="obq"),
        lambda: mx.quantize_mxfp6(W, np.eye(32, dtype=np.float32)),
        lambda: mx.pack_mxfp6(np.zeros((4, 48), np.uint8), np.ones((4, 1), np.float32)),
        lambda: mx.pack_mxfp6(idx, np.ones((4, 3), np.float32)),
        lambda: mx.pack_mxfp6(idx.astype(np.int32), S),
        lambda: mx.unpack_mxfp6(np.zeros((4, 32), np.uint8), E),                # 42.7 codes a row
        lambda: mx.unpack_mxfp6(np.zeros((4, 36), np.uint8), E),                # 48 codes: no whole number of blocks
        lambda: mx.unpack_mxfp6(codes, np.full((4, 3), 127, np.uint8)),
        lambda: mx.unpack_mxfp6(codes, S),
        lambda: mx.dequantize_mxfp6(codes, E, dtype=torch.float64),
        lambda: mx.dequantize_mxfp6(codes, E, dtype=torch.bfloat16),            # NumPy has no bfloat16
        lambda: mx.dequantize_mxfp6(np.zeros((4, 36), np.uint8), E),
        lambda: mx.matmul_mx(a8, aE, codes, E, weights="mxfp6"),
        lambda: mx.matmul_mx(a4, aE, codes, E, activations="mxfp4", weights=W6),      # nobody wants W6A4
        lambda: mx.matmul_mx(a8, aE, np.zeros((4, 32), np.uint8), E, weights=W6),     # MXFP4 codes are no MXFP6 layer
        lambda: mx.matmul_mx(a8, aE, np.zeros((4, 36), np.uint8), E, weights=W6),     # no whole number of blocks
        lambda: mx.matmul_mx(a8, aE, np.zeros((4, 72), np.uint8), np.full((4, 3), 127, np.uint8), weights=W6),  # mismatched K
        lambda: mx.matmul_mx(a6, aE, np.zeros((4, 72), np.uint8), np.full((4, 3), 127, np.uint8), activations=W6, weights=W6),
        lambda: mx.matmul_mx(a6, aE, codes, E, weights=W6),                           # (3, 48) bytes are 48 columns of MXFP8
        lambda: mx.linear_mxfp6(x, codes, E, activations="mxfp4"),
        lambda: mx.linear_mxfp6(x, codes, E, activations="mxfp6"),
        lambda: mx.linear_mxfp6(x, np.zeros((4, 32), np.uint8), E),
        lambda: mx.linear_mxfp6(np.zeros((3, 96), np.float32), codes, E),             # mismatched K
        lambda: mx.linear_mxfp6(x, codes, E, bias=np.zeros(5, np.float32)),
        lambda: mx.linear_mxfp4(x, codes, E),                                          # 48 bytes a row: 96 columns of MXFP4
        lambda: mx.MXLinear(64, 8, weights="mxfp6"),
        lambda: mx.MXLinear(64, 8, activations="mxfp4", weights=W6),
    ):
        with pytest.raises(ValueError):
            call()


def test_numpy_calls_have_no_cpu_path(monkeypatch):
    from sleekit_amd import _device, mx

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_device, "_gpu_seen", False)
    W, H = np.zeros((4, 64), np.float32), np.eye(64, dtype=np.float32)
    codes, E = np.zeros((4, 48), np.uint8), np.full((4, 2), 127, np.uint8)
    for call in (
        lambda: mx.compute_mx_scales(W, weights=W6),
        lambda: mx.quantize_mxfp6(W, H),
        lambda: mx.pack_mxfp6(np.zeros((4, 64), np.uint8), np.ones((4, 2), np.float32)),
        lambda: mx.unpack_mxfp6(codes, E),
        lambda: mx.dequantize_mxfp6(codes, E),
        lambda: mx.linear_mxfp6(np.zeros((3, 64), np.float32), codes, E),
    ):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_state_dicts_keep_their_keys():
    import collections

    from sleekit_amd import mx, rotation

    default = mx.MXLinear(64, 8)
    assert default.weights == "mxfp4" and sorted(default.state_dict()) == ["bias", "codes", "scales"] and default.codes.shape == (8, 32)
    w6 = mx.MXLinear(64, 8, weights=W6)
    assert w6.codes.shape == (8, 48) and w6.state_dict()["_extra_state"] == {"weights": W6} and "weights=mxfp6_e2m3" in repr(w6)
    w6a6 = mx.MXLinear(64, 8, activations=W6, weights=W6)
    assert w6a6.state_dict()["_extra_state"] == {"activations": W6, "weights": W6}
    assert mx.MXLinear(64, 8, activations=W6).state_dict()["_extra_state"] == {"activations": W6}
    copy = mx.MXLinear(64, 8, weights=W6)
    copy.load_state_dict(w6a6.state_dict())
    assert copy.activations == W6 and copy.weights == W6
    copy.load_state_dict(w6.state_dict())
    assert copy.activations == "mxfp8"
    with pytest.raises(RuntimeError, match="weights|size mismatch"):   # an MXFP6 state is no MXFP4 layer, and the other way round
        default.load_state_dict(w6.state_dict())
    with pytest.raises(RuntimeError, match="weights|size mismatch"):
        w6.load_state_dict(default.state_dict())
    with pytest.raises(RuntimeError, match="activations"):
        w6.load_state_dict(dict(w6.state_dict(), _extra_state={"weights": W6, "activations": "mxfp4"}))
    assert default.codes.shape == (8, 32) and w6.codes.shape == (8, 48)
    # from_result reads the format off the widths
    Result = collections.namedtuple("Result", "codes scales rotation")
    lin = torch.nn.Linear(64, 8)
    E = torch.full((8, 2), 127, dtype=torch.uint8)
    rot = rotation.Rotation._of(torch.ones(64), 32)
    m6 = mx.MXLinear.from_result(lin, Result(torch.zeros((8, 48), dtype=torch.uint8), E, rot), activations=W6)
    m4 = mx.MXLinear.from_result(lin, Result(torch.zeros((8, 32), dtype=torch.uint8), E, rot))
    assert (m6.weights, m6.activations, m4.weights) == (W6, W6, "mxfp4")
    for width in (40, 24, 64, 47):
        with pytest.raises(ValueError):
            mx.MXLinear.from_result(lin, Result(torch.zeros((8, width), dtype=torch.uint8), E, rot))
    with pytest.raises(ValueError):
        mx.MXLinear.from_result(lin, Result(torch.zeros((8, 48), dtype=torch.uint8), E, rot), activations="mxfp4")
    r6 = rotation.RotatedLinear.from_result(lin, Result(torch.zeros((8, 48), dtype=torch.uint8), E, rot), fused=True, activations=W6)
    assert r6.fused and r6.inner.weights == W6 and r6.inner.activations == W6


# ---------------------------------------------------------------------------------------------------------------- error table
def output_errors(seed):
    """tests/test_mx_act6_cpu.py's output_errors (the same layer, tokens, rotation and seeds) with the weights rounded to
    nearest in MXFP4 and in MXFP6 under their non-saturating scales: relative output error of W4A8, W4A6, W6A8, W6A6,
    an array (2, 4) indexed [rotated][case]."""
    from sleekit_amd import synth

    W = synth.make_weights(64, 256, seed)
    x = synth.make_activations(128, 256, seed).astype(np.float32)
    want = x.astype(np.float64) @ W.astype(np.float64).T
    signs = rotation_model.signs_for(256, seed)
    out = np.zeros((2, 4))
    for rotated in (False, True):
        xr = rotation_model.transform(x, 256, signs) if rotated else x
        Wr = rotation_model.transform(W, 256, signs) if rotated else W
        W4 = mx_act4_model.dequantize_act4_model(*mx_act4_model.quantize_act4_model(Wr))
        W6q = mx_act6_model.dequantize_act6_model(*mx_act6_model.quantize_act6_model(Wr))
        a8 = mx_gemm_model.dequantize_act_model(*mx_gemm_model.quantize_act_model(xr))
        a6 = mx_act6_model.dequantize_act6_model(*mx_act6_model.quantize_act6_model(xr))
        out[int(rotated)] = [np.linalg.norm(a @ w.T - want) / np.linalg.norm(want) for w, a in ((W4, a8), (W4, a6), (W6q, a8), (W6q, a6))]
    return out


def test_output_error_table():
    t = np.array([output_errors(seed) for seed in SEEDS])  # (seed, rotated, case)
    for r, name in enumerate(("plain", "rotated, block 256")):
        print(f"{name:20s} " + "  ".join(f"{case} {t[:, r, i].mean():.4f} [{t[:, r, i].min():.4f} .. {t[:, r, i].max():.4f}]"
                                        for i, case in enumerate(("W4A8", "W4A6", "W6A8", "W6A6"))))
    assert np.isfinite(t).all() and (t > 0).all()
    for r in (0, 1):  # plain and rotated, on every seed
        w4a8, w4a6, w6a8, w6a6 = t[:, r].T
        assert (w6a8 < w4a8).all() and (w6a6 < w4a6).all(), (r, t[:, r])
