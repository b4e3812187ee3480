"""CPU checks of the rotating form of the fused gate/up product: the header and the prototypes of the two entries, their
argument errors before any launch, the Python surface (matmul_mx_glu / matmul_mx_glu_experts take rotation=) and its refusals
before the device, and the composed model (tests/mx_glu_rot_model.py) against its parts.  Nothing here needs a GPU."""

import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import mx_glu_model
import mx_glu_rot_model as model
import rotation_model
from conftest import ROOT

ENTRIES = {"slk_mx_gemm_glu_rot": "slk_mx_gemm_glu", "slk_mx_gemm_glu_experts_rot": "slk_mx_gemm_glu_experts"}
INF = float("inf")


def declared(text, name):
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert decl, f"{name} is not declared"
    return [" ".join(a.split()) for a in decl.group(1).split(",")]


def test_entries_are_declared_exported_and_prototyped():
    """Each _rot entry is declared with the plain entry's arguments plus `int block, const float *signs` before the stream,
    exported by the library, and prototyped with ctypes types that match the declaration; the ABI version stays 8."""
    from sleekit_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sleekit_amd.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    for name, plain in ENTRIES.items():
        args, base = declared(text, name), declared(text, plain)
        assert args == base[:-1] + ["int block", "const float *signs"] + base[-1:], (name, args)
        assert name in exported and hasattr(_lib.lib, name)
        res, argtypes = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            scalar = {"float": ctypes.c_float, "int": ctypes.c_int, "size_t": ctypes.c_size_t}.get(a.split()[0]) if "*" not in a else None
            assert t is (scalar or ctypes.c_void_p), (name, a)
        assert _lib.PROTOTYPES[plain][1] == argtypes[:len(base) - 1] + argtypes[-1:]   # (the plain entry keeps its signature)
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_do_not_touch_the_gpu():
    """Bad arguments are rejected on the host before any launch (safe without a GPU); 64 stands for an aligned pointer."""
    from sleekit_amd import _lib

    L, p, q = _lib.lib, 64, 72  # q: off 16-byte alignment
    FP8, FP4, W4, W6 = _lib.MX_ACT_FP8, _lib.MX_ACT_FP4, _lib.MX_W_FP4, _lib.MX_W_FP6

    def gemm(a=p, asc=p, w=p, ws=p, bias=None, M=4, N=32, K=32, a_fmt=FP8, w_fmt=W4, alpha=1.0, limit=INF, shift=0.0, interleaved=0, h=p, hs=p, flag=p,
             block=32, signs=p):
        return L.slk_mx_gemm_glu_rot(a, asc, w, ws, bias, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h, hs, flag, block, signs, None)

    def experts(a=p, asc=p, w=p, ws=p, bias=None, offsets=p, E=2, M=4, N=32, K=32, a_fmt=FP8, w_fmt=W4, alpha=1.0, limit=INF, shift=0.0, interleaved=0,
                h=p, hs=p, flag=p, work=p, ws_bytes=1 << 20, block=32, signs=p):
        return L.slk_mx_gemm_glu_experts_rot(a, asc, w, ws, bias, offsets, E, M, N, K, a_fmt, w_fmt, alpha, limit, shift, interleaved, h, hs, flag, work,
                                             ws_bytes, block, signs, None)

    def refused(rc, word):
        assert rc == _lib.E_ARG
        assert word.encode() in L.slk_last_error(), (word, L.slk_last_error())

    for call in (gemm, experts):
        # what is new: the block and the signs (NULL signs are allowed: nothing here names them)
        for block in (0, 1, 3, 6, 24, 48, 64, 4096, -32):
            refused(call(block=block), "block must be a power of two in 2..32")
            refused(call(block=block, signs=None), "block must be a power of two in 2..32")
        refused(call(block=3), "(got 3)")
        for block in (2, 4, 8, 16, 32):
            refused(call(block=block, signs=q), "signs must be aligned")
        # everything the plain entries refuse, ahead of it: a bad block behind a bad argument gives that argument's text
        for kw, word in ((dict(limit=0.0), "limit"), (dict(limit=float("nan")), "limit"), (dict(alpha=INF), "alpha"), (dict(shift=-INF), "shift"),
                         (dict(interleaved=2), "interleaved"), (dict(M=0), "M"), (dict(flag=None), "flag"), (dict(a_fmt=3), "a_fmt"),
                         (dict(w_fmt=2), "w_fmt"), (dict(a_fmt=FP4, w_fmt=W6), "MXFP6 layer"), (dict(N=1 << 30), "below 2^30")):
            refused(call(**kw), word)
            refused(call(block=64, signs=q, **kw), word)
        for name in ("a", "asc", "w", "ws", "h", "hs"):
            refused(call(**{name: None}), "null")
        for name in ("a", "w", "h"):
            refused(call(**{name: q}), "aligned to 16 bytes")
            assert b"signs" not in L.slk_last_error()
        for N in (0, 16, 48, -32):
            refused(call(N=N), "multiple of 32")
        for K in (0, 16, 48):
            refused(call(K=K), "K must be")
    refused(gemm(M=65535 * 64 + 1), "row tiles")
    refused(experts(M=64 * 65535, ws_bytes=1 << 30), "row tiles")
    refused(experts(offsets=None), "offsets")
    refused(experts(E=0), "experts")
    refused(experts(E=_lib.MX_MAX_EXPERTS + 1), "experts")
    refused(experts(work=None), "workspace")
    refused(experts(work=66), "workspace")
    refused(experts(ws_bytes=L.slk_mx_experts_workspace_bytes(2, 4) - 1), "too small")
    refused(experts(ws_bytes=L.slk_mx_experts_workspace_bytes(2, 4) - 1, block=5), "too small")


def operands(M=4, N=32, K=64, E=None):
    lead = () if E is None else (E,)
    return (np.zeros((M, K), np.uint8), np.full((M, K // 32), 127, np.uint8),
            np.zeros(lead + (2 * N, K // 2), np.uint8), np.full(lead + (2 * N, K // 32), 127, np.uint8))


def test_rotation_is_a_keyword_of_both_products():
    """matmul_mx_glu and matmul_mx_glu_experts take a trailing keyword rotation=None, a Rotation over the N hidden features.
    Every call here would need the GPU if it got past its checks: NumPy operands, and a ValueError, never a TypeError or a
    RuntimeError."""
    from sleekit_amd import mx
    from sleekit_amd.rotation import Rotation

    for f in (mx.matmul_mx_glu, mx.matmul_mx_glu_experts):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "rotation" and last.default is None, f.__name__
    a, asc, w, ws = operands(N=64)
    ea, easc, ew, ews = operands(N=64, E=2)
    offsets = np.array([0, 2, 4], np.int32)
    rot128, rot64 = Rotation(128, block=32, device="cpu"), Rotation(64, block=32, device="cpu")
    for call, text in (
        (lambda: mx.matmul_mx_glu(a, asc, w, ws, rotation=rot128), "the rotation has 128 features but the up layer gives 64"),
        (lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets, rotation=rot128), "the rotation has 128 features but the up layers give 64"),
        (lambda: mx.matmul_mx_glu(a, asc, w, ws, rotation="hadamard"), r"rotation must be a Rotation \(got str\)"),
        (lambda: mx.matmul_mx_glu(a, asc, w, ws, rotation=32), r"rotation must be a Rotation \(got int\)"),
        (lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets, rotation=object()), r"rotation must be a Rotation \(got object\)"),
        # the checks that came before the rotation still come first
        (lambda: mx.matmul_mx_glu(a, asc, w[:96], ws[:96], rotation=rot64), "multiple of 32"),
        (lambda: mx.matmul_mx_glu_experts(ea, easc, ew, ews, offsets[:2], rotation=rot64), "offsets must be int32"),
    ):
        with pytest.raises(ValueError, match=text):
            call()


def test_model_is_its_parts():
    """The composed model is hidden_model's float32 h, rotation_model.transform and the format's quantizer model: without
    signs and with a block of 2 the rotated pair is ((a + b) c, (a - b) c), and the unrotated h is hidden_model's."""
    rng = np.random.default_rng(3)
    M, N = 5, 64
    sums = rng.integers(-40, 41, (M, 2 * N)).astype(np.float64) / 8.0
    bias = (rng.integers(-64, 65, 2 * N) / 8.0).astype(np.float32)
    gate = dict(alpha=0.0, limit=3.0, shift=1.0, interleaved=True)
    h = model.hidden_f32(sums, bias, **gate)
    assert h.dtype == np.float32 and h.shape == (M, N)
    for activations, quantize in mx_glu_model.QUANTIZE.items():
        plain = mx_glu_model.hidden_model(sums, bias, activations, **gate)
        assert all(np.array_equal(g, w) for g, w in zip(quantize(h), plain))
        c = np.float32(1.0 / np.sqrt(2.0))
        pair = np.stack(((h[:, 0::2] + h[:, 1::2]) * c, (h[:, 0::2] - h[:, 1::2]) * c), axis=2).reshape(M, N)
        assert all(np.array_equal(g, w) for g, w in zip(model.hidden_rot_model(sums, bias, activations, 2, **gate), quantize(pair)))
        signs = rotation_model.signs_for(N, 11)
        for block in (2, 4, 8, 16, 32):
            want = quantize(rotation_model.transform(h, block, signs))
            got = model.hidden_rot_model(sums, bias, activations, block, signs, **gate)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            assert not np.array_equal(got[0], plain[0])
