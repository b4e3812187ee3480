"""CPU checks of slk_gptq_quantize_layers' boundary: the entry exists and is declared, and bad arguments are refused on the
host before any launch (the made-up addresses are never dereferenced on the device)."""

import ctypes

E_ARG_CASES = ("null W entry", "null order entry", "null U entry", "null scale entry", "null Hessian entry", "17 layers", "no layers",
               "group scales", "group size", "rows_per_layer % 64", "H without row_err", "scale without unscale", "unknown flag")


def ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def test_entry_exists():
    from sleekit_amd import _lib

    assert hasattr(_lib.lib, "slk_gptq_quantize_layers") and "slk_gptq_quantize_layers" in _lib.PROTOTYPES
    assert _lib.lib.slk_abi_version() == 8


def test_argument_errors_come_back_before_any_launch():
    from sleekit_amd import _lib

    L = _lib.lib
    A = 4096  # a non-null address; every call below is refused before it could be used

    def q(batch=2, rpl=64, n=128, W=None, scale=None, order=None, U=None, H=None, row_err=None, gscale=None, g=0, flags=0, ws=0):
        full = ptrs(*[A] * max(batch, 1))
        return L.slk_gptq_quantize_layers(W or full, scale, order or full, U or full, H, 0.01, gscale, g, batch, rpl, n, 8, -1.0, 1.0, None,
                                          32, 8, flags, A, None, None, row_err, A, ws, None)

    got = {
        "null W entry": q(W=ptrs(A, None)),
        "null order entry": q(order=ptrs(A, None)),
        "null U entry": q(U=ptrs(None, A)),
        "null scale entry": q(scale=ptrs(A, None), flags=1),
        "null Hessian entry": q(H=ptrs(A, None), row_err=A),
        "17 layers": q(batch=17),
        "no layers": q(batch=0),
        "group scales": q(gscale=ptrs(A, A), g=32),
        "group size": q(g=32),
        "rows_per_layer % 64": q(rpl=96),
        "H without row_err": q(H=ptrs(A, A)),
        "scale without unscale": q(scale=ptrs(A, A), H=ptrs(A, A), row_err=A),
        "unknown flag": q(flags=4),
    }
    assert set(got) == set(E_ARG_CASES)
    for case, code in got.items():
        assert code == _lib.E_ARG, case
    assert q(W=ptrs(A, None)) == _lib.E_ARG and b"layer 1" in L.slk_last_error()
    assert q(U=ptrs(None, A)) == _lib.E_ARG and b"layer 0" in L.slk_last_error()
    assert q(batch=17) == _lib.E_ARG and b"table" in L.slk_last_error()
    assert q(gscale=ptrs(A, A), g=32) == _lib.E_ARG and b"group scales" in L.slk_last_error()
    assert q(rpl=96) == _lib.E_ARG and b"multiple of 64" in L.slk_last_error()
    assert q(scale=ptrs(A, A), H=ptrs(A, A), row_err=A) == _lib.E_ARG and b"SLK_LOOP_UNSCALE" in L.slk_last_error()
    # well-formed arguments get as far as the workspace check (still no launch): one ragged layer, a full table, both forms
    assert q(batch=1, rpl=96) == _lib.E_WS
    assert q(batch=16) == _lib.E_WS
    assert q(scale=ptrs(A, A), H=ptrs(A, A), row_err=A, flags=1) == _lib.E_WS
