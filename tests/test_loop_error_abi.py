"""CPU checks of slk_gptq_quantize_batch_error's boundary: the workspace covers its arena, bad arguments are refused on
the host before any launch, the option exists."""

import ctypes


def test_workspace_covers_the_arena_without_the_slack():
    """Qp and Eg (R n floats each), the inverse orders (batch n ints), the diagonal means (64 floats a layer): four
    256-byte-aligned takes, inside slk_workspace_bytes(_batch) less its 64 KB of slack."""
    from sleekit_amd import _lib

    L = _lib.lib
    for batch in (1, 2, 8, 64):
        for rpl in (64, 128, 1152, 4096):
            for n in (4, 7, 96, 1100, 4096, 11008):
                R = batch * rpl
                need = 2 * R * n * 4 + batch * n * 4 + batch * 64 * 4 + 4 * 256
                assert int(L.slk_workspace_bytes_batch(batch, rpl, n)) - (1 << 16) >= need, (batch, rpl, n)
                if batch == 1:
                    assert int(L.slk_workspace_bytes(R, n)) - (1 << 16) >= need, (rpl, n)
    for R in (1, 16, 100):  # ragged single layers
        for n in (1, 7, 172):
            assert int(L.slk_workspace_bytes(R, n)) - (1 << 16) >= 2 * R * n * 4 + n * 4 + 64 * 4 + 4 * 256, (R, n)


def test_bad_arguments_are_refused_before_any_launch():
    from sleekit_amd import _lib

    L = _lib.lib
    one = (ctypes.c_void_p * 1)(8)
    none = (ctypes.c_void_p * 1)(None)

    def call(scale=None, H=one, flags=0, row_err=8, batch=1):
        return L.slk_gptq_quantize_batch_error(8, scale, None, 8, H, 0.01, batch, 64, 64, 8, -1.0, 1.0, None, 32, 8, flags, 8, None, None,
                                               row_err, None, 0, None)

    # the carried error is that of the de-scaled Q: row scales need SLK_LOOP_UNSCALE
    assert call(scale=8) == _lib.E_ARG and b"SLK_LOOP_UNSCALE" in L.slk_last_error()
    assert call(H=None) == _lib.E_ARG and call(row_err=None) == _lib.E_ARG
    assert call(H=none) == _lib.E_ARG and b"null Hessian" in L.slk_last_error()
    assert call(flags=4) == _lib.E_ARG and b"unknown flags" in L.slk_last_error()
    assert call(batch=65) == _lib.E_ARG
    # well-formed arguments get as far as the workspace check (still no launch)
    assert call() == _lib.E_WS and call(scale=8, flags=1) == _lib.E_WS


def test_the_option_is_a_switch_of_the_library():
    from sleekit_amd import _lib, engine

    old = _lib.lib.slk_get_option(b"no_loop_error")
    with _lib.option("no_loop_error", 1):
        assert not engine.loop_error_route()
    with _lib.option("no_loop_error", 0):
        assert engine.loop_error_route()
    assert _lib.lib.slk_get_option(b"SLK_NO_LOOP_ERROR") == old
