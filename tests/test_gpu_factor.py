"""The factorisation (factor.hip, prepare.hip) held to exact and float64 references at its edges, through the public entry
points only ("What the factor tests hold").

  1. matrices whose factor is known in closed form (factor_model.exact_case): U bit for bit, in every form;
  2. random Hessians against float64 LAPACK at the widths where the host's block arithmetic changes;
  3. hard matrices (condition 2e5 .. 6e7): the residual against the reference's own;
  4. the status word: its VALUE, at the strip, tile and block edges, under padding, in a batch, for 0 and NaN;
  5. independence from what the allocator left in A, the workspace and U;
  6. the multi-GPU payload: pack, unpack, unpack_upper and its batch form, word for word.
tests/test_factor_model_cpu.py proves on the CPU that each comparison made here fails on a factor that is subtly wrong.
The references are built once per module; nothing here tries to make a kernel fault, hang or time out
(SLK_INFO_HANDOFF_TIMEOUT stands for a hang and is not provoked).
"""

import ctypes

import numpy as np
import pytest
import torch

import factor_model as fm
from sleekit_amd import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from sleekit_amd import _device, _lib, engine, obq

    class NS:
        pass

    ns = NS()
    ns.dev, ns.lib, ns.engine, ns.obq = _device, _lib, engine, obq
    yield ns
    _cases.clear()
    _refs.clear()
    torch.cuda.synchronize()
    _device.release_workspaces()
    torch.cuda.empty_cache()


_cases = {}
_refs = {}


def exact(n, seed, scaled=False, dense=True):
    """exact_case with its M (float32 and float64) and U on the device, built once."""
    key = (n, seed, scaled, dense)
    if key not in _cases:
        c = fm.exact_case(n, seed, scaled, dense)
        del c["V"]  # (the closed form's other half: not needed here, 138 MB at 4160 columns)
        c["M32"] = torch.from_numpy(c["M"].astype(np.float32)).to(DEV)
        c["U_dev"] = torch.from_numpy(c["U"]).to(DEV)
        _cases[key] = c
    return _cases[key]


def bits(t):
    return t.contiguous().view(torch.int64)


def lower_is_plus_zero(U):
    return not bool(bits(U).tril(-1).any())


def expect_exact(U, c, what):
    """U == the closed form element for element, +0.0 below the diagonal; the failure names the first wrong tile."""
    if torch.equal(U, c["U_dev"]) and lower_is_plus_zero(U):
        return
    fm.assert_exact(U.cpu().numpy(), c["U"], what)
    raise AssertionError(f"{what}: differs from the closed form on the device but not on the host")


def status(info):
    return [int(v) for v in info.reshape(-1).cpu().tolist()]


# =========================================================================== 1. closed-form factors
EXACT_WIDTHS = [130, 1100, 4160]  # three tiles with padding; five outer blocks of 256; 65 tiles in outer blocks of 512, forks


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", EXACT_WIDTHS)
def test_exact_factor_in_every_form(amd, n, scaled):
    """Every pivot is 1 (scaled: a power of 4) and every number the factorisation forms an integer (over 16): U is the closed
    form bit for bit -- through the float64 load path, the float32 path plain and looking ahead, the three panel forms and
    both rows-below kernels.  A dropped, doubled or misplaced slice of K, tile of the inverse or of the flip is an integer
    error in a named tile.  rsqrt_newton gives 1 for 1 and 2^-e for 4^e exactly (measured: the scaled case is bit-exact)."""
    c = exact(n, 500 + n, scaled)
    U = amd.obq.compute_hessian_chol(torch.from_numpy(c["M"]).to(DEV))
    expect_exact(U, c, "compute_hessian_chol")
    for ahead in (False, True):
        order, U, info = amd.engine.factorize(c["M32"], n, 0.0, amd.lib.ORDER_NONE, lookahead=ahead)
        assert status(info) == [0] and torch.equal(order.cpu(), torch.arange(n))
        expect_exact(U, c, f"factorize(lookahead={ahead})")
    for form in (1, 2, 3):
        with amd.lib.option("panel_split", form):
            _, U, info = amd.engine.factorize(c["M32"], n, 0.0, amd.lib.ORDER_NONE)
        assert status(info) == [0]
        expect_exact(U, c, f"panel_split={form}")
    for wide in (1, 2):
        with amd.lib.option("rows_below_wide", wide):
            _, U, info = amd.engine.factorize(c["M32"], n, 0.0, amd.lib.ORDER_NONE)
        assert status(info) == [0]
        expect_exact(U, c, f"rows_below_wide={wide}")


@pytest.mark.parametrize("n", EXACT_WIDTHS)
def test_exact_factor_under_the_diagonal_order(amd, n):
    """ORDER_DIAG at damp 0 on the closed form without its dense block, whose diagonal is 2, ..., 2, 1: ties across the whole
    width, which the stable order leaves where they are -- order = arange(n), U the closed form."""
    c = exact(n, 600 + n, dense=False)
    assert np.array_equal(np.diag(c["M"]), np.r_[np.full(n - 1, 2.0), 1.0])
    order, U, info = amd.engine.factorize(c["M32"], n, 0.0, amd.lib.ORDER_DIAG)
    assert status(info) == [0] and torch.equal(order.cpu(), torch.arange(n))
    expect_exact(U, c, "factorize(ORDER_DIAG)")


@pytest.mark.parametrize("n", EXACT_WIDTHS)
def test_exact_factor_in_a_batch_of_three(amd, n):
    """Three different exact matrices of one width (unscaled, scaled, unscaled) in one batch, under both rows-below kernels."""
    cs = [exact(n, 500 + n, False), exact(n, 500 + n, True), exact(n, 700 + n, False)]
    for wide in (0, 1, 2):
        with amd.lib.option("rows_below_wide", wide):
            order, U, info = amd.engine.factorize_batch([c["M32"] for c in cs], n, 0.0, amd.lib.ORDER_NONE)
        assert status(info) == [0, 0, 0]
        for b, c in enumerate(cs):
            assert torch.equal(order[b].cpu(), torch.arange(n))
            expect_exact(U[b], c, f"factorize_batch[{b}], rows_below_wide={wide}")


# =========================================================================== 2. random Hessians against float64 LAPACK
def reference(n, seed):
    """(H on the device, order, P and U_ref on the device) of the synthetic layer (T = 2 n tokens) at 1 % damping, once."""
    key = (n, seed)
    if key not in _refs:
        H = synth.make_layer_device(8, n, seed, DEV, keep=("H",))["H"]
        order, P, U_ref = fm.reference(H.cpu().numpy(), 0.01)
        _refs[key] = (H, torch.from_numpy(order), torch.from_numpy(P).to(DEV), torch.from_numpy(U_ref).to(DEV))
    return _refs[key]


def expect_reference(order, U, info, ref, what):
    """The project's bounds (test_order_and_factor): the order identical, max |U - triu(U_ref)| <= 1e-9 max |U_ref|,
    max |U^T U P - I| < 1e-8 (float64 products on the device: rocBLAS, independent of the code under test)."""
    H, order_ref, P, U_ref = ref
    assert status(info) == [0], what
    assert torch.equal(order.cpu(), order_ref), what
    assert lower_is_plus_zero(U), what
    fwd, res = fm.forward_error(U, U_ref), fm.residual(U, P)
    print(f"{what}: max |U - U_ref| / max |U_ref| = {fwd:.3g}, max |U^T U P - I| = {res:.3g}")
    fm.check_forward(U, U_ref)
    fm.check_residual(U, P)


# 1 .. 65: one tile with 63, 62, 1 and 0 padding rows, two tiles of which the second is 63/64 identity;  255 .. 257: one
# outer block of 256 with no trailing update, a second one that is almost all padding;  1728 | 1729: 27 | 28 tile rows --
# LOOKAHEAD_MIN_TILES + OUTER / TILE = 28 is where a look-ahead factorisation first forks, and only its first block does;
# 4095 | 4096: one ld, 16 outer blocks of 256 | 8 of 512, forks that stop in the middle;  4097: 65 tile rows, a last outer
# block of one tile, a last inverse node without a second half at every level, 63 padding rows
WIDTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1728, 1729, 4095, 4096, 4097]


@pytest.mark.parametrize("n", WIDTHS)
def test_factor_against_lapack_where_the_block_arithmetic_changes(amd, n):
    ref = reference(n, 5000 + n)
    H = ref[0]
    for ahead in (False, True):
        order, U, info = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG, lookahead=ahead)
        expect_reference(order, U, info, ref, f"n={n} lookahead={ahead}")
    if n >= 1728:
        # a batch of two: the first held to the reference, the second (another layer) to the defining property and to its
        # own single call
        H2 = synth.make_layer_device(8, n, 6000 + n, DEV, keep=("H",))["H"]
        o1, U1, i1 = amd.engine.factorize(H2, n, 0.01, amd.lib.ORDER_DIAG)
        order, U, info = amd.engine.factorize_batch([H, H2], n, 0.01, amd.lib.ORDER_DIAG)
        assert status(info) == [0, 0] and status(i1) == [0]
        expect_reference(order[0], U[0], info[0], ref, f"n={n} batch[0]")
        assert torch.equal(order[1], o1) and torch.equal(U[1], U1)
        d = H2.diagonal().cpu().numpy()
        P2 = H2[o1][:, o1].double()
        P2.diagonal().add_(float(np.float32(0.01) * d.mean()))
        fm.check_residual(U[1], P2)


def test_batch_of_19_takes_both_rows_below_kernels_by_the_automatic_rule(amd):
    """1100 columns in a batch of 19: 4 * below_tiles * batch is 1064 for the first outer block (the wide kernel) and 760 for
    the second (the narrow one) -- the smallest batch at which ONE factorisation uses both by the rule.  Equal to 19 single
    calls bit for bit; one of them held to the reference."""
    n, B = 1100, 19
    assert amd.lib.lib.slk_get_option(b"rows_below_wide") == 0
    ld = amd.lib.lib.slk_factor_ld(n)
    assert [4 * ((ld - k) // 64) * B >= 1024 for k in (256, 512)] == [True, False]
    ref = reference(n, 5000 + n)
    Hs = [ref[0]] + [synth.make_layer_device(8, n, 7000 + b, DEV, keep=("H",))["H"] for b in range(1, B)]
    order, U, info = amd.engine.factorize_batch(Hs, n, 0.01, amd.lib.ORDER_DIAG)
    assert status(info) == [0] * B
    for b, H in enumerate(Hs):
        o1, U1, i1 = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
        assert status(i1) == [0] and torch.equal(order[b], o1) and torch.equal(bits(U[b]), bits(U1)), b
    expect_reference(order[0], U[0], info[0], ref, "batch of 19, layer 0")


# =========================================================================== 3. hard matrices
HARD = [(n, damp, graded) for n in (1100, 1792) for damp in (1e-4, 1e-6) for graded in (False, True)]


@pytest.mark.parametrize("n,damp,graded", HARD)
def test_hard_matrices_lose_no_more_than_lapack(amd, n, damp, graded):
    """T = n / 4 tokens (rank-deficient before damping), damp 1e-4 | 1e-6, plain and graded (H <- D H D, D = exp(uniform(-3,
    3))): condition numbers 2e5 .. 6e7, where a forward comparison with LAPACK means nothing.  Instead

        resid(U_gpu) <= 4 resid(U_ref),   resid(U) = max |U^T U P - I|, the same float64 expression on the same P.

    Both are a Cholesky factorisation of the reversed matrix and a triangular inverse, so they share the bound c n eps cond;
    the GPU sums in tile order and takes its pivots' reciprocal square roots from two Newton steps (a couple of ulp instead of
    half an ulp per pivot): a small integer covers that, an order of magnitude would mean lost digits.
    Measured on the MI355X (plain and look-ahead alike), resid(U_gpu) / resid(U_ref), for (damp 1e-4, 1e-4 graded, 1e-6, 1e-6
    graded):  n = 1100: 0.038, 0.111, 0.070, 0.167;  n = 1792: 0.029, 0.046, 0.065, 0.073 (residuals 2e-11 .. 1.1e-8 against
    3e-10 .. 1.7e-7: the reference's general inverse, np.linalg.inv, loses more than the device's triangular one)."""
    H = fm.hard_hessian(n, 8000 + n, graded)
    order_ref, P, U_ref = fm.reference(H, damp)
    P_d, U_ref_d, H_d = torch.from_numpy(P).to(DEV), torch.from_numpy(U_ref).to(DEV), torch.from_numpy(H).to(DEV)
    for ahead in (False, True):
        order, U, info = amd.engine.factorize(H_d, n, damp, amd.lib.ORDER_DIAG, lookahead=ahead)
        assert status(info) == [0] and torch.equal(order.cpu(), torch.from_numpy(order_ref))
        assert lower_is_plus_zero(U)
        got, want = fm.residual(U, P_d), fm.residual(U_ref_d, P_d)
        print(f"hard n={n} damp={damp:g} graded={graded} lookahead={ahead}: resid {got:.3g}, reference {want:.3g}, ratio {got / want:.3f}")
        fm.check_hard(U, U_ref_d, P_d)


def filled(count, dtype, byte):
    t = torch.empty(count, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(byte)
    return t


def raw_factor(amd, n, byte, form, Hs=None, Ms=None):
    """U and info of the raw entries on buffers (A, the whole workspace, U, info, order) filled with `byte` beforehand:
    slk_hessian_prepare(_batch) at 1 % damping under ORDER_DIAG on the float32 Hessians Hs, or slk_factor_load on the float64
    matrices Ms (no damping, no order), then slk_chol_inverse_upper in the form asked for (plain | lookahead | batch)."""
    lib, s = amd.lib.lib, amd.dev.stream_handle()
    B = len(Ms) if Ms is not None else len(Hs)
    assert B == 1 or form == "batch"
    ld = lib.slk_factor_ld(n)
    ws_bytes = lib.slk_factor_workspace_bytes_batch(B, n) if form == "batch" else lib.slk_workspace_bytes(0, n)
    ws = filled(ws_bytes, torch.uint8, byte)
    A = filled(B * ld * ld, torch.float64, byte)
    U = filled(B * n * n, torch.float64, byte).view(B, n, n)
    info = filled(B, torch.int32, byte)
    order = filled(B * n, torch.int64, byte)
    ptr = amd.dev.ptr
    if Ms is not None:
        for b, M in enumerate(Ms):
            assert M.dtype == torch.float64 and M.shape == (n, n) and M.is_contiguous()
            amd.lib.check(lib.slk_factor_load(ptr(M), n, ptr(A[b * ld * ld:]), s))
    elif form == "batch":
        ptrs = (ctypes.c_void_p * B)(*[ptr(H) for H in Hs])
        amd.lib.check(lib.slk_hessian_prepare_batch(ptrs, B, n, 0.01, amd.lib.ORDER_DIAG, ptr(order), ptr(A), ptr(ws), ws_bytes, s))
    else:
        amd.lib.check(lib.slk_hessian_prepare(ptr(Hs[0]), n, 0.01, amd.lib.ORDER_DIAG, None, ptr(order), ptr(A), ptr(ws), ws_bytes, s))
    if form == "batch":
        amd.lib.check(lib.slk_chol_inverse_upper_batch(ptr(A), B, n, ptr(U), ptr(info), ptr(ws), ws_bytes, s))
    elif form == "lookahead":
        amd.lib.check(lib.slk_chol_inverse_upper_lookahead(ptr(A), n, ptr(U), ptr(info), ptr(ws), ws_bytes, s))
    else:
        amd.lib.check(lib.slk_chol_inverse_upper(ptr(A), n, ptr(U), ptr(info), ptr(ws), ws_bytes, s))
    torch.cuda.synchronize()
    return U, info


# =========================================================================== 4. the status word
def bad_matrix(c, pivots):
    """M of the exact case with the pivots {index k in the factorisation's order: value} forced: float64 and float32 on the
    device, and the status word it must give."""
    M = c["M"]
    for k, value in pivots.items():
        M = fm.with_pivot(dict(c, M=M), k, value)
    want = min(pivots)
    assert fm.first_bad_pivot(M) == want
    return torch.from_numpy(M).to(DEV), torch.from_numpy(M.astype(np.float32)).to(DEV), want + 1


def is_nan_case(pivots):
    return any(v != v for v in pivots.values())


def status_of(amd, n, pivots, M64, M32, lookahead=False):
    """The status words of one bad matrix through the float64 load path and through the float32 path (damp 0, no order).
    A NaN on the diagonal of a float32 Hessian reaches EVERY pivot through the damping term, damp * mean(diag H), here as in
    the reference (0 * NaN is NaN): that path then reports pivot 0, and the load path, which does not damp, the NaN's own."""
    _, info = raw_factor(amd, n, 0x00, "lookahead" if lookahead else "plain", Ms=[M64])
    _, _, info32 = amd.engine.factorize(M32, n, 0.0, amd.lib.ORDER_NONE, lookahead=lookahead)
    return status(info) + status(info32)


STATUS_CASES = (
    [{k: -1.0} for k in (0, 15, 16, 63, 64, 256, 300, 1099)]  # strip and tile edges of the diagonal-tile kernel; past a
    # trailing update; the last real row, ahead of 52 padding rows
    + [{700: -1.0, 130: -1.0}, {64: 0.0}, {300: 0.0}, {0: float("nan")}, {17: float("nan")}, {511: float("nan")}, {1099: float("nan")}]
)


@pytest.mark.parametrize("scaled", [False, True])
def test_status_word_names_the_first_bad_pivot(amd, scaled):
    """info - 1 is the first index k, in the order of the factorisation (row k of the index-reversed matrix, permuted column
    n - 1 - k), whose pivot is not > 0: -1 exactly (the exact matrices with one diagonal entry lowered: rounding cannot move
    it), exactly 0, or NaN (!(pivot > 0), as LAPACK's DISNAN) -- in the chain and both panel forms."""
    n = 1100
    c = exact(n, 500 + n, scaled)
    for pivots in STATUS_CASES:
        M64, M32, want = bad_matrix(c, pivots)
        for form in (0, 1, 2, 3):
            with amd.lib.option("panel_split", form):
                got = status_of(amd, n, pivots, M64, M32)
            assert got == [want, 1 if is_nan_case(pivots) else want], (pivots, form)


def test_status_word_looking_ahead_and_in_a_batch(amd):
    n = 1792  # 28 tile rows: the look-ahead form forks
    c = exact(n, 500 + n)
    for pivots in ({0: -1.0}, {300: -1.0}, {1600: 0.0}, {n - 1: float("nan")}):
        M64, M32, want = bad_matrix(c, pivots)
        for form in (0, 1, 2, 3):
            with amd.lib.option("panel_split", form):
                got = status_of(amd, n, pivots, M64, M32, lookahead=True)
            assert got == [want, 1 if is_nan_case(pivots) else want], (pivots, form)
    # a batch of three with the bad matrix in the middle: its neighbours' status is 0 and their U what they give alone
    n = 1100
    left, right = exact(n, 500 + n, False), exact(n, 500 + n, True)
    sides = [torch.from_numpy(x["M"]).to(DEV) for x in (left, right)]
    for pivots in ({0: -1.0}, {300: -1.0}, {1099: -1.0}, {64: float("nan")}):
        M64, M32, want = bad_matrix(left, pivots)
        for form in (0, 1, 2, 3):
            with amd.lib.option("panel_split", form):
                U64, info64 = raw_factor(amd, n, 0x00, "batch", Ms=[sides[0], M64, sides[1]])
                _, U, info = amd.engine.factorize_batch([left["M32"], M32, right["M32"]], n, 0.0, amd.lib.ORDER_NONE)
            assert status(info64) == [0, want, 0], (pivots, form)
            assert status(info) == [0, 1 if is_nan_case(pivots) else want, 0], (pivots, form)
            for got in (U64, U):
                expect_exact(got[0], left, "the bad matrix's left neighbour")
                expect_exact(got[2], right, "the bad matrix's right neighbour")
    # ... and what the user is told cannot be taken for a column of H
    with pytest.raises(np.linalg.LinAlgError, match="pivot 300 in the order of the factorisation"):
        amd.obq.compute_hessian_chol(torch.from_numpy(fm.with_pivot(left, 300, -1.0)).to(DEV))


# =========================================================================== 5. independence from dirty buffers
@pytest.mark.parametrize("form", ["plain", "lookahead", "batch", "load"])
@pytest.mark.parametrize("n", [1100, 4160])  # multiples of 4: slk_hessian_prepare's gather skips the tiles above the diagonal
def test_factor_does_not_depend_on_what_the_buffers_held(amd, n, form):
    """"No kernel reads the tiles above the diagonal", nor anything else that nothing wrote: with A, the whole workspace (X, S,
    the flags) and U full of NaN bytes (0xFF) the factor is, bit for bit, the one that zero-filled buffers give."""
    Hs = [synth.make_layer_device(8, n, 9000 + n + b, DEV, keep=("H",))["H"] for b in range(2 if form == "batch" else 1)]
    Ms = None
    if form == "load":
        Ms = [Hs[0].double()]
        Ms[0].diagonal().add_(0.01 * float(Hs[0].diagonal().mean()))
    clean, info0 = raw_factor(amd, n, 0x00, form, Hs, Ms)
    dirty, info1 = raw_factor(amd, n, 0xFF, form, Hs, Ms)
    assert status(info0) == status(info1) == [0] * len(Hs)
    assert lower_is_plus_zero(dirty) and bool(torch.isfinite(dirty).all())
    assert torch.equal(bits(dirty), bits(clean))
    for b, H in enumerate(Hs):  # and it is the factor: the engine's call on this H
        if form != "load":
            _, U, _ = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
            assert torch.equal(bits(U), bits(dirty[b]))


# =========================================================================== 6. the payload
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1100])  # odd n: the pairing of rows (i, n - 1 - i) has an unpaired middle row
def test_payload_round_trip(amd, n):
    lib, ptr, s = amd.lib.lib, amd.dev.ptr, amd.dev.stream_handle()
    words = lib.slk_factor_payload_words(n)
    assert words == fm.payload_words(n)
    for info_value in (0, 7, 0x7FFFFFFF):
        U_h, order_h = fm.payload_case(n, 40 + n)
        want = fm.payload_of(U_h, order_h, info_value)
        assert len(want) == words
        U, order = torch.from_numpy(U_h).to(DEV), torch.from_numpy(order_h).to(DEV)
        info = torch.tensor([info_value], dtype=torch.int32, device=DEV)
        payload = torch.full((words + 1,), SENTINEL, dtype=torch.int64, device=DEV)
        amd.lib.check(lib.slk_factor_pack(ptr(U), ptr(order), ptr(info), n, ptr(payload), s))
        got = payload.cpu().numpy()
        assert np.array_equal(got[:words], want) and got[words] == SENTINEL
        # unpack: the square U with +0.0 below the diagonal, whatever the buffer held
        U2, order2, info2 = filled(n * n, torch.float64, 0xFF).view(n, n), filled(n, torch.int64, 0xFF), filled(1, torch.int32, 0xFF)
        amd.lib.check(lib.slk_factor_unpack(ptr(payload), n, ptr(U2), ptr(order2), ptr(info2), s))
        assert np.array_equal(U2.cpu().numpy().view(np.int64), U_h.view(np.int64))
        assert torch.equal(order2, order) and status(info2) == [info_value]
        # unpack_upper: the diagonal and above only -- every word below the diagonal is left as it was
        U3 = torch.full((n, n), SENTINEL, dtype=torch.int64, device=DEV)
        order3, info3 = filled(n, torch.int64, 0xFF), filled(1, torch.int32, 0xFF)
        amd.lib.check(lib.slk_factor_unpack_upper(ptr(payload), n, ptr(U3), ptr(order3), ptr(info3), s))
        got3 = U3.cpu().numpy()
        upper = np.triu(np.ones((n, n), dtype=bool))
        assert np.array_equal(got3[upper], U_h.view(np.int64)[upper]) and (got3[~upper] == SENTINEL).all()
        assert torch.equal(order3, order) and status(info3) == [info_value]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1100])
def test_payload_batch_unpack(amd, n, B):
    """A round's payloads into stacked factors in one launch: a verdict word after each payload; verdict = NULL is accepted."""
    lib, ptr, s = amd.lib.lib, amd.dev.ptr, amd.dev.stream_handle()
    words = lib.slk_factor_payload_words(n)
    cases = [fm.payload_case(n, 60 + 7 * b + n) for b in range(B)]
    infos = [(0, 7, 0x7FFFFFFF, 1, 1100)[b] for b in range(B)]
    payloads = []
    for (U_h, order_h), info_value, b in zip(cases, infos, range(B)):
        p = np.concatenate([fm.payload_of(U_h, order_h, info_value), np.array([3 + b], dtype=np.int64)])
        payloads.append(torch.from_numpy(p).to(DEV))
    ptrs = (ctypes.c_void_p * B)(*[ptr(p) for p in payloads])
    upper = np.triu(np.ones((n, n), dtype=bool))
    for with_verdict in (True, False):
        U = torch.full((B, n, n), SENTINEL, dtype=torch.int64, device=DEV)
        order, info = filled(B * n, torch.int64, 0xFF).view(B, n), filled(B, torch.int32, 0xFF)
        verdict = filled(B, torch.int32, 0xFF) if with_verdict else None
        amd.lib.check(lib.slk_factor_unpack_upper_batch(ptrs, B, n, ptr(U), ptr(order), ptr(info), ptr(verdict), s))
        got = U.cpu().numpy()
        for b, (U_h, order_h) in enumerate(cases):
            assert np.array_equal(got[b][upper], U_h.view(np.int64)[upper]) and (got[b][~upper] == SENTINEL).all(), b
            assert np.array_equal(order[b].cpu().numpy(), order_h)
        assert status(info) == infos
        if with_verdict:
            assert status(verdict) == [3 + b for b in range(B)]
