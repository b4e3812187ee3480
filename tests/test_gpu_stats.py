"""The running statistics on the MI355X (slk_hessian_accumulate, Sleekit.add_batch) against tests/stats_model.py.

What is held, and why it can be held exactly:
  * integer inputs (-4 .. 4): every product and every partial sum is a small integer, so any order of float32 sums gives
    the same bits on every kernel, and the documented update  H = fl(fl(H f) + fl(v / cnt))  must come out bit for bit;
  * three-piece inputs, s (1.5 + e2 2^-9 + e3 2^-19) on a thin pattern: each element has three non-zero bfloat16 pieces,
    every six-term entry is a multiple of 2^-20 with sum |terms| < 16, so the bfloat16 MFMA's float32 sums are exact in any
    order as well -- and the six-term value is NOT the float64 product: the exact test pins the six pairs of mfma_bf16x3.h;
  * random inputs: the float32 kernel within its own worst case, (T + 3) u with u = 2^-24 (|X|^T |X|) / c', and the
    default path within twice the float32 kernel's MEASURED figure on the same input (a dropped third-order term costs 30
    to 100 u at these depths; at T = 200 it would cost 19 against 10 and the rule would stop discriminating).
tests/test_stats_model_cpu.py shows, without a GPU, that each comparison here fails for each mistake it is there to find.
"""

import numpy as np
import pytest
import torch

import stats_model as sm

pytestmark = pytest.mark.gpu

_models = {}


def cached(key, make):
    if key not in _models:
        _models[key] = make()
    return _models[key]


def host(t):
    return t.detach().cpu().numpy()


def accumulate(H, mean, X, count, ws="full"):
    """slk_hessian_accumulate on device tensors.  ws: "full" (what add_batch passes), None (a NULL workspace) or a byte count."""
    from sleekit_amd import _device as dev, _lib

    n, T = H.shape[0], X.shape[0]
    assert X.shape[1] == n and X.dtype == torch.float32 and X.stride() == (n, 1)
    scratch, full = dev.workspace(0, n)
    if ws is None:
        ptr, nbytes = 0, 0
    elif ws == "full":
        ptr, nbytes = scratch.data_ptr(), full
    else:
        assert ws <= full
        ptr, nbytes = scratch.data_ptr(), int(ws)
    _lib.check(_lib.lib.slk_hessian_accumulate(H.data_ptr(), mean.data_ptr(), X.data_ptr(), n, T, int(count), ptr, nbytes,
                                               dev.stream_handle()))


def run_batches(Xs, ws="full", count=0):
    """[(H, mean) on the host after each batch], from zero statistics."""
    n = Xs[0].shape[1]
    H = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    m = torch.zeros(n, dtype=torch.float32, device="cuda")
    out = []
    for X in Xs:
        accumulate(H, m, torch.from_numpy(np.array(X)).cuda(), count, ws)
        count += X.shape[0]
        out.append((host(H), host(m)))
    return out


def model_batches(Xs, pieces=False, room=None):
    """The model's (H, mean) after each batch; asserts that the products and sums are exact in float32."""
    out = []
    n = Xs[0].shape[1]
    H, m, count = np.zeros((n, n), np.float32), np.zeros(n, np.float32), 0
    for X in Xs:
        chunk = sm.chunk_tokens(X.shape[0], room) if pieces else None
        H, m = sm.accumulate_model(H, m, X, count, chunk=chunk, pieces=pieces, exact=True)
        count += X.shape[0]
        out.append((H, m))
    return out


def assert_bits(got, want, what, without_term=None):
    if sm.same_bits(got, want):
        return
    if without_term is None:
        at = sm.first_difference(got, want)
        raise AssertionError(f"{what}: first difference at {at}: got {float(got[at])!r}, model {float(want[at])!r}; "
                             f"{int((got != want).sum())} entries differ")
    raise AssertionError(f"{what}: {sm.explain_mismatch(got, want, without_term)}")


def assert_symmetric(H, what):
    assert sm.same_bits(H, np.ascontiguousarray(H.T)), f"{what}: H is not bit-wise symmetric, first at {sm.first_difference(H, H.T)}"


# -------------------------------------------------------------------------------------------- 1. float32 kernel, integers
@pytest.mark.parametrize("n", sm.F32_N)
def test_float32_kernel_integers(n):
    """k_hessian_tiles and k_mean_update bit for bit: widths with no whole tile, one past a tile, n % 4 != 0, and at n = 260
    with T = 32 and 48 the unguarded 16-byte branch (tiles 0 and 1) beside the guarded one (tile 2) in one launch."""
    for T in sm.F32_T:
        X = sm.integers(T, n, 1000 * n + T)
        (H, m), = run_batches([X])
        (wH, wm), = cached(("f32", n, T), lambda: model_batches([X]))
        assert_bits(H, wH, f"H, n {n} T {T}")
        assert_bits(m, wm, f"mean, n {n} T {T}")
        assert_symmetric(H, f"n {n} T {T}")


@pytest.mark.parametrize("how", ["switch", "null", "small"])
@pytest.mark.parametrize("n", sm.F32_FORCED_N)
def test_float32_kernel_whole_tiles(slkopt, n, how):
    """n % 128 == 0 on the float32 kernel: by SLK_NO_BF16_HESSIAN, by a NULL workspace, and by a workspace with room for
    31 tokens (below the 32 the bfloat16 path needs).  T % 16 == 0 takes the unguarded branch in every tile."""
    if how == "switch":
        slkopt.setenv("SLK_NO_BF16_HESSIAN", "1")
    ws = {"switch": "full", "null": None, "small": sm.ws_bytes_for(n, 31)}[how]
    for T in sm.F32_T:
        X = sm.integers(T, n, 1000 * n + T)
        (H, m), = run_batches([X], ws=ws)
        (wH, wm), = cached(("f32", n, T), lambda: model_batches([X]))
        assert_bits(H, wH, f"H, n {n} T {T} ({how})")
        assert_bits(m, wm, f"mean, n {n} T {T} ({how})")
        assert_symmetric(H, f"n {n} T {T} ({how})")


def test_float32_kernel_input_off_alignment():
    """An X that starts 4 bytes off a 16-byte boundary (n = 260, n % 4 == 0): the 16-byte branch must not be taken."""
    n = 260
    for T in (17, 32, 48):
        X = sm.integers(T, n, 1000 * n + T)
        flat = torch.zeros(T * n + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(T, n)
        view.copy_(torch.from_numpy(np.array(X)))
        assert view.data_ptr() % 16 == 4
        H = torch.zeros((n, n), dtype=torch.float32, device="cuda")
        m = torch.zeros(n, dtype=torch.float32, device="cuda")
        accumulate(H, m, view, 0)
        (wH, wm), = cached(("f32", n, T), lambda: model_batches([X]))
        assert_bits(host(H), wH, f"H, T {T}")
        assert_bits(host(m), wm, f"mean, T {T}")


@pytest.mark.parametrize("n", sm.F32_BATCH_N)
def test_float32_kernel_batches(n):
    """Two and three batches of unequal length: count_before > 0, c' a power of two (32) and not (17, 65, 48, 75); then one
    call on top of 2^31 + 5 tokens, where c' is past int32 and not a float32."""
    for k, Ts in enumerate(sm.F32_BATCHES):
        Xs = [sm.integers(T, n, 10 * n + 100 * k + i) for i, T in enumerate(Ts)]
        for i, ((H, m), (wH, wm)) in enumerate(zip(run_batches(Xs), model_batches(Xs))):
            assert_bits(H, wH, f"H, n {n} after batch {i} of {Ts}")
            assert_bits(m, wm, f"mean, n {n} after batch {i} of {Ts}")
            assert_symmetric(H, f"n {n} after batch {i} of {Ts}")
    X0, X1 = sm.integers(16, n, 2), sm.integers(17, n, 3)
    H = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    m = torch.zeros(n, dtype=torch.float32, device="cuda")
    accumulate(H, m, torch.from_numpy(np.array(X0)).cuda(), 0)
    accumulate(H, m, torch.from_numpy(np.array(X1)).cuda(), sm.BIG_COUNT)
    wH, wm = sm.accumulate_model(*sm.accumulate_batches([X0]), X1, sm.BIG_COUNT, exact=True)
    assert_bits(host(H), wH, "H on top of 2^31 + 5 tokens")
    assert_bits(host(m), wm, "mean on top of 2^31 + 5 tokens")


# ------------------------------------------------------------------------------------------------------ 2. bfloat16 path
def bf16_inputs(kind, n, T):
    build = sm.integers if kind == "integers" else sm.three_piece
    return [build(T, n, 100 + n + T), build(T, n, 200 + n + T)]


@pytest.mark.parametrize("staged", [False, True], ids=["dma", "staged"])
@pytest.mark.parametrize("kind", ["integers", "three_piece"])
def test_bf16_path_bit_exact(slkopt, kind, staged):
    """k_split3_transposed and k_hessian_tiles_bf16 bit for bit against the six-term model: one K-round (T = 32), a second
    round zero-padded past the tokens (40), an even number of rounds (64), an odd number and six tiles (n = 384, T = 96:
    per_xcd does not divide the tile count); the whole workspace and room for 32 and 64 tokens (chunks 64 + 32, 3 x 32,
    32 + 8); a second batch on top of the first, whose later chunks must NOT be scaled by the factor again."""
    if staged:
        slkopt.setenv("SLK_NO_BF16_DMA", "1")
    for n, T in sm.BF16_SHAPES:
        Xs = bf16_inputs(kind, n, T)
        for room in sm.BF16_ROOMS:
            ws = "full" if room is None else sm.ws_bytes_for(n, room)
            want = cached(("bf16", kind, n, T, room), lambda: model_batches(Xs, pieces=True, room=room))
            for i, ((H, m), (wH, wm)) in enumerate(zip(run_batches(Xs, ws=ws), want)):
                what = f"{kind}, n {n} T {T}, room {room}, batch {i}, {'staged' if staged else 'dma'}"

                def without(pair):
                    terms = [p for p in sm.SIX if p != pair]
                    H0, m0, c0 = (want[0][0], want[0][1], T) if i else (np.zeros((n, n), np.float32), np.zeros(n, np.float32), 0)
                    return sm.accumulate_model(H0, m0, Xs[i], c0, chunk=sm.chunk_tokens(T, room), pieces=True, terms=terms)[0]

                assert_bits(H, wH, "H, " + what, without)
                assert_bits(m, wm, "mean, " + what)
                assert_symmetric(H, what)


# -------------------------------------------------------------------------------------------------------- 3. random, sharp
@pytest.mark.parametrize("n,T", sm.SHARP_SHAPES)
def test_random_data_sharp(slkopt, n, T):
    """max |H - H64| / u, u = 2^-24 (|X|^T |X|) / c': the float32 kernel within (T + 3) u (T fused steps, a divide, a scale,
    an add), the default path and the staged one within twice the float32 kernel's figure on the same input.  Measured on
    an MI355X, in u (float32 kernel / default path; the staged path gives the default's figures; the test prints them):
        n 128 T 32: 5.068 / 3.550      n 128 T 64: 4.471 / 5.864      n 256 T 32: 4.560 / 4.396      n 256 T 64: 6.791 / 5.368"""
    X = sm.block_gaussian(T, n, 40 + n + T)
    slkopt.setenv("SLK_NO_BF16_HESSIAN", "1")
    (H32, _), = run_batches([X])
    slkopt.delenv("SLK_NO_BF16_HESSIAN")
    (Hd, _), = run_batches([X])
    slkopt.setenv("SLK_NO_BF16_DMA", "1")
    (Hs, _), = run_batches([X])
    f32, dflt, staged = (sm.figure(H, X, T) for H in (H32, Hd, Hs))
    print(f"n {n} T {T}: float32 kernel {f32:.3f} u, default path {dflt:.3f} u, staged {staged:.3f} u")
    assert f32 <= T + 3, (n, T, f32)
    assert dflt <= 2 * f32, (n, T, dflt, f32)
    assert staged <= 2 * f32, (n, T, staged, f32)
    assert_symmetric(Hd, f"n {n} T {T}")


# ------------------------------------------------------------------------------------------------------------------ 4. mean
@pytest.mark.parametrize("n", sm.MEAN_N)
def test_mean_integers(n):
    """k_mean_update at its loop edges: T around 8 (one token per thread group), 24 / 25 (the four-sum loop's first trip),
    32 / 33 (no tail / a tail of one), 57 and 65; two batches each, bit for bit -- and H with it."""
    for T in sm.MEAN_T:
        Xs = [sm.integers(T, n, 7 * n + T), sm.integers(T, n, 7 * n + T + 1000)]
        for i, ((H, m), (wH, wm)) in enumerate(zip(run_batches(Xs), model_batches(Xs))):
            assert_bits(m, wm, f"mean, n {n} T {T} batch {i}")
            assert_bits(H, wH, f"H, n {n} T {T} batch {i}")


@pytest.mark.parametrize("n", sm.MEAN_N)
def test_mean_random(n):
    """Random data on top of an earlier batch: |mean - mean64| <= T 2^-24 sum |x| / c' (any order of T float32 additions)
    + 2 roundings of the magnitude of the result's terms (the scale, the divide and the add: 2^-24 |mean f|, 2^-24 |s| / c'
    and 2^-24 of their sum); three calls from the same state give the same bits."""
    for T in (33, 57, 200):
        X0, X = sm.block_gaussian(40, n, 5 * n + T) + np.float32(0.3), sm.block_gaussian(T, n, 5 * n + T + 1) + np.float32(0.3)
        H0, m0 = (torch.from_numpy(a).cuda() for a in run_batches([X0])[0])
        Xd = torch.from_numpy(np.array(X)).cuda()
        got = []
        for _ in range(3):
            H, m = H0.clone(), m0.clone()
            accumulate(H, m, Xd, 40)
            got.append((host(H), host(m)))
        for H, m in got[1:]:
            assert sm.same_bits(m, got[0][1]) and sm.same_bits(H, got[0][0]), (n, T)
        after = 40 + T
        f, cnt = float(np.float32(40 / after)), float(np.float32(after))
        m0h = host(m0).astype(np.float64)
        s_abs = np.abs(X.astype(np.float64)).sum(axis=0)
        want = m0h * f + X.astype(np.float64).sum(axis=0) / cnt
        bound = T * 2.0 ** -24 * s_abs / after + 2 * 2.0 ** -24 * (np.abs(m0h) * f + s_abs / after)
        err = np.abs(got[0][1] - want)
        assert (err <= bound).all(), (n, T, float((err / bound).max()))


# -------------------------------------------------------------------------------------------------------- 5. non-finite
@pytest.mark.parametrize("n,T,staged", [(130, 17, False), (128, 40, False), (128, 40, True)],
                         ids=["float32-guarded", "bf16-dma", "bf16-staged"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_input_stays_where_it_is(slkopt, value, n, T, staged):
    """A NaN or an Inf at X[T-1][n-1], with T % 16 != 0 so that the guarded loads and the zero padding are in play: every
    H[i][j] with i, j != n - 1 and every mean[j != n - 1] is bit-equal to the run with that element set to 0."""
    if staged:
        slkopt.setenv("SLK_NO_BF16_DMA", "1")
    X = np.array(sm.block_gaussian(T, n, 60 + n))
    X[T - 1, n - 1] = 0.0
    (H0, m0), = run_batches([X])
    X[T - 1, n - 1] = value
    (H1, m1), = run_batches([X])
    assert_bits(H1[:n - 1, :n - 1], H0[:n - 1, :n - 1], "H away from the last feature")
    assert_bits(m1[:n - 1], m0[:n - 1], "mean away from the last feature")
    assert not np.isfinite(H1[n - 1, n - 1]) and not np.isfinite(m1[n - 1])
    assert_symmetric(np.nan_to_num(H1, nan=7.0, posinf=8.0, neginf=9.0), "with the non-finite entries named")


# -------------------------------------------------------------------------------------------- 6. the core's other caller
@pytest.mark.parametrize("staged", [False, True], ids=["dma", "staged"])
@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "not-symmetric"])
def test_layer_product_bit_exact(slkopt, symmetric, staged):
    """G = (W - Q) H out of k_error_tiles_bf16 (the product the local search starts from), Q = 0, W and H three-piece built,
    R = 130 (a second row tile of two rows): bit for bit against the six-term model.  An H that is not symmetric (one sign
    flipped above the diagonal) goes through the planes of H^T.  The row errors by the tolerance they have everywhere."""
    from sleekit_amd import engine

    if staged:
        slkopt.setenv("SLK_NO_BF16_DMA", "1")
    for R, n, mod in sm.G_SHAPES:
        W, H = sm.three_piece_layer(R, n, 300 + n, mod, symmetric)
        want64 = sm.six_term(W.T, H)
        want = want64.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), want64)
        Wd, Hd = torch.from_numpy(np.array(W)).cuda(), torch.from_numpy(np.array(H)).cuda()
        err, G = engine.row_errors(Wd, torch.zeros_like(Wd), Hd, want_G=True)
        assert_bits(host(G), want, f"G, {R} x {n}, {'symmetric' if symmetric else 'not symmetric'} H",
                    lambda pair: sm.six_term(W.T, H, [p for p in sm.SIX if p != pair]).astype(np.float32))
        D = W.astype(np.float64)
        np.testing.assert_allclose(host(err), ((D @ H.astype(np.float64)) * D).sum(axis=1), rtol=1e-5)


# -------------------------------------------------------------------------------------------------------- 7. public surface
def test_add_batch_is_the_direct_call():
    """Sleekit.add_batch gives the H and mean of slk_hessian_accumulate bit for bit (three-piece input, two batches, the
    second as a (2, 20, 128) activation); a float16 and a bfloat16 input give what their .float() gives."""
    from sleekit_amd.statistics import Sleekit

    n = 128
    Xs = [sm.three_piece(40, n, 7), sm.three_piece(40, n, 8)]
    st = Sleekit(torch.nn.Linear(n, 4).cuda())
    direct = run_batches(Xs)
    for i, X in enumerate(Xs):
        Xd = torch.from_numpy(np.array(X)).cuda()
        st.add_batch(Xd.view(2, 20, n) if i else Xd)
        assert st.count == 40 * (i + 1)
        assert_bits(host(st.hessian), direct[i][0], f"hessian after batch {i}")
        assert_bits(host(st.mean), direct[i][1], f"mean after batch {i}")
    assert_bits(direct[1][0], model_batches(Xs, pieces=True)[1][0], "H against the model")
    for dtype in (torch.float16, torch.bfloat16):
        a, b = Sleekit(torch.nn.Linear(n, 4).cuda()), Sleekit(torch.nn.Linear(n, 4).cuda())
        for seed in (9, 10):
            Xh = torch.from_numpy(np.array(sm.block_gaussian(40, n, seed))).cuda().to(dtype)
            a.add_batch(Xh)
            b.add_batch(Xh.float())
        assert_bits(host(a.hessian), host(b.hessian), f"hessian of a {dtype} input")
        assert_bits(host(a.mean), host(b.mean), f"mean of a {dtype} input")


@pytest.mark.parametrize("n", sm.STRIP_N)
def test_strip_mean_bit_exact(n):
    """slk_hessian_strip_mean = H - np.outer(m, m) in float32: one product, one subtraction, no fused step."""
    from sleekit_amd import _device as dev, _lib

    X = sm.block_gaussian(50, n, 70 + n) + np.float32(0.3)
    H = (X.T @ X / np.float32(50)).astype(np.float32)
    m = X.mean(axis=0).astype(np.float32)
    Hd, md = torch.from_numpy(H).cuda(), torch.from_numpy(m).cuda()
    out = torch.empty_like(Hd)
    _lib.check(_lib.lib.slk_hessian_strip_mean(Hd.data_ptr(), md.data_ptr(), n, out.data_ptr(), dev.stream_handle()))
    want = (H - np.outer(m, m)).astype(np.float32)
    assert np.outer(m, m).dtype == np.float32
    assert_bits(host(out), want, f"n {n}")
