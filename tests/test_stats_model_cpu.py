"""Every comparison of tests/test_gpu_stats.py is run here against the model of a WRONG kernel (the mutations of
stats_model.accumulate_model / six_term) and must fail, at the shapes the GPU file uses; the builders' exactness conditions
are asserted at every one of those shapes.  No GPU.

Which GPU test a mistake would fail:
  a dropped or wrongly paired piece product (one of the six MFMA lines of mfma_bf16x3.h)
        test_bf16_path_bit_exact[three_piece-*], test_random_data_sharp, test_layer_product_bit_exact
  a dropped token, padding that is not zero, two features swapped, the mirror store skipped
        test_float32_kernel_integers, test_bf16_path_bit_exact, test_random_data_sharp
  the running-mean factor applied on every chunk (`t0 == 0 ? factor : 1.0f` in slk_hessian_accumulate)
        test_bf16_path_bit_exact, its second batch, wherever the workspace makes more than one chunk
  the count taken as T instead of c'
        test_float32_kernel_batches, test_bf16_path_bit_exact (second batch), test_mean_integers (second batch)
  the mean's tail loop dropped
        test_mean_integers
"""

import numpy as np
import pytest

import stats_model as sm

same = sm.same_bits


def distinct_features(X):
    """Two features whose columns differ (swapping equal ones is no mistake), the second from the far end."""
    n = X.shape[1]
    return next((a, b) for a in range(n) for b in range(n - 1, a, -1) if not np.array_equal(X[:, a], X[:, b]))


def bf16_batches(kind, n, T):
    build = sm.integers if kind == "integers" else sm.three_piece
    return [build(T, n, 100 + n + T), build(T, n, 200 + n + T)]


# ------------------------------------------------------------------------------------------------------------ the builders
def test_split3_is_exact_to_24_bits():
    """The three pieces add up to the float32 they came from, and each is a bfloat16."""
    x = sm.block_gaussian(64, 128, 5)
    p = sm.split3(x)
    assert np.array_equal(p[0].astype(np.float64) + p[1] + p[2], x.astype(np.float64))
    for q in p:
        assert not (q.view(np.uint32) & 0xFFFF).any()
    # ties go to even: 1 + 2^-8 is half way between the bfloat16 neighbours 1 and 1 + 2^-7
    assert sm.bf16_round(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [1.0, 1 + 2.0 ** -6]


def test_builders_exact_at_every_gpu_shape():
    for ns, Ts in ((sm.F32_N + sm.F32_FORCED_N, sm.F32_T), (sm.MEAN_N, sm.MEAN_T)):
        for n in ns:
            for T in Ts:
                sm.integers(T, n, 1)
    for n, T in sm.BF16_SHAPES:
        sm.integers(T, n, 1)
        for seed in (100 + n + T, 200 + n + T):
            X = sm.three_piece(T, n, seed)
            for pair, part in zip(sm.SIX, sm.six_term_parts(X, X)):  # each of the six terms shows in hundreds of entries
                assert (part != 0).sum() >= 200, (n, T, pair)
    sm.three_piece(40, 128, 7)  # the public-surface test's input
    for R, n, mod in sm.G_SHAPES:
        for symmetric in (True, False):
            W, H = sm.three_piece_layer(R, n, 300 + n, mod, symmetric)
            whole = sm.six_term(W.T, H)
            assert (whole != W.astype(np.float64) @ H.astype(np.float64)).sum() * 2 > (whole != 0).sum()
            for pair, part in zip(sm.SIX, sm.six_term_parts(W.T, H)):
                assert (part != 0).sum() >= 200, (n, pair)


def test_builder_refuses_a_pattern_too_dense():
    """Modulus 8 at 96 tokens would put sum |terms| at 27: the builder asserts rather than give an order-dependent input."""
    with pytest.raises(AssertionError):
        sm.three_piece(96, 384, 1, modulus=8)
    with pytest.raises(AssertionError):
        sm.three_piece_layer(130, 256, 1, 32)


def test_model_against_float64():
    """The unmutated model is the documented update: within float32 roundings of the float64 statistics."""
    X1, X2 = sm.block_gaussian(75, 130, 1), sm.block_gaussian(40, 130, 2)
    H, m = sm.accumulate_batches([X1, X2])
    X = np.concatenate([X1, X2]).astype(np.float64)
    np.testing.assert_allclose(H, X.T @ X / 115, rtol=0, atol=4 * 2.0 ** -24 * (np.abs(X).T @ np.abs(X) / 115).max())
    np.testing.assert_allclose(m, X.mean(axis=0), rtol=0, atol=4 * 2.0 ** -24 * np.abs(X).mean(axis=0).max())
    Hp, mp = sm.accumulate_batches([X1, X2], pieces=True, room=32)
    np.testing.assert_allclose(Hp, X.T @ X / 115, rtol=0, atol=8 * 2.0 ** -24 * (np.abs(X).T @ np.abs(X) / 115).max())
    assert same(mp, m)


def test_chunks_and_tail_tokens():
    assert [sm.chunk_tokens(96, r) for r in sm.BF16_ROOMS] == [96, 32, 64]  # one chunk, 3 x 32, 64 + 32
    assert [sm.chunk_tokens(40, r) for r in sm.BF16_ROOMS] == [64, 32, 64]  # one chunk, 32 + 8, one chunk
    assert sm.mean_main_loop_tokens(24) == [] and sm.mean_main_loop_tokens(25) == [0, 8, 16, 24]
    assert sm.mean_main_loop_tokens(32) == list(range(32)) and sm.mean_main_loop_tokens(33) == list(range(32))
    assert sm.mean_main_loop_tokens(57) == list(range(32)) + [32, 40, 48, 56]


# ------------------------------------------------------------------------------------------- 1. float32 kernel, integers
def test_float32_integer_comparison_fails_for_each_mistake():
    for n in sm.F32_N + sm.F32_FORCED_N:
        for T in sm.F32_T:
            X = sm.integers(T, n, 1000 * n + T)
            H, m = sm.accumulate_batches([X], exact=True)
            assert same(H, H.T)
            if n < 5:
                continue  # (a single feature of a few tokens can be all zeros: the larger widths carry the proof)
            assert not same(H, sm.accumulate_batches([X], drop_token=T - 1)[0]), (n, T)
            assert not same(H, sm.accumulate_batches([X], drop_token=0)[0]), (n, T)
            assert not same(H, sm.accumulate_batches([X], swap_features=distinct_features(X))[0]), (n, T)
            Hs = sm.accumulate_batches([X], skip_mirror=True)[0]
            assert not same(H, Hs) and not same(Hs, Hs.T), (n, T)
            if T % 16:  # the kernel's K depth is a multiple of 16: the rows past T must count for nothing
                assert not same(H, sm.accumulate_batches([X], pad_to=16)[0]), (n, T)


def test_float32_batches_fail_for_each_mistake():
    for n in sm.F32_BATCH_N:
        for k, Ts in enumerate(sm.F32_BATCHES):
            Xs = [sm.integers(T, n, 10 * n + 100 * k + i) for i, T in enumerate(Ts)]
            H, m = sm.accumulate_batches(Xs, exact=True)
            Hc, mc = sm.accumulate_batches(Xs, cnt_is_T=True)
            assert not same(H, Hc) and not same(m, mc)
            assert not same(H, sm.accumulate_batches(Xs, drop_token=0)[0])
    # a count past 2^31: the factor and the divisor are not what a 32-bit count gives
    X = sm.integers(17, 130, 3)
    H0, m0 = sm.accumulate_batches([sm.integers(16, 130, 2)])
    H, m = sm.accumulate_model(H0, m0, X, sm.BIG_COUNT, exact=True)
    Hw, mw = sm.accumulate_model(H0, m0, X, sm.BIG_COUNT - 2 ** 32)  # (negative: what an `int` would hold)
    assert not same(H, Hw) and not same(m, mw)
    assert not same(H, H0) and not same(m, m0)  # the batch still shows: small entries take up the new, tiny terms
    assert np.float32(sm.BIG_COUNT + 17) == np.float32(2.0 ** 31)  # cnt rounds: 2^31 + 22 is not a float32


# ------------------------------------------------------------------------------------------------------ 2. bfloat16 path
@pytest.mark.parametrize("kind", ["integers", "three_piece"])
def test_bf16_comparison_fails_for_each_mistake(kind):
    for n, T in sm.BF16_SHAPES:
        Xs = bf16_batches(kind, n, T)
        for room in sm.BF16_ROOMS:
            chunks = -(-T // sm.chunk_tokens(T, room))
            for batches in (Xs[:1], Xs):
                H, m = sm.accumulate_batches(batches, pieces=True, room=room, exact=True)
                assert same(H, H.T)

                def wrong(**mutation):
                    return sm.accumulate_batches(batches, pieces=True, room=room, **mutation)[0]

                case = (kind, n, T, room, len(batches))
                for pair in sm.SIX if kind == "three_piece" else [(1, 1)]:
                    assert not same(H, wrong(terms=[p for p in sm.SIX if p != pair])), (case, pair)
                if kind == "three_piece":
                    assert not same(H, wrong(terms=sm.WRONG_PAIRING)), case
                assert not same(H, wrong(drop_token=T - 1)), case
                assert not same(H, wrong(swap_features=distinct_features(batches[-1]))), case
                assert not same(H, wrong(skip_mirror=True)), case
                if T % 32:
                    assert not same(H, wrong(pad_to=32)), case
                if len(batches) == 2:
                    assert not same(H, wrong(cnt_is_T=True)), case
                    if chunks > 1:
                        assert not same(H, wrong(factor_every_chunk=True)), case
    # the factor mistake needs a chunked second batch: the shapes provide one with two chunks and one with three
    assert -(-96 // sm.chunk_tokens(96, 32)) == 3 and -(-96 // sm.chunk_tokens(96, 64)) == 2 and -(-40 // sm.chunk_tokens(40, 32)) == 2


def test_three_piece_input_separates_the_six_terms_from_the_full_product():
    """The exact test pins the six-term form: the full float64 product rounded to float32 is another matrix."""
    for n, T in sm.BF16_SHAPES:
        X = sm.three_piece(T, n, 100 + n + T)
        assert not same(sm.accumulate_batches([X], pieces=True)[0], sm.accumulate_batches([X], pieces=False)[0])


def test_mismatch_report_names_the_missing_term():
    X = sm.three_piece(40, 128, 140 + 128)
    want = sm.accumulate_batches([X], pieces=True)[0]

    def without(pair):
        return sm.accumulate_batches([X], pieces=True, terms=[p for p in sm.SIX if p != pair])[0]

    assert sm.explain_mismatch(want, want, without) == ""
    text = sm.explain_mismatch(without((1, 3)), want, without)
    assert "first difference at (" in text and "a missing term a1 b3 gives this value and the whole matrix" in text
    spoiled = want.copy()
    spoiled[5, 21] += 1
    assert "first difference at (5, 21)" in sm.explain_mismatch(spoiled, want, without)
    assert "no single missing term" in sm.explain_mismatch(spoiled, want, without)


# -------------------------------------------------------------------------------------------------------- 3. random, sharp
@pytest.mark.parametrize("n,T", sm.SHARP_SHAPES)
def test_sharp_figure_exceeds_twice_the_float32_chain_for_each_mistake(n, T):
    """The simulated float32 chain stays within T + 3 units, the simulated six-term sum within twice the chain's figure,
    and every mistake the random test can see lands above twice the chain's figure.  (Padding needs T % 32 != 0, the
    chunk factor and the count a second batch: the exact tests hold those.)"""
    X = sm.block_gaussian(T, n, 40 + n + T)
    chain = sm.figure(sm.finish(sm.float32_chain(X), T), X, T)
    six = sm.figure(sm.finish(sm.six_term_chain(X), T), X, T)
    print(f"n {n} T {T}: float32 chain {chain:.2f}, six-term {six:.2f}")
    assert chain <= T + 3 and six <= 2 * chain

    def wrong(**mutation):
        return sm.figure(sm.finish(sm.six_term_chain(X, **mutation), T), X, T)

    for pair in sm.SIX:
        fig = wrong(terms=[p for p in sm.SIX if p != pair])
        print(f"    without a{pair[0]} b{pair[1]}: {fig:.1f}")
        assert fig > 2 * chain, (pair, fig, chain)
    assert wrong(terms=sm.WRONG_PAIRING) > 2 * chain
    assert wrong(drop_token=T - 1) > 2 * chain
    assert wrong(swap_features=(1, n - 2)) > 2 * chain
    unmirrored = sm.finish(sm.six_term_chain(X), T)
    unmirrored[np.triu_indices(n, 1)] = 0
    assert sm.figure(unmirrored, X, T) > 2 * chain


# ------------------------------------------------------------------------------------------------------------------ 4. mean
def test_mean_comparison_fails_for_each_mistake():
    seen_tail = 0
    for n in sm.MEAN_N:
        for T in sm.MEAN_T:
            Xs = [sm.integers(T, n, 7 * n + T), sm.integers(T, n, 7 * n + T + 1000)]
            m = sm.accumulate_batches(Xs, exact=True)[1]
            if n < 31:
                continue
            assert not same(m, sm.accumulate_batches(Xs, cnt_is_T=True)[1]), (n, T)
            if T % 32:  # the tail loop has tokens
                assert len(sm.mean_main_loop_tokens(T)) < T
                assert not same(m, sm.accumulate_batches(Xs, mean_tail_dropped=True)[1]), (n, T)
                seen_tail += 1
            else:
                assert len(sm.mean_main_loop_tokens(T)) == T
    assert seen_tail >= 20


# -------------------------------------------------------------------------------------------- 6. the core's other caller
@pytest.mark.parametrize("symmetric", [True, False])
def test_layer_product_comparison_fails_for_each_mistake(symmetric):
    for R, n, mod in sm.G_SHAPES:
        W, H = sm.three_piece_layer(R, n, 300 + n, mod, symmetric)
        G = sm.six_term(W.T, H).astype(np.float32)
        assert np.array_equal(G.astype(np.float64), sm.six_term(W.T, H))
        for pair in sm.SIX:
            assert not same(G, sm.six_term(W.T, H, [p for p in sm.SIX if p != pair]).astype(np.float32)), (n, pair)
        assert not same(G, sm.six_term(W.T, H, sm.WRONG_PAIRING).astype(np.float32))
        Ws = W.copy()
        Ws[:, [1, n - 2]] = W[:, [n - 2, 1]]
        assert not same(G, sm.six_term(Ws.T, H).astype(np.float32))
        assert not same(G[:R - 1], sm.six_term(W[1:].T, H).astype(np.float32))  # rows displaced by one
        if not symmetric:  # the planes of H used where those of H^T belong
            assert not same(G, sm.six_term(W.T, np.ascontiguousarray(H.T)).astype(np.float32))
