"""The rows below a diagonal block made in the chain's own launch (factor.hip, k_chol_chain_below), held bit
for bit to the forms that existed before it, through the public entry points only:

    carried   chain_carries_below = 1: one launch per outer block wherever the cap on waiting workgroups allows
    apart     chain_carries_below = 2: the chain, then k_chol_rows_below (16 rows per workgroup)
    wide      rows_below_wide = 1:     the chain, then k_chol_chain<true> (64 rows per workgroup: the carried rows' arithmetic)

U, the order and the status word are compared as bits; where a reference is at hand (float64 LAPACK, the closed form) the
bounds of tests/test_gpu_factor.py apply as well.  The launch counts of slk_profile_report say which route a call took.
Nothing here tries to make a kernel fault, hang or time out (SLK_INFO_HANDOFF_TIMEOUT stands for a hang and is not provoked).
"""

import numpy as np
import pytest
import torch

import factor_model as fm
import test_gpu_factor as tf
from sleekit_amd import synth
from test_gpu_factor import amd  # noqa: F401  (the module's fixture: the package, and the references' clean-up)

pytestmark = pytest.mark.gpu

DEV = tf.DEV
CAP = 80  # factor.hip, CHAIN_CARRY_CAP


def launches(amd, call):
    """(result of call(), {kernel name: launches}) -- the factorisation's launches by the names slk_profile_* books them under."""
    lib = amd.lib.lib
    amd.lib.check(lib.slk_profile_reset())
    amd.lib.check(lib.slk_profile_enable(1))
    try:
        out = call()
        torch.cuda.synchronize()
        rep = amd.lib.profile_report()
    finally:
        lib.slk_profile_enable(0)
        lib.slk_profile_reset()
    return out, {r["kernel"]: int(r["launches"]) for r in rep}


def blocks(n, batch=1):
    """Per outer block of the chain: (nb, below_tiles, carried by the rule of factor.hip)."""
    ld = 64 * ((n + 63) // 64)
    outer = 512 if n >= 4096 else 256
    out = []
    for k0 in range(0, ld, outer):
        k1 = min(k0 + outer, ld)
        nb, below = (k1 - k0) // 64, (ld - k1) // 64
        out.append((nb, below, below > 0 and (nb + below) * batch <= CAP))
    return out


def three_ways(amd, Hs, n, damp, mode):
    """(order, U, info) of the carried route, and the same from the two-launch forms; asserts the routes by their launches."""
    batch = len(Hs) > 1
    run = (lambda: amd.engine.factorize_batch(Hs, n, damp, mode)) if batch else (lambda: amd.engine.factorize(Hs[0], n, damp, mode))
    bl = blocks(n, len(Hs))
    with_below = sum(1 for b in bl if b[1] > 0)
    carried = sum(1 for b in bl if b[2])
    with amd.lib.option("chain_carries_below", 1):
        got, count = launches(amd, run)
    assert count.get("chol_chain", 0) == len(bl) and count.get("chol_rows_below", 0) == with_below - carried, (count, bl)
    with amd.lib.option("chain_carries_below", 2):
        apart, count = launches(amd, run)
    assert count.get("chol_chain", 0) == len(bl) and count.get("chol_rows_below", 0) == with_below, (count, bl)
    with amd.lib.option("chain_carries_below", 1), amd.lib.option("rows_below_wide", 1):
        wide, count = launches(amd, run)  # (rows_below_wide names the second launch's kernel: it forces the two launches)
    assert count.get("chol_rows_below", 0) == with_below, (count, bl)
    for other, what in ((apart, "apart"), (wide, "wide")):
        assert torch.equal(got[0], other[0]), f"order differs from {what}"
        assert torch.equal(tf.bits(got[1]), tf.bits(other[1])), f"U differs from {what}"
        assert tf.status(got[2]) == tf.status(other[2]), f"status differs from {what}"
    return got


def test_option_is_in_the_table(amd):
    lib = amd.lib.lib
    assert lib.slk_get_option(b"chain_carries_below") == 0
    with amd.lib.option("chain_carries_below", 2):
        assert lib.slk_get_option(b"SLK_CHAIN_CARRIES_BELOW") == 2
    assert lib.slk_get_option(b"chain_carries_below") == 0


# 257 | 320: ld 320, blocks of 256 -- 4 panels + 1 row below, the smallest grid with both roles;  576: rows below in two
# consecutive blocks (5, then 1);  4096 | 4160: blocks of 512 -- 8 panels with 56 | 57 rows below down to 0 | 1 (the
# headline's form, and the odd last block)
@pytest.mark.parametrize("n", [257, 320, 576, 4096, 4160])
def test_carried_rows_equal_both_launch_forms(amd, n):
    assert [b[1] for b in blocks(n)][:2] == {257: [1, 0], 320: [1, 0], 576: [5, 1], 4096: [56, 48], 4160: [57, 49]}[n]
    assert all(b[2] for b in blocks(n) if b[1] > 0)  # under the cap in every block
    ref = tf.reference(n, 5000 + n)
    order, U, info = three_ways(amd, [ref[0]], n, 0.01, amd.lib.ORDER_DIAG)
    tf.expect_reference(order, U, info, ref, f"n={n}, rows below carried")


def test_batch_of_three_is_three_single_calls(amd):
    """blockIdx.z: a later matrix's chain is dispatched behind an earlier matrix's waiting rows."""
    n = 576
    assert [b[2] for b in blocks(n, 3)] == [True, True, False]
    Hs = [tf.reference(n, 5000 + n)[0]] + [synth.make_layer_device(8, n, 7100 + b, DEV, keep=("H",))["H"] for b in (1, 2)]
    order, U, info = three_ways(amd, Hs, n, 0.01, amd.lib.ORDER_DIAG)
    assert tf.status(info) == [0, 0, 0]
    for b, H in enumerate(Hs):
        with amd.lib.option("chain_carries_below", 2):
            o1, U1, i1 = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
        assert tf.status(i1) == [0] and torch.equal(order[b], o1) and torch.equal(tf.bits(U[b]), tf.bits(U1)), b
    tf.expect_reference(order[0], U[0], info[0], tf.reference(n, 5000 + n), "batch of 3, layer 0")


def test_over_the_cap_the_two_launches_stay(amd):
    """1100 columns in a batch of 19: 18 x 19 workgroups in the first block, 14 x 19 in the second -- over the cap in every
    block, so chain_carries_below = 1 and the rule launch what = 2 launches (three_ways counts them)."""
    n, B = 1100, 19
    assert [b[2] for b in blocks(n, B)] == [False] * 5
    ref = tf.reference(n, 5000 + n)
    Hs = [ref[0]] + [synth.make_layer_device(8, n, 7000 + b, DEV, keep=("H",))["H"] for b in range(1, B)]
    order, U, info = three_ways(amd, Hs, n, 0.01, amd.lib.ORDER_DIAG)
    (o0, U0, i0), count = launches(amd, lambda: amd.engine.factorize_batch(Hs, n, 0.01, amd.lib.ORDER_DIAG))  # the rule
    assert count.get("chol_rows_below", 0) == 4
    assert torch.equal(o0, order) and torch.equal(tf.bits(U0), tf.bits(U)) and tf.status(i0) == tf.status(info) == [0] * B
    for b, H in enumerate(Hs):
        with amd.lib.option("chain_carries_below", 2):
            o1, U1, i1 = amd.engine.factorize(H, n, 0.01, amd.lib.ORDER_DIAG)
        assert tf.status(i1) == [0] and torch.equal(order[b], o1) and torch.equal(tf.bits(U[b]), tf.bits(U1)), b
    tf.expect_reference(order[0], U[0], info[0], ref, "batch of 19, layer 0")


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [320, 576])
def test_exact_integer_matrices_through_the_carried_route(amd, n, scaled):
    """The closed form of factor_model.exact_case: every number the factorisation forms is an integer (over 16), so a dropped
    or doubled slice of K in a carried row is an integer error in a named tile."""
    c = tf.exact(n, 500 + n, scaled)
    order, U, info = three_ways(amd, [c["M32"]], n, 0.0, amd.lib.ORDER_NONE)
    assert tf.status(info) == [0] and torch.equal(order.cpu(), torch.arange(n))
    tf.expect_exact(U, c, f"rows below carried, n={n}")


@pytest.mark.parametrize("k", [0, 70, 255])
def test_not_positive_definite_in_the_first_block(amd, k):
    """A pivot of -1 in panel 0, 1 and 3 of the first block at 576 columns, whose rows below ride along: the status word is
    the two-launch form's, first bad column + 1 -- never the timeout's."""
    n = 576
    c = tf.exact(n, 500 + n)
    _, M32, want = tf.bad_matrix(c, {k: -1.0})
    _, _, info = three_ways(amd, [M32], n, 0.0, amd.lib.ORDER_NONE)
    assert tf.status(info) == [want] and want == k + 1 and want != amd.dev.HANDOFF_TIMEOUT
