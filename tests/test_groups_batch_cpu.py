"""CPU checks of group scales over a batch of layers and through sleekit_amd.dist: the batch entry point's argument errors,
its workspace bound, the bucketing that keeps grouped, per-row-scaled and unscaled layers apart, and the stream's refusals
(made before anything runs, with a stand-in backend: no device is touched)."""

import pytest
import torch

from sleekit_amd import dist as sdist

E_ARG_CASES = ("batch 0", "batch 65", "rows_per_layer % 64", "no orders", "g does not divide n", "null gscale", "unscale flag")


def test_batch_entry_exists():
    from sleekit_amd import _lib, groups

    assert hasattr(_lib.lib, "slk_gptq_quantize_grouped_batch") and "slk_gptq_quantize_grouped_batch" in _lib.PROTOTYPES
    assert callable(groups.run_loop_batch_grouped)
    assert _lib.lib.slk_abi_version() == 8


def test_batch_argument_errors_come_back_before_any_launch():
    """SLK_E_ARG on the host: the (made-up, never dereferenced) addresses are not touched."""
    from sleekit_amd import _lib

    L = _lib.lib
    A = 4096  # a non-null address; every call below is refused before it could be used

    def q(batch=2, rpl=64, n=128, g=32, S=A, order=A, flags=0):
        return L.slk_gptq_quantize_grouped_batch(A, S, g, order, A, batch, rpl, n, 8, -1.0, 1.0, None, 32, 8, flags, A, None, None, A,
                                                 1 << 30, None)

    got = {
        "batch 0": q(batch=0),
        "batch 65": q(batch=65),
        "rows_per_layer % 64": q(rpl=96),
        "no orders": q(order=None),
        "g does not divide n": q(g=48),
        "null gscale": q(S=None),
        "unscale flag": q(flags=1),  # SLK_LOOP_UNSCALE: not a grouped flag
    }
    assert set(got) == set(E_ARG_CASES)
    for case, code in got.items():
        assert code == _lib.E_ARG, case
    assert q(g=48) == _lib.E_ARG and b"divide" in L.slk_last_error()
    assert q(batch=65) == _lib.E_ARG and b"batch" in L.slk_last_error()
    assert q(rpl=96) == _lib.E_ARG and b"multiple of 64" in L.slk_last_error()
    assert q(order=None) == _lib.E_ARG and b"orders" in L.slk_last_error()
    assert q(batch=1, rpl=96, order=None, flags=1) == _lib.E_ARG  # batch 1 takes any row count and no order, not the flag


def _arena(sizes):
    """Bytes the loop's Arena takes for these buffers: every take starts on a 256-byte boundary (common.h)."""
    used = 0
    for size in sizes:
        used = (used + 255) // 256 * 256 + size
    return used


def test_workspace_bound_holds_by_arithmetic():
    """slk_workspace_bytes_batch covers the grouped loop's arena -- Qp, Eg (R n floats each), the inverse orders and the
    group tables (batch n ints each) -- without the 64 KB slack, at every batch size including 1."""
    from sleekit_amd import _lib

    L = _lib.lib
    for batch in (1, 2, 5, 8, 64):
        for rpl in (64, 128, 320, 4096):
            for n in (64, 128, 768, 1100, 3072, 4096, 11008, 28672):
                R = batch * rpl
                need = _arena([4 * R * n, 4 * R * n, 4 * batch * n, 4 * batch * n])
                have = int(L.slk_workspace_bytes_batch(batch, rpl, n))
                assert have - (1 << 16) >= need, (batch, rpl, n, have, need)
    # the existing sizes do not move
    assert int(L.slk_workspace_bytes_batch(1, 64, 128)) == int(L.slk_workspace_bytes(64, 128)) + 128 * 8 + 4096


def _layer(R, n, kind, **extra):
    lay = dict(W=torch.zeros(R, n), H=torch.eye(n))
    if kind == "row":
        lay["scale"] = torch.ones(R)
    elif kind is not None and kind != "unscaled":
        lay["gscale"], lay["group_size"] = torch.ones(R, n // kind), kind
    lay.update(extra)
    return lay


KINDS = (64, 128, "row", "unscaled")


def _mixed(R, n, copies=2):
    """`copies` layers of every kind, interleaved as a model's order would have them."""
    return [_layer(R, n, kind, id=i * len(KINDS) + k) for i in range(copies) for k, kind in enumerate(KINDS)]


def _kinds_of(layers, members):
    return {sdist._layer_kind(layers[l]) for l in members}


def test_layer_kind_tells_the_scales_apart():
    assert sdist._layer_kind(_layer(64, 256, "unscaled")) == "unscaled"
    assert sdist._layer_kind(_layer(64, 256, "row")) == "row"
    assert sdist._layer_kind(_layer(64, 256, 64)) == ("group", 64)
    assert sdist._layer_kind(_layer(64, 256, 128)) != sdist._layer_kind(_layer(64, 256, 64))


def test_plan_rounds_keeps_kinds_apart():
    layers = _mixed(128, 256, copies=3)
    rounds, root = sdist.plan_rounds(layers, 8)
    assert len(rounds) == 4 and sorted(l for r in rounds for l in r) == list(range(len(layers)))
    for members in rounds:
        assert len(members) == 3 and len(_kinds_of(layers, members)) == 1
    assert [sdist._layer_kind(layers[r[0]]) for r in rounds] == [("group", 64), ("group", 128), "row", "unscaled"]


def test_short_rounds_keep_kinds_apart():
    class Backend(sdist.Backend):
        local_batch, short_rows = 8, 6144

    layers = _mixed(1024, 4096, copies=3)
    rounds = sdist._short_rounds(layers, list(range(len(layers))), Backend())
    assert sorted(l for r in rounds for l in r) == list(range(len(layers)))
    assert len(rounds) == 4
    for members in rounds:
        assert len(_kinds_of(layers, members)) == 1


def test_group_rounds_keep_kinds_apart():
    class Backend(sdist.Backend):
        def group_limit(self, layer, rows):
            return 64

    layers = _mixed(256, 768, copies=4)
    rounds, _ = sdist.plan_rounds(layers, 2)
    groups = sdist._group_rounds(rounds, layers, Backend(), 0, 2)
    assert len(groups) == 4
    for g in groups:
        assert len(_kinds_of(layers, [l for r in g for l in rounds[r]])) == 1


def test_can_batch_keeps_kinds_apart():
    from sleekit_amd import codebook

    be = sdist.HipBackend(codebook.UniformCodebook(8, -1, 1), "diag", 0.01, 0)
    for a in KINDS:
        for b in KINDS:
            pair = [_layer(128, 256, a), _layer(128, 256, b)]
            assert be.can_batch(pair, 0, 128) == (a == b), (a, b)


class _Untouched:
    """A backend that must not be reached: quantize_stream refuses before any factorisation or collective."""

    def __init__(self, moves=0):
        self.moves = moves

    def __getattr__(self, name):
        raise AssertionError(f"backend.{name} reached")


def test_stream_refuses_a_local_search_with_group_scales():
    layers = [_layer(64, 256, "row"), _layer(64, 256, 64)]
    with pytest.raises(NotImplementedError, match="group scales"):
        sdist.quantize_stream(layers, _Untouched(moves=5))


@pytest.mark.parametrize(
    "bad",
    [
        dict(gscale=torch.ones(64, 8)),                             # wrong shape for g = 64
        dict(gscale=torch.ones(32, 4)),                             # wrong row count
        dict(gscale=torch.ones(64, 4, dtype=torch.float64)),        # not float32
        dict(group_size=48, gscale=torch.ones(64, 5)),              # g does not divide n
        dict(group_size=0),                                         # g < 1
        dict(group_size=64.0),                                      # not an int
        dict(scale=torch.ones(64)),                                 # both scale kinds
        dict(group_size=None),                                      # gscale without group_size
    ],
)
def test_stream_refuses_bad_group_scales(bad):
    lay = _layer(64, 256, 64)
    lay.update(bad)
    if lay.get("group_size") is None:
        del lay["group_size"]
    with pytest.raises(ValueError, match="layer 1"):
        sdist.quantize_stream([_layer(64, 256, "unscaled"), lay], _Untouched())
