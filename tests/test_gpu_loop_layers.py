"""The column loop over layers that are NOT one stack (slk_gptq_quantize_layers through engine.gptq_loop with lists of
tensors): the same bits as a loop per layer -- Q, idx, the scaled errors E and the carried row errors -- wherever the layers'
W, scale, order and U lie, and through quantize_stream's stacks of full-height layers (HipBackend.tall_stack).

Shapes: the smallest at which the layer indexing can go wrong.  64 and 128 rows a layer are one and two trailing row tiles
(with 32-row window workgroups the layer boundary falls between two workgroups); 96 columns are one window and no trailing
update; 544 are eight windows of 68 columns (leaves of 32 / 32 / 4), trailing updates with K = 68 (a guarded last K-step) over
interior and edge column tiles."""

import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DAMP = 0.01


def _codebook(levels):
    from sleekit_amd import codebook, engine

    return engine.require_uniform(codebook.UniformCodebook(levels, -1, 1))


_made = {}


def _layers(rpl, B, n):
    """B synthetic layers with their factors, every W, scale, order and U an allocation of its own, made kind by kind and
    last layer first with odd-sized spacers in between: no two of a call's tensors are neighbours in layer order.
    Made once per shape and left unchanged."""
    from sleekit_amd import _lib, engine, synth

    if (rpl, B, n) in _made:
        return _made[(rpl, B, n)]
    dev = torch.device("cuda", 0)
    host = [synth.make_layer(rpl, n, 7300 + 17 * b + n + rpl) for b in range(B)]
    Hs = [torch.from_numpy(L["H"]).to(dev) for L in host]
    facs = [engine.factorize(H, n, DAMP, _lib.ORDER_MODES["diag"]) for H in Hs]
    spacers, out = [], dict(H=Hs, W=[None] * B, scale=[None] * B, order=[None] * B, U=[None] * B, host=host)
    for kind in ("U", "W", "order", "scale"):
        for b in reversed(range(B)):
            src = dict(U=facs[b][1], order=facs[b][0], W=torch.from_numpy(host[b]["W"]), scale=torch.from_numpy(host[b]["scale"]))[kind]
            out[kind][b] = src.to(dev).clone()
            spacers.append(torch.empty(1000 + 24 * b + 8 * len(spacers), dtype=torch.uint8, device=dev))
    for b in range(B):
        assert int(facs[b][2].item()) == 0
    out["spacers"] = spacers
    _made[(rpl, B, n)] = out
    return out


_refs = {}


def _reference(rpl, B, n, levels):
    """B separate single-layer loops on the same tensors (the route as it was): computed once per case, never changed."""
    from sleekit_amd import engine

    key = (rpl, B, n, levels)
    if key not in _refs:
        L = _layers(rpl, B, n)
        _refs[key] = [engine.gptq_loop(L["W"][b], _codebook(levels), L["order"][b], L["U"][b], 32, 8, scale=L["scale"][b], want_E=True,
                                       unscale=True, Hs=[L["H"][b]], damp=DAMP) for b in range(B)]
    return _refs[key]


def _check(got, want, picks=None):
    """got: the stacked (Q, idx, E, row_err) of one call over the layers `picks` (default: all, in order)."""
    picks = range(len(want)) if picks is None else picks
    for slot, b in enumerate(picks):
        for name, g, w in zip(("Q", "idx", "E", "row_err"), got, want[b]):
            assert torch.equal(g[slot], w), (name, slot, b)


def _loop(L, levels, picks=None, U=None):
    from sleekit_amd import engine

    picks = range(len(L["W"])) if picks is None else picks
    U = L["U"] if U is None else U
    return engine.gptq_loop([L["W"][b] for b in picks], _codebook(levels), [L["order"][b] for b in picks], [U[b] for b in picks], 32, 8,
                            scale=[L["scale"][b] for b in picks], want_E=True, unscale=True, Hs=[L["H"][b] for b in picks], damp=DAMP)


@pytest.mark.parametrize("n", [96, 544])
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("rpl", [64, 128])
def test_layers_anywhere_equal_a_loop_per_layer(rpl, B, n):
    from sleekit_amd import _lib

    L = _layers(rpl, B, n)
    for levels in (8, 3):
        want = _reference(rpl, B, n, levels)
        try:
            for window_rows in (16, 32):
                _lib.set_option("window_rows", window_rows)
                got = _loop(L, levels)
                assert got[0].shape == (B, rpl, n) and got[3].shape == (B, rpl)
                _check(got, want)
        finally:
            _lib.set_option("window_rows", 0)
        _check(_loop(L, levels), want)  # and the library's own choice of window rows


def test_unscaled_layers_and_the_plain_loop():
    """No scales and no carried error: the other form of the same entry."""
    from sleekit_amd import engine

    L, cb = _layers(128, 2, 544), _codebook(8)
    Q, idx, E, err = engine.gptq_loop(L["W"], cb, L["order"], L["U"], 32, 8, want_E=True)
    assert err is None
    for b in range(2):
        q1, i1, e1, _ = engine.gptq_loop(L["W"][b], cb, L["order"][b], L["U"][b], 32, 8, want_E=True)
        assert torch.equal(Q[b], q1) and torch.equal(idx[b], i1) and torch.equal(E[b], e1), b


@pytest.mark.parametrize("offset_bytes", [16, 8])
def test_a_factor_off_its_allocation_start(offset_bytes):
    """One U 16 bytes into a larger buffer: aligned for the period kernel and for nothing wider.  One U 8 bytes in: the whole
    call takes the general window kernel, and the trailing update its guarded loads.  The same bits either way."""
    rpl, B, n = 128, 2, 544
    L = _layers(rpl, B, n)
    k = offset_bytes // 8
    buf = torch.zeros(n * n + 4, dtype=torch.float64, device=L["U"][1].device)
    moved = buf[k:k + n * n].view(n, n)
    moved.copy_(L["U"][1])
    assert moved.data_ptr() % 16 == offset_bytes % 16 and moved.data_ptr() % 32 != 0 and moved.is_contiguous()
    for levels in (8, 3):
        _check(_loop(L, levels, U=[L["U"][0], moved]), _reference(rpl, B, n, levels))


def test_layers_in_another_order_than_they_lie_in_memory():
    rpl, B, n = 64, 3, 544
    L = _layers(rpl, B, n)
    dev = L["W"][0].device
    # one allocation per kind, the layers in it in order 0, 1, 2; the call takes them as 2, 0, 1
    packed = dict(L)
    for kind in ("W", "scale", "order", "U"):
        stack = torch.stack(L[kind]).to(dev)
        packed[kind] = [stack[b] for b in range(B)]
    picks = [2, 0, 1]
    assert packed["U"][2].data_ptr() > packed["U"][0].data_ptr()
    _check(_loop(packed, 8, picks=picks), _reference(rpl, B, n, 8), picks)


def test_indices_are_the_oracles():
    """One case held to the CPU oracle's indices, as test_batch_entry_points does for the stacked entry."""
    from oracle import grid, scaling_ref

    rpl, B, n = 64, 2, 544
    L = _layers(rpl, B, n)
    _, idx, _, _ = _loop(L, 8)
    g = grid.UniformGrid(8, -1, 1)
    for b, host in enumerate(L["host"]):
        want = scaling_ref.quantize_scaled(host["W"], host["scale"], g, host["H"], "diag", DAMP, 0)
        assert np.array_equal(idx[b].cpu().numpy(), g.index(scaling_ref.divide_rows(want, host["scale"], 0))), b


def _stream_layers(count, bad=None):
    from sleekit_amd import synth

    dev = torch.device("cuda", 0)
    layers = []
    for i in range(count):
        host = synth.make_layer(128, 544, 7700 + i)
        lay = {k: torch.from_numpy(host[k]).to(dev) for k in ("W", "H", "scale")}
        assert torch.equal(lay["H"], lay["H"].T)
        lay["symmetric"] = True
        layers.append(lay)
    if bad is not None:
        layers[bad]["H"] = layers[bad]["H"].clone()
        layers[bad]["H"][300, 300] = -2.0
    return layers


def _backend(tall_stack, calls=None):
    from sleekit_amd import codebook
    from sleekit_amd import dist as sdist

    be = sdist.HipBackend(codebook.UniformCodebook(8, -1, 1), "diag", DAMP, 0, with_error=True, overlap=(3, 1))
    be.local_batch = 1  # layer by layer: the route of full-height layers
    be.tall_stack = tall_stack
    if calls is not None:
        run_tall = be.run_tall
        be.run_tall = lambda members, factors: (calls.append(len(members)), run_tall(members, factors))[1]
    return be


@pytest.mark.parametrize("count", [2, 3])
def test_stream_stacks_of_two_equal_layer_by_layer(count):
    """quantize_stream on side streams (3, 1), unjoined: pairs of same-shaped layers through one loop (a remainder of one
    through the same call) give the shards of the layer-by-layer route bit for bit, each with its own status word."""
    from sleekit_amd import _device as sdev
    from sleekit_amd import dist as sdist

    layers = _stream_layers(count)
    try:
        sdev.lazy_errors = True
        calls = []
        want = sdist.quantize_stream(layers, _backend(1, calls), join=False)
        torch.cuda.synchronize()
        sdev.raise_pending()
        assert calls == []
        got = sdist.quantize_stream(layers, _backend(2, calls), join=False)
        torch.cuda.synchronize()
        sdev.raise_pending()
        assert calls == ([2] if count == 2 else [2, 1])
    finally:
        sdev.lazy_errors = False
        sdev._pending_info.clear()
    assert len(got) == count
    for l, (a, b) in enumerate(zip(got, want)):
        assert a["rows"] == b["rows"] == (0, 128)
        for key in ("Q", "idx", "row_err"):
            assert torch.equal(a[key], b[key]), (l, key)
        assert a["info"].shape == (1,) and int(a["info"].item()) == 0
    assert len({sh["info"].data_ptr() for sh in got}) == count  # a status word per layer


def test_indefinite_hessian_in_the_second_layer_of_a_stack_raises_naming_it():
    from sleekit_amd import _device as sdev
    from sleekit_amd import dist as sdist

    layers = _stream_layers(3, bad=1)
    try:
        sdev.lazy_errors = True
        calls = []
        sdist.quantize_stream(layers, _backend(2, calls), join=False)
        torch.cuda.synchronize()
        assert calls == [2, 1]
        with pytest.raises(np.linalg.LinAlgError, match=r"layer 1 \(128 x 544\)"):
            sdev.raise_pending()
    finally:
        sdev.lazy_errors = False
        sdev._pending_info.clear()
