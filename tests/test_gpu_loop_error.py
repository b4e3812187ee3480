"""The layer error the loop carries (slk_gptq_quantize_batch_error) through the callers that select it: HipBackend.run_rows,
the batched rounds and quantize_stream.  A layer that VOUCHES `symmetric=True` gets it (no product of its own); everything
else keeps the product, bit for bit.

Bounds (relative): every row within 1e-5 of the float64 product of the returned Q, the layer's mean within 1e-6 -- the
bounds the suite holds the layer error to; against the kernel's own NumPy model (tests/loop_error_model.py: the same
formula from the oracle's E) within 2e-6 per row: float32 output rounding (6e-8) plus summation order in float64 (1e-13),
the rest being room for the cancellation in scale^2 * S_E - lambda * S_d (lambda * S_d is below a few percent of the result).
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loop_error_model as model
from oracle.grid import TableGrid, UniformGrid


@pytest.fixture(scope="module")
def amd():
    import sleekit_amd
    from sleekit_amd import _lib, codebook, dist, engine, groups, synth

    class NS:
        pass

    ns = NS()
    ns.lib, ns.codebook, ns.dist, ns.engine, ns.groups, ns.synth, ns.pkg = _lib, codebook, dist, engine, groups, synth, sleekit_amd
    return ns


class Products:
    """Counts the calls of the product routes (engine.row_errors_batch / row_errors) while it is open."""

    def __init__(self, engine):
        self.engine, self.calls = engine, 0

    def __enter__(self):
        self.saved = (self.engine.row_errors_batch, self.engine.row_errors)

        def batch(*a, **k):
            self.calls += 1
            return self.saved[0](*a, **k)

        def single(*a, **k):
            self.calls += 1
            return self.saved[1](*a, **k)

        self.engine.row_errors_batch, self.engine.row_errors = batch, single
        return self

    def __exit__(self, *exc):
        self.engine.row_errors_batch, self.engine.row_errors = self.saved
        return False


def device_layer(amd, R, n, seed, scaled=True, strip=False, vouch=True):
    L = amd.synth.make_layer_device(R, n, seed, torch.device("cuda"))
    lay = dict(W=L["W"], H=L["H"])
    if strip:  # H - m m^T, made as bench.py's cfg3 makes it
        out = torch.empty_like(L["H"])
        from sleekit_amd import _device as dev

        amd.lib.check(amd.lib.lib.slk_hessian_strip_mean(dev.ptr(L["H"]), dev.ptr(L["mean"]), n, dev.ptr(out), dev.stream_handle()))
        lay["H"] = out
    if scaled:
        lay["scale"] = L["scale"]
    assert torch.equal(lay["H"], lay["H"].T)
    if vouch:
        lay["symmetric"] = True
    return lay


def unvouched(lay):
    return {k: v for k, v in lay.items() if k != "symmetric"}


def exact_rows(lay, Q):
    """(W - Q) H (W - Q)^T per row in float64 on the device, of the float32 values as stored."""
    D = lay["W"].double() - Q.double()
    return ((D @ lay["H"].double()) * D).sum(dim=1)


def check_against_float64(lay, shard, what):
    want = exact_rows(lay, shard["Q"])
    got = shard["row_err"].double()
    rows = float(((got - want).abs() / want).max())
    mean = float((got.mean() - want.mean()).abs() / want.mean())
    print(f"{what}: worst row {rows:.3g} of float64, layer mean {mean:.3g}")
    assert rows <= 1e-5, what
    assert mean <= 1e-6, what
    return rows


def same_shard(a, b):
    assert torch.equal(a["Q"], b["Q"])
    assert (a["idx"] is None) == (b["idx"] is None) and (a["idx"] is None or torch.equal(a["idx"], b["idx"]))
    if "info" in a or "info" in b:
        assert torch.equal(a["info"], b["info"])


def make_codebook(amd, kind):
    """(device codebook, oracle grid) of `kind`: a number of levels, or "nf4"."""
    if kind == "nf4":
        return amd.codebook.Codebook.nf4(), TableGrid.nf4()
    return amd.codebook.UniformCodebook(kind, -1, 1), UniformGrid(kind, -1.0, 1.0)


# (R, n, seed, codebook, order, row scales, H - m m^T)
ROWS_CASES = [
    (100, 320, 5101, 8, "diag", True, False),
    (48, 172, 5102, 3, "none", True, False),
    (128, 1100, 5103, 16, "diag", False, False),
    (100, 320, 5104, 4, "err", False, False),
    (70, 320, 5105, "nf4", "diag", True, False),
    (64, 2048, 5106, 8, "diag", True, False),
    (128, 1100, 5107, 3, "diag", True, True),  # cfg3's stripped H
]


@pytest.mark.parametrize("R,n,seed,kind,order,scaled,strip", ROWS_CASES, ids=lambda v: str(v))
def test_run_rows_takes_the_loops_error(amd, R, n, seed, kind, order, scaled, strip):
    cb, grid = make_codebook(amd, kind)
    lay = device_layer(amd, R, n, seed, scaled, strip)
    be = amd.dist.HipBackend(cb, order, 0.01, 0, with_error=True, overlap=False)
    with Products(amd.engine) as p:
        fac = be.factorize(lay)
        shard = dict(be.run_rows(lay, 0, R, fac), info=fac[2])
        assert p.calls == 0
        plain_lay = unvouched(lay)
        fac0 = be.factorize(plain_lay)
        plain = dict(be.run_rows(plain_lay, 0, R, fac0), info=fac0[2])
        assert p.calls == 1
    same_shard(shard, plain)
    check_against_float64(lay, shard, f"run_rows {R}x{n} {kind} {order}")
    # the product route's own distance, for the record, and the two routes against each other
    check_against_float64(lay, plain, f"  (product route) {R}x{n}")
    # the kernel's NumPy model from the oracle's E
    host = {k: v.cpu().numpy() for k, v in lay.items() if isinstance(v, torch.Tensor)}
    Qw, E = model.quantize(host["W"], host["H"], grid, host.get("scale"), order)
    if not np.array_equal(Qw, shard["Q"].cpu().numpy()):
        pytest.fail("the oracle's Q differs from the GPU's on this layer: the model cannot be compared")
    want = model.carried_row_errors(host["W"], Qw, E, host["H"], 0.01, host.get("scale")).astype(np.float64)
    got = shard["row_err"].cpu().numpy().astype(np.float64)
    off = float((np.abs(got - want) / want).max())
    print(f"  against the NumPy model: worst row {off:.3g}")
    assert off <= 2e-6


def test_batched_rounds_take_the_loops_error(amd):
    """run_round_local on a ragged stack of three 1100 x 1600 (padded to 1152 rows a layer) and run_round_stacked on layers
    factored one by one: no product, the unvouched round's Q / idx / info, the float64 product's rows."""
    cb = amd.codebook.UniformCodebook(8, -1, 1)
    be = amd.dist.HipBackend(cb, "diag", 0.01, 0, with_error=True, overlap=False)
    lays = [device_layer(amd, 1100, 1600, 5200 + i) for i in range(3)]
    with Products(amd.engine) as p:
        shards = be.run_round_local(lays)
        assert p.calls == 0
        plain = be.run_round_local([unvouched(l) for l in lays])
        assert p.calls == 1
        again = be.run_round_local(lays)
    for lay, a, b, c in zip(lays, shards, plain, again):
        same_shard(a, b)
        assert a["row_err"].shape == (1100,)
        assert torch.equal(a["row_err"], c["row_err"])  # two runs: the same bits
        check_against_float64(lay, a, "run_round_local 1100x1600")
    # unscaled, 4 levels, factored one by one
    cb4 = amd.codebook.UniformCodebook(4, -1, 1)
    be4 = amd.dist.HipBackend(cb4, "diag", 0.01, 0, with_error=True, overlap=False)
    lays = [device_layer(amd, 64, 2048, 5210 + i, scaled=False) for i in range(3)]
    with Products(amd.engine) as p:
        shards = be4.run_round_stacked(lays, [be4.factorize(l) for l in lays])
        assert p.calls == 0
        plain = be4.run_round_stacked([unvouched(l) for l in lays], [be4.factorize(unvouched(l)) for l in lays])
        assert p.calls == 1
    for lay, a, b in zip(lays, shards, plain):
        same_shard(a, b)
        check_against_float64(lay, a, "run_round_stacked 64x2048")


def test_stream_on_side_streams_big_layers(amd):
    """quantize_stream with join=False on the side streams: one 4096 x 4096 layer with a golden seed and 512 rows of
    4096 x 11008; two runs and overlap=False against the default streams give the same bits."""
    from sleekit_amd import _device as sdev

    cb = amd.codebook.UniformCodebook(8, -1, 1)
    lays = [device_layer(amd, 4096, 4096, 1007), device_layer(amd, 512, 11008, 5301)]
    runs = []
    for overlap in (True, True, False):
        be = amd.dist.HipBackend(cb, "diag", 0.01, 0, with_error=True, overlap=overlap)
        with Products(amd.engine) as p:
            out = amd.dist.quantize_stream(lays, be, join=False)
            assert p.calls == 0
        torch.cuda.synchronize()
        sdev.raise_pending()
        runs.append(out)
    for a, b in ((runs[0], runs[1]), (runs[0], runs[2])):
        for x, y in zip(a, b):
            same_shard(x, y)
            assert torch.equal(x["row_err"], y["row_err"])
    for lay, sh in zip(lays, runs[0]):
        check_against_float64(lay, sh, f"quantize_stream {tuple(lay['W'].shape)}")
    # the same layers unvouched: the product, the same Q
    be = amd.dist.HipBackend(cb, "diag", 0.01, 0, with_error=True)
    with Products(amd.engine) as p:
        plain = amd.dist.quantize_stream([unvouched(l) for l in lays], be)
        assert p.calls == 2
    for x, y in zip(runs[0], plain):
        same_shard(x, y)
        rel = float(((x["row_err"].double() - y["row_err"].double()).abs() / y["row_err"].double()).max())
        print(f"carried against the product route: worst row {rel:.3g}")
        assert rel <= 2e-5  # (each within 1e-5 of float64)


def test_fallbacks_keep_the_product_bit_for_bit(amd):
    """Unvouched, an H made asymmetric by one element, a local search, grouped layers, err order with scales (the loop then
    runs on a pre-divided copy) and the option: each gives the row_err it gives with "no_loop_error" set, bit for bit."""
    cb = amd.codebook.UniformCodebook(8, -1, 1)
    R, n = 128, 320
    base = device_layer(amd, R, n, 5401)
    skew = unvouched(base)
    skew["H"] = base["H"].clone()
    skew["H"][3, 200] *= 1.0 + 2.0 ** -20
    grouped = dict(W=base["W"], H=base["H"], symmetric=True, group_size=32,
                   gscale=(base["W"].abs().reshape(R, n // 32, 32).amax(dim=2) + 0.05).contiguous())

    def run(lay, order="diag", moves=0, stacked=False):
        be = amd.dist.HipBackend(cb, order, 0.01, moves, with_error=True, overlap=False)
        with Products(amd.engine) as p:
            if stacked:
                sh = be.run_round_local([lay, lay])[0]
            else:
                sh = be.run_rows(lay, 0, R, be.factorize(lay))
        return sh, p.calls

    cases = [("unvouched", unvouched(base), {}, 1), ("asymmetric H", skew, {}, 1), ("moves = 5", base, dict(moves=5), 0),
             ("grouped", grouped, {}, 1), ("grouped round", grouped, dict(stacked=True), 1), ("unvouched round", unvouched(base), dict(stacked=True), 1),
             ("err order with scales", base, dict(order="err"), 1)]
    for name, lay, kw, products in cases:
        got, calls = run(lay, **kw)
        assert calls == products, name
        with amd.lib.option("no_loop_error", 1):
            want, calls = run(lay, **kw)
        assert calls == products, name
        assert torch.equal(got["row_err"], want["row_err"]) and torch.equal(got["Q"], want["Q"]), name
    # the option itself: a vouched layer goes back to the product, in rows and in rounds
    for stacked in (False, True):
        carried, calls = run(base, stacked=stacked)
        assert calls == 0
        with amd.lib.option("no_loop_error", 1):
            want, calls = run(base, stacked=stacked)
            assert calls == 1
        plain, _ = run(unvouched(base), stacked=stacked)
        assert torch.equal(want["row_err"], plain["row_err"]) and torch.equal(want["Q"], carried["Q"])
        assert not torch.equal(want["row_err"], carried["row_err"])  # (close, not bit-equal: said so in the header)


def test_indefinite_hessian_still_raises_naming_the_layer(amd):
    """Vouched layers, one with a Hessian that is not positive definite: the reference's LinAlgError, naming the layer --
    through the batched round of small layers and through the layer-by-layer route."""
    cb = amd.codebook.UniformCodebook(8, -1, 1)
    small = [device_layer(amd, 128, 192, 5500 + i) for i in range(4)]
    small[2]["H"] = small[2]["H"].clone()
    small[2]["H"][100, 100] = -2.0
    be = amd.dist.HipBackend(cb, "diag", 0.01, 0, with_error=True)
    with pytest.raises(np.linalg.LinAlgError, match=r"layer 2 \(128 x 192\)"):
        amd.dist.quantize_stream(small, be)
    wide = [device_layer(amd, 64, 1600, 5510 + i) for i in range(2)]
    wide[1]["H"] = wide[1]["H"].clone()
    wide[1]["H"][900, 900] = -2.0
    be2 = amd.dist.HipBackend(cb, "diag", 0.01, 0, with_error=True)
    be2.local_batch = 1  # layer by layer
    with pytest.raises(np.linalg.LinAlgError, match=r"layer 1 \(64 x 1600\)"):
        amd.dist.quantize_stream(wide, be2)
