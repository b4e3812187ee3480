"""The randomized Hadamard rotation on the MI355X: slk_hadamard_rows against tests/rotation_model.py bit for bit, then
Rotation.hessian, the rotated path of Sleekit against the oracles on the rotated pair, RotatedLinear, and the error ratio
the rotation is for.

The butterfly network fixes both operands of every addition, so the kernel is held to the model's BITS on random data as
well as on integers (NaNs compared as NaN).  Shapes (tests/rotation_model.py, "the GPU matrix"): a lane holds 16
consecutive columns, so blocks 2, 8, 16 stay in registers, 32 .. 1024 cross the lanes of a wave, 2048 and 4096 cross 2 and
4 waves; one block a row and three; 1, 5 and 67 rows.  tests/test_rotation_cpu.py shows that a wrong stage order, a reversed
subtraction, signs on the wrong side, a missing factor and a shifted block boundary each change the model's bits at every
one of these shapes.

Tolerances.  The layer test: |y - y64| <= (K + 1) 2^-23 sum |x' w| (+ |bias|), the bound of DESIGN.md section 14 for K
float32 additions and the bias.  The bias test: rtol 1e-5 on a float32 row sum, as everywhere in this suite.  The error
ratio: at most 0.6, against 0.39 (3-bit) and 0.40 (MXFP4) measured with the float64 reference on the same inputs and signs.
"""

import numpy as np
import pytest
import torch

import rotation_model as model

pytestmark = pytest.mark.gpu

CODE = {"f32": 0, "bf16": 1, "f16": 2, "f64": 3}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def to_torch(x, kind):
    """A model array on the device (bfloat16 travels as its bits)."""
    if kind == "bf16":
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def from_torch(t, kind):
    if kind == "bf16":
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def raw(xd, y_kind, block, signs=None, transposed=False, out=None):
    """slk_hadamard_rows itself on a contiguous (rows, n) device tensor; signs a float32 device tensor or None."""
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib

    rows, n = xd.shape
    assert xd.is_contiguous() and (signs is None or (signs.dtype == torch.float32 and signs.numel() == n))
    x_kind = {v: k for k, v in TORCH.items()}[xd.dtype]
    if out is None:
        out = torch.empty((rows, n), dtype=TORCH[y_kind], device=xd.device)
    _lib.check(_lib.lib.slk_hadamard_rows(dev.ptr(xd), CODE[x_kind], dev.ptr(out), CODE[y_kind], rows, n, block, dev.ptr(signs),
                                          1 if transposed else 0, dev.stream_handle()))
    return out


def first_difference(got, want, kind):
    bad = np.argwhere((model.bits_of(got) != model.bits_of(want)) & ~(model.is_nan(got, kind) & model.is_nan(want, kind)))
    r, c = bad[0]
    return f"{len(bad)} of {want.size} differ, first at ({r}, {c}): got {got[r, c]!r}, want {want[r, c]!r}"


# ---------------------------------------------------------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("block", model.BLOCKS)
def test_kernel_equals_the_model_bit_for_bit(block):
    butterflies = {}
    for width in model.WIDTHS:
        n = width * block
        for x_kind, y_kind in model.KINDS:
            for data in model.DATA:
                x67, s = model.case_input(x_kind, data, block, n)
                xd, sd = to_torch(x67, x_kind), torch.from_numpy(s).cuda()
                for signs in (None, s):
                    for transposed in (False, True):
                        key = (n, x_kind, data, signs is not None, transposed)
                        if key not in butterflies:  # (shared by the output kinds of one input kind)
                            butterflies[key] = model.transform(model.to_compute(x67, x_kind), block, signs, transposed)
                        want = model.to_kind(butterflies[key], y_kind)
                        for rows in model.ROWS:
                            got = from_torch(raw(xd[:rows], y_kind, block, None if signs is None else sd, transposed), y_kind)
                            assert model.same(got, want[:rows], y_kind), (
                                f"block {block}, n {n}, rows {rows}, {x_kind} -> {y_kind}, {data}, signs {signs is not None}, "
                                f"transposed {transposed}: " + first_difference(got, want[:rows], y_kind))


def test_public_surface_equals_the_model():
    from sleekit_amd import Rotation

    n, block = 192, 64
    x, s = model.make_input("f32", "random", 10, n, 11), model.signs_for(n, 11)
    rot = Rotation.from_signs(s, block)
    assert rot.n == n and rot.block == block and rot.signs.is_cuda and rot.signs.dtype == torch.float32
    want = model.rows_model(x, "f32", "f32", block, s)
    got = rot.apply(x)  # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and model.same(got, want, "f32")
    back = rot.apply_t(got)
    assert model.same(back, model.rows_model(want, "f32", "f32", block, s, True), "f32")
    # an orthogonal matrix and its transpose: the model's bound (7 roundings a pass, sum |v| c <= 8 max |v| for a block of 64)
    # for the way there, and for the way back on values of up to 8 max |x|
    assert np.abs(back - x).max() <= 7 * 2.0 ** -24 * (8 + 64) * np.abs(x).max() * (1 + 2.0 ** -20)
    xd = torch.from_numpy(x).cuda().reshape(2, 5, n)
    got = rot.apply(xd)
    assert got.is_cuda and tuple(got.shape) == (2, 5, n) and model.same(got.reshape(10, n).cpu().numpy(), want, "f32")
    low = rot.apply(xd.bfloat16())
    xb = model.to_kind(x, "bf16")
    assert low.dtype == torch.bfloat16 and model.same(from_torch(low.reshape(10, n), "bf16"), model.rows_model(xb, "bf16", "bf16", block, s), "bf16")
    wide = rot.apply(xd.bfloat16(), dtype=torch.float32)
    assert wide.dtype == torch.float32 and model.same(wide.reshape(10, n).cpu().numpy(), model.rows_model(xb, "bf16", "f32", block, s), "f32")
    half = rot.apply_t(x.astype(np.float16))
    assert half.dtype == np.float16 and model.same(half, model.rows_model(x.astype(np.float16), "f16", "f16", block, s, True), "f16")
    d = rot.apply(x.astype(np.float64))
    assert d.dtype == np.float64 and model.same(d, model.rows_model(x.astype(np.float64), "f64", "f64", block, s), "f64")
    assert tuple(rot.apply(x[0]).shape) == (n,) and model.same(rot.apply(x[0])[None], want[:1], "f32")
    for call in (lambda: rot.apply(x[:, :64]), lambda: rot.apply(x.astype(np.float64), dtype=torch.float32),
                 lambda: rot.apply(x, dtype=torch.float64), lambda: rot.apply(x, dtype=torch.bfloat16),
                 lambda: rot.apply(x.astype(np.int32)), lambda: Rotation.from_signs(s * 2, block), lambda: Rotation.from_signs(s, 128)):
        with pytest.raises(ValueError):
            call()
    # the seeded rule on the device is the host's
    from sleekit_amd import rotation

    assert np.array_equal(Rotation(n, seed=5).signs.cpu().numpy(), rotation.make_signs(n, 5)) and Rotation(n).block == 64


# ---------------------------------------------------------------------------------------------------------------- 2. one case each
def test_rows_past_65535():
    rows, n = 65537, 32
    x, s = model.make_input("f32", "random", rows, n, 21), model.signs_for(n, 21)
    got = raw(torch.from_numpy(x).cuda(), "f32", 32, torch.from_numpy(s).cuda()).cpu().numpy()
    want = model.rows_model(x, "f32", "f32", 32, s)
    assert model.same(got, want, "f32"), first_difference(got, want, "f32")


@pytest.mark.parametrize("kind,block,n", [("f32", 64, 192), ("bf16", 4096, 4096), ("f64", 2, 6)])
def test_in_place(kind, block, n):
    x, s = model.make_input(kind, "random", 5, n, 22), model.signs_for(n, 22)
    xd = to_torch(x, kind)
    out = raw(xd, kind, block, torch.from_numpy(s).cuda(), True, out=xd)
    assert out.data_ptr() == xd.data_ptr()
    want = model.rows_model(x, kind, kind, block, s, True)
    assert model.same(from_torch(xd, kind), want, kind), first_difference(from_torch(xd, kind), want, kind)


@pytest.mark.parametrize("kind,block,n", [("f32", 2, 48), ("bf16", 2, 48), ("bf16", 128, 128), ("f32", 128, 128)])
def test_one_element_past_a_16_byte_boundary(kind, block, n):
    rows = 5
    x, s = model.make_input(kind, "random", rows, n, 23), model.signs_for(n, 23)
    want = model.rows_model(x, kind, kind, block, s)
    buf = torch.zeros(rows * n + 1, dtype=TORCH[kind], device="cuda")
    view = buf[1:].view(rows, n)
    view.copy_(to_torch(x, kind))
    sbuf = torch.zeros(n + 1, device="cuda")
    sview = sbuf[1:]
    sview.copy_(torch.from_numpy(s))
    obuf = torch.zeros(rows * n + 1, dtype=TORCH[kind], device="cuda")
    oview = obuf[1:].view(rows, n)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0 and sview.data_ptr() % 16 != 0 and oview.data_ptr() % 16 != 0
    sd = torch.from_numpy(s).cuda()
    for xin, signs, out in ((view, sd, None), (to_torch(x, kind), sview, None), (to_torch(x, kind), sd, oview), (view, sview, oview)):
        got = from_torch(raw(xin, kind, block, signs, False, out=out), kind)
        assert model.same(got, want, kind), first_difference(got, want, kind)
    assert float(obuf[0]) == 0.0  # nothing written in front of the view


def test_repeated_calls_are_bit_equal():
    x, s = model.make_input("f32", "random", 67, 8192, 24), model.signs_for(8192, 24)
    xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda()
    first = raw(xd, "f32", 4096, sd)
    for _ in range(3):
        assert torch.equal(raw(xd, "f32", 4096, sd).view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("kind", ["f32", "bf16", "f64"])
def test_non_finite_stays_in_its_block(kind):
    rows, n, block = 5, 192, 64
    x, s = model.make_input(kind, "random", rows, n, 25), model.signs_for(n, 25)
    x = model.to_compute(x, kind)
    x[3, 127] = 0  # the last element of block 1 of row 3
    base = from_torch(raw(to_torch(model.to_kind(x, kind), kind), kind, block, torch.from_numpy(s).cuda()), kind)
    for bad in (np.nan, np.inf, -np.inf):
        for transposed in (False, True):
            x[3, 127] = 0
            zero = from_torch(raw(to_torch(model.to_kind(x, kind), kind), kind, block, torch.from_numpy(s).cuda(), transposed), kind)
            x[3, 127] = bad
            xin = model.to_kind(x, kind)
            got = from_torch(raw(to_torch(xin, kind), kind, block, torch.from_numpy(s).cuda(), transposed), kind)
            assert model.same(got, model.rows_model(xin, kind, kind, block, s, transposed), kind)
            touched = np.zeros((rows, n), bool)
            touched[3, 64:128] = True
            assert np.array_equal(model.bits_of(got)[~touched], model.bits_of(zero)[~touched]), bad
            assert not np.isfinite(model.to_compute(got, kind)[touched]).any(), bad
    assert np.isfinite(model.to_compute(base, kind)).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the Hessian
@pytest.fixture(scope="module")
def layer3():
    """synth.make_layer(64, 256, 3): the layer of the measurements (made once, read only)."""
    from sleekit_amd import synth

    L = synth.make_layer(64, 256, 3)
    for a in (L["W"], L["H"], L["mean"], L["scale"]):
        a.setflags(write=False)
    return L


@pytest.mark.parametrize("block", [64, 256])
def test_rotated_hessian(layer3, block):
    from sleekit_amd import Rotation

    rot = Rotation(256, block=block, seed=3)
    s = rot.signs.cpu().numpy()
    got = rot.hessian(torch.from_numpy(np.array(layer3["H"])).cuda())
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (256, 256)
    assert torch.equal(got.view(torch.int32), got.t().contiguous().view(torch.int32))  # bit-symmetric
    want = model.hessian_model(layer3["H"], block, s)
    assert model.same(got.cpu().numpy(), want, "f32"), first_difference(got.cpu().numpy(), want, "f32")
    host = rot.hessian(np.array(layer3["H"]))  # NumPy in, NumPy out
    assert isinstance(host, np.ndarray) and model.same(host, want, "f32")
    # R^T H R is similar to H: the same trace, to float32 rounding of 256 terms
    assert abs(float(np.trace(want.astype(np.float64)) - np.trace(layer3["H"].astype(np.float64)))) <= 1e-5 * np.trace(layer3["H"].astype(np.float64))
    with pytest.raises(ValueError):
        rot.hessian(layer3["H"][:128, :128])


# ---------------------------------------------------------------------------------------------------------------- 4. plumbing
def sleekit_on(L, rotation=None, bias=None):
    """Sleekit over nn.Linear(256, 64) holding the layer's weight (and `bias`, or zeros), with the layer's statistics set."""
    import torch.nn as nn

    from sleekit_amd import Sleekit

    R, n = L["W"].shape
    lin = nn.Linear(n, R).cuda()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(np.array(L["W"])))
        lin.bias.copy_(torch.from_numpy(np.zeros(R, np.float32) if bias is None else bias))
    st = Sleekit(lin, rotation=rotation)
    st.hessian.copy_(torch.from_numpy(np.array(L["H"])))
    st.mean.copy_(torch.from_numpy(np.array(L["mean"])))
    st.count = L["T"]
    return lin, st


@pytest.fixture(scope="module")
def rotated3(layer3):
    """(rot, W', H') of layer3 under Rotation(256, seed=3): W' and H' read back from the device."""
    from sleekit_amd import Rotation

    rot = Rotation(256, seed=3)
    assert rot.block == 256
    Wr = rot.apply(torch.from_numpy(np.array(layer3["W"])).cuda()).cpu().numpy()
    Hr = rot.hessian(torch.from_numpy(np.array(layer3["H"])).cuda()).cpu().numpy()
    Wr.setflags(write=False)
    Hr.setflags(write=False)
    return rot, Wr, Hr


def test_per_row_path_equals_the_oracle_on_the_rotated_pair(layer3, rotated3):
    from oracle import grid, scaling_ref
    from sleekit_amd import synth

    rot, Wr, Hr = rotated3
    scale = synth.make_scale(Wr)
    lin, st = sleekit_on(layer3)
    res = st.quantize_packed(3, scale=scale, rotation=rot)
    g = grid.UniformGrid(8, -1, 1)
    want = scaling_ref.quantize_scaled(np.array(Wr), scale, g, np.array(Hr), "diag", 0.01, 0)
    idx = g.index(scaling_ref.divide_rows(want, scale, 0))
    assert res.rotation is rot and np.array_equal(res.idx.cpu().numpy(), idx)
    assert np.array_equal(res.S.cpu().numpy(), scale)
    back = rot.apply_t(res.Q)
    assert torch.equal(lin.weight.data.view(torch.int32), back.view(torch.int32))
    assert model.same(back.cpu().numpy(), model.rows_model(res.Q.cpu().numpy(), "f32", "f32", 256, rot.signs.cpu().numpy(), True), "f32")


def test_grouped_offsets_path_equals_the_model_on_the_rotated_pair(layer3, rotated3):
    import groups_offsets_model as gom
    from groups_model import oracle_grid

    rot, Wr, Hr = rotated3
    lin, st = sleekit_on(layer3)
    res = st.quantize_packed(3, group_size=32, offsets="mid", rotation=rot)
    O, S, Q = gom.offsets_model(np.array(Wr), np.array(Hr), "8", 32, "diag", "mse", 0.01, 32, 8)
    assert np.array_equal(res.O.cpu().numpy(), O) and np.array_equal(res.S.cpu().numpy(), S)
    assert model.same(res.Q.cpu().numpy(), Q, "f32")
    idx = oracle_grid("8").index((Q - np.repeat(O, 32, axis=1)) / np.repeat(S, 32, axis=1)).astype(np.uint8)
    assert np.array_equal(res.idx.cpu().numpy(), idx) and model.same(gom.rebuild(idx, S, O, "8", 32), Q, "f32")
    assert torch.equal(lin.weight.data.view(torch.int32), rot.apply_t(res.Q).view(torch.int32)) and res.rotation is rot


def test_mxfp4_path_equals_the_model_on_the_rotated_pair(layer3):
    import groups_model
    import mx_model
    from sleekit_amd import Rotation

    rot = Rotation(256, block=128, seed=3)
    Wr = rot.apply(torch.from_numpy(np.array(layer3["W"])).cuda()).cpu().numpy()
    Hr = rot.hessian(torch.from_numpy(np.array(layer3["H"])).cuda()).cpu().numpy()
    lin, st = sleekit_on(layer3, rotation=rot)  # (quantize_mxfp4 keeps its parameter list: the object's rotation)
    res = st.quantize_mxfp4(scale_mode="mse")
    S, E = mx_model.scales_model(Wr, Hr, "mse")
    grd = mx_model.e2m1_grid()
    Q = groups_model.model_grouped(Wr, S, grd, Hr, 32, "diag", 0.01, 32, 8)
    idx = groups_model.indices(Q, S, grd, 32)
    assert np.array_equal(res.idx.cpu().numpy(), idx) and np.array_equal(res.S.cpu().numpy(), S)
    assert np.array_equal(res.codes.cpu().numpy(), mx_model.pack_model(idx, S)[0]) and np.array_equal(res.scales.cpu().numpy(), E)
    assert model.same(res.Q.cpu().numpy(), Q, "f32") and res.rotation is rot
    assert torch.equal(lin.weight.data.view(torch.int32), rot.apply_t(res.Q).view(torch.int32))


def test_bias_correction_in_the_original_basis(layer3, rotated3):
    from sleekit_amd import synth

    rot = rotated3[0]
    b0 = (0.1 * synth.normal_grid(3, 11, 1, 64)[0]).astype(np.float32)
    lin, st = sleekit_on(layer3, bias=b0)
    res = st.quantize(3, bias_correction=True, rotation=rot)
    back = lin.weight.data.cpu().numpy().astype(np.float64)
    assert torch.equal(lin.weight.data.view(torch.int32), rot.apply_t(res.Q).view(torch.int32))
    shift = ((layer3["W"].astype(np.float64) - back) * layer3["mean"].astype(np.float64)).sum(axis=1)
    got = lin.bias.data.cpu().numpy()
    print(f"bias shift: max |shift| = {np.abs(shift).max():.3e}, max |bias - (b0 + shift)| / |bias| = "
          f"{(np.abs(got - (b0 + shift)) / np.abs(got)).max():.3e}")
    assert np.abs(shift).max() > 0
    np.testing.assert_allclose(got, b0.astype(np.float64) + shift, rtol=1e-5)


def test_no_rotation_is_the_call_without_the_keyword(layer3):
    out = []
    for kw in (dict(), dict(rotation=None)):
        for call, args in (("quantize", dict(bias_correction=True)), ("quantize_packed", dict(group_size=32, offsets="mid"))):
            lin, st = sleekit_on(layer3)
            res = getattr(st, call)(3, **args, **kw)
            out.append((lin.weight.data.clone(), lin.bias.data.clone(), res))
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[2].idx, b[2].idx) and a[2].rotation is None and b[2].rotation is None
    # the object's rotation is quantize_mxfp4's alone: quantize without the keyword does not rotate
    from sleekit_amd import Rotation

    lin, st = sleekit_on(layer3, rotation=Rotation(256, seed=3))
    res = st.quantize(3, bias_correction=True)
    assert res.rotation is None and torch.equal(lin.weight.data.view(torch.int32), out[0][0].view(torch.int32))
    assert torch.equal(res.idx, out[0][2].idx)
    lin, st = sleekit_on(layer3)
    with pytest.raises(ValueError):
        st.quantize(3, rotation=Rotation(128))
    with pytest.raises(ValueError):
        st.quantize(3, rotation="hadamard")


# ---------------------------------------------------------------------------------------------------------------- 5. the layer
@pytest.mark.parametrize("form", ["packed", "mxfp4"])
def test_rotated_layer_runs(layer3, form):
    from sleekit_amd import MXLinear, PackedLinear, RotatedLinear, Rotation, packing
    from sleekit_amd.codebook import UniformCodebook

    K, N = 256, 64
    cb = UniformCodebook(8, -1, 1)
    b0 = (0.1 * np.arange(-32, 32) / 32).astype(np.float32)
    if form == "packed":
        rot = Rotation(K, seed=3)
        lin, st = sleekit_on(layer3, bias=b0)
        res = st.quantize_packed(3, group_size=32, rotation=rot)
    else:
        rot = Rotation(K, block=128, seed=3)
        lin, st = sleekit_on(layer3, rotation=rot, bias=b0)
        res = st.quantize_mxfp4()
    mod = RotatedLinear.from_result(lin, res, cb)
    assert isinstance(mod.inner, PackedLinear if form == "packed" else MXLinear) and mod.block == rot.block
    assert torch.equal(mod.signs, rot.signs) and sorted(k for k in mod.state_dict() if not k.startswith("inner.")) == ["_extra_state", "signs"]
    fresh_inner = PackedLinear(K, N, cb, group_size=32).cuda() if form == "packed" else MXLinear(K, N).cuda()
    fresh = RotatedLinear(fresh_inner, Rotation.from_signs(np.ones(K, np.float32), 2))
    fresh.load_state_dict(mod.state_dict())
    assert fresh.block == rot.block and torch.equal(fresh.signs, rot.signs)
    for M in (1, 16, 33):
        x = torch.from_numpy(model.block_gaussian(M, K, 40 + M).astype(np.float32)).cuda()
        for xin in (x, x.bfloat16(), x.half()):
            y = mod(xin)
            xr = rot.apply(xin)
            assert xr.dtype == xin.dtype and y.dtype == xin.dtype and tuple(y.shape) == (M, N)
            assert np.array_equal(model.bits_of(from_torch(y.float(), "f32")), model.bits_of(from_torch(mod.inner(xr).float(), "f32")))
            assert np.array_equal(model.bits_of(from_torch(fresh(xin).float(), "f32")), model.bits_of(from_torch(y.float(), "f32")))
        if form == "packed":
            P = packing.pack_indices(res.idx, 3)
            w = packing.dequantize_packed(P, K, cb, group_scales=res.S, dtype=torch.bfloat16).double().cpu().numpy()
            xr = rot.apply(x).bfloat16().double().cpu().numpy()
            bias = lin.bias.data.double().cpu().numpy()
            want = xr @ w.T + bias
            limit = (K + 1) * 2.0 ** -23 * (np.abs(xr) @ np.abs(w).T + np.abs(bias))
            err = np.abs(mod(x).double().cpu().numpy() - want)
            print(f"rotated packed layer M = {M}: max err / bound = {(err / limit).max():.3e}")
            assert (err <= limit).all()
    assert tuple(mod(x[0]).shape) == (N,)
    # .half() / .bfloat16() cast the signs like every float buffer; the transform still reads n float32 of +-1
    import copy

    for cast, dtype in (("half", torch.float16), ("bfloat16", torch.bfloat16)):
        low = getattr(copy.deepcopy(mod), cast)()
        assert low.signs.dtype == dtype and low.rotation.signs.dtype == torch.float32 and torch.equal(low.rotation.signs, rot.signs)
        xl = x.to(dtype)
        assert np.array_equal(model.bits_of(from_torch(low(xl).float(), "f32")), model.bits_of(from_torch(low.inner(rot.apply(xl)).float(), "f32")))
        assert np.array_equal(model.bits_of(from_torch(low.rotation.apply(xl).float(), "f32")), model.bits_of(from_torch(rot.apply(xl).float(), "f32")))
    with pytest.raises(ValueError):  # signs that are no float tensor never reach the kernel
        Rotation._of(torch.ones(K, dtype=torch.int32, device="cuda"), 2)
    with pytest.raises(ValueError):
        RotatedLinear.from_result(lin, sleekit_on(layer3)[1].quantize_packed(3), cb)  # no rotation on the result
    with pytest.raises(ValueError):
        RotatedLinear(mod.inner, Rotation(128))


# ---------------------------------------------------------------------------------------------------------------- 6. what it is for
def test_rotation_lowers_the_layer_error(layer3):
    """The mean layer error (W - W^) H (W - W^)^T in the original basis, with and without the rotation.  The float64 reference
    gives rotated / plain = 0.39 for the 3-bit per-row "mse" recipe (0.02615 -> 0.01019, block 256) and 0.40 for MXFP4 with
    "mse" scales (0.008368 -> 0.003353, block 128) on these inputs and signs; the cap 0.6 leaves room for the float32 rotation
    of W on the device."""
    from sleekit_amd import Rotation, obq

    W, H = torch.from_numpy(np.array(layer3["W"])).cuda(), torch.from_numpy(np.array(layer3["H"])).cuda()
    errors = {}
    for name, rot in (("3-bit", Rotation(256, seed=3)), ("mxfp4", Rotation(256, block=128, seed=3))):
        for rotated in (False, True):
            if name == "3-bit":
                lin, st = sleekit_on(layer3)
                st.quantize(3, scaling_mode="mse", rotation=rot if rotated else None)
            else:  # (quantize_mxfp4 keeps its parameter list: the object's rotation)
                lin, st = sleekit_on(layer3, rotation=rot if rotated else None)
                st.quantize_mxfp4(scale_mode="mse")
            errors[name, rotated] = float(obq.quantization_error(W, lin.weight.data, H))
    print("mean layer error, plain -> rotated: " + "; ".join(f"{n} {errors[n, False]:.4g} -> {errors[n, True]:.4g} "
                                                           f"(ratio {errors[n, True] / errors[n, False]:.3f})" for n in ("3-bit", "mxfp4")))
    for name in ("3-bit", "mxfp4"):
        assert errors[name, True] <= 0.6 * errors[name, False], (name, errors)
