"""The packed-index linear layer on the MI355X: the MFMA operand map with identity activations bit for bit, exact integer
products bit for bit, random data within a derived bound against the float64 model, operand equality with
dequantize_packed through the public surface, the module end to end, and repeated calls.

Sizes the shapes were chosen from: up to T = 16 rows of x a workgroup is one 16-column tile of Y
whose 8 waves take units of 4 chunks (128 columns of K) in turn, 1024 columns a pass; above, a workgroup is a 64 x 64
tile of Y and a K-step is 64 columns (two chunks).  The weights come from a per-(row, group) table where the codebook has
at most 64 entries and either there are no group scales, or g is a multiple of 32 (few rows) / 64 (tiles) with
2 * levels <= g; otherwise each element is de-quantized directly.  The shapes below take both forms in both kernels.

The one tolerance of this file is `bound`: |y - y64| <= adds * 2^-23 * sum_k |x_k w_k|, the first-order worst case of
`adds` float32 additions in any order, rounded or truncated (the products are exact in float32: 8 + 8 or 11 + 11
significant bits); adds is K, or K + 1 with a bias.  A misplaced element costs about sum |x w| / sqrt(K), far above it.
Largest |err| / sum |x w| seen on the MI355X: see DESIGN.md section 14.

The identity test's group scales are powers of two that differ between neighbouring rows and groups, 2^((7 n + 3 k) % 15 -
6), that is 2^-6 .. 2^8: with values of magnitude up to 128 and offsets up to 3 every weight is finite in float16 (at most
32771) and none is a 16-bit subnormal (at least 2^-6 where it is not zero), so 0 * w stays 0; a (33, 13) grid has more cells
than that range has powers of two, so they cannot all differ.
"""

import numpy as np
import pytest
import torch

import packed_gemm_model as model
from packing_model import codebook_values, dequantize_model, pack_model

pytestmark = pytest.mark.gpu

T = 16  # the few-rows kernel's largest M
COMPUTE = [torch.bfloat16, torch.float16]


def bits_of(x):
    if isinstance(x, torch.Tensor):  # (NumPy has no bfloat16: the bits leave torch as integers)
        x = x.contiguous().view({2: torch.int16, 4: torch.int32}[x.element_size()]).cpu().numpy()
    x = np.asarray(x)
    return np.ascontiguousarray(x).view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def bound(adds, sum_abs):
    return adds * 2.0 ** -23 * sum_abs


def values_of(cb):
    from sleekit_amd.codebook import UniformCodebook

    if isinstance(cb, UniformCodebook):
        return codebook_values(len(cb), cb.min_val, cb.max_val)
    return np.asarray(cb.values, np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. map
@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("b", range(1, 9))
def test_operand_map_identity(b, compute):
    """X = rows of the identity times a power of two: Y is those columns of Wc exactly -- one product a sum, and the zeros
    stay zeros.  Every (row, group of 8) has its own scale and offset and neighbouring indices differ, so a neighbour's
    scale, offset, index or quarter changes the answer."""
    from sleekit_amd import packing
    from sleekit_amd.codebook import Codebook

    levels = 1 << b
    cb = Codebook(np.arange(levels, dtype=np.float32) - levels // 2)  # distinct, exact in both compute types
    for K in (64, 104):
        for N in (16, 33):
            n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
            P = pack_model(((7 * n + 3 * k) % levels).astype(np.uint8), b)
            ng, kg = np.meshgrid(np.arange(N), np.arange(K // 8), indexing="ij")
            S = (2.0 ** ((7 * ng + 3 * kg) % 15 - 6)).astype(np.float32)
            O = ((ng + 2 * kg) % 7 - 3).astype(np.float32)
            Wc, _ = model.weights_model(P, K, b, values_of(cb), compute, group_scales=S, offsets=O)
            assert np.isfinite(Wc).all() and (np.abs(Wc[Wc != 0]) >= 2.0 ** -14).all()
            want = (4.0 * Wc.T).astype(np.float32)  # (K, N): row m of Y is column m of Wc, times 4
            X = torch.eye(K, dtype=compute, device="cuda") * 4
            dev_args = dict(group_scales=torch.from_numpy(S).cuda(), offsets=torch.from_numpy(O).cuda(), dtype=torch.float32)
            Pd = torch.from_numpy(P.view(np.int32)).cuda()
            calls = [(m0, min(m0 + 16, K)) for m0 in range(0, K, 16)] + ([(0, K)] if K > T else [])
            for m0, m1 in calls:
                got = packing.linear_packed(X[m0:m1], Pd, cb, **dev_args).cpu().numpy()
                assert got.shape == (m1 - m0, N) and got.dtype == np.float32
                wrong = np.argwhere(bits_of(got) != bits_of(want[m0:m1]))
                if wrong.size:
                    m, col = wrong[0]
                    read = np.flatnonzero(want[:, col] == got[m, col]).tolist()
                    raise AssertionError(f"b = {b}, K = {K}, N = {N}, rows {m0}:{m1}: {len(wrong)} differ, first y[{m0 + m}][{col}] = "
                                         f"{got[m, col]!r}, want 4 W[{col}][{m0 + m}] = {want[m0 + m, col]!r}; it is 4 W[{col}][k] for k in {read[:6]}")


# ---------------------------------------------------------------------------------------------------------------- 2. exact
# (M, N, K, kind, codebook, group size, x dtype); kinds: 0 none, 1 per row, 2 group scales, 3 group scales and offsets.
# codebooks: "t" the table -4 .. 3, "u" UniformCodebook(8, -3.5, 3.5), "c" five levels at 3 bits with stored indices up to
# 7 (the clamp), "w" the table at 4-bit storage (bits above index_bits).  The two last shapes are this file's own: group
# scales from a table in the tile kernel (g % 64 == 0) and in the few-rows kernel with two groups a unit.
EXACT = [(1, 1, 8, 3, "t", 8, "f32"), (1, 16, 128, 2, "u", 32, "bf16"), (16, 1, 96, 1, "t", None, "f16"), (17, 33, 160, 3, "u", 32, "f32"),
         (15, 47, 4128, 2, "t", 96, "f16"), (T, 17, 160, 0, "u", None, "bf16"), (T + 1, 17, 160, 1, "c", None, "f32"),
         (130, 200, 544, 3, "w", 32, "bf16"), (33, 16, 2080, 0, "t", None, "f16"), (3, 5, 40, 3, "c", 8, "f32"),
         (65, 40, 256, 3, "t", 64, "bf16"), (16, 40, 256, 2, "u", 64, "f32")]
X_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("M,N,K,kind,cbk,g,xd", EXACT)
def test_exact_integers_bit_for_bit(M, N, K, kind, cbk, g, xd, compute):
    from sleekit_amd import packing
    from sleekit_amd.codebook import Codebook, UniformCodebook

    rng = np.random.default_rng(M * 1000 + N * 7 + K)
    cb = {"t": Codebook(np.arange(-4.0, 4.0)), "w": Codebook(np.arange(-4.0, 4.0)), "u": UniformCodebook(8, -3.5, 3.5),
          "c": Codebook(np.arange(-2.0, 3.0))}[cbk]
    bits = 4 if cbk == "w" else 3
    idx = rng.integers(0, 8, (N, K)).astype(np.uint8)  # ("c": indices 5 .. 7 are clamped to the last value)
    P = pack_model(idx, bits)
    G = K // g if g else 0
    scale = rng.choice([0.5, 1.0, 2.0], N).astype(np.float32) if kind == 1 else None
    S = rng.choice([0.5, 1.0, 2.0], (N, G)).astype(np.float32) if kind >= 2 else None
    O = rng.integers(-2, 3, (N, G)).astype(np.float32) if kind == 3 else None
    x = torch.from_numpy(rng.integers(-4, 5, (M, K)).astype(np.float32)).to(X_DTYPES[xd])
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32) if (M + N) % 2 else None
    # the test's own inputs make every order of float32 additions exact: the weights are multiples of 1/4 of magnitude at
    # most 10 that the compute type holds exactly, so all terms (and the bias) are multiples of q = 2^-3 of magnitude at
    # most 40, and every partial sum is a multiple of q below 2^24 q
    Wc, W32 = model.weights_model(P, K, bits, values_of(cb), compute, scale, S, O)
    assert np.array_equal(Wc, W32.astype(np.float64)) and np.abs(Wc).max() <= 10 and (Wc * 4 == np.rint(Wc * 4)).all()
    assert K * 40 + 8 < 2 ** 24 * 2.0 ** -3
    want, _ = model.linear_model(x, P, K, bits, values_of(cb), compute, scale, S, O, bias)
    got = packing.linear_packed(x.cuda(), torch.from_numpy(P.view(np.int32)).cuda(), cb, bits, scale, S, g if kind >= 2 else None, O, bias,
                                dtype=torch.float32, compute=compute).cpu().numpy()
    assert got.shape == (M, N) and got.dtype == np.float32
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}"
    assert np.array_equal(bits_of(got), bits_of(want.astype(np.float32)))


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("M,N,K,kind,bits", [(16, 17, 160, 0, 7), (16, 17, 160, 1, 8), (33, 17, 160, 0, 8), (33, 17, 104, 1, 7)])
def test_exact_wide_codebook_direct_bit_for_bit(M, N, K, kind, bits, compute):
    """A codebook above 64 entries is de-quantized element by element in both kernels; without group scales (none, or
    per row) that form is met nowhere else.  The table is k / 16, k = -2^(b-1) .. 2^(b-1) - 1: at most 8 significant bits,
    exact in both compute types, as are its products with the scales 0.5, 1, 2.  All terms (and the bias) are multiples of
    q = 2^-5 of magnitude at most 16 * 4, so every partial sum is a multiple of q below 2^24 q and any order is exact."""
    from sleekit_amd import packing
    from sleekit_amd.codebook import Codebook

    rng = np.random.default_rng(M + 10 * K + bits)
    levels = 1 << bits
    cb = Codebook((np.arange(levels) - levels // 2) / 16.0)
    P = pack_model(rng.integers(0, levels, (N, K)).astype(np.uint8), bits)
    scale = rng.choice([0.5, 1.0, 2.0], N).astype(np.float32) if kind == 1 else None
    x = torch.from_numpy(rng.integers(-4, 5, (M, K)).astype(np.float32))
    bias = (rng.integers(-64, 65, N) / 8.0).astype(np.float32)
    Wc, W32 = model.weights_model(P, K, bits, values_of(cb), compute, scale)
    assert np.array_equal(Wc, W32.astype(np.float64)) and np.abs(Wc).max() <= 16 and (Wc * 32 == np.rint(Wc * 32)).all()
    assert K * 64 + 8 < 2 ** 24 * 2.0 ** -5
    want, _ = model.linear_model(x, P, K, bits, values_of(cb), compute, scale, bias=bias)
    got = packing.linear_packed(x.cuda(), torch.from_numpy(P.view(np.int32)).cuda(), cb, scale=scale, bias=bias, compute=compute).cpu().numpy()
    wrong = np.argwhere(got.astype(np.float64) != want)
    assert wrong.size == 0, f"{len(wrong)} of {M * N} differ, first at {wrong[:4].tolist()}: got {got[tuple(wrong[0])]}, want {want[tuple(wrong[0])]}"
    assert np.array_equal(bits_of(got), bits_of(want.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------------- 3. bound
NF4 = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
       -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]


def block_gaussian(rng, M, K):
    """Gaussian data whose blocks of 8 have magnitudes 2^-3 .. 2^3, kept off the 16-bit subnormals."""
    mag = 2.0 ** rng.integers(-3, 4, (M, K // 8))
    x = (rng.standard_normal((M, K)) * np.repeat(mag, 8, axis=1)).astype(np.float32)
    return np.where(np.abs(x) < 2.0 ** -10, np.float32(2.0 ** -10), x)


def random_layer(rng, kind, N, K):
    """(codebook, bits, P, scale, S, O, g) of test 3's three kinds of layer."""
    from sleekit_amd.codebook import Codebook, UniformCodebook

    if kind == "grouped":
        cb, g = UniformCodebook(8, -1, 1), (128 if K % 128 == 0 else 32)  # (160 and 544 are no multiples of 128)
        S = rng.uniform(0.01, 0.1, (N, K // g)).astype(np.float32)
        O = rng.uniform(-0.05, 0.05, (N, K // g)).astype(np.float32)
        P = pack_model(rng.integers(0, 8, (N, K)).astype(np.uint8), 3)
        for _ in range(100):  # an offset that all but cancels a value leaves a 16-bit subnormal: draw that group's again
            W = dequantize_model(P, K, 3, values_of(cb), group_scales=S, offsets=O)
            tiny = (np.abs(W) < 2.0 ** -10).reshape(N, K // g, g).any(axis=2)
            if not tiny.any():
                break
            O[tiny] = rng.uniform(-0.05, 0.05, int(tiny.sum())).astype(np.float32)
        return cb, 3, P, None, S, O, g
    if kind == "nf4":
        return (Codebook(NF4), 4, pack_model(rng.integers(0, 16, (N, K)).astype(np.uint8), 4), rng.uniform(0.01, 0.1, N).astype(np.float32),
                None, None, None)
    return UniformCodebook(4, -1, 1), 2, pack_model(rng.integers(0, 4, (N, K)).astype(np.uint8), 2), None, None, None, None


@pytest.mark.parametrize("compute", COMPUTE)
@pytest.mark.parametrize("kind", ["grouped", "nf4", "plain"])
@pytest.mark.parametrize("M,N,K", [(17, 33, 160), (64, 80, 1024), (8, 8, 11008), (130, 72, 544)])
def test_random_data_within_the_bound(M, N, K, kind, compute):
    from sleekit_amd import packing

    rng = np.random.default_rng(K + M)
    cb, bits, P, scale, S, O, g = random_layer(rng, kind, N, K)
    x = torch.from_numpy(block_gaussian(rng, M, K))
    if compute == torch.float16:
        x = x.half()
    bias = rng.standard_normal(N).astype(np.float32)
    Wc, _ = model.weights_model(P, K, bits, values_of(cb), compute, scale, S, O)
    assert (np.abs(Wc[Wc != 0]) >= 2.0 ** -14).all()  # no 16-bit subnormal among the weights
    want, sum_abs = model.linear_model(x, P, K, bits, values_of(cb), compute, scale, S, O)
    Pd = torch.from_numpy(P.view(np.int32)).cuda()
    got = packing.linear_packed(x.cuda(), Pd, cb, bits, scale, S, g, O, dtype=torch.float32).cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"packed_gemm {kind} {M}x{N}x{K} {compute}: max |err| / sum|xw| = {(err / sum_abs).max():.3e} (bound {K * 2.0 ** -23:.3e})")
    assert (err <= bound(K, sum_abs)).all(), (err / sum_abs).max()
    want, sum_abs = model.linear_model(x, P, K, bits, values_of(cb), compute, scale, S, O, bias)
    got = packing.linear_packed(x.cuda(), Pd, cb, bits, scale, S, g, O, bias, dtype=torch.float32).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= bound(K + 1, sum_abs)).all()


# ---------------------------------------------------------------------------------------------------------------- 4. operands
@pytest.mark.parametrize("compute", COMPUTE)
def test_operands_are_dequantize_packed(compute):
    """linear_packed on the identity returns the transposed layer dequantize_packed rebuilds in the compute type."""
    from sleekit_amd import groups, packing, synth
    from sleekit_amd.codebook import UniformCodebook

    L = synth.make_layer(48, 160, 77)
    cb, g = UniformCodebook(8, -1, 1), 32
    W, H = torch.from_numpy(L["W"]).cuda(), torch.from_numpy(L["H"]).cuda()
    O = groups.compute_group_offsets(W, g)
    S = groups.compute_group_scaling(W, cb, g, H, mode="mse", offsets=O)
    _, idx = groups.quantize_grouped_asym(W, S, O, cb, H, g, return_indices=True)
    P = packing.pack_indices(idx, 3)
    want = packing.dequantize_packed(P, 160, cb, group_scales=S, offsets=O, dtype=compute).float().T.contiguous()
    eye = torch.eye(160, dtype=compute, device="cuda")
    for rows in (slice(0, 160), slice(0, 16), slice(144, 160)):  # the tile kernel, and the few-rows kernel at both ends
        got = packing.linear_packed(eye[rows], P, cb, group_scales=S, offsets=O, dtype=torch.float32)
        assert np.array_equal(bits_of(got), bits_of(want[rows])), rows


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def quantized_module(**kw):
    import torch.nn as nn

    from sleekit_amd import PackedLinear, Sleekit
    from sleekit_amd.codebook import UniformCodebook

    torch.manual_seed(5)
    lin = nn.Linear(160, 48, bias=kw.pop("bias", True)).cuda()
    st = Sleekit(lin)
    for _ in range(3):
        st.add_batch(torch.randn(64, 160, device="cuda") + 0.3)
    nbits = kw.pop("nbits", 3)
    res = st.quantize_packed(nbits, **kw)
    cb = UniformCodebook(2 ** nbits, -1, 1)
    return lin, res, cb, PackedLinear.from_result(lin, res, cb)


def test_module_end_to_end():
    import torch.nn as nn
    import torch.nn.functional as F

    from sleekit_amd import PackedLinear, packing

    lin, res, cb, mod = quantized_module(group_size=32, offsets="mid", bias_correction=True)
    assert tuple(res.S.shape) == (48, 5) and tuple(res.O.shape) == (48, 5)
    P = packing.pack_indices(res.idx, 3)
    assert torch.equal(mod.words, P)
    # the packed layer is the quantized layer: its float32 de-quantization is the weight quantize left in the module
    assert torch.equal(packing.dequantize_packed(P, 160, cb, group_scales=res.S, offsets=res.O), lin.weight.data)
    x = torch.randn(2, 5, 160, device="cuda")
    got = mod(x)
    want = packing.linear_packed(x, P, cb, group_scales=res.S, offsets=res.O, bias=lin.bias.data)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5, 48) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    for c, xin in ((torch.bfloat16, x), (torch.bfloat16, x.bfloat16()), (torch.float16, x.half())):
        y32 = packing.linear_packed(xin, P, cb, group_scales=res.S, offsets=res.O, bias=lin.bias.data, dtype=torch.float32)
        xc, wc = xin.to(c).double().reshape(10, 160), lin.weight.data.to(c).double()
        ref = F.linear(xc, wc, lin.bias.data.double())
        limit = bound(161, (xc.abs() @ wc.abs().T + lin.bias.data.double().abs()).cpu().numpy())
        assert (np.abs((y32.reshape(10, 48).double() - ref).cpu().numpy()) <= limit).all(), c
        y = mod(xin)  # the output dtype follows x
        assert y.dtype == xin.dtype and tuple(y.shape) == (2, 5, 48) and np.array_equal(bits_of(y), bits_of(y32.to(xin.dtype)))
        for explicit in (torch.bfloat16, torch.float16):
            z = packing.linear_packed(xin, P, cb, group_scales=res.S, offsets=res.O, bias=lin.bias.data, dtype=explicit)
            assert z.dtype == explicit and np.array_equal(bits_of(z), bits_of(y32.to(explicit)))
    # compute= overrides the type that follows x
    assert torch.equal(packing.linear_packed(x.half(), P, cb, group_scales=res.S, offsets=res.O, dtype=torch.float32, compute=torch.bfloat16),
                       packing.linear_packed(x.half().bfloat16(), P, cb, group_scales=res.S, offsets=res.O, dtype=torch.float32))
    assert tuple(mod(x[0, 0]).shape) == (48,) and torch.equal(mod(x[0, 0]), got[0, 0])
    # a view that starts off a 16-byte boundary
    buf = torch.zeros(10 * 160 + 1, device="cuda")
    view = buf[1:].view(2, 5, 160)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and torch.equal(mod(view), got)
    assert sorted(mod.state_dict()) == ["bias", "group_scales", "offsets", "values", "words"]
    copy = PackedLinear(160, 48, cb, group_size=32, offsets=True).cuda()
    copy.load_state_dict(mod.state_dict())
    assert torch.equal(copy(x).view(torch.int32), got.view(torch.int32))
    nobias = PackedLinear.from_result(nn.Linear(160, 48, bias=False).cuda(), res, cb)
    assert nobias.bias is None and sorted(nobias.state_dict()) == ["group_scales", "offsets", "values", "words"]
    assert torch.equal(nobias(x), packing.linear_packed(x, P, cb, group_scales=res.S, offsets=res.O))
    with pytest.raises(ValueError):
        PackedLinear.from_result(nn.Conv1d(160, 48, 1).cuda(), res, cb)
    with pytest.raises(ValueError):
        PackedLinear.from_result(nn.Linear(128, 48).cuda(), res, cb)


def test_module_per_row_and_numpy():
    from sleekit_amd import packing

    lin, res, cb, mod = quantized_module(nbits=4)
    assert tuple(res.S.shape) == (48,) and res.O is None and sorted(mod.state_dict()) == ["bias", "scale", "values", "words"]
    P = packing.pack_indices(res.idx, 4)
    assert torch.equal(packing.dequantize_packed(P, 160, cb, scale=res.S), lin.weight.data)
    x = torch.randn(7, 160, device="cuda")
    got = mod(x)
    Pn, Sn, bn = P.cpu().numpy().view(np.uint32), res.S.cpu().numpy(), lin.bias.data.cpu().numpy()
    want, sum_abs = model.linear_model(x.cpu(), Pn, 160, 4, values_of(cb), torch.bfloat16, scale=Sn, bias=bn)
    assert (np.abs(got.double().cpu().numpy() - want) <= bound(161, sum_abs)).all()
    y = packing.linear_packed(x.cpu().numpy(), Pn, cb, scale=Sn, bias=bn)  # NumPy in, NumPy out
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and np.array_equal(bits_of(y), bits_of(got))
    h = packing.linear_packed(x.half().cpu().numpy(), Pn, cb, scale=Sn, bias=bn)
    assert isinstance(h, np.ndarray) and h.dtype == np.float16 and np.array_equal(bits_of(h), bits_of(mod(x.half())))
    # quantize_packed is quantize: the same layer, the same indices
    lin2, res2, _, _ = quantized_module(nbits=4)
    assert torch.equal(lin2.weight.data, lin.weight.data) and torch.equal(res2.idx, res.idx)


def test_quantize_packed_is_quantize():
    import torch.nn as nn

    from sleekit_amd import Sleekit

    for kw in (dict(), dict(group_size=32), dict(group_size=32, offsets="mid", bias_correction=True)):
        out = []
        for packed in (False, True):
            torch.manual_seed(9)
            lin = nn.Linear(160, 48).cuda()
            st = Sleekit(lin)
            st.add_batch(torch.randn(96, 160, device="cuda") + 0.2)
            res = (st.quantize_packed if packed else st.quantize)(3, **kw)
            out.append((lin.weight.data.clone(), lin.bias.data.clone(), res))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2].idx, out[1][2].idx), kw
        assert out[1][2].S is not None and (out[1][2].O is not None) == ("offsets" in kw)


# ---------------------------------------------------------------------------------------------------------------- 6. the rest
@pytest.mark.parametrize("M", [16, 130])
def test_repeated_calls_are_bit_equal(M):
    from sleekit_amd import packing

    from sleekit_amd.codebook import UniformCodebook

    rng = np.random.default_rng(M)
    N, K, g = 200, 4128, 96
    cb = UniformCodebook(8, -1, 1)
    P = torch.from_numpy(pack_model(rng.integers(0, 8, (N, K)).astype(np.uint8), 3).view(np.int32)).cuda()
    S = torch.from_numpy(rng.uniform(0.01, 0.1, (N, K // g)).astype(np.float32)).cuda()
    O = torch.from_numpy(rng.uniform(-0.05, 0.05, (N, K // g)).astype(np.float32)).cuda()
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    first = packing.linear_packed(x, P, cb, group_scales=S, offsets=O)
    for _ in range(3):
        assert torch.equal(packing.linear_packed(x, P, cb, group_scales=S, offsets=O).view(torch.int32), first.view(torch.int32))
