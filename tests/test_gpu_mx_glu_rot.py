"""The fused gate/up product in front of a rotated down layer on the MI355X (matmul_mx_glu(rotation=); slk_mx_gemm_glu_rot,
slk_mx_gemm_glu_experts_rot): the epilogue rotates each MX block of h before it quantizes it, and its codes and scale bytes
are those of the public three steps -- matmul_mx to float32, glu to float32, Rotation.apply to float32 and the format's
quantizer -- and of the composed NumPy model (tests/mx_glu_rot_model.py) on exact integer data.

The shapes (M, N hidden columns, K) are tests/test_gpu_mx_glu.py's, the ones that split the forms: (1, 32, 32) the minimum;
(17, 96, 160) and (64, 160, 2080) the few-rows form, ragged and at its last M; (65, 96, 160) and (130, 160, 2080) the
many-rows form with a 64-column tile of one live block.  The blocks 2 .. 32 each switch on another stage: 2, 4, 8 stay in a
lane's registers (for E2M3, which holds 16 elements a lane, 16 as well), 16 crosses lane distance 1 and 32 lane distance 2
(for E2M3: 32 crosses distance 1).  Every block and every format pair meets every shape; the layout, the bias and the gate's
parameters take turns over the blocks so that each (shape, pair) sees both layouts, with and without bias.

Every comparison is equality of bits."""

import numpy as np
import pytest
import torch

import mx6_model
import mx_experts_model
import mx_gemm_model
import mx_glu_model
import mx_glu_rot_model as model
from test_gpu_mx_experts import ENCODE, PAIRS, W4, W6, bits, block_gaussian, random_experts
from test_gpu_mx_glu import BITS, SHAPES, guarded, layer, quantizer, same

pytestmark = pytest.mark.gpu

BLOCKS = (2, 4, 8, 16, 32)
# (gate, interleaved, bias) of the i-th block: both layouts, bias and none, both gates within any five
TURNS = [("gpt-oss", True, True), ("swiglu", False, False), ("gpt-oss", False, True), ("swiglu", True, False), ("gpt-oss", True, False)]
GATES = {"swiglu": mx_glu_model.SWIGLU, "gpt-oss": mx_glu_model.GPT_OSS}


def gaussian_operands(mx, rng, M, N, K, activations, weights):
    a_codes, a_scales = quantizer(mx, activations)(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t[0]).cuda() for t in random_experts(rng, 1, 2 * N, K, 118, 123, weights))
    bias = torch.from_numpy(rng.standard_normal(2 * N).astype(np.float32)).cuda()
    return a_codes, a_scales, codes, scales, bias


def three_steps(mx, rot, a_codes, a_scales, codes, scales, bias, activations, weights, interleaved, gate):
    """The parent's route, in public calls: the product to float32, the gate to float32, the rotation to float32, the quantizer."""
    y = mx.matmul_mx(a_codes, a_scales, codes, scales, bias, dtype=torch.float32, activations=activations, weights=weights)
    h = mx.glu(y, interleaved=interleaved, dtype=torch.float32, **gate)
    return quantizer(mx, activations)(rot.apply(h, dtype=torch.float32)), h


# ---------------------------------------------------------------------------------------------------------------- 1. the parent's route
@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_equals_the_public_three_steps(shape, activations, weights):
    """Block-Gaussian data, every block: codes and scale bytes of matmul_mx_glu(rotation=) are those of the three public steps,
    the flag stays 0, and a repeated call gives the same bits."""
    from sleekit_amd import mx, rotation

    M, N, K = shape
    rng = np.random.default_rng(31 + 1000 * M + N + K + len(activations) + 3 * len(weights))
    a_codes, a_scales, codes, scales, bias = gaussian_operands(mx, rng, M, N, K, activations, weights)
    kw = dict(activations=activations, weights=weights)
    seen = set()
    for block, (name, interleaved, with_bias) in zip(BLOCKS, TURNS):
        rot, b = rotation.Rotation(N, block=block, seed=block + M), bias if with_bias else None
        want, h = three_steps(mx, rot, a_codes, a_scales, codes, scales, b, activations, weights, interleaved, GATES[name])
        assert bool(torch.isfinite(h).all())
        hc, hs, flag = mx._matmul_mx_glu(a_codes, a_scales, codes, scales, b, interleaved=interleaved, rotation=rot, **kw, **GATES[name])
        what = f"{shape} {activations} x {weights} block {block} {name} interleaved {interleaved} bias {with_bias}"
        assert tuple(hc.shape) == (M, N * BITS[activations] // 8) and tuple(hs.shape) == (M, N // 32)
        same((hc, hs), want, what)
        assert int(flag.item()) == 0
        again = mx.matmul_mx_glu(a_codes, a_scales, codes, scales, b, interleaved=interleaved, rotation=rot, **kw, **GATES[name])
        same(again, (hc, hs), "a repeated call: " + what)
        plain = mx.matmul_mx_glu(a_codes, a_scales, codes, scales, b, interleaved=interleaved, **kw, **GATES[name])
        assert not torch.equal(plain[0], hc)   # (the rotation reaches the codes)
        seen.add(hc.cpu().numpy().tobytes())
    assert len(seen) == len(BLOCKS)


@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integers_against_the_composed_model(shape, activations, weights):
    """The inputs of tests/test_gpu_mx_glu.py's exact test (integer activations in +-4 under scale bytes 126 .. 128, weights
    under the same, a bias in eighths, alpha = 0: every sum exact in float32 in any order, the gate without a transcendental)
    against mx_glu_rot_model: the float32 additions of the butterflies are NumPy's, each rounded once, in the contract's order."""
    from sleekit_amd import mx, rotation

    M, N, K = shape
    rng = np.random.default_rng(1000 * M + 7 * N + K + len(activations) + 3 * len(weights))
    a_codes = ENCODE[activations](rng.integers(-4, 5, (M, K)).astype(np.float64))
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    codes, scales = (t[0] for t in random_experts(rng, 1, 2 * N, K, 126, 128, weights))
    bias = (rng.integers(-64, 65, 2 * N) / 8.0).astype(np.float32)
    A = mx_experts_model.DEQUANTIZE_ACT[activations](a_codes, a_scales)
    Wmax = np.abs(mx6_model.dequantize_model(codes, scales) if weights == W6 else mx_gemm_model.weights_model(codes, scales)).max()
    q = 2.0 ** -3 if weights == W4 else 2.0 ** -5
    assert np.abs(A).max() <= 8 and (A * 2 == np.rint(A * 2)).all() and Wmax <= (12 if weights == W4 else 15)
    assert K * 8 * Wmax + 8 < 2 ** 24 * q and (weights != W4 or K * 96 + 8 < 2 ** 21)
    sums = mx_glu_model.sums_model(a_codes, a_scales, codes, scales, activations, weights)
    dev = tuple(torch.from_numpy(t).cuda() for t in (a_codes, a_scales, codes, scales))
    bias_d = torch.from_numpy(bias).cuda()
    for i, block in enumerate(BLOCKS):
        interleaved, with_bias = bool(i & 1), i % 3 != 1
        gate = dict(alpha=0.0, limit=3.0 if i < 3 else None, shift=float(i & 1), interleaved=interleaved)
        rot = rotation.Rotation(N, block=block, seed=7 * block + M)
        want = model.hidden_rot_model(sums, bias if with_bias else None, activations, block, rot.signs.cpu().numpy(), **gate)
        got = mx.matmul_mx_glu(*dev, bias_d if with_bias else None, activations=activations, weights=weights, rotation=rot, **gate)
        same(got, want, f"{shape} {activations} x {weights} block {block} {gate} bias {with_bias}")


# ---------------------------------------------------------------------------------------------------------------- 2. the route
@pytest.mark.parametrize("activations,weights", [PAIRS[0], PAIRS[1], PAIRS[4]])
@pytest.mark.parametrize("M", [17, 65])
def test_a_block_of_32_stays_fused(M, activations, weights, monkeypatch):
    """With the elementwise gate made to raise, gated_mlp_mx behind a down rotation of block 32 still returns -- nothing takes
    the three-step route -- and its bits are those of the run without the patch and of fused=False; a block of 64 (N = 192)
    needs the three steps and raises."""
    from sleekit_amd import mx, rotation

    K, Nd = 160, 48
    rng = np.random.default_rng(M + len(activations))
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    kw = dict(activations=activations, weights=weights, interleaved=True, **mx_glu_model.GPT_OSS)
    runs = {}
    for N, block in ((96, 32), (192, 64)):
        (uc, us, ub), (dc, ds, db) = layer(rng, 2 * N, K, weights), layer(rng, Nd, N, weights)
        rot = rotation.Rotation(N, block=block, seed=4)
        runs[block] = lambda fused=True, a=(x, uc, us, dc, ds, ub, db), rot=rot: mx.gated_mlp_mx(*a, down_rotation=rot, fused=fused, **kw)
    want, want64 = runs[32](), runs[64]()
    assert np.array_equal(bits(want), bits(runs[32](fused=False))) and np.array_equal(bits(want64), bits(runs[64](fused=False)))

    def no_glu(*args, **kwargs):
        raise AssertionError("the three-step route was taken")

    monkeypatch.setattr(mx, "_glu", no_glu)
    got = runs[32]()
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(AssertionError, match="three-step route"):
        runs[64]()
    with pytest.raises(AssertionError, match="three-step route"):
        runs[32](fused=False)


# ---------------------------------------------------------------------------------------------------------------- 3. isolation
@pytest.mark.parametrize("activations", ["mxfp8", "mxfp4", "mxfp6_e2m3"])
@pytest.mark.parametrize("M,block", [(17, 32), (65, 32), (17, 8), (65, 4), (65, 16)])
def test_an_outlier_stays_in_its_own_block(M, block, activations):
    """An up bias of 2^60 on one hidden column makes that column of h huge and finite in every row.  Every other MX block of
    every row keeps its codes and its scale byte.  In the rows where the outlier is at least 2^52 (silu(gate) at least 2^-8:
    most rows) its own MX block takes a scale byte at least 16 above the unplanted one, every element of its Hadamard block
    is non-zero, and, for a Hadamard block below 32, the rest of its MX block is zeros: those elements are the unplanted
    rotation's, below 2^20, under a scale of at least 2^49.5 / 448 > 2^40, and the finest grid (E4M3) sends what is below
    2^-10 of the scale to zero -- had the outlier leaked past its Hadamard block they would be of its size."""
    from sleekit_amd import mx, rotation

    N, K, j = 96, 160, 41   # column 41: MX block 1, element 9
    rng = np.random.default_rng(5 * M + block)
    a_codes, a_scales, codes, scales, bias = gaussian_operands(mx, rng, M, N, K, activations, W4)
    rot = rotation.Rotation(N, block=block, seed=2)
    kw = dict(activations=activations, weights=W4)
    base = mx.matmul_mx_glu(a_codes, a_scales, codes, scales, bias, rotation=rot, **kw)   # (SwiGLU: no clamp on the outlier)
    planted = bias.clone()
    planted[N + j] = 2.0 ** 60   # (not interleaved: the up row of hidden column j)
    got = mx.matmul_mx_glu(a_codes, a_scales, codes, scales, planted, rotation=rot, **kw)
    per, own = 32 * BITS[activations] // 8, j // 32   # bytes of codes an MX block; the outlier's MX block
    gc, bc = (t[0].cpu().numpy().reshape(M, N // 32, per) for t in (got, base))
    gs, bs = (t[1].cpu().numpy() for t in (got, base))
    others = [b for b in range(N // 32) if b != own]
    assert np.array_equal(gc[:, others], bc[:, others]) and np.array_equal(gs[:, others], bs[:, others])
    # which rows carry a large outlier, and how large the unplanted rotated h is: from the elementwise route
    h0 = mx.glu(mx.matmul_mx(a_codes, a_scales, codes, scales, bias, **kw), dtype=torch.float32)
    h1 = mx.glu(mx.matmul_mx(a_codes, a_scales, codes, scales, planted, **kw), dtype=torch.float32)
    assert bool(torch.isfinite(h1).all()) and float(rot.apply(h0, dtype=torch.float32).abs().max()) < 2.0 ** 20
    rows = (h1[:, j].abs() >= 2.0 ** 52).cpu().numpy()
    assert rows.sum() >= M // 2
    assert (gs[rows, own].astype(int) >= bs[rows, own].astype(int) + 16).all()
    values = mx_experts_model.DEQUANTIZE_ACT[activations](got[0].cpu().numpy(), got[1].cpu().numpy())[rows, 32 * own:32 * own + 32]
    inside = np.zeros(32, bool)
    inside[(j % 32) // block * block:(j % 32) // block * block + block] = True
    assert (np.abs(values[:, inside]) > 0).all() and (values[:, ~inside] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4. non-finite
@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_non_finite_raises_the_flag(shape, activations, weights):
    """Activation scale bytes of 254 against weight scale bytes of 254: the sums overflow.  The flag is raised, as the rotating
    quantizer's on the elementwise route's h, and the public call raises (the outputs are then not meaningful, the quantizers'
    rule: the butterflies turn infinities into NaNs whose sign no contract fixes); with finite data the flag stays 0 and codes
    and scale bytes are that route's."""
    from sleekit_amd import mx, rotation

    M, N, K = shape
    rng = np.random.default_rng(M + N)
    a_codes, a_scales, codes, scales, _ = gaussian_operands(mx, rng, M, N, K, activations, weights)
    rot = rotation.Rotation(N, block=32 if M < 65 else 16, seed=1)
    kw = dict(activations=activations, weights=weights, **mx_glu_model.GPT_OSS)
    for big, raised in ((True, 1), (False, 0)):
        asc, wsc = (torch.full_like(a_scales, 254), torch.full_like(scales, 254)) if big else (a_scales, scales)
        hc, hs, flag = mx._matmul_mx_glu(a_codes, asc, codes, wsc, None, interleaved=True, rotation=rot, **kw)
        h = mx.glu(mx.matmul_mx(a_codes, asc, codes, wsc, activations=activations, weights=weights), interleaved=True, dtype=torch.float32,
                   **mx_glu_model.GPT_OSS)
        assert bool(torch.isfinite(h).all()) != big
        wc, ws, wflag = mx._rotate_quantize_act(h, M, N, rot, mx._FORMATS[activations])
        assert int(flag.item()) == raised == int(wflag.item())
        if not big:
            same((hc, hs), (wc, ws), f"{shape} {activations} x {weights}")
        else:
            with pytest.raises(ValueError, match="finite"):
                mx.matmul_mx_glu(a_codes, asc, codes, wsc, interleaved=True, rotation=rot, **kw)


# ---------------------------------------------------------------------------------------------------------------- 5, 6. the C entry
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_null_signs_and_nothing_written_past_the_outputs(case):
    """The C entry on h_codes and h_scales of exactly their sizes with 256 sentinel bytes behind each, at every shape (the
    pair and the block take turns): the guards are unchanged; signs = NULL gives the bits of N signs of +1, which are the three
    steps' under Rotation.from_signs of the same; and the public call's signs give the public call's bits."""
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, mx, rotation

    (M, N, K), (activations, weights), block = SHAPES[case], PAIRS[case], BLOCKS[::-1][case]
    rng = np.random.default_rng(3 * M + N)
    a_codes, a_scales, codes, scales, bias = gaussian_operands(mx, rng, M, N, K, activations, weights)
    fmt, wf = mx._FORMATS[activations], mx._WEIGHTS[weights]
    nc, ns = M * N * fmt.bits // 8, M * N // 32
    a_codes, codes = dev.aligned(a_codes), dev.aligned(codes)
    rot = rotation.Rotation(N, block=block, seed=6)
    ones = torch.ones(N, dtype=torch.float32, device="cuda")
    out = []
    for signs in (None, ones, rot.signs):
        hc, hs, flag = guarded(nc), guarded(ns), torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib.slk_mx_gemm_glu_rot(dev.ptr(a_codes), dev.ptr(a_scales), dev.ptr(codes), dev.ptr(scales), dev.ptr(bias), M, N, K, fmt.c_fmt,
                                                wf.c_fmt, 1.702, 7.0, 1.0, 0, dev.ptr(hc), dev.ptr(hs), dev.ptr(flag), block,
                                                None if signs is None else dev.ptr(dev.aligned(signs)), dev.stream_handle()))
        assert (hc[nc:] == 0xA5).all() and (hs[ns:] == 0xA5).all() and int(flag.item()) == 0
        out.append((hc[:nc].reshape(M, -1), hs[:ns].reshape(M, -1)))
    what = f"{SHAPES[case]} {activations} x {weights} block {block}"
    same(out[0], out[1], "NULL signs against signs of +1: " + what)
    kw = dict(activations=activations, weights=weights, **mx_glu_model.GPT_OSS)
    same(out[2], mx.matmul_mx_glu(a_codes, a_scales, codes, scales, bias, rotation=rot, **kw), what)
    assert not torch.equal(out[0][0], out[2][0])
    # all +1: the transform without step 1
    y = mx.matmul_mx(a_codes, a_scales, codes, scales, bias, dtype=torch.float32, activations=activations, weights=weights)
    h = mx.glu(y, dtype=torch.float32, **mx_glu_model.GPT_OSS)
    plus = rotation.Rotation.from_signs(ones, block)
    same(out[0], quantizer(mx, activations)(plus.apply(h, dtype=torch.float32)), "signs of +1 against the three steps: " + what)


# ---------------------------------------------------------------------------------------------------------------- 7. experts
EXPERT_COUNTS = [(0, 1, 17, 65), (15, 64, 0, 130), (16, 17, 63, 0)]


@pytest.mark.parametrize("case", range(len(PAIRS)))
def test_experts_equal_the_dense_rotated_call_on_every_slice(case):
    """E = 4 with an empty expert and row counts on both sides of 16 and of 64, one rotation shared by all experts: each
    expert's rows are matmul_mx_glu(rotation=) of that slice, and the whole is the three-step route over experts."""
    from sleekit_amd import mx, rotation

    (activations, weights), counts, block = PAIRS[case], EXPERT_COUNTS[case % 3], BLOCKS[::-1][case]
    N, K, E, M = 96, 160, len(counts), sum(counts)
    rng = np.random.default_rng(600 + case)
    a_codes, a_scales = quantizer(mx, activations)(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t).cuda() for t in random_experts(rng, E, 2 * N, K, 118, 123, weights))
    bias = torch.from_numpy(rng.standard_normal((E, 2 * N)).astype(np.float32)).cuda()
    offsets = mx_experts_model.offsets_of(counts)
    offsets_d = torch.from_numpy(offsets).cuda()
    rot = rotation.Rotation(N, block=block, seed=13)
    kw = dict(activations=activations, weights=weights)
    for gate, interleaved, b in ((mx_glu_model.GPT_OSS, True, bias), (mx_glu_model.SWIGLU, False, None)):
        hc, hs = mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets_d, b, interleaved=interleaved, rotation=rot, **kw, **gate)
        assert tuple(hc.shape) == (M, N * BITS[activations] // 8) and tuple(hs.shape) == (M, N // 32)
        for e in range(E):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            if hi > lo:
                alone = mx.matmul_mx_glu(a_codes[lo:hi], a_scales[lo:hi], codes[e], scales[e], None if b is None else b[e], interleaved=interleaved,
                                         rotation=rot, **kw, **gate)
                same((hc[lo:hi], hs[lo:hi]), alone, f"expert {e} of {counts}, rows {lo} .. {hi - 1}, block {block}")
        unfused = mx._matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets_d, b, activations, weights, interleaved=interleaved, fused=False,
                                            rotation=rot, **gate)
        same((hc, hs), unfused[:2], "the three-step route over experts")
        assert int(unfused[2].item()) == 0 and int(unfused[3].item()) == 0
        same(mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets_d, b, interleaved=interleaved, rotation=rot, **kw, **gate), (hc, hs),
             "a repeated call")


@pytest.mark.parametrize("offsets", [[0, 40, 30, 83], [1, 30, 83], [0, 30, 82], [0, 30, 84]])
def test_invalid_offsets_raise_flag_0_and_write_nothing(offsets):
    """Decreasing, first not 0, last not M: flag[0] is raised, flag[1] is not, and sentinel-filled outputs keep every byte."""
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, mx, rotation

    M, N, K, E = 83, 96, 160, len(offsets) - 1
    rng = np.random.default_rng(9)
    a_codes, a_scales = mx.quantize_mxfp8(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t).cuda() for t in random_experts(rng, E, 2 * N, K, 118, 123, W4))
    bad = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    rot = rotation.Rotation(N, block=32, seed=3)
    with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
        mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, bad, rotation=rot)
    hc, hs, flags = guarded(M * N, 0x5A), guarded(M * N // 32, 0x5A), torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = _lib.lib.slk_mx_experts_workspace_bytes(E, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a_codes, codes, signs = dev.aligned(a_codes), dev.aligned(codes), dev.aligned(rot.signs)
    _lib.check(_lib.lib.slk_mx_gemm_glu_experts_rot(dev.ptr(a_codes), dev.ptr(a_scales), dev.ptr(codes), dev.ptr(scales), None, dev.ptr(bad), E, M, N, K,
                                                    _lib.MX_ACT_FP8, _lib.MX_W_FP4, 1.0, float("inf"), 0.0, 0, dev.ptr(hc), dev.ptr(hs), dev.ptr(flags),
                                                    dev.ptr(ws), nbytes, 32, dev.ptr(signs), dev.stream_handle()))
    assert flags.tolist() == [1, 0] and (hc == 0x5A).all() and (hs == 0x5A).all()
    good = torch.tensor([0] * E + [M], dtype=torch.int32, device="cuda")   # and the next call is not held up by the last flag
    got = mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, good, rotation=rot)
    same(got, mx.matmul_mx_glu(a_codes, a_scales, codes[E - 1], scales[E - 1], rotation=rot), "all rows of the last expert")


@pytest.mark.parametrize("activations", ["mxfp8", "mxfp4", "mxfp6_e2m3"])
def test_forward_tokens_behind_a_down_rotation(activations, monkeypatch):
    """T = 40 tokens, k = 2 of E = 4 experts (expert 3 unused, the others with 9, 71 rows and none): forward_tokens with a
    down rotation of block 32 equals its fused=False run, forward on the sorted rows equals its own, and the fused run never
    calls the elementwise gate."""
    from sleekit_amd import mx, rotation

    T, k, E, N, K, Nd = 40, 2, 4, 96, 160, 48
    rng = np.random.default_rng(12)
    x = torch.from_numpy(block_gaussian(rng, T, K)).cuda()
    ids = np.zeros((T, k), np.int64)
    ids[:, 0], ids[:, 1] = 1, 1
    ids[:9, 0] = 0
    ids = torch.from_numpy(ids).cuda()
    gates = torch.from_numpy(rng.random((T, k)).astype(np.float32)).cuda()
    up, down = mx.MXExperts(E, K, 2 * N, activations=activations).cuda(), mx.MXExperts(E, N, Nd, activations=activations).cuda()
    for mod, rows, cols in ((up, 2 * N, K), (down, Nd, N)):
        c, s = random_experts(rng, E, rows, cols, 118, 123, W4)
        mod.codes.copy_(torch.from_numpy(c)), mod.scales.copy_(torch.from_numpy(s)), mod.bias.copy_(torch.from_numpy(rng.standard_normal((E, rows)).astype(np.float32)))
    mlp = mx.MXExpertsMLP(up, down, interleaved=True, **mx_glu_model.GPT_OSS)
    rot = rotation.Rotation(N, block=32, seed=21)
    want = mlp.forward_tokens(x, ids, gates, fused=False, down_rotation=rot)
    order, offsets = mx.sort_by_expert(ids, E)
    assert offsets.tolist() == [0, 9, 80, 80, 80]
    want_rows = mlp(x[order // k], offsets, fused=False, down_rotation=rot)
    assert not np.array_equal(bits(want), bits(mlp.forward_tokens(x, ids, gates)))

    def no_glu(*args, **kwargs):
        raise AssertionError("the three-step route was taken")

    monkeypatch.setattr(mx, "_glu", no_glu)
    got = mlp.forward_tokens(x, ids, gates, down_rotation=rot)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, Nd)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(mlp(x[order // k], offsets, down_rotation=rot)), bits(want_rows))
