"""The gated MX MLP on the MI355X: the fused gate/up product (matmul_mx_glu; slk_mx_gemm_glu) bit for bit against the NumPy
model on exact integer data and against its own three steps on Gaussian data, the gate (glu; slk_mx_glu) against the float64
model within a derived bound, the non-finite flag, the bounds of the output buffers, the expert-grouped form against the dense
one, and the Python surface end to end.

The shapes (M, N hidden columns, K) are the smallest that reach every path: (1, 32, 32) the minimum; (17, 96, 160) the
split-K form with a ragged row tile, K no multiple of 128 and three blocks; (64, 160, 2080) that form's last M and a second
2048-column pass with a partial step; (65, 96, 160) the tiled form's first M, ragged rows and a 64-column tile with one live
block; (130, 160, 2080) the tiled form at larger M and K.

The one tolerance of this file is gate_bound (check 3); everything else is equality of bits.
"""

import numpy as np
import pytest
import torch

import mx6_model
import mx_experts_model
import mx_gemm_model
import mx_glu_model as model
from test_gpu_mx_experts import ENCODE, PAIRS, W4, W6, bits, block_gaussian, random_experts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32), (17, 96, 160), (64, 160, 2080), (65, 96, 160), (130, 160, 2080)]
GATES = {"swiglu": model.SWIGLU, "gpt-oss": model.GPT_OSS}
BITS = {"mxfp8": 8, "mxfp4": 4, "mxfp6_e2m3": 6}


def quantizer(mx, activations):
    return {"mxfp8": mx.quantize_mxfp8, "mxfp4": mx.quantize_mxfp4_act, "mxfp6_e2m3": mx.quantize_mxfp6_act}[activations]


def same(got, want, what):
    """Two (codes, scale bytes) pairs, equal byte for byte."""
    for g, w, name in zip(got, want, ("codes", "scale bytes")):
        g, w = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (g, w))
        assert g.shape == w.shape and g.dtype == np.uint8 and w.dtype == np.uint8, (what, name, g.shape, w.shape)
        wrong = np.argwhere(g != w)
        assert wrong.size == 0, f"{what}: {len(wrong)} of {g.size} {name} differ, first at {wrong[:4].tolist()}: got {g[tuple(wrong[0])]}, want {w[tuple(wrong[0])]}"


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integers_bit_for_bit(shape, activations, weights):
    """Shares nothing with the project's kernels: with alpha = 0 the gate has no transcendental (s = 0.5 exactly), and with
    integer activations in +-4 under scale bytes 126 .. 128, weights under the same and a bias in multiples of 1 / 8 every
    term and every partial sum is a multiple of q below 2^24 q (the construction and conditions of
    tests/test_gpu_mx_experts.py's test of this name), so the float32 sums are exact in any order; the gate's four remaining
    operations are each rounded once in float32 by NumPy as on the GPU, and the quantizer models are exact.  Both layouts,
    with and without bias, limit 3 and None, shift 0 and 1."""
    from sleekit_amd import mx

    M, N, K = shape
    rng = np.random.default_rng(1000 * M + 7 * N + K + len(activations) + 3 * len(weights))
    a_codes = ENCODE[activations](rng.integers(-4, 5, (M, K)).astype(np.float64))
    a_scales = (127 + rng.integers(-1, 2, (M, K // 32))).astype(np.uint8)
    codes, scales = (t[0] for t in random_experts(rng, 1, 2 * N, K, 126, 128, weights))
    bias = (rng.integers(-64, 65, 2 * N) / 8.0).astype(np.float32)
    A = mx_experts_model.DEQUANTIZE_ACT[activations](a_codes, a_scales)
    Wmax = np.abs(mx6_model.dequantize_model(codes, scales) if weights == W6 else mx_gemm_model.weights_model(codes, scales)).max()
    q = 2.0 ** -3 if weights == W4 else 2.0 ** -5   # A in halves; W in quarters (E2M1) or sixteenths (E2M3)
    assert np.abs(A).max() <= 8 and (A * 2 == np.rint(A * 2)).all() and Wmax <= (12 if weights == W4 else 15)
    assert K * 8 * Wmax + 8 < 2 ** 24 * q and (weights != W4 or K * 96 + 8 < 2 ** 21)
    sums = model.sums_model(a_codes, a_scales, codes, scales, activations, weights)
    dev = tuple(torch.from_numpy(t).cuda() for t in (a_codes, a_scales, codes, scales))
    bias_d = torch.from_numpy(bias).cuda()
    for interleaved in (False, True):
        for b, b_d in ((None, None), (bias, bias_d)):
            for limit in (3.0, None):
                for shift in (0.0, 1.0):
                    gate = dict(alpha=0.0, limit=limit, shift=shift, interleaved=interleaved)
                    want = model.hidden_model(sums, b, activations, **gate)
                    got = mx.matmul_mx_glu(*dev, b_d, activations=activations, weights=weights, **gate)
                    assert tuple(got[0].shape) == (M, N * BITS[activations] // 8) and tuple(got[1].shape) == (M, N // 32)
                    same(got, want, f"{shape} {activations} x {weights} {gate} bias {b is not None}")


# ---------------------------------------------------------------------------------------------------------------- 2. three steps
@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_equals_its_three_steps(shape, activations, weights):
    """Block-Gaussian data: the fused product's codes, scale bytes and flag are those of matmul_mx to float32, glu to float32
    and the format's quantizer, at SwiGLU and gpt-oss parameters, in both layouts, with and without bias."""
    from sleekit_amd import mx

    M, N, K = shape
    rng = np.random.default_rng(77 + 1000 * M + N + K + len(activations) + 3 * len(weights))
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    a_codes, a_scales = quantizer(mx, activations)(x)
    codes, scales = (torch.from_numpy(t[0]).cuda() for t in random_experts(rng, 1, 2 * N, K, 118, 123, weights))
    bias = torch.from_numpy(rng.standard_normal(2 * N).astype(np.float32)).cuda()
    kw = dict(activations=activations, weights=weights)
    seen = set()
    for name, gate in GATES.items():
        for interleaved in (False, True):
            for b in (None, bias):
                y = mx.matmul_mx(a_codes, a_scales, codes, scales, b, dtype=torch.float32, **kw)
                h = mx.glu(y, interleaved=interleaved, dtype=torch.float32, **gate)
                assert h.dtype == torch.float32 and tuple(h.shape) == (M, N) and bool(torch.isfinite(h).all())
                want = quantizer(mx, activations)(h)
                hc, hs, flag = mx._matmul_mx_glu(a_codes, a_scales, codes, scales, b, interleaved=interleaved, **kw, **gate)
                same((hc, hs), want, f"{shape} {activations} x {weights} {name} interleaved {interleaved} bias {b is not None}")
                assert int(flag.item()) == 0
                same(mx.matmul_mx_glu(a_codes, a_scales, codes, scales, b, interleaved=interleaved, **kw, **gate), want, "the public call")
                seen.add(bits(h).tobytes())
    assert len(seen) == 8   # (the parameters, the layout and the bias all reach h)


# ---------------------------------------------------------------------------------------------------------------- 3. the gate
def gate_bound(g, u, alpha=1.0, limit=None, shift=0.0):
    """|h - h64| allowed for float32 inputs g, u, from the operations mx_glu uses (sleekit_amd/csrc/mxglu.h), eps = 2^-24:
      t = alpha g'            one rounding: |dt| <= |t| eps                (g', u' are exact: comparisons and selections)
      e = expf(-t)            relative error |dt| (the argument's) + 2 eps (expf is within 1 ulp = 2^-23 relative)
      d = 1 + e               the error of e enters with weight e / d <= 1; one rounding: + eps
      s = 1 / d               IEEE division: + eps
      b = g' s                + eps
      a = u' + shift          one rounding: eps, relative to a
      h = a b                 + eps
    so |h - h64| <= (|t| + 7) eps |h64|, taken up to second order (a factor 1 + 2^-10).  Below the normal range a result is
    rounded on the denormal grid instead, 2^-150 absolute: s (which reaches h times |a g'|), b (times |a|) and h itself.  And
    where -t > 88, e may be above float32's largest number: then d is +inf and s is 0 in place of a true s <= 2^-126, which
    reaches h as |a g'| s64.  Nothing is taken from what the GPU returns; the largest |err| / bound seen on the MI355X is in
    DESIGN.md section 26."""
    eps, tiny = 2.0 ** -24, 2.0 ** -150
    f = lambda v: np.float64(np.float32(v))  # noqa: E731
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    lim = np.inf if limit is None else f(limit)
    gc, uc = np.minimum(g, lim), np.clip(u, -lim, lim)
    with np.errstate(over="ignore", under="ignore"):
        t = f(alpha) * gc
        s64 = 1.0 / (1.0 + np.exp(-t))
        a = np.abs(uc + f(shift))
        h64 = np.abs(model.gate_f64(g, u, alpha, limit, shift))
        s_abs = np.where(-t > 88.0, s64 + tiny, tiny)
        return (np.abs(t) + 7.0) * eps * (1.0 + 2.0 ** -10) * h64 + a * (np.abs(gc) * s_abs + tiny) + tiny


def grid_values(limit):
    v = [np.arange(-20 * 64, 20 * 64 + 1) / 64.0, [0.0, -0.0, 88.0, -88.0, 1e30, -1e30]]
    if limit is not None:
        L = np.float32(limit)
        v.append([L, -L, np.nextafter(L, np.float32(np.inf)), np.nextafter(L, np.float32(0)), -np.nextafter(L, np.float32(np.inf)),
                  -np.nextafter(L, np.float32(0))])
    v = np.concatenate([np.asarray(p, np.float32) for p in v])
    return np.concatenate([v, np.zeros(-len(v) % 4, np.float32)])  # (a multiple of 4 columns: the kernel's vector form)


@pytest.mark.parametrize("name", list(GATES))
def test_gate_against_float64_on_a_dense_grid(name):
    """Every pair (g, u) of the grid -1280 / 64 .. 1280 / 64, the clamp's edges (limit and its two neighbours, both signs), +-0,
    +-88 and +-1e30, as one matrix Y = [G | U]: |glu - float64 model| <= gate_bound.  Where |h64| is at or above 2^128 the
    float32 result must be the infinity of its sign (between 2^127 and there either is right); a NaN never appears."""
    from sleekit_amd import mx

    gate = GATES[name]
    v = grid_values(gate["limit"])
    n = len(v)
    Y = np.empty((n, 2 * n), np.float32)
    Y[:, :n], Y[:, n:] = v[:, None], v[None, :]
    got = mx.glu(torch.from_numpy(Y).cuda(), dtype=torch.float32, **gate)
    h = got.cpu().numpy().astype(np.float64)
    G, U = np.broadcast_to(v[:, None], (n, n)), np.broadcast_to(v[None, :], (n, n))
    want = model.gate_f64(G, U, **gate)
    assert not np.isnan(h).any() and not np.isnan(want).any()
    safe, over = np.abs(want) < 2.0 ** 127, np.abs(want) >= 2.0 ** 128
    assert (h[over] == np.sign(want[over]) * np.inf).all() and (name != "swiglu" or over.any())
    ratio = np.abs(h[safe] - want[safe]) / gate_bound(G[safe], U[safe], **gate)
    worst = np.argmax(ratio)
    print(f"mx_glu {name}: {n} x {n} pairs, max |err| / bound = {ratio.max():.3f} at g = {G[safe][worst]!r}, u = {U[safe][worst]!r}")
    assert ratio.max() <= 1.0, (ratio.max(), G[safe][worst], U[safe][worst])
    # the 16-bit outputs are the float32 output rounded once
    for dtype in (torch.bfloat16, torch.float16):
        assert np.array_equal(bits(mx.glu(torch.from_numpy(Y).cuda(), dtype=dtype, **gate)), bits(got.to(dtype)))


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("N", [7, 32])
def test_gate_layouts_inputs_and_nan(N, interleaved):
    """The two layouts pick the stated columns (N = 7: the scalar form; 32: the vector form), 16-bit inputs are read as their
    float32 values, leading dimensions are kept, NumPy in gives NumPy out, and a NaN in g or u gives a NaN in h."""
    from sleekit_amd import mx

    rng = np.random.default_rng(N)
    Y = (rng.standard_normal((3, 5, 2 * N)) * 4).astype(np.float32)
    gc, uc = model.columns(N, interleaved)
    first = None
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        Yd = torch.from_numpy(Y).cuda().to(dtype)
        h = mx.glu(Yd, interleaved=interleaved, dtype=torch.float32, **model.GPT_OSS)
        assert tuple(h.shape) == (3, 5, N) and h.dtype == torch.float32
        Yf = Yd.float()
        split = torch.cat([Yf[..., torch.from_numpy(gc).cuda()], Yf[..., torch.from_numpy(uc).cuda()]], dim=-1).contiguous()   # the same pairs, not interleaved
        assert np.array_equal(bits(h), bits(mx.glu(split, dtype=torch.float32, **model.GPT_OSS)))
        assert mx.glu(Yd, interleaved=interleaved, **model.GPT_OSS).dtype == dtype
        first = h if first is None else first
    err = np.abs(first.cpu().numpy() - model.glu_f64(Y, interleaved=interleaved, **model.GPT_OSS))
    assert (err <= gate_bound(*model.split(Y, interleaved), **model.GPT_OSS)).all()
    out = mx.glu(Y, interleaved=interleaved, **model.GPT_OSS)
    assert isinstance(out, np.ndarray) and np.array_equal(bits(out), bits(first))
    bad = Y.copy()
    bad[0, 0, gc[1]], bad[1, 2, uc[N - 1]] = np.nan, np.nan
    for gate in GATES.values():
        h = mx.glu(torch.from_numpy(bad).cuda(), interleaved=interleaved, **gate).cpu().numpy()
        assert np.isnan(h[0, 0, 1]) and np.isnan(h[1, 2, N - 1]) and np.isnan(h).sum() == 2


# ---------------------------------------------------------------------------------------------------------------- 4. non-finite
@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_non_finite_raises_the_flag(shape, activations, weights):
    """Activation scale bytes of 254 against weight scale bytes of 254: the sums overflow.  The flag is raised, the public
    call raises, and codes and scale bytes are the three-step route's; with the scale bytes back to finite data the flag stays 0."""
    from sleekit_amd import mx

    M, N, K = shape
    rng = np.random.default_rng(M + N)
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    a_codes, a_scales = quantizer(mx, activations)(x)
    codes, scales = (torch.from_numpy(t[0]).cuda() for t in random_experts(rng, 1, 2 * N, K, 118, 123, weights))
    kw = dict(activations=activations, weights=weights, **model.GPT_OSS)
    fmt = mx._FORMATS[activations]
    for big, raised in ((True, 1), (False, 0)):
        asc, wsc = (torch.full_like(a_scales, 254), torch.full_like(scales, 254)) if big else (a_scales, scales)
        hc, hs, flag = mx._matmul_mx_glu(a_codes, asc, codes, wsc, None, interleaved=True, **kw)
        h = mx.glu(mx.matmul_mx(a_codes, asc, codes, wsc, activations=activations, weights=weights), interleaved=True, dtype=torch.float32, **model.GPT_OSS)
        assert bool(torch.isfinite(h).all()) != big
        wc, ws, wflag = mx._quantize_act(h, M, N, fmt)
        assert int(flag.item()) == raised == int(wflag.item())
        same((hc, hs), (wc, ws), f"{shape} {activations} x {weights} scale bytes 254: {big}")
        if big:
            with pytest.raises(ValueError, match="finite"):
                mx.matmul_mx_glu(a_codes, asc, codes, wsc, interleaved=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
GUARD = 256


def guarded(nbytes, fill=0xA5):
    """A device buffer of nbytes + GUARD bytes, all `fill`; 256-byte blocks keep the start on 16 bytes."""
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_nothing_is_written_past_the_outputs(shape, activations, weights):
    """h_codes and h_scales of exactly their stated sizes with 256 sentinel bytes behind each: the guard is unchanged, and
    what lies before it is the public call's."""
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, mx

    M, N, K = shape
    rng = np.random.default_rng(3 * M + N)
    a_codes, a_scales = quantizer(mx, activations)(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t[0]).cuda() for t in random_experts(rng, 1, 2 * N, K, 118, 123, weights))
    fmt, wf = mx._FORMATS[activations], mx._WEIGHTS[weights]
    nc, ns = M * N * fmt.bits // 8, M * N // 32
    hc, hs, flag = guarded(nc), guarded(ns), torch.zeros(1, dtype=torch.int32, device="cuda")
    a_codes, codes = dev.aligned(a_codes), dev.aligned(codes)
    _lib.check(_lib.lib.slk_mx_gemm_glu(dev.ptr(a_codes), dev.ptr(a_scales), dev.ptr(codes), dev.ptr(scales), None, M, N, K, fmt.c_fmt, wf.c_fmt,
                                        1.702, 7.0, 1.0, 0, dev.ptr(hc), dev.ptr(hs), dev.ptr(flag), dev.stream_handle()))
    assert (hc[nc:] == 0xA5).all() and (hs[ns:] == 0xA5).all() and int(flag.item()) == 0
    want = mx.matmul_mx_glu(a_codes, a_scales, codes, scales, activations=activations, weights=weights, **model.GPT_OSS)
    same((hc[:nc].reshape(M, -1), hs[:ns].reshape(M, -1)), want, f"{shape} {activations} x {weights}")


# ---------------------------------------------------------------------------------------------------------------- 6. experts
EXPERT_SHAPES = [((0, 1, 17, 65, 0), 96, 160), ((64, 65, 16), 32, 160), ((15, 0, 47, 130), 160, 2080)]
EXPERT_CASES = [(0, a, w) for a, w in PAIRS] + [(1, "mxfp8", W4), (2, "mxfp8", W4)]


def expert_operands(mx, shape, activations, weights):
    counts, N, K = EXPERT_SHAPES[shape]
    E, M = len(counts), sum(counts)
    rng = np.random.default_rng(500 + shape + len(activations) + 3 * len(weights))
    a_codes, a_scales = quantizer(mx, activations)(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t).cuda() for t in random_experts(rng, E, 2 * N, K, 118, 123, weights))
    bias = torch.from_numpy(rng.standard_normal((E, 2 * N)).astype(np.float32)).cuda()
    return a_codes, a_scales, codes, scales, bias, mx_experts_model.offsets_of(counts)


@pytest.mark.parametrize("shape,activations,weights", EXPERT_CASES)
def test_experts_equal_the_dense_call_on_every_slice(shape, activations, weights):
    from sleekit_amd import mx

    counts, N, K = EXPERT_SHAPES[shape]
    a_codes, a_scales, codes, scales, bias, offsets = expert_operands(mx, shape, activations, weights)
    offsets_d = torch.from_numpy(offsets).cuda()
    kw = dict(activations=activations, weights=weights)
    for gate, interleaved, b in ((model.GPT_OSS, True, bias), (model.SWIGLU, False, None)):
        hc, hs = mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets_d, b, interleaved=interleaved, **kw, **gate)
        assert tuple(hc.shape) == (sum(counts), N * BITS[activations] // 8) and tuple(hs.shape) == (sum(counts), N // 32)
        for e in range(len(counts)):
            lo, hi = int(offsets[e]), int(offsets[e + 1])
            if hi > lo:
                alone = mx.matmul_mx_glu(a_codes[lo:hi], a_scales[lo:hi], codes[e], scales[e], None if b is None else b[e], interleaved=interleaved,
                                         **kw, **gate)
                same((hc[lo:hi], hs[lo:hi]), alone, f"expert {e} of {counts}, rows {lo} .. {hi - 1}")
        unfused = mx._matmul_mx_glu_experts(a_codes, a_scales, codes, scales, offsets_d, b, activations, weights, interleaved=interleaved, fused=False, **gate)
        same((hc, hs), unfused[:2], "the three-step route over experts")
        assert int(unfused[2].item()) == 0 and int(unfused[3].item()) == 0


@pytest.mark.parametrize("offsets", [[0, 40, 30, 83], [1, 30, 83], [0, 30, 82], [0, 30, 84]])
def test_invalid_offsets_raise_flag_0_and_write_nothing(offsets):
    """Decreasing, first not 0, last not M: flag[0] is raised, flag[1] is not, and sentinel-filled outputs keep every byte."""
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, mx

    M, N, K, E = 83, 96, 160, len(offsets) - 1
    rng = np.random.default_rng(9)
    a_codes, a_scales = mx.quantize_mxfp8(torch.from_numpy(block_gaussian(rng, M, K)).cuda())
    codes, scales = (torch.from_numpy(t).cuda() for t in random_experts(rng, E, 2 * N, K, 118, 123, W4))
    bad = torch.tensor(offsets, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
        mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, bad)
    hc, hs, flags = guarded(M * N, 0x5A), guarded(M * N // 32, 0x5A), torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = _lib.lib.slk_mx_experts_workspace_bytes(E, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a_codes, codes = dev.aligned(a_codes), dev.aligned(codes)
    _lib.check(_lib.lib.slk_mx_gemm_glu_experts(dev.ptr(a_codes), dev.ptr(a_scales), dev.ptr(codes), dev.ptr(scales), None, dev.ptr(bad), E, M, N, K,
                                                _lib.MX_ACT_FP8, _lib.MX_W_FP4, 1.0, float("inf"), 0.0, 0, dev.ptr(hc), dev.ptr(hs), dev.ptr(flags),
                                                dev.ptr(ws), nbytes, dev.stream_handle()))
    assert flags.tolist() == [1, 0] and (hc == 0x5A).all() and (hs == 0x5A).all()
    good = torch.tensor([0] * E + [M], dtype=torch.int32, device="cuda")   # and the next call is not held up by the last flag
    got = mx.matmul_mx_glu_experts(a_codes, a_scales, codes, scales, good)
    same(got, mx.matmul_mx_glu(a_codes, a_scales, codes[E - 1], scales[E - 1]), "all rows of the last expert")


# ---------------------------------------------------------------------------------------------------------------- 7. the surface
def layer(rng, rows, K, weights):
    codes, scales = (torch.from_numpy(t[0]).cuda() for t in random_experts(rng, 1, rows, K, 118, 123, weights))
    return codes, scales, torch.from_numpy(rng.standard_normal(rows).astype(np.float32)).cuda()


@pytest.mark.parametrize("activations,weights", PAIRS)
@pytest.mark.parametrize("M", [17, 65])
def test_gated_mlp_is_its_public_steps(M, activations, weights):
    """gated_mlp_mx fused and unfused, the public calls written out, MXGatedMLP.forward and the rotations, bit for bit."""
    from sleekit_amd import mx, rotation

    N, K, Nd = 96, 160, 48
    rng = np.random.default_rng(M)
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    (uc, us, ub), (dc, ds, db) = layer(rng, 2 * N, K, weights), layer(rng, Nd, N, weights)
    kw = dict(activations=activations, weights=weights)
    gate = dict(interleaved=True, **model.GPT_OSS)
    got = mx.gated_mlp_mx(x, uc, us, dc, ds, ub, db, **kw, **gate)
    assert got.dtype == torch.float32 and tuple(got.shape) == (M, Nd)
    assert np.array_equal(bits(got), bits(mx.gated_mlp_mx(x, uc, us, dc, ds, ub, db, fused=False, **kw, **gate)))
    a = quantizer(mx, activations)(x)
    h = mx.matmul_mx_glu(*a, uc, us, ub, **kw, **gate)
    assert np.array_equal(bits(got), bits(mx.matmul_mx(*h, dc, ds, db, **kw)))
    y = mx.matmul_mx(*a, uc, us, ub, dtype=torch.float32, **kw)
    h3 = quantizer(mx, activations)(mx.glu(y, dtype=torch.float32, **gate))
    assert np.array_equal(bits(got), bits(mx.matmul_mx(*h3, dc, ds, db, **kw)))
    # the output dtype follows x, or `dtype`; leading dimensions are kept; NumPy in, NumPy out
    half = mx.gated_mlp_mx(x.half().reshape(1, M, K), uc, us, dc, ds, ub, db, **kw, **gate)
    assert half.dtype == torch.float16 and tuple(half.shape) == (1, M, Nd)
    assert np.array_equal(bits(mx.gated_mlp_mx(x.half(), uc, us, dc, ds, ub, db, dtype=torch.float32, **kw, **gate).half()), bits(half[0]))
    out = mx.gated_mlp_mx(*(t.cpu().numpy() for t in (x, uc, us, dc, ds, ub, db)), **kw, **gate)
    assert isinstance(out, np.ndarray) and np.array_equal(bits(out), bits(got))
    # the module
    up, down = mx.MXLinear(K, 2 * N, activations=activations, weights=weights).cuda(), mx.MXLinear(N, Nd, activations=activations, weights=weights).cuda()
    for mod, (c, s, b) in ((up, (uc, us, ub)), (down, (dc, ds, db))):
        mod.codes.copy_(c), mod.scales.copy_(s), mod.bias.copy_(b)
    mlp = mx.MXGatedMLP(up, down, **gate)
    assert np.array_equal(bits(mlp(x)), bits(got)) and np.array_equal(bits(mlp(x, fused=False)), bits(got))
    # a rotation on x runs inside the quantizer; one on h takes the three-step route
    rot, rot_h = rotation.Rotation(K, block=32, seed=9), rotation.Rotation(N, block=32, seed=4)
    turned = mx.gated_mlp_mx(x, uc, us, dc, ds, ub, db, rotation=rot, **kw, **gate)
    assert np.array_equal(bits(turned), bits(mx.gated_mlp_mx(rot.apply(x, dtype=torch.float32), uc, us, dc, ds, ub, db, **kw, **gate)))
    assert np.array_equal(bits(turned), bits(mlp(x, rotation=rot))) and not np.array_equal(bits(turned), bits(got))
    behind = mx.gated_mlp_mx(x, uc, us, dc, ds, ub, db, down_rotation=rot_h, **kw, **gate)
    hr = quantizer(mx, activations)(rot_h.apply(mx.glu(y, dtype=torch.float32, **gate), dtype=torch.float32))
    assert np.array_equal(bits(behind), bits(mx.matmul_mx(*hr, dc, ds, db, **kw)))
    bad = x.clone()
    bad[M - 1, 7] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        mx.gated_mlp_mx(bad, uc, us, dc, ds, ub, db, **kw, **gate)


def routed_sum(y, T, k, gates):
    """MXExperts.forward_tokens' combine, written out: (T k, N) rows in (T, k) order -> the ordered float32 sum."""
    y = y.reshape(T, k, -1).float()
    total = y[:, 0] if gates is None else y[:, 0] * gates[:, 0:1]
    for j in range(1, k):
        total = total + (y[:, j] if gates is None else y[:, j] * gates[:, j:j + 1])
    return total


@pytest.mark.parametrize("gated", [True, False])
def test_forward_tokens_against_a_loop_of_gated_mlps(gated):
    """T = 8 tokens, k = 2 of E = 4 experts: MXExpertsMLP.forward_tokens equals a Python loop over experts of MXGatedMLP on
    each expert's tokens followed by the same ordered float32 sum, and MXExperts.forward_tokens on the same inputs gives the
    bits of its routine as it stood before the helper was shared, inlined here."""
    from sleekit_amd import mx

    T, k, E, N, K, Nd = 8, 2, 4, 96, 160, 48
    rng = np.random.default_rng(12)
    x = torch.from_numpy(block_gaussian(rng, T, K)).cuda()
    ids = torch.from_numpy(np.stack([rng.permutation(E)[:k] for _ in range(T)])).cuda()
    gates = torch.from_numpy(rng.random((T, k)).astype(np.float32)).cuda() if gated else None
    up, down = mx.MXExperts(E, K, 2 * N).cuda(), mx.MXExperts(E, N, Nd).cuda()
    for mod, rows, cols in ((up, 2 * N, K), (down, Nd, N)):
        c, s = random_experts(rng, E, rows, cols, 118, 123, W4)
        mod.codes.copy_(torch.from_numpy(c)), mod.scales.copy_(torch.from_numpy(s)), mod.bias.copy_(torch.from_numpy(rng.standard_normal((E, rows)).astype(np.float32)))
    gate = dict(interleaved=True, **model.GPT_OSS)
    mlp = mx.MXExpertsMLP(up, down, **gate)
    got = mlp.forward_tokens(x, ids, gates)
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, Nd)
    assert np.array_equal(bits(got), bits(mlp.forward_tokens(x, ids, gates, fused=False)))
    per = torch.zeros((T, k, Nd), device="cuda")
    for e in range(E):
        one = mx.MXGatedMLP(mx.MXLinear(K, 2 * N), mx.MXLinear(N, Nd), **gate).cuda()
        for sub, src in ((one.up, up), (one.down, down)):
            sub.codes.copy_(src.codes[e]), sub.scales.copy_(src.scales[e]), sub.bias.copy_(src.bias[e])
        t, j = torch.nonzero(ids == e, as_tuple=True)
        if len(t):
            per[t, j] = one(x[t])
    assert np.array_equal(bits(got), bits(routed_sum(per, T, k, gates)))
    # forward on sorted rows is what forward_tokens runs
    order, offsets = mx.sort_by_expert(ids, E)
    assert np.array_equal(bits(mlp(x[order // k], offsets)), bits(per.reshape(T * k, Nd)[order]))
    # MXExperts.forward_tokens: the routine before the move, inlined
    y = mx.linear_mx_experts(x[order // k], up.codes, up.scales, offsets, up.bias)
    back = torch.empty_like(order)
    back[order] = torch.arange(order.numel(), device=order.device)
    assert np.array_equal(bits(up.forward_tokens(x, ids, gates)), bits(routed_sum(y[back], T, k, gates)))
    beyond = ids.clone()
    beyond[T // 2, 1] = E
    with pytest.raises(ValueError, match="0 .. 3"):
        mlp.forward_tokens(x, beyond, gates)
    with pytest.raises(ValueError, match=r"offsets\[0\] == 0"):
        mlp(x[order // k], offsets.flip(0).contiguous())


# ---------------------------------------------------------------------------------------------------------------- 8. which message wins
def tiny_mlp(mx, rng, E=2, K=32, N=32, Nd=16):
    """MXExpertsMLP of E experts: up layers of 2 N = 64 rows, down layers 16 x 32, MXFP8 on MXFP4."""
    up, down = mx.MXExperts(E, K, 2 * N).cuda(), mx.MXExperts(E, N, Nd).cuda()
    for mod, rows, cols in ((up, 2 * N, K), (down, Nd, N)):
        c, s = random_experts(rng, E, rows, cols, 118, 123, W4)
        mod.codes.copy_(torch.from_numpy(c)), mod.scales.copy_(torch.from_numpy(s))
    return mx.MXExpertsMLP(up, down)


@pytest.mark.parametrize("fused", [True, False])
def test_two_raised_flags_give_the_first_message(fused, monkeypatch):
    """E = 2, M = 4, K = 32, N = 32.  (a) a NaN in x and offsets that break the rule: the finite message; (b) a NaN in x and an
    expert id of E: the id message; (c) finite x against an up layer of scale bytes 254, so that h overflows: the finite message;
    (d) valid x and invalid offsets: the offsets rule, and the result's buffer keeps its sentinel.  (Invalid offsets are refused
    by the prologue before any address is made from them.)"""
    from sleekit_amd import mx

    E, M, K, N, Nd = 2, 4, 32, 32, 16
    rng = np.random.default_rng(27)
    mlp = tiny_mlp(mx, rng)
    x = torch.from_numpy(block_gaussian(rng, M, K)).cuda()
    nan = x.clone()
    nan[1, 3] = float("nan")
    bad_offsets = torch.tensor([0, 3, 2], dtype=torch.int32, device="cuda")

    def message(call):
        with pytest.raises(ValueError) as raised:
            call()
        return str(raised.value)

    assert message(lambda: mlp(nan, bad_offsets, fused=fused)) == mx._H_FINITE                                           # (a)
    assert message(lambda: mlp.forward_tokens(nan, torch.tensor([[0], [1], [E], [0]], device="cuda"), fused=fused)) == mx._ids_message(E)  # (b)
    up = (mlp.up.codes[0], torch.full_like(mlp.up.scales[0], 254))                                                      # (c)
    assert bool(torch.isfinite(x).all())
    assert message(lambda: mx.gated_mlp_mx(100.0 * x, *up, mlp.down.codes[0], mlp.down.scales[0], fused=fused)) == mx._H_FINITE
    # (d): every (M, Nd) float32 buffer the call allocates starts as sentinel bytes; the last of them is the result's
    made, empty = [], torch.empty

    def sentinel_empty(*args, **kw):
        t = empty(*args, **kw)
        if tuple(t.shape) == (M, Nd) and t.dtype == torch.float32:
            t.view(torch.uint8).fill_(0x5A)
            made.append(t)
        return t

    monkeypatch.setattr(torch, "empty", sentinel_empty)
    assert message(lambda: mlp(x, bad_offsets, fused=fused)) == mx._OFFSETS_RULE
    monkeypatch.undo()
    assert made and bool((made[-1].view(torch.uint8) == 0x5A).all())
