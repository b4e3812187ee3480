"""Group-wise scales on the MI355X (sleekit_amd.groups) against the reference's own grouped results (tests/golden/groups.npz,
made by tests/golden/make_golden_groups.py) and against the per-row path already pinned.

Run on the GPU box:  python -m pytest tests/test_gpu_groups.py -m gpu -q
"""

import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from sleekit_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    assert torch.cuda.is_available(), "these tests need the GPU"
    data = np.load(os.path.join(GOLDEN, "groups.npz"))
    return data, json.loads(str(data["meta"]))


def codebook(name):
    from sleekit_amd.codebook import Codebook, UniformCodebook

    return Codebook.nf4() if name == "nf4" else UniformCodebook(int(name), -1, 1)


def sha(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_case(c, S, device=False, **kw):
    from sleekit_amd import groups

    L = synth.make_layer(c["R"], c["n"], c["seed"])
    W, H = L["W"], L["H"]
    if device:
        W, H, S = (torch.from_numpy(x).cuda() for x in (W, H, np.ascontiguousarray(S)))
    return groups.quantize_grouped(W, S, codebook(c["codebook"]), H, c["g"], c["act_order"], c["damp"], c["min_block_size"],
                                   c["num_blocks"], **kw)


def test_loop_matches_the_reference(fx):
    data, meta = fx
    for i, c in enumerate(meta["cases"]):
        Q = run_case(c, data[f"S_{i}"])
        assert isinstance(Q, np.ndarray) and Q.dtype == np.float32
        assert sha(Q) == c["sha256_Q"], f"case {i}: {c}"


def test_loop_on_device_tensors(fx):
    data, meta = fx
    for i, c in enumerate(meta["cases"]):
        Q = run_case(c, data[f"S_{i}"], device=True)
        assert isinstance(Q, torch.Tensor) and Q.is_cuda and Q.dtype == torch.float32
        assert sha(Q) == c["sha256_Q"], f"case {i}: {c}"


def test_indices_rebuild_q(fx):
    from sleekit_amd import groups

    data, meta = fx
    for i, c in enumerate(meta["cases"]):
        if codebook(c["codebook"]).__len__() > 256:
            continue
        S = data[f"S_{i}"]
        Q, idx = run_case(c, S, return_indices=True)
        assert idx.dtype == np.uint8 and idx.shape == Q.shape and sha(Q) == c["sha256_Q"]
        if f"idx_{i}" in data.files:  # the reference's own indices, kept for the smaller cases
            assert np.array_equal(idx, data[f"idx_{i}"]), f"case {i}: {c}"
        back = groups.dequantize_grouped(idx, S, codebook(c["codebook"]), c["g"])
        assert np.array_equal(bits(back), bits(Q)), f"case {i}: {c}"


def test_window_rows_and_latency_flag_give_the_same_bits(fx):
    from sleekit_amd import _lib

    data, meta = fx
    for i in (1, 9, 13, 26):
        c = meta["cases"][i]
        for rows in (16, 32):
            with _lib.option("window_rows", rows):
                assert sha(run_case(c, data[f"S_{i}"])) == c["sha256_Q"], (i, rows)


def large_scales(big):
    """The 4096 x 4096 layer and its group scales from the device search, held to the reference's hash."""
    from sleekit_amd import groups

    L = synth.make_layer_device(big["R"], big["n"], big["seed"], torch.device("cuda"))
    S = groups.compute_group_scaling(L["W"], codebook(big["codebook"]), big["g"], L["H"], big["mode"])
    return L, S


def test_large_layer_group_scales(fx):
    _, meta = fx
    _, S = large_scales(meta["large"])
    assert S.dtype == torch.float32 and sha(S) == meta["large"]["sha256_S"]


def test_large_layer_matches_the_reference_hash(fx):
    from sleekit_amd import groups

    _, meta = fx
    big = meta["large"]
    L, S = large_scales(big)
    assert sha(S) == big["sha256_S"], "the loop's input differs from the reference's scales (see test_large_layer_group_scales)"
    Q = groups.quantize_grouped(L["W"], S, codebook(big["codebook"]), L["H"], big["g"], big["act_order"], big["damp"])
    assert sha(Q) == big["sha256_Q"]


def test_group_scales_match_the_reference(fx):
    """Every mode bit for bit, except that the hessian modes' errors come out of a product summed in another order than
    the BLAS's (and hessianN's in float32 where the reference promotes to float64): there a pick may differ, to a
    neighbouring grid point -- the deviation sleekit_amd.scaling documents for the per-row search."""
    from sleekit_amd import groups

    data, meta = fx
    for i, c in enumerate(meta["cases"]):
        L = synth.make_layer(c["R"], c["n"], c["seed"])
        S = groups.compute_group_scaling(L["W"], codebook(c["codebook"]), c["g"], L["H"], c["mode"])
        want = data[f"S_{i}"]
        assert S.shape == want.shape and S.dtype == np.float32
        same = bits(S) == bits(want)
        if c["mode"].startswith("hessian"):
            assert same.mean() >= 0.95, (i, c, same.mean())
            np.testing.assert_allclose(S, want, rtol=0.05)
        else:
            assert same.all(), (i, c, np.argwhere(~same)[:5])


def test_whole_rows_with_power_of_two_scales_match_the_per_row_path():
    """g = n and per-row scales 2^k: scaling by 2^k commutes with every rounding, so the grouped loop on unscaled weights
    and quantize_with_scaling (scaled loop, de-scaled after) give the same bits."""
    from sleekit_amd import codebook as cbm
    from sleekit_amd import groups, scaling

    R, n = 96, 256
    L = synth.make_layer(R, n, 6101)
    W, H = L["W"], L["H"]
    k = np.floor(np.log2(np.abs(W).max(axis=1))).astype(np.int32)
    s = np.ldexp(np.float32(1), k).astype(np.float32)
    cb = cbm.UniformCodebook(8, -1, 1)
    for order in ("none", "diag", "pivot"):
        want = scaling.quantize_with_scaling(W, s, cb, H, act_order=order, damp=0.01)
        got = groups.quantize_grouped(W, s[:, None].copy(), cb, H, n, act_order=order, damp=0.01)
        assert np.array_equal(bits(got), bits(want)), order


def test_sleekit_quantize_with_group_size():
    import torch.nn as nn

    import sleekit_amd
    from sleekit_amd import _device as dev
    from sleekit_amd import _lib, groups
    from sleekit_amd.codebook import UniformCodebook

    torch.manual_seed(0)
    layer = nn.Linear(256, 96).cuda()
    st = sleekit_amd.Sleekit(layer)
    X = torch.from_numpy(synth.make_activations(1024, 256, 77)).float().cuda()
    st.add_batch(X)
    W0 = layer.weight.data.clone()
    b0 = layer.bias.data.clone()
    st.quantize(3, group_size=128, scaling_mode="diag", order_mode="sqerr", bias_correction=True, damp=0.03)
    cb = UniformCodebook(8, -1, 1)
    Hc = torch.empty_like(st.hessian)
    _lib.check(_lib.lib.slk_hessian_strip_mean(dev.ptr(st.hessian), dev.ptr(st.mean), 256, dev.ptr(Hc), dev.stream_handle()))
    S = groups.compute_group_scaling(W0, cb, 128, Hc, "diag")
    Q = groups.quantize_grouped(W0, S, cb, Hc, 128, "sqerr", 0.03)
    assert np.array_equal(bits(layer.weight.data), bits(Q))
    bias = b0 + ((W0 - Q) * st.mean).sum(dim=1)
    assert np.array_equal(bits(layer.bias.data), bits(bias))


def test_refusals_and_indefinite_hessian():
    import torch.nn as nn

    import sleekit_amd
    from sleekit_amd import groups
    from sleekit_amd.codebook import UniformCodebook

    layer = nn.Linear(64, 32).cuda()
    st = sleekit_amd.Sleekit(layer)
    st.add_batch(torch.randn(256, 64, device="cuda"))
    with pytest.raises(NotImplementedError):
        st.quantize(3, group_size=32, nb_ls_moves=5)
    with pytest.raises(NotImplementedError):
        st.quantize(3, group_size=32, scaling_mode="obq")
    cb = UniformCodebook(8, -1, 1)
    W = synth.make_weights(32, 64, 7)
    for mode in ("obq", "norm"):
        with pytest.raises(NotImplementedError):
            groups.compute_group_scaling(W, cb, 32, np.eye(64, dtype=np.float32), mode)
    with pytest.raises(ValueError):
        groups.quantize_grouped(W, np.ones((32, 2), np.float32), cb, np.eye(64, dtype=np.float32), 48)
    H = -np.eye(64, dtype=np.float32)
    with pytest.raises(np.linalg.LinAlgError):
        groups.quantize_grouped(W, np.ones((32, 2), np.float32), cb, H, 32, damp=0.0)
