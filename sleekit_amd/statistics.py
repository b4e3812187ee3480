"""`Sleekit`: the GPTQ-style layer adapter of the reference (sleekit/statistics.py:12-199), kept on the GPU.

    st = Sleekit(layer); st.add_batch(x) ...; st.quantize_sleekit_light(3)      # or .quantize(nbits, ...)

What each piece maps to:

* `add_batch` -- the running mean and Hessian of statistics.py:76-87 -- is ONE call of `slk_hessian_accumulate`
  per batch (float32-grade products of bfloat16 pieces on the matrix cores when the feature count is a multiple
  of 128, the float32 MFMA otherwise).  Samples are handed over as ROWS (T, n); the reference holds them as
  columns (n, T): same statistics.  Convolutions are seen through `torch.nn.functional.unfold` like there
  (statistics.py:44-69): pure data movement.
* `quantize` (statistics.py:146-190): scale selection (`sleekit_amd.scaling.compute_scaling`), the device
  pipeline (`engine.quantize_layer`) and the bias correction `bias += ((W - Q) * mean).sum(1)`, all on device
  tensors -- the reference goes through `.numpy()` for every one of them (statistics.py:162-166).
* the three presets (statistics.py:107-144) are rows of `_PRESETS`.

`ExpertStatistics` is the same running mean and Hessian for the E experts of a mixture-of-experts layer, one grouped call
a batch (`slk_hessian_accumulate_experts`, or `slk_hessian_accumulate_experts_mx` for rows that exist as MX codes only):

    up = ExpertStatistics(E, K);  up.add_tokens(x, expert_ids)            # (T, K) rows, (T, k) routing
    results = mx.quantize_experts(Ws, up.hessians())
"""

import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _device as dev
from . import _lib
from . import engine
from .codebook import UniformCodebook
from .scaling import compute_scaling

_SUPPORTED = (nn.Linear, nn.Conv1d, nn.Conv2d)

# keyword arguments of Sleekit.quantize behind quantize_<name>(nbits)
_PRESETS = {
    "basic": dict(scaling_mode="mse", order_mode="diag", bias_correction=False, damp=0.01, nb_ls_moves=0),
    "sleekit_light": dict(scaling_mode="diag", order_mode="sqerr", bias_correction=True, damp=0.03, nb_ls_moves=0),
    "sleekit_heavy": dict(scaling_mode="hessian", order_mode="sqerr", bias_correction=True, damp=0.03, nb_ls_moves=100),
}
_PRESET_NOTES = {
    "basic": "plain GPTQ-like settings, none of the improvements (statistics.py:107-118)",
    "sleekit_light": 'the "light" recipe (statistics.py:120-131)',
    "sleekit_heavy": 'the "heavy" recipe, 100 local-search moves (statistics.py:133-144)',
}


def _windows_as_rows(x, layer):
    """Every receptive field of a convolution as one row of length channels * prod(kernel) (statistics.py:44-69)."""
    kernel, dilation, padding, stride = layer.kernel_size, layer.dilation, layer.padding, layer.stride
    if isinstance(layer, nn.Conv1d):
        # a (k, 1) two-dimensional convolution over a trailing axis of length one
        x = x[None] if x.ndim == 2 else x
        x = x[..., None]
        kernel, dilation, padding, stride = (kernel[0], 1), (dilation[0], 1), (padding[0], 0), (stride[0], 1)
    elif x.ndim == 3:
        x = x[None]
    cols = F.unfold(x, kernel, dilation, padding, stride)  # (batch, features, positions)
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def _preset_method(name):
    def run(self, nbits):
        return self.quantize(nbits, **_PRESETS[name])

    run.__name__ = "quantize_" + name
    run.__doc__ = f"quantize(nbits) with {_PRESET_NOTES[name]}."
    return run


class Sleekit:
    """Running statistics of one layer's inputs and its quantization; interface of the reference's class."""

    def __init__(self, layer, rotation=None):
        if not isinstance(layer, _SUPPORTED):
            raise ValueError(f"Unsupported layer type {type(layer)}")
        if not layer.weight.is_cuda:
            raise RuntimeError("sleekit_amd.Sleekit accumulates on the GPU: move the layer to the device first")
        self.layer = layer
        features = layer.weight[0].numel()  # columns of the weight seen as an (out, features) matrix
        self.count = 0
        self.mean = torch.zeros(features, dtype=torch.float32, device=self.device)
        self.hessian = torch.zeros((features, features), dtype=torch.float32, device=self.device)
        # the Rotation quantize_mxfp4 uses (None: none); quantize and quantize_packed take theirs as a keyword and ignore this
        self.rotation = self._check_rotation(rotation)

    @property
    def device(self):
        return self.layer.weight.device

    def _prepare_input(self, inp):
        """(T, features) float32 samples of a batch of activations, one per row (statistics.py:37-74 gives the transpose)."""
        x = inp.to(self.device)
        rows = x.reshape(-1, x.shape[-1]) if isinstance(self.layer, nn.Linear) else _windows_as_rows(x, self.layer)
        assert rows.ndim == 2
        return rows.float().contiguous()

    def add_batch(self, inp, out=None):
        """mean <- mean c / (c + T) + sum / (c + T), hessian likewise with X^T X: statistics.py:76-87, one kernel call."""
        samples = self._prepare_input(inp)
        tokens, features = samples.shape
        assert features == self.mean.numel()
        scratch, scratch_bytes = dev.workspace(0, features)
        rc = _lib.lib.slk_hessian_accumulate(dev.ptr(self.hessian), dev.ptr(self.mean), dev.ptr(samples), features, tokens,
                                             int(self.count), dev.ptr(scratch), scratch_bytes, dev.stream_handle())
        _lib.check(rc)
        self.count += tokens

    def export(self, path, npy_format=False):
        """bias / weight / mean / hessian as four .pt (or .npy) files in `path`: what the experiments load (statistics.py:89-105)."""
        os.makedirs(path, exist_ok=True)
        for name in ("bias", "weight", "mean", "hessian"):
            value = getattr(self.layer, name) if name in ("bias", "weight") else getattr(self, name)
            host = value.detach().cpu()
            if npy_format:
                import numpy as np

                np.save(os.path.join(path, f"{name}.npy"), host.numpy())
            else:
                torch.save(host, os.path.join(path, f"{name}.pt"))

    quantize_basic = _preset_method("basic")
    quantize_sleekit_light = _preset_method("sleekit_light")
    quantize_sleekit_heavy = _preset_method("sleekit_heavy")

    def _check_rotation(self, rotation):
        """`rotation` (None: none); a ValueError unless it is a Rotation over the layer's features."""
        if rotation is None:
            return None
        from .rotation import Rotation

        if not isinstance(rotation, Rotation):
            raise ValueError(f"rotation must be a sleekit_amd.Rotation (got {type(rotation).__name__})")
        if rotation.n != self.mean.numel():
            raise ValueError(f"the rotation has {rotation.n} features but the layer has {self.mean.numel()}")
        return rotation

    def _weight_and_hessian(self, bias_correction, rotation=None):
        """The weight as an (out, features) float32 matrix and the Hessian to quantize against: H - mean mean^T under
        bias_correction (a copy), else H itself.  With a rotation R, the pair in the rotated basis: (W R, R^T H R), the mean
        stripped first."""
        weight = self.layer.weight.data.flatten(1).float().contiguous()
        H = self.hessian
        if bias_correction:
            centred = torch.empty_like(H)
            _lib.check(_lib.lib.slk_hessian_strip_mean(dev.ptr(H), dev.ptr(self.mean), H.shape[0], dev.ptr(centred), dev.stream_handle()))
            H = centred
        if rotation is not None:
            return rotation.apply(weight), rotation.hessian(H)
        return weight, H

    def _store(self, result, weight, bias_correction, rotation=None):
        """result.Q becomes the layer's weight; under bias_correction the expected output shift moves into the bias.
        With a rotation R the layer's weight is Q R^T -- on unrotated inputs the function the rotated layer computes on
        rotated ones -- and the shift is taken in the original basis; Q, idx and the scales stay in the rotated one."""
        if rotation is not None:
            return self._store_rotated(result, bias_correction, rotation)
        target = self.layer.weight
        target.data = result.Q.reshape(target.shape).to(target.dtype)
        if bias_correction:
            shift = ((weight - result.Q) * self.mean).sum(dim=1)
            self.layer.bias.data += shift.to(self.layer.bias.dtype)
        return result

    def _store_rotated(self, result, bias_correction, rotation):
        target = self.layer.weight
        weight = target.data.flatten(1).float().contiguous()
        back = rotation.apply_t(result.Q)
        target.data = back.reshape(target.shape).to(target.dtype)
        if bias_correction:
            shift = ((weight - back) * self.mean).sum(dim=1)
            self.layer.bias.data += shift.to(self.layer.bias.dtype)
        result.rotation = rotation
        return result

    def quantize(self, nbits, scaling_mode="mse", order_mode="diag", bias_correction=False, damp=0.01, nb_ls_moves=0,
                 grid_size=100, min_factor=0.05, max_factor=1.0, scale=None, rotation=None, offsets=None, group_size=None):
        """The layer's weight replaced by its `nbits` quantization, in place (statistics.py:146-190).

        bias_correction: quantize against H - mean mean^T and move the expected output shift into the bias.
        `scale` (optional, (out,) float32): this per-row scale instead of the scale search.
        group_size (optional): one scale per row and per group of `group_size` input features (sleekit_amd.groups):
        compute_group_scaling, then quantize_grouped; `scale`, if given, is then the (out, features / group_size) group
        scales.  Local search and the "obq" scaling mode are not available with group scales.
        offsets (optional, with group_size): an offset per row and group beside the scale (the asymmetric group quantizer
        of sleekit_amd.groups): "mid" for each group's midpoint, or an (out, features / group_size) array used as given;
        the scale search then runs on the centred weight.  The result carries S and O (result.S, result.O) beside idx.
        rotation (optional, a sleekit_amd.Rotation R over the layer's features): everything above runs on (W R, R^T H R); the
        layer's weight becomes Q R^T, while result.Q, idx and the scales stay in the rotated basis and result.rotation is R
        (what RotatedLinear.from_result wraps the stored layer in).  A `scale` given is a scale of W R.  None: no
        rotation (the object's `rotation` attribute is quantize_mxfp4's alone).
        """
        if offsets is not None and group_size is None:
            raise ValueError("offsets need group_size: an offset per row and group of input features")
        return self._quantize(False, nbits, scaling_mode, order_mode, bias_correction, damp, nb_ls_moves, grid_size, min_factor,
                              max_factor, scale, group_size, offsets, rotation)

    def _quantize(self, keep_scales, nbits, scaling_mode, order_mode, bias_correction, damp, nb_ls_moves, grid_size, min_factor,
                  max_factor, scale, group_size, offsets, rotation=None):
        """`quantize`; keep_scales (quantize_packed): the result carries the scales it was made with on every path."""
        rotation = self._check_rotation(rotation)
        if group_size is not None:
            return self._quantize_grouped(nbits, scaling_mode, order_mode, bias_correction, damp, nb_ls_moves, grid_size, min_factor,
                                          max_factor, scale, group_size, offsets, keep_scales, rotation)
        codebook = UniformCodebook(2**nbits, -1, 1)
        weight, H = self._weight_and_hessian(bias_correction, rotation)
        if scale is None:
            scale = compute_scaling(weight, codebook, H=H, mode=scaling_mode, grid_size=grid_size, min_factor=min_factor,
                                    max_factor=max_factor)
        scale = dev.to_device(scale)
        result = engine.quantize_layer(weight, H, codebook, scale, order_mode, damp, nb_ls_moves)
        if keep_scales:
            result.S = scale
        return self._store(result, weight, bias_correction, rotation)

    def _quantize_grouped(self, nbits, scaling_mode, order_mode, bias_correction, damp, nb_ls_moves, grid_size, min_factor,
                          max_factor, scale, group_size, offsets=None, keep_scales=False, rotation=None):
        from . import groups

        if nb_ls_moves > 0:
            raise NotImplementedError("local search with group scales is not supported (nb_ls_moves must be 0)")
        if scaling_mode == "obq":
            raise NotImplementedError('the "obq" scaling mode is not supported with group scales')
        codebook = UniformCodebook(2**nbits, -1, 1)
        weight, H = self._weight_and_hessian(bias_correction, rotation)
        search = dict(H=H, mode=scaling_mode, grid_size=grid_size, min_factor=min_factor, max_factor=max_factor)
        if isinstance(offsets, str):
            if offsets != "mid":
                raise ValueError(f'offsets must be "mid" or an (out, features / group_size) array, not "{offsets}"')
            # the midpoints and the centred weight in one pass; the scale search of the centred weight is the search with offsets
            offsets, centred = groups.compute_group_offsets(weight, group_size, centred=True)
            if scale is None:
                scale = groups.compute_group_scaling(centred, codebook, group_size, **search)
            del centred
        elif offsets is not None:
            offsets = dev.to_device(offsets)
        if scale is None:
            scale = groups.compute_group_scaling(weight, codebook, group_size, offsets=offsets, **search)
        scale = dev.to_device(scale)
        result = groups.quantize_layer_grouped(weight, scale, codebook, H, group_size, order_mode, damp, offsets=offsets)
        if offsets is not None:
            result.S, result.O = scale, offsets
        elif keep_scales:
            result.S = scale
        return self._store(result, weight, bias_correction, rotation)

    def quantize_packed(self, nbits, scaling_mode="mse", order_mode="diag", bias_correction=False, damp=0.01, nb_ls_moves=0,
                        grid_size=100, min_factor=0.05, max_factor=1.0, scale=None, rotation=None, offsets=None, group_size=None):
        """`quantize` with the same arguments and the same result, which also carries its scales on EVERY path: result.S is
        (out,) per row or (out, features / group_size) grouped, result.O the group offsets when there are any -- what
        packing.PackedLinear.from_result packs beside result.idx.  (`quantize` keeps the scales of the offset path only.)"""
        if offsets is not None and group_size is None:
            raise ValueError("offsets need group_size: an offset per row and group of input features")
        return self._quantize(True, nbits, scaling_mode, order_mode, bias_correction, damp, nb_ls_moves, grid_size, min_factor,
                              max_factor, scale, group_size, offsets, rotation)

    def quantize_mxfp4(self, scale_mode="mse", order_mode="diag", bias_correction=False, damp=0.01, nb_ls_moves=0):
        """The layer's weight replaced by its MXFP4 quantization, in place (sleekit_amd.mx): power-of-two scales per block of
        32 input features (scale_mode "max", "mse" or "diag"), FP4 E2M1 elements, nb_ls_moves of the local search after the
        loop.  bias_correction as in `quantize`.  The result (the grouped loop's) carries S, and the packed form as
        result.codes (uint8 (out, features / 2)) and result.scales (E8M0 bytes (out, features / 32)).  The object's rotation
        (`Sleekit(layer, rotation=R)`, or `st.rotation = R`; `st.rotation = None` turns it off) applies as in `quantize`:
        the blocks of 32 are then blocks of rotated features.  (This method's parameter list is kept as it was: the rotation is not a keyword here.)"""
        from . import mx

        rotation = self._check_rotation(self.rotation)
        weight, H = self._weight_and_hessian(bias_correction, rotation)
        packed, result = mx.quantize_layer_mxfp4(weight, H, order_mode, damp, scale_mode, nb_ls_moves)
        result.S, result.codes, result.scales = packed.S, packed.codes, packed.scales
        return self._store(result, weight, bias_correction, rotation)

    def quantize_mxfp6(self, scale_mode="mse", order_mode="diag", bias_correction=False, damp=0.01, nb_ls_moves=0):
        """quantize_mxfp4's twin for MXFP6 (sleekit_amd.mx, MXFP6 LAYERS): FP6 E2M3 elements, 6.25 bits a weight, the same scale
        modes, loop, local search, bias correction and rotation.  result.codes is uint8 (out, 3 features / 4)."""
        from . import mx

        rotation = self._check_rotation(self.rotation)
        weight, H = self._weight_and_hessian(bias_correction, rotation)
        packed, result = mx.quantize_layer_mxfp6(weight, H, order_mode, damp, scale_mode, nb_ls_moves)
        result.S, result.codes, result.scales = packed.S, packed.codes, packed.scales
        return self._store(result, weight, bias_correction, rotation)

    def free(self):
        self.layer = self.mean = self.hessian = None
        self.count = 0


class ExpertStatistics:
    """Running statistics of the inputs of E experts of one shape: `hessian` (E, n, n), `mean` (E, n) float32 and `counts` (E,)
    int64, all on the device.  A batch is one grouped call whatever the routing: each expert's statistics are bit for bit
    what `Sleekit.add_batch` makes of that expert's rows, an expert without rows is not touched, and the host reads neither
    the routing nor the counts.  E = 1 with offsets [0, M] is the dense case: a single layer's statistics, also from codes."""

    def __init__(self, num_experts, features, device=None):
        if isinstance(num_experts, bool) or not isinstance(num_experts, int) or not 1 <= num_experts <= _lib.MX_MAX_EXPERTS:
            raise ValueError(f"num_experts must be 1 .. {_lib.MX_MAX_EXPERTS} (got {num_experts!r})")
        if isinstance(features, bool) or not isinstance(features, int) or features < 1:
            raise ValueError(f"features must be a positive int (got {features!r})")
        self.device = torch.device(device) if device is not None else dev.require_gpu()
        if self.device.type != "cuda":
            raise RuntimeError("sleekit_amd.ExpertStatistics accumulates on the GPU")
        self.num_experts, self.features = num_experts, features
        self.hessian = torch.zeros((num_experts, features, features), dtype=torch.float32, device=self.device)
        self.mean = torch.zeros((num_experts, features), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros(num_experts, dtype=torch.int64, device=self.device)

    def _offsets(self, offsets):
        from . import mx

        mx._check_offsets(offsets, self.num_experts)
        return dev.to_device(offsets, torch.int32)

    def _workspace(self, features, rows):
        return dev.scratch(_lib.lib.slk_hessian_experts_workspace_bytes(self.num_experts, features, rows), "expert_stats")

    def _add_rows(self, rows, offsets, also=()):
        """`rows` (M, n) float32 on the device, sorted by expert under the device `offsets`; the flags are read once, after the launches."""
        from . import mx

        M = rows.shape[0]
        flag = torch.empty(1, dtype=torch.int32, device=rows.device)
        ws, ws_bytes = self._workspace(self.features, M)
        _lib.check(_lib.lib.slk_hessian_accumulate_experts(dev.ptr(self.hessian), dev.ptr(self.mean), dev.ptr(rows), dev.ptr(offsets),
                                                            self.num_experts, self.features, M, dev.ptr(self.counts), dev.ptr(flag),
                                                            dev.ptr(ws), ws_bytes, dev.stream_handle()))
        mx._raise_flags(*also, (flag, mx._OFFSETS_RULE))

    def _rows(self, x, what):
        from . import mx

        M, n = mx._matrix(x, what, mx._ACT)
        if n != self.features:
            raise ValueError(f"{what} has {n} columns but the statistics are of {self.features} features")
        return dev.to_device(x, mx._torch_dtype(x)).float().contiguous()

    def add_batch(self, x_sorted, offsets):
        """One batch of rows already sorted by expert: x_sorted (M, n) float32, bfloat16 or float16 (converted to float32 as
        Sleekit.add_batch converts), offsets int32 (E + 1,) as mx.matmul_mx_experts takes them.  Offsets that break the rule
        change nothing and are a ValueError, raised after the launches by one read of the call's flag."""
        rows = self._rows(x_sorted, "x_sorted")
        self._add_rows(rows, self._offsets(offsets))

    def add_tokens(self, x, expert_ids):
        """One batch of routed tokens: x (T, n) and expert_ids (T,) or (T, k), sorted by mx.sort_by_expert's rule on the
        device; a token counts once for each expert it goes to.  Ids outside 0 .. E - 1 are a ValueError (read with the
        call's flag), and nothing is accumulated then: the grouped call is given offsets that break the rule."""
        from . import mx

        rows = self._rows(x, "x")
        T = rows.shape[0]
        if not isinstance(expert_ids, (np.ndarray, torch.Tensor)) or expert_ids.ndim not in (1, 2) or expert_ids.shape[0] != T or \
                (expert_ids.ndim == 2 and expert_ids.shape[1] < 1):
            raise ValueError(f"expert_ids must be ({T},) or ({T}, k) for x of {T} rows; got {tuple(getattr(expert_ids, 'shape', ()))}")
        k = 1 if expert_ids.ndim == 1 else int(expert_ids.shape[1])
        order, offsets, bad = mx._sorted_by_expert(mx._expert_ids(expert_ids, self.num_experts), self.num_experts)
        offsets = offsets - bad  # (bad ids: offsets[0] == -1 breaks the rule on the device, so nothing is accumulated)
        self._add_rows(rows[order // k], offsets, ((bad, mx._ids_message(self.num_experts)),))

    def add_codes(self, a_codes, a_scales, offsets, activations="mxfp8"):
        """One batch of rows that exist as MX codes, sorted by expert: a_codes / a_scales as the activation quantizers and
        mx.matmul_mx_glu* write them, in the format `activations`.  The statistics are those of the de-quantized rows; the
        product is one bfloat16 MFMA pass (every such value is a bfloat16 exactly).  An E8M0 NaN (scale byte 255) is a
        ValueError."""
        from . import mx

        fmt = mx._activations(activations, mx._STATS_CODES_ONLY)
        M, n = mx._act_operands(a_codes, a_scales, fmt)
        if n != self.features:
            raise ValueError(f"a_codes has {n} columns but the statistics are of {self.features} features")
        offsets = self._offsets(offsets)
        ac, asc = (dev.aligned(dev.to_device(t, torch.uint8)) for t in (a_codes, a_scales))
        flag = torch.empty(2, dtype=torch.int32, device=ac.device)
        ws, ws_bytes = self._workspace(32, M)
        _lib.check(_lib.lib.slk_hessian_accumulate_experts_mx(dev.ptr(self.hessian), dev.ptr(self.mean), dev.ptr(ac), dev.ptr(asc), fmt.c_fmt,
                                                               dev.ptr(offsets), self.num_experts, n, M, dev.ptr(self.counts), dev.ptr(flag),
                                                               dev.ptr(ws), ws_bytes, dev.stream_handle()))
        mx._raise_flags((flag[0], mx._OFFSETS_RULE), (flag[1], "a scale byte of the activations is 255: E8M0's NaN"))

    def hessians(self, fill_unseen=True):
        """The (E, n, n) Hessians, what mx.quantize_experts takes.  fill_unseen: an expert that has seen no token gets the
        identity (GPTQ under H = I is round-to-nearest) in place of its zero matrix -- torch ops on the device, no host read."""
        if not fill_unseen:
            return self.hessian
        eye = torch.eye(self.features, dtype=torch.float32, device=self.device)
        return torch.where((self.counts == 0)[:, None, None], eye, self.hessian)

    def free(self):
        self.hessian = self.mean = self.counts = None
