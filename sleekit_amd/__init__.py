"""sleekit_amd: MI355X-native GPTQ/OBQ layer quantization behind the sleekit function surface.

    from sleekit_amd import obq, scaling, codebook, groups, packing, mx, rotation, Sleekit, MXLinear, MXExperts, PackedLinear
    from sleekit_amd import MXGatedMLP, MXExpertsMLP, ExpertStatistics
    from sleekit_amd import Rotation, RotatedLinear
    from sleekit_amd import routing, route_topk, sort_experts

mirrors `sleekit.obq`, `sleekit.scaling`, `sleekit.codebook` and `sleekit.Sleekit` of
Coloquinte/sleekit for the hot path.  Submodules are imported lazily
so that `sleekit_amd.synth` (pure NumPy test-data generation) stays importable before the
HIP library is built; everything else needs libsleekit_amd.so and fails loudly without it.
"""

import importlib

# (Streams only overlap when they sit in different hardware queues, DESIGN.md "Hardware queues".  The package leaves the
# queue count to the process environment: the GPU is shared, and more queues per process than the machine allows are not
# ours to take.)

_SUBMODULES = ("codebook", "obq", "scaling", "statistics", "engine", "dist", "synth", "groups", "packing", "mx", "rotation", "routing", "_lib", "_device")


def __getattr__(name):
    if name in _SUBMODULES:
        return importlib.import_module(f"{__name__}.{name}")
    if name in ("Sleekit", "ExpertStatistics"):
        return getattr(importlib.import_module(f"{__name__}.statistics"), name)
    if name in ("MXLinear", "MXExperts", "MXGatedMLP", "MXExpertsMLP"):
        return getattr(importlib.import_module(f"{__name__}.mx"), name)
    if name in ("route_topk", "sort_experts", "Routing"):
        return getattr(importlib.import_module(f"{__name__}.routing"), name)
    if name == "PackedLinear":
        return importlib.import_module(f"{__name__}.packing").PackedLinear
    if name in ("Rotation", "RotatedLinear"):
        return getattr(importlib.import_module(f"{__name__}.rotation"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
