"""Local search on group-scaled layers without a GPU: the NumPy model (tests/groups_ls_model.py) against the reference's
own moves (tests/golden/groups_ls.npz, tests/golden/make_golden_groups_ls.py), and the library's new entry point."""

import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from groups_ls_model import local_search_grouped, trace_of  # noqa: E402
from groups_model import oracle_grid, rebuild  # noqa: E402
from ls_evidence import explain_rows  # noqa: E402
from sleekit_amd import synth  # noqa: E402

FIX = np.load(os.path.join(HERE, "golden", "groups_ls.npz"))
META = json.loads(str(FIX["meta"]))
CASES = META["cases"]


def case_inputs(i):
    """W, H (float32), S, Q0 of fixture case i, Q0 rebuilt from its indices."""
    c = CASES[i]
    L = synth.make_layer(c["R"], c["n"], c["seed"])
    if c["zero_group"] is not None:
        z, g = c["zero_group"], c["g"]
        L["W"][:, z * g:(z + 1) * g] = 0
    S = FIX[f"S_{i}"]
    Q0 = rebuild(FIX[f"idx0_{i}"], S, c["codebook"], c["g"])
    return L["W"].astype(np.float32), L["H"].astype(np.float32), S, Q0


def near(i):
    return {k: FIX[f"near_{i}/{k}"] for k in ("rows", "choice", "runner", "ratio")}


def row_hashes(idx):
    import hashlib

    return np.array([int.from_bytes(hashlib.sha256(np.ascontiguousarray(r).tobytes()).digest()[:8], "little") for r in idx],
                    dtype=np.uint64)


def check_against_fixture(i, idx, trace):
    """idx: the searched indices; trace: the moves taken.  Rows must match the reference's, or be proven near-ties."""
    c = CASES[i]
    bad = np.flatnonzero(row_hashes(idx) != FIX[f"row_hash_{i}"])
    if f"idx_{i}" in FIX:
        assert np.array_equal(np.flatnonzero((idx != FIX[f"idx_{i}"]).any(axis=1)), bad)
    explain_rows(bad, trace, near(i))
    return len(bad), c


def model_indices(i):
    c = CASES[i]
    W, H, S, Q0 = case_inputs(i)
    grd = oracle_grid(c["codebook"])
    records = []
    Q = local_search_grouped(W, Q0, S, grd, H, c["g"], c["moves"], records)
    s = np.repeat(S, c["g"], axis=1)
    return grd.index(Q / s).astype(np.uint8), trace_of(records), Q, S, c


def test_fixture_cover():
    gs = {c["g"] for c in CASES}
    ns = {c["n"] for c in CASES}
    assert {1, 32, 128} <= gs and any(g % 2 == 1 and g > 1 for g in gs) and any(c["g"] == c["n"] for c in CASES)
    assert {96, 172, 768, 1024, 3072} <= ns
    assert {"2", "3", "8", "16", "nf4"} <= {c["codebook"] for c in CASES}
    assert {1, 10, 100} <= {c["moves"] for c in CASES}
    assert any(c["zero_group"] is not None for c in CASES)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_model_follows_the_reference(i):
    idx, trace, Q, S, c = model_indices(i)
    differ, _ = check_against_fixture(i, idx, trace)
    assert differ <= len(near(i)["rows"])
    # the indices rebuild the searched values bit for bit (the search only moves between group-quantizer values)
    back = rebuild(idx, S, c["codebook"], c["g"])
    assert np.array_equal(back.view(np.uint32), Q.view(np.uint32))


def test_zero_moves_return_the_input():
    W, H, S, Q0 = case_inputs(0)
    assert local_search_grouped(W, Q0, S, oracle_grid(CASES[0]["codebook"]), H, CASES[0]["g"], 0) is Q0


def test_library_exports_the_grouped_search():
    from sleekit_amd import _lib, groups

    assert _lib.lib.slk_abi_version() == 8
    assert hasattr(_lib.lib, "slk_local_search_grouped")
    assert callable(groups.local_search_grouped)
    import inspect

    params = list(inspect.signature(groups.quantize_grouped).parameters)
    assert params[-2:] == ["return_indices", "nb_ls_moves"]
    assert "nb_ls_moves" in inspect.signature(groups.quantize_layer_grouped).parameters
