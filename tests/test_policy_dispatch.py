"""The host decisions of the policy-pass dispatch (csrc/policy.hip: the instance
lists, the pass plan, the scratch sizes) against tests/golden/policy_dispatch.json,
recorded by tools/policy_dispatch_record.py from the library of the commit before
the dispatch layer was rewritten (the file names it).  Every kernel instance has a
shape in the sweep; with the kernels themselves unchanged, what a pass computes
can move only through these answers.  No GPU: the entry points are host
arithmetic."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import policy_dispatch_record as R   # noqa: E402

import pass_ref   # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "policy_dispatch.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from mjrl_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _shapes(golden):
    return [tuple(s) for s in golden["shapes"]]


def test_recorded_sweep_covers_every_instance(golden):
    """The committed record holds the sweep the tool defines: a shape for every case
    of pass_ref.CASES (one per kernel instance, as given and as padded), the shapes
    of test_scratch_size_is_monotonic, unsupported shapes, the k_wgrad_all spill
    exception, and every row count of R.TS."""
    assert len(golden["commit"]) == 40
    assert golden["T"] == R.TS
    shapes = set(_shapes(golden))
    for c in pass_ref.CASES:
        assert (c.n, c.m) + tuple(c.hidden) in shapes and (c.n, c.m) + tuple(c.kernel_hidden) in shapes, c.id
    assert set(R.EXTRA_SHAPES) <= shapes
    for mode in R.MODES:
        assert set(golden[mode]) == {R.shape_key(*s) for s in shapes}
        assert any(rec["init"] == -2 for rec in golden[mode].values())    # MJRL_ESHAPE
    # what the record says of the instances the cases anchor agrees with the cases
    for c in pass_ref.CASES:
        rec = golden["default"][R.shape_key(c.n, c.m, *c.kernel_hidden)]
        assert rec["init"] == 0 and rec["shape"][:2] == [c.expect["np"], c.expect["mp"]], c.id
        assert rec["fused_path"] == c.expect["path"], c.id
        assert rec["split_supported"] or c.family != "kx", c.id
    # MJRL_AMD_WGRAD_OLD=1 shows: it takes k_wgrad_all's 256 slices out of the scratch size
    assert golden["default"] != golden["wgrad_old"]


def test_dispatch_matches_the_record(golden, lib):
    """In this process (MJRL_AMD_WGRAD_OLD as the caller has it, unset in the suite)."""
    mode = "wgrad_old" if os.environ.get("MJRL_AMD_WGRAD_OLD", "")[:1] == "1" else "default"
    from mjrl_amd import _lib
    got = R.probe(lib, _shapes(golden), golden["T"], _lib.Shape)
    for key, rec in golden[mode].items():
        assert got[key] == rec, key


@pytest.mark.parametrize("mode", sorted(R.MODES))
def test_dispatch_matches_the_record_in_a_child(golden, lib, mode):
    """Both settings of MJRL_AMD_WGRAD_OLD, each read by a fresh process."""
    got = R.probe_in_child(mode, _shapes(golden))
    for key, rec in golden[mode].items():
        assert got[key] == rec, (mode, key)
