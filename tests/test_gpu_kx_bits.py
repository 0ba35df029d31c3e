"""Every output bit of the split-f16 policy passes (csrc/kx.h k_kx: FWD with the
separate and with the fused pack, FVP; EVAL serial and pipelined, csrc/kxe.h)
against tests/golden/kx_bits.json: a SHA-256 per output array.

The record was written by `tools/kx_bits.py --write` from the build of the commit
before the tile loops' operand scaling was rewritten (profiles/r09a/README.md
names it); the kernels' arithmetic is fixed since, so any later change to them
must leave these bytes alone or replace the record on purpose.  Rows T = 1, 33, 97
(a lone ragged tile; one full tile + 1 row; three full tiles + 1 row) for
(MP, KG) = (32, 12) and (16, 4), T = 33 for the other four instantiations.  The
seeded inputs (tools/kx_bits.py inputs) hold observation columns spanning
1e-6 .. 1e3, an all-zero column, an all-zero observation row, a tangent whose W1
block is all zero (the M = 0 branch of pow2_scale) and a row with |adv| = 1e30.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kx_bits_tool", os.path.join(ROOT, "tools", "kx_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "kx_bits.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN) == sorted(TOOL.case_name(*c) for c in TOOL.CASES)
    shapes = {(mp, kg) for mp, kg, _ in TOOL.CASES}
    assert shapes == set(TOOL.SHAPES) and len(shapes) == 6
    for big in ((32, 12), (16, 4)):
        assert {T for mp, kg, T in TOOL.CASES if (mp, kg) == big} == {1, 33, 97}


@pytest.mark.parametrize("mp,kg,T", TOOL.CASES, ids=[TOOL.case_name(*c) for c in TOOL.CASES])
def test_output_bits(mp, kg, T):
    want = GOLDEN[TOOL.case_name(mp, kg, T)]
    arrays = TOOL.case_arrays(mp, kg, T)
    got = TOOL.digest(arrays)
    # FWD (both packs), FVP (both tangents), EVAL (both kernels): all there
    for k in ("fwd_gsum", "fwd_a0", "fwd_a1", "fwd_mu0", "fwd_ll0", "fwdpack_gsum", "fwdpack_a0", "fwdpack_xs",
              "fwdpack_xu", "fvp_v_gsum", "fvp_v0_gsum", "eval_serial_sums", "eval_serial_rpart", "eval_pipe_sums",
              "eval_pipe_rpart"):
        assert k in got, k
    bad = TOOL.compare(TOOL.case_name(mp, kg, T), got, want)
    assert not bad, "\n".join(bad)
    # and the two EVAL kernels agree with each other
    assert got["eval_pipe_sums"]["sha256"] == got["eval_serial_sums"]["sha256"]
    assert got["eval_pipe_rpart"]["sha256"] == got["eval_serial_rpart"]["sha256"]
