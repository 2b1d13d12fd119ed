"""What the assembly kernel leaves in the workspace is bitwise what it was before the lean
assembly's hand-off went through LDS and out as one block of 16-byte stores:
tests/golden/setup_parent.json holds the SHA-256 that the parent commit's library gave for each
case of tests/golden/make_setup_parent.py -- the ranges the assembly owns (g, compact Hr, X, H_dv,
f_dv; wheel blocks and raw rows with wheel rows) of a zero-filled workspace after assemble_into,
for Go2 at 1 and 5 envs under three contact masks, an env whose M is not positive definite (NaN
bits), per-env task weights, WaLTER, WaLTER with wheel rows, the two-model call, and Go2 four envs
past the default small_batch_max (first and last four envs of 4,100)."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_setup_parent", os.path.join(GOLDEN, "make_setup_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "setup_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    assert gen.run_case(cid) == PARENT[cid], cid
