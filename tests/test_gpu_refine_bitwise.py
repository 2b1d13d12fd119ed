"""The solves that run the interior point's fused refinement are bitwise what they were before its
step loop was re-scheduled for the one-wave kernels (DESIGN.md §5 "The refinement's steps"):
tests/golden/refine_parent.json holds the SHA-256 of (tau, x, status, iters, and the warm state
where there is one) that the parent commit's library gave for each case of
tests/golden/make_refine_parent.py -- Go2 and WaLTER cold through the single call and the split
entry points at 1, 4, 5 and 67 envs, Go2 warm ticks, envs that take several refinement rounds
beside one-round wave-mates and alone, and a wheel-row and a two-wave batch, which the change
leaves alone."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_refine_parent", os.path.join(GOLDEN, "make_refine_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "refine_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    got = gen.run_case(cid)
    assert got == PARENT[cid], cid
    if cid.startswith("cold-"):
        assert got["single"] == got["split"]


def test_multi_round_envs_do_not_depend_on_their_wave_mates(gpu):
    """Each env of go2_unrefined_joint_states.npz placed in the mixed batch gives, beside its
    one-round wave-mates, the bits it gives alone (nenv = 1) -- and every env ends OK."""
    res, st = gen.multi_round()
    assert (st == 0).all(), st
    for pos in gen.MIXED_AT:
        assert res[f"env{pos}"] == res[f"alone{pos}"], pos
        assert res[f"alone{pos}"] == PARENT["multi_round"][f"alone{pos}"], pos
