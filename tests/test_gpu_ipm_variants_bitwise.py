"""The interior point's kernel variants beside the default small-batch ones are bitwise what they
were before its header was split and its wave body cut into named phases (DESIGN.md §5 "The split
of the wave body"): tests/golden/ipm_variants_parent.json holds the SHA-256 of (tau, x, status,
iters, the duals where asked for, and the warm state where there is one) that the parent commit's
library gave for each case of tests/golden/make_ipm_variants_parent.py -- the wheel rows cold and
warm, the warm start past one wave per SIMD with its separate refinement and fix-up launches,
solves without the refinement, and the duals on the default kernels."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_ipm_variants_parent", os.path.join(GOLDEN, "make_ipm_variants_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ipm_variants_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    assert gen.run_case(cid) == PARENT[cid], cid


def test_wheel_batches_end_ok(gpu):
    for n in gen.WHEEL_NENVS:
        for out in gen.wheels_cold(n)[1]:
            assert (out.status == 0).all(), (n, out.status)
    for st in gen.wheels_warm()[1]:
        assert (st == 0).all(), st


@pytest.mark.parametrize("robot", gen.ROBOTS)
def test_warm_two_wave_ticks_iterate(gpu, robot):
    for it in gen.warm_two_wave(robot)[1][1:]:
        assert (it > 0).any(), it
