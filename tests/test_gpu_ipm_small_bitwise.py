"""The one-wave interior point on small batches is bitwise what it was before its iteration loop
was restructured (DESIGN.md §5 "Issue slots"): tests/golden/ipm_small_parent.json holds the
SHA-256 of (tau, x, status, iters, and the warm state where there is one) that the parent commit's
library gave for each case of tests/golden/make_ipm_small_parent.py -- partial last waves, the
split entry points and the single call, warm ticks with a contact-mode switch, an env rejected as
NUMERICAL beside healthy wave-mates, and the stalled joint-state envs' fix-up pass."""
import importlib.util
import json
import os

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_ipm_small_parent", os.path.join(GOLDEN, "make_ipm_small_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ipm_small_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    got = gen.run_case(cid)
    assert got == PARENT[cid], cid
    if cid.startswith("cold-"):
        assert got["single"] == got["split"]


@pytest.mark.parametrize("robot", gen.ROBOTS)
def test_rejected_env_leaves_wave_mates_unchanged(gpu, robot):
    _, bad, good = gen.indefinite(robot)
    torch.cuda.synchronize()
    st = bad.status.cpu().numpy()
    assert st[gen.BAD_ENV] == 2, st   # OSC_SOLVE_NUMERICAL
    mates = [e for e in range(5) if e != gen.BAD_ENV]
    assert (st[mates] == 0).all(), st
    for name in ("tau", "x", "status", "iters"):
        assert torch.equal(getattr(bad, name)[mates], getattr(good, name)[mates]), name
