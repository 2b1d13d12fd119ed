"""The Go2 one-wave interior point is bitwise what it was before its start (iteration -1, the
least-squares initial point) was peeled out of the iteration loop (DESIGN.md §5 "The start,
peeled"): tests/golden/ipm_start_parent.json holds the SHA-256 of (tau, x, status, iters, and
where the entry has them the duals and the warm state) that the parent commit's library gave for
each case of tests/golden/make_ipm_start_parent.py -- cold solves at 1, 3, 4, 5 and 61 envs with
the contact mask all ones, Bernoulli and all zeros, warm ticks on all-warm waves (start skipped)
and on waves mixing warm and cold envs (start runs, warm rows take over), max_iter 0, 1 and 2, an
invalid env of the _env entry beside valid wave-mates, the two-model call, and envs that take a
second refinement round beside one-round wave-mates."""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_ipm_start_parent", os.path.join(GOLDEN, "make_ipm_start_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ipm_start_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    assert gen.run_case(cid) == PARENT[cid], cid


def test_invalid_env_alone_is_numerical(gpu):
    st = gen.env_invalid()[1]
    assert st[gen.BAD_ENV] == 2, st   # OSC_SOLVE_NUMERICAL
    assert (np.delete(st, gen.BAD_ENV) == 0).all(), st


def test_cold_envs_change_the_mixed_wave_only_from_their_tick_on(gpu):
    """The mixed case really mixes: tick 0 (all cold) agrees with the all-warm run, tick 1 (envs
    1 and 2 cold again) does not."""
    w, m = gen.warm(4), gen.warm(4, gen.WARM_COLD_ENVS)
    assert w["tick0"] == m["tick0"]
    assert w["tick1"] != m["tick1"]
