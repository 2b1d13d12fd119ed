"""The interior point is bitwise what it was before the refresh of the rows' residual was restricted
to the envs that go on iterating, and before that block and the re-centring ahead of it became
branch-free in the one-wave kernels (DESIGN.md §5 "The refresh of the rows' residual"):
tests/golden/ipm_fresh_parent.json holds the SHA-256 of (tau, x, status, iters, and where the entry
has them the duals and the warm state) that the parent commit's library gave for each case of
tests/golden/make_ipm_fresh_parent.py -- Go2 cold at 1, 3, 4, 5 and 61 envs with the contact mask
all ones, Bernoulli and all zeros, a wave whose envs stop at least 3 iterations apart, a wave
re-centred at a low restart_iter beside a done wave-mate, max_iter 0, 1 and 2, warm ticks on an
all-warm wave and on one mixing warm and cold envs, an invalid env of the _env entry beside valid
wave-mates, WaLTER at 4 and 5 envs, the two-wave Go2 kernel, the two-model call, and envs that
take a second refinement round beside one-round wave-mates."""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location(
    "make_ipm_fresh_parent", os.path.join(GOLDEN, "make_ipm_fresh_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "ipm_fresh_parent.json")) as _f:
    PARENT = json.load(_f)["cases"]


def test_every_case_has_a_parent_hash():
    assert sorted(PARENT) == sorted(gen.case_ids())


def test_parent_spread_wave_stops_iterations_apart():
    """On the parent, the spread wave's envs stop at least SPREAD_MIN iterations apart: the refresh
    that is now skipped ran beside done wave-mates."""
    it = PARENT["spread"]["iters"]
    assert len(it) == 4 and max(it) - min(it) >= gen.SPREAD_MIN, it
    assert gen.spread_ok(PARENT["spread"])


def test_parent_restart_wave_recentres_beside_a_done_env():
    """On the parent, an env of the restart wave is done before RESTART_ITER and the re-centring
    there changes another env's iteration count."""
    assert gen.restart_ok(PARENT["restart"]), PARENT["restart"]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", gen.case_ids())
def test_bitwise_equal_to_parent(gpu, cid):
    assert gen.run_case(cid) == PARENT[cid], cid


@pytest.mark.gpu
def test_invalid_env_alone_is_numerical(gpu):
    st = gen.env_invalid()[1]
    assert st[gen.BAD_ENV] == 2, st   # OSC_SOLVE_NUMERICAL
    assert (np.delete(st, gen.BAD_ENV) == 0).all(), st


@pytest.mark.gpu
def test_cold_envs_change_the_mixed_wave_only_from_their_tick_on(gpu):
    """The mixed case really mixes: tick 0 (all cold) agrees with the all-warm run, tick 1 (envs
    1 and 2 cold again) does not."""
    w, m = gen.warm(), gen.warm(gen.WARM_COLD_ENVS)
    assert w["tick0"] == m["tick0"]
    assert w["tick1"] != m["tick1"]
