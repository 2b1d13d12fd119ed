"""CPU preconditions of tests/test_gpu_descriptors.py, from the oracle alone: every env of every
descriptor variant (tests/desc_variants.py) certifies, and enough rows of every kind are active
at the optimum that a GPU kernel with one row wrong cannot pass -- floors, so a later change to
the synthetic inputs cannot quietly empty the GPU tests.

Counts measured with oracle/qp_exact.py's start made strictly interior for any box, as
(Go2, WaLTER) over 61 envs:

  model    u_lo      u_hi      pyramid   fz_lo     fz_hi
  tight    362, 225  350, 249  216, 437  74, 130   99, 182
  absent   118, 95   111, 87   201, 393  28, 53    0, 0
  lifted   343, 213  304, 181  356, 669  57, 132   101, 153
"""
import numpy as np
import pytest

import desc_variants as dv
from osc_amd.synth import SEED_BASE, generate
from osc_qp import build_qp, load_model

FLOORS = {"tight": dict(u_lo=150, u_hi=150, pyramid=150, fz_lo=40, fz_hi=75),
          "lifted": dict(u_lo=150, u_hi=150, pyramid=150, fz_lo=40, fz_hi=75),
          "absent": dict(u_lo=60, u_hi=60, pyramid=150, fz_lo=20)}


@pytest.mark.parametrize("robot", dv.ROBOTS)
@pytest.mark.parametrize("name", dv.NAMES)
def test_variant_certifies_and_covers_every_row_kind(name, robot):
    x, _ = dv.oracle(name, robot)          # raises on an env that does not certify
    assert x.shape == (dv.NENV, dv.model(name, robot).n)
    got = dv.active_counts(dv.model(name, robot), dv.inputs(name, robot)["mask"], x)
    print(f"\n{name} {robot}: {got}")
    for k, floor in FLOORS[name].items():
        assert got[k] >= floor, (name, robot, k, got)
    if name == "absent":
        assert got["fz_hi"] == 0, got


def test_tight_mask_is_fractional():
    for robot in dv.ROBOTS:
        assert set(np.unique(dv.inputs("tight", robot)["mask"])) == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("robot", dv.ROBOTS)
def test_pinned_variant_certifies(robot):
    """l == u on one torque: an equality row to the oracle (OSQP in the reference handles it)."""
    mdl = dv.model("pinned", robot)
    x, _ = dv.oracle("pinned", robot)
    assert np.abs(x[:, mdl.nv + 2] - 1.5).max() <= 1e-12


def test_overrides_refuse_unknown_fields_and_keep_the_shipped_qp():
    with pytest.raises(KeyError):
        load_model("unitree_go2", overrides={"friction": 0.5})
    for robot in dv.ROBOTS:
        d = generate(robot, 1, SEED_BASE + 7100, "tumbling", "bernoulli")
        a = [d[k][0] for k in ("M", "C", "J", "b", "T", "mask")]
        base, same = load_model(robot), load_model(robot, overrides={})
        for f in ("H", "f", "A", "l", "u"):
            np.testing.assert_array_equal(getattr(build_qp(base, *a), f), getattr(build_qp(same, *a), f))


def test_shipped_batches_leave_row_kinds_inactive():
    """The gap the variants close, on 32 envs of the seeds and scenarios of two
    test_fresh_batch_vs_oracle batches (Go2 standing 7001, WaLTER tumbling 7004): the fz cap (1e4)
    is never active, and WaLTER's torque bounds (+-1000) never are; Go2's torque bounds are 239
    times and pyramid rows 376 times.  (The batches are generated at 32 envs, which is where
    these figures come from; the generator draws whole arrays, so these are not the first 32 of
    the 128-env batches -- among those, one WaLTER torque sits at +1000 and the fz cap is as
    inactive.)"""
    got = {}
    for robot, scenario, mask_mode, seed in (("unitree_go2", "standing", "ones", 7001),
                                             ("walter_sr", "tumbling", "bernoulli", 7004)):
        d = generate(robot, 32, SEED_BASE + seed, scenario, mask_mode)
        mdl = load_model(robot)
        x, _ = dv.solve_oracle(mdl, d)
        got[robot] = dv.active_counts(mdl, d["mask"], x)
    print(f"\n{got}")
    assert got["unitree_go2"]["fz_hi"] == 0 and got["walter_sr"]["fz_hi"] == 0, got
    assert got["walter_sr"]["u_lo"] + got["walter_sr"]["u_hi"] == 0, got
    assert got["unitree_go2"]["u_lo"] + got["unitree_go2"]["u_hi"] > 0, got
    assert got["unitree_go2"]["pyramid"] + got["walter_sr"]["pyramid"] > 0, got
