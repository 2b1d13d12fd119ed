"""CPU tests of the plant's reference (tests/plant_ref.py) and of the binding of
include/osc_plant.h: what tests/test_gpu_plant.py measures the GPU against is itself checked here,
on the oracle, and the new entries' argument errors come back without a device.
   1. a matched plant reproduces the QP's own acceleration to rounding;
   2. the behaviour the feature exists for: a payload the controller does not know, and a push;
   3. the numpy model of the kernel's LDL' and the bar it sets;
   4. the binding: the header's declarations, the struct, the refusals, the no-ground sentence."""
import ctypes
import os
import re

import numpy as np
import pytest

import plant_ref as pr
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_plant.h")
K_MATCHED = 20


# ---- 1. matched plant -----------------------------------------------------------------------------------

def test_matched_plant_reproduces_dv():
    """go2_case, K = 20: |qacc - dv|_inf <= 1e-11 max(1, |dv|_inf) at every tick -- the QP's
    dynamics row is an equality, so M^-1 (B u + Jc' z - C) is its dv up to the solves' rounding
    (measured: 7.5e-14 over 100 ticks)."""
    r = pr.go2_behaviour("matched")
    worst = 0.0
    for t in range(K_MATCHED):
        d = np.abs(r["qacc"][t] - r["dv"][t]).max()
        worst = max(worst, d)
        assert d <= 1e-11 * max(1.0, np.abs(r["dv"][t]).max()), (t, d)
    print(f"\nmatched plant: max |qacc - dv| over {K_MATCHED} ticks {worst:.2e}")


# ---- 2. behaviour -----------------------------------------------------------------------------------------

def z_error(r):
    return float(r["qpos"][-1][2] - r["pos_ref"][2])


def test_an_unknown_payload_sags_and_a_known_one_does_not():
    """go2_case, K = 100.  The trunk 1.5 x heavier in the plant only: the base ends below its
    reference (z error < -0.005; measured -0.00745).  Matched, and both 1.5 x: still above it and
    converging (> +0.005; measured +0.00646 for both) -- the controller compensates for a mass it
    knows."""
    ez = {w: z_error(pr.go2_behaviour(w)) for w in ("matched", "plant", "both")}
    print(f"\nz error after 100 ticks: {ez}")
    assert ez["plant"] < -0.005
    assert ez["matched"] > 0.005 and ez["both"] > 0.005


def test_a_push_moves_the_base():
    """30 N along x over ticks 10..19 moves the final base x by more than 5e-4 against no push
    (measured 9.6e-4)."""
    dx = float(pr.go2_behaviour("push")["qpos"][-1][0] - pr.go2_behaviour("matched")["qpos"][-1][0])
    print(f"\nfinal base x, push against no push: {dx:.3e}")
    assert abs(dx) > 5e-4


# ---- 3. the LDL' model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("robot", [pr.GO2, pr.WALTER])
def test_ldl_model_error_sets_the_bar(robot):
    """The float64 model of the kernel's unpivoted LDL' on the GPU test's own inputs (67 envs, drawn
    inertial parameters) against the refined reference: its worst error x 10 is the GPU test's bar,
    which must lie below cond(M) n eps with margin (1e-10) for that test to mean anything; numpy's
    pivoted LU on the same inputs is printed next to it."""
    c = pr.fd_case(robot)
    mdl = pr.load_model(robot)
    lu = max(pr.fd_error(pr.forward_dynamics(mdl, c["M"][e], c["C"][e], c["J"][e], c["u"][e],
                                             c["z"][e], c["qfrc"][e]), c["ref"][e])
             for e in range(len(c["ref"])))
    print(f"\n{robot}: cond(M) <= {c['cond'].max():.2e}, ldl_model worst {c['model_err'].max():.2e},"
          f" numpy LU worst {lu:.2e}, |qacc| <= {np.abs(c['ref']).max():.1f}, bar {pr.fd_bar(robot):.2e}")
    assert np.isfinite(c["ref"]).all() and c["model_err"].max() > 0
    assert 10 * c["model_err"].max() <= pr.FD_BAR_MAX
    assert c["cond"].max() * mdl.nv * np.finfo(float).eps <= pr.FD_BAR_MAX


def test_ldl_model_refuses_an_indefinite_matrix():
    c = pr.fd_case(pr.GO2)
    M = np.array(c["M"][0])
    M[4, 4] = -M[4, 4]
    assert np.isnan(pr.ldl_model(M, np.ones(len(M)))).all()


# ---- 4. the library's boundary ---------------------------------------------------------------------------

def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.PLANT_SYMBOLS) and len(declared) == 3
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS) |
                           set(_lib.KIN_ENV_SYMBOLS) | set(_lib.KIN_BACKWARD_SYMBOLS) |
                           set(_lib.ROLLOUT_BACKWARD_SYMBOLS) | set(_lib.ROLLOUT_SCHEDULE_SYMBOLS))
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump
    body = re.search(r"typedef struct \{([^}]*)\} osc_rollout_plant;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in _lib.OscRolloutPlant._fields_]
    assert ctypes.sizeof(_lib.OscRolloutPlant) == 32           # the unit's static_assert
    unit = open(os.path.join(REPO, "operational-space-control_amd", "csrc",
                             "osc_rollout.hip")).read()
    assert re.search(r"sizeof\(osc_rollout_plant\) == 32", unit)
    assert ctypes.sizeof(_lib.OscRolloutArgs) == 184           # the block it rides on is unchanged
    from osc_amd.build import SOURCES
    assert "osc_forward_dynamics.hip" in SOURCES


def test_the_header_says_there_is_no_ground():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    assert "The contact forces are still whatever the QP chose, applied to the plant as given " \
        "forces; there is still no ground." in text
    for what in ("gradients through the plant", "wrench on an arbitrary body",
                 "constraint reactions", "two-model grids", "host feeds", "controller shim",
                 "wheel rows"):
        assert what in text, what


def test_refusals_come_back_without_a_device():
    """Every new entry refuses NULL handles (and what it can check before it needs them) without
    touching a device."""
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.osc_batch_forward_dynamics(None, 4, p, p, p, p, 12, p, 12, p, p, None) == 1
    assert L.osc_batch_forward_dynamics(None, 0, None, None, None, None, 0, None, 0, None, None,
                                        None) == 1
    nb = ctypes.c_size_t(7)
    assert L.osc_rollout_plant_workspace_bytes(None, None, 4, 4, ctypes.byref(nb)) == 1
    assert L.osc_rollout_plant_workspace_bytes(None, None, 4, 4, None) == 1
    assert nb.value == 7
    ra, pl = _lib.OscRolloutArgs(), _lib.OscRolloutPlant()
    assert L.osc_batch_rollout_plant(None, None, 4, ctypes.byref(ra), None, None, None,
                                     ctypes.byref(pl), None) == 1
    pl.qfrc_applied = ctypes.addressof(buf)
    assert L.osc_batch_rollout_plant(None, None, 4, ctypes.byref(ra), None, None, None,
                                     ctypes.byref(pl), None) == 1
    assert L.osc_batch_rollout_plant(None, None, 4, None, None, None, None, None, None) == 1
