"""CPU tests of the closed-loop rollout (include/osc_rollout.h): the reference loop built from
the oracle closes (Go2 converges onto its base reference), and the new C-ABI entries resolve and
refuse bad arguments without a GPU."""
import ctypes
import os
import re

import numpy as np

import rollout_ref
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_go2_closed_loop_converges_on_the_oracle():
    """Go2, standing gains, dt 0.002, base reference (0.01, -0.01, -0.02) m away: after 300 ticks
    the base-position error is <= 0.03 x its initial value (measured 0.0030; 0.69 at 50 ticks, so
    a loop that stalls fails)."""
    km, model, qpos, qvel, mask, pd = rollout_ref.go2_case()
    h = rollout_ref.rollout(km, model, qpos, qvel, mask, 300, rollout_ref.DT, pd=pd)
    r50 = rollout_ref.error_ratio(h["qpos"][50], qpos, pd[0])
    r = rollout_ref.error_ratio(h["qpos"][300], qpos, pd[0])
    print(f"\nGo2 oracle rollout: error ratio {r50:.4f} at 50 ticks, {r:.5f} at 300; "
          f"max |tau| {np.abs(h['tau']).max():.2f} N m")
    assert np.isfinite(h["qpos"]).all() and np.isfinite(h["qvel"]).all()
    assert r <= 0.03, r


def test_rollout_symbols_resolve_and_match_header():
    L = _lib.lib()
    text = open(os.path.join(REPO, "include", "osc_rollout.h")).read()
    declared = set(re.findall(r"^\s*int\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.ROLLOUT_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump
    # osc_rollout_args as the header lays it out (LP64): the ctypes twin has the same size
    assert ctypes.sizeof(_lib.OscRolloutArgs) == 184


def test_rollout_argument_errors_without_a_gpu():
    """Every malformed call is OSC_ERR_INVALID_ARGUMENT before any device call.  (A model handle
    needs a device, so here the handles are NULL throughout; tests/test_gpu_rollout.py repeats
    nticks < 0, dt <= 0 and the too-small workspace with real handles.)"""
    L = _lib.lib()
    INVALID = 1
    nb = ctypes.c_size_t()
    assert L.osc_rollout_workspace_bytes(None, None, 4, 3, ctypes.byref(nb)) == INVALID
    assert L.osc_rollout_workspace_bytes(None, None, -1, 3, ctypes.byref(nb)) == INVALID
    assert L.osc_rollout_workspace_bytes(None, None, 4, -1, ctypes.byref(nb)) == INVALID
    assert L.osc_rollout_workspace_bytes(None, None, 4, 3, None) == INVALID
    assert L.osc_batch_integrate(None, 1, 0.002, None, 18, None, None, None, None, None) == INVALID
    assert L.osc_batch_integrate(None, -1, 0.002, None, 18, None, None, None, None, None) == INVALID

    def call(**kw):
        a = _lib.OscRolloutArgs()
        a.nticks, a.dt = 2, 0.002
        nenv = kw.pop("nenv", 4)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.osc_batch_rollout(None, None, nenv, ctypes.byref(a), None)

    assert call() == INVALID                              # NULL handles
    assert call(nenv=-1) == INVALID
    assert call(nticks=-1) == INVALID
    assert call(dt=0.0) == INVALID and call(dt=-0.002) == INVALID
    assert call(workspace=256, workspace_bytes=16) == INVALID   # far too small for any model
    assert L.osc_batch_rollout(None, None, 4, None, None) == INVALID
