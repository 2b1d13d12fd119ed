"""CPU tests of the backward pass (include/osc_backward.h): the reference adjoint of
tests/backward_ref.py is pinned by central differences of the oracle itself on every env of the
batches tests/test_gpu_backward.py compares on the GPU, the library's formulation (reduced
coordinates, projector onto the active rows' null space) is checked against it in numpy, and the
new C-ABI entry resolves and refuses bad arguments without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import backward_ref as br
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(b, r) for r in br.ROBOTS for b in br.BATCHES]
IDS = [f"{b}-{r}" for b, r in CASES]
H = 1e-4
FD_TOL = 1e-7
NORM_TOL = 1e-5     # the contract of tests/test_gpu_parity.py
# envs left out of the GPU comparison, by name: (batch, robot) -> env indices.  None is needed:
# the reference agrees with the oracle's own differences on every env of every batch.
EXCLUDED: dict = {}


def test_no_env_is_excluded():
    assert all(len(v) <= 0.02 * br.NENV for v in EXCLUDED.values())
    assert EXCLUDED == {}


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_reference_agrees_with_oracle_differences(batch, robot):
    """Every env: |fd - g.d| / (|g| |d|) <= 1e-7 at h = 1e-4, d a random direction of b, gx random
    over all of x (within an active set x* is exactly affine).  An env whose working set leaves no
    free direction has g = 0 exactly (the reference returns <= 1e-26) and the ratio is 0 / 0:
    there the difference itself must vanish to the rounding of the oracle's two optima,
    |fd| <= 8 eps |gx| |x| / h (every such env of `tight`, and only of `tight`).
    Measured: <= 5.4e-10 on the shipped models' batches, <= 5.4e-11 on `absent`, <= 6.1e-9 on
    the envs of `tight` that have a free direction."""
    mdl, d = br.model_of(batch, robot), br.inputs(batch, robot)
    xs, _ = br.oracle(batch, robot)
    gx = br.grad_seed(batch, robot)
    _, gb = br.reference(batch, robot)
    nrm = np.linalg.norm(gb, axis=1)
    rng = np.random.default_rng(99)
    worst, pinned = 0.0, 0
    for e in range(br.NENV):
        dirn = rng.standard_normal(mdl.s)
        fd = br.directional_fd(mdl, *br.env_args(d, e), gx[e], dirn, H)
        if nrm[e] <= 1e-12 * nrm.max():
            pinned += 1
            noise = 8.0 * np.finfo(float).eps * np.linalg.norm(gx[e]) * np.linalg.norm(xs[e]) / H
            assert abs(fd) <= noise, (e, fd, noise)
            continue
        m = abs(fd - gb[e] @ dirn) / (nrm[e] * np.linalg.norm(dirn))
        worst = max(worst, m)
        assert m <= FD_TOL, (e, m)
    print(f"\n{batch} {robot}: worst {worst:.2e}, {pinned} envs without a free direction")
    assert pinned == 0 or batch == "tight"


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_projector_formulation_matches_reference(batch, robot):
    """The library's formulation in numpy (backward_ref.projector_adjoint, one refinement step)
    against the full-space KKT reference on the oracle's duals, in the GPU tests' metric, gx over
    all of x and on tau alone: within the contract on every env.  Measured: <= 5.0e-9 (WaLTER
    standing; 4.9e-6 without the refinement step), <= 1.7e-11 on Go2."""
    mdl, d = br.model_of(batch, robot), br.inputs(batch, robot)
    _, ys = br.oracle(batch, robot)
    for tau_only in (False, True):
        gx = br.grad_seed(batch, robot, tau_only)
        gT, gb = br.reference(batch, robot, tau_only)
        out = [br.projector_adjoint(mdl, *br.env_args(d, e), gx[e], ys[e]) for e in range(br.NENV)]
        eb = br.env_errors(np.array([o[1] for o in out]), gb)
        eT = br.env_errors(np.array([o[0] for o in out]), gT)
        print(f"\n{batch} {robot} tau_only={tau_only}: worst {max(eb.max(), eT.max()):.2e}")
        assert eb.max() <= NORM_TOL and eT.max() <= NORM_TOL, (tau_only, eb.argmax(), eb.max())
        assert np.array_equal(gb, -np.concatenate(
            [gT[:, :, :3].reshape(br.NENV, -1), gT[:, :, 3:].reshape(br.NENV, -1)], axis=1))


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_torque_threshold_rule_names_the_oracle_set(batch, robot):
    """The torque rows' relative threshold (the library's duals carry rounding residues there)
    loses nothing on these batches: on the oracle's duals it names exactly the rows with a
    non-zero multiplier."""
    mdl, d = br.model_of(batch, robot), br.inputs(batch, robot)
    _, ys = br.oracle(batch, robot)
    u0 = mdl.nv + 4 * mdl.nc + mdl.nv
    for e in range(br.NENV):
        tq, _ = br.active_set(mdl, d["mask"][e], ys[e])
        assert np.array_equal(tq, ys[e][u0:u0 + mdl.nu] != 0.0), e


def test_a_seed_on_tau_alone_vanishes_on_most_tight_envs():
    """Why gx covers all of x: with every torque on its bound dL/dT of a loss on tau alone is zero
    identically -- on more than half of the Go2 `tight` envs -- and a test seeded on tau alone
    would pass on zeros there."""
    _, gb = br.reference("tight", "unitree_go2", True)
    zero = np.abs(gb).max(axis=1) <= 1e-12 * np.abs(gb).max()
    _, gb_all = br.reference("tight", "unitree_go2", False)
    zero_all = np.abs(gb_all).max(axis=1) <= 1e-12 * np.abs(gb_all).max()
    print(f"\ntight Go2: {zero.sum()} of {br.NENV} envs with a zero tau-only gradient, "
          f"{zero_all.sum()} with gx over all of x")
    assert zero.sum() > br.NENV // 2 and zero_all.sum() < zero.sum()


def test_backward_symbols_resolve_and_match_header():
    L = _lib.lib()
    text = open(os.path.join(REPO, "include", "osc_backward.h")).read()
    declared = set(re.findall(r"^\s*int\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.BACKWARD_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump


def test_backward_argument_errors_without_a_gpu():
    """A NULL model or nenv < 0 is OSC_ERR_INVALID_ARGUMENT before any device call (a model handle
    needs a device: tests/test_gpu_backward.py repeats the checks with real handles)."""
    L = _lib.lib()
    INVALID = 1
    args = [None] * 8 + [ctypes.c_size_t(0), None]
    assert L.osc_batch_solve_backward(None, 4, *args) == INVALID
    assert L.osc_batch_solve_backward(None, 0, *args) == INVALID
    assert L.osc_batch_solve_backward(None, -1, *args) == INVALID


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                    reason="hipcc not available")
def test_backward_unit_has_no_dpp_hazard_and_no_scratch(tmp_path):
    """csrc/osc_backward.hip as the product build compiles it: tools/check_dpp_hazards.py finds no
    DPP read of a VGPR within two wait states of its VALU write (the unit's DPP statements are the
    interior point's, osc_ipm_ldl.hpp, each with its own guard), and the compiler's resource
    report shows 0 bytes of scratch for both models' kernels."""
    from osc_amd.build import SOURCES, UNIT_FLAGS, compile_flags
    assert "osc_backward.hip" in SOURCES
    out = tmp_path / "osc_backward.s"
    src = os.path.join(REPO, "operational-space-control_amd", "csrc", "osc_backward.hip")
    r = subprocess.run([HIPCC, *compile_flags(), *UNIT_FLAGS.get("osc_backward.hip", []),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        "-o", str(out), src], check=True, capture_output=True, text=True)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert scratch == ["0", "0"], r.stderr[-2000:]
    h = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_dpp_hazards.py"),
                        str(out)], capture_output=True, text=True)
    assert h.returncode == 0 and "0 DPP hazards" in h.stdout, h.stdout[-2000:]
