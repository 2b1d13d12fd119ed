"""CPU tests of the backward pass with respect to the dynamics inputs (include/osc_backward.h,
osc_batch_solve_backward_data): the reference adjoint of tests/backward_data_ref.py is pinned by
central differences of the oracle itself along directions of C, J, M and one site's w_pos on the
batches tests/test_gpu_backward_data.py compares on the GPU; the library's formulation is checked
against it in numpy; the new C-ABI entry resolves and refuses bad arguments without a GPU; and
the new unit compiles for gfx950 without a DPP hazard."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import backward_data_ref as bd
import backward_ref as br
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(b, r) for r in br.ROBOTS for b in br.BATCHES]
IDS = [f"{b}-{r}" for b, r in CASES]
NORM_TOL = 1e-5     # the contract of tests/test_gpu_parity.py
# Central differences at H and H / 2, the step relative to the input's scale (the env's largest
# |entry| of M, J, C; the model's largest w_pos).  x* is not affine in M, J, W, so the difference
# carries an O(h^2) term: both errors are recorded below.
H = 2e-6
# 10 x the worst error at H / 2 over every batch, robot and direction, never looser than 1e-3 (a
# sign, a transposition or a missing term is an O(1) error)
FD_WORST_HALF = 6.1e-7
FD_TOL = min(10.0 * FD_WORST_HALF, 1e-3)
MAX_EXCLUDED = 3    # envs of a batch whose working set moves at theta +- H
DIRECTIONS = ("C", "J", "M", "w_pos")


def same_face(A, nv, rows_a, rows_b):
    """Two working sets name the same face: their one-sided rows (constant rows of A: pyramid and
    box rows; the nv dynamics rows are in every working set) span the same space.  Index sets
    alone would not do: at a contact on the pyramid's apex five rows are active on three forces
    and the oracle's working set holds any independent three of them."""
    a, b = sorted(r for r in rows_a if r >= nv), sorted(r for r in rows_b if r >= nv)
    if a == b:
        return True
    rank = lambda idx: np.linalg.matrix_rank(A[idx]) if idx else 0
    return rank(a) == rank(b) == rank(sorted(set(a) | set(b)))


@functools.lru_cache(maxsize=None)
def fd_errors(batch, robot):
    """direction -> (error at H [NENV], error at H / 2 [NENV], working set moved at +-H [NENV],
    pinned [NENV]); error = |fd - g.d| / (|g| |d|), g the reference gradient of the input the
    direction is in (for w_pos: the three rows' sum against the norm of the env's whole row-weight
    gradient).  pinned: an env whose working set leaves no free direction and whose contact forces
    are zero has g = 0 for J and the weights (below 1e-12 of the batch's largest |g|) and the
    ratio is 0 / 0: there the error is |fd| over the rounding of the oracle's two optima,
    8 eps |gx| |x| / h, times FD_TOL -- within the bar iff the difference itself vanishes to
    rounding (tests/test_backward_ref.py's rule)."""
    mdl, d = br.model_of(batch, robot), br.inputs(batch, robot)
    xs, ys = br.oracle(batch, robot)
    gx = br.grad_seed(batch, robot)
    ref = bd.reference_data(batch, robot)
    rng = np.random.default_rng(1234 + 7 * br.BATCHES.index(batch) + br.ROBOTS.index(robot))
    out = {k: (np.zeros(br.NENV), np.zeros(br.NENV), np.zeros(br.NENV, bool),
               np.zeros(br.NENV, bool)) for k in DIRECTIONS}
    gmax = dict(C=np.abs(ref["C"]).max(), J=np.abs(ref["J"]).max(), M=np.abs(ref["M"]).max(),
                w_pos=np.abs(ref["wrow"]).max())
    for e in range(br.NENV):
        args = br.env_args(d, e)
        M, C, J = args[:3]
        qp = bd.build_qp(mdl, *args)
        base = frozenset(br.working_rows(qp, ys[e]))
        sym = rng.standard_normal(M.shape)
        site = e % mdl.ns
        dirs = dict(C=("C", np.abs(C).max() * rng.standard_normal(C.shape), ref["C"][e]),
                    J=("J", np.abs(J).max() * rng.standard_normal(J.shape), ref["J"][e]),
                    M=("M", np.abs(M).max() * 0.5 * (sym + sym.T), ref["M"][e]),
                    w_pos=(("w_pos", site), mdl.w_pos.max(), None))
        for name, (which, dirn, g) in dirs.items():
            if name == "w_pos":
                g = ref["wrow"][e]
                gd = g[3 * site:3 * site + 3].sum() * dirn
                den = np.linalg.norm(g) * abs(dirn)
            else:
                gd = float(np.ravel(g) @ np.ravel(dirn))
                den = np.linalg.norm(g) * np.linalg.norm(dirn)
            pinned = np.abs(g).max() <= 1e-12 * gmax[name]
            out[name][3][e] = pinned
            for slot, h in ((0, H), (1, 0.5 * H)):
                fd, wp, wm = bd.directional_fd_data(mdl, *args, gx[e], which, dirn, h)
                if pinned:
                    noise = 8.0 * np.finfo(float).eps * np.linalg.norm(gx[e]) * np.linalg.norm(xs[e]) / h
                    out[name][slot][e] = FD_TOL * abs(fd) / noise
                else:
                    out[name][slot][e] = abs(fd - gd) / den
                if slot == 0:
                    out[name][2][e] = not (same_face(qp.A, mdl.nv, wp, base) and
                                           same_face(qp.A, mdl.nv, wm, base))
    return out


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_reference_agrees_with_oracle_differences(batch, robot):
    """Every env, gx random over all of x, central differences of the oracle's optimum at H = 2e-6
    and H / 2 (relative to the input's scale) along a random direction of C, of J, of M (symmetric)
    and of one site's w_pos (site e % ns): |fd - g.d| / (|g| |d|) <= FD_TOL at H / 2.  An env is
    left out of a direction only where the oracle's own working set at theta + H d or theta - H d
    differs from the one at theta -- checked here, at most 3 of 61 per batch over all directions --
    and never out of C's, which is affine.

    Worst errors measured, at H / at H/2, over the envs that are not left out (`out`: envs left
    out of that direction; `zero`: envs with a zero gradient, whose difference vanishes to within
    0.013 of the rounding bound):
      Go2     standing  C 7.3e-12 / 2.0e-11  J 1.3e-9 / 3.2e-10   M 1.5e-7 / 3.7e-8   w_pos 2.2e-10 / 1.7e-10
              tumbling  C 1.6e-11 / 1.7e-11  J 2.9e-10 / 7.2e-11  M 2.1e-7 / 5.3e-8   w_pos 1.9e-10 / 1.8e-10
              tight     C 1.1e-11 / 2.5e-11  J 2.8e-11 / 3.3e-11 (2 zero)  M 2.4e-6 / 6.1e-7 (1 out)
                        w_pos 7.7e-10 / 1.9e-9 (30 zero)
              absent    C 2.6e-11 / 3.7e-11  J 6.1e-10 / 1.5e-10  M 8.5e-9 / 2.1e-9   w_pos 1.2e-10 / 1.8e-10
      WaLTER  standing  C 7.8e-11 / 7.8e-11  J 2.6e-10 / 6.6e-11  M 4.8e-10 / 1.4e-10 w_pos 6.5e-10 / 1.9e-9
              tumbling  C 5.4e-11 / 7.8e-11  J 3.7e-9 / 9.3e-10   M 3.0e-9 / 7.6e-10  w_pos 1.6e-9 / 1.6e-9
              tight     C 1.4e-11 / 2.4e-11  J 2.0e-10 / 4.9e-11  M 9.5e-7 / 2.4e-7 (1 out)
                        w_pos 8.3e-9 / 1.7e-8 (14 zero)
              absent    C 3.8e-11 / 8.7e-11  J 2.0e-7 / 5.0e-8 (1 out)  M 7.7e-9 / 1.9e-9  w_pos 6.7e-10 / 6.8e-10
    Along J and M the error at H/2 is a quarter of the error at H -- the differences' own O(h^2)
    term, converging on the reference; along C (affine) and w_pos it is the rounding of the
    oracle's optima over h.  At most one env of a batch is left out.  (At H = 2e-5 the M errors
    were 100 x these and up to nine envs of a batch crossed to another working set.)"""
    res = fd_errors(batch, robot)
    moved = np.zeros(br.NENV, bool)
    for name in DIRECTIONS:
        eh, eh2, mv, pin = res[name]
        keep = ~mv if name != "C" else np.ones(br.NENV, bool)
        moved |= ~keep
        assert not pin.any() or (batch == "tight" and name in ("J", "w_pos"))
        print(f"\n{batch} {robot} {name}: worst {eh[keep & ~pin].max():.2e} at H, "
              f"{eh2[keep & ~pin].max():.2e} at H/2; {int((~keep).sum())} envs left out "
              f"{np.nonzero(~keep)[0].tolist()}; {int(pin.sum())} envs with a zero gradient")
    print(f"{batch} {robot}: {int(moved.sum())} envs left out over all directions")
    assert moved.sum() <= MAX_EXCLUDED
    for name in DIRECTIONS:
        eh, eh2, mv, _ = res[name]
        keep = ~mv if name != "C" else np.ones(br.NENV, bool)
        assert eh2[keep].max() <= FD_TOL, (name, int(np.argmax(np.where(keep, eh2, 0.0))), eh2[keep].max())


@pytest.mark.parametrize("batch,robot", CASES, ids=IDS)
def test_projector_formulation_matches_reference(batch, robot):
    """The library's formulation in numpy (backward_data_ref.projector_adjoint_data: the first
    entry's w and v, one factored solve with M -- numpy's Cholesky here, an LDL^T in the kernel --
    without a refinement step) against the
    full-space reference on the oracle's optimum, per output in backward_ref.env_errors' metric, gx
    over all of x and on tau alone: within the contract on every env.  Measured, worst per robot:
    Go2 3.8e-9 (dL/dM, `absent`), WaLTER 9.0e-7 (dL/dM and dL/dC, standing); a refinement step of
    the M solve changes neither (the error is v's), so the kernel has none."""
    mdl, d = br.model_of(batch, robot), br.inputs(batch, robot)
    xs, ys = br.oracle(batch, robot)
    for tau_only in (False, True):
        gx = br.grad_seed(batch, robot, tau_only)
        ref = bd.reference_data(batch, robot, tau_only)
        out = [bd.projector_adjoint_data(mdl, *br.env_args(d, e), gx[e], xs[e], ys[e])
               for e in range(br.NENV)]
        for k in bd.OUTPUTS:
            err = br.env_errors(np.array([o[k] for o in out]), ref[k])
            print(f"\n{batch} {robot} tau_only={tau_only} {k}: worst {err.max():.2e}")
            assert err.max() <= NORM_TOL, (tau_only, k, int(err.argmax()), err.max())
        # dL/dT and dL/db are the first entry's reference
        gT, gb = br.reference(batch, robot, tau_only)
        assert np.array_equal(ref["T"], gT) and np.array_equal(ref["b"], gb)


def test_backward_data_symbols_resolve_and_match_header():
    L = _lib.lib()
    text = open(os.path.join(REPO, "include", "osc_backward.h")).read()
    declared = set(re.findall(r"^\s*int\s+(osc_\w+)\s*\(", text, re.M))
    assert "osc_batch_solve_backward_data" in declared
    assert declared == set(_lib.BACKWARD_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    # the header's argument list, in order, against the ctypes prototype
    proto = re.search(r"int\s+osc_batch_solve_backward_data\s*\((.*?)\)\s*;", text, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    assert names == ["model", "nenv", "M", "J", "b", "T", "contact_mask", "x", "y", "status",
                     "grad_x", "grad_M", "grad_C", "grad_J", "grad_wrow", "grad_T", "grad_b",
                     "workspace", "workspace_bytes", "stream"]
    assert len(L.osc_batch_solve_backward_data.argtypes) == len(names)
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump


def test_backward_data_argument_errors_without_a_gpu():
    """A NULL model or nenv < 0 is OSC_ERR_INVALID_ARGUMENT before any device call (a model handle
    needs a device: tests/test_gpu_backward_data.py repeats the checks with real handles)."""
    L = _lib.lib()
    INVALID = 1
    args = [None] * 16 + [ctypes.c_size_t(0), None]
    assert L.osc_batch_solve_backward_data(None, 4, *args) == INVALID
    assert L.osc_batch_solve_backward_data(None, 0, *args) == INVALID
    assert L.osc_batch_solve_backward_data(None, -1, *args) == INVALID


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                    reason="hipcc not available")
def test_backward_data_unit_has_no_dpp_hazard_and_no_scratch(tmp_path):
    """csrc/osc_backward_data.hip as the product build compiles it: two kernels,
    tools/check_dpp_hazards.py finds no DPP read of a VGPR within two wait states of its VALU write
    (the unit's DPP statements are the shared w / v stage's), and the compiler's resource report
    shows 0 bytes of scratch for Go2's kernel.  Reported: Go2 256 VGPRs + 38 AGPRs, 0 bytes of
    scratch, 8,768 bytes of LDS per wavefront; WaLTER 256 VGPRs + 13 AGPRs, 0 bytes of scratch,
    14,144 bytes of LDS -- both at one wavefront per SIMD with the AGPRs as spill space (at two
    waves per SIMD Go2's kernel spills 128 bytes per lane to scratch)."""
    from osc_amd.build import SOURCES, UNIT_FLAGS, compile_flags
    assert "osc_backward_data.hip" in SOURCES
    out = tmp_path / "osc_backward_data.s"
    src = os.path.join(REPO, "operational-space-control_amd", "csrc", "osc_backward_data.hip")
    r = subprocess.run([HIPCC, *compile_flags(), *UNIT_FLAGS.get("osc_backward_data.hip", []),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        "-o", str(out), src], check=True, capture_output=True, text=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(names) == 2 and len(scratch) == 2, r.stderr[-2000:]
    report = dict(zip(("go2" if "DimsILi18E" in n else "walter" for n in names), scratch))
    print("\nscratch bytes per lane:", report)
    assert set(report) == {"go2", "walter"}
    assert report["go2"] == "0", r.stderr[-2000:]
    h = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_dpp_hazards.py"),
                        str(out)], capture_output=True, text=True)
    assert h.returncode == 0 and "0 DPP hazards" in h.stdout, h.stdout[-2000:]
