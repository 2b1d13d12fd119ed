"""CPU tests of the backward pass with per-env parameters (include/osc_backward_env.h,
osc_batch_solve_backward_env): the reference adjoint of tests/backward_env_ref.py is pinned by
central differences of the oracle itself along directions of the seven per-env fields on
tests/env_params_cases.py's batch, the fz_lb convention is asserted where it applies, the
library's formulation is checked against the reference in numpy, the new C-ABI entry resolves and
refuses bad arguments without a GPU, and the new unit compiles for gfx950 without a DPP hazard."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import backward_env_ref as be
import backward_ref as br
import env_params_cases as ec
from osc_amd import _lib
from test_backward_data_ref import same_face

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_backward_env.h")
NORM_TOL = 1e-5     # the contract of tests/test_gpu_parity.py
# Central differences at H and H / 2, the step relative to the field's scale: 1 for mu, the env's
# fz_ub and fz_lb, the env's largest finite |torque bound|, the model's largest w_pos / w_rot.
H = 1e-5
# 10 x the worst error at H / 2 over both robots and every direction, never looser than 1e-3 (a
# sign, a missing mask or a wrong row is an O(1) error): tests/test_backward_data_ref.py's rule
FD_WORST_HALF = 7.5e-8
FD_TOL = min(10.0 * FD_WORST_HALF, 1e-3)
MAX_EXCLUDED = 3    # envs of a batch whose working set moves at theta +- H, over all directions
DIRECTIONS = ("mu", "fz_ub", "u_lb", "u_ub", "fz_lb", "w_pos", "w_rot")
# the oracle certifies its optimum to this (qp_exact.certified): two optima that should coincide
# differ by no more than it, relative to |gx| |x|
ORACLE_TOL = 1e-8


@functools.lru_cache(maxsize=None)
def fd_errors(robot):
    """direction -> (error at H [NENV], error at H / 2, working set moved at +-H, skipped, pinned),
    error = |fd - g.d| / (|g| |d|) with g the reference gradient of the field the direction is in
    (w_pos / w_rot: one site, against the norm of the env's whole w_pos / w_rot gradient).
    skipped: the direction does not exist for the env (fz_lb on an env with fz_lb = 0:
    test_fz_lb_convention; no finite torque bound on that side).  pinned: the env's gradient of
    the field is zero (below 1e-12 of the batch's largest |g|: an inactive fz_ub, no pyramid row
    active, a working set that leaves no free direction) and the ratio is 0 / 0: there the error is
    |fd| over the rounding of the oracle's two optima, 8 eps |gx| |x| / h, times FD_TOL -- within
    the bar iff the difference itself vanishes to rounding (tests/test_backward_data_ref.py's
    rule)."""
    d, p = ec.inputs(robot), ec.params(robot)
    gx, ref = be.grad_seed(robot), be.reference_env(robot)
    xs, ys = ec.oracle(robot)
    gmax = {k: np.abs(ref[k]).max() for k in DIRECTIONS}
    base_mdl = ec.env_model(robot, p, 0)
    inf = base_mdl.infinity / 1e10
    rng = np.random.default_rng(777 + be.ROBOTS.index(robot))
    out = {k: (np.zeros(be.NENV), np.zeros(be.NENV), np.zeros(be.NENV, bool),
               np.zeros(be.NENV, bool), np.zeros(be.NENV, bool)) for k in DIRECTIONS}
    for e in range(be.NENV):
        _, base, qp = be.loss_at(robot, d, p, e, gx[e])
        assert base == frozenset(br.working_rows(qp, ys[e]))
        site = e % base_mdl.ns
        dirs = {}
        dirs["mu"] = (1.0, ref["mu"][e] * 1.0, abs(ref["mu"][e]))
        dirs["fz_ub"] = (p["fz_ub"][e], ref["fz_ub"][e] * p["fz_ub"][e],
                         abs(ref["fz_ub"][e]) * p["fz_ub"][e])
        if p["fz_lb"][e] > 0.0:
            dirs["fz_lb"] = (p["fz_lb"][e], ref["fz_lb"][e] * p["fz_lb"][e],
                             abs(ref["fz_lb"][e]) * p["fz_lb"][e])
        for k in ("u_lb", "u_ub"):
            fin = np.abs(p[k][e]) < inf
            if fin.any():
                dirn = np.where(fin, np.abs(p[k][e][fin]).max() * rng.standard_normal(fin.shape), 0.0)
                dirs[k] = (dirn, float(ref[k][e] @ dirn),
                           np.linalg.norm(ref[k][e]) * np.linalg.norm(dirn))
        for k in ("w_pos", "w_rot"):
            dirn = np.zeros(base_mdl.ns)
            dirn[site] = getattr(base_mdl, k).max()
            dirs[k] = (dirn, float(ref[k][e] @ dirn), np.linalg.norm(ref[k][e]) * np.abs(dirn).max())
        for name in DIRECTIONS:
            if name not in dirs:
                out[name][3][e] = True
                continue
            dirn, gd, den = dirs[name]
            for slot, h in ((0, H), (1, 0.5 * H)):
                fd, wp, wm = be.directional_fd_env(robot, d, p, e, gx[e], name, dirn, h)
                if np.abs(ref[name][e]).max() <= 1e-12 * gmax[name]:   # (pinned)
                    noise = 8.0 * np.finfo(float).eps * np.linalg.norm(gx[e]) * np.linalg.norm(xs[e]) / h
                    out[name][slot][e] = FD_TOL * abs(fd) / noise
                    out[name][4][e] = True
                else:
                    out[name][slot][e] = abs(fd - gd) / den
                if slot == 0:
                    out[name][2][e] = not (same_face(qp.A, base_mdl.nv, wp, base) and
                                           same_face(qp.A, base_mdl.nv, wm, base))
    return out


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_reference_agrees_with_oracle_differences(robot):
    """Every env, gx random over all of x, central differences of the oracle's optimum at H = 1e-5
    and H / 2 (relative to the field's scale) along mu, fz_ub, a random direction over the finite
    entries of u_lb and of u_ub, fz_lb on the envs with fz_lb > 0, and one site's w_pos and w_rot
    (site e % ns): |fd - g.d| / (|g| |d|) <= FD_TOL at H / 2.  An env is left out of a direction
    only where the oracle's own working set at theta +- H d names another face -- checked here, at
    most 3 of 61 over all directions.

    Worst errors measured, at H / at H/2, over the envs with a non-zero gradient (no env of
    either robot is left out of any direction; `zero`: envs with a zero gradient, whose difference
    vanishes to within 0.01 of the rounding bound):
      Go2     mu 9.1e-10 / 8.6e-10 (2 zero)   fz_ub 3.0e-8 / 7.5e-8 (4 zero)   u_lb 1.7e-10 / 2.6e-10
              u_ub 3.7e-10 / 2.3e-9   fz_lb 7.5e-9 / 1.8e-8 (18 envs, 9 zero)
              w_pos 1.5e-9 / 1.1e-9 (22 zero)   w_rot 2.2e-9 / 5.5e-10 (22 zero)
      WaLTER  mu 9.8e-9 / 2.5e-9   fz_ub 5.3e-10 / 2.3e-9 (1 zero)   u_lb 8.3e-10 / 6.6e-10
              u_ub 1.9e-10 / 3.8e-10   fz_lb 1.8e-9 / 1.5e-9 (26 envs, 5 zero)
              w_pos 2.9e-10 / 4.5e-10 (9 zero)   w_rot 1.1e-9 / 2.7e-10 (9 zero)
    x* is affine in the bounds within a face, so their errors are the rounding of the oracle's
    optima over h and grow as h halves; along mu and the weights the error at H carries the
    differences' O(h^2)
    term."""
    res = fd_errors(robot)
    moved = np.zeros(be.NENV, bool)
    for name in DIRECTIONS:
        eh, eh2, mv, skip, pin = res[name]
        keep = ~mv & ~skip
        moved |= mv
        print(f"\n{robot} {name}: worst {eh[keep & ~pin].max():.2e} at H, "
              f"{eh2[keep & ~pin].max():.2e} at H/2; {int(mv.sum())} envs left out "
              f"{np.nonzero(mv)[0].tolist()}; {int(skip.sum())} envs without the direction; "
              f"{int(pin.sum())} envs with a zero gradient (worst "
              f"{max(eh[keep & pin].max(initial=0.0), eh2[keep & pin].max(initial=0.0)) / FD_TOL:.2g}"
              " of the rounding bound)")
    print(f"{robot}: {int(moved.sum())} envs left out over all directions")
    assert moved.sum() <= MAX_EXCLUDED
    for name in DIRECTIONS:
        eh, eh2, mv, skip, pin = res[name]
        keep = ~mv & ~skip
        assert (keep & ~pin).sum() >= 8, name
        assert eh2[keep].max() <= FD_TOL, (name, int(np.argmax(np.where(keep, eh2, 0.0))), eh2[keep].max())


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_fz_lb_convention(robot):
    """On the envs with fz_lb = 0 the reference gives exactly 0 -- the left derivative at the
    pyramid's apex -- and the oracle's own backward difference (L(theta) - L(theta - h)) / h
    vanishes: |L(theta) - L(theta - h)| <= ORACLE_TOL |gx| |x| (measured: 3.1e-17 |gx| |x| on
    Go2, 4.3e-17 on WaLTER).  On the envs with fz_lb > 0 the row is an ordinary bound
    (test_reference_agrees_with_oracle_differences)."""
    d, p = ec.inputs(robot), ec.params(robot)
    gx, ref = be.grad_seed(robot), be.reference_env(robot)
    xs, _ = ec.oracle(robot)
    zero = np.nonzero(p["fz_lb"] == 0.0)[0]
    assert len(zero) >= 30
    assert (ref["fz_lb"][zero] == 0.0).all()
    worst = 0.0
    for e in zero:
        l0, _, _ = be.loss_at(robot, d, p, e, gx[e])
        l1, _, _ = be.loss_at(robot, d, be.perturbed(p, e, "fz_lb", -H * 5.0), e, gx[e])
        worst = max(worst, abs(l0 - l1) / (np.linalg.norm(gx[e]) * np.linalg.norm(xs[e])))
    print(f"\n{robot}: {len(zero)} envs with fz_lb = 0, worst |L - L(-h)| / (|gx| |x|) {worst:.2e}")
    assert worst <= ORACLE_TOL


def test_every_field_has_gradients_to_check():
    """The batch exercises every field: a non-zero reference gradient on at least 8 envs, and the
    counts of the issue's prototype (Go2 / WaLTER): mu 59 / 61, fz_ub 57 / 60, fz_lb 9 / 21 -- only
    among the 18 / 26 envs with fz_lb = 5 -- and the torque bounds on all 61."""
    want = {"unitree_go2": dict(mu=59, fz_ub=57, fz_lb=9, five=18),
            "walter_sr": dict(mu=61, fz_ub=60, fz_lb=21, five=26)}
    for robot in be.ROBOTS:
        ref, p = be.reference_env(robot), ec.params(robot)
        nz = {k: np.abs(ref[k].reshape(be.NENV, -1)).max(axis=1) > 0.0 for k in be.FIELDS}
        print(f"\n{robot}: " + "  ".join(f"{k} {int(v.sum())}" for k, v in nz.items()))
        for k in be.FIELDS:
            assert nz[k].sum() >= 8, (robot, k)
        five = p["fz_lb"] == 5.0
        assert five.sum() == want[robot]["five"] and not nz["fz_lb"][~five].any()
        for k in ("mu", "fz_ub", "fz_lb"):
            assert nz[k].sum() == want[robot][k], (robot, k, int(nz[k].sum()))
        assert nz["u_lb"].all() and nz["u_ub"].all()
        # no joint has a gradient on both of its bounds
        assert not ((ref["u_lb"] != 0.0) & (ref["u_ub"] != 0.0)).any()


@pytest.mark.parametrize("robot", be.ROBOTS)
def test_kernel_formulation_matches_reference(robot):
    """The library's formulation in numpy (backward_env_ref.kernel_model_env: rho from w and v
    after one refinement step, the Gram-Schmidt's kept rows, the <= 3 x 3 least squares) against
    the full-space reference on the oracle's optimum, in backward_ref.env_errors' metric, gx over
    all of x and on tau alone: within the contract on every env.  Measured, worst over the five
    fields: Go2 2.6e-12 (fz_ub), WaLTER 1.0e-11 (u_lb)."""
    d, p = ec.inputs(robot), ec.params(robot)
    xs, ys = ec.oracle(robot)
    for tau_only in (False, True):
        gx, ref = be.grad_seed(robot, tau_only), be.reference_env(robot, tau_only)
        out = [be.kernel_model_env(ec.env_model(robot, p, e), *br.env_args(d, e), gx[e], xs[e],
                                   ys[e]) for e in range(be.NENV)]
        for k in ("mu", "u_lb", "u_ub", "fz_lb", "fz_ub"):
            err = br.env_errors(np.array([o[k] for o in out]), ref[k])
            print(f"\n{robot} tau_only={tau_only} {k}: worst {err.max():.2e}")
            assert err.max() <= NORM_TOL, (tau_only, k, int(err.argmax()), err.max())


def test_backward_env_symbols_resolve_and_match_header():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.BACKWARD_ENV_SYMBOLS) == {"osc_batch_solve_backward_env"}
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS))
    proto = re.search(r"int\s+osc_batch_solve_backward_env\s*\((.*?)\)\s*;", text, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    assert names == ["model", "nenv", "M", "J", "b", "T", "contact_mask", "env_params", "x", "y",
                     "status", "grad_x", "grad_M", "grad_C", "grad_J", "grad_wrow", "grad_T",
                     "grad_b", "grads", "workspace", "workspace_bytes", "stream"]
    assert len(L.osc_batch_solve_backward_env.argtypes) == len(names)
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump


def test_grads_struct_has_the_header_fields_in_order():
    from osc_amd.solver import EnvGrads, EnvParams
    body = re.search(r"typedef struct \{(.*?)\} osc_env_grads;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"double\*\s+(\w+);", body)
    assert fields == [n for n, _ in _lib.OscEnvGrads._fields_] == list(EnvParams.FIELDS)
    assert EnvGrads.FIELDS == EnvParams.FIELDS
    assert ctypes.sizeof(_lib.OscEnvGrads) == 7 * ctypes.sizeof(ctypes.c_void_p)


def test_backward_env_argument_errors_without_a_gpu():
    """A NULL model or nenv < 0 is OSC_ERR_INVALID_ARGUMENT before any device call, with and
    without the two blocks (tests/test_gpu_backward_env.py repeats the checks with real handles)."""
    L = _lib.lib()
    INVALID = 1
    ep, eg = _lib.OscEnvParams(), _lib.OscEnvGrads()
    for blk, grd in ((None, None), (ctypes.byref(ep), ctypes.byref(eg))):
        args = [None] * 5 + [blk] + [None] * 10 + [grd, None, ctypes.c_size_t(0), None]
        for nenv in (4, 0, -1):
            assert L.osc_batch_solve_backward_env(None, nenv, *args) == INVALID


def test_env_grads_errors_raise_on_the_host():
    import torch
    from osc_amd.robots import dims
    from osc_amd.solver import EnvGrads
    d, n = dims("unitree_go2"), 7
    with pytest.raises(TypeError):
        EnvGrads(mu=np.zeros(n))
    with pytest.raises(ValueError, match="mu"):
        EnvGrads(mu=torch.zeros(n + 1, dtype=torch.float64)).to_struct(n, d, "cpu")
    with pytest.raises(ValueError, match="u_lb"):
        EnvGrads(u_lb=torch.zeros((n, d["nu"]), dtype=torch.float32)).to_struct(n, d, "cpu")
    with pytest.raises(ValueError, match="w_pos"):
        EnvGrads(w_pos=torch.zeros((d["ns"], n), dtype=torch.float64).t()).to_struct(n, d, "cpu")
    c = EnvGrads(fz_ub=torch.zeros(n, dtype=torch.float64)).to_struct(n, d, "cpu")
    assert c.fz_ub and not c.mu


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                    reason="hipcc not available")
def test_backward_env_unit_has_no_dpp_hazard(tmp_path):
    """csrc/osc_backward_env.hip as the product build compiles it: twelve kernels (Go2 and WaLTER,
    with and without the per-env reads, each as the data half, the parameter half and both),
    tools/check_dpp_hazards.py finds no DPP read of a VGPR within two wait states of its VALU
    write, and the compiler's resource report shows 0 bytes of scratch for every kernel (printed).
    Every kernel holds 256 VGPRs at one wavefront per SIMD with the AGPRs as spill space, as
    osc_backward_data.hip; the AGPR counts are in profiles/backward_env/kernel_resources.txt."""
    from osc_amd.build import SOURCES, UNIT_FLAGS, compile_flags
    assert "osc_backward_env.hip" in SOURCES
    out = tmp_path / "osc_backward_env.s"
    src = os.path.join(REPO, "operational-space-control_amd", "csrc", "osc_backward_env.hip")
    r = subprocess.run([HIPCC, *compile_flags(), *UNIT_FLAGS.get("osc_backward_env.hip", []),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                        "-o", str(out), src], check=True, capture_output=True, text=True)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    assert len(names) == 12 and len(scratch) == 12, r.stderr[-2000:]

    def tag(n):     # <Dims<nv, ...>, ENV, DATA, PAR>
        env, data, par = re.search(r"EELb([01])ELb([01])ELb([01])E", n).groups()
        return ("go2" if "DimsILi18E" in n else "walter") + ("-env" if env == "1" else "") + \
            {"11": "-both", "10": "-data", "01": "-par"}[data + par]

    report = dict(zip((tag(n) for n in names), scratch))
    print("\nscratch bytes per lane:", report)
    assert set(report) == {r + e + h for r in ("go2", "walter") for e in ("", "-env")
                           for h in ("-both", "-data", "-par")}
    assert all(v == "0" for v in report.values()), report
    h = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_dpp_hazards.py"),
                        str(out)], capture_output=True, text=True)
    assert h.returncode == 0 and "0 DPP hazards" in h.stdout, h.stdout[-2000:]
