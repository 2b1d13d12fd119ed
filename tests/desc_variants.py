"""Model descriptors other than the shipped YAML files, for tests/test_desc_variants.py (CPU) and
tests/test_gpu_descriptors.py (GPU): the override dict for OSCBatchSolver(desc_overrides=...), the
matching oracle model (oracle/osc_qp.load_model(overrides=...)), the input batch, the oracle's
certified optimum of every env (computed once per process and shared) and the count of rows
active at it.

  tight   torque boxes [-3, 1], [0.5, 4], [-6, -2], [-1, 8] by q % 4 (two exclude 0), fz in
          [0, 30] mask, mu 0.35, w_torque 3e-3, w_reg 2e-3, per-site weights rescaled, and a mask
          of 0 / 0.5 / 1: every row kind active, the fz cap included; no shipped constant survives
  absent  torques one-sided either way or unbounded by q % 3, fz in [0, inf), mu 1.2, infinity
          1e20 (bounds given as +-1e20): rows switched off by the threshold, itself not the
          shipped one
  lifted  torques +-12, fz in [5, 40] mask, mu 0.5: a non-zero fz lower bound
  pinned  tight with u_lb[2] == u_ub[2] == 1.5: a box without interior.  The oracle solves it
          (an equality row); the library refuses it at model creation (tests/test_abi.py)
"""
import functools

import numpy as np

from osc_amd.synth import SEED_BASE, generate
from osc_qp import build_qp, load_model
from qp_exact import certified, solve_exact

NENV = 61            # a partial last wavefront (four envs per wavefront)
SEED = SEED_BASE + 7100
ROBOTS = ("unitree_go2", "walter_sr")
NAMES = ("tight", "absent", "lifted")


def overrides(name: str, robot: str) -> dict:
    base = load_model(robot)
    q = np.arange(base.nu)
    inf = base.infinity
    if name in ("tight", "pinned"):
        lin = np.linspace
        o = dict(u_lb=np.array([-3.0, 0.5, -6.0, -1.0])[q % 4], u_ub=np.array([1.0, 4.0, -2.0, 8.0])[q % 4],
                 z_lb=[-inf, -inf, 0.0], z_ub=[inf, inf, 30.0], mu=0.35, w_torque=3e-3, w_reg=2e-3,
                 w_pos=base.w_pos * lin(0.2, 3.0, base.ns), w_rot=base.w_rot * lin(2.0, 0.1, base.ns))
        if name == "pinned":
            o["u_lb"][2] = o["u_ub"][2] = 1.5
    elif name == "absent":
        inf = 1e20
        o = dict(u_lb=np.array([-inf, 2.0, -inf])[q % 3], u_ub=np.array([-1.0, inf, inf])[q % 3],
                 z_lb=[-inf, -inf, 0.0], z_ub=[inf, inf, inf], mu=1.2, infinity=inf)
    elif name == "lifted":
        o = dict(u_lb=np.full(base.nu, -12.0), u_ub=np.full(base.nu, 12.0),
                 z_lb=[-inf, -inf, 5.0], z_ub=[inf, inf, 40.0], mu=0.5)
    else:
        raise KeyError(name)
    return {k: (float(v) if np.ndim(v) == 0 else [float(t) for t in v]) for k, v in o.items()}


def model(name: str, robot: str):
    return load_model(robot, overrides=overrides(name, robot))


def fractional_mask(mask: np.ndarray) -> np.ndarray:
    """tight's mask: each entry times 0.5 or 1 (the mask scales the fz bounds)."""
    return mask * np.random.default_rng(5).choice([0.5, 1.0], mask.shape)


@functools.lru_cache(maxsize=None)
def inputs(name: str, robot: str) -> dict:
    d = generate(robot, NENV, SEED, "tumbling", "bernoulli")
    if name in ("tight", "pinned"):
        d["mask"] = fractional_mask(d["mask"])
    return d


def solve_oracle(mdl, d: dict, envs=None):
    """(x, y) of the oracle's certified optimum of each env; solve_exact raises on an env it
    cannot certify, and a certificate above 1e-8 is refused here."""
    xs, ys = [], []
    for e in (range(d["M"].shape[0]) if envs is None else envs):
        a = [d[k][e] for k in ("M", "C", "J", "b", "T", "mask")]
        sol = solve_exact(mdl, build_qp(mdl, *a), *a[:3])
        assert certified(sol.cert, 1e-8), (mdl.name, e, sol.cert)
        xs.append(sol.x)
        ys.append(sol.y)
    return np.array(xs), np.array(ys)


@functools.lru_cache(maxsize=None)
def oracle(name: str, robot: str):
    return solve_oracle(model(name, robot), inputs(name, robot))


def active_counts(mdl, mask: np.ndarray, x: np.ndarray) -> dict:
    """Rows active at the design vectors x (nenv, n): torque bounds within 1e-9, fz at its lower
    bound within 1e-9 on contacts with a non-zero mask, fz at its cap within 1e-7, pyramid rows
    |+-fx +- fy - mu fz| <= 1e-9 where fz > 1e-9.  Absent rows (|bound| >= 1e20) never count."""
    nv, nu, nc = mdl.nv, mdl.nu, mdl.nc
    u = x[:, nv:nv + nu]
    z = x[:, nv + nu:].reshape(-1, nc, 3)
    fz = z[:, :, 2]
    lo, hi = mdl.z_lb[2] * mask, mdl.z_ub[2] * mask
    on = mask != 0
    pyr = 0
    for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        pyr += int(((np.abs(sx * z[:, :, 0] + sy * z[:, :, 1] - mdl.mu * fz) <= 1e-9) & (fz > 1e-9)).sum())
    return dict(
        u_lo=int(((np.abs(mdl.u_lb) < 1e20) & (np.abs(u - mdl.u_lb) <= 1e-9)).sum()),
        u_hi=int(((np.abs(mdl.u_ub) < 1e20) & (np.abs(u - mdl.u_ub) <= 1e-9)).sum()),
        pyramid=pyr,
        fz_lo=int((on & (np.abs(lo) < 1e20) & (np.abs(fz - lo) <= 1e-9)).sum()),
        fz_hi=int((on & (np.abs(hi) < 1e20) & (np.abs(fz - hi) <= 1e-7)).sum()))
