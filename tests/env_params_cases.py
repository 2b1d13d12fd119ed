"""Per-env parameter cases (include/osc_env_params.h, osc_amd.solver.EnvParams) for
tests/test_env_params_ref.py (CPU) and tests/test_gpu_env_params.py (GPU): the input batch, one
draw of friction, torque box, fz bounds and task weights per env, each env's oracle model
(oracle/osc_qp.load_model(overrides=<env e's values>)) and its certified optimum, computed once per
process and shared.

Batch: generate(robot, 61, SEED_BASE + 7300, "tumbling", "bernoulli") with desc_variants'
fractional mask (0 / 0.5 / 1 scaling the fz bounds).  Per env, from default_rng(SEED_BASE + 7300)
in this order:
  s ~ U(0.5, 2)       torque boxes s x ([-3, 0.5, -6, -1], [1, 4, -2, 8])[q % 4]; on envs with
                      e % 7 == 3, u_lb = -infinity where q % 3 == 0 and u_ub = +infinity where
                      q % 3 == 1 (one-sided boxes: rows switched off by the threshold)
  mu ~ U(0.2, 1.2)
  fz_lb from {0, 0, 5}, fz_ub ~ U(15, 60)
  w_pos, w_rot        the model's values x exp(U(ln 0.2, ln 5)) per site
"""
import functools

import numpy as np

import desc_variants as dv
from osc_amd.synth import SEED_BASE, generate
from osc_qp import load_model

NENV = 61
SEED = SEED_BASE + 7300
ROBOTS = dv.ROBOTS
FIELDS = ("mu", "u_lb", "u_ub", "fz_lb", "fz_ub", "w_pos", "w_rot")


@functools.lru_cache(maxsize=None)
def inputs(robot: str) -> dict:
    d = generate(robot, NENV, SEED, "tumbling", "bernoulli")
    d["mask"] = dv.fractional_mask(d["mask"])
    return d


def draw_params(robot: str, rng, nenv: int = NENV) -> dict:
    """One draw of the seven per-env arrays (numpy float64), env by env in the documented order."""
    base = load_model(robot)
    q = np.arange(base.nu)
    lo4, hi4 = np.array([-3.0, 0.5, -6.0, -1.0])[q % 4], np.array([1.0, 4.0, -2.0, 8.0])[q % 4]
    p = dict(mu=np.empty(nenv), u_lb=np.empty((nenv, base.nu)), u_ub=np.empty((nenv, base.nu)),
             fz_lb=np.empty(nenv), fz_ub=np.empty(nenv), w_pos=np.empty((nenv, base.ns)),
             w_rot=np.empty((nenv, base.ns)))
    for e in range(nenv):
        s = rng.uniform(0.5, 2.0)
        p["u_lb"][e], p["u_ub"][e] = s * lo4, s * hi4
        if e % 7 == 3:
            p["u_lb"][e][q % 3 == 0] = -base.infinity
            p["u_ub"][e][q % 3 == 1] = base.infinity
        p["mu"][e] = rng.uniform(0.2, 1.2)
        p["fz_lb"][e] = rng.choice([0.0, 0.0, 5.0])
        p["fz_ub"][e] = rng.uniform(15.0, 60.0)
        p["w_pos"][e] = base.w_pos * np.exp(rng.uniform(np.log(0.2), np.log(5.0), base.ns))
        p["w_rot"][e] = base.w_rot * np.exp(rng.uniform(np.log(0.2), np.log(5.0), base.ns))
    return p


@functools.lru_cache(maxsize=None)
def params(robot: str) -> dict:
    return draw_params(robot, np.random.default_rng(SEED))


def model_constants(robot: str, nenv: int = NENV) -> dict:
    """The seven arrays filled with the model's own constants."""
    m = load_model(robot)
    rep = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, float), (nenv,) + np.shape(v)))
    return dict(mu=rep(m.mu), u_lb=rep(m.u_lb), u_ub=rep(m.u_ub), fz_lb=rep(m.z_lb[2]),
                fz_ub=rep(m.z_ub[2]), w_pos=rep(m.w_pos), w_rot=rep(m.w_rot))


def env_overrides(robot: str, p: dict, e: int) -> dict:
    """Env e's values as a descriptor override dict (OSCBatchSolver(desc_overrides=...),
    load_model(overrides=...))."""
    base = load_model(robot)
    return dict(mu=float(p["mu"][e]), u_lb=[float(v) for v in p["u_lb"][e]],
                u_ub=[float(v) for v in p["u_ub"][e]],
                z_lb=[float(base.z_lb[0]), float(base.z_lb[1]), float(p["fz_lb"][e])],
                z_ub=[float(base.z_ub[0]), float(base.z_ub[1]), float(p["fz_ub"][e])],
                w_pos=[float(v) for v in p["w_pos"][e]], w_rot=[float(v) for v in p["w_rot"][e]])


def env_model(robot: str, p: dict, e: int):
    return load_model(robot, overrides=env_overrides(robot, p, e))


def solve_oracle(robot: str, d: dict, p: dict):
    """(x, y) of the oracle's certified optimum (1e-8) of every env, each from its own model."""
    xs, ys = [], []
    for e in range(d["M"].shape[0]):
        x, y = dv.solve_oracle(env_model(robot, p, e), d, envs=[e])
        xs.append(x[0])
        ys.append(y[0])
    return np.array(xs), np.array(ys)


@functools.lru_cache(maxsize=None)
def oracle(robot: str):
    return solve_oracle(robot, inputs(robot), params(robot))


def redraw_mu_and_boxes(robot: str, p: dict, rng) -> dict:
    """p with mu and the torque boxes drawn anew (the same finite / absent pattern: a warm start
    carries over such a change; a bound appearing or vanishing would need a cold start)."""
    fresh = draw_params(robot, rng, p["mu"].shape[0])
    return dict(p, mu=fresh["mu"], u_lb=fresh["u_lb"], u_ub=fresh["u_ub"])


@functools.lru_cache(maxsize=None)
def warm_ticks(robot: str) -> tuple:
    """Four ticks (inputs, params, oracle x): the drawn batch, then three steps of the 1 % random
    walk with mu and the torque boxes redrawn at each."""
    from osc_amd.synth import random_walk
    d, p = inputs(robot), params(robot)
    rng = np.random.default_rng(SEED + 1)
    ticks = [(d, p, oracle(robot)[0])]
    for _ in range(3):
        d, p = random_walk(d, rng), redraw_mu_and_boxes(robot, p, rng)
        ticks.append((d, p, solve_oracle(robot, d, p)[0]))
    return tuple(ticks)


def active_counts(robot: str, d: dict, p: dict, x: np.ndarray) -> dict:
    """desc_variants.active_counts summed over the envs, each against its own model."""
    tot = dict(u_lo=0, u_hi=0, pyramid=0, fz_lo=0, fz_hi=0)
    for e in range(x.shape[0]):
        c = dv.active_counts(env_model(robot, p, e), d["mask"][e:e + 1], x[e:e + 1])
        for k in tot:
            tot[k] += c[k]
    return tot
