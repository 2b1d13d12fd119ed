"""Bitwise fingerprints of the solves that run the interior point's fused refinement (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_refine_parent.py <parent commit> \
        > tests/golden/refine_parent.json

Made with the library of the commit before the fused refinement's step loop was re-scheduled
(DESIGN.md §5 "The refinement's steps"), a change that must leave every result bit for bit what
it was.  tests/test_gpu_refine_bitwise.py imports the cases from here and checks that the current
build reproduces each SHA-256 of (tau, x, status, iters, and the warm state where there is one).
The cases:
  * Go2 and WaLTER cold, the single call and the split entry points, at 1, 4, 5 and 67 envs (one
    env, one full wave, partial last waves);
  * Go2 warm ticks over 3 steps at 5 envs (the fused warm kernel and its same-launch fix-up pass);
  * the multi-round path: envs of go2_unrefined_joint_states.npz, which need more than one
    refinement round (round > 0 re-reads Hr from the workspace), at different lanes of two waves
    beside one-round wave-mates, and each of them alone -- per-env digests, which must agree;
  * one wheel-row batch and one two-wave batch (small_batch_max = 0), which the change leaves alone.
Regenerate only for an intentional numerical change of these kernels, and say so in the commit.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "operational-space-control_amd"))

ROBOTS = ("unitree_go2", "walter_sr")
WHEELS = "walter_sr_wheels"
NENVS = (1, 4, 5, 67)
WARM_NENV = 5          # two waves, the second with one valid row
MIXED_NENV = 7         # a full wave and a partial one
# position in the mixed batch -> row of go2_unrefined_joint_states.npz (seeds 11, 13 and 14)
MIXED_AT = {1: 0, 2: 3, 4: 7, 6: 11}
KEYS = ("M", "C", "J", "b", "T", "mask")
SEED = 900

_solvers: dict = {}


def solver_for(robot, **tuning):
    from osc_amd.robots import config_path
    from osc_amd.solver import OSCBatchSolver
    key = (robot, tuple(sorted(tuning.items())))
    if key not in _solvers:
        yaml = None
        if robot == WHEELS:
            yaml = os.path.join(os.path.dirname(config_path(WHEELS)),
                                "walter_sr_wheels_noslip_config.yaml")
        _solvers[key] = OSCBatchSolver(robot, yaml, tuning=tuning or None)
    return _solvers[key]


def _digest(*tensors) -> str:
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def _result(out, *more) -> str:
    return _digest(out.tau, out.x, out.status, out.iters, *more)


def _env_result(out, e) -> str:
    return _digest(out.tau[e], out.x[e], out.status[e], out.iters[e])


def _inputs(robot, nenv, scen="standing", mask="ones", seed=0):
    from osc_amd.synth import SEED_BASE, generate
    return generate(robot, nenv, SEED_BASE + SEED + seed, scen, mask)


def cold(robot, nenv) -> dict:
    """The single call and the split entry points, each into fresh outputs."""
    s = solver_for(robot)
    args = s.prepare(**_inputs(robot, nenv, "tumbling", "bernoulli"))
    one = s.alloc_outputs(nenv, want_x=True)
    s.solve_into(one, *args)
    two = s.alloc_outputs(nenv, want_x=True)
    s.assemble_into(two, *args)
    s.solve_assembled_into(two, args[5])
    return {"single": _result(one), "split": _result(two)}


def warm() -> dict:
    """Go2: three warm ticks on a 1 % walk."""
    from osc_amd.synth import random_walk
    s = solver_for("unitree_go2")
    d = _inputs("unitree_go2", WARM_NENV, "tumbling", "ones", seed=1)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(WARM_NENV)
    out = s.alloc_outputs(WARM_NENV, want_x=True)
    res = {}
    for tick in range(3):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
        s.solve_warm_into(out, state, *s.prepare(**d))
        res[f"tick{tick}"] = _result(out, state)
    return res


def multi_round():
    """-> (fingerprints, the mixed batch's statuses).  `mixed`: the whole batch; `env<p>`: the
    env at position p inside it; `alone<p>`: the same env solved at nenv = 1."""
    s = solver_for("unitree_go2")
    z = np.load(os.path.join(HERE, "go2_unrefined_joint_states.npz"))
    d = _inputs("unitree_go2", MIXED_NENV, "standing", "ones", seed=2)
    for pos, row in MIXED_AT.items():
        for k in KEYS:
            d[k][pos] = z[k][row]
    out = s.solve(**d, want_x=True)
    res = {"mixed": _result(out)}
    for pos in MIXED_AT:
        res[f"env{pos}"] = _env_result(out, pos)
        one = s.solve(**{k: d[k][pos:pos + 1].copy() for k in KEYS}, want_x=True)
        res[f"alone{pos}"] = _env_result(one, 0)
    return res, out.status.cpu().numpy().copy()


def wheels() -> dict:
    import torch
    from osc_amd.synth import SEED_BASE, WALTER_WHEEL_DOFS, WHEEL_RADIUS, wheel_directions
    s = solver_for(WHEELS)
    assert s.wheels
    d = _inputs(WHEELS, 5, "tumbling", "bernoulli", seed=3)
    wd = wheel_directions(WHEELS, d, np.array(WALTER_WHEEL_DOFS), np.full(8, WHEEL_RADIUS),
                          SEED_BASE + SEED + 50)
    out = s.alloc_outputs(5, want_x=True)
    s.solve_into(out, *s.prepare(**d), wheel_dir=torch.from_numpy(wd).to(s.device))
    return {"x": _result(out)}


def two_wave() -> dict:
    s = solver_for("unitree_go2", small_batch_max=0)
    return {"x": _result(s.solve(**_inputs("unitree_go2", 5, "tumbling", "bernoulli", seed=4),
                                 want_x=True))}


def case_ids():
    return ([f"cold-{r}-{n}" for r in ROBOTS for n in NENVS] +
            ["warm", "multi_round", "wheels", "two_wave"])


def run_case(cid: str) -> dict:
    kind, *rest = cid.split("-")
    if kind == "cold":
        return cold(rest[0], int(rest[1]))
    if kind == "multi_round":
        return multi_round()[0]
    return {"warm": warm, "wheels": wheels, "two_wave": two_wave}[kind]()


def main(argv) -> None:
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    res, st = multi_round()   # the fixture is only worth keeping if every env ends OK
    assert (st == 0).all(), st
    for pos in MIXED_AT:
        assert res[f"env{pos}"] == res[f"alone{pos}"], pos
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
