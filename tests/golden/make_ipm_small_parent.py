"""Bitwise fingerprints of small batches through the interior point's one-wave kernels (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_ipm_small_parent.py <parent commit> \
        > tests/golden/ipm_small_parent.json

Made with the library of the commit before the interior point's iteration loop was restructured
(selects for its small lane-varying branches, the start's selects and the per-iteration
parameter loads hoisted: DESIGN.md §5 "Issue slots"), a change that must leave every result bit
for bit what it was.
tests/test_gpu_ipm_small_bitwise.py imports the cases from here and checks that the current build
reproduces each SHA-256.  The batches are tiny on purpose: partial last waves (whole DPP rows
with `valid` false), one- and many-wave launches, the split entry points against the single call,
warm ticks with a cold restart beside warm wave-mates, an env that comes back NUMERICAL beside
healthy wave-mates, and the stalled joint-state envs that take the same-launch fix-up pass.
Regenerate only for an intentional numerical change of the default kernels, and say so in the
commit.
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
NENVS = (1, 3, 4, 5, 67)
INPUTS = (("standing", "ones"), ("standing", "bernoulli"), ("tumbling", "ones"),
          ("tumbling", "bernoulli"))
STALLED = {"unitree_go2": "go2_stalled_joint_states.npz",
           "walter_sr": "walter_stalled_joint_states.npz"}
WARM_NENV = 5          # two waves, the second with one valid row
WARM_SWITCH_ENV = 1    # third tick: this env's contact mask changes (cold beside warm wave-mates)
BAD_ENV = 2            # the env given an indefinite M; 0, 1 and 3 share its wavefront
SEED = 700

_solvers: dict = {}


def solver_for(robot):
    from osc_amd.solver import OSCBatchSolver
    if robot not in _solvers:
        _solvers[robot] = OSCBatchSolver(robot)
    return _solvers[robot]


def _digest(*tensors) -> str:
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def _result(out, *more) -> str:
    return _digest(out.tau, out.x, out.status, out.iters, *more)


def _inputs(robot, nenv, scen, mask, seed=0):
    from osc_amd.synth import SEED_BASE, generate
    return generate(robot, nenv, SEED_BASE + SEED + seed, scen, mask)


def cold(robot, nenv, scen, mask) -> dict:
    """The single call and the split entry points, each into fresh outputs."""
    s = solver_for(robot)
    args = s.prepare(**_inputs(robot, nenv, scen, mask))
    one = s.alloc_outputs(nenv, want_x=True)
    s.solve_into(one, *args)
    two = s.alloc_outputs(nenv, want_x=True)
    s.assemble_into(two, *args)
    s.solve_assembled_into(two, args[5])
    return {"single": _result(one), "split": _result(two)}


def warm(robot) -> dict:
    """Three warm ticks on a 1 % walk; the third with one env's contact mask switched."""
    from osc_amd.synth import random_walk
    s = solver_for(robot)
    d = _inputs(robot, WARM_NENV, "tumbling", "ones", seed=1)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(WARM_NENV)
    out = s.alloc_outputs(WARM_NENV, want_x=True)
    res = {}
    for tick in range(3):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
        if tick == 2:
            d["mask"][WARM_SWITCH_ENV, 0] = 0.0
        s.solve_warm_into(out, state, *s.prepare(**d))
        res[f"tick{tick}"] = _result(out, state)
    return res


def indefinite(robot):
    """(fingerprint of the batch with BAD_ENV's M indefinite, its outputs, the healthy batch's)"""
    s = solver_for(robot)
    d = _inputs(robot, 5, "tumbling", "bernoulli", seed=2)
    good = s.solve(**d, want_x=True)
    lo = np.linalg.eigvalsh(d["M"][BAD_ENV])[0]   # smallest eigenvalue shifted to -0.05
    d["M"][BAD_ENV] -= (lo + 0.05) * np.eye(d["M"].shape[1])
    bad = s.solve(**d, want_x=True)
    return {"batch": _result(bad)}, bad, good


def stalled(robot) -> dict:
    """The stalled joint-state envs (tests/golden/*_stalled_joint_states.npz) as one small batch:
    the interior point leaves them at max_iter and the same launch's cold fix-up pass re-solves."""
    s = solver_for(robot)
    z = np.load(os.path.join(HERE, STALLED[robot]))
    d = {k: z[k] for k in ("M", "C", "J", "b", "T", "mask")}
    out = s.solve(**d, want_x=True)
    state = s.alloc_warm_state(d["M"].shape[0])
    wout = s.alloc_outputs(d["M"].shape[0], want_x=True)
    s.solve_warm_into(wout, state, *s.prepare(**d))
    return {"cold": _result(out), "warm": _result(wout, state)}


def case_ids():
    ids = [f"cold-{r}-{n}-{sc}-{m}" for r in ROBOTS for n in NENVS for sc, m in INPUTS]
    for r in ROBOTS:
        ids += [f"warm-{r}", f"indefinite-{r}", f"stalled-{r}"]
    return ids


def run_case(cid: str) -> dict:
    kind, robot, *rest = cid.split("-")
    if kind == "cold":
        return cold(robot, int(rest[0]), rest[1], rest[2])
    if kind == "warm":
        return warm(robot)
    if kind == "indefinite":
        return indefinite(robot)[0]
    return stalled(robot)


def main(argv) -> None:
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    for robot in ROBOTS:   # the fixture is only worth keeping if the env really is rejected
        _, bad, _ = indefinite(robot)
        assert int(bad.status[BAD_ENV]) == 2, (robot, bad.status)   # OSC_SOLVE_NUMERICAL
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
