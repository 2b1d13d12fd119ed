"""Bitwise fingerprints of the interior point's kernel variants that the default small batches of
make_ipm_small_parent.py do not reach (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_ipm_variants_parent.py <parent commit> \
        > tests/golden/ipm_variants_parent.json

Made with the library of the commit before the interior point's header was split into its parts
and its wave body into named phases (DESIGN.md §5 "The split of the wave body"), a change that
must leave every result bit for bit what it was.  tests/test_gpu_ipm_variants_bitwise.py imports
the cases from here and checks that the current build reproduces each SHA-256.  The cases:
  * the wheel no-slip rows (the D::WH code): cold solves with and without the duals, warm ticks;
  * the warm start past one wave per SIMD (small_batch_max = 0): the two-wave warm kernel, the
    separate refinement kernel, then the two-wave fused kernel as the cold fix-up pass -- warm
    ticks with a contact-mode switch, and the stalled joint-state envs;
  * no refinement (refine_steps = 0), one wave and two waves per SIMD;
  * the duals requested on the default kernels (flags bit 1), y in the digest.
Every batch is at most 67 envs.  Regenerate only for an intentional numerical change of these
kernels, and say so in the commit.
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
WHEEL_NENVS = (1, 5, 67)
STALLED = {"unitree_go2": "go2_stalled_joint_states.npz",
           "walter_sr": "walter_stalled_joint_states.npz"}
NENV = 5               # two waves, the second with one valid row
WARM_SWITCH_ENV = 1    # third tick: this env's contact mask changes (cold beside warm wave-mates)
TWO_WAVE = {"small_batch_max": 0}
SEED = 800

_solvers: dict = {}


def solver_for(robot, **tuning):
    """One solver per (robot, tuning); WHEELS: the model with the no-slip rows switched on."""
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
    extra = (out.y,) if out.y is not None else ()
    return _digest(out.tau, out.x, out.status, out.iters, *extra, *more)


def _inputs(robot, nenv, seed=0):
    from osc_amd.synth import SEED_BASE, generate
    return generate(robot, nenv, SEED_BASE + SEED + seed, "tumbling", "bernoulli")


def _wheel_dir(s, d, seed=0):
    import torch
    from osc_amd.synth import SEED_BASE, WALTER_WHEEL_DOFS, WHEEL_RADIUS, wheel_directions
    wd = wheel_directions(WHEELS, d, np.array(WALTER_WHEEL_DOFS), np.full(8, WHEEL_RADIUS),
                          SEED_BASE + SEED + 50 + seed)
    return torch.from_numpy(wd).to(s.device)


def wheels_cold(nenv):
    """-> (fingerprints, [the solves' outputs]): x alone, and x with the duals."""
    s = solver_for(WHEELS)
    assert s.wheels
    d = _inputs(WHEELS, nenv, seed=10)
    args, wd = s.prepare(**d), _wheel_dir(s, d)
    res, outs = {}, []
    for name, want_y in (("x", False), ("xy", True)):
        out = s.alloc_outputs(nenv, want_x=True, want_y=want_y)
        s.solve_into(out, *args, wheel_dir=wd)
        res[name] = _result(out)
        outs.append(out)
    return res, outs


def wheels_warm():
    """Three warm ticks on a 1 % walk, the wheel directions re-derived from the walked state."""
    from osc_amd.synth import random_walk
    s = solver_for(WHEELS)
    d = _inputs(WHEELS, NENV, seed=11)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(NENV)
    out = s.alloc_outputs(NENV, want_x=True)
    res, sts = {}, []
    for tick in range(3):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
        s.solve_warm_into(out, state, *s.prepare(**d), wheel_dir=_wheel_dir(s, d))
        res[f"tick{tick}"] = _result(out, state)
        sts.append(out.status.cpu().numpy().copy())
    return res, sts


def warm_two_wave(robot):
    """Three warm ticks past one wave per SIMD; the third with one env's contact mask switched.
    -> (fingerprints, each tick's iteration counts)"""
    from osc_amd.synth import random_walk
    s = solver_for(robot, **TWO_WAVE)
    d = _inputs(robot, NENV, seed=1)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(NENV)
    out = s.alloc_outputs(NENV, want_x=True)
    res, its = {}, []
    for tick in range(3):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
        if tick == 2:
            d["mask"][WARM_SWITCH_ENV, 0] = 1.0 - d["mask"][WARM_SWITCH_ENV, 0]
        s.solve_warm_into(out, state, *s.prepare(**d))
        res[f"tick{tick}"] = _result(out, state)
        its.append(out.iters.cpu().numpy().copy())
    return res, its


def stalled_two_wave(robot) -> dict:
    """The stalled joint-state envs through the three-launch warm sequence: the warm kernel leaves
    them at max_iter, the two-wave fused kernel's cold fix-up pass re-solves them."""
    s = solver_for(robot, **TWO_WAVE)
    z = np.load(os.path.join(HERE, STALLED[robot]))
    d = {k: z[k] for k in ("M", "C", "J", "b", "T", "mask")}
    n = d["M"].shape[0]
    state = s.alloc_warm_state(n)
    out = s.alloc_outputs(n, want_x=True)
    s.solve_warm_into(out, state, *s.prepare(**d))
    return {"warm": _result(out, state)}


def norefine(robot) -> dict:
    """refine_steps = 0: the interior point alone, one wave and two waves per SIMD."""
    d = _inputs(robot, NENV, seed=2)
    res = {}
    for name, tune in (("one_wave", {}), ("two_wave", TWO_WAVE)):
        res[name] = _result(solver_for(robot, refine_steps=0, **tune).solve(**d, want_x=True))
    return res


def duals(robot) -> dict:
    return {"xy": _result(solver_for(robot).solve(**_inputs(robot, NENV, seed=3), want_x=True,
                                                  want_y=True))}


def case_ids():
    ids = [f"wheels_cold-{n}" for n in WHEEL_NENVS] + ["wheels_warm"]
    for r in ROBOTS:
        ids += [f"warm_two_wave-{r}", f"stalled_two_wave-{r}", f"norefine-{r}", f"duals-{r}"]
    return ids


def run_case(cid: str) -> dict:
    kind, *rest = cid.split("-")
    if kind == "wheels_cold":
        return wheels_cold(int(rest[0]))[0]
    if kind == "wheels_warm":
        return wheels_warm()[0]
    return {"warm_two_wave": lambda r: warm_two_wave(r)[0], "stalled_two_wave": stalled_two_wave,
            "norefine": norefine, "duals": duals}[kind](rest[0])


def main(argv) -> None:
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    # the fixture is only worth keeping if each batch really takes its path
    for n in WHEEL_NENVS:
        for o in wheels_cold(n)[1]:
            assert (o.status.cpu().numpy() == 0).all(), (n, o.status)
    for st in wheels_warm()[1]:
        assert (st == 0).all(), st
    for robot in ROBOTS:
        for it in warm_two_wave(robot)[1][1:]:   # the warm ticks run the interior point
            assert (it > 0).any(), (robot, it)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
