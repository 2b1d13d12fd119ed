"""Bitwise fingerprints of the Go2 solves whose results depend on the one-wave interior point's
start block and on the fused refinement's prologue (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_ipm_start_parent.py <parent commit> \
        > tests/golden/ipm_start_parent.json

Made with the library of the commit before the start (iteration -1, the least-squares initial
point) was peeled out of the one-wave kernels' iteration loop (DESIGN.md §5 "The start, peeled"),
a change that must leave every result bit for bit what it was.
tests/test_gpu_ipm_start_bitwise.py imports the cases from here and checks that the current build
reproduces each SHA-256 of (tau, x, status, iters, and where the entry has them the duals y and
the warm state).  Go2 only, at 1, 3, 4, 5 and 61 envs (one env row, a partial wave, a full wave,
a full plus a partial one, many waves).  The cases:
  * cold, standing and tumbling inputs, contact mask all ones, Bernoulli(0.75) and all zeros (no
    contact row active: the rows of the initial fit differ per row kind), with and without duals;
  * warm ticks on waves whose envs are all warm (the start is skipped);
  * warm ticks on a 4-env wave whose envs 1 and 2 had their warm state invalidated (the start
    runs, the warm rows take over at iteration 0);
  * max_iter 0, 1 and 2 (the loop's exit test sits right after the start);
  * the _env entry with one invalid env (mu = NaN) among valid wave-mates;
  * the two-model call at 4 + 4 envs (its pair kernel holds Go2's wave body);
  * the envs of go2_unrefined_joint_states.npz that take a second refinement round, beside
    one-round wave-mates (make_refine_parent.py's mixed batch).
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

GO2, WALTER = "unitree_go2", "walter_sr"
NENVS = (1, 3, 4, 5, 61)
SCENARIOS = ("standing", "tumbling")
MASKS = ("ones", "bernoulli", "zeros")
MAX_ITERS = (0, 1, 2)
WARM_COLD_ENVS = (1, 2)    # the 4-env wave's envs whose warm state is invalidated before a tick
BAD_ENV = 2                # the _env batch's env with mu = NaN; 0, 1 and 3 share its wavefront
# position in the multi-round batch -> row of go2_unrefined_joint_states.npz (as make_refine_parent)
MIXED_NENV = 7
MIXED_AT = {1: 0, 2: 3, 4: 7, 6: 11}
KEYS = ("M", "C", "J", "b", "T", "mask")
SEED = 1100

_solvers: dict = {}


def solver_for(robot=GO2, max_iter=None):
    from osc_amd.solver import OSCBatchSolver
    key = (robot, max_iter)
    if key not in _solvers:
        _solvers[key] = OSCBatchSolver(robot, max_iter=max_iter)
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


def _inputs(robot, nenv, scen, mask, seed=0):
    from osc_amd.synth import SEED_BASE, generate
    return generate(robot, nenv, SEED_BASE + SEED + seed, scen, mask)


def cold(nenv, scen, mask, max_iter=None) -> dict:
    """The plain call, and the call that also returns the duals."""
    s = solver_for(GO2, max_iter)
    args = s.prepare(**_inputs(GO2, nenv, scen, mask))
    out = s.alloc_outputs(nenv, want_x=True)
    s.solve_into(out, *args)
    dual = s.alloc_outputs(nenv, want_x=True, want_y=True)
    s.solve_into(dual, *args)
    return {"x": _result(out), "dual": _result(dual, dual.y)}


def warm(nenv, cold_envs=()) -> dict:
    """Four warm ticks on a 1 % walk.  Tick 0 starts every env cold; before ticks 1 and 3 the
    valid flag of `cold_envs` (the first double of an env's warm-state record) is cleared, so
    those envs start cold beside warm wave-mates; tick 2 finds every env warm."""
    from osc_amd.synth import random_walk
    s = solver_for()
    d = _inputs(GO2, nenv, "tumbling", "ones", seed=1)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(nenv)
    rec = state.numel() // nenv
    out = s.alloc_outputs(nenv, want_x=True)
    res = {}
    for tick in range(4):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
        if tick in (1, 3):
            for e in cold_envs:
                state[e * rec] = 0.0
        s.solve_warm_into(out, state, *s.prepare(**d))
        res[f"tick{tick}"] = _result(out, state)
    return res


def env_invalid():
    """-> (fingerprint, statuses) of the _env call with BAD_ENV's friction NaN."""
    import torch
    from osc_amd.solver import EnvParams
    s = solver_for()
    d = _inputs(GO2, 5, "tumbling", "bernoulli", seed=2)
    mu = np.random.default_rng(SEED + 1).uniform(0.3, 1.0, 5)
    mu[BAD_ENV] = np.nan
    out = s.solve(**d, want_x=True, env_params=EnvParams(mu=torch.from_numpy(mu).to(s.device)))
    torch.cuda.synchronize()
    return {"batch": _result(out)}, out.status.cpu().numpy().copy()


def multi() -> dict:
    from osc_amd.solver import solve_multi_into
    jobs = []
    for robot, seed in ((GO2, 3), (WALTER, 4)):
        s = solver_for(robot)
        out = s.alloc_outputs(4, want_x=True)
        jobs.append((s, out, s.prepare(**_inputs(robot, 4, "tumbling", "bernoulli", seed=seed))))
    solve_multi_into(jobs)
    return {s.robot: _result(out) for s, out, _ in jobs}


def multi_round():
    """-> (fingerprints, statuses): make_refine_parent.py's batch of envs that need a second
    refinement round, at different lanes of two waves beside one-round wave-mates."""
    s = solver_for()
    z = np.load(os.path.join(HERE, "go2_unrefined_joint_states.npz"))
    from osc_amd.synth import SEED_BASE, generate
    d = generate(GO2, MIXED_NENV, SEED_BASE + 900 + 2, "standing", "ones")
    for pos, row in MIXED_AT.items():
        for k in KEYS:
            d[k][pos] = z[k][row]
    out = s.solve(**d, want_x=True)
    res = {"mixed": _result(out)}
    for pos in MIXED_AT:
        res[f"env{pos}"] = _digest(out.tau[pos], out.x[pos], out.status[pos], out.iters[pos])
    return res, out.status.cpu().numpy().copy()


def case_ids():
    ids = [f"cold-{n}-{sc}-{m}" for n in NENVS for sc in SCENARIOS for m in MASKS]
    ids += [f"warm-{n}" for n in NENVS] + ["warmmixed-4", "warmmixed-5"]
    ids += [f"maxiter-{k}" for k in MAX_ITERS]
    return ids + ["envinvalid", "multi", "multiround"]


def run_case(cid: str) -> dict:
    kind, *rest = cid.split("-")
    if kind == "cold":
        return cold(int(rest[0]), rest[1], rest[2])
    if kind == "warm":
        return warm(int(rest[0]))
    if kind == "warmmixed":
        return warm(int(rest[0]), WARM_COLD_ENVS)
    if kind == "maxiter":
        return cold(5, "tumbling", "bernoulli", max_iter=int(rest[0]))
    if kind == "envinvalid":
        return env_invalid()[0]
    if kind == "multi":
        return multi()
    return multi_round()[0]


def main(argv) -> None:
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    # the fixtures are only worth keeping if they take the paths they are named for
    st = env_invalid()[1]
    assert st[BAD_ENV] == 2 and (np.delete(st, BAD_ENV) == 0).all(), st   # OSC_SOLVE_NUMERICAL
    assert (multi_round()[1] == 0).all()
    w, m = warm(4), warm(4, WARM_COLD_ENVS)
    assert w["tick0"] == m["tick0"] and w["tick1"] != m["tick1"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
