"""Bitwise fingerprints of the solves whose results depend on when the interior point refreshes
the rows' residual rp = G y + s - h, and on the re-centring block ahead of it (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_ipm_fresh_parent.py <parent commit> \
        > tests/golden/ipm_fresh_parent.json

Made with the library of the commit before the refresh was restricted to the envs that go on
iterating (DESIGN.md §5 "The refresh of the rows' residual"), a change that must leave every result
bit for bit what it was.  tests/test_gpu_ipm_fresh_bitwise.py imports the cases from here and
checks that the current build reproduces each SHA-256 of (tau, x, status, iters, and where the
entry has them the duals y and the warm state).  The cases:
  * Go2 cold (tumbling) at 1, 3, 4, 5 and 61 envs (one env row, a partial wave, a full wave, a full
    plus a partial one, many waves), contact mask all ones, Bernoulli(0.75) and all zeros, with
    and without duals;
  * "spread": a Go2 wave of 4 whose envs stop at least 3 iterations apart, so the skipped refresh
    demonstrably runs beside done wave-mates (the parent's iters are kept beside the hash);
  * "restart": restart_iter tuned down to RESTART_ITER on a wave of 4 whose env RESTART_FREE_ENV
    has no contact (its torque box alone: few iterations), so the re-centring block and the
    `restart` arm of the refresh run beside a wave-mate that is done already (the parent's iters
    with and without the tuning are kept: an env stops before RESTART_ITER, another's count
    changes with the tuning);
  * max_iter 0, 1 and 2;
  * warm ticks on a wave whose envs are all warm and on one whose envs 1 and 2 are cold again, two
    ticks each after the cold first one;
  * the _env entry with one invalid env (mu = NaN) among valid wave-mates;
  * WaLTER (eps_mu = 1e-8: envs with 1e-8 < mu <= 1e-6 must still refresh) at 4 and 5 envs;
  * Go2 at 5 envs with small_batch_max = 0: the two-wave kernel;
  * the two-model call at 4 + 4 envs;
  * the envs of go2_unrefined_joint_states.npz that take a second refinement round, beside
    one-round wave-mates (make_refine_parent.py's mixed batch).
SPREAD_SEED, RESTART_ITER and RESTART_SEED were picked on the parent: `--pick` runs the two
searches (the first seed, and the lowest restart_iter from 2, that meet the case's condition),
uses what it finds and records it under "picked".
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
MASKS = ("ones", "bernoulli", "zeros")
MAX_ITERS = (0, 1, 2)
WALTER_NENVS = (4, 5)
WARM_COLD_ENVS = (1, 2)    # the mixed wave's envs whose warm state is invalidated before a tick
BAD_ENV = 2                # the _env batch's env with mu = NaN; 0, 1 and 3 share its wavefront
SPREAD_MIN = 3             # the spread wave: max - min of the parent's iters, at least
SPREAD_SEED = 3            # (picked on the parent, see above)
RESTART_FREE_ENV = 1       # the restart wave's env without contacts
RESTART_ITER = 8           # (picked on the parent: the lowest from 2 ...
RESTART_SEED = 3           #  ... and the first seed that meet the case's condition)
RESTART_ITERS = range(2, 13)
PICK_RANGE = 32
TWO_WAVE = {"small_batch_max": 0}
# position in the multi-round batch -> row of go2_unrefined_joint_states.npz (as make_refine_parent)
MIXED_NENV = 7
MIXED_AT = {1: 0, 2: 3, 4: 7, 6: 11}
KEYS = ("M", "C", "J", "b", "T", "mask")
SEED = 1200

_solvers: dict = {}


def solver_for(robot=GO2, max_iter=None, **tuning):
    from osc_amd.solver import OSCBatchSolver
    key = (robot, max_iter, tuple(sorted(tuning.items())))
    if key not in _solvers:
        _solvers[key] = OSCBatchSolver(robot, max_iter=max_iter, tuning=tuning or None)
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


def _iters(out) -> list:
    return [int(v) for v in out.iters.cpu().numpy()]


def _inputs(robot, nenv, mask, seed=0):
    from osc_amd.synth import SEED_BASE, generate
    return generate(robot, nenv, SEED_BASE + SEED + seed, "tumbling", mask)


def cold(robot, nenv, mask, max_iter=None, **tuning) -> dict:
    """The plain call, and the call that also returns the duals."""
    s = solver_for(robot, max_iter, **tuning)
    args = s.prepare(**_inputs(robot, nenv, mask))
    out = s.alloc_outputs(nenv, want_x=True)
    s.solve_into(out, *args)
    dual = s.alloc_outputs(nenv, want_x=True, want_y=True)
    s.solve_into(dual, *args)
    return {"x": _result(out), "dual": _result(dual, dual.y)}


def spread(seed=None) -> dict:
    """One Go2 wave; "iters" is what the library that made the fingerprint counted."""
    d = _inputs(GO2, 4, "bernoulli", seed=100 + (SPREAD_SEED if seed is None else seed))
    out = solver_for().solve(**d, want_x=True)
    return {"x": _result(out), "iters": _iters(out), "status": [int(v) for v in out.status.cpu()]}


def spread_ok(res) -> bool:
    return max(res["iters"]) - min(res["iters"]) >= SPREAD_MIN and not any(res["status"])


def restart(seed=None) -> dict:
    """One Go2 wave, env RESTART_FREE_ENV without contacts, re-centred at iteration RESTART_ITER;
    "iters_default" is the same wave's count with the model's own restart_iter."""
    d = _inputs(GO2, 4, "bernoulli", seed=200 + (RESTART_SEED if seed is None else seed))
    d["mask"][RESTART_FREE_ENV] = 0.0
    out = solver_for(restart_iter=RESTART_ITER).solve(**d, want_x=True)
    ref = solver_for().solve(**d, want_x=True)
    return {"x": _result(out), "iters": _iters(out), "iters_default": _iters(ref),
            "status": [int(v) for v in out.status.cpu()]}


def restart_ok(res) -> bool:
    """An env is done before the re-centring, which changes a wave-mate's course."""
    return (min(res["iters"]) < RESTART_ITER and not any(res["status"]) and
            any(a > RESTART_ITER and a != b for a, b in zip(res["iters"], res["iters_default"])))


def pick(case, ok) -> int:
    for seed in range(PICK_RANGE):
        if ok(case(seed)):
            return seed
    raise RuntimeError(f"no seed below {PICK_RANGE} meets the condition of {case.__name__}")


def warm(cold_envs=()) -> dict:
    """Three ticks on a 1 % walk of one wave.  Tick 0 starts every env cold; before ticks 1 and 2
    the valid flag of `cold_envs` (the first double of an env's warm-state record) is cleared, so
    those envs start cold beside warm wave-mates."""
    from osc_amd.synth import random_walk
    s = solver_for()
    d = _inputs(GO2, 4, "ones", seed=1)
    rng = np.random.default_rng(SEED)
    state = s.alloc_warm_state(4)
    rec = state.numel() // 4
    out = s.alloc_outputs(4, want_x=True)
    res = {}
    for tick in range(3):
        if tick > 0:
            d = random_walk(d, rng, 0.01)
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
    d = _inputs(GO2, 5, "bernoulli", seed=2)
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
        jobs.append((s, out, s.prepare(**_inputs(robot, 4, "bernoulli", seed=seed))))
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
    ids = [f"cold-{n}-{m}" for n in NENVS for m in MASKS]
    ids += ["spread", "restart"] + [f"maxiter-{k}" for k in MAX_ITERS]
    ids += ["warm", "warmmixed", "envinvalid"] + [f"walter-{n}" for n in WALTER_NENVS]
    return ids + ["twowave", "multi", "multiround"]


def run_case(cid: str) -> dict:
    kind, *rest = cid.split("-")
    if kind == "cold":
        return cold(GO2, int(rest[0]), rest[1])
    if kind == "spread":
        return spread()
    if kind == "restart":
        return restart()
    if kind == "maxiter":
        return cold(GO2, 5, "bernoulli", max_iter=int(rest[0]))
    if kind == "warm":
        return warm()
    if kind == "warmmixed":
        return warm(WARM_COLD_ENVS)
    if kind == "envinvalid":
        return env_invalid()[0]
    if kind == "walter":
        return cold(WALTER, int(rest[0]), "bernoulli")
    if kind == "twowave":
        return cold(GO2, 5, "bernoulli", **TWO_WAVE)
    if kind == "multi":
        return multi()
    return multi_round()[0]


def main(argv) -> None:
    global SPREAD_SEED, RESTART_ITER, RESTART_SEED
    picked = None
    if "--pick" in argv:
        argv = [a for a in argv if a != "--pick"]
        SPREAD_SEED = pick(spread, spread_ok)
        for RESTART_ITER in RESTART_ITERS:
            try:
                RESTART_SEED = pick(restart, restart_ok)
                break
            except RuntimeError:
                continue
        else:
            raise RuntimeError("no restart_iter and seed meet the restart case's condition")
        picked = {"SPREAD_SEED": SPREAD_SEED, "RESTART_ITER": RESTART_ITER,
                  "RESTART_SEED": RESTART_SEED}
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    if picked:
        out["picked"] = picked
    # the fixtures are only worth keeping if they take the paths they are named for
    assert spread_ok(out["cases"]["spread"]), out["cases"]["spread"]
    assert restart_ok(out["cases"]["restart"]), out["cases"]["restart"]
    st = env_invalid()[1]
    assert st[BAD_ENV] == 2 and (np.delete(st, BAD_ENV) == 0).all(), st   # OSC_SOLVE_NUMERICAL
    assert (multi_round()[1] == 0).all()
    w, m = warm(), warm(WARM_COLD_ENVS)
    assert w["tick0"] == m["tick0"] and w["tick1"] != m["tick1"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
