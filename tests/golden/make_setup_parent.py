"""Bitwise fingerprints of what the assembly kernel hands to the interior point (GPU only).

    OSC_LIB_PATH=<libosc_batch.so> python tests/golden/make_setup_parent.py <parent commit> \
        > tests/golden/setup_parent.json

Made with the library of the commit before the lean assembly's hand-off went through LDS and out as
one block of 16-byte stores, a change that must leave every stored bit what
it was.  tests/test_gpu_setup_bitwise.py imports the cases from here and checks that the current
build reproduces each SHA-256.  A case zero-fills the workspace, calls assemble_into and hashes,
env by env, only the ranges the assembly owns: g, Hr (in its workspace layout: compact without
wheel rows), X, H_dv and f_dv -- with wheel rows also the wheel blocks (rows, bases, transforms,
rotation, pins) and the raw rows of the fallback.  NaNs are hashed as the bits they are.
The cases:
  * Go2 at 1 and 5 envs with every contact on, one contact off (a different one per env) and all
    off;
  * Go2, 5 envs, one of them with a mass matrix that is not positive definite (its block is NaN);
  * Go2 with per-env w_pos / w_rot at 3 envs (osc_setup_env_kernel);
  * WaLTER at 1 and 5 envs with a Bernoulli mask; WaLTER with wheel rows at 2 envs;
  * the two-model call (osc_batch_solve_multi) on WaLTER x 3 + Go2 x 2 -- its assembly half is not
    reachable on its own, so the digest is of each job's outputs and its workspace's assembly
    ranges after the whole call;
  * Go2 at BIG_NENV = 4,100 envs -- four past the default small_batch_max of a 256-CU device,
    more blocks than one round of resident waves -- hashed on the first and the last four envs.
Regenerate only for an intentional numerical change of the assembly, and say so in the commit.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "operational-space-control_amd"))

GO2, WALTER, WHEELS = "unitree_go2", "walter_sr", "walter_sr_wheels"
SEED = 1000
BIG_NENV = 4100
MASKS = ("ones", "one_off", "zeros")

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


def owned_ranges(s) -> tuple:
    """(doubles per env, [(lo, hi), ...]) of the workspace ranges the assembly writes
    (csrc/osc_device.hpp Dims: [g | Hr | X | H_dv | f_dv | sol | wheel blocks | raw rows])."""
    from osc_amd import _lib
    d = s.dims
    nv, nu, nc = d["nv"], d["nu"], d["nc"]
    ev = lambda a: (a + 1) // 2 * 2
    ny = nu + 3 * nc
    ny1p = ev(ny + 1)
    nrl = (2 * nu + 6 * nc + 15) // 16
    nw = 2 * nc if s.wheels else 0
    hr_size = ny * ny if s.wheels else (ny - 16) * ny + 136
    w_hr = ev(ny)
    w_x = w_hr + ev(hr_size)
    w_hd = w_x + nv * ny1p
    w_gd = w_hd + nv * nv
    w_sol = w_gd + ev(nv)
    w_nu = w_sol + ev(ny) + nrl * 16 + 2
    ranges = [(0, ny), (w_hr, w_hr + hr_size), (w_x, w_hd), (w_hd, w_gd), (w_gd, w_gd + nv)]
    size = w_nu
    if s.wheels:
        w_aw = w_nu + ev(nw)
        w_pin = w_aw + nw * ny1p + nw * nv + 2 * nw * nw + ny * ny
        w_rm = w_pin + ev(ny)
        w_rc = w_rm + nv * nv
        w_rj = w_rc + ev(nv)
        w_rb = w_rj + 3 * nc * nv
        w_rd = w_rb + ev(3 * nc)
        size = w_rd + ev(6 * nc)
        ranges += [(w_aw, w_pin + ny), (w_rm, w_rm + nv * nv), (w_rc, w_rc + nv), (w_rj, w_rb),
                   (w_rb, w_rb + 3 * nc), (w_rd, w_rd + 6 * nc)]
    eb = ctypes.c_size_t()
    assert _lib.lib().osc_workspace_env_bytes(s._h, ctypes.byref(eb)) == 0
    assert eb.value == 8 * size, (eb.value, size)
    return size, ranges


def ws_digest(s, out, envs=None) -> str:
    """SHA-256 over the owned ranges of `envs` (default: all) of out.workspace, env by env."""
    import torch
    torch.cuda.synchronize()
    nenv = out.tau.shape[0]
    size, ranges = owned_ranges(s)
    w = out.workspace[:nenv * size].cpu().numpy().reshape(nenv, size)
    h = hashlib.sha256()
    for e in (range(nenv) if envs is None else envs):
        for lo, hi in ranges:
            h.update(w[e, lo:hi].tobytes())
    return h.hexdigest()


def _inputs(robot, nenv, mask="ones", seed=0, scen="tumbling"):
    from osc_amd.synth import SEED_BASE, generate
    gen_mask = mask if mask in ("ones", "zeros", "bernoulli") else "ones"
    d = generate(robot, nenv, SEED_BASE + SEED + seed, scen, gen_mask)
    if mask == "one_off":
        nc = d["mask"].shape[1]
        for e in range(nenv):
            d["mask"][e, (e + 1) % nc] = 0.0
    return d


def assemble(s, d, envs=None, **kw) -> str:
    nenv = int(d["M"].shape[0])
    args = s.prepare(**d)
    out = s.alloc_outputs(nenv)
    out.workspace.zero_()
    s.assemble_into(out, *args, **kw)
    return ws_digest(s, out, envs)


def go2(nenv, mask) -> dict:
    return {"ws": assemble(solver_for(GO2), _inputs(GO2, nenv, mask, seed=nenv))}


def non_spd() -> dict:
    d = _inputs(GO2, 5, "ones", seed=10)
    d["M"][2] = -d["M"][2]
    s = solver_for(GO2)
    return {"ws": assemble(s, d), "bad_env": assemble(s, d, envs=[2])}


def env_weights() -> dict:
    from osc_amd.solver import EnvParams
    d = _inputs(GO2, 3, "bernoulli", seed=11)
    rng = np.random.default_rng(SEED + 11)
    ns = solver_for(GO2).dims["ns"]
    ep = EnvParams(w_pos=rng.uniform(0.5, 20.0, (3, ns)), w_rot=rng.uniform(0.5, 20.0, (3, ns)))
    return {"ws": assemble(solver_for(GO2), d, env_params=ep)}


def walter(nenv) -> dict:
    return {"ws": assemble(solver_for(WALTER), _inputs(WALTER, nenv, "bernoulli", seed=20 + nenv))}


def wheels() -> dict:
    import torch
    from osc_amd.synth import SEED_BASE, WALTER_WHEEL_DOFS, WHEEL_RADIUS, wheel_directions
    s = solver_for(WHEELS)
    assert s.wheels
    d = _inputs(WHEELS, 2, "bernoulli", seed=30)
    wd = wheel_directions(WHEELS, d, np.array(WALTER_WHEEL_DOFS), np.full(8, WHEEL_RADIUS),
                          SEED_BASE + SEED + 31)
    return {"ws": assemble(s, d, wheel_dir=torch.from_numpy(wd).to(s.device))}


def multi() -> dict:
    import torch
    from osc_amd.solver import solve_multi_into
    jobs = []
    for robot, nenv, seed in ((WALTER, 3, 40), (GO2, 2, 41)):
        s = solver_for(robot)
        out = s.alloc_outputs(nenv, want_x=True)
        out.workspace.zero_()
        jobs.append((s, out, s.prepare(**_inputs(robot, nenv, "bernoulli", seed=seed))))
    solve_multi_into(jobs)
    torch.cuda.synchronize()
    res = {}
    for s, out, _ in jobs:
        h = hashlib.sha256()
        for t in (out.tau, out.x, out.status, out.iters):
            h.update(t.cpu().numpy().tobytes())
        res[s.robot] = {"out": h.hexdigest(), "ws": ws_digest(s, out)}
    return res


def big() -> dict:
    d = _inputs(GO2, BIG_NENV, "bernoulli", seed=50, scen="standing")
    ends = list(range(4)) + list(range(BIG_NENV - 4, BIG_NENV))
    return {"ws": assemble(solver_for(GO2), d, envs=ends)}


def case_ids():
    return ([f"go2-{n}-{m}" for n in (1, 5) for m in MASKS] +
            ["non_spd", "env_weights", "walter-1", "walter-5", "wheels", "multi", "big"])


def run_case(cid: str) -> dict:
    kind, *rest = cid.split("-")
    if kind == "go2":
        return go2(int(rest[0]), rest[1])
    if kind == "walter":
        return walter(int(rest[0]))
    return {"non_spd": non_spd, "env_weights": env_weights, "wheels": wheels, "multi": multi,
            "big": big}[kind]()


def main(argv) -> None:
    lib = os.environ.get("OSC_LIB_PATH")
    out = {"parent": argv[0] if argv else "unknown",
           "lib_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest() if lib else "in-tree",
           "cases": {cid: run_case(cid) for cid in case_ids()}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1:])
