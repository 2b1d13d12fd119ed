"""Cost of the per-env parameters (include/osc_env_params.h): solve_into and
solve_warm_into with and without env_params on the same inputs, the EnvParams block filled with
the model's own constants (so both solve the same QPs, bitwise), Go2 at 4,096 and 65,536 envs and
WaLTER Sr at 4,096 (tumbling batches, Bernoulli masks), in one process with the two alternating.
HIP events around REP back-to-back launches, two warm-up rounds, seven timed rounds alternating
existing / per-env; median [min, max] per launch.  Warm ticks carry their warm state and alternate
between the batch and a 1 % random-walk step of it.  One JSON line per configuration.

    python tools/env_params_timing.py [--small]          (--small: 4,096 envs only)

The existing entry against a build of the parent commit is an A/B across processes with
tools/ab_time.py (raw ctypes: a library without the _env symbols loads too), one library per
process, the processes interleaved: profiles/env_params/ab_timing.json."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "operational-space-control_amd")]
from osc_amd.solver import EnvParams, OSCBatchSolver
from osc_amd.synth import SEED_BASE, generate, random_walk

REP = 10
small = "--small" in sys.argv
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REP):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def model_constants(solver, nenv):
    """EnvParams of the model's own constants, device tensors."""
    d, n = solver.desc, solver.dims
    full = lambda v, w: torch.tensor(list(v)[:w], dtype=torch.float64, device=dev).repeat(nenv, 1)
    col = lambda v: torch.full((nenv,), float(v), dtype=torch.float64, device=dev)
    return EnvParams(mu=col(d.mu), u_lb=full(d.u_lb, n["nu"]), u_ub=full(d.u_ub, n["nu"]),
                     fz_lb=col(d.z_lb[2]), fz_ub=col(d.z_ub[2]), w_pos=full(d.w_pos, n["ns"]),
                     w_rot=full(d.w_rot, n["ns"]))


for robot, sizes in (("unitree_go2", (4096, 65536)), ("walter_sr", (4096,))):
    solver = OSCBatchSolver(robot)
    for nenv in ((4096,) if small else sizes):
        inp = generate(robot, nenv, SEED_BASE + 11, "tumbling", "bernoulli")
        a = solver.prepare(**inp)
        b = solver.prepare(**random_walk(inp, np.random.default_rng(3)))
        ep = model_constants(solver, nenv)
        outs = [solver.alloc_outputs(nenv, want_x=True) for _ in range(4)]
        warms = [solver.alloc_warm_state(nenv) for _ in range(2)]
        fns = dict(
            cold=lambda i: solver.solve_into(outs[0], *a),
            cold_env=lambda i: solver.solve_into(outs[1], *a, env_params=ep),
            warm=lambda i: solver.solve_warm_into(outs[2], warms[0], *(b if i % 2 else a)),
            warm_env=lambda i: solver.solve_warm_into(outs[3], warms[1], *(b if i % 2 else a),
                                                      env_params=ep))
        for _ in range(2):
            for f in fns.values():
                timed(f)
        t = {k: [] for k in fns}
        for _ in range(7):
            for k, f in fns.items():
                t[k].append(timed(f))
        same = all(torch.equal(getattr(outs[0], k), getattr(outs[1], k)) and
                   torch.equal(getattr(outs[2], k), getattr(outs[3], k))
                   for k in ("tau", "x", "status", "iters"))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps(dict(robot=robot, nenv=nenv, rep=REP,
                              status_ok=int((outs[1].status == 0).sum().item()),
                              bitwise_equal=bool(same),
                              cold_ms=stats(t["cold"]), cold_env_ms=stats(t["cold_env"]),
                              warm_ms=stats(t["warm"]), warm_env_ms=stats(t["warm_env"]),
                              cold_env_over_cold=med["cold_env"] / med["cold"],
                              warm_env_over_warm=med["warm_env"] / med["warm"])), flush=True)
        del a, b, ep, outs, warms
        torch.cuda.empty_cache()
