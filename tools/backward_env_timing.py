"""Backward-pass measurement of DESIGN.md §3.7: osc_batch_solve_backward_env against
osc_batch_solve_backward_data of the same run, Go2 and WaLTER Sr at 4,096 and 65,536 envs
(tumbling batches, Bernoulli masks, the model's constants):
  (a) backward_data_into, all six outputs                              the yardstick
  (b) backward_env_into, the same six outputs, a model-constants block
  (c) (b) plus all seven parameter gradients
  (d) the parameter gradients of mu and the bounds only (no solve with M, no pass over J)
HIP events around REP back-to-back launches of each, two warm-up rounds, seven timed rounds
alternating (a) (b) (c) (d); median [min, max] per launch.  One JSON line per configuration.

    python tools/backward_env_timing.py [--small] [--out FILE]   (--small: 4,096 envs only)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "operational-space-control_amd")]
from osc_amd.solver import EnvGrads, EnvParams, OSCBatchSolver
from osc_amd.synth import SEED_BASE, generate

REP = 10
small = "--small" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REP):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


lines = []
for robot in ("unitree_go2", "walter_sr"):
    solver = OSCBatchSolver(robot)
    d, desc = solver.dims, solver.desc
    for nenv in ((4096,) if small else (4096, 65536)):
        M, C, J, b, T, mask = solver.prepare(**generate(robot, nenv, SEED_BASE + 11, "tumbling",
                                                        "bernoulli"))
        rep = lambda v: torch.tensor(np.broadcast_to(np.asarray(v, float), (nenv,) + np.shape(v)).copy(),
                                     device=dev)
        blk = EnvParams(mu=rep(desc.mu), u_lb=rep(list(desc.u_lb)[:d["nu"]]),
                        u_ub=rep(list(desc.u_ub)[:d["nu"]]), fz_lb=rep(desc.z_lb[2]),
                        fz_ub=rep(desc.z_ub[2]), w_pos=rep(list(desc.w_pos)[:d["ns"]]),
                        w_rot=rep(list(desc.w_rot)[:d["ns"]]))
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        solver.solve_into(out, M, C, J, b, T, mask, env_params=blk)
        gx = torch.randn((nenv, d["n"]), dtype=torch.float64, device=dev)
        new = lambda *s: torch.empty((nenv,) + s, dtype=torch.float64, device=dev)
        g = dict(grad_M=new(d["nv"], d["nv"]), grad_C=new(d["nv"]), grad_J=new(d["s"], d["nv"]),
                 grad_wrow=new(d["s"]), grad_T=new(d["ns"], 6), grad_b=new(d["s"]))
        g2 = {k: torch.empty_like(v) for k, v in g.items()}
        eg = EnvGrads.empty(nenv, d, dev)
        eg_par = EnvGrads.empty(nenv, d, dev, ("mu", "u_lb", "u_ub", "fz_lb", "fz_ub"))
        # (the parameter block is staged once: the timed calls pass device tensors only)
        calls = dict(
            a=lambda: solver.backward_data_into(out, M, J, b, T, mask, gx, **g),
            b=lambda: solver.backward_env_into(out, M, J, b, T, mask, gx, env_params=blk, **g2),
            c=lambda: solver.backward_env_into(out, M, J, b, T, mask, gx, env_params=blk,
                                               env_grads=eg, **g2),
            d=lambda: solver.backward_env_into(out, M, J, b, T, mask, gx, env_params=blk,
                                               env_grads=eg_par))
        for _ in range(2):
            for fn in calls.values():
                timed(fn)
        t = {k: [] for k in calls}
        for _ in range(7):
            for k, fn in calls.items():
                t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        line = dict(robot=robot, nenv=nenv, rep=REP, status_ok=int((out.status == 0).sum().item()),
                    backward_data_ms=stats(t["a"]), backward_env_data_ms=stats(t["b"]),
                    backward_env_all_ms=stats(t["c"]), backward_env_params_only_ms=stats(t["d"]),
                    b_over_a=med["b"] / med["a"], c_over_a=med["c"] / med["a"],
                    d_over_a=med["d"] / med["a"],
                    data_bitwise=all(bool(torch.equal(g[k], g2[k])) for k in g),
                    param_grads_finite=all(bool(torch.isfinite(getattr(eg, k)).all().item())
                                           for k in EnvGrads.FIELDS))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del M, C, J, b, T, mask, blk, out, gx, g, g2, eg, eg_par, calls
        torch.cuda.empty_cache()
if out_path:
    with open(out_path, "w") as f:
        json.dump(lines, f, indent=1)
