"""Backward-pass measurement of DESIGN.md §3.5: osc_batch_solve_backward and
osc_batch_solve_backward_data (all six outputs) against the forward solve_into with duals of the
same run, Go2 and WaLTER Sr at 4,096 and 65,536 envs (tumbling
batches, Bernoulli masks), and the forward with and without the duals the backward needs.  HIP
events around REP back-to-back launches of each, two warm-up rounds, seven timed rounds
alternating forward+duals / forward / backward / backward_data; median [min, max] per launch.  One JSON line per
configuration.

    python tools/backward_timing.py [--small]          (--small: 4,096 envs only)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/backward_timing.py --profile
        (Go2 and WaLTER, 4,096 envs, three forward + backward + backward_data rounds: the
        per-kernel times;
        profile in a run of its own)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "operational-space-control_amd")]
from osc_amd.solver import OSCBatchSolver
from osc_amd.synth import SEED_BASE, generate

REP = 10
profile, small = "--profile" in sys.argv, "--small" in sys.argv
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


for robot in ("unitree_go2", "walter_sr"):
    solver = OSCBatchSolver(robot)
    d = solver.dims
    for nenv in ((4096,) if (profile or small) else (4096, 65536)):
        args = solver.prepare(**generate(robot, nenv, SEED_BASE + 11, "tumbling", "bernoulli"))
        J, mask = args[2], args[5]
        out_y = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        out_n = solver.alloc_outputs(nenv, want_x=True)
        gx = torch.randn((nenv, d["n"]), dtype=torch.float64, device=dev)
        gT = torch.empty((nenv, d["ns"], 6), dtype=torch.float64, device=dev)
        gb = torch.empty((nenv, d["s"]), dtype=torch.float64, device=dev)
        fwd_y = lambda: solver.solve_into(out_y, *args)
        fwd_n = lambda: solver.solve_into(out_n, *args)
        bwd = lambda: solver.backward_into(out_y, J, mask, gx, gT, gb)
        gM = torch.empty((nenv, d["nv"], d["nv"]), dtype=torch.float64, device=dev)
        gC = torch.empty((nenv, d["nv"]), dtype=torch.float64, device=dev)
        gJ = torch.empty((nenv, d["s"], d["nv"]), dtype=torch.float64, device=dev)
        gW = torch.empty((nenv, d["s"]), dtype=torch.float64, device=dev)
        gT2, gb2 = torch.empty_like(gT), torch.empty_like(gb)
        bwd_d = lambda: solver.backward_data_into(out_y, args[0], J, args[3], args[4], mask, gx,
                                                  gM, gC, gJ, gW, gT2, gb2)
        if profile:
            for _ in range(3):
                fwd_y(); bwd(); bwd_d()
            torch.cuda.synchronize()
            print("profiled 3 forward + backward + backward_data rounds:", robot, nenv)
            continue
        for _ in range(2):
            timed(fwd_y); timed(fwd_n); timed(bwd); timed(bwd_d)
        ty, tn, tb, td = [], [], [], []
        for _ in range(7):
            ty.append(timed(fwd_y)); tn.append(timed(fwd_n)); tb.append(timed(bwd))
            td.append(timed(bwd_d))
        ok = int((out_y.status == 0).sum().item())
        print(json.dumps(dict(robot=robot, nenv=nenv, rep=REP, status_ok=ok,
                              grad_finite=bool(torch.isfinite(gT).all().item()),
                              forward_with_duals_ms=stats(ty), forward_ms=stats(tn),
                              backward_ms=stats(tb), backward_data_ms=stats(td),
                              data_grad_finite=bool(torch.isfinite(gM).all().item() and
                                                    torch.isfinite(gJ).all().item()),
                              same_grad_T=bool(torch.equal(gT, gT2)),
                              backward_data_over_forward_with_duals=float(np.median(td) / np.median(ty)),
                              backward_over_forward_with_duals=float(np.median(tb) / np.median(ty)),
                              duals_cost_ms=float(np.median(ty) - np.median(tn)))), flush=True)
        del args, J, mask, out_y, out_n, gx, gT, gb, gM, gC, gJ, gW, gT2, gb2
        torch.cuda.empty_cache()
