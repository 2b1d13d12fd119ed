"""Cost of the kinematics' backward pass (include/osc_kin_backward.h) on Go2, next
to the forward it recomputes and to the solve's backward it chains with, all in one process.  HIP
events around REP back-to-back launches after two warm-up passes, ROUNDS interleaved rounds; per
entry the median [min, max] over the rounds:
  kin             osc_batch_kinematics
  kin_bwd         osc_batch_kinematics_backward, all five cotangents -> grad_qpos, grad_qvel
  kin_bwd_mcjb    the same without grad_site_xpos (what the chain passes)
  kin_bwd_params  the same with the three parameter blocks and their three gradients as well
  solve_bwd       osc_batch_solve_backward_data -> grad_M, grad_C, grad_J, grad_b
  chain_bwd       solve_bwd then kin_bwd_mcjb: the two-launch backward of solve_differentiable_qpos
One JSON line per size, with the bytes each backward launch reads and writes per env.

    python tools/kin_backward_timing.py     (KIN_BWD_SIZES="4096,65536", KIN_BWD_ROUNDS=5)
"""
import json
import os
import sys

REP = 20
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "operational-space-control_amd"))


def main():
    import numpy as np
    import torch
    from osc_amd.kinematics import (KinEnvGrads, KinEnvParams, KinematicsBatch, load_tree,
                                    random_states)
    from osc_amd.solver import OSCBatchSolver
    from osc_amd.synth import generate
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    sizes = [int(s) for s in os.environ.get("KIN_BWD_SIZES", "4096,65536").split(",")]
    rounds = int(os.environ.get("KIN_BWD_ROUNDS", "5"))
    o = dict(dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP

    for nenv in sizes:
        qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5))
        d = generate(robot, nenv, 11, "standing", "ones")
        T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
        ko = kb.alloc(nenv, want_sites=True)
        kb.compute_into(ko, qp, qv)
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        solver.solve_into(out, ko.M, ko.C, ko.J, ko.b, T, mask)
        gx = torch.randn((nenv, solver.dims["n"]), **o)
        g = dict(M=torch.randn_like(ko.M), C=torch.randn_like(ko.C), J=torch.randn_like(ko.J),
                 b=torch.randn_like(ko.b), x=torch.randn_like(ko.site_xpos))
        gq, gv = torch.empty_like(qp), torch.empty_like(qv)
        kp = KinEnvParams(mass_scale=torch.ones((nenv, kb.nbody), **o),
                          com_offset=torch.zeros((nenv, kb.nbody, 3), **o),
                          armature_scale=torch.ones((nenv, kb.nv), **o))
        kg = KinEnvGrads.empty(nenv, kb.nbody, kb.nv, dev, KinEnvParams.FIELDS)

        def kin_bwd(sites=True, params=False):
            kb.backward_into(qp, qv, grad_M=g["M"], grad_C=g["C"], grad_J=g["J"], grad_b=g["b"],
                             grad_site_xpos=g["x"] if sites else None, grad_qpos=gq, grad_qvel=gv,
                             kin_params=kp if params else None, kin_grads=kg if params else None)

        def solve_bwd():
            solver.backward_data_into(out, ko.M, ko.J, ko.b, T, mask, gx, grad_M=g["M"],
                                      grad_C=g["C"], grad_J=g["J"], grad_b=g["b"])

        fns = dict(kin=lambda: kb.compute_into(ko, qp, qv), kin_bwd=kin_bwd,
                   kin_bwd_mcjb=lambda: kin_bwd(sites=False),
                   kin_bwd_params=lambda: kin_bwd(params=True), solve_bwd=solve_bwd,
                   chain_bwd=lambda: (solve_bwd(), kin_bwd(sites=False)))
        for _ in range(2):
            for f in fns.values():
                timed(f)
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                t[k].append(timed(f))
        nq, nv, ns, nb = kb.nq, kb.nv, kb.ns, kb.nbody
        cot = nv * nv + nv + 6 * ns * nv + 6 * ns + 3 * ns
        rec = dict(robot=robot, nenv=nenv, rep=REP, rounds=rounds,
                   status_ok=int((out.status == 0).sum().item()),
                   kin_bwd_bytes_per_env=8 * (2 * (nq + nv) + cot),
                   kin_bwd_params_bytes_per_env=8 * (2 * (nq + nv) + cot + 2 * (4 * nb + nv)),
                   kin_bytes_per_env=8 * (nq + nv + cot))
        rec.update({k + "_ms": [round(x, 5) for x in v] for k, v in t.items()})
        rec.update({k + "_median_ms": round(float(np.median(v)), 5) for k, v in t.items()})
        print(json.dumps(rec), flush=True)
        del qp, qv, T, mask, ko, out, gx, g, gq, gv, kp, kg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
