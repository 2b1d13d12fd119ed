"""Cost of the rollout's backward pass (include/osc_rollout_backward.h) on Go2, held
targets, K = 20 ticks, next to the forward rollout and to the parts it is made of, all in one
process.  HIP events around REP back-to-back calls after two warm-up passes, ROUNDS interleaved
rounds; per entry the median [min, max] over the rounds, in ms PER TICK:
  fwd           osc_batch_rollout (warm, with histories) / K
  bwd           osc_batch_rollout_backward -> grad_qpos0, grad_qvel0, grad_T / K
  recompute     osc_batch_kinematics + the cold solve with x and duals (one tick)
  solve_bwd     osc_batch_solve_backward_data -> grad_M, grad_C, grad_J, grad_b, grad_T
  kin_bwd       osc_batch_kinematics_backward from those four
  step_adj      osc_batch_integrate_backward alone (one of the two new launches per tick)
  new           bwd - recompute - solve_bwd - kin_bwd: the two new launches per tick (the combine
                kernel has no entry of its own), plus whatever the back-to-back parts hide
One JSON line per size.

    python tools/rollout_backward_timing.py   (ROLLOUT_BWD_SIZES="4096,65536", ROLLOUT_BWD_ROUNDS=5)
"""
import json
import os
import sys

REP = 3
K = 20
DT = 0.002
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "operational-space-control_amd"))


def main():
    import numpy as np
    import torch
    from osc_amd.kinematics import KinematicsBatch, load_tree, random_states
    from osc_amd.solver import OSCBatchSolver
    from osc_amd.synth import generate
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    sizes = [int(s) for s in os.environ.get("ROLLOUT_BWD_SIZES", "4096,65536").split(",")]
    rounds = int(os.environ.get("ROLLOUT_BWD_ROUNDS", "5"))
    o = dict(dtype=torch.float64, device=dev)

    def timed(fn, rep, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rep):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (rep * per)

    for nenv in sizes:
        qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5,
                                                                     vel_scale=0.1))
        d = generate(robot, nenv, 11, "standing", "ones")
        T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
        ws_f = torch.empty((kb.rollout_workspace_bytes(solver, nenv, K) // 8 + 2,), **o)
        ws_b = torch.empty((kb.rollout_backward_workspace_bytes(solver, nenv) // 8 + 2,), **o)
        res = kb.rollout(solver, qp, qv, mask, K, DT, T=T, history=True, workspace=ws_f)
        gqh, gvh = torch.randn_like(res.qpos_hist), torch.randn_like(res.qvel_hist)
        gth = torch.randn_like(res.tau_hist)
        # one tick's parts, on the last slab
        ko = kb.alloc(nenv)
        out = solver.alloc_outputs(nenv, want_x=True, want_y=True)
        gx = torch.randn((nenv, solver.dims["n"]), **o)
        g = dict(M=torch.empty_like(ko.M), C=torch.empty_like(ko.C), J=torch.empty_like(ko.J),
                 b=torch.empty_like(ko.b), T=torch.empty_like(T))
        gq, gv = torch.empty_like(qp), torch.empty_like(qv)
        q1, v1, v2 = res.qpos_hist[K - 1], res.qvel_hist[K - 1], res.qvel_hist[K]

        def recompute():
            kb.compute_into(ko, q1, v1)
            solver.solve_into(out, ko.M, ko.C, ko.J, ko.b, T, mask)

        def solve_bwd():
            solver.backward_data_into(out, ko.M, ko.J, ko.b, T, mask, gx, grad_M=g["M"],
                                      grad_C=g["C"], grad_J=g["J"], grad_b=g["b"], grad_T=g["T"])

        def kin_bwd():
            kb.backward_into(q1, v1, grad_M=g["M"], grad_C=g["C"], grad_J=g["J"], grad_b=g["b"],
                             grad_qpos=gq, grad_qvel=gv)

        def step_adj():
            kb.integrate_backward_into(q1, v2, out.x[:, :kb.nv], DT, status=out.status,
                                       grad_qpos_new=gqh[K], grad_qvel_new=gvh[K], grad_qpos=gq,
                                       grad_qvel=gv, grad_qacc=gx[:, :kb.nv])

        fns = dict(
            fwd=(lambda: kb.rollout(solver, qp, qv, mask, K, DT, T=T, history=True,
                                    workspace=ws_f), REP, K),
            bwd=(lambda: kb.rollout_backward(solver, res, mask, DT, T=T, grad_qpos_hist=gqh,
                                             grad_qvel_hist=gvh, grad_tau_hist=gth,
                                             want=("qpos0", "qvel0", "T"), workspace=ws_b), REP, K),
            recompute=(recompute, REP * K, 1), solve_bwd=(solve_bwd, REP * K, 1),
            kin_bwd=(kin_bwd, REP * K, 1), step_adj=(step_adj, REP * K, 1))
        for _ in range(2):
            for f in fns.values():
                timed(*f)
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                t[k].append(timed(*f))
        med = {k: float(np.median(v)) for k, v in t.items()}
        rec = dict(robot=robot, nenv=nenv, nticks=K, rep=REP, rounds=rounds,
                   status_ok=int((res.status_hist == 0).sum().item()), status_all=nenv * K)
        rec.update({k + "_ms": [round(x, 5) for x in v] for k, v in t.items()})
        rec.update({k + "_median_ms": round(m, 5) for k, m in med.items()})
        rec["new_median_ms"] = round(med["bwd"] - med["recompute"] - med["solve_bwd"] -
                                     med["kin_bwd"], 5)
        print(json.dumps(rec), flush=True)
        del res, gqh, gvh, gth, ko, out, gx, g, gq, gv, ws_f, ws_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
