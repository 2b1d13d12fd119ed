"""Cost of the scheduled rollout (include/osc_rollout_schedule.h) on Go2 next to the
plain rollout and its backward, all in one process.  HIP events around REP whole rollouts of K = 50
ticks after a warm-up pass, ROUNDS interleaved rounds; per entry the median [min, max] over the
rounds (each opened by one unrecorded forward pass, so that no forward entry follows a backward
one), in ms PER TICK.  The schedules repeat the held values (and the feed-forward is zero), so
every entry solves the same problems and the differences are the interface's own:
  a_held, a_pd         osc_batch_rollout, held and PD targets (warm, with histories)
  b_held, b_pd         osc_batch_rollout_sched with an empty schedule: the same launches
  c_held_seq           held mode, T and the mask from the schedule alone: pointer offsets, no launch
  c_held_add           held mode, a held T plus T_seq: the addition, one launch per tick
  d_pd_ff_ref          PD targets + feed-forward + a position-reference sequence: one launch per tick
  e_bwd_held           osc_batch_rollout_backward -> grad_qpos0, grad_qvel0, grad_T
  e_bwd_held_seq       ..._backward_sched, T and the mask from the schedule, grad_T_seq as well
  e_bwd_pd             osc_batch_rollout_backward, PD targets -> grad_qpos0, grad_qvel0
  e_bwd_pd_seq         ..._backward_sched on d's forward -> also grad_T_seq, grad_pos_ref_seq,
                       grad_quat_ref, grad_gains (the combine's schedule outputs, and the recompute's addition)
One JSON line per size.

    python tools/rollout_schedule_timing.py   (ROLLOUT_SCHED_SIZES="4096,65536", ROLLOUT_SCHED_ROUNDS=5)
"""
import json
import os
import sys

REP = 2
K = 50
DT = 0.002
GAINS = (150.0, 25.0, 50.0, 10.0)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "operational-space-control_amd"))


def main():
    import numpy as np
    import torch
    from osc_amd.kinematics import KinematicsBatch, RolloutSchedule, load_tree, random_states
    from osc_amd.solver import OSCBatchSolver
    from osc_amd.synth import generate
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    sizes = [int(s) for s in os.environ.get("ROLLOUT_SCHED_SIZES", "4096,65536").split(",")]
    rounds = int(os.environ.get("ROLLOUT_SCHED_ROUNDS", "5"))
    o = dict(dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (REP * K)

    for nenv in sizes:
        qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5,
                                                                     vel_scale=0.1))
        d = generate(robot, nenv, 11, "standing", "ones")
        T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
        pos_ref = qp[:, 0:3] + torch.tensor([0.01, -0.01, -0.02], **o)
        quat_ref = np.array([1.0, 0.0, 0.0, 0.0])
        pd = (pos_ref, quat_ref, GAINS)
        tile = lambda a: a.unsqueeze(0).expand(K, *a.shape).contiguous()
        T_seq, mask_seq, ref_seq, ff = tile(T), tile(mask), tile(pos_ref), torch.zeros_like(tile(T))
        ws_f = torch.empty((kb.rollout_workspace_bytes(solver, nenv, K) // 8 + 2,), **o)
        ws_b = torch.empty((kb.rollout_backward_workspace_bytes(solver, nenv) // 8 + 2,), **o)
        fwd = lambda m, **kw: kb.rollout(solver, qp, qv, m, K, DT, history=True, workspace=ws_f,
                                         **kw)
        s_seq = RolloutSchedule(T=T_seq, mask=mask_seq)
        s_pd = RolloutSchedule(T=ff, pos_ref=ref_seq)
        pd_seq = (None, quat_ref, GAINS)
        res_h, res_p = fwd(mask, T=T), fwd(mask, pd=pd)
        gqh, gvh = torch.randn_like(res_h.qpos_hist), torch.randn_like(res_h.qvel_hist)
        gth = torch.randn_like(res_h.tau_hist)
        bwd = lambda res, m, want, **kw: kb.rollout_backward(
            solver, res, m, DT, grad_qpos_hist=gqh, grad_qvel_hist=gvh, grad_tau_hist=gth,
            want=want, workspace=ws_b, **kw)
        fns = dict(
            a_held=lambda: fwd(mask, T=T), a_pd=lambda: fwd(mask, pd=pd),
            b_held=lambda: fwd(mask, T=T, schedule=RolloutSchedule()),
            b_pd=lambda: fwd(mask, pd=pd, schedule=RolloutSchedule()),
            c_held_seq=lambda: fwd(None, schedule=s_seq),
            c_held_add=lambda: fwd(mask, T=T, schedule=RolloutSchedule(T=ff)),
            d_pd_ff_ref=lambda: fwd(mask, pd=pd_seq, schedule=s_pd),
            e_bwd_held=lambda: bwd(res_h, mask, ("qpos0", "qvel0", "T"), T=T),
            e_bwd_held_seq=lambda: bwd(res_h, None, ("qpos0", "qvel0", "T_seq"), schedule=s_seq),
            e_bwd_pd=lambda: bwd(res_p, mask, ("qpos0", "qvel0"), pd=pd),
            e_bwd_pd_seq=lambda: bwd(res_p, mask, ("qpos0", "qvel0", "T_seq", "pos_ref_seq",
                                                   "quat_ref", "gains"), pd=pd_seq, schedule=s_pd))
        same = {k: bool(torch.equal(fns[k]().qpos_hist, (res_h if "held" in k else res_p).qpos_hist))
                for k in ("b_held", "b_pd", "c_held_seq", "c_held_add", "d_pd_ff_ref")}
        for f in fns.values():
            timed(f)
        t = {k: [] for k in fns}
        for _ in range(rounds):
            timed(fns["a_held"])     # lead-in, not recorded: every recorded forward entry then
            for k, f in fns.items():     # follows a forward rollout, not the last round's backward
                t[k].append(timed(f))
        rec = dict(robot=robot, nenv=nenv, nticks=K, rep=REP, rounds=rounds,
                   status_ok=int((res_h.status_hist == 0).sum().item()), status_all=nenv * K,
                   histories_bitwise_the_plain_rollouts=same)
        rec.update({k + "_ms": [round(x, 5) for x in v] for k, v in t.items()})
        rec.update({k + "_median_ms": round(float(np.median(v)), 5) for k, v in t.items()})
        print(json.dumps(rec), flush=True)
        del res_h, res_p, gqh, gvh, gth, T_seq, mask_seq, ref_seq, ff, ws_f, ws_b, s_seq, s_pd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
