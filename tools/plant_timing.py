"""Cost of the rollout against a plant (include/osc_plant.h) on Go2 next to the
plain rollout, all in one process.  HIP events around REP whole rollouts of K = 50 ticks after a
warm-up pass, ROUNDS interleaved rounds; per entry the median [min, max] over the rounds, in ms
PER TICK.  Warm start, held targets, no histories:
  a_rollout      osc_batch_rollout
  b_null_plant   osc_batch_rollout_plant with an all-NULL plant: the same launches
  c_qfrc         a held qfrc_applied only: + the forward-dynamics launch per tick (the tick's M, C)
  d_kin_qfrc     plant kin_params + qfrc_applied: + the plant's kinematics launch per tick as well
and the forward-dynamics entry alone on one batch (fd_alone_us, microseconds per launch).
One JSON line per size.

    python tools/plant_timing.py   (PLANT_SIZES="4096,65536", PLANT_ROUNDS=5)
"""
import json
import os
import sys

REP = 2
K = 50
DT = 0.002
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "operational-space-control_amd"))


def main():
    import numpy as np
    import torch
    from osc_amd.kinematics import (KinEnvParams, KinematicsBatch, Plant, load_tree,
                                    random_states)
    from osc_amd.solver import OSCBatchSolver
    from osc_amd.synth import generate
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    sizes = [int(s) for s in os.environ.get("PLANT_SIZES", "4096,65536").split(",")]
    rounds = int(os.environ.get("PLANT_ROUNDS", "5"))
    o = dict(dtype=torch.float64, device=dev)
    nv, nu = kb.nv, solver.dims["nu"]

    def timed(fn, per=REP * K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / per

    for nenv in sizes:
        qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5,
                                                                     vel_scale=0.1))
        d = generate(robot, nenv, 11, "standing", "ones")
        T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
        rng = np.random.default_rng(11)
        qfrc = torch.from_numpy(rng.uniform(-3, 3, (nenv, nv))).to(dev)
        ms = torch.from_numpy(rng.uniform(0.8, 1.25, (nenv, kb.nbody))).to(dev)
        ws = torch.empty((kb.rollout_workspace_bytes(solver, nenv, K, plant=True) // 8 + 2,), **o)
        run = lambda **kw: kb.rollout(solver, qp, qv, mask, K, DT, T=T, workspace=ws, **kw)
        p_c = Plant(qfrc_applied=qfrc)
        p_d = Plant(kin_params=KinEnvParams(mass_scale=ms), qfrc_applied=qfrc)
        fns = dict(a_rollout=lambda: run(), b_null_plant=lambda: run(plant=Plant()),
                   c_qfrc=lambda: run(plant=p_c), d_kin_qfrc=lambda: run(plant=p_d))
        ref = run()
        same = bool(torch.equal(run(plant=Plant()).qpos, ref.qpos))
        bad = {k: int((fns[k]().bad_ticks != 0).sum().item()) for k in fns}
        k0 = kb.compute(qp, qv, want_sites=False)
        x = torch.zeros((nenv, nv + nu + 3 * solver.dims["nc"]), **o)
        qacc = torch.empty((nenv, nv), **o)
        fd = lambda: kb.forward_dynamics_into(solver, qacc, k0.M, k0.C, k0.J, x[:, nv:nv + nu],
                                              x[:, nv + nu:], qfrc)
        for f in fns.values():
            timed(f)
        t = {k: [] for k in fns}
        t_fd = []
        for _ in range(rounds):
            for k, f in fns.items():
                t[k].append(timed(f))
            t_fd.append(1e3 * timed(lambda: [fd() for _ in range(K)]))
        rec = dict(robot=robot, nenv=nenv, nticks=K, rep=REP, rounds=rounds,
                   envs_with_bad_ticks=bad, null_plant_bitwise_the_rollout=same)
        rec.update({k + "_ms": [round(v, 5) for v in vs] for k, vs in t.items()})
        rec.update({k + "_median_ms": round(float(np.median(vs)), 5) for k, vs in t.items()})
        rec.update(fd_alone_us=[round(v, 3) for v in t_fd],
                   fd_alone_median_us=round(float(np.median(t_fd)), 3))
        print(json.dumps(rec), flush=True)
        del ws, ref, k0, x, qacc, qfrc, ms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
