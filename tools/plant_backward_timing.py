"""Cost of gradients through the plant (include/osc_plant_backward.h) on Go2, all in
one process, HIP events, ROUNDS interleaved rounds after a warm-up pass, the median [min, max] over
the rounds; one JSON line per size.

Per tick (ms) of the backward of a KR-tick rollout -- cold, held targets, a cotangent on the last
slab; grad qpos0 and qvel0, plus the plant's own gradients where there is a plant:
  e_backward     osc_batch_rollout_backward
  f_null_plant   osc_batch_rollout_plant_backward on a result without a plant: the same launches
  g_qfrc         a held qfrc_applied only, its gradient too: + the forward dynamics, its backward
                 and the routing launch per tick
  h_kin_qfrc     plant kin_params + qfrc_applied, the mass_scale gradient too: + the plant's
                 kinematics and its backward per tick as well
The new kernel alone (microseconds per launch over REP x K launches; the kinematics' M, C, J of
drawn states, u and z as strided views of an x-shaped buffer, a drawn cotangent):
  a_forward      osc_batch_forward_dynamics, for scale
  b_backward     osc_batch_forward_dynamics_backward, all six outputs (grad_u, grad_z strided)
  c_vectors      the same with grad_M and grad_Jc NULL: the factorisation and the solve, no outer
                 products
  d_no_contact   z = NULL: grad_M, grad_C, grad_u, grad_qfrc

    python tools/plant_backward_timing.py   (PLANT_SIZES="4096,65536", PLANT_ROUNDS=5)
"""
import json
import os
import sys

REP = 2
K = 50      # launches per repetition of the kernel-alone entries
KR = 10     # ticks of the rollouts whose backward is timed
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "operational-space-control_amd"))


def rollout_backward(torch, np, kb, solver, tree, nenv, rounds):
    """The per-tick entries e .. h of the module docstring: name -> times."""
    from osc_amd.kinematics import KinEnvParams, Plant, random_states
    from osc_amd.synth import generate
    dev = kb.device
    qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11, joint_range=0.5,
                                                                 vel_scale=0.1))
    d = generate("unitree_go2", nenv, 11, "standing", "ones")
    T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
    rng = np.random.default_rng(11)
    qfrc = torch.from_numpy(rng.uniform(-3, 3, (nenv, kb.nv))).to(dev)
    ms = torch.from_numpy(rng.uniform(0.8, 1.25, (nenv, kb.nbody))).to(dev)
    ws = torch.empty((kb.rollout_plant_backward_workspace_bytes(solver, nenv) // 8 + 2,),
                     dtype=torch.float64, device=dev)
    fwd = lambda plant: kb.rollout(solver, qp, qv, mask, KR, 0.002, T=T, warm=False, history=True,
                                   plant=plant)
    plants = dict(e_backward=None, f_null_plant=None, g_qfrc=Plant(qfrc_applied=qfrc),
                  h_kin_qfrc=Plant(kin_params=KinEnvParams(mass_scale=ms), qfrc_applied=qfrc))
    want = dict(e_backward=("qpos0", "qvel0"), f_null_plant=("qpos0", "qvel0"),
                g_qfrc=("qpos0", "qvel0", "plant.qfrc_applied"),
                h_kin_qfrc=("qpos0", "qvel0", "plant.qfrc_applied", "plant.kin.mass_scale"))
    res = {k: fwd(p) for k, p in plants.items()}
    gq = torch.zeros_like(res["e_backward"].qpos_hist)
    gq[-1] = 1.0
    call = lambda k: (kb.rollout_backward if k == "e_backward" else kb.rollout_plant_backward)(
        solver, res[k], mask, 0.002, T=T, grad_qpos_hist=gq, want=want[k], workspace=ws)

    def timed(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (REP * KR)

    same = bool(torch.equal(call("e_backward")["qpos0"], call("f_null_plant")["qpos0"]))
    for k in plants:
        timed(k)
    t = {k: [] for k in plants}
    for _ in range(rounds):
        for k in plants:
            t[k].append(timed(k))
    rec = dict(backward_nticks=KR, null_plant_bitwise_the_backward=same,
               envs_with_bad_ticks={k: int((r.bad_ticks != 0).sum().item())
                                    for k, r in res.items()})
    rec.update({k + "_ms": [round(v, 5) for v in vs] for k, vs in t.items()})
    rec.update({k + "_median_ms": round(float(np.median(vs)), 5) for k, vs in t.items()})
    return rec


def main():
    import numpy as np
    import torch
    from osc_amd.kinematics import KinematicsBatch, load_tree, random_states
    from osc_amd.solver import OSCBatchSolver
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    sizes = [int(s) for s in os.environ.get("PLANT_SIZES", "4096,65536").split(",")]
    rounds = int(os.environ.get("PLANT_ROUNDS", "5"))
    o = dict(dtype=torch.float64, device=dev)
    nv, nu, nz = kb.nv, solver.dims["nu"], 3 * solver.dims["nc"]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP * K):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / (REP * K)

    for nenv in sizes:
        qp, qv = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5,
                                                                     vel_scale=0.1))
        rng = np.random.default_rng(11)
        draw = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s)).to(dev)
        k0 = kb.compute(qp, qv, want_sites=False)
        x, gx = torch.zeros((nenv, nv + nu + nz), **o), torch.empty((nenv, nv + nu + nz), **o)
        x[:, nv:nv + nu], x[:, nv + nu:] = draw(-20, 20, nenv, nu), draw(0, 40, nenv, nz)
        u, z = x[:, nv:nv + nu], x[:, nv + nu:]
        qfrc, g = draw(-3, 3, nenv, nv), draw(-1, 1, nenv, nv)
        qacc = torch.empty((nenv, nv), **o)
        gM, gC, gJc = (torch.empty(s, **o) for s in ((nenv, nv, nv), (nenv, nv), (nenv, nz, nv)))
        gf = torch.empty((nenv, nv), **o)
        gu, gz = gx[:, nv:nv + nu], gx[:, nv + nu:]
        fwd = lambda: kb.forward_dynamics_into(solver, qacc, k0.M, k0.C, k0.J, u, z, qfrc)
        bw = lambda J_, z_, **out: kb.forward_dynamics_backward(solver, k0.M, J_, z_, qacc, g,
                                                                **out)
        fns = dict(a_forward=fwd,
                   b_backward=lambda: bw(k0.J, z, grad_M=gM, grad_C=gC, grad_Jc=gJc, grad_u=gu,
                                         grad_z=gz, grad_qfrc=gf),
                   c_vectors=lambda: bw(k0.J, z, grad_C=gC, grad_u=gu, grad_z=gz, grad_qfrc=gf),
                   d_no_contact=lambda: bw(None, None, grad_M=gM, grad_C=gC, grad_u=gu,
                                           grad_qfrc=gf))
        for f in fns.values():
            timed(f)
        bad = int((~torch.isfinite(qacc).all(dim=1)).sum().item())
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                t[k].append(timed(f))
        rec = dict(robot=robot, nenv=nenv, launches=REP * K, rounds=rounds, envs_with_nan_qacc=bad)
        rec.update({k + "_us": [round(v, 3) for v in vs] for k, vs in t.items()})
        rec.update({k + "_median_us": round(float(np.median(vs)), 3) for k, vs in t.items()})
        rec.update(rollout_backward(torch, np, kb, solver, tree, nenv, rounds))
        print(json.dumps(rec), flush=True)
        del k0, x, gx, qacc, gM, gC, gJc, gf, qfrc, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
