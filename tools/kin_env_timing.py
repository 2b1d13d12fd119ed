"""Cost of the per-env kinematics parameters (include/osc_kin_env_params.h): A/B
across source trees, e.g. this tree against a checkout of its parent commit, each with its own
built library.  Every tree runs in its own child process (its own osc_amd package and library), the
processes interleaved round by round.  Per tree and size, HIP events around REP back-to-back
launches after two warm-up passes:
  kin        osc_batch_kinematics
  tick_warm  osc_batch_solve_qpos_warm, the state alternating between two joint-state batches
and, where the tree has them,
  kin_env        osc_batch_kinematics_env with all three fields (kin_env_<field>: that one alone)
  tick_warm_env  osc_batch_solve_qpos_env, warm, with both blocks
The blocks hold identity values (1, 0, 1) and the model's own constants, so every variant solves
the same QPs and the iteration counts are equal.  One JSON line per (tree, round, size).

    python tools/kin_env_timing.py TREE [TREE ...]     (TREE: a directory holding osc_amd/;
                                                        KIN_ENV_SIZES="4096,65536", KIN_ENV_ROUNDS=5)
"""
import json
import os
import subprocess
import sys

REP = 20


def child(pkg, sizes):
    sys.path.insert(0, pkg)
    import numpy as np
    import torch
    from osc_amd import kinematics as K
    from osc_amd.kinematics import KinematicsBatch, load_tree, random_states
    from osc_amd.solver import EnvParams, OSCBatchSolver
    from osc_amd.synth import generate
    robot = "unitree_go2"
    dev = torch.device("cuda", 0)
    tree = load_tree(robot)
    kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver(robot)
    has_env = hasattr(K, "KinEnvParams")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(REP):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP

    for nenv in sizes:
        qa, va = (torch.from_numpy(a).to(dev) for a in random_states(tree, nenv, 11,
                                                                     joint_range=0.5))
        qb = qa + 0.01
        d = generate(robot, nenv, 11, "standing", "ones")
        T, mask = torch.from_numpy(d["T"]).to(dev), torch.from_numpy(d["mask"]).to(dev)
        ko = kb.alloc(nenv)
        outs = [solver.alloc_outputs(nenv) for _ in range(2)]
        warms = [solver.alloc_warm_state(nenv) for _ in range(2)]
        ws = torch.empty((kb.workspace_bytes(solver, nenv) // 8 + 2,), dtype=torch.float64,
                         device=dev)
        fns = dict(
            kin=lambda i: kb.compute_into(ko, qa, va),
            tick_warm=lambda i: kb.solve_warm_into(solver, outs[0], warms[0], qb if i % 2 else qa,
                                                   va, T, mask, ws))
        if has_env:
            o = dict(dtype=torch.float64, device=dev)
            kp = K.KinEnvParams(mass_scale=torch.ones((nenv, kb.nbody), **o),
                                com_offset=torch.zeros((nenv, kb.nbody, 3), **o),
                                armature_scale=torch.ones((nenv, kb.nv), **o))
            m, n = solver.desc, solver.dims
            full = lambda v, w: torch.tensor(list(v)[:w], **o).repeat(nenv, 1)
            col = lambda v: torch.full((nenv,), float(v), **o)
            ep = EnvParams(mu=col(m.mu), u_lb=full(m.u_lb, n["nu"]), u_ub=full(m.u_ub, n["nu"]),
                           fz_lb=col(m.z_lb[2]), fz_ub=col(m.z_ub[2]), w_pos=full(m.w_pos, n["ns"]),
                           w_rot=full(m.w_rot, n["ns"]))
            for f in K.KinEnvParams.FIELDS:   # one field alone: where the kernel's extra time goes
                one = K.KinEnvParams(**{f: getattr(kp, f)})
                fns["kin_env_" + f] = lambda i, one=one: kb.compute_into(ko, qa, va, kin_params=one)
            fns.update(
                kin_env=lambda i: kb.compute_into(ko, qa, va, kin_params=kp),
                tick_warm_env=lambda i: kb.solve_warm_into(
                    solver, outs[1], warms[1], qb if i % 2 else qa, va, T, mask, ws,
                    env_params=ep, kin_params=kp))
        for _ in range(2):
            for f in fns.values():
                timed(f)
        t = {k: [] for k in fns}
        for _ in range(3):
            for k, f in fns.items():
                t[k].append(timed(f))
        rec = dict(robot=robot, nenv=nenv, rep=REP,
                   status_ok=int((outs[0].status == 0).sum().item()),
                   iters=int(outs[0].iters.sum().item()))
        if has_env:
            rec.update(status_ok_env=int((outs[1].status == 0).sum().item()),
                       iters_env=int(outs[1].iters.sum().item()))
        rec.update({k + "_ms": [round(x, 5) for x in v] for k, v in t.items()})
        rec.update({k + "_median_ms": round(float(np.median(v)), 5) for k, v in t.items()})
        print(json.dumps(rec), flush=True)
        del qa, va, qb, T, mask, ko, outs, warms, ws
        torch.cuda.empty_cache()


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2], [int(s) for s in sys.argv[3].split(",")])
        return
    sizes = os.environ.get("KIN_ENV_SIZES", "4096,65536")
    for r in range(int(os.environ.get("KIN_ENV_ROUNDS", "5"))):
        for tree in sys.argv[1:]:
            out = subprocess.run([sys.executable, __file__, "--child", os.path.abspath(tree), sizes],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(out.stderr[-2000:], file=sys.stderr)
                sys.exit(out.returncode)
            for line in out.stdout.splitlines():
                if not line.startswith("{"):
                    continue
                rec = json.loads(line)
                rec.update(tree=tree, round=r)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
