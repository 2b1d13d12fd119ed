"""Rollout measurement of DESIGN.md §7: Go2, 4,096 envs, 200 warm ticks in PD mode -- one
osc_batch_rollout call against the same ticks driven from Python (osc_pd_base_targets +
solve_warm_into + integrate_into per tick), HIP events around each, two warm-up runs, seven timed
runs alternating; the two must agree bitwise.  Prints one JSON line.

    python tools/rollout_bench.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rollout_bench.py --profile
        (two rollouts only, for the per-kernel times; profile in a run of its own)"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "operational-space-control_amd")]
from osc_amd import _lib
from osc_amd.kinematics import KinematicsBatch, load_tree, random_states
from osc_amd.solver import OSCBatchSolver

NENV, NTICKS, DT = 4096, 200, 0.002
GAINS = (150.0, 25.0, 50.0, 10.0)
profile = "--profile" in sys.argv

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
tree = load_tree("unitree_go2")
kb, solver = KinematicsBatch(tree=tree), OSCBatchSolver("unitree_go2")
d = solver.dims
nq, nv, ns, nu = kb.nq, kb.nv, d["ns"], d["nu"]
qpos0, qvel0 = random_states(tree, NENV, 7, base_pos_zero=False, joint_range=0.5, vel_scale=0.0)
rng = np.random.default_rng(7)
pos_ref = qpos0[:, :3] + 0.02 * rng.standard_normal((NENV, 3))
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
q0, v0, pref, qref, mask = t(qpos0), t(qvel0), t(pos_ref), t([1.0, 0, 0, 0]), t(np.ones((NENV, d["nc"])))
p = lambda x: ctypes.c_void_p(x.data_ptr())
L = _lib.lib()
stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

# ---- the rollout call, everything preallocated ----
qp, qv = q0.clone(), v0.clone()
tau = torch.zeros((NENV, nu), dtype=torch.float64, device=dev)
bad = torch.zeros((NENV,), dtype=torch.int32, device=dev)
ws = torch.empty((kb.rollout_workspace_bytes(solver, NENV, NTICKS) // 8 + 2,), dtype=torch.float64, device=dev)
a = _lib.OscRolloutArgs()
a.nticks, a.dt, a.flags, a.target_mode = NTICKS, DT, _lib.ROLLOUT_WARM, _lib.ROLLOUT_TARGETS_PD_BASE
a.pos_ref, a.pos_ref_per_env, a.quat_ref, a.quat_ref_per_env = pref.data_ptr(), 1, qref.data_ptr(), 0
a.gains[:] = GAINS
a.contact_mask, a.qpos, a.qvel, a.tau, a.bad_ticks = (x.data_ptr() for x in (mask, qp, qv, tau, bad))
a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8


def run_rollout():
    qp.copy_(q0); qv.copy_(v0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = L.osc_batch_rollout(solver._h, kb._h, NENV, ctypes.byref(a), stream)
    e1.record()
    assert rc == 0, rc
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


# ---- the same ticks from Python ----
out = solver.alloc_outputs(NENV, want_x=True)
wstate = solver.alloc_warm_state(NENV)
qws = torch.empty((kb.workspace_bytes(solver, NENV) // 8 + 2,), dtype=torch.float64, device=dev)
Td = torch.empty((NENV, ns, 6), dtype=torch.float64, device=dev)
lq, lv = q0.clone(), v0.clone()
lbad = torch.zeros((NENV,), dtype=torch.int32, device=dev)
gains = (ctypes.c_double * 4)(*GAINS)
xdv = out.x[:, :nv]


def run_loop():
    lq.copy_(q0); lv.copy_(v0); wstate.zero_(); lbad.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(NTICKS):
        base = [lq[:, 0:3].contiguous(), lq[:, 3:7].contiguous(), lv[:, 0:3].contiguous(),
                lv[:, 3:6].contiguous()]
        L.osc_pd_base_targets(NENV, ns, *[p(x) for x in base], p(pref), 1, p(qref), 0, gains, p(Td), stream)
        kb.solve_warm_into(solver, out, wstate, lq, lv, Td, mask, qws)
        kb.integrate_into(lq, lv, xdv, DT, status=out.status, bad_ticks=lbad)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if profile:
    run_rollout()
    run_rollout()
    print("profiled 2 rollouts of", NTICKS, "ticks")
    sys.exit(0)

for _ in range(2):
    run_rollout(); run_loop()
assert torch.equal(qp, lq) and torch.equal(qv, lv) and torch.equal(bad, lbad), "rollout != loop"
r, l = [], []
for _ in range(7):
    r.append(run_rollout()); l.append(run_loop())
res = dict(nenv=NENV, nticks=NTICKS, bad_ticks_total=int(bad.sum().item()),
           rollout_ms=dict(median=float(np.median(r)), min=min(r), max=max(r)),
           loop_ms=dict(median=float(np.median(l)), min=min(l), max=max(l)),
           rollout_ticks_per_s=NTICKS / (np.median(r) * 1e-3),
           loop_ticks_per_s=NTICKS / (np.median(l) * 1e-3),
           rollout_ms_per_tick=float(np.median(r)) / NTICKS,
           loop_ms_per_tick=float(np.median(l)) / NTICKS)
# the existing warm joint-state tick alone on the final state (no step, no producer), same batch
ts = []
for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(NTICKS):
        kb.solve_warm_into(solver, out, wstate, lq, lv, Td, mask, qws)
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / NTICKS)
res["warm_tick_alone_ms_fixed_state"] = float(np.median(ts))
print(json.dumps(res))
