"""Host side of the GPU kinematics front end (include/osc_kinematics.h).

Reference interface this mirrors (paths relative to the reference's operational-space-control/):
  * update_mj_data()   unitree_go2/operational_space_controller.h:350-374
      -> KinematicsBatch.state_to_qpos(...) (qpos = [0,0,0, quat, q_m], qvel = [v, w, qd_m])
  * update_osc_data()  :376-455 (mj_fullM, qfrc_bias, mj_jac / mj_jacDot per site)
      -> KinematicsBatch.compute(qpos, qvel) -> (M, C, J, b, site_xpos), the inputs of
         OSCBatchSolver.solve
  * the whole tick (update_mj_data .. solve_optimization, :546-573)
      -> KinematicsBatch.solve(solver, qpos, qvel, T, mask)   (osc_batch_solve_qpos)
Beyond the reference (include/osc_rollout.h): KinematicsBatch.rollout(...) runs K closed-loop
ticks on the device by integrating the QP's own acceleration (an idealised rollout over the
controller's model, not a simulator), KinematicsBatch.integrate_into(...) is its step alone.
include/osc_plant.h: KinematicsBatch.forward_dynamics(...) is qacc = M^-1 (B u + Jc' z + qfrc - C),
and rollout(..., plant=Plant(...)) integrates that of a plant with its own mass / COM / armature
and applied forces instead of the QP's dv (still no ground).
include/osc_plant_backward.h: KinematicsBatch.forward_dynamics_backward(...) is the forward
dynamics' vector-Jacobian product and rollout_plant_backward(...) the plant rollout's backward
(autograd.forward_dynamics_differentiable and rollout_plant_differentiable wrap the pairs).
The kinematic tree comes from operational-space-control_amd/config/<robot>_kinematics.json
(illustrative trees: the reference's MJCF files are not vendored) or from any osc_kin_desc.
Launches go through the C-ABI on the current torch stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses
import json
import os

import numpy as np
import torch

from . import _lib
from .robots import CONFIG_DIR

KIN_ROBOTS = {"unitree_go2": "unitree_go2", "walter_sr": "walter_sr",
              "walter_sr_wheels": "walter_sr"}   # wheels config: same robot, other weights


def kin_json_path(robot: str) -> str:
    return os.path.join(CONFIG_DIR, f"{KIN_ROBOTS.get(robot, robot)}_kinematics.json")


def load_tree(robot: str) -> dict:
    with open(kin_json_path(robot)) as f:
        return json.load(f)


@dataclasses.dataclass
class KinOutputs:
    M: torch.Tensor            # (nenv, nv, nv)
    C: torch.Tensor            # (nenv, nv)
    J: torch.Tensor            # (nenv, 6ns, nv)
    b: torch.Tensor            # (nenv, 6ns)
    site_xpos: torch.Tensor | None = None   # (nenv, ns, 3)


@dataclasses.dataclass
class KinEnvParams:
    """Per-env inertial parameters of the kinematics (osc_kin_env_params,
    include/osc_kin_env_params.h), each None (= the model's value for every env) or a float64
    torch tensor / numpy array, env-major:
      mass_scale (nenv, nbody)       m' = s m and Ib' = s Ib (density scaling)
      com_offset (nenv, nbody, 3)    ipos' = ipos + d, body frame
      armature_scale (nenv, nv)      dof_armature' = a dof_armature
    Shapes and dtypes are checked on the host when a KinematicsBatch takes the block (ValueError
    before any launch); the values are checked per env on the device, where an invalid env (a NaN
    or non-finite value, a mass_scale <= 0, an armature_scale < 0) gets NaN M and C, so that its
    solve returns OSC_SOLVE_NUMERICAL, and leaves the others untouched."""
    mass_scale: object = None
    com_offset: object = None
    armature_scale: object = None

    FIELDS = ("mass_scale", "com_offset", "armature_scale")

    def __post_init__(self):
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is None:
                continue
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise TypeError(f"KinEnvParams.{name}: expected torch.Tensor or numpy array")
            if a.dtype not in (np.float64, torch.float64):
                raise ValueError(f"KinEnvParams.{name}: expected float64, got {a.dtype}")

    def to_device(self, nenv: int, nbody: int, nv: int, device) -> tuple:
        """(osc_kin_env_params struct, the device tensors it points to -- keep them alive until
        the launch is enqueued).  Raises ValueError on a wrong shape, before anything is copied."""
        want = dict(mass_scale=(nenv, nbody), com_offset=(nenv, nbody, 3),
                    armature_scale=(nenv, nv))
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is not None and tuple(a.shape) != want[name]:
                raise ValueError(f"KinEnvParams.{name}: expected shape {want[name]}, got "
                                 f"{tuple(a.shape)}")
        c, keep = _lib.OscKinEnvParams(), []
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is None:
                continue
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(np.ascontiguousarray(a))
            a = a.to(device=device).contiguous()
            keep.append(a)
            setattr(c, name, a.data_ptr())
        return c, keep


@dataclasses.dataclass
class KinEnvGrads:
    """Gradient outputs of KinematicsBatch.backward_into with respect to the per-env parameters
    (osc_kin_env_grads, include/osc_kin_backward.h): float64 device tensors in KinEnvParams'
    shapes, each None (= not computed)."""
    mass_scale: torch.Tensor | None = None
    com_offset: torch.Tensor | None = None
    armature_scale: torch.Tensor | None = None

    @classmethod
    def empty(cls, nenv: int, nbody: int, nv: int, device, fields) -> "KinEnvGrads":
        shape = dict(mass_scale=(nenv, nbody), com_offset=(nenv, nbody, 3),
                     armature_scale=(nenv, nv))
        return cls(**{k: torch.empty(shape[k], dtype=torch.float64, device=device)
                      for k in fields})


class KinematicsBatch:
    def __init__(self, robot: str | None = None, tree: dict | None = None,
                 device: torch.device | int | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("KinematicsBatch needs a HIP device (no CPU fallback exists)")
        if tree is None and robot is None:
            raise ValueError("robot or tree required")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        desc = (_lib.kin_desc_from_dict(tree) if tree is not None else
                _lib.kin_desc_from_json(None, kin_json_path(robot)))
        self.desc = desc
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = _lib.lib().osc_kin_model_create(ctypes.byref(desc), ctypes.byref(h))
        if rc != 0:
            raise _lib.OSCError("osc_kin_model_create", rc)
        self._h = h
        nq, nv, ns = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.lib().osc_kin_model_dims(h, ctypes.byref(nq), ctypes.byref(nv), ctypes.byref(ns))
        self.nq, self.nv, self.ns = nq.value, nv.value, ns.value
        nb = ctypes.c_int32()
        _lib.lib().osc_kin_model_nbody(h, ctypes.byref(nb))
        self.nbody = nb.value   # after the MJCF reader's split of multi-joint bodies

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().osc_kin_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, a, shape, name):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        a = a.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        return a

    @staticmethod
    def _stream(stream, device):
        return (torch.cuda.current_stream(device) if stream is None else stream).cuda_stream

    def alloc(self, nenv: int, want_sites: bool = False) -> KinOutputs:
        o = dict(device=self.device, dtype=torch.float64)
        nv, s = self.nv, 6 * self.ns
        return KinOutputs(torch.empty((nenv, nv, nv), **o), torch.empty((nenv, nv), **o),
                          torch.empty((nenv, s, nv), **o), torch.empty((nenv, s), **o),
                          torch.empty((nenv, self.ns, 3), **o) if want_sites else None)

    def _kin_block(self, kin_params, nenv):
        """(osc_kin_env_params struct, tensors to keep alive) of a call with kin_params; host-side
        shape / dtype errors raise here, before any launch."""
        if not isinstance(kin_params, KinEnvParams):
            raise TypeError("kin_params: expected a KinEnvParams")
        return kin_params.to_device(nenv, self.nbody, self.nv, self.device)

    def _blocks(self, solver, env_params, kin_params, nenv):
        """byref arguments (osc_env_params*, osc_kin_env_params*) of an _env entry -- None = NULL --
        and what they point to."""
        keep, e, k = [], None, None
        if env_params is not None:
            c, kk = solver._env_block(env_params, nenv)
            keep += [c] + kk
            e = ctypes.byref(c)
        if kin_params is not None:
            c, kk = self._kin_block(kin_params, nenv)
            keep += [c] + kk
            k = ctypes.byref(c)
        return e, k, keep

    def compute_into(self, out: KinOutputs, qpos, qvel, stream=None,
                     kin_params=None) -> KinOutputs:
        """osc_batch_kinematics; with kin_params (a KinEnvParams) osc_batch_kinematics_env."""
        nenv = out.M.shape[0]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if kin_params is not None:
            c, keep = self._kin_block(kin_params, nenv)
            rc = _lib.lib().osc_batch_kinematics_env(
                self._h, nenv, ptr(qpos), ptr(qvel), ctypes.byref(c), ptr(out.M), ptr(out.C),
                ptr(out.J), ptr(out.b), ptr(out.site_xpos),
                ctypes.c_void_p(self._stream(stream, self.device)))
            if rc != 0:
                raise _lib.OSCError("osc_batch_kinematics_env", rc)
            return out
        rc = _lib.lib().osc_batch_kinematics(self._h, nenv, ptr(qpos), ptr(qvel), ptr(out.M),
                                             ptr(out.C), ptr(out.J), ptr(out.b),
                                             ptr(out.site_xpos),
                                             ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_kinematics", rc)
        return out

    def backward_into(self, qpos, qvel, grad_M=None, grad_C=None, grad_J=None, grad_b=None,
                      grad_site_xpos=None, grad_qpos=None, grad_qvel=None, kin_params=None,
                      kin_grads=None, stream=None):
        """osc_batch_kinematics_backward (include/osc_kin_backward.h), launch only: the
        vector-Jacobian product of compute_into.  grad_M .. grad_site_xpos are the cotangents
        (None = zero), grad_qpos (nenv, nq) / grad_qvel (nenv, nv) the outputs (None = not
        computed), kin_params the forward call's KinEnvParams, kin_grads a KinEnvGrads whose
        non-None fields are filled.  All float64 contiguous tensors on this device."""
        nenv = int(qpos.shape[0])
        nv, s = self.nv, 6 * self.ns
        want = dict(qpos=(nenv, self.nq), qvel=(nenv, nv), grad_M=(nenv, nv, nv),
                    grad_C=(nenv, nv), grad_J=(nenv, s, nv), grad_b=(nenv, s),
                    grad_site_xpos=(nenv, self.ns, 3), grad_qpos=(nenv, self.nq),
                    grad_qvel=(nenv, nv), mass_scale=(nenv, self.nbody),
                    com_offset=(nenv, self.nbody, 3), armature_scale=(nenv, nv))
        got = dict(qpos=qpos, qvel=qvel, grad_M=grad_M, grad_C=grad_C, grad_J=grad_J,
                   grad_b=grad_b, grad_site_xpos=grad_site_xpos, grad_qpos=grad_qpos,
                   grad_qvel=grad_qvel)
        if kin_grads is not None:
            if not isinstance(kin_grads, KinEnvGrads):
                raise TypeError("kin_grads: expected a KinEnvGrads")
            got.update({n: getattr(kin_grads, n) for n in KinEnvParams.FIELDS})
        for name, t in got.items():
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or \
                    t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous float64 tensor on {self.device}")
            if tuple(t.shape) != want[name]:
                raise ValueError(f"{name}: expected shape {want[name]}, got {tuple(t.shape)}")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        kp, keep = None, []
        if kin_params is not None:
            c, keep = self._kin_block(kin_params, nenv)
            keep.append(c)
            kp = ctypes.byref(c)
        kg = None
        if kin_grads is not None:
            cg = _lib.OscKinEnvGrads()
            for n in KinEnvParams.FIELDS:
                t = getattr(kin_grads, n)
                setattr(cg, n, t.data_ptr() if t is not None else None)
            kg = ctypes.byref(cg)
        rc = _lib.lib().osc_batch_kinematics_backward(
            self._h, nenv, ptr(qpos), ptr(qvel), kp, ptr(grad_M), ptr(grad_C), ptr(grad_J),
            ptr(grad_b), ptr(grad_site_xpos), ptr(grad_qpos), ptr(grad_qvel), kg,
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_kinematics_backward", rc)
        return grad_qpos, grad_qvel

    def compute(self, qpos, qvel, want_sites: bool = True, kin_params=None) -> KinOutputs:
        nenv = int(qpos.shape[0])
        qpos = self._dev(qpos, (nenv, self.nq), "qpos")
        qvel = self._dev(qvel, (nenv, self.nv), "qvel")
        with torch.cuda.device(self.device):
            return self.compute_into(self.alloc(nenv, want_sites), qpos, qvel,
                                     kin_params=kin_params)

    def state_to_qpos(self, body_rotation, linear_body_velocity, angular_body_velocity,
                      motor_position, motor_velocity, stream=None):
        """update_mj_data's packing (osc.h:357-361) for SoA batches of State fields."""
        nenv = int(body_rotation.shape[0])
        nu = self.nq - 7
        args = [self._dev(body_rotation, (nenv, 4), "body_rotation"),
                self._dev(linear_body_velocity, (nenv, 3), "linear_body_velocity"),
                self._dev(angular_body_velocity, (nenv, 3), "angular_body_velocity"),
                self._dev(motor_position, (nenv, nu), "motor_position"),
                self._dev(motor_velocity, (nenv, nu), "motor_velocity")]
        qpos = torch.empty((nenv, self.nq), dtype=torch.float64, device=self.device)
        qvel = torch.empty((nenv, self.nv), dtype=torch.float64, device=self.device)
        rc = _lib.lib().osc_state_to_qpos(nenv, nu, *[ctypes.c_void_p(a.data_ptr()) for a in args],
                                          ctypes.c_void_p(qpos.data_ptr()),
                                          ctypes.c_void_p(qvel.data_ptr()),
                                          ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_state_to_qpos", rc)
        return qpos, qvel

    def workspace_bytes(self, solver, nenv: int) -> int:
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_qpos_workspace_bytes(solver._h, self._h, nenv, ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_qpos_workspace_bytes", rc)
        return nb.value

    def env_workspace_bytes(self, solver, nenv: int) -> int:
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_qpos_env_workspace_bytes(solver._h, self._h, nenv, ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_qpos_env_workspace_bytes", rc)
        return nb.value

    def _solve_env_into(self, solver, out, warm, qpos, qvel, T, mask, workspace, stream,
                        env_params, kin_params):
        """osc_batch_solve_qpos_env (warm None = cold), launch only."""
        nenv = out.tau.shape[0]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        e, k, keep = self._blocks(solver, env_params, kin_params, nenv)
        ex = _lib.OscSolveExtras(None, out.y.data_ptr() if out.y is not None else None)
        rc = _lib.lib().osc_batch_solve_qpos_env(
            solver._h, self._h, nenv, ptr(qpos), ptr(qvel), ptr(T), ptr(mask), e, k,
            ctypes.byref(ex), ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters), ptr(warm),
            ctypes.c_size_t(0 if warm is None else warm.numel() * 8), ptr(workspace),
            ctypes.c_size_t(0 if workspace is None else workspace.numel() * 8),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_qpos_env", rc)
        return out

    def solve_into(self, solver, out, qpos, qvel, T, mask, workspace, stream=None,
                   env_params=None, kin_params=None):
        """osc_batch_solve_qpos: kinematics + QP assembly + interior point, launch only.  With
        env_params (a solver.EnvParams) or kin_params (a KinEnvParams) osc_batch_solve_qpos_env,
        its workspace a tensor of env_workspace_bytes."""
        if env_params is not None or kin_params is not None:
            return self._solve_env_into(solver, out, None, qpos, qvel, T, mask, workspace, stream,
                                        env_params, kin_params)
        nenv = out.tau.shape[0]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_solve_qpos(
            solver._h, self._h, nenv, ptr(qpos), ptr(qvel), ptr(T), ptr(mask), ptr(out.tau),
            ptr(out.x), ptr(out.status), ptr(out.iters), ptr(workspace),
            ctypes.c_size_t(0 if workspace is None else workspace.numel() * 8),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_qpos", rc)
        return out

    def solve_warm_into(self, solver, out, warm, qpos, qvel, T, mask, workspace, stream=None,
                        env_params=None, kin_params=None):
        """osc_batch_solve_qpos_warm: the tick from joint states, warm-started from `warm`.  With
        env_params or kin_params osc_batch_solve_qpos_env with that warm state."""
        if env_params is not None or kin_params is not None:
            if warm is None:
                raise ValueError("solve_warm_into: warm state required")
            return self._solve_env_into(solver, out, warm, qpos, qvel, T, mask, workspace, stream,
                                        env_params, kin_params)
        nenv = out.tau.shape[0]
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_solve_qpos_warm(
            solver._h, self._h, nenv, ptr(qpos), ptr(qvel), ptr(T), ptr(mask), ptr(out.tau),
            ptr(out.x), ptr(out.status), ptr(out.iters), ptr(warm),
            ctypes.c_size_t(0 if warm is None else warm.numel() * 8), ptr(workspace),
            ctypes.c_size_t(0 if workspace is None else workspace.numel() * 8),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_qpos_warm", rc)
        return out

    def solve(self, solver, qpos, qvel, T, mask, want_x: bool = False, env_params=None,
              kin_params=None):
        d = solver.dims
        nenv = int(qpos.shape[0])
        qpos = self._dev(qpos, (nenv, self.nq), "qpos")
        qvel = self._dev(qvel, (nenv, self.nv), "qvel")
        T = self._dev(T, (nenv, d["ns"], 6), "T")
        mask = self._dev(mask, (nenv, d["nc"]), "mask")
        env = env_params is not None or kin_params is not None
        if env:   # (shape errors: before anything is allocated or launched)
            self._blocks(solver, env_params, kin_params, nenv)
        out = solver.alloc_outputs(nenv, want_x)
        nbytes = self.env_workspace_bytes(solver, nenv) if env else \
            self.workspace_bytes(solver, nenv)
        ws = torch.empty((max(nbytes // 8, 2),), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            return self.solve_into(solver, out, qpos, qvel, T, mask, ws, env_params=env_params,
                                   kin_params=kin_params)

    # ---- closed-loop rollout over the controller's own model (include/osc_rollout.h) ----

    def integrate_into(self, qpos, qvel, qacc, dt, status=None, bad_ticks=None, stream=None):
        """osc_batch_integrate, in place on device tensors: qvel += dt qacc, then qpos =
        integratePos(qpos, qvel, dt).  qacc (nenv, nv) may be a strided view with contiguous rows,
        such as x[:, :nv] of a solve; an env whose status is OSC_SOLVE_NUMERICAL or whose qacc is
        not finite is left unchanged and counted in bad_ticks (int32), as every not-OK status is."""
        nenv = int(qpos.shape[0])
        if qacc.dim() != 2 or tuple(qacc.shape) != (nenv, self.nv) or \
                (self.nv > 1 and qacc.stride(1) != 1):
            raise ValueError(f"qacc: expected (nenv, {self.nv}) with contiguous rows")
        for name, t, dt_ in (("qpos", qpos, torch.float64), ("qvel", qvel, torch.float64),
                             ("qacc", qacc, torch.float64), ("status", status, torch.int32),
                             ("bad_ticks", bad_ticks, torch.int32)):
            if t is not None and (t.dtype != dt_ or t.device != self.device):
                raise ValueError(f"{name}: expected a {dt_} tensor on {self.device}")
        if not (qpos.is_contiguous() and qvel.is_contiguous()):
            raise ValueError("qpos / qvel: contiguous tensors required (updated in place)")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_integrate(
            self._h, nenv, float(dt), ptr(qacc), qacc.stride(0) if nenv > 1 else self.nv,
            ptr(status), ptr(qpos), ptr(qvel), ptr(bad_ticks),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_integrate", rc)
        return qpos, qvel

    # ---- forward dynamics and the rollout's plant (include/osc_plant.h) ----

    def forward_dynamics_into(self, solver, qacc, M, C, J, u, z=None, qfrc_applied=None,
                              stream=None):
        """osc_batch_forward_dynamics, launch only: qacc = M^-1 (B u + Jc' z + qfrc_applied - C)
        into qacc (nenv, nv), a contiguous float64 device tensor.  M (nenv, nv, nv), C (nenv, nv)
        and J (nenv, 6 ns, nv; may be None when z is) are contiguous; u (nenv, nu) and z
        (nenv, 3 nc) may be strided views with contiguous rows, such as x[:, nv:nv + nu] and
        x[:, nv + nu:] of a solve; qfrc_applied (nenv, nv) contiguous.  z / qfrc_applied None = no
        contact force / no applied force.  An env whose M is not positive definite, or with a
        non-finite input, gets a NaN row."""
        d = solver.dims
        nenv, nv = int(qacc.shape[0]), self.nv
        rows = dict(u=(u, d["nu"]), z=(z, 3 * d["nc"]))
        dense = dict(qacc=(qacc, (nenv, nv)), M=(M, (nenv, nv, nv)), C=(C, (nenv, nv)),
                     J=(J, (nenv, 6 * self.ns, nv)), qfrc_applied=(qfrc_applied, (nenv, nv)))
        for name, (t, shape) in dense.items():
            if t is None:
                if name in ("qacc", "M", "C") or (name == "J" and z is not None):
                    raise ValueError(f"{name}: required")
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or \
                    t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected a contiguous float64 tensor of shape {shape} "
                                 f"on {self.device}")
        stride = {}
        for name, (t, w) in rows.items():
            if t is None:
                if name == "u":
                    raise ValueError("u: required")
                stride[name] = 0
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or \
                    t.device != self.device or tuple(t.shape) != (nenv, w) or \
                    (w > 1 and t.stride(1) != 1):
                raise ValueError(f"{name}: expected (nenv, {w}) float64 with contiguous rows on "
                                 f"{self.device}")
            stride[name] = t.stride(0) if nenv > 1 else w
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_forward_dynamics(
            solver._h, nenv, ptr(M), ptr(C), ptr(J), ptr(u), stride["u"], ptr(z), stride["z"],
            ptr(qfrc_applied), ptr(qacc), ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_forward_dynamics", rc)
        return qacc

    def forward_dynamics(self, solver, qpos, qvel, tau, z=None, qfrc_applied=None,
                         kin_params=None):
        """qacc (nenv, nv) of joint states under torques tau (nenv, nu), contact forces z
        (nenv, 3 nc) and generalised applied forces qfrc_applied (nenv, nv), each of the last two
        optional: compute(kin_params=) and then forward_dynamics_into."""
        d = solver.dims
        nenv = int(qpos.shape[0])
        tau = self._dev(tau, (nenv, d["nu"]), "tau")
        z = None if z is None else self._dev(z, (nenv, 3 * d["nc"]), "z")
        f = None if qfrc_applied is None else self._dev(qfrc_applied, (nenv, self.nv),
                                                        "qfrc_applied")
        k = self.compute(qpos, qvel, want_sites=False, kin_params=kin_params)
        qacc = torch.empty((nenv, self.nv), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            return self.forward_dynamics_into(solver, qacc, k.M, k.C, k.J, tau, z, f)

    def forward_dynamics_backward(self, solver, M, J, z, qacc, grad_qacc, grad_M=None,
                                  grad_C=None, grad_Jc=None, grad_u=None, grad_z=None,
                                  grad_qfrc=None, stream=None):
        """osc_batch_forward_dynamics_backward (include/osc_plant_backward.h), launch only: with
        w = M^-1 grad_qacc, into the outputs that are given (None = not computed; at least one)
            grad_M (nenv, nv, nv) = -w qacc' (not symmetrised), grad_C (nenv, nv) = -w,
            grad_Jc (nenv, 3 nc, nv) = z w' (the contact rows only), grad_qfrc (nenv, nv) = w,
            grad_u (nenv, nu) = w[nv - nu:], grad_z (nenv, 3 nc) = Jc w.
        M, J and z are what forward_dynamics_into took (z None: J, grad_Jc and grad_z must be None
        too; J may be None unless grad_z is wanted) and qacc what it returned.  z, grad_qacc,
        grad_u and grad_z may be strided views with contiguous rows; everything else is
        contiguous.  An env the forward gave a NaN row, or with a non-finite entry in what is
        read here, gets zeros in every output.  Returns the dict of the outputs given."""
        d = solver.dims
        nenv, nv, nz = int(qacc.shape[0]), self.nv, 3 * d["nc"]
        dense = dict(M=(M, (nenv, nv, nv)), J=(J, (nenv, 6 * self.ns, nv)),
                     qacc=(qacc, (nenv, nv)), grad_M=(grad_M, (nenv, nv, nv)),
                     grad_C=(grad_C, (nenv, nv)), grad_Jc=(grad_Jc, (nenv, nz, nv)),
                     grad_qfrc=(grad_qfrc, (nenv, nv)))
        rows = dict(z=(z, nz), grad_qacc=(grad_qacc, nv), grad_u=(grad_u, d["nu"]),
                    grad_z=(grad_z, nz))
        if z is None and (J is not None or grad_Jc is not None or grad_z is not None):
            raise ValueError("z is None: J, grad_Jc and grad_z must be None as well")
        if grad_z is not None and J is None:
            raise ValueError("J: required for grad_z")
        outs = dict(M=grad_M, C=grad_C, Jc=grad_Jc, u=grad_u, z=grad_z, qfrc=grad_qfrc)
        if all(t is None for t in outs.values()):
            raise ValueError("forward_dynamics_backward: at least one output is required")
        for name, (t, shape) in dense.items():
            if t is None:
                if name in ("M", "qacc"):
                    raise ValueError(f"{name}: required")
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or \
                    t.device != self.device or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected a contiguous float64 tensor of shape {shape} "
                                 f"on {self.device}")
        stride = {}
        for name, (t, w) in rows.items():
            if t is None:
                if name == "grad_qacc":
                    raise ValueError("grad_qacc: required")
                stride[name] = 0
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or \
                    t.device != self.device or tuple(t.shape) != (nenv, w) or \
                    (w > 1 and t.stride(1) != 1) or (nenv > 1 and t.stride(0) < w):
                raise ValueError(f"{name}: expected (nenv, {w}) float64 with contiguous rows on "
                                 f"{self.device}")
            stride[name] = t.stride(0) if nenv > 1 else w
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_forward_dynamics_backward(
            solver._h, nenv, ptr(M), ptr(J), ptr(z), stride["z"], ptr(qacc), ptr(grad_qacc),
            stride["grad_qacc"], ptr(grad_M), ptr(grad_C), ptr(grad_Jc), ptr(grad_u),
            stride["grad_u"], ptr(grad_z), stride["grad_z"], ptr(grad_qfrc),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_forward_dynamics_backward", rc)
        return {k: t for k, t in outs.items() if t is not None}

    def _plant_block(self, plant, res, nenv, nticks, history):
        """(osc_rollout_plant struct, what it points to) of a rollout with plant=; with history the
        result's qacc_hist is allocated when the plant has a field.  Shape errors raise here."""
        if not isinstance(plant, Plant):
            raise TypeError("plant: expected a Plant")
        c, keep = _lib.OscRolloutPlant(), []
        if plant.kin_params is not None:
            kc, kk = self._kin_block(plant.kin_params, nenv)
            keep += [kc] + kk
            c.kin_params = ctypes.pointer(kc)
        if plant.qfrc_applied is not None:
            f = plant.qfrc_applied
            f = f if isinstance(f, torch.Tensor) else np.asarray(f, dtype=np.float64)
            if f.ndim == 3:
                f = self._dev(f, (nticks, nenv, self.nv), "plant.qfrc_applied")
                c.qfrc_applied_seq = f.data_ptr()
            else:
                f = self._dev(f, (nenv, self.nv), "plant.qfrc_applied")
                c.qfrc_applied = f.data_ptr()
            keep.append(f)
        if plant.active:
            res.plant = plant
            if history:
                res.qacc_hist = torch.zeros((nticks, nenv, self.nv), dtype=torch.float64,
                                            device=self.device)
                c.qacc_hist = res.qacc_hist.data_ptr()
        return c, keep

    def rollout_workspace_bytes(self, solver, nenv: int, nticks: int, env: bool = False,
                                plant: bool = False) -> int:
        """osc_rollout_workspace_bytes, (env) osc_rollout_env_workspace_bytes or (plant)
        osc_rollout_plant_workspace_bytes."""
        nb = ctypes.c_size_t()
        name = "osc_rollout_plant_workspace_bytes" if plant else \
            "osc_rollout_env_workspace_bytes" if env else "osc_rollout_workspace_bytes"
        rc = getattr(_lib.lib(), name)(solver._h, self._h, nenv, nticks, ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError(name, rc)
        return nb.value

    def _schedule(self, schedule, solver, nenv, nticks, pd_mode):
        """(osc_rollout_schedule, tensors name -> device tensor, per_env name -> 0 / 1) of a
        RolloutSchedule, its shapes validated against nticks."""
        d = solver.dims
        if not isinstance(schedule, RolloutSchedule):
            raise TypeError("schedule must be a RolloutSchedule")
        c, t, per_env = _lib.OscRolloutSchedule(), {}, {}
        if schedule.T is not None:
            t["T"] = self._dev(schedule.T, (nticks, nenv, d["ns"], 6), "schedule.T")
            c.T_seq = t["T"].data_ptr()
        if schedule.mask is not None:
            t["mask"] = self._dev(schedule.mask, (nticks, nenv, d["nc"]), "schedule.mask")
            c.mask_seq = t["mask"].data_ptr()
        for name, w in (("pos_ref", 3), ("quat_ref", 4)):
            r = getattr(schedule, name)
            if r is None:
                continue
            if not pd_mode:
                raise ValueError(f"schedule.{name}: a reference sequence needs PD targets (pd=)")
            r = r if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64)
            per_env[name] = int(r.ndim == 3)
            t[name] = self._dev(r, (nticks, nenv, w) if per_env[name] else (nticks, w),
                                "schedule." + name)
            setattr(c, name + "_seq", t[name].data_ptr())
        return c, t, per_env

    def _pd_args(self, a, pd, nenv, per_env_seq):
        """Fill a's PD fields from pd = (pos_ref, quat_ref, gains); a reference may be None when
        the schedule carries it (per_env_seq).  Returns the reference tensors (None = absent)."""
        pos_ref, quat_ref, gains = pd
        refs = {}
        for name, r, w in (("pos_ref", pos_ref, 3), ("quat_ref", quat_ref, 4)):
            if r is None:
                if name not in per_env_seq:
                    raise ValueError(f"{name}: None needs a schedule that carries it")
                setattr(a, name + "_per_env", per_env_seq[name])
                refs[name] = None
                continue
            r = r if isinstance(r, torch.Tensor) else np.asarray(r, dtype=np.float64)
            per = int(r.ndim == 2)
            if name in per_env_seq:     # the sequence's layout rules; it is what every tick reads
                per = per_env_seq[name]
            r = self._dev(r, (nenv, w) if per else (w,), name)
            setattr(a, name, r.data_ptr())
            setattr(a, name + "_per_env", per)
            refs[name] = r
        a.target_mode = _lib.ROLLOUT_TARGETS_PD_BASE
        a.gains[:] = [float(g) for g in gains]
        return refs

    def _target_args(self, a, T, pd, nenv, d, per_env_seq):
        """Fill a's target fields: PD targets from pd (_pd_args), else held targets T (None: the
        schedule's T alone).  Returns the tensors a points to."""
        if pd is not None:
            return [r for r in self._pd_args(a, pd, nenv, per_env_seq).values() if r is not None]
        a.target_mode = _lib.ROLLOUT_TARGETS_HELD
        if T is None:
            return []
        T = self._dev(T, (nenv, d["ns"], 6), "T")
        a.T = T.data_ptr()
        return [T]

    def rollout(self, solver, qpos, qvel, mask, nticks: int, dt: float, T=None, pd=None,
                warm: bool = True, history: bool = False, stream=None,
                workspace="alloc", env_params=None, kin_params=None,
                schedule=None, plant=None) -> "RolloutResult":
        """osc_batch_rollout: nticks ticks of kinematics -> targets -> solve -> step on the
        device, one enqueue, no host sync.  An idealised rollout over the controller's model, not
        a simulator: no ground, no contact detection; `mask` is an input, held constant unless
        the schedule carries one per tick.
        schedule (a RolloutSchedule): osc_batch_rollout_sched, inputs that change over the ticks.
        schedule.T (nticks, nenv, ns, 6) is ADDED to the tick's targets (the held T, which may
        then be None = 0, or the PD targets: a feed-forward); schedule.mask (nticks, nenv, nc)
        and schedule.pos_ref / quat_ref ((nticks, 3 | 4) shared or (nticks, nenv, 3 | 4) per env)
        replace the held ones, which may then be None (pd = (None, None, gains)).
        Exactly one of T (nenv, ns, 6), targets held over the rollout, and pd = (pos_ref,
        quat_ref, gains), osc_pd_base_targets of the current state every tick (references (3,) /
        (4,) shared or (nenv, 3) / (nenv, 4) per env; gains (kp_lin, kd_lin, kp_ang, kd_ang)).
        Inputs (torch tensors or numpy arrays) are copied: the caller's arrays are not modified.
        workspace: "alloc" = a tensor of rollout_workspace_bytes, None = the library's
        stream-ordered scratch, or a float64 device tensor.
        env_params (a solver.EnvParams) / kin_params (a KinEnvParams): osc_batch_rollout_env, both
        blocks held constant over the rollout; an env with invalid parameters stays frozen.
        plant (a Plant): osc_batch_rollout_plant (include/osc_plant.h): the step integrates the
        plant's forward dynamics of the tick's torques and contact forces -- its own mass / COM /
        armature, pushed by qfrc_applied -- instead of the QP's dv; the controller keeps using
        kin_params.  Still no ground: the contact forces are whatever the QP chose.  With
        history=True the result carries qacc_hist.  None or Plant() is bitwise the call without."""
        if T is not None and pd is not None:
            raise ValueError("at most one of T and pd may be given")
        if T is None and pd is None and (schedule is None or schedule.T is None):
            raise ValueError("one of T, pd and schedule.T must be given")
        d = solver.dims
        nenv, nticks = int(qpos.shape[0]), int(nticks)
        if schedule is not None and nticks < 0:
            raise ValueError("nticks < 0")
        nslab = max(nticks, 0)      # (a negative nticks without a schedule: the library's refusal)
        o = dict(device=self.device, dtype=torch.float64)
        qpos = self._dev(qpos, (nenv, self.nq), "qpos").clone()
        qvel = self._dev(qvel, (nenv, self.nv), "qvel").clone()
        sc, st, per_env_seq = (None, {}, {}) if schedule is None else \
            self._schedule(schedule, solver, nenv, nticks, pd is not None)
        a = _lib.OscRolloutArgs()
        a.nticks, a.dt, a.flags = nticks, float(dt), _lib.ROLLOUT_WARM if warm else 0
        keep = [qpos, qvel, sc] + list(st.values())
        if mask is not None:
            mask = self._dev(mask, (nenv, d["nc"]), "mask")
            a.contact_mask = mask.data_ptr()
            keep.append(mask)
        elif "mask" not in st:
            raise ValueError("mask: None needs a schedule that carries it")
        env = env_params is not None or kin_params is not None
        ep, kp, blocks = self._blocks(solver, env_params, kin_params, nenv) if env else \
            (None, None, [])
        keep += blocks
        keep += self._target_args(a, T, pd, nenv, d, per_env_seq)
        res = RolloutResult(qpos, qvel, torch.zeros((nenv, d["nu"]), **o),
                            torch.zeros((nenv,), device=self.device, dtype=torch.int32))
        if history:
            res.qpos_hist = torch.zeros((nslab + 1, nenv, self.nq), **o)
            res.qvel_hist = torch.zeros((nslab + 1, nenv, self.nv), **o)
            res.tau_hist = torch.zeros((nslab, nenv, d["nu"]), **o)
            res.status_hist = torch.zeros((nslab, nenv), device=self.device, dtype=torch.int32)
            a.qpos_hist, a.qvel_hist = res.qpos_hist.data_ptr(), res.qvel_hist.data_ptr()
            a.tau_hist, a.status_hist = res.tau_hist.data_ptr(), res.status_hist.data_ptr()
        pl = None
        if plant is not None:
            pl, pkeep = self._plant_block(plant, res, nenv, nslab, history)
            keep += [pl] + pkeep
        if isinstance(workspace, str):
            workspace = torch.empty((max(self.rollout_workspace_bytes(
                solver, nenv, nslab, env=env, plant=pl is not None) // 8, 2),), **o)
        if workspace is not None:
            a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
        a.qpos, a.qvel = qpos.data_ptr(), qvel.data_ptr()
        a.tau, a.bad_ticks = res.tau.data_ptr(), res.bad_ticks.data_ptr()
        s = ctypes.c_void_p(self._stream(stream, self.device))
        scp = ctypes.byref(sc) if sc is not None else None
        head = (solver._h, self._h, nenv, ctypes.byref(a))
        if pl is not None:
            entry, tail = "osc_batch_rollout_plant", (scp, ep, kp, ctypes.byref(pl), s)
        elif sc is not None:
            entry, tail = "osc_batch_rollout_sched", (scp, ep, kp, s)
        elif env:
            entry, tail = "osc_batch_rollout_env", (ep, kp, s)
        else:
            entry, tail = "osc_batch_rollout", (s,)
        with torch.cuda.device(self.device):
            rc = getattr(_lib.lib(), entry)(*head, *tail)
        if rc != 0:
            raise _lib.OSCError(entry, rc)
        res._keep = keep + [workspace]   # inputs and scratch stay alive until the stream is done
        return res

    # ---- the rollout's backward pass (include/osc_rollout_backward.h) ----

    def _grad_tensor(self, t, shape, name, dtype=torch.float64):
        """A launch-only argument: None, or a contiguous tensor of `dtype` and `shape` here."""
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or \
                not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous {dtype} tensor on {self.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def integrate_backward_into(self, qpos, qvel_new, qacc, dt, status=None, grad_qpos_new=None,
                                grad_qvel_new=None, grad_qpos=None, grad_qvel=None, grad_qacc=None,
                                stream=None):
        """osc_batch_integrate_backward, launch only: the vector-Jacobian product of integrate_into.
        qpos is the step's input, qvel_new its output velocity, qacc (nenv, nv) its accelerations
        (a strided view with contiguous rows is fine; read for the freeze rule only), status the
        status it was given.  grad_qpos_new / grad_qvel_new are the cotangents (None = zero);
        grad_qpos, grad_qvel and grad_qacc (which may be a strided view like qacc) the outputs
        (None = not computed).  A frozen env passes its cotangents through and gets grad_qacc 0."""
        nenv = int(qpos.shape[0])
        for name, t in (("qacc", qacc), ("grad_qacc", grad_qacc)):
            if t is not None and (t.dim() != 2 or tuple(t.shape) != (nenv, self.nv) or
                                  (self.nv > 1 and t.stride(1) != 1) or
                                  t.dtype != torch.float64 or t.device != self.device):
                raise ValueError(f"{name}: expected float64 (nenv, {self.nv}) with contiguous rows "
                                 f"on {self.device}")
        sq, sv = (nenv, self.nq), (nenv, self.nv)
        qpos = self._grad_tensor(qpos, sq, "qpos")
        qvel_new = self._grad_tensor(qvel_new, sv, "qvel_new")
        status = self._grad_tensor(status, (nenv,), "status", torch.int32)
        gqn = self._grad_tensor(grad_qpos_new, sq, "grad_qpos_new")
        gvn = self._grad_tensor(grad_qvel_new, sv, "grad_qvel_new")
        gq = self._grad_tensor(grad_qpos, sq, "grad_qpos")
        gv = self._grad_tensor(grad_qvel, sv, "grad_qvel")
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        stride = lambda t: t.stride(0) if t is not None and nenv > 1 else self.nv
        rc = _lib.lib().osc_batch_integrate_backward(
            self._h, nenv, float(dt), ptr(qpos), ptr(qvel_new), ptr(status), ptr(qacc),
            stride(qacc), ptr(gqn), ptr(gvn), ptr(gq), ptr(gv), ptr(grad_qacc), stride(grad_qacc),
            ctypes.c_void_p(self._stream(stream, self.device)))
        if rc != 0:
            raise _lib.OSCError("osc_batch_integrate_backward", rc)
        return grad_qpos, grad_qvel, grad_qacc

    def rollout_backward_workspace_bytes(self, solver, nenv: int) -> int:
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_rollout_backward_workspace_bytes(solver._h, self._h, nenv,
                                                             ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_rollout_backward_workspace_bytes", rc)
        return nb.value

    ROLLOUT_GRADS = ("qpos0", "qvel0", "T") + \
        tuple("env." + k for k in ("mu", "u_lb", "u_ub", "fz_lb", "fz_ub", "w_pos", "w_rot")) + \
        tuple("kin." + k for k in KinEnvParams.FIELDS)
    # include/osc_rollout_schedule.h's outputs (osc_rollout_schedule_grads, in its field order)
    ROLLOUT_SCHEDULE_GRADS = ("T_seq", "pos_ref", "quat_ref", "pos_ref_seq", "quat_ref_seq", "gains")

    def rollout_backward(self, solver, result, mask, dt, T=None, pd=None, grad_qpos_hist=None,
                         grad_qvel_hist=None, grad_tau_hist=None, env_params=None,
                         kin_params=None, want=("qpos0", "qvel0"), stream=None,
                         workspace="alloc", schedule=None) -> dict:
        """osc_batch_rollout_backward: the vector-Jacobian product of rollout(..., history=True),
        one enqueue, no host sync.  `result` is that call's RolloutResult (its histories are the
        checkpoints), mask / dt / T or pd / env_params / kin_params that call's arguments.  The
        cotangents grad_qpos_hist (nticks + 1, nenv, nq), grad_qvel_hist (nticks + 1, nenv, nv)
        and grad_tau_hist (nticks, nenv, nu) are contiguous float64 device tensors or None
        (= zero); a loss on the final state is a cotangent on the last slab.  `want` names the
        gradients to compute, out of ROLLOUT_GRADS: "qpos0", "qvel0", "T" (held targets only: the
        sum over the ticks), "env.<field>" of solver.EnvParams, "kin.<field>" of KinEnvParams.
        With schedule= (the forward's RolloutSchedule) or one of ROLLOUT_SCHEDULE_GRADS in `want`
        the call is osc_batch_rollout_backward_sched (include/osc_rollout_schedule.h): "T_seq"
        (nticks, nenv, ns, 6), every tick's grad_T, stored and not summed -- the gradient of
        schedule.T, in PD mode the feed-forward's; "pos_ref" / "quat_ref", the held PD references'
        gradients summed over the ticks; "pos_ref_seq" / "quat_ref_seq", per tick, when the
        schedule carries the reference; "gains" (4,).  A shared reference's gradient and the
        gains' come back summed over the envs ((3,), (4,), (nticks, 3), ...), a per-env
        reference's per env.  dt and the mask get no gradient.
        Returns a dict name -> tensor."""
        if getattr(result, "plant", None) is not None:
            raise NotImplementedError(
                "rollout_backward: the result came from a rollout against a plant, and the "
                "matched model's gradients would be wrong for it (include/osc_plant.h, DESIGN.md "
                "§7.5); rollout_plant_backward differentiates through the plant")
        return self._rollout_backward(solver, result, mask, dt, T, pd, grad_qpos_hist,
                                      grad_qvel_hist, grad_tau_hist, env_params, kin_params, want,
                                      stream, workspace, schedule, False, None)

    def rollout_plant_backward_workspace_bytes(self, solver, nenv: int) -> int:
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_rollout_plant_backward_workspace_bytes(solver._h, self._h, nenv,
                                                                   ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_rollout_plant_backward_workspace_bytes", rc)
        return nb.value

    PLANT_GRADS = ("plant.qfrc_applied",) + tuple("plant.kin." + k for k in KinEnvParams.FIELDS)

    def rollout_plant_backward(self, solver, result, mask, dt, T=None, pd=None,
                               grad_qpos_hist=None, grad_qvel_hist=None, grad_tau_hist=None,
                               grad_qacc_hist=None, env_params=None, kin_params=None,
                               want=("qpos0", "qvel0"), stream=None, workspace="alloc",
                               schedule=None) -> dict:
        """osc_batch_rollout_plant_backward (include/osc_plant_backward.h): rollout_backward
        through the plant of rollout(..., history=True, plant=...), which is taken from
        result.plant.  One more cotangent, grad_qacc_hist (nticks, nenv, nv), and in `want`, next
        to rollout_backward's names, PLANT_GRADS: "plant.qfrc_applied" -- (nenv, nv), the sum over
        the ticks, for a held force (or none: the gradient at zero), (nticks, nenv, nv) for a
        per-tick one -- and "plant.kin.<field>" of the plant's KinEnvParams (it must have one).
        kin_params / "kin.<field>" stay the CONTROLLER's.  A result without a plant is
        rollout_backward, bitwise.  Returns a dict name -> tensor."""
        return self._rollout_backward(solver, result, mask, dt, T, pd, grad_qpos_hist,
                                      grad_qvel_hist, grad_tau_hist, env_params, kin_params, want,
                                      stream, workspace, schedule, True, grad_qacc_hist)

    def _rollout_backward(self, solver, result, mask, dt, T, pd, grad_qpos_hist, grad_qvel_hist,
                          grad_tau_hist, env_params, kin_params, want, stream, workspace,
                          schedule, plant_call, grad_qacc_hist) -> dict:
        """rollout_backward and rollout_plant_backward (plant_call: the entry that takes a plant,
        whose block is NULL when the result has none)."""
        from .solver import EnvGrads
        me = "rollout_plant_backward" if plant_call else "rollout_backward"
        plant = getattr(result, "plant", None) if plant_call else None
        want = tuple(want)
        sched_call = schedule is not None or any(w in self.ROLLOUT_SCHEDULE_GRADS for w in want)
        if T is not None and pd is not None:
            raise ValueError("at most one of T and pd may be given")
        if T is None and pd is None and (schedule is None or schedule.T is None):
            raise ValueError("one of T, pd and schedule.T must be given")
        if result.qpos_hist is None or result.qvel_hist is None or result.status_hist is None:
            raise ValueError(f"{me}: the forward call needs history=True")
        for w in want:
            if w not in self.ROLLOUT_GRADS + self.ROLLOUT_SCHEDULE_GRADS + \
                    (self.PLANT_GRADS if plant is not None else ()):
                raise ValueError(f"{me}: unknown gradient {w!r}")
        if not want:
            raise ValueError(f"{me}: nothing asked for")
        if pd is not None and "T" in want:
            raise ValueError(f"{me}: no grad_T with PD targets")
        d = solver.dims
        nticks, nenv = int(result.status_hist.shape[0]), int(result.qpos_hist.shape[1])
        o = dict(device=self.device, dtype=torch.float64)
        a = _lib.OscRolloutBackwardArgs()
        a.nticks, a.dt = nticks, float(dt)
        keep = []
        sc, st, per_env_seq = (None, {}, {}) if schedule is None else \
            self._schedule(schedule, solver, nenv, nticks, pd is not None)
        keep += [sc] + list(st.values())
        if mask is not None:
            mask = self._dev(mask, (nenv, d["nc"]), "mask")
            a.contact_mask = mask.data_ptr()
            keep.append(mask)
        elif "mask" not in st:
            raise ValueError("mask: None needs a schedule that carries it")
        env = env_params is not None or kin_params is not None
        ep, kp, blocks = self._blocks(solver, env_params, kin_params, nenv) if env else \
            (None, None, [])
        keep += blocks
        keep += self._target_args(a, T, pd, nenv, d, per_env_seq)
        hq = self._grad_tensor(result.qpos_hist, (nticks + 1, nenv, self.nq), "qpos_hist")
        hv = self._grad_tensor(result.qvel_hist, (nticks + 1, nenv, self.nv), "qvel_hist")
        hs = self._grad_tensor(result.status_hist, (nticks, nenv), "status_hist", torch.int32)
        gqh = self._grad_tensor(grad_qpos_hist, (nticks + 1, nenv, self.nq), "grad_qpos_hist")
        gvh = self._grad_tensor(grad_qvel_hist, (nticks + 1, nenv, self.nv), "grad_qvel_hist")
        gth = self._grad_tensor(grad_tau_hist, (nticks, nenv, d["nu"]), "grad_tau_hist")
        ptr = lambda t: t.data_ptr() if t is not None else None
        a.qpos_hist, a.qvel_hist = hq.data_ptr(), hv.data_ptr()
        a.status_hist = hs.data_ptr()
        a.grad_qpos_hist, a.grad_qvel_hist, a.grad_tau_hist = ptr(gqh), ptr(gvh), ptr(gth)
        out = RolloutGrads()
        shape = dict(qpos0=(nenv, self.nq), qvel0=(nenv, self.nv), T=(nenv, d["ns"], 6))
        for w in want:
            if w in shape:
                out[w] = torch.empty(shape[w], **o)
        a.grad_qpos0, a.grad_qvel0, a.grad_T = (ptr(out.get(k)) for k in ("qpos0", "qvel0", "T"))
        efields = [w[4:] for w in want if w.startswith("env.")]
        kfields = [w[4:] for w in want if w.startswith("kin.")]
        if efields:
            eg = EnvGrads.empty(nenv, d, self.device, efields)
            ceg = eg.to_struct(nenv, d, self.device)
            a.env_grads = ctypes.pointer(ceg)
            keep.append(ceg)
            out.update({"env." + k: getattr(eg, k) for k in efields})
        if kfields:
            kg = KinEnvGrads.empty(nenv, self.nbody, self.nv, self.device, kfields)
            ckg = _lib.OscKinEnvGrads(**{k: getattr(kg, k).data_ptr() for k in kfields})
            a.kin_grads = ctypes.pointer(ckg)
            keep.append(ckg)
            out.update({"kin." + k: getattr(kg, k) for k in kfields})
        pl = None
        if plant is not None:     # the forward's plant block, the cotangent, the plant's gradients
            pl = _lib.OscRolloutPlantBackward()
            if plant.kin_params is not None:
                kc, kk = self._kin_block(plant.kin_params, nenv)
                keep += [kc] + kk
                pl.kin_params = ctypes.pointer(kc)
            seq = False
            if plant.qfrc_applied is not None:
                f = plant.qfrc_applied
                f = f if isinstance(f, torch.Tensor) else np.asarray(f, dtype=np.float64)
                seq = f.ndim == 3
                f = self._dev(f, (nticks, nenv, self.nv) if seq else (nenv, self.nv),
                              "plant.qfrc_applied")
                setattr(pl, "qfrc_applied_seq" if seq else "qfrc_applied", f.data_ptr())
                keep.append(f)
            gah = self._grad_tensor(grad_qacc_hist, (nticks, nenv, self.nv), "grad_qacc_hist")
            pl.grad_qacc_hist = ptr(gah)
            keep.append(gah)
            if "plant.qfrc_applied" in want:
                g = torch.empty((nticks, nenv, self.nv) if seq else (nenv, self.nv), **o)
                setattr(pl, "grad_qfrc_applied_seq" if seq else "grad_qfrc_applied", g.data_ptr())
                out["plant.qfrc_applied"] = g
            pfields = [w[10:] for w in want if w.startswith("plant.kin.")]
            if pfields:
                if plant.kin_params is None:
                    raise ValueError("rollout_plant_backward: plant.kin.<field> needs a plant "
                                     "with kin_params")
                pg = KinEnvGrads.empty(nenv, self.nbody, self.nv, self.device, pfields)
                cpg = _lib.OscKinEnvGrads(**{k: getattr(pg, k).data_ptr() for k in pfields})
                pl.kin_grads = ctypes.pointer(cpg)
                keep.append(cpg)
                out.update({"plant.kin." + k: getattr(pg, k) for k in pfields})
        elif grad_qacc_hist is not None:
            raise ValueError(f"{me}: grad_qacc_hist, but the result has no plant and no qacc_hist")
        if isinstance(workspace, str):
            nbytes = self.rollout_plant_backward_workspace_bytes(solver, nenv) if pl is not None \
                else self.rollout_backward_workspace_bytes(solver, nenv)
            workspace = torch.empty((max(nbytes // 8, 2),), **o)
        if workspace is not None:
            a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
        s = ctypes.c_void_p(self._stream(stream, self.device))
        raw, sg = {}, None
        if sched_call:   # the library's outputs are per env
            sshape = dict(T_seq=(nticks, nenv, d["ns"], 6), pos_ref=(nenv, 3), quat_ref=(nenv, 4),
                          pos_ref_seq=(nticks, nenv, 3), quat_ref_seq=(nticks, nenv, 4),
                          gains=(nenv, 4))
            raw = {w: torch.empty(sshape[w], **o) for w in want if w in sshape}
            sg = _lib.OscRolloutScheduleGrads(**{"grad_" + w: t.data_ptr() for w, t in raw.items()})
        ref = lambda c: ctypes.byref(c) if c is not None else None
        head = (solver._h, self._h, nenv, ctypes.byref(a))
        if plant_call:
            entry, tail = "osc_batch_rollout_plant_backward", (ref(sc), ref(sg), ep, kp, ref(pl), s)
        elif sched_call:
            entry, tail = "osc_batch_rollout_backward_sched", (ref(sc), ref(sg), ep, kp, s)
        else:
            entry, tail = "osc_batch_rollout_backward", (ep, kp, s)
        with torch.cuda.device(self.device):
            rc = getattr(_lib.lib(), entry)(*head, *tail)
        if rc != 0:
            raise _lib.OSCError(entry, rc)
        for w, t in raw.items():     # a shared reference's and the gains': summed over the envs
            if w == "gains":
                t = t.sum(0)
            elif w in ("pos_ref", "quat_ref") and not getattr(a, w + "_per_env"):
                t = t.sum(0)
            elif w in ("pos_ref_seq", "quat_ref_seq") and not per_env_seq[w[:-4]]:
                t = t.sum(1)
            out[w] = t
        keep += [sg, pl] + list(raw.values())
        out._keep = keep + [workspace, hq, hv, hs, gqh, gvh, gth]   # alive until the stream is done
        return out


@dataclasses.dataclass
class RolloutSchedule:
    """Inputs of a rollout that change over its ticks (osc_rollout_schedule,
    include/osc_rollout_schedule.h); torch tensors or numpy arrays, tick-major, each optional.
    A base trajectory to follow is pos_ref / quat_ref; a gait is a stance / swing pattern in mask
    with swing-foot targets in T; a target sequence to optimise is T."""
    T: object = None          # (nticks, nenv, ns, 6): ADDED to the tick's held or PD targets
    mask: object = None       # (nticks, nenv, nc): tick t's contact mask
    pos_ref: object = None    # PD targets: (nticks, 3) shared or (nticks, nenv, 3) per env
    quat_ref: object = None   # likewise with 4


@dataclasses.dataclass
class Plant:
    """The plant of a rollout when it is not the controller's model (osc_rollout_plant,
    include/osc_plant.h).  kin_params: the PLANT's KinEnvParams (None = the controller's own);
    qfrc_applied: MuJoCo's generalised applied force, (nenv, nv) held over the rollout or
    (nticks, nenv, nv) per tick -- on a free root, entries 0..2 are a world-frame force at the base
    origin; a wrench on another body is the caller's J' f.  Plant() with neither is no plant."""
    kin_params: object = None
    qfrc_applied: object = None

    @property
    def active(self) -> bool:
        return self.kin_params is not None or self.qfrc_applied is not None


class RolloutGrads(dict):
    """rollout_backward's result: gradient name -> tensor."""
    _keep: list | None = None


@dataclasses.dataclass
class RolloutResult:
    qpos: torch.Tensor                        # (nenv, nq) state after the last tick
    qvel: torch.Tensor                        # (nenv, nv)
    tau: torch.Tensor                         # (nenv, nu) the last tick's torques
    bad_ticks: torch.Tensor                   # (nenv,) int32: ticks whose solve was not OK
    qpos_hist: torch.Tensor | None = None     # (nticks + 1, nenv, nq), slab 0 = the initial state
    qvel_hist: torch.Tensor | None = None     # (nticks + 1, nenv, nv)
    tau_hist: torch.Tensor | None = None      # (nticks, nenv, nu)
    status_hist: torch.Tensor | None = None   # (nticks, nenv) int32
    qacc_hist: torch.Tensor | None = None     # (nticks, nenv, nv): a plant rollout's accelerations
    plant: object = None                      # the Plant the rollout ran against (None: matched)
    _keep: list | None = None


def _tree_joints(tree: dict):
    """(type, body) of every joint in qpos order: a body's "joints" list, else its "joint"."""
    out = []
    for i, b in enumerate(tree["bodies"]):
        if "joints" in b:
            out += [(j["type"], i) for j in b["joints"]]
        elif b["joint"] != "none":
            out.append((b["joint"], i))
    return out


def random_states(tree: dict, nenv: int, seed: int, base_pos_zero: bool = True,
                  joint_range: float = 1.0, vel_scale: float = 1.0):
    """Seeded synthetic joint states for a tree: unit base / ball quaternions, hinge angles
    uniform in +-joint_range, slides in +-0.3 joint_range, velocities N(0, vel_scale^2); base
    position 0 as update_mj_data sets it (osc.h:358-359) unless base_pos_zero is False."""
    rng = np.random.default_rng(seed)
    joints = _tree_joints(tree)
    nqj = {"free": 7, "ball": 4, "slide": 1, "hinge": 1}
    nvj = {"free": 6, "ball": 3, "slide": 1, "hinge": 1}
    nq = sum(nqj[t] for t, _ in joints)
    nv = sum(nvj[t] for t, _ in joints)
    qpos = np.zeros((nenv, nq))
    qvel = vel_scale * rng.standard_normal((nenv, nv))
    qa = 0
    for t, _ in joints:
        if t == "free":
            if not base_pos_zero:
                qpos[:, qa:qa + 3] = 0.3 * rng.standard_normal((nenv, 3))
            q = rng.standard_normal((nenv, 4))
            qpos[:, qa + 3:qa + 7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        elif t == "ball":
            q = rng.standard_normal((nenv, 4))
            qpos[:, qa:qa + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
        elif t == "hinge":
            qpos[:, qa] = rng.uniform(-joint_range, joint_range, size=nenv)
        else:
            qpos[:, qa] = rng.uniform(-0.3 * joint_range, 0.3 * joint_range, size=nenv)
        qa += nqj[t]
    return qpos, qvel


def kinematics_pair_into(kin_a: KinematicsBatch, out_a: KinOutputs, qpos_a, qvel_a,
                         kin_b: KinematicsBatch, out_b: KinOutputs, qpos_b, qvel_b,
                         stream=None) -> None:
    """osc_batch_kinematics_pair (include/osc_mixed.h): two models' kinematics in one grid, each
    model's M, C, J, b bitwise compute_into's."""
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    side = lambda k, o, qp, qv: [k._h, o.M.shape[0], ptr(qp), ptr(qv), ptr(o.M), ptr(o.C),
                                 ptr(o.J), ptr(o.b)]
    rc = _lib.lib().osc_batch_kinematics_pair(
        *side(kin_a, out_a, qpos_a, qvel_a), *side(kin_b, out_b, qpos_b, qvel_b),
        ctypes.c_void_p(KinematicsBatch._stream(stream, kin_a.device)))
    if rc != 0:
        raise _lib.OSCError("osc_batch_kinematics_pair", rc)
