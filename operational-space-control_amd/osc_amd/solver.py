"""Host-side batched OSC solver: the reference's per-tick QP for a whole batch of environments.

Reference interface this mirrors (paths relative to the reference's operational-space-control/):
  * OperationalSpaceController(xml_path, control_rate_us, OsqpSettings)   osc.h:108
      -> OSCBatchSolver(robot, yaml_path, eps_mu, max_iter)   (model from the same YAML schema)
  * update_optimization_data() + update_optimization() + solve_optimization()  osc.h:457-536
      -> OSCBatchSolver.solve(M, C, J, b, T, mask)          (all environments in one launch)
  * get_torque_command() -> tau;  get_solution() -> x        osc.h:230-238
  * OsqpSolver::dual_solution -> y (want_y)                  osc.h:534-535
  * wheel no-slip rows (walter_sr_wheels/autogen/autogen.py:128-240, commented out upstream):
    a model whose YAML switches them on takes the per-env wheel directions (wheel_dir)
  * absl::Status error convention -> OSCError with the osc_status code.

Inputs are torch float64 CUDA tensors already resident in HBM (numpy arrays are copied to the
current device for convenience).  Everything is launched through the C-ABI
(include/osc_batch.h) on the current torch stream.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib
from .robots import config_path, dims


@dataclasses.dataclass
class SolveResult:
    tau: torch.Tensor          # (nenv, nu)
    x: torch.Tensor | None     # (nenv, nv + nu + 3nc) design vector (dv, u, z)
    status: torch.Tensor       # (nenv,) int32, 0 = converged
    iters: torch.Tensor        # (nenv,) int32, interior-point iterations
    workspace: torch.Tensor | None = None   # device scratch (reduced QP per env)
    y: torch.Tensor | None = None           # (nenv, dual_rows) dual solution (OSQP convention)


class EnvParams:
    """Per-env friction, torque and normal-force bounds and task weights (osc_env_params,
    include/osc_env_params.h), each None (= the model's value for every env) or a float64 torch
    tensor / numpy array, env-major:
      mu (nenv,), u_lb / u_ub (nenv, nu), fz_lb / fz_ub (nenv,), w_pos / w_rot (nenv, ns).
    Shapes and dtypes are checked on the host when a solver takes the block (ValueError before any
    launch); the values are checked per env on the device, where an invalid env (u_lb >= u_ub, a
    NaN, a non-finite mu or weight) returns OSC_SOLVE_NUMERICAL and leaves the others untouched."""
    FIELDS = ("mu", "u_lb", "u_ub", "fz_lb", "fz_ub", "w_pos", "w_rot")

    def __init__(self, mu=None, u_lb=None, u_ub=None, fz_lb=None, fz_ub=None, w_pos=None,
                 w_rot=None):
        self.mu, self.u_lb, self.u_ub, self.fz_lb, self.fz_ub = mu, u_lb, u_ub, fz_lb, fz_ub
        self.w_pos, self.w_rot = w_pos, w_rot
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is None:
                continue
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise TypeError(f"EnvParams.{name}: expected torch.Tensor or numpy array")
            if a.dtype not in (np.float64, torch.float64):
                raise ValueError(f"EnvParams.{name}: expected float64, got {a.dtype}")

    def shapes(self, nenv: int, dims: dict) -> dict:
        return dict(mu=(nenv,), u_lb=(nenv, dims["nu"]), u_ub=(nenv, dims["nu"]), fz_lb=(nenv,),
                    fz_ub=(nenv,), w_pos=(nenv, dims["ns"]), w_rot=(nenv, dims["ns"]))

    def to_device(self, nenv: int, dims: dict, device) -> tuple:
        """(osc_env_params struct, the device tensors it points to -- keep them alive until the
        launch is enqueued).  Raises ValueError on a wrong shape, before anything is copied."""
        want = self.shapes(nenv, dims)
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is not None and tuple(a.shape) != want[name]:
                raise ValueError(f"EnvParams.{name}: expected shape {want[name]}, got "
                                 f"{tuple(a.shape)}")
        c, keep = _lib.OscEnvParams(), []
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


class EnvGrads:
    """Gradients of a loss with respect to the per-env parameters (osc_env_grads,
    include/osc_backward_env.h): the mirror of EnvParams for outputs.  Each field is None (= not
    computed) or a contiguous float64 torch tensor on the solver's device, shaped as EnvParams';
    OSCBatchSolver.backward_env_into fills them.  Shape, dtype, device and layout are checked on
    the host when a solver takes the block (ValueError before any launch)."""
    FIELDS = EnvParams.FIELDS

    def __init__(self, mu=None, u_lb=None, u_ub=None, fz_lb=None, fz_ub=None, w_pos=None,
                 w_rot=None):
        self.mu, self.u_lb, self.u_ub, self.fz_lb, self.fz_ub = mu, u_lb, u_ub, fz_lb, fz_ub
        self.w_pos, self.w_rot = w_pos, w_rot
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is not None and not isinstance(a, torch.Tensor):
                raise TypeError(f"EnvGrads.{name}: expected torch.Tensor")

    @classmethod
    def empty(cls, nenv: int, dims: dict, device, fields=None) -> "EnvGrads":
        """Uninitialised tensors for `fields` (default: all seven)."""
        sh = EnvParams().shapes(nenv, dims)
        return cls(**{k: torch.empty(sh[k], dtype=torch.float64, device=device)
                      for k in (cls.FIELDS if fields is None else fields)})

    def to_struct(self, nenv: int, dims: dict, device) -> "_lib.OscEnvGrads":
        want = EnvParams().shapes(nenv, dims)
        c = _lib.OscEnvGrads()
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is None:
                continue
            if a.dtype != torch.float64:
                raise ValueError(f"EnvGrads.{name}: expected float64, got {a.dtype}")
            if tuple(a.shape) != want[name]:
                raise ValueError(f"EnvGrads.{name}: expected shape {want[name]}, got "
                                 f"{tuple(a.shape)}")
            if a.device != torch.device(device) or not a.is_contiguous():
                raise ValueError(f"EnvGrads.{name}: expected a contiguous tensor on {device}")
            setattr(c, name, a.data_ptr())
        return c


class OSCBatchSolver:
    def __init__(self, robot: str, yaml_path: str | None = None, eps_mu: float | None = None,
                 max_iter: int | None = None, device: torch.device | int | None = None,
                 tuning: dict | None = None, desc_overrides: dict | None = None):
        """tuning: fields of osc_model_tuning (include/osc_batch.h) to change from the model's
        defaults, e.g. {"small_batch_max": 0} (solver policy only, never the QP).
        desc_overrides: fields of osc_model_desc to change after the YAML is read -- these DO
        change the QP -- e.g. {"mu": 0.35, "u_lb": [-3.0] * 12, "z_ub": [1e30, 1e30, 30.0]}; an
        array field takes a sequence that replaces its leading entries."""
        if not torch.cuda.is_available():
            raise RuntimeError("OSCBatchSolver needs a HIP device (no CPU fallback exists)")
        self.robot = robot
        self.dims = dims(robot)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        desc = _lib.desc_from_yaml(robot, yaml_path or config_path(robot))
        if eps_mu is not None:
            desc.eps_mu = float(eps_mu)
        if max_iter is not None:
            desc.max_iter = int(max_iter)
        for k, v in (desc_overrides or {}).items():
            if k not in dict(_lib.OscModelDesc._fields_):
                raise KeyError(f"osc_model_desc has no field {k!r}")
            field = getattr(desc, k)
            if isinstance(field, ctypes.Array):
                v = list(v)
                if len(v) > len(field):
                    raise ValueError(f"{k}: at most {len(field)} values, got {len(v)}")
                field[:len(v)] = v
            else:
                setattr(desc, k, v)
        self.desc = desc
        self.wheels = desc.wheel_rows != 0
        tune = _lib.OscModelTuning()
        rc = _lib.lib().osc_model_tuning_defaults(ctypes.byref(desc), ctypes.byref(tune))
        if rc != 0:
            raise _lib.OSCError("osc_model_tuning_defaults", rc)
        for k, v in (tuning or {}).items():
            if k not in dict(_lib.OscModelTuning._fields_):
                raise KeyError(f"osc_model_tuning has no field {k!r}")
            setattr(tune, k, v)
        self.tuning = tune
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = _lib.lib().osc_model_create_tuned(ctypes.byref(desc), ctypes.byref(tune),
                                                   ctypes.byref(h))
        if rc != 0:
            raise _lib.OSCError("osc_model_create", rc)
        self._h = h
        rows = ctypes.c_int32()
        _lib.lib().osc_dual_rows(self._h, ctypes.byref(rows))
        self.dual_rows = rows.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().osc_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _as_dev(self, a, shape, name):
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{name}: expected torch.Tensor or numpy array")
        a = a.to(device=self.device, dtype=torch.float64).contiguous()
        if tuple(a.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(a.shape)}")
        return a

    def alloc_outputs(self, nenv: int, want_x: bool = False, want_y: bool = False):
        d = self.dims
        opts = dict(device=self.device)
        tau = torch.empty((nenv, d["nu"]), dtype=torch.float64, **opts)
        x = torch.empty((nenv, d["n"]), dtype=torch.float64, **opts) if (want_x or want_y) else None
        y = torch.empty((nenv, self.dual_rows), dtype=torch.float64, **opts) if want_y else None
        status = torch.empty((nenv,), dtype=torch.int32, **opts)
        iters = torch.empty((nenv,), dtype=torch.int32, **opts)
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_workspace_bytes(self._h, nenv, ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_workspace_bytes", rc)
        ws = torch.empty((max(nb.value // 8, 2),), dtype=torch.float64, **opts)
        return SolveResult(tau, x, status, iters, ws, y)

    def _env_block(self, env_params, nenv, wheel_dir=None):
        """(byref(osc_env_params), byref(osc_solve_extras) factory, tensors to keep alive) of an
        _env call; host-side shape / dtype errors raise here, before any launch."""
        if not isinstance(env_params, EnvParams):
            raise TypeError("env_params: expected an EnvParams")
        if wheel_dir is not None:
            raise ValueError("env_params: models with wheel rows are not supported")
        c, keep = env_params.to_device(nenv, self.dims, self.device)
        return c, keep

    def solve_into(self, out: SolveResult, M, C, J, b, T, mask, stream=None,
                   wheel_dir=None, env_params=None) -> SolveResult:
        """Launch only (no allocation, no host sync): the benchmarked call.  osc_batch_solve, or
        osc_batch_solve_ex when the model has wheel rows or duals are wanted (out.y); with
        env_params (an EnvParams) osc_batch_solve_env."""
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        wsb = ctypes.c_size_t(0 if out.workspace is None else out.workspace.numel() * 8)
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv, wheel_dir)
            ex = _lib.OscSolveExtras(None, out.y.data_ptr() if out.y is not None else None)
            rc = _lib.lib().osc_batch_solve_env(
                self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T), ptr(mask), ctypes.byref(c),
                ctypes.byref(ex), ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters),
                ptr(out.workspace), wsb, ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve_env", rc)
            return out
        if wheel_dir is None and out.y is None:
            rc = _lib.lib().osc_batch_solve(self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T),
                                            ptr(mask), ptr(out.tau), ptr(out.x), ptr(out.status),
                                            ptr(out.iters), ptr(out.workspace), wsb,
                                            ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve", rc)
            return out
        ex = _lib.OscSolveExtras(wheel_dir.data_ptr() if wheel_dir is not None else None,
                                 out.y.data_ptr() if out.y is not None else None)
        rc = _lib.lib().osc_batch_solve_ex(self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T),
                                           ptr(mask), ctypes.byref(ex), ptr(out.tau), ptr(out.x),
                                           ptr(out.status), ptr(out.iters), ptr(out.workspace), wsb,
                                           ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_ex", rc)
        return out

    def assemble_into(self, out: SolveResult, M, C, J, b, T, mask, stream=None,
                      wheel_dir=None, env_params=None) -> SolveResult:
        """First half of solve_into: every env's reduced QP into out.workspace (env_params: its
        task weights act here, osc_batch_assemble_env)."""
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        wsb = ctypes.c_size_t(out.workspace.numel() * 8)
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv, wheel_dir)
            rc = _lib.lib().osc_batch_assemble_env(
                self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T), ptr(mask), ctypes.byref(c),
                None, ptr(out.workspace), wsb, ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_assemble_env", rc)
            return out
        if wheel_dir is None:
            rc = _lib.lib().osc_batch_assemble(self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b),
                                               ptr(T), ptr(mask), ptr(out.workspace), wsb,
                                               ctypes.c_void_p(s))
        else:
            rc = _lib.lib().osc_batch_assemble_ex(self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b),
                                                  ptr(T), ptr(mask), ptr(wheel_dir),
                                                  ptr(out.workspace), wsb, ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_assemble", rc)
        return out

    def solve_assembled_into(self, out: SolveResult, mask, stream=None,
                             env_params=None) -> SolveResult:
        """Second half of solve_into: interior-point solve of the assembled workspace
        (env_params: its mu and bounds act here, osc_batch_solve_assembled_env)."""
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv)
            rc = _lib.lib().osc_batch_solve_assembled_env(
                self._h, nenv, ptr(mask), ctypes.byref(c), None, ptr(out.tau), ptr(out.x),
                ptr(out.status), ptr(out.iters), ptr(out.workspace),
                ctypes.c_size_t(out.workspace.numel() * 8), ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve_assembled_env", rc)
            return out
        rc = _lib.lib().osc_batch_solve_assembled(self._h, nenv, ptr(mask), ptr(out.tau),
                                                  ptr(out.x), ptr(out.status), ptr(out.iters),
                                                  ptr(out.workspace),
                                                  ctypes.c_size_t(out.workspace.numel() * 8),
                                                  ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_assembled", rc)
        return out

    def backward_into(self, out: SolveResult, J, mask, grad_x, grad_T, grad_b,
                      stream=None) -> None:
        """Launch only: osc_batch_solve_backward (include/osc_backward.h).  dL/dT into grad_T
        (nenv, ns, 6) and dL/db into grad_b (nenv, 6 ns), either None, from grad_x = dL/dx
        (nenv, nv + nu + 3 nc) over the whole design vector.  `out` is the SolveResult of the
        forward solve_into with x and y on the same J and mask; its workspace must not have been
        reused since.  An env whose status is not 0 gets zero gradients."""
        if out.y is None or out.workspace is None:
            raise ValueError("backward_into needs the forward solve's duals and workspace "
                             "(alloc_outputs(want_x=True, want_y=True))")
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_solve_backward(
            self._h, nenv, ptr(J), ptr(mask), ptr(out.y), ptr(out.status), ptr(grad_x),
            ptr(grad_T), ptr(grad_b), ptr(out.workspace),
            ctypes.c_size_t(out.workspace.numel() * 8), ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_backward", rc)

    def backward_data_into(self, out: SolveResult, M, J, b, T, mask, grad_x, grad_M=None,
                           grad_C=None, grad_J=None, grad_wrow=None, grad_T=None, grad_b=None,
                           stream=None) -> None:
        """Launch only: osc_batch_solve_backward_data (include/osc_backward.h).  From grad_x =
        dL/dx (nenv, nv + nu + 3 nc): dL/dM into grad_M (nenv, nv, nv), dL/dC into grad_C
        (nenv, nv), dL/dJ into grad_J (nenv, 6 ns, nv), the per-row weight gradient into grad_wrow
        (nenv, 6 ns; a site's w_pos / w_rot gradient is the sum of its three rows), dL/dT into
        grad_T (nenv, ns, 6) and dL/db into grad_b (nenv, 6 ns) -- each None or a tensor; a None
        is not computed.  `out` is the SolveResult of the forward solve_into with x and y on the
        same M, J, b, T and mask; its workspace must not have been reused since.  An env whose
        status is not 0 gets zeros."""
        if out.x is None or out.y is None or out.workspace is None:
            raise ValueError("backward_data_into needs the forward solve's design vector, duals "
                             "and workspace (alloc_outputs(want_x=True, want_y=True))")
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_solve_backward_data(
            self._h, nenv, ptr(M), ptr(J), ptr(b), ptr(T), ptr(mask), ptr(out.x), ptr(out.y),
            ptr(out.status), ptr(grad_x), ptr(grad_M), ptr(grad_C), ptr(grad_J), ptr(grad_wrow),
            ptr(grad_T), ptr(grad_b), ptr(out.workspace),
            ctypes.c_size_t(out.workspace.numel() * 8), ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_backward_data", rc)

    def backward_env_into(self, out: SolveResult, M, J, b, T, mask, grad_x, env_params=None,
                          grad_M=None, grad_C=None, grad_J=None, grad_wrow=None, grad_T=None,
                          grad_b=None, env_grads=None, stream=None) -> None:
        """Launch only: osc_batch_solve_backward_env (include/osc_backward_env.h).  As
        backward_data_into after a forward solve_into / solve_warm_into with env_params (the same
        EnvParams block; None after a forward call without one), and the gradients of the per-env
        parameters into env_grads (an EnvGrads; each field None or a tensor).  A None output is
        not computed; with only mu / bound gradients asked for, the solve with M and the pass over
        J are skipped.  An env whose status is not 0 gets zeros."""
        if out.x is None or out.y is None or out.workspace is None:
            raise ValueError("backward_env_into needs the forward solve's design vector, duals "
                             "and workspace (alloc_outputs(want_x=True, want_y=True))")
        nenv = out.tau.shape[0]
        keep, cp, cg = None, None, None
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv)
            cp = ctypes.byref(c)
        if env_grads is not None:
            if not isinstance(env_grads, EnvGrads):
                raise TypeError("env_grads: expected an EnvGrads")
            g = env_grads.to_struct(nenv, self.dims, self.device)
            cg = ctypes.byref(g)
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        rc = _lib.lib().osc_batch_solve_backward_env(
            self._h, nenv, ptr(M), ptr(J), ptr(b), ptr(T), ptr(mask), cp, ptr(out.x), ptr(out.y),
            ptr(out.status), ptr(grad_x), ptr(grad_M), ptr(grad_C), ptr(grad_J), ptr(grad_wrow),
            ptr(grad_T), ptr(grad_b), cg, ptr(out.workspace),
            ctypes.c_size_t(out.workspace.numel() * 8), ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_backward_env", rc)

    def alloc_warm_state(self, nenv: int) -> torch.Tensor:
        """Zero-filled warm state (osc_warm_state_bytes): every env starts cold on its first tick."""
        nb = ctypes.c_size_t()
        rc = _lib.lib().osc_warm_state_bytes(self._h, nenv, ctypes.byref(nb))
        if rc != 0:
            raise _lib.OSCError("osc_warm_state_bytes", rc)
        return torch.zeros((max(nb.value // 8, 2),), dtype=torch.float64, device=self.device)

    def solve_warm_into(self, out: SolveResult, warm: torch.Tensor, M, C, J, b, T, mask,
                        stream=None, wheel_dir=None, env_params=None) -> SolveResult:
        """osc_batch_solve_warm: as solve_into, starting from (and updating) `warm`, the previous
        tick's solution (the reference's SetWarmStart, operational_space_controller.h:519-526);
        osc_batch_solve_warm_ex with wheel rows or duals (out.y); with env_params
        osc_batch_solve_warm_env (the values may change from tick to tick; an env whose set of
        finite bounds changes needs its valid flag cleared, include/osc_env_params.h)."""
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv, wheel_dir)
            ex = _lib.OscSolveExtras(None, out.y.data_ptr() if out.y is not None else None)
            rc = _lib.lib().osc_batch_solve_warm_env(
                self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T), ptr(mask), ctypes.byref(c),
                ctypes.byref(ex), ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters),
                ptr(warm), ctypes.c_size_t(warm.numel() * 8), ptr(out.workspace),
                ctypes.c_size_t(0 if out.workspace is None else out.workspace.numel() * 8),
                ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve_warm_env", rc)
            return out
        if wheel_dir is not None or out.y is not None:
            ex = _lib.OscSolveExtras(wheel_dir.data_ptr() if wheel_dir is not None else None,
                                     out.y.data_ptr() if out.y is not None else None)
            rc = _lib.lib().osc_batch_solve_warm_ex(
                self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T), ptr(mask),
                ctypes.byref(ex), ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters),
                ptr(warm), ctypes.c_size_t(warm.numel() * 8), ptr(out.workspace),
                ctypes.c_size_t(0 if out.workspace is None else out.workspace.numel() * 8),
                ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve_warm_ex", rc)
            return out
        rc = _lib.lib().osc_batch_solve_warm(self._h, nenv, ptr(M), ptr(C), ptr(J), ptr(b), ptr(T),
                                             ptr(mask), ptr(out.tau), ptr(out.x), ptr(out.status),
                                             ptr(out.iters), ptr(warm),
                                             ctypes.c_size_t(0 if warm is None else warm.numel() * 8),
                                             ptr(out.workspace),
                                             ctypes.c_size_t(0 if out.workspace is None else
                                                             out.workspace.numel() * 8),
                                             ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_warm", rc)
        return out

    def solve_assembled_warm_into(self, out: SolveResult, warm: torch.Tensor, mask,
                                  stream=None, env_params=None) -> SolveResult:
        nenv = out.tau.shape[0]
        s = (torch.cuda.current_stream(self.device) if stream is None else stream).cuda_stream
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if env_params is not None:
            c, keep = self._env_block(env_params, nenv)
            rc = _lib.lib().osc_batch_solve_assembled_warm_env(
                self._h, nenv, ptr(mask), ctypes.byref(c), None, ptr(out.tau), ptr(out.x),
                ptr(out.status), ptr(out.iters), ptr(warm), ctypes.c_size_t(warm.numel() * 8),
                ptr(out.workspace), ctypes.c_size_t(out.workspace.numel() * 8),
                ctypes.c_void_p(s))
            if rc != 0:
                raise _lib.OSCError("osc_batch_solve_assembled_warm_env", rc)
            return out
        rc = _lib.lib().osc_batch_solve_assembled_warm(
            self._h, nenv, ptr(mask), ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters),
            ptr(warm), ctypes.c_size_t(0 if warm is None else warm.numel() * 8),
            ptr(out.workspace), ctypes.c_size_t(out.workspace.numel() * 8),
            ctypes.c_void_p(s))
        if rc != 0:
            raise _lib.OSCError("osc_batch_solve_assembled_warm", rc)
        return out

    def prepare(self, M, C, J, b, T, mask):
        d = self.dims
        nenv = int(M.shape[0])
        return (self._as_dev(M, (nenv, d["nv"], d["nv"]), "M"),
                self._as_dev(C, (nenv, d["nv"]), "C"),
                self._as_dev(J, (nenv, d["s"], d["nv"]), "J"),
                self._as_dev(b, (nenv, d["s"]), "b"),
                self._as_dev(T, (nenv, d["ns"], 6), "T"),
                self._as_dev(mask, (nenv, d["nc"]), "mask"))

    def solve(self, M, C, J, b, T, mask, want_x: bool = False, want_y: bool = False,
              wheel_dir=None, env_params=None) -> SolveResult:
        args = self.prepare(M, C, J, b, T, mask)
        nenv = int(args[0].shape[0])
        if env_params is not None:      # (shape errors: before anything is allocated or launched)
            self._env_block(env_params, nenv, wheel_dir)
        if wheel_dir is not None:
            wheel_dir = self._as_dev(wheel_dir, (nenv, self.dims["nc"], 6), "wheel_dir")
        out = self.alloc_outputs(nenv, want_x, want_y)
        with torch.cuda.device(self.device):
            return self.solve_into(out, *args, wheel_dir=wheel_dir, env_params=env_params)


def solve_multi_into(jobs, stream=None, env_params=None) -> None:
    """osc_batch_solve_multi: several models' batches in one call on one stream (BASELINE
    configs[4]: Go2 + WaLTER Sr per GPU).  `jobs` = [(solver, SolveResult, (M, C, J, b, T,
    mask)[, wheel_dir]), ...] with device tensors from solver.prepare / solver.alloc_outputs
    (wheel_dir: the wheel-row models' directions, [nenv, nc, 6])."""
    if env_params is not None:
        raise NotImplementedError("solve_multi_into: per-env parameters are not supported by the "
                                  "multi-model call (solve each model with solve_into)")
    arr = (_lib.OscBatchJob * len(jobs))()
    ptr = lambda t: t.data_ptr() if t is not None else None
    dev = None
    for j, job in zip(arr, jobs):
        solver, out, inputs = job[:3]
        j.wheel_dir = ptr(job[3]) if len(job) > 3 else None
        M, C, J, b, T, mask = inputs
        j.model = solver._h.value
        j.nenv = out.tau.shape[0]
        j.M, j.C, j.J, j.b, j.T, j.contact_mask = (ptr(t) for t in (M, C, J, b, T, mask))
        j.tau, j.x, j.status, j.iters = ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters)
        j.workspace = ptr(out.workspace)
        j.workspace_bytes = out.workspace.numel() * 8
        dev = solver.device
    s = (torch.cuda.current_stream(dev) if stream is None else stream).cuda_stream
    rc = _lib.lib().osc_batch_solve_multi(arr, len(jobs), ctypes.c_void_p(s))
    if rc != 0:
        raise _lib.OSCError("osc_batch_solve_multi", rc)


@dataclasses.dataclass
class TickJob:
    """One model's tick inside tick_multi_into (osc_tick_job, include/osc_mixed.h).
    inputs: (M, C, J, b, T, mask) device tensors, or with `kin` (a KinematicsBatch of the same
    robot) (qpos, qvel, T, mask).  warm: the job's warm-state tensor (solver.alloc_warm_state),
    None = cold.  workspace: with `kin` a tensor of kin.workspace_bytes(solver, nenv); without,
    out.workspace is used."""
    solver: OSCBatchSolver
    out: SolveResult
    inputs: tuple
    kin: object | None = None
    warm: torch.Tensor | None = None
    workspace: torch.Tensor | None = None


def tick_jobs_array(jobs):
    """The osc_tick_job array of a list of TickJob (device pointers only: keep `jobs` alive)."""
    arr = (_lib.OscTickJob * max(len(jobs), 1))()
    ptr = lambda t: t.data_ptr() if t is not None else None
    for j, job in zip(arr, jobs):
        out = job.out
        j.model = job.solver._h.value
        j.nenv = out.tau.shape[0]
        if job.kin is not None:
            j.kin = job.kin._h.value
            qpos, qvel, T, mask = job.inputs
            j.qpos, j.qvel = ptr(qpos), ptr(qvel)
        else:
            M, C, J, b, T, mask = job.inputs
            j.M, j.C, j.J, j.b = ptr(M), ptr(C), ptr(J), ptr(b)
        j.T, j.contact_mask = ptr(T), ptr(mask)
        j.tau, j.x, j.status, j.iters = ptr(out.tau), ptr(out.x), ptr(out.status), ptr(out.iters)
        if job.warm is not None:
            j.warm_state, j.warm_state_bytes = ptr(job.warm), job.warm.numel() * 8
        ws = job.workspace if job.workspace is not None else out.workspace
        if ws is not None:
            j.workspace, j.workspace_bytes = ptr(ws), ws.numel() * ws.element_size()
    return arr


def tick_multi_into(jobs, stream=None, env_params=None) -> None:
    """osc_batch_tick_multi: several models' ticks in one call on one stream -- the mixed-robot
    tick with warm starts and joint-state inputs per job (BASELINE configs[4]).  `jobs` is a list
    of TickJob; each job's results are bitwise those of its single-model call."""
    if env_params is not None:
        raise NotImplementedError("tick_multi_into: per-env parameters are not supported by the "
                                  "mixed-robot tick (solve each model with solve_into)")
    arr = tick_jobs_array(jobs)
    dev = jobs[-1].solver.device if jobs else None
    s = (torch.cuda.current_stream(dev) if stream is None else stream).cuda_stream
    rc = _lib.lib().osc_batch_tick_multi(arr, len(jobs), ctypes.c_void_p(s))
    if rc != 0:
        raise _lib.OSCError("osc_batch_tick_multi", rc)
