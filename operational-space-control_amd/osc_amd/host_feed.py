"""Host-fed batched control tick (include/osc_host_feed.h).

Every tick's inputs start in pinned host memory -- where the reference's control loop finds the
State and task targets the simulation thread wrote (unitree_go2/operational_space_controller.h:
546-573) -- cross PCIe in one copy, are solved on the GPU, and the torques come back.  Tick k's
copy overlaps tick k-1's solve (depth 2).  Two input forms: the post-kinematics QP inputs
(M, C, J, b, T, mask) or joint states (qpos, qvel, T, mask) through the GPU kinematics.

    feed = HostFeed(solver, nenv, form="qp", depth=2, warm=False)
    feed.inputs(k)["M"][:] = ...      # numpy views of the pinned slot of tick k
    feed.submit(k)
    tau, status, iters = feed.wait(k)  # numpy views of the pinned outputs (valid until k + depth)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


class HostFeed:
    def __init__(self, solver, nenv: int, form: str = "qp", depth: int = 2, warm: bool = False,
                 kin=None):
        """solver: an OSCBatchSolver (its model and device); kin: a KinematicsBatch for
        form="joint_states" (the same robot)."""
        import torch
        self.solver, self.nenv, self.form, self.depth = solver, nenv, form, depth
        d = solver.dims
        self.nu, self.nv, self.ns, self.nc = d["nu"], d["nv"], d["ns"], d["nc"]
        self.nq = kin.nq if kin is not None else None
        f = {"qp": _lib.FEED_QP, "joint_states": _lib.FEED_JOINT_STATES}[form]
        h = ctypes.c_void_p()
        with torch.cuda.device(solver.device):
            rc = _lib.lib().osc_host_feed_create(solver._h, kin._h if kin is not None else None,
                                                 nenv, f, _lib.FEED_WARM if warm else 0, depth,
                                                 ctypes.byref(h))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_create", rc)
        self._h = h
        self._kin = kin   # (kept alive: the feed holds its handle)
        self.next = 0
        self.in_bytes = 0
        self.out_bytes = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().osc_host_feed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _view(addr, shape, dtype=np.float64):
        n = int(np.prod(shape))
        ct = ctypes.c_double if dtype == np.float64 else ctypes.c_int32
        return np.ctypeslib.as_array((ct * n).from_address(addr)).reshape(shape)

    def inputs(self, tick: int) -> dict:
        """Numpy views of tick `tick`'s pinned input slot (blocks until the slot is free)."""
        s = _lib.OscFeedInputs()
        rc = _lib.lib().osc_host_feed_inputs(self._h, tick, ctypes.byref(s))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_inputs", rc)
        self.in_bytes = s.bytes
        n = self.nenv
        out = {"T": self._view(s.T, (n, self.ns, 6)),
               "mask": self._view(s.contact_mask, (n, self.nc))}
        if self.form == "qp":
            out.update(M=self._view(s.M, (n, self.nv, self.nv)), C=self._view(s.C, (n, self.nv)),
                       J=self._view(s.J, (n, 6 * self.ns, self.nv)),
                       b=self._view(s.b, (n, 6 * self.ns)))
        else:
            out.update(qpos=self._view(s.qpos, (n, self.nq)), qvel=self._view(s.qvel, (n, self.nv)))
        return out

    def submit(self, tick: int) -> None:
        rc = _lib.lib().osc_host_feed_submit(self._h, tick)
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_submit", rc)
        self.next = tick + 1

    def wait(self, tick: int):
        """(tau, status, iters) numpy views of tick `tick`'s pinned outputs."""
        o = _lib.OscFeedOutputs()
        rc = _lib.lib().osc_host_feed_wait(self._h, tick, ctypes.byref(o))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_wait", rc)
        self.out_bytes = o.bytes
        n = self.nenv
        return (self._view(o.tau, (n, self.nu)), self._view(o.status, (n,), np.int32),
                self._view(o.iters, (n,), np.int32))

    def timing(self, tick: int) -> dict:
        t = _lib.OscFeedTiming()
        rc = _lib.lib().osc_host_feed_timing(self._h, tick, ctypes.byref(t))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_timing", rc)
        return {"h2d_ms": t.h2d_ms, "solve_ms": t.solve_ms, "d2h_ms": t.d2h_ms,
                "kin_ms": t.kin_ms, "latency_ms": t.h2d_start_to_d2h_end_ms}


class _FeedHandle:
    """Owns an osc_host_feed and what it borrows (the parts' models and kin handles).  Every view
    MixedHostFeed hands out refers to it, so the pinned memory outlives the MixedHostFeed object
    for as long as any view is held."""

    def __init__(self, handle, keep):
        self.h, self.keep = handle, keep

    def close(self):
        if self.h is not None and self.h.value:
            _lib.lib().osc_host_feed_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _owned_view(owner, addr, shape, dtype=np.float64):
    """A numpy view of foreign memory at `addr` whose base chain keeps `owner` alive."""
    n = int(np.prod(shape))
    ct = ctypes.c_double if dtype == np.float64 else ctypes.c_int32
    buf = (ct * n).from_address(addr)
    buf._owner = owner   # the array refers to buf (buffer protocol), buf to the owner
    return np.ctypeslib.as_array(buf).reshape(shape)


class MixedHostFeed:
    """The two-model host feed (include/osc_mixed.h): one pinned block, one H2D and one D2H copy
    per tick for both parts, the solve osc_batch_tick_multi.

        feed = MixedHostFeed([(walter_solver, 4096), (go2_solver, 4096)], form="qp", depth=2,
                             warm=True)            # joint states: (solver, nenv, kin) per part
        feed.inputs(k, 0)["M"][:] = ...; feed.inputs(k, 1)["M"][:] = ...
        feed.submit(k)
        tau, status, iters = feed.wait(k, 1)

    The views returned by inputs() / wait() keep the native feed alive: they stay readable after
    the MixedHostFeed object itself is gone (close() destroys the feed at once; do not use views
    after calling it)."""

    def __init__(self, parts, form: str = "qp", depth: int = 2, warm: bool = False):
        import torch
        self.form, self.depth = form, depth
        self.parts = [tuple(p) + (None,) * (3 - len(p)) for p in parts]
        f = {"qp": _lib.FEED_QP, "joint_states": _lib.FEED_JOINT_STATES}[form]
        arr = (_lib.OscFeedPart * max(len(self.parts), 1))()
        for a, (solver, nenv, kin) in zip(arr, self.parts):
            a.model = solver._h.value
            a.kin = kin._h.value if kin is not None else None
            a.nenv = nenv
        h = ctypes.c_void_p()
        device = self.parts[0][0].device if self.parts else None
        with torch.cuda.device(device):
            rc = _lib.lib().osc_host_feed_create_multi(arr, len(self.parts), f,
                                                       _lib.FEED_WARM if warm else 0, depth,
                                                       ctypes.byref(h))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_create_multi", rc)
        self._owner = _FeedHandle(h, [p for part in self.parts for p in (part[0], part[2])])
        self.in_bytes = 0
        self.out_bytes = 0

    def close(self):
        self._owner.close()

    def _dims(self, part):
        if not 0 <= part < len(self.parts):
            raise _lib.OSCError("MixedHostFeed", 1)
        solver, nenv, kin = self.parts[part]
        d = solver.dims
        return nenv, d["nu"], d["nv"], d["ns"], d["nc"], (kin.nq if kin is not None else None)

    def inputs(self, tick: int, part: int) -> dict:
        """Numpy views of part `part`'s arrays in tick `tick`'s pinned input slot."""
        n, nu, nv, ns, nc, nq = self._dims(part)
        s = _lib.OscFeedInputs()
        rc = _lib.lib().osc_host_feed_inputs_part(self._owner.h, tick, part, ctypes.byref(s))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_inputs_part", rc)
        self.in_bytes = s.bytes
        v = lambda addr, shape: _owned_view(self._owner, addr, shape)
        out = {"T": v(s.T, (n, ns, 6)), "mask": v(s.contact_mask, (n, nc))}
        if self.form == "qp":
            out.update(M=v(s.M, (n, nv, nv)), C=v(s.C, (n, nv)), J=v(s.J, (n, 6 * ns, nv)),
                       b=v(s.b, (n, 6 * ns)))
        else:
            out.update(qpos=v(s.qpos, (n, nq)), qvel=v(s.qvel, (n, nv)))
        return out

    def submit(self, tick: int) -> None:
        rc = _lib.lib().osc_host_feed_submit(self._owner.h, tick)
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_submit", rc)

    def wait(self, tick: int, part: int):
        """(tau, status, iters) numpy views of part `part`'s pinned outputs of tick `tick`."""
        n, nu = self._dims(part)[:2]
        o = _lib.OscFeedOutputs()
        rc = _lib.lib().osc_host_feed_wait_part(self._owner.h, tick, part, ctypes.byref(o))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_wait_part", rc)
        self.out_bytes = o.bytes
        return (_owned_view(self._owner, o.tau, (n, nu)),
                _owned_view(self._owner, o.status, (n,), np.int32),
                _owned_view(self._owner, o.iters, (n,), np.int32))

    def timing(self, tick: int) -> dict:
        t = _lib.OscFeedTiming()
        rc = _lib.lib().osc_host_feed_timing(self._owner.h, tick, ctypes.byref(t))
        if rc != 0:
            raise _lib.OSCError("osc_host_feed_timing", rc)
        return {"h2d_ms": t.h2d_ms, "solve_ms": t.solve_ms, "d2h_ms": t.d2h_ms,
                "kin_ms": t.kin_ms, "latency_ms": t.h2d_start_to_d2h_end_ms}
