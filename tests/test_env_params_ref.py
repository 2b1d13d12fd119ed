"""CPU tests of the per-env parameters (include/osc_env_params.h, osc_amd.solver.EnvParams): the
precondition of tests/test_gpu_env_params.py -- every env of the drawn batch certifies at the
oracle and every row kind is active often enough for the GPU parity test to mean something -- and
the library's boundary: the header's declarations are the exported symbols, the ABI version is
unchanged, argument errors come back without a device, EnvParams refuses wrong shapes and dtypes
before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import env_params_cases as ec
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_env_params.h")


@pytest.mark.parametrize("robot", ec.ROBOTS)
def test_precondition_every_env_certifies_and_every_row_kind_is_active(robot):
    """env_params_cases.oracle raises unless every env certifies at 1e-8.  Active rows at the
    optimum, summed over the 61 envs (u_lo / u_hi / pyramid / fz_lo / fz_hi): Go2 346 / 338 / 253 /
    47 / 110, WaLTER 237 / 204 / 563 / 101 / 197; the condition is at least 20 of each."""
    x, y = ec.oracle(robot)
    assert x.shape[0] == ec.NENV and np.isfinite(x).all() and np.isfinite(y).all()
    counts = ec.active_counts(robot, ec.inputs(robot), ec.params(robot), x)
    print(f"\n{robot}: active rows {counts}")
    assert all(v >= 20 for v in counts.values()), counts


def test_draw_is_what_the_docstring_says():
    p = ec.params("unitree_go2")
    assert ((p["mu"] >= 0.2) & (p["mu"] <= 1.2)).all()
    assert set(np.unique(p["fz_lb"])) == {0.0, 5.0}
    assert ((p["fz_ub"] >= 15.0) & (p["fz_ub"] <= 60.0)).all()
    inf = 1e20
    absent_lo = np.abs(p["u_lb"]) >= inf
    assert absent_lo.any(axis=1).tolist() == [e % 7 == 3 for e in range(ec.NENV)]
    assert ((p["u_lb"] < p["u_ub"])).all()
    assert len(np.unique(p["mu"])) == ec.NENV           # per env, not per batch


def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", open(HEADER).read(),
                              re.M))
    assert declared == set(_lib.ENV_PARAMS_SYMBOLS) and len(declared) == 5
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS))
    assert L.osc_abi_version() == 4          # additive: ABI 4 callers are untouched


def test_struct_has_the_header_fields_in_order():
    body = re.search(r"typedef struct \{(.*?)\} osc_env_params;", open(HEADER).read(), re.S).group(1)
    fields = re.findall(r"const double\*\s+(\w+);", body)
    assert fields == [n for n, _ in _lib.OscEnvParams._fields_] == list(ec.FIELDS)
    assert ctypes.sizeof(_lib.OscEnvParams) == 7 * ctypes.sizeof(ctypes.c_void_p)


def test_bad_arguments_without_a_device():
    L = _lib.lib()
    ep = _lib.OscEnvParams()
    none6, none4 = [None] * 6, [None] * 4
    # a NULL model is refused by every entry, with and without a parameter block
    for blk in (None, ctypes.byref(ep)):
        assert L.osc_batch_solve_env(None, 1, *none6, blk, None, *none4, None, 0, None) == 1
        assert L.osc_batch_solve_warm_env(None, 1, *none6, blk, None, *none4, None, 0, None, 0,
                                          None) == 1
        assert L.osc_batch_assemble_env(None, 1, *none6, blk, None, None, 0, None) == 1
        assert L.osc_batch_solve_assembled_env(None, 1, None, blk, None, *none4, None, 0, None) == 1
        assert L.osc_batch_solve_assembled_warm_env(None, 1, None, blk, None, *none4, None, 0, None,
                                                    0, None) == 1


def test_env_params_shape_and_dtype_errors_raise_on_the_host():
    """Before any device call: the constructor checks types and dtypes, to_device checks the shapes
    first and touches the device only after all of them passed."""
    from osc_amd.robots import dims
    from osc_amd.solver import EnvParams
    d = dims("unitree_go2")
    n = 7
    with pytest.raises(ValueError):
        EnvParams(mu=np.ones(n, dtype=np.float32))
    with pytest.raises(ValueError):
        EnvParams(u_lb=np.ones((n, d["nu"]), dtype=np.int64))
    with pytest.raises(TypeError):
        EnvParams(mu=[0.5] * n)
    bad_shapes = dict(mu=(n + 1,), u_lb=(n, d["nu"] + 1), u_ub=(d["nu"], n), fz_lb=(n, 1),
                      fz_ub=(n - 1,), w_pos=(n, d["ns"] + 1), w_rot=(n,))
    for name, shape in bad_shapes.items():
        with pytest.raises(ValueError, match=name):
            EnvParams(**{name: np.ones(shape)}).to_device(n, d, "cuda:0")
    good = EnvParams(**{k: np.ones(s) for k, s in EnvParams().shapes(n, d).items()})
    assert good.shapes(n, d)["w_pos"] == (n, d["ns"])
    assert EnvParams().to_device(n, d, "cuda:0")[1] == []      # all None: nothing to copy
