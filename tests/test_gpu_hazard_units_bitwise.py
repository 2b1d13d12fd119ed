"""The same call twice gives the same bits, for the kernels whose units the hazard scan
(tests/test_asm_hazards.py) reached last: the forward dynamics, its vector-Jacobian product and the
three backward kernels of the solve.  They share the inline-asm LDL' and lane-mask selects
(csrc/osc_ipm_ldl.hpp, csrc/osc_device.hpp), whose data hazards the compiler does not pad; a pair
left short shows as a value that differs on some waves of some launches, which is what a repeat
can catch and a comparison at a tolerance cannot.  67 envs (16 full wavefronts and a partial one),
Go2 and WaLTER Sr, every output of each call compared bit for bit and required finite."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import env_params_cases as ec
import test_gpu_backward_env as tbe
import test_gpu_plant as tp
import test_gpu_plant_backward as tpb
from osc_amd.synth import generate

pytestmark = pytest.mark.gpu

ROBOTS = [tp.GO2, tp.WALTER]
N = 67
SEED = 20260


def bitwise(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                          np.ascontiguousarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def solved(robot, block):
    """((inputs, forward solve with x, y and the workspace, per-env block or None), gx), shared by
    the backward tests and left unchanged; block: solve with drawn per-env parameters."""
    rng = np.random.default_rng(SEED)
    d = generate(robot, N, SEED, "tumbling", "bernoulli")
    fwd = tbe.forward(robot, p=ec.draw_params(robot, rng, N) if block else None, d=d)
    assert (fwd[1].status.cpu().numpy() == 0).all()
    gx = rng.standard_normal(tuple(fwd[1].x.shape))
    return fwd, gx


def same_twice(call):
    a, b = call(), call()
    assert a.keys() == b.keys() and a
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert bitwise(a[k], b[k]), k
    assert any(np.abs(v).max() > 0.0 for v in a.values())


@pytest.mark.parametrize("robot", ROBOTS)
def test_forward_dynamics_twice(gpu, robot):
    same_twice(lambda: {"qacc": tp.fd_run(robot, slice(0, N))})


@pytest.mark.parametrize("robot", ROBOTS)
def test_forward_dynamics_backward_twice(gpu, robot):
    same_twice(lambda: tpb.run(robot, slice(0, N)))


@pytest.mark.parametrize("robot", ROBOTS)
def test_backward_twice(gpu, robot):
    fwd, gx = solved(robot, False)
    s = tbe.solver(robot)
    (M, C, J, b, T, mask), out, _ = fwd

    def call():
        g = torch.from_numpy(gx).to(s.device)
        gT = torch.full((N, s.dims["ns"], 6), float("nan"), dtype=torch.float64, device=s.device)
        gb = torch.full((N, s.dims["s"]), float("nan"), dtype=torch.float64, device=s.device)
        s.backward_into(out, J, mask, g, gT, gb)
        torch.cuda.synchronize()
        return {"T": gT.cpu().numpy(), "b": gb.cpu().numpy()}
    same_twice(call)


@pytest.mark.parametrize("robot", ROBOTS)
def test_backward_data_twice(gpu, robot):
    fwd, gx = solved(robot, False)
    same_twice(lambda: tbe.backward_data(robot, fwd, gx))


@pytest.mark.parametrize("robot", ROBOTS)
def test_backward_env_twice(gpu, robot):
    fwd, gx = solved(robot, True)
    same_twice(lambda: tbe.backward(robot, fwd, gx))
