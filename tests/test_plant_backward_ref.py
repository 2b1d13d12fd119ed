"""CPU tests of the forward dynamics' backward reference (tests/plant_backward_ref.py) and of the
binding of include/osc_plant_backward.h: what tests/test_gpu_plant_backward.py measures the GPU
against is itself checked here, and the new entry's argument errors come back without a device.
   1. the closed-form vector-Jacobian product against central differences of
      plant_ref.forward_dynamics, every input;
   2. the numpy model of the kernel's LDL' on the cotangent and the bar it sets;
   3. the binding: the header's declarations, the ABI version, the refusals; osc_plant.h keeps its
      three declarations and its sentences."""
import ctypes
import os
import re

import numpy as np
import pytest

import plant_backward_ref as pbr
import plant_ref as pr
from osc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "osc_plant_backward.h")
FD_TOL = 1e-5            # the project's contract for a gradient against finite differences


# ---- 1. the closed form against finite differences --------------------------------------------------

def central(f, x, dx, h):
    """Richardson's central difference of the scalar f along dx: O(h^4)."""
    d = lambda s: (f(x + s * dx) - f(x - s * dx)) / (2 * s)
    return (4 * d(h / 2) - d(h)) / 3


@pytest.mark.parametrize("robot", [pr.GO2, pr.WALTER])
def test_closed_form_against_finite_differences(robot):
    """Envs 0..2 of bw_case: <grad_a, da> of the closed form against the Richardson central
    difference of g . forward_dynamics along a drawn direction da, for a in M (a symmetric
    direction, as M is), C, J (all rows: the closed form is zero off the contact rows), u, z and
    qfrc; relative disagreement <= 1e-5 (measured <= 5e-10: the function is linear in all but M)."""
    c, model = pbr.bw_case(robot), pr.load_model(robot)
    rng = np.random.default_rng(3)
    rows = pbr.contact_rows(model)
    worst = {}
    for e in range(3):
        x0 = dict(M=c["M"][e], C=c["C"][e], J=c["J"][e], u=c["u"][e], z=c["z"][e], qfrc=c["qfrc"][e])
        g = c["g"][e]
        qacc = pr.forward_dynamics(model, x0["M"], x0["C"], x0["J"], x0["u"], x0["z"], x0["qfrc"])
        grads = pbr.fd_vjp(model, x0["J"], x0["z"], qacc, np.linalg.solve(x0["M"], g))
        gJ = np.zeros_like(x0["J"])
        gJ[rows] = grads["Jc"]
        grads = dict(grads, J=gJ)
        for name in ("M", "C", "J", "u", "z", "qfrc"):
            dx = rng.standard_normal(x0[name].shape)
            if name == "M":    # symmetric, and scaled as M is (joint inertias are ~1e-2)
                sd = np.sqrt(np.diag(x0["M"]))
                dx = 0.5 * (dx + dx.T) * np.outer(sd, sd) / len(sd)

            def f(v, name=name):
                a = dict(x0, **{name: v})
                return float(g @ pr.forward_dynamics(model, a["M"], a["C"], a["J"], a["u"], a["z"],
                                                     a["qfrc"]))
            num = central(f, x0[name], dx, 1e-3)
            ana = float((grads[name] * dx).sum())
            rel = abs(num - ana) / max(abs(num), 1.0)
            worst[name] = max(worst.get(name, 0.0), rel)
            assert rel <= FD_TOL, (robot, e, name, num, ana)
    print(f"\n{robot}: closed form vs central differences, worst relative {worst}")


def test_closed_form_without_contact_forces():
    c, model = pbr.bw_case(pr.GO2), pr.load_model(pr.GO2)
    out = pbr.fd_vjp(model, None, None, c["qacc"][0], c["w_ref"][0])
    assert sorted(out) == ["C", "M", "qfrc", "u"]
    assert np.array_equal(out["u"], c["w_ref"][0][model.nv - model.nu:])


# ---- 2. the LDL' model ----------------------------------------------------------------------------------

@pytest.mark.parametrize("robot", [pr.GO2, pr.WALTER])
def test_ldl_model_of_w_sets_the_bar(robot):
    """plant_ref.ldl_model of w = M^-1 g on the GPU test's own inputs against plant_ref.refined: its
    worst error x 10 is the GPU test's bar, which must lie below FD_BAR_MAX for that test to mean
    anything.  |w|_inf >= 1 in every env, so the GPU test's metric is a relative one for the
    outputs that are w."""
    c = pbr.bw_case(robot)
    err = c["bw_model_err"]
    wmin = np.abs(c["w_ref"]).max(axis=1).min()
    print(f"\n{robot}: ldl_model of w worst {err.max():.2e}, min |w|_inf {wmin:.2f}, "
          f"bar {pbr.bw_bar(robot):.2e}")
    assert np.isfinite(c["w_ref"]).all() and err.max() > 0
    assert 10 * err.max() <= pr.FD_BAR_MAX
    assert wmin >= 1.0
    # the closed form on the model's w is within the same bar of the closed form on the refined w
    model = pr.load_model(robot)
    for e in range(len(err)):
        got = pbr.fd_vjp(model, c["J"][e], c["z"][e], c["qacc"][e], c["w_model"][e])
        for k in pbr.OUTPUTS:
            assert pbr.out_errors(got[k][None], c["grads"][k][e][None])[0] <= pbr.bw_bar(robot), \
                (e, k)


# ---- 3. the library's boundary ---------------------------------------------------------------------------

def test_header_declarations_are_the_exported_symbols():
    L = _lib.lib()
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.PLANT_BACKWARD_SYMBOLS) and len(declared) == 3
    for name in declared:
        assert hasattr(L, name), name
    assert not declared & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.MIXED_SYMBOLS) |
                           set(_lib.ROLLOUT_SYMBOLS) | set(_lib.BACKWARD_SYMBOLS) |
                           set(_lib.ENV_PARAMS_SYMBOLS) | set(_lib.BACKWARD_ENV_SYMBOLS) |
                           set(_lib.KIN_ENV_SYMBOLS) | set(_lib.KIN_BACKWARD_SYMBOLS) |
                           set(_lib.ROLLOUT_BACKWARD_SYMBOLS) | set(_lib.ROLLOUT_SCHEDULE_SYMBOLS) |
                           set(_lib.PLANT_SYMBOLS))
    assert L.osc_abi_version() == 4            # purely additive: no ABI bump
    assert len(L.osc_batch_forward_dynamics_backward.argtypes) == 18
    body = re.search(r"typedef struct \{([^}]*)\} osc_rollout_plant_backward;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [n for n, _ in _lib.OscRolloutPlantBackward._fields_]
    assert ctypes.sizeof(_lib.OscRolloutPlantBackward) == 56    # the unit's static_assert
    unit = open(os.path.join(REPO, "operational-space-control_amd", "csrc",
                             "osc_rollout_backward.hip")).read()
    assert re.search(r"sizeof\(osc_rollout_plant_backward\) == 56", unit)
    assert ctypes.sizeof(_lib.OscRolloutBackwardArgs) == 208    # the block it rides on is unchanged
    assert ctypes.sizeof(_lib.OscRolloutPlant) == 32
    from osc_amd.build import SOURCES
    assert "osc_forward_dynamics_backward.hip" in SOURCES


def test_osc_plant_h_keeps_its_declarations_and_sentences():
    text = open(os.path.join(REPO, "include", "osc_plant.h")).read()
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(osc_\w+)\s*\(", text, re.M))
    assert declared == set(_lib.PLANT_SYMBOLS) and len(declared) == 3
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    assert "gradients through the plant" in flat
    assert "there is still no ground." in flat
    assert "osc_plant_backward.h" in flat


def test_refusals_come_back_without_a_device():
    """The new entry refuses a NULL model, whatever else it is given, without touching a device."""
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = L.osc_batch_forward_dynamics_backward
    assert f(None, 4, p, p, p, 12, p, p, 18, p, p, p, p, 12, p, 12, p, None) == 1
    assert f(None, 0, None, None, None, 0, None, None, 0, None, None, None, None, 0, None, 0,
             None, None) == 1
    assert f(None, -1, p, p, p, 12, p, p, 18, p, None, None, None, 0, None, 0, None, None) == 1
    assert not any(buf)
    nb = ctypes.c_size_t(7)
    assert L.osc_rollout_plant_backward_workspace_bytes(None, None, 4, ctypes.byref(nb)) == 1
    assert L.osc_rollout_plant_backward_workspace_bytes(None, None, 4, None) == 1
    assert nb.value == 7
    ba, pl = _lib.OscRolloutBackwardArgs(), _lib.OscRolloutPlantBackward()
    f = L.osc_batch_rollout_plant_backward
    assert f(None, None, 4, ctypes.byref(ba), None, None, None, None, ctypes.byref(pl), None) == 1
    pl.grad_qfrc_applied = ctypes.addressof(buf)
    assert f(None, None, 4, ctypes.byref(ba), None, None, None, None, ctypes.byref(pl), None) == 1
    assert f(None, None, 4, None, None, None, None, None, None, None) == 1
    assert not any(buf)


# ---- 4. the chain of the whole plant rollout's backward ----------------------------------------------------

def test_chain_forward_equals_the_plant_rollout_reference():
    c = pbr.chain_case()
    import kin_env_ref as ker
    for e in (0, 3):
        kc = ker.env_model(c["tree"], mass_scale=c["ms"][e])
        kp = ker.env_model(c["tree"], **{k: c["plant_" + k][e] for k in
                                         ("mass_scale", "com_offset", "armature_scale")})
        ref = pr.rollout(kc, kp, c["model"], c["qpos"][e], c["qvel"][e], c["mask"][e], pbr.CHAIN_K,
                         pr.DT, T=c["T"][e], qfrc_seq=c["qfrc_seq"][:, e])
        for k in ("qpos", "qvel", "tau", "qacc"):
            got = c["out"][e][1][k]
            assert np.abs(got - ref[k]).max() <= 1e-9 * (1 + np.abs(ref[k]).max()), (e, k)


@pytest.mark.parametrize("e", range(pbr.CHAIN_NENV))
def test_chain_equals_finite_differences_of_the_plant_rollout(e):
    """plant_backward_ref.chain on chain_case (rollout_backward_ref.assert_clean ran at every env
    and tick: none left out) against Richardson central differences (4 D(h/2) - D(h)) / 3 of
    plant_ref.rollout's loss along one drawn direction in qvel0, qfrc_seq (h = 0.1) and the plant's
    mass_scale, com_offset and armature_scale (h = 1e-3; the armature direction constant per joint
    and zero where the scale is 0): |g.d - fd| <= 1e-5 max(|fd|, 1)."""
    import kin_env_ref as ker
    c = pbr.chain_case()
    tree, mdl = c["tree"], c["model"]
    g = c["out"][e][0]
    cot = {k: c["cot_" + k][:, e] for k in ("qpos", "qvel", "tau", "qacc")}
    kc = ker.env_model(tree, mass_scale=c["ms"][e])
    x0 = dict(qvel0=c["qvel"][e], qfrc_seq=c["qfrc_seq"][:, e],
              mass_scale=c["plant_mass_scale"][e], com_offset=c["plant_com_offset"][e],
              armature_scale=c["plant_armature_scale"][e])
    names = dict(qvel0="qvel0", qfrc_seq="plant.qfrc_applied", mass_scale="plant.kin.mass_scale",
                 com_offset="plant.kin.com_offset", armature_scale="plant.kin.armature_scale")

    def loss(x):
        kp = ker.env_model(tree, mass_scale=x["mass_scale"], com_offset=x["com_offset"],
                           armature_scale=x["armature_scale"])
        r = pr.rollout(kc, kp, mdl, c["qpos"][e], x["qvel0"], c["mask"][e], pbr.CHAIN_K, pr.DT,
                       T=c["T"][e], qfrc_seq=x["qfrc_seq"])
        return sum((cot[k] * r[k]).sum() for k in cot)

    rng = np.random.default_rng(200 + e)
    for name, h in (("qfrc_seq", 0.1), ("qvel0", 1e-3), ("mass_scale", 1e-3),
                    ("com_offset", 1e-3), ("armature_scale", 1e-3)):
        if name == "armature_scale":
            nd = ker.joint_dofs(tree)
            d = np.repeat(rng.standard_normal(len(nd)), nd) * (x0[name] != 0.0)
        else:
            d = rng.standard_normal(x0[name].shape)
        d = d / np.abs(d).max()
        D = lambda s: (loss(dict(x0, **{name: x0[name] + s * d})) -
                       loss(dict(x0, **{name: x0[name] - s * d}))) / (2 * s)
        fd = (4 * D(h / 2) - D(h)) / 3
        got = float((g[names[name]] * d).sum())
        err = abs(got - fd) / max(abs(fd), 1.0)
        print(f"env {e} {name}: g.d {got:+.6e} fd {fd:+.6e} err {err:.2e}")
        assert err <= FD_TOL, (name, got, fd)


def test_the_behaviour_on_the_cpu_chain():
    """Identifying a payload on the oracle (behaviour_case): dL/d mass_scale[trunk] is negative and
    within 1e-5 of the central difference of two oracle rollouts at h = 1e-3 (measured 1.15e-6: the
    difference's truncation); ten times that disagreement, 1e-5 at most, is the GPU test's bar."""
    b = pbr.behaviour_case()
    print(f"\nbehaviour on the CPU chain: grad {b['grad']:.6e} fd {b['fd']:.6e} "
          f"disagreement {b['disagreement']:.2e}, GPU bar {pbr.behaviour_bar():.2e}")
    assert b["grad"] < 0
    assert b["disagreement"] <= FD_TOL
