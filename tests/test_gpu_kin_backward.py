"""GPU tests of the kinematics' backward pass (include/osc_kin_backward.h,
osc_batch_kinematics_backward; csrc/osc_kin_backward.hip; KinematicsBatch.backward_into and
osc_amd.autograd.kinematics_differentiable / solve_differentiable_qpos) against the torch
reference tests/kin_backward_ref.py, which tests/test_kin_backward_ref.py pins to finite
differences of the oracle:
   1. parity on the shipped Go2 and WaLTER trees, four random trees and a tree at the table limits
      (16 bodies, 32 dofs, 32 sites), each cotangent alone and all together;
   2. the per-env parameters' gradients, a NULL forward field, invalid envs;
   3. structure: batch independence, reproducibility, linearity, quaternion and translation
      properties;
   4. memory: guard bands (tests/guard.py), NULL outputs, refusals;
   5. autograd: gradcheck, what gets a gradient, a tensor on the wrong device;
   6. the chain qpos, qvel, mass_scale -> M, C, J, b -> x, tau -> loss against the CPU chain.

Shapes: 5 envs (a full wave of four one-env rows plus a one-env tail; the limit tree runs two envs
per workgroup), 9 once.  Error per env and output: |g - g_ref|_inf / (1 + |g_ref|_inf).  Bar:
1e-11 -- the forward's bar is 1e-12 (worst measured 2.8e-15), and a gradient entry sums 30-50 x
more products than a forward entry (about 900 for Go2, 1,700 for WaLTER), which allows one more
decade.  The chain: backward_ref.env_errors and 1e-5 (NORM_TOL), as tests/test_gpu_backward_data.py.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kin_backward_ref as kbr
import kin_env_ref as ker
import kinematics as kin
from guard import assert_guards_intact, guarded, guarded_like
from kin_trees import chain_tree, mixed_tree, random_tree
from osc_amd import _lib
from osc_amd.kinematics import (KinEnvGrads, KinEnvParams, KinematicsBatch, load_tree,
                                random_states)

pytestmark = pytest.mark.gpu

TOL = 1e-11
NENV = 5
NMAX = 9
GO2, WALTER = "unitree_go2", "walter_sr"
OUT, IN = kbr.OUTPUTS, kbr.INPUTS
FIELDS = KinEnvParams.FIELDS
COT_SETS = [(k,) for k in OUT] + [OUT]


def limit_tree(seed=11):
    """A tree at the table limits: 16 bodies (a free root, six balls, eight hinges, one welded),
    nv = 6 + 18 + 8 = 32, 32 sites."""
    t = random_tree(seed, nbody=16, nsite=32, weld_p=0.0)
    for i, b in enumerate(t["bodies"][1:], start=1):
        b["joint"] = "ball" if i <= 6 else "hinge" if i <= 14 else "none"
    return t


TREES = {GO2: lambda: load_tree(GO2), WALTER: lambda: load_tree(WALTER),
         "random_1": lambda: random_tree(1), "random_fixed": lambda: random_tree(4, free_root=False),
         "chain": lambda: chain_tree(2), "mixed_3": lambda: mixed_tree(3), "limit": limit_tree}


@functools.lru_cache(maxsize=None)
def setup(name):
    """(tree, oracle model, KinematicsBatch, states, drawn parameters, cotangents) of a tree, NMAX
    envs, shared by the tests (left unchanged)."""
    tree = TREES[name]()
    m = kin.KinModel(tree)
    kb = KinematicsBatch(tree=tree)
    assert (kb.nq, kb.nv, kb.ns, kb.nbody) == (m.nq, m.nv, m.ns, m.nbody)
    qpos, qvel = random_states(tree, NMAX, 200 + len(name), base_pos_zero=False)
    return tree, m, kb, qpos, qvel, ker.draw(tree, NMAX, 300 + len(name)), \
        kbr.draw_cotangents(m, NMAX, 400 + len(name))


def pick(cots, keys, rows=slice(None)):
    return {k: cots[k][rows] for k in keys}


@functools.lru_cache(maxsize=None)
def reference(name, nenv, with_params):
    """The torch reference's gradients of the first nenv envs for every set of COT_SETS (one
    forward per env; computed once, read-only)."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, nenv)
    params = {k: v[rows] for k, v in p.items()} if with_params else None
    return kbr.batch_vjp_multi(tree, qpos[rows], qvel[rows], params,
                               [pick(cots, ks, rows) for ks in COT_SETS])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def block(p, fields=FIELDS, rows=slice(None)):
    return KinEnvParams(**{k: dev(p[k][rows]) for k in fields})


def shapes(kb, n):
    return dict(qpos=(n, kb.nq), qvel=(n, kb.nv), mass_scale=(n, kb.nbody),
                com_offset=(n, kb.nbody, 3), armature_scale=(n, kb.nv))


def backward(kb, qpos, qvel, cots, want=IN, kin_params=None):
    """name -> gradient (numpy) of the outputs in `want`, the others passed as NULL; cots: dict of
    numpy cotangents (absent = NULL).  Outputs start as NaN."""
    n = qpos.shape[0]
    sh = shapes(kb, n)
    o = {k: torch.full(sh[k], float("nan"), dtype=torch.float64, device=kb.device) for k in want}
    g = {k: dev(v) for k, v in cots.items()}
    fields = [k for k in FIELDS if k in o]
    kg = KinEnvGrads(**{k: o[k] for k in fields}) if fields else None
    kb.backward_into(dev(qpos), dev(qvel), grad_M=g.get("M"), grad_C=g.get("C"),
                     grad_J=g.get("J"), grad_b=g.get("b"), grad_site_xpos=g.get("site_xpos"),
                     grad_qpos=o.get("qpos"), grad_qvel=o.get("qvel"), kin_params=kin_params,
                     kin_grads=kg)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def errors(g, ref):
    """Per env: |g - ref|_inf / (1 + |ref|_inf)."""
    g, ref = g.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    return np.abs(g - ref).max(axis=1) / (1 + np.abs(ref).max(axis=1))


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. parity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name,nenv", [(n, NENV) for n in TREES] + [("random_1", NMAX)])
def test_parity_with_the_torch_reference(gpu, name, nenv):
    """Each cotangent alone and all together, every env, grad_qpos and grad_qvel (the parameter
    gradients at the identity too) within 1e-11 of the reference.

    Worst measured on an MI355X per tree, grad qpos / qvel / mass_scale / com_offset (armature_scale
    is exact):
      Go2            1.8e-14 / 4.8e-15 / 6.2e-16 / 1.1e-15
      WaLTER         4.8e-15 / 2.6e-15 / 9.3e-16 / 1.0e-15
      random_1       6.1e-15 / 1.4e-15 / 1.0e-15 / 8.1e-16   (9 envs: 6.1e-15 / 1.5e-15 / 1.0e-15 / 9.0e-16)
      random_fixed   2.5e-15 / 1.7e-15 / 9.7e-16 / 8.2e-16
      chain          3.2e-15 / 2.1e-15 / 5.7e-15 / 3.0e-15
      mixed_3        2.0e-15 / 1.1e-15 / 1.6e-15 / 1.7e-15
      limit          3.8e-15 / 4.7e-15 / 3.2e-15 / 3.2e-15
    None exceeds 1e-12."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, nenv)
    ref = reference(name, nenv, False)
    worst = dict.fromkeys(IN, 0.0)
    for ks, r in zip(COT_SETS, ref):
        got = backward(kb, qpos[rows], qvel[rows], pick(cots, ks, rows))
        for k in IN:
            assert np.isfinite(got[k]).all(), (ks, k)
            e = errors(got[k], r[k])
            worst[k] = max(worst[k], e.max())
            assert e.max() <= TOL, (ks, k, int(e.argmax()), e.max())
    print(f"\nkin backward {name} nenv={nenv}: worst " +
          "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- 2. per-env parameters -----------------------------------------------------------------------

@pytest.mark.parametrize("name", [GO2, "random_1"])
def test_parameter_gradients_with_drawn_parameters(gpu, name):
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, NENV)
    ref = reference(name, NENV, True)
    for ks, r in zip(COT_SETS, ref):
        got = backward(kb, qpos[rows], qvel[rows], pick(cots, ks, rows),
                       kin_params=block(p, rows=rows))
        errs = {k: errors(got[k], r[k]).max() for k in IN}
        print(f"\nkin backward params {name} {ks if len(ks) == 1 else 'all'}: " +
              "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k in IN:
            assert errs[k] <= TOL, (ks, k, errs[k])
    assert np.abs(ref[-1]["mass_scale"]).max() > 1 and np.abs(ref[-1]["com_offset"]).max() > 1


@pytest.mark.parametrize("name", [GO2, "random_1"])
def test_null_forward_field_is_the_identity_array(gpu, name):
    """The gradient of a field whose forward pointer is NULL is the gradient at the identity-valued
    array, within the bar -- each field alone NULL among drawn others, and all three."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, NENV)
    ident = ker.identity(tree, NMAX)
    for null in [(f,) for f in FIELDS] + [FIELDS]:
        given = tuple(f for f in FIELDS if f not in null)
        full = dict(p, **{f: ident[f] for f in null})
        a = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows),
                     kin_params=block(p, given, rows) if given else None)
        b = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows),
                     kin_params=block(full, rows=rows))
        for k in IN:
            assert errors(a[k], b[k]).max() <= TOL, (null, k)


INVALID = {"mass NaN": ("mass_scale", (2, 2), np.nan), "mass 0": ("mass_scale", (2, 0), 0.0),
           "mass -1": ("mass_scale", (2, 12), -1.0), "com +inf": ("com_offset", (2, 4, 1), np.inf),
           "armature -0.5": ("armature_scale", (2, 17), -0.5)}


@pytest.mark.parametrize("what", list(INVALID))
def test_invalid_env_gets_zeros_and_the_others_are_untouched(gpu, what):
    tree, m, kb, qpos, qvel, p, cots = setup(GO2)
    rows = slice(0, NENV)
    field, idx, value = INVALID[what]
    bad = {k: v[rows].copy() for k, v in p.items()}
    bad[field][idx] = value
    good = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows),
                    kin_params=block(p, rows=rows))
    got = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows), kin_params=block(bad))
    others = [e for e in range(NENV) if e != 2]
    for k in IN:
        assert (got[k][2] == 0.0).all(), k
        assert bitwise(got[k][others], good[k][others]), k
        assert np.abs(good[k][2]).max() > 0, k


# ---- 3. structure --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GO2, "limit"])
def test_batch_independence_and_reproducibility(gpu, name):
    """Batches of 1, 4 and 5 envs: every env bitwise its one-env call and what it is in the batch
    of 5; two identical calls bitwise equal."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    run = lambda rows: backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows),
                                kin_params=block(p, rows=rows))
    full = run(slice(0, NENV))
    again = run(slice(0, NENV))
    for k in IN:
        assert bitwise(full[k], again[k]), k
    for n in (1, 4):
        part = run(slice(0, n))
        for k in IN:
            assert bitwise(part[k], full[k][:n]), (n, k)
    for e in range(1, NENV):
        one = run(slice(e, e + 1))
        for k in IN:
            assert bitwise(one[k], full[k][e:e + 1]), (e, k)


@pytest.mark.parametrize("name", [GO2, "mixed_3", "limit"])
def test_linearity(gpu, name):
    """All cotangents together equal the sum of each alone, within the bar."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, NENV)
    run = lambda ks: backward(kb, qpos[rows], qvel[rows], pick(cots, ks, rows),
                              kin_params=block(p, rows=rows))
    parts = [run((k,)) for k in OUT]
    whole = run(OUT)
    for k in IN:
        e = errors(sum(q[k] for q in parts), whole[k]).max()
        print(f"\nlinearity {name} {k}: {e:.2e}")
        assert e <= TOL, k


@pytest.mark.parametrize("name", [GO2, WALTER, "mixed_3", "limit"])
def test_quaternion_and_translation_properties(gpu, name):
    """Without grad_site_xpos nothing depends on a free root's position; a quaternion's four
    gradient components are orthogonal to it (the kernel's own normalisation)."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, NENV)
    g = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT[:4], rows), want=("qpos",))["qpos"]
    scale = 1 + np.abs(g).max(axis=1)
    nquat = 0
    for j in m.joints:
        qa = j["qadr"]
        if j["type"] == "free":
            assert (np.abs(g[:, qa:qa + 3]).max(axis=1) <= TOL * scale).all()
            qa += 3
        if j["type"] in ("free", "ball"):
            nquat += 1
            dot = np.einsum("ei,ei->e", g[:, qa:qa + 4], qpos[rows, qa:qa + 4])
            assert (np.abs(dot) <= TOL * scale).all(), (j["type"], np.abs(dot).max())
            assert np.abs(g[:, qa:qa + 4]).max() > 1e-3
    assert nquat >= 1


# ---- 4. memory -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GO2, "limit"])
def test_no_access_outside_the_arrays(gpu, name):
    """Every input, cotangent and output between guard bands at its exact size: the bands are
    intact, the inputs unmodified, and the results bitwise the ordinary call's whether the bands
    around the inputs hold 0x00 or 0xFF."""
    tree, m, kb, qpos, qvel, p, cots = setup(name)
    rows = slice(0, NENV)
    ref = backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows),
                   kin_params=block(p, rows=rows))
    sh = shapes(kb, NENV)
    for pad in (0x00, 0xFF):
        fill = 0xA5 if pad == 0 else 0x5A
        ins = {k: guarded_like(dev(v[rows]), pad) for k, v in
               dict(p, qpos=qpos, qvel=qvel, **{"grad_" + k: cots[k] for k in OUT}).items()}
        kept = {k: v.clone() for k, v in ins.items()}
        o = {k: guarded(sh[k], torch.float64, gpu, fill=fill) for k in IN}
        kb.backward_into(ins["qpos"], ins["qvel"], **{"grad_" + k: ins["grad_" + k] for k in OUT},
                         grad_qpos=o["qpos"], grad_qvel=o["qvel"],
                         kin_params=KinEnvParams(**{k: ins[k] for k in FIELDS}),
                         kin_grads=KinEnvGrads(**{k: o[k] for k in FIELDS}))
        torch.cuda.synchronize()
        for k in IN:
            assert_guards_intact(o[k], k)
            assert bitwise(o[k].cpu().numpy(), ref[k]), (k, hex(pad))
        for k, t in ins.items():
            assert_guards_intact(t, "input " + k)
            assert torch.equal(t, kept[k]), k


def test_null_outputs_leave_the_others_unchanged(gpu):
    tree, m, kb, qpos, qvel, p, cots = setup(GO2)
    rows = slice(0, NENV)
    run = lambda want: backward(kb, qpos[rows], qvel[rows], pick(cots, OUT, rows), want=want,
                                kin_params=block(p, rows=rows))
    full = run(IN)
    for drop in IN:
        part = run(tuple(k for k in IN if k != drop))
        assert drop not in part
        for k in part:
            assert bitwise(part[k], full[k]), (drop, k)
    for only in IN:
        assert bitwise(run((only,))[only], full[only]), only


def test_refusals_leave_the_outputs_untouched(gpu):
    tree, m, kb, qpos, qvel, p, cots = setup(GO2)
    L, n = _lib.lib(), NENV
    SENT = -12345.0
    sh = shapes(kb, n)
    o = {k: torch.full(sh[k], SENT, dtype=torch.float64, device=gpu) for k in IN}
    qp, qv, gM, ms = dev(qpos[:n]), dev(qvel[:n]), dev(cots["M"][:n]), dev(p["mass_scale"][:n])
    vp = ctypes.c_void_p
    ptr = lambda t: vp(t.data_ptr())
    kg = _lib.OscKinEnvGrads(*[o[k].data_ptr() for k in FIELDS])
    stream = vp(torch.cuda.current_stream(gpu).cuda_stream)

    def call(h=kb._h, nenv=n, qpos=ptr(qp), qvel=ptr(qv), kp=None, gM=ptr(gM), gq=ptr(o["qpos"]),
             gv=ptr(o["qvel"]), kg=ctypes.byref(kg)):
        return L.osc_batch_kinematics_backward(h, nenv, qpos, qvel, kp, gM, None, None, None, None,
                                               gq, gv, kg, stream)

    odd_p = _lib.OscKinEnvParams(mass_scale=ms.data_ptr() + 4)
    odd_g = _lib.OscKinEnvGrads(com_offset=o["com_offset"].data_ptr() + 4)
    calls = {"NULL kin": dict(h=None), "nenv < 0": dict(nenv=-1), "NULL qpos": dict(qpos=None),
             "NULL qvel": dict(qvel=None), "odd qpos": dict(qpos=vp(qp.data_ptr() + 4)),
             "odd cotangent": dict(gM=vp(gM.data_ptr() + 4)),
             "odd output": dict(gq=vp(o["qpos"].data_ptr() + 4)),
             "odd parameter": dict(kp=ctypes.byref(odd_p)),
             "odd parameter gradient": dict(kg=ctypes.byref(odd_g)),
             "every output NULL": dict(gq=None, gv=None, kg=None)}
    for what, kw in calls.items():
        assert call(**kw) == 1, what
        torch.cuda.synchronize()
        for k in IN:
            assert (o[k] == SENT).all(), (what, k)
    assert call(nenv=0) == 0
    torch.cuda.synchronize()
    assert all((o[k] == SENT).all() for k in IN)
    assert call() == 0
    torch.cuda.synchronize()
    assert not any((o[k] == SENT).any() for k in IN)


# ---- 5. autograd -----------------------------------------------------------------------------------

def test_gradcheck(gpu):
    from osc_amd.autograd import kinematics_differentiable
    tree, m, kb, qpos, qvel, p, cots = setup("mixed_3")
    # (armature scales off zero: the differences step to either side, and a negative one is invalid)
    leaves = [dev(a[:2]).requires_grad_(True) for a in
              (qpos, qvel, p["mass_scale"], p["com_offset"], p["armature_scale"] + 0.5)]

    def fn(qp, qv, ms, dc, arm):
        return kinematics_differentiable(kb, qp, qv, KinEnvParams(ms, dc, arm), want_sites=True)

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-5)


def test_autograd_fills_only_what_is_asked(gpu):
    from osc_amd.autograd import kinematics_differentiable
    tree, m, kb, qpos, qvel, p, cots = setup(GO2)
    n = NENV
    qp, qv = dev(qpos[:n]).requires_grad_(True), dev(qvel[:n])
    ms, dc = dev(p["mass_scale"][:n]).requires_grad_(True), dev(p["com_offset"][:n])
    kp = KinEnvParams(mass_scale=ms, com_offset=dc, armature_scale=p["armature_scale"][:n])
    outs = kinematics_differentiable(kb, qp, qv, kin_params=kp)
    assert len(outs) == 4
    plain = kb.compute(dev(qpos[:n]), dev(qvel[:n]), want_sites=False, kin_params=kp)
    for a, k in zip(outs, OUT):
        assert torch.equal(a.detach(), getattr(plain, k)), k
    g = {k: dev(cots[k][:n]) for k in OUT[:4]}
    sum((a * g[k]).sum() for a, k in zip(outs, OUT)).backward()
    assert qv.grad is None and dc.grad is None
    ref = backward(kb, qpos[:n], qvel[:n], pick(cots, OUT[:4], slice(0, n)),
                   want=("qpos", "mass_scale"), kin_params=kp)
    assert bitwise(qp.grad.cpu().numpy(), ref["qpos"])
    assert bitwise(ms.grad.cpu().numpy(), ref["mass_scale"])
    # five outputs with want_sites; no parameters at all
    qv2 = dev(qvel[:n]).requires_grad_(True)
    outs = kinematics_differentiable(kb, dev(qpos[:n]), qv2, want_sites=True)
    assert len(outs) == 5
    outs[1].sum().backward()
    assert qv2.grad is not None and torch.isfinite(qv2.grad).all()
    with pytest.raises(ValueError):
        kinematics_differentiable(kb, qp, qv, kin_params=KinEnvParams(
            mass_scale=torch.ones((n, kb.nbody), dtype=torch.float64, requires_grad=True)))
    with pytest.raises(TypeError):
        kinematics_differentiable(kb, qp, qv, kin_params=dict(mass_scale=ms))


# ---- 6. the chain ----------------------------------------------------------------------------------

CHAIN_SEED = 7
# Feet that carry load at the optimum of each env's QP.  A foot that would rest at the friction
# pyramid's apex (zero force: its pyramid rows at zero slack with zero multipliers, weakly active)
# is masked off instead, which pins its force and drops those rows; chain_reference asserts that
# what is left has no weakly active row, for every env.
CHAIN_MASK = [[0, 1, 1, 0], [1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 1], [1, 1, 1, 1]]


def chain_inputs():
    from osc_qp import load_model
    tree = load_tree(GO2)
    mdl = load_model(GO2)
    from osc_amd.synth import generate
    qpos, qvel = random_states(tree, NENV, CHAIN_SEED, joint_range=0.5, vel_scale=0.1)
    rng = np.random.default_rng(CHAIN_SEED)
    T = generate(GO2, NENV, CHAIN_SEED, "standing", "ones")["T"]
    mask = np.array(CHAIN_MASK, dtype=np.float64)
    ms = ker.draw(tree, NENV, CHAIN_SEED + 1)["mass_scale"]
    c = rng.standard_normal((NENV, mdl.n))
    return tree, mdl, qpos, qvel, T, mask, ms, c


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The CPU chain: the oracle's M, C, J, b of each env's own tree, its certified optimum, the
    reference adjoint of the solve (tests/backward_data_ref.py) with gx = c + 2 tau on the torque
    block, then the torch reference's VJP.  Every env must have a clean working set: no one-sided
    row that is active with a (near-)zero multiplier or inactive with (near-)zero slack."""
    import backward_data_ref as bd
    from osc_qp import build_qp
    from qp_exact import _constraints, certified, solve_exact
    tree, mdl, qpos, qvel, T, mask, ms, c = chain_inputs()
    m = kin.KinModel(tree)
    out, taus = [], []
    for e in range(NENV):
        p = dict(mass_scale=ms)
        M, C, J, b = ker.kinematics(tree, p, e, qpos[e], qvel[e])
        qp = build_qp(mdl, M, C, J, b, T[e], mask[e])
        sol = solve_exact(mdl, qp, M, C, J)
        assert certified(sol.cert, 1e-8), (e, sol.cert)
        ymax = 1 + np.abs(sol.y).max()
        for i, sign, bound in _constraints(qp)[1]:
            slack = bound - sign * (qp.A[i] @ sol.x)
            if sol.y[i] * sign > 0:      # this side of the row is in the working set
                assert abs(sol.y[i]) > 1e-4 * ymax, ("weakly active row", e, i, sol.y[i])
            elif sol.y[i] == 0:
                assert slack > 1e-6 * (1 + abs(bound)), ("weakly active row", e, i, slack)
        gx = c[e].copy()
        tau = sol.x[mdl.nv:mdl.nv + mdl.nu]
        gx[mdl.nv:mdl.nv + mdl.nu] += 2.0 * tau
        g = bd.reference_adjoint_data(mdl, M, C, J, b, T[e], mask[e], gx, sol.x, sol.y)
        out.append(kbr.vjp(m, qpos[e], qvel[e], dict(mass_scale=ms[e]),
                           dict(M=g["M"], C=g["C"], J=g["J"], b=g["b"])))
        taus.append(tau)
    return {k: np.stack([o[k] for o in out]) for k in IN}, np.array(taus)


def test_chain_through_the_solve(gpu):
    """solve_differentiable_qpos on Go2, 5 envs, loss tau^2 + x . c: grad qpos, grad qvel and grad
    mass_scale against the CPU chain, every env, within 1e-5 (backward_ref.env_errors); forward tau
    bitwise KinematicsBatch.solve's."""
    import backward_ref as br
    from osc_amd.autograd import solve_differentiable_qpos
    from osc_amd.solver import OSCBatchSolver
    from test_gpu_parity import NORM_TOL
    tree, mdl, qpos, qvel, T, mask, ms, c = chain_inputs()
    ref, tau_ref = chain_reference()
    s, kb = OSCBatchSolver(GO2), KinematicsBatch(tree=tree)
    qp, qv = dev(qpos).requires_grad_(True), dev(qvel).requires_grad_(True)
    msd = dev(ms).requires_grad_(True)
    tau, x, status = solve_differentiable_qpos(s, kb, qp, qv, dev(T), dev(mask),
                                               kin_params=KinEnvParams(mass_scale=msd))
    assert (status == 0).all(), status
    plain = kb.solve(s, dev(qpos), dev(qvel), dev(T), dev(mask),
                     kin_params=KinEnvParams(mass_scale=dev(ms)))
    torch.cuda.synchronize()
    assert torch.equal(tau.detach(), plain.tau)
    assert np.abs(tau.detach().cpu().numpy() - tau_ref).max() <= 1e-5 * (1 + np.abs(tau_ref).max())
    (tau.square().sum() + (x * dev(c)).sum()).backward()
    got = dict(qpos=qp.grad, qvel=qv.grad, mass_scale=msd.grad)
    for k, t in got.items():
        e = br.env_errors(t.cpu().numpy(), ref[k])
        print(f"\nchain {k}: worst {e.max():.3e} (env {e.argmax()})")
        assert e.max() <= NORM_TOL, (k, int(e.argmax()), e.max())
