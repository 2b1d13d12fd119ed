"""CPU reference of the forward dynamics' vector-Jacobian product
(include/osc_plant_backward.h).  With qacc = M^-1 (B u + Jc' z + qfrc - C), g the cotangent of qacc
and w = M^-1 g (M symmetric):
    grad_M = -w qacc' (all nv^2 entries, not symmetrised),  grad_C = -w,  grad_qfrc = w,
    grad_u = w[nb:],  grad_Jc = z w' (the contact rows only),  grad_z = Jc w.
fd_vjp is that closed form in float64 numpy; tests/test_plant_backward_ref.py pins it to central
differences of plant_ref.forward_dynamics.  bw_case adds drawn cotangents to plant_ref.fd_case,
with w from plant_ref.refined (the reference of the GPU test) and from plant_ref.ldl_model (the
numpy model of the kernel's solve, whose error sets that test's bar).

TEST INFRASTRUCTURE ONLY.  It lives under tests/ because oracle/ is not to change."""
import functools

import numpy as np

import plant_ref as pr

OUTPUTS = ("M", "C", "Jc", "u", "z", "qfrc")


def contact_rows(model):
    return slice(3 * model.ns - 3 * model.nc, 3 * model.ns)


def fd_vjp(model, J, z, qacc, w):
    """The six gradients of one env from w = M^-1 g; z None: no Jc and z entries."""
    nb = model.nv - model.nu
    out = dict(M=-np.outer(w, qacc), C=-w, qfrc=w.copy(), u=w[nb:].copy())
    if z is not None:
        out["Jc"] = np.outer(z, w)
        out["z"] = J[contact_rows(model)] @ w
    return out


@functools.lru_cache(maxsize=None)
def bw_case(robot, nenv=67, seed=11):
    """plant_ref.fd_case(robot) with `g` ~ U(-10, 10) (the range of its applied force) as the
    cotangent of qacc; `qacc` the refined forward result; `w_ref` the refined w, `w_model` the
    numpy LDL' model's, `model_err` its error per env (plant_ref.fd_error); `ref` the closed form
    on w_ref, name -> (nenv, ...) arrays.  Read-only."""
    c = dict(pr.fd_case(robot, nenv, seed))
    model = pr.load_model(robot)
    rng = np.random.default_rng(seed + 3)
    g = rng.uniform(-10, 10, (nenv, model.nv))
    w_ref = np.array([pr.refined(c["M"][e], g[e]) for e in range(nenv)])
    w_model = np.array([pr.ldl_model(c["M"][e], g[e]) for e in range(nenv)])
    err = np.array([pr.fd_error(w_model[e], w_ref[e]) for e in range(nenv)])
    per_env = [fd_vjp(model, c["J"][e], c["z"][e], c["ref"][e], w_ref[e]) for e in range(nenv)]
    ref = {k: np.array([p[k] for p in per_env]) for k in OUTPUTS}
    c.update(g=g, qacc=c["ref"], w_ref=w_ref, w_model=w_model, bw_model_err=err)
    for a in list(c.values()) + list(ref.values()):
        a.setflags(write=False)
    c["grads"] = ref
    return c


def bw_bar(robot):
    """Ten times the worst error of ldl_model's w on bw_case(robot) (the margin covers the kernel's
    FMA ordering, as plant_ref.fd_bar), in any case not above plant_ref.FD_BAR_MAX."""
    return min(10.0 * float(bw_case(robot)["bw_model_err"].max()), pr.FD_BAR_MAX)


def out_errors(got, ref):
    """Per env: |got - ref|_inf / max(|ref|_inf, 1)."""
    got, ref = np.asarray(got).reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1)
    return np.abs(got - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1.0)


# ---- the whole plant rollout's backward, one env -----------------------------------------------------------

def chain(tree, mdl, qpos0, qvel0, mask, nticks, dt, cot, T=None, pd=None, kin_params=None,
          plant_params=None, qfrc_seq=None, clean=True, where=""):
    """One env: the forward rollout against a plant on the oracle (plant_ref.rollout's tick) and the
    gradient of sum(cot[k] * hist[k]) over k in qpos, qvel, tau, qacc, composed of the existing
    oracle pieces -- rollout_backward_ref.step_vjp and pd_vjp, backward_data_ref.
    reference_adjoint_data, kin_backward_ref.vjp TWICE (the controller's and the plant's
    parameters) -- and the closed form fd_vjp above.
      kin_params    None or dict: the CONTROLLER's own arrays
      plant_params  None (the plant shares the controller's) or dict: the PLANT's own arrays
      qfrc_seq      None or (nticks, nv): the applied force of every tick
      clean         rollout_backward_ref.assert_clean at every tick (no weakly active row)
    Returns (grads, hist): grads = dict(qpos0, qvel0, T (held), "kin.<field>", "plant.kin.<field>",
    "plant.qfrc_applied" (nticks, nv)), the sums in the order K-1 .. 0; hist = dict(qpos, qvel,
    tau, qacc)."""
    import torch  # noqa: F401  (rollout_backward_ref needs it)

    import backward_data_ref as bd
    import kin_backward_ref as kbr
    import kin_env_ref as ker
    import kinematics as kin
    import rollout_backward_ref as rbr
    from osc_qp import build_qp
    from qp_exact import certified, solve_exact
    assert (T is None) != (pd is None)
    m = kin.KinModel(tree)
    nv, nu, nb = mdl.nv, mdl.nu, mdl.nv - mdl.nu
    rows = contact_rows(mdl)
    one = lambda p: None if p is None else {k: np.asarray(v)[None] for k, v in p.items()}
    kinem = lambda p1, q, v: ker.kinematics(tree, p1, 0, q, v) if p1 is not None else \
        kin.kinematics(m, q, v)
    c1, p1 = one(kin_params), one(plant_params)
    qh, vh, th, ah, ticks = [np.array(qpos0, float)], [np.array(qvel0, float)], [], [], []
    for t in range(nticks):
        q, v = qh[-1], vh[-1]
        if pd is not None:
            Tt = rbr.pd_targets(mdl.ns, rbr._t(q[0:3]), rbr._t(q[3:7]), rbr._t(v[0:3]),
                                rbr._t(v[3:6]), rbr._t(pd[0]), rbr._t(pd[1]), pd[2]).numpy()
        else:
            Tt = np.asarray(T, float)
        M, C, J, b = kinem(c1, q, v)
        qp = build_qp(mdl, M, C, J, b, Tt, mask)
        sol = solve_exact(mdl, qp, M, C, J)
        if clean:
            rbr.assert_clean(qp, sol, (where, t))
        else:
            assert certified(sol.cert, 1e-8), (where, t, sol.cert)
        Mp, Cp = (M, C) if p1 is None else kinem(p1, q, v)[:2]
        f = None if qfrc_seq is None else qfrc_seq[t]
        qacc = pr.forward_dynamics(mdl, Mp, Cp, J, sol.x[nv:nv + nu], sol.x[nv + nu:], f)
        qn, vn = rbr.step(m, rbr._t(q), rbr._t(v), rbr._t(qacc), dt)
        qh.append(qn.numpy())
        vh.append(vn.numpy())
        th.append(sol.x[nv:nv + nu].copy())
        ah.append(qacc)
        ticks.append((M, C, J, b, Tt, sol, Mp, qacc))
    gq, gv = np.array(cot["qpos"][nticks], float), np.array(cot["qvel"][nticks], float)
    sums, gf = {}, np.zeros((nticks, nv))

    def add(k, v):
        sums[k] = v if k not in sums else sums[k] + v

    for t in range(nticks - 1, -1, -1):
        M, C, J, b, Tt, sol, Mp, qacc = ticks[t]
        dq, dvv, da = rbr.step_vjp(m, qh[t], vh[t], qacc, dt, gq, gv)
        w = np.linalg.solve(Mp, da + cot["qacc"][t])
        fd = fd_vjp(mdl, J, sol.x[nv + nu:], qacc, w)
        gf[t] = fd["qfrc"]
        gx = np.zeros(mdl.n)
        gx[nv:nv + nu] = cot["tau"][t] + fd["u"]
        gx[nv + nu:] = fd["z"]
        g = bd.reference_adjoint_data(mdl, M, C, J, b, Tt, mask, gx, sol.x, sol.y)
        gJ = np.array(g["J"], float)
        gJ[rows] += fd["Jc"]
        gM, gC = np.array(g["M"], float), np.array(g["C"], float)
        if plant_params is None:
            gM, gC = gM + fd["M"], gC + fd["C"]
        k = kbr.vjp(m, qh[t], vh[t], kin_params, dict(M=gM, C=gC, J=gJ, b=g["b"]))
        gq, gv = dq + k["qpos"], dvv + k["qvel"]
        if plant_params is not None:
            kp = kbr.vjp(m, qh[t], vh[t], plant_params, dict(M=fd["M"], C=fd["C"]))
            gq, gv = gq + kp["qpos"], gv + kp["qvel"]
            for name in plant_params:
                add("plant.kin." + name, kp[name])
        if pd is not None:
            gp, gqt, gl, ga = rbr.pd_vjp(mdl.ns, qh[t][3:7], pd[0], pd[1], pd[2], g["T"])
            gq[0:3] += gp
            gq[3:7] += gqt
            gv[0:3] += gl
            gv[3:6] += ga
        else:
            add("T", g["T"])
        gq = gq + cot["qpos"][t]
        gv = gv + cot["qvel"][t]
        for name in (kin_params or {}):
            add("kin." + name, k[name])
    grads = dict(qpos0=gq, qvel0=gv, **sums)
    grads["plant.qfrc_applied"] = gf
    return grads, dict(qpos=np.array(qh), qvel=np.array(vh), tau=np.array(th).reshape(nticks, nu),
                       qacc=np.array(ah).reshape(nticks, nv))


CHAIN_K = 3
CHAIN_NENV = 5
HELD_MASK = [[0, 1, 1, 0], [1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 0, 1], [1, 1, 1, 1]]   # tests/
# test_rollout_backward_ref.py's held case, restated (that module needs a built library to import)


@functools.lru_cache(maxsize=None)
def chain_case():
    """The Go2 case of the chain, clean at all 5 envs x 3 ticks: states random_states(seed 7),
    targets generate(seed 7, "standing", "ones"), HELD_MASK, the controller's mass_scale from
    kin_env_ref.draw(seed 8), the plant's three fields from draw(seed 9), the applied force
    rng(9).uniform(-2, 2) held over K = 3 with +30 on column 0 at tick 1; cotangents on every slab
    of the four histories.  Inputs and, per env, chain's (grads, hist); read-only."""
    import kin_env_ref as ker
    from osc_amd.kinematics import load_tree, random_states
    from osc_amd.synth import generate
    tree, mdl = load_tree(pr.GO2), pr.load_model(pr.GO2)
    n, K = CHAIN_NENV, CHAIN_K
    qpos, qvel = random_states(tree, n, 7, joint_range=0.5, vel_scale=0.1)
    T = np.array(generate(pr.GO2, n, 7, "standing", "ones")["T"])
    ms = ker.draw(tree, n, 8)["mass_scale"]
    plant = ker.draw(tree, n, 9)
    f = np.random.default_rng(9).uniform(-2, 2, (n, mdl.nv))
    seq = np.broadcast_to(f, (K, n, mdl.nv)).copy()
    seq[1, :, 0] += 30.0
    rng = np.random.default_rng(17)
    cot = dict(qpos=rng.standard_normal((K + 1, n, qpos.shape[1])),
               qvel=rng.standard_normal((K + 1, n, mdl.nv)),
               tau=0.1 * rng.standard_normal((K, n, mdl.nu)),
               qacc=0.01 * rng.standard_normal((K, n, mdl.nv)))
    c = dict(qpos=qpos, qvel=qvel, T=T, mask=np.array(HELD_MASK, dtype=np.float64), ms=ms,
             qfrc_seq=seq, **{"plant_" + k: v for k, v in plant.items()},
             **{"cot_" + k: v for k, v in cot.items()})
    for a in c.values():
        a.setflags(write=False)
    c["tree"], c["model"] = tree, mdl
    c["out"] = [chain(tree, mdl, qpos[e], qvel[e], c["mask"][e], K, pr.DT,
                      {k: v[:, e] for k, v in cot.items()}, T=T[e],
                      kin_params=dict(mass_scale=ms[e]),
                      plant_params={k: plant[k][e] for k in plant}, qfrc_seq=seq[:, e], where=e)
                for e in range(n)]
    return c


def chain_grads(c):
    """chain_case's gradients env-major (plant.qfrc_applied tick-major: (K, nenv, nv))."""
    out = {k: np.stack([o[0][k] for o in c["out"]]) for k in c["out"][0][0]}
    out["plant.qfrc_applied"] = np.moveaxis(out["plant.qfrc_applied"], 0, 1)
    return out


# ---- the behaviour: identifying a payload ----------------------------------------------------------------

BEHAVIOUR_K = 20
BEHAVIOUR_H = 1e-3


@functools.lru_cache(maxsize=None)
def behaviour_case():
    """rollout_ref.go2_case, PD targets, K = 20: the log is the base-height history of a plant
    whose trunk is plant_ref.TRUNK_SCALE x heavier; the loss is the squared base-height history
    error of a plant at 1.0 x.  dict(log, grad: chain's dL/d mass_scale[trunk], fd: the central
    difference of two oracle rollouts at h = 1e-3, disagreement: |grad - fd| / |fd|)."""
    import kin_env_ref as ker
    import rollout_ref
    from osc_amd.kinematics import load_tree
    km, mdl, qpos, qvel, mask, pdt = rollout_ref.go2_case()
    tree = load_tree(pr.GO2)
    K = BEHAVIOUR_K

    def heights(scale):
        kp = ker.env_model(tree, mass_scale=pr.go2_mass_scale(tree, scale))
        return pr.rollout(km, kp, mdl, qpos, qvel, mask, K, pr.DT, pd=pdt)["qpos"][:, 2]

    log = heights(pr.TRUNK_SCALE)
    z = heights(1.0)
    cot = dict(qpos=np.zeros((K + 1, km.nq)), qvel=np.zeros((K + 1, km.nv)),
               tau=np.zeros((K, mdl.nu)), qacc=np.zeros((K, km.nv)))
    cot["qpos"][:, 2] = 2.0 * (z - log)
    g, _ = chain(tree, mdl, qpos, qvel, mask, K, pr.DT, cot, pd=pdt,
                 plant_params=dict(mass_scale=pr.go2_mass_scale(tree, 1.0)), clean=False,
                 where="behaviour")
    L = lambda s: float(((heights(s) - log) ** 2).sum())
    h = BEHAVIOUR_H
    fd = (L(1.0 + h) - L(1.0 - h)) / (2 * h)
    grad = float(g["plant.kin.mass_scale"][0])
    return dict(log=log, grad=grad, fd=fd, disagreement=abs(grad - fd) / abs(fd))


def behaviour_bar():
    """Ten times the CPU chain's own disagreement with its central difference, 1e-5 at most."""
    return min(10.0 * behaviour_case()["disagreement"], 1e-5)
