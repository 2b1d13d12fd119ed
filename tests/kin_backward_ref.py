"""Reference of the kinematics' backward pass (include/osc_kin_backward.h) for
tests/test_kin_backward_ref.py (CPU) and tests/test_gpu_kin_backward.py (GPU): a float64 CPU torch
restatement of oracle/kinematics.py's `kinematics` and `site_positions` -- the same formulation,
line for line (COM Jacobians, Kane's method), not the kernel's spatial-vector one -- differentiated
by torch autograd.  The per-env parameters are applied as tests/kin_env_ref.py applies them: mass and
diaginertia x mass_scale, ipos + com_offset, dof armature x armature_scale.

    M, C, J, b, x = forward(m, qpos, qvel, p)         one env; m: kinematics.KinModel; torch tensors
    g = vjp(m, qpos, qvel, params, cots)              one env, numpy in / out
    G = batch_vjp(tree, qpos, qvel, params, cots)     env-major numpy arrays
"""
import numpy as np
import torch

import kinematics as kin

F64 = torch.float64
OUTPUTS = ("M", "C", "J", "b", "site_xpos")
INPUTS = ("qpos", "qvel", "mass_scale", "com_offset", "armature_scale")


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def quat2mat(q):
    w, x, y, z = (q / torch.linalg.vector_norm(q)).unbind()
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])


def axis_angle(a, t):
    a = np.asarray(a, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = _t([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return torch.eye(3, dtype=F64) + torch.sin(t) * K + (1 - torch.cos(t)) * (K @ K)


def cross(a, b):
    return torch.linalg.cross(a, b)


def fk(m, qpos):
    """oracle forward(): lists of body positions / frames and joint anchors / axes."""
    xpos, xmat = [None] * m.nbody, [None] * m.nbody
    anchor, axis = [None] * m.njnt, [None] * m.njnt
    for i, b in enumerate(m.bodies):
        p = b["parent"]
        pp = xpos[p] if p >= 0 else torch.zeros(3, dtype=F64)
        pR = xmat[p] if p >= 0 else torch.eye(3, dtype=F64)
        pos = pp + pR @ _t(b["pos"])
        R = pR @ _t(kin.quat2mat(b["quat"]))
        for ji in m.body_joints[i]:
            j = m.joints[ji]
            qa = j["qadr"]
            if j["type"] == "free":
                pos = qpos[qa:qa + 3]
                R = quat2mat(qpos[qa + 3:qa + 7])
                anchor[ji] = pos
                continue
            axis[ji] = R @ _t(j["axis"])
            if j["type"] == "slide":
                pos = pos + axis[ji] * qpos[qa]
                anchor[ji] = pos
                continue
            anchor[ji] = pos + R @ _t(j["pos"])
            if j["type"] == "hinge":
                R = R @ axis_angle(j["axis"], qpos[qa])
            else:
                R = R @ quat2mat(qpos[qa:qa + 4])
            pos = anchor[ji] - R @ _t(j["pos"])
        xpos[i], xmat[i] = pos, R
    return xpos, xmat, anchor, axis


def point_jacobian(m, f, bi, point):
    xpos, xmat, anchor, axis = f
    z = torch.zeros(3, dtype=F64)
    Jp, Jr = [z] * m.nv, [z] * m.nv
    eye = torch.eye(3, dtype=F64)
    for c in m.chain(bi):
        for ji in m.body_joints[c]:
            j = m.joints[ji]
            da = j["dadr"]
            if j["type"] == "free":
                for k in range(3):
                    Jp[da + k] = eye[:, k]
                    a = xmat[c][:, k]
                    Jr[da + 3 + k] = a
                    Jp[da + 3 + k] = cross(a, point - xpos[c])
            elif j["type"] == "ball":
                for k in range(3):
                    a = xmat[c][:, k]
                    Jr[da + k] = a
                    Jp[da + k] = cross(a, point - anchor[ji])
            elif j["type"] == "hinge":
                Jr[da] = axis[ji]
                Jp[da] = cross(axis[ji], point - anchor[ji])
            else:
                Jp[da] = axis[ji]
    return torch.stack(Jp, dim=1), torch.stack(Jr, dim=1)


def bias_motion(m, f, qvel):
    xpos, xmat, anchor, axis = f
    z = torch.zeros(3, dtype=F64)
    w, al, o, vo, ao = ([None] * m.nbody for _ in range(5))

    def state_at(fr, x):
        fw, fal, fo, fvo, fao = fr
        r = x - fo
        return fvo + cross(fw, r), fao + cross(fal, r) + cross(fw, cross(fw, r))

    for i, b in enumerate(m.bodies):
        p = b["parent"]
        fr = (w[p], al[p], o[p], vo[p], ao[p]) if p >= 0 else (z, z, z, z, z)
        for ji in m.body_joints[i]:
            j = m.joints[ji]
            da = j["dadr"]
            fw, fal = fr[0], fr[1]
            if j["type"] == "free":
                fr = (xmat[i] @ qvel[da + 3:da + 6], z, xpos[i], qvel[da:da + 3], z)
            elif j["type"] in ("hinge", "ball"):
                v0, a0 = state_at(fr, anchor[ji])
                wj = axis[ji] * qvel[da] if j["type"] == "hinge" else xmat[i] @ qvel[da:da + 3]
                fr = (fw + wj, fal + cross(fw, wj), anchor[ji], v0, a0)
            else:
                v0, a0 = state_at(fr, anchor[ji])
                vr = axis[ji] * qvel[da]
                fr = (fw, fal, anchor[ji], v0 + vr, a0 + 2.0 * cross(fw, vr))
        w[i], al[i] = fr[0], fr[1]
        if m.body_joints[i]:
            o[i], vo[i], ao[i] = fr[2], fr[3], fr[4]
        else:
            o[i] = xpos[i]
            vo[i], ao[i] = state_at(fr, xpos[i])

    def accel(bi, x):
        return state_at((w[bi], al[bi], o[bi], vo[bi], ao[bi]), x)
    return w, al, accel


def forward(m, qpos, qvel, p=None):
    """(M, C, J, b, site_xpos) of one env as torch tensors; p: dict of torch tensors mass_scale
    (nbody,), com_offset (nbody, 3), armature_scale (nv,), each optional."""
    p = p or {}
    f = fk(m, qpos)
    xpos, xmat, _, _ = f
    w, al, accel = bias_motion(m, f, qvel)
    arm = _t(m.armature)
    if p.get("armature_scale") is not None:
        arm = arm * p["armature_scale"]
    M = torch.diag(arm)
    C = torch.zeros(m.nv, dtype=F64)
    g = _t(m.gravity)
    for i, b in enumerate(m.bodies):
        mass, ipos, Ib = b["mass"], _t(b["ipos"]), _t(m.Ibody[i])
        if p.get("mass_scale") is not None:
            mass = p["mass_scale"][i] * mass
            Ib = p["mass_scale"][i] * Ib
        if p.get("com_offset") is not None:
            ipos = ipos + p["com_offset"][i]
        com = xpos[i] + xmat[i] @ ipos
        Jc, Jw = point_jacobian(m, f, i, com)
        Iw = xmat[i] @ Ib @ xmat[i].T
        M = M + mass * Jc.T @ Jc + Jw.T @ Iw @ Jw
        _, a_com = accel(i, com)
        C = C + Jc.T @ (mass * (a_com - g)) + Jw.T @ (Iw @ al[i] + cross(w[i], Iw @ w[i]))
    Jps, Jrs, bps, brs, xs = [], [], [], [], []
    for s in m.sites:
        bi = s["body"]
        x = xpos[bi] + xmat[bi] @ _t(s["pos"])
        jb = s.get("jac_body", bi)
        Jp, Jr = point_jacobian(m, f, jb, x)
        _, a = accel(jb, x)
        Jps.append(Jp); Jrs.append(Jr); bps.append(a); brs.append(al[jb]); xs.append(x)
    return M, C, torch.cat(Jps + Jrs), torch.cat(bps + brs), torch.stack(xs)


def vjp_multi(m, qpos, qvel, params, cot_list):
    """One env, one forward, several cotangent sets: for each dict in cot_list (keys of OUTPUTS,
    numpy, absent = zero) the dict of gradients (keys of INPUTS, numpy; the parameter gradients
    are taken at the given params, identity where absent)."""
    ident = dict(mass_scale=np.ones(m.nbody), com_offset=np.zeros((m.nbody, 3)),
                 armature_scale=np.ones(m.nv))
    vals = dict(qpos=qpos, qvel=qvel)
    for k, v in ident.items():
        vals[k] = v if params is None or params.get(k) is None else params[k]
    leaves = {k: _t(v).clone().requires_grad_(True) for k, v in vals.items()}
    outs = dict(zip(OUTPUTS, forward(m, leaves["qpos"], leaves["qvel"], leaves)))
    res = []
    for cots in cot_list:
        loss = sum((outs[k] * _t(c).reshape(outs[k].shape)).sum() for k, c in cots.items()
                   if c is not None)
        gs = torch.autograd.grad(loss, [leaves[k] for k in INPUTS], retain_graph=True,
                                 allow_unused=True)
        res.append({k: (np.zeros(leaves[k].shape) if g is None else g.numpy().copy())
                    for k, g in zip(INPUTS, gs)})
    return res


def vjp(m, qpos, qvel, params, cots):
    return vjp_multi(m, qpos, qvel, params, [cots])[0]


def batch_vjp_multi(tree, qpos, qvel, params, cot_list):
    """Env-major: qpos (nenv, nq), params dict of (nenv, ...) arrays or None, cot_list a list of
    dicts of (nenv, ...) arrays.  Returns a list (one per cotangent set) of dicts of env-major
    gradient arrays."""
    m = kin.KinModel(tree)
    nenv = qpos.shape[0]
    per_env = []
    for e in range(nenv):
        pe = None if params is None else {k: (None if v is None else v[e])
                                          for k, v in params.items()}
        per_env.append(vjp_multi(m, qpos[e], qvel[e], pe,
                                 [{k: (None if c is None else c[e]) for k, c in cots.items()}
                                  for cots in cot_list]))
    return [{k: np.stack([per_env[e][i][k] for e in range(nenv)]) for k in INPUTS}
            for i in range(len(cot_list))]


def batch_vjp(tree, qpos, qvel, params, cots):
    return batch_vjp_multi(tree, qpos, qvel, params, [cots])[0]


def out_shapes(m, nenv=None):
    s = dict(M=(m.nv, m.nv), C=(m.nv,), J=(6 * m.ns, m.nv), b=(6 * m.ns,), site_xpos=(m.ns, 3))
    return s if nenv is None else {k: (nenv,) + v for k, v in s.items()}


def draw_cotangents(m, nenv, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(v) for k, v in out_shapes(m, nenv).items()}
