"""Reference of the per-env inertial parameters (include/osc_kin_env_params.h,
osc_amd.kinematics.KinEnvParams) for tests/test_kin_env_ref.py (CPU) and
tests/test_gpu_kin_env.py (GPU): env e's tree is the model's tree with the three parameters
applied to its fields, and the existing oracle (oracle/kinematics.py) runs on it unchanged.

  mass_scale s      (nbody,)     mass and diaginertia x s (density scaling)
  com_offset d      (nbody, 3)   ipos + d
  armature_scale a  (nv,)        each joint's armature x the a of its dofs

Every dof of one joint shares an armature in the tree schema, so a per-dof `a` is expressible only
when it is constant over each joint's dofs: draw() draws one value per joint and repeats it, and
env_tree() refuses anything else.  The trees here carry one joint per body (the kernel's
descriptor), so body b of the tree is body b of the kinematics model."""
import copy

import numpy as np

import kinematics as kin

NV = kin.KinModel.NV


def _body_joints(b):
    """The joint dicts of a body and the key their armature lives under."""
    if "joints" in b:
        return [(j, j["type"]) for j in b["joints"]]
    return [] if b["joint"] == "none" else [(b, b["joint"])]


def env_tree(tree: dict, mass_scale=None, com_offset=None, armature_scale=None) -> dict:
    """A deep copy of `tree` with one env's parameters applied (None = leave the field alone)."""
    t = copy.deepcopy(tree)
    d = 0
    for i, b in enumerate(t["bodies"]):
        if mass_scale is not None:
            s = float(mass_scale[i])
            b["mass"] = s * b["mass"]
            b["diaginertia"] = [s * v for v in b["diaginertia"]]
        if com_offset is not None:
            b["ipos"] = [float(p) + float(o) for p, o in zip(b["ipos"], com_offset[i])]
        for j, kind in _body_joints(b):
            n = NV[kind]
            if armature_scale is not None:
                a = np.asarray(armature_scale[d:d + n], dtype=np.float64)
                if not (a == a[0]).all():
                    raise ValueError("armature_scale differs within one joint's dofs")
                j["armature"] = float(a[0]) * j.get("armature", 0.0)
            d += n
    return t


def env_model(tree: dict, mass_scale=None, com_offset=None, armature_scale=None) -> kin.KinModel:
    return kin.KinModel(env_tree(tree, mass_scale, com_offset, armature_scale))


def joint_dofs(tree: dict) -> list:
    """Number of dofs of every joint, in dof order."""
    return [NV[kind] for b in tree["bodies"] for _, kind in _body_joints(b)]


def draw(tree: dict, nenv: int, seed: int) -> dict:
    """One draw of the three arrays (numpy float64, env-major): s ~ U(0.5, 2), d ~ U(-0.05, 0.05)
    per coordinate scaled so that |d| <= 0.05 m, a ~ U(0, 3) per joint, repeated over the joint's
    dofs, with a = 0 exactly on the joints (e + k) % 5 == 0 of env e."""
    rng = np.random.default_rng(seed)
    nbody = len(tree["bodies"])
    nd = joint_dofs(tree)
    s = rng.uniform(0.5, 2.0, size=(nenv, nbody))
    d = rng.uniform(-1.0, 1.0, size=(nenv, nbody, 3))
    d *= 0.05 * rng.uniform(0.0, 1.0, size=(nenv, nbody, 1)) / np.linalg.norm(d, axis=2,
                                                                              keepdims=True)
    a_j = rng.uniform(0.0, 3.0, size=(nenv, len(nd)))
    for e in range(nenv):
        a_j[e, [k for k in range(len(nd)) if (e + k) % 5 == 0]] = 0.0
    a = np.repeat(a_j, nd, axis=1)
    return dict(mass_scale=s, com_offset=d, armature_scale=a)


def identity(tree: dict, nenv: int) -> dict:
    nbody, nv = len(tree["bodies"]), sum(joint_dofs(tree))
    return dict(mass_scale=np.ones((nenv, nbody)), com_offset=np.zeros((nenv, nbody, 3)),
                armature_scale=np.ones((nenv, nv)))


def kinematics(tree: dict, p: dict, e: int, qpos, qvel, fields=None):
    """The oracle's (M, C, J, b) of env e under the named fields of p (default: all in p)."""
    kw = {k: p[k][e] for k in (p if fields is None else fields)}
    return kin.kinematics(env_model(tree, **kw), qpos, qvel)
