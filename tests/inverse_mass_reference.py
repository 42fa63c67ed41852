"""The fp64 references of the inverse-mass queries (rsb_apply_inverse_mass, rsb_get_frame_delassus; include/rsb.h), the inputs and the error measures
the CPU tests (tests/test_inverse_mass_reference.py), the restatement tool (tools/inverse_mass_restatement.py) and the GPU tests
(tests/test_gpu_inverse_mass.py) share.  No test lives here.

Cases: six of tests/test_dynamics_reference.dyn_case's - two floating random trees, a fixed-base one, the 40-body tree, the two shipped models (N = 67
or 64) - with their float32-rounded configurations.  A = M_ref + D: Oracle.mass_matrix (the armature on its diagonal) plus diag(joint_diag).
  X_ref     = solve(A, B), the joint block for a fixed base (its six base rows zero)
  JMinv_ref = J_ref A^-1, G_ref = J_ref A^-1 J_ref^T, J_ref the rows of test_dynamics_reference.jacobians (= rsb_get_frame_jacobians) stacked: 3 per
              frame (J_lin) or 6 (J_lin, then J_rot)
Inputs: B is N(0, 1) rounded to float32 from a fixed seed, [N, 5, nv]; R = 1 takes its first column.  joint_diag is None or a fixed-seed
uniform(0, 0.5) on the joints, rounded to float32, zero on the six base entries.  Frame offsets are rounded to float32: what the device receives.
Every function caches its result; nobody writes into what it returns."""
import functools

import numpy as np

from common import f32
from test_dynamics_reference import dyn_case, jacobians, kinematics

CASES = ["floating0", "floating5", "fixed2", "tree40", "anymal", "atlas"]
R_RANDOM = 5
# (right-hand sides, with joint_diag) of the solve; "eye": B = identity, X = A^-1
SOLVE_VARIANTS = [("r1", False), ("r5", False), ("r5", True), ("eye", False)]

BOX_URDF = """<?xml version="1.0"?>
<robot name="box">
  <link name="box">
    <inertial><origin xyz="0.03 -0.02 0.05"/><mass value="3.5"/>
      <inertia ixx="0.04" ixy="0.003" ixz="-0.002" iyy="0.07" iyz="0.004" izz="0.09"/></inertial>
    <collision><origin xyz="0 0 0"/><geometry><sphere radius="0.1"/></geometry></collision>
  </link>
</robot>
"""


def _f32_frames(frames):
    return [(int(b), tuple(float(np.float32(x)) for x in off)) for b, off in frames]


@functools.lru_cache(maxsize=None)
def frame_sets(name):
    """{key: [(body, offset)]}: "one"; "three" - the case's frames, two on one body and one on another; "ancestor" - a frame on the last body and one on
    its parent; the quadruped's four "feet"; "sixteen" frames on floating0 (96 rows with angular: far more than nv)"""
    c = dyn_case(name)
    b1 = c.nb - 1
    sets = {"one": _f32_frames(c.frames[:1]), "three": _f32_frames(c.frames),
            "ancestor": _f32_frames([(b1, (0.05, -0.02, 0.1)), (int(c.blob.parent[b1]), (0.02, 0.03, -0.04))])}
    if name == "anymal":
        sets["feet"] = _f32_frames([(int(c.blob.col_body[s]), tuple(c.blob.col_pos[s])) for s in c.model.collision_indices("_foot")])
    if name == "floating0":
        rng = np.random.default_rng(16)
        sets["sixteen"] = _f32_frames([(k % c.nb, rng.uniform(-0.2, 0.2, 3)) for k in range(16)])
    return sets


def delassus_variants(name):
    """[(frame set, angular, with joint_diag)] every Delassus check runs over"""
    return [(k, a, False) for k in frame_sets(name) for a in (False, True)] + [("three", True, True)]


@functools.lru_cache(maxsize=None)
def joint_diag(name):
    c = dyn_case(name)
    d = np.zeros(c.nv)
    d[6:] = f32(np.random.default_rng(7700 + c.nv).uniform(0.0, 0.5, c.nv - 6))
    return d


@functools.lru_cache(maxsize=None)
def rhs(name, which):
    """B [N, R, nv] float64 holding float32 values: "r5" random, "r1" its first column, "eye" the identity (R = nv)"""
    c = dyn_case(name)
    if which == "eye":
        return np.broadcast_to(np.eye(c.nv), (c.N, c.nv, c.nv)).copy()
    B = f32(np.random.default_rng(7600 + c.nv).normal(size=(c.N, R_RANDOM, c.nv)))
    return B[:, :1].copy() if which == "r1" else B


@functools.lru_cache(maxsize=None)
def system(name, with_diag):
    """A = M_ref + D [N, nv, nv], fp64 (the whole matrix; a fixed base's tests use A[:, 6:, 6:])"""
    c = dyn_case(name)
    return c.M + (np.diag(joint_diag(name)) if with_diag else 0.0)


@functools.lru_cache(maxsize=None)
def inverse_reference(name, with_diag):
    """A^-1 [N, nv, nv]; fixed base: the inverse of the joint block, the base rows and columns zero"""
    c, A = dyn_case(name), system(name, with_diag)
    out = np.zeros_like(A)
    out[:, c.j0:, c.j0:] = np.linalg.inv(A[:, c.j0:, c.j0:])
    return out


@functools.lru_cache(maxsize=None)
def solve_reference(name, which, with_diag):
    """X_ref [N, R, nv] = solve(A, B) per env and column"""
    c, A, B = dyn_case(name), system(name, with_diag), rhs(name, which)
    X = np.zeros_like(B)
    for e in range(c.N):
        X[e, :, c.j0:] = np.linalg.solve(A[e, c.j0:, c.j0:], B[e, :, c.j0:].T).T
    return X


@functools.lru_cache(maxsize=None)
def stacked_jacobian(name, key, angular):
    """J_ref [N, kF, nv]: per frame the three rows of J_lin, with angular followed by the three of J_rot"""
    c = dyn_case(name)
    frames = frame_sets(name)[key]
    kk = 6 if angular else 3
    J = np.zeros((c.N, kk * len(frames), c.nv))
    for e in range(c.N):
        k = kinematics(c.blob, c.gc[e])
        for f, (body, off) in enumerate(frames):
            Jl, Jr = jacobians(c.blob, k, body, k.p[body] + k.R[body] @ np.asarray(off, float))
            J[e, kk * f:kk * f + 3] = Jl
            if angular:
                J[e, kk * f + 3:kk * f + 6] = Jr
    return J


@functools.lru_cache(maxsize=None)
def delassus_reference(name, key, angular, with_diag):
    """(G_ref [N, kF, kF], JMinv_ref [N, kF, nv])"""
    J, Ai = stacked_jacobian(name, key, angular), inverse_reference(name, with_diag)
    JM = np.einsum("eki,eij->ekj", J, Ai)
    return np.einsum("eki,eli->ekl", JM, J), JM


# ------------------------------------------------------------------------------------------------------------------------------ error measures
def x_error(X, X_ref):
    """per env: max|X - X_ref| / (1 + max|X_ref|)"""
    X = np.asarray(X, np.float64)
    n = len(X)
    return np.abs(X - X_ref).reshape(n, -1).max(axis=1) / (1 + np.abs(X_ref).reshape(n, -1).max(axis=1))


def rel_error(G, G_ref):
    """per env: max|G - G_ref| / max|G_ref| (G and JMinv)"""
    G = np.asarray(G, np.float64)
    n = len(G)
    return np.abs(G - G_ref).reshape(n, -1).max(axis=1) / np.abs(G_ref).reshape(n, -1).max(axis=1)


def residual_ratio(A, X, B, j0):
    """The conditioning-free bar of a solve, per env: max over the columns of |A x - b|_inf / (2e-5 (1 + S)), S the largest row of |A||x| + |b| - the
    project's inverse-dynamics bar.  A [N, nv, nv], X and B [N, R, nv]; the joint block from j0 on."""
    A, X, B = A[:, j0:, j0:], np.asarray(X, np.float64)[:, :, j0:], B[:, :, j0:]
    res = np.abs(np.einsum("eij,erj->eri", A, X) - B).max(axis=2)
    S = (np.einsum("eij,erj->eri", np.abs(A), np.abs(X)) + np.abs(B)).max(axis=2)
    return (res / (2e-5 * (1 + S))).max(axis=1)


def product_ratio(G, J, JMinv):
    """per env: max|G - J JMinv^T| / (2e-5 (1 + S)), S the largest entry of |J||JMinv|^T (the sum of the absolute terms of an entry), in fp64"""
    G, JM = np.asarray(G, np.float64), np.asarray(JMinv, np.float64)
    n = len(G)
    res = np.abs(G - np.einsum("eki,eli->ekl", J, JM)).reshape(n, -1).max(axis=1)
    S = np.einsum("eki,eli->ekl", np.abs(J), np.abs(JM)).reshape(n, -1).max(axis=1)
    return res / (2e-5 * (1 + S))
