"""The fp64 references of the inverse-mass queries (tests/inverse_mass_reference.py), CPU tier: each is pinned a second way before any device is
compared with it.
  X_ref       M^-1 b = Oracle.aba(q, 0, b) - Oracle.aba(q, 0, 0) on the floating bases (the oracle's articulated-body algorithm shares nothing with
              solve(Oracle.mass_matrix, b)); A X_ref = B to rounding; with joint_diag the Woodbury identity against the plain inverse.
  G_ref       symmetric, positive semidefinite, rank <= nv; JMinv_ref A = J_ref; for a single free body G of a point in closed form,
              I / m - [r]x I_w^-1 [r]x, r from the centre of mass, and G of its angular rows I_w^-1.
  the restatement of the kernel's algorithm (tools/inverse_mass_restatement.py) agrees with the references in float64 on a few envs of every case."""
import os
import sys

import numpy as np
import pytest

from common import ROOT, f32
from test_dynamics_reference import dyn_case, jacobians, kinematics, quat_to_rot
import inverse_mass_reference as ref


@pytest.mark.parametrize("name", ref.CASES)
def test_solve_reference_against_the_oracles_aba(built_lib, name):
    c = dyn_case(name)
    B, X = ref.rhs(name, "r5"), ref.solve_reference(name, "r5", False)
    A = ref.system(name, False)
    assert ref.residual_ratio(A, X, B, c.j0).max() <= 1e-6      # (a bar of 2e-5: the fp64 solve sits seven orders below it)
    if c.fixed:
        assert not X[:, :, :6].any()
        return
    zero = np.zeros(c.nv)
    worst = 0.0
    for e in range(0, c.N, 4):
        a0 = c.o.aba(c.gc[e], zero, zero)
        for r in range(B.shape[1]):
            got = c.o.aba(c.gc[e], zero, B[e, r]) - a0
            worst = max(worst, np.abs(got - X[e, r]).max() / (1 + np.abs(X[e, r]).max()))
    print(f"{name}: solve(M, b) vs aba(q, 0, b) - aba(q, 0, 0): {worst:.2e}")
    assert worst <= 1e-8, (name, worst)


@pytest.mark.parametrize("name", ref.CASES)
def test_joint_diag_reference(built_lib, name):
    """(M + D)^-1 = M^-1 - M^-1 (D^-1 + M^-1)^-1 M^-1 on the joints D acts on; D is zero on the base, positive on every joint, below 0.5"""
    c, d = dyn_case(name), ref.joint_diag(name)
    assert not d[:6].any() and (d[6:] > 0).all() and (d[6:] < 0.5).all() and np.array_equal(d, f32(d))
    Mi, Ai = ref.inverse_reference(name, False), ref.inverse_reference(name, True)
    for e in range(0, c.N, 8):
        Mjj = Mi[e][6:, 6:]
        want = Mi[e] - Mi[e][:, 6:] @ np.linalg.solve(np.diag(1.0 / d[6:]) + Mjj, Mi[e][6:, :])
        assert np.abs(want - Ai[e]).max() <= 1e-9 * (1 + np.abs(Ai[e]).max()), (name, e)
    assert not np.array_equal(ref.solve_reference(name, "r5", True), ref.solve_reference(name, "r5", False))
    assert np.array_equal(ref.rhs(name, "r1"), ref.rhs(name, "r5")[:, :1]) and ref.rhs(name, "r5").shape == (c.N, 5, c.nv)


@pytest.mark.parametrize("name", ref.CASES)
def test_delassus_reference_properties(built_lib, name):
    c = dyn_case(name)
    for key, angular, with_diag in ref.delassus_variants(name):
        G, JM = ref.delassus_reference(name, key, angular, with_diag)
        J, A = ref.stacked_jacobian(name, key, angular), ref.system(name, with_diag)
        k = (6 if angular else 3) * len(ref.frame_sets(name)[key])
        assert G.shape == (c.N, k, k) and JM.shape == (c.N, k, c.nv)
        scale = np.abs(G).reshape(c.N, -1).max(axis=1)
        assert (np.abs(G - G.transpose(0, 2, 1)).reshape(c.N, -1).max(axis=1) <= 1e-12 * scale).all(), (name, key)
        ev = np.linalg.eigvalsh(0.5 * (G + G.transpose(0, 2, 1)))
        assert (ev.min(axis=1) >= -1e-10 * scale).all(), (name, key, ev.min())
        assert ((ev > 1e-9 * scale[:, None]).sum(axis=1) <= c.nv - c.j0).all(), (name, key)
        assert ref.residual_ratio(A, JM, J, c.j0).max() <= 1e-6, (name, key)
        if c.fixed:
            assert not JM[:, :, :6].any()
    if name == "floating0":
        assert ref.delassus_reference(name, "sixteen", True, False)[0].shape[1] == 96 > c.nv
    if name == "anymal":
        feet = ref.frame_sets(name)["feet"]
        assert len(feet) == 4 and len({b for b, _ in feet}) == 4
    three = ref.frame_sets(name)["three"]
    assert three[0][0] == three[1][0] and (three[2][0] != three[0][0] or c.nb == 2)      # (floating0 has two bodies: nb - 1 == nb // 2)
    anc = ref.frame_sets(name)["ancestor"]
    assert anc[1][0] == c.blob.parent[anc[0][0]]


def test_free_body_closed_form(built_lib):
    """one free body: G of the point at r from the centre of mass is I / m - [r]x I_w^-1 [r]x, its angular block I_w^-1, the coupling -[r]x I_w^-1 -
    from jacobians() and Oracle.mass_matrix as the references above are built"""
    from raisimlib_amd import Model
    from common import Oracle
    model = Model(urdf_string=ref.BOX_URDF)
    blob = model.blob
    o = Oracle(blob)
    rng = np.random.default_rng(5)
    skew = lambda a: np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ii = blob.inertia[0]
    Ib = np.array([[ii[0], ii[1], ii[2]], [ii[1], ii[3], ii[4]], [ii[2], ii[4], ii[5]]])
    for _ in range(8):
        q = np.r_[rng.uniform(-2, 2, 3), rng.normal(size=4)]
        q[3:7] /= np.linalg.norm(q[3:7])
        off = rng.uniform(-0.3, 0.3, 3)
        k = kinematics(blob, q)
        Jl, Jr = jacobians(blob, k, 0, k.p[0] + k.R[0] @ off)
        J = np.vstack([Jl, Jr])
        G = J @ np.linalg.solve(o.mass_matrix(q), J.T)
        R = quat_to_rot(q[3:7])
        Iwi = np.linalg.inv(R @ Ib @ R.T)
        r = R @ (off - np.array(blob.com[0][:]))
        want = np.block([[np.eye(3) / blob.mass[0] - skew(r) @ Iwi @ skew(r), -skew(r) @ Iwi], [Iwi @ skew(r), Iwi]])
        assert np.abs(G - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_agrees_in_float64(built_lib, name):
    """the kernel's algorithm in float64 numpy on three envs of the case, every variant: 1e-10 of the references' own scale (the tool's full run
    reports 1e-15 .. 1e-12)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import inverse_mass_restatement as rs
    c = dyn_case(name)
    envs = (0, c.N // 2, c.N - 1)
    for with_diag in (False, True):
        d = ref.joint_diag(name) if with_diag else np.zeros(c.nv)
        facs = {e: rs.factor(c.blob, c.gc[e], d, np.float64) for e in envs}
        for which, wd in ref.SOLVE_VARIANTS:
            if wd != with_diag or (which == "eye" and c.nv > 20):
                continue
            X = np.array([rs.solve(facs[e], ref.rhs(name, which)[e]) for e in envs])
            assert ref.x_error(X, ref.solve_reference(name, which, with_diag)[list(envs)]).max() <= 1e-10, (name, which)
        for key, angular, wd in ref.delassus_variants(name):
            if wd != with_diag or key == "sixteen":
                continue
            out = [rs.delassus(facs[e], ref.frame_sets(name)[key], angular) for e in envs]
            Gr, JMr = ref.delassus_reference(name, key, angular, with_diag)
            G = np.array([o[0] for o in out])
            assert np.array_equal(G, G.transpose(0, 2, 1))
            assert ref.rel_error(G, Gr[list(envs)]).max() <= 1e-10 and ref.rel_error(np.array([o[1] for o in out]), JMr[list(envs)]).max() <= 1e-10, (name, key)
