"""The fp64 references of the dynamics queries (rsb_inverse_dynamics, rsb_forward_dynamics; include/rsb.h), CPU tier, and the cases every dynamics
test shares.

newton_euler() is the reference for the joint reaction wrenches: the textbook world-frame Newton-Euler recursion in numpy - velocities and classical
accelerations of the body origins down the tree, each body's net force and its moment about ITS OWN joint origin, then the backward recursion
F_p += F_i, N_p += N_i + (p_i - p_p) x F_i.  It is a second formulation next to the oracle's common-frame spatial RNEA (oracle/rsb_oracle.c), shares no
code with it, and is pinned against it here on every case: its tau against Oracle.inverse_dynamics to 1e-9 of its own scale, with the loads taken off
through Oracle.point_jacobian (a torque as a force couple).  Besides tau, joint_force and joint_torque it returns, for each of them, the sum of the
absolute values of the terms it added: the scale the device's rounding is measured against (2e-5 (1 + scale), tests/test_gpu_dynamics.py).

Cases: test_gpu_slow_path.case's 8 floating and 6 fixed random trees (2 - 17 links, prismatic joints, rotor inertia, tilted gravity, N = 67), its
40-body tree, and the two shipped models at N = 64.  udot, tau and the loads are N(0, 1) rounded to float32; a fixed base's six rows hold noise.  Three
loads: two on one body (force + torque, force only), one torque-only on another.

The forward-dynamics yardstick E32(case) - the error of a float32 Cholesky solve of the oracle's own system - is computed and printed here."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg

from common import Oracle, f32, standing_states
from test_gpu_slow_path import CASES, case

NAMES = [f"{k}{i}" for k, i in CASES] + ["tree40", "anymal", "atlas"]


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def _abs_cross(a, b):
    """sum of the absolute values of the terms of a x b, b given by ITS sum of absolute terms"""
    return np.abs(_skew(a)) @ np.abs(b)


def quat_to_rot(qt):
    w, x, y, z = np.asarray(qt, float) / np.linalg.norm(qt)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _rot_axis(a, q):
    return np.cos(q) * np.eye(3) + (1 - np.cos(q)) * np.outer(a, a) + np.sin(q) * _skew(a)


def kinematics(blob, q, u=None, udot=None):
    """World transforms, joint axes, velocities and classical accelerations of every body's origin.  A fixed base neither moves nor accelerates."""
    nb = blob.nb
    z = np.zeros(3)
    u = np.zeros(blob.nv) if u is None else np.asarray(u, float)
    ud = np.zeros(blob.nv) if udot is None else np.asarray(udot, float)
    moves = not blob.fixed_base
    k = SimpleNamespace(R=[quat_to_rot(q[3:7])], p=[np.array(q[:3], float)], a=[z], w=[u[3:6] * moves], v=[u[0:3] * moves], al=[ud[3:6] * moves], ac=[ud[0:3] * moves])
    for i in range(1, nb):
        par = blob.parent[i]
        ax, Rt, pt = np.array(blob.axis[i][:]), np.array(blob.rtree[i][:]).reshape(3, 3), np.array(blob.ptree[i][:])
        wp, vp, alp, acp = k.w[par], k.v[par], k.al[par], k.ac[par]
        qi, qd, qdd = q[6 + i], u[5 + i], ud[5 + i]
        if blob.jtype[i] == 1:
            R = k.R[par] @ Rt @ _rot_axis(ax, qi)
            a, d = R @ ax, k.R[par] @ pt
            k.w.append(wp + a * qd); k.al.append(alp + a * qdd + np.cross(wp, a) * qd)
            k.v.append(vp + np.cross(wp, d)); k.ac.append(acp + np.cross(alp, d) + np.cross(wp, np.cross(wp, d)))
        else:
            R = k.R[par] @ Rt
            a = R @ ax
            d = k.R[par] @ pt + a * qi
            k.w.append(wp); k.al.append(alp)
            k.v.append(vp + np.cross(wp, d) + a * qd)
            k.ac.append(acp + np.cross(alp, d) + np.cross(wp, np.cross(wp, d)) + 2 * np.cross(wp, a) * qd + a * qdd)
        k.R.append(R); k.a.append(a); k.p.append(k.p[par] + d)
    return k


def jacobians(blob, k, body, point, floating=None):
    """J_lin, J_rot [3, nv] of a world point fixed on `body`.  A fixed base keeps its six, zero, columns; floating=True fills them as if it floated:
    J^T w is then the load's share of the wrench that holds the base."""
    Jl, Jr = np.zeros((3, blob.nv)), np.zeros((3, blob.nv))
    if (not blob.fixed_base) if floating is None else floating:
        Jl[:, :3] = np.eye(3); Jl[:, 3:6] = -_skew(point - k.p[0]); Jr[:, 3:6] = np.eye(3)
    j = body
    while j >= 1:
        if blob.jtype[j] == 1:
            Jl[:, 5 + j] = np.cross(k.a[j], point - k.p[j]); Jr[:, 5 + j] = k.a[j]
        else:
            Jl[:, 5 + j] = k.a[j]
        j = blob.parent[j]
    return Jl, Jr


def newton_euler(blob, q, u, udot, gravity, loads=()):
    """loads: (body, world point, world force, world torque).  -> tau [nv], joint_force [nb, 3], joint_torque [nb, 3] (what the parent exerts on
    body i through joint i, the torque about p_i) and the three sums of absolute terms (s_tau [nv]; s_force, s_torque [nb, 3])."""
    nb, g = blob.nb, np.asarray(gravity, float)
    ud = np.zeros(blob.nv) if udot is None else np.asarray(udot, float)
    k = kinematics(blob, q, u, ud)
    F, Nn, SF, SN = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3))
    for i in range(nb):
        m, rc = blob.mass[i], k.R[i] @ np.array(blob.com[i][:])
        ii = blob.inertia[i]
        Iw = k.R[i] @ np.array([[ii[0], ii[1], ii[2]], [ii[1], ii[3], ii[4]], [ii[2], ii[4], ii[5]]]) @ k.R[i].T
        acom = k.ac[i] + np.cross(k.al[i], rc) + np.cross(k.w[i], np.cross(k.w[i], rc))
        F[i] = m * acom - m * g
        SF[i] = np.abs(m * acom) + np.abs(m * g)
        Nn[i] = Iw @ k.al[i] + np.cross(k.w[i], Iw @ k.w[i]) + np.cross(rc, m * acom) - np.cross(rc, m * g)
        SN[i] = np.abs(Iw @ k.al[i]) + np.abs(np.cross(k.w[i], Iw @ k.w[i])) + _abs_cross(rc, m * acom) + _abs_cross(rc, m * g)
    for body, point, force, torque in loads:
        F[body] -= force; SF[body] += np.abs(force)
        Nn[body] -= torque + np.cross(point - k.p[body], force)
        SN[body] += np.abs(torque) + _abs_cross(point - k.p[body], force)
    for i in range(nb - 1, 0, -1):
        par, d = blob.parent[i], k.p[i] - k.p[blob.parent[i]]
        F[par] += F[i]; SF[par] += SF[i]
        Nn[par] += Nn[i] + np.cross(d, F[i]); SN[par] += SN[i] + _abs_cross(d, SF[i])
    tau, st = np.zeros(blob.nv), np.zeros(blob.nv)
    tau[0:3], tau[3:6], st[0:3], st[3:6] = F[0], Nn[0], SF[0], SN[0]
    for i in range(1, nb):
        X, SX = (Nn, SN) if blob.jtype[i] == 1 else (F, SF)
        tau[5 + i] = k.a[i] @ X[i] + blob.armature[i] * ud[5 + i]
        st[5 + i] = np.abs(k.a[i]) @ SX[i] + abs(blob.armature[i] * ud[5 + i])
    return tau, F, Nn, st, SF, SN


def load_list(c, k, e):
    """the case's three loads on env e as newton_euler takes them"""
    out = []
    for f, (body, off) in enumerate(c.frames):
        out.append((body, k.p[body] + k.R[body] @ np.asarray(off, float), c.force[e, f], c.torque[e, f]))
    return out


@functools.lru_cache(maxsize=None)
def dyn_case(name):
    """One model with its float32-rounded states and inputs (nobody writes into them); shared by the CPU and GPU dynamics tests."""
    from raisimlib_amd import Model, rsc_path
    if name in ("anymal", "atlas"):
        model = Model(urdf_path=rsc_path(f"{name}_c_like.urdf" if name == "anymal" else "atlas_like.urdf"))
        n, gravity = 64, (0.0, 0.0, -9.81)
        rng = np.random.default_rng(9100 + len(name))
        if name == "anymal":
            gc, gv = standing_states(n, seed=3)
        else:
            gc = np.zeros((n, model.nq)); gc[:, 0:2] = rng.uniform(-1, 1, (n, 2)); gc[:, 2] = rng.uniform(0.9, 1.4, n)
            qq = rng.normal(size=(n, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
            gc[:, 7:] = rng.uniform(-0.6, 0.6, (n, model.nq - 7))
            gv = rng.normal(size=(n, model.nv))
        gc, gv = f32(gc), f32(gv)
        o = Oracle(model.blob); o.p.gravity[:] = gravity
        M = np.array([o.mass_matrix(q) for q in gc]); h = np.array([o.nonlinearities(q, u) for q, u in zip(gc, gv)])
        fixed = False
    else:
        c0 = case("floating", 1, n_links=40) if name == "tree40" else case(name.rstrip("0123456789"), int(name[-1]))
        model, gc, gv, o, M, h, gravity, fixed, n = c0.model, c0.gc, c0.gv, c0.o, c0.M, c0.h, c0.gravity, c0.fixed, len(c0.gc)
        rng = np.random.default_rng(9000 + c0.rng_seed % 1000)
    nb, nv = model.nb, model.nv
    b1, b2 = nb - 1, nb // 2
    frames = [(b1, (0.05, -0.02, 0.1)), (b1, (-0.1, 0.03, 0.0)), (b2, (0.0, 0.04, -0.06))]
    force, torque = rng.normal(size=(n, 3, 3)), rng.normal(size=(n, 3, 3))
    force[:, 2] = 0.0; torque[:, 1] = 0.0
    return SimpleNamespace(name=name, model=model, blob=model.blob, N=n, nb=nb, nv=nv, fixed=bool(fixed), j0=6 if fixed else 0, gravity=tuple(gravity), gc=gc, gv=gv,
                           o=o, M=M, h=h, udot=f32(rng.normal(size=(n, nv))), tau=f32(rng.normal(size=(n, nv))), frames=frames, force=f32(force), torque=f32(torque))


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """newton_euler over the case's envs.  variant: "h" (udot = None), "udot", "loads" (udot and the three loads), "static" (u = udot = 0).
    -> namespace of arrays tau, jf, jt, s_tau, s_jf, s_jt (leading axis N)"""
    c = dyn_case(name)
    rows = []
    for e in range(c.N):
        u = np.zeros(c.nv) if variant == "static" else c.gv[e]
        ud = c.udot[e] if variant in ("udot", "loads") else None
        loads = load_list(c, kinematics(c.blob, c.gc[e]), e) if variant == "loads" else ()
        rows.append(newton_euler(c.blob, c.gc[e], u, ud, c.gravity, loads))
    return SimpleNamespace(**{n: np.array([r[i] for r in rows]) for i, n in enumerate(("tau", "jf", "jt", "s_tau", "s_jf", "s_jt"))})


def masked(c, x):
    """a fixed base's six rows as the oracle has to see them: zero"""
    x = np.array(x, float)
    if c.fixed:
        x[..., :6] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def load_jacobians(name):
    """per env: sum_f J_lin^T force + J_rot^T torque [N, nv], sum |J^T||w| [N, nv] of the case's loads, and the first with a fixed base's six columns
    filled as a floating base's"""
    c = dyn_case(name)
    gen, mag, full = np.zeros((c.N, c.nv)), np.zeros((c.N, c.nv)), np.zeros((c.N, c.nv))
    for e in range(c.N):
        k = kinematics(c.blob, c.gc[e])
        for body, point, force, torque in load_list(c, k, e):
            Jl, Jr = jacobians(c.blob, k, body, point)
            gen[e] += Jl.T @ force + Jr.T @ torque
            mag[e] += np.abs(Jl.T) @ np.abs(force) + np.abs(Jr.T) @ np.abs(torque)
            Jl, Jr = jacobians(c.blob, k, body, point, floating=True)
            full[e] += Jl.T @ force + Jr.T @ torque
    return gen, mag, full


def tau_scale(name, variant):
    """S_e of the inverse-dynamics bar: the env's largest row of |M||udot| + |h| + sum |J^T||w| (joint block of a fixed base for M)"""
    c = dyn_case(name)
    ud = masked(c, c.udot) if variant in ("udot", "loads") else np.zeros((c.N, c.nv))
    rows = np.einsum("eij,ej->ei", np.abs(c.M), np.abs(ud)) + np.abs(c.h)
    if variant == "loads":
        rows = rows + load_jacobians(name)[1]
    return rows.max(axis=1)


@functools.lru_cache(maxsize=None)
def forward_reference(name, with_loads=True):
    """udot_ref [N, nv] = solve(M_ref, tau - h_ref + J^T w) in fp64 (joint block for a fixed base, base rows zero), the same by a float32 Cholesky of
    f32(M_ref) on a float32 right-hand side, and E32 = max_e |udot_32 - udot_ref| / (1 + max|udot_ref|)."""
    c = dyn_case(name)
    rhs = c.tau - c.h + (load_jacobians(name)[0] if with_loads else 0.0)
    ref, low = np.zeros((c.N, c.nv)), np.zeros((c.N, c.nv))
    j0 = c.j0
    for e in range(c.N):
        Mr, r = c.M[e][j0:, j0:], rhs[e][j0:]
        ref[e, j0:] = np.linalg.solve(Mr, r)
        L = np.linalg.cholesky(Mr.astype(np.float32))
        low[e, j0:] = scipy.linalg.cho_solve((L, True), r.astype(np.float32))
        assert low.dtype == np.float64 and L.dtype == np.float32
    e32 = max(np.abs(low[e] - ref[e]).max() / (1 + np.abs(ref[e]).max()) for e in range(c.N))
    return SimpleNamespace(udot=ref, udot32=low, E32=float(e32), rhs=rhs)


# ------------------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", NAMES)
def test_newton_euler_tau_matches_the_oracle(built_lib, name):
    """tau of newton_euler against Oracle.inverse_dynamics, every env, <= 1e-9 of the row's own scale: with udot = 0 (= the oracle's h), with udot, and
    with the three loads, whose generalized forces are taken off the oracle's tau through Oracle.point_jacobian - a torque t as the couple of
    +-(t x d) / |d|^2 at +-d / 2 about the frame's point, d perpendicular to t."""
    c = dyn_case(name)
    worst = 0.0
    for variant in ("h", "udot", "loads"):
        r = reference(name, variant)
        for e in range(c.N):
            q, u = c.gc[e], masked(c, c.gv[e])
            ud = masked(c, c.udot[e]) if variant != "h" else np.zeros(c.nv)
            want = c.o.inverse_dynamics(q, u, ud)
            if variant == "h":
                assert np.abs(want - c.h[e])[c.j0:].max() <= 1e-9 * (1 + np.abs(c.h[e]).max())
            if variant == "loads":      # (a fixed base's six columns come back as if it floated: J^T w is then the share of the holding wrench)
                k = kinematics(c.blob, q)
                for f, (body, off) in enumerate(c.frames):
                    off = np.asarray(off, float)
                    _, J = c.o.point_jacobian(q, body, off)
                    want = want - J.T @ c.force[e, f]
                    t = c.torque[e, f]
                    if np.abs(t).max() > 0:
                        d = np.cross(t, [1.0, 0.3, -0.2]); d *= 0.2 / np.linalg.norm(d)
                        fc = np.cross(t, d) / (d @ d)
                        for sgn in (1.0, -1.0):
                            _, J = c.o.point_jacobian(q, body, off + sgn * 0.5 * (k.R[body].T @ d))
                            want = want - sgn * (J.T @ fc)
            err = np.abs(r.tau[e] - want) / (1e-12 + r.s_tau[e])
            worst = max(worst, err.max())
            assert err.max() <= 1e-9, (name, variant, e, err.max())
    print(f"{name}: newton_euler tau vs oracle, worst error / scale {worst:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_joint_wrench_identities_and_static_closed_form(built_lib, name):
    """The identities of rsb.h on the reference: a_i . joint_torque_i (revolute) / a_i . joint_force_i (prismatic) + armature_i udot_i = tau_i, the
    base rows of tau are (joint_force_0, joint_torque_0); and at rest (u = udot = 0) joint_force_i = -(subtree mass) g,
    joint_torque_i = -sum_k m_k (c_k - p_i) x g over the subtree."""
    c = dyn_case(name)
    r = reference(name, "loads")
    blob = c.blob
    for e in range(c.N):
        k = kinematics(blob, c.gc[e])
        assert np.array_equal(r.tau[e, :3], r.jf[e, 0]) and np.array_equal(r.tau[e, 3:6], r.jt[e, 0])
        for i in range(1, c.nb):
            X = r.jt if blob.jtype[i] == 1 else r.jf
            assert abs(k.a[i] @ X[e, i] + blob.armature[i] * masked(c, c.udot[e])[5 + i] - r.tau[e, 5 + i]) <= 1e-12 * (1 + r.s_tau[e, 5 + i])
    s = reference(name, "static")
    g = np.asarray(c.gravity)
    for e in range(0, c.N, 8):
        k = kinematics(blob, c.gc[e])
        com = [k.p[i] + k.R[i] @ np.array(blob.com[i][:]) for i in range(c.nb)]
        for i in range(c.nb):
            sub = [j for j in range(i, c.nb) if i in _ancestors(blob, j)]
            f = -sum(blob.mass[j] for j in sub) * g
            t = -sum(blob.mass[j] * np.cross(com[j] - k.p[i], g) for j in sub)
            assert np.abs(s.jf[e, i] - f).max() <= 1e-9 * (1 + s.s_jf[e, i].max()) and np.abs(s.jt[e, i] - t).max() <= 1e-9 * (1 + s.s_jt[e, i].max()), (name, e, i)


def _ancestors(blob, j):
    out = set()
    while j >= 0:
        out.add(j)
        j = blob.parent[j] if j > 0 else -1
    return out


def test_forward_dynamics_yardstick(built_lib):
    """udot_ref and E32 of every case (forward_reference), with the three loads.  Oracle.aba agrees with udot_ref to 1e-8 relative on the floating
    bases; E32 is finite and below 1e-2 everywhere: the systems are well enough conditioned to test a float32 solve with.  The printed table is the
    yardstick of tests/test_gpu_dynamics.py::test_forward_dynamics."""
    print()
    for name in NAMES:
        c, fr = dyn_case(name), forward_reference(name)
        if not c.fixed:
            for e in range(c.N):
                a = c.o.aba(c.gc[e], c.gv[e], fr.rhs[e] + c.h[e])
                assert np.abs(a - fr.udot[e]).max() <= 1e-8 * (1 + np.abs(fr.udot[e]).max()), (name, e)
        cond = max(np.linalg.cond(c.M[e][c.j0:, c.j0:]) for e in range(c.N))
        print(f"  {name:10s} nv {c.nv:3d}  max cond(M) {cond:9.3e}  max|udot_ref| {np.abs(fr.udot).max():9.3e}  E32 {fr.E32:.3e}")
        assert np.isfinite(fr.E32) and fr.E32 < 1e-2, (name, fr.E32)
