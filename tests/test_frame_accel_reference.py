"""The fp64 references of the frame-acceleration queries (rsb_get_frame_accelerations, rsb_get_frame_jacobian_rates, rsb_imu_observe; include/rsb.h),
CPU tier, pinned on every case of test_dynamics_reference.NAMES (14 random trees with prismatic joints, the 40-body tree, both shipped models).

ref_accel() is built from test_dynamics_reference.kinematics (world-frame velocities and classical accelerations of the body origins) and the point
formula  lin_acc = ac_i + alpha_i x o + omega_i x (omega_i x o),  ang_acc = alpha_i,  o = R_i offset.  A twin recursion with every term replaced by its
absolute value gives, per frame and component, the sum of the absolute values of the terms that made up the result (as newton_euler does for its
sums): the scale the device's float32 rounding is measured against, 2e-5 (1 + S) in tests/test_gpu_frame_accel.py.  RSB_ACC_PROPER adds |g|,
RSB_ACC_LOCAL maps the sums through |R^T|.

ref_jacobian_rates() is the column table of rsb.h, with (a_j, p_j, omega_j, v_j) of chain body j and the point (p, v):
    base linear 0 | base angular k: e_k x (v - v_base) | revolute j: (omega_j x a_j) x (p - p_j) + a_j x (v - v_j), omega_j x a_j | prismatic j: omega_j x a_j, 0
and the per-entry sums of absolute terms (a difference counts as its two terms), reduced to one S per frame and matrix by the maximum.

Pins: the analytic rates against central differences of `jacobians` along config_add(q, +-h u) and, a second time, of Oracle.point_jacobian (the
oracle shares no code with the numpy recursion); the identity acc = J udot + Jdot u; closed forms (rest, a spinning free body, a pendulum)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from common import PENDULUM_URDF, Oracle, config_add, f32, sphere_urdf
from test_dynamics_reference import NAMES, dyn_case, jacobians, kinematics

H = 1e-5       # central-difference step along u
FD_BAR = 1e-7  # |analytic - difference| <= FD_BAR (1 + max|ref|): the difference's own truncation error is ~1e-9 at H


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def _ac(a, b):
    """sum of the absolute values of the terms of a x b, b given by ITS sum of absolute terms"""
    return np.abs(_skew(a)) @ np.abs(b)


def offset_frames(c):
    """the case's frames for the CPU pins: every body origin + its three offset frames (offsets as float32 holds them)"""
    return [(i, np.zeros(3)) for i in range(c.nb)] + [(int(b), f32(off)) for b, off in c.frames]


def abs_accelerations(blob, k, u, udot):
    """the twin of kinematics' acceleration recursion: per body the sums of the absolute values of the terms of alpha_i and ac_i"""
    u = np.asarray(u, float)
    ud = np.zeros(blob.nv) if udot is None else np.asarray(udot, float)
    moves = not blob.fixed_base
    sal, sac = [np.abs(ud[3:6]) * moves], [np.abs(ud[0:3]) * moves]
    for i in range(1, blob.nb):
        par = blob.parent[i]
        wp, a, d = k.w[par], k.a[i], k.p[i] - k.p[par]
        qd, qdd = u[5 + i], ud[5 + i]
        centripetal = np.abs(_skew(wp)) @ (np.abs(_skew(wp)) @ np.abs(d))
        if blob.jtype[i] == 1:
            sal.append(sal[par] + np.abs(a * qdd) + _ac(wp, a) * abs(qd))
            sac.append(sac[par] + _ac(d, sal[par]) + centripetal)
        else:
            sal.append(sal[par])
            sac.append(sac[par] + _ac(d, sal[par]) + centripetal + 2 * _ac(wp, a) * abs(qd) + np.abs(a * qdd))
    return sal, sac


def ref_accel(blob, q, u, udot, frames, gravity=(0.0, 0.0, 0.0), local=False, proper=False):
    """-> namespace of lin, ang [F, 3] (world frame; local: R^T x; proper: lin - gravity), s_lin, s_ang [F, 3] (the sums of absolute terms of each
    component), R [F, 3, 3] and w [F, 3] (the body's rotation and world angular velocity: the gyro reads R^T w)"""
    k = kinematics(blob, q, u, udot)
    sal, sac = abs_accelerations(blob, k, u, udot)
    F = len(frames)
    r = SimpleNamespace(lin=np.zeros((F, 3)), ang=np.zeros((F, 3)), s_lin=np.zeros((F, 3)), s_ang=np.zeros((F, 3)), R=np.zeros((F, 3, 3)), w=np.zeros((F, 3)))
    for n, (body, off) in enumerate(frames):
        R, w, al, ac = k.R[body], k.w[body], k.al[body], k.ac[body]
        o = R @ np.asarray(off, float)
        r.lin[n] = ac + np.cross(al, o) + np.cross(w, np.cross(w, o))
        r.s_lin[n] = sac[body] + _ac(o, sal[body]) + np.abs(_skew(w)) @ (np.abs(_skew(w)) @ np.abs(o))
        r.ang[n], r.s_ang[n], r.R[n], r.w[n] = al, sal[body], R, w
    return with_flags(r, gravity, local, proper)


def with_flags(r, gravity, local, proper):
    """a world-frame, classical result of ref_accel under RSB_ACC_PROPER (lin - g, the sums + |g|) and RSB_ACC_LOCAL (R^T x, the sums through |R^T|)"""
    lin, s_lin, ang, s_ang = r.lin, r.s_lin, r.ang, r.s_ang
    if proper:
        g = np.asarray(gravity, float)
        lin, s_lin = lin - g, s_lin + np.abs(g)
    if local:
        Rt = np.swapaxes(r.R, 1, 2)
        lin, s_lin = np.einsum("fij,fj->fi", Rt, lin), np.einsum("fij,fj->fi", np.abs(Rt), s_lin)
        ang, s_ang = np.einsum("fij,fj->fi", Rt, ang), np.einsum("fij,fj->fi", np.abs(Rt), s_ang)
    return SimpleNamespace(lin=lin, ang=ang, s_lin=s_lin, s_ang=s_ang, R=r.R, w=r.w)


def ref_jacobian_rates(blob, q, u, frames):
    """-> Jdot_lin, Jdot_rot [F, 3, nv] along u, and S_lin, S_rot [F]: the largest per-entry sum of absolute terms of each matrix"""
    k = kinematics(blob, q, u)
    F, nv = len(frames), blob.nv
    Jl, Jr, Sl, Sr = np.zeros((F, 3, nv)), np.zeros((F, 3, nv)), np.zeros((F, 3, nv)), np.zeros((F, 3, nv))
    for n, (body, off) in enumerate(frames):
        o = k.R[body] @ np.asarray(off, float)
        p, v = k.p[body] + o, k.v[body] + np.cross(k.w[body], o)
        if not blob.fixed_base:
            for c in range(3):
                e = np.eye(3)[c]
                Jl[n, :, 3 + c] = np.cross(e, v - k.v[0])
                Sl[n, :, 3 + c] = _ac(e, np.abs(v) + np.abs(k.v[0]))
        j = body
        while j >= 1:
            a, wa = k.a[j], np.cross(k.w[j], k.a[j])
            s_wa = _ac(k.w[j], a)
            if blob.jtype[j] == 1:
                Jl[n, :, 5 + j] = np.cross(wa, p - k.p[j]) + np.cross(a, v - k.v[j])
                Sl[n, :, 5 + j] = _ac(wa, np.abs(p) + np.abs(k.p[j])) + _ac(a, np.abs(v) + np.abs(k.v[j]))
                Jr[n, :, 5 + j], Sr[n, :, 5 + j] = wa, s_wa
            else:
                Jl[n, :, 5 + j], Sl[n, :, 5 + j] = wa, s_wa
            j = blob.parent[j]
    return Jl, Jr, Sl.max(axis=(1, 2)), Sr.max(axis=(1, 2))


def ref_jacobians(blob, q, frames):
    """J_lin, J_rot [F, 3, nv] of test_dynamics_reference.jacobians"""
    k = kinematics(blob, q)
    out = [jacobians(blob, k, body, k.p[body] + k.R[body] @ np.asarray(off, float)) for body, off in frames]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def masked_u(c, x):
    x = np.array(x, float)
    if c.fixed:
        x[:6] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def rates_of(name, n_env=8):
    """ref_jacobian_rates of the first envs of a case on its CPU frames (shared by the pins)"""
    c = dyn_case(name)
    fr = offset_frames(c)
    return fr, [ref_jacobian_rates(c.blob, c.gc[e], c.gv[e], fr) for e in range(n_env)]


# ------------------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", NAMES)
def test_jacobian_rates_against_central_differences_of_the_numpy_jacobians(built_lib, name):
    """pin 1: analytic Jdot_lin, Jdot_rot against (J(q (+) h u) - J(q (-) h u)) / 2h of `jacobians`, h = 1e-5: <= 1e-7 (1 + max|ref|)"""
    c = dyn_case(name)
    fr, rates = rates_of(name)
    worst = 0.0
    for e in range(8):
        u = masked_u(c, c.gv[e])
        Jlp, Jrp = ref_jacobians(c.blob, config_add(c.gc[e], H * u, c.fixed), fr)
        Jlm, Jrm = ref_jacobians(c.blob, config_add(c.gc[e], -H * u, c.fixed), fr)
        for got, want in ((rates[e][0], (Jlp - Jlm) / (2 * H)), (rates[e][1], (Jrp - Jrm) / (2 * H))):
            err = np.abs(got - want).max() / (1 + np.abs(want).max())
            worst = max(worst, err)
            assert err <= FD_BAR, (name, e, err)
    print(f"{name}: analytic Jdot vs central differences of jacobians, worst {worst:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_jacobian_rates_against_central_differences_of_the_oracle(built_lib, name):
    """pin 2: Jdot_lin against central differences of Oracle.point_jacobian, same bar (a fixed base's six columns come back from the oracle as if it
    floated: they are not part of this ABI's matrix and are left out)"""
    c = dyn_case(name)
    fr, rates = rates_of(name)
    worst = 0.0
    for e in range(8):
        u = masked_u(c, c.gv[e])
        qp, qm = config_add(c.gc[e], H * u, c.fixed), config_add(c.gc[e], -H * u, c.fixed)
        for n, (body, off) in enumerate(fr):
            want = (c.o.point_jacobian(qp, body, off)[1] - c.o.point_jacobian(qm, body, off)[1]) / (2 * H)
            err = np.abs(rates[e][0][n] - want)[:, c.j0:].max() / (1 + np.abs(want[:, c.j0:]).max())
            worst = max(worst, err)
            assert err <= FD_BAR, (name, e, n, err)
    print(f"{name}: analytic Jdot_lin vs central differences of the oracle, worst {worst:.2e}")


@pytest.mark.parametrize("name", NAMES)
def test_acceleration_is_J_udot_plus_Jdot_u(built_lib, name):
    """pin 3: ref lin_acc = J_lin udot + Jdot_lin u and ref ang_acc = J_rot udot + Jdot_rot u, <= 1e-9 (1 + S)"""
    c = dyn_case(name)
    fr, rates = rates_of(name)
    for e in range(8):
        u, ud = masked_u(c, c.gv[e]), masked_u(c, c.udot[e])
        r = ref_accel(c.blob, c.gc[e], c.gv[e], c.udot[e], fr)
        Jl, Jr = ref_jacobians(c.blob, c.gc[e], fr)
        lin, ang = Jl @ ud + rates[e][0] @ u, Jr @ ud + rates[e][1] @ u
        assert (np.abs(r.lin - lin).max(axis=1) <= 1e-9 * (1 + r.s_lin.max(axis=1))).all(), (name, e)
        assert (np.abs(r.ang - ang).max(axis=1) <= 1e-9 * (1 + r.s_ang.max(axis=1))).all(), (name, e)
        bias = ref_accel(c.blob, c.gc[e], c.gv[e], None, fr)
        assert (np.abs(bias.lin - rates[e][0] @ u).max(axis=1) <= 1e-9 * (1 + bias.s_lin.max(axis=1))).all(), (name, e)


@pytest.mark.parametrize("name", NAMES)
def test_at_rest_an_accelerometer_reads_minus_gravity(built_lib, name):
    """closed form: u = udot = 0 with PROPER | LOCAL gives -R^T g at every frame"""
    c = dyn_case(name)
    fr = offset_frames(c)
    g = np.asarray(c.gravity)
    for e in range(8):
        r = ref_accel(c.blob, c.gc[e], np.zeros(c.nv), np.zeros(c.nv), fr, gravity=c.gravity, local=True, proper=True)
        for n in range(len(fr)):
            assert np.abs(r.lin[n] + r.R[n].T @ g).max() <= 1e-12 and not r.ang[n].any()
            assert np.allclose(r.s_lin[n], np.abs(r.R[n].T) @ np.abs(g))


def sphere_case():
    """the single free body of sphere_urdf spinning: (model, q, u, frames, omega)"""
    from raisimlib_amd import Model
    model = Model(urdf_string=sphere_urdf(2.0, 0.1))
    rng = np.random.default_rng(5)
    qt = rng.normal(size=4)
    q = f32(np.r_[0.3, -0.2, 1.0, qt / np.linalg.norm(qt)])
    w = f32([1.5, -2.0, 0.7])
    u = np.r_[0.0, 0.0, 0.0, w]
    return model, q, u, [(0, f32((0.05, -0.02, 0.1))), (0, f32((0.0, 0.1, 0.0)))], w


def pendulum_case(L=0.7, angle=0.4, qd=1.3, qdd=-2.1):
    """PENDULUM_URDF at rest but for its hinge: (model, q, u, udot, frames, L, qd, qdd)"""
    from raisimlib_amd import Model
    model = Model(urdf_string=PENDULUM_URDF.format(l=L, m=1.0))
    q = f32([0, 0, 0, 1, 0, 0, 0, angle])
    u, ud = np.zeros(7), np.zeros(7)
    u[6], ud[6] = f32(qd), f32(qdd)
    return model, q, u, ud, [(1, f32((0.0, 0.0, -L)))], float(f32(L)), float(f32(qd)), float(f32(qdd))


def test_a_spinning_free_body(built_lib):
    """closed form: the free body of sphere_urdf spinning at omega about its resting origin: lin_acc = omega x (omega x o), ang_acc = 0"""
    model, q, u, fr, w = sphere_case()
    r = ref_accel(model.blob, q, u, None, fr)
    for n, (_, off) in enumerate(fr):
        o = r.R[n] @ off
        assert np.abs(r.lin[n] - np.cross(w, np.cross(w, o))).max() <= 1e-14 and not r.ang[n].any()
    Jl, Jr, _, _ = ref_jacobian_rates(model.blob, q, u, fr)
    assert np.abs(Jl @ u - r.lin).max() <= 1e-14 and not Jr.any()


def test_a_pendulum(built_lib):
    """closed form: the bob of PENDULUM_URDF: lin_acc = qdd L t - qd^2 L r, r the unit vector hinge -> bob, t = axis x r"""
    model, q, u, ud, fr, L, qd, qdd = pendulum_case()
    r = ref_accel(model.blob, q, u, ud, fr)
    rhat = r.R[0] @ np.array([0.0, 0.0, -1.0])
    that = np.cross([0.0, 1.0, 0.0], rhat)
    assert np.abs(r.lin[0] - (qdd * L * that - qd * qd * L * rhat)).max() <= 1e-14
    assert np.abs(r.ang[0] - np.array([0.0, qdd, 0.0])).max() <= 1e-14
