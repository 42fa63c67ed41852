"""The fp64 reference of the dynamics derivatives (rsb_inverse_dynamics_derivatives, rsb_forward_dynamics_derivatives; include/rsb.h), CPU tier.

tangent_newton_euler() is test_dynamics_reference.newton_euler restated in forward mode: every quantity of the world-frame Newton-Euler recursion
carries, next to its value, its derivative along all 3 nv directions at once (nv tangent coordinates x of gc, nv components of gv, nv of udot), for
all envs of a case in one numpy pass.  It is written in the reference's formulation - moments about each body's OWN joint origin, the backward
recursion N_p += N_i + (p_i - p_p) x F_i - not in the device's (moments about the base origin, subtree sums), and takes a dtype:
    float64   D_ref, the reference, with S, per entry the sum of the absolute values of the terms it added (as newton_euler returns for tau):
              the scale the device's rounding is measured against, |D_dev - D_ref| <= c (1 + S)  (tests/test_gpu_dynamics_derivatives.py);
    float32   D32, the yardstick: Y32(case) = max |D32 - D_ref| / (1 + S), what a float32 evaluation of the same formulas loses.
The retraction (rsb.h): x_j, j < 3 moves the base origin along world axis j; 3 <= j < 6 turns the base about WORLD axis j - 3 (quaternion multiplied
on the left); j >= 6 is joint coordinate j - 6 + 7 of gc.  gv, udot, gravity and a load's world force and torque are held fixed as arrays; a load's
point is fixed on its body.  A fixed base has no base directions: its six columns are zero.

D_ref is pinned here, on the first and the last env of every case, (a) against Richardson-extrapolated central differences (steps h, h / 2) of
newton_euler itself under that retraction, with the loads, and (b) against the same differences through Oracle.inverse_dynamics (other code, no
loads): per entry  |D_ref - D_R| <= |D(h / 2) - D(h)| + 1e-9 (1 + S).  The first term is the difference scheme's own estimate of the O(h^2) error of
D(h), which dominates the error of the extrapolated value; the second is the differences' rounding, eps S / h with h = 1e-3, with margin.  A missing
term or a wrong sign is O(S).  (c) dtau_dudot against Oracle.mass_matrix to 1e-9 of scale on every env."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg

from test_dynamics_reference import NAMES, dyn_case, forward_reference, kinematics, load_list, masked, newton_euler, quat_to_rot

VARIANTS = ("h", "udot", "loads")      # udot = None; udot; udot and the three loads


class Du:
    """value v [N, ...] and tangent t [N, ..., K]"""

    def __init__(self, v, t):
        self.v, self.t = v, t

    def __add__(a, b):
        return Du(a.v + b.v, a.t + b.t)

    def __sub__(a, b):
        return Du(a.v - b.v, a.t - b.t)

    def times(a, c):
        """by a constant"""
        return Du(a.v * c, a.t * c)


def const(v, K):
    return Du(v, np.zeros(v.shape + (K,), v.dtype))


def cross(a, b):
    return Du(np.cross(a.v, b.v), np.cross(a.t, b.v[..., None], axis=1) + np.cross(a.v[..., None], b.t, axis=1))


def mv(A, x):
    return Du(np.einsum("nij,nj->ni", A.v, x.v), np.einsum("nijk,nj->nik", A.t, x.v) + np.einsum("nij,njk->nik", A.v, x.t))


def mm(A, B):
    return Du(np.einsum("nij,njl->nil", A.v, B.v), np.einsum("nijk,njl->nilk", A.t, B.v) + np.einsum("nij,njlk->nilk", A.v, B.t))


def tr(A):
    return Du(A.v.swapaxes(1, 2), A.t.swapaxes(1, 2))


def sv(s, x):
    """scalar s (v [N], t [N, K]) times vector x"""
    return Du(s.v[:, None] * x.v, s.t[:, None, :] * x.v[:, :, None] + s.v[:, None, None] * x.t)


def dot(a, b):
    return Du(np.einsum("ni,ni->n", a.v, b.v), np.einsum("nik,ni->nk", a.t, b.v) + np.einsum("ni,nik->nk", a.v, b.t))


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def _abs_skew(a):
    """|[a]x| for a [N, 3] -> [N, 3, 3]"""
    a = np.abs(a)
    z = np.zeros_like(a[:, 0])
    return np.stack([np.stack([z, a[:, 2], a[:, 1]], 1), np.stack([a[:, 2], z, a[:, 0]], 1), np.stack([a[:, 1], a[:, 0], z], 1)], 1)


def _abs_cross_t(a, S, b, St):
    """the sum of absolute terms of d (a x b): |da| x S_b + |a| x S_db, a a Du, S [N, 3] and St [N, 3, K] the sums of b and of its tangent"""
    def ac(A, B):
        return np.stack([A[:, 2] * B[:, 1] + A[:, 1] * B[:, 2], A[:, 2] * B[:, 0] + A[:, 0] * B[:, 2], A[:, 1] * B[:, 0] + A[:, 0] * B[:, 1]], 1)
    return ac(np.abs(a.t), S[:, :, None]) + ac(np.abs(a.v)[:, :, None], St)


def tangent_newton_euler(blob, q, u, udot, gravity, loads=(), dtype=np.float64, about_base=False):
    """q [N, nq], u [N, nv], udot [N, nv] or None; loads: (body, offset in the body frame, world force [N, 3], world torque [N, 3]).
    -> tau [N, nv], D [N, nv, 3 nv] = (dtau_dq | dtau_dv | dtau_dudot), S [N, nv, 3 nv] the sums of absolute terms of D's entries.
    about_base: the DEVICE's formulation of the same recursion (rsb_dynamics_derivatives.hip) - every moment about the base origin o = p_0, plain
    sums over the subtrees, the joint's torque shifted back, N_i - (p_i - o) x F_i - which in float32 loses what that shift cancels; S then
    describes the terms of the other formulation and is not to be used."""
    f = lambda x: np.asarray(x, np.float64).astype(dtype)
    nb, nv, N, K = blob.nb, blob.nv, len(q), 3 * blob.nv
    q, u = f(q), f(u)
    ud = np.zeros((N, nv), dtype) if udot is None else f(udot)
    g = f(gravity)
    moves = not blob.fixed_base
    one = np.ones(N, dtype)

    def seeded(v, at):
        """v [N] or [N, 3] with unit tangents: at = direction index of (component 0)"""
        d = const(v, K)
        if at is not None:
            if v.ndim == 1:
                d.t[:, at] = 1
            else:
                for k in range(3):
                    d.t[:, k, at + k] = 1
        return d

    R0 = np.stack([quat_to_rot(x) for x in q[:, 3:7]]).astype(dtype)
    R = [const(R0, K)]
    p = [seeded(q[:, :3].copy(), 0 if moves else None)]
    if moves:
        for a in range(3):
            R[0].t[:, :, :, 3 + a] = np.einsum("ij,njl->nil", f(_skew(np.eye(3)[a])), R0)
    zero3 = np.zeros((N, 3), dtype)
    w = [seeded(u[:, 3:6].copy(), nv + 3) if moves else const(zero3, K)]
    al = [seeded(ud[:, 3:6].copy(), 2 * nv + 3) if moves else const(zero3, K)]
    ac = [seeded(ud[:, 0:3].copy(), 2 * nv) if moves else const(zero3, K)]
    ax_w = [const(zero3, K)]
    qdd = [None]
    I3 = np.eye(3, dtype=dtype)
    for i in range(1, nb):
        par = blob.parent[i]
        ax, Rt, pt = f(blob.axis[i][:]), f(blob.rtree[i][:]).reshape(3, 3), f(blob.ptree[i][:])
        axN, ptN, RtN = const(np.tile(ax, (N, 1)), K), const(np.tile(pt, (N, 1)), K), const(np.tile(Rt, (N, 1, 1)), K)
        qi, qd, qa = seeded(q[:, 6 + i].copy(), 5 + i), seeded(u[:, 5 + i].copy(), nv + 5 + i), seeded(ud[:, 5 + i].copy(), 2 * nv + 5 + i)
        wp, alp, acp = w[par], al[par], ac[par]
        if blob.jtype[i] == 1:
            cs, sn = np.cos(qi.v), np.sin(qi.v)
            aa, sk = np.outer(ax, ax), f(_skew(ax))
            Rq = Du(cs[:, None, None] * I3 + (1 - cs)[:, None, None] * aa + sn[:, None, None] * sk,
                    (-sn[:, None, None] * I3 + sn[:, None, None] * aa + cs[:, None, None] * sk)[..., None] * qi.t[:, None, None, :])
            Ri = mm(mm(R[par], RtN), Rq)
            a, d = mv(Ri, axN), mv(R[par], ptN)
            w.append(wp + sv(qd, a))
            al.append(alp + sv(qa, a) + sv(qd, cross(wp, a)))
            ac.append(acp + cross(alp, d) + cross(wp, cross(wp, d)))
        else:
            Ri = mm(R[par], RtN)
            a = mv(Ri, axN)
            d = mv(R[par], ptN) + sv(qi, a)
            w.append(wp)
            al.append(alp)
            ac.append(acp + cross(alp, d) + cross(wp, cross(wp, d)) + sv(qd, cross(wp, a)).times(2) + sv(qa, a))
        R.append(Ri); ax_w.append(a); p.append(p[par] + d); qdd.append(qa)
    F, Nn, SF, SN, SdF, SdN = [], [], [], [], [], []
    for i in range(nb):
        m = dtype(blob.mass[i])
        com = const(np.tile(f(blob.com[i][:]), (N, 1)), K)
        ii = blob.inertia[i]
        Ib = const(np.tile(f([[ii[0], ii[1], ii[2]], [ii[1], ii[3], ii[4]], [ii[2], ii[4], ii[5]]]), (N, 1, 1)), K)
        rc = mv(R[i], com)
        lev = (p[i] - p[0]) + rc if about_base else rc
        Iw = mm(mm(R[i], Ib), tr(R[i]))
        macom = (ac[i] + cross(al[i], rc) + cross(w[i], cross(w[i], rc))).times(m)
        mg = const(np.tile(m * g, (N, 1)), K)
        t1, t2, t3, t4 = mv(Iw, al[i]), cross(w[i], mv(Iw, w[i])), cross(lev, macom), cross(lev, mg)
        F.append(macom - mg)
        Nn.append(t1 + t2 + t3 - t4)
        SF.append(np.abs(macom.v) + np.abs(mg.v))
        SN.append(np.abs(t1.v) + np.abs(t2.v) + np.einsum("nij,nj->ni", _abs_skew(rc.v), np.abs(macom.v)) + np.einsum("nij,nj->ni", _abs_skew(rc.v), np.abs(mg.v)))
        SdF.append(np.abs(macom.t))
        SdN.append(np.abs(t1.t) + np.abs(t2.t) + np.abs(t3.t) + np.abs(t4.t))
    for body, off, force, torque in loads:
        fo, to = const(f(force), K), const(f(torque), K)
        arm = mv(R[body], const(np.tile(f(off), (N, 1)), K))
        if about_base:
            arm = (p[body] - p[0]) + arm
        lever = cross(arm, fo)
        F[body] = F[body] - fo
        Nn[body] = Nn[body] - (to + lever)
        SF[body] = SF[body] + np.abs(fo.v)
        SN[body] = SN[body] + np.abs(to.v) + np.einsum("nij,nj->ni", _abs_skew(arm.v), np.abs(fo.v))
        SdN[body] = SdN[body] + np.abs(lever.t)
    for i in range(nb - 1, 0, -1):
        par = blob.parent[i]
        d = p[i] - p[par]
        SdN[par] = SdN[par] + SdN[i] + _abs_cross_t(d, SF[i], F[i], SdF[i])
        SN[par] = SN[par] + SN[i] + np.einsum("nij,nj->ni", _abs_skew(d.v), SF[i])
        SF[par] = SF[par] + SF[i]; SdF[par] = SdF[par] + SdF[i]
        Nn[par] = Nn[par] + Nn[i] + cross(d, F[i]) if not about_base else Nn[par] + Nn[i]
        F[par] = F[par] + F[i]
    tau, D, S = np.zeros((N, nv), dtype), np.zeros((N, nv, K), dtype), np.zeros((N, nv, K), dtype)
    tau[:, 0:3], tau[:, 3:6], D[:, 0:3], D[:, 3:6], S[:, 0:3], S[:, 3:6] = F[0].v, Nn[0].v, F[0].t, Nn[0].t, SdF[0], SdN[0]
    for i in range(1, nb):
        X, SX, SdX = (Nn[i] - cross(p[i] - p[0], F[i]) if about_base else Nn[i], SN[i], SdN[i]) if blob.jtype[i] == 1 else (F[i], SF[i], SdF[i])
        a, arm = ax_w[i], dtype(blob.armature[i])
        t = dot(a, X)
        tau[:, 5 + i] = t.v + arm * qdd[i].v
        D[:, 5 + i] = t.t + arm * qdd[i].t
        S[:, 5 + i] = np.einsum("nik,ni->nk", np.abs(a.t), SX) + np.einsum("ni,nik->nk", np.abs(a.v), SdX) + np.abs(arm * qdd[i].t)
    del one
    return tau, D, S


def case_loads(c):
    return [(body, off, c.force[:, k], c.torque[:, k]) for k, (body, off) in enumerate(c.frames)]


@functools.lru_cache(maxsize=None)
def derivative_reference(name, variant, dtype_name="float64", at_forward=False, about_base=False):
    """tangent_newton_euler over the case's envs -> namespace tau [N, nv], dq, dv, dudot [N, nv, nv] and their sums of absolute terms s_dq, s_dv, s_dudot.
    variant: "h" (udot = None), "udot", "loads" (udot and the three loads).  at_forward: udot is udot_ref = FD(tau) of forward_reference (with the
    loads for "loads", without for any other variant) - the point the forward-dynamics derivatives are taken at."""
    c = dyn_case(name)
    if at_forward:
        ud = forward_reference(name, variant == "loads").udot
    else:
        ud = c.udot if variant in ("udot", "loads") else None
    tau, D, S = tangent_newton_euler(c.blob, c.gc, c.gv, ud, c.gravity, case_loads(c) if variant == "loads" else (), np.dtype(dtype_name).type, about_base)
    nv = c.nv
    return SimpleNamespace(tau=tau, dq=D[:, :, :nv], dv=D[:, :, nv:2 * nv], dudot=D[:, :, 2 * nv:], s_dq=S[:, :, :nv], s_dv=S[:, :, nv:2 * nv], s_dudot=S[:, :, 2 * nv:])


@functools.lru_cache(maxsize=None)
def y32(name, about_base=False):
    """Y32(case) = max over the variants, matrices, envs and entries of |D32 - D_ref| / (1 + S); about_base: YD32, with D32 in the device's formulation"""
    worst = 0.0
    for variant in VARIANTS:
        r, lo = derivative_reference(name, variant), derivative_reference(name, variant, "float32", about_base=about_base)
        for k in ("dq", "dv", "dudot"):
            worst = max(worst, float((np.abs(getattr(lo, k).astype(np.float64) - getattr(r, k)) / (1 + getattr(r, "s_" + k))).max()))
    return worst


@functools.lru_cache(maxsize=None)
def aba32(name, with_loads):
    """udot [N, nv] of the device's articulated-body algorithm restated in float32 numpy (tools/dynamics_aba_restatement.py): the point a float32
    pipeline takes its forward-dynamics derivatives at"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from dynamics_aba_restatement import aba
    c = dyn_case(name)
    out = np.zeros((c.N, c.nv), np.float32)
    for e in range(c.N):
        loads = load_list(c, kinematics(c.blob, c.gc[e]), e) if with_loads else ()
        out[e] = aba(c.blob, c.gc[e], c.gv[e], c.tau[e], c.gravity, loads, np.float32)
    if c.fixed:
        out[:, :6] = 0
    return out


@functools.lru_cache(maxsize=None)
def forward_derivative_reference(name, variant):
    """X_ref = -solve(M_ref, D_ref at udot_ref) per env (joint block for a fixed base, base rows zero), Minv_ref, and per entry the scale
    |Minv_ref| (1 + S): the right-hand side -D is itself only known to c (1 + S), and X is linear in it, so that is the sum of absolute terms a bar
    of the form c (1 + scale) has to be measured against (for dudot_dtau = Minv_ref the scale is |Minv_ref|).  Two float32 yardsticks, both
    max |X32 - X_ref| / (1 + scale):  FY32, a float32 Cholesky solve of the float32-ROUNDED reference system (f32(M_ref), f32(D_ref));  FP32, the
    same solve of the float32-EVALUATED system (f32(M_ref), D32 = the device's formulation in float32 at aba32, the float32 articulated-body
    solution) - what a float32 pipeline that computes its acceleration and its right-hand side itself loses.  variant: "udot" (tau, no loads) or "loads"."""
    c = dyn_case(name)
    r = derivative_reference(name, variant, at_forward=True)
    _, D32, _ = tangent_newton_euler(c.blob, c.gc, c.gv, aba32(name, variant == "loads"), c.gravity, case_loads(c) if variant == "loads" else (), np.float32, True)
    lo = dict(dq=D32[:, :, :c.nv], dv=D32[:, :, c.nv:2 * c.nv])
    j0, nv = c.j0, c.nv
    out = SimpleNamespace(dq=np.zeros((c.N, nv, nv)), dv=np.zeros((c.N, nv, nv)), dtau=np.zeros((c.N, nv, nv)), s_dq=np.zeros((c.N, nv, nv)), s_dv=np.zeros((c.N, nv, nv)),
                          s_dtau=np.zeros((c.N, nv, nv)), udot=forward_reference(name, variant == "loads").udot)
    worst = [0.0, 0.0]
    for e in range(c.N):
        Mr = c.M[e][j0:, j0:]
        Mi = np.linalg.inv(Mr)
        L = np.linalg.cholesky(Mr.astype(np.float32))
        out.dtau[e, j0:, j0:] = Mi
        out.s_dtau[e, j0:, j0:] = np.abs(Mi)
        for k in ("dq", "dv"):
            Dk, Sk = getattr(r, k)[e][j0:], getattr(r, "s_" + k)[e][j0:]
            X = -np.linalg.solve(Mr, Dk)
            getattr(out, k)[e, j0:] = X
            scale = np.abs(Mi) @ (1 + Sk)
            getattr(out, "s_" + k)[e, j0:] = scale
            for n, rhs in enumerate((Dk.astype(np.float32), lo[k][e][j0:])):
                X32 = -scipy.linalg.cho_solve((L, True), rhs).astype(np.float64)
                assert rhs.dtype == np.float32
                worst[n] = max(worst[n], float((np.abs(X32 - X) / (1 + scale)).max()))
    out.FY32, out.FP32 = worst
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the tests
def _retract(q, j, h):
    q = np.array(q, float)
    if j < 3:
        q[j] += h
    elif j < 6:
        e = np.eye(3)[j - 3] * np.sin(h / 2)
        a, b = np.array([np.cos(h / 2), *e]), q[3:7] / np.linalg.norm(q[3:7])
        q[3:7] = [a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))]
    else:
        q[7 + j - 6] += h
    return q


def _differences(fun, c, e, h):
    """central differences of fun(q, u, udot) -> tau along all 3 nv directions -> [nv, 3 nv] (a fixed base's six columns stay zero)"""
    nv = c.nv
    q, u, ud = c.gc[e].astype(float), c.gv[e].astype(float), c.udot[e].astype(float)
    out = np.zeros((nv, 3 * nv))
    for j in range(c.j0, nv):
        out[:, j] = (fun(_retract(q, j, h), u, ud) - fun(_retract(q, j, -h), u, ud)) / (2 * h)
        for k, base in ((1, u), (2, ud)):
            lo, hi = base.copy(), base.copy()
            lo[j] -= h; hi[j] += h
            out[:, k * nv + j] = ((fun(q, hi, ud) - fun(q, lo, ud)) if k == 1 else (fun(q, u, hi) - fun(q, u, lo))) / (2 * h)
    return out


def _richardson(fun, c, e, h=1e-3):
    d1, d2 = _differences(fun, c, e, h), _differences(fun, c, e, h / 2)
    return (4 * d2 - d1) / 3, np.abs(d2 - d1)


@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_differences_of_newton_euler_and_of_the_oracle(built_lib, name):
    """pins (a) and (b) of the module docstring on the first and the last env, and the reference's own tau against newton_euler's"""
    c = dyn_case(name)
    r = derivative_reference(name, "loads")
    plain = derivative_reference(name, "udot")
    worst = [0.0, 0.0]
    for e in (0, c.N - 1):
        def ne(q, u, ud, e=e):
            return newton_euler(c.blob, q, u, ud, c.gravity, load_list(c, kinematics(c.blob, q), e))[0]

        def orc(q, u, ud):
            return c.o.inverse_dynamics(q, masked(c, u), masked(c, ud))
        want = ne(c.gc[e].astype(float), c.gv[e].astype(float), c.udot[e].astype(float))
        assert np.abs(r.tau[e] - want).max() <= 1e-10 * (1 + np.abs(want).max())
        for k, (fun, ref, rows) in enumerate(((ne, r, slice(0, None)), (orc, plain, slice(c.j0, None)))):
            D = np.concatenate([ref.dq[e], ref.dv[e], ref.dudot[e]], axis=1)
            S = np.concatenate([ref.s_dq[e], ref.s_dv[e], ref.s_dudot[e]], axis=1)
            DR, est = _richardson(fun, c, e)
            ratio = (np.abs(D - DR) / (est + 1e-9 * (1 + S)))[rows]
            worst[k] = max(worst[k], ratio.max())
            assert ratio.max() <= 1.0, (name, e, k, ratio.max(), np.unravel_index(ratio[rows].argmax(), ratio[rows].shape))
            assert np.abs(D).max() > 1e-3
    print(f"{name}: |D_ref - Richardson| / (|D(h/2) - D(h)| + 1e-9 (1 + S)), worst entry: newton_euler {worst[0]:.3f}, oracle {worst[1]:.3f}")


@pytest.mark.parametrize("name", NAMES)
def test_known_answers(built_lib, name):
    """(c) dtau_dudot = M (Oracle.mass_matrix) to 1e-9 of scale.  Columns j < 3 of dtau_dq are exact zeros, with and without loads; a fixed base's six
    columns are zero in every matrix; dtau_dv = 0 at gv = 0; at gv = udot = 0 without loads the joint-joint block of dtau_dq is symmetric (the
    Hessian of the potential); dtau_dq is linear in the load; the forward reference solves M X = -D."""
    c = dyn_case(name)
    j0, nv = c.j0, c.nv
    for variant in VARIANTS:
        r = derivative_reference(name, variant)
        assert np.abs(r.dudot[:, j0:, j0:] - c.M[:, j0:, j0:]).max() <= 1e-9 * (1 + np.abs(c.M).max()), (name, variant)
        assert not r.dq[:, :, :max(3, j0)].any() and not r.dv[:, :, :j0].any() and not r.dudot[:, :, :j0].any()
        assert np.isfinite(r.dq).all() and np.isfinite(r.dv).all()
    zero = np.zeros_like(c.gv)
    _, D, S = tangent_newton_euler(c.blob, c.gc, zero, None, c.gravity)
    assert np.abs(D[:, :, nv:2 * nv]).max() == 0.0
    G = D[:, 6:, 6:nv]
    assert np.abs(G - G.swapaxes(1, 2)).max() <= 1e-10 * (1 + np.abs(S[:, 6:, 6:nv]).max())
    _, D0, _ = tangent_newton_euler(c.blob, c.gc, c.gv, c.udot, c.gravity)
    loads = case_loads(c)
    _, D1, S1 = tangent_newton_euler(c.blob, c.gc, c.gv, c.udot, c.gravity, loads)
    _, D2, _ = tangent_newton_euler(c.blob, c.gc, c.gv, c.udot, c.gravity, [(b, o, 2 * fo, 2 * to) for b, o, fo, to in loads])
    assert np.abs((D2 - D0) - 2 * (D1 - D0))[:, :, :nv].max() <= 1e-10 * (1 + S1.max())
    assert np.abs(D1 - D0)[:, :, :nv].max() > 1e-3 and np.abs(D1 - D0)[:, :, nv:].max() == 0.0
    fr = forward_derivative_reference(name, "loads")
    ref = derivative_reference(name, "loads", at_forward=True)
    for e in (0, c.N - 1):
        assert np.abs(c.M[e][j0:, j0:] @ fr.dq[e][j0:] + ref.dq[e][j0:]).max() <= 1e-8 * (1 + ref.s_dq[e].max())
        assert (fr.s_dq[e][j0:] >= np.abs(fr.dq[e][j0:]) * (1 - 1e-9)).all()
        assert not fr.dq[e][:j0].any() and not fr.dq[e][:, :j0].any()


def test_float32_yardsticks(built_lib):
    """Y32 and YD32 (inverse-dynamics matrices: the reference's and the device's formulation in float32), FY32 and FP32 (forward-dynamics matrices: the float32 Cholesky solve of the float32-rounded, and of the
    float32-evaluated, reference system) of every case, printed: the constants of tests/test_gpu_dynamics_derivatives.py.  Reproduce with
        python -m pytest tests/test_dynamics_derivatives_reference.py::test_float32_yardsticks -s"""
    print()
    for name in NAMES:
        fr = [forward_derivative_reference(name, v) for v in ("udot", "loads")]
        y, yd, fy, fp = y32(name), y32(name, True), max(r.FY32 for r in fr), max(r.FP32 for r in fr)
        print(f'  "{name}": ({y:.3e}, {yd:.3e}, {fy:.3e}, {fp:.3e}),')
        assert np.isfinite([y, yd, fy, fp]).all() and 0 < y < 1e-3 and 0 < yd < 1e-3
