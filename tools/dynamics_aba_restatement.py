"""The articulated-body algorithm of csrc/rsb_dynamics.hip (aba_kernel) restated in numpy, one env at a time, every step in the dtype asked for:
the common frame with world axes and the env's base origin as its origin, inertias as (J, H, M) blocks, the up pass gathering children in ascending
body order, an LDL^T solve at the base.  In float64 it checks the formulation against solve(M, tau - h + J^T w); in float32 it says what a correct
float32 device can reach on the cases of tests/test_dynamics_reference.py - the figure next to E32 (the float32 Cholesky solve of the oracle's own
system) in the docstring of tests/test_gpu_dynamics.py::test_forward_dynamics.  CPU only:  python tools/dynamics_aba_restatement.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def skew(a, T):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], T)


def aba(blob, q, u, tau, gravity, loads, T):
    """loads: (body, world point, force, torque).  -> udot [nv] in dtype T"""
    from test_dynamics_reference import kinematics
    k = kinematics(blob, q, u)      # (transforms and velocities in float64, rounded below: the rounding of the walk is not what is measured here)
    nb, nv = blob.nb, blob.nv
    c = lambda x: np.asarray(x, T)
    o, g = k.p[0], c(gravity)
    J, H, M, pA, S, cb = [], [], [], [], [None], [None]
    for i in range(nb):
        m, R, w, v = T(blob.mass[i]), c(k.R[i]), c(k.w[i]), c(k.v[i])
        po = c(k.p[i] - o)
        r = po + R @ c(blob.com[i][:])
        ii = blob.inertia[i]
        Iw = R @ c([[ii[0], ii[1], ii[2]], [ii[1], ii[3], ii[4]], [ii[2], ii[4], ii[5]]]) @ R.T
        fm = m * (v + np.cross(w, R @ c(blob.com[i][:])))
        nm = Iw @ w + np.cross(r, fm)
        vo = v - np.cross(w, po)
        fe, ne = np.zeros(3, T), np.zeros(3, T)
        for body, point, force, torque in loads:
            if body == i:
                fe = fe + c(force); ne = ne + c(torque) + np.cross(c(point - o), c(force))
        pA.append(np.r_[np.cross(w, nm) + np.cross(vo, fm) - ne, np.cross(w, fm) - fe].astype(T))
        J.append((Iw + m * ((r @ r) * np.eye(3, dtype=T) - np.outer(r, r))).astype(T)); H.append(m * skew(r, T)); M.append(m * np.eye(3, dtype=T))
        if i >= 1:
            par, a = blob.parent[i], c(k.a[i])
            s = np.r_[a, np.cross(po, a)] if blob.jtype[i] == 1 else np.r_[np.zeros(3, T), a]
            wp, vop = c(k.w[par]), c(k.v[par]) - np.cross(c(k.w[par]), c(k.p[par] - o))
            S.append(s.astype(T))
            cb.append((np.r_[np.cross(wp, s[:3]), np.cross(wp, s[3:]) + np.cross(vop, s[:3])] * T(u[5 + i])).astype(T))
    U, iD, uu = [None] * nb, [None] * nb, [None] * nb
    level = [0] * nb
    for i in range(1, nb):
        level[i] = level[blob.parent[i]] + 1
    pub = [None] * nb
    for lv in range(max(level), 0, -1):
        for i in range(nb):
            if level[i] != lv:
                continue
            sa, sl = S[i][:3], S[i][3:]
            U[i] = np.r_[J[i] @ sa + H[i] @ sl, H[i].T @ sa + M[i] @ sl].astype(T)
            iD[i] = T(1) / (sa @ U[i][:3] + sl @ U[i][3:] + T(blob.armature[i]))
            uu[i] = T(tau[5 + i]) - (sa @ pA[i][:3] + sl @ pA[i][3:])
            Ja = J[i] - np.outer(U[i][:3], U[i][:3]) * iD[i]; Ha = H[i] - np.outer(U[i][:3], U[i][3:]) * iD[i]; Ma = M[i] - np.outer(U[i][3:], U[i][3:]) * iD[i]
            pa = pA[i] + np.r_[Ja @ cb[i][:3] + Ha @ cb[i][3:], Ha.T @ cb[i][:3] + Ma @ cb[i][3:]] + U[i] * (uu[i] * iD[i])
            pub[i] = (Ja.astype(T), Ha.astype(T), Ma.astype(T), pa.astype(T))
        for j in range(nb):
            if level[j] != lv - 1:
                continue
            for i in range(j + 1, nb):
                if blob.parent[i] == j:
                    J[j] = J[j] + pub[i][0]; H[j] = H[j] + pub[i][1]; M[j] = M[j] + pub[i][2]; pA[j] = pA[j] + pub[i][3]
    udot = np.zeros(nv, T)
    A = [None] * nb
    if blob.fixed_base:
        A[0] = np.r_[np.zeros(3, T), -g]
    else:
        K = np.block([[J[0], H[0]], [H[0].T, M[0]]]).astype(T)
        rhs = np.r_[c(tau[3:6]) - pA[0][:3], c(tau[0:3]) - pA[0][3:]].astype(T)
        L = np.linalg.cholesky(K)
        A[0] = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).astype(T)
        udot[0:3] = A[0][3:] + np.cross(c(k.w[0]), c(k.v[0])) + g
        udot[3:6] = A[0][:3]
    for i in range(1, nb):
        Ap = A[blob.parent[i]] + cb[i]
        qdd = (uu[i] - U[i] @ Ap) * iD[i]
        udot[5 + i] = qdd
        A[i] = (Ap + S[i] * qdd).astype(T)
    return udot


def main():
    from test_dynamics_reference import NAMES, dyn_case, forward_reference, kinematics, load_list
    print("case        E32 (fp32 Cholesky of the oracle's M)   ABA restated in fp32   ABA restated in fp64   (max over the envs of |udot - udot_ref| / (1 + max|udot_ref|))")
    for name in NAMES:
        c, fr = dyn_case(name), forward_reference(name)
        worst = {}
        for T in (np.float32, np.float64):
            w = 0.0
            for e in range(c.N):
                u = c.gv[e].copy()
                if c.fixed:
                    u[:6] = 0.0
                got = aba(c.blob, c.gc[e], u, c.tau[e], c.gravity, load_list(c, kinematics(c.blob, c.gc[e]), e), T).astype(np.float64)
                w = max(w, np.abs(got - fr.udot[e]).max() / (1 + np.abs(fr.udot[e]).max()))
            worst[T] = w
        print(f"{name:10s}  {fr.E32:.3e}                               {worst[np.float32]:.3e}              {worst[np.float64]:.3e}", flush=True)


if __name__ == "__main__":
    main()
