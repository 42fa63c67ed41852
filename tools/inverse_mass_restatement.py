"""The algorithm of csrc/rsb_inverse_mass.hip (solve_kernel, delassus_kernel) restated in numpy, one env at a time, every step in the dtype asked
for: the chain walk (world transforms from the base quaternion and the joint angles, positions accumulated from the base position and taken
relative to it afterwards, as walk_chain does); the common frame with world axes and the env's base origin as its origin, inertias as (J, H, M)
blocks; the articulated-inertia up pass ONCE (children gathered in ascending body order, D = S^T U + armature + joint_diag, an LDL^T of the base's
6 x 6 block) - in the dtype `factor_in` (the kernel: float64, its results rounded to the working dtype; float32 shows what the pass costs when it
is run like aba_kernel's); then per column the bias-force up pass, the base back-substitution and the acceleration down pass; a Delassus column
starts from minus a unit world force at the frame's point (or a unit torque on its body) and entry (i, c), i <= c, is read off the spatial
acceleration of frame i's body and mirrored.
In float64 it checks the formulation against the references of tests/inverse_mass_reference.py; in float32 it says what a correct float32 device can
reach on those cases - the table IM32 / G32 / JM32 of tests/test_gpu_inverse_mass.py, each the maximum over the envs and over the variants that
file runs (inverse_mass_reference.SOLVE_VARIANTS, delassus_variants).  CPU only:  python tools/inverse_mass_restatement.py [case ...]"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def skew(a, T):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], T)


def walk(blob, q, T, const):
    """walk_chain's recursion without velocities, in dtype T, from the model's constants rounded to `const`: (R, p - o, a) of every body"""
    c = lambda x: np.asarray(np.asarray(x, const), T)
    qq = np.asarray(q, T)
    w, x, y, z = qq[3:7] * (T(1) / np.sqrt(qq[3:7] @ qq[3:7]))
    R = [np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], T)]
    p, a = [np.zeros(3, T)], [np.zeros(3, T)]
    for i in range(1, blob.nb):
        par = blob.parent[i]
        ax, Rt, pt = c(blob.axis[i][:]), c(blob.rtree[i][:]).reshape(3, 3), c(blob.ptree[i][:])
        qi = qq[6 + i]
        d = R[par] @ pt
        if blob.jtype[i] == 1:
            sn, cs = np.sin(qi), np.cos(qi)
            Rq = (cs * np.eye(3, dtype=T) + (T(1) - cs) * np.outer(ax, ax) + sn * skew(ax, T)).astype(T)
            Ri = R[par] @ (Rt @ Rq)
            ai = Ri @ ax
        else:
            Ri = R[par] @ Rt
            ai = Ri @ ax
            d = d + ai * qi
        R.append(Ri.astype(T)); a.append(ai.astype(T)); p.append((p[par] + d).astype(T))
    return R, p, a


def factor(blob, q, diag, T, factor_in=np.float64):
    """phase 1: everything of the env that does not depend on the column - the walk, the bodies' inertias about o, the joints' spatial axes, the
    articulated-inertia up pass and the base's LDL^T - in factor_in, from the model's constants and q rounded to T (what the device holds); what the
    columns use (S, U, 1 / D, L, 1 / Dg, and R, p - o of the frames' bodies) rounded to T."""
    nb = blob.nb
    TF = factor_in
    c = lambda x: np.asarray(np.asarray(x, T), TF)      # a constant as the device holds it, in the dtype phase 1 computes in
    Rw, pw, aw = walk(blob, c(q), TF, T)
    J, H, M, S, R, po = [], [], [], [None], [], []
    for i in range(nb):
        m, Ri = TF(T(blob.mass[i])), Rw[i]
        p = pw[i]
        r = p + Ri @ c(blob.com[i][:])
        ii = blob.inertia[i]
        Iw = (Ri @ c([[ii[0], ii[1], ii[2]], [ii[1], ii[3], ii[4]], [ii[2], ii[4], ii[5]]])) @ Ri.T
        J.append((Iw + m * ((r @ r) * np.eye(3, dtype=TF) - np.outer(r, r))).astype(TF)); H.append((m * skew(r, TF)).astype(TF)); M.append(m * np.eye(3, dtype=TF))
        R.append(Ri.astype(T)); po.append(p.astype(T))
        if i >= 1:
            a = aw[i]
            S.append((np.r_[a, np.cross(p, a)] if blob.jtype[i] == 1 else np.r_[np.zeros(3, TF), a]).astype(TF))
    level = [0] * nb
    for i in range(1, nb):
        level[i] = level[blob.parent[i]] + 1
    kids = [[i for i in range(j + 1, nb) if blob.parent[i] == j] for j in range(nb)]
    U, iD = [None] * nb, [None] * nb
    for lv in range(max(level), 0, -1):
        pub = {}
        for i in range(nb):
            if level[i] != lv:
                continue
            sa, sl = S[i][:3], S[i][3:]
            Ud = np.r_[J[i] @ sa + H[i] @ sl, H[i].T @ sa + M[i] @ sl].astype(TF)
            iDd = TF(1) / (((sa @ Ud[:3] + sl @ Ud[3:]) + TF(T(blob.armature[i]))) + TF(T(diag[5 + i])))
            U[i], iD[i] = Ud.astype(T), T(iDd)
            pub[i] = ((J[i] - np.outer(Ud[:3], Ud[:3]) * iDd).astype(TF), (H[i] - np.outer(Ud[:3], Ud[3:]) * iDd).astype(TF),
                      (M[i] - np.outer(Ud[3:], Ud[3:]) * iDd).astype(TF))
        for j in range(nb):
            if level[j] == lv - 1:
                for i in kids[j]:
                    J[j] = J[j] + pub[i][0]; H[j] = H[j] + pub[i][1]; M[j] = M[j] + pub[i][2]
    L, iDg = np.eye(6, dtype=TF), np.zeros(6, TF)
    if not blob.fixed_base:
        K = np.block([[J[0], H[0]], [H[0].T, M[0]]]).astype(TF)
        Dg = np.zeros(6, TF)
        for j in range(6):
            d = K[j, j]
            for kx in range(j):
                d = d - L[j, kx] * L[j, kx] * Dg[kx]
            Dg[j] = d; iDg[j] = TF(1) / d
            for i in range(j + 1, 6):
                s = K[i, j]
                for kx in range(j):
                    s = s - L[i, kx] * L[j, kx] * Dg[kx]
                L[i, j] = s * iDg[j]
    return SimpleNamespace(T=T, nb=nb, nv=blob.nv, fixed=bool(blob.fixed_base), parent=list(blob.parent[:nb]), level=level, kids=kids,
                           S=[None if x is None else x.astype(T) for x in S], U=U, iD=iD, L=L.astype(T), iDg=iDg.astype(T), R=R, po=po)


def column(F, b=None, load=None):
    """phase 2 for one column.  b [nv] (None: zeros); load = (body, bias force 6): what a Delassus column starts from.
    -> (udot [nv], spatial accelerations [nb, 6], angular first)"""
    T, nb = F.T, F.nb
    b = np.zeros(F.nv, T) if b is None else np.asarray(b, T)
    p = [np.zeros(6, T) for _ in range(nb)]
    if load is not None:
        p[load[0]] = np.asarray(load[1], T)
    uu = [T(0)] * nb
    for lv in range(max(F.level), 0, -1):
        pub = {}
        for i in range(nb):
            if F.level[i] == lv:
                uu[i] = b[5 + i] - (F.S[i][:3] @ p[i][:3] + F.S[i][3:] @ p[i][3:])
                pub[i] = (p[i] + F.U[i] * (uu[i] * F.iD[i])).astype(T)
        for j in range(nb):
            if F.level[j] == lv - 1:
                for i in F.kids[j]:
                    p[j] = p[j] + pub[i]
    udot, A = np.zeros(F.nv, T), [None] * nb
    A[0] = np.zeros(6, T)
    if not F.fixed:
        x = np.r_[b[3:6] - p[0][:3], b[0:3] - p[0][3:]].astype(T)
        for i in range(6):
            for kx in range(i):
                x[i] = x[i] - F.L[i, kx] * x[kx]
        x = (x * F.iDg).astype(T)
        for i in range(5, -1, -1):
            for kx in range(i + 1, 6):
                x[i] = x[i] - F.L[kx, i] * x[kx]
        A[0] = x
        udot[0:3], udot[3:6] = x[3:], x[:3]
    for i in range(1, nb):
        Ap = A[F.parent[i]]
        qdd = (uu[i] - (F.U[i][:3] @ Ap[:3] + F.U[i][3:] @ Ap[3:])) * F.iD[i]
        udot[5 + i] = qdd
        A[i] = (Ap + F.S[i] * qdd).astype(T)
    return udot, A


def solve(F, B):
    """X [R, nv] for B [R, nv]"""
    return np.array([column(F, b)[0] for b in B])


def delassus(F, frames, angular):
    """(G [kF, kF], JMinv [kF, nv]) of the frames [(body, offset)]"""
    T = F.T
    kk = 6 if angular else 3
    n = kk * len(frames)
    r = [F.po[body] + F.R[body] @ np.asarray(off, T) for body, off in frames]
    G, JM = np.zeros((n, n), T), np.zeros((n, F.nv), T)
    for c in range(n):
        f, a = divmod(c, kk)
        e = np.zeros(3, T); e[a % 3] = 1
        bias = np.r_[-np.cross(r[f], e), -e] if a < 3 else np.r_[-e, np.zeros(3, T)]
        JM[c], A = column(F, None, (frames[f][0], bias.astype(T)))
        for i in range(c + 1):
            fi, ai = divmod(i, kk)
            acc = A[frames[fi][0]]
            G[i, c] = G[c, i] = (acc[3 + ai] + np.cross(acc[:3], r[fi])[ai]) if ai < 3 else acc[ai - 3]
    return G, JM


def figures(name, T, factor_in=np.float64):
    """(IM, G, JM, gate): the three error measures of the restatement in dtype T on one case, each the maximum over the envs and the variants, and the
    largest residual |A x - b| over its bar 2e-5 (1 + largest row of |A||x| + |b|) of the solves"""
    import inverse_mass_reference as ref
    from test_dynamics_reference import dyn_case
    c = dyn_case(name)
    im = g = jm = gate = 0.0
    zero = np.zeros(c.nv)
    for with_diag in (False, True):
        svar = [w for w, d in ref.SOLVE_VARIANTS if d == with_diag and w != "r1"]      # (r1 is r5's first column)
        dvar = [(k, a) for k, a, d in ref.delassus_variants(name) if d == with_diag]
        facs = [factor(c.blob, c.gc[e], ref.joint_diag(name) if with_diag else zero, T, factor_in) for e in range(c.N)]
        for which in svar:
            X = np.array([solve(facs[e], ref.rhs(name, which)[e]) for e in range(c.N)])
            im = max(im, ref.x_error(X, ref.solve_reference(name, which, with_diag)).max())
            gate = max(gate, ref.residual_ratio(ref.system(name, with_diag), X, ref.rhs(name, which), c.j0).max())
        for key, angular in dvar:
            out = [delassus(facs[e], ref.frame_sets(name)[key], angular) for e in range(c.N)]
            Gr, JMr = ref.delassus_reference(name, key, angular, with_diag)
            g = max(g, ref.rel_error(np.array([o[0] for o in out]), Gr).max())
            jm = max(jm, ref.rel_error(np.array([o[1] for o in out]), JMr).max())
    return im, g, jm, gate


def main():
    import inverse_mass_reference as ref
    names = sys.argv[1:] or ref.CASES
    print("X: max|X - X_ref| / (1 + max|X_ref|); G, JMinv: max|. - ref| / max|ref|; gate: |A x - b| / (2e-5 (1 + largest row of |A||x| + |b|)); each the max over envs and variants")
    print("            float32, factorisation in float64 (the kernel)  | all float32 (aba_kernel's way)                  | all float64")
    print("case        IM32       G32        JM32       gate       | IM         G          JM         gate       | IM64       G64        JM64       gate")
    for name in names:
        cols = [figures(name, np.float32), figures(name, np.float32, np.float32), figures(name, np.float64)]
        print(f"{name:10s}  " + "  | ".join("  ".join(f"{x:.3e}" for x in col) for col in cols), flush=True)


if __name__ == "__main__":
    main()
