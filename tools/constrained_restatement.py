"""The arithmetic of csrc/rsb_constrained.hip (held_solve_kernel) restated in numpy, one env at a time, on inputs that are themselves restatements of
what the device hands it: udot_f from tools/dynamics_aba_restatement.aba in float32, G and JMinv from tools/inverse_mass_restatement (float32 columns,
the factorisation in float64: delassus_kernel), the frames' accelerations J udot_f + Jdot gv (velocities J gv) from the fp64 recursion on that
udot_f, rounded to float32.  The kernel's steps, each in the dtype asked for: rho = damping * max diag G in float32; the root-free Cholesky
W D^-1 W^T of G + rho I, left-looking, column by column, the sum over k in ascending order; the pivot rule of rsb.h; the forward substitution by
columns, the scaling, the back substitution; lambda rounded to float32; x = x_f + JMinv^T lambda accumulated in float32 in row order.

For every case and variant of tests/constrained_reference.py it prints, for the factorisation in float32 and in float64, the worst env's two gates
(residual over 2e-5 (1 + S), tests/constrained_reference.gates), whether every env has the status its class asks for, and on the regular sets the
forward errors max|x - x_ref| / (1 + max|x_ref|) of lambda and of udot / dgv; then per case the figures the GPU test takes its forward bars from
(LAM32 / X32, dynamics and impulse: the maximum over the case's regular variants, with the float32 factorisation - the kernel's).
CPU only:  python tools/constrained_restatement.py [case ...] > profiles/constrained_restatement.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PIVOT_TOL = np.float32(1e-5)      # RSB_HELD_PIVOT_TOL


def held_solve(G, JM, xf, a, t, damping, T, fixed):
    """one env.  G [m, m], JM [m, nv], xf [nv], a [m], t [m] float32; T: the dtype of the factorisation and the substitutions
    -> (x [nv] float32, lambda [m] float32, status, the first refused pivot over RSB_HELD_PIVOT_TOL times its entry)"""
    f = np.float32
    m = len(G)
    rho = T(f(damping) * G.diagonal().max())
    A = G.astype(T)
    d0 = A.diagonal() + rho
    W = np.tril(A)
    W[np.arange(m), np.arange(m)] = d0
    iD = np.zeros(m, T)
    bad, first = False, 0.0      # first: the first refused pivot over its threshold (< 1: how far below)
    for j in range(m):
        s = W[j:, j].copy()
        for k in range(j):
            s -= W[j:, k] * W[j, k] * iD[k]
        W[j:, j] = s
        pivot_bad = not (s[0] > T(PIVOT_TOL) * d0[j]) or not np.isfinite(s[0])
        if pivot_bad and not bad:
            first = float(s[0] / (T(PIVOT_TOL) * d0[j]))
        bad = bad or pivot_bad
        iD[j] = T(0) if pivot_bad else T(1) / s[0]
    x = (t - a).astype(f).astype(T)
    for k in range(m - 1):
        x[k + 1:] -= W[k + 1:, k] * (x[k] * iD[k])
    x *= iD
    for k in range(m - 1, 0, -1):
        x[:k] -= W[k, :k] * iD[:k] * x[k]
    lam = np.zeros(m, f) if bad else x.astype(f)
    out = xf.astype(f).copy()
    if not bad:
        for i in range(m):
            out += JM[i].astype(f) * lam[i]
    if fixed:
        out[:6] = 0
    return out, lam, int(bad), first


def device_inputs(name, key, angular, with_diag):
    """per env, float32: (udot_f, G, JMinv, a_f = J udot_f + Jdot gv, v = J gv) as restatements of the device's own queries"""
    import constrained_reference as cr
    import inverse_mass_reference as imr
    from dynamics_aba_restatement import aba
    from inverse_mass_restatement import delassus, factor
    from test_dynamics_reference import dyn_case
    from test_frame_accel_reference import ref_accel
    c, frames, kk = dyn_case(name), cr.frame_sets(name)[key], 6 if angular else 3
    u = cr.gv_of(c)
    f = np.float32
    diag = imr.joint_diag(name) if with_diag else np.zeros(c.nv)
    uf, Gs, JMs, af, vs = [], [], [], [], []
    J = cr.stacked_jacobian(name, key, angular)
    for e in range(c.N):
        tau = np.array(c.tau[e])
        if c.fixed:
            tau[:6] = 0
        ud = aba(c.blob, c.gc[e], u[e], tau, c.gravity, [], f)
        if c.fixed:
            ud[:6] = 0
        uf.append(ud)
        G, JM = delassus(factor(c.blob, c.gc[e], diag, f), frames, angular)
        Gs.append(G); JMs.append(JM)
        r = ref_accel(c.blob, c.gc[e], u[e], ud.astype(np.float64), frames)
        af.append(np.concatenate([np.r_[r.lin[n], r.ang[n]][:kk] for n in range(len(frames))]).astype(f))
        vs.append((J[e] @ u[e]).astype(f))
    return uf, Gs, JMs, af, vs


def run(name, key, angular, damping, T, cache):
    """-> dict of the variant's worst figures, dynamics and impulse"""
    import constrained_reference as cr
    from test_dynamics_reference import dyn_case
    c = dyn_case(name)
    out = {}
    for impulse in (False, True):
        ck = (name, key, angular, impulse)
        if ck not in cache:
            cache[ck] = device_inputs(name, key, angular, impulse)      # (the impulse runs with joint_diag)
        uf, Gs, JMs, af, vs = cache[ck]
        t = cr.target(name, key, angular, "vel" if impulse else "acc")
        xs, lams, sts, firsts = [], [], [], []
        for e in range(c.N):
            x, lam, st, first = held_solve(Gs[e], JMs[e], np.zeros(c.nv, np.float32) if impulse else uf[e], vs[e] if impulse else af[e], t[e].astype(np.float32), damping, T, c.fixed)
            xs.append(x); lams.append(lam); sts.append(st); firsts.append(first)
        xs, lams, sts = np.array(xs), np.array(lams), np.array(sts)
        want = 0 if cr.solvable(name, key, angular, damping) else 1
        tag = "imp" if impulse else "dyn"
        out[tag + "_status_ok"] = bool((sts == want).all())
        out[tag + "_status_hist"] = (int((sts == 0).sum()), int((sts == 1).sum()))
        if want == 1:
            out[tag + "_refused"] = float(np.nanmax(np.where(np.isfinite(firsts), firsts, np.nan))) if np.isfinite(firsts).any() else float("nan")
        if want == 0 and (sts == 0).all():
            dyn, con = cr.gates(name, key, angular, damping, impulse, xs, lams, t, impulse, None if impulse else np.array(uf))
            out[tag + "_gates"] = (float(dyn.max()), float(con.max()))
            if damping == 0:
                xr, lr = cr.impulse_reference(name, key, angular, 0.0, True) if impulse else cr.dynamics_reference(name, key, angular, 0.0)
                out[tag + "_fwd"] = (float(cr.forward_error(lams, lr).max()), float(cr.forward_error(xs, xr).max()))
    return out


def main():
    import constrained_reference as cr
    names = sys.argv[1:] or cr.CASES
    print("tools/constrained_restatement.py: held_solve_kernel's arithmetic in numpy on float32 restatements of its inputs.  gates: the worst env's (dynamics row, constraint row)")
    print("residual over 2e-5 (1 + S); refused pivot / threshold: the largest over the envs of the first refused pivot over 1e-5 times its entry (dependent sets: < 1, the margin); status: every env has the status of its class (solved, singular counts); fwd: (lambda, udot or dgv) max|x - x_ref| / (1 + max|x_ref|), regular sets")
    summary = {}
    for name in names:
        cache = {}
        for key, angular, damping in cr.variants(name):
            m = cr.rows_of(name, key, angular)
            cls = "regular" if cr.regular(name, key, angular) else "dependent"
            for T in (np.float32, np.float64):
                r = run(name, key, angular, damping, T, cache)
                line = f"{name:10s} {key:9s} ang={int(angular)} m={m:2d} damping={damping:.0e} {cls:9s} factor={T.__name__:7s}"
                for tag in ("dyn", "imp"):
                    line += f" | {tag}: status {'ok ' if r[tag + '_status_ok'] else 'BAD'} {r[tag + '_status_hist']}"
                    if tag + "_refused" in r:
                        line += " refused pivot / threshold <= %.3f" % r[tag + "_refused"]
                    if tag + "_gates" in r:
                        line += " gates %.3f %.3f" % r[tag + "_gates"]
                    if tag + "_fwd" in r:
                        line += " fwd %.3e %.3e" % r[tag + "_fwd"]
                        if T is np.float32:
                            s = summary.setdefault(name, {"dyn": [0.0, 0.0], "imp": [0.0, 0.0]})
                            s[tag] = [max(s[tag][0], r[tag + "_fwd"][0]), max(s[tag][1], r[tag + "_fwd"][1])]
                print(line, flush=True)
    print("the forward figures of the float32 factorisation (the kernel's) per case, the maximum over its regular variants: LAM32, UD32 (dynamics), ILAM32, DGV32 (impulse)")
    for name, s in summary.items():
        print(f"  {name:10s} LAM32 {s['dyn'][0]:.3e}  UD32 {s['dyn'][1]:.3e}  ILAM32 {s['imp'][0]:.3e}  DGV32 {s['imp'][1]:.3e}")


if __name__ == "__main__":
    main()
