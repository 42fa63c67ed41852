"""The fp64 references of the held-frame queries (rsb_constrained_forward_dynamics, rsb_frame_impulse; include/rsb.h), the inputs and the error
measures the CPU tests (tests/test_constrained_reference.py), the restatement tool (tools/constrained_restatement.py) and the GPU tests
(tests/test_gpu_constrained.py) share.  No test lives here.

The reference solves the KKT system directly, one (n + m) linear solve per env, n the joint block's size (nv, or nv - 6 on a fixed base):
    dynamics   [ M   -J^T  ] [ udot   ]   [ tau - h            ]          impulse   [ M + D  -J^T  ] [ dgv    ]   [ 0               ]
               [ J   rho I ] [ lambda ] = [ target - Jdot gv   ]                    [ J      rho I ] [ lambda ] = [ target - J gv   ]
a second formulation next to the device's Schur route (G + rho I) lambda = target - a_f; schur() is that route in fp64, for the pin of one against
the other.  M, h: the case's (Oracle.mass_matrix / nonlinearities); J: inverse_mass_reference.stacked_jacobian; Jdot gv: test_frame_accel_reference.
ref_accel without udot; D = diag(inverse_mass_reference.joint_diag); rho = damping * max diag(J (M + D)^-1 J^T).

Cases: floating0, fixed2, anymal, atlas of test_dynamics_reference.dyn_case, every env.  variants(case) lists every (frame set, angular, damping) the
GPU tests run.  A frame set's class is read off the fp64 Cholesky of its UNDAMPED G_ref: "regular" (the smallest pivot relative to its own diagonal
entry is >= 1e-3 on every env) or "dependent" (<= 1e-9 on every env); tests/test_constrained_reference.py pins that nothing lies in between.  A
regular set runs without damping, a dependent one without (status 1) and with DAMP (status 0; its pivots are then >= DAMP / (1 + DAMP) of their
entries).  Inputs: tau is the case's; target_acc / target_vel are N(0, 1)
rounded to float32 from a fixed seed.  Every function caches its result; nobody writes into what it returns."""
import functools

import numpy as np

from common import f32
from test_dynamics_reference import dyn_case
from test_frame_accel_reference import ref_accel
import inverse_mass_reference as imr

C_BAR = 2e-5      # the project's inverse-dynamics bar, the one inverse_mass_reference.residual_ratio uses
CASES = ["floating0", "fixed2", "anymal", "atlas"]
DAMP = 1e-4       # the damping the dependent sets are solved with
# The forward figures of the kernel's arithmetic restated in numpy float32 (tools/constrained_restatement.py, the last table of
# profiles/constrained_restatement.txt): per case the maximum over the envs and the regular variants of max|x - x_ref| / (1 + max|x_ref|), for
# (lambda, udot) of the dynamics and (lambda, dgv) of the impulse.  tests/test_constrained_reference.py recomputes them on the CPU and holds them to
# these values; tests/test_gpu_constrained.py takes 4 x them as its forward bars.
FWD32 = {"floating0": {"dyn": (1.018e-06, 4.189e-06), "imp": (8.392e-07, 1.248e-06)},
         "anymal": {"dyn": (7.376e-06, 6.642e-06), "imp": (2.339e-06, 2.320e-06)},
         "atlas": {"dyn": (7.456e-04, 7.099e-04), "imp": (1.865e-04, 2.115e-04)}}


def _f32_frames(frames):
    return [(int(b), tuple(float(np.float32(x)) for x in off)) for b, off in frames]


@functools.lru_cache(maxsize=None)
def frame_sets(name):
    """inverse_mass_reference.frame_sets of the case ("one", "three", "ancestor", the quadruped's "feet", floating0's "sixteen") and the lists of
    this feature: "twice" - one (body, offset) named two times: dependent for every env; "six" / "eleven" frames spread over the bodies of the
    humanoid and of floating0 (36 / 66 angular rows: more than nv); on the humanoid "hold3" - both feet and the torso, 18 angular rows - and
    "hold8" - hands, feet, forearms and shanks, 24 linear rows"""
    c = dyn_case(name)
    sets = dict(imr.frame_sets(name))
    rng = np.random.default_rng(4100 + c.nb)
    spread = lambda n: _f32_frames([(int(b), rng.uniform(-0.2, 0.2, 3)) for b in np.linspace(1 if c.nb > n else 0, c.nb - 1, n).round().astype(int)])
    sets["twice"] = [sets["one"][0], sets["three"][2], sets["one"][0]]
    if name in ("atlas", "floating0"):
        sets["six"] = spread(6)
        sets["eleven"] = spread(11)
    if name == "atlas":
        leaf = [i for i in range(c.nb) if i not in set(c.blob.parent[:c.nb])]      # head, hands, feet
        assert leaf == [4, 11, 18, 24, 30]
        r2 = np.random.default_rng(41)
        o = [r2.uniform(-0.2, 0.2, 3) for _ in range(8)]
        sets["hold3"] = _f32_frames([(24, o[0]), (30, o[1]), (3, o[2])])
        sets["hold8"] = _f32_frames([(b, o[i]) for i, b in enumerate((11, 18, 24, 30, 8, 15, 21, 27))])
    return sets


# (frame set, angular, damping, class, m) per case: the row counts straddle the lane-group edges 16 | 32 | 64 and the second row of a lane
_SETS = {      # (frame set, angular): m
    "floating0": [("one", False), ("one", True), ("three", True), ("six", True), ("eleven", True), ("sixteen", True), ("twice", False)],      # 3 6 | 18 36 66 96 9
    "fixed2": [("one", False), ("ancestor", False), ("three", True), ("twice", False)],                                                       # | 3 6 18 9: every chain has <= 2 joints
    "anymal": [("one", False), ("one", True), ("feet", False), ("feet", True), ("twice", False)],                                             # 3 6 12 | 24 9
    "atlas": [("one", False), ("hold3", True), ("hold8", False), ("ancestor", True), ("six", True), ("eleven", True)],                        # 3 18 24 | 12 36 66
}


def variants(name):
    """[(frame set, angular, damping)] of the case: every set without damping and, where it is dependent, also with DAMP"""
    out = []
    for key, angular in _SETS[name]:
        out.append((key, angular, 0.0))
        if not regular(name, key, angular, 0.0):
            out.append((key, angular, DAMP))
    return out


def rows_of(name, key, angular):
    return (6 if angular else 3) * len(frame_sets(name)[key])


@functools.lru_cache(maxsize=None)
def stacked_jacobian(name, key, angular):
    """J_ref [N, m, nv] of this file's frame sets (inverse_mass_reference.stacked_jacobian looks its own sets up)"""
    if key in imr.frame_sets(name):
        return imr.stacked_jacobian(name, key, angular)
    from test_dynamics_reference import jacobians, kinematics
    c, frames, kk = dyn_case(name), frame_sets(name)[key], 6 if angular else 3
    J = np.zeros((c.N, kk * len(frames), c.nv))
    for e in range(c.N):
        k = kinematics(c.blob, c.gc[e])
        for f, (body, off) in enumerate(frames):
            Jl, Jr = jacobians(c.blob, k, body, k.p[body] + k.R[body] @ np.asarray(off, float))
            J[e, kk * f:kk * f + 3] = Jl
            if angular:
                J[e, kk * f + 3:kk * f + 6] = Jr
    return J


def gv_of(c):
    """the case's velocities as the device sees them: a fixed base's six rows do not move"""
    u = np.array(c.gv, float)
    if c.fixed:
        u[:, :6] = 0.0
    return u


@functools.lru_cache(maxsize=None)
def bias(name, key, angular):
    """Jdot gv [N, m]: the frames' accelerations at udot = 0, rows ordered as J's"""
    c, frames, kk = dyn_case(name), frame_sets(name)[key], 6 if angular else 3
    u = gv_of(c)
    out = np.zeros((c.N, kk * len(frames)))
    for e in range(c.N):
        r = ref_accel(c.blob, c.gc[e], u[e], None, frames)
        for f in range(len(frames)):
            out[e, kk * f:kk * f + 3] = r.lin[f]
            if angular:
                out[e, kk * f + 3:kk * f + 6] = r.ang[f]
    return out


@functools.lru_cache(maxsize=None)
def target(name, key, angular, which):
    """target_acc ("acc") / target_vel ("vel") [N, m] float64 holding float32 values"""
    c = dyn_case(name)
    m = rows_of(name, key, angular)
    return f32(np.random.default_rng(4200 + m + (7 if which == "vel" else 0) + c.nv).normal(size=(c.N, m)))


@functools.lru_cache(maxsize=None)
def delassus(name, key, angular, with_diag):
    """(G_ref [N, m, m], JMinv_ref [N, m, nv]) with this file's J"""
    J, Ai = stacked_jacobian(name, key, angular), imr.inverse_reference(name, with_diag)
    JM = np.einsum("eki,eij->ekj", J, Ai)
    return np.einsum("eki,eli->ekl", JM, J), JM


def rho_of(name, key, angular, with_diag, damping):
    G = delassus(name, key, angular, with_diag)[0]
    return damping * np.einsum("eii->ei", G).max(axis=1)


@functools.lru_cache(maxsize=None)
def pivots(name, key, angular, with_diag, damping):
    """per env: the smallest pivot of the fp64 Cholesky of G_ref + rho I relative to its own diagonal entry (row by row, no pivoting; a pivot that is
    not positive ends the env's factorisation with that value)"""
    G, rho = delassus(name, key, angular, with_diag)[0], rho_of(name, key, angular, with_diag, damping)
    out = np.zeros(len(G))
    for e, (A, r) in enumerate(zip(G, rho)):
        A = A + r * np.eye(len(A))
        d0 = np.diag(A).copy()
        worst = np.inf
        for j in range(len(A)):
            worst = min(worst, A[j, j] / d0[j] if d0[j] > 0 else 0.0)      # (a row of zeros: a frame on a fixed base's root)
            if not A[j, j] > 0:
                break
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j]) / A[j, j]
        out[e] = worst
    return out


def _kkt(A, J, rho, top, bottom, j0):
    """per env: solve [[A, -J^T], [J, rho I]] [x; lambda] = [top; bottom] on the joint block -> (x [N, nv], lambda [N, m])"""
    N, m, nv = J.shape
    x, lam = np.zeros((N, nv)), np.zeros((N, m))
    n = nv - j0
    for e in range(N):
        K = np.block([[A[e][j0:, j0:], -J[e][:, j0:].T], [J[e][:, j0:], rho[e] * np.eye(m)]])
        s = np.linalg.solve(K, np.r_[top[e][j0:], bottom[e]])
        x[e, j0:], lam[e] = s[:n], s[n:]
    return x, lam


@functools.lru_cache(maxsize=None)
def dynamics_reference(name, key, angular, damping, with_target=True):
    """(udot_ref [N, nv], lambda_ref [N, m]) of rsb_constrained_forward_dynamics(tau = the case's, target_acc = target(..., "acc") or zeros)"""
    c = dyn_case(name)
    J = stacked_jacobian(name, key, angular)
    t = target(name, key, angular, "acc") if with_target else np.zeros(J.shape[:2])
    return _kkt(c.M, J, rho_of(name, key, angular, False, damping), c.tau - c.h, t - bias(name, key, angular), c.j0)


@functools.lru_cache(maxsize=None)
def impulse_reference(name, key, angular, damping, with_diag, with_target=True):
    """(dgv_ref [N, nv], lambda_ref [N, m]) of rsb_frame_impulse(target_vel = target(..., "vel") or zeros)"""
    c = dyn_case(name)
    J = stacked_jacobian(name, key, angular)
    t = target(name, key, angular, "vel") if with_target else np.zeros(J.shape[:2])
    v = np.einsum("eki,ei->ek", J, gv_of(c))
    return _kkt(imr.system(name, with_diag), J, rho_of(name, key, angular, with_diag, damping), np.zeros((c.N, c.nv)), t - v, c.j0)


def schur(name, key, angular, damping, with_diag, x_free, a_free, t):
    """the Schur route in fp64: (G + rho I) lambda = t - a_free, x = x_free + JMinv^T lambda -> (x, lambda)"""
    G, JM = delassus(name, key, angular, with_diag)
    rho = rho_of(name, key, angular, with_diag, damping)
    lam = np.array([np.linalg.solve(G[e] + rho[e] * np.eye(G.shape[1]), t[e] - a_free[e]) for e in range(len(G))])
    return x_free + np.einsum("eki,ek->ei", JM, lam), lam


@functools.lru_cache(maxsize=None)
def free_dynamics(name):
    """udot_f [N, nv] = solve(M, tau - h) on the joint block, fp64"""
    c = dyn_case(name)
    out = np.zeros((c.N, c.nv))
    for e in range(c.N):
        out[e, c.j0:] = np.linalg.solve(c.M[e][c.j0:, c.j0:], (c.tau[e] - c.h[e])[c.j0:])
    return out


def held_single(model, q, u, tau, frames, angular, gravity, rho=0.0, target=None):
    """one env of any model, for the closed-form pins: the KKT solve of the dynamics with M, h from the oracle -> (udot [nv], lambda [m], udot_f [nv])"""
    from common import Oracle
    from test_dynamics_reference import jacobians, kinematics
    blob = model.blob
    o = Oracle(blob); o.p.gravity[:] = gravity
    q, u = np.asarray(q, float), np.asarray(u, float)
    j0 = 6 if blob.fixed_base else 0
    M, h = o.mass_matrix(q)[j0:, j0:], o.nonlinearities(q, u)[j0:]
    k, kk = kinematics(blob, q), 6 if angular else 3
    J = np.zeros((kk * len(frames), blob.nv))
    for f, (body, off) in enumerate(frames):
        Jl, Jr = jacobians(blob, k, body, k.p[body] + k.R[body] @ np.asarray(off, float))
        J[kk * f:kk * f + 3] = Jl
        if angular:
            J[kk * f + 3:kk * f + 6] = Jr
    J = J[:, j0:]
    r = ref_accel(blob, q, u, None, frames)
    b = np.concatenate([np.r_[r.lin[n], r.ang[n]][:kk] for n in range(len(frames))])
    m, n = len(J), len(M)
    t = np.zeros(m) if target is None else np.asarray(target, float)
    K = np.block([[M, -J.T], [J, rho * np.eye(m)]])
    s = np.linalg.solve(K, np.r_[np.asarray(tau, float)[j0:] - h, t - b])
    udot, uf = np.zeros(blob.nv), np.zeros(blob.nv)
    udot[j0:], uf[j0:] = s[:n], np.linalg.solve(M, np.asarray(tau, float)[j0:] - h)
    return udot, s[n:], uf


# ------------------------------------------------------------------------------------------------------------------------------ error measures
def gates(name, key, angular, damping, with_diag, x, lam, t, impulse, x_free=None):
    """The two conditioning-free gates per env, each residual over its bar C_BAR (1 + S), evaluated in fp64 with the reference's matrices and the
    device's x (udot, or dgv) and lambda:
      dynamics row    |A x + h - tau - J^T lambda|_inf,  S the largest row of |A||x| + |h| + |tau| + |J^T||lambda|       (impulse: A (gv + x) - A gv,
                      i.e. |A x - J^T lambda| with S from |A||x| + |J^T||lambda|)
      constraint row  |J x + b - t + rho lambda|_inf, b = Jdot gv (impulse: J gv),  S2 the largest row of |J||x_free| + |J||JMinv^T||lambda| + |b| + |t| +
                      (|G| + rho)|lambda|   (x_free: udot_f, None = zeros for the impulse)
    -> (dynamics ratio [N], constraint ratio [N])"""
    c = dyn_case(name)
    j0 = c.j0
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    A = imr.system(name, with_diag)[:, j0:, j0:]
    J = stacked_jacobian(name, key, angular)[:, :, j0:]
    G, JM = delassus(name, key, angular, with_diag)
    JM = JM[:, :, j0:]
    rho = rho_of(name, key, angular, with_diag, damping)
    xs = x[:, j0:]
    Jtl, aJtl = np.einsum("eki,ek->ei", J, lam), np.einsum("eki,ek->ei", np.abs(J), np.abs(lam))
    Ax, aAx = np.einsum("eij,ej->ei", A, xs), np.einsum("eij,ej->ei", np.abs(A), np.abs(xs))
    if impulse:
        res, S = np.abs(Ax - Jtl), aAx + aJtl
        b = np.einsum("eki,ei->ek", J, gv_of(c)[:, j0:])
    else:
        h, tau = c.h[:, j0:], c.tau[:, j0:]
        res, S = np.abs(Ax + h - tau - Jtl), aAx + np.abs(h) + np.abs(tau) + aJtl
        b = bias(name, key, angular)
    dyn = res.max(axis=1) / (C_BAR * (1 + S.max(axis=1)))
    xf = np.zeros_like(xs) if x_free is None else np.asarray(x_free, np.float64)[:, j0:]
    res2 = np.abs(np.einsum("eki,ei->ek", J, xs) + b - t + rho[:, None] * lam)
    S2 = (np.einsum("eki,ei->ek", np.abs(J), np.abs(xf)) + np.einsum("eki,eli,el->ek", np.abs(J), np.abs(JM), np.abs(lam)) + np.abs(b) + np.abs(t)
          + np.einsum("ekl,el->ek", np.abs(G), np.abs(lam)) + rho[:, None] * np.abs(lam))
    con = res2.max(axis=1) / (C_BAR * (1 + S2.max(axis=1)))
    return dyn, con


def forward_error(x, x_ref):
    """per env: max|x - x_ref| / (1 + max|x_ref|)"""
    x = np.asarray(x, np.float64)
    return np.abs(x - x_ref).max(axis=1) / (1 + np.abs(x_ref).max(axis=1))


def regular(name, key, angular, damping=0.0, with_diag=False):
    """the class of a frame set, from the pivots of its UNDAMPED G_ref: True regular (every env's smallest relative pivot >= 1e-3), False dependent
    (every env's <= 1e-9); AssertionError in the gap.  `damping` is accepted and ignored: the class is the set's."""
    p = pivots(name, key, angular, with_diag, 0.0)
    if p.min() >= 1e-3:
        return True
    assert p.max() <= 1e-9, (name, key, angular, p.min(), p.max())
    return False


def solvable(name, key, angular, damping):
    """status 0 is expected on every env: a regular set, or any set with damping (its pivots are then >= damping / (1 + damping) of their entries)"""
    return damping > 0 or regular(name, key, angular)
