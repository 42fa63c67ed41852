"""What the inverse-kinematics tests share (rsb_inverse_kinematics; include/rsb.h): the variants, reachable targets, the fp64 evaluation of a result and
a restatement of the device's iteration in numpy float32.  No test lives here; tests/test_ik_reference.py (CPU) and tests/test_gpu_ik.py use it.

Cases: floating0, fixed2 (N = 67), anymal, atlas (N = 64) of test_dynamics_reference.dyn_case, EVERY env.  variants(case) lists (frame set, angular,
base free); the row counts m = kF cover the kernel's branches: 3 and 12 (a 16-lane group), 6 and 24 with angular rows (16 / 32 lanes), 36 (64 lanes)
and 72, 96 (64 lanes, a lane owns two rows).  Several frames may sit on one body: the row count is what matters.  Every set runs with the base held
(dof_mask None) and, on a floating base, with every coordinate free.

Targets are REACHABLE BY CONSTRUCTION: the fp64 forward kinematics (test_dynamics_reference.kinematics) of start (+) delta, start the case's
float32 states, delta uniform in +-0.3 rad on the free revolute joints and the base rotation and +-0.1 m on the free prismatic joints and the base
position, times DELTA's scale for the variant (1.0 unless listed there), rounded to float32.  (+) is the device's: joints and base origin add, the base
quaternion is multiplied on the left by exp(delta[3:6]).

evaluate() is the yardstick: positions and rotation rows of a float32 gc in fp64.  restate() is the device's iteration step by step in float32, all
envs at once (an env that has stopped is frozen): sums over Jacobian columns and rows in ascending order, the left-looking root-free Cholesky with the
pivot rule, the two substitutions, the clip, the update.  Libm and fused multiply-adds differ from the device's, so it is a restatement of the
arithmetic, not of the bits: the tests compare iteration counts and residuals.  Its three `wrong` modes break one convention each."""
import functools
from types import SimpleNamespace

import numpy as np

from test_dynamics_reference import dyn_case, kinematics
import inverse_mass_reference as imr

CASES = ["floating0", "fixed2", "anymal", "atlas"]
MAX_ITER, DAMPING, MAX_STEP, POS_TOL, ROT_TOL = 30, 1e-3, 0.5, 1e-4, 1e-4      # what the GPU tests run with
CONVERGED, MAX_ITER_STATUS, SINGULAR = 0, 1, 2
PIVOT_TOL = np.float32(1e-5)      # RSB_HELD_PIVOT_TOL
POS_BAR, ROT_BAR = 1e-5, 6e-5     # the frame-position bar of tests/test_gpu_frames.py; 2e-5 per entry of R through the three-term sums of R_t R^T
# (case, frame set, angular, base free) -> scale of delta, where 1.0 does not meet the convergence condition of tests/test_ik_reference.py: with
# orientation rows some directions of J J^T lie below rho = 1e-3 max diag and shrink by rho / (sigma^2 + rho) per step only.  At 1.0 the restatement
# left 5, 21, 0 (16 steps), 38, 45, 2 and 7 envs of these seven short of the tolerances after 30 steps; at the scales below it needs 9, 7, 9, 9, 10, 3, 5.
DELTA = {("anymal", "feet", True, True): 0.1, ("atlas", "limbs", True, False): 0.03, ("atlas", "limbs", True, True): 0.1, ("atlas", "six", True, False): 0.03,
         ("atlas", "six", True, True): 0.03, ("atlas", "twelve", True, False): 0.03, ("atlas", "twelve", True, True): 0.03}

F32 = np.float32


def _f32_frames(frames):
    return [(int(b), tuple(float(F32(x)) for x in off)) for b, off in frames]


@functools.lru_cache(maxsize=None)
def frame_sets(name):
    c = dyn_case(name)
    rng = np.random.default_rng(5200 + c.nb)
    last = c.nb - 1
    spread = lambda n: _f32_frames([(int(b), rng.uniform(-0.2, 0.2, 3)) for b in np.linspace(1, last, n).round().astype(int)])
    sets = {"one": _f32_frames(c.frames[:1])}
    if name == "anymal":
        sets["feet"] = imr.frame_sets(name)["feet"]
    if name == "atlas":
        sets["limbs"] = _f32_frames([(b, rng.uniform(-0.1, 0.1, 3)) for b in (11, 18, 24, 30)])      # hands and feet
        sets["six"] = spread(6)
        sets["twelve"] = spread(12)
    if name == "floating0":
        sets["sixteen"] = spread(16)
    return sets


_SETS = {      # (frame set, angular): m
    "floating0": [("one", False), ("one", True), ("sixteen", True)],                        # 3 6 96
    "fixed2": [("one", False), ("one", True)],                                              # 3 6
    "anymal": [("one", False), ("feet", False), ("feet", True)],                            # 3 12 24
    "atlas": [("limbs", False), ("limbs", True), ("six", True), ("twelve", True)],          # 12 24 36 72
}


def variants(name):
    """[(frame set, angular, base free)]"""
    c = dyn_case(name)
    return [(key, ang, free) for key, ang in _SETS[name] for free in ((False,) if c.fixed else (False, True))]


def rows_of(name, key, angular):
    return (6 if angular else 3) * len(frame_sets(name)[key])


def dof_mask(name, base_free):
    """None (the joints, base held) or the all-ones mask"""
    return np.ones(dyn_case(name).nv, np.uint8) if base_free else None


def free_columns(name, base_free):
    c = dyn_case(name)
    free = np.ones(c.nv, bool)
    free[:6] = base_free and not c.fixed
    return free


# ------------------------------------------------------------------------------------------------------------------------------ fp64
def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_exp(w):
    ph = np.linalg.norm(w)
    return np.array([1.0, *(0.5 * w)]) if ph <= 1e-12 else np.array([np.cos(0.5 * ph), *(np.sin(0.5 * ph) / ph * w)])


def plus(q, d):
    """q (+) d in fp64, d in gv's coordinates"""
    out = np.array(q, float)
    out[:3] += d[:3]
    qt = quat_mul(quat_exp(d[3:6]), out[3:7] / np.linalg.norm(out[3:7]))
    out[3:7] = qt / np.linalg.norm(qt)
    out[7:] += d[6:]
    return out


def rot_vector(S):
    """the world-frame rotation vector of S, the formulas of rsb.h"""
    v = 0.5 * np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])
    n, cs = np.linalg.norm(v), 0.5 * (np.trace(S) - 1.0)
    return v * (np.arctan2(n, cs) / n) if n > 1e-6 else v


def forward(blob, q, frames):
    """fp64: positions [F, 3] and rotations [F, 3, 3] of the frames at q"""
    k = kinematics(blob, np.asarray(q, float))
    return (np.array([k.p[b] + k.R[b] @ np.asarray(off, float) for b, off in frames]), np.array([k.R[b] for b, _ in frames]))


@functools.lru_cache(maxsize=None)
def problem(name, key, angular, base_free):
    """start [N, nq] float32 (the case's states), target_pos [N, F, 3] and target_rot [N, F, 9] float32 (None without angular)"""
    c, frames = dyn_case(name), frame_sets(name)[key]
    free = free_columns(name, base_free)
    scale = DELTA.get((name, key, angular, base_free), 1.0)
    rng = np.random.default_rng(6100 + 100 * CASES.index(name) + 4 * len(frames) + 2 * angular + base_free)
    start = np.ascontiguousarray(c.gc, F32)
    tp, tr = np.zeros((c.N, len(frames), 3)), np.zeros((c.N, len(frames), 9))
    for e in range(c.N):
        d = np.zeros(c.nv)
        d[:3] = rng.uniform(-0.1, 0.1, 3); d[3:6] = rng.uniform(-0.3, 0.3, 3)
        for i in range(1, c.nb):
            d[5 + i] = rng.uniform(-0.3, 0.3) if c.blob.jtype[i] == 1 else rng.uniform(-0.1, 0.1)
        d *= scale * free
        p, R = forward(c.blob, plus(start[e].astype(float), d), frames)
        tp[e], tr[e] = p, R.reshape(len(frames), 9)
    return SimpleNamespace(start=start, target_pos=np.ascontiguousarray(tp, F32), target_rot=np.ascontiguousarray(tr, F32) if angular else None)


def evaluate(name, key, gc, target_pos, target_rot=None):
    """fp64 at the float32 gc [n, nq] -> (largest |position row| [n], largest |rotation row| [n] (zeros without target_rot), largest |target| [n])"""
    c, frames = dyn_case(name), frame_sets(name)[key]
    n = len(gc)
    ep, er = np.zeros(n), np.zeros(n)
    tp = np.asarray(target_pos, float).reshape(n, len(frames), 3)
    for e in range(n):
        p, R = forward(c.blob, gc[e], frames)
        ep[e] = np.abs(tp[e] - p).max()
        if target_rot is not None:
            Rt = np.asarray(target_rot[e], float).reshape(len(frames), 3, 3)
            er[e] = max(np.abs(rot_vector(Rt[f] @ R[f].T)).max() for f in range(len(frames)))
    return ep, er, np.abs(tp).reshape(n, -1).max(axis=1)


def bars(tmax, angular):
    """the residual bars of tests/test_gpu_ik.py, per env: (position, rotation)"""
    return POS_TOL + POS_BAR * (1 + tmax), (ROT_TOL + ROT_BAR) * np.ones_like(tmax) if angular else np.zeros_like(tmax)


# ------------------------------------------------------------------------------------------------------------------------------ float32
def _kin32(blob, q):
    """float32 kinematics of all envs at once, walk_chain's formulas: R [nb][N,3,3], p [nb][N,3], a [nb][N,3]"""
    N = len(q)
    qt = q[:, 3:7]
    inn = F32(1) / np.sqrt((qt * qt).sum(axis=1, dtype=F32))
    w, x, y, z = (qt * inn[:, None]).T
    R0 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).astype(F32).reshape(N, 3, 3)
    R, p, a = [R0], [q[:, :3].copy()], [np.zeros((N, 3), F32)]
    eye = np.eye(3, dtype=F32)
    for i in range(1, blob.nb):
        par = blob.parent[i]
        ax, Rt, pt = np.array(blob.axis[i][:], F32), np.array(blob.rtree[i][:], F32).reshape(3, 3), np.array(blob.ptree[i][:], F32)
        qi = q[:, 6 + i]
        d = R[par] @ pt
        if blob.jtype[i] == 1:
            sn, cs = np.sin(qi)[:, None, None], np.cos(qi)[:, None, None]
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], F32)
            Rq = cs * eye + (1 - cs) * np.outer(ax, ax).astype(F32) + sn * K
            Rn = R[par] @ (Rt @ Rq)
            an = Rn @ ax
        else:
            Rn = R[par] @ Rt
            an = Rn @ ax
            d = d + an * qi[:, None]
        R.append(Rn.astype(F32)); a.append(an.astype(F32)); p.append((p[par] + d).astype(F32))
    return R, p, a


def _rows32(R, p, frames, tp, tr, rot_sign):
    """e [N, m] and the frames' points [F][N, 3]"""
    kk = 6 if tr is not None else 3
    N = len(tp)
    e, pts = np.zeros((N, kk * len(frames)), F32), []
    for f, (b, off) in enumerate(frames):
        pt = p[b] + R[b] @ np.array(off, F32)
        pts.append(pt)
        e[:, kk * f:kk * f + 3] = tp[:, f] - pt
        if tr is not None:
            S = tr[:, f].reshape(N, 3, 3) @ R[b].transpose(0, 2, 1)
            v = F32(0.5) * np.stack([S[:, 2, 1] - S[:, 1, 2], S[:, 0, 2] - S[:, 2, 0], S[:, 1, 0] - S[:, 0, 1]], axis=1)
            n = np.sqrt((v * v).sum(axis=1, dtype=F32))
            cs = F32(0.5) * (S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2] - F32(1))
            with np.errstate(divide="ignore", invalid="ignore"):
                k = np.where(n > F32(1e-6), np.arctan2(n, cs) / n, F32(1)).astype(F32)
            e[:, kk * f + 3:kk * f + 6] = F32(rot_sign) * v * k[:, None]
    return e, pts


def _jac32(blob, fixed, p, a, frames, pts, kk, cols):
    """J [N, m, nv] float32, columns outside `cols` zero"""
    N, nv = len(pts[0]), 6 + blob.nb - 1
    J = np.zeros((N, kk * len(frames), nv), F32)
    for f, (b, _) in enumerate(frames):
        pt, r0 = pts[f], kk * f
        if not fixed:
            r = pt - p[0]
            J[:, r0 + 0, 0] = 1; J[:, r0 + 1, 1] = 1; J[:, r0 + 2, 2] = 1
            J[:, r0 + 0, 4] = r[:, 2]; J[:, r0 + 0, 5] = -r[:, 1]
            J[:, r0 + 1, 3] = -r[:, 2]; J[:, r0 + 1, 5] = r[:, 0]
            J[:, r0 + 2, 3] = r[:, 1]; J[:, r0 + 2, 4] = -r[:, 0]
            if kk == 6:
                J[:, r0 + 3, 3] = 1; J[:, r0 + 4, 4] = 1; J[:, r0 + 5, 5] = 1
        j = b
        while j >= 1:
            if blob.jtype[j] == 1:
                J[:, r0:r0 + 3, 5 + j] = np.cross(a[j], pt - p[j]).astype(F32)
                if kk == 6:
                    J[:, r0 + 3:r0 + 6, 5 + j] = a[j]
            else:
                J[:, r0:r0 + 3, 5 + j] = a[j]
            j = blob.parent[j]
    J[:, :, ~cols] = 0
    return J


def _solve32(J, e, damping):
    """y [N, m] of (J J^T + rho I) y = e by the device's root-free Cholesky, and bad [N]: a refused pivot or max diag = 0"""
    N, m, nv = J.shape
    A = np.zeros((N, m, m), F32)
    for d in range(nv):      # sums over the columns in ascending order
        A += J[:, :, d, None] * J[:, None, :, d]
    idx = np.arange(m)
    gmax = A[:, idx, idx].max(axis=1)
    rho = (F32(damping) * gmax).astype(F32)
    A[:, idx, idx] += rho[:, None]
    d0 = A[:, idx, idx].copy()
    W, iD = A, np.zeros((N, m), F32)
    bad = ~(gmax > 0)
    for j in range(m):
        s = W[:, j:, j].copy()
        for k in range(j):
            s -= W[:, j:, k] * W[:, j, k, None] * iD[:, k, None]
        W[:, j:, j] = s
        piv = s[:, 0]
        refused = ~(piv > PIVOT_TOL * d0[:, j]) | ~np.isfinite(piv)
        bad |= refused
        with np.errstate(divide="ignore", invalid="ignore"):
            iD[:, j] = np.where(refused, F32(0), F32(1) / piv)
    x = e.copy()
    for k in range(m - 1):
        yk = x[:, k] * iD[:, k]
        x[:, k + 1:] -= W[:, k + 1:, k] * yk[:, None]
    x *= iD
    for k in range(m - 1, 0, -1):
        x[:, :k] -= W[:, k, :k] * iD[:, :k] * x[:, k, None]
    return x, bad


def restate(name, key, start, target_pos, target_rot=None, mask=None, max_iter=MAX_ITER, damping=DAMPING, pos_tol=POS_TOL, rot_tol=ROT_TOL, max_step=MAX_STEP,
            wrong=None):
    """The device's iteration in numpy float32, all envs at once -> gc [N, nq] float32, error [N, 2], iterations [N], status [N].
    wrong: None, "rot_sign" (the rotation rows negated), "quat_right" (the base quaternion multiplied on the right), "unmasked" (the held columns
    stay in J; the update still moves the free coordinates only)."""
    c, frames = dyn_case(name), frame_sets(name)[key]
    blob, nv = c.blob, c.nv
    q = np.array(start, F32)
    N = len(q)
    tp = np.asarray(target_pos, F32).reshape(N, len(frames), 3)
    tr = None if target_rot is None else np.asarray(target_rot, F32).reshape(N, len(frames), 9)
    kk = 3 if tr is None else 6
    free = np.zeros(nv, bool)
    free[6:] = True
    if mask is not None:
        free = np.asarray(mask) != 0
    if c.fixed:
        free[:6] = False
    cols = np.ones(nv, bool) if wrong == "unmasked" else free
    if c.fixed:
        cols = cols.copy(); cols[:6] = False
    live = np.ones(N, bool)
    status, iters, err = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros((N, 2), F32)
    for it in range(max_iter + 1):
        R, p, a = _kin32(blob, q)
        e, pts = _rows32(R, p, frames, tp, tr, -1.0 if wrong == "rot_sign" else 1.0)
        pos = np.abs(e.reshape(N, len(frames), kk)[:, :, :3]).reshape(N, -1).max(axis=1)
        rot = np.abs(e.reshape(N, len(frames), kk)[:, :, 3:]).reshape(N, -1).max(axis=1) if kk == 6 else np.zeros(N, F32)
        err[live, 0], err[live, 1], iters[live] = pos[live], rot[live], it
        done = (pos <= F32(pos_tol)) & (rot <= F32(rot_tol))
        status[live & done] = CONVERGED
        if it == max_iter:
            status[live & ~done] = MAX_ITER_STATUS
            break
        live = live & ~done
        if not live.any():
            break
        J = _jac32(blob, c.fixed, p, a, frames, pts, kk, cols)
        y, bad = _solve32(J, e, damping)
        status[live & bad] = SINGULAR
        live = live & ~bad
        dq = np.zeros((N, nv), F32)
        for i in range(J.shape[1]):      # J^T y in row order
            dq += J[:, i, :] * y[:, i, None]
        s = np.abs(dq).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            sc = np.where(s > F32(max_step), F32(max_step) / s, F32(1)).astype(F32)
        dq = dq * sc[:, None]
        upd = q.copy()
        for d in np.flatnonzero(free):
            if d < 3:
                upd[:, d] = q[:, d] + dq[:, d]
            elif d >= 6:
                upd[:, d + 1] = q[:, d + 1] + dq[:, d]
        if free[3:6].any():
            w = dq[:, 3:6] * free[3:6].astype(F32)
            ph = np.sqrt((w * w).sum(axis=1, dtype=F32))
            with np.errstate(divide="ignore", invalid="ignore"):
                sh = np.where(ph > F32(1e-6), np.sin(F32(0.5) * ph) / ph, F32(0.5)).astype(F32)
            ew = np.where(ph > F32(1e-6), np.cos(F32(0.5) * ph), F32(1)).astype(F32)
            ex = (sh[:, None] * w).astype(F32)
            qn = q[:, 3:7] * (F32(1) / np.sqrt((q[:, 3:7] ** 2).sum(axis=1, dtype=F32)))[:, None]
            A_, B_ = (np.concatenate([ew[:, None], ex], axis=1), qn)
            if wrong == "quat_right":
                A_, B_ = B_, A_
            pq = np.stack([A_[:, 0] * B_[:, 0] - A_[:, 1] * B_[:, 1] - A_[:, 2] * B_[:, 2] - A_[:, 3] * B_[:, 3],
                           A_[:, 0] * B_[:, 1] + A_[:, 1] * B_[:, 0] + A_[:, 2] * B_[:, 3] - A_[:, 3] * B_[:, 2],
                           A_[:, 0] * B_[:, 2] - A_[:, 1] * B_[:, 3] + A_[:, 2] * B_[:, 0] + A_[:, 3] * B_[:, 1],
                           A_[:, 0] * B_[:, 3] + A_[:, 1] * B_[:, 2] - A_[:, 2] * B_[:, 1] + A_[:, 3] * B_[:, 0]], axis=1).astype(F32)
            upd[:, 3:7] = pq * (F32(1) / np.sqrt((pq * pq).sum(axis=1, dtype=F32)))[:, None]
        q[live] = upd[live]
    return q, err, iters, status


@functools.lru_cache(maxsize=None)
def restated(name, key, angular, base_free):
    """restate() on the variant's problem at the GPU tests' settings"""
    pr = problem(name, key, angular, base_free)
    return restate(name, key, pr.start, pr.target_pos, pr.target_rot, dof_mask(name, base_free))
