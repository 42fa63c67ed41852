"""The step's impulse balance: the fp64 reference, the contact-record laws and the populations that the CPU tests (tests/test_step_balance_reference.py)
and the GPU tests (tests/test_gpu_step_balance.py) share.  No test lives here; all of it is fp64 numpy over the Oracle bindings.

One statement holds for whatever iterate a contact solve returns, converged or not: the velocity the step returns is the one its own reported impulses
produce (oracle/rsb_oracle.c, step_impl, read backwards):
    A (u+ - u) = dt (tau - h) + sum_k J_k^T lam_k + (one unreported scalar per joint outside its range, on that joint's row only)
    A = M(q) + diag(B),   B_d = dt (kd_d + dt kp_d) for a PD joint whose torque is not effort-clipped, else 0
tau is Oracle.actuation, M, h and J are the oracle's queries; lam_k, the position and the body come from the contact records of the step under test, the
two entries of a self-collision both enter the sum.  No contact solver and no sweep count appears in it.

balance() states it per env; record_laws() the laws every contact record obeys by construction; CASES names the populations and case() builds one, once."""
import functools
from types import SimpleNamespace

import numpy as np

from common import Oracle, f32, standing_states
from raisimlib_amd import Model, rsc_path, workload

SELF_A, SELF_B = 0x10000, 0x20000
C_STEP = 2e-4            # the project's one-step bar (header of tests/test_gpu_parity.py), in velocity space
STOP_MARGIN = 1e-5       # no drawn joint lies this close to a stop: which side it is on does not depend on the number format


# ------------------------------------------------------------------------------------------------------------------------------ the balance
def body_pose(o, q, b):
    """(r, R): world position of body b's origin and its rotation, from point_jacobian at the origin and the three unit offsets"""
    r, _ = o.point_jacobian(q, b, np.zeros(3))
    R = np.stack([o.point_jacobian(q, b, e)[0] - r for e in np.eye(3)], axis=1)
    return r, R


def record_jacobians(o, q, con):
    """[J_k] (3 x nv each): Oracle.point_jacobian of the record's body at the body-local image of the record's world position"""
    poses, out = {}, []
    for c in con:
        b = int(c["body"])
        if b not in poses:
            poses[b] = body_pose(o, q, b)
        r, R = poses[b]
        out.append(o.point_jacobian(q, b, R.T @ (np.asarray(c["position"], np.float64) - r))[1])
    return out


def joint_ranges(blob):
    lo = np.array([blob.q_lower[i] for i in range(1, blob.nb)], np.float64)
    hi = np.array([blob.q_upper[i] for i in range(1, blob.nb)], np.float64)
    return lo, hi


def pd_diagonal(o, q, u, kp, kd, pt, dtg, tau_ff=None):
    """(B [nv], clipped [nv] bool): the implicit PD's joint-space inertia dt (kd + dt kp), zero on an effort-clipped joint (a constant torque source) and
    without a PD controller (FORCE_AND_TORQUE)"""
    blob, dt, nv = o.blob, o.p.dt, o.nv
    eff = np.array([blob.effort[i] for i in range(1, blob.nb)], np.float64)
    t = np.zeros(nv - 6) if tau_ff is None else np.array(tau_ff[6:], np.float64)
    B = np.zeros(nv)
    if o.p.control_mode == 1 and kp is not None and kd is not None:
        t = t + kp[6:] * (pt[7:] - q[7:] - dt * u[6:]) + kd[6:] * (dtg[6:] - u[6:])
        B[6:] = dt * (kd[6:] + dt * kp[6:])
    clipped = np.zeros(nv, bool)
    clipped[6:] = (eff > 0) & (np.abs(t) > eff)
    B[clipped] = 0.0
    return B, clipped


def balance_env(o, q0, u0, u1, con, kp, kd, pt, dtg, tau_ff=None, bdiag=None):
    """One env of balance(); con: its contact records (a structured array cut to its count).  bdiag replaces B (the sensitivity tests)."""
    blob, dt, nv = o.blob, o.p.dt, o.nv
    fixed = bool(blob.fixed_base)
    j0 = 6 if fixed else 0
    q0, u0, u1 = np.array(q0, np.float64), np.array(u0, np.float64), np.array(u1, np.float64)
    if fixed:
        u0[:6] = 0.0
    B, clipped = pd_diagonal(o, q0, u0, kp, kd, pt, dtg, tau_ff)
    if bdiag is not None:
        B = np.asarray(bdiag, np.float64)
    A = (o.mass_matrix(q0) + np.diag(B))[j0:, j0:]
    drive = dt * (o.actuation(q0, u0, kp, kd, pt, dtg, tau_ff) - o.nonlinearities(q0, u0))[j0:]
    du = (u1 - u0)[j0:]
    imp = [J[:, j0:].T @ np.asarray(c["impulse"], np.float64) for J, c in zip(record_jacobians(o, q0, con), con)]
    b = drive + (np.sum(imp, axis=0) if imp else 0.0)
    r = A @ du - b
    S = np.abs(A) @ np.abs(du) + np.abs(drive) + (np.sum(np.abs(imp), axis=0) if imp else 0.0)   # (per row: |A||du| + |dt (tau - h)| + sum |J^T lam|)
    lo, hi = joint_ranges(blob)
    qj = q0[7:]
    below, above = (lo < hi) & (qj < lo), (lo < hi) & (qj > hi)
    row = np.nonzero(below | above)[0] + 6 - j0                      # rows of L in the block
    sign = np.where(below, 1.0, -1.0)[below | above]
    r0 = r.copy()
    r0[row] = 0.0
    Ai = np.linalg.inv(A)
    delta = Ai @ r0
    U = max(np.abs(u0[j0:]).max(initial=0), np.abs(u1[j0:]).max(initial=0), np.abs(Ai @ drive).max(initial=0),
            np.sum([np.abs(Ai @ x) for x in imp], axis=0).max(initial=0) if imp else 0.0)
    return SimpleNamespace(r=r, r0=r0, S=S, delta=delta, dmax=float(np.abs(delta).max(initial=0)), U=float(U), x=Ai @ b, A=A, b=b,
                           lim_row=row, lim_sr=sign * r[row], lim_rowsum=np.abs(A[row]).sum(axis=1), lim_S=S[row],
                           limited=len(row) > 0, clipped=bool(clipped.any()), clipped_dofs=np.nonzero(clipped)[0],
                           r0_rel=float((np.abs(r0) / np.maximum(S, 1e-300)).max(initial=0)), u_inf=float(np.abs(u0[j0:]).max(initial=0)))


def balance(o, q0, u0, u1, contacts, kp, kd, pt, dtg, tau_ff=None):
    """Per env (a list of namespaces; contacts: per env its records, cut to its count):
      r        = A (u1 - u0) - b, b = dt (tau - h) + sum J_k^T lam_k; the joint block and rows of a fixed base, u0[:6] taken as zero
      lim_row  = L, the rows of the joints with lower < upper whose q0 lies outside the range (compared in float64, the blob's own type)
      r0       = r with the rows of L zeroed;  S the row's sum of absolute terms;  r0_rel = max |r0| / S
      delta    = A^-1 r0: the velocity the unexplained generalised impulse would produce;  dmax = |delta|_inf
      U        = max(|u0|, |u1|, |A^-1 dt (tau - h)|, sum_k |A^-1 J_k^T lam_k|)_inf
      lim_sr   = s_j r_j per joint of L, s = +1 below the lower stop and -1 above the upper one;  lim_rowsum = sum_k |A_jk|"""
    N = len(q0)
    kp = None if kp is None else np.asarray(kp, np.float64)
    kd = None if kd is None else np.asarray(kd, np.float64)
    return [balance_env(o, q0[e], u0[e], u1[e], contacts[e], kp, kd, np.asarray(pt[e], np.float64), np.asarray(dtg[e], np.float64),
                        None if tau_ff is None else np.asarray(tau_ff[e], np.float64)) for e in range(N)]


def assert_no_joint_at_a_stop(blob, q0):
    lo, hi = joint_ranges(blob)
    ranged = lo < hi
    qj = np.asarray(q0, np.float64)[:, 7:][:, ranged]
    gap = np.minimum(np.abs(qj - lo[ranged]), np.abs(qj - hi[ranged])).min(initial=1.0)
    assert gap > STOP_MARGIN, f"a joint lies {gap:.1e} from a stop"


# ------------------------------------------------------------------------------------------------------------------------------ record laws
LAWS = ("normal", "unilateral", "cone", "body", "count", "pair")


def record_laws(contacts, counts, mu_of, n_bodies, kmax):
    """Per env the worst violation of each law of a contact list (0: none), {law: [N]}:
      normal      ||normal| - 1| beyond 1e-6
      unilateral  -(lam . n) where negative
      cone        |lam - (lam . n) n| beyond mu (lam . n)(1 + 1e-4) + 1e-7 (test_contacts_report's numbers, along the record's normal);
                  mu = mu_of(primitive, -1) against the terrain, mu_of(primitive of SELF_A, primitive of SELF_B) for a self-collision
      body        1 per record whose body index lies outside the model
      count       count beyond kmax (or below 0)
      pair        1 per SELF_A record not followed by its SELF_B - same position and depth, opposite normal and impulse, bit for bit - and per SELF_B
                  record that follows no SELF_A"""
    N = len(counts)
    out = {k: np.zeros(N) for k in LAWS}
    for e in range(N):
        n = int(counts[e])
        out["count"][e] = max(0, n - kmax, -n)
        con = contacts[e][:max(0, min(n, kmax))]
        k = 0
        while k < len(con):
            c = con[k]
            code = int(c["collision"])
            nrm, lam = np.asarray(c["normal"], np.float64), np.asarray(c["impulse"], np.float64)
            prim_b = -1
            if code & SELF_B:
                out["pair"][e] += 1
            if code & SELF_A:
                ok = k + 1 < len(con) and (int(con[k + 1]["collision"]) & SELF_B) != 0
                if ok:
                    d = con[k + 1]
                    ok = (np.array_equal(c["position"], d["position"]) and c["depth"] == d["depth"]
                          and np.array_equal(-np.asarray(c["normal"]), d["normal"]) and np.array_equal(-np.asarray(c["impulse"]), d["impulse"]))
                    prim_b = int(d["collision"]) & 0xffff
                    if not 0 <= int(d["body"]) < n_bodies:
                        out["body"][e] += 1
                if not ok:
                    out["pair"][e] += 1
            if not 0 <= int(c["body"]) < n_bodies:
                out["body"][e] += 1
            out["normal"][e] = max(out["normal"][e], abs(np.linalg.norm(nrm) - 1.0) - 1e-6)
            ln = lam @ nrm
            out["unilateral"][e] = max(out["unilateral"][e], -ln)
            mu = mu_of(code & 0xffff, prim_b)
            out["cone"][e] = max(out["cone"][e], np.linalg.norm(lam - ln * nrm) - (mu * ln * (1 + 1e-4) + 1e-7))
            k += 2 if (code & SELF_A) and prim_b >= 0 else 1
    return out


def material_lookup(o, default_mu, col_mu=None, self_mu=None):
    """mu_of for record_laws: the primitive's material against the terrain, the pair's for a self-collision, else the world's default"""
    pairs = {(int(i), int(j)): k for k, (i, j) in enumerate(o.self_pairs())} if self_mu is not None else {}

    def mu_of(a, b):
        if b >= 0:
            return default_mu if self_mu is None else float(self_mu[pairs[(min(a, b), max(a, b))]])
        return default_mu if col_mu is None else float(col_mu[a])
    return mu_of


def normal_velocities(o, q0, u1, con, prim_ok=None):
    """(v_n+, lam_n) of the terrain contacts of one env: v_n+ = n . J u1 (erp 0), lam_n = lam . n; prim_ok [ncol] bool: only the contacts of these
    collision primitives (those without restitution, where a population has some)"""
    keep = [k for k, c in enumerate(con) if not int(c["collision"]) & (SELF_A | SELF_B) and (prim_ok is None or prim_ok[int(c["collision"]) & 0xffff])]
    J = record_jacobians(o, q0, con[keep])
    u1 = np.asarray(u1, np.float64)
    vn = np.array([np.asarray(con[k]["normal"], np.float64) @ (Jk @ u1) for k, Jk in zip(keep, J)])
    ln = np.array([np.asarray(con[k]["normal"], np.float64) @ np.asarray(con[k]["impulse"], np.float64) for k in keep])
    return vn, ln


def normal_figure(o, q0, u1, contacts, counts, select, prim_ok=None):
    """(worst of -v_n+ and of v_n+ where lam_n > 0, number of contacts) over the terrain contacts of the selected envs: how far a solve that met its exit
    test is from v_n+ >= 0, lam_n v_n+ = 0"""
    worst, n = 0.0, 0
    for e in np.nonzero(select)[0]:
        vn, ln = normal_velocities(o, q0[e], u1[e], contacts[e][:counts[e]], prim_ok)
        n += len(vn)
        worst = max(worst, (-vn).max(initial=0), vn[ln > 0].max(initial=0))
    return worst, n


def normal_bar(o, figure):
    """T of a population: 4 x the larger of the oracle's own figure on its converged envs and the solver's exit threshold (the figure follows from that
    threshold and, for a fixed base or a limit row, from the compliance of the block; below the threshold the oracle's figure measures nothing the
    fp32 solve is held to: on the quadruped's standing populations the fp64 figure is 2e-8 .. 2e-7 and a correct fp32 solve that met the same exit test
    ends at 4e-7 .. 6e-7).  Where the oracle's figure lies below the threshold - most quadruped populations - T is 4e-5 and the device's figures sit
    10 to 100 times below it: the law has little bite there and more on the fixed bases and the tight knees, whose T comes from the figure."""
    return 4.0 * max(figure, o.p.threshold)


# ------------------------------------------------------------------------------------------------------------------------------ populations
def _fuzz_gains(rng, nv):
    kp = np.zeros(nv, np.float32); kd = np.zeros(nv, np.float32)
    kp[6:] = rng.uniform(0, 60, nv - 6); kd[6:] = rng.uniform(0, 1.0, nv - 6)
    return kp, kd


def _case(name, model, gc, gv, pt, kp, kd, **kw):
    """One population: float32-rounded states and targets (what the device receives), held in float64; `settings` is what the world and the oracle are
    both set to (make_oracle here, the GPU tests' make_world)."""
    N = len(gc)
    c = SimpleNamespace(name=name, model=model, N=N, gc=f32(gc), gv=f32(gv), pt=f32(pt), dtg=np.zeros((N, model.nv)), kp=np.asarray(kp, np.float32),
                        kd=np.asarray(kd, np.float32), tau_ff=None, mode=1, kmax=8, lpe=0, ground=None, heightmap=None, materials=None, mu=0.8,
                        slip_rule=0, scheme="semi_implicit", theta=1.0, recipe=None, warm=False)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    if c.tau_ff is not None:
        c.tau_ff = f32(c.tau_ff)
    return c


def make_oracle(c):
    o = Oracle(c.model.blob)
    o.p.kmax, o.p.control_mode, o.p.mu, o.p.slip_rule, o.p.integ_theta = c.kmax, c.mode, c.mu, c.slip_rule, c.theta
    if c.recipe is not None:
        c.recipe.setup_oracle(o, c.N, 0)
    if c.ground is not None:
        o.set_ground(c.ground)
    if c.heightmap is not None:
        o.set_heightmap(*c.heightmap)
    if c.materials is not None:
        o.set_collision_materials(*c.materials)
    return o


def oracle_step(c, substeps=1, q=None, u=None, warm=None):
    o = make_oracle(c)
    ref = o.step_batch(c.gc if q is None else q, c.gv if u is None else u, substeps, c.kp.astype(np.float64), c.kd.astype(np.float64), c.pt, c.dtg,
                       c.tau_ff, want_contacts=True, lam_warm=o.new_warm_state(c.N) if warm is None else warm)
    return o, ref


def fuzz_floating(seed, N=128):
    """tests/test_gpu_fuzz.py::test_random_tree_one_step_parity[seed], redrawn with the same seed and draws"""
    from test_gpu_fuzz import random_urdf
    rng = np.random.default_rng(1000 + seed)
    model = Model(urdf_string=random_urdf(rng, int(rng.integers(2, 11))))
    nq, nv = model.nq, model.nv
    kmax = 16 if model.ncol > 8 else 8
    gc = np.zeros((N, nq)); gc[:, 0:2] = rng.uniform(-1, 1, (N, 2)); gc[:, 2] = rng.uniform(0.0, 0.5, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.5, 0.5, (N, nq - 7))
    gv = rng.normal(size=(N, nv)) * 1.0
    kp, kd = _fuzz_gains(rng, nv)
    pt = gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (N, nq - 7))
    mu = float(rng.choice([0.3, 0.8, 1.2]))
    return _case(f"fuzz floating {seed}", model, gc, gv, pt, kp, kd, kmax=kmax, mu=mu)


def fuzz_fixed(seed, N=128):
    """tests/test_gpu_fuzz.py::test_random_fixed_base_tree_parity[seed]: the ground at -0.25, 16 slots"""
    from test_gpu_fuzz import random_urdf
    rng = np.random.default_rng(4000 + seed)
    model = Model(urdf_string=random_urdf(rng, int(rng.integers(3, 9))).replace('"l0"', '"world"'))
    assert model.blob.fixed_base == 1
    nq, nv = model.nq, model.nv
    gc = np.zeros((N, nq)); gc[:, 3] = 1.0
    gc[:, 7:] = rng.uniform(-1.5, 1.5, (N, nq - 7))
    gv = np.zeros((N, nv)); gv[:, 6:] = rng.normal(size=(N, nv - 6))
    kp, kd = _fuzz_gains(rng, nv)
    pt = gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (N, nq - 7))
    return _case(f"fuzz fixed {seed}", model, gc, gv, pt, kp, kd, kmax=16, ground=-0.25)


def fuzz_heightmap(seed, N=128):
    """The models and terrains of tests/test_gpu_fuzz.py::test_random_tree_three_substeps_on_a_height_map[seed] and its order of draws, but NOT its
    population: N envs instead of its 96 (so every draw after the model differs), and a joint drawn within 1e-4 of a stop is moved to 1e-4 from it on the
    side it is on (seed 2 draws one 8e-6 from a stop, where float32 and float64 could rank it differently)."""
    from raisimlib_amd.world import heightmap_perlin
    from test_gpu_fuzz import random_urdf
    rng = np.random.default_rng(2000 + seed)
    model = Model(urdf_string=random_urdf(rng, int(rng.integers(3, 9))))
    nq, nv = model.nq, model.nv
    kmax = 16 if model.ncol > 8 else 8
    H = heightmap_perlin(48, 48, 4.8, 4.8, frequency=0.6, z_scale=0.2, seed=int(rng.integers(1, 1000)))
    gc = np.zeros((N, nq)); gc[:, 0:2] = rng.uniform(-1.5, 1.5, (N, 2)); gc[:, 2] = rng.uniform(0.0, 0.5, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.4, 0.4, (N, nq - 7))
    lo, hi = joint_ranges(model.blob)
    for stop in (lo, hi):       # (seed 2 draws a joint 8e-6 from a stop: a joint within 1e-4 of one is put 1e-4 from it, on the side it is on)
        near = (np.abs(gc[:, 7:] - stop) < 1e-4) & (lo < hi)
        gc[:, 7:] = np.where(near, stop + np.where(gc[:, 7:] < stop, -1e-4, 1e-4), gc[:, 7:])
    gv = rng.normal(size=(N, nv)) * 0.5
    kp = np.zeros(nv, np.float32); kd = np.zeros(nv, np.float32); kp[6:] = 30.0; kd[6:] = 0.5
    return _case(f"fuzz height map {seed}", model, gc, gv, gc, kp, kd, kmax=kmax, heightmap=(48, 48, 4.8, 4.8, 0.0, 0.0, H))


def tree17(N=67):
    """a 17-link tree of the fuzz generator (past the 16-body instantiation of the step kernel's classes), the floating fuzz draws, a ragged block"""
    from test_gpu_fuzz import random_urdf
    rng = np.random.default_rng(1700)
    model = Model(urdf_string=random_urdf(rng, 17))
    assert model.nb == 17
    nq, nv = model.nq, model.nv
    gc = np.zeros((N, nq)); gc[:, 0:2] = rng.uniform(-1, 1, (N, 2)); gc[:, 2] = rng.uniform(0.0, 0.5, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.5, 0.5, (N, nq - 7))
    gv = rng.normal(size=(N, nv))
    kp, kd = _fuzz_gains(rng, nv)
    pt = gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (N, nq - 7))
    return _case("17-link tree", model, gc, gv, pt, kp, kd, kmax=16)


@functools.lru_cache(maxsize=None)
def anymal():
    return Model(urdf_path=rsc_path("anymal_c_like.urdf"))


def anymal_standing(lpe, N=128):
    gc, gv = standing_states(N, seed=100 + lpe)
    kp, kd = workload.anymal_gains()
    pt = gc.copy()
    pt[:, 7:] = workload.ANYMAL_NOMINAL_JOINTS + np.random.default_rng(1).uniform(-0.3, 0.3, (N, 12))
    return _case(f"anymal standing, {lpe} lanes per env", anymal(), gc, gv, pt, kp, kd, lpe=lpe)


def anymal_sliding(rule, N=128):
    gc, gv = standing_states(N, seed=33, vel=1.5)
    kp, kd = workload.anymal_gains()
    return _case(f"anymal sliding, {rule} slip rule", anymal(), gc, gv, gc, kp, kd, slip_rule=1 if rule == "coulomb" else 0)


def anymal_tight_knees(N=128):
    """the model of tests/test_gpu_parity.py::test_joint_limit_rows_parity: knees and hips with a tight range, many joints past a stop"""
    import re
    txt = open(rsc_path("anymal_c_like.urdf")).read()
    tight = re.sub(r'(<joint name="[A-Z]{2}_KFE".*?)lower="-6.28" upper="6.28"', r'\1lower="-1.0" upper="1.0"', txt, flags=re.S)
    tight = re.sub(r'(<joint name="[A-Z]{2}_HFE".*?)lower="-6.28" upper="6.28"', r'\1lower="-0.5" upper="0.5"', tight, flags=re.S)
    model = Model(urdf_string=tight)
    gc, gv = standing_states(N, seed=77, z=(0.45, 0.9), vel=2.0)
    gc[:, 7:] += np.random.default_rng(2).uniform(-0.5, 0.5, (N, 12))
    kp, kd = workload.anymal_gains()
    return _case("anymal tight knees", model, gc, gv, gc, kp, kd)


def anymal_contorted(z, kmax, N=128):
    from test_gpu_parity import _contorted_states
    gc, gv = _contorted_states(N, 316, z)
    kp, kd = workload.anymal_gains()
    return _case(f"anymal contorted z {z[0]:g}, {kmax} slots", anymal(), gc, gv, gc, kp, kd, kmax=kmax)


def anymal_side(N=64):
    from test_gpu_solver_handover import SIDE_SEED, side_population
    gc, gv, pt, _, _ = side_population(anymal(), SIDE_SEED, N)
    kp, kd = workload.anymal_gains()
    return _case("anymal on its side", anymal(), gc, gv, pt, kp, kd)


def anymal_materials(N=128):
    """per-primitive materials with restitution (tests/test_gpu_parity.py::test_per_primitive_materials_parity)"""
    m = anymal()
    rng = np.random.default_rng(5)
    mats = (rng.uniform(0.2, 1.3, m.ncol), rng.uniform(0.0, 0.6, m.ncol) * (rng.random(m.ncol) < 0.5), rng.uniform(0.0, 0.3, m.ncol))
    gc, gv = standing_states(N, seed=77, vel=1.0)
    kp, kd = workload.anymal_gains()
    return _case("anymal per-primitive materials", m, gc, gv, gc, kp, kd, materials=mats)


def anymal_torque(N=128):
    """FORCE_AND_TORQUE with random feed-forward, near the ground"""
    gc, gv = standing_states(N, seed=13)
    tau = np.random.default_rng(0).normal(size=(N, 18)) * 5
    kp, kd = workload.anymal_gains()
    return _case("anymal force and torque", anymal(), gc, gv, gc, kp, kd, tau_ff=tau, mode=0)


def anymal_clipped(N=128):
    """PD targets 1.5 rad from the state on about half of the joints, gains doubled: kp 100 x 1.5 = 150 N m against the 80 N m effort limit - every env
    holds clipped joints (constant torque sources, B = 0) beside PD joints (B on)"""
    gc, gv = standing_states(N, seed=41, vel=2.0)
    rng = np.random.default_rng(42)
    pt = gc.copy(); pt[:, 7:] += 1.5 * np.where(rng.random((N, 12)) < 0.5, -1.0, 1.0) * (rng.random((N, 12)) < 0.5)
    kp, kd = workload.anymal_gains()
    return _case("anymal clipped effort", anymal(), gc, gv, pt, 2.0 * kp, kd)


def anymal_scheme(scheme, N=128):
    gc, gv = standing_states(N, seed=5, z=(0.45, 0.6), vel=0.5)
    kp, kd = workload.anymal_gains()
    return _case(f"anymal {scheme}", anymal(), gc, gv, gc, kp, kd, scheme=scheme, theta={"euler": 0.0, "trapezoid": 0.5}[scheme])


def atlas(regime, N=32, preroll=6):
    """bench.Recipe(5, ..., regime), the recipe of tests/test_gpu_configs35.py - a relative of that file's populations, not the same one: there the device
    rolls 4096 envs through the benchmark loop, resets included, into its stationary mix; here the recipe's initial population is rolled `preroll` control
    steps forward by the ORACLE (a CPU-only definition both test files share): feet loaded, the collapsing regime on its way down, nobody reset, no joint
    past a stop and hardly an unconverged env.  The recipe's settings (16 slots, multi-contact depth 2, the Anderson step) on both sides."""
    import sys
    from common import ROOT
    sys.path.insert(0, ROOT)
    import bench
    recipe = bench.Recipe(5, -1.0, regime)
    gc, gv = recipe.initial_state(N, 0)
    c = _case(f"atlas {regime}", recipe.model, gc, gv, recipe.targets(N, 0, 0), recipe.kp, recipe.kd, kmax=recipe.kmax, recipe=recipe)
    o = make_oracle(c)
    q, u, warm = c.gc, c.gv, o.new_warm_state(N)
    for k in range(preroll):
        r = o.step_batch(q, u, workload.SUBSTEPS, c.kp.astype(np.float64), c.kd.astype(np.float64), f32(recipe.targets(N, k, 0)), c.dtg, lam_warm=warm)
        q, u = r["q"], r["u"]
    c.gc, c.gv, c.pt = f32(q), f32(u), f32(recipe.targets(N, preroll, 0))
    return c


CASES = {}
for _s in range(12):
    CASES[f"fuzz_floating{_s}"] = functools.partial(fuzz_floating, _s)
for _s in range(6):
    CASES[f"fuzz_fixed{_s}"] = functools.partial(fuzz_fixed, _s)
for _s in range(3):
    CASES[f"fuzz_heightmap{_s}"] = functools.partial(fuzz_heightmap, _s)
CASES["tree17"] = tree17
for _l in (16, 32, 64):
    CASES[f"anymal_standing_lpe{_l}"] = functools.partial(anymal_standing, _l)
CASES["anymal_standing_ragged"] = functools.partial(anymal_standing, 16, 67)
for _r in ("energy", "coulomb"):
    CASES[f"anymal_sliding_{_r}"] = functools.partial(anymal_sliding, _r)
CASES["anymal_tight_knees"] = anymal_tight_knees
for _z, _t in (((2.0, 2.1), "air"), ((0.25, 0.5), "ground")):
    for _k in (8, 16):
        CASES[f"anymal_contorted_{_t}_k{_k}"] = functools.partial(anymal_contorted, _z, _k)
CASES["anymal_side"] = anymal_side
CASES["anymal_materials"] = anymal_materials
CASES["anymal_torque"] = anymal_torque
CASES["anymal_clipped"] = anymal_clipped
for _sch in ("euler", "trapezoid"):
    CASES[f"anymal_{_sch}"] = functools.partial(anymal_scheme, _sch)
for _reg in ("standing", "collapsing"):
    CASES[f"atlas_{_reg}"] = functools.partial(atlas, _reg)
WARM_CASES = ["anymal_standing_lpe16", "fuzz_fixed3", "atlas_standing"]      # integrate(3), get_state(), integrate(1): the last step, warm-started


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def mu_of_case(c, o):
    return material_lookup(o, c.mu, None if c.materials is None else c.materials[0])


def law_primitives(c):
    """the collision primitives whose terrain contacts are held to v_n+ = 0: all (None), or those without restitution where a population has materials"""
    return None if c.materials is None else np.asarray(c.materials[1]) == 0.0
