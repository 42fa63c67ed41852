"""The slow, accurate path beside the fused step kernel, on random trees and fixed bases: rsb_integrate1's query kernel (fp32 CRBA + RNEA, one thread
per env), rsb_get_mass_matrix / rsb_get_nonlinearities / rsb_get_inverse_mass_matrix, and IntegrationScheme::RUNGE_KUTTA_4, which is built on them.

Models: tests/test_gpu_fuzz.py's generator (revolute and prismatic joints, rotated joint frames, branching), post-processed here as a string: a
rotor_inertia on every other joint, the root renamed "world" for the fixed bases, and every joint's range opened to +-6 (the states below put joints
anywhere in +-1.2: a joint past a +-0.3 stop would bring the step kernel's limit rows into steps that are meant to be free motion).  Link counts are
listed, not drawn: 2 .. 17, both sides of the query kernel's 16-body instantiation.  N = 67 envs: one full 64-thread block and a tail of 3.

Tolerances are the project's bars (header of tests/test_gpu_parity.py) unless a docstring derives its own; EVERY env of EVERY seed has to meet them."""
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest

from common import Oracle, config_add, f32, rk4_reference
from raisimlib_amd import BatchedWorld, Model, _capi
from test_gpu_fuzz import random_urdf

pytestmark = pytest.mark.gpu

N = 67
LINKS = {"floating": (2, 5, 9, 12, 16, 17, 17, 7), "fixed": (3, 6, 10, 17, 14, 8)}
CASES = [(kind, i) for kind in ("floating", "fixed") for i in range(len(LINKS[kind]))]
TILTED = (1.5, -2.0, -9.0)
DEFAULT_GRAVITY = (0.0, 0.0, -9.81)
EPS = 2.0 ** -23


def _ids(c):
    return f"{c[0]}{c[1]}"


def open_joint_ranges(urdf):
    return re.sub(r'lower="[^"]*" upper="[^"]*"', 'lower="-6.0" upper="6.0"', urdf)


def add_rotor_inertia(urdf):
    """rotor_inertia on the <dynamics> of every other joint (j1, j3, ..): 0.01 .. 0.05.  Returns the new string and {joint number: value}."""
    rotor = {}

    def put(m):
        j = int(m.group(1))
        if j % 2 == 0:
            return m.group(0)
        rotor[j] = 0.01 * (1 + j % 5)
        return f'{m.group(0)[:-2]} rotor_inertia="{rotor[j]:.2f}"/>'
    out = re.sub(r'<joint name="j(\d+)".*?<dynamics damping="[^"]*"/>', put, urdf, flags=re.S)
    return out, rotor


def strip_damping(urdf):
    return re.sub(r'damping="[^"]*"', 'damping="0"', urdf)


def fix_base(urdf):
    return urdf.replace('"l0"', '"world"')


def random_states(rng, nq, nv, lift=0.0):
    gc = np.zeros((N, nq)); gc[:, 0:2] = rng.uniform(-1, 1, (N, 2)); gc[:, 2] = lift + rng.uniform(0.0, 0.5, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-1.2, 1.2, (N, nq - 7))
    gv = rng.normal(size=(N, nv))          # (the six base rows of a fixed base too: nothing may read them)
    return f32(gc), f32(gv)


def oracle_queries(o, gc, gv):
    """the oracle's M and h of every env; a fixed base's velocity rows are passed as zero"""
    uq = gv.copy()
    if o.blob.fixed_base:
        uq[:, :6] = 0.0
    return np.array([o.mass_matrix(q) for q in gc]), np.array([o.nonlinearities(q, u) for q, u in zip(gc, uq)])


@functools.lru_cache(maxsize=None)
def case(kind, i, lift=0.0, n_links=None):
    """One model with its states and the oracle's answers, computed once and shared (nobody writes into them)."""
    rng = np.random.default_rng((7000 if kind == "floating" else 8000) + i)
    n_links = n_links or LINKS[kind][i]
    plain = open_joint_ranges(random_urdf(rng, n_links))
    if n_links > 17:            # the 40-body tree: one sphere (the root's) - the query kernels read no collision geometry
        first = plain.index("</collision>") + len("</collision>")
        plain = plain[:first] + re.sub(r"<collision>.*?</collision>", "", plain[first:], flags=re.S)
    if kind == "fixed":
        plain = fix_base(plain)
    urdf, by_joint = add_rotor_inertia(plain)
    model, plain_model = Model(urdf_string=urdf), Model(urdf_string=plain)
    rotor = {model.joint_index(f"j{j}"): v for j, v in by_joint.items()}          # by body: the loader orders the bodies itself
    assert model.blob.fixed_base == (kind == "fixed") and model.blob.nb == n_links and model.nv == n_links + 5
    for b in range(1, n_links):
        assert model.blob.armature[b] == pytest.approx(rotor.get(b, 0.0)) and plain_model.blob.armature[b] == 0.0
    gravity = DEFAULT_GRAVITY if i % 2 == 0 else TILTED
    gc, gv = random_states(rng, model.nq, model.nv, lift)
    o = Oracle(model.blob); o.p.gravity[:] = gravity
    M, h = oracle_queries(o, gc, gv)
    M_plain = np.array([Oracle(plain_model.blob).mass_matrix(q) for q in gc])
    return SimpleNamespace(kind=kind, i=i, fixed=kind == "fixed", j0=6 if kind == "fixed" else 0, urdf=urdf, model=model, rotor=rotor, gravity=gravity,
                           gc=gc, gv=gv, o=o, M=M, h=h, M_plain=M_plain, rng_seed=int(rng.integers(1 << 30)),
                           prismatic='type="prismatic"' in urdf)


def new_world(c, model=None, gv=None):
    w = BatchedWorld(model or c.model, N)
    w.set_gravity(c.gravity)
    w.set_state(c.gc, c.gv if gv is None else gv)
    return w


@functools.lru_cache(maxsize=None)
def device_queries(kind, i, n_links=None):
    c = case(kind, i, n_links=n_links) if n_links else case(kind, i)
    w = new_world(c)
    w.integrate1()
    out = SimpleNamespace(M=w.get_mass_matrix(), h=w.get_nonlinearities(), Minv=w.get_inverse_mass_matrix() if not n_links else None)
    w.close()
    return out


def test_the_generated_models_reach_the_paths_they_are_meant_to(built_lib):
    cs = [case(*k) for k in CASES]
    for kind in ("floating", "fixed"):
        assert sum(c.prismatic for c in cs if c.kind == kind) >= 3
        assert all(c.rotor for c in cs if c.kind == kind and c.model.nb > 2)
    assert sum(c.model.nb > 16 for c in cs) >= 2 and sum(c.model.nb <= 16 for c in cs) >= 2       # rsb_query_kernel<32> and <16>
    assert {c.gravity for c in cs} == {DEFAULT_GRAVITY, TILTED}


def check_query_parity(c, d):
    j0 = c.j0
    for e in range(N):
        Mr, hr = c.M[e][j0:, j0:], c.h[e][j0:]
        M, h = d.M[e][j0:, j0:], d.h[e][j0:]
        dM, dh = np.abs(M - Mr).max(), np.abs(h - hr).max()
        assert dM <= 1e-5 * np.abs(Mr).max(), (c.kind, c.i, e, dM / np.abs(Mr).max())
        assert dh <= 2e-5 * (1 + np.abs(hr).max()), (c.kind, c.i, e, dh / (1 + np.abs(hr).max()))
        assert np.array_equal(d.M[e], d.M[e].T)
        for b, rotor in c.rotor.items():           # the armature sits on the diagonal, on top of the armature-free CRBA value
            k = b + 5
            assert abs(float(d.M[e][k, k]) - c.M_plain[e][k, k] - rotor) <= 1e-5 * np.abs(Mr).max(), (c.kind, c.i, e, b)


@pytest.mark.parametrize("kind,i", CASES, ids=map(_ids, CASES))
def test_query_parity_on_random_trees(built_lib, kind, i):
    """M and h of rsb_integrate1 against the oracle at the project's bars (1e-5 of max|M|; 2e-5 (1 + max|h|)): prismatic joints, armature, tilted
    gravity, a ragged last block.  Floating bases: every row; fixed bases: the joint block / joint rows (the base rows describe a body that cannot
    move).  A fixed base's velocity rows hold N(0, 1) noise here: h's joint rows do not depend on a single bit of them."""
    c, d = case(kind, i), device_queries(kind, i)
    check_query_parity(c, d)
    if c.fixed:
        gv0 = c.gv.copy(); gv0[:, :6] = 0.0
        w = new_world(c, gv=gv0)
        w.integrate1()
        h0 = w.get_nonlinearities()
        w.close()
        assert np.array_equal(d.h[:, 6:], h0[:, 6:]), (i, np.abs(d.h[:, 6:] - h0[:, 6:]).max())


def test_query_parity_on_a_tree_of_40_bodies(built_lib):
    """rsb_query_kernel<64> (33 .. 64 bodies): the same generator at 40 links, one sphere; the same bars."""
    c, d = case("floating", 1, n_links=40), device_queries("floating", 1, n_links=40)
    assert c.model.nb == 40 and c.model.ncol == 1 and c.prismatic
    check_query_parity(c, d)


def fp32_cholesky_inverse(M):
    """M^-1 = L^-T L^-1 from an fp32 Cholesky factor, every step in fp32 numpy: what rsb_minv_kernel computes, restated."""
    L = np.linalg.cholesky(M.astype(np.float32))
    Li = np.linalg.solve(L, np.eye(len(M), dtype=np.float32)).astype(np.float32)
    return (Li.T @ Li).astype(np.float32)


C_INVERSE = 4 * 0.2203      # see test_inverse_mass_matrix_on_random_trees


@pytest.mark.parametrize("kind,i", CASES, ids=map(_ids, CASES))
def test_inverse_mass_matrix_on_random_trees(built_lib, kind, i):
    """rsb_get_inverse_mass_matrix: max|Minv M_oracle - I| < 2e-4 for nv <= 20 (the bound of test_mass_matrix_and_nonlinearities_query), and for the
    larger systems < C cond(M_oracle) 2^-23, cond measured per env, with C = 4 x 0.2203 = 0.881 (6.8e-5 at fixed3's worst env, cond 651; the
    single-model 5e-2 this replaces was 700 x that).  Where C comes from, all on the CPU (tools/slow_path_fp32_restatement.py), per model with
    nv > 20 (floating4, floating5, floating6, fixed3), as max over the 67 envs of residual / (cond 2^-23):
      fp32 numpy Cholesky inverse (fp32_cholesky_inverse) of the ORACLE's M ........ 0.0331  0.0060  0.0027  0.0097
      the kernel's own loop order in fp32 numpy, of the oracle's M .................. 0.0323  0.0098  0.0022  0.0099
      the same, of M from the query kernel's CRBA restated in fp32 numpy ............ 0.0413  0.0743  0.0203  0.2203
    The first line, times 4, is 0.132 - and a correct device misses it: 0.159 at fixed3 (env 4: residual 1.153e-5 against 1.027e-5; the three
    floating models: 0.055, 0.039, 0.016).  The inverse that
    the device returns is that of ITS M, whose fp32 rounding (relative 1e-6 of max|M|, a tenth of the M bar) the product with the oracle's M sees in
    full; the third line restates that whole path and misses the first bound by the same kind of amount (0.2203), so C is 4 x the third line's worst.
    Bit-symmetric.
    Fixed bases: the six base rows and columns are exactly zero and the joint block is the inverse of M[6:, 6:] - the base held, not floating."""
    c, d = case(kind, i), device_queries(kind, i)
    j0, nv, worst = c.j0, c.model.nv, 0.0
    for e in range(N):
        Mr, Mi = c.M[e][j0:, j0:], d.Minv[e].astype(np.float64)
        assert np.array_equal(d.Minv[e], d.Minv[e].T)
        assert not Mi[:j0].any() and not Mi[:, :j0].any()
        bound = 2e-4 if nv <= 20 else C_INVERSE * np.linalg.cond(Mr) * EPS
        res = np.abs(Mi[j0:, j0:] @ Mr - np.eye(nv - j0)).max()
        worst = max(worst, res / (np.linalg.cond(Mr) * EPS))
        assert res < bound, (kind, i, e, res, bound)
    print(f"{kind}{i}: nv {nv}, max residual / (cond 2^-23) = {worst:.4f}")


@pytest.mark.parametrize("kind,i", CASES, ids=map(_ids, CASES))
def test_the_step_kernel_and_the_query_kernels_state_the_same_dynamics(built_lib, kind, i):
    """ABA in LDS (the step kernel) against CRBA + RNEA (the query kernel), no shared code and no oracle in between: 5 m above the ground (no contact),
    FORCE_AND_TORQUE with random joint torques, no damping, one semi-implicit integrate(): u1 = u0 + dt M^-1 (tau - h), solved in fp64 over the
    DEVICE's own M and h, within the one-step bar 2e-4 (1 + |u|_inf) - and the same over the oracle's M and h.  Fixed bases: joint block, joint rows."""
    c = case(kind, i, lift=5.0)
    model = Model(urdf_string=strip_damping(c.urdf))
    rng = np.random.default_rng(c.rng_seed)
    tau = np.zeros((N, model.nv)); tau[:, 6:] = rng.normal(size=(N, model.nv - 6)) * 3.0
    tau = f32(tau)
    w = new_world(c, model=model)
    w.set_control_mode(0); w.set_self_collision(False)
    w.set_pd_gains(np.zeros(model.nv, np.float32), np.zeros(model.nv, np.float32))
    w.set_generalized_force(tau)
    w.integrate1()
    M, h = w.get_mass_matrix().astype(np.float64), w.get_nonlinearities().astype(np.float64)
    dt = w.get_time_step()
    w.integrate(1)
    q1, u1 = w.get_state(); cnt, _ = w.get_contacts()
    w.close()
    assert cnt.sum() == 0 and np.isfinite(u1).all()
    j0 = c.j0
    if c.fixed:      # the base stays: position and velocity rows exactly; the quaternion is renormalised by the step (2 ulp: the rows hold an fp32-rounded unit quaternion)
        assert np.array_equal(q1[:, :3], c.gc[:, :3].astype(np.float32)) and np.abs(q1[:, 3:7] - c.gc[:, 3:7]).max() <= 2 * EPS and not u1[:, :6].any()
    for which, (Ms, hs) in (("device", (M, h)), ("oracle", (c.M, c.h))):
        for e in range(N):
            pred = c.gv[e][j0:] + dt * np.linalg.solve(Ms[e][j0:, j0:], (tau[e] - hs[e])[j0:])
            err = np.abs(u1[e][j0:] - pred).max() / (1 + np.abs(pred).max())
            assert err <= 2e-4, (which, kind, i, e, err)


def test_runge_kutta_4_fixed_base_pendulum_matches_the_exact_period(built_lib):
    """test_runge_kutta_4_pendulum_matches_the_exact_period's pendulum (l = 0.5, released at 1 rad, dt = T / 300, T from the elliptic integral) bolted
    to the world instead of hung from a 1e9 kg anchor - the same physics, so the same thresholds: back at the start within 2e-4 after 300 steps, the
    semi-implicit scheme more than 20 x further off.  The base velocity rows hold 0.3 (as in test_fixed_base_pendulum_period): nothing may read them."""
    from scipy.special import ellipk
    from test_oracle_kat import FIXED_PENDULUM
    G, l, th0, n = 9.81, 0.5, 1.0, 64
    T = 4.0 * np.sqrt(l / G) * ellipk(np.sin(th0 / 2) ** 2)
    dt = T / 300
    off = {}
    for scheme in ("runge_kutta_4", "semi_implicit"):
        m = Model(urdf_string=FIXED_PENDULUM.format(l=l, m=1.0))
        assert m.blob.fixed_base == 1
        w = BatchedWorld(m, n)
        w.set_time_step(dt)
        w.set_integration_scheme(scheme)
        w.set_pd_gains(np.zeros(m.nv, np.float32), np.zeros(m.nv, np.float32))
        gc = np.zeros(m.nq); gc[3] = 1.0; gc[7] = th0
        gv = np.zeros(m.nv); gv[:6] = 0.3
        w.set_state(np.tile(gc, (n, 1)), np.tile(gv, (n, 1)))
        w.integrate(300)
        q, u = w.get_state()
        w.close()
        assert np.ptp(q, axis=0).max() == 0.0 and np.ptp(u, axis=0).max() == 0.0            # all 64 envs bit-identical
        assert np.array_equal(q[:, :7], np.tile(gc[:7].astype(np.float32), (n, 1)))         # the base rows of gc untouched
        assert np.abs(u[:, :6]).max() < 1e-7                                                # (test_fixed_base_pendulum_period's requirement)
        off[scheme] = max(abs(q[0, 7] - th0), abs(u[0, 6]) * np.sqrt(l / G))
    assert off["runge_kutta_4"] < 2e-4 and off["semi_implicit"] > 20 * off["runge_kutta_4"], off


def rk4_setup(c):
    """PD gains, targets and feed-forward torques for a Runge-Kutta step in the air.  The scheme's PD is explicit, and the generator's lightest links
    weigh 0.3 kg with 1.5e-3 kg m^2: gains are kept where such a joint is not stiff at dt = 2.5 ms (kp <= 10: omega dt <= 0.2; kd <= 0.2: kd dt / I <= 0.33),
    so that the step tests the scheme, not the amplification of rounding by a spring at the edge of its stability region."""
    rng = np.random.default_rng(c.rng_seed + 1)
    nv = c.model.nv
    kp = np.zeros(nv, np.float32); kd = np.zeros(nv, np.float32)
    kp[6:] = rng.uniform(0, 10, nv - 6); kd[6:] = rng.uniform(0, 0.2, nv - 6)
    pt = c.gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (N, c.model.nq - 7)); pt = f32(pt)
    tau = np.zeros((N, nv)); tau[:, 6:] = rng.normal(size=(N, nv - 6)); tau = f32(tau)
    return kp, kd, pt, tau


def rk4_world(c, kp, kd, pt, tau):
    w = new_world(c)
    w.set_self_collision(False)
    w.set_integration_scheme("runge_kutta_4")
    w.set_pd_gains(kp, kd); w.set_pd_target(pt, np.zeros((N, c.model.nv))); w.set_generalized_force(tau)
    return w


RK4_CASES = [("fixed", 1), ("fixed", 2), ("fixed", 3), ("floating", 2), ("floating", 4), ("floating", 5)]


@pytest.mark.parametrize("kind,i", RK4_CASES, ids=map(_ids, RK4_CASES))
def test_runge_kutta_4_one_step_parity_on_random_trees(built_lib, kind, i):
    """One RUNGE_KUTTA_4 step in the air against common.rk4_reference (the fp64 restatement over the oracle's queries that
    test_runge_kutta_4_step_against_an_fp64_restatement_over_the_oracles_queries uses) at that test's bars, |du| < 3e-4 (1 + |u0|_inf) and |dq| < 5e-6:
    fixed bases (the joints answer through M[6:, 6:], the base frozen, its velocity rows noise) and floating trees with prismatic joints."""
    c = case(kind, i, lift=5.0)
    assert c.fixed or c.prismatic
    kp, kd, pt, tau = rk4_setup(c)
    w = rk4_world(c, kp, kd, pt, tau)
    dt = w.get_time_step()
    w.integrate(1)
    q1, u1 = w.get_state(); cnt, _ = w.get_contacts()
    w.close()
    assert cnt.sum() == 0
    j0 = c.j0
    if c.fixed:
        assert np.array_equal(q1[:, :7], c.gc[:, :7].astype(np.float32)) and not u1[:, :6].any()
    for e in range(N):
        theta, du = rk4_reference(c.o, dt, kp.astype(np.float64), kd.astype(np.float64), c.gc[e], c.gv[e], pt[e], tau_ff=tau[e])
        eu = np.abs(u1[e] - (c.gv[e] + du))[j0:].max() / (1 + np.abs(c.gv[e][j0:]).max())
        eq = np.abs(q1[e] - config_add(c.gc[e], theta, c.fixed)).max()
        assert eu < 3e-4 and eq < 5e-6, (kind, i, e, eu, eq)


MASKED_CASES = [("fixed", 2), ("floating", 2)]


@pytest.mark.parametrize("kind,i", MASKED_CASES, ids=map(_ids, MASKED_CASES))
def test_runge_kutta_4_masked_integrate(built_lib, kind, i):
    """rsb_integrate_masked under RUNGE_KUTTA_4, every third env masked out: those keep gc and gv bit for bit, the others step exactly as in a world
    that steps them all, and the feed-forward torque rows - which the scheme overwrites with its effective force and restores - read back unchanged."""
    c = case(kind, i, lift=5.0)
    kp, kd, pt, tau = rk4_setup(c)
    mask = np.ones(N, np.uint8); mask[::3] = 0
    a, b = rk4_world(c, kp, kd, pt, tau), rk4_world(c, kp, kd, pt, tau)
    q0, u0 = a.get_state()
    a.integrate_masked(mask, 1); b.integrate(1)
    (qa, ua), (qb, ub) = a.get_state(), b.get_state()
    tff = a.get_field(_capi.RSB_F_TAU_FF)
    a.close(); b.close()
    on = mask.astype(bool)
    assert np.array_equal(qa[~on], q0[~on]) and np.array_equal(ua[~on], u0[~on])
    assert np.array_equal(qa[on], qb[on]) and np.array_equal(ua[on], ub[on]) and not np.array_equal(qb[on], q0[on])
    assert np.array_equal(tff, tau.astype(np.float32))
