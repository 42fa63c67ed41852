"""Every env of a step held to the step's own impulse balance (tests/step_balance_reference.py), converged or not.

Parity with the oracle ends where a contact solve misses its exit test: fp32 and fp64 stop a non-converging iteration at different points.  What holds at
every iterate is that the velocity the step returns is the one its own reported impulses produce,
    A (u1 - u0) = dt (tau - h) + sum_k J_k^T lam_k + (one unreported scalar per joint outside its range, on that joint's row only),   A = M + diag(B),
with tau, M, h and J the oracle's and lam_k, position and body the device's own rsb_get_contacts records.  One integrate(1) from a known state, then on
EVERY env of every population, none left out:
    max |delta| <= C (1 + U),  delta = A^-1 r0 the velocity the unexplained generalised impulse would produce;
    every limit row's s_j r_j >= -C (1 + |u|_inf) sum_k |A_jk|  (|u|_inf over u0 and u1);
    q1 = config_add(q0, dt (theta u1 + (1 - theta) u0)) within 2e-6 + 1e-6 |q|;  a fixed base keeps q[:7] and u[:6] = 0;
    the contact records obey record_laws;  the overflow bit of the flags equals the oracle's (more candidates than slots).
C = 2e-4 is the project's one-step bar (tests/test_gpu_slow_path.py::test_the_step_kernel_and_the_query_kernels_state_the_same_dynamics meets it in the same
velocity-space form without contacts); U carries the terms contacts add.  The device meets it as it stands: over the 47 runs below (5 446 envs: 498
unconverged and 38 overflowed by the device's own flags, 1 720 past a stop, 150 effort-clipped) the worst delta / (C (1 + U)) is 0.195 (Atlas, collapsing), the
worst limit row 0.017 of its bar; no float32 restatement of the kernel was needed and C stayed 2e-4.
Envs whose device flags have bits 0 and 2 clear also meet v_n+ = n . J u1 >= -T and lam_n v_n+ <= T lam_n at every terrain contact of a primitive
without restitution, T = 4 x max(the oracle's own figure on its converged envs of the population, the solver's exit threshold) (normal_bar: the floor
makes T = 4e-5 on most quadruped populations, 10 to 100 times what the device leaves there).

test_parity_record writes measured-over-bar per case to profiles/step_balance_parity.txt."""
import functools
import os

import numpy as np
import pytest

import step_balance_reference as sb
from common import ROOT, config_add
from raisimlib_amd import BatchedWorld

pytestmark = pytest.mark.gpu

C = sb.C_STEP
MODES = ("cold", "warm", "warm_off")        # one step from the drawn state | integrate(3), get_state(), integrate(1) | the same with the warm start off
RUNS = [(name, "cold") for name in sb.CASES] + [(name, mode) for mode in MODES[1:] for name in sb.WARM_CASES]


def make_world(c):
    w = BatchedWorld(c.model, c.N)
    w.set_max_contacts(c.kmax)
    if c.lpe:
        w.set_lanes_per_env(c.lpe)
    w.set_control_mode(c.mode)
    if c.recipe is not None:
        c.recipe.setup_world(w, c.N, 0)
    if c.ground is not None:
        w.add_ground(c.ground)
    if c.heightmap is not None:
        w.add_height_map(*c.heightmap)
    if c.materials is not None:
        w.set_collision_materials(*c.materials)
    w.set_default_friction(c.mu)
    w.set_slip_rule(c.slip_rule)
    w.set_integration_scheme(c.scheme)
    w.set_pd_gains(c.kp, c.kd)
    w.set_pd_target(c.pt, c.dtg)
    if c.tau_ff is not None:
        w.set_generalized_force(c.tau_ff)
    return w


@functools.lru_cache(maxsize=None)
def device_run(name, mode):
    """The step under test and everything it is held to, computed once: (case, oracle, q0, u0, the device's q1, u1, counts, records, flags, the oracle's
    step from the same state, the balance of every env)"""
    c = sb.case(name)
    w = make_world(c)
    assert w.get_time_step() == pytest.approx(sb.make_oracle(c).p.dt, rel=1e-6)
    w.set_state(c.gc, c.gv)
    q0, u0 = c.gc, c.gv
    if mode != "cold":
        w.set_solver_warm_start(mode == "warm")
        w.integrate(3)
        q0, u0 = (a.astype(np.float64) for a in w.get_state())          # (no set_state in between: with the warm start on, the next solve starts from this one)
    w.integrate(1)
    q1, u1 = w.get_state()
    cnt, con = w.get_contacts()
    fl = w.get_flags()
    w.close()
    o, ref = sb.oracle_step(c, q=q0, u=u0)
    kept = np.clip(cnt, 0, c.kmax)
    res = sb.balance(o, q0, u0, u1, [con[e][:kept[e]] for e in range(c.N)], c.kp, c.kd, c.pt, c.dtg, c.tau_ff)
    return c, o, q0, u0, q1, u1, cnt, con, fl, ref, res


def figures(name, mode):
    """measured over bar: the worst delta / (C (1 + U)) and the worst limit-row figure -s_j r_j / (C (1 + |u|_inf) sum_k |A_jk|) of a run"""
    c, o, q0, u0, q1, u1, cnt, con, fl, ref, res = device_run(name, mode)
    d = np.array([x.dmax / (C * (1 + x.U)) for x in res])
    lim = np.array([(-x.lim_sr / (C * (1 + max(x.u_inf, np.abs(u1[e]).max())) * x.lim_rowsum)).max(initial=0) for e, x in enumerate(res)])
    return d, lim


@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_every_env_meets_the_impulse_balance(built_lib, name, mode):
    c, o, q0, u0, q1, u1, cnt, con, fl, ref, res = device_run(name, mode)
    assert np.isfinite(q1).all() and np.isfinite(u1).all()
    if mode == "cold":
        sb.assert_no_joint_at_a_stop(c.model.blob, q0)
    else:        # a state the device left: nothing keeps it off a stop, and only a joint ON the float32 image of a stop could be ranked two ways
        lo, hi = sb.joint_ranges(c.model.blob)
        assert not ((q0[:, 7:] == lo.astype(np.float32)) | (q0[:, 7:] == hi.astype(np.float32)))[:, lo < hi].any()
    d, lim = figures(name, mode)
    print(f"{name} {mode}: N {c.N}, device unconverged {int(((fl & 4) != 0).sum())} overflowed {int((fl & 1).sum())} limited {sum(x.limited for x in res)} "
          f"clipped {sum(x.clipped for x in res)}; worst delta / (C (1 + U)) {d.max():.3f} (env {int(d.argmax())}), worst limit row {lim.max():.3f}")
    # the balance and the limit rows' sign: every env
    assert np.all(d <= 1.0), (name, mode, int(d.argmax()), d.max(), int((d > 1).sum()))
    assert np.all(lim <= 1.0), (name, mode, int(lim.argmax()), lim.max())
    # the configuration moves with the velocities the scheme names: every env
    fixed = bool(c.model.blob.fixed_base)
    dt = o.p.dt
    v0 = u0.copy()
    if fixed:
        v0[:, :6] = 0.0
    for e in range(c.N):
        want = config_add(q0[e], dt * (c.theta * u1[e].astype(np.float64) + (1 - c.theta) * v0[e]), fixed)
        assert np.all(np.abs(q1[e] - want) <= 2e-6 + 1e-6 * np.abs(want)), (name, mode, e, np.abs(q1[e] - want).max())
    if fixed:
        assert np.array_equal(q1[:, :7], q0[:, :7].astype(np.float32)) and not u1[:, :6].any()
    # the records: every env
    laws = sb.record_laws(con, cnt, sb.mu_of_case(c, o), c.model.nb, c.kmax)
    for law, v in laws.items():
        assert not v.any(), (name, mode, law, int(np.argmax(v)), v.max())
    # overflow: more candidates than slots, as the oracle counts them from the same state
    assert np.array_equal(fl & 1, ref["flags"] & 1), (name, mode, np.nonzero((fl & 1) != (ref["flags"] & 1))[0])


@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_converged_envs_end_on_the_contact_law(built_lib, name, mode):
    """device flags bits 0 and 2 clear, erp 0: v_n+ >= -T and lam_n v_n+ <= T lam_n at every reported terrain contact of a primitive without restitution
    (all of them but in the per-primitive materials population, where the contacts of the primitives with restitution 0 are held to it)"""
    c, o, q0, u0, q1, u1, cnt, con, fl, ref, res = device_run(name, mode)
    prims = sb.law_primitives(c)
    fig, n_ref = sb.normal_figure(o, q0, ref["u"], ref["contacts"], ref["n_contacts"], (ref["flags"] & 5) == 0, prims)
    T = sb.normal_bar(o, fig)
    conv = (fl & 5) == 0
    worst, n_dev = 0.0, 0
    for e in np.nonzero(conv)[0]:
        vn, ln = sb.normal_velocities(o, q0[e], u1[e], con[e][:cnt[e]], prims)
        n_dev += len(vn)
        worst = max(worst, (-vn).max(initial=0), (vn * (ln > 0)).max(initial=0))
        assert np.all(vn >= -T) and np.all(ln * vn <= T * ln), (name, mode, e, vn, ln, T)
    if prims is not None:
        assert prims.any() and not prims.all() and n_dev >= 50, (name, n_dev)       # (both kinds of primitive, and enough contacts left to hold to the law)
    print(f"{name} {mode}: {int(conv.sum())} converged envs, {n_dev} contacts, worst figure {worst:.2e}, T {T:.2e} (oracle's figure {fig:.2e} over {n_ref} contacts)")


def test_the_device_populations_hold_the_envs_parity_cannot_reach(built_lib):
    """the guards of the CPU file, by the device's own flags: the runs above are not a check of converged envs under another name"""
    n = dict(unconverged=0, overflow=0, limited=0, self_collision=0, clipped=0)
    for name, mode in RUNS:
        c, o, q0, u0, q1, u1, cnt, con, fl, ref, res = device_run(name, mode)
        n["unconverged"] += int(((fl & 4) != 0).sum())
        n["overflow"] += int(((fl & 1) != 0).sum())
        n["limited"] += sum(x.limited for x in res)
        n["self_collision"] += sum(bool((con[e][:cnt[e]]["collision"] & sb.SELF_A).any()) for e in range(c.N))
        n["clipped"] += sum(x.clipped for x in res)
    print(n)
    assert n["unconverged"] >= 100 and n["overflow"] >= 10 and n["limited"] >= 500 and n["self_collision"] >= 50 and n["clipped"] >= 30, n


def test_parity_record(built_lib):
    """measured over bar per case, written to profiles/step_balance_parity.txt"""
    lines = ["tests/test_gpu_step_balance.py::test_parity_record",
             "device fp32 step vs the impulse balance over the oracle's fp64 M, h, tau, J and the device's own contact records; every env of every case.",
             f"delta: worst |A^-1 r0|_inf / (C (1 + U)), C = {C:g}; limit row: worst -s_j r_j / (C (1 + |u|_inf) sum_k |A_jk|); both have to stay <= 1.",
             "normal: worst of -v_n+ and v_n+ (where lam_n > 0) over the terrain contacts (primitives without restitution) of the device's converged envs, and its bar T = 4 max(oracle's figure, exit threshold).",
             "counts by the device's flags: unc = unconverged, ovf = overflowed; lim = envs with a joint past a stop, clip = envs with an effort-clipped joint"]
    for name, mode in RUNS:
        c, o, q0, u0, q1, u1, cnt, con, fl, ref, res = device_run(name, mode)
        d, lim = figures(name, mode)
        prims = sb.law_primitives(c)
        fig, _ = sb.normal_figure(o, q0, ref["u"], ref["contacts"], ref["n_contacts"], (ref["flags"] & 5) == 0, prims)
        got, _ = sb.normal_figure(o, q0, u1, con, cnt, (fl & 5) == 0, prims)
        normal = f"normal {got:.1e} (T {sb.normal_bar(o, fig):.1e})"
        lines.append(f"  {name + ' ' + mode:38s} N {c.N:3d} nb {c.model.nb:2d}  unc {int(((fl & 4) != 0).sum()):3d} ovf {int((fl & 1).sum()):3d} lim {sum(x.limited for x in res):3d} "
                     f"clip {sum(x.clipped for x in res):3d}   delta {d.max():.3f}  limit row {lim.max():.3f}  {normal}")
    with open(os.path.join(ROOT, "profiles", "step_balance_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
