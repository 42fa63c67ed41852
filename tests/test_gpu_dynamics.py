"""Batched inverse dynamics with joint reaction wrenches and contact-free forward dynamics on the device (rsb_inverse_dynamics, rsb_forward_dynamics;
raisimlib_amd/csrc/rsb_dynamics.hip) against fp64 references on the float32-rounded state the device saw.  Cases, inputs and references:
tests/test_dynamics_reference.py (14 random trees with prismatic joints, rotor inertia and tilted gravity at N = 67, a 40-body tree, the two shipped
models at N = 64).  EVERY env of EVERY case has to meet its bar.

Bars.
  tau            |tau - ref| <= 2e-5 (1 + S_e), S_e the env's largest row of |M_ref||udot| + |h_ref| + sum |J^T||w|: the project's bar for h
                 (tests/test_gpu_slow_path.py) extended by the terms the new inputs add.  ref = Oracle.inverse_dynamics - J^T w.
  joint wrenches 2e-5 (1 + s), s the largest component of the reference's sum of absolute terms for that env, body and output (newton_euler).
  udot           |udot - udot_ref| / (1 + max|udot_ref|) <= 4 ABA32(case), ABA32 the error of the kernel's algorithm restated in float32 numpy
                 (test_forward_dynamics says why not 4 E32, the float32 Cholesky solve of the oracle's own system); and the round trip
                 inverse_dynamics(forward_dynamics(tau)) = tau at the tau bar, which is free of conditioning.
The parity test writes the largest error / bar per quantity and model to profiles/r12_dynamics_parity.txt."""
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from common import ROOT, Oracle, f32, sphere_urdf, standing_states
from raisimlib_amd import BatchedWorld, Model, _capi, workload
from test_dynamics_reference import (NAMES, dyn_case, forward_reference, jacobians, kinematics, load_jacobians, masked, newton_euler, reference,
                                     tau_scale)

pytestmark = pytest.mark.gpu

ALL = dict(tau=True, joint_force=True, joint_torque=True)
OUT = ("tau", "joint_force", "joint_torque")


def new_world(c, n=None, gv=None):
    n = n or c.N
    w = BatchedWorld(c.model, n)
    w.set_gravity(c.gravity)
    w.set_state(c.gc[:n], (c.gv if gv is None else gv)[:n])
    return w


def loads_of(c, n=None):
    n = n or c.N
    return (c.frames, c.force[:n], c.torque[:n])


@functools.lru_cache(maxsize=None)
def device(name):
    """everything the device says about one case, computed once in one world"""
    c = dyn_case(name)
    w = new_world(c)
    d = SimpleNamespace()
    d.h = w.inverse_dynamics(None, **ALL)
    d.udot = w.inverse_dynamics(c.udot, **ALL)
    d.loads = w.inverse_dynamics(c.udot, loads=loads_of(c), **ALL)
    d.fd = w.forward_dynamics(c.tau, loads=loads_of(c))
    d.fd_plain = w.forward_dynamics(c.tau)
    d.round = w.inverse_dynamics(d.fd, loads=loads_of(c))["tau"]
    w.set_generalized_force(c.tau)
    d.fd_ff = w.forward_dynamics(None, loads=loads_of(c))
    w.integrate1()
    d.h_query = w.get_nonlinearities()
    w.set_state(c.gc, np.zeros_like(c.gv))
    d.static = w.inverse_dynamics(None, **ALL)
    w.close()
    return d


def oracle_tau(c, variant):
    """Oracle.inverse_dynamics of every env (a fixed base's rows of u and udot passed as zero) minus the loads' generalized force, the six base
    columns taken as a floating base's: for a fixed base they give the loads' share of the holding wrench"""
    out = np.zeros((c.N, c.nv))
    for e in range(c.N):
        ud = masked(c, c.udot[e]) if variant != "h" else np.zeros(c.nv)
        out[e] = c.o.inverse_dynamics(c.gc[e], masked(c, c.gv[e]), ud)
    if variant == "loads":
        out -= load_jacobians(c.name)[2]
    return out


def tau_ratio(c, got, want, variant, scale=None):
    s = tau_scale(c.name, variant) if scale is None else scale
    return np.abs(got.astype(np.float64) - want).max(axis=1) / (2e-5 * (1 + s))


def wrench_ratios(got, ref):
    """error / bar per env and body of joint_force and joint_torque"""
    rf = np.abs(got["joint_force"].astype(np.float64) - ref.jf).max(axis=2) / (2e-5 * (1 + ref.s_jf.max(axis=2)))
    rt = np.abs(got["joint_torque"].astype(np.float64) - ref.jt).max(axis=2) / (2e-5 * (1 + ref.s_jt.max(axis=2)))
    return rf, rt


@pytest.mark.parametrize("name", NAMES)
def test_inverse_dynamics_parity(built_lib, name):
    """tau against the oracle with udot = NULL (also against the oracle's h and the device's own rsb_get_nonlinearities), with udot, and with three
    loads: two on one body, one torque-only."""
    c, d = dyn_case(name), device(name)
    for variant in ("h", "udot", "loads"):
        r = tau_ratio(c, getattr(d, variant)["tau"], oracle_tau(c, variant), variant)
        print(f"{name} {variant}: tau error / bar, worst env {r.max():.3f}")
        assert r.max() <= 1.0, (name, variant, int(r.argmax()), r.max())
    j0 = c.j0
    s = tau_scale(name, "h")
    for e in range(c.N):
        assert np.abs(d.h["tau"][e].astype(np.float64) - c.h[e])[j0:].max() <= 2e-5 * (1 + s[e]), (name, e)
        assert np.abs(d.h["tau"][e].astype(np.float64) - d.h_query[e])[j0:].max() <= 2e-5 * (1 + s[e]), (name, e)


@pytest.mark.parametrize("name", NAMES)
def test_joint_wrenches(built_lib, name):
    """joint_force / joint_torque against the numpy Newton-Euler reference, every env and body, in all three variants; the identities of rsb.h on the
    device's own outputs (axis projections + armature = tau at the same bar, the base rows of tau ARE the base joint's wrench, bit for bit); at rest
    joint_force_i = -(subtree mass) g and joint_torque_i = -sum m_k (c_k - p_i) x g (the reference's "static" variant, pinned to that closed form on
    the CPU)."""
    c, d = dyn_case(name), device(name)
    blob = c.blob
    for variant in ("h", "udot", "loads", "static"):
        got, ref = getattr(d, variant), reference(name, variant)
        rf, rt = wrench_ratios(got, ref)
        print(f"{name} {variant}: joint_force {rf.max():.3f}, joint_torque {rt.max():.3f} of the bar")
        assert rf.max() <= 1.0 and rt.max() <= 1.0, (name, variant, rf.max(), rt.max())
        assert np.array_equal(got["tau"][:, :3], got["joint_force"][:, 0]) and np.array_equal(got["tau"][:, 3:6], got["joint_torque"][:, 0])
        ud = masked(c, c.udot) if variant in ("udot", "loads") else np.zeros((c.N, c.nv))
        for e in range(c.N):
            k = kinematics(blob, c.gc[e])
            for i in range(1, c.nb):
                X, S = (got["joint_torque"], ref.s_jt) if blob.jtype[i] == 1 else (got["joint_force"], ref.s_jf)
                lhs = k.a[i] @ X[e, i].astype(np.float64) + blob.armature[i] * ud[e, 5 + i]
                assert abs(lhs - got["tau"][e, 5 + i]) <= 2e-5 * (1 + S[e, i].max()), (name, variant, e, i)


def settled(model, gc0, gv0, quadruped):
    """the world after 5 control steps on the ground (self-collision on), with what it holds: state, contacts, dt"""
    n = len(gc0)
    w = BatchedWorld(model, n)
    w.add_ground(0.0)
    if quadruped:
        w.set_control_mode(1)
        w.set_pd_gains(*workload.anymal_gains())
    w.set_state(gc0, gv0)
    for k in range(5):
        if quadruped:
            w.set_pd_target(workload.anymal_targets(n, k), np.zeros((n, model.nv)))
        w.integrate(workload.SUBSTEPS)
    gc, gv = w.get_state()
    cnt, con = w.get_contacts()
    return w, f32(gc), f32(gv), cnt, con


@pytest.mark.parametrize("which", ["anymal", "sphere"])
def test_contacts(built_lib, anymal, which):
    """RSB_DYN_CONTACTS: the quadruped after 5 control steps from standing_states on the ground (N = 64, self-collision on) and a sphere resting on the
    plane.  The results equal the references with the contact list read back (get_contacts) and applied as impulse / dt at `position` on `body`, at the
    bars of the parity tests; forward dynamics with the same contacts meets its round trip.  At least one env holds 3 or more contacts.  (This
    population produces no self-collision pair: the standing quadruped's links do not touch each other within five steps; the record type is covered
    as any other record is - by body and position - and the print below says how many there were.)"""
    n = 64
    rng = np.random.default_rng(77)
    if which == "anymal":
        model = anymal
        gc0, gv0 = standing_states(n, seed=12)
    else:
        model = Model(urdf_string=sphere_urdf(2.0, 0.1))
        gc0 = np.zeros((n, 7)); gc0[:, 0:2] = rng.uniform(-1, 1, (n, 2)); gc0[:, 2] = 0.1; gc0[:, 3] = 1.0
        gv0 = np.zeros((n, 6)); gv0[:, :2] = rng.uniform(-0.2, 0.2, (n, 2))
    w, gc, gv, cnt, con = settled(model, gc0, gv0, which == "anymal")
    dt = w.get_time_step()
    udot, tau = f32(rng.normal(size=(n, model.nv))), f32(rng.normal(size=(n, model.nv)))
    got = w.inverse_dynamics(udot, contacts=True, **ALL)
    plain = w.inverse_dynamics(udot, **ALL)
    fd = w.forward_dynamics(tau, contacts=True)
    back = w.inverse_dynamics(fd, contacts=True)["tau"]
    w.close()
    selfc = int(sum(((con[e, :cnt[e]]["collision"] & 0x30000) != 0).sum() for e in range(n)))      # RSB_CONTACT_SELF_A | RSB_CONTACT_SELF_B
    print(f"{which}: contacts per env min {cnt.min()} max {cnt.max()}, self-collision entries {selfc}")
    assert cnt.max() >= (3 if which == "anymal" else 1) and cnt.sum() > 0
    assert not np.array_equal(got["tau"], plain["tau"])
    o = Oracle(model.blob)
    blob = model.blob
    for e in range(n):
        loads = [(int(r["body"]), r["position"].astype(np.float64), r["impulse"].astype(np.float64) / dt, np.zeros(3)) for r in con[e, :cnt[e]]]
        t, jf, jt, st, sf, sn = newton_euler(blob, gc[e], gv[e], udot[e], (0.0, 0.0, -9.81), loads)
        k = kinematics(blob, gc[e])
        M, h = o.mass_matrix(gc[e]), o.nonlinearities(gc[e], gv[e])
        want, mag = o.inverse_dynamics(gc[e], gv[e], udot[e]), np.zeros(model.nv)
        for body, point, force, _ in loads:
            Jl, _ = jacobians(blob, k, body, point)
            want = want - Jl.T @ force
            mag += np.abs(Jl.T) @ np.abs(force)
        S = (np.abs(M) @ np.abs(udot[e]) + np.abs(h) + mag).max()
        assert np.abs(got["tau"][e] - want).max() <= 2e-5 * (1 + S), (which, e, np.abs(got["tau"][e] - want).max() / (2e-5 * (1 + S)))
        assert np.abs(t - want).max() <= 1e-9 * (1 + S)
        assert (np.abs(got["joint_force"][e] - jf).max(axis=1) <= 2e-5 * (1 + sf.max(axis=1))).all(), (which, e)
        assert (np.abs(got["joint_torque"][e] - jt).max(axis=1) <= 2e-5 * (1 + sn.max(axis=1))).all(), (which, e)
        S2 = (np.abs(M) @ np.abs(fd[e].astype(np.float64)) + np.abs(h) + mag).max()
        assert np.abs(back[e] - tau[e]).max() <= 2e-5 * (1 + S2), (which, e)


# tools/dynamics_aba_restatement.py, float32 column: max over the envs of |udot - udot_ref| / (1 + max|udot_ref|) of the kernel's algorithm in float32 numpy
ABA32 = {"floating0": 5.393e-07, "floating1": 3.562e-06, "floating2": 2.853e-06, "floating3": 2.750e-06, "floating4": 9.356e-06, "floating5": 8.380e-06,
         "floating6": 8.304e-06, "floating7": 5.353e-06, "fixed0": 9.179e-07, "fixed1": 1.070e-06, "fixed2": 1.019e-06, "fixed3": 9.207e-06, "fixed4": 6.784e-06,
         "fixed5": 5.179e-06, "tree40": 1.115e-05, "anymal": 1.005e-06, "atlas": 5.464e-04}


def udot_ratio(c, got, fr):
    """error / (4 ABA32) per env"""
    return np.array([np.abs(got[e].astype(np.float64) - fr.udot[e]).max() / (1 + np.abs(fr.udot[e]).max()) for e in range(c.N)]) / (4 * ABA32[c.name])


@pytest.mark.parametrize("name", NAMES)
def test_forward_dynamics(built_lib, name):
    """udot against solve(M_ref, tau - h_ref + J^T w) in fp64 with the three loads, every env: |udot - udot_ref| / (1 + max|udot_ref|) <= 4 ABA32(case).
    The first yardstick, 4 E32 - four times what a float32 Cholesky solve of the oracle's own fp64-assembled system loses
    (test_dynamics_reference.test_forward_dynamics_yardstick prints E32: 2.2e-7 .. 2.4e-6) - is tighter than a correct float32 device reaches, as
    test_gpu_slow_path.test_inverse_mass_matrix_on_random_trees found for its first one: E32 sees neither the float32 rounding of h and J^T w (the
    right-hand side is assembled in fp64 there) nor that of the articulated inertias.  Established on the CPU before any device figure was looked at:
    the kernel's algorithm restated in float32 numpy (tools/dynamics_aba_restatement.py; in float64 the same code agrees with udot_ref to 1e-12) ends
    at ABA32 = 5.4e-7 (floating0: 2.1 E32) .. 1.1e-5 (tree40: 5.1 E32), up to 34 E32 on the 17-link trees (fixed3 9.2e-6 against E32 2.7e-7) and
    5.5e-4 = 285 E32 on the humanoid (cond(M) 4.6e5, |udot| up to 5.4e3).  So the bar is 4 x ABA32(case), the same margin over the restatement that
    predecessor took, for the reason it gives: a correct device solves ITS fp32 system.  Both figures per case are in the table above and in the
    tool's output; the device's own are in profiles/r12_dynamics_parity.txt (measured on an MI355X after the bar was fixed: 0.10 .. 0.75 of 4 ABA32,
    which is 0.16 .. 63 x the first yardstick 4 E32 - 11 of the 17 cases miss that one, the humanoid by 63 x).
    Fixed bases: udot[:, :6] == 0 exactly.  The round trip inverse_dynamics(forward_dynamics(tau)) returns tau at the inverse-dynamics bar (a backward
    error: free of conditioning).  tau = None reads the feed-forward rows rsb_set_generalized_force wrote: the same bits."""
    c, d = dyn_case(name), device(name)
    assert np.isfinite(d.fd).all() and np.isfinite(d.fd_plain).all()
    if c.fixed:
        assert not d.fd[:, :6].any() and not d.fd_plain[:, :6].any()
    assert np.array_equal(d.fd_ff, d.fd) and not np.array_equal(d.fd_plain, d.fd)
    mag = load_jacobians(name)[1]
    S = (np.einsum("eij,ej->ei", np.abs(c.M), np.abs(masked(c, d.fd.astype(np.float64)))) + np.abs(c.h) + mag).max(axis=1)
    for e in range(c.N):
        diff = (d.round[e].astype(np.float64) - c.tau[e])[c.j0:]
        assert np.abs(diff).max() <= 2e-5 * (1 + S[e]), (name, e, np.abs(diff).max() / (2e-5 * (1 + S[e])))
    fr = forward_reference(name)
    r = udot_ratio(c, d.fd, fr)
    print(f"{name}: E32 {fr.E32:.3e}, ABA32 {ABA32[name]:.3e}, udot error / (4 ABA32), worst env {r.max():.3f} (= {r.max() * ABA32[name] / fr.E32:.2f} x 4 E32)")
    assert r.max() <= 1.0, (name, int(r.argmax()), r.max())


def guarded(shape, torch_device=None):
    """(buffer with one guard row before and after, the view of the rows between): a store outside the output shows in the guards"""
    full = (shape[0] + 2,) + tuple(shape[1:])
    if torch_device is None:
        buf = np.full(full, 7.0, np.float32)
    else:
        import torch
        buf = torch.full(full, 7.0, dtype=torch.float32, device=torch_device)
    return buf, buf[1:-1]


def guards_intact(buf):
    a = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    return bool(np.all(a[0] == 7.0) and np.all(a[-1] == 7.0))


@pytest.mark.parametrize("name", ["floating5", "fixed2", "tree40", "anymal"])
def test_determinism_memory_spaces_and_single_outputs(built_lib, name):
    """Worlds of 1, 7, 8, 9 and all envs from the first rows of the same batch (env blocks of 15, 25, 6 and 19 envs: tails, and workgroup borders
    crossed): env e's outputs have the bits of the full world's - in host arrays and in torch tensors, with all outputs together and each alone - and
    the rows around every output are untouched."""
    import torch
    dev0 = torch.device("cuda:0")
    c, full = dyn_case(name), device(name)
    host = lambda v: v if isinstance(v, np.ndarray) else v.cpu().numpy()
    for n in (1, 7, 8, 9, c.N):
        w = new_world(c, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        shapes = dict(tau=(n, c.nv), joint_force=(n, c.nb, 3), joint_torque=(n, c.nb, 3))
        for td in (None, dev0):
            put = (lambda a: a) if td is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(td))
            loads = (c.frames, put(c.force[:n]), put(c.torque[:n]))
            udot, tau = put(c.udot[:n]), put(c.tau[:n])
            bufs = {k: guarded(s, td) for k, s in shapes.items()}
            got = w.inverse_dynamics(udot, loads=loads, out={k: v for k, (_, v) in bufs.items()})
            bu, vu = guarded((n, c.nv), td)
            assert w.forward_dynamics(tau, loads=loads, out=vu) is vu
            if td is not None:
                torch.cuda.synchronize()
            for k in OUT:
                assert np.array_equal(host(got[k]), full.loads[k][:n]) and guards_intact(bufs[k][0]), (name, n, td, k)
            assert np.array_equal(host(vu), full.fd[:n]) and guards_intact(bu), (name, n, td)
            for k in OUT:                       # each output alone: the others are NULL
                b1, v1 = guarded(shapes[k], td)
                w.inverse_dynamics(udot, loads=loads, out={k: v1})
                assert np.array_equal(host(v1), full.loads[k][:n]) and guards_intact(b1), (name, n, td, k)
        one = w.inverse_dynamics(None, tau=False, joint_torque=True)
        assert sorted(one) == ["joint_torque"] and np.array_equal(one["joint_torque"], full.h["joint_torque"][:n])
        w.close()


@pytest.mark.parametrize("name", ["fixed1", "fixed3"])
def test_a_fixed_bases_rows_do_not_matter(built_lib, name):
    """other noise in the six base rows of gv, udot and tau of a fixed base: not one bit of any output changes"""
    c, full = dyn_case(name), device(name)
    rng = np.random.default_rng(1)
    gv, udot, tau = c.gv.copy(), c.udot.copy(), c.tau.copy()
    for x in (gv, udot, tau):
        x[:, :6] = f32(rng.normal(size=(c.N, 6)) * 10)
    w = new_world(c, gv=gv)
    got = w.inverse_dynamics(udot, loads=loads_of(c), **ALL)
    fd = w.forward_dynamics(tau, loads=loads_of(c))
    w.close()
    for k in OUT:
        assert np.array_equal(got[k], full.loads[k]), k
    assert np.array_equal(fd, full.fd)


def test_queries_leave_the_world_alone_and_follow_pipelined_steps(built_lib):
    """Control steps of the benchmark's quadruped world, K = 3.  (a) lock-step with both queries (contacts on) between the steps: the state after every
    step and the contact list after the last are those of a run without the queries, bit for bit - the third step would show a changed warm state.
    (b) pipelined, the queries enqueued without an explicit join: the results of the lock-step run at the same point."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, K = 128, 3
    r = bench.Recipe(2, -1.0)
    model = r.model
    gc0, gv0 = standing_states(n, seed=9)
    dev = torch.device("cuda:0")
    bank = torch.from_numpy(np.stack([r.targets(n, k, 0).astype(np.float32) for k in range(K)])).to(dev)
    g0, v0 = torch.from_numpy(gc0.astype(np.float32)).to(dev), torch.from_numpy(gv0.astype(np.float32)).to(dev)
    feet = np.asarray(r.feet, np.int32)
    rng = np.random.default_rng(4)
    udot, tau = f32(rng.normal(size=(n, model.nv))), f32(rng.normal(size=(n, model.nv)))
    runs = {}
    for mode in ("plain", "queried", "pipelined"):
        w = BatchedWorld(model, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        r.setup_world(w, n, 0)
        w.set_state(gc0, gv0)
        w.set_pd_target(None, np.zeros((n, model.nv), np.float32))
        obs = torch.zeros((K, n, w.obs_dim(len(feet))), dtype=torch.float32, device=dev)
        if mode == "pipelined":
            assert w.set_step_pipelining(True) is not False and w.step_pipelining_enabled()
        step = w.control_step_plan(workload.SUBSTEPS, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), n)
        states, answers = [], []
        for k in range(K):
            step(bank[k].data_ptr())
            if mode != "plain":
                answers.append((w.inverse_dynamics(udot, contacts=True, **ALL), w.forward_dynamics(tau, contacts=True)))
            if mode != "pipelined":
                states.append(w.get_state())
        states.append(w.get_state())
        runs[mode] = (states, w.get_contacts(), answers)
        w.close()
    for (qa, ua), (qb, ub) in zip(runs["plain"][0], runs["queried"][0]):
        assert np.array_equal(qa, qb) and np.array_equal(ua, ub)
    assert np.array_equal(runs["plain"][1][0], runs["queried"][1][0]) and runs["plain"][1][1].tobytes() == runs["queried"][1][1].tobytes()
    assert runs["plain"][1][0].sum() > 0
    for (ia, fa), (ib, fb) in zip(runs["queried"][2], runs["pipelined"][2]):
        for k in OUT:
            assert np.array_equal(ia[k], ib[k]), k
        assert np.array_equal(fa, fb)
    assert np.array_equal(runs["pipelined"][0][-1][0], runs["plain"][0][-1][0])


def test_bad_input_fails_loudly_and_touches_nothing(built_lib, anymal):
    """every argument error of rsb.h: RSB_E_INVALID, a message, the guard pattern of the outputs intact"""
    n = 8
    gc, gv = workload.random_state(anymal.nq, anymal.nv, n, seed=4)
    w = BatchedWorld(anymal, n)
    w.set_state(gc, gv)
    L, h = w.L, w.handle
    out = np.full((n, 3 * anymal.nv), 7.0, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    inp = np.zeros((n, 64 * 3), np.float32)
    q = inp.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 2)()
    fr[1].body = 3
    bad_body, bad_off = (_capi.Frame * 1)(), (_capi.Frame * 1)()
    bad_body[0].body = anymal.nb
    bad_off[0].offset[1] = float("nan")
    cases = [
        (lambda: L.rsb_inverse_dynamics(h, q, None, 0, None, None, 0, None, None, None, 0), b"every output is NULL"),
        (lambda: L.rsb_forward_dynamics(h, q, None, 0, None, None, 0, None, 1), b"NULL"),
        (lambda: L.rsb_inverse_dynamics(h, q, fr, -1, q, q, 0, p, p, p, 0), b"n_frames"),
        (lambda: L.rsb_inverse_dynamics(h, q, fr, 65, q, q, 0, p, p, p, 0), b"n_frames"),
        (lambda: L.rsb_forward_dynamics(h, q, fr, 65, q, q, 0, p, 0), b"n_frames"),
        (lambda: L.rsb_inverse_dynamics(h, q, fr, 2, None, None, 0, p, p, p, 0), b"both NULL"),
        (lambda: L.rsb_forward_dynamics(h, q, fr, 2, None, None, 0, p, 0), b"both NULL"),
        (lambda: L.rsb_inverse_dynamics(h, q, None, 2, q, q, 0, p, p, p, 0), b"frames is NULL"),
        (lambda: L.rsb_inverse_dynamics(h, q, bad_body, 1, q, None, 0, p, p, p, 0), b"body"),
        (lambda: L.rsb_forward_dynamics(h, q, bad_off, 1, None, q, 0, p, 0), b"non-finite"),
        (lambda: L.rsb_inverse_dynamics(h, q, None, 0, None, None, 2, p, p, p, 0), b"flag"),
        (lambda: L.rsb_forward_dynamics(h, q, None, 0, None, None, 6, p, 0), b"flag"),
        (lambda: L.rsb_inverse_dynamics(h, q, None, 0, None, None, 0, p, p, p, 2), b"space"),
        (lambda: L.rsb_forward_dynamics(h, q, None, 0, None, None, 0, p, -1), b"space"),
    ]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k          # RSB_E_INVALID
        assert msg in L.rsb_last_error(), (k, L.rsb_last_error())
        assert np.all(out == 7.0), k
    with pytest.raises(ValueError):
        w.inverse_dynamics(tau=False)
    with pytest.raises(ValueError):
        w.inverse_dynamics(out={"wrench": out})
    with pytest.raises(ValueError):
        w.forward_dynamics(np.zeros((n, 3), np.float32))
    assert L.rsb_inverse_dynamics(h, None, None, 0, None, None, 0, p, None, None, 0) == 0      # n_frames = 0 with frames NULL is a valid call
    w.close()


def test_parity_record(built_lib):
    """The largest error / bar per quantity and model over all cases and variants, written to profiles/r12_dynamics_parity.txt (the figures DESIGN.md
    quotes).  Every figure has to be <= 1: this is the union of the parity tests above."""
    lines, fails = [], []
    for name in NAMES:
        c, d = dyn_case(name), device(name)
        worst = dict(tau=0.0, joint_force=0.0, joint_torque=0.0)
        for variant in ("h", "udot", "loads", "static"):
            got, ref = getattr(d, variant), reference(name, variant)
            if variant != "static":
                worst["tau"] = max(worst["tau"], tau_ratio(c, got["tau"], oracle_tau(c, variant), variant).max())
            rf, rt = wrench_ratios(got, ref)
            worst["joint_force"], worst["joint_torque"] = max(worst["joint_force"], rf.max()), max(worst["joint_torque"], rt.max())
        fr = forward_reference(name, True)
        worst["udot"] = udot_ratio(c, d.fd, fr).max()
        lines.append(f"  {name:10s} N {c.N:3d} nb {c.nb:3d}  tau {worst['tau']:.3f}  joint_force {worst['joint_force']:.3f}  joint_torque {worst['joint_torque']:.3f}  "
                     f"udot {worst['udot']:.3f} (ABA32 {ABA32[name]:.2e}, E32 {fr.E32:.2e})\n")
        fails += [(name, k, v) for k, v in worst.items() if not v <= 1.0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r12_dynamics_parity.txt"), "w") as f:
        f.write("tests/test_gpu_dynamics.py::test_parity_record\n"
                "device fp32 vs fp64 references on the float32-rounded state; largest error / bar over the envs and the variants (udot = NULL, udot, udot + three loads, at rest).\n"
                "bars: tau 2e-5 (1 + S_e), S_e = largest row of |M||udot| + |h| + sum |J^T||w|; joint wrenches 2e-5 (1 + sum of absolute terms); udot 4 ABA32 (1 + max|udot_ref|)\n" +
                "".join(lines))
    print("".join(lines))
    assert not fails, fails
