"""Batched centre of mass, momentum, energy and the centroidal momentum matrix on the device (rsb_get_centroidal, rsb_get_centroidal_momentum_matrix;
raisimlib_amd/csrc/rsb_centroidal.hip) against the fp64 oracle on the float32-rounded state the device saw.

Reference per env, from the oracle alone: T, U = Oracle.energy; P, L_0 = Oracle.momentum (about the world origin); c_i, J_i = Oracle.point_jacobian(q, i,
com_i), c = sum m_i c_i / M, L_c = L_0 - c x P; column d of A = (P, L_0 - c x P) of Oracle.momentum(q, e_d).  For a fixed-base model the base entries of
u are zeroed before the oracle is called.
Bounds per env: the project's bars of its fp32 queries (1e-5 positions, 2e-5 velocities; tests/test_gpu_frames.py) times the output's physical scale, with
M the total mass, v_max the largest body-COM speed of the env and r_max the largest body-COM distance from c (both from the oracle):
  com 1e-5 (1 + |c|)      com_vel 2e-5 (1 + v_max)      lin_mom 2e-5 M (1 + v_max)      ang_mom 2e-5 M (1 + v_max)(1 + r_max)
  kinetic 4e-5 (1 + T)    potential 1e-5 M |g| (1 + |c|)      A 1e-5 (1 + max |A_ref|) over the env's matrix
Every env of every case is compared.  The parity test writes the largest error / bound it saw per quantity and model to
profiles/r11_centroidal_parity.txt.
"""
import os

import numpy as np
import pytest

from common import ROOT, Oracle, f32, sphere_urdf, standing_states
from raisimlib_amd import BatchedWorld, Model, _capi, workload
from test_gpu_frames import ARM_URDF

pytestmark = pytest.mark.gpu

N = 67
NAMES = ("com", "com_vel", "lin_mom", "ang_mom", "kinetic", "potential")
ALL = {n: True for n in NAMES}
G = np.array([0.0, 0.0, -9.81])
_cache = {}


def masses(model):
    return np.array([model.blob.mass[i] for i in range(model.nb)])


def bars(M, cn, vmax, rmax, T, gn=9.81):
    return dict(com=1e-5 * (1 + cn), com_vel=2e-5 * (1 + vmax), lin_mom=2e-5 * M * (1 + vmax), ang_mom=2e-5 * M * (1 + vmax) * (1 + rmax),
                kinetic=4e-5 * (1 + T), potential=1e-5 * M * gn * (1 + cn))


def oracle_centroidal(o, model, q, u):
    """-> reference dict of one env (q, u fp64: the float32-rounded row), with the scales of its bounds"""
    b, m = model.blob, masses(model)
    u = u.copy()
    if b.fixed_base:
        u[:6] = 0.0
    T, U = o.energy(q, u)
    P, L0 = o.momentum(q, u)
    ci, vi = np.zeros((model.nb, 3)), np.zeros((model.nb, 3))
    for i in range(model.nb):
        ci[i], J = o.point_jacobian(q, i, np.array([b.com[i][k] for k in range(3)]))
        if b.fixed_base:
            J = J.copy(); J[:, :6] = 0.0
        vi[i] = J @ u
    M = m.sum()
    c = (m[:, None] * ci).sum(axis=0) / M
    A = np.zeros((6, model.nv))
    for d in range(6 if b.fixed_base else 0, model.nv):
        e = np.zeros(model.nv); e[d] = 1.0
        Pd, Ld = o.momentum(q, e)
        A[:3, d], A[3:, d] = Pd, Ld - np.cross(c, Pd)
    return dict(com=c, com_vel=P / M, lin_mom=P, ang_mom=L0 - np.cross(c, P), kinetic=T, potential=U, A=A, M=M,
                vmax=float(np.linalg.norm(vi, axis=1).max()), rmax=float(np.linalg.norm(ci - c, axis=1).max()))


def stepped(model, name, gc0, gv0):
    """what the device holds after 5 control steps from (gc0, gv0) on flat ground: contacts and large joint velocities"""
    n = gc0.shape[0]
    w = BatchedWorld(model, n)
    w.add_ground(0.0)
    w.set_control_mode(1)
    if name == "anymal_c_like":
        w.set_pd_gains(*workload.anymal_gains())
        targets = lambda k: workload.anymal_targets(n, k)
    else:
        w.set_max_contacts(16)
        w.set_pd_gains(*workload.atlas_gains(model.nv))
        targets = lambda k: workload.atlas_targets(n, k, model.nq)
    w.set_state(gc0, gv0)
    contacts = 0
    for k in range(5):
        w.set_pd_target(targets(k), np.zeros((n, model.nv)))
        w.integrate(workload.SUBSTEPS)
        contacts += int(w.get_contacts()[0].sum())
    gc, gv = w.get_state()
    w.close()
    assert contacts > 0 and np.all(np.isfinite(gc)) and np.all(np.isfinite(gv))
    return gc, gv


def case(name, anymal, atlas):
    """the state batch of one model (float32, as the device holds it), the device's outputs for it and the oracle's references; computed once"""
    if name in _cache:
        return _cache[name]
    model = anymal if name == "anymal_c_like" else atlas
    if name == "anymal_c_like":
        gc0, gv0 = standing_states(N, seed=21)
    else:
        gc0, gv0 = workload.random_state(model.nq, model.nv, N, seed=22, z_range=(0.9, 1.2))
    far = np.arange(N) % 4 == 0                       # one env in four stands 50 m from the origin
    ang = np.random.default_rng(5).uniform(0, 2 * np.pi, N)
    gc0[far, 0] += 50.0 * np.cos(ang[far]); gc0[far, 1] += 50.0 * np.sin(ang[far])
    gc0, gv0 = gc0.astype(np.float32), gv0.astype(np.float32)
    gc1, gv1 = stepped(model, name, gc0, gv0)
    half = N // 2 + 1
    gc, gv = gc0.copy(), gv0.copy()
    gc[half:], gv[half:] = gc1[half:], gv1[half:]     # rows [half, N): after the control steps
    assert far[:half].any() and far[half:].any()
    w = BatchedWorld(model, N)
    w.set_state(gc, gv)
    dev = w.centroidal(**ALL)
    dev["A"] = w.centroidal_momentum_matrix()
    w.close()
    o = Oracle(model.blob)
    ref = [oracle_centroidal(o, model, f32(gc[e]), f32(gv[e])) for e in range(N)]
    _cache[name] = (model, gc, gv, dev, ref)
    return _cache[name]


def ratios(dev, ref, e):
    """error / bound of every quantity of env e"""
    r = ref[e]
    b = bars(r["M"], np.linalg.norm(r["com"]), r["vmax"], r["rmax"], r["kinetic"])
    out = {n: float(np.abs(np.asarray(dev[n][e], np.float64) - r[n]).max() / b[n]) for n in NAMES}
    out["A"] = float(np.abs(dev["A"][e].astype(np.float64) - r["A"]).max() / (1e-5 * (1 + np.abs(r["A"]).max())))
    return out


def test_parity_with_the_oracle(anymal, atlas):
    """ANYmal-like and Atlas-like, N = 67: half the envs at drawn states, half after 5 control steps on the ground, one in four 50 m from the origin;
    all six outputs and the matrix within their bounds in every env.
    Measured on an MI355X (profiles/r11_centroidal_parity.txt): see the file; the largest error / bound of any quantity is reported there."""
    report, fails = [], []
    for name in ("anymal_c_like", "atlas_like"):
        model, gc, gv, dev, ref = case(name, anymal, atlas)
        worst = {}
        for e in range(N):
            for n, v in ratios(dev, ref, e).items():
                if v > worst.get(n, (0.0, -1))[0]:
                    worst[n] = (v, e)
        print(name, {n: f"{v:.3f} (env {e})" for n, (v, e) in worst.items()})
        report.append(f"{name}: N = {N}, {model.nb} bodies, envs {N // 2 + 1}..{N - 1} after 5 control steps, every fourth env 50 m from the origin\n" +
                      "".join(f"  {n:9s} largest error / bound over the envs = {v:.3f}   (env {e})\n" for n, (v, e) in worst.items()))
        fails += [(name, n, v, e) for n, (v, e) in worst.items() if not v <= 1.0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r11_centroidal_parity.txt"), "w") as f:
        f.write("tests/test_gpu_centroidal.py::test_parity_with_the_oracle\n"
                "device fp32 vs the fp64 oracle on the float32-rounded state; bounds per env: com 1e-5 (1 + |c|), com_vel 2e-5 (1 + v_max), lin_mom 2e-5 M (1 + v_max),\n"
                "ang_mom 2e-5 M (1 + v_max)(1 + r_max), kinetic 4e-5 (1 + T), potential 1e-5 M |g| (1 + |c|), A 1e-5 (1 + max |A_ref|)\n" + "".join(report))
    assert not fails, fails


def test_consistency_without_the_oracle(anymal, atlas):
    """A gv = (lin_mom, ang_mom) under the momentum bounds; A[:, :3, :3] = M 1 to 1e-6 M; A[:, 3:, 3:6] symmetric to the A bound; com_vel M = lin_mom."""
    for name in ("anymal_c_like", "atlas_like"):
        model, gc, gv, dev, ref = case(name, anymal, atlas)
        M = model.total_mass()
        for e in range(N):
            r = ref[e]
            b = bars(r["M"], np.linalg.norm(r["com"]), r["vmax"], r["rmax"], r["kinetic"])
            A = dev["A"][e].astype(np.float64)
            h = A @ f32(gv[e])
            assert np.abs(h[:3] - dev["lin_mom"][e]).max() <= b["lin_mom"], (name, e)
            assert np.abs(h[3:] - dev["ang_mom"][e]).max() <= b["ang_mom"], (name, e)
            assert np.abs(A[:3, :3] - M * np.eye(3)).max() <= 1e-6 * M, (name, e)
            assert np.abs(A[3:, 3:6] - A[3:, 3:6].T).max() <= 1e-5 * (1 + np.abs(r["A"]).max()), (name, e)
            assert np.abs(dev["com_vel"][e].astype(np.float64) * M - dev["lin_mom"][e]).max() <= b["lin_mom"], (name, e)


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


def test_indexing_determinism_memory_spaces_and_single_outputs(anymal, atlas):
    """Worlds of N = 1, 7, 8, 9, 19, 20 and 67 from the first rows of the same batch (the env blocks - 19 envs per workgroup at 13 bodies, 8 at 31 - have
    tails and cross workgroups): env e's outputs have the bits of the 67-env world's, in host arrays and in torch tensors, with every output asked for
    alone; the rows around every output are untouched."""
    import torch
    dev0 = torch.device("cuda:0")
    for name in ("anymal_c_like", "atlas_like"):
        model, gc, gv, full, _ = case(name, anymal, atlas)
        shapes = lambda n: dict(com=(n, 3), com_vel=(n, 3), lin_mom=(n, 3), ang_mom=(n, 3), kinetic=(n,), potential=(n,))
        for n in (1, 7, 8, 9, 19, 20, 67):
            w = BatchedWorld(model, n)
            w.set_stream(torch.cuda.current_stream().cuda_stream)
            w.set_state(gc[:n], gv[:n])
            for td in (None, dev0):
                bufs = {k: guarded(s, td) for k, s in shapes(n).items()}
                got = w.centroidal(out={k: v for k, (_, v) in bufs.items()})
                bA, vA = guarded((n, 6, model.nv), td)
                assert w.centroidal_momentum_matrix(out=vA) is vA
                if td is not None:
                    torch.cuda.synchronize()
                host = lambda v: v if isinstance(v, np.ndarray) else v.cpu().numpy()
                for k in NAMES:
                    assert np.array_equal(host(got[k]), full[k][:n]), (name, n, td, k)
                    assert guards_intact(bufs[k][0]), (name, n, td, k)
                assert np.array_equal(host(vA), full["A"][:n]) and guards_intact(bA), (name, n, td)
                for k in NAMES:                       # each output alone: the others are NULL
                    b1, v1 = guarded(shapes(n)[k], td)
                    w.centroidal(out={k: v1})
                    assert np.array_equal(host(v1), full[k][:n]) and guards_intact(b1), (name, n, td, k)
            one = w.centroidal(com=False, ang_mom=True)
            assert sorted(one) == ["ang_mom"] and np.array_equal(one["ang_mom"], full["ang_mom"][:n])
            w.close()


def quat_rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def check(dev, e, ref, M, vmax, rmax, names=NAMES):
    b = bars(M, np.linalg.norm(ref["com"]), vmax, rmax, ref["kinetic"], gn=np.linalg.norm(ref.get("g", G)))
    for n in names:
        err = np.abs(np.asarray(dev[n][e], np.float64) - ref[n]).max()
        assert err <= b[n], (n, e, err, b[n])


def test_free_sphere_in_closed_form_and_in_free_fall(built_lib):
    """A free sphere whose centre of mass sits off its centre, spinning and translating: com = p + R c, P = m v_c with v_c = v + w x R c, L_c = I w (isotropic),
    T = 1/2 m v_c^2 + 1/2 I w^2, U = -m g . com.  After 8 sub-steps of free fall P = m (v_c + 8 dt g) within 2e-5 m (1 + |v|).  (|c| = 0.03 m and |w| of
    the order of 1 rad/s: what the semi-implicit step itself adds to P, of the order of m |c| w^2 dt^2 per sub-step, stays below a tenth of that bound.)"""
    m, rad, dt, n = 2.0, 0.1, 0.0025, 20
    blob = Model(urdf_string=sphere_urdf(m, rad)).blob
    c = f32((0.02, -0.015, 0.01))
    for k in range(3):
        blob.com[0][k] = c[k]
    ball = Model(blob=blob)
    I = 0.4 * m * rad * rad
    gc, gv = workload.random_state(ball.nq, ball.nv, n, seed=8, z_range=(5.0, 6.0))
    gv[:, 3:] = np.random.default_rng(8).uniform(-1, 1, (n, 3))
    gc, gv = f32(gc), f32(gv)
    w = BatchedWorld(ball, n)
    w.add_ground(0.0)
    w.set_time_step(dt)
    w.set_state(gc, gv)
    dev = w.centroidal(**ALL)
    A = w.centroidal_momentum_matrix()
    vc0 = np.zeros((n, 3))
    for e in range(n):
        R = quat_rot(gc[e, 3:7])
        Rc = R @ c
        vc = gv[e, :3] + np.cross(gv[e, 3:], Rc)
        vc0[e] = vc
        com = gc[e, :3] + Rc
        ref = dict(com=com, com_vel=vc, lin_mom=m * vc, ang_mom=I * gv[e, 3:], kinetic=0.5 * m * vc @ vc + 0.5 * I * gv[e, 3:] @ gv[e, 3:], potential=-m * G @ com)
        check(dev, e, ref, m, np.linalg.norm(vc), 0.0)
        Aref = np.zeros((6, 6)); Aref[:3, :3] = m * np.eye(3); Aref[3:, 3:] = I * np.eye(3)
        Aref[:3, 3:] = -m * np.array([[0, -Rc[2], Rc[1]], [Rc[2], 0, -Rc[0]], [-Rc[1], Rc[0], 0]])      # e x (m R c)
        assert np.abs(A[e] - Aref).max() <= 1e-5 * (1 + np.abs(Aref).max()), e
    w.integrate(8)
    P = w.centroidal(com=False, lin_mom=True)["lin_mom"]
    cnt, _ = w.get_contacts()
    assert cnt.sum() == 0
    w.close()
    for e in range(n):
        v = vc0[e] + 8 * dt * G
        err = np.abs(P[e] - m * v).max()
        print("free fall, env", e, "error / bound", err / (2e-5 * m * (1 + np.linalg.norm(v))))
        assert err <= 2e-5 * m * (1 + np.linalg.norm(v)), (e, err)


def test_two_link_arm_on_a_fixed_base_in_closed_form_and_gravity(built_lib):
    """The arm of tests/test_gpu_frames.py rooted at `world` (mount 1 kg at (0, 0, 0.5); upper 1 kg, centre of mass 0.15 m out on the rotating x axis; slider
    0.5 kg, 0.4 m + d out), with non-zero base entries in gv that must be ignored: all outputs against the closed form, the six base columns of A exactly zero.
    Then rsb_set_gravity: potential follows the new vector, every other output keeps its bits."""
    model = Model(urdf_string=ARM_URDF)
    assert model.blob.fixed_base == 1 and model.nb == 3 and model.nv == 8
    n = 20
    rng = np.random.default_rng(3)
    th, d = f32(rng.uniform(-3, 3, n)), f32(rng.uniform(-0.2, 0.4, n))
    thd, dd = f32(rng.normal(size=n)), f32(rng.normal(size=n))
    gc = np.zeros((n, 9)); gc[:, 3] = 1.0; gc[:, 7], gc[:, 8] = th, d
    gv = np.zeros((n, 8)); gv[:, :6] = rng.normal(size=(n, 6)); gv[:, 6], gv[:, 7] = thd, dd
    w = BatchedWorld(model, n)
    w.set_state(gc, gv)
    dev = w.centroidal(**ALL)
    A = w.centroidal_momentum_matrix()
    mass, izz = np.array([1.0, 1.0, 0.5]), np.array([1e-2, 1e-2, 1e-3])
    M = mass.sum()
    refs = []
    for e in range(n):
        c, s, L = np.cos(th[e]), np.sin(th[e]), 0.4 + d[e]
        ci = np.array([[0, 0, 0.5], [0.15 * c, 0.15 * s, 0.5], [L * c, L * s, 0.5]])
        vi = np.array([[0, 0, 0], [-0.15 * thd[e] * s, 0.15 * thd[e] * c, 0], [-L * thd[e] * s + dd[e] * c, L * thd[e] * c + dd[e] * s, 0]])
        wz = np.array([0, thd[e], thd[e]])
        com = (mass[:, None] * ci).sum(axis=0) / M
        P = (mass[:, None] * vi).sum(axis=0)
        L0 = (mass[:, None] * np.cross(ci, vi)).sum(axis=0) + np.array([0, 0, (izz * wz).sum()])
        T = 0.5 * (mass * (vi * vi).sum(axis=1)).sum() + 0.5 * (izz * wz * wz).sum()
        ref = dict(com=com, com_vel=P / M, lin_mom=P, ang_mom=L0 - np.cross(com, P), kinetic=T, potential=-M * G @ com)
        vmax, rmax = np.linalg.norm(vi, axis=1).max(), np.linalg.norm(ci - com, axis=1).max()
        check(dev, e, ref, M, vmax, rmax)
        refs.append((ref, vmax, rmax))
        u = f32(gv[e]); u[:6] = 0.0
        h = A[e].astype(np.float64) @ u
        b = bars(M, np.linalg.norm(com), vmax, rmax, T)
        assert np.abs(h[:3] - P).max() <= b["lin_mom"] and np.abs(h[3:] - ref["ang_mom"]).max() <= b["ang_mom"], e
    assert np.all(A[:, :, :6] == 0.0)
    g2 = np.array([0.5, -0.3, -3.7])
    w.set_gravity(g2)
    dev2 = w.centroidal(**ALL)
    assert np.array_equal(w.centroidal_momentum_matrix(), A)
    w.close()
    for k in NAMES[:-1]:
        assert np.array_equal(dev2[k], dev[k]), k
    assert not np.array_equal(dev2["potential"], dev["potential"])
    for e, (ref, vmax, rmax) in enumerate(refs):
        check(dev2, e, dict(ref, potential=-M * g2 @ ref["com"], g=g2), M, vmax, rmax, names=("potential",))


def test_follows_the_state_in_lockstep_pipelined_and_resident_runs(built_lib):
    """The queries enqueued behind rsb_control_step in lock-step, behind a pipelined run without an explicit join and behind a resident rsb_control_steps
    launch equal, bit for bit, the queries of a second world that was set to the first world's downloaded state."""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, K = 512, 5
    r = bench.Recipe(2, -1.0)
    model = r.model
    gc0, gv0 = standing_states(n, seed=9)
    dev = torch.device("cuda:0")
    bank = torch.from_numpy(np.stack([r.targets(n, k, 0).astype(np.float32) for k in range(K)])).to(dev)
    g0, v0 = torch.from_numpy(gc0.astype(np.float32)).to(dev), torch.from_numpy(gv0.astype(np.float32)).to(dev)
    feet = np.asarray(r.feet, np.int32)
    states = {}
    for mode in ("lockstep", "pipelined", "resident"):
        w = BatchedWorld(model, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        r.setup_world(w, n, 0)
        w.set_state(gc0, gv0)
        w.set_pd_target(None, np.zeros((n, model.nv), np.float32))
        od = w.obs_dim(len(feet))
        obs = torch.zeros((K, n, od), dtype=torch.float32, device=dev)
        if mode == "resident":
            w.set_step_residency(True)
            assert w.residency_status(0)
            w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K, obs.data_ptr(), n * od, feet, feet, g0.data_ptr(), v0.data_ptr(), n)(K, 0)
        else:
            if mode == "pipelined":
                assert w.set_step_pipelining(True) is not False and w.step_pipelining_enabled()
            step = w.control_step_plan(workload.SUBSTEPS, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), n)
            for k in range(K):
                step(bank[k].data_ptr())
        got = w.centroidal(**ALL)          # enqueued behind the steps: joins the pipeline / follows the resident launch on the world's stream
        got["A"] = w.centroidal_momentum_matrix()
        gc, gv = w.get_state()
        assert not np.array_equal(gc, gc0.astype(np.float32))
        if mode == "resident":
            assert w.residency_launches() == 1
        w.close()
        twin = BatchedWorld(model, n)
        twin.set_state(gc, gv)
        want = twin.centroidal(**ALL)
        want["A"] = twin.centroidal_momentum_matrix()
        twin.close()
        for k, v in want.items():
            assert np.array_equal(got[k], v), (mode, k)
        states[mode] = (gc, gv)
    for mode in ("pipelined", "resident"):
        assert np.array_equal(states[mode][0], states["lockstep"][0]) and np.array_equal(states[mode][1], states["lockstep"][1]), mode


def test_bad_input_fails_loudly_and_touches_nothing(anymal):
    """every output NULL, a bad space: RSB_E_INVALID; a model without mass: RSB_E_UNSUPPORTED; a message each time, the outputs untouched"""
    import ctypes as C
    n = 8
    gc, gv = workload.random_state(anymal.nq, anymal.nv, n, seed=4)
    w = BatchedWorld(anymal, n)
    w.set_state(gc, gv)
    L, h = w.L, w.handle
    out = np.full((n, 6 * anymal.nv), 7.0, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    cases = [
        (lambda: L.rsb_get_centroidal(h, None, None, None, None, None, None, 0), b"every output is NULL"),
        (lambda: L.rsb_get_centroidal(h, None, None, None, None, None, None, 1), b"every output is NULL"),
        (lambda: L.rsb_get_centroidal(h, p, None, None, None, None, None, 2), b"space"),
        (lambda: L.rsb_get_centroidal(h, p, p, p, p, p, p, -1), b"space"),
        (lambda: L.rsb_get_centroidal_momentum_matrix(h, None, 0), b"NULL"),
        (lambda: L.rsb_get_centroidal_momentum_matrix(h, p, 2), b"space"),
    ]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k          # RSB_E_INVALID
        assert msg in L.rsb_last_error(), (k, L.rsb_last_error())
        assert np.all(out == 7.0), k
    with pytest.raises(ValueError):
        w.centroidal(com=False)
    with pytest.raises(ValueError):
        w.centroidal(out={"momentum": out})
    w.close()
    blob = Model(urdf_string=sphere_urdf(2.0, 0.1)).blob
    blob.mass[0] = 0.0
    ghost = Model(blob=blob)
    w = BatchedWorld(ghost, n)
    L, h = w.L, w.handle
    for call in (lambda: L.rsb_get_centroidal(h, p, p, p, p, p, p, 0), lambda: L.rsb_get_centroidal_momentum_matrix(h, p, 0)):
        assert call() == -3          # RSB_E_UNSUPPORTED
        assert b"total mass is not positive" in L.rsb_last_error()
        assert np.all(out == 7.0)
    with pytest.raises(_capi.RsbError, match="total mass"):
        w.centroidal()
    w.close()
