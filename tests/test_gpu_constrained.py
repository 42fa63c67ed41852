"""Batched constrained dynamics and frame impulses on the device (rsb_constrained_forward_dynamics, rsb_frame_impulse;
raisimlib_amd/csrc/rsb_constrained.hip) through the C-ABI, against the fp64 KKT references of tests/constrained_reference.py on the float32-rounded
state the device saw.  Cases: floating0, fixed2 (N = 67), anymal, atlas (N = 64), EVERY env of EVERY variant (constrained_reference.variants: m = 3, 6,
9, 12, 18, 24, 36, 66, 96 rows; 67 envs at m = 96 are 34 workgroups).

Accuracy gates (free of conditioning; evaluated in fp64 with the reference's matrices and the device's udot / dgv and lambda, on every env with
status 0; c = 2e-5, the project's inverse-dynamics bar; constrained_reference.gates):
  dynamics row    |M udot + h - tau - J^T lambda|_inf <= c (1 + S), S the largest row of |M||udot| + |h| + |tau| + |J^T||lambda|
  constraint row  |J udot + Jdot gv - target_acc + rho lambda|_inf <= c (1 + S2), S2 the largest row of |J||udot_f| + |J||JMinv^T||lambda| + |Jdot gv| +
                  |target_acc| + (|G| + rho)|lambda|
  the impulse: the same with M + D, dgv (M (gv + dgv) - M gv), J gv and target_vel; fixed bases: the joint block.
Forward error, regular sets only: max|lambda - lambda_ref| / (1 + max|lambda_ref|) and the same for udot / dgv, at most 4 x the figure the kernel's
arithmetic restated in numpy float32 reaches on the case (tools/constrained_restatement.py -> profiles/constrained_restatement.txt, computed on the
CPU before any device run; the margin of 4 is the sibling queries').  The humanoid's figures are those of its free acceleration (UD32 of its one-frame
set is rsb_forward_dynamics' own 5.5e-4).
Status: a regular set 0 on every env; a dependent set without damping 1 on every env, lambda zeros and udot the bits of rsb_forward_dynamics (dgv
zeros); the same set with damping 1e-4 0 on every env and within both gates.
test_parity_record writes the device's measured ratios to profiles/constrained_parity.txt."""
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from common import ROOT, f32, standing_states
from raisimlib_amd import BatchedWorld, _capi, workload
from test_dynamics_reference import dyn_case
import constrained_reference as cr
import inverse_mass_reference as imr

pytestmark = pytest.mark.gpu

# constrained_reference.FWD32: the float32 restatement's forward figures, recomputed and pinned on the CPU by tests/test_constrained_reference.py
LAM32, UD32 = ({n: f["dyn"][k] for n, f in cr.FWD32.items()} for k in (0, 1))
ILAM32, DGV32 = ({n: f["imp"][k] for n, f in cr.FWD32.items()} for k in (0, 1))


def new_world(c, n=None):
    n = n or c.N
    w = BatchedWorld(c.model, n)
    w.set_state(c.gc[:n], c.gv[:n])
    return w


def t32(name, key, angular, which, n=None):
    return np.ascontiguousarray(cr.target(name, key, angular, which)[:n], np.float32)


def diag32(name):
    return imr.joint_diag(name).astype(np.float32)


def run_dyn(w, name, key, angular, damping, n=None, **kw):
    c = dyn_case(name)
    return w.constrained_forward_dynamics(cr.frame_sets(name)[key], tau=np.ascontiguousarray(c.tau[:n], np.float32), angular=angular,
                                          target_acc=t32(name, key, angular, "acc", n), damping=damping, **kw)


def run_imp(w, name, key, angular, damping, n=None, **kw):
    return w.frame_impulse(cr.frame_sets(name)[key], angular=angular, target_vel=t32(name, key, angular, "vel", n), joint_diag=diag32(name), damping=damping, **kw)


@functools.lru_cache(maxsize=None)
def device(name):
    """everything the device says about one case, computed once in one world"""
    c = dyn_case(name)
    w = new_world(c)
    d = SimpleNamespace(dyn={}, imp={}, uf=w.forward_dynamics(np.ascontiguousarray(c.tau, np.float32)))
    for v in cr.variants(name):
        d.dyn[v] = run_dyn(w, name, *v)
        d.imp[v] = run_imp(w, name, *v)
    q, u = w.get_state()
    assert np.array_equal(q, c.gc.astype(np.float32)) and np.array_equal(u, c.gv.astype(np.float32))      # no bit of the world changed
    w.close()
    return d


def ratios(name, v, out, impulse):
    """(dynamics gate, constraint gate, lambda forward / bar or None, udot / dgv forward / bar or None), per env"""
    key, angular, damping = v
    d = device(name)
    x, lam = out["dgv" if impulse else "udot"], out["lambda"]
    t = cr.target(name, key, angular, "vel" if impulse else "acc")
    dyn, con = cr.gates(name, key, angular, damping, impulse, x, lam, t, impulse, None if impulse else d.uf)
    fl = fx = None
    if cr.regular(name, key, angular):
        xr, lr = cr.impulse_reference(name, key, angular, 0.0, True) if impulse else cr.dynamics_reference(name, key, angular, 0.0)
        fl = cr.forward_error(lam, lr) / (4 * (ILAM32 if impulse else LAM32)[name])
        fx = cr.forward_error(x, xr) / (4 * (DGV32 if impulse else UD32)[name])
    return dyn, con, fl, fx


def check_variant(name, v, out, impulse, worst=None):
    key, angular, damping = v
    c, d = dyn_case(name), device(name)
    x, lam, st = out["dgv" if impulse else "udot"], out["lambda"], out["status"]
    m = cr.rows_of(name, key, angular)
    tag = f"{name} {key} ang={angular} damping={damping} {'impulse' if impulse else 'dynamics'}"
    assert x.shape == (c.N, c.nv) and lam.shape == (c.N, m) and st.shape == (c.N,) and st.dtype == np.int32
    if c.fixed:
        assert not x[:, :6].any(), tag
    if not cr.solvable(name, key, angular, damping):
        assert (st == _capi.RSB_HELD_SINGULAR).all(), (tag, np.flatnonzero(st != 1))
        assert not lam.any(), tag
        assert (not x.any()) if impulse else (x.tobytes() == d.uf.tobytes()), tag
        return
    assert (st == _capi.RSB_HELD_SOLVED).all(), (tag, np.flatnonzero(st != 0))
    assert np.isfinite(x).all() and np.isfinite(lam).all(), tag
    dyn, con, fl, fx = ratios(name, v, out, impulse)
    line = f"{tag}: dynamics row / gate {dyn.max():.3f}, constraint row / gate {con.max():.3f}"
    if fl is not None:
        line += f", lambda error / bar {fl.max():.3f}, {'dgv' if impulse else 'udot'} error / bar {fx.max():.3f}"
    print(line)
    if worst is not None:
        for k, val in (("dyn", dyn), ("con", con), ("lam", fl), ("x", fx)):
            if val is not None:
                worst[k] = max(worst.get(k, 0.0), float(val.max()))
        return
    assert dyn.max() <= 1.0 and con.max() <= 1.0, (tag, int(dyn.argmax()), dyn.max(), int(con.argmax()), con.max())
    if fl is not None:
        assert fl.max() <= 1.0 and fx.max() <= 1.0, (tag, fl.max(), fx.max())


@pytest.mark.parametrize("name", cr.CASES)
def test_constrained_forward_dynamics(built_lib, name):
    """every variant of the case: status, the two gates and on the regular sets the forward bars, on every env"""
    d = device(name)
    for v in cr.variants(name):
        check_variant(name, v, d.dyn[v], False)


@pytest.mark.parametrize("name", cr.CASES)
def test_frame_impulse(built_lib, name):
    """the same for the impulse, with joint_diag"""
    d = device(name)
    for v in cr.variants(name):
        check_variant(name, v, d.imp[v], True)
    v = cr.variants(name)[-1]
    if cr.solvable(name, *v):      # joint_diag changes the result
        w = new_world(dyn_case(name))
        plain = w.frame_impulse(cr.frame_sets(name)[v[0]], angular=v[1], target_vel=t32(name, v[0], v[1], "vel"), damping=v[2])
        w.close()
        assert not np.array_equal(plain["dgv"], d.imp[v]["dgv"])


@pytest.mark.parametrize("name", cr.CASES)
def test_cross_checks_through_the_other_kernels(built_lib, name):
    """No reference's solution is involved: with the device's own udot, rsb_get_frame_accelerations at the held frames gives target_acc - rho lambda
    within c (1 + S2); after rsb_set_state(gv + dgv) rsb_get_frame_kinematics' velocities are target_vel - rho lambda within the impulse's c (1 + S2);
    with lambda handed to rsb_forward_dynamics as loads at the frames, it returns a udot that meets the dynamics gate with that lambda."""
    c, d = dyn_case(name), device(name)
    w = new_world(c)
    tau = np.ascontiguousarray(c.tau, np.float32)
    for v in cr.variants(name):
        key, angular, damping = v
        if not cr.solvable(name, *v):
            continue
        frames, kk = cr.frame_sets(name)[key], 6 if angular else 3
        F = len(frames)
        stack = lambda lin, ang: np.concatenate([lin, ang], axis=2).reshape(c.N, -1) if angular else lin.reshape(c.N, -1)
        out = d.dyn[v]
        lam = out["lambda"].astype(np.float64)
        t = cr.target(name, key, angular, "acc")
        acc = w.frame_accelerations(frames, udot=out["udot"], lin=True, ang=True)
        got = stack(acc["lin"], acc["ang"]).astype(np.float64)
        rho = cr.rho_of(name, key, angular, False, damping)
        S2 = bar_scale(name, key, angular, damping, False, out["udot"], lam, t, d.uf)
        res = np.abs(got - t + rho[:, None] * lam).max(axis=1)
        assert (res <= cr.C_BAR * (1 + S2)).all(), (name, v, (res / (cr.C_BAR * (1 + S2))).max())
        l3 = lam.reshape(c.N, F, kk)
        force = np.ascontiguousarray(l3[:, :, :3], np.float32)
        torque = np.ascontiguousarray(l3[:, :, 3:], np.float32) if angular else None
        u2 = w.forward_dynamics(tau, loads=(frames, force, torque))
        dyn, _ = cr.gates(name, key, angular, damping, False, u2, lam, t, False, d.uf)
        assert dyn.max() <= 1.0, (name, v, dyn.max())
        # the impulse: a world of its own state
        imp = d.imp[v]
        tv = cr.target(name, key, angular, "vel")
        w.set_state(None, (c.gv + imp["dgv"].astype(np.float64)).astype(np.float32))
        kin = w.frame_kinematics(frames, pos=False, lin_vel=True, ang_vel=True)
        w.set_state(None, c.gv)
        gotv = stack(kin["lin_vel"], kin["ang_vel"]).astype(np.float64)
        li = imp["lambda"].astype(np.float64)
        rhoi = cr.rho_of(name, key, angular, True, damping)
        S2i = bar_scale(name, key, angular, damping, True, imp["dgv"], li, tv, None)
        # (gv + dgv is rounded to float32 once more on the way in: one rounding of |J||gv + dgv|, inside c S2's |J gv| + |J||JMinv^T||lambda| terms)
        resv = np.abs(gotv - tv + rhoi[:, None] * li).max(axis=1)
        assert (resv <= cr.C_BAR * (1 + S2i)).all(), (name, v, (resv / (cr.C_BAR * (1 + S2i))).max())
    w.close()


def bar_scale(name, key, angular, damping, impulse, x, lam, t, x_free):
    """S2 of constrained_reference.gates, per env"""
    c = dyn_case(name)
    j0 = c.j0
    J = np.abs(cr.stacked_jacobian(name, key, angular)[:, :, j0:])
    G, JM = cr.delassus(name, key, angular, impulse)
    rho = cr.rho_of(name, key, angular, impulse, damping)
    lam = np.abs(np.asarray(lam, np.float64))
    xf = np.zeros((c.N, c.nv - j0)) if x_free is None else np.abs(np.asarray(x_free, np.float64)[:, j0:])
    b = np.einsum("eki,ei->ek", cr.stacked_jacobian(name, key, angular)[:, :, j0:], cr.gv_of(c)[:, j0:]) if impulse else cr.bias(name, key, angular)
    S2 = (np.einsum("eki,ei->ek", J, xf) + np.einsum("eki,eli,el->ek", J, np.abs(JM[:, :, j0:]), lam) + np.abs(b) + np.abs(t)
          + np.einsum("ekl,el->ek", np.abs(G), lam) + rho[:, None] * lam)
    return S2.max(axis=1)


def guarded(shape, torch_device=None, dtype=np.float32):
    """(buffer with one guard row before and after, the view of the rows between): a store outside the output shows in the guards"""
    full = (shape[0] + 2,) + tuple(shape[1:])
    if torch_device is None:
        buf = np.full(full, 7, dtype)
    else:
        import torch
        buf = torch.full(full, 7, dtype=torch.float32 if dtype == np.float32 else torch.int32, device=torch_device)
    return buf, buf[1:-1]


def guards_intact(buf):
    a = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    return bool(np.all(a[0] == 7) and np.all(a[-1] == 7))


HOUSE = [("floating0", ("sixteen", True, cr.DAMP)), ("fixed2", ("three", True, cr.DAMP)), ("anymal", ("feet", False, 0.0)), ("atlas", ("eleven", True, cr.DAMP)),
         ("atlas", ("hold8", False, 0.0))]


@pytest.mark.parametrize("name,v", HOUSE, ids=lambda x: x if isinstance(x, str) else f"{x[0]}-{int(x[1])}")
def test_determinism_memory_spaces_and_single_outputs(built_lib, name, v):
    """Worlds of 1, 7, 8, 9 and all envs from the first rows of the same batch (tails, and workgroup borders crossed: 16, 8, 4 and 2 envs per workgroup at m = 12, 18 and 24, 66, 96):
    env e's outputs have the bits of the full world's - in host arrays and in torch tensors, all outputs together and each alone - and the rows
    around every output are untouched.  target = None and zeros give the same bits; tau = None reads the resident feed-forward rows."""
    import torch
    dev0 = torch.device("cuda:0")
    c, full = dyn_case(name), device(name)
    key, angular, damping = v
    frames, m = cr.frame_sets(name)[key], cr.rows_of(name, key, angular)
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    for n in (1, 7, 8, 9, c.N):
        w = new_world(c, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        for impulse in (False, True):
            lead = "dgv" if impulse else "udot"
            ref = (full.imp if impulse else full.dyn)[v]
            shapes = {lead: ((n, c.nv), np.float32), "lambda": ((n, m), np.float32), "status": ((n,), np.int32)}
            for td in (None, dev0):
                put = (lambda a: np.ascontiguousarray(a, np.float32)) if td is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(td))
                tgt = put(cr.target(name, key, angular, "vel" if impulse else "acc")[:n])
                tau = put(c.tau[:n])

                def call(out):
                    if impulse:
                        return w.frame_impulse(frames, angular=angular, target_vel=tgt, joint_diag=diag32(name), damping=damping, out=out)
                    return w.constrained_forward_dynamics(frames, tau=tau, angular=angular, target_acc=tgt, damping=damping, out=out)
                bufs = {k: guarded(s, td, dt) for k, (s, dt) in shapes.items()}
                got = call({k: b[1] for k, b in bufs.items()})
                if td is not None:
                    torch.cuda.synchronize()
                for k in shapes:
                    assert got[k] is bufs[k][1]
                    assert np.array_equal(host(got[k]), ref[k][:n]) and guards_intact(bufs[k][0]), (name, n, td, impulse, k)
                for k in shapes:      # each output alone: the others are NULL
                    b1, v1 = guarded(shapes[k][0], td, shapes[k][1])
                    call({k: v1})
                    if td is not None:
                        torch.cuda.synchronize()
                    assert np.array_equal(host(v1), ref[k][:n]) and guards_intact(b1), (name, n, td, impulse, k)
        # NULL targets are zeros, a NULL tau the resident rows
        z = np.zeros((n, m), np.float32)
        tau = np.ascontiguousarray(c.tau[:n], np.float32)
        a = w.constrained_forward_dynamics(frames, tau=tau, angular=angular, target_acc=None, damping=damping)
        b = w.constrained_forward_dynamics(frames, tau=tau, angular=angular, target_acc=z, damping=damping)
        w.set_generalized_force(tau)
        r = w.constrained_forward_dynamics(frames, tau=None, angular=angular, target_acc=z, damping=damping)
        ia = w.frame_impulse(frames, angular=angular, target_vel=None, damping=damping)
        ib = w.frame_impulse(frames, angular=angular, target_vel=z, damping=damping)
        for k in ("udot", "lambda", "status"):
            assert a[k].tobytes() == b[k].tobytes() == r[k].tobytes(), (name, n, k)
        for k in ("dgv", "lambda", "status"):
            assert ia[k].tobytes() == ib[k].tobytes(), (name, n, k)
        assert not np.array_equal(a["lambda"], full.dyn[v]["lambda"][:n])      # (the targets matter)
        w.close()


def test_a_fixed_bases_rows_do_not_matter(built_lib):
    """other noise in the six base rows of tau, gv and target-free joint_diag of a fixed base: not one bit changes"""
    name, v = "fixed2", ("three", True, cr.DAMP)
    c, full = dyn_case(name), device(name)
    rng = np.random.default_rng(1)
    tau, gv = c.tau.astype(np.float32), c.gv.astype(np.float32)
    tau[:, :6] = rng.normal(size=(c.N, 6)) * 10
    gv[:, :6] = rng.normal(size=(c.N, 6)) * 10
    dg = diag32(name).copy()
    dg[:6] = [3.0, -1.0, np.nan, np.inf, 0.5, -0.0]
    w = BatchedWorld(c.model, c.N)
    w.set_state(c.gc, gv)
    frames = cr.frame_sets(name)[v[0]]
    a = w.constrained_forward_dynamics(frames, tau=tau, angular=True, target_acc=t32(name, v[0], True, "acc"), damping=v[2])
    b = w.frame_impulse(frames, angular=True, target_vel=t32(name, v[0], True, "vel"), joint_diag=dg, damping=v[2])
    w.close()
    for k in ("udot", "lambda", "status"):
        assert a[k].tobytes() == full.dyn[v][k].tobytes(), k
    for k in ("dgv", "lambda", "status"):
        assert b[k].tobytes() == full.imp[v][k].tobytes(), k
    assert not a["udot"][:, :6].any() and not b["dgv"][:, :6].any()


def test_a_regular_and_a_dependent_call_share_a_world(built_lib):
    """The quadruped's four feet (regular) and a list that names one (body, offset) twice (dependent for every env), called in turn on one world
    into separate outputs: the dependent call reports status 1 for every env and leaves lambda zero and udot = rsb_forward_dynamics' bits, the
    regular one reports 0 and repeats its bits after the dependent one ran; neither touches the other's outputs nor the world."""
    name = "anymal"
    c, full = dyn_case(name), device(name)
    w = new_world(c)
    reg, dep = ("feet", False, 0.0), ("twice", False, 0.0)
    first = run_dyn(w, name, *reg)
    keep = {k: a.copy() for k, a in first.items()}
    bad = run_dyn(w, name, *dep)
    assert all(first[k].tobytes() == keep[k].tobytes() for k in keep)
    again = run_dyn(w, name, *reg)
    ibad, ireg = run_imp(w, name, *dep), run_imp(w, name, *reg)
    q, u = w.get_state()
    w.close()
    assert (bad["status"] == 1).all() and not bad["lambda"].any() and bad["udot"].tobytes() == full.uf.tobytes()
    assert (ibad["status"] == 1).all() and not ibad["lambda"].any() and not ibad["dgv"].any()
    assert (again["status"] == 0).all() and all(again[k].tobytes() == keep[k].tobytes() == full.dyn[reg][k].tobytes() for k in keep)
    assert all(ireg[k].tobytes() == full.imp[reg][k].tobytes() for k in ireg)
    assert np.array_equal(q, c.gc.astype(np.float32)) and np.array_equal(u, c.gv.astype(np.float32))


def test_queries_leave_the_world_alone_and_follow_pipelined_steps(built_lib):
    """Control steps of the benchmark's quadruped world, K = 3.  (a) lock-step with both queries between the steps: the state after every step and the
    contact list after the last are those of a run without the queries, bit for bit.  (b) pipelined, the queries enqueued without an explicit join:
    the results of the lock-step run at the same point."""
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
    foot_frames = [(int(model.blob.col_body[s]), tuple(float(np.float32(x)) for x in model.blob.col_pos[s])) for s in r.feet]
    tau = f32(np.random.default_rng(4).normal(size=(n, model.nv))).astype(np.float32)
    dg = np.zeros(model.nv, np.float32)
    dg[6:] = 0.1
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
                answers.append((w.constrained_forward_dynamics(foot_frames, tau=tau), w.frame_impulse(foot_frames, joint_diag=dg)))
            if mode != "pipelined":
                states.append(w.get_state())
        states.append(w.get_state())
        runs[mode] = (states, w.get_contacts(), answers)
        w.close()
    for (qa, ua), (qb, ub) in zip(runs["plain"][0], runs["queried"][0]):
        assert np.array_equal(qa, qb) and np.array_equal(ua, ub)
    assert np.array_equal(runs["plain"][1][0], runs["queried"][1][0]) and runs["plain"][1][1].tobytes() == runs["queried"][1][1].tobytes()
    assert runs["plain"][1][0].sum() > 0
    for (da, ia), (db, ib) in zip(runs["queried"][2], runs["pipelined"][2]):
        assert all(da[k].tobytes() == db[k].tobytes() for k in da) and all(ia[k].tobytes() == ib[k].tobytes() for k in ia)
        assert (da["status"] == 0).all() and (ia["status"] == 0).all()
    assert not np.array_equal(runs["queried"][2][0][0]["udot"], runs["queried"][2][-1][0]["udot"])      # (the state moved between the answers)
    assert np.array_equal(runs["pipelined"][0][-1][0], runs["plain"][0][-1][0])


def test_bad_input_fails_loudly_and_touches_nothing(built_lib, anymal):
    """every argument error of rsb.h: RSB_E_INVALID, a message naming the function, the guard pattern of the outputs intact"""
    n = 8
    gc, gv = workload.random_state(anymal.nq, anymal.nv, n, seed=4)
    w = BatchedWorld(anymal, n)
    w.set_state(gc, gv)
    L, h, nv = w.L, w.handle, anymal.nv
    out = np.full((n, 6 * 6 + 6 * nv), 7.0, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    sto = np.full(n, 7, np.int32)
    s = sto.ctypes.data_as(C.c_void_p)
    inp = np.zeros((n, 2 * nv), np.float32)
    q = inp.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 17)()
    fr[1].body = 3
    bad_body, bad_off = (_capi.Frame * 1)(), (_capi.Frame * 1)()
    bad_body[0].body = anymal.nb
    bad_off[0].offset[1] = float("nan")

    def diag(k, val):
        d = np.zeros(nv, np.float32)
        d[k] = val
        return d
    diags = [diag(7, -0.1), diag(9, np.nan), diag(nv - 1, np.inf), diag(2, 0.25), diag(4, 0.25)]
    dyn = lambda W=h, tau=q, f=fr, nf=2, fl=0, t=q, dmp=0.0, u=p, lm=p, st=s, sp=0: L.rsb_constrained_forward_dynamics(W, tau, f, nf, fl, t, dmp, u, lm, st, sp)
    imp = lambda W=h, f=fr, nf=2, fl=0, t=q, dg=None, dmp=0.0, u=p, lm=p, st=s, sp=0: L.rsb_frame_impulse(W, f, nf, fl, t, dg, dmp, u, lm, st, sp)
    cases = []
    for fn, who in ((dyn, b"rsb_constrained_forward_dynamics"), (imp, b"rsb_frame_impulse")):
        cases += [
            (lambda fn=fn: fn(W=None), who + b": null world"),
            (lambda fn=fn: fn(sp=2), who + b": space"),
            (lambda fn=fn: fn(sp=-1), who + b": space"),
            (lambda fn=fn: fn(u=None, lm=None, st=None), who + b": every output is NULL"),
            (lambda fn=fn: fn(nf=0), who + b": n_frames"),
            (lambda fn=fn: fn(nf=17), who + b": n_frames"),
            (lambda fn=fn: fn(f=None), who + b": n_frames"),
            (lambda fn=fn: fn(f=bad_body, nf=1), who + b": frame 0: body"),
            (lambda fn=fn: fn(f=bad_off, nf=1, fl=1), who + b": frame 0: non-finite"),
            (lambda fn=fn: fn(fl=2), who + b": unknown flag"),
            (lambda fn=fn: fn(fl=5), who + b": unknown flag"),
            (lambda fn=fn: fn(dmp=-1e-3), who + b": damping"),
            (lambda fn=fn: fn(dmp=float("nan")), who + b": damping"),
            (lambda fn=fn: fn(dmp=float("inf")), who + b": damping"),
        ]
    for dg in diags:
        dp = dg.ctypes.data_as(C.c_void_p)
        cases.append((lambda dp=dp: imp(dg=dp), b"rsb_frame_impulse: joint_diag"))
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k          # RSB_E_INVALID
        assert msg in L.rsb_last_error(), (k, L.rsb_last_error())
        assert np.all(out == 7.0) and np.all(sto == 7), k
    with pytest.raises(ValueError):
        w.constrained_forward_dynamics([1], tau=np.zeros((n, nv + 1), np.float32))
    with pytest.raises(ValueError):
        w.constrained_forward_dynamics([1], target_acc=np.zeros((n, 4), np.float32))
    with pytest.raises(ValueError):
        w.frame_impulse([1], dgv=False, lam=False, status=False)
    with pytest.raises(ValueError):
        w.frame_impulse([1], out={"Lambda": out})
    with pytest.raises(ValueError):
        w.frame_impulse([1], joint_diag=np.zeros(3, np.float32))
    assert dyn() == 0 and imp() == 0      # valid calls after all of them
    assert (sto == 0).all()
    w.close()


def test_parity_record(built_lib):
    """The largest error / bar per quantity and case over all envs and solved variants, written to profiles/constrained_parity.txt (the figures
    DESIGN.md quotes).  Every figure has to be <= 1: this is the union of the parity tests above."""
    lines, fails = [], []
    for name in cr.CASES:
        c, d = dyn_case(name), device(name)
        for impulse in (False, True):
            worst = {}
            for v in cr.variants(name):
                check_variant(name, v, (d.imp if impulse else d.dyn)[v], impulse, worst)
            fwd = (f"   forward: lambda {worst['lam']:.3f}  {'dgv' if impulse else 'udot'} {worst['x']:.3f}" if "lam" in worst else "   forward: no regular set")
            lines.append(f"  {name:10s} N {c.N:3d} nb {c.nb:3d}  {'impulse ' if impulse else 'dynamics'}  gates: dynamics row {worst['dyn']:.3f}  constraint row {worst['con']:.3f}{fwd}\n")
            fails += [(name, impulse, k, val) for k, val in worst.items() if not val <= 1.0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "constrained_parity.txt"), "w") as f:
        f.write("tests/test_gpu_constrained.py::test_parity_record\n"
                "device fp32 vs the fp64 KKT references on the float32-rounded state; largest error / bar over the envs and the solved variants (m = 3 .. 96 rows, regular sets and\n"
                "dependent sets with damping 1e-4; the impulse with joint_diag).  gates: |M udot + h - tau - J^T lambda| over 2e-5 (1 + largest row of the absolute terms), |J udot +\n"
                "Jdot gv - target + rho lambda| over 2e-5 (1 + S2).  forward (regular sets): max|x - x_ref| / (1 + max|x_ref|) over 4 x the float32 restatement's figure\n"
                "(profiles/constrained_restatement.txt)\n" + "".join(lines))
    print("".join(lines))
    assert not fails, fails
