"""Batched inverse-mass solves and frame Delassus matrices on the device (rsb_apply_inverse_mass, rsb_get_frame_delassus;
raisimlib_amd/csrc/rsb_inverse_mass.hip) through the C-ABI, against the fp64 references of tests/inverse_mass_reference.py on the float32-rounded
configuration the device saw.  Cases: floating0, floating5, fixed2, tree40 (N = 67), anymal, atlas (N = 64).  EVERY env of EVERY variant has to meet
its bars.  With A = M_ref + diag(joint_diag):

Conditioning-free bars (the gate; the project's inverse-dynamics bar, derived, not measured).
  X       per env and column |A x - b|_inf <= 2e-5 (1 + S), S the largest row of |A||x| + |b|
  JMinv   the same for each row k against J_ref^T e_k
  G       |G - J_ref JMinv_dev^T| <= 2e-5 (1 + largest entry of |J_ref||JMinv_dev|^T), evaluated in fp64
Forward bars.  Each error measure - X: max|X - X_ref| / (1 + max|X_ref|), G and JMinv: max|. - ref| / max|ref|, per env - is at most 4 x the figure
the kernel's algorithm restated in numpy reaches on the case (tools/inverse_mass_restatement.py; its output is profiles/inverse_mass_restatement.txt;
in float64 throughout the same code agrees with the references to 1.1e-15 .. 1.2e-12).  The margin of 4 is the one
tests/test_gpu_dynamics.py::test_forward_dynamics took over ITS restatement, for the reason its docstring gives: a correct device solves its own fp32
system.
How the figures came about.  The restatement was first run with everything in float32, as aba_kernel computes (the tool's middle columns), before any
device figure was looked at: IM32 2.8e-7 (floating0) .. 5.1e-4 (the humanoid, cond(M) 4.6e5).  A kernel written that way met every forward bar and every
gate but one: |A x - b| of the humanoid's unit right-hand sides came to 2.6 x the gate on the device, and to 3.2 x in the float32 restatement itself -
the algorithm, not the device.  The restatement located the loss in phase 1 (in the common frame a distal joint's D, a few 1e-4, is what is left of
inertias about the base origin of order 1): with phase 1 in float64 and the columns in float32 it meets the gate at 0.30 and the humanoid's IM32 falls
to 3.1e-7.  The kernel was changed to that, the restatement to state exactly that (the walk included), and the table below is its output, again taken
on the CPU before the changed kernel ran.
test_parity_record writes the device's measured ratios to profiles/inverse_mass_parity.txt."""
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
import inverse_mass_reference as ref

pytestmark = pytest.mark.gpu

# tools/inverse_mass_restatement.py, its first three columns (float32 with phase 1 in float64: the kernel): the maximum over the envs and the variants of
# this file of the kernel's algorithm in numpy
IM32 = {"floating0": 1.594e-07, "floating5": 3.534e-07, "fixed2": 3.650e-07, "tree40": 3.136e-07, "anymal": 3.098e-07, "atlas": 3.076e-07}
G32 = {"floating0": 2.819e-07, "floating5": 4.170e-07, "fixed2": 2.286e-07, "tree40": 8.450e-07, "anymal": 7.060e-07, "atlas": 1.188e-06}
JM32 = {"floating0": 6.110e-07, "floating5": 3.020e-07, "fixed2": 1.528e-07, "tree40": 2.282e-06, "anymal": 5.678e-07, "atlas": 2.301e-06}


def new_world(c, n=None):
    n = n or c.N
    w = BatchedWorld(c.model, n)
    w.set_state(c.gc[:n], c.gv[:n])
    return w


def diag_of(name, with_diag):
    return ref.joint_diag(name).astype(np.float32) if with_diag else None


def b32(name, which, n=None):
    return np.ascontiguousarray(ref.rhs(name, which)[:n], np.float32)


@functools.lru_cache(maxsize=None)
def device(name):
    """everything the device says about one case, computed once in one world"""
    c = dyn_case(name)
    w = new_world(c)
    d = SimpleNamespace(X={}, D={})
    for which, wd in ref.SOLVE_VARIANTS:
        d.X[which, wd] = w.apply_inverse_mass(b32(name, which), joint_diag=diag_of(name, wd))
    for key, angular, wd in ref.delassus_variants(name):
        d.D[key, angular, wd] = w.frame_delassus(ref.frame_sets(name)[key], angular=angular, joint_diag=diag_of(name, wd), G=True, JMinv=True)
    w.close()
    return d


def solve_ratios(name, which, wd, X):
    """(residual / gate, forward error / (4 IM32)) per env"""
    c = dyn_case(name)
    gate = ref.residual_ratio(ref.system(name, wd), X, ref.rhs(name, which), c.j0)
    return gate, ref.x_error(X, ref.solve_reference(name, which, wd)) / (4 * IM32[name])


def delassus_ratios(name, key, angular, wd, out):
    """(JMinv rows / gate, G product / gate, G forward / (4 G32), JMinv forward / (4 JM32)) per env"""
    c = dyn_case(name)
    J = ref.stacked_jacobian(name, key, angular)
    Gr, JMr = ref.delassus_reference(name, key, angular, wd)
    return (ref.residual_ratio(ref.system(name, wd), out["JMinv"], J, c.j0), ref.product_ratio(out["G"], J, out["JMinv"]),
            ref.rel_error(out["G"], Gr) / (4 * G32[name]), ref.rel_error(out["JMinv"], JMr) / (4 * JM32[name]))


@pytest.mark.parametrize("name", ref.CASES)
def test_apply_inverse_mass(built_lib, name):
    """R = 1, R = 5 (with and without joint_diag) and R = nv with B = identity - X is then A^-1, compared with inv(M_ref): every env meets the gate and
    the forward bar.  A fixed base: the six base rows of X are exactly zero, and of A^-1 the base rows AND columns.  joint_diag changes the result."""
    c, d = dyn_case(name), device(name)
    for which, wd in ref.SOLVE_VARIANTS:
        X = d.X[which, wd]
        assert X.shape == ref.rhs(name, which).shape and X.dtype == np.float32 and np.isfinite(X).all()
        gate, fwd = solve_ratios(name, which, wd, X)
        print(f"{name} {which} diag={wd}: residual / gate {gate.max():.3f}, error / (4 IM32) {fwd.max():.3f}")
        assert gate.max() <= 1.0, (name, which, wd, int(gate.argmax()), gate.max())
        assert fwd.max() <= 1.0, (name, which, wd, int(fwd.argmax()), fwd.max())
        if c.fixed:
            assert not X[:, :, :6].any()
    assert np.array_equal(d.X["r1", False], d.X["r5", False][:, :1])      # a column does not depend on its neighbours
    assert not np.array_equal(d.X["r5", True], d.X["r5", False])
    if c.fixed:
        assert not d.X["eye", False][:, :6, :].any()


@pytest.mark.parametrize("name", ref.CASES)
def test_frame_delassus(built_lib, name):
    """Linear and angular rows of: one frame; the case's three frames (two on one body, one on another); a frame on a body and one on its parent; the
    quadruped's four feet; 16 frames x 6 rows on floating0 (G is 96 x 96 of rank <= nv: nothing inverts it).  Gates and forward bars on every env;
    G equals its transpose bit for bit; every diagonal entry of a linear row on a moving body is > 0; a fixed base's columns of JMinv are zero."""
    c, d = dyn_case(name), device(name)
    for key, angular, wd in ref.delassus_variants(name):
        out = d.D[key, angular, wd]
        frames = ref.frame_sets(name)[key]
        kk = 6 if angular else 3
        G, JM = out["G"], out["JMinv"]
        assert G.shape == (c.N, kk * len(frames), kk * len(frames)) and JM.shape == (c.N, kk * len(frames), c.nv)
        assert np.isfinite(G).all() and np.isfinite(JM).all()
        assert np.array_equal(G, G.transpose(0, 2, 1)), (name, key, angular)
        for f, (body, _) in enumerate(frames):
            if body > 0 or not c.fixed:
                for a in range(3):
                    assert (G[:, kk * f + a, kk * f + a] > 0).all(), (name, key, f, a)
        if c.fixed:
            assert not JM[:, :, :6].any()
        rows, prod, gf, jf = delassus_ratios(name, key, angular, wd, out)
        print(f"{name} {key} angular={angular} diag={wd}: JMinv rows / gate {rows.max():.3f}, G - J JMinv^T / gate {prod.max():.3f}, "
              f"G error / (4 G32) {gf.max():.3f}, JMinv error / (4 JM32) {jf.max():.3f}")
        assert rows.max() <= 1.0 and prod.max() <= 1.0, (name, key, angular, wd, rows.max(), prod.max())
        assert gf.max() <= 1.0 and jf.max() <= 1.0, (name, key, angular, wd, gf.max(), jf.max())
    assert not np.array_equal(d.D["three", True, True]["G"], d.D["three", True, False]["G"])
    lin, ang = d.D["three", False, False], d.D["three", True, False]      # the linear rows are the same rows in both layouts
    pick = [6 * f + a for f in range(3) for a in range(3)]
    assert np.array_equal(lin["JMinv"], ang["JMinv"][:, pick]) and np.array_equal(lin["G"], ang["G"][:, pick][:, :, pick])


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
    """Worlds of 1, 7, 8, 9 and all envs from the first rows of the same batch (tails, and workgroup borders crossed): env e's outputs have the bits of
    the full world's - in host arrays and in torch tensors, both Delassus outputs together and each alone, X out of place and in place - and the rows
    around every output are untouched.  joint_diag = None and an all-zero joint_diag give the same bits."""
    import torch
    dev0 = torch.device("cuda:0")
    c, full = dyn_case(name), device(name)
    host = lambda v: v if isinstance(v, np.ndarray) else v.cpu().numpy()
    frames = ref.frame_sets(name)["three"]
    dg = diag_of(name, True)
    for n in (1, 7, 8, 9, c.N):
        w = new_world(c, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        shapes = dict(G=(n, 18, 18), JMinv=(n, 18, c.nv))
        for td in (None, dev0):
            put = (lambda a: a) if td is None else (lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(td))
            B = put(b32(name, "r5", n))
            bx, vx = guarded((n, 5, c.nv), td)
            assert w.apply_inverse_mass(B, joint_diag=dg, out=vx) is vx
            bi, vi = guarded((n, 5, c.nv), td)
            vi[...] = B
            assert w.apply_inverse_mass(vi, joint_diag=dg, out=vi) is vi      # X == B
            bufs = {k: guarded(s, td) for k, s in shapes.items()}
            got = w.frame_delassus(frames, angular=True, joint_diag=dg, out={k: v for k, (_, v) in bufs.items()})
            if td is not None:
                torch.cuda.synchronize()
            assert np.array_equal(host(vx), full.X["r5", True][:n]) and guards_intact(bx), (name, n, td)
            assert np.array_equal(host(vi), full.X["r5", True][:n]) and guards_intact(bi), (name, n, td)
            for k in shapes:
                assert np.array_equal(host(got[k]), full.D["three", True, True][k][:n]) and guards_intact(bufs[k][0]), (name, n, td, k)
            for k in shapes:                       # each output alone: the other is NULL
                b1, v1 = guarded(shapes[k], td)
                w.frame_delassus(frames, angular=True, joint_diag=dg, out={k: v1})
                if td is not None:
                    torch.cuda.synchronize()
                assert np.array_equal(host(v1), full.D["three", True, True][k][:n]) and guards_intact(b1), (name, n, td, k)
        one = w.frame_delassus(frames, angular=True, G=False, JMinv=True)
        assert sorted(one) == ["JMinv"] and np.array_equal(one["JMinv"], full.D["three", True, False]["JMinv"][:n])
        zeros = np.zeros(c.nv, np.float32)
        assert np.array_equal(w.apply_inverse_mass(b32(name, "r5", n), joint_diag=zeros), full.X["r5", False][:n])
        assert np.array_equal(w.frame_delassus(frames, angular=True, joint_diag=zeros)["G"], full.D["three", True, False]["G"][:n])
        w.close()


def test_a_fixed_bases_rows_do_not_matter(built_lib):
    """other noise in the six base rows of B, and anything at all in the six base entries of joint_diag of a fixed base: not one bit changes"""
    name = "fixed2"
    c, full = dyn_case(name), device(name)
    rng = np.random.default_rng(1)
    B = b32(name, "r5")
    B[:, :, :6] = rng.normal(size=(c.N, 5, 6)) * 10
    dg = diag_of(name, True).copy()
    dg[:6] = [3.0, -1.0, np.nan, np.inf, 0.5, -0.0]
    w = new_world(c)
    X = w.apply_inverse_mass(B, joint_diag=dg)
    D = w.frame_delassus(ref.frame_sets(name)["three"], angular=True, joint_diag=dg, G=True, JMinv=True)
    w.close()
    assert np.array_equal(X, full.X["r5", True])
    assert np.array_equal(D["G"], full.D["three", True, True]["G"]) and np.array_equal(D["JMinv"], full.D["three", True, True]["JMinv"])


def test_queries_leave_the_world_alone_and_follow_pipelined_steps(built_lib):
    """Control steps of the benchmark's quadruped world, K = 3.  (a) lock-step with both queries between the steps: the state after every step and the
    contact list after the last are those of a run without the queries, bit for bit - the third step would show a changed warm state.  (b) pipelined,
    the queries enqueued without an explicit join: the results of the lock-step run at the same point."""
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
    rng = np.random.default_rng(4)
    B = f32(rng.normal(size=(n, 2, model.nv))).astype(np.float32)
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
                answers.append((w.apply_inverse_mass(B, joint_diag=dg), w.frame_delassus(foot_frames, joint_diag=dg, G=True, JMinv=True)))
            if mode != "pipelined":
                states.append(w.get_state())
        states.append(w.get_state())
        runs[mode] = (states, w.get_contacts(), answers)
        w.close()
    for (qa, ua), (qb, ub) in zip(runs["plain"][0], runs["queried"][0]):
        assert np.array_equal(qa, qb) and np.array_equal(ua, ub)
    assert np.array_equal(runs["plain"][1][0], runs["queried"][1][0]) and runs["plain"][1][1].tobytes() == runs["queried"][1][1].tobytes()
    assert runs["plain"][1][0].sum() > 0
    for (xa, da), (xb, db) in zip(runs["queried"][2], runs["pipelined"][2]):
        assert np.array_equal(xa, xb) and np.array_equal(da["G"], db["G"]) and np.array_equal(da["JMinv"], db["JMinv"])
    assert not np.array_equal(runs["queried"][2][0][0], runs["queried"][2][-1][0])      # (the configuration moved between the answers)
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
    inp = np.zeros((n, 2 * nv), np.float32)
    q = inp.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 17)()
    fr[1].body = 3
    bad_body, bad_off = (_capi.Frame * 1)(), (_capi.Frame * 1)()
    bad_body[0].body = anymal.nb
    bad_off[0].offset[1] = float("nan")

    def diag(k, v):
        d = np.zeros(nv, np.float32)
        d[k] = v
        return d
    diags = [diag(7, -0.1), diag(9, np.nan), diag(nv - 1, np.inf), diag(2, 0.25), diag(4, 0.25)]
    solve, dela = b"rsb_apply_inverse_mass", b"rsb_get_frame_delassus"
    cases = [
        (lambda: L.rsb_apply_inverse_mass(None, q, 1, None, p, 0), solve + b": null world"),
        (lambda: L.rsb_get_frame_delassus(None, fr, 2, 0, None, p, p, 0), dela + b": null world"),
        (lambda: L.rsb_apply_inverse_mass(h, q, 1, None, p, 2), solve + b": space"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 2, 0, None, p, p, -1), dela + b": space"),
        (lambda: L.rsb_apply_inverse_mass(h, q, 0, None, p, 0), solve + b": n_rhs"),
        (lambda: L.rsb_apply_inverse_mass(h, q, -3, None, p, 0), solve + b": n_rhs"),
        (lambda: L.rsb_apply_inverse_mass(h, q, 6 + 64, None, p, 0), solve + b": n_rhs"),
        (lambda: L.rsb_apply_inverse_mass(h, None, 1, None, p, 0), solve + b": B or X is NULL"),
        (lambda: L.rsb_apply_inverse_mass(h, q, 1, None, None, 0), solve + b": B or X is NULL"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 0, 0, None, p, p, 0), dela + b": n_frames"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 17, 0, None, p, p, 0), dela + b": n_frames"),
        (lambda: L.rsb_get_frame_delassus(h, None, 2, 0, None, p, p, 0), dela + b": n_frames"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 2, 0, None, None, None, 0), dela + b": every output is NULL"),
        (lambda: L.rsb_get_frame_delassus(h, bad_body, 1, 0, None, p, p, 0), dela + b": frame 0: body"),
        (lambda: L.rsb_get_frame_delassus(h, bad_off, 1, 1, None, p, None, 0), dela + b": frame 0: non-finite"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 2, 2, None, p, p, 0), dela + b": unknown flag"),
        (lambda: L.rsb_get_frame_delassus(h, fr, 2, 5, None, p, p, 0), dela + b": unknown flag"),
    ]
    for dg in diags:
        dp = dg.ctypes.data_as(C.c_void_p)
        cases.append((lambda dp=dp: L.rsb_apply_inverse_mass(h, q, 1, dp, p, 0), solve + b": joint_diag"))
        cases.append((lambda dp=dp: L.rsb_get_frame_delassus(h, fr, 2, 1, dp, p, p, 0), dela + b": joint_diag"))
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k          # RSB_E_INVALID
        assert msg in L.rsb_last_error(), (k, L.rsb_last_error())
        assert np.all(out == 7.0), k
    with pytest.raises(ValueError):
        w.apply_inverse_mass(np.zeros((n, nv + 1), np.float32))
    with pytest.raises(ValueError):
        w.apply_inverse_mass(inp[:, :nv], joint_diag=np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        w.frame_delassus([1], G=False, JMinv=False)
    with pytest.raises(ValueError):
        w.frame_delassus([1], out={"Lambda": out})
    assert L.rsb_apply_inverse_mass(h, q, 2, None, p, 0) == 0      # a valid call after all of them
    w.close()


def test_parity_record(built_lib):
    """The largest error / bar per quantity and case over all envs and variants, written to profiles/inverse_mass_parity.txt (the figures DESIGN.md
    quotes).  Every figure has to be <= 1: this is the union of the parity tests above."""
    lines, fails = [], []
    for name in ref.CASES:
        c, d = dyn_case(name), device(name)
        worst = dict(X_gate=0.0, X=0.0, JMinv_gate=0.0, G_gate=0.0, G=0.0, JMinv=0.0)
        for which, wd in ref.SOLVE_VARIANTS:
            gate, fwd = solve_ratios(name, which, wd, d.X[which, wd])
            worst["X_gate"], worst["X"] = max(worst["X_gate"], gate.max()), max(worst["X"], fwd.max())
        for key, angular, wd in ref.delassus_variants(name):
            rows, prod, gf, jf = delassus_ratios(name, key, angular, wd, d.D[key, angular, wd])
            for k, v in (("JMinv_gate", rows), ("G_gate", prod), ("G", gf), ("JMinv", jf)):
                worst[k] = max(worst[k], v.max())
        lines.append(f"  {name:10s} N {c.N:3d} nb {c.nb:3d}  gates: X {worst['X_gate']:.3f}  JMinv {worst['JMinv_gate']:.3f}  G {worst['G_gate']:.3f}   forward: "
                     f"X {worst['X']:.3f} (IM32 {IM32[name]:.2e})  G {worst['G']:.3f} (G32 {G32[name]:.2e})  JMinv {worst['JMinv']:.3f} (JM32 {JM32[name]:.2e})\n")
        fails += [(name, k, v) for k, v in worst.items() if not v <= 1.0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "inverse_mass_parity.txt"), "w") as f:
        f.write("tests/test_gpu_inverse_mass.py::test_parity_record\n"
                "device fp32 vs fp64 references on the float32-rounded configuration; largest error / bar over the envs and the variants (R = 1, 5, nv; five frame sets, linear and\n"
                "angular rows; with and without joint_diag).  gates: |A x - b| and |A JMinv_k^T - J_k^T| over 2e-5 (1 + largest row of |A||x| + |b|), |G - J JMinv^T| over\n"
                "2e-5 (1 + largest entry of |J||JMinv|^T).  forward: max|X - X_ref| / (1 + max|X_ref|) over 4 IM32, max|G - G_ref| / max|G_ref| over 4 G32, the same for JMinv over 4 JM32\n" +
                "".join(lines))
    print("".join(lines))
    assert not fails, fails
