"""Batched inverse kinematics on the device (rsb_inverse_kinematics; raisimlib_amd/csrc/rsb_ik.hip) through BatchedWorld.inverse_kinematics and the
C-ABI, on the variants of tests/ik_reference.py: floating0, fixed2 (N = 67), anymal, atlas (N = 64), m = 3, 6, 12, 24, 36, 72, 96 rows, the base held
and free, EVERY env.  Settings: max_iter 30, damping 1e-3, max_step 0.5, tolerances 1e-4 (ik_reference); tests/test_ik_reference.py holds the numpy
float32 restatement to at most 15 steps on every env of every variant before any device run.

Residual bars, evaluated in fp64 at the float32 gc_out (ik_reference.evaluate / bars):
  position   |pos - target|_inf <= pos_tol + 1e-5 (1 + max|target|)      the added term is the frame-position bar of tests/test_gpu_frames.py
  rotation   rotation rows      <= rot_tol + 6e-5                          the same bar, 2e-5 per entry of R, through the three-term sums of R_t R^T
and the reported `error` agrees with the fp64 evaluation within the added terms.  test_parity_record writes the measured figures to
profiles/ik_parity.txt."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from common import ROOT
from raisimlib_amd import BatchedWorld, Model, _capi
from test_dynamics_reference import dyn_case, jacobians, kinematics
import ik_reference as ik

pytestmark = pytest.mark.gpu

SETTINGS = dict(max_iter=ik.MAX_ITER, damping=ik.DAMPING, pos_tol=ik.POS_TOL, rot_tol=ik.ROT_TOL, max_step=ik.MAX_STEP)


def new_world(c, n=None, first=0):
    n = n or c.N
    w = BatchedWorld(c.model, n)
    w.set_state(c.gc[first:first + n], c.gv[first:first + n])
    return w


def solve(w, name, v, rows=slice(None), **kw):
    key, angular, base_free = v
    pr = ik.problem(name, *v)
    args = dict(SETTINGS)
    args.update(kw)
    return w.inverse_kinematics(ik.frame_sets(name)[key], pr.target_pos[rows], None if pr.target_rot is None else pr.target_rot[rows],
                                dof_mask=ik.dof_mask(name, base_free), **args)


@functools.lru_cache(maxsize=None)
def device(name):
    """every variant of the case solved once in one world; the state and the contact list before and after"""
    c = dyn_case(name)
    w = new_world(c)
    if name in ("anymal", "atlas"):      # the shipped models take one step first: the contact list then holds something
        w.integrate()
        w.set_state(c.gc, c.gv)          # (the variants start from the case's rows: gc_init None reads them)
    state0, con0 = w.get_state(), w.get_contacts()
    d = SimpleNamespace(out={v: solve(w, name, v) for v in ik.variants(name)})
    state1, con1 = w.get_state(), w.get_contacts()
    d.world_kept = all(a.tobytes() == b.tobytes() for a, b in zip(state0, state1)) and all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(con0, con1))
    w.close()
    return d


def figures(name, v, out, rows=slice(None)):
    """per env: position residual / bar, rotation residual / bar, |error - fp64| over the added terms (position, rotation)"""
    key, angular, _ = v
    pr = ik.problem(name, *v)
    ep, er, tmax = ik.evaluate(name, key, out["gc"], pr.target_pos[rows], None if pr.target_rot is None else pr.target_rot[rows])
    bp, br = ik.bars(tmax, angular)
    dp = np.abs(out["error"][:, 0] - ep) / (ik.POS_BAR * (1 + tmax))
    dr = np.abs(out["error"][:, 1] - er) / ik.ROT_BAR
    return ep / bp, (er / br if angular else np.zeros_like(er)), dp, dr


@pytest.mark.parametrize("name", ik.CASES)
def test_residual_and_status(built_lib, name):
    c, d = dyn_case(name), device(name)
    print()
    for v in ik.variants(name):
        out = d.out[v]
        assert out["gc"].shape == (c.N, c.model.nq) and out["error"].shape == (c.N, 2) and out["status"].dtype == np.int32 and out["iterations"].dtype == np.int32
        rp, rr, dp, dr = figures(name, v, out)
        print(f"  {name} {v} m={ik.rows_of(name, v[0], v[1])}: iterations <= {out['iterations'].max()}, position / bar {rp.max():.3f}, rotation / bar {rr.max():.3f}, "
              f"error vs fp64 / added term {dp.max():.3f} {dr.max():.3f}")
        assert (out["status"] == _capi.RSB_IK_CONVERGED).all(), (name, v, np.flatnonzero(out["status"]))
        assert (out["iterations"] <= ik.MAX_ITER).all() and (out["iterations"] >= 0).all()
        assert rp.max() <= 1.0 and rr.max() <= 1.0, (name, v, rp.max(), rr.max())
        assert dp.max() <= 1.0 and dr.max() <= 1.0, (name, v, dp.max(), dr.max())
        if not v[1]:
            assert not out["error"][:, 1].any()


def held_entries(name, base_free):
    c = dyn_case(name)
    free = ik.free_columns(name, base_free)
    held = np.ones(c.model.nq, bool)
    held[:3] = ~free[:3]; held[3:7] = not free[3:6].any(); held[7:] = ~free[6:]
    return held


@pytest.mark.parametrize("name", ik.CASES)
def test_held_coordinates_and_world_state(built_lib, name):
    c, d = dyn_case(name), device(name)
    assert d.world_kept      # get_state and the contact list: the bits from before the calls
    start = np.ascontiguousarray(c.gc, np.float32)
    for v in ik.variants(name):
        held = held_entries(name, v[2])
        assert d.out[v]["gc"][:, held].tobytes() == start[:, held].tobytes(), (name, v)
    # a partial mask: two joints and one base rotation free; everything else keeps its bits, the quaternion moves only with the rotation
    v = ik.variants(name)[0]
    mask = np.zeros(c.nv, np.uint8)
    mask[[c.nv - 1, c.nv - 2]] = 1
    if not c.fixed:
        mask[4] = 1
    pr = ik.problem(name, *v)
    w = new_world(c)
    out = w.inverse_kinematics(ik.frame_sets(name)[v[0]], pr.target_pos, pr.target_rot, dof_mask=mask, **SETTINGS)
    w.close()
    keep = np.ones(c.model.nq, bool)
    keep[[c.model.nq - 1, c.model.nq - 2]] = False
    if not c.fixed:
        keep[3:7] = False
    assert out["gc"][:, keep].tobytes() == start[:, keep].tobytes()
    assert not np.array_equal(out["gc"][:, ~keep], start[:, ~keep])


PICK = [(n, v) for n in ik.CASES for v in (ik.variants(n)[0], ik.variants(n)[-1])]


@pytest.mark.parametrize("name,v", PICK, ids=[f"{n}-{v[0]}-{int(v[1])}{int(v[2])}" for n, v in PICK])
def test_independence_bit_for_bit(built_lib, name, v):
    import torch
    c, full = dyn_case(name), device(name).out[v]
    names = ("gc", "error", "iterations", "status")
    same = lambda a, b, rows=slice(None): all(np.asarray(a[k]).tobytes() == np.asarray(b[k][rows]).tobytes() for k in a)
    # env e alone in a world of one
    for e in (0, c.N // 2, c.N - 1):
        w = new_world(c, 1, first=e)
        assert same(solve(w, name, v, rows=slice(e, e + 1)), full, slice(e, e + 1)), (name, v, e)
        w.close()
    w = new_world(c)
    # any subset of outputs
    for sub in (("gc",), ("error",), ("iterations",), ("status",), ("gc", "status"), ("error", "iterations")):
        got = solve(w, name, v, **{k: k in sub for k in names})
        assert set(got) == set(sub) and same(got, full), (name, v, sub)
    # gc_init NULL against the resident rows passed explicitly
    assert same(solve(w, name, v, gc_init=np.ascontiguousarray(c.gc, np.float32)), full)
    # torch device buffers against numpy host buffers
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda:0")
    pr = ik.problem(name, *v)
    put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    bufs = {"gc": torch.full((c.N + 2, c.model.nq), 7.0, device=dev), "error": torch.full((c.N + 2, 2), 7.0, device=dev),
            "iterations": torch.full((c.N + 2,), 7, dtype=torch.int32, device=dev), "status": torch.full((c.N + 2,), 7, dtype=torch.int32, device=dev)}
    got = w.inverse_kinematics(ik.frame_sets(name)[v[0]], put(pr.target_pos), put(pr.target_rot), gc_init=put(c.gc), dof_mask=ik.dof_mask(name, v[2]),
                               out={k: b[1:-1] for k, b in bufs.items()}, **SETTINGS)
    torch.cuda.synchronize()
    assert same({k: t.cpu().numpy() for k, t in got.items()}, full)
    for k, b in bufs.items():      # the rows around every output are untouched
        a = b.cpu().numpy()
        assert (a[0] == 7).all() and (a[-1] == 7).all(), k
    w.close()


MIXED = [("anymal", ("feet", False, False)), ("atlas", ("limbs", True, False)), ("floating0", ("sixteen", True, False))]


@pytest.mark.parametrize("name,v", MIXED, ids=[f"{n}-{v[0]}" for n, v in MIXED])
def test_mixed_batch(built_lib, name, v):
    """odd envs get a target 10 m away (the base is held: out of reach): the even envs carry the regular run's bits, the odd ones run out of steps
    with a finite iterate"""
    c, full = dyn_case(name), device(name).out[v]
    pr = ik.problem(name, *v)
    tp = pr.target_pos.copy()
    tp[1::2, :, 0] += 10.0
    w = new_world(c)
    out = w.inverse_kinematics(ik.frame_sets(name)[v[0]], tp, pr.target_rot, dof_mask=ik.dof_mask(name, v[2]), **SETTINGS)
    w.close()
    for k in out:
        assert out[k][0::2].tobytes() == full[k][0::2].tobytes(), (name, v, k)
    assert (out["status"][1::2] == _capi.RSB_IK_MAX_ITER).all() and (out["iterations"][1::2] == ik.MAX_ITER).all()
    assert np.isfinite(out["gc"]).all() and np.isfinite(out["error"]).all()
    ep, er, tmax = ik.evaluate(name, v[0], out["gc"][1::2], tp[1::2], None if pr.target_rot is None else pr.target_rot[1::2])
    assert (np.abs(out["error"][1::2, 0] - ep) <= ik.POS_BAR * (1 + tmax)).all() and (np.abs(out["error"][1::2, 1] - er) <= ik.ROT_BAR).all()
    assert (ep > 1.0).all()


@pytest.mark.parametrize("name", ["anymal", "fixed2"])
def test_evaluation_only(built_lib, name):
    """max_iter = 0: gc_out carries the start's bits; the status says whether the start meets the tolerances"""
    c = dyn_case(name)
    v = ik.variants(name)[-1]
    pr = ik.problem(name, *v)
    start = np.ascontiguousarray(c.gc, np.float32)
    w = new_world(c)
    out = solve(w, name, v, max_iter=0)
    assert out["gc"].tobytes() == start.tobytes() and not out["iterations"].any()
    ep, er, tmax = ik.evaluate(name, v[0], start, pr.target_pos, pr.target_rot)
    assert (np.abs(out["error"][:, 0] - ep) <= ik.POS_BAR * (1 + tmax)).all() and (np.abs(out["error"][:, 1] - er) <= ik.ROT_BAR).all()
    far = (ep > ik.POS_TOL + ik.POS_BAR * (1 + tmax)) | (er > ik.ROT_TOL + ik.ROT_BAR)      # clearly outside / inside the tolerances in fp64
    near = (ep < ik.POS_TOL - ik.POS_BAR * (1 + tmax)) & (er < ik.ROT_TOL - ik.ROT_BAR)
    assert far.sum() >= c.N - 2 and (out["status"][far] == _capi.RSB_IK_MAX_ITER).all() and (out["status"][near] == _capi.RSB_IK_CONVERGED).all()
    # the frames' own places as targets: converged at once
    kin = w.frame_kinematics(ik.frame_sets(name)[v[0]], pos=True, rot=True)
    here = w.inverse_kinematics(ik.frame_sets(name)[v[0]], kin["pos"], kin["rot"] if v[1] else None, dof_mask=ik.dof_mask(name, v[2]), **dict(SETTINGS, max_iter=0))
    assert (here["status"] == _capi.RSB_IK_CONVERGED).all() and here["gc"].tobytes() == start.tobytes() and not here["iterations"].any()
    # ... and with steps allowed nothing moves either
    here = w.inverse_kinematics(ik.frame_sets(name)[v[0]], kin["pos"], kin["rot"] if v[1] else None, dof_mask=ik.dof_mask(name, v[2]), **SETTINGS)
    assert (here["status"] == _capi.RSB_IK_CONVERGED).all() and here["gc"].tobytes() == start.tobytes() and not here["iterations"].any()
    w.close()


def test_dependent_rows(built_lib):
    """the same point listed twice: singular without damping (no step taken), solvable with it"""
    name = "anymal"
    c = dyn_case(name)
    v = ("one", False, False)
    pr = ik.problem(name, *v)
    frames = ik.frame_sets(name)["one"] * 2
    tp = np.ascontiguousarray(np.repeat(pr.target_pos, 2, axis=1))
    start = np.ascontiguousarray(c.gc, np.float32)
    w = new_world(c)
    out = w.inverse_kinematics(frames, tp, **dict(SETTINGS, damping=0.0))
    assert (out["status"] == _capi.RSB_IK_SINGULAR).all() and not out["iterations"].any() and out["gc"].tobytes() == start.tobytes()
    out = w.inverse_kinematics(frames, tp, **SETTINGS)
    w.close()
    assert (out["status"] == _capi.RSB_IK_CONVERGED).all()
    ep, _, tmax = ik.evaluate(name, "one", out["gc"], pr.target_pos)
    assert (ep <= ik.bars(tmax, False)[0]).all()


L1, L2, ELBOW_UPPER = 0.4, 0.3, 1.0
ARM = f"""<?xml version="1.0"?>
<robot name="planar_arm">
  <link name="world"/>
  <link name="mount"><inertial><origin xyz="0 0 0"/><mass value="0.5"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial></link>
  <joint name="bolt" type="fixed"><origin xyz="0 0 0"/><parent link="world"/><child link="mount"/></joint>
  <link name="upper"><inertial><origin xyz="0.2 0 0"/><mass value="1"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial></link>
  <joint name="shoulder" type="revolute"><origin xyz="0 0 0"/><parent link="mount"/><child link="upper"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-3" upper="3"/></joint>
  <link name="fore"><inertial><origin xyz="0.15 0 0"/><mass value="1"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial></link>
  <joint name="elbow" type="revolute"><origin xyz="{L1} 0 0"/><parent link="upper"/><child link="fore"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-2.5" upper="{ELBOW_UPPER}"/></joint>
</robot>
"""


def arm_tip(q1, q2):
    """rotation about y by q takes x to (cos q, 0, -sin q)"""
    return np.stack([L1 * np.cos(q1) + L2 * np.cos(q1 + q2), np.zeros_like(q1), -(L1 * np.sin(q1) + L2 * np.sin(q1 + q2))], axis=-1)


def test_two_link_arm_closed_form_and_joint_limits(built_lib):
    model = Model(urdf_string=ARM)
    assert model.blob.fixed_base and model.nv == 8 and float(model.blob.q_upper[2]) == ELBOW_UPPER
    n = 6
    tip = [(2, (L2, 0.0, 0.0))]
    start = np.zeros((n, model.nq), np.float32)
    start[:, 3] = 1.0
    start[:, 7] = np.linspace(-0.4, 0.6, n); start[:, 8] = 0.5      # the elbow's positive branch
    w = BatchedWorld(model, n)
    w.set_state(start, np.zeros((n, model.nv), np.float32))

    def fp64(gc, target):
        p = np.array([(lambda k: k.p[2] + k.R[2] @ np.array(tip[0][1]))(kinematics(model.blob, g.astype(float))) for g in gc])
        return np.abs(p - target).max(axis=1)

    # inside the limits: the law of cosines on the start's branch
    q1, q2 = np.linspace(0.3, -0.5, n), np.linspace(0.2, 0.9, n)
    target = arm_tip(q1, q2).astype(np.float32)
    out = w.inverse_kinematics(tip, target[:, None, :], **SETTINGS)
    assert (out["status"] == _capi.RSB_IK_CONVERGED).all()
    t64 = target.astype(float)
    r2 = t64[:, 0] ** 2 + t64[:, 2] ** 2
    elbow = np.arccos((r2 - L1 * L1 - L2 * L2) / (2 * L1 * L2))      # positive: the start's branch
    for e in range(n):
        g = out["gc"][e].astype(float)
        k = kinematics(model.blob, g)
        Jl, _ = jacobians(model.blob, k, 2, k.p[2] + k.R[2] @ np.array(tip[0][1]))
        Jinv = np.linalg.inv(Jl[[0, 2]][:, [6, 7]])
        bound = np.abs(Jinv).sum(axis=1).max() * (ik.POS_TOL + ik.POS_BAR * (1 + np.abs(t64[e]).max()))
        assert abs(g[8] - elbow[e]) <= bound, (e, g[8], elbow[e], bound)
    # the elbow beyond its upper limit: reached without the flag ...
    q2 = np.full(n, 1.3)
    target = arm_tip(q1, q2).astype(np.float32)
    out = w.inverse_kinematics(tip, target[:, None, :], **SETTINGS)
    assert (out["status"] == _capi.RSB_IK_CONVERGED).all() and (out["gc"][:, 8] > np.float32(ELBOW_UPPER)).all()
    assert (fp64(out["gc"], target.astype(float)) <= ik.POS_TOL + ik.POS_BAR * (1 + np.abs(target).max(axis=1))).all()
    # ... and with it every iterate stays inside, the target is not met and the error is the fp64 one
    lo, hi = np.float32(model.blob.q_lower[2]), np.float32(model.blob.q_upper[2])
    for steps in (0, 1, 2, 3, 5, 8, 13, ik.MAX_ITER):
        lim = w.inverse_kinematics(tip, target[:, None, :], joint_limits=True, **dict(SETTINGS, max_iter=steps))
        assert (lim["gc"][:, 8] >= lo).all() and (lim["gc"][:, 8] <= hi).all() and (np.abs(lim["gc"][:, 7]) <= np.float32(3.0)).all(), steps
        assert (lim["status"] != _capi.RSB_IK_CONVERGED).all(), steps
        assert (np.abs(lim["error"][:, 0] - fp64(lim["gc"], target.astype(float))) <= ik.POS_BAR * (1 + np.abs(target).max(axis=1))).all(), steps
    assert (lim["status"] == _capi.RSB_IK_MAX_ITER).all() and (lim["iterations"] == ik.MAX_ITER).all()
    w.close()


def test_argument_errors(built_lib):
    """every listed argument error: RSB_E_INVALID, the outputs untouched, a message that names the function"""
    L = built_lib
    c = dyn_case("anymal")
    w = new_world(c, 4)
    n, nq, nv = 4, c.model.nq, c.nv
    F = 2
    fr = (_capi.Frame * F)()
    for k in range(F):
        fr[k].body = c.nb - 1 - k
    tp, tr, q0 = np.zeros((n, F, 3), np.float32), np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, F, 1)), np.ascontiguousarray(c.gc[:n], np.float32)
    outs = [np.full((n, nq), 7, np.float32), np.full((n, 2), 7, np.float32), np.full(n, 7, np.int32), np.full(n, 7, np.int32)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = dict(h=w.handle, fr=fr, F=F, flags=0, tp=tp, tr=None, q0=q0, mask=None, opt=_capi.IkOptions(10, 1e-3, 1e-4, 1e-4, 0.5), outs=outs, space=0)

    def call(**kw):
        a = dict(good); a.update(kw)
        opt = a["opt"]
        return L.rsb_inverse_kinematics(a["h"], a["fr"], a["F"], a["flags"], p(a["tp"]), p(a["tr"]), p(a["q0"]), p(a["mask"]), None if opt is None else C.byref(opt),
                                        *[p(o) for o in a["outs"]], a["space"])
    assert call() == 0 and not (outs[2] == 7).all()
    for o in outs:
        o[...] = 7
    bad_frame, nan_frame = (_capi.Frame * F)(), (_capi.Frame * F)()
    bad_frame[0].body = c.nb
    nan_frame[0].offset[1] = float("nan")
    O = _capi.IkOptions
    bad = {"null world": dict(h=None), "bad space": dict(space=2), "every output NULL": dict(outs=[None] * 4), "n_frames 0": dict(F=0),
           "n_frames 17": dict(fr=(_capi.Frame * 17)(), F=17), "frames NULL": dict(fr=None), "bad body": dict(fr=bad_frame), "non-finite offset": dict(fr=nan_frame),
           "unknown flag": dict(flags=4), "target_pos NULL": dict(tp=None), "target_rot without the flag": dict(tr=tr), "the flag without target_rot": dict(flags=1),
           "opt NULL": dict(opt=None), "max_iter < 0": dict(opt=O(-1, 1e-3, 1e-4, 1e-4, 0.5)), "damping < 0": dict(opt=O(10, -1e-3, 1e-4, 1e-4, 0.5)),
           "damping nan": dict(opt=O(10, float("nan"), 1e-4, 1e-4, 0.5)), "pos_tol < 0": dict(opt=O(10, 1e-3, -1e-4, 1e-4, 0.5)),
           "rot_tol inf": dict(opt=O(10, 1e-3, 1e-4, float("inf"), 0.5)), "max_step < 0": dict(opt=O(10, 1e-3, 1e-4, 1e-4, -0.5)),
           "max_step nan": dict(opt=O(10, 1e-3, 1e-4, 1e-4, float("nan"))), "max_step 0": dict(opt=O(10, 1e-3, 1e-4, 1e-4, 0.0)),
           "a mask that frees nothing": dict(mask=np.zeros(nv, np.uint8))}
    for what, kw in bad.items():
        assert call(**kw) == -1, what
        assert L.rsb_last_error().startswith(b"rsb_inverse_kinematics: "), (what, L.rsb_last_error())
        assert all((o == 7).all() for o in outs), what
    w.close()
    # a fixed base's six mask entries are ignored: freeing only them frees nothing
    cf = dyn_case("fixed2")
    wf = new_world(cf, 2)
    mask = np.zeros(cf.nv, np.uint8); mask[:6] = 1
    with pytest.raises(_capi.RsbError, match="rsb_inverse_kinematics"):
        wf.inverse_kinematics(ik.frame_sets("fixed2")["one"], np.zeros((2, 1, 3), np.float32), dof_mask=mask)
    wf.close()


def test_parity_record(built_lib):
    """per variant: the largest residual over its bar and the largest iteration count on the device and in the restatement -> profiles/ik_parity.txt"""
    lines = ["rsb_inverse_kinematics on the device against the fp64 evaluation and the numpy float32 restatement (tests/test_gpu_ik.py::test_parity_record).",
             f"settings: max_iter {ik.MAX_ITER}, damping {ik.DAMPING}, max_step {ik.MAX_STEP}, pos_tol {ik.POS_TOL}, rot_tol {ik.ROT_TOL}; every env of every variant.",
             "bars: position pos_tol + 1e-5 (1 + max|target|), rotation rot_tol + 6e-5; a ratio <= 1 meets its bar.",
             "", f"{'case':10s} {'frames':8s} {'ang':>3s} {'base':>5s} {'m':>3s}  {'pos/bar':>8s} {'rot/bar':>8s}  {'iters dev':>9s} {'iters f32':>9s}"]
    for name in ik.CASES:
        for v in ik.variants(name):
            out = device(name).out[v]
            rp, rr, _, _ = figures(name, v, out)
            it32 = ik.restated(name, *v)[2]
            lines.append(f"{name:10s} {v[0]:8s} {int(v[1]):3d} {'free' if v[2] else 'held':>5s} {ik.rows_of(name, v[0], v[1]):3d}  {rp.max():8.3f} {rr.max():8.3f}  "
                         f"{int(out['iterations'].max()):9d} {int(it32.max()):9d}")
    with open(os.path.join(ROOT, "profiles", "ik_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
