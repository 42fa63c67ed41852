"""Batched frame accelerations, Jacobian rates and IMU readings on the device (rsb_get_frame_accelerations, rsb_get_frame_jacobian_rates,
rsb_imu_observe; raisimlib_amd/csrc/rsb_frame_accel.hip) against the fp64 references of tests/test_frame_accel_reference.py on the float32-rounded
state and udot the device saw.  Cases: test_dynamics_reference.NAMES (14 random trees with prismatic joints and tilted gravity at N = 67, the 40-body
tree, the two shipped models at N = 64).  Frames: every body origin, every collision primitive's centre and the case's three offset frames, in calls
of at most 64 frames, one of them exactly 64.  EVERY env and frame of EVERY case has to meet its bar.

Bars, both the project's (tests/test_gpu_dynamics.py, tests/test_gpu_frames.py):
  lin_acc, ang_acc, the accelerometer columns, Jdot_lin, Jdot_rot   |dev - ref| <= 2e-5 (1 + S), S the largest component of the reference's sum of
                                                                    absolute terms for that env, frame and quantity;
  the gyro columns                                                  max |dev - ref| <= 2e-5 (1 + max |ref|) per env, the bar of ang_vel.
N x F and the workgroups: the trees' N = 67 leaves the last workgroup of both kernels partly filled in at least one call of every case (asserted);
the shipped models' N = 64 is a multiple of the 64 pairs a workgroup of the rates kernel takes - their tails are those of the 1- and 63-env worlds
of test_determinism_and_plumbing, which give the bits of the 64-env world.
test_parity_record writes the largest error / bar per quantity and model to profiles/frame_accel_parity.txt."""
import ctypes as C
import functools
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from common import ROOT, f32, standing_states
from raisimlib_amd import BatchedWorld, _capi, workload
from test_dynamics_reference import NAMES, dyn_case
from test_frame_accel_reference import pendulum_case, ref_accel, ref_jacobian_rates, sphere_case, with_flags
from test_gpu_frames import all_frames, chunks_of, frames_f32

pytestmark = pytest.mark.gpu

FLAGS = list(itertools.product((False, True), (False, True)))      # (local, proper)
BAR = 2e-5


def case_frames(c):
    return all_frames(c.model) + frames_f32(c.frames)


def case_calls(c):
    """the calls of a case: lists of indices into case_frames(c), at most 64 each, one of exactly 64 (it lists frames again where there are fewer)"""
    return chunks_of(list(range(len(case_frames(c)))))


def pairs_per_workgroup(blob):
    """of frame_jacobian_rates_kernel, as rsb_get_frame_jacobian_rates computes it: 13 floats of head + 13 per level, odd pitch, 48 KB"""
    pitch = (13 + 13 * max(1, blob.depth - 1)) | 1
    return max(1, min(64, 12288 // pitch))


def new_world(c, n=None, gv=None):
    n = n or c.N
    w = BatchedWorld(c.model, n)
    w.set_gravity(c.gravity)
    w.set_state(c.gc[:n], (c.gv if gv is None else gv)[:n])
    return w


def query(w, frames, udot):
    """everything the three entry points say about one call's frames: acc[(has_udot, local, proper)] = {"lin", "ang"}, rates = {"lin", "rot"},
    imu[has_udot]"""
    d = SimpleNamespace(acc={}, imu={})
    for ud in (udot, None):
        for local, proper in FLAGS:
            d.acc[(ud is not None, local, proper)] = w.frame_accelerations(frames, ud, local=local, proper=proper, lin=True, ang=True)
        d.imu[ud is not None] = w.imu_observe(frames, ud)
    d.rates = w.frame_jacobian_rates(frames, lin=True, rot=True)
    return d


@functools.lru_cache(maxsize=None)
def device(name):
    """per call (chunk of frames) of one case: the frames and query() of them, all from one world; each output alone is compared on the way"""
    c = dyn_case(name)
    w = new_world(c)
    out, frames = [], case_frames(c)
    for idx in case_calls(c):
        fr = [frames[i] for i in idx]
        d = query(w, fr, c.udot)
        for (has, local, proper), both in d.acc.items():      # each output alone: the other is NULL
            ud = c.udot if has else None
            lin = w.frame_accelerations(fr, ud, local=local, proper=proper, lin=True, ang=False)
            ang = w.frame_accelerations(fr, ud, local=local, proper=proper, lin=False, ang=True)
            assert sorted(lin) == ["lin"] and sorted(ang) == ["ang"]
            assert np.array_equal(lin["lin"], both["lin"]) and np.array_equal(ang["ang"], both["ang"]), (name, has, local, proper)
        assert np.array_equal(w.frame_jacobian_rates(fr, lin=True, rot=False)["lin"], d.rates["lin"])
        assert np.array_equal(w.frame_jacobian_rates(fr, lin=False, rot=True)["rot"], d.rates["rot"])
        out.append((fr, d))
    w.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """per call: acc[(has_udot, local, proper)] = [ref_accel per env], rates = [ref_jacobian_rates per env]; computed once per env on all the
    case's frames, a call picks its own"""
    c = dyn_case(name)
    frames = case_frames(c)
    rates = [ref_jacobian_rates(c.blob, c.gc[e], c.gv[e], frames) for e in range(c.N)]
    acc = {}
    for has in (True, False):
        world = [ref_accel(c.blob, c.gc[e], c.gv[e], c.udot[e] if has else None, frames) for e in range(c.N)]
        for local, proper in FLAGS:
            acc[(has, local, proper)] = [with_flags(x, c.gravity, local, proper) for x in world]
    out = []
    for idx in case_calls(c):
        pick = lambda x: SimpleNamespace(**{k: v[idx] for k, v in vars(x).items()})
        out.append(SimpleNamespace(acc={key: [pick(x) for x in xs] for key, xs in acc.items()}, rates=[tuple(a[idx] for a in r) for r in rates]))
    return out


def ratios(name):
    """the largest error / bar per quantity over every call, variant, env and frame of one case"""
    c = dyn_case(name)
    worst = dict(lin_acc=0.0, ang_acc=0.0, accelerometer=0.0, gyro=0.0, Jdot_lin=0.0, Jdot_rot=0.0)
    for (fr, d), r in zip(device(name), reference(name)):
        for key, refs in r.acc.items():
            got = d.acc[key]
            for e, ref in enumerate(refs):
                rl = np.abs(got["lin"][e].astype(np.float64) - ref.lin).max(axis=1) / (BAR * (1 + ref.s_lin.max(axis=1)))
                ra = np.abs(got["ang"][e].astype(np.float64) - ref.ang).max(axis=1) / (BAR * (1 + ref.s_ang.max(axis=1)))
                worst["lin_acc"], worst["ang_acc"] = max(worst["lin_acc"], rl.max()), max(worst["ang_acc"], ra.max())
        for has in (True, False):
            imu = d.imu[has].astype(np.float64)
            for e, ref in enumerate(r.acc[(has, True, True)]):
                rl = np.abs(imu[e, :, :3] - ref.lin).max(axis=1) / (BAR * (1 + ref.s_lin.max(axis=1)))
                gyro = np.einsum("fji,fj->fi", ref.R, ref.w)
                rg = np.abs(imu[e, :, 3:] - gyro).max() / (BAR * (1 + np.abs(gyro).max()))
                worst["accelerometer"], worst["gyro"] = max(worst["accelerometer"], rl.max()), max(worst["gyro"], rg)
        for e, (jl, jr, sl, sr) in enumerate(r.rates):
            rl = np.abs(d.rates["lin"][e].astype(np.float64) - jl).max(axis=(1, 2)) / (BAR * (1 + sl))
            rr = np.abs(d.rates["rot"][e].astype(np.float64) - jr).max(axis=(1, 2)) / (BAR * (1 + sr))
            worst["Jdot_lin"], worst["Jdot_rot"] = max(worst["Jdot_lin"], rl.max()), max(worst["Jdot_rot"], rr.max())
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_parity(built_lib, name):
    """every env and frame of the case: both accelerations with udot given and NULL under all four flag combinations (all outputs together; each
    alone has the same bits), the IMU rows, both Jacobian rates"""
    c = dyn_case(name)
    sizes = [len(fr) for fr, _ in device(name)]
    assert 64 in sizes and max(sizes) <= 64
    if c.N % 64:
        ppb = pairs_per_workgroup(c.blob)
        assert any((c.N * s) % ppb and (c.N * s) % 256 for s in sizes), (name, sizes, ppb)
    worst = ratios(name)
    print(f"{name}: error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (name, worst)
    for fr, d in device(name):      # the accelerometer columns are the local proper acceleration, bit for bit
        for has in (True, False):
            assert np.array_equal(d.imu[has][:, :, :3], d.acc[(has, True, True)]["lin"])
        if c.fixed:
            assert not d.rates["lin"][..., :6].any() and not d.rates["rot"][..., :6].any()


def chain_urdf(n):
    """a serial chain of n links (tree depth n): revolute joints about alternating axes, every fifth joint prismatic, tilted joint frames"""
    axes = ("1 0 0", "0 1 0", "0 0 1")
    out = ['<?xml version="1.0"?>', '<robot name="chain">']
    for i in range(n):
        out.append(f'  <link name="l{i}"><inertial><origin xyz="0.02 0 -0.03"/><mass value="{1.0 + 0.1 * i}"/>'
                   '<inertia ixx="0.01" ixy="0" ixz="0" iyy="0.012" iyz="0" izz="0.008"/></inertial></link>')
    for i in range(1, n):
        kind = "prismatic" if i % 5 == 0 else "revolute"
        out.append(f'  <joint name="j{i}" type="{kind}"><origin xyz="{0.05 * (i % 3)} {0.04 * ((i + 1) % 2)} -0.1" rpy="{0.1 * (i % 4)} {-0.15 * (i % 3)} 0.2"/>'
                   f'<parent link="l{i - 1}"/><child link="l{i}"/><axis xyz="{axes[i % 3]}"/><limit effort="100" velocity="100" lower="-3" upper="3"/></joint>')
    out.append("</robot>")
    return "\n".join(out)


def test_a_deep_chain_takes_fewer_pairs_per_workgroup(built_lib):
    """A serial chain of 17 bodies (tree depth 17, the deepest the step kernel is built for): the chain records of 64 pairs no longer fit the 48 KB,
    a workgroup of the rates kernel takes 55, and 5 envs x 18 frames fill one workgroup and part of a second.  Every output at the bars above."""
    from raisimlib_amd import Model
    model = Model(urdf_string=chain_urdf(17))
    blob, n = model.blob, 5
    assert blob.depth == 17 and pairs_per_workgroup(blob) == 55
    rng = np.random.default_rng(17)
    gc = np.zeros((n, model.nq)); gc[:, :3] = rng.uniform(-1, 1, (n, 3))
    qq = rng.normal(size=(n, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.8, 0.8, (n, model.nq - 7))
    gc, gv, udot = f32(gc), f32(rng.normal(size=(n, model.nv))), f32(rng.normal(size=(n, model.nv)))
    frames = frames_f32([(i, (0.0, 0.0, 0.0)) for i in range(model.nb)] + [(model.nb - 1, (0.05, -0.02, 0.1))])
    assert (n * len(frames)) % 55
    w = BatchedWorld(model, n)
    w.set_state(gc, gv)
    acc = w.frame_accelerations(frames, udot, lin=True, ang=True)
    rates = w.frame_jacobian_rates(frames, lin=True, rot=True)
    w.close()
    for e in range(n):
        ref = ref_accel(blob, gc[e], gv[e], udot[e], frames)
        jl, jr, sl, sr = ref_jacobian_rates(blob, gc[e], gv[e], frames)
        assert (np.abs(acc["lin"][e] - ref.lin).max(axis=1) <= BAR * (1 + ref.s_lin.max(axis=1))).all(), e
        assert (np.abs(acc["ang"][e] - ref.ang).max(axis=1) <= BAR * (1 + ref.s_ang.max(axis=1))).all(), e
        assert (np.abs(rates["lin"][e] - jl).max(axis=(1, 2)) <= BAR * (1 + sl)).all(), e
        assert (np.abs(rates["rot"][e] - jr).max(axis=(1, 2)) <= BAR * (1 + sr)).all(), e
        assert np.abs(jl).max() > 0.1 and np.abs(jr).max() > 0.1


def test_consistency_with_the_jacobians_and_kinematics(built_lib):
    """ANYmal-like, N = 64, on the device's own outputs: lin_acc(udot) - lin_acc(NULL) = J_lin udot with J_lin of rsb_get_frame_jacobians,
    lin_acc(NULL) = Jdot_lin gv, the same two for ang; and the gyro is R^T ang_vel of rsb_get_frame_kinematics - all under the bars above."""
    c = dyn_case("anymal")
    w = new_world(c)
    for (fr, d), r in zip(device("anymal"), reference("anymal")):
        J = w.frame_jacobians(fr, lin=True, rot=True)
        kin = w.frame_kinematics(fr, pos=False, rot=True, ang_vel=True)
        full, bias = d.acc[(True, False, False)], d.acc[(False, False, False)]
        for e in range(c.N):
            ref = r.acc[(True, False, False)][e]
            bl, ba = BAR * (1 + ref.s_lin.max(axis=1)), BAR * (1 + ref.s_ang.max(axis=1))
            for out, Jm, Jd, bar in (("lin", J["lin"], d.rates["lin"], bl), ("ang", J["rot"], d.rates["rot"], ba)):
                diff = full[out][e].astype(np.float64) - bias[out][e]
                assert (np.abs(diff - Jm[e].astype(np.float64) @ c.udot[e]).max(axis=1) <= bar).all(), (out, e)
                assert (np.abs(bias[out][e] - Jd[e].astype(np.float64) @ c.gv[e]).max(axis=1) <= bar).all(), (out, e)
            gyro = np.einsum("fji,fj->fi", kin["rot"][e].astype(np.float64), kin["ang_vel"][e].astype(np.float64))
            assert np.abs(d.imu[True][e, :, 3:] - gyro).max() <= BAR * (1 + np.abs(gyro).max()), e
    w.close()


def test_determinism_and_plumbing(built_lib):
    """ANYmal-like: a subset / permutation of the frames gives the bits of the all-frames call; RSB_HOST and RSB_DEVICE (torch tensors on torch's
    stream) give the same bits; udot NULL equals udot of zeros as numbers; worlds of 1, 63 and 4096 envs give, env for env, the bits of the 64-env
    world; a row stride of 6 F + 5 leaves the five guard columns of every row as they were, in host and in device memory."""
    import torch
    c = dyn_case("anymal")
    N = c.N
    frames = case_frames(c)[:64]
    F = len(frames)
    w = new_world(c)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    full = query(w, frames, c.udot)
    pick = [int(i) for i in np.random.default_rng(0).permutation(F)[:9]]
    sub = query(w, [frames[i] for i in pick], c.udot)
    one = query(w, [frames[5]], c.udot)
    for key in full.acc:
        for n in ("lin", "ang"):
            assert np.array_equal(sub.acc[key][n], full.acc[key][n][:, pick]) and np.array_equal(one.acc[key][n][:, 0], full.acc[key][n][:, 5]), (key, n)
    for n in ("lin", "rot"):
        assert np.array_equal(sub.rates[n], full.rates[n][:, pick]) and np.array_equal(one.rates[n][:, 0], full.rates[n][:, 5]), n
    for has in (True, False):
        assert np.array_equal(sub.imu[has], full.imu[has][:, pick])
    zeros = w.frame_accelerations(frames, np.zeros_like(c.udot), lin=True, ang=True)
    assert np.array_equal(zeros["lin"], full.acc[(False, False, False)]["lin"]) and np.array_equal(zeros["ang"], full.acc[(False, False, False)]["ang"])
    assert np.array_equal(w.imu_observe(frames, np.zeros_like(c.udot)), full.imu[False])
    # RSB_DEVICE: torch tensors in, results in them, nothing synchronised by the library (the world runs on torch's stream here)
    dev = torch.device("cuda:0")
    tud = torch.from_numpy(np.ascontiguousarray(c.udot, np.float32)).to(dev)
    ta = {n: torch.full((N, F, 3), 7.0, dtype=torch.float32, device=dev) for n in ("lin", "ang")}
    tj = {n: torch.full((N, F, 3, c.nv), 7.0, dtype=torch.float32, device=dev) for n in ("lin", "rot")}
    ti = torch.full((N, F, 6), 7.0, dtype=torch.float32, device=dev)
    assert w.frame_accelerations(frames, tud, local=True, proper=True, out=ta) is ta and w.frame_jacobian_rates(frames, out=tj) is tj
    assert w.imu_observe(frames, tud, out=ti) is ti
    for n in ("lin", "ang"):
        assert np.array_equal(ta[n].cpu().numpy(), full.acc[(True, True, True)][n]), n
    assert np.array_equal(tj["lin"].cpu().numpy(), full.rates["lin"]) and np.array_equal(tj["rot"].cpu().numpy(), full.rates["rot"])
    assert np.array_equal(ti.cpu().numpy(), full.imu[True])
    only = {"ang": torch.full((N, F, 3), 7.0, dtype=torch.float32, device=dev)}
    w.frame_accelerations(frames, None, out=only)
    assert np.array_equal(only["ang"].cpu().numpy(), full.acc[(False, False, False)]["ang"])
    # the IMU rows inside a wider observation: columns [0, 6 F) of rows of 6 F + 5 floats, the five guard columns untouched
    stride = 6 * F + 5
    obs = torch.full((N, stride), 7.0, dtype=torch.float32, device=dev)
    w.imu_observe(frames, tud, out=obs, row_stride=stride)
    host = np.full((N, stride), 7.0, np.float32)
    w.imu_observe(frames, c.udot, out=host, row_stride=stride)
    for got in (obs.cpu().numpy(), host):
        assert np.array_equal(got[:, :6 * F].reshape(N, F, 6), full.imu[True]) and np.all(got[:, 6 * F:] == 7.0)
    shifted = torch.full((N, stride), 7.0, dtype=torch.float32, device=dev)      # ... and behind other columns: a view's data pointer
    w.imu_observe(frames[:3], tud, out=shifted[:, 4:], row_stride=stride)
    got = shifted.cpu().numpy()
    assert np.array_equal(got[:, 4:22].reshape(N, 3, 6), full.imu[True][:, :3]) and np.all(got[:, :4] == 7.0) and np.all(got[:, 22:] == 7.0)
    w.close()
    # grid tails: an env's results depend on its own rows alone
    for n in (1, 63, 4096):      # (the 4096-env world asks for the nine picked frames: 4096 x 64 Jacobian rates are 113 MB to bring back)
        idx = np.arange(n) % N
        sel = pick if n == 4096 else list(range(F))
        fr = [frames[i] for i in sel]
        at = np.ix_(idx, sel)
        w = BatchedWorld(c.model, n)
        w.set_gravity(c.gravity)
        w.set_state(c.gc[idx], c.gv[idx])
        a = w.frame_accelerations(fr, c.udot[idx], local=True, proper=True, lin=True, ang=True)
        j = w.frame_jacobian_rates(fr, lin=True, rot=True)
        m = w.imu_observe(fr, c.udot[idx])
        w.close()
        for k in ("lin", "ang"):
            assert np.array_equal(a[k], full.acc[(True, True, True)][k][at]), (n, k)
        assert np.array_equal(j["lin"], full.rates["lin"][at]) and np.array_equal(j["rot"], full.rates["rot"][at]), n
        assert np.array_equal(m, full.imu[True][at]), n


@pytest.mark.parametrize("name", ["fixed1", "fixed3"])
def test_a_fixed_bases_rows_do_not_matter(built_lib, name):
    """other noise in the six base rows of gv and udot of a fixed base: not one bit of any output changes"""
    c = dyn_case(name)
    rng = np.random.default_rng(1)
    gv, udot = c.gv.copy(), c.udot.copy()
    for x in (gv, udot):
        x[:, :6] = f32(rng.normal(size=(c.N, 6)) * 10)
    w = new_world(c, gv=gv)
    for fr, d in device(name):
        got = query(w, fr, udot)
        for key in d.acc:
            assert np.array_equal(got.acc[key]["lin"], d.acc[key]["lin"]) and np.array_equal(got.acc[key]["ang"], d.acc[key]["ang"]), key
        assert np.array_equal(got.rates["lin"], d.rates["lin"]) and np.array_equal(got.rates["rot"], d.rates["rot"])
        assert np.array_equal(got.imu[True], d.imu[True]) and np.array_equal(got.imu[False], d.imu[False])
    w.close()


def test_queries_leave_the_world_alone_and_follow_pipelined_steps(built_lib):
    """Control steps of the benchmark's quadruped world, K = 3.  (a) lock-step with all three queries between the steps: the state after every step
    and the contact list after the last are those of a run without the queries, bit for bit - the third step would show a changed warm state.
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
    udot = f32(np.random.default_rng(4).normal(size=(n, model.nv)))
    frames = frames_f32([(0, (0.1, 0.0, 0.05)), (model.nb - 1, (0.0, 0.0, -0.1)), (6, (0.0, 0.0, 0.0))])
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
                a = w.frame_accelerations(frames, udot, lin=True, ang=True)
                j = w.frame_jacobian_rates(frames, lin=True, rot=True)
                answers.append((a["lin"], a["ang"], j["lin"], j["rot"], w.imu_observe(frames, udot)))
            if mode != "pipelined":
                states.append(w.get_state())
        states.append(w.get_state())
        runs[mode] = (states, w.get_contacts(), answers)
        w.close()
    for (qa, ua), (qb, ub) in zip(runs["plain"][0], runs["queried"][0]):
        assert np.array_equal(qa, qb) and np.array_equal(ua, ub)
    assert np.array_equal(runs["plain"][1][0], runs["queried"][1][0]) and runs["plain"][1][1].tobytes() == runs["queried"][1][1].tobytes()
    assert runs["plain"][1][0].sum() > 0
    for xs, ys in zip(runs["queried"][2], runs["pipelined"][2]):
        for x, y in zip(xs, ys):
            assert np.array_equal(x, y)
    assert np.array_equal(runs["pipelined"][0][-1][0], runs["plain"][0][-1][0])


def test_bad_input_fails_loudly_and_touches_nothing(built_lib, anymal):
    """every argument error of rsb.h: RSB_E_INVALID, a message, the sentinel in the outputs intact"""
    n = 8
    gc, gv = workload.random_state(anymal.nq, anymal.nv, n, seed=4)
    w = BatchedWorld(anymal, n)
    w.set_state(gc, gv)
    L, h = w.L, w.handle
    out = np.full((n, 2 * 3 * anymal.nv + 64), 7.0, np.float32)
    p = out.ctypes.data_as(C.c_void_p)
    ud = np.zeros((n, anymal.nv), np.float32)
    q = ud.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 2)()
    fr[1].body = 3
    bad_body, bad_off = (_capi.Frame * 1)(), (_capi.Frame * 1)()
    bad_body[0].body = anymal.nb
    bad_off[0].offset[1] = float("nan")
    cases = [
        (lambda: L.rsb_get_frame_accelerations(h, fr, 2, q, 0, None, None, 0), b"every output is NULL"),
        (lambda: L.rsb_get_frame_jacobian_rates(h, fr, 2, None, None, 0), b"every output is NULL"),
        (lambda: L.rsb_imu_observe(h, fr, 2, q, None, 0, 0), b"NULL"),
        (lambda: L.rsb_get_frame_accelerations(h, fr, 0, q, 0, p, p, 0), b"n_frames"),
        (lambda: L.rsb_get_frame_accelerations(h, None, 2, q, 0, p, p, 0), b"n_frames"),
        (lambda: L.rsb_get_frame_jacobian_rates(h, fr, 65, p, p, 0), b"n_frames"),
        (lambda: L.rsb_imu_observe(h, fr, -1, q, p, 0, 0), b"n_frames"),
        (lambda: L.rsb_get_frame_accelerations(h, bad_body, 1, q, 0, p, p, 0), b"body"),
        (lambda: L.rsb_get_frame_jacobian_rates(h, bad_off, 1, p, p, 0), b"non-finite"),
        (lambda: L.rsb_imu_observe(h, bad_body, 1, q, p, 0, 0), b"body"),
        (lambda: L.rsb_get_frame_accelerations(h, fr, 2, q, 4, p, p, 0), b"flag"),
        (lambda: L.rsb_get_frame_accelerations(h, fr, 2, q, -1, p, p, 0), b"flag"),
        (lambda: L.rsb_imu_observe(h, fr, 2, q, p, 6 * 2 - 1, 0), b"row_stride"),
        (lambda: L.rsb_imu_observe(h, fr, 2, q, p, -3, 1), b"row_stride"),
        (lambda: L.rsb_get_frame_accelerations(h, fr, 2, q, 0, p, p, 2), b"space"),
        (lambda: L.rsb_get_frame_jacobian_rates(h, fr, 2, p, p, -1), b"space"),
        (lambda: L.rsb_imu_observe(h, fr, 2, q, p, 0, 7), b"space"),
    ]
    for k, (call, msg) in enumerate(cases):
        assert call() == -1, k          # RSB_E_INVALID
        assert msg in L.rsb_last_error(), (k, L.rsb_last_error())
        assert np.all(out == 7.0), k
    with pytest.raises(ValueError):
        w.frame_accelerations([0], lin=False)
    with pytest.raises(ValueError):
        w.frame_jacobian_rates([0], out={"J": out})
    with pytest.raises(ValueError):
        w.frame_accelerations([0], np.zeros((n, 3), np.float32))
    with pytest.raises(ValueError):
        w.imu_observe([0], row_stride=9)
    assert L.rsb_imu_observe(h, fr, 2, None, p, 12, 0) == 0 and np.all(out.ravel()[n * 12:] == 7.0)      # row_stride = 6 F is the dense call
    w.close()


def test_closed_forms(built_lib):
    """through the C-ABI: the spinning free body (lin_acc = omega x (omega x o)), the pendulum (qdd L t - qd^2 L r) and a robot at rest, where every
    accelerometer reads -R^T g and every gyro zero"""
    model, q, u, fr, om = sphere_case()
    w = BatchedWorld(model, 3)
    w.set_state(np.tile(q, (3, 1)), np.tile(u, (3, 1)))
    got = w.frame_accelerations(fr, None, lin=True, ang=True)
    ref = ref_accel(model.blob, q, u, None, fr)
    w.close()
    for n, (_, off) in enumerate(fr):
        want = np.cross(om, np.cross(om, ref.R[n] @ off))
        assert np.abs(got["lin"][:, n] - want).max() <= BAR * (1 + ref.s_lin[n].max()) and not got["ang"].any()
    model, q, u, ud, fr, L, qd, qdd = pendulum_case()
    w = BatchedWorld(model, 2)
    w.set_state(np.tile(q, (2, 1)), np.tile(u, (2, 1)))
    got = w.frame_accelerations(fr, np.tile(ud, (2, 1)), lin=True, ang=True)
    w.close()
    ref = ref_accel(model.blob, q, u, ud, fr)
    rhat = ref.R[0] @ np.array([0.0, 0.0, -1.0])
    want = qdd * L * np.cross([0.0, 1.0, 0.0], rhat) - qd * qd * L * rhat
    assert np.abs(got["lin"][:, 0] - want).max() <= BAR * (1 + ref.s_lin[0].max())
    assert np.abs(got["ang"][:, 0] - np.array([0.0, qdd, 0.0])).max() <= BAR * (1 + ref.s_ang[0].max())
    c = dyn_case("anymal")
    frames = case_frames(c)[:64]
    w = BatchedWorld(c.model, c.N)
    w.set_gravity(c.gravity)
    w.set_state(c.gc, np.zeros_like(c.gv))
    imu = w.imu_observe(frames, None)
    rot = w.frame_kinematics(frames, pos=False, rot=True)["rot"].astype(np.float64)
    w.close()
    g = np.asarray(c.gravity)
    want = -np.einsum("efji,j->efi", rot, g)
    assert np.abs(imu[:, :, :3] - want).max() <= BAR * (1 + np.abs(g).max()) and not imu[:, :, 3:].any()


def test_parity_record(built_lib):
    """The largest error / bar per quantity and model over all calls and variants, written to profiles/frame_accel_parity.txt (the figures DESIGN.md
    quotes).  Every figure has to be <= 1: this is the union of the parity tests above."""
    lines, fails = [], []
    for name in NAMES:
        c, worst = dyn_case(name), ratios(name)
        lines.append(f"  {name:10s} N {c.N:3d} nb {c.nb:3d} depth {c.blob.depth:2d}  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "\n")
        fails += [(name, k, v) for k, v in worst.items() if not v <= 1.0]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "frame_accel_parity.txt"), "w") as f:
        f.write("tests/test_gpu_frame_accel.py::test_parity_record\n"
                "device fp32 vs fp64 references on the float32-rounded state and udot; largest error / bar over the envs, the frames (every body origin, every\n"
                "collision centre, three offset frames) and the variants (udot given and NULL, world / local, classical / proper).\n"
                "bars: lin_acc, ang_acc, accelerometer, Jdot_lin, Jdot_rot 2e-5 (1 + sum of absolute terms); gyro 2e-5 (1 + max|ref|) per env\n" +
                "".join(lines))
    print("".join(lines))
    assert not fails, fails
