"""Batched contact sensors on the device (rsb_get_body_contact_wrenches, rsb_contact_observe, rsb_contact_timers;
raisimlib_amd/csrc/rsb_contact_sensor.hip) against the fp64 reference of tests/contact_sensor_reference.py fed from get_contacts() and get_state()
of the same world.

Populations (population_inputs): N = 67 - not a multiple of the envs a workgroup owns (12 with the quadruped's 20 frames, 6 with the humanoid's 42), so
the last workgroup is partial - of the ANYmal-like model at kmax 8 and the Atlas-like model at kmax 16, forty control steps after: env e % 4 == 0
held 3 m up (count 0), == 1 standing under nominal targets, == 2 tipped over at the start and driven by random PD targets (non-foot bodies touch; every
other one of them starts sunk into the ground, as after a bad reset, and sits at count == kmax with the overflow flag set), == 3 the benchmark's own targets; one env in four (e % 16 in 0, 5, 10, 15) 50 m from the
origin.  Plus the KAT file's three-link self-collision chain and a fixed-base arm touching the ground.  Frames: every body origin, the feet, three
offset frames; all four flag combinations.

Bars, the project's query bars:
  force, torque, normal force, slip   |dev - ref| <= 2e-5 (1 + S), S the reference's sum of absolute terms (the largest component for vectors)
  count                               equal
  contact flag                        equal wherever the reference's normal force is further than its bar from the threshold (1 N); the share of
                                      (env, frame) pairs this leaves out is printed and has to stay under 1 %
The kernel's arithmetic restated in float32 numpy on the oracle's run of the same populations (a throw-away, before the first device run) ended at
error / bar 0.024 force, 0.016 torque, 0.003 normal force, 0.009 slip (ANYmal-like) and 0.023, 0.009, 0.005, 0.005 (Atlas-like): correct fp32
meets the bars with a factor of 40 to spare, and no (env, frame) pair had its normal force within its bar of the threshold.
test_parity_record writes the largest error / bar per quantity and model to profiles/contact_sensor_parity.txt."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

from common import ROOT, Oracle, f32, sphere_urdf
from contact_sensor_reference import inv_dt_of, sensor_reference, timers_reference
from raisimlib_amd import BatchedWorld, Model, _capi, workload
from test_dynamics_reference import jacobians, kinematics
from test_gpu_frames import frames_f32

pytestmark = pytest.mark.gpu

N = 67
BAR = 2e-5
THRESHOLD = 1.0
STEPS = 40
TIP = 1.57                                      # the tipped quarter: rad the quadruped rolls onto its side / the humanoid pitches onto its front by
AMP = dict(anymal=1.0, atlas=0.2)               # ... the noise on its PD targets, rad (the humanoid's gains are sixty times the quadruped's)
SUNK = dict(anymal=0.1, atlas=-0.6)             # ... and the base height every other env of it starts at: a reset into the ground, more spheres touch than kmax holds
COMBOS = list(itertools.product((False, True), (True, False)))      # (local, include_self)
G = 9.81

ARM_URDF = """<?xml version="1.0"?>
<robot name="arm">
  <link name="world"/>
  <link name="mount"><inertial><origin xyz="0 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial></link>
  <joint name="bolt" type="fixed"><origin xyz="0 0 0.4"/><parent link="world"/><child link="mount"/></joint>
  <link name="upper"><inertial><origin xyz="0.15 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial></link>
  <joint name="shoulder" type="revolute"><origin xyz="0 0 0"/><parent link="mount"/><child link="upper"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
  <link name="fore"><inertial><origin xyz="0.1 0 0"/><mass value="0.5"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial>
    <collision><origin xyz="0.25 0 0"/><geometry><sphere radius="0.05"/></geometry></collision></link>
  <joint name="elbow" type="revolute"><origin xyz="0.3 0 0"/><parent link="upper"/><child link="fore"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
</robot>
"""


@functools.lru_cache(maxsize=None)
def recipe(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench.Recipe(2 if name == "anymal" else 5, -1.0)


def quarters(n):
    e = np.arange(n)
    return e % 4, np.isin(e % 16, (0, 5, 10, 15))


def quat_mul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def population_inputs(name, n=N, steps=STEPS):
    """-> (gc0, gv0, [PD position targets per control step]) of the four quarters, float32-rounded"""
    r = recipe(name)
    nq = r.model.nq
    gc, gv = r.initial_state(n, 0)
    gc, gv = np.array(gc, np.float64), np.zeros_like(np.asarray(gv, np.float64))
    quarter, far = quarters(n)
    gc[quarter == 0, 2] += 3.0
    axis = (1.0, 0.0, 0.0) if name == "anymal" else (0.0, 1.0, 0.0)
    gc[quarter == 2, 3:7] = quat_mul(gc[quarter == 2, 3:7], np.array([np.cos(TIP / 2), *(np.sin(TIP / 2) * np.array(axis))]))
    gc[np.flatnonzero(quarter == 2)[::2], 2] = SUNK[name]
    gc[far, 0] += 50.0
    rng = np.random.default_rng(5)
    nominal = np.asarray(gc[0, 7:])
    targets = []
    for k in range(steps):
        pt = np.array(r.targets(n, k, 0), np.float64)
        pt[quarter == 1, 7:] = nominal
        pt[quarter == 2, 7:] += rng.uniform(-AMP[name], AMP[name], (int((quarter == 2).sum()), nq - 7))
        targets.append(f32(pt))
    return f32(gc), f32(gv), targets


def population_frames(name):
    r = recipe(name)
    b, nb = r.model.blob, r.model.nb
    fr = [(i, (0.0, 0.0, 0.0)) for i in range(nb)] + [(int(b.col_body[s]), tuple(b.col_pos[s])) for s in r.feet]
    return frames_f32(fr + [(0, (0.3, 0.1, -0.05)), (nb - 1, (0.02, -0.01, 0.05)), (nb // 2, (0.0, 0.04, -0.06))])


def answers(w, frames):
    """everything the two read-only entry points say about the frames: {(local, include_self): (force, torque, count, rows)}, each output asked for
    alone giving the same bits on the way"""
    out = {}
    for local, include_self in COMBOS:
        a = w.body_contact_wrenches(frames, local=local, include_self=include_self, force=True, torque=True, count=True)
        for name in ("force", "torque", "count"):
            alone = w.body_contact_wrenches(frames, local=local, include_self=include_self, **{k: k == name for k in ("force", "torque", "count")})
            assert sorted(alone) == [name] and np.array_equal(alone[name], a[name]), (local, include_self, name)
        rows = w.contact_observe(frames, threshold=THRESHOLD, local=local, include_self=include_self)
        assert np.array_equal(rows[:, :, 1:4], a["force"])
        out[(local, include_self)] = (a["force"], a["torque"], a["count"], rows)
    return out


@functools.lru_cache(maxsize=None)
def device(name):
    """the population's world after its forty control steps (left open for the tests that go on with it), what it holds and its answers"""
    r = recipe(name)
    gc0, gv0, targets = population_inputs(name)
    w = BatchedWorld(r.model, N)
    r.setup_world(w, N, 0)
    w.add_ground(0.0)
    w.set_state(gc0, gv0)
    zero = np.zeros((N, r.model.nv), np.float32)
    for pt in targets:
        w.set_pd_target(pt, zero)
        w.integrate(workload.SUBSTEPS)
    gc, gv = w.get_state()
    cnt, con = w.get_contacts()
    frames = population_frames(name)
    return dict(w=w, gc=f32(gc), gv=f32(gv), cnt=cnt, con=con, flags=w.get_flags(), frames=frames, got=answers(w, frames), kmax=w.max_contacts(),
                inv_dt=inv_dt_of(w.get_time_step()))


def reference_of(blob, gc, gv, cnt, con, frames, inv_dt):
    """{(local, include_self): [sensor_reference per env]}"""
    return {(local, inc): [sensor_reference(blob, gc[e], gv[e], cnt[e], con[e], frames, inv_dt, local=local, no_self=not inc, threshold=THRESHOLD)
                           for e in range(len(gc))] for local, inc in COMBOS}


@functools.lru_cache(maxsize=None)
def reference(name):
    d = device(name)
    return reference_of(recipe(name).model.blob, d["gc"], d["gv"], d["cnt"], d["con"], d["frames"], d["inv_dt"])


def compare(got, ref, worst=None):
    """the largest error / bar per quantity over every combination, env and frame; counts and flags asserted on the way -> (worst, excluded share)"""
    worst = worst if worst is not None else dict(force=0.0, torque=0.0, normal=0.0, slip=0.0)
    near = total = 0
    for key, refs in ref.items():
        force, torque, count, rows = got[key]
        for e, r in enumerate(refs):
            worst["force"] = max(worst["force"], (np.abs(force[e] - r.force).max(axis=1) / (BAR * (1 + r.s_force.max(axis=1)))).max())
            worst["torque"] = max(worst["torque"], (np.abs(torque[e] - r.torque).max(axis=1) / (BAR * (1 + r.s_torque.max(axis=1)))).max())
            worst["normal"] = max(worst["normal"], (np.abs(rows[e, :, 4] - r.normal) / (BAR * (1 + r.s_normal))).max())
            worst["slip"] = max(worst["slip"], (np.abs(rows[e, :, 5] - r.slip) / (BAR * (1 + r.s_slip))).max())
            assert np.array_equal(count[e], r.count), (key, e)
            clear = np.abs(r.normal - THRESHOLD) > BAR * (1 + r.s_normal)
            assert np.array_equal(rows[e, clear, 0], r.flag[clear]), (key, e)
            assert np.array_equal(rows[e, :, 0], (rows[e, :, 4] > np.float32(THRESHOLD)).astype(np.float32))
            near += int((~clear).sum()); total += clear.size
    return worst, near / total


@pytest.mark.parametrize("name", ["anymal", "atlas"])
def test_parity(built_lib, name):
    """every env, frame and flag combination of the population against the reference; the population is what the module's docstring says it is"""
    d, r = device(name), recipe(name)
    quarter, far = quarters(N)
    cnt, con, kmax, blob = d["cnt"], d["con"], d["kmax"], r.model.blob
    foot_bodies = {int(blob.col_body[s]) for s in r.feet}
    assert kmax == (8 if name == "anymal" else 16) and (cnt[quarter == 0] == 0).all() and (cnt[quarter == 1] > 0).all()
    off_foot = [e for e in np.flatnonzero(quarter == 2) if any(int(b) not in foot_bodies for b in con[e, :min(cnt[e], kmax)]["body"])]
    full = [e for e in range(N) if cnt[e] >= kmax and d["flags"][e] & 1]
    print(f"{name}: contacts per env {cnt.tolist()}; tipped envs with a non-foot body on the ground {len(off_foot)}; envs at count == kmax with the overflow flag {full}")
    assert len(off_foot) >= 4 and len(full) >= 1 and (np.abs(d["gc"][far, 0]) > 40).all()
    epb = min(256 // len(d["frames"]), 12288 // (((kmax * 12) | 1) + 1))
    assert N % epb, (N, epb)      # the last workgroup is partial
    worst, excluded = compare(d["got"], reference(name))
    print(f"{name}: error / bar " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; contact flags not compared (normal force within its bar of the threshold): {100 * excluded:.3f} % of the pairs")
    assert all(v <= 1.0 for v in worst.values()), (name, worst)
    assert excluded < 0.01
    rows = d["got"][(False, True)][3]
    assert rows[quarter == 1][:, :, 0].sum() >= (quarter == 1).sum() and not rows[quarter == 0].any()
    local, world = d["got"][(True, True)], d["got"][(False, True)]
    assert np.array_equal(local[3][:, :, 5], world[3][:, :, 5]) and np.array_equal(local[3][:, :, 4], world[3][:, :, 4]) and not np.array_equal(local[0], world[0])


def test_parity_record(built_lib):
    lines = ["contact sensors, device against the fp64 reference (tests/test_gpu_contact_sensor.py): largest error / bar, bar = 2e-5 (1 + S)",
             f"populations of N = {N}, {STEPS} control steps, four flag combinations, every body origin + the feet + three offset frames"]
    for name in ("anymal", "atlas"):
        worst, excluded = compare(device(name)["got"], reference(name))
        lines.append(f"{name:7s} " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()) + f"  flags not compared {100 * excluded:.3f} % of the pairs")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "contact_sensor_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def test_self_collision_chain_and_fixed_base_arm(built_lib):
    """The KAT file's three-link chain folding its hand onto its torso: the two bodies' forces are opposite, NO_SELF makes both exactly zero, parity.
    A two-link arm on a fixed base resting its hand on the ground: parity, and noise in the base rows of gv changes no bit."""
    from test_oracle_kat import FOLDER
    n = 7
    model = Model(urdf_string=FOLDER)
    w = BatchedWorld(model, n)
    w.set_gravity([0, 0, 0])
    w.set_pd_gains(np.array([0] * 6 + [40.0, 40.0]), np.array([0] * 6 + [2.0, 2.0]))
    w.set_pd_target(np.tile([0, 0, 0, 0, 0, 0, 0, 0.3, 3.1], (n, 1)), np.zeros((n, 8)))
    q0 = np.tile([0, 0, 1.0, 1, 0, 0, 0, 0.0, 2.0], (n, 1)); q0[:, 0] = np.arange(n)
    w.set_state(q0, np.zeros((n, 8)))
    for k in range(100):
        w.integrate(4)
        cnt, con = w.get_contacts()
        if (cnt == 2).all():
            break
    assert (cnt == 2).all() and (con[:, :2]["collision"] & 0x30000).all()
    frames = frames_f32([(0, (0.0, 0.0, 0.0)), (1, (0.0, 0.0, 0.0)), (2, (0.0, 0.0, -0.3)), (2, (0.0, 0.0, 0.0))])
    gc, gv = w.get_state()
    got = answers(w, frames)
    worst, _ = compare(got, reference_of(model.blob, f32(gc), f32(gv), cnt, con, frames, inv_dt_of(w.get_time_step())))
    w.close()
    print("chain: error / bar", worst)
    assert all(v <= 1.0 for v in worst.values())
    force, _, count, rows = got[(False, True)]
    assert np.abs(force[:, 0]).max() > 0.1 and np.allclose(force[:, 0], -force[:, 2], rtol=1e-6, atol=0) and not force[:, 1].any()
    assert count.tolist() == [[1, 0, 1, 1]] * n and np.array_equal(force[:, 2], force[:, 3])
    for local in (False, True):
        f0, t0, c0, r0 = got[(local, False)]
        assert not f0.any() and not t0.any() and not c0.any() and not r0.any()

    arm = Model(urdf_string=ARM_URDF)
    assert arm.blob.fixed_base == 1 and arm.nb == 3
    w = BatchedWorld(arm, n)
    w.add_ground(0.0)
    q0 = np.zeros((n, arm.nq)); q0[:, 3] = 1.0; q0[:, 7] = 0.6 + 0.02 * np.arange(n); q0[:, 8] = 0.3
    w.set_state(q0, np.zeros((n, arm.nv)))
    w.integrate(120)
    cnt, con = w.get_contacts()
    gc, gv = w.get_state()
    assert (cnt == 1).all() and (con[:, 0]["body"] == 2).all()
    frames = frames_f32([(0, (0.0, 0.0, 0.0)), (1, (0.1, 0.0, 0.0)), (2, (0.25, 0.0, 0.0)), (2, (0.0, 0.0, 0.0))])
    got = answers(w, frames)
    worst, _ = compare(got, reference_of(arm.blob, f32(gc), f32(gv), cnt, con, frames, inv_dt_of(w.get_time_step())))
    print("arm: error / bar", worst)
    assert all(v <= 1.0 for v in worst.values()) and got[(False, True)][0][:, 2, 2].min() > 0.5
    noisy = gv.copy(); noisy[:, :6] = np.random.default_rng(1).normal(size=(n, 6))
    w.set_state(None, noisy)
    cnt2, con2 = w.get_contacts()
    assert np.array_equal(cnt2, cnt) and con2.tobytes() == con.tobytes()
    again = answers(w, frames)
    w.close()
    for key in got:
        for a, b in zip(got[key], again[key]):
            assert np.array_equal(a, b), key


@pytest.mark.parametrize("name", ["anymal", "atlas"])
def test_body_wrenches_as_loads_give_the_inverse_dynamics_with_contacts(built_lib, name):
    """the device's own outputs cross-checked: force and torque of every body origin from the new query, fed as loads to rsb_inverse_dynamics,
    against rsb_inverse_dynamics(RSB_DYN_CONTACTS) without loads: tau agrees under that call's bar 2e-5 (1 + S_e), S_e = max(|h| + sum |J^T| |f|)"""
    d, model = device(name), recipe(name).model
    w, blob = d["w"], model.blob
    origins = frames_f32([(i, (0.0, 0.0, 0.0)) for i in range(model.nb)])
    wr = w.body_contact_wrenches(origins, force=True, torque=True)
    a = w.inverse_dynamics(None, loads=(origins, wr["force"], wr["torque"]))["tau"]
    b = w.inverse_dynamics(None, contacts=True)["tau"]
    assert not np.array_equal(b, w.inverse_dynamics(None)["tau"])
    o = Oracle(blob)
    worst = 0.0
    for e in range(N):
        k = kinematics(blob, d["gc"][e])
        mag = np.zeros(model.nv)
        for r in d["con"][e, :min(d["cnt"][e], d["kmax"])]:
            Jl, _ = jacobians(blob, k, int(r["body"]), r["position"].astype(np.float64))
            mag += np.abs(Jl.T) @ np.abs(r["impulse"].astype(np.float64) * d["inv_dt"])
        S = (np.abs(o.nonlinearities(d["gc"][e], d["gv"][e])) + mag).max()
        worst = max(worst, np.abs(a[e].astype(np.float64) - b[e]).max() / (BAR * (1 + S)))
    print(f"{name}: |tau(loads) - tau(contacts)| / bar {worst:.3f}")
    assert worst <= 1.0


def tile(x, n=64):
    return np.tile(np.asarray(x, np.float64), (n, 1))


def test_standing_anymal_feet_carry_its_weight(anymal):
    """test_standing_anymal_carries_its_weight's robot, 1500 sub-steps, rtol 2e-4: the four feet's force_z sum to M g, every contact flag is 1, and the
    feet slip by less than that test's velocity bound (2e-3 on every entry of gv) times the levers the entries act through: the base's linear rate
    itself, its angular rate and three leg joints at less than 0.8 m each"""
    n = 64
    w = BatchedWorld(anymal, n)
    kp = np.zeros(18, np.float32); kd = np.zeros(18, np.float32); kp[6:] = 400.0; kd[6:] = 10.0
    q0 = np.zeros(19); q0[2] = 0.60; q0[3] = 1; q0[7:] = workload.ANYMAL_NOMINAL_JOINTS
    w.set_pd_gains(kp, kd); w.set_pd_target(tile(q0), tile(np.zeros(18))); w.set_state(tile(q0), tile(np.zeros(18)))
    w.integrate(1500)
    b = anymal.blob
    feet = frames_f32([(int(b.col_body[s]), tuple(b.col_pos[s])) for s in anymal.collision_indices("_foot")])
    rows = w.contact_observe(feet, threshold=THRESHOLD)
    force = w.body_contact_wrenches(feet)["force"]
    w.close()
    assert len(feet) == 4 and np.allclose(force[:, :, 2].sum(1), anymal.total_mass() * G, rtol=2e-4) and np.allclose(rows[:, :, 4].sum(1), anymal.total_mass() * G, rtol=2e-4)
    assert (rows[:, :, 0] == 1.0).all() and rows[:, :, 5].max() < 2e-3 * (1 + 4 * 0.8)


def test_sliding_sphere_slips_at_its_speed_and_drags_at_mu(built_lib):
    """test_sliding_friction_decelerates_at_mu_g's sphere: the tangential force is mu times the normal force at rtol 1e-5, and the slip equals the
    speed of the sphere's lowest point in the resident state under the slip bar.  That is |u_x + (omega x d)_x|, d the record's position from the
    centre, and not |u_x|: friction spins the sphere up by 2.5 mu g dt / r = 0.4905 rad/s per step, so after the first step the material point is
    0.04905 m/s slower than the centre (2.93133 against 2.98038 measured) - the definition of column 5, v = v_b + omega_b x (position_c - p_b)."""
    n, r, mu = 64, 0.1, 0.8
    w = BatchedWorld(Model(urdf_string=sphere_urdf(2.0, r)), n)
    w.set_control_mode(1)
    w.set_state(tile([0, 0, r - 1e-5, 1, 0, 0, 0]), tile([3.0, 0, 0, 0, 0, 0]))
    for k in range(10):
        w.integrate(1)
        q, u = w.get_state()
        rows = w.contact_observe([0], threshold=THRESHOLD)[:, 0]
        S = np.linalg.norm(u[:, :3], axis=1) + np.linalg.norm(u[:, 3:], axis=1) * (2 * np.linalg.norm(q[:, :3], axis=1) + r)
        cnt, con = w.get_contacts()
        assert (cnt == 1).all()
        d = con[:, 0]["position"].astype(np.float64) - q[:, :3]
        point = u[:, :3].astype(np.float64) + np.cross(u[:, 3:].astype(np.float64), d)
        assert (np.abs(rows[:, 5] - np.abs(point[:, 0])) <= BAR * (1 + S)).all() and np.abs(point[:, 1]).max() < 1e-6, k
        assert np.allclose(u[:, 0] - point[:, 0], 2.5 * mu * G * 0.0025 * (k + 1), rtol=1e-3)      # the spin's share, r omega_y
        assert np.allclose(np.hypot(rows[:, 1], rows[:, 2]), mu * rows[:, 4], rtol=1e-5) and (rows[:, 0] == 1.0).all() and (rows[:, 1] < 0).all()
        assert np.array_equal(rows[:, 3], rows[:, 4])      # a horizontal plane: the normal force is force_z
    w.close()


def test_free_fall_reads_exactly_zero(anymal):
    n = 7
    w = BatchedWorld(anymal, n)
    gc, gv = workload.anymal_initial_state(n)
    gc[:, 2] += 2.0
    w.set_state(gc, np.random.default_rng(0).normal(size=gv.shape))
    w.integrate(4)
    frames = population_frames("anymal")
    for key, (force, torque, count, rows) in answers(w, frames).items():
        assert not force.any() and not torque.any() and not count.any() and not rows.any(), key
    air = np.full((n, len(frames)), 0.5, np.float32); ct = np.full((n, len(frames)), 0.25, np.float32); td = np.full((n, len(frames)), 7.0, np.float32)
    w.contact_timers(frames, 0.02, air, ct, td)
    w.close()
    assert (air == np.float32(0.5) + np.float32(0.02)).all() and not ct.any() and not td.any()


def test_bit_identity_of_frames_sizes_spaces_and_strides(built_lib):
    """a permutation and a subset of the frames; worlds of 1, 7, 64 and 67 envs; host against device buffers; guard rows around every output;
    a row stride larger than 6 F leaves every other float of a patterned buffer alone"""
    import torch
    name = "anymal"
    d, model = device(name), recipe(name).model
    w, frames, F = d["w"], d["frames"], len(d["frames"])
    force, torque, count, rows = d["got"][(True, False)]
    perm = np.random.default_rng(3).permutation(F)
    sub = perm[:7]
    for idx in (perm, sub):
        fr = [frames[i] for i in idx]
        a = w.body_contact_wrenches(fr, local=True, include_self=False, force=True, torque=True, count=True)
        assert np.array_equal(a["force"], force[:, idx]) and np.array_equal(a["torque"], torque[:, idx]) and np.array_equal(a["count"], count[:, idx])
        assert np.array_equal(w.contact_observe(fr, threshold=THRESHOLD, local=True, include_self=False), rows[:, idx])
    # worlds of other sizes holding the first n envs' state and contact list (written through the raw field pointers) answer with the same bits
    gc, gv = w.get_state()
    dev = torch.device("cuda:0")
    for n in (1, 7, 64):
        w2 = BatchedWorld(model, n)
        recipe(name).setup_world(w2, n, 0)
        w2.set_state(gc[:n], gv[:n])
        for field, src in ((_capi.RSB_F_CONTACTS, d["con"][:n]), (_capi.RSB_F_CONTACT_COUNT, d["cnt"][:n])):
            _copy_to_device(w2, w2.device_ptr(field), np.ascontiguousarray(src).view(np.uint8).reshape(-1))
        a = w2.body_contact_wrenches(frames, local=True, include_self=False, force=True, torque=True, count=True)
        r2 = w2.contact_observe(frames, threshold=THRESHOLD, local=True, include_self=False)
        w2.close()
        assert np.array_equal(a["force"], force[:n]) and np.array_equal(a["torque"], torque[:n]) and np.array_equal(a["count"], count[:n]), n
        assert np.array_equal(r2, rows[:n]), n
    # device buffers with guard rows: one allocation per output, the output in its middle
    guard = 64
    def guarded(numel, dtype):
        t = torch.full((numel + 2 * guard,), 7, dtype=dtype, device=dev)
        return t, t[guard:guard + numel]
    tf, vf = guarded(N * F * 3, torch.float32); tt, vt = guarded(N * F * 3, torch.float32); tc, vc = guarded(N * F, torch.int32)
    w.body_contact_wrenches(frames, local=True, include_self=False, out=dict(force=vf, torque=vt, count=vc))
    tr, vr = guarded(N * F * 6, torch.float32)
    w.contact_observe(frames, threshold=THRESHOLD, local=True, include_self=False, out=vr)
    torch.cuda.synchronize()
    for t, v, want in ((tf, vf, force), (tt, vt, torque), (tc, vc, count), (tr, vr, rows)):
        assert np.array_equal(v.cpu().numpy().reshape(want.shape), want)
        assert (t[:guard] == 7).all() and (t[-guard:] == 7).all()
    # a row stride: host and device, every other float keeps its pattern
    stride = 6 * F + 5
    wide = np.full((N, stride), 7.0, np.float32)
    w.contact_observe(frames, threshold=THRESHOLD, local=True, include_self=False, out=wide, row_stride=stride)
    assert np.array_equal(wide[:, :6 * F].reshape(N, F, 6), rows) and (wide[:, 6 * F:] == 7.0).all()
    obs = torch.full((N, stride + 3), 7.0, dtype=torch.float32, device=dev)
    w.contact_observe(frames, threshold=THRESHOLD, local=True, include_self=False, out=obs[:, 3:], row_stride=stride + 3)
    torch.cuda.synchronize()
    got = obs.cpu().numpy()
    assert np.array_equal(got[:, 3:3 + 6 * F].reshape(N, F, 6), rows) and (got[:, :3] == 7.0).all() and (got[:, 3 + 6 * F:] == 7.0).all()


def _copy_to_device(w, ptr, raw):
    """host bytes -> the device address ptr, through the C-ABI's own copy (rsb_device_copy, kind 0)"""
    import ctypes as C
    from raisimlib_amd._capi import check
    check(w.L.rsb_device_copy(w.handle, C.c_void_p(ptr), raw.ctypes.data_as(C.c_void_p), raw.size, 0), "rsb_device_copy")


def test_queries_between_control_steps_change_nothing_and_a_pipelined_world_answers_alike(built_lib):
    """three control steps deep: a run with the three queries between its steps equals a run without, in state, contact records and flags; a
    pipelined world (joined by the queries) gives the answers of the lock-step one"""
    import torch
    from common import standing_states
    n, K = 64, 3
    r = recipe("anymal")
    model = r.model
    gc0, gv0 = standing_states(n, seed=9)
    dev = torch.device("cuda:0")
    bank = torch.from_numpy(np.stack([r.targets(n, k, 0).astype(np.float32) for k in range(K)])).to(dev)
    g0, v0 = torch.from_numpy(gc0.astype(np.float32)).to(dev), torch.from_numpy(gv0.astype(np.float32)).to(dev)
    feet = np.asarray(r.feet, np.int32)
    frames = population_frames("anymal")
    F = len(frames)
    results = {}
    for mode in ("plain", "queried", "pipelined"):
        w = BatchedWorld(model, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        r.setup_world(w, n, 0)
        w.set_state(gc0, gv0)
        w.set_pd_target(None, np.zeros((n, model.nv), np.float32))
        od = w.obs_dim(len(feet))
        obs = torch.zeros((K, n, od), dtype=torch.float32, device=dev)
        if mode == "pipelined":
            assert w.set_step_pipelining(True) is not False and w.step_pipelining_enabled()
        step = w.control_step_plan(workload.SUBSTEPS, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), n)
        air = torch.zeros((n, F), dtype=torch.float32, device=dev); ct = torch.zeros_like(air); td = torch.zeros_like(air)
        wrench = dict(force=torch.zeros((n, F, 3), dtype=torch.float32, device=dev), torque=torch.zeros((n, F, 3), dtype=torch.float32, device=dev))
        rows = torch.zeros((n, F, 6), dtype=torch.float32, device=dev)
        seen = []
        for k in range(K):
            step(bank[k].data_ptr())
            if mode != "plain":
                w.body_contact_wrenches(frames, out=wrench)
                w.contact_observe(frames, threshold=THRESHOLD, out=rows)
                w.contact_timers(frames, 0.01, air, ct, td)
                seen.append([t.clone() for t in (wrench["force"], wrench["torque"], rows, air, ct, td)])
        gc, gv = w.get_state()
        cnt, con = w.get_contacts()
        results[mode] = (gc, gv, cnt, con.tobytes(), w.get_flags(), [[t.cpu().numpy() for t in s] for s in seen])
        w.close()
    for mode in ("queried", "pipelined"):
        for a, b in zip(results[mode][:5], results["plain"][:5]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, mode
    assert results["plain"][2].sum() > 0
    for sa, sb in zip(results["queried"][5], results["pipelined"][5]):
        for a, b in zip(sa, sb):
            assert np.array_equal(a, b)
    assert np.abs(results["queried"][5][-1][0]).max() > 1.0


def test_timers_follow_the_table_on_a_dropped_robot(anymal):
    """twenty calls interleaved with control steps on robots dropped from a few heights (they land, some bounce back off their feet): bit-identical to
    the float32 replay of the table driven by the device's own contact flags; reset_mask zeroes exactly the masked envs; touchdown is non-zero
    only on the first contact call after a flight and equals the flight time accumulated until then"""
    n, dt = 7, 0.01
    w = BatchedWorld(anymal, n)
    w.set_pd_gains(*workload.anymal_gains())
    gc, gv = workload.anymal_initial_state(n)
    gc[:, 2] += 0.005 + 0.01 * np.arange(n)
    w.set_state(gc, np.zeros_like(gv))
    w.set_pd_target(gc, np.zeros_like(gv))
    b = anymal.blob
    feet = frames_f32([(int(b.col_body[s]), tuple(b.col_pos[s])) for s in anymal.collision_indices("_foot")])
    F = len(feet)
    air = np.zeros((n, F), np.float32); ct = np.zeros((n, F), np.float32); td = np.zeros((n, F), np.float32)
    ra, rc = air.copy(), ct.copy()
    flights = np.zeros((n, F), np.float32)
    landings = 0
    for k in range(20):
        w.integrate(workload.SUBSTEPS)
        contact = w.contact_observe(feet, threshold=THRESHOLD)[:, :, 0] == 1.0
        reset = np.zeros(n, np.uint8)
        if k == 12:
            reset[[1, 4]] = 1
        w.contact_timers(feet, dt, air, ct, td, reset_mask=reset if k % 2 == 0 or k == 12 else None)
        before = ra.copy()
        ra, rc, rt = timers_reference(contact, dt, ra, rc, reset)
        assert np.array_equal(air, ra) and np.array_equal(ct, rc) and np.array_equal(td, rt), k
        if k == 12:
            assert not air[[1, 4]].any() and not ct[[1, 4]].any() and not td[[1, 4]].any()
        first = contact & (before > 0) & ~reset.astype(bool)[:, None]
        assert np.array_equal(td != 0, first) and np.array_equal(td[first], before[first])
        landings += int(first.sum())
    w.close()
    assert landings >= n and ct.max() > 0
    # either timer alone carries the bits of both together
    only_air = np.zeros((n, F), np.float32); only_ct = np.zeros((n, F), np.float32)
    w = BatchedWorld(anymal, n)
    w.set_state(gc, np.zeros_like(gv))
    w.integrate(1)
    both_a, both_c = np.full((n, F), 0.5, np.float32), np.full((n, F), 0.25, np.float32)
    only_air[:] = 0.5; only_ct[:] = 0.25
    w.contact_timers(feet, dt, both_a, both_c)
    w.contact_timers(feet, dt, only_air, None)
    w.contact_timers(feet, dt, None, only_ct)
    w.close()
    assert np.array_equal(only_air, both_a) and np.array_equal(only_ct, both_c)


def test_bad_input_fails_loudly_and_touches_nothing(anymal):
    import ctypes as C
    w = BatchedWorld(anymal, 3)
    L, h = w.L, w.handle
    fr, n = w._frames([0, 1])
    buf = (C.c_float * 256)(*([7.0] * 256))
    bad_body, _ = w._frames([anymal.nb])
    bad_off, _ = w._frames([(0, (float("nan"), 0.0, 0.0))])
    calls = [
        (lambda: L.rsb_get_body_contact_wrenches(h, fr, n, 0, buf, buf, buf, 2), "space"),
        (lambda: L.rsb_get_body_contact_wrenches(h, fr, n, 0, None, None, None, 0), "every output is NULL"),
        (lambda: L.rsb_get_body_contact_wrenches(h, fr, 0, 0, buf, None, None, 0), "n_frames"),
        (lambda: L.rsb_get_body_contact_wrenches(h, fr, 65, 0, buf, None, None, 0), "n_frames"),
        (lambda: L.rsb_get_body_contact_wrenches(h, bad_body, 1, 0, buf, None, None, 0), "body"),
        (lambda: L.rsb_get_body_contact_wrenches(h, bad_off, 1, 0, buf, None, None, 0), "offset"),
        (lambda: L.rsb_get_body_contact_wrenches(h, fr, n, 4, buf, None, None, 0), "unknown flag bits"),
        (lambda: L.rsb_contact_observe(h, fr, n, 8, 1.0, buf, 0, 0), "unknown flag bits"),
        (lambda: L.rsb_contact_observe(h, fr, n, 0, -1.0, buf, 0, 0), "force_threshold"),
        (lambda: L.rsb_contact_observe(h, fr, n, 0, float("inf"), buf, 0, 0), "force_threshold"),
        (lambda: L.rsb_contact_observe(h, fr, n, 0, float("nan"), buf, 0, 0), "force_threshold"),
        (lambda: L.rsb_contact_observe(h, fr, n, 0, 1.0, None, 0, 0), "out"),
        (lambda: L.rsb_contact_observe(h, fr, n, 0, 1.0, buf, 6 * n - 1, 0), "row_stride"),
        (lambda: L.rsb_contact_timers(h, fr, n, 0, 1.0, 0.0, None, buf, buf, buf, 0), "dt"),
        (lambda: L.rsb_contact_timers(h, fr, n, 0, 1.0, float("inf"), None, buf, buf, buf, 0), "dt"),
        (lambda: L.rsb_contact_timers(h, fr, n, 0, -0.5, 0.02, None, buf, buf, buf, 0), "force_threshold"),
        (lambda: L.rsb_contact_timers(h, fr, n, 0, 1.0, 0.02, None, None, None, buf, 0), "both NULL"),
        (lambda: L.rsb_contact_timers(h, fr, n, 16, 1.0, 0.02, None, buf, buf, buf, 0), "unknown flag bits"),
    ]
    for call, what in calls:
        assert call() == -1, what
        msg = L.rsb_last_error().decode()
        assert what in msg and msg.startswith(("rsb_get_body_contact_wrenches: ", "rsb_contact_observe: ", "rsb_contact_timers: ")), (what, msg)
    assert all(x == 7.0 for x in buf)
    w.close()
