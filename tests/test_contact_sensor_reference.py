"""tests/contact_sensor_reference.py pinned on the CPU: hand-made record lists on the ANYmal-like model with closed-form answers - one record at the
frame point, two opposite records that cancel, a pure couple, a record on another body, self-collision entries with and without NO_SELF, LOCAL axes,
the slip of a spinning and translating base, a count beyond kmax - and the timer table of rsb_contact_timers on a hand-written sequence."""
import numpy as np

from common import f32
from contact_sensor_reference import inv_dt_of, make_records, sensor_reference, timers_reference
from test_dynamics_reference import kinematics

DT = 0.0025
SELF_A, SELF_B = 0x10000, 0x20000
Z = (0.0, 0.0, 1.0)


def state(anymal, seed=3):
    rng = np.random.default_rng(seed)
    q = np.zeros(anymal.nq)
    q[:3] = (0.3, -0.2, 0.55)
    qq = rng.normal(size=4)
    q[3:7] = qq / np.linalg.norm(qq)
    q[7:] = rng.uniform(-0.6, 0.6, anymal.nq - 7)
    return f32(q), f32(rng.normal(size=anymal.nv))


def frame_point(anymal, q, body, off):
    k = kinematics(anymal.blob, q)
    return k.p[body] + k.R[body] @ np.asarray(off, float), k.R[body]


def test_closed_forms(anymal):
    blob, inv = anymal.blob, inv_dt_of(DT)
    assert inv == 400.0
    q, u = state(anymal)
    body, off = 6, f32((0.02, -0.01, -0.3))
    frames = [(body, off), (0, np.zeros(3))]
    pf, R = frame_point(anymal, q, body, off)
    imp = np.array([0.01, -0.02, 0.05])
    # one record at the frame point
    r = sensor_reference(blob, q, u, 1, make_records([(pf, Z, imp, body, 4)]), frames, inv)
    assert np.allclose(r.force[0], f32(imp) * 400.0, rtol=0, atol=1e-12) and np.abs(r.torque[0]).max() < 1e-5 and r.count.tolist() == [1, 0]
    assert np.isclose(r.normal[0], float(f32(imp)[2]) * 400.0) and r.flag.tolist() == [1.0, 0.0] and not r.force[1].any() and r.slip[1] == 0.0
    assert np.allclose(r.s_force[0], np.abs(f32(imp)) * 400.0)
    # two opposite records cancel; the scale does not
    r = sensor_reference(blob, q, u, 2, make_records([(pf, Z, imp, body, 4), (pf, Z, -imp, body, 5)]), frames, inv)
    assert not r.force[0].any() and not r.torque[0].any() and r.count[0] == 2 and r.normal[0] == 0.0 and r.flag[0] == 0.0
    assert np.allclose(r.s_force[0], 2 * np.abs(f32(imp)) * 400.0) and r.s_torque[0].min() > 0
    # a pure couple: +f at p_f + d, -f at p_f - d
    d = np.array([0.1, 0.0, 0.0])
    recs = make_records([(pf + d, Z, imp, body, 4), (pf - d, Z, -imp, body, 5)])
    r = sensor_reference(blob, q, u, 2, recs, frames, inv)
    lever = (f32(pf + d) - f32(pf - d))      # what the float32 positions hold
    assert np.abs(r.force[0]).max() == 0.0 and np.allclose(r.torque[0], np.cross(lever, f32(imp) * 400.0), atol=1e-9)
    # LOCAL: the same vectors in the axes of the frame's body; the slip and the normal force do not change
    rl = sensor_reference(blob, q, u, 2, recs, frames, inv, local=True)
    assert np.allclose(rl.torque[0], R.T @ r.torque[0]) and rl.slip[0] == r.slip[0] and rl.normal[0] == r.normal[0]
    # a record on another body is not owned; only count entries act; a count beyond kmax is clamped
    r = sensor_reference(blob, q, u, 1, make_records([(pf, Z, imp, body + 1, 4)]), frames, inv)
    assert not r.force.any() and not r.count.any() and not r.slip.any()
    r = sensor_reference(blob, q, u, 1, make_records([(pf, Z, imp, body + 1, 4), (pf, Z, imp, body, 4)]), frames, inv)
    assert not r.force.any()
    r = sensor_reference(blob, q, u, 9, make_records([(pf, Z, imp, body, 4)] * 2), frames, inv)
    assert r.count[0] == 2
    # self-collision entries: both act, each on its own body, unless NO_SELF leaves them out
    recs = make_records([(pf, Z, imp, body, 4 | SELF_A), (pf, (0, 0, -1.0), -imp, 0, 1 | SELF_B), (pf, Z, 2 * imp, body, 7)])
    r = sensor_reference(blob, q, u, 3, recs, frames, inv)
    assert np.allclose(r.force[0], 3 * f32(imp) * 400.0) and np.allclose(r.force[1], -f32(imp) * 400.0) and r.count.tolist() == [2, 1]
    r = sensor_reference(blob, q, u, 3, recs, frames, inv, no_self=True)
    assert np.allclose(r.force[0], 2 * f32(imp) * 400.0) and not r.force[1].any() and r.count.tolist() == [1, 0]


def test_slip_of_a_spinning_sliding_base(anymal):
    """the base translating with v and spinning with omega about z over a horizontal plane: the material point at p_b + d slides with v + omega x d"""
    blob, inv = anymal.blob, inv_dt_of(DT)
    q = np.zeros(anymal.nq); q[:3] = (1.0, 2.0, 0.5); q[3] = 1.0
    u = np.zeros(anymal.nv); u[:3] = (0.3, -0.4, 0.7); u[3:6] = (0.0, 0.0, 2.0)
    d = np.array([0.25, 0.0, -0.5])
    recs = make_records([(q[:3] + d, Z, (0.0, 0.0, 0.01), 0, 0), (q[:3], Z, (0.0, 0.0, 0.01), 0, 1)])
    r = sensor_reference(blob, q, u, 2, recs, [(0, np.zeros(3))], inv)
    want = max(np.hypot(0.3, -0.4 + 2.0 * 0.25), np.hypot(0.3, 0.4))      # v_z leaves with the normal part
    assert np.isclose(r.slip[0], want, rtol=1e-7) and np.isclose(r.normal[0], 8.0, rtol=1e-6)
    assert r.s_slip[0] >= np.linalg.norm(u[:3]) + 2.0 * np.linalg.norm(q[:3])
    # a fixed base does not move, whatever its rows hold
    import copy
    fixed = copy.copy(blob); fixed.fixed_base = 1
    assert sensor_reference(fixed, q, u, 2, recs, [(0, np.zeros(3))], inv).slip[0] == 0.0


def test_timer_table():
    """one foot of one env plus a second env that is reset half way: flight, touchdown, stance, lift-off"""
    dt = np.float32(0.02)
    contact = [True, True, False, False, False, True, True, False]
    air = np.zeros((2, 1), np.float32); ct = np.zeros((2, 1), np.float32)
    seen = []
    for k, c in enumerate(contact):
        reset = np.array([0, 1 if k == 4 else 0], np.uint8)
        air, ct, td = timers_reference(np.array([[c], [c]]), dt, air, ct, reset)
        seen.append((float(air[0, 0]), float(ct[0, 0]), float(td[0, 0]), float(air[1, 0]), float(td[1, 0])))
    one, two, three = float(dt), float(dt + dt), float(np.float32(dt + dt) + dt)
    assert [s[:3] for s in seen] == [(0.0, one, 0.0), (0.0, two, 0.0), (one, 0.0, 0.0), (two, 0.0, 0.0), (three, 0.0, 0.0), (0.0, one, three), (0.0, two, 0.0),
                                     (one, 0.0, 0.0)]
    assert [s[3:] for s in seen][4:6] == [(0.0, 0.0), (0.0, 0.0)]      # the reset env: its flight restarts, its touchdown reports none
    # a missing timer is taken as zero
    a, c, td = timers_reference(np.array([[True]]), dt, None, np.full((1, 1), 0.5, np.float32))
    assert float(c[0, 0]) == float(np.float32(0.5) + dt) and float(td[0, 0]) == 0.0 and float(a[0, 0]) == 0.0
