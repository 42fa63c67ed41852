"""Shared helpers for the test-suite (tests/ is one of the three places allowed to use oracle/)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import Oracle  # noqa: E402
from raisimlib_amd import workload  # noqa: E402


def f32(a):
    """Round to float32 and back: the exact inputs the device sees, in fp64 for the oracle."""
    return np.asarray(a, np.float32).astype(np.float64)


SPHERE_URDF = """<?xml version="1.0"?>
<robot name="ball">
  <link name="ball">
    <inertial><origin xyz="0 0 0"/><mass value="{m}"/>
      <inertia ixx="{i}" ixy="0" ixz="0" iyy="{i}" iyz="0" izz="{i}"/></inertial>
    <collision><origin xyz="0 0 0"/><geometry><sphere radius="{r}"/></geometry></collision>
  </link>
</robot>
"""


def sphere_urdf(m=2.0, r=0.1):
    return SPHERE_URDF.format(m=m, r=r, i=0.4 * m * r * r)


PENDULUM_URDF = """<?xml version="1.0"?>
<robot name="pendulum">
  <link name="anchor">
    <inertial><origin xyz="0 0 0"/><mass value="1e9"/>
      <inertia ixx="1e9" ixy="0" ixz="0" iyy="1e9" iyz="0" izz="1e9"/></inertial>
  </link>
  <link name="bob">
    <inertial><origin xyz="0 0 -{l}"/><mass value="{m}"/>
      <inertia ixx="1e-9" ixy="0" ixz="0" iyy="1e-9" iyz="0" izz="1e-9"/></inertial>
  </link>
  <joint name="hinge" type="revolute">
    <origin xyz="0 0 0"/><parent link="anchor"/><child link="bob"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/>
  </joint>
</robot>
"""


def standing_states(n, seed=0, z=(0.46, 0.62), joint_noise=0.25, vel=0.5):
    """Physically plausible ANYmal states near the ground (upright +-0.2 rad, feet touching or about to)."""
    rng = np.random.default_rng(seed)
    gc = np.zeros((n, 19))
    gc[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    gc[:, 2] = rng.uniform(z[0], z[1], n)
    rpy = np.c_[rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-np.pi, np.pi, n)]
    cr, sr, cp, sp, cy, sy = (np.cos(rpy[:, 0] / 2), np.sin(rpy[:, 0] / 2), np.cos(rpy[:, 1] / 2), np.sin(rpy[:, 1] / 2),
                              np.cos(rpy[:, 2] / 2), np.sin(rpy[:, 2] / 2))
    gc[:, 3] = cr * cp * cy + sr * sp * sy
    gc[:, 4] = sr * cp * cy - cr * sp * sy
    gc[:, 5] = cr * sp * cy + sr * cp * sy
    gc[:, 6] = cr * cp * sy - sr * sp * cy
    gc[:, 7:] = workload.ANYMAL_NOMINAL_JOINTS + rng.uniform(-joint_noise, joint_noise, (n, 12))
    gv = rng.normal(size=(n, 18)) * vel
    return gc, gv


def config_add(q0, th, fixed_base=False):
    """q0 (+) th, th in velocity space (base linear, base rotation vector in the world frame, joints); a fixed base stays where it is."""
    q = q0.copy()
    if not fixed_base:
        a, b = th[3:6], q0[3:7]
        ang = np.linalg.norm(a)
        d = np.r_[np.cos(ang / 2), (np.sin(ang / 2) / ang if ang > 1e-12 else 0.5) * a]
        q[:3] += th[:3]
        q[3:7] = np.array([d[0] * b[0] - d[1] * b[1] - d[2] * b[2] - d[3] * b[3], d[0] * b[1] + d[1] * b[0] + d[2] * b[3] - d[3] * b[2],
                           d[0] * b[2] - d[1] * b[3] + d[2] * b[0] + d[3] * b[1], d[0] * b[3] + d[1] * b[2] - d[2] * b[1] + d[3] * b[0]])
        q[3:7] /= np.linalg.norm(q[3:7])
    q[7:] += th[6:]
    return q


def rk4_reference(o, dt, kp, kd, q0, u0, pt, tau_ff=None, pd=True):
    """One RUNGE_KUTTA_4 step without contacts, restated in fp64 numpy over the ORACLE's M(q) and h(q, u): the classical four stages of
    q' = u, u' = M^-1 (tau - h) with tau = feed-forward + explicit PD at the stage's own state (velocity target 0), clipped at the joint's effort
    limit, minus the passive joint damping; the base orientation advanced by Munthe-Kaas stages (dexp^-1 to second order).  A fixed base is
    frozen: its velocity rows count as zero whatever they hold, and the joints answer through the joint block M[6:, 6:] alone.
    Returns (theta, du): the configuration increment in velocity space (apply with config_add) and the velocity increment."""
    nv, nb, fixed = o.nv, o.nb, bool(o.blob.fixed_base)
    j0 = 6 if fixed else 0
    damping = np.array([o.blob.damping[b] for b in range(1, nb)])
    effort = np.array([o.blob.effort[b] for b in range(1, nb)])

    def accel(q, u):
        tau = np.zeros(nv) if tau_ff is None else np.array(tau_ff, np.float64)
        if pd:
            tau[6:] += kp[6:] * (pt[7:] - q[7:]) + kd[6:] * (0.0 - u[6:])
        tau[6:] = np.where(effort > 0, np.clip(tau[6:], -effort, effort), tau[6:]) - damping * u[6:]
        uq = u.copy()
        uq[:j0] = 0.0
        a = np.zeros(nv)
        a[j0:] = np.linalg.solve(o.mass_matrix(q)[j0:, j0:], (tau - o.nonlinearities(q, uq))[j0:])
        return a

    ks, kv = [], []
    for i, c in enumerate((0.0, 0.5, 0.5, 1.0)):
        th = c * dt * kv[-1] if i else np.zeros(nv)
        q = config_add(q0, th, fixed); u = u0 + (c * dt * ks[-1] if i else 0.0)
        a = accel(q, u)
        v = u.copy()
        v[:j0] = 0.0
        if not fixed:
            t3 = th[3:6]
            v[3:6] = u[3:6] - 0.5 * np.cross(t3, u[3:6]) + np.cross(t3, np.cross(t3, u[3:6])) / 12.0
        ks.append(a); kv.append(v)
    du = dt / 6 * (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3])
    theta = dt / 6 * (kv[0] + 2 * kv[1] + 2 * kv[2] + kv[3])
    return theta, du
