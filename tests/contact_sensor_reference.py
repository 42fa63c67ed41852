"""The fp64 reference of the contact sensors (rsb_get_body_contact_wrenches, rsb_contact_observe, rsb_contact_timers; include/rsb.h): pure numpy.

sensor_reference() takes one env's record list (what get_contacts() returns for it), its state and the model blob, and gives every output of the
three entry points for a list of frames together with, for each, the sum of the absolute values of the terms of the expression AS WRITTEN - the scale
the device's fp32 rounding is measured against (|dev - ref| <= 2e-5 (1 + S), the project's query bar):
    force   S = sum_c |f_c|                                   (per component; LOCAL: |R^T| S)
    torque  S = sum_c (|[position_c]x| + |[p_f]x|) |f_c|      (the record's position is a world-frame fp32 number and position_c - p_f cancels, so
                                                               both products count; LOCAL: |R^T| S)
    normal  S = sum_c sum_k |impulse_ck normal_ck| inv_dt
    slip    S = |v_b| + |omega_b| (|position_c| + |p_b|)      (norms; the largest over the owned records)
Body poses and velocities come from the world-frame recursion of tests/test_dynamics_reference.py (kinematics()).  A record acts as impulse * inv_dt
with inv_dt = float32(1 / dt), the device's own factor, so that the comparison measures the reduction and not the rounding of 1 / dt.

timers_reference() is the table of rsb_contact_timers in float32, one call."""
from types import SimpleNamespace

import numpy as np

from test_dynamics_reference import _skew, kinematics

SELF_MASK = 0x10000 | 0x20000      # RSB_CONTACT_SELF_A | RSB_CONTACT_SELF_B


def inv_dt_of(dt):
    """(float)(1.0 / dt), as the device forms it"""
    return float(np.float32(1.0 / float(dt)))


def make_records(rows):
    """rows of (position, normal, impulse, body, collision) -> a record array in get_contacts()'s dtype"""
    from raisimlib_amd.world import CONTACT_DTYPE
    rec = np.zeros(len(rows), CONTACT_DTYPE)
    for k, (pos, nrm, imp, body, col) in enumerate(rows):
        rec[k]["position"], rec[k]["normal"], rec[k]["impulse"], rec[k]["body"], rec[k]["collision"] = pos, nrm, imp, body, col
    return rec


def sensor_reference(blob, q, u, count, records, frames, inv_dt, local=False, no_self=False, threshold=1.0, kmax=None):
    """one env.  records: its row of get_contacts() (the first min(count, kmax) entries act); frames: (body, offset) pairs.
    -> force, torque [F,3], count [F], normal, slip, flag [F] and s_force, s_torque [F,3], s_normal, s_slip [F]"""
    k = kinematics(blob, np.asarray(q, float), np.asarray(u, float))
    kmax = len(records) if kmax is None else kmax
    n = int(min(max(int(count), 0), kmax))
    F = len(frames)
    r = SimpleNamespace(force=np.zeros((F, 3)), torque=np.zeros((F, 3)), count=np.zeros(F, np.int32), normal=np.zeros(F), slip=np.zeros(F),
                        s_force=np.zeros((F, 3)), s_torque=np.zeros((F, 3)), s_normal=np.zeros(F), s_slip=np.zeros(F))
    touched = {int(b) for b in records["body"][:n]}
    for f, (body, off) in enumerate(frames):
        if body not in touched:
            continue
        R, pb, wb, vb = k.R[body], k.p[body], k.w[body], k.v[body]
        off = np.asarray(off, float)
        pf = pb + R @ off
        s_pf = np.abs(pb) + np.abs(R) @ np.abs(off)
        for c in range(n):
            rec = records[c]
            if int(rec["body"]) != body or (no_self and int(rec["collision"]) & SELF_MASK):
                continue
            pos, nrm, imp = (np.asarray(rec[name], float) for name in ("position", "normal", "impulse"))
            fo = imp * inv_dt
            r.force[f] += fo
            r.s_force[f] += np.abs(fo)
            r.torque[f] += np.cross(pos - pf, fo)
            r.s_torque[f] += np.abs(_skew(np.abs(pos))) @ np.abs(fo) + np.abs(_skew(s_pf)) @ np.abs(fo)
            r.normal[f] += float(imp @ nrm) * inv_dt
            r.s_normal[f] += float(np.abs(imp * nrm).sum()) * inv_dt
            r.count[f] += 1
            v = vb + np.cross(wb, pos - pb)
            t = v - float(v @ nrm) * nrm
            r.slip[f] = max(r.slip[f], float(np.linalg.norm(t)))
            r.s_slip[f] = max(r.s_slip[f], float(np.linalg.norm(vb) + np.linalg.norm(wb) * (np.linalg.norm(pos) + np.linalg.norm(pb))))
        if local:
            r.force[f], r.torque[f] = R.T @ r.force[f], R.T @ r.torque[f]
            r.s_force[f], r.s_torque[f] = np.abs(R.T) @ r.s_force[f], np.abs(R.T) @ r.s_torque[f]
    r.flag = (r.normal > threshold).astype(np.float64)
    return r


def timers_reference(contact, dt, air, ct, reset=None):
    """one call of rsb_contact_timers in float32.  contact [N,F] bool, air / ct [N,F] float32 (either may be None: taken as zeros), reset [N] or None
    -> (air, ct, touchdown), float32"""
    contact = np.asarray(contact, bool)
    dt = np.float32(dt)
    zero = np.zeros(contact.shape, np.float32)
    a_old = zero if air is None else np.asarray(air, np.float32)
    c_old = zero if ct is None else np.asarray(ct, np.float32)
    rs = np.zeros(contact.shape, bool) if reset is None else np.broadcast_to(np.asarray(reset).astype(bool)[:, None], contact.shape)
    td = np.where(contact & ~rs, a_old, zero).astype(np.float32)
    a = np.where(~contact & ~rs, a_old + dt, zero).astype(np.float32)
    c = np.where(contact & ~rs, c_old + dt, zero).astype(np.float32)
    return a, c, td
