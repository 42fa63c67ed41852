"""Seam carry (raisimlib_amd/csrc/step_spec.h RSB_SEAM_CARRY): in the specialised code objects that run the quad forms of the tree passes, the base's and the joints'
state crosses the boundary between two sub-steps in registers, and the lane's constants and the actuation's five scalars are fetched in one batch with one wait; the
barrier that closes the update pass stays where it was.  Every float is still the same expression of the same operands, rounded as before, so the results must be the
bits of the code it replaces, which stays selectable at compile time (-DRSB_X_NO_SEAM_CARRY through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

Every case below is run by two child processes, one per variant (both children run all the cases, side by side: one interpreter start and one library load per
variant), and q, u, the contact records (impulses), the done flags and the observation block of every control step are compared byte for byte.  The cases are the
smallest worlds in which a carried register can go stale:
  targets5      5 envs - two waves, the second with one env and three rows of non-env lanes - 6 control steps of 4 sub-steps, noisy PD targets that change at every
                control step (a target frozen for longer than a control step shows here)
  drop8         8 envs, six of them upside down and falling from staggered heights: their base spheres reach the ground in different control steps, the envs are
                reset there and go on from the reset state (registers carried over a reset show here); lock-step launches
  drop8_resident / drop8_pipelined / drop8_closed_loop   the same envs through one resident launch of 6 control steps, through the pipelined class, and through the
                resident closed loop with the linear stage: the seam at a control-step boundary in each class
  early_term    set_early_termination(True), 8 envs upside down 1.0, 3.5, 6.0 ... 18.5 mm above touching and falling at 2 m/s = 5 mm per sub-step: envs 0, 1 die in
                sub-step 1, envs 2, 3 in sub-step 2, 4, 5 in sub-step 3 of the first control step (a dead env's lanes must carry their OLD values)
  joint_limit   envs in the air with one joint 0.01 rad inside its limit and moving outwards at 30 rad/s: it is past the limit after the first sub-step, and the limit's
                row exists from the second sub-step on only if lim_out is formed from the carried q
  trapezoid     set_integration_scheme("trapezoid"): the class in which the velocity that moves the positions is not the stored one
  atlas         the Atlas-like humanoid, 4 envs, 2 control steps: no quad form, no seam carry - the switch must change nothing"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["targets5", "drop8", "drop8_resident", "drop8_pipelined", "drop8_closed_loop", "early_term", "joint_limit", "trapezoid", "atlas"]

_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
from raisimlib_amd import workload
from test_gpu_resident import Open
from test_gpu_closed_loop import Loop

K = 6
out = {{}}


def upside_down(gc, gv, i, clearance, vz=-2.0):
    # base spheres (radius 0.1 at the base's height) `clearance` above the ground, legs in the air
    gc[i, 2] = 0.1 + clearance
    gc[i, 3:7] = [0.0, 1.0, 0.0, 0.0]
    gv[i, 2] = vz


def drop_state(n):
    gc, gv = workload.anymal_initial_state(n)
    for i in range(2, n):      # (envs 0, 1 stand; env i touches after (i - 2) control steps: 20 mm per control step at 2 m/s)
        upside_down(gc, gv, i, 0.001 + 0.020 * (i - 2))
        gv[i, 3:6] = [0.1 * i, -0.05 * i, 0.2]
    return gc, gv


def noisy_bank(n, period, seed):
    rng = np.random.default_rng(seed)
    bank = np.stack([workload.anymal_targets(n, k) for k in range(period)])
    bank[:, :, 7:] += rng.normal(0.0, 0.4, bank[:, :, 7:].shape)
    return torch.from_numpy(bank.astype(np.float32)).to("cuda:0")


def record(name, o, obs, done, spec=True):
    f = o.final(False)
    _, n_spec, n_gen = o.w.specialization_status()
    assert (n_spec > 0 and n_gen == 0) if spec else True, (name, n_spec, n_gen)
    out[name + ".q"], out[name + ".u"], out[name + ".cnt"] = f["q"], f["u"], f["cnt"]
    out[name + ".con"] = np.frombuffer(f["con"], np.uint8)
    out[name + ".flags"] = f["flags"]
    out[name + ".obs"], out[name + ".done"] = obs.cpu().numpy(), done.cpu().numpy()
    o.w.close()


def open_case(name, n, resident=False, pipelined=False, state=None, setup=None, config=2, steps=K):
    o = Open(config, n, resident, pipelined=pipelined, period=K)
    o.w.set_specialization("compile")
    if setup:
        setup(o.w)
    if config == 2:
        o.bank = noisy_bank(n, K, 11)
    if state is not None:
        o.w.set_state(*state)
    obs, done = o.run(steps)
    if resident:
        assert o.w.residency_launches() == 1, name
    record(name, o, obs, done)


open_case("targets5", 5)
open_case("drop8", 8, state=drop_state(8))
open_case("drop8_resident", 8, resident=True, state=drop_state(8))
open_case("drop8_pipelined", 8, pipelined=True, state=drop_state(8))

# the resident closed loop, linear stage: the envs start in - and are reset to - the drop states
import bench
lp = Loop(bench.Recipe(2, -1.0).model, 8, False, stage="linear")
lp.env.world.set_specialization("compile")
lp.env.world.set_step_residency(True)
assert lp.env.world.residency_status(1)
lp.env.set_reset_states(*[a.astype(np.float32) for a in drop_state(8)])
lp.env.reset()
ro = lp.rollout_buffers(K)
lp.run(K, ro)
lp.env.world.synchronize()
f = lp.final()
_, n_spec, n_gen = lp.env.world.specialization_status()
assert n_spec > 0 and n_gen == 0 and lp.env.world.residency_launches() == 1, (n_spec, n_gen)
name = "drop8_closed_loop"
out[name + ".q"], out[name + ".u"], out[name + ".cnt"], out[name + ".con"], out[name + ".flags"] = f["q"], f["u"], f["cnt"], np.frombuffer(f["con"], np.uint8), f["flags"]
out[name + ".obs"], out[name + ".done"] = ro["ob"].cpu().numpy(), ro["done"].cpu().numpy()
out[name + ".act"], out[name + ".reward"] = ro["act"].cpu().numpy(), ro["reward"].cpu().numpy()
lp.close()

gc, gv = workload.anymal_initial_state(8)
for i in range(8):
    upside_down(gc, gv, i, 0.001 + 0.0025 * i)
open_case("early_term", 8, state=(gc, gv), setup=lambda w: w.set_early_termination(True))

gc, gv = workload.anymal_initial_state(8)
for i, (j, sg) in enumerate([(2, 1.0), (5, -1.0), (7, 1.0), (10, -1.0)]):      # (envs 0..3 in the air, one joint each at its limit; envs 4..7 stand)
    gc[i, 2] = 1.5
    gc[i, 7 + j] = sg * 6.27
    gv[i, 6 + j] = sg * 30.0
open_case("joint_limit", 8, state=(gc, gv))

open_case("trapezoid", 8, state=drop_state(8), setup=lambda w: w.set_integration_scheme("trapezoid"))
open_case("atlas", 4, config=5, steps=2)
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """both variants' results of every case: two child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("seam_carry")
    procs = {}
    for tag, defs in (("carry", ""), ("plain", "-DRSB_X_NO_SEAM_CARRY")):
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
    res = {}
    try:
        for tag, (p, path, spec) in procs.items():
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, (tag, err[-3000:])
            res[tag] = np.load(path)
            res[tag + ".objects"] = sorted(f for f in os.listdir(spec) if f.endswith(".hsaco"))
    finally:      # (a time-out or a failed child: neither child stays behind on the card)
        for p, _, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    # (each variant compiled and ran code objects of its own, one per kernel class and switch set of the cases)
    assert len(res["carry.objects"]) >= 7 and len(res["carry.objects"]) == len(res["plain.objects"]), (res["carry.objects"], res["plain.objects"])
    assert not set(res["carry.objects"]) & set(res["plain.objects"])
    return res


@pytest.mark.parametrize("case", CASES)
def test_seam_carry_equals_the_round_trip_through_lds_bit_for_bit(variants, case):
    a, b = variants["carry"], variants["plain"]
    keys = sorted(k for k in a.files if k.startswith(case + "."))
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "done", "obs"} and keys == sorted(k for k in b.files if k.startswith(case + "."))
    print(case, {k.split(".", 1)[1]: int((a[k] != b[k]).sum()) for k in keys})      # (entries that differ, per array)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (k, int((a[k] != b[k]).sum()))
    q, u, done, flags, obs = a[case + ".q"], a[case + ".u"], a[case + ".done"], a[case + ".flags"], a[case + ".obs"]
    assert np.isfinite(q).all() and np.isfinite(u).all()
    # the case did what it is there for
    if case == "targets5":
        assert q.shape[0] == 5 and int(a[case + ".cnt"].sum()) > 0
    if case.startswith("drop8") or case == "trapezoid":
        assert done.shape[0] == 6 and (done.sum(axis=1) > 0).sum() >= 3, done.sum(axis=1)      # resets in several control steps of the run
    if case == "early_term":
        assert done[0, :6].all(), done[0]      # envs 0..5 died inside the first control step, in sub-steps 1, 1, 2, 2, 3, 3
    if case == "joint_limit":
        nq = q.shape[1]
        for i, (j, sg) in enumerate([(2, 1.0), (5, -1.0), (7, 1.0), (10, -1.0)]):
            # the effort-clipped actuator alone (80 N m) cannot stop 30 rad/s within one control step: the limit's row did
            assert sg * obs[0, i, nq + 6 + j] < 5.0, (i, obs[0, i, 7 + j], obs[0, i, nq + 6 + j])
