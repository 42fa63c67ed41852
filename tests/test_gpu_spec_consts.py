"""The contact solve's scalar settings as constants of the specialised code objects (raisimlib_amd/csrc/step_spec.h: the key fields MU ... MAX_ITER).  Three things can go wrong,
and each is silent wrong physics or a silent loss of speed:

  twin identity    a literal lets the compiler re-form an expression (a reciprocal folded on the host, a product fused where it was rounded): the default code
                   objects must give the bits of their twins compiled with -DRSB_X_NO_SPEC_CONSTS (through $RSB_SPEC_EXTRA_DEFS, part of a code object's key), which read
                   the fields from the kernel arguments as before.  Two child processes, one per variant, each compiling its code objects once into a directory of its
                   own, run every case; q, u, contact records, counts, flags, sweep counts and every control step's obs block and done flags are compared byte for byte.
                     flat64_plain / _pipelined / _resident   ANYmal on flat ground, 64 envs, 12 control steps, PD targets that change at every step, 24 envs upside down
                                                             at staggered heights: they touch, terminate and are reset in different control steps
                     flat8_resident                          8 envs: two env blocks, one resident launch
                     side64                                  the population of tests/test_gpu_solver_handover.py: six and more contacts, self-collisions, joints past a limit
                     atlas32                                 the humanoid, 32 envs, 6 control steps
  key separation   a constant baked in without the key being extended: a world that differs from the benchmark's in ONE of the new fields, with a directory that holds
                   nothing but the manifest's code objects and the default mode (RSB_SPEC_CACHED), must run its ahead-of-time class - and so equal an RSB_SPEC_OFF run byte
                   for byte.  One world per field, 16 envs, two control steps, lock-step and resident.
  setter mid-life  set_default_friction on a live world: specialised, generic, specialised again; the trajectory is the RSB_SPEC_OFF trajectory.
                   The time step is no key field: set_time_step on a live world keeps the class, and the code object must honour the new value.
                   Both trajectories are the RSB_SPEC_OFF trajectories."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from raisimlib_amd import _capi
from test_spec_host import _lines, _name

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN = "-DRSB_X_NO_SPEC_CONSTS"
CASES = ["flat64_plain", "flat64_pipelined", "flat64_resident", "flat8_resident", "side64", "atlas32"]
KEYS = ("q", "u", "cnt", "con", "flags", "iters", "obs", "done")
SELF_A = 0x10000
# one setter call per new field that changes that field alone (the benchmark worlds hold the library's defaults: rsb_world.h)
VARIANTS = {
    "MU": "w.set_default_friction(0.7)",
    "ERP": "w.set_erp(0.2)",
    "ALPHA_INIT": "w.set_contact_solver_param(0.9, 1.0, 1.0, 150, 1e-5)",
    "ALPHA_MIN": "w.set_contact_solver_param(1.0, 0.9, 1.0, 150, 1e-5)",
    "ALPHA_DECAY": "w.set_contact_solver_param(1.0, 1.0, 0.95, 150, 1e-5)",
    "THRESHOLD": "w.set_contact_solver_param(1.0, 1.0, 1.0, 150, 1e-6)",
    "STALL_FACTOR": "w.set_solver_stagnation_exit(4, 0.6)",
    "MAX_ITER": "w.set_contact_solver_param(1.0, 1.0, 1.0, 100, 1e-5)",
}

_HEAD = r"""
import json, os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, workload
from test_gpu_resident import Open

out = {{}}


def drop_state(n, period=12):
    # envs with i % 8 >= 5 hang upside down, base spheres (radius 0.1) 1 mm + 20 mm x (i % period) above the ground, falling at 2 m/s = 20 mm per control step
    gc, gv = workload.anymal_initial_state(n)
    for i in range(n):
        if i % 8 >= 5:
            gc[i, 2] = 0.1 + 0.001 + 0.020 * (i % period)
            gc[i, 3:7] = [0.0, 1.0, 0.0, 0.0]
            gv[i, 2] = -2.0
            gv[i, 3:6] = [0.01 * i, -0.005 * i, 0.2]
    return gc, gv


def noisy_bank(n, period, seed):
    rng = np.random.default_rng(seed)
    bank = np.stack([workload.anymal_targets(n, k) for k in range(period)])
    bank[:, :, 7:] += rng.normal(0.0, 0.4, bank[:, :, 7:].shape)
    return torch.from_numpy(bank.astype(np.float32)).to("cuda:0")


def record(name, o, obs, done):
    f = o.final(False)
    out[name + ".q"], out[name + ".u"], out[name + ".cnt"] = f["q"], f["u"], f["cnt"]
    out[name + ".con"] = np.frombuffer(f["con"], np.uint8)
    out[name + ".flags"], out[name + ".iters"] = f["flags"], f["iters"]
    out[name + ".obs"], out[name + ".done"] = obs.cpu().numpy(), done.cpu().numpy()
    st = o.w.specialization_status()
    o.w.close()
    return st
"""

_TWIN_CHILD = _HEAD + r"""
from test_gpu_solver_handover import side_population, SIDE_SEED, SIDE_N, SIDE_K


def open_case(name, n, steps, resident=False, pipelined=False, config=2):
    o = Open(config, n, resident, pipelined=pipelined, period=steps)
    o.w.set_specialization("compile")
    if config == 2:
        o.bank = noisy_bank(n, steps, 11)
        o.w.set_state(*drop_state(n))
    obs, done = o.run(steps)
    if resident:
        assert o.w.residency_launches() == 1, name
    _, n_spec, n_gen = record(name, o, obs, done)
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)


open_case("flat64_plain", 64, 12)
open_case("flat64_pipelined", 64, 12, pipelined=True)
open_case("flat64_resident", 64, 12, resident=True)
open_case("flat8_resident", 8, 12, resident=True)
open_case("atlas32", 32, 6, config=5)

# the population off the common path (tests/test_gpu_solver_handover.py), without the termination rule: the envs lie on their trunks
r = bench.Recipe(2, -1.0)
gc, gv, pt, lo, hi = side_population(r.model, SIDE_SEED, SIDE_N)
feet = np.asarray(r.feet, np.int32)
bank = torch.from_numpy(pt[None].copy()).to("cuda:0")
w = BatchedWorld(r.model, SIDE_N)
w.set_stream(torch.cuda.current_stream().cuda_stream)
r.setup_world(w, SIDE_N, 0)
w.set_specialization("compile")
w.set_state(gc, gv)
w.set_pd_target(pt, np.zeros((SIDE_N, r.model.nv), np.float32))
od = w.obs_dim(len(feet))
obs = torch.zeros((SIDE_K, SIDE_N, od), dtype=torch.float32, device="cuda:0")
done = torch.full((SIDE_K, SIDE_N), 7, dtype=torch.uint8, device="cuda:0")
cnts, cons = [], []
for j in range(SIDE_K):
    fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), 1, obs[j].data_ptr(), SIDE_N * od, feet, None, 0, 0, SIDE_N, done[j].data_ptr(), SIDE_N)
    fn(1, 0)
    w.synchronize()
    cnt, con = w.get_contacts()
    con = con.copy(); con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0
    cnts.append(cnt.copy()); cons.append(con)
q, u = w.get_state()
_, n_spec, n_gen = w.specialization_status()
assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
cons = np.stack(cons)
out.update({{"side64.q": q, "side64.u": u, "side64.cnt": np.stack(cnts), "side64.con": np.frombuffer(cons.tobytes(), np.uint8), "side64.collision": cons["collision"],
            "side64.flags": w.get_flags(), "side64.iters": w.get_solver_iterations(), "side64.obs": obs.cpu().numpy(), "side64.done": done.cpu().numpy(),
            "side64.lo": lo, "side64.hi": hi}})
w.close()
np.savez({out!r}, **out)
"""

_KEY_CHILD = _HEAD + r"""
VARIANTS = {variants!r}
status = {{}}


def run(name, mode, resident, setter):
    o = Open(2, 16, resident, period=2)
    w = o.w
    w.set_specialization(mode)
    o.bank = noisy_bank(16, 2, 5)
    w.set_state(*drop_state(16, period=2))
    if setter:
        exec(setter, {{"w": w}})
    obs, done = o.run(2)
    if resident:
        assert w.residency_launches() == 1, name
    _, n_spec, n_gen = record(name, o, obs, done)
    status[name] = [n_spec, n_gen]


for resident in (False, True):
    cls = "resident" if resident else "plain"
    run(f"SAME.{{cls}}.cached", "cached", resident, None)      # (the benchmark's settings: the manifest's code object runs)
    for field, setter in VARIANTS.items():
        for mode in ("cached", "off"):
            run(f"{{field}}.{{cls}}.{{mode}}", mode, resident, setter)

# a setter on a live world: the friction coefficient (a key field: the class changes) and the time step (no key field: the code object must read it at every launch)
for tag, setter, values in (("SETTER", "set_default_friction", (0.8, 0.7, 0.8)), ("SETDT", "set_time_step", (workload.DT, 0.002, workload.DT))):
    for mode in ("cached", "off"):
        o = Open(2, 16, False, period=3)
        w = o.w
        w.set_specialization(mode)
        o.bank = noisy_bank(16, 3, 7)
        w.set_state(*drop_state(16, period=2))
        seen, parts = [], []
        for v in values:
            getattr(w, setter)(v)
            obs, done = o.run(1)
            seen.append(list(w.specialization_status()[1:]))
            parts.append((obs.cpu().numpy(), done.cpu().numpy()))
        status[tag + "." + mode] = seen
        name = tag + ".plain." + mode
        f = o.final(False)
        out[name + ".q"], out[name + ".u"], out[name + ".cnt"], out[name + ".con"] = f["q"], f["u"], f["cnt"], np.frombuffer(f["con"], np.uint8)
        out[name + ".flags"], out[name + ".iters"] = f["flags"], f["iters"]
        out[name + ".obs"], out[name + ".done"] = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        w.close()
np.savez({out!r}, **out)
json.dump(status, open({out!r} + ".json", "w"))
"""


def _child(script, env, timeout=600):
    p = subprocess.Popen([sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return p


@pytest.fixture(scope="module")
def twins(built_lib, tmp_path_factory):
    """both variants' results of every case: two child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("spec_consts")
    procs = {}
    for tag, defs in (("consts", ""), ("twin", TWIN)):
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (_child(_TWIN_CHILD.format(root=ROOT, out=path), env), path, spec)
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
    # (plain, pipelined and resident quadruped classes and the humanoid's: each variant compiled and ran four code objects of its own)
    assert len(res["consts.objects"]) == len(res["twin.objects"]) >= 4, (res["consts.objects"], res["twin.objects"])
    assert not set(res["consts.objects"]) & set(res["twin.objects"])
    return res


@pytest.mark.parametrize("case", CASES)
def test_constants_give_the_bits_of_the_kernel_argument_reads(twins, case):
    a, b = twins["consts"], twins["twin"]
    keys = [f"{case}.{k}" for k in KEYS]
    print(case, {k: int((a[k] != b[k]).sum()) for k in keys})      # (entries that differ, per array)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (k, int((a[k] != b[k]).sum()))
    q, u, cnt, done = a[case + ".q"], a[case + ".u"], a[case + ".cnt"], a[case + ".done"]
    assert np.isfinite(q).all() and np.isfinite(u).all() and int(cnt.sum()) > 0 and int(a[case + ".iters"].sum()) > 0
    # the case did what it is there for
    if case.startswith("flat64"):
        assert done.shape == (12, 64) and (done.sum(axis=1) > 0).sum() >= 4, done.sum(axis=1)      # resets in several control steps of the run
        assert len(np.unique(a[case + ".obs"][:, 0, 7:19], axis=0)) == 12                              # (and a joint state that moves with the changing targets)
    if case == "flat8_resident":
        assert done.shape == (12, 8) and done.sum() > 0
    if case == "side64":
        col = a["side64.collision"]
        live = np.arange(col.shape[2])[None, None, :] < cnt[:, :, None]
        nq = q.shape[1]
        qj = a["side64.obs"][:-1, :, 7:nq]
        six, selfc, limit = int((cnt >= 6).sum()), int((((col & SELF_A) != 0) & live).any(axis=2).sum()), int(((qj > a["side64.hi"]) | (qj < a["side64.lo"])).any(axis=2).sum())
        print(f"env-steps with >= 6 contacts {six}, with a self-collision {selfc}, that start with a joint beyond its limit {limit}")
        assert six > 0 and limit > 0, (six, selfc, limit)
    if case == "atlas32":
        assert q.shape[0] == 32 and a[case + ".obs"].shape[0] == 6


@pytest.fixture(scope="module")
def keyed(built_lib, tmp_path_factory):
    """the key-separation and setter runs: one child in the default mode whose code-object directory holds the manifest's objects and nothing else"""
    tmp = tmp_path_factory.mktemp("spec_keys")
    spec = tmp / "spec"
    spec.mkdir()
    src = _capi.lib().rsb_spec_dir().decode()
    for line in _lines():
        rc, n = _name(line)
        assert rc == 0
        shutil.copy(os.path.join(src, n), spec / n)
    env = dict(os.environ, RSB_SPEC_DIR=str(spec))
    for k in ("RSB_SPECIALIZE", "RSB_SPEC_EXTRA_DEFS", "RSB_SPEC_EXTRA_FLAGS", "RSB_SPEC_RECORD"):
        env.pop(k, None)
    path = str(tmp / "keys.npz")
    p = _child(_KEY_CHILD.format(root=ROOT, out=path, variants=VARIANTS), env)
    try:
        _, err = p.communicate(timeout=600)
    finally:
        if p.poll() is None:
            p.kill()
            p.communicate()
    assert p.returncode == 0, err[-3000:]
    assert sorted(os.listdir(spec)) == sorted(_name(l)[1] for l in _lines())      # (nothing was compiled on the way)
    return np.load(path), json.load(open(path + ".json"))


def _same(res, a, b):
    for k in KEYS:
        x, y = res[f"{a}.{k}"], res[f"{b}.{k}"]
        assert x.tobytes() == y.tobytes(), (a, b, k, int((x != y).sum()))


def test_the_benchmark_settings_still_find_the_manifest_objects(keyed):
    _, status = keyed
    for cls in ("plain", "resident"):
        n_spec, n_gen = status[f"SAME.{cls}.cached"]
        assert n_spec > 0 and n_gen == 0, (cls, n_spec, n_gen)


@pytest.mark.parametrize("cls", ["plain", "resident"])
@pytest.mark.parametrize("field", list(VARIANTS))
def test_a_world_with_another_value_runs_the_ahead_of_time_class(keyed, field, cls):
    res, status = keyed
    n_spec, n_gen = status[f"{field}.{cls}.cached"]
    assert n_spec == 0 and n_gen > 0, (field, cls, n_spec, n_gen)
    assert status[f"{field}.{cls}.off"][0] == 0
    _same(res, f"{field}.{cls}.cached", f"{field}.{cls}.off")
    # (whether two control steps of 16 envs can show the other value at all is printed, not asserted: the sweep limit is never reached here)
    print(field, cls, "differs from the benchmark settings' run:", res[f"{field}.{cls}.cached.q"].tobytes() != res[f"SAME.{cls}.cached.q"].tobytes())


def test_a_setter_on_a_live_world_changes_the_class_and_never_the_results(keyed):
    res, status = keyed
    seen = status["SETTER.cached"]      # [specialised, generic] launches after each of the three steps
    assert seen[0][0] > 0 and seen[0][1] == 0, seen
    assert seen[1][0] == seen[0][0] and seen[1][1] > 0, seen
    assert seen[2][0] > seen[1][0] and seen[2][1] == seen[1][1], seen
    assert all(s[0] == 0 for s in status["SETTER.off"])
    _same(res, "SETTER.plain.cached", "SETTER.plain.off")


def test_set_time_step_on_a_live_world_is_read_by_the_code_object(keyed):
    """the time step is no key field: the launches stay specialised, so the code object has to take the new value from its arguments - the trajectory with a
    step at dt = 0.002 in the middle equals the RSB_SPEC_OFF trajectory, and differs from one at the default time step throughout"""
    res, status = keyed
    seen = status["SETDT.cached"]
    assert [s[1] for s in seen] == [0, 0, 0] and seen[0][0] > 0 and seen[2][0] > seen[1][0] > seen[0][0], seen
    _same(res, "SETDT.plain.cached", "SETDT.plain.off")
    assert res["SETDT.plain.cached.q"].tobytes() != res["SETTER.plain.off.q"].tobytes()
