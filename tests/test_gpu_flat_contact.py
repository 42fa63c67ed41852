"""Flat contact form (raisimlib_amd/csrc/step_spec.h RSB_FLAT_CONTACT): in the quadruped's specialised code objects the contact columns and the impulse scatter that
ends the solve run without an exec-mask region per tree level - a level the contact's body does not have is computed on body 1's row and discarded by selects on the
results, its column entry and its atomic add go to a padding entry of the lane's own contact column.  Every float keeps its expression and its operand order, so every result must
be the bits of the code it replaces, which stays selectable at compile time (-DRSB_X_NO_FLAT_CONTACT, and per part -DRSB_X_NO_FLAT_COLUMNS / -DRSB_X_NO_FLAT_SCATTER,
through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

Every case is run by one child process per variant (8 envs = two workgroups of the resident class, 3 control steps and a second launch of 2 from the warm records) and
every control step's obs block and done flags, the final state, the contact records, flags and sweep counts are compared byte for byte; the part switches run the mixed
population (resident) and the dump.  The cases are the smallest worlds in which the form can go wrong:
  standing        targets at the pose: four feet per env, every contact at level 3 (the common wave)
  mixed_*         env 0 stands (with a hip joint at its limit: a limit row at level 1 - the hips carry no collision primitive), env 1 hangs in the air (no contact at all), env 2 lies on its back (base contacts, level 0), envs 3..7 lie
                  on a side with joints anywhere in their range (thighs, shanks, feet: levels 2, 3; six and more contacts - the column loop's second trip;
                  self-collisions; joints beyond their limits): wave 0 holds contacts of levels 0, 1, 2 and 3 at once.  No termination rule.  Run through the
                  lock-step (contact records of every control step), pipelined, resident and closed-loop (linear stage) classes
  dump            the mixed population through the profiling twin: the dumped contact problem (G, c) and impulses of the env with the most contacts
  joint_limit     envs in the air with one joint at its limit and moving outwards: a limit row from the second sub-step on
  restitution     every primitive with restitution 0.5 above 0.1 m/s, the robots dropped at 1 m/s: the feet bounce
  reset           six envs upside down and falling from staggered heights: reset in different control steps of the launch, beside live ones
  inf1            env 1 starts with an infinite joint velocity: its wave's other envs are untouched
  heightmap       the reset population on config 3's height map"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF_A = 0x10000
MIXED_SEED = 1      # (picked on the CPU: see mixed_population)
STAND = 0.56        # base height at which the nominal pose's feet touch the ground (the benchmark's start is a drop from 0.6)
LIMITS = [(2, 1.0), (5, -1.0), (7, 1.0), (10, -1.0)]

CASES = ["standing", "mixed_lockstep", "mixed_pipelined", "mixed_resident", "mixed_closed", "dump", "joint_limit", "restitution", "reset", "inf1", "heightmap"]
PART_CASES = ["mixed_resident", "dump"]
VARIANTS = {"flat": ("", CASES), "twin": ("-DRSB_X_NO_FLAT_CONTACT", CASES), "no_columns": ("-DRSB_X_NO_FLAT_COLUMNS", PART_CASES), "no_scatter": ("-DRSB_X_NO_FLAT_SCATTER", PART_CASES)}


def mixed_population(model, seed=MIXED_SEED):
    """8 envs: see the module's text.  The hips - the bodies of level 1 - carry no collision primitive, so wave 0's row at level 1 is a joint-limit row: env 0 stands
    with its first hip joint 0.01 rad inside its limit and moving outwards at 30 rad/s (a whole turn away from the nominal angle: the same pose).
    (The seed is one for which the fp64 oracle's run of these envs holds, at the end of the three control steps, contacts of levels 0, 2 and 3 in wave 0, envs with
    six to eight contacts, self-collisions and joints beyond their limits, env 0's hip beyond its limit after the first sub-step, and env 1 never touches.)"""
    from raisimlib_amd import workload
    from test_gpu_solver_handover import side_population
    gc, gv, pt, lo, hi = side_population(model, seed, 8)
    g0, v0 = workload.anymal_initial_state(8)
    for i in (0, 1, 2):
        gc[i], gv[i], pt[i] = g0[i], v0[i], g0[i]
    gc[0, 2] = STAND; gc[0, 7] = 6.27; gv[0, 6] = 30.0
    gc[1, 2] += 1.0
    gc[2, 2] = 0.1 + 0.001; gc[2, 3:7] = [0.0, 1.0, 0.0, 0.0]; gv[2, 2] = -0.5
    return gc.astype(np.float32), gv.astype(np.float32), pt.astype(np.float32), lo, hi


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, workload
from test_gpu_closed_loop import Loop
from test_gpu_flat_contact import mixed_population, LIMITS, STAND

K, N = 3, 8
cases = {cases!r}
dev = torch.device("cuda:0")
out = {{}}
r2 = bench.Recipe(2, -1.0)
mgc, mgv, mpt, lo, hi = mixed_population(r2.model)
out["lo"], out["hi"] = lo, hi
out["level"] = np.array([r2.model.blob.level[i] for i in range(r2.model.blob.nb)], np.int32)


def drop_state(n):
    # envs 0, 1 stand; env i >= 2 is upside down, its base spheres (radius 0.1) 1 mm + 10 mm x (i - 2) above the ground, falling at 2 m/s = 20 mm per control step
    gc, gv = workload.anymal_initial_state(n)
    for i in range(2, n):
        gc[i, 2] = 0.1 + 0.001 + 0.010 * (i - 2)
        gc[i, 3:7] = [0.0, 1.0, 0.0, 0.0]
        gv[i, 2] = -2.0
        gv[i, 3:6] = [0.1 * i, -0.05 * i, 0.2]
    return gc, gv


def masked(w):
    cnt, con = w.get_contacts()
    con = con.copy()
    con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0      # (slots past an env's count hold what an earlier launch left there)
    return cnt.copy(), con


def open_case(name, config=2, mode="resident", state=None, pt=None, terminate=True, setup=None, case=None):
    if (case or name) not in cases:
        return
    r = bench.Recipe(config, -1.0)
    w = BatchedWorld(r.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    if setup:
        setup(w)
    w.set_specialization("compile")
    gc0, gv0 = r.initial_state(N, 0) if state is None else state
    w.set_state(gc0, gv0)
    w.set_pd_target(None, np.zeros((N, r.model.nv), np.float32))
    if pt is None:
        rng = np.random.default_rng(11)
        bank = np.stack([r.targets(N, k, 0) for k in range(K + 2)]).astype(np.float32)
        if config == 2:
            bank[:, :, 7:] += rng.normal(0.0, 0.4, bank[:, :, 7:].shape).astype(np.float32)      # (targets that change at every control step)
    else:
        bank = np.repeat(pt[None], K + 2, axis=0)
    bank = torch.from_numpy(np.ascontiguousarray(bank)).to(dev)
    feet = np.asarray(r.feet, np.int32)
    od = w.obs_dim(len(feet))
    gr, vr = r.initial_state(N, 0)      # (a reset env goes on from the recipe's start)
    g0 = torch.from_numpy(np.asarray(gr, np.float32)).to(dev); v0 = torch.from_numpy(np.asarray(vr, np.float32)).to(dev)
    if mode == "resident":
        w.set_step_residency(True)
        assert w.residency_status(0), name
    if mode == "pipelined":
        assert w.set_step_pipelining(True), name

    def launch(nsteps, k0, tag):
        obs = torch.zeros((nsteps, N, od), dtype=torch.float32, device=dev)
        done = torch.full((nsteps, N), 7, dtype=torch.uint8, device=dev)
        if terminate:
            fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K + 2, obs.data_ptr(), N * od, feet, feet, g0.data_ptr(), v0.data_ptr(), N, done.data_ptr(), N)
        else:
            fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K + 2, obs.data_ptr(), N * od, feet, None, 0, 0, N, done.data_ptr(), N)
        p = name + tag
        if mode == "lockstep":      # one launch per control step: the contact records of every one of them
            cnts, cons = [], []
            for j in range(nsteps):
                fn(1, k0 + j)
                w.synchronize()
                c, cn = masked(w)
                cnts.append(c); cons.append(cn)
            out[p + ".cnt_steps"] = np.stack(cnts); out[p + ".body_steps"] = np.stack(cons)["body"]; out[p + ".collision_steps"] = np.stack(cons)["collision"]
            out[p + ".con_steps"] = np.frombuffer(np.stack(cons).tobytes(), np.uint8)
        else:
            l0 = w.residency_launches()
            fn(nsteps, k0)
            w.synchronize()
            assert w.residency_launches() == l0 + (1 if mode == "resident" else 0), name
        q, u = w.get_state()
        cnt, con = masked(w)
        out[p + ".q"], out[p + ".u"], out[p + ".cnt"], out[p + ".con"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8)
        out[p + ".flags"], out[p + ".iters"] = w.get_flags(), w.get_solver_iterations()
        out[p + ".obs"], out[p + ".done"] = obs.cpu().numpy(), done.cpu().numpy()
    launch(K, 0, "")
    launch(2, K, "+2")      # (starts from the warm records the first launch left)
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    w.close()


gc, gv = workload.anymal_initial_state(N)
gc[:, 2] = STAND
open_case("standing", state=(gc, gv), pt=gc.astype(np.float32))      # (targets at the pose: the robots stand still on four feet)
for mode in ("lockstep", "pipelined", "resident"):
    open_case("mixed_" + mode, mode=mode, state=(mgc, mgv), pt=mpt, terminate=False)

if "mixed_closed" in cases:
    name = "mixed_closed"
    lp = Loop(r2.model, N, False, stage="linear")
    lp.env.world.set_specialization("compile")
    lp.env.world.set_step_residency(True)
    assert lp.env.world.residency_status(1)
    lp.env.set_reset_states(mgc, mgv)
    lp.env.reset()
    ro = lp.rollout_buffers(K)
    lp.run(K, ro)
    lp.env.world.synchronize()
    f = lp.final()
    _, n_spec, n_gen = lp.env.world.specialization_status()
    assert n_spec > 0 and n_gen == 0 and lp.env.world.residency_launches() == 1, (name, n_spec, n_gen)
    out[name + ".q"], out[name + ".u"], out[name + ".cnt"], out[name + ".con"] = f["q"], f["u"], f["cnt"], np.frombuffer(f["con"], np.uint8)
    out[name + ".flags"], out[name + ".iters"] = f["flags"], f["iters"]
    out[name + ".obs"], out[name + ".done"] = ro["ob"].cpu().numpy(), ro["done"].cpu().numpy()
    out[name + ".act"], out[name + ".reward"] = ro["act"].cpu().numpy(), ro["reward"].cpu().numpy()
    lp.close()

if "dump" in cases:
    # the contact problem of the env with the most contacts after K control steps, dumped by the profiling twin (a specialised code object of its own)
    def world():
        w = BatchedWorld(r2.model, N)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        r2.setup_world(w, N, 0)
        w.set_specialization("compile")
        w.set_state(mgc, mgv)
        w.set_pd_target(mpt, np.zeros((N, r2.model.nv), np.float32))
        return w
    w = world()
    for j in range(K):
        w.integrate(workload.SUBSTEPS)
    w.synchronize()
    e = int(np.argmax(w.get_contacts()[0]))
    w.close()
    w = world()
    w.debug_select_env(e)
    for j in range(K):
        w.integrate(workload.SUBSTEPS)
    w.synchronize()
    nc, G, c, lam = w.debug_contact_problem()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
    q, u = w.get_state()
    cnt, con = masked(w)
    w.close()
    out["dump.env"], out["dump.nc"], out["dump.G"], out["dump.c"], out["dump.lam"] = e, nc, G, c, lam
    out["dump.q"], out["dump.u"], out["dump.cnt"], out["dump.con"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8)

gc, gv = workload.anymal_initial_state(N)
for i, (j, sg) in enumerate(LIMITS):      # (envs 0..3 in the air, one joint each 0.01 rad inside its limit and moving outwards at 30 rad/s; envs 4..7 stand)
    gc[i, 2] = 1.5
    gc[i, 7 + j] = sg * 6.27
    gv[i, 6 + j] = sg * 30.0
open_case("joint_limit", state=(gc, gv))

gc, gv = workload.anymal_initial_state(N)
gc[:, 2] = STAND + 0.003; gv[:, 2] = -1.0
ncol = r2.model.ncol
open_case("restitution", state=(gc, gv), pt=gc.astype(np.float32), setup=lambda w: w.set_collision_materials(None, np.full(ncol, 0.5), np.full(ncol, 0.1)))
open_case("inelastic", state=(gc, gv), pt=gc.astype(np.float32), case="restitution")      # (the same drop without the material: what the case is told apart from)

open_case("reset", state=drop_state(N))
gc, gv = workload.anymal_initial_state(N)
gv[1, 6 + 4] = np.inf
open_case("inf1", state=(gc, gv))
gc0, _ = workload.anymal_initial_state(N)
gc3, gv3 = bench.Recipe(3, -1.0).initial_state(N, 0)
gd, vd = drop_state(N)
gd[:, :2] = gc3[:, :2]; gd[:2] = gc3[:2]; gd[2:, 2] += gc3[2:, 2] - gc0[0, 2]      # (the drop population as far above config 3's terrain as it was above the flat ground)
open_case("heightmap", config=3, state=(gd, vd))
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """every variant's results: child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("flat_contact")
    procs = {}
    for tag, (defs, cases) in VARIANTS.items():
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path, cases=cases)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
    res = {}
    try:
        for tag, (p, path, spec) in procs.items():
            _, err = p.communicate(timeout=600)
            assert p.returncode == 0, (tag, err[-3000:])
            res[tag] = np.load(path)
            res[tag + ".objects"] = sorted(f for f in os.listdir(spec) if f.endswith(".hsaco"))
    finally:      # (a time-out or a failed child: no child stays behind on the card)
        for p, _, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    # (each variant compiled and ran code objects of its own: lock-step, pipelined, resident, closed loop, height map, profiling twin)
    assert len(res["flat.objects"]) >= 6 and len(res["flat.objects"]) == len(res["twin.objects"]), (res["flat.objects"], res["twin.objects"])
    assert len(res["no_columns.objects"]) >= 2 and len(res["no_scatter.objects"]) >= 2
    sets = [set(res[t + ".objects"]) for t in VARIANTS]
    assert all(not (sets[i] & sets[j]) for i in range(4) for j in range(i))
    return res


def _keys(a, case):
    return sorted(k for k in a.files if k.split(".", 1)[0] in (case, case + "+2"))


def _same(a, b, case, tag):
    keys = _keys(a, case)
    assert keys and keys == _keys(b, case), (case, tag)
    print(case, tag, {k: int((a[k] != b[k]).sum()) for k in keys})      # (entries that differ, per array)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k, int((a[k] != b[k]).sum()))
    return keys


@pytest.mark.parametrize("case", CASES)
def test_flat_contact_form_equals_the_level_regions_bit_for_bit(variants, case):
    a = variants["flat"]
    keys = _same(a, variants["twin"], case, "twin")
    if case in PART_CASES:
        _same(a, variants["no_columns"], case, "no_columns")
        _same(a, variants["no_scatter"], case, "no_scatter")
    if case == "dump":
        assert int(a["dump.nc"]) >= 6 and np.abs(a["dump.G"]).sum() > 0 and np.abs(a["dump.lam"]).sum() > 0 and np.isfinite(a["dump.c"]).all()
        return
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    q, u, done, obs, cnt = a[case + ".q"], a[case + ".u"], a[case + ".done"], a[case + ".obs"], a[case + ".cnt"]
    nq = q.shape[1]
    # the case did what it is there for
    if case == "standing":
        assert (cnt == 4).all() and not done.any() and np.isfinite(obs).all()
    if case == "mixed_lockstep":
        lev, cs, body, col = a["level"], a[case + ".cnt_steps"], a[case + ".body_steps"], a[case + ".collision_steps"]
        live = np.arange(body.shape[2])[None, None, :] < cs[:, :, None]
        wave0 = [set(lev[body[k, :4][live[k, :4]]].tolist()) for k in range(cs.shape[0])]
        selfc = int((((col & SELF_A) != 0) & live).any(axis=2).sum())
        qj = obs[:, :, 7:nq]
        limit = int(((qj > a["hi"]) | (qj < a["lo"])).any(axis=2).sum())
        print("levels in wave 0 per control step", wave0, "counts", cs.tolist(), "env-steps with a self-collision", selfc, "that end with a joint beyond its limit", limit)
        assert any(s >= {0, 2, 3} for s in wave0), wave0
        assert obs[0, 0, nq + 6] < 5.0, obs[0, 0, nq + 6]      # (level 1: env 0's hip was stopped by its limit's row - the effort-clipped actuator alone cannot within one control step)
        assert (cs >= 6).any() and not cs[:, 1].any() and (cs[:, 0] >= 2).all()
        assert selfc > 0 and limit > 0
        assert np.isfinite(q).all() and np.isfinite(u).all()
    if case.startswith("mixed"):
        assert np.isfinite(obs).all()
        if case == "mixed_closed":      # (the env's task terminates on a contact that is no foot's and resets to the same population: every control step starts from it)
            assert done[:, 2].all() and int(done[:, 3:].sum()) > 0, done
        else:
            assert a[case + ".cnt"].tolist() == a["mixed_lockstep.cnt"].tolist() and int(cnt.max()) >= 6      # (the same control steps in another class)
    if case == "joint_limit":
        for i, (j, sg) in enumerate(LIMITS):
            # the effort-clipped actuator alone (80 N m) cannot stop 30 rad/s within one control step: the limit's row did
            assert sg * obs[0, i, nq + 6 + j] < 5.0, (i, obs[0, i, 7 + j], obs[0, i, nq + 6 + j])
    if case == "restitution":
        _same(a, variants["twin"], "inelastic", "twin")
        vz, vz_plain = obs[0, :, nq + 2], a["inelastic.obs"][0, :, nq + 2]
        print("base vz after the first control step: with restitution", vz.tolist(), "without", vz_plain.tolist())
        assert (vz > vz_plain + 0.01).all()      # the feet left the ground again with half their approach speed (fp64 oracle: the base falls 0.03 m/s slower after this control step)
    if case in ("reset", "heightmap"):
        assert set(np.unique(done)) <= {0, 1} and (done.sum(axis=1) > 0).sum() >= (2 if case == "reset" else 1), done.sum(axis=1)      # resets in several control steps of the launch (uneven ground: in one at least)
    if case == "inf1":
        assert done[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and not done[1:].any(), done
        assert np.isfinite(q).all() and np.isfinite(u).all() and not np.isfinite(obs[0, 1]).all() and np.isfinite(obs[:, [0, 2, 3]]).all()
        # (envs 0, 2, 3 share the wave with env 1: compared bit for bit above, and finite)
