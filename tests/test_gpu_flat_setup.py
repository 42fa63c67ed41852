"""Flat set-up and end of the contact solve (raisimlib_amd/csrc/step_spec.h RSB_FLAT_SETUP): in the quadruped's specialised code objects the solver reads what the
lane index addresses in one batch, what the contact record addresses in a second one, and takes or drops the results by selects; the warm table is cleared by straight
stores; the end reads once and holds one region.  Every float keeps its expression and its operand order, so every result must be the bits of the code it replaces,
which stays selectable at compile time (-DRSB_X_NO_FLAT_SETUP, and per part -DRSB_X_NO_FLAT_SETUP_HEAD / -DRSB_X_NO_FLAT_SETUP_END, through $RSB_SPEC_EXTRA_DEFS,
part of a code object's key).

Every case is run by one child process per variant: 8 envs (two waves of four), 20 control steps with resets where the case has a termination rule, and a second launch
of 2 control steps from the warm records the first one left (the host API does not read the warm table: it is compared through what that launch computes from it).
Every control step's obs block and done flags, the final state, the contact records, flags and sweep counts are compared byte for byte.  Every case runs through the
lock-step (contact records of every control step), pipelined, resident and closed-loop (linear stage) classes.  The cases are the ones in which an empty or clamped
lane or a rare row can go wrong:
  standing    targets at the pose: four feet per env, no lane beyond them (the common wave)
  counts      wave 0 holds an env in the air (no contact: every lane reads a clamped slot), one that lands on one foot of a tilted base (one contact, then two ..), one
              that stands (four, and a hip at its limit: a joint-limit row with an id >= ncol, a cold start from a clamped warm row) and one on its back; wave 1 lies
              on a side with joints anywhere in their range (five to eight contacts: every slot in use, self-collision pairs - mu from SELFT, an inert second entry -
              and joints beyond their limits).  No termination rule
  joint_limit envs in the air with one joint at its limit and moving outwards: the only row of the env is a limit row
  inf1        env 1 starts with an infinite joint velocity: its wave's other envs are untouched
  heightmap   robots dropped upside down on config 3's height map (its class): resets in different control steps, beside live envs"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF_A = 0x10000
COUNTS_SEED = 1      # (picked on the CPU with the fp64 oracle: see counts_population)
MODES = ["lockstep", "pipelined", "resident", "closed"]
CASES = ["standing", "counts", "joint_limit", "inf1", "heightmap"]
PART_CASES = ["counts"]
VARIANTS = {"flat": ("", CASES), "twin": ("-DRSB_X_NO_FLAT_SETUP", CASES), "no_head": ("-DRSB_X_NO_FLAT_SETUP_HEAD", PART_CASES), "no_end": ("-DRSB_X_NO_FLAT_SETUP_END", PART_CASES)}


def counts_population(model, seed=COUNTS_SEED):
    """8 envs: the mixed population of tests/test_gpu_flat_contact.py (env 0 stands with a hip at its limit, env 2 lies on its back, envs 3..7 on a side) with env 1,
    which hangs in the air there, replaced by TWO roles over the 20 control steps: it starts 0.12 m above the standing height, tilted by 0.15 rad of roll and of pitch, and
    falls - no contact for the first control steps, then one foot, then more."""
    from test_gpu_flat_contact import STAND, mixed_population
    gc, gv, pt, lo, hi = mixed_population(model, seed)
    r, p = 0.15, 0.15
    quat = np.array([np.cos(r / 2) * np.cos(p / 2), np.sin(r / 2) * np.cos(p / 2), np.cos(r / 2) * np.sin(p / 2), -np.sin(r / 2) * np.sin(p / 2)])
    gc[1, 2] = STAND + 0.12
    gc[1, 3:7] = quat / np.linalg.norm(quat)
    return gc, gv, pt, lo, hi


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, workload
from test_gpu_closed_loop import Loop
from test_gpu_flat_contact import LIMITS, STAND
from test_gpu_flat_setup import counts_population

K, N = 20, 8
cases, modes = {cases!r}, {modes!r}
dev = torch.device("cuda:0")
out = {{}}
r2 = bench.Recipe(2, -1.0)
cgc, cgv, cpt, lo, hi = counts_population(r2.model)
out["lo"], out["hi"] = lo, hi


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


def open_case(name, mode, config=2, state=None, pt=None, terminate=True):
    r = bench.Recipe(config, -1.0)
    w = BatchedWorld(r.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
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
        bank = np.repeat(np.asarray(pt, np.float32)[None], K + 2, axis=0)
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
        p = name + "." + mode + tag
        if mode == "lockstep":      # one launch per control step: the contact records of every one of them
            cnts, cons = [], []
            for j in range(nsteps):
                fn(1, k0 + j)
                w.synchronize()
                c, cn = masked(w)
                cnts.append(c); cons.append(cn)
            out[p + ":cnt_steps"] = np.stack(cnts); out[p + ":collision_steps"] = np.stack(cons)["collision"]
            out[p + ":con_steps"] = np.frombuffer(np.stack(cons).tobytes(), np.uint8)
        else:
            l0 = w.residency_launches()
            fn(nsteps, k0)
            w.synchronize()
            assert w.residency_launches() == l0 + (1 if mode == "resident" else 0), name
        q, u = w.get_state()
        cnt, con = masked(w)
        out[p + ":q"], out[p + ":u"], out[p + ":cnt"], out[p + ":con"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8)
        out[p + ":flags"], out[p + ":iters"] = w.get_flags(), w.get_solver_iterations()
        out[p + ":obs"], out[p + ":done"] = obs.cpu().numpy(), done.cpu().numpy()
    launch(K, 0, "")
    launch(2, K, "+2")      # (starts from the warm records the first launch left)
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    w.close()


def closed_case(name, config=2, state=None):
    # the vectorised env with the linear stage in the resident launch; its task terminates on a contact that is no foot's and resets to the case's own population
    r = bench.Recipe(config, -1.0)
    lp = Loop(r.model, N, False, stage="linear")
    w = lp.env.world
    if config == 3:
        maps, env_map = r.terrain(N, 0)
        w.add_height_map(128, 128, workload.HEIGHTMAP_SIZE, workload.HEIGHTMAP_SIZE, 0.0, 0.0, maps[0])
    w.set_specialization("compile")
    w.set_step_residency(True)
    assert w.residency_status(1), name
    gc0, gv0 = r.initial_state(N, 0) if state is None else state
    lp.env.set_reset_states(np.asarray(gc0, np.float32), np.asarray(gv0, np.float32))
    lp.env.reset()
    p = name + ".closed"
    for tag, nsteps in (("", K), ("+2", 2)):
        l0 = w.residency_launches()
        ro = lp.rollout_buffers(nsteps)
        lp.run(nsteps, ro)
        w.synchronize()
        f = lp.final()
        assert w.residency_launches() == l0 + 1, name
        out[p + tag + ":q"], out[p + tag + ":u"], out[p + tag + ":cnt"], out[p + tag + ":con"] = f["q"], f["u"], f["cnt"], np.frombuffer(f["con"], np.uint8)
        out[p + tag + ":flags"], out[p + tag + ":iters"] = f["flags"], f["iters"]
        out[p + tag + ":obs"], out[p + tag + ":done"] = ro["ob"].cpu().numpy(), ro["done"].cpu().numpy()
        out[p + tag + ":act"], out[p + tag + ":reward"] = ro["act"].cpu().numpy(), ro["reward"].cpu().numpy()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    lp.close()


def case(name, **kw):
    if name not in cases:
        return
    for mode in modes:
        if mode == "closed":
            closed_case(name, config=kw.get("config", 2), state=kw.get("state"))
        else:
            open_case(name, mode, **kw)


gc, gv = workload.anymal_initial_state(N)
gc[:, 2] = STAND
case("standing", state=(gc, gv), pt=gc.astype(np.float32))      # (targets at the pose: the robots stand still on four feet)
case("counts", state=(cgc, cgv), pt=cpt, terminate=False)
gc, gv = workload.anymal_initial_state(N)
for i, (j, sg) in enumerate(LIMITS):      # (envs 0..3 in the air, one joint each 0.01 rad inside its limit and moving outwards at 30 rad/s; envs 4..7 stand)
    gc[i, 2] = 1.5
    gc[i, 7 + j] = sg * 6.27
    gv[i, 6 + j] = sg * 30.0
case("joint_limit", state=(gc, gv))
gc, gv = workload.anymal_initial_state(N)
gv[1, 6 + 4] = np.inf
case("inf1", state=(gc, gv))
gc0, _ = workload.anymal_initial_state(N)
gc3, gv3 = bench.Recipe(3, -1.0).initial_state(N, 0)
gd, vd = drop_state(N)
gd[:, :2] = gc3[:, :2]; gd[:2] = gc3[:2]; gd[2:, 2] += gc3[2:, 2] - gc0[0, 2]      # (the drop population as far above config 3's terrain as it was above the flat ground)
case("heightmap", config=3, state=(gd, vd))
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """every variant's results: child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("flat_setup")
    procs = {}
    for tag, (defs, cases) in VARIANTS.items():
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path, cases=cases, modes=MODES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
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
    # (each variant compiled and ran code objects of its own: lock-step, pipelined, resident, closed loop, on flat ground and on the height map)
    assert len(res["flat.objects"]) >= 8 and len(res["flat.objects"]) == len(res["twin.objects"]), (res["flat.objects"], res["twin.objects"])
    assert len(res["no_head.objects"]) >= 4 and len(res["no_end.objects"]) >= 4
    sets = [set(res[t + ".objects"]) for t in VARIANTS]
    assert all(not (sets[i] & sets[j]) for i in range(4) for j in range(i))
    return res


def _keys(a, case, mode):
    return sorted(k for k in a.files if k.split(":", 1)[0] in (f"{case}.{mode}", f"{case}.{mode}+2"))


def _same(a, b, case, mode, tag):
    keys = _keys(a, case, mode)
    assert keys and keys == _keys(b, case, mode), (case, mode, tag)
    print(case, mode, tag, {k: int((a[k] != b[k]).sum()) for k in keys})      # (entries that differ, per array)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k, int((a[k] != b[k]).sum()))
    return keys


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_flat_setup_equals_the_chained_reads_bit_for_bit(variants, case, mode):
    a = variants["flat"]
    keys = _same(a, variants["twin"], case, mode, "twin")
    if case in PART_CASES:
        _same(a, variants["no_head"], case, mode, "no_head")
        _same(a, variants["no_end"], case, mode, "no_end")
    names = {k.split(":", 1)[1] for k in keys}
    assert names >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    p = f"{case}.{mode}"
    q, u, done, obs, cnt = a[p + ":q"], a[p + ":u"], a[p + ":done"], a[p + ":obs"], a[p + ":cnt"]
    nq = q.shape[1]
    assert a[p + "+2:obs"].shape[0] in (2, 3)      # (the second launch ran)
    if mode == "closed":      # (the env task's own termination rule and observation: the bit-for-bit comparison is what this class is here for)
        assert obs.shape[0] == 21 and np.isfinite(a[p + ":reward"][:, 0]).all()
        return
    # the case did what it is there for
    if mode == "lockstep":      # (one launch per control step: each wrote row 0 of obs and done - only the contact records of every control step are read here)
        if case == "counts":
            cs, col = a[p + ":cnt_steps"], a[p + ":collision_steps"]
            live = np.arange(col.shape[2])[None, None, :] < cs[:, :, None]
            selfc = int((((col & SELF_A) != 0) & live).any(axis=2).sum())
            print("contacts per control step and env", cs.T.tolist(), "env-steps with a self-collision", selfc)
            wave0 = set(cs[:, :4].ravel().tolist())
            assert wave0 >= {0, 1, 4}, wave0                                                   # an empty env, a single contact, the four feet - in ONE wave
            assert set(cs.ravel().tolist()) >= {0, 1, 4, 5, 8}, set(cs.ravel().tolist())      # ... and five contacts (the exchange's straight part) and every slot in use
            assert selfc > 0
        return
    if case == "standing":
        assert (cnt == 4).all() and not done.any() and np.isfinite(obs).all()
    if case == "counts":
        assert np.isfinite(obs).all() and np.isfinite(q).all() and np.isfinite(u).all()
        qj = obs[:, :, 7:nq]
        limit = int(((qj > a["hi"]) | (qj < a["lo"])).any(axis=2).sum())
        print("env-steps that end with a joint beyond its limit", limit)
        assert limit > 0
        assert obs[0, 0, nq + 6] < 5.0, obs[0, 0, nq + 6]      # (env 0's hip was stopped by its limit's row - the effort-clipped actuator alone cannot within one control step)
        assert a[p + ":cnt"].tolist() == a[f"{case}.lockstep:cnt"].tolist()      # (the same control steps in another class)
    if case == "joint_limit":
        from test_gpu_flat_contact import LIMITS
        for i, (j, sg) in enumerate(LIMITS):
            # the effort-clipped actuator alone (80 N m) cannot stop 30 rad/s within one control step: the limit's row did
            assert sg * obs[0, i, nq + 6 + j] < 5.0, (i, obs[0, i, 7 + j], obs[0, i, nq + 6 + j])
    if case == "heightmap":
        assert set(np.unique(done)) <= {0, 1} and (done.sum(axis=1) > 0).sum() >= 1, done.sum(axis=1)      # resets within the launch, beside live envs
    if case == "inf1":
        assert done[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0], done
        assert np.isfinite(q).all() and np.isfinite(u).all() and not np.isfinite(obs[0, 1]).all() and np.isfinite(obs[:, [0, 2, 3]]).all()
        # (envs 0, 2, 3 share the wave with env 1: compared bit for bit above, and finite)
