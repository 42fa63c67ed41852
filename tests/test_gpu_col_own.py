"""Own-lane form of the plane's collision test (raisimlib_amd/csrc/step_spec.h RSB_COL_OWN; step_phase_collision.inc): in the quadruped's specialised code objects a
lane tests the collision primitives of ITS body with the pose the down pass left in its registers, takes what it tests from registers pinned at the launch's start,
forms a contact's slot from the ballots of all passes and the table's lower-index lanes.  Every float keeps
its expression and operand order and the contacts keep primitive order, so every result must be the bits of the primitive-order loop it replaces, which stays
selectable at compile time (-DRSB_X_NO_COL_OWN through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

One child process per variant runs 8 and 64 envs (2 and 16 waves) lock-step, pipelined and resident, with self-collision on and off, and records contact counts and
records (impulses), flags, done, sweep counts, gc and gv and the obs blocks after 1 and after 8 control steps; everything is compared byte for byte.  The envs of a wave
are in different cases (population(); the fp64 oracle confirms on the CPU which primitives each of them has down at the start):
  0, 6  only feet down                                       (pass 1, the common wave)
  1, 7  only primitives of pass 1 down, a thigh's lower end among them
  2     on its back, tilted: only the base spheres 1, 2, 3 down - lanes 13, 14, 15, which hold the base's pose beside lane 0
  3     all 20 down: with 8 contact slots the first eight in primitive order and flag bit 0; a world with 16 slots (the 16-slot class: key off) holds sixteen
  4     nothing down
  5     on its back, flat: the four base spheres (lane 0 and lanes 13-15)
The 8-env worlds run with the termination rule and resets (a primitive that is no foot ends the episode: `illegal`), the 64-env worlds and the 16-slot world
without: their first control step's records show the cases.
A four-chain model with a cylinder (rim primitives) reports the key off and runs the same bits under both variants."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import Oracle, f32
from test_up_quads_host import _chains_urdf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {"form": "", "twin": "-DRSB_X_NO_COL_OWN"}
MODES = ("lockstep", "pipelined", "resident")
WORLDS = [(n, mode, selfc) for n in (8, 64) for mode in MODES for selfc in (True, False)]
CASES = [f"{mode}_{n}_{'self' if selfc else 'noself'}" for n, mode, selfc in WORLDS] + ["slots16", "cylinder"]
PASS1 = {5, 7, 9, 11, 13, 15, 17, 19}
# (found on the CPU with the fp64 oracle: random orientations and joint angles, lowered until two primitives touch)
_PASS1_A = [0.0525, 0.0946, 0.9, -0.6846, -0.154, 0.6998, -0.1336, 0.3107, 0.4689, -1.0902, 0.4463, 0.3774, 1.1131, -0.6077, -1.0872, 0.1314, 1.0738, -1.1392, -0.8789]
_PASS1_B = [0.0525, 0.0946, 0.9, -0.2868, -0.8475, 0.3413, -0.2882, -1.367, 1.1941, 1.0074, 1.4659, -0.4929, 0.9507, -0.5593, -0.722, -0.4532, 0.4395, 0.0844, -0.2296]
_BACK_TILTED = [0.023714611999043733, 0.9996875162757026, 0.0, 0.007904870666347912]      # upside down, then 0.05 rad about the diagonal through base spheres 1 and 2
EXPECT = {0: {7, 11, 15, 19}, 1: {9, 19}, 2: {1, 2, 3}, 3: set(range(20)), 4: set(), 5: {0, 1, 2, 3}, 6: {7, 11, 15, 19}, 7: {7, 13}}


def population(n):
    """gc, gv, targets of n envs: env e is in case e % 8 of the module's text (the later groups of eight shifted in x, y and with seeded joint velocities)"""
    from raisimlib_amd import workload
    gc, gv = workload.anymal_initial_state(n)
    rng = np.random.default_rng(3)
    for e in range(n):
        k = e % 8
        if k in (1, 7):
            gc[e] = _PASS1_A if k == 1 else _PASS1_B
            gc[e, 3:7] /= np.linalg.norm(gc[e, 3:7])
        elif k == 2:
            gc[e, 3:7] = _BACK_TILTED; gc[e, 2] = 0.095
        elif k == 5:
            gc[e, 3:7] = [0.0, 1.0, 0.0, 0.0]; gc[e, 2] = 0.095
        else:
            gc[e, 2] = {0: 0.56, 3: -0.1, 4: 1.6, 6: 0.55}[k]
        gc[e, 0:2] += 0.01 * (e // 8)
        if e >= 8:
            gv[e, 6:] = rng.normal(0.0, 0.2, 12)
    return gc, gv, gc.astype(np.float32)


def cylinder_urdf():
    """four chains of two bodies with a cylinder on the base: two rim primitives, which the base's lanes 0 and 9..15 would hold in one pass"""
    return _chains_urdf(4, 2).replace('name="base"><inertial>', 'name="base"><collision><geometry><cylinder radius="0.03" length="0.1"/></geometry></collision><inertial>')


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, Model, workload
from test_gpu_col_own import population, cylinder_urdf, WORLDS

cases = {cases!r}
dev = torch.device("cuda:0")
out = {{}}
r = bench.Recipe(2, -1.0)
K = 8


def masked(w):
    cnt, con = w.get_contacts()
    con = con.copy()
    con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0      # (slots past an env's count hold what an earlier launch left there)
    return cnt.copy(), con


def world_case(name, N, mode, selfc, kmax=8):
    if name not in cases:
        return
    w = BatchedWorld(r.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    if kmax != 8:
        w.set_max_contacts(kmax)
    w.set_self_collision(selfc)
    w.set_specialization("compile")
    gc, gv, pt = population(N)
    w.set_state(gc, gv)
    w.set_pd_target(None, np.zeros((N, r.model.nv), np.float32))
    bank = torch.from_numpy(np.ascontiguousarray(np.repeat(pt[None], K + 1, axis=0))).to(dev)
    feet = np.asarray(r.feet, np.int32)
    od = w.obs_dim(len(feet))
    gr, vr = r.initial_state(N, 0)      # (a reset env goes on from the recipe's start)
    g0 = torch.from_numpy(np.asarray(gr, np.float32)).to(dev); v0 = torch.from_numpy(np.asarray(vr, np.float32)).to(dev)
    if mode == "resident":
        w.set_step_residency(True)
        assert w.residency_status(0), name
    if mode == "pipelined":
        w.set_step_pipelining(True)
    for nsteps, k0, tag in ((1, 0, "@1"), (K - 1, 1, "@8")):
        obs = torch.zeros((nsteps, N, od), dtype=torch.float32, device=dev)
        done = torch.full((nsteps, N), 7, dtype=torch.uint8, device=dev)
        if N == 8 and kmax == 8:      # (the termination rule and resets)
            fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K + 1, obs.data_ptr(), N * od, feet, feet, g0.data_ptr(), v0.data_ptr(), N, done.data_ptr(), N)
        else:
            fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K + 1, obs.data_ptr(), N * od, feet, None, 0, 0, N, done.data_ptr(), N)
        if mode == "lockstep":
            for j in range(nsteps):
                fn(1, k0 + j)
        else:
            fn(nsteps, k0)
        w.synchronize()
        q, u = w.get_state()
        cnt, con = masked(w)
        p = name + tag
        out[p + ".q"], out[p + ".u"], out[p + ".cnt"], out[p + ".con"], out[p + ".collision"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8), con["collision"].copy()
        out[p + ".flags"], out[p + ".iters"] = w.get_flags(), w.get_solver_iterations()
        out[p + ".obs"], out[p + ".done"] = obs.cpu().numpy(), done.cpu().numpy()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    w.close()


for N, mode, selfc in WORLDS:
    world_case(mode + "_" + str(N) + "_" + ("self" if selfc else "noself"), N, mode, selfc)
world_case("slots16", 8, "lockstep", True, kmax=16)

if "cylinder" in cases:
    model = Model(urdf_string=cylinder_urdf())
    assert model.col_own() is None and len(model.up_quads()) == 2      # (both quad forms run at the default eight contact slots: the rim primitives alone turn the key off)
    assert Model(urdf_string=cylinder_urdf().replace("cylinder", "sphere").replace(' length="0.1"', "")).col_own() is not None
    N, nq, nv = 8, model.nq, model.nv
    rng = np.random.default_rng(77)
    gc = np.zeros((N, nq)); gc[:, 2] = rng.uniform(0.0, 0.4, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.5, 0.5, (N, nq - 7))
    gv = rng.normal(size=(N, nv))
    w = BatchedWorld(model, N)
    w.set_specialization("compile")
    w.set_pd_gains(np.zeros(nv, np.float32), np.zeros(nv, np.float32)); w.set_pd_target(gc, np.zeros((N, nv))); w.set_state(gc, gv)
    for j in range(2):
        w.integrate(workload.SUBSTEPS)
    w.synchronize()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
    q, u = w.get_state()
    cnt, con = masked(w)
    out["cylinder.q"], out["cylinder.u"], out["cylinder.cnt"], out["cylinder.con"], out["cylinder.flags"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8), w.get_flags()
    out["cylinder.kmax"] = w.max_contacts()
    w.close()
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """every variant's results: child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("col_own")
    procs = {}
    for tag, defs in VARIANTS.items():
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path, cases=CASES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
    res = {}
    try:
        for tag, (p, path, spec) in procs.items():
            _, err = p.communicate(timeout=900)
            assert p.returncode == 0, (tag, err[-3000:])
            res[tag] = np.load(path)
            res[tag + ".objects"] = sorted(f for f in os.listdir(spec) if f.endswith(".hsaco"))
    finally:      # (a time-out or a failed child: no child stays behind on the card)
        for p, _, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    # (each variant compiled and ran code objects of its own: three classes with and without self-collision, the 16-slot class, the cylinder model's)
    sets = [set(res[t + ".objects"]) for t in VARIANTS]
    assert len(sets[0]) >= 8 and len(sets[0]) == len(sets[1]) and not (sets[0] & sets[1]), [sorted(s) for s in sets]
    return res


def test_the_designed_envs_have_their_primitives_down_at_the_start(anymal):
    """the fp64 oracle's collision detection on the eight designed states (CPU): which primitives touch the plane"""
    o = Oracle(anymal.blob)
    o.p.kmax = 16
    gc, _, _ = population(8)
    for e in range(8):
        _, _, con, _, _ = o.step(f32(gc[e]), np.zeros(anymal.nv))
        ids = {int(c) & 0xffff for c in con["collision"]}
        want = EXPECT[e] if len(EXPECT[e]) <= 16 else set(range(16))      # (the oracle holds sixteen records)
        assert ids == want, (e, sorted(ids))
    own = anymal.col_own()
    assert own is not None and {int(p) for p in own["prim"][1] if p >= 0} == PASS1 and [int(p) for p in own["prim"][0, 13:]] == [1, 2, 3]


def _keys(a, case):
    return sorted(k for k in a.files if k.split(".", 1)[0].split("@")[0] == case)


@pytest.mark.parametrize("case", CASES)
def test_own_lane_collision_test_equals_the_primitive_order_loop_bit_for_bit(variants, case):
    a, b = variants["form"], variants["twin"]
    keys = _keys(a, case)
    assert keys and keys == _keys(b, case), case
    for tag, o in [("twin", b)]:
        print(case, tag, {k: int((a[k] != o[k]).sum()) for k in keys})      # (entries that differ, per array)
        for k in keys:
            assert a[k].tobytes() == o[k].tobytes(), (tag, k, int((a[k] != o[k]).sum()))
    if case == "cylinder":
        assert np.isfinite(a["cylinder.q"]).all() and int(a["cylinder.cnt"].sum()) > 0
        return
    # the case did what it is there for: the first control step's records
    cnt, col, flags, done = a[case + "@1.cnt"], a[case + "@1.collision"], a[case + "@1.flags"], a[case + "@1.done"]
    kmax = 16 if case == "slots16" else 8
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    n = cnt.shape[0]
    print(case, "contacts after the first control step", cnt[:8].tolist(), "flags", flags[:8].tolist(), "done", done[0, :8].tolist())
    if n == 8 and kmax == 8:      # (the termination rule: a primitive that is no foot resets the env, and a reset env reports no contact)
        # (envs 1 and 7 - a thigh's end and a foot down at the start - keep a contact to the control step's end only where self-collision holds their pose)
        assert done[0, [2, 3, 5]].all() and not done[0, [0, 4, 6]].any() and cnt[0] == 4 and cnt[6] == 4 and cnt[4] == 0, (done[0].tolist(), cnt.tolist())
        assert not case.endswith("_self") or done[0].tolist() == [0, 1, 1, 1, 0, 1, 0, 1], done[0].tolist()
        return
    for e in range(3, n, 8):      # all 20 down: the first kmax primitives in order, and the overflow bit
        assert cnt[e] == kmax and [int(c) & 0xffff for c in col[e, :kmax]] == list(range(kmax)) and (flags[e] & 1), (e, cnt[e], col[e].tolist(), flags[e])
    for e in range(n):
        ids = [int(c) & 0xffff for c in col[e, :cnt[e]] if not (int(c) & 0x30000)]
        assert ids == sorted(ids), (e, ids)      # primitive order
    assert cnt[0] == 4 and not (flags[0] & 1) and cnt[4] == 0 and cnt[5] > 0 and all(int(c) & 0xffff in (0, 1, 2, 3) for c in col[5, :cnt[5]])
    assert cnt[2] > 0 and all(int(c) & 0xffff in (0, 1, 2, 3) for c in col[2, :cnt[2]])
    assert case.endswith("noself") or {int(c) & 0xffff for c in col[1, :cnt[1]]} & {5, 9, 13, 17}      # (a thigh's lower end, still down where self-collision holds the pose)
    assert np.isfinite(a[case + "@8.q"][0::8]).all()
