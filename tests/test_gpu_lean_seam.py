"""Lean seam (raisimlib_amd/csrc/step_spec.h RSB_LEAN_SEAM): in the open-loop resident code objects of the quadruped, a control step that is not the launch's last leaves
through step_phase_seam_lean.inc - launch constants hoisted in front of the control-step loop, no trip loops, the foot forces handed over by row broadcasts, the
carried registers refilled only behind a reset - instead of the generic epilogue and boundary code.  Pure data movement: every float written must be the bits of
the code it replaces, which stays selectable at compile time (-DRSB_X_NO_LEAN_SEAM through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

Every case is run by two child processes, one per variant (both run all the cases), and the observation block and the done flags of EVERY control step, and what the
world holds after the launch - q, u, the contact records, flags, iteration counts - are compared byte for byte; the warm records have no reader of their own, so a
second launch of two control steps starts from them and is compared as well.  The cases are the smallest worlds in which the seam can go wrong:
  targets8 / targets8_stride0   8 envs, two waves, 6 control steps; a target bank of period 4 entered at slice 3 (the slice index wraps twice); the force slots name
                the feet in a permuted order plus one primitive that never touches; the obs block with a stride per control step, and once more with stride 0
                (every step overwrites the one block)
  targets5 / targets5_stride0   the same with 5 envs - the second wave with one env and three rows of non-env lanes.  A resident launch needs a whole number of
                workgroups (rsb_world.hip: choose_step_class), so these control steps run as six launches of the plain class: the switch must change nothing
  drop8_rows1 / drop8_rowsN     8 envs, six upside down and falling from staggered heights: resets in different control steps (reset row, warm table cleared, done
                set in exactly that step); one reset row for all envs, and a row per env
  inf1          env 1 of 4 starts with an infinite joint velocity: flag 2, and the env is terminated in the first control step
  heightmap     8 envs of the drop population on config 3's height map (the resident code object with the terrain compiled in)
  closed8s / closed8   the two populations (8 standing envs, the drop population) through the resident closed loop with the linear stage (classes | 128: the generic code on both sides)
  atlas         the Atlas-like humanoid, 4 envs, 2 control steps: no seam carry, no lean seam - the switch must change nothing"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["targets8", "targets8_stride0", "targets5", "targets5_stride0", "drop8_rows1", "drop8_rowsN", "inf1", "heightmap", "closed8s", "closed8", "atlas"]

_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, workload
from test_gpu_closed_loop import Loop

K = 6
dev = torch.device("cuda:0")
out = {{}}


def drop_state(n):
    # envs 0, 1 stand; env i >= 2 is upside down, its base spheres (radius 0.1) 1 mm + 20 mm x (i - 2) above the ground, falling at 2 m/s = 20 mm per control step
    gc, gv = workload.anymal_initial_state(n)
    for i in range(2, n):
        gc[i, 2] = 0.1 + 0.001 + 0.020 * (i - 2)
        gc[i, 3:7] = [0.0, 1.0, 0.0, 0.0]
        gv[i, 2] = -2.0
        gv[i, 3:6] = [0.1 * i, -0.05 * i, 0.2]
    return gc, gv


def open_case(name, config, n, steps=K, period=K, first=0, stride=True, slots=None, state=None, rows="N", spec=True, resident=True):
    r = bench.Recipe(config, -1.0)
    w = BatchedWorld(r.model, n)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, n, 0)
    w.set_specialization("compile")
    gc0, gv0 = r.initial_state(n, 0)
    if state is not None:
        w.set_state(*state)
    else:
        w.set_state(gc0, gv0)
    w.set_pd_target(None, np.zeros((n, r.model.nv), np.float32))
    rng = np.random.default_rng(11)
    bank = np.stack([r.targets(n, k, 0) for k in range(period)]).astype(np.float32)
    if config == 2:
        bank[:, :, 7:] += rng.normal(0.0, 0.4, bank[:, :, 7:].shape).astype(np.float32)      # (targets that change at every control step)
    bank = torch.from_numpy(bank).to(dev)
    feet = np.asarray(r.feet, np.int32)
    fidx = feet if slots is None else np.asarray(slots(feet), np.int32)
    od = w.obs_dim(len(fidx))
    reset = (gc0, gv0) if state is None else state      # (a reset env goes on from the case's own start)
    if rows == "1":
        g0 = torch.from_numpy(gc0[:1].astype(np.float32)).to(dev); v0 = torch.from_numpy(gv0[:1].astype(np.float32)).to(dev); nrows = 1
    else:
        g0 = torch.from_numpy(reset[0].astype(np.float32)).to(dev); v0 = torch.from_numpy(reset[1].astype(np.float32)).to(dev); nrows = n
    w.set_step_residency(True)
    assert w.residency_status(0) == resident, name

    def launch(nsteps, k0, tag):
        obs = torch.zeros((nsteps if stride else 1, n, od), dtype=torch.float32, device=dev)
        done = torch.full((nsteps, n), 7, dtype=torch.uint8, device=dev)
        fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), period, obs.data_ptr(), n * od if stride else 0, fidx, feet, g0.data_ptr(), v0.data_ptr(), nrows, done.data_ptr(), n)
        l0 = w.residency_launches()
        fn(nsteps, k0)
        w.synchronize()
        assert w.residency_launches() == l0 + (1 if resident else 0), name
        q, u = w.get_state()
        cnt, con = w.get_contacts()
        con = con.copy()
        con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0      # (slots past an env's count hold what an earlier launch left there)
        p = name + tag
        out[p + ".q"], out[p + ".u"], out[p + ".cnt"], out[p + ".con"] = q, u, cnt, np.frombuffer(con.tobytes(), np.uint8)
        out[p + ".flags"], out[p + ".iters"] = w.get_flags(), w.get_solver_iterations()
        out[p + ".obs"], out[p + ".done"] = obs.cpu().numpy(), done.cpu().numpy()
    launch(steps, first, "")
    launch(2, first + steps, "+2")      # (starts from the warm records the first launch left)
    _, n_spec, n_gen = w.specialization_status()
    assert (n_spec > 0 and n_gen == 0) if spec else True, (name, n_spec, n_gen)
    w.close()


permuted = lambda feet: [feet[2], feet[0], feet[3], feet[1], 0]      # (primitive 0: a base sphere - a standing robot never touches with it)
open_case("targets8", 2, 8, period=4, first=3, slots=permuted)
open_case("targets8_stride0", 2, 8, period=4, first=3, slots=permuted, stride=False)
open_case("targets5", 2, 5, period=4, first=3, slots=permuted, resident=False)
open_case("targets5_stride0", 2, 5, period=4, first=3, slots=permuted, stride=False, resident=False)
open_case("drop8_rows1", 2, 8, state=drop_state(8), rows="1")
open_case("drop8_rowsN", 2, 8, state=drop_state(8), rows="N")
gc, gv = workload.anymal_initial_state(4)
gv[1, 6 + 4] = np.inf
open_case("inf1", 2, 4, state=(gc, gv), rows="1")
gc3, gv3 = bench.Recipe(3, -1.0).initial_state(8, 0)
gd, vd = drop_state(8)
gd[:, :2] = gc3[:, :2]; gd[:2] = gc3[:2]; gd[2:, 2] += gc3[2:, 2] - gc[0, 2]      # (the drop population as far above config 3's terrain as it was above the flat ground)
open_case("heightmap", 3, 8, state=(gd, vd), rows="N")
open_case("atlas", 5, 4, steps=2)


def closed_case(name, n, state):
    lp = Loop(bench.Recipe(2, -1.0).model, n, False, stage="linear")
    lp.env.world.set_specialization("compile")
    lp.env.world.set_step_residency(True)
    assert lp.env.world.residency_status(1)
    lp.env.set_reset_states(*[a.astype(np.float32) for a in state])
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


closed_case("closed8s", 8, workload.anymal_initial_state(8))
closed_case("closed8", 8, drop_state(8))
np.savez({out!r}, **out)
"""


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """both variants' results of every case: two child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("lean_seam")
    procs = {}
    for tag, defs in (("lean", ""), ("generic", "-DRSB_X_NO_LEAN_SEAM")):
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
    # (each variant compiled and ran code objects of its own: flat ground, height map, closed loop, humanoid)
    assert len(res["lean.objects"]) >= 4 and len(res["lean.objects"]) == len(res["generic.objects"]), (res["lean.objects"], res["generic.objects"])
    assert not set(res["lean.objects"]) & set(res["generic.objects"])
    return res


@pytest.mark.parametrize("case", CASES)
def test_lean_seam_equals_the_generic_epilogue_bit_for_bit(variants, case):
    a, b = variants["lean"], variants["generic"]
    keys = sorted(k for k in a.files if k.split(".", 1)[0] in (case, case + "+2"))
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "done", "obs", "flags", "iters"} and keys == sorted(k for k in b.files if k.split(".", 1)[0] in (case, case + "+2"))
    print(case, {k: int((a[k] != b[k]).sum()) for k in keys})      # (entries that differ, per array)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (k, int((a[k] != b[k]).sum()))
    q, u, done, obs = a[case + ".q"], a[case + ".u"], a[case + ".done"], a[case + ".obs"]
    # the case did what it is there for
    if case.startswith("targets"):
        assert q.shape[0] == int(case[7]) and int(a[case + ".cnt"].sum()) > 0 and np.isfinite(obs).all() and not done.any()
        nq, nu = q.shape[1], u.shape[1]
        f = obs[..., nq + nu:].reshape(*obs.shape[:2], 5, 3)
        assert (np.abs(f[..., :4, 2]) > 1.0).any() and not f[..., 4, :].any()      # feet's slots carried forces, the base's never
        if not case.endswith("stride0"):
            assert obs.shape[0] == 6 and all(np.abs(obs[k] - obs[k + 1]).max() > 0 for k in range(5))      # six blocks, each its own control step's
    if case.startswith("drop8") or case == "heightmap":
        assert done.shape[0] == 6 and set(np.unique(done)) <= {0, 1}
        assert (done.sum(axis=1) > 0).sum() >= (3 if case.startswith("drop8") else 1), done.sum(axis=1)      # resets in several control steps of the launch (uneven ground: in one at least)
    if case == "inf1":
        assert done[0].tolist() == [0, 1, 0, 0] and not done[1:].any(), done      # terminated in the first control step, and only there
        assert np.isfinite(q).all() and np.isfinite(u).all() and not np.isfinite(obs[0, 1]).all()      # its observation is the state it ended in
    if case.startswith("closed"):
        assert np.isfinite(obs).all()
