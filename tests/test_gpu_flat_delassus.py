"""Flat Delassus form (raisimlib_amd/csrc/step_spec.h RSB_FLAT_DELASSUS; step_phase_delassus.inc): in the quadruped's specialised code objects the pair loop reads
the two columns' rows and three floats of the contact records in one batch, by every lane, takes the shared prefix of the two support chains from a closed form of
the body indices, and drops what a lane without a pair computes into a sink.  Every float keeps its expression and its operand order, so every result must be the
bits of the loop it replaces, which stays selectable at compile time (-DRSB_X_NO_FLAT_DELASSUS through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

The child process, the populations and the comparison are those of tests/test_gpu_flat_setup.py: one child per variant, 8 envs (two waves of four), 20 control steps
and a second launch of 2, through the lock-step, pipelined, resident and closed-loop classes; obs, done, the final state, the contact records, flags and sweep counts
are compared byte for byte.  What each case is here for:
  standing    four feet per env: pairs 10-15 of every env do not exist (clamped lanes, sink stores) - the common wave
  counts      wave 0: envs with 0, 1 and 2 contacts (nc below the wave's ncw: whole envs of clamped lanes) beside a four-contact env with a hip at its limit (a
              limit row's diagonal) and one on its back; wave 1 lies on a side: five to eight contacts - a second and a third trip of the pair loop, self-collision
              entries with their fold, blocks 5-7
  joint_limit the env's only row is a limit row
  inf1        one env with an infinite joint velocity: its wave's other envs are untouched
  heightmap   config 3's class, with resets"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_flat_setup import CASES, MODES, ROOT, SELF_A, _CHILD, _same

pytestmark = pytest.mark.gpu

VARIANTS = {"flat": "", "twin": "-DRSB_X_NO_FLAT_DELASSUS"}


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """both variants' results: two child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("flat_delassus")
    procs = {}
    for tag, defs in VARIANTS.items():
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path, cases=CASES, modes=MODES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
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
    assert not set(res["flat.objects"]) & set(res["twin.objects"])
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_flat_delassus_equals_the_pair_loop_bit_for_bit(variants, case, mode):
    a = variants["flat"]
    keys = _same(a, variants["twin"], case, mode, "twin")
    assert {k.split(":", 1)[1] for k in keys} >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    p = f"{case}.{mode}"
    assert a[p + "+2:obs"].shape[0] in (2, 3)      # (the second launch ran)
    if mode == "closed":
        return
    q, u, done, obs, cnt = a[p + ":q"], a[p + ":u"], a[p + ":done"], a[p + ":obs"], a[p + ":cnt"]
    nq = q.shape[1]
    # the case did what it is there for
    if mode == "lockstep":
        if case == "counts":      # (the contact records of every control step)
            cs, col = a[p + ":cnt_steps"], a[p + ":collision_steps"]
            live = np.arange(col.shape[2])[None, None, :] < cs[:, :, None]
            selfc = int((((col & SELF_A) != 0) & live).any(axis=2).sum())
            print("contacts per control step and env", cs.T.tolist(), "env-steps with a self-collision", selfc)
            wave0, wave1 = cs[:, :4], cs[:, 4:]
            assert set(wave0.ravel().tolist()) >= {0, 1, 2, 4}, set(wave0.ravel().tolist())      # envs with 0, 1 and 2 contacts beside the four feet, in ONE wave
            assert ((wave0.min(axis=1) < 4) & (wave0.max(axis=1) >= 4)).any()                      # ... in the same control step: nc below the wave's ncw
            assert (wave1.max(axis=1) > 5).any() and cs.max() == 8, wave1.max(axis=1).tolist()    # a wave with ncw > 5: later trips of the pair loop, blocks 5-7
            assert selfc > 0                                                                        # ... and self-collision entries with their fold
        return
    if case == "standing":
        assert (cnt == 4).all() and not done.any() and np.isfinite(obs).all()
    if case == "counts":
        assert np.isfinite(obs).all() and np.isfinite(q).all() and np.isfinite(u).all()
        # the limit row (joint-limit rows are no contact records - the epilogue reports contacts only - so the row is shown by what it did): env 0's hip, driven into
        # its limit, was stopped within the first control step, which the effort-clipped actuator alone cannot do
        assert obs[0, 0, nq + 6] < 5.0, obs[0, 0, nq + 6]
        qj = obs[:, :, 7:nq]
        assert int(((qj > a["hi"]) | (qj < a["lo"])).any(axis=2).sum()) > 0
        assert a[p + ":cnt"].tolist() == a[f"{case}.lockstep:cnt"].tolist()      # (the same control steps in another class)
    if case == "joint_limit":
        from test_gpu_flat_contact import LIMITS
        for i, (j, sg) in enumerate(LIMITS):
            assert sg * obs[0, i, nq + 6 + j] < 5.0, (i, obs[0, i, 7 + j], obs[0, i, nq + 6 + j])
    if case == "heightmap":
        assert set(np.unique(done)) <= {0, 1} and (done.sum(axis=1) > 0).sum() >= 1, done.sum(axis=1)      # resets within the launch, beside live envs
    if case == "inf1":
        assert done[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0], done
        assert np.isfinite(q).all() and np.isfinite(u).all() and not np.isfinite(obs[0, 1]).all() and np.isfinite(obs[:, [0, 2, 3]]).all()
