"""Sweep control (raisimlib_amd/csrc/step_spec.h RSB_SWEEP_CONTROL; step_phase_solver.inc, step_slip_pk.h): in the code objects of the packed solve the direction
refresh's rare continuations (energy check, basin check, global search) sit behind one wave-uniform test, and the two loops of the sweep run bottom-tested on scalar
counters.  Neither part touches an arithmetic instruction and a lane that did not ask for a refresh never uses its verdict, so every result must be the bits of the
code it replaces, which stays selectable at compile time (-DRSB_X_NO_SWEEP_CONTROL, and per part -DRSB_X_NO_SWEEP_CONTROL_RARE / -DRSB_X_NO_SWEEP_CONTROL_LOOP,
through $RSB_SPEC_EXTRA_DEFS, part of a code object's key).

The machinery is tests/test_gpu_pk_solve.py's (one child process per variant, each with a code-object directory of its own; its cases and modes: lock-step,
pipelined, resident, closed loop, height map with resets, inf1, sliding, spinning), here with 8 envs = two waves, 20 control steps and a second launch of 2 from
the warm records: every control step's obs block and done flags, the final state, the contact records, flags and sweep counts are compared byte for byte.
Three more cases run lock-step through the profiling twin, whose counters (rsb_debug_wave_sweep_control, per launch and wave) say what the refresh did - a case that
does not run the code proves nothing:
  sliding_ctl, spinning_ctl   the rare test fired and did not fire within one launch; energy checks ran and steps were refused; global searches ran; the basin
                              check ran in its quad form (first sweeps of waves with at most four contacts per env)
  mixed_ctl                   the mixed population: the basin check's serial form (a wave with more than four contacts in an env), more than one pass per sweep
                              (two contacts on one limb), a multi-contact env (three on one limb: three passes per sweep)
and one runs the mixed population resident with max_iter = 2, a code object of its own: an env is left unconverged (flag 4)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_flat_contact as tf
import test_gpu_pk_solve as tp

pytestmark = pytest.mark.gpu

ROOT = tf.ROOT
CTL_CASES = ["sliding_ctl", "spinning_ctl", "mixed_ctl"]
CASES = [*tp.CASES, *CTL_CASES, "maxiter"]
COUNTERS = "-DRSB_X_SWEEP_COUNTERS"      # (compiles the counters into the profiling twins; every other code object compiles the same code with or without it)
VARIANTS = {"form": "", "twin": "-DRSB_X_NO_SWEEP_CONTROL", "no_rare": "-DRSB_X_NO_SWEEP_CONTROL_RARE", "no_loop": "-DRSB_X_NO_SWEEP_CONTROL_LOOP"}
# columns of rsb_debug_wave_sweep_control
NEWTON1, RARE1, RARE2, ENERGY1, ENERGY2, BASIN_QUAD, BASIN_SERIAL, SEARCH1, SEARCH2, NONE1, NONE2, REFUSED = range(12)

_MORE = r"""

def ctl_case(name, gc, gv, pt):
    if name not in cases:
        return
    w = BatchedWorld(r2.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r2.setup_world(w, N, 0)
    w.set_specialization("compile")
    w.set_state(gc, gv)
    w.set_pd_target(pt, np.zeros((N, r2.model.nv), np.float32))
    w.debug_phase_cycles(True, False)
    prof, ctl = [], []
    for j in range(K):
        w.integrate(workload.SUBSTEPS)
        prof.append(w.debug_wave_profile()[:, 2:7])      # sweeps, largest contact count, global searches, Newton blocks, contact solves
        ctl.append(w.debug_wave_sweep_control())
    w.synchronize()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    out[name + ".q"], out[name + ".u"] = w.get_state()
    out[name + ".flags"], out[name + ".iters"], out[name + ".prof"] = w.get_flags(), w.get_solver_iterations(), np.stack(prof)
    out["counters_" + name + ".ctl"] = np.stack(ctl)      # (what ran where differs between the variants by design: not compared)
    w.close()


gc, _ = workload.anymal_initial_state(N)
gc[:, 2] = STAND
_, gv = workload.anymal_initial_state(N)
gv[:, 0] = 1.0 + 0.1 * np.arange(N); gv[:, 1] = 1.0 + 0.1 * np.arange(N)
ctl_case("sliding_ctl", gc, gv, gc.astype(np.float32))
_, gv = workload.anymal_initial_state(N)
gv[:, 5] = 4.0 * (1.0 + 0.1 * np.arange(N))
ctl_case("spinning_ctl", gc, gv, gc.astype(np.float32))
ctl_case("mixed_ctl", mgc, mgv, mpt)
open_case("maxiter", state=(mgc, mgv), pt=mpt, terminate=False, setup=lambda w: w.set_contact_solver_param(1.0, 1.0, 1.0, 2, 1e-5))
"""
_HEAD, _SAVE = tp._CHILD.rsplit("np.savez(", 1)
assert _HEAD.count("K, N = 3, 8") == 1
_CHILD = _HEAD.replace("K, N = 3, 8", "K, N = 20, 8") + _MORE + "np.savez(" + _SAVE


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """every variant's results: child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("sweep_control")
    procs = {}
    for tag, defs in VARIANTS.items():
        spec = tmp / f"spec_{tag}"
        spec.mkdir()
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=(defs + " " + COUNTERS).strip())
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp / f"{tag}.npz")
        procs[tag] = (subprocess.Popen([sys.executable, "-c", _CHILD.format(root=ROOT, out=path, cases=CASES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), path, spec)
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
    # (each variant compiled and ran code objects of its own: lock-step, pipelined, resident, closed loop, height map, profiling twin, max_iter = 2)
    sets = [set(res[t + ".objects"]) for t in VARIANTS]
    assert all(len(s) >= 7 and len(s) == len(sets[0]) for s in sets), [sorted(s) for s in sets]
    assert all(not (sets[i] & sets[j]) for i in range(len(sets)) for j in range(i))
    return res


@pytest.mark.parametrize("case", CASES)
def test_sweep_control_equals_the_code_it_replaces_bit_for_bit(variants, case):
    a = variants["form"]
    for tag in ("twin", "no_rare", "no_loop"):
        keys = tf._same(a, variants[tag], case, tag)
    if case == "dump":
        assert int(a["dump.nc"]) >= 6 and np.abs(a["dump.G"]).sum() > 0 and np.abs(a["dump.lam"]).sum() > 0 and np.isfinite(a["dump.c"]).all()
        return
    if case in CTL_CASES:
        assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "flags", "iters", "prof"}
        prof = a[case + ".prof"]
        sweeps, ncw, newton, solves = prof[:, :, 0], prof[:, :, 1], prof[:, :, 3], prof[:, :, 4]
        assert np.isfinite(a[case + ".q"]).all() and (newton > 0).any()
        for tag in VARIANTS:
            c = variants[tag]["counters_" + case + ".ctl"]
            print(case, tag, "launches x waves summed:", dict(zip(("newton first", "rare first", "rare later", "energy first", "energy later", "basin quad", "basin serial",
                                                                  "search first", "search later", "none first", "none later", "refused"), c.sum(axis=(0, 1)).tolist())),
                  "Newton blocks", int(newton.sum()), "sweeps", int(sweeps.sum()), "solves", int(solves.sum()), "largest contact count", int(ncw.max()))
            fired = c[:, :, RARE1] + c[:, :, RARE2]
            assert (c < 0xffff).all()
            # (the test's verdict is a function of the step alone: the same in every variant, compiled or only counted)
            assert (fired == variants["form"]["counters_" + case + ".ctl"][:, :, RARE1] + variants["form"]["counters_" + case + ".ctl"][:, :, RARE2]).all()
            if case in ("sliding_ctl", "spinning_ctl"):
                assert ((fired > 0) & (fired < newton)).any(), (fired.tolist(), newton.tolist())      # fired and did not fire within one launch of one wave
                assert (c[:, :, SEARCH1] + c[:, :, SEARCH2]).sum() > 0 and c[:, :, BASIN_QUAD].sum() > 0
                both = np.concatenate([variants[tag]["counters_" + k + ".ctl"] for k in ("sliding_ctl", "spinning_ctl")])
                assert (both[:, :, ENERGY1] + both[:, :, ENERGY2]).sum() > 0 and both[:, :, REFUSED].sum() > 0
            if case == "mixed_ctl":
                assert c[:, :, BASIN_SERIAL].sum() > 0 and int(ncw.max()) > 4
                assert (solves > sweeps).any()               # more than one pass per sweep
                assert (solves > 2 * sweeps).any()           # ... and a third in some sub-step: a limb with three contacts, the multi-contact settings' env
            if tag in ("form", "no_loop"):      # (behind the test nothing runs unless it fired)
                assert (c[:, :, ENERGY1] + c[:, :, ENERGY2] <= fired).all() and (c[:, :, NONE1] + c[:, :, NONE2] == newton - fired).all()
        return
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    obs, cnt, done, flags = a[case + ".obs"], a[case + ".cnt"], a[case + ".done"], a[case + ".flags"]
    if case != "mixed_closed":      # (the closed loop's rollout is one launch, with the observation it starts from in front)
        assert obs.shape[0] == 20 and a[case + "+2.obs"].shape[0] == 2
    else:
        assert obs.shape[0] >= 20
    if case == "standing":
        assert (cnt == 4).all() and not done.any() and np.isfinite(obs).all()
    if case.startswith("mixed"):
        assert np.isfinite(obs).all()
    if case == "mixed_lockstep":
        assert int(a[case + ".cnt_steps"].max()) >= 6      # (more than four contacts per env: the serial basin scan, the exchange's tail, several passes per sweep)
    if case == "maxiter":
        assert ((flags & 4) != 0).any() or ((a[case + "+2.flags"] & 4) != 0).any(), (flags.tolist(), a[case + ".iters"].tolist())
    if case in ("reset", "heightmap"):
        assert set(np.unique(done)) <= {0, 1} and done.sum() > 0, done.sum(axis=1)      # resets within the launch
    if case == "inf1":
        assert done[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
        assert not np.isfinite(obs[0, 1]).all() and np.isfinite(obs[:, [0, 2, 3]]).all()      # (envs 0, 2, 3 share the wave with env 1: compared bit for bit above, and finite)
    if case in ("sliding", "spinning"):
        tf._same(a, variants["twin"], case + "_prof", "twin")
        c = a[case + "_prof.counters"]
        assert (c[:, :, 3] > 0).any() and int(c[:, :, 2].sum()) > 0      # Newton blocks and global searches ran
