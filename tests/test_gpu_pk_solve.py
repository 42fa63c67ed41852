"""Packed fp32 form of the contact solve (raisimlib_amd/csrc/step_spec.h RSB_PK_SOLVE; step_slip_pk.h): in the quadruped's specialised code objects the sweep loop's
paired expressions (stick impulse, tangential velocity, refresh coefficients, Newton step, rotation, energy check, impulse update) run as v_pk_fma_f32 /
v_pk_mul_f32 / v_pk_add_f32 on register pairs.  The packed instructions round each half as their scalar twins do and the source spells out which products are
fused, so every result must be the bits of the scalar form, which stays selectable at compile time (-DRSB_X_NO_PK_SOLVE through $RSB_SPEC_EXTRA_DEFS, part of a
code object's key).  (The form has one part: no part switches.)

The machinery is tests/test_gpu_flat_contact.py's: one child process per variant (8 envs, 3 control steps and a second launch of 2 from the warm records), every
control step's obs block and done flags, the final state, the contact records, flags and sweep counts compared byte for byte; the dump is G, c and the impulses of
the fullest env through the profiling twin.  Its cases (joint_limit aside), and two that exist for the direction refresh:
  sliding     standing robots with 1 m/s (+ 10 % per env) of base velocity along x and y: every foot slips, the Newton refresh runs in every sweep
  spinning    4 rad/s (+ 10 % per env) of yaw: the slip directions turn between sub-steps - steps above 0.02 rad with their energy check, rejected steps, the
              inherited direction's basin check, the global search
Both also run lock-step through the profiling twin, whose counters (Newton blocks, global searches per wave) must be positive: a case that does not run the code
proves nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_flat_contact as tf

pytestmark = pytest.mark.gpu

ROOT = tf.ROOT
CASES = ["standing", "mixed_lockstep", "mixed_pipelined", "mixed_resident", "mixed_closed", "dump", "restitution", "reset", "inf1", "heightmap", "sliding", "spinning"]
VARIANTS = {"packed": ("", CASES), "scalar": ("-DRSB_X_NO_PK_SOLVE", CASES)}

# the flat-contact child with two more cases in front of its last line (the np.savez)
_MORE = r"""

def refresh_case(name, gv):
    if name not in cases:
        return
    gc, _ = workload.anymal_initial_state(N)
    gc[:, 2] = STAND
    open_case(name, state=(gc, gv), pt=gc.astype(np.float32))
    # the same start lock-step through the profiling twin: its counters say what ran
    w = BatchedWorld(r2.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r2.setup_world(w, N, 0)
    w.set_specialization("compile")
    w.set_state(gc, gv)
    w.set_pd_target(gc.astype(np.float32), np.zeros((N, r2.model.nv), np.float32))
    w.debug_phase_cycles(True, False)
    prof = []
    for j in range(K):
        w.integrate(workload.SUBSTEPS)
        prof.append(w.debug_wave_profile())
    w.synchronize()
    _, n_spec, n_gen = w.specialization_status()
    assert n_spec > 0 and n_gen == 0, (name, n_spec, n_gen)
    out[name + "_prof.q"], out[name + "_prof.u"] = w.get_state()
    out[name + "_prof.flags"], out[name + "_prof.iters"] = w.get_flags(), w.get_solver_iterations()
    out[name + "_prof.counters"] = np.stack(prof)[:, :, 2:7]      # sweeps, largest contact count, global searches, Newton blocks, contact solves - per launch and wave
    w.close()


_, gv = workload.anymal_initial_state(N)
gv[:, 0] = 1.0 + 0.1 * np.arange(N); gv[:, 1] = 1.0 + 0.1 * np.arange(N)
refresh_case("sliding", gv)
_, gv = workload.anymal_initial_state(N)
gv[:, 5] = 4.0 * (1.0 + 0.1 * np.arange(N))
refresh_case("spinning", gv)
"""
_HEAD, _SAVE = tf._CHILD.rsplit("np.savez(", 1)
_CHILD = _HEAD + _MORE + "np.savez(" + _SAVE


@pytest.fixture(scope="module")
def variants(built_lib, tmp_path_factory):
    """every variant's results: child processes side by side, each with a code-object cache of its own"""
    tmp = tmp_path_factory.mktemp("pk_solve")
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
    assert len(res["packed.objects"]) >= 6 and len(res["packed.objects"]) == len(res["scalar.objects"]), (res["packed.objects"], res["scalar.objects"])
    assert not set(res["packed.objects"]) & set(res["scalar.objects"])
    return res


@pytest.mark.parametrize("case", CASES)
def test_packed_solve_equals_the_scalar_form_bit_for_bit(variants, case):
    a = variants["packed"]
    keys = tf._same(a, variants["scalar"], case, "scalar")
    if case == "dump":
        assert int(a["dump.nc"]) >= 6 and np.abs(a["dump.G"]).sum() > 0 and np.abs(a["dump.lam"]).sum() > 0 and np.isfinite(a["dump.c"]).all()
        return
    assert {k.split(".", 1)[1] for k in keys} >= {"q", "u", "con", "cnt", "done", "obs", "flags", "iters"}
    obs, cnt, done = a[case + ".obs"], a[case + ".cnt"], a[case + ".done"]
    if case == "standing":
        assert (cnt == 4).all() and not done.any() and np.isfinite(obs).all()
    if case.startswith("mixed"):
        assert np.isfinite(obs).all()
        if case != "mixed_closed":
            assert int(cnt.max()) >= 6      # (more than four contacts per env: the serial basin scan beside the packed loop, self-collision folds)
    if case in ("sliding", "spinning"):
        tf._same(a, variants["scalar"], case + "_prof", "scalar")
        c = a[case + "_prof.counters"]
        newton, search, sweeps = int(c[:, :, 3].sum()), int(c[:, :, 2].sum()), int(c[:, :, 0].sum())
        print(case, "sweeps", sweeps, "Newton blocks", newton, "global searches", search, "per launch and wave:", c[:, :, 2:4].tolist())
        assert np.isfinite(obs).all() and (cnt >= 1).all()
        assert (c[:, :, 3] > 0).all(), c[:, :, 3]      # the refresh ran in every launch of every wave
        assert search > 0, c[:, :, 2]                  # ... and at least one solve fell back to the global search


def test_packed_slip_helpers_equal_the_scalar_ones_on_random_coefficient_sets(tmp_path):
    """tools/ubench/pk_slip.hip: kc, slip_newton, slip_rotate and slip_E, scalar against packed, 65 536 random sets, zero mismatches"""
    from raisimlib_amd import build as _b
    exe = str(tmp_path / "pk_slip")
    cmd = ["/opt/rocm/bin/hipcc", *[f for f in _b.FLAGS if f not in ("-fPIC", "-Wall", "-Wno-unused-function")], "-I", os.path.join(ROOT, "include"), "-I", _b.CSRC,
           os.path.join(ROOT, "tools", "ubench", "pk_slip.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "total 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-1000:])
    accepted = int(r.stdout.split("accepted Newton steps")[1].split(",")[0])
    large = int(r.stdout.split("steps above 0.02 rad")[1].split()[0])
    assert accepted > 1000 and large > 1000, r.stdout      # (both sides of the energy check ran)
