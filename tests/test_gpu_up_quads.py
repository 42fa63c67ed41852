"""The quad form of the up pass (four lanes per body in the specialised code objects of the quadruped: raisimlib_amd/csrc/step_phase_tree_up.inc, step_spec.h
RSB_UP_QUADS) splits OUTPUTS over the four lanes and never a sum, so it must give the bits of the lane = body loop it replaces.  That loop stays selectable at
compile time (-DRSB_X_NO_UP_QUADS through $RSB_SPEC_EXTRA_DEFS, which is part of a code object's key): the same world is run in two child processes, one per variant,
and everything it holds after 20 control steps is compared byte for byte.  A model outside the quad form's worlds (five bodies on one level) keeps the lane = body loop
in its specialised code object, a model of four chains of two bodies runs the quad form at another tree depth: both are checked against the oracle at the tolerances of
tests/test_gpu_fuzz.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import Oracle, f32
from raisimlib_amd import BatchedWorld, Model
from test_up_quads_host import _chains_urdf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
from test_gpu_resident import Open
o = Open({config}, 1024, {resident})
assert len(o.recipe.model.up_quads()) == 3
o.w.set_specialization("compile")
obs, done = o.run(20)
f = o.final(False)
_, n_spec, n_gen = o.w.specialization_status()
assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
assert o.w.residency_launches() == (1 if {resident} else 0)
_, con = o.w.get_contacts()
np.savez({out!r}, obs=obs.cpu().numpy(), done=done.cpu().numpy(), q=f["q"], u=f["u"], cnt=f["cnt"], con=np.frombuffer(f["con"], np.uint8), flags=f["flags"], iters=f["iters"])
o.w.close()
"""


@pytest.mark.parametrize("config", [2, 3], ids=["flat", "heightmap"])
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
def test_quads_equal_the_lane_per_body_loop_bit_for_bit(built_lib, tmp_path, config, resident):
    """q, u, contact records (impulses), contact counts, solver flags and iteration counts after 20 control steps of the benchmark population, and every control
    step's obs block and done flags on the way"""
    spec = tmp_path / "spec"
    spec.mkdir()
    out = {}
    for tag, defs in (("quads", ""), ("lanes", "-DRSB_X_NO_UP_QUADS")):
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp_path / f"{tag}.npz")
        p = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, config=config, resident=resident, out=path)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stderr[-3000:])
        out[tag] = np.load(path)
    assert len([f for f in os.listdir(spec) if f.endswith(".hsaco")]) == 2, os.listdir(spec)      # (each variant compiled and ran a code object of its own)
    a, b = out["quads"], out["lanes"]
    assert int(a["cnt"].sum()) > 0 and np.isfinite(a["q"]).all() and np.isfinite(a["u"]).all()
    for key in ("q", "u", "con", "cnt", "iters", "flags", "obs", "done"):
        assert a[key].tobytes() == b[key].tobytes(), (key, int((a[key] != b[key]).sum()))


@pytest.mark.parametrize("chains,length,levels", [(5, 2, 0), (4, 2, 2)], ids=["five_on_a_level", "four_chains_of_two"])
def test_other_chain_models_match_the_oracle(built_lib, chains, length, levels):
    """five bodies on a level: the specialised code object keeps the lane = body loop; four chains of two bodies: the quad form at another tree depth than the quadruped's"""
    rng = np.random.default_rng(77)
    model = Model(urdf_string=_chains_urdf(chains, length))
    assert len(model.up_quads()) == levels and model.nb == 1 + chains * length
    nq, nv, N = model.nq, model.nv, 128
    kmax = 16 if model.ncol > 8 else 8
    gc = np.zeros((N, nq)); gc[:, 0:2] = rng.uniform(-1, 1, (N, 2)); gc[:, 2] = rng.uniform(0.0, 0.5, N)
    qq = rng.normal(size=(N, 4)); gc[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    gc[:, 7:] = rng.uniform(-0.5, 0.5, (N, nq - 7))
    gv = rng.normal(size=(N, nv)) * 1.0
    kp = np.zeros(nv, np.float32); kd = np.zeros(nv, np.float32)
    kp[6:] = rng.uniform(0, 60, nv - 6); kd[6:] = rng.uniform(0, 1.0, nv - 6)
    pt = gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (N, nq - 7))
    w = BatchedWorld(model, N); w.set_max_contacts(kmax)
    w.set_specialization("compile")
    o = Oracle(model.blob); o.p.kmax = kmax
    dtg = np.zeros((N, nv))
    w.set_pd_gains(kp, kd); w.set_pd_target(pt, dtg); w.set_state(gc, gv)
    w.integrate(1)
    q1, u1 = w.get_state(); cnt, _ = w.get_contacts(); fl = w.get_flags()
    _, n_spec, n_gen = w.specialization_status()
    ref = o.step_batch(f32(gc), f32(gv), 1, kp.astype(np.float64), kd.astype(np.float64), f32(pt), dtg)
    w.close()
    assert n_spec == 1 and n_gen == 0, (n_spec, n_gen)
    assert np.array_equal(cnt, ref["n_contacts"])
    conv = ((ref["flags"] | fl) & 5) == 0
    assert conv.mean() > 0.6, conv.mean()
    eu = np.abs(u1 - ref["u"]).max(axis=1) / (1 + np.abs(ref["u"]).max(axis=1))
    eq = np.abs(q1 - ref["q"]).max(axis=1)
    assert np.isfinite(q1).all() and np.isfinite(u1).all()
    assert eu[conv].max() < 2e-3 and np.median(eu) < 2e-5 and eq[conv].max() < 2e-5, (eu[conv].max(), np.median(eu), eq[conv].max())
