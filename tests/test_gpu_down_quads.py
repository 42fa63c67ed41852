"""The quad form of the down pass's level loop (four lanes per body in the specialised code objects of the quadruped: raisimlib_amd/csrc/step_phase_tree_down.inc,
step_spec.h RSB_DOWN_QUADS) splits OUTPUTS over the four lanes and never a sum, and evaluates every float by the expression of the lane = body loop it replaces, so it
must give that loop's bits.  The loop stays selectable at compile time beside the up pass's quad form (-DRSB_X_NO_DOWN_QUADS through $RSB_SPEC_EXTRA_DEFS, part of a code
object's key): the same world is run in two child processes, one per variant, and everything it holds after 20 control steps is compared byte for byte.  The benchmark
robot has revolute joints only and three levels: chain models of another depth and with one prismatic joint per chain run the quad form against the oracle at the
tolerances of tests/test_gpu_fuzz.py; five bodies on a level stay on the lane = body loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import Oracle, f32
from raisimlib_amd import BatchedWorld, Model
from test_gpu_up_quads import _CHILD
from test_up_quads_host import _chains_urdf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("config", [2, 3], ids=["flat", "heightmap"])
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
def test_down_quads_equal_the_lane_per_body_loop_bit_for_bit(built_lib, tmp_path, config, resident):
    """q, u, contact records (impulses), contact counts, solver flags and iteration counts after 20 control steps of the benchmark population, and every control
    step's obs block and done flags on the way"""
    spec = tmp_path / "spec"
    spec.mkdir()
    out = {}
    for tag, defs in (("quads", ""), ("lanes", "-DRSB_X_NO_DOWN_QUADS")):
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


def _chains_urdf_prismatic(n_chains, length, prismatic_at, sphere_links):
    """_chains_urdf with link `prismatic_at` of every chain on a prismatic joint (axis 0 0 1, limits +-0.6) and collision spheres on the links of `sphere_links` only"""
    parts = ['<robot name="chains"><link name="base"><inertial><mass value="8"/><inertia ixx="0.2" ixy="0" ixz="0" iyy="0.3" iyz="0" izz="0.4"/></inertial></link>']
    for c in range(n_chains):
        for k in range(length):
            col = '<collision><geometry><sphere radius="0.04"/></geometry></collision>' if k in sphere_links else ""
            parts.append(f'<link name="c{c}_{k}"><inertial><mass value="1"/><inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial>{col}</link>')
            parent = "base" if k == 0 else f"c{c}_{k - 1}"
            if k == prismatic_at:
                kind, axis, lim = "prismatic", "0 0 1", 'lower="-0.6" upper="0.6"'
            else:
                kind, axis, lim = "revolute", "0 1 0", 'lower="-6" upper="6"'
            parts.append(f'<joint name="j{c}_{k}" type="{kind}"><origin xyz="{0.1 * c:.2f} 0.05 -0.15"/><parent link="{parent}"/><child link="c{c}_{k}"/>'
                         f'<axis xyz="{axis}"/><limit effort="0" velocity="50" {lim}/></joint>')
    parts.append("</robot>")
    return "\n".join(parts)


_MODELS = {
    "five_on_a_level": (lambda: _chains_urdf(5, 2), 5, 2, 0),
    "four_chains_of_two": (lambda: _chains_urdf(4, 2), 4, 2, 2),
    "four_of_two_prismatic_leaf": (lambda: _chains_urdf_prismatic(4, 2, 1, (0, 1)), 4, 2, 2),
    "four_of_two_prismatic_root": (lambda: _chains_urdf_prismatic(4, 2, 0, (0, 1)), 4, 2, 2),
    "four_of_three_prismatic_middle": (lambda: _chains_urdf_prismatic(4, 3, 1, (1, 2)), 4, 3, 3),
    "four_of_three_prismatic_leaf": (lambda: _chains_urdf_prismatic(4, 3, 2, (1, 2)), 4, 3, 3),
}


@pytest.mark.parametrize("name", list(_MODELS))
def test_other_chain_models_match_the_oracle(built_lib, name):
    """one integrate() of 128 seeded envs against the oracle, as tests/test_gpu_up_quads.py does.  The quad form runs at contact capacity 8 only: the models that must
    run it keep ncol <= 8 (spheres on eight links), so that kmax = 8 and the specialised code object cannot fall back to the lane = body loop unnoticed"""
    urdf, chains, length, levels = _MODELS[name]
    rng = np.random.default_rng(77)
    model = Model(urdf_string=urdf())
    assert len(model.up_quads()) == levels and model.nb == 1 + chains * length
    if levels:
        assert model.ncol <= 8, model.ncol
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
    eu = np.abs(u1 - ref["u"]).max(axis=1) / (1 + np.abs(ref["u"]).max(axis=1))
    eq = np.abs(q1 - ref["q"]).max(axis=1)
    print(f"{name}: converged {conv.mean():.3f} contacts mean {cnt.mean():.2f} max {int(cnt.max())} eu max {eu[conv].max():.3e} median {np.median(eu):.3e} eq max {eq[conv].max():.3e}")
    assert conv.mean() > 0.6, conv.mean()
    assert np.isfinite(q1).all() and np.isfinite(u1).all()
    assert eu[conv].max() < 2e-3 and np.median(eu) < 2e-5 and eq[conv].max() < 2e-5, (eu[conv].max(), np.median(eu), eq[conv].max())
