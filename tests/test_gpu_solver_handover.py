"""The contact solver's hand-over in the square-layout classes (contact capacity 8): the Delassus blocks are stored in the row-block form the solver's registers take
them in (raisimlib_amd/csrc/step_types.h: g_row_pitch; step_kernel.h: gblk_load; step_phase_delassus.inc, step_phase_solver.inc).  All of it is data movement: no sum
changes its order, no expression changes, so every result must keep its bits.  The dense rows it replaces stay selectable at compile time (-DRSB_X_G_SQUARE through
$RSB_SPEC_EXTRA_DEFS, part of a code object's key): the same world is run in two child processes, one per variant, and everything it holds afterwards is compared byte
for byte - the benchmark populations, a population that leaves the common path (six and more contacts per env, self-collisions, joint-limit rows), a fixed-base model
(kernel class bit 1: the compliance block) and the debug dump of one env's contact problem."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_up_quads import _CHILD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = "-DRSB_X_G_SQUARE"
KEYS = ("q", "u", "con", "cnt", "iters", "flags", "obs", "done")
SELF_A = 0x10000

SIDE_SEED, SIDE_N, SIDE_K = 1, 64, 8      # (seed picked on the CPU: the oracle's run of this population holds 1204 env-sub-steps with >= 6 contacts, 1381 with a
#                                            self-collision and 179 that start with a joint beyond its limit)
FIXED_SEED = 3                            # tests/test_gpu_fuzz.py::test_random_fixed_base_tree_parity[3]: three links, the smallest of its models whose links reach the ground


def side_population(model, seed, n):
    """ANYmal-like envs lying on their left or right side just above the ground, joint coordinates drawn over the full joint range, unit joint velocities,
    PD targets within 0.3 rad of the pose"""
    rng = np.random.default_rng(seed)
    b = model.blob
    lo = np.array([b.q_lower[i] for i in range(1, b.nb)]); hi = np.array([b.q_upper[i] for i in range(1, b.nb)])
    gc = np.zeros((n, model.nq)); gc[:, 0:2] = rng.uniform(-1, 1, (n, 2)); gc[:, 2] = rng.uniform(0.18, 0.32, n)
    roll = np.where(rng.random(n) < 0.5, 0.5, -0.5) * np.pi + rng.uniform(-0.2, 0.2, n)
    yaw = rng.uniform(-np.pi, np.pi, n)
    w1, x1, y1, z1 = np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)
    w2, x2, y2, z2 = np.cos(roll / 2), np.sin(roll / 2), 0 * roll, 0 * roll
    gc[:, 3:7] = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)
    gc[:, 7:] = rng.uniform(lo, hi, (n, model.nq - 7))
    gv = rng.normal(size=(n, model.nv))
    pt = gc.copy(); pt[:, 7:] += rng.uniform(-0.3, 0.3, (n, model.nq - 7))
    return gc.astype(np.float32), gv.astype(np.float32), pt.astype(np.float32), lo, hi


def _pair(tmp_path, script, n_objects, **fmt):
    """the child `script` once per variant, each with a code-object cache of its own kind in one directory; returns the two result files"""
    spec = tmp_path / "spec"
    spec.mkdir()
    out = {}
    for tag, defs in (("new", ""), ("old", OLD)):
        env = dict(os.environ, RSB_SPEC_DIR=str(spec), RSB_SPEC_EXTRA_DEFS=defs)
        env.pop("RSB_SPECIALIZE", None)
        path = str(tmp_path / f"{tag}.npz")
        p = subprocess.run([sys.executable, "-c", script.format(root=ROOT, out=path, **fmt)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stderr[-3000:])
        out[tag] = np.load(path)
    assert len([f for f in os.listdir(spec) if f.endswith(".hsaco")]) == 2 * n_objects, os.listdir(spec)      # (each variant compiled and ran code objects of its own)
    return out["new"], out["old"]


def _same(a, b, keys):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), (key, int((a[key] != b[key]).sum()))


@pytest.mark.parametrize("config", [2, 3], ids=["flat", "heightmap"])
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
def test_benchmark_populations_keep_their_bits(built_lib, tmp_path, config, resident):
    """q, u, contact records (impulses), contact counts, solver flags and iteration counts after 20 control steps of the benchmark population, and every control
    step's obs block and done flags on the way"""
    a, b = _pair(tmp_path, _CHILD, 1, config=config, resident=resident)
    assert int(a["cnt"].sum()) > 0 and np.isfinite(a["q"]).all() and np.isfinite(a["u"]).all()
    _same(a, b, KEYS)


_SIDE_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np, torch
import bench
from raisimlib_amd import BatchedWorld, workload
from test_gpu_solver_handover import side_population
N, K = {n}, {k}
r = bench.Recipe(2, -1.0)
gc, gv, pt, lo, hi = side_population(r.model, {seed}, N)
feet = np.asarray(r.feet, np.int32)
bank = torch.from_numpy(pt[None].copy()).to("cuda:0")

def world():
    w = BatchedWorld(r.model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    r.setup_world(w, N, 0)
    w.set_specialization("compile")
    w.set_state(gc, gv)
    w.set_pd_target(pt, np.zeros((N, r.model.nv), np.float32))
    return w

# K control steps without the termination rule (the envs lie on their trunks): obs block and done flags of every step, contact records of every step
w = world()
od = w.obs_dim(len(feet))
obs = torch.zeros((K, N, od), dtype=torch.float32, device="cuda:0")
done = torch.full((K, N), 7, dtype=torch.uint8, device="cuda:0")
cnts, cons = [], []
for j in range(K):
    fn = w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), 1, obs[j].data_ptr(), N * od, feet, None, 0, 0, N, done[j].data_ptr(), N)
    fn(1, 0)
    w.synchronize()
    cnt, con = w.get_contacts()
    con = con.copy(); con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0      # (slots past an env's count hold what an earlier step left there)
    cnts.append(cnt.copy()); cons.append(con)
q, u = w.get_state()
_, n_spec, n_gen = w.specialization_status()
assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
flags, iters = w.get_flags(), w.get_solver_iterations()
w.close()
cnts = np.stack(cnts); cons = np.stack(cons)

# the contact problem of the env with the most contacts after the last step, dumped by the profiling twin (its own specialised code object) on the same run
e = int(np.argmax(cnts[-1]))
w = world()
w.debug_select_env(e)
for j in range(K):
    w.integrate(workload.SUBSTEPS)
w.synchronize()
nc, G, c, lam = w.debug_contact_problem()
_, n_spec, n_gen = w.specialization_status()
assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
q2, u2 = w.get_state()
w.close()
np.savez({out!r}, obs=obs.cpu().numpy(), done=done.cpu().numpy(), q=q, u=u, cnt=cnts, con=np.frombuffer(cons.tobytes(), np.uint8), collision=cons["collision"], flags=flags, iters=iters,
         dbg_env=e, dbg_nc=nc, dbg_G=G, dbg_c=c, dbg_lam=lam, q2=q2, u2=u2, lo=lo, hi=hi)
"""


def test_a_population_off_the_common_path_keeps_its_bits(built_lib, tmp_path):
    """64 envs lying on a side with joints anywhere in their range, 8 control steps: blocks 5-7 of the exchange (six and more contacts), the self-collision fold and
    joint-limit rows must all occur on the device - read from its contact records and, for the limit rows (they are rows of the solve, not contacts: the records do not
    list them), from the joint coordinates a control step ends with, which the next sub-step starts from - and then everything is compared as above.  The profiling twin's
    dump of one env's contact problem (G as a dense matrix, c, lambda) is compared too."""
    a, b = _pair(tmp_path, _SIDE_CHILD, 2, n=SIDE_N, k=SIDE_K, seed=SIDE_SEED)
    assert np.isfinite(a["q"]).all() and np.isfinite(a["u"]).all()
    cnt, col = a["cnt"], a["collision"]
    live = np.arange(col.shape[2])[None, None, :] < cnt[:, :, None]
    six = int((cnt >= 6).sum()); selfc = int((((col & SELF_A) != 0) & live).any(axis=2).sum())
    nq = a["q"].shape[1]
    qj = a["obs"][:-1, :, 7:nq]                                  # joint coordinates at the end of control steps 0 .. K - 2 (the obs row starts with q)
    limit = int(((qj > a["hi"]) | (qj < a["lo"])).any(axis=2).sum())
    print(f"env-steps with >= 6 contacts {six}, with a self-collision {selfc}, that start with a joint beyond its limit {limit}; dump: env {int(a['dbg_env'])} with {int(a['dbg_nc'])} contacts")
    assert six > 0 and selfc > 0 and limit > 0, (six, selfc, limit)
    _same(a, b, KEYS)
    assert int(a["dbg_nc"]) >= 1 and np.abs(a["dbg_G"]).sum() > 0
    assert np.array_equal(a["dbg_G"], a["dbg_G"].T)              # (the dump is the dense symmetric matrix whatever the storage)
    _same(a, b, ("dbg_env", "dbg_nc", "dbg_G", "dbg_c", "dbg_lam", "q2", "u2"))
    assert a["q2"].tobytes() == a["q"].tobytes() and a["u2"].tobytes() == a["u"].tobytes()      # (and the twin ran the same steps)


_FIXED_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join({root!r}, "tests")); sys.path.insert(0, {root!r})
import numpy as np
from raisimlib_amd import BatchedWorld, Model
from test_gpu_fuzz import random_urdf
rng = np.random.default_rng(4000 + {seed})
n_links = int(rng.integers(3, 9))
model = Model(urdf_string=random_urdf(rng, n_links).replace('"l0"', '"world"'))
assert model.blob.fixed_base == 1 and n_links == 3
nq, nv, N = model.nq, model.nv, 32
gc = np.zeros((N, nq)); gc[:, 3] = 1.0
gc[:, 7:] = rng.uniform(-1.5, 1.5, (N, nq - 7))
gv = np.zeros((N, nv)); gv[:, 6:] = rng.normal(size=(N, nv - 6))
kp = np.zeros(nv, np.float32); kd = np.zeros(nv, np.float32); kp[6:] = 30.0; kd[6:] = 0.5
w = BatchedWorld(model, N); w.set_max_contacts(8); w.add_ground(-0.25)
w.set_specialization("compile")
w.set_pd_gains(kp, kd); w.set_pd_target(gc, np.zeros((N, nv))); w.set_state(gc, gv)
cnts = []
for j in range(4):
    w.integrate(1)
    cnts.append(w.get_contacts()[0].copy())
q, u = w.get_state(); cnt, con = w.get_contacts()
con = con.copy(); con[np.arange(con.shape[1])[None, :] >= cnt[:, None]] = 0
_, n_spec, n_gen = w.specialization_status()
assert n_spec > 0 and n_gen == 0, (n_spec, n_gen)
np.savez({out!r}, q=q, u=u, cnt=np.stack(cnts), con=np.frombuffer(con.tobytes(), np.uint8), flags=w.get_flags(), iters=w.get_solver_iterations())
w.close()
"""


def test_a_fixed_base_model_keeps_its_bits(built_lib, tmp_path):
    """kernel class bit 1 (the compliance added to every contact's own block) at contact capacity 8: 32 envs of a three-link fixed-base tree, four steps"""
    a, b = _pair(tmp_path, _FIXED_CHILD, 1, seed=FIXED_SEED)
    assert int(a["cnt"].sum()) > 0 and np.isfinite(a["q"]).all() and np.isfinite(a["u"]).all()
    _same(a, b, ("q", "u", "con", "cnt", "iters", "flags"))
