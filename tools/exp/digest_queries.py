"""digest of every output of the ten batched query entry points (frames, terrain, centroidal, dynamics), host and device forms, at N = 41 over four worlds:
anymal after 20 control steps on height maps (contact records, RSB_DYN_CONTACTS), atlas, and a floating and a fixed random tree with prismatic joints
under tilted gravity.  One line per (world, entry point, output, space): two libraries that are the same arithmetic (RSB_LIB_PATH) print the same lines"""
import os, sys, hashlib
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from raisimlib_amd import BatchedWorld, Model, _capi, rsc_path, workload
from test_dynamics_reference import dyn_case
from test_gpu_slow_path import CASES, case
N = 41
DEV = torch.device("cuda:0")
rng = np.random.default_rng(4100)


def line(world, entry, name, space, a):
    a = np.ascontiguousarray(a)
    print(f"{world:9s} {entry:34s} {name:12s} {space:6s} sha1 {hashlib.sha1(a.tobytes()).hexdigest()[:16]}  -0.0 entries {int((np.signbit(a) & (a == 0)).sum())}", flush=True)


def queries(world, w, model, contacts):
    nb, nv = model.nb, model.nv
    frames = [(nb - 1, (0.05, -0.02, 0.1)), (nb - 1, (-0.1, 0.03, 0.0)), (nb // 2, (0.0, 0.04, -0.06))]
    f32 = lambda *s: rng.normal(size=s).astype(np.float32)
    udot, tau, force, torque = f32(N, nv), f32(N, nv), f32(N, 3, 3), f32(N, 3, 3)
    force[:, 2] = 0.0; torque[:, 1] = 0.0
    gc = w.get_state()[0]
    xy = (gc[:, None, :2] + rng.uniform(-1.5, 1.5, (N, 7, 2))).astype(np.float32)
    ro = np.concatenate([xy[:, :5], gc[:, None, 2:3] + rng.uniform(0.2, 1.0, (N, 5, 1)).astype(np.float32)], axis=2)
    rd = f32(N, 5, 3); rd[:, :, 2] = -np.abs(rd[:, :, 2])
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, 11), np.linspace(-0.3, 0.3, 3), indexing="ij")
    pattern = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
    P, wide = pattern.shape[0], 3 * pattern.shape[0] + 5
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    for space in ("host", "device"):
        d = space == "device"
        t = (lambda a: torch.from_numpy(a).to(DEV)) if d else (lambda a: a)
        full = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV) if d else np.full(s, 7.0, np.float32)
        back = lambda a: a.cpu().numpy() if d else a
        def put(entry, res):
            for k, v in res.items():
                line(world, entry, k, space, back(v))
        put("rsb_get_frame_kinematics", w.frame_kinematics(frames, out={"pos": full(N, 3, 3), "rot": full(N, 3, 3, 3), "lin_vel": full(N, 3, 3), "ang_vel": full(N, 3, 3)}))
        put("rsb_get_frame_jacobians", w.frame_jacobians(frames, out={"lin": full(N, 3, 3, nv), "rot": full(N, 3, 3, nv)}))
        w.set_generalized_force(tau)
        w.add_external_wrench(frames[0], t(force[:, 0].copy()), t(torque[:, 0].copy()), t(mask))
        w.add_external_wrench(frames[2], None, t(torque[:, 2].copy()), None)
        line(world, "rsb_add_external_wrench", "tau_ff", space, w.get_field(_capi.RSB_F_TAU_FF))
        out = {"height": full(N, 7), "normal": full(N, 7, 3)}
        w.terrain_height(t(xy), out=out)
        put("rsb_get_terrain_height", out)
        for yaw in (True, False):
            put("rsb_height_scan", {"yaw" if yaw else "world": w.height_scan(frames, t(pattern), yaw_aligned=yaw, out=full(N, 3, P))})
        put("rsb_height_scan", {"row_stride": w.height_scan(frames, t(pattern), out=full(N, wide), row_stride=wide)})
        put("rsb_ray_test", {"dist": w.ray_test(t(ro), t(rd), 4.0, out=full(N, 5))})
        put("rsb_get_centroidal", w.centroidal(out={k: full(N, 3) for k in ("com", "com_vel", "lin_mom", "ang_mom")} | {"kinetic": full(N), "potential": full(N)}))
        put("rsb_get_centroidal_momentum_matrix", {"A": w.centroidal_momentum_matrix(out=full(N, 6, nv))})
        loads = (frames, t(force), t(torque))
        put("rsb_inverse_dynamics", w.inverse_dynamics(t(udot), loads=loads, contacts=contacts, out={"tau": full(N, nv), "joint_force": full(N, nb, 3), "joint_torque": full(N, nb, 3)}))
        put("rsb_inverse_dynamics", {"h": w.inverse_dynamics(None, out={"tau": full(N, nv)})["tau"]})
        put("rsb_forward_dynamics", {"udot": w.forward_dynamics(t(tau), loads=loads, contacts=contacts, out=full(N, nv))})
        put("rsb_forward_dynamics", {"udot_ff": w.forward_dynamics(None, out=full(N, nv))})


def world_of(model, gc, gv, gravity=None):
    w = BatchedWorld(model, N)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    if gravity is not None:
        w.set_gravity(gravity)
    w.set_state(gc[:N], gv[:N])
    return w


# anymal: 20 control steps on three height maps
anymal = Model(urdf_path=rsc_path("anymal_c_like.urdf"))
maps, env_map = workload.env_heightmaps(3, xs=64, ys=64), np.arange(N, dtype=np.int32) % 3
w = BatchedWorld(anymal, N)
w.set_stream(torch.cuda.current_stream().cuda_stream)
w.add_height_maps(maps, 16.0, 16.0, 0.0, 0.0, env_map)
w.set_pd_gains(*workload.anymal_gains())
w.set_state(*workload.anymal_initial_state_on_maps(N, maps, env_map, 16.0))
for k in range(20):
    w.set_pd_target(workload.anymal_targets(N, k).astype(np.float32), np.zeros((N, anymal.nv), np.float32)); w.integrate(workload.SUBSTEPS)
counts = w.get_contacts()[0]
q, u = w.get_state()
print(f"anymal after 20 control steps: {int(counts.sum())} contact records in {int((counts > 0).sum())} envs, state digest {hashlib.sha1(q.tobytes() + u.tobytes()).hexdigest()[:12]}", flush=True)
assert counts.sum() > 0
queries("anymal", w, anymal, True)
w.close()

atlas = Model(urdf_path=rsc_path("atlas_like.urdf"))
w = world_of(atlas, *workload.random_state(atlas.nq, atlas.nv, N, seed=4, joint_range=1.0))
queries("atlas", w, atlas, False)
w.close()

for kind in ("floating", "fixed"):
    i = next(i for k, i in CASES if k == kind and case(k, i).prismatic)
    c = dyn_case(f"{kind}{i}")
    print(f"{kind}{i}: {c.nb} bodies, gravity {c.gravity}", flush=True)
    w = world_of(c.model, c.gc, c.gv, c.gravity)
    queries(f"{kind}{i}", w, c.model, False)
    w.close()
