"""Ray casts and sensor-mounted ray scans that also hit the robot, on the device (rsb_ray_cast, rsb_ray_scan; raisimlib_amd/csrc/rsb_ray_scan.hip)
against the fp64 reference of tests/ray_bodies_reference.py: body poses from the oracle's forward kinematics on the float32-rounded state, shapes
from the blob, and a PROPERTY check of every device answer with tol = 1e-5 (1 + max(|origin|, max_dist)) - see that module.  The terrain's side of
the check is check_ray of tests/test_gpu_terrain_query.py on that file's 9 x 7 maps (three of them, mixed over the envs), or a plane in closed form.
The worst residual per case, in units of tol, goes to profiles/ray_scan_parity.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_bodies_reference as rb
import test_gpu_terrain_query as tq
from common import ROOT, Oracle, f32, sphere_urdf, standing_states
from raisimlib_amd import BatchedWorld, Model, _capi, depth_camera_rays, lidar_rays, workload
from terrain_reference import random_map

pytestmark = pytest.mark.gpu

NONE, TERRAIN = _capi.RSB_RAY_HIT_NONE, _capi.RSB_RAY_HIT_TERRAIN
REPORT = {}

# a fixed base; a revolute and a prismatic joint; a sphere on the base, a capsule and a box on the arm, a cylinder on the slide
SHAPES_URDF = """<?xml version="1.0"?>
<robot name="shapes">
  <link name="world"/>
  <link name="mount"><inertial><origin xyz="0 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial>
    <collision><origin xyz="0 0 0"/><geometry><sphere radius="0.15"/></geometry></collision></link>
  <joint name="bolt" type="fixed"><origin xyz="0 0 1.0"/><parent link="world"/><child link="mount"/></joint>
  <link name="arm"><inertial><origin xyz="0.3 0 0"/><mass value="1"/><inertia ixx="1e-2" ixy="0" ixz="0" iyy="1e-2" iyz="0" izz="1e-2"/></inertial>
    <collision><origin xyz="0.3 0 0" rpy="0 1.5707963 0"/><geometry><capsule radius="0.06" length="0.4"/></geometry></collision>
    <collision><origin xyz="0.75 0 0" rpy="0.3 0.2 0.1"/><geometry><box size="0.2 0.3 0.1"/></geometry></collision></link>
  <joint name="shoulder" type="revolute"><origin xyz="0.25 0 0"/><parent link="mount"/><child link="arm"/><axis xyz="0 1 0"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
  <link name="slide"><inertial><origin xyz="0 0 0"/><mass value="0.5"/><inertia ixx="1e-3" ixy="0" ixz="0" iyy="1e-3" iyz="0" izz="1e-3"/></inertial>
    <collision><origin xyz="0 0 -0.2" rpy="0.4 0 0"/><geometry><cylinder radius="0.08" length="0.3"/></geometry></collision></link>
  <joint name="rail" type="prismatic"><origin xyz="0.4 0.35 0"/><parent link="arm"/><child link="slide"/><axis xyz="0 0 1"/>
    <limit effort="0" velocity="100" lower="-10" upper="10"/></joint>
</robot>
"""


def record(section, lines):
    REPORT[section] = lines
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ray_scan_parity.txt"), "w") as f:
        f.write("tests/test_gpu_ray_scan.py: the property check of tests/ray_bodies_reference.py on every device answer, fp64 reference on the\n"
                "float32-rounded state; worst residual in units of tol = 1e-5 (1 + max(|origin|, max_dist))\n")
        for name in sorted(REPORT):
            f.write(f"{name}\n" + "".join(f"  {l}\n" for l in REPORT[name]))


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


class MapTerrain:
    """the terrain's side of rb.check_answer on a height map: check_ray and the breakpoints of tests/test_gpu_terrain_query.py"""

    def __init__(self, oracle):
        self.o = oracle

    def check(self, o, d, max_dist, t):
        return tq.check_ray(self.o, o, d, max_dist, t)

    def deepest_before(self, o, dn, max_dist, t_end):
        bp = tq.ray_breakpoints(o, dn, max_dist)
        if bp is None:
            return 0.0
        s = bp[2][bp[2] <= t_end]
        return max(0.0, -min(tq.gap(self.o, o, dn, x) for x in s)) if s.size else 0.0


def scan_maps():
    """three maps of the geometry check_ray knows, as tests/terrain_reference.random_map makes them (heights within +- 0.4 cells)"""
    return np.stack([random_map(tq.XS, tq.YS, tq.X_SIZE, tq.Y_SIZE, tq.CX, tq.CY, 0.4, seed).h32 for seed in (21, 22, 23)])


def make_world(model, N, terrain):
    """terrain "plane": z = 0.05; "maps": scan_maps() mixed over the envs -> (world, the check's terrain object per env)"""
    w = BatchedWorld(model, N)
    if terrain == "plane":
        w.add_ground(0.05)
        return w, [rb.PlaneTerrain(0.05)] * N
    maps = scan_maps()
    env_map = (np.arange(N, dtype=np.int32) * 2) % 3
    w.add_height_maps(maps, tq.X_SIZE, tq.Y_SIZE, tq.CX, tq.CY, env_map)
    per_map = [MapTerrain(o) for o in tq.map_oracles(model, maps)]
    return w, [per_map[m] for m in env_map]


class Scene:
    """the reference's view of the robot in N envs: world-frame shapes and body poses from the oracle on the float32-rounded state"""

    def __init__(self, model, gc):
        o = Oracle(model.blob)
        self.shapes = rb.shapes_of(model.blob)
        self.poses = [rb.body_poses(o, f32(q)) for q in gc]
        self.world = [[rb.to_world(s, p) for s in self.shapes] for p in self.poses]

    def scan_rays(self, e, frames, dirs):
        """-> origins [F, 3], directions [F, P, 3] of env e in world coordinates, bodies [F]"""
        o = np.array([self.poses[e][b][1] + self.poses[e][b][0] @ f32(off) for b, off in frames])
        d = np.array([dirs.astype(np.float64) @ self.poses[e][b][0].T for b, _ in frames])
        return o, d, [b for b, _ in frames]

    def allowed(self, body, bodies, own):
        return [bodies and (own or s["body"] != body) for s in self.shapes]


def check_scan(scene, terrains, frames, dirs, max_dist, out, hit, bodies, own):
    """every ray of a ray_scan call -> (worst residual / tol, failures, body hits, terrain hits)"""
    worst, bad, nb, nt = 0.0, [], 0, 0
    for e in range(out.shape[0]):
        o, d, fb = scene.scan_rays(e, frames, dirs)
        for f in range(len(frames)):
            allowed = scene.allowed(fb[f], bodies, own)
            for k in range(dirs.shape[0]):
                ok, res, why = rb.check_answer(scene.world[e], allowed, o[f], d[f, k], max_dist, float(out[e, f, k]), int(hit[e, f, k]), terrains[e])
                worst = max(worst, res)
                nb, nt = nb + (hit[e, f, k] >= 0), nt + (hit[e, f, k] == TERRAIN)
                if not ok:
                    bad.append((e, f, k, float(out[e, f, k]), int(hit[e, f, k]), why))
    return worst, bad, int(nb), int(nt)


# ---- 1. every shape kind ------------------------------------------------------------------------------------------------------------------------
def shapes_model():
    m = Model(urdf_string=SHAPES_URDF)
    assert m.blob.fixed_base == 1 and m.nb == 3
    kinds = sorted((s["kind"], s["body"]) for s in rb.shapes_of(m.blob))
    assert kinds == [("box", 1), ("capsule", 1), ("cylinder", 2), ("sphere", 0)], kinds
    return m


def shapes_states(N, seed=1):
    rng = np.random.default_rng(seed)
    gc = np.zeros((N, 9))
    gc[:, 3] = 1.0
    gc[:, 7], gc[:, 8] = rng.uniform(-0.3, 0.3, N), rng.uniform(-0.1, 0.15, N)
    return gc


def aimed_pattern(scene, frame, P, seed):
    """directions in the axes of the frame's body: for each shape of env 0 three into it, two just beside it and one well past it, the rest down
    and around"""
    rng = np.random.default_rng(seed)
    body, off = frame
    R, p = scene.poses[0][body]
    o = p + R @ f32(off)
    dirs = []
    for s in scene.world[0]:
        c = s["centre"] if "centre" in s else 0.5 * (s["a"] + s["b"])
        size = s.get("radius", None) or float(np.linalg.norm(s["half"], axis=1).min())
        to = c - o
        if np.linalg.norm(to) < 1e-6:
            to = np.array([1.0, 0.0, 0.0])
        side = np.cross(to, rng.normal(size=3))
        side /= np.linalg.norm(side)
        for scale in (0.0, 0.5, 0.9, 1.02, 1.3, 6.0):
            dirs.append(R.T @ (to + scale * size * side))
    while len(dirs) < P:
        v = rng.normal(size=3)
        v[2] = -abs(v[2]) - 0.3 * (len(dirs) % 2)
        dirs.append(v * rng.uniform(0.5, 3.0))
    return np.array(dirs[:P]).astype(np.float32)


@pytest.mark.parametrize("terrain", ["plane", "maps"])
def test_properties_of_every_shape_kind(terrain):
    N, P, max_dist = 5, 37, 5.0
    model = shapes_model()
    gc = shapes_states(N)
    dev_gc = gc.copy()
    dev_gc[1, 3] = 1.7      # the base quaternion is normalised first
    scene = Scene(model, gc)
    box = next(s for s in scene.shapes if s["kind"] == "box")
    frames = [(0, (0.1, -0.9, 0.7)), (1, tuple(box["centre"] + [0.01, -0.02, 0.01]))]      # outside everything; inside the box, on the box's body
    dirs = aimed_pattern(scene, frames[0], P, seed=2)
    w, terrains = make_world(model, N, terrain)
    w.set_state(dev_gc, np.zeros((N, model.nv)))
    lines, failures = [], []
    for name, kw in (("BODIES", dict(bodies=True)), ("BODIES | OWN_BODY", dict(bodies=True, own_body=True)), ("0", dict(bodies=False))):
        out, hit = w.ray_scan(frames, dirs, max_dist, hit=True, **kw)
        assert out.shape == (N, 2, P) and hit.shape == (N, 2, P) and hit.dtype == np.int32
        worst, bad, nb, nt = check_scan(scene, terrains, frames, dirs, max_dist, out, hit, kw["bodies"], kw.get("own_body", False))
        print(f"ray_scan {terrain} flags {name}: worst residual {worst:.3g} tol, {nb} body hits, {nt} terrain hits of {N * 2 * P}, {len(bad)} violations {bad[:4]}")
        lines.append(f"rsb_ray_scan flags {name:18s} worst residual {worst:.3e} tol   ({nb} body hits, {nt} terrain hits of {N * 2 * P} rays, {len(bad)} violations)")
        failures += bad
        seen = {int(h) for h in hit[:, 0].ravel() if h >= 0}      # what the sensor outside everything hits
        if name == "0":
            assert nb == 0
        elif name == "BODIES":
            assert seen == {s["prim"] for s in scene.shapes if s["body"] != 0}, seen      # every shape but the one of its own body
            assert not np.any(hit[:, 1] == box["prim"])                  # the sensor in the box sees through its mount ...
        else:
            assert seen == {s["prim"] for s in scene.shapes}, seen      # every shape kind is hit from outside
            assert np.all(hit[:, 1] == box["prim"]) and np.all(out[:, 1] == 0.0)      # ... unless asked: an origin inside a shape gives 0
    # world-space rays from inside and outside every shape kind
    rng = np.random.default_rng(3)
    org, dr = np.zeros((N, P, 3)), rng.normal(size=(N, P, 3))
    for e in range(N):
        for r in range(P):
            s = scene.world[e][r % 4]
            c = s["centre"] if "centre" in s else s["a"] + rng.uniform(0.2, 0.8) * (s["b"] - s["a"])      # (a cylinder ends flat: keep off its caps)
            size = s.get("radius", None) or float(np.linalg.norm(s["half"], axis=1).min())
            if r % 8 < 4:
                org[e, r] = c + 0.5 * size * rng.uniform(-1, 1, 3) / np.sqrt(3.0)      # inside
                assert rb.phi(s, org[e, r].astype(np.float32).astype(np.float64)) < -1e-3
            else:
                away = rng.normal(size=3)
                org[e, r] = c + away / np.linalg.norm(away) * rng.uniform(0.3, 1.5)
                org[e, r, 2] = max(org[e, r, 2], 0.45)
                dr[e, r] = (c - org[e, r]) + rng.normal(size=3) * size * (0.5 if r % 3 else 1.5)
    org32, dr32 = org.astype(np.float32), dr.astype(np.float32)
    dist, hit = w.ray_cast(org32, dr32, max_dist, hit=True)
    w.close()
    worst, bad, inside_hits = 0.0, [], 0
    for e in range(N):
        for r in range(P):
            ok, res, why = rb.check_answer(scene.world[e], [True] * 4, org32[e, r].astype(np.float64), dr32[e, r].astype(np.float64), max_dist, float(dist[e, r]), int(hit[e, r]), terrains[e])
            worst = max(worst, res)
            if not ok:
                bad.append((e, r, float(dist[e, r]), int(hit[e, r]), why))
            if r % 8 < 4:
                inside_hits += dist[e, r] == 0.0 and hit[e, r] >= 0
    print(f"ray_cast {terrain}: worst residual {worst:.3g} tol, {len(bad)} violations {bad[:4]}")
    lines.append(f"rsb_ray_cast flags BODIES             worst residual {worst:.3e} tol   ({int((hit >= 0).sum())} body hits, {int((hit == TERRAIN).sum())} terrain hits of {N * P} rays, {len(bad)} violations)")
    record(f"1 every shape kind, fixed base + revolute + prismatic, N = 5, F = 2, P = 37, {terrain}", lines)
    assert inside_hits == N * sum(r % 8 < 4 for r in range(P)), inside_hits      # every origin inside a shape gives 0
    assert not failures and not bad, (failures[:10], bad[:10])


# ---- 2. robot models ----------------------------------------------------------------------------------------------------------------------------
def atlas_states(model, N):
    gc, gv = workload.random_state(model.nq, model.nv, N, seed=4, joint_range=0.4)
    rng = np.random.default_rng(12)
    gc[:, 0:2], gc[:, 2] = rng.uniform(-0.5, 0.5, (N, 2)), rng.uniform(0.95, 1.1, N)
    yaw = rng.uniform(-np.pi, np.pi, N)
    gc[:, 3], gc[:, 4:6], gc[:, 6] = np.cos(yaw / 2), rng.uniform(-0.05, 0.05, (N, 2)), np.sin(yaw / 2)
    return gc, gv


@pytest.mark.parametrize("robot", ["anymal", "atlas"])
def test_depth_cameras_on_the_robot_models(robot, anymal, atlas):
    """a 16 x 12 camera on a mast over the base / the head looking down (its own body's shapes count), and one on a shank / a foot looking up"""
    max_dist = 5.0
    down, up = (depth_camera_rays(16, 12, 1.4).astype(np.float64) @ rot("y", np.pi / 2).T).astype(np.float32), (depth_camera_rays(16, 12, 1.0).astype(np.float64) @ rot("y", -np.pi / 2).T).astype(np.float32)
    if robot == "anymal":
        model, N = anymal, 8
        gc, gv = standing_states(N, seed=5)
        cams = [((0, (0.0, 0.0, 0.5)), down), ((model.body_index("LF_SHANK"), (0.05, 0.0, -0.3)), up)]
    else:
        model, N = atlas, 3
        gc, gv = atlas_states(model, N)
        cams = [((model.body_index("head"), (0.0, 0.0, 0.5)), down), ((model.body_index("l_foot"), (0.0, 0.0, 0.05)), up)]
    scene = Scene(model, gc)
    w, terrains = make_world(model, N, "maps")
    w.set_state(gc, gv)
    worst, bad, nb, nt, total = 0.0, [], 0, 0, 0
    for frame, dirs in cams:
        out, hit = w.ray_scan([frame], dirs, max_dist, own_body=True, hit=True)
        a, b, c, d = check_scan(scene, terrains, [frame], dirs, max_dist, out, hit, True, True)
        worst, bad, nb, nt, total = max(worst, a), bad + b, nb + c, nt + d, total + out.size
    w.close()
    print(f"{robot}: worst residual {worst:.3g} tol, {nb} body hits, {nt} terrain hits of {total}, {len(bad)} violations {bad[:4]}")
    record(f"2 {robot}-like, N = {N}, two 16 x 12 cameras, three maps", [f"worst residual {worst:.3e} tol   ({nb} body hits, {nt} terrain hits of {total} rays, {len(bad)} violations)"])
    assert nb >= total / 10 and nt >= total / 10, (nb, nt, total)
    assert not bad, bad[:10]


# ---- 3. rsb_ray_cast and rsb_ray_test -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terrain", ["plane", "maps"])
def test_ray_cast_carries_the_bits_of_ray_test(anymal, terrain):
    N, R, max_dist = 6, 150, 6.0
    o32, d32 = tq.ray_inputs(N, R, hmax=0.2)      # (the maps' heights stay within +- 0.4 cells = 0.2)
    gc, gv = standing_states(N, seed=5)
    scene = Scene(anymal, gc)
    for e in range(N):      # a third of the rays start above the robot and look at one of its shapes
        for r in range(0, R, 3):
            s = scene.world[e][(r // 3) % len(scene.world[e])]
            c = s["centre"] if "centre" in s else 0.5 * (s["a"] + s["b"])
            o32[e, r] = c + [0.3, -0.2, 0.8]
            d32[e, r] = c - o32[e, r].astype(np.float64)
    d32[0, 1], d32[0, 2], o32[0, 4, 1] = [0.0, np.nan, -1.0], [0.0, 0.0, 0.0], np.nan
    w, _ = make_world(anymal, N, terrain)
    w.set_state(gc, gv)
    ref = w.ray_test(o32, d32, max_dist)
    plain, hit0 = w.ray_cast(o32, d32, max_dist, bodies=False, hit=True)
    assert np.array_equal(plain.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(hit0, np.where(ref >= 0, TERRAIN, NONE))
    dist, hit = w.ray_cast(o32, d32, max_dist, hit=True)
    w.close()
    ground = hit == TERRAIN
    assert (hit >= 0).sum() >= N * R // 6 and ground.sum() >= N * R // 6 and (hit == NONE).sum() >= 3
    assert np.array_equal(dist[ground].view(np.uint32), ref[ground].view(np.uint32))
    assert np.array_equal(dist[hit == NONE], ref[hit == NONE]) and np.all(dist[hit == NONE] == -1.0)
    body = hit >= 0
    assert np.all(dist[body] >= 0) and np.all((ref[body] < 0) | (dist[body] < ref[body]))      # a body wins only where it is strictly nearer


# ---- 4. known answers -------------------------------------------------------------------------------------------------------------------------
def test_a_ball_in_closed_form():
    r, N, max_dist = 0.1, 3, 4.0
    model = Model(urdf_string=sphere_urdf(r=r))
    gc = np.zeros((N, 7))
    gc[:, 0], gc[:, 1], gc[:, 2], gc[:, 3] = [0.5, -1.0, 2.0], [0.25, 0.0, -3.0], [1.0, 2.5, 0.75], 1.0
    tol = 1e-5 * (1.0 + max(np.abs(gc[:, :3]).max() + 2.0, max_dist))
    w = BatchedWorld(model, N)
    w.add_ground(0.0)
    w.set_state(gc, np.zeros((N, 6)))
    above = [(0, (0.0, 0.0, 2.0))]
    ang = 0.03
    dirs = np.array([[0, 0, -1.0], [np.sin(ang), 0, -np.cos(ang)], [0, 0, 1.0], [0, 1.0, 0], [0.2, 0, -1.0], [0, 0, 0], [np.nan, 0, -1.0]], np.float32) * 2.5
    out, hit = w.ray_scan(above, dirs, max_dist, own_body=True, hit=True)
    assert np.all(np.abs(out[:, 0, 0] - (2.0 - r)) <= tol) and np.all(hit[:, 0, 0] == 0)      # centrally from above: h - r
    slant = 2.0 * np.cos(ang) - np.sqrt(r * r - (2.0 * np.sin(ang)) ** 2)
    assert np.all(np.abs(out[:, 0, 1] - slant) <= tol) and np.all(hit[:, 0, 1] == 0)
    assert np.all(out[:, 0, 2:4] == -1.0) and np.all(hit[:, 0, 2:4] == NONE) and np.all(out[:, 0, 5:] == -1.0) and np.all(hit[:, 0, 5:] == NONE)
    ground = (gc[:, 2] + 2.0) * np.sqrt(1.04)
    assert np.all(np.where(ground <= max_dist, np.abs(out[:, 0, 4] - ground) <= tol, out[:, 0, 4] == -1.0))
    assert np.all(hit[:, 0, 4] == np.where(ground <= max_dist, TERRAIN, NONE)) and (ground <= max_dist).sum() == 2
    see_through = w.ray_scan(above, dirs, max_dist)      # without OWN_BODY the ball does not see itself: the plane below it
    assert np.all(np.abs(see_through[:, 0, 0] - np.where(gc[:, 2] + 2.0 <= max_dist, gc[:, 2] + 2.0, -1.0)) <= tol)
    # PLANAR: range times the cosine to the body's x axis; the ball is yawed and pitched so that x looks down and sideways
    q = np.array([np.cos(0.35), 0.0, np.sin(0.35), 0.0]) * 1.0
    gc2 = gc.copy()
    gc2[:, 3:7] = q
    w.set_state(gc2, np.zeros((N, 6)))
    cam = depth_camera_rays(5, 3, 1.0)
    rng_, rng_hit = w.ray_scan([(0, (0.0, 0.0, 0.0))], cam, max_dist, hit=True)
    depth = w.ray_scan([(0, (0.0, 0.0, 0.0))], cam, max_dist, planar=True)
    assert (rng_hit == TERRAIN).sum() >= 15 and (rng_hit == NONE).sum() >= 5
    assert np.all(np.abs(depth - np.where(rng_ >= 0, rng_.astype(np.float64) * cam[:, 0].astype(np.float64), -1.0)) <= tol)
    # MISS_MAX: a miss reports max_dist (PLANAR: times the same cosine)
    far = w.ray_scan([(0, (0.0, 0.0, 0.0))], cam, max_dist, miss_max=True)
    far_depth = w.ray_scan([(0, (0.0, 0.0, 0.0))], cam, max_dist, miss_max=True, planar=True)
    assert np.array_equal(far, np.where(rng_hit == NONE, np.float32(max_dist), rng_))
    assert np.all(np.abs(far_depth - far.astype(np.float64) * cam[:, 0]) <= tol)
    # a ray from inside the ball gives 0, whatever its direction
    inside, inside_hit = w.ray_scan([(0, (0.03, -0.02, 0.05))], lidar_rays(8, [-0.5, 0.0, 0.9]), max_dist, own_body=True, hit=True)
    assert np.all(inside == 0.0) and np.all(inside_hit == 0)
    o = (gc2[:, None, :3] + [0.03, -0.02, 0.05]).repeat(4, axis=1).astype(np.float32)
    d, h = w.ray_cast(o, np.tile(np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1.0]], np.float32), (N, 1, 1)), max_dist, hit=True, miss_max=True)
    assert np.all(d == 0.0) and np.all(h == 0)
    up = w.ray_cast((gc2[:, None, :3] + [0, 0, 0.5]).astype(np.float32), np.tile(np.array([[[0, 0, 1.0]]], np.float32), (N, 1, 1)), max_dist, miss_max=True)
    assert np.all(up == np.float32(max_dist))
    w.close()


# ---- 5. composition, strides, limits, memory spaces -------------------------------------------------------------------------------------------
ANYMAL_FRAMES = [("base", (0.3, 0.0, 0.1)), ("LF_SHANK", (0.05, 0.0, -0.3)), ("RH_THIGH", (0.0, -0.1, 0.0))]


def test_ray_scan_is_frame_kinematics_plus_ray_cast(anymal):
    N, max_dist = 7, 4.0
    gc, gv = standing_states(N, seed=8)
    frames = [(anymal.body_index(b), off) for b, off in ANYMAL_FRAMES]
    dirs = np.concatenate([depth_camera_rays(9, 7, 1.3), lidar_rays(12, [-0.6, -0.2]), -lidar_rays(5, [1.2])])
    F, P = len(frames), dirs.shape[0]
    w, _ = make_world(anymal, N, "maps")
    w.set_state(gc, gv)
    out, hit = w.ray_scan(frames, dirs, max_dist, hit=True)
    k = w.frame_kinematics(frames, pos=True, rot=True)
    o = np.repeat(k["pos"][:, :, None, :], P, axis=2).astype(np.float32)
    d = np.einsum("nfij,pj->nfpi", k["rot"].astype(np.float64), dirs.astype(np.float64)).astype(np.float32)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-5
    dist, hit_c = w.ray_cast(o.reshape(N, F * P, 3), d.reshape(N, F * P, 3), max_dist, hit=True)
    dist, hit_c = dist.reshape(N, F, P), hit_c.reshape(N, F, P)
    # ray_cast sees the mount's own shapes, ray_scan does not: compare where the cast did not stop at the frame's own body
    body_of = {int(s["prim"]): s["body"] for s in rb.shapes_of(anymal.blob)}
    own = np.array([[[h >= 0 and body_of[int(h)] == frames[f][0] for h in hit_c[e, f]] for f in range(F)] for e in range(N)])
    tol = 1e-5 * (1.0 + np.maximum(np.abs(o).max(axis=-1), max_dist))
    print(f"composition: max |scan - cast| / tol = {(np.abs(out - dist) / tol)[~own].max():.3g}; {int(own.sum())} rays of the cast stop at the mount")
    assert own.sum() < N * F * P // 4 and (hit >= 0).sum() >= 20
    assert np.all(np.abs(out - dist)[~own] <= tol[~own]) and np.array_equal(hit[~own], hit_c[~own])
    with_own = w.ray_scan(frames, dirs, max_dist, own_body=True)
    assert np.all(np.abs(with_own - dist) <= tol)
    # a frame's scan does not depend on the other frames listed, nor a direction's answer on the other directions
    a, b = frames[1], frames[0]
    both = w.ray_scan([a, b], dirs, max_dist)
    assert np.array_equal(both[:, 0], w.ray_scan([a], dirs, max_dist)[:, 0]) and np.array_equal(both[:, 1], w.ray_scan([b], dirs, max_dist)[:, 0])
    assert np.array_equal(both[:, 0], out[:, 1]) and np.array_equal(both[:, 1], out[:, 0])
    assert np.array_equal(w.ray_scan(frames, dirs[5:40], max_dist), out[:, :, 5:40])
    w.close()


def test_strides_limits_and_memory_spaces(anymal):
    import torch
    dev = torch.device("cuda:0")
    N, max_dist, head = 3, 4.0, 5
    gc, gv = standing_states(N, seed=6)
    frames = [(anymal.body_index(b), off) for b, off in ANYMAL_FRAMES]
    dirs = np.concatenate([depth_camera_rays(11, 7, 1.2) @ rot("y", 0.7).T.astype(np.float32), lidar_rays(6, [-0.9])]).astype(np.float32)      # P = 83
    F, P = len(frames), dirs.shape[0]
    assert (N * F * P) % 64 and P % 2
    w, _ = make_world(anymal, N, "maps")
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    w.set_state(gc, gv)
    out, hit = w.ray_scan(frames, dirs, max_dist, hit=True)
    only_hit = torch.full((N, F, P), 7, dtype=torch.int32, device=dev)      # hit alone: the ranges are not written anywhere
    assert w.ray_scan(frames, torch.from_numpy(dirs).to(dev), max_dist, out={"hit": only_hit}) is only_hit and np.array_equal(only_hit.cpu().numpy(), hit)
    # row_stride on the host: guard columns untouched
    stride = F * P + 7
    buf = np.full((N, stride), -12345.678, np.float32)
    sentinel = buf[0, 0].copy()
    w.ray_scan(frames, dirs, max_dist, out=buf, row_stride=stride)
    assert np.array_equal(buf[:, :F * P].reshape(N, F, P), out) and np.all(buf[:, F * P:].view(np.uint32) == sentinel.view(np.uint32))
    # ... and on the device, into the tail columns of an observation tensor; device pointers follow the stream: a step is enqueued before, nothing synchronises
    obs = torch.full((N, head + F * P), 7.0, dtype=torch.float32, device=dev)
    thit = torch.full((N, F, P), 7, dtype=torch.int32, device=dev)
    tdirs = torch.from_numpy(dirs).to(dev)
    w.integrate(2)
    w.ray_scan(frames, tdirs, max_dist, out={"out": obs[:, head:], "hit": thit}, row_stride=head + F * P)
    after, after_hit = w.ray_scan(frames, dirs, max_dist, hit=True)      # RSB_HOST, the same state
    got = obs.cpu().numpy()
    assert np.all(got[:, :head] == 7.0)
    assert np.array_equal(got[:, head:].reshape(N, F, P).view(np.uint32), after.view(np.uint32)) and np.array_equal(thit.cpu().numpy(), after_hit)
    assert not np.array_equal(after, out)      # the scan follows the state
    o32, d32 = tq.ray_inputs(N, 41, hmax=0.2)
    o32[:, ::2] = (gc[:, None, :3] + [0.4, 0.1, 0.9]).astype(np.float32)
    d32[:, ::2] = np.array([-0.4, -0.1, -0.9], np.float32) + 0.1 * d32[:, ::2]
    tdist = torch.full((N, 41), 7.0, dtype=torch.float32, device=dev)
    tchit = torch.full((N, 41), 7, dtype=torch.int32, device=dev)
    w.ray_cast(torch.from_numpy(o32).to(dev), torch.from_numpy(d32).to(dev), max_dist, out={"dist": tdist, "hit": tchit})
    hdist, hhit = w.ray_cast(o32, d32, max_dist, hit=True)
    assert np.array_equal(tdist.cpu().numpy().view(np.uint32), hdist.view(np.uint32)) and np.array_equal(tchit.cpu().numpy(), hhit) and (hhit >= 0).sum() >= 5
    w.close()
    # the limit itself, N = 2: every direction's answer is the one it has in a short call; grid tails: N * F * P no multiple of anything
    w, _ = make_world(anymal, 2, "plane")
    w.set_state(gc[:2], gv[:2])
    big = np.resize(dirs, (_capi.RSB_MAX_RAY_POINTS, 3))
    full = w.ray_scan([frames[0]], big, max_dist, own_body=True)
    assert full.shape == (2, 1, _capi.RSB_MAX_RAY_POINTS)
    short = w.ray_scan([frames[0]], dirs, max_dist, own_body=True)      # (np.resize repeats the pattern)
    assert np.array_equal(full, np.tile(short, (1, 1, _capi.RSB_MAX_RAY_POINTS // P + 1))[:, :, :_capi.RSB_MAX_RAY_POINTS]) and (short >= 0).any()
    w.close()
    for n in (1, 3):
        w, _ = make_world(anymal, n, "plane")
        w.set_state(gc[:n], gv[:n])
        for fr, pat in ((frames, dirs[:83]), (frames[:2], np.resize(dirs, (521, 3))), (frames, np.resize(dirs, (1031, 3)))):      # one chunk, a chunk and a tail, several chunks
            got = w.ray_scan(fr, pat, max_dist)
            for f, frame in enumerate(fr):
                assert np.array_equal(got[:, f, :83], w.ray_scan([frame], dirs[:83], max_dist)[:, 0]), (n, len(fr), pat.shape)
        w.close()


# ---- 6. world modes ---------------------------------------------------------------------------------------------------------------------------
def test_follows_the_state_in_lockstep_pipelined_and_resident_runs(built_lib):
    """After 5 control steps on standing ANYmals - lock-step, pipelined and resident - the scan and the cast pass the property check on the state
    get_state() returns, the three modes give the same bits, and the queries leave the world as it was bit for bit."""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, K, max_dist = 512, 5, 4.0
    r = bench.Recipe(2, -1.0)
    model = r.model
    gc0, gv0 = standing_states(n, seed=9)
    dev = torch.device("cuda:0")
    bank = torch.from_numpy(np.stack([r.targets(n, k, 0).astype(np.float32) for k in range(K)])).to(dev)
    g0, v0 = torch.from_numpy(gc0.astype(np.float32)).to(dev), torch.from_numpy(gv0.astype(np.float32)).to(dev)
    feet = np.asarray(r.feet, np.int32)
    frames = [(0, (0.0, 0.0, 0.5))]
    dirs = (depth_camera_rays(8, 6, 1.4).astype(np.float64) @ rot("y", np.pi / 2).T).astype(np.float32)
    o32 = (gc0[:, None, :3] + [0.0, 0.0, 1.0]).repeat(3, axis=1).astype(np.float32)
    d32 = np.tile(np.array([[0, 0, -1.0], [0.2, 0.1, -1.0], [1.0, 0, 0.1]], np.float32), (n, 1, 1))
    results = {}
    for mode in ("lockstep", "pipelined", "resident"):
        w = BatchedWorld(model, n)
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        r.setup_world(w, n, 0)
        w.set_state(gc0, gv0)
        w.set_pd_target(None, np.zeros((n, model.nv), np.float32))
        od = w.obs_dim(len(feet))
        obs = torch.zeros((K, n, od), dtype=torch.float32, device=dev)
        if mode == "resident":
            w.set_step_residency(True)
            assert w.residency_status(0)
            w.control_steps_plan(workload.SUBSTEPS, bank.data_ptr(), K, obs.data_ptr(), n * od, feet, feet, g0.data_ptr(), v0.data_ptr(), n)(K, 0)
        else:
            if mode == "pipelined":
                assert w.set_step_pipelining(True) is not False and w.step_pipelining_enabled()
            step = w.control_step_plan(workload.SUBSTEPS, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), n)
            for k in range(K):
                step(bank[k].data_ptr())
        scan, shit = w.ray_scan(frames, dirs, max_dist, own_body=True, hit=True)      # enqueued behind the steps: joins the pipeline / follows the resident launch
        gc, gv = w.get_state()
        counts, contacts = w.get_contacts()
        dist, chit = w.ray_cast(o32, d32, max_dist, hit=True)
        gc2, gv2 = w.get_state()
        counts2, contacts2 = w.get_contacts()
        assert np.array_equal(gc, gc2) and np.array_equal(gv, gv2) and np.array_equal(counts, counts2) and contacts.tobytes() == contacts2.tobytes()
        assert not np.array_equal(gc, gc0.astype(np.float32))
        results[mode] = (scan, shit, dist, chit, gc, gv)
        w.close()
    for mode in ("pipelined", "resident"):
        for a, b in zip(results[mode], results["lockstep"]):
            assert np.array_equal(a, b), mode
    scan, shit, dist, chit, gc, _ = results["lockstep"]
    some = np.arange(0, n, 97)
    scene = Scene(model, gc[some])
    plane = [rb.PlaneTerrain(0.0)] * len(some)      # (the flat terrain of the benchmark's config 2)
    worst, bad, nb, nt = check_scan(scene, plane, frames, dirs, max_dist, scan[some], shit[some], True, True)
    print(f"after 5 control steps: worst residual {worst:.3g} tol, {nb} body hits, {nt} terrain hits, {len(bad)} violations {bad[:4]}")
    assert not bad and nb >= 10 and nt >= 10, bad[:10]
    for i, e in enumerate(some):
        for k in range(3):
            ok, res, why = rb.check_answer(scene.world[i], [True] * len(scene.shapes), o32[e, k].astype(np.float64), d32[e, k].astype(np.float64), max_dist, float(dist[e, k]), int(chit[e, k]), plane[i])
            assert ok, (e, k, float(dist[e, k]), int(chit[e, k]), why)
    assert (chit == TERRAIN).sum() >= n and (chit == NONE).sum() >= n // 2      # two rays look down, one up and away


def test_the_world_is_left_bit_for_bit(anymal):
    N = 16
    gc, gv = standing_states(N, seed=3)
    w, _ = make_world(anymal, N, "maps")
    w.set_state(gc, gv)
    w.integrate(4)
    before = (*w.get_state(), *[np.asarray(a).tobytes() for a in w.get_contacts()])
    dirs = lidar_rays(16, [-0.8, -0.3, 0.2])
    for kw in (dict(), dict(own_body=True, planar=True, miss_max=True), dict(bodies=False)):
        w.ray_scan([(0, (0.0, 0.0, 0.3)), (3, (0.0, 0.0, 0.0))], dirs, 3.0, hit=True, **kw)
    o32, d32 = tq.ray_inputs(N, 20, hmax=0.2)
    w.ray_cast(o32, d32, 3.0, hit=True)
    after = (*w.get_state(), *[np.asarray(a).tobytes() for a in w.get_contacts()])
    w.integrate(4)
    q1, u1 = w.get_state()
    w.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    w2, _ = make_world(anymal, N, "maps")      # ... and steps on as a world that was never asked
    w2.set_state(gc, gv)
    w2.integrate(4)
    w2.integrate(4)
    q2, u2 = w2.get_state()
    w2.close()
    assert np.array_equal(q1, q2) and np.array_equal(u1, u2)


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(anymal, built_lib):
    L = built_lib
    N = 2
    w = BatchedWorld(anymal, N)
    w.add_ground(0.0)
    buf = np.zeros(N * 4200 * 3, np.float32)
    out = np.full(N * 4200, 5.0, np.float32)
    hit = np.full(N * 4200, 5, np.int32)
    p, q, h = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), hit.ctypes.data_as(C.c_void_p)
    fr = (_capi.Frame * 2)()
    bad = (_capi.Frame * 1)()
    bad[0].body = anymal.nb
    nan = (_capi.Frame * 1)()
    nan[0].offset[1] = float("nan")
    H = w.handle
    cases = [
        lambda: L.rsb_ray_cast(None, p, p, 4, 1.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, 1, q, h, 2),
        lambda: L.rsb_ray_cast(H, None, p, 4, 1.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, None, 4, 1.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, 1, None, None, 0),
        lambda: L.rsb_ray_cast(H, p, p, 0, 1.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 0.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, -1.0, 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, float("inf"), 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, float("nan"), 1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, 16, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, -1, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, _capi.RSB_RAY_BODIES | _capi.RSB_RAY_OWN_BODY, q, h, 0),
        lambda: L.rsb_ray_cast(H, p, p, 4, 1.0, _capi.RSB_RAY_PLANAR, q, h, 0),
        lambda: L.rsb_ray_scan(None, fr, 1, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 1, 1.0, q, 0, h, 3),
        lambda: L.rsb_ray_scan(H, None, 1, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 0, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, _capi.RSB_MAX_FRAMES + 1, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, bad, 1, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, nan, 1, p, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, None, 4, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 1, 1.0, None, 0, None, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 0, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, _capi.RSB_MAX_RAY_POINTS + 1, 1, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 1, 0.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 1, float("inf"), q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 1, float("nan"), q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 1, p, 4, 16, 1.0, q, 0, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 2, p, 4, 1, 1.0, q, 7, h, 0),
        lambda: L.rsb_ray_scan(H, fr, 2, p, 4, 1, 1.0, q, -1, h, 0),
    ]
    for k, call in enumerate(cases):
        assert call() == -1, k      # RSB_E_INVALID
        msg = L.rsb_last_error()
        assert len(msg) > 15 and (b"rsb_ray_cast" in msg or b"rsb_ray_scan" in msg), (k, msg)
    assert np.all(out == 5.0) and np.all(hit == 5)      # nothing was launched
    # every flag bit and the limits themselves are accepted
    pat = np.zeros((_capi.RSB_MAX_RAY_POINTS, 3), np.float32)
    pat[:, 2] = -1.0
    assert w.ray_scan([0], pat, 2.0, own_body=True, planar=True, miss_max=True).shape == (N, 1, _capi.RSB_MAX_RAY_POINTS)
    assert w.ray_scan([0] * _capi.RSB_MAX_FRAMES, pat[:3], 2.0).shape == (N, _capi.RSB_MAX_FRAMES, 3)
    w.close()
