"""The device's sphere x height-map narrow phase (step_terrain.h, the height-map branch of step_phase_collision.inc) DIRECTLY against the
independent brute force of tests/terrain_reference.py - not against the oracle, which is the same algorithm line for line.

One world = one 24-sphere rake, N = 64 envs, three maps (env_map = e % 3; the maps are one terrain at three levels, each env's pose shifted with
its map, so an env that reads another map's heights is off by >= 0.125 m) and four poses ((e // 3) % 4: the designed one, and up to three
moved by whole cells and a little in z, so the envs of one wave differ in which spheres are near and which touch).  rsb_get_contacts() after
integrate(1) at zero gravity and velocity: the contacts detected at the state that was set.  16, 32 and 64 lanes per env; 16 contact slots.

Bars.  tie = 2^-18: the candidate key keeps 18 mantissa bits of the squared distance, the scan position ranks what is equal in those.
bar = 3e-6 m: what tests/test_gpu_kat.py uses for this narrow phase at coordinates within +-3 m (fp32: 2.4e-7 per coordinate and a handful of
operations).  |normal| = 1 to 1e-6 (8 ulp).  A floor() of the window rule within 1e-4 of an integer is a
tie in fp32 (coordinates of 3 m over a cell of 0.09 m: 1e-5 grid units).  At most 1 % of the placements may be excluded.
The worst value per quantity, regime and lane mapping goes to profiles/terrain_contact_parity.txt."""
import os

import numpy as np
import pytest

import terrain_reference as tr
from common import ROOT
from raisimlib_amd import BatchedWorld, Model

pytestmark = pytest.mark.gpu

N, LANES = 64, (16, 32, 64)
TIE, BAR, UNIT, FLOOR = 2.0 ** -18, 3e-6, 1e-6, 1e-4
SHIFTS = (0.0, 0.25, -0.125)
TALLY = {lpe: tr.Tally() for lpe in LANES}
FAMILY_COUNT = np.zeros(len(tr.FAMILIES), int)
SECTIONS = {}
DONE = set()


def once(key, sweep, *args):
    """every sweep feeds the tallies exactly once, whichever tests of this file run and in whichever order"""
    if key not in DONE:
        sweep(*args)
        DONE.add(key)


def write_report():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "terrain_contact_parity.txt"), "w") as f:
        f.write("tests/test_gpu_terrain_contact.py: worst value per quantity, device fp32 vs the fp64 brute force of tests/terrain_reference.py on the\n"
                f"float32-rounded state (bars: off-mesh and distance excess {BAR:g} m with tie {TIE:.3g}, |n| - 1 {UNIT:g}; excluded share <= 1 %)\n")
        for lpe in LANES:
            f.write(f"first contacts, {lpe} lanes per env\n" + "".join(f"  {l}\n" for l in TALLY[lpe].lines()))
        for name in sorted(SECTIONS):
            f.write(f"{name}\n" + "".join(f"  {l}\n" for l in SECTIONS[name]))


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def rake_world(model, grids, geom, env_map, q, lpe):
    w = BatchedWorld(model, N)
    w.set_gravity([0.0, 0.0, 0.0])
    w.set_max_contacts(16)
    w.set_lanes_per_env(lpe)
    w.add_height_maps(np.stack([g.h32 for g in grids]), *geom[2:], env_map)
    w.set_state(q, np.zeros((N, 6)))
    return w


def first_contacts(con, cnt):
    """one env's list -> per-primitive arrays of the first contacts, matched by the collision id; asserts primitive order"""
    c = con[:cnt]
    ids = c["collision"]
    assert (ids < 0x10000).all() and (np.diff(ids) > 0).all(), ids
    rep = np.zeros(tr.N_SPHERES, bool); pos = np.zeros((tr.N_SPHERES, 3)); nrm = np.zeros((tr.N_SPHERES, 3)); dep = np.zeros(tr.N_SPHERES)
    rep[ids] = True; pos[ids] = c["position"]; nrm[ids] = c["normal"]; dep[ids] = c["depth"]
    return rep, pos, nrm, dep


def run_design(base, geom, d, rng, label):
    """one rake on the three levels of `base`, all three lane mappings; -> number of distinct poses among the four"""
    grids = [tr.Grid(base.h + s, *geom[2:]) for s in SHIFTS]
    model = Model(urdf_string=tr.rake_urdf(d.offsets, d.radii))
    off, rad = f32(d.offsets), f32(d.radii)
    poses = [d.q]
    for _ in range(3):
        v = tr.variant_pose(base, d, rng, off, rad, BAR, FLOOR)
        poses.append(d.q if v is None else v)
    env_map = (np.arange(N) % 3).astype(np.int32)
    pose_of = (np.arange(N) // 3) % 4
    q = np.array([poses[j] for j in pose_of])
    q[:, 2] += np.array(SHIFTS)[env_map]
    q = q.astype(np.float32)
    assert np.abs(q[:, :3]).max() <= 3.0
    ids_by_lanes = []
    exact = np.arange(tr.N_SPHERES) == 0
    for lpe in LANES:
        w = rake_world(model, grids, geom, env_map, q, lpe)
        w.integrate(1)
        cnt, con = w.get_contacts()
        flags = w.get_flags()
        w.close()
        assert (flags & 3 == 0).all(), (label, lpe, flags)
        ids_by_lanes.append([tuple(con[e][:cnt[e]]["collision"]) for e in range(N)])
        groups = {}
        for e in range(N):
            groups.setdefault((int(pose_of[e]), int(env_map[e])), []).append(e)
        for (j, m), envs in sorted(groups.items()):
            e0 = envs[0]
            for e in envs[1:]:      # envs sharing a pose and a map: bit-identical
                assert cnt[e] == cnt[e0] and con[e][:cnt[e]].tobytes() == con[e0][:cnt[e0]].tobytes(), (label, lpe, e0, e)
            c = tr.sphere_centres(q[e0].astype(np.float64), off)
            v = tr.verdict(grids[m], c, rad, *first_contacts(con[e0], cnt[e0]), tie=TIE, bar=BAR, unit_tol=UNIT, exact=exact, floor_margin=FLOOR)
            TALLY[lpe].add(v, f"{label} lanes {lpe} pose {j} map {m} env {e0}")
            if not v["excluded"].any():
                assert cnt[e0] == v["ref_hit"].sum() <= 16, (label, lpe, e0, cnt[e0], v["ref_hit"].sum())
    assert ids_by_lanes[0] == ids_by_lanes[1] == ids_by_lanes[2], label      # the three lane mappings report the same contacts
    np.add.at(FAMILY_COUNT, d.family, 1)
    return len(set(map(tuple, poses)))


def no_failures(f0):
    for lpe in LANES:
        assert len(TALLY[lpe].failures) == f0[lpe], TALLY[lpe].failures[f0[lpe]:f0[lpe] + 10]


def failures_now():
    return {lpe: len(TALLY[lpe].failures) for lpe in LANES}


MODES = ("interior", "edge", "on_border", "interior")
CASES = [("9x7", (9, 7, 4.0, 2.25, 0.25, -0.125), (0.04, 0.30), 8, False),
         ("2x2", (2, 2, 0.5, 0.375, 0.25, -0.125), (0.04, 0.30), 3, False),
         ("2x5", (2, 5, 0.5, 1.5, -0.25, 0.125), (0.04, 0.30), 3, False),
         ("33x33", (33, 33, 4.0, 4.0, 0.25, -0.25), (0.04, 0.125), 2, False),
         ("33x33 r = 1.2 cells", (33, 33, 3.0, 3.0, 0.25, -0.25), (1.2 * 3.0 / 32,) * 2, 4, True),
         ("33x33 r = 2.5 cells", (33, 33, 3.0, 3.0, 0.25, -0.25), (2.5 * 3.0 / 32,) * 2, 4, True)]


@pytest.mark.parametrize("name,geom,radii,count,big", CASES, ids=[c[0] for c in CASES])
def test_first_contacts_against_the_brute_force(built_lib, name, geom, radii, count, big):
    """every amplitude (0.05, 0.3, 0.8 x cell) x `count` rakes; r <= cell against the whole mesh, r > cell against the documented window"""
    once(name, sweep_first, name, geom, radii, count, big)


def sweep_first(name, geom, radii, count, big):
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    f0 = failures_now()
    distinct = 0
    for a, amp in enumerate((0.05, 0.3, 0.8)):
        base = tr.random_map(*geom, amplitude=amp, seed=500 + 10 * a + len(name))
        for k in range(count):
            mode = ("interior", "edge")[(a + k) % 2] if big else MODES[(a + k) % 4]
            d = tr.design_rake(base, rng, *radii, mode=mode, generic_only=big)
            distinct += run_design(base, geom, d, rng, f"{name} amp {amp} rake {k}")
    assert distinct >= 2 * 3 * count      # the whole-cell variants exist: the envs of a wave do differ
    write_report()
    no_failures(f0)


def test_beyond_the_border_of_the_wall_map(built_lib):
    """5 x 5 samples over 2 m x 2 m, flat except a last column 1.5 m high: spheres beyond that border whose lowest point is above the map's highest
    sample report nothing, lower ones meet the level surface z = 1.5 with normal z; the rake around its borders and corners"""
    once("wall", sweep_wall)


def sweep_wall():
    grid = tr.wall_map()
    geom = (5, 5, 2.0, 2.0, 0.0, 0.0)
    model = Model(urdf_string=tr.rake_urdf(np.zeros((1, 3)), [0.2]))
    zs = np.array([1.5 + 0.2 + 0.1, 1.5 + 0.2 + 0.3, 1.5 + 0.2 - 0.05, 1.5 - 0.1])
    want = np.array([0.0, 0.0, 0.05, 0.3])
    q = np.zeros((N, 7), np.float32); q[:, 3] = 1.0
    q[:, 0], q[:, 1], q[:, 2] = 1.1, np.array([0.3, -0.5, 1.2, -1.3])[np.arange(N) % 4], zs[(np.arange(N) // 4) % 4]
    w = BatchedWorld(model, N)
    w.set_gravity([0.0, 0.0, 0.0]); w.add_height_map(*grid.args()); w.set_state(q, np.zeros((N, 6))); w.integrate(1)
    cnt, con = w.get_contacts()
    w.close()
    wd = want[(np.arange(N) // 4) % 4]
    assert np.array_equal(cnt, (wd > 0).astype(cnt.dtype)), cnt
    hit = wd > 0
    assert np.abs(con[hit, 0]["depth"] - wd[hit]).max() <= BAR and (con[hit, 0]["normal"] == np.array([0, 0, 1], np.float32)).all()
    rng = np.random.default_rng(6)
    f0 = failures_now()
    for k in range(3):
        d = tr.design_rake(grid, rng, 0.04, 0.30, mode=("edge", "on_border")[k % 2], raised_gap=(0.1, 0.3))
        run_design(grid, geom, d, rng, f"wall map rake {k}")
    write_report()
    no_failures(f0)


# ---- the second flank -------------------------------------------------------------------------------------------------------------------------
def flank_maps(which):
    if which == "rough":
        return tr.random_map(13, 11, 3.0, 2.5, 0.25, -0.25, amplitude=0.5, seed=21), (0.9 * 0.25, 0.25)
    return tr.corrugated_map(which), (0.12, 0.25)


@pytest.mark.parametrize("angle_deg", [45.0, 26.0])
@pytest.mark.parametrize("which", ["x", "y", "diag", "rough"])
def test_second_flank_against_the_brute_force(built_lib, which, angle_deg):
    """rsb_set_heightmap_contacts(2, angle): V-valleys one cell apart along x, along y and along the diagonals (flanks 62 deg apart), and a rough map
    at r ~ cell.  8 of the rake's spheres may touch (8 + 8 contacts fill the 16 slots), 16 are raised; first contacts by the first-contact verdict,
    second ones by tr.second_flank_verdict with the device's own first normal."""
    from raisimlib_amd._capi import RSB_CONTACT_SECOND
    grid, radii = flank_maps(which)
    geom = (grid.xs, grid.ys, grid.xsize, grid.ysize, grid.cx, grid.cy)
    rng = np.random.default_rng(int(angle_deg) + len(which))
    low = lambda i: i % 3 != 0      # noqa: E731
    tally = tr.Tally()
    n = n_excl = n_second = 0
    worst = dict(e_mesh=0.0, e_excess=0.0, e_point=0.0)
    failures = []
    for k in range(3):
        d = tr.design_rake(grid, rng, *radii, mode="interior", generic_only=True, raised_fn=low, allow_below=False, clearance=(0.3, 0.98))
        model = Model(urdf_string=tr.rake_urdf(d.offsets, d.radii))
        off, rad = f32(d.offsets), f32(d.radii)
        poses = [d.q]
        for _ in range(3):
            v = tr.variant_pose(grid, d, rng, off, rad, BAR, FLOOR, max_hits=8, regime0_only=True)
            poses.append(d.q if v is None else v)
        pose_of = np.arange(N) % 4
        q = np.array([poses[j] for j in pose_of]).astype(np.float32)
        ids_by_lanes = []
        for lpe in LANES:
            w = BatchedWorld(model, N)
            w.set_gravity([0.0, 0.0, 0.0]); w.set_max_contacts(16); w.set_lanes_per_env(lpe)
            w.add_height_map(*grid.args())
            w.set_heightmap_contacts(2, angle_deg)
            w.set_state(q, np.zeros((N, 6))); w.integrate(1)
            cnt, con = w.get_contacts(); flags = w.get_flags()
            w.close()
            assert (flags & 3 == 0).all(), (which, lpe, flags)
            ids_by_lanes.append([tuple(con[e][:cnt[e]]["collision"]) for e in range(N)])
            for j in range(4):
                e0 = j
                for e in range(j + 4, N, 4):
                    assert cnt[e] == cnt[e0] and con[e][:cnt[e]].tobytes() == con[e0][:cnt[e0]].tobytes(), (which, lpe, e0, e)
                ce = con[e0][:cnt[e0]]
                sec = (ce["collision"] & RSB_CONTACT_SECOND) != 0
                nf = int((~sec).sum())
                assert not sec[:nf].any() and sec[nf:].all() and (np.diff(ce["collision"][nf:]) > 0).all()      # all first contacts, then the second ones, each in primitive order
                c = tr.sphere_centres(q[e0].astype(np.float64), off)
                rep, pos, nrm, dep = first_contacts(ce, nf)
                v1 = tr.verdict(grid, c, rad, rep, pos, nrm, dep, tie=TIE, bar=BAR, unit_tol=UNIT, floor_margin=FLOOR)
                tally.add(v1, f"second flank {which} {angle_deg} rake {k} lanes {lpe} pose {j}")
                ids2 = ce["collision"][nf:] & 0xffff
                rep2 = np.zeros(tr.N_SPHERES, bool); pos2 = np.zeros((tr.N_SPHERES, 3)); nrm2 = np.zeros((tr.N_SPHERES, 3)); dep2 = np.zeros(tr.N_SPHERES)
                rep2[ids2] = True; pos2[ids2] = ce["position"][nf:]; nrm2[ids2] = ce["normal"][nf:]; dep2[ids2] = ce["depth"][nf:]
                assert not (rep2 & ~rep).any()
                v2 = tr.second_flank_verdict(grid, c, rad, rep, nrm, rep2, pos2, nrm2, dep2, np.radians(angle_deg), TIE, BAR, UNIT)
                n += tr.N_SPHERES; n_excl += int((v2["excluded"] | v1["excluded"]).sum()); n_second += int(rep2.sum())
                for key in worst:
                    worst[key] = max(worst[key], float(v2[key].max()))
                failures += [(which, angle_deg, k, lpe, j, int(i), v2["why"][i]) for i in np.nonzero(v2["bad"] & ~v2["excluded"])[0]]
        assert ids_by_lanes[0] == ids_by_lanes[1] == ids_by_lanes[2]
    SECTIONS[f"second flank, {which}, min angle {angle_deg:g} deg (all lane mappings)"] = [
        f"n = {n} placements, {n_second} second contacts, excluded {n_excl}  off-mesh {worst['e_mesh']:.2e}  distance excess {worst['e_excess']:+.2e}  "
        f"from the qualifying triangle's closest point {worst['e_point']:.2e}"] + tally.lines()[:1]
    write_report()
    print(SECTIONS[f"second flank, {which}, min angle {angle_deg:g} deg (all lane mappings)"])
    assert not tally.failures, tally.failures[:10]
    assert not failures, failures[:10]
    assert n_second >= 20 and n_excl <= 0.01 * n, (n_second, n_excl, n)


# ---- the capsule's barrel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("along", ["y", "x"])
def test_capsule_barrel_against_the_sampled_brute_force(built_lib, along):
    """rsb_set_capsule_contacts: the 0.6 m capsule of test_capsule_lying_across_a_ridge_rests_on_its_cylinder across one straight tent ridge (one
    dip), 32 random yaws, tilts and offsets (two envs each).  Reference: 4001 samples of the axis through the brute force -> d*.  A reported barrel
    contact has its centre on the axis segment, its terrain point on the mesh and d* - 0.013 L <= depth <= d* + bar (0.013 L: the search's final
    sample spacing; distance is 1-Lipschitz); it IS reported whenever d* exceeds both end depths by 1e-4 + 0.013 L, and never when d* <= -bar."""
    from raisimlib_amd._capi import RSB_CONTACT_CAPSULE
    from test_oracle_kat import LOG_URDF
    grid = tr.ridge_map(along, xs=7 if along == "y" else 5, ys=5 if along == "y" else 7)      # (48 triangles: 32 x 4001 samples go through all of them)
    model = Model(urdf_string=LOG_URDF)
    b = model.blob
    assert b.ncol == 2
    ends, r = f32(np.array([list(b.col_pos[i]) for i in range(2)])), float(np.float32(b.col_radius[0]))
    L = float(np.linalg.norm(ends[1] - ends[0]))
    rng = np.random.default_rng(3 if along == "y" else 4)
    q = np.zeros((N, 7), np.float32)
    for j in range(32):
        yaw = rng.uniform(-0.6, 0.6) + (np.pi if j % 2 else 0.0) + (np.pi / 2 if along == "x" else 0.0)
        pitch = rng.uniform(-0.12, 0.12)
        qy, qp = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]), np.array([np.cos(pitch / 2), 0, np.sin(pitch / 2), 0])
        quat = np.array([qy[0] * qp[0], -qy[3] * qp[2], qy[0] * qp[2], qy[3] * qp[0]])
        axis = tr.quat_to_rot(quat)[:, 0]
        s = rng.uniform(-0.22, 0.22)                                       # where along the capsule the ridge line passes under it
        pen = rng.uniform(5e-4, 2e-2) if j % 8 else -rng.uniform(1e-3, 1e-2)      # (every 8th hovers above the ridge)
        cross = np.array([0.0, rng.uniform(-0.15, 0.15), 0.15 + r - pen]) if along == "y" else np.array([rng.uniform(-0.15, 0.15), 0.0, 0.15 + r - pen])
        q[2 * j] = q[2 * j + 1] = np.r_[cross - s * axis, quat]
    w = BatchedWorld(model, N)
    w.set_gravity([0.0, 0.0, 0.0]); w.set_max_contacts(16)
    w.add_height_map(*grid.args())
    w.set_capsule_contacts(True)
    w.set_state(q, np.zeros((N, 6))); w.integrate(1)
    cnt, con = w.get_contacts(); flags = w.get_flags()
    w.close()
    assert (flags & 3 == 0).all()
    slack = 0.013 * L
    n_rep = n_must = 0
    worst = dict(axis=0.0, mesh=0.0, above=-1.0, below=-1.0)
    for j in range(32):
        e = 2 * j
        assert cnt[e] == cnt[e + 1] and con[e][:cnt[e]].tobytes() == con[e + 1][:cnt[e]].tobytes()
        qe = q[e].astype(np.float64)
        a, bb = tr.sphere_centres(qe, ends)
        dstar, da, db = tr.capsule_reference(grid, a, bb, r)
        ce = con[e][:cnt[e]]
        barrel = ce[(ce["collision"] & RSB_CONTACT_CAPSULE) != 0]
        assert len(barrel) <= 1 and (len(ce) == 0 or len(barrel) == 0 or ce["collision"][-1] == barrel["collision"][0])
        must = dstar > max(da, db, 0.0) + 1e-4 + slack
        n_must += must
        if must:
            assert len(barrel) == 1, (along, j, dstar, da, db)
        if dstar <= -BAR:
            assert len(barrel) == 0, (along, j, dstar)
        if len(barrel):
            n_rep += 1
            c = barrel[0]
            assert c["collision"] == (0 | RSB_CONTACT_CAPSULE)
            pos, nrm, dep = c["position"].astype(np.float64), c["normal"].astype(np.float64), float(c["depth"])
            assert abs(np.linalg.norm(nrm) - 1.0) <= UNIT
            e_axis = float(tr.point_segment_distance(pos + r * nrm, a, bb))
            e_mesh = float(grid.closest((pos + dep * nrm)[None])[0][0])
            worst = dict(axis=max(worst["axis"], e_axis), mesh=max(worst["mesh"], e_mesh), above=max(worst["above"], dep - dstar), below=max(worst["below"], dstar - dep))
            assert e_axis <= BAR and e_mesh <= BAR, (along, j, e_axis, e_mesh)
            assert dstar - slack <= dep <= dstar + BAR, (along, j, dep, dstar, slack)
    SECTIONS[f"capsule barrel, ridge along {along} (32 poses)"] = [
        f"{n_rep} barrel contacts ({n_must} had to be there): centre off the axis {worst['axis']:.2e}, terrain point off the mesh {worst['mesh']:.2e}, "
        f"depth - d* <= {worst['above']:+.2e} (bar {BAR:g}), d* - depth <= {worst['below']:.2e} (allowed {slack:.2e})"]
    print(SECTIONS[f"capsule barrel, ridge along {along} (32 poses)"])
    write_report()
    assert n_must >= 10 and n_rep >= n_must


def test_the_sweep_as_a_whole(built_lib):
    """over all first-contact sweeps of this file (those that have not run yet run here): every family and regime was there in every lane
    mapping; <= 1 % excluded"""
    for case in CASES:
        once(case[0], sweep_first, *case)
    once("wall", sweep_wall)
    for lpe in LANES:
        t = TALLY[lpe]
        print(f"{lpe} lanes per env"); [print(" ", l) for l in t.lines()]
        assert t.n.sum() >= 5000 and (t.n >= 100).all() and (t.hits >= 50).all(), (lpe, t.n, t.hits)
        assert t.excluded_share() <= 0.01, (lpe, t.excluded_share())
        assert not t.failures, t.failures[:10]
    print(dict(zip(tr.FAMILIES, FAMILY_COUNT.tolist())))
    assert (FAMILY_COUNT[:7] >= 10).all() and FAMILY_COUNT[7] >= 5, FAMILY_COUNT      # (only the sphere at the base position can sit ON the border)
    write_report()
