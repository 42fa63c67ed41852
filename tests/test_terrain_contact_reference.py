"""The oracle's sphere x height-map narrow phase (oracle/rsb_oracle.c, terrain_contact_ex) against the independent brute force of
tests/terrain_reference.py: Oracle.step's contact list of the 24-sphere rake, at the state that was set (gravity and velocity zero), over every
placement family, map and regime the reference's docstring names.

Bars.  tie = 2e-6: the oracle ranks equally close features by scan order, a later candidate must be closer by 4e-6 in SQUARED distance, so the
reported feature may be farther than the closest one by a factor 1 + 2e-6.  bar = 1e-9 m: fp64 on coordinates of a few metres leaves ~1e-15; 1e-9
is far above that and far below any feature of the maps.  |normal| = 1 to 1e-12.  At most 1 % of the placements may be excluded."""
import numpy as np
import pytest

import terrain_reference as tr
from common import Oracle
from raisimlib_amd import Model

TIE, BAR, UNIT = 2e-6, 1e-9, 1e-12
TALLY = tr.Tally()
FAMILY_COUNT = np.zeros(len(tr.FAMILIES), int)
BELOW_COUNT = [0]
CLEARANCE = []
DONE = set()


def once(key, sweep, *args):
    """every sweep feeds the tallies exactly once, whichever tests of this file run and in whichever order"""
    if key not in DONE:
        sweep(*args)
        DONE.add(key)


def oracle_for(model, grid=None):
    o = Oracle(model.blob)
    o.p.gravity[0] = o.p.gravity[1] = o.p.gravity[2] = 0.0
    o.p.kmax = 16
    if grid is not None:
        o.set_heightmap(*grid.args())
    return o


def blob_spheres(model):
    b = model.blob
    assert b.ncol == tr.N_SPHERES
    return np.array([list(b.col_pos[i]) for i in range(b.ncol)]), np.array([b.col_radius[i] for i in range(b.ncol)])


def by_primitive(con, ncol=tr.N_SPHERES):
    """the contact list -> per-primitive arrays, matched by the collision id; also: ids ascending (primitive order)"""
    ids = con["collision"]
    assert (ids < 0x10000).all() and (np.diff(ids) > 0).all(), ids
    rep = np.zeros(ncol, bool); pos = np.zeros((ncol, 3)); nrm = np.zeros((ncol, 3)); dep = np.zeros(ncol)
    rep[ids] = True; pos[ids] = con["position"]; nrm[ids] = con["normal"]; dep[ids] = con["depth"]
    return rep, pos, nrm, dep


def check_design(d, grid, label):
    model = Model(urdf_string=tr.rake_urdf(d.offsets, d.radii))
    off, rad = blob_spheres(model)
    assert np.array_equal(off, d.offsets) and np.array_equal(rad, d.radii)      # the URDF round-trips the doubles
    q = d.q.copy(); q[3:7] /= np.linalg.norm(q[3:7])
    o = oracle_for(model, grid)
    _, _, con, _, flags = o.step(q, np.zeros(6))
    assert flags & 3 == 0, (label, flags)
    c = tr.sphere_centres(q, off)
    v = tr.verdict(grid, c, rad, *by_primitive(con), tie=TIE, bar=BAR, unit_tol=UNIT, exact=np.arange(tr.N_SPHERES) == 0)
    raised = np.array([tr.is_raised(i) for i in range(tr.N_SPHERES)])
    assert not v["ref_hit"][raised].any() and (c[raised, 2] - rad[raised] > grid.hmax).all()      # the rake's own promise: at most 16 can touch
    TALLY.add(v, label)
    np.add.at(FAMILY_COUNT, d.family, 1)
    BELOW_COUNT[0] += int(d.below.sum())
    h, _, _ = grid.under(c[:, 0], c[:, 1])
    CLEARANCE.extend(((c[:, 2] - h) / rad)[~raised & ~d.below])
    return v


MODES = ("interior", "interior", "edge", "on_border")
# (name, map constructor arguments (xs, ys, xsize, ysize, cx, cy), radii, designs per amplitude): sizes and centres are dyadic, the grid is exact in float32
SMALL_R = [("9x7", (9, 7, 4.0, 2.25, 0.25, -0.125), (0.04, 0.30), 84),
           ("2x2", (2, 2, 0.5, 0.375, 0.25, -0.125), (0.04, 0.30), 12),
           ("2x5", (2, 5, 0.5, 1.5, -0.25, 0.125), (0.04, 0.30), 12),
           ("33x33", (33, 33, 4.0, 4.0, 0.25, -0.25), (0.04, 0.125), 14)]


@pytest.mark.parametrize("name,geom,radii,count", SMALL_R, ids=[s[0] for s in SMALL_R])
def test_spheres_no_larger_than_a_cell_against_the_whole_mesh(built_lib, name, geom, radii, count):
    once(name, sweep_small, name, geom, radii, count)


def sweep_small(name, geom, radii, count):
    rng = np.random.default_rng(sum(map(ord, name)))
    n0, f0 = TALLY.n.sum(), len(TALLY.failures)
    for a, amp in enumerate((0.05, 0.3, 0.8)):
        grid = tr.random_map(*geom, amplitude=amp, seed=100 * a + len(name))
        assert radii[1] <= min(grid.dx, grid.dy)
        for k in range(count):
            d = tr.design_rake(grid, rng, *radii, mode=MODES[k % 4])
            check_design(d, grid, f"{name} amp {amp} design {k}")
    assert TALLY.n.sum() - n0 == 3 * count * tr.N_SPHERES
    assert len(TALLY.failures) == f0, TALLY.failures[f0:f0 + 10]


@pytest.mark.parametrize("ratio", [1.2, 2.5])
def test_spheres_larger_than_a_cell_against_the_documented_window(built_lib, ratio):
    """33 x 33 samples, cell 3/32 m; r = ratio x cell; generic placements (a floor() of the window rule on an integer is a tie and excluded)"""
    once(ratio, sweep_window, ratio)


def sweep_window(ratio):
    rng = np.random.default_rng(int(10 * ratio))
    f0 = len(TALLY.failures)
    for a, amp in enumerate((0.05, 0.3, 0.8)):
        grid = tr.random_map(33, 33, 3.0, 3.0, 0.25, -0.25, amplitude=amp, seed=40 + a)
        r = ratio * grid.dx
        for k in range(12):
            d = tr.design_rake(grid, rng, r, r, mode=("interior", "edge")[k % 2], generic_only=True)
            v = check_design(d, grid, f"r/cell {ratio} amp {amp} design {k}")
            assert (v["regime"][v["regime"] <= 1] == 1).all()
    assert len(TALLY.failures) == f0, TALLY.failures[f0:f0 + 10]


def test_beyond_the_border_of_the_wall_map(built_lib):
    """The convention beyond the footprint, beside a steep border cell: 5 x 5 samples over 2 m x 2 m, flat except a last column 1.5 m high.  A sphere
    0.1 m beyond that border whose lowest point is above the map's highest sample reports nothing (the outermost triangle's tilted plane, continued
    outwards, once gave depths of +0.105 and +0.042 there); lower ones meet the level surface z = 1.5 with normal z; depth is continuous across
    the flat borders."""
    once("wall", sweep_wall)


def sweep_wall():
    grid = tr.wall_map()
    f0 = len(TALLY.failures)
    model = Model(urdf_string=tr.rake_urdf(np.zeros((1, 3)), [0.2]))
    o = oracle_for(model, grid)
    for z, want in ((1.5 + 0.2 + 0.1, None), (1.5 + 0.2 + 0.3, None), (1.5 + 0.2 - 0.05, 0.05), (1.5 - 0.1, 0.3)):
        for y in (0.3, -0.5, 1.2, -1.3):
            _, _, con, _, _ = o.step([1.1, y, z, 1, 0, 0, 0], np.zeros(6))
            if want is None:
                assert len(con) == 0, (z, y, con)
            else:
                assert len(con) == 1 and abs(con[0]["depth"] - want) < 1e-12 and np.array_equal(con[0]["normal"], [0, 0, 1]), (z, y, con)
    for x_in, x_out, y in ((-1.0, -1.000001, 0.3), (0.3, 0.3, -1.0)):      # across the flat near borders: depth 0.1 on both sides
        d_in = o.step([x_in, y, 0.1, 1, 0, 0, 0], np.zeros(6))[2]
        d_out = o.step([x_out, y - (1e-6 if x_in == x_out else 0.0), 0.1, 1, 0, 0, 0], np.zeros(6))[2]
        assert abs(d_in[0]["depth"] - 0.1) < 1e-9 and abs(d_out[0]["depth"] - 0.1) < 1e-9
    # ... and the rake around its borders and corners
    rng = np.random.default_rng(5)
    for k in range(24):
        d = tr.design_rake(grid, rng, 0.04, 0.30, mode=("edge", "on_border")[k % 2], raised_gap=(0.1, 0.3))
        check_design(d, grid, f"wall map design {k}")
    assert len(TALLY.failures) == f0, TALLY.failures[f0:f0 + 10]


def test_three_maps_per_world_through_the_batched_step(built_lib):
    """orc_step_batch with hm_index (env_map = e % 3): three different 9 x 7 maps, one rake, each env at the pose designed on ITS map's twin -
    a wrong per-env map offset puts an env on another map's heights"""
    once("three maps", sweep_three_maps)


def sweep_three_maps():
    rng = np.random.default_rng(77)
    geom = (9, 7, 4.0, 2.25, 0.25, -0.125)
    f0 = len(TALLY.failures)
    for k in range(8):
        base = tr.random_map(*geom, amplitude=0.3, seed=300 + k)
        shifts = (0.0, 0.25, -0.125)
        grids = [tr.Grid(base.h + s, *geom[2:]) for s in shifts]
        d = tr.design_rake(base, rng, 0.04, 0.30, mode=MODES[k % 4])
        model = Model(urdf_string=tr.rake_urdf(d.offsets, d.radii))
        off, rad = blob_spheres(model)
        N = 6
        env_map = np.arange(N) % 3
        q = np.tile(d.q, (N, 1)); q[:, 3:7] /= np.linalg.norm(d.q[3:7])
        q[:, 2] += np.array(shifts)[env_map]
        o = oracle_for(model)
        o.set_heightmaps(np.stack([g.h32 for g in grids]), *geom[2:], env_map)
        res = o.step_batch(q, np.zeros((N, 6)), 1, want_contacts=True, lam_warm=o.new_warm_state(N))
        assert (res["flags"] & 3 == 0).all()
        for e in range(N):
            con = res["contacts"][e][:res["n_contacts"][e]]
            v = tr.verdict(grids[env_map[e]], tr.sphere_centres(q[e], off), rad, *by_primitive(con), tie=TIE, bar=BAR, unit_tol=UNIT, exact=np.arange(tr.N_SPHERES) == 0)
            TALLY.add(v, f"three maps design {k} env {e}")
            np.add.at(FAMILY_COUNT, d.family, 1)
    assert len(TALLY.failures) == f0, TALLY.failures[f0:f0 + 10]


def test_the_sweep_as_a_whole(built_lib):
    """>= 10 000 placements over all sweeps of this file (those that have not run yet run here), every family and regime present, clearances over
    the whole range, <= 1 % excluded"""
    for case in SMALL_R:
        once(case[0], sweep_small, *case)
    for ratio in (1.2, 2.5):
        once(ratio, sweep_window, ratio)
    once("wall", sweep_wall)
    once("three maps", sweep_three_maps)
    for line in TALLY.lines():
        print(line)
    print(dict(zip(tr.FAMILIES, FAMILY_COUNT.tolist())), "below the surface:", BELOW_COUNT[0])
    assert TALLY.n.sum() >= 10000, TALLY.n
    assert (TALLY.n >= 300).all() and (TALLY.hits >= 100).all(), (TALLY.n, TALLY.hits)
    assert (FAMILY_COUNT >= 100).all(), FAMILY_COUNT
    cl = np.array(CLEARANCE)
    assert cl.min() < 0.06 and cl.max() > 1.25 and cl.min() >= 0.02 - 1e-9 and cl.max() <= 1.3 + 1e-9 and np.histogram(cl, 8, (0.02, 1.3))[0].min() > 200
    assert TALLY.excluded_share() <= 0.01, TALLY.excluded_share()
    assert not TALLY.failures, TALLY.failures[:10]
