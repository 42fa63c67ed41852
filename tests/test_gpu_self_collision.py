"""The device's self-collision - candidate list (enumerate_self_pairs), sweep and rare path of step_phase_collision.inc, slot assembly with the joint-limit rows,
per-pair materials (upload_image -> d_self_mat -> SELFT, restitution on the folded row in step_phase_columns.inc) - DIRECTLY against the brute force and the
closed forms of tests/self_collision_reference.py, not against the oracle (its algorithmic twin).

Lists.  The designed combs of the reference (models A: 170 candidate pairs, B: exactly 64, C: with a capsule, a cylinder and two boxes; <= 11 bodies), N = 64 envs,
16, 32 and 64 lanes per env on the ahead-of-time kernel classes (specialisation off).  rsb_get_contacts / rsb_get_flags after integrate(1) at zero gravity and
velocity: the contacts of the state that was set.  Ids, bodies, order, counts and the overflow bit are compared exactly; a joint past its limit also by what its row
does (erp 0.2: a row that got a slot sends the joint back at erp x 0.05 rad / dt = 4 rad/s, one without a slot leaves it at the recoil of the self-collisions, ~1e-3).

Bars, derived, not fitted.  bar = 3e-6 m on position and depth: tests/test_gpu_terrain_contact.py derives 3e-6 m for ONE rigid transform of a sphere offset at
coordinates within +-3 m (12.5 ulp of 2.4e-7).  Here coordinates stay within +-1 m (ulp 1.2e-7: 1.5e-6 per transform) and a centre passes two rotating levels (base,
elbow; the slider in between only adds along an axis): 2 x 1.5e-6 = 3e-6.  Normal: 2 bar / d_min = 1.2e-4 with d_min = 0.05 m, the smallest centre distance of a
designed hit (both centres move by up to bar).  |n| = 1 to 1e-6 (8 ulp).  Tie band: a pair with | dist - (r_i + r_j) | < 2 bar = 6e-6 m may be reported or not;
the designed families keep >= 1e-4 m from it (tests/test_self_collision_reference.py checks that and the 1 % cap on the CPU), only the grazing family (overlaps
1e-7 .. 1e-5 m) uses it.  Coincident centres sit at an unrotated, untranslated base, so the device's own centre distance stays below its 1e-6 guard.

Materials.  Couples of the reference (six couples of sliders on a fixed base - the world root and twelve moving bodies -, zero gravity, erp 0, no gains, no damping,
no effort limits).  Bar = the larger of the closed forms' floor (Couples.bars: solver threshold 1e-5 + the Delassus block's compliance, 2.6e-5 / 1.8e-5 m/s head-on,
4.6e-5 / 3.1e-5 friction; the oracle sits at 1.6e-5 / 8.0e-6 and 3.6e-5 / 2.1e-5) and the bar of the existing closed-form tests of the same quantity
(test_restitution_bounces_the_ball: 2e-5 m/s, test_sliding_friction_decelerates_at_mu_g: 3e-6 m/s).  No env may report an unconverged solve (flag bit 2).

The worst value per quantity and lane mapping goes to profiles/self_collision_parity.txt.  Measured on an MI355X, the same at 16, 32 and 64 lanes: position
<= 7.4e-8 m, depth <= 4.6e-8 m, normal <= 9.3e-7, | |n| - 1 | <= 1.1e-7, 7 of 10880 placements of the main world in the tie band (the grazing family's); materials:
head-on A <= 1.8e-5 m/s, B <= 9.0e-6, friction A <= 4.1e-5, B <= 2.1e-5 (the compliance, as on the oracle), inactive sliders exactly at rest, every solve converged."""
import os

import numpy as np
import pytest

import self_collision_reference as sr
from common import ROOT
from raisimlib_amd import BatchedWorld, Model

pytestmark = pytest.mark.gpu

N, LANES = sr.N_ENVS, sr.LANES
BAR, UNIT = 3e-6, 1e-6
TIE = 2 * BAR
SCENES = [("A", "main"), ("A", "ignore"), ("A", "overflow 8"), ("A", "overflow 5"), ("A", "overflow 16"), ("B", "main"), ("C", "shapes")]
SECTIONS = {}


def write_report():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "self_collision_parity.txt"), "w") as f:
        f.write("tests/test_gpu_self_collision.py: worst value per quantity, device fp32 vs the fp64 brute force and closed forms of tests/self_collision_reference.py on the\n"
                f"float32-rounded state (bars: position and depth {BAR:g} m, normal {2 * BAR / 0.05:g}, | |n| - 1 | {UNIT:g}, tie band {TIE:g} m; materials: see each line)\n")
        for name in sorted(SECTIONS):
            f.write(f"{name}\n" + "".join(f"  {l}\n" for l in SECTIONS[name]))


def device_world(model, lpe, kmax=16, ground=None, erp=0.0, ignore=()):
    w = BatchedWorld(model, N)
    w.set_specialization("off")      # ahead-of-time kernel classes only
    w.set_gravity([0.0, 0.0, 0.0])
    w.set_erp(erp)
    w.set_max_contacts(kmax)
    w.set_lanes_per_env(lpe)
    w.add_ground(-5.0 if ground is None else ground)
    for a, b in ignore:
        w.ignore_collision_between(a, b)
    return w


def step_from(w, q, u=None):
    w.set_state(q, np.zeros((N, w.nv)) if u is None else u)
    w.integrate(1)
    cnt, con = w.get_contacts()
    flags = w.get_flags()
    q1, u1 = w.get_state()
    assert np.isfinite(q1).all() and np.isfinite(u1).all() and (flags & 2 == 0).all()
    return cnt, con, flags, u1.astype(np.float64)


@pytest.mark.parametrize("which,name", SCENES, ids=[f"{w}-{n.replace(' ', '-')}" for w, n in SCENES])
def test_lists_against_the_brute_force(built_lib, which, name):
    comb, model, scenes = sr.designed(which)
    sc = scenes[name]
    pairs = sr.candidate_pairs(comb.T, sc.ignore)
    ids_by_lanes, lines = [], []
    for lpe in LANES:
        w = device_world(model, lpe, sc.kmax, sc.ground, sc.erp, sc.ignore)
        assert np.array_equal(w.self_collision_pairs(), pairs)
        cnt, con, flags, u1 = step_from(w, sc.q)
        _, n_spec, n_aot = w.specialization_status()
        assert n_spec == 0 and n_aot >= 1
        tally = sr.Tally()
        sr.check_scene(sc, comb.T, pairs, cnt, con, flags, u1, TIE, BAR, UNIT, True, tally, name=f"{which} {name} lanes {lpe}")
        if name == "ignore":      # the switch: off - no entry anywhere, the candidate list stays; on again - the same lists, bit for bit
            w.set_self_collision(False)
            cnt0, _, flags0, _ = step_from(w, sc.q)
            assert not cnt0.any() and not (flags0 & 1).any() and np.array_equal(w.self_collision_pairs(), pairs)
            w.set_self_collision(True)
            cnt2, con2, flags2, _ = step_from(w, sc.q)
            assert np.array_equal(cnt2, cnt) and np.array_equal(flags2 & 1, flags & 1) and all(con2[e][:cnt[e]].tobytes() == con[e][:cnt[e]].tobytes() for e in range(N))
        w.close()
        ids_by_lanes.append([tuple(con[e][:cnt[e]]["collision"]) for e in range(N)])
        lines.append(f"{lpe} lanes per env: " + tally.lines()[0])
        print(lines[-1])
        SECTIONS[f"lists, model {which}, {name}"] = lines
        write_report()
        assert not tally.failures, tally.failures[:10]
        if not any(l.startswith("grazing") for l in sc.label):
            assert tally.tied == 0
        assert tally.tied <= 0.01 * tally.placements and tally.hits >= 6
    assert ids_by_lanes[0] == ids_by_lanes[1] == ids_by_lanes[2] or any(l.startswith("grazing") for l in sc.label)
    if name == "ignore":      # the hits on the ignored bodies are gone, the others stay: against the full list the same states hold two hits per designed env
        full = sr.candidate_pairs(comb.T)
        assert len(full) > len(pairs)
        for e in range(0, 16, 2):
            c = sr.centres(comb.T, sc.q[e], single=True)
            d, rs = sr.pair_distances(comb.T, full, c, single=True)
            assert (d < rs).sum() == 2 and len(ids_by_lanes[0][e]) == 2


def test_the_designs_reach_the_edges(built_lib):
    """the residues of n_self, the pass boundaries, the dropped hit with its odd slot, the coincident pairs, mixed lanes, the 1 % cap: with this file's tie band"""
    sr.assert_the_designs_reach_the_edges(TIE)


# ---- per-pair materials ------------------------------------------------------------------------------------------------------------------------------
def couples(tangent):
    model = Model(urdf_string=sr.couples_urdf(sr.K_COUPLES, sr.MASS_A, sr.MASS_B, tangent))
    assert model.blob.fixed_base == 1
    return model, sr.Couples(tangent, model.blob)


def material_bars(c, u, want):
    ba, bb = c.bars(u, want)
    return max(ba, 2e-5), max(bb, 3e-6 if c.tangent else 2e-5)


def check_materials(w, c, q, u, want, asserted, what, worst):
    cnt, con, flags, u1 = step_from(w, q, u)
    assert (flags == 0).all(), (what, flags)      # nothing overflowed, every solve converged
    ea, eb, ei = c.errors(u1, want, asserted)
    ba, bb = material_bars(c, u, want)
    worst[what] = (ea, ba, eb, bb, ei)
    return cnt, u1


@pytest.mark.parametrize("tangent", [False, True], ids=["head-on", "friction"])
def test_per_pair_materials_against_the_closed_forms(built_lib, tangent):
    model, c = couples(tangent)
    case = "friction" if tangent else "head-on"
    lines = []
    for lpe in LANES:
        worst = {}
        w = device_world(model, lpe, ignore=c.ignore)
        assert np.array_equal(w.self_collision_pairs(), c.pairs)
        default = (0.37, 0.45, 0.09)
        w.set_default_material(*default)
        uniform = tuple(np.full(sr.K_COUPLES, v) for v in default)
        # no call at all: the world's material
        q, u, want_d, as_d = c.state(*uniform)
        cnt, _ = check_materials(w, c, q, u, want_d, as_d, "no call", worst)
        assert np.array_equal(cnt, 2 * c.active.sum(axis=1))
        # one entry per pair
        w.set_self_collision_materials(sr.MU, sr.REST, sr.THR)
        q, u, want, asserted = c.state(sr.MU, sr.REST, sr.THR)
        assert asserted[c.active].all()
        _, u1 = check_materials(w, c, q, u, want, asserted, "per pair", worst)
        if not tangent:
            for k in range(sr.K_COUPLES):
                ia, ib = 5 + c.body_a[k], 5 + c.body_b[k]
                dp = np.abs(sr.MASS_A[k] * (u1[:, ia] - u[:, ia]) + sr.MASS_B[k] * (u1[:, ib] - u[:, ib])).max()
                assert dp <= 2.5 * 2e-5, (k, dp)      # momentum: both velocities within the restitution bar, masses <= 2.5 kg
        ba, bb = material_bars(c, u, want)
        for shift in (1, 2, 3):      # a neighbour's entry is orders of magnitude outside the bar
            _, _, wrong, _ = c.state(np.roll(sr.MU, shift), np.roll(sr.REST, shift), np.roll(sr.THR, shift))
            assert max(c.errors(u1, wrong, asserted)[:2]) > 100 * max(ba, bb)
        # switched off and on again: the overrides are still there
        w.set_self_collision(False)
        cnt, _, _, u_off = step_from(w, q, u)
        assert not cnt.any() and np.array_equal(u_off, u)
        w.set_self_collision(True)
        check_materials(w, c, q, u, want, asserted, "after off and on", worst)
        # a second call with permuted values: the table is uploaded again
        perm = np.array([3, 5, 0, 4, 1, 2])
        w.set_self_collision_materials(sr.MU[perm], sr.REST[perm], sr.THR[perm])
        qp, up, want_p, as_p = c.state(sr.MU[perm], sr.REST[perm], sr.THR[perm])
        check_materials(w, c, qp, up, want_p, as_p, "permuted", worst)
        # NULL arrays: back to the world's material
        w.set_self_collision_materials(None, None, None)
        check_materials(w, c, q, u, want_d, as_d, "NULL arrays", worst)
        # the list changes (the last couple's own bodies are ignored): the overrides are gone, the other couples follow the world's material, the last passes through
        w.set_self_collision_materials(sr.MU, sr.REST, sr.THR)
        w.ignore_collision_between(c.body_a[-1], c.body_b[-1])
        assert np.array_equal(w.self_collision_pairs(), c.pairs[:-1])
        want_i, as_i = want_d.copy(), as_d.copy()
        want_i[:, 5 + c.body_a[-1]], want_i[:, 5 + c.body_b[-1]] = u[:, 5 + c.body_a[-1]], u[:, 5 + c.body_b[-1]]
        cnt, _ = check_materials(w, c, q, u, want_i, as_i, "after the list changed", worst)
        assert np.array_equal(cnt, 2 * c.active[:, :-1].sum(axis=1))
        w.close()
        lines += [f"{lpe} lanes per env, {what}: A off by {v[0]:.2e} m/s (bar {v[1]:.2e}), B by {v[2]:.2e} (bar {v[3]:.2e}), inactive sliders {v[4]:.1e}" for what, v in worst.items()]
        SECTIONS[f"materials, {case}"] = lines
        write_report()
        print("\n".join(lines[-len(worst):]))
        for what, (ea, ba, eb, bb, ei) in worst.items():
            assert ea <= ba and eb <= bb and ei <= 1e-9, (case, lpe, what, ea, ba, eb, bb, ei)
