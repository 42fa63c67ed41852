"""The oracle's self-collision (oracle/rsb_oracle.c: self_pair_ok, "Self-collision" and "joint limits" in step_impl) against the independent brute force of
tests/self_collision_reference.py on the designed combs - so the oracle is pinned too, and the reference is exercised without a GPU - and the oracle's per-pair
materials (set_self_collision(mu=, restitution=, res_threshold=)) against closed forms.

Bars of the list comparison.  fp64 on coordinates below 1 m leaves ~1e-16; bar = 1e-9 m on position and depth, 2 bar / d_min = 4e-8 on the normal (d_min = 0.05 m),
|n| = 1 to 1e-12, tie band 2e-9 m (no designed placement is that close: the grazing family starts at 1e-7).

Closed forms (Couples in the reference: six couples of sliders on a fixed base, zero gravity, erp 0, one integrate()).  Measured floor of the oracle against them:
head-on 1.6e-5 m/s on A and 8.0e-6 on B, friction 3.6e-5 on A and 2.1e-5 on B's tangential speed.  That is the Delassus block's compliance to the digit
(Couples.bars derives it: 1e-4 of the block's mean diagonal, twice on a fixed base; the solver's stopping threshold 1e-5 is added on top, which gives 2.6e-5 / 1.8e-5 and
4.6e-5 / 3.1e-5 as the bars).  A neighbouring couple's material entry misses the closed form by 4e-2 m/s and more: three orders of magnitude.  Of the rule "each couple's
other side lies on the wrong side of another couple's threshold" the two ends cannot be had: the slow side of the smallest threshold is below every threshold, the fast
side of the largest above every one; there the restitution coefficient (>= 30 % apart) tells the couples apart."""
import numpy as np
import pytest

import self_collision_reference as sr
from common import Oracle

TIE, BAR, UNIT = 2e-9, 1e-9, 1e-12
SCENES = [("A", "main"), ("A", "ignore"), ("A", "overflow 8"), ("A", "overflow 5"), ("A", "overflow 16"), ("B", "main"), ("C", "shapes")]
RESULTS = {}


def ignore_matrix(nb, ignore):
    m = np.zeros((nb, nb), np.uint8)
    for a, b in ignore:
        m[a, b] = m[b, a] = 1
    return m


def run_oracle(model, sc):
    o = Oracle(model.blob)
    o.p.gravity[0] = o.p.gravity[1] = o.p.gravity[2] = 0.0
    o.p.kmax, o.p.erp = sc.kmax, sc.erp
    o.set_ground(-5.0 if sc.ground is None else sc.ground)
    o.set_self_collision(True, ignore=ignore_matrix(o.nb, sc.ignore) if sc.ignore else None)
    return o, o.step_batch(sc.q, np.zeros((sr.N_ENVS, o.nv)), 1, want_contacts=True)


def oracle_result(which, name):
    if (which, name) not in RESULTS:
        comb, model, scenes = sr.designed(which)
        RESULTS[which, name] = run_oracle(model, scenes[name])
    return RESULTS[which, name]


def check(which, name, perturb=None):
    comb, model, scenes = sr.designed(which)
    sc = scenes[name]
    o, res = oracle_result(which, name)
    pairs = sr.candidate_pairs(comb.T, sc.ignore)
    assert np.array_equal(o.self_pairs(), pairs)
    tally = sr.Tally()
    sr.check_scene(sc, comb.T, pairs, res["n_contacts"], res["contacts"], res["flags"], res["u"], TIE, BAR, UNIT, False, tally, perturb, name=f"{which} {name}")
    return tally


@pytest.mark.parametrize("which,name", SCENES, ids=[f"{w}-{n.replace(' ', '-')}" for w, n in SCENES])
def test_oracle_lists_against_the_brute_force(built_lib, which, name):
    """candidate list, ids, bodies, order, counts, overflow bit, positions, normals and depths of every env; where a joint is past its limit, also whether its
    row got a slot (by what the row does to the joint's velocity)"""
    tally = check(which, name)
    print(tally.lines()[0])
    assert not tally.failures, tally.failures[:10]
    assert tally.tied == 0 and tally.hits >= 6


def test_the_designs_reach_the_edges(built_lib):
    """what the issue asks the inputs to reach, asserted from the reference alone - with the DEVICE's tie band (6e-6 m), the wider one"""
    sr.assert_the_designs_reach_the_edges(6e-6)


PERTURBATIONS = {
    "one pair swapped in order": ("A", "main", lambda comb: sr.swap_two_hits),
    "a normal's sign flipped": ("A", "main", lambda comb: sr.flip_a_normal),
    "the point moved to c_i - r_i n": ("A", "main", lambda comb: sr.point_on_the_surface_of_i()),
    "the odd slot not given to the limit row": ("A", "overflow 5", lambda comb: sr.odd_slot_withheld(5)),
    "a hit at pair n_self - 1 removed": ("A", "main", lambda comb: sr.drop_the_last_pair(comb.pairs[-1])),
}


@pytest.mark.parametrize("what", list(PERTURBATIONS))
def test_the_comparison_notices(built_lib, what):
    """the comparison that passes above fails once the reference's expected list is perturbed"""
    which, name, make = PERTURBATIONS[what]
    assert not check(which, name).failures
    tally = check(which, name, make(sr.designed(which)[0]))
    print(what, "->", tally.failures[:2])
    assert tally.failures


# ---- per-pair materials against closed forms -----------------------------------------------------------------------------------------------------------
def couples(tangent):
    from raisimlib_amd import Model
    model = Model(urdf_string=sr.couples_urdf(sr.K_COUPLES, sr.MASS_A, sr.MASS_B, tangent))
    assert model.blob.fixed_base == 1
    return model, sr.Couples(tangent, model.blob)


def oracle_step(model, c, q, u, materials, default=None):
    o = Oracle(model.blob)
    o.p.gravity[0] = o.p.gravity[1] = o.p.gravity[2] = 0.0
    o.p.erp, o.p.kmax = 0.0, 16
    o.set_ground(-5.0)
    if default is not None:
        o.p.mu, o.p.restitution, o.p.res_threshold = default
    mu, rest, thr = materials if materials is not None else (None, None, None)
    o.set_self_collision(True, ignore=ignore_matrix(o.nb, c.ignore), mu=mu, restitution=rest, res_threshold=thr)
    assert np.array_equal(o.self_pairs(), c.pairs)
    res = o.step_batch(q, u, 1, want_contacts=True)
    assert (res["flags"] == 0).all() and np.array_equal(res["n_contacts"], 2 * c.active.sum(axis=1))      # every solve converged, nothing overflowed
    return res["u"]


@pytest.mark.parametrize("tangent", [False, True], ids=["head-on", "friction"])
def test_oracle_per_pair_materials_against_the_closed_forms(built_lib, tangent):
    model, c = couples(tangent)
    q, u, want, asserted = c.state(sr.MU, sr.REST, sr.THR)
    assert asserted[c.active].all()
    u1 = oracle_step(model, c, q, u, (sr.MU, sr.REST, sr.THR))
    ea, eb, ei = c.errors(u1, want, asserted)
    ba, bb = c.bars(u, want)
    print(f"{'friction' if tangent else 'head-on'}: A off by {ea:.2e} (bar {ba:.2e}), B by {eb:.2e} (bar {bb:.2e}), inactive sliders move at {ei:.1e}")
    assert ea <= ba and eb <= bb and ei <= 1e-12
    if not tangent:      # momentum of every couple
        for k in range(sr.K_COUPLES):
            ia, ib = 5 + c.body_a[k], 5 + c.body_b[k]
            assert np.abs(sr.MASS_A[k] * (u1[:, ia] - u[:, ia]) + sr.MASS_B[k] * (u1[:, ib] - u[:, ib])).max() <= 1e-12
    for shift in (1, 2, 3):      # a neighbour's entry (wrong pair index) or a swapped column is orders of magnitude outside the bar
        _, _, wrong, _ = c.state(np.roll(sr.MU, shift), np.roll(sr.REST, shift), np.roll(sr.THR, shift))
        wa, wb, _ = c.errors(u1, wrong, asserted)
        assert max(wa, wb) > 100 * max(ba, bb), (shift, wa, wb)
    _, _, wrong, _ = c.state(sr.REST, sr.MU, sr.THR)
    assert max(c.errors(u1, wrong, asserted)[:2]) > 100 * max(ba, bb)


@pytest.mark.parametrize("tangent", [False, True], ids=["head-on", "friction"])
def test_oracle_without_per_pair_materials_uses_the_worlds(built_lib, tangent):
    model, c = couples(tangent)
    default = (0.37, 0.45, 0.09)
    uniform = tuple(np.full(sr.K_COUPLES, v) for v in default)
    q, u, want, asserted = c.state(*uniform)
    u1 = oracle_step(model, c, q, u, None, default)
    ea, eb, _ = c.errors(u1, want, asserted)
    ba, bb = c.bars(u, want)
    assert asserted[c.active].mean() > 0.5 and ea <= ba and eb <= bb, (ea, ba, eb, bb)
