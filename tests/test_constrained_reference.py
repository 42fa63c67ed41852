"""The fp64 reference of the held-frame queries (tests/constrained_reference.py), CPU tier: the reference pinned against a second route and against
closed forms, the comparison's sensitivity, and the inputs of the GPU tests (tests/test_gpu_constrained.py).

  - the KKT solve against the Schur route (G + rho I) lambda = t - a_f, x = x_f + JMinv^T lambda, to 1e-9 of 1 + max|ref|, on every variant that is
    solved: dynamics and impulse (the impulse with joint_diag);
  - a free box held at its centre of mass with angular rows under gravity: udot = 0, lambda = (-m g, 0);
  - a pendulum whose tip is held at rest: udot = 0 (three rows on one degree of freedom are dependent: solved with rho = 1e-8 G_max, udot is then
    udot_f rho / (rho + G_max) < 1e-8 |udot_f|);
  - an impulse with target_vel = 0 and damping = 0 never raises 0.5 gv^T (M + D) gv and gives J (gv + dgv) = 0;
  - a 1e-3 relative error planted in lambda trips the gates, dynamics and impulse: lambda alone the dynamics row, lambda carried into
    x = x_f + JMinv^T lambda the constraint row, and the forward bar 4 x FWD32 wherever that bar is below the planted error (the humanoid's,
    4 x 7.5e-4, is not: its free acceleration is that uncertain in float32, and the bar is the issue's);
  - the restatement (tools/constrained_restatement.py: held_solve_kernel's arithmetic in numpy float32 on float32 restatements of its inputs), run
    here on every variant and every env, dynamics and impulse: both gates <= 1, every env the status of its class, and the forward maxima over each
    case's regular variants equal to constrained_reference.FWD32 - the figures the GPU test takes its forward bars from;
  - the inputs.  Every frame set is, by the fp64 Cholesky of its undamped G_ref on every env, regular (smallest pivot over its own diagonal entry
    >= 1e-3) or dependent (<= 1e-9), nothing in between, with and without joint_diag: RSB_HELD_PIVOT_TOL = 1e-5 sits 100 x below the one and 1e4 x
    above the other.  A dependent set run with damping d has every pivot >= d / (1 + d) of its entry (rho / (G_ii + rho), G_ii <= G_max): with
    DAMP = 1e-4 ten times the tolerance.  The row counts 3, 6, 9, 12, 18, 24, 36, 66, 96 straddle the lane-group edges 16 | 32 | 64 | second row."""
import numpy as np
import pytest

import constrained_reference as cr
import inverse_mass_reference as imr
from test_dynamics_reference import dyn_case

ALL = [(n, k, a, d) for n in cr.CASES for k, a, d in cr.variants(n)]
SOLVED = [v for v in ALL if cr.solvable(*v)]
REGULAR = [v for v in ALL if cr.regular(*v[:3])]
ids = lambda v: f"{v[0]}-{v[1]}-{'ang' if v[2] else 'lin'}-{v[3]:.0e}"


@pytest.mark.parametrize("v", SOLVED, ids=ids)
def test_kkt_against_schur(built_lib, v):
    name, key, angular, damping = v
    c = dyn_case(name)
    J = cr.stacked_jacobian(name, key, angular)
    uf = cr.free_dynamics(name)
    a_f = np.einsum("eki,ei->ek", J, uf) + cr.bias(name, key, angular)
    x, lam = cr.dynamics_reference(name, key, angular, damping)
    xs, ls = cr.schur(name, key, angular, damping, False, uf, a_f, cr.target(name, key, angular, "acc"))
    assert cr.forward_error(xs, x).max() <= 1e-9 and cr.forward_error(ls, lam).max() <= 1e-9, (cr.forward_error(xs, x).max(), cr.forward_error(ls, lam).max())
    v0 = np.einsum("eki,ei->ek", J, cr.gv_of(c))
    x, lam = cr.impulse_reference(name, key, angular, damping, True)
    xs, ls = cr.schur(name, key, angular, damping, True, np.zeros((c.N, c.nv)), v0, cr.target(name, key, angular, "vel"))
    assert cr.forward_error(xs, x).max() <= 1e-9 and cr.forward_error(ls, lam).max() <= 1e-9, (cr.forward_error(xs, x).max(), cr.forward_error(ls, lam).max())
    if c.fixed:
        assert not x[:, :6].any()


def test_a_free_box_held_at_its_centre_of_mass(built_lib):
    from raisimlib_amd import Model
    model = Model(urdf_string=imr.BOX_URDF)
    g = (0.3, -0.2, -9.81)
    rng = np.random.default_rng(2)
    qt = rng.normal(size=4)
    q = np.r_[0.1, 0.2, 0.9, qt / np.linalg.norm(qt)]
    udot, lam, uf = cr.held_single(model, q, np.zeros(6), np.zeros(6), [(0, (0.03, -0.02, 0.05))], True, g)
    assert np.abs(udot).max() <= 1e-12 and np.abs(uf[:3] - g).max() <= 1e-12
    assert np.abs(lam - np.r_[-3.5 * np.asarray(g), 0, 0, 0]).max() <= 1e-11


def test_a_pendulum_whose_tip_is_held(built_lib):
    from common import PENDULUM_URDF, f32
    from raisimlib_amd import Model
    L = 0.7
    model = Model(urdf_string=PENDULUM_URDF.replace("anchor", "world").format(l=L, m=1.0))      # (a root link named "world": a fixed base)
    assert model.blob.fixed_base == 1
    q, frames, nv = f32([0, 0, 0, 1, 0, 0, 0, 0.4]), [(1, (0.0, 0.0, -L))], model.nv
    tau = np.zeros(nv); tau[-1] = 0.7
    _, _, uf = cr.held_single(model, q, np.zeros(nv), tau, frames, False, (0, 0, -9.81), rho=1.0)      # (rho = 1: only udot_f is wanted)
    assert abs(uf[-1]) > 1.0
    Gmax = L * L / (1.0 * L * L)      # j j^T / M of a point mass on a massless rod: its largest eigenvalue, >= every diagonal entry
    udot, lam, _ = cr.held_single(model, q, np.zeros(nv), tau, frames, False, (0, 0, -9.81), rho=1e-8 * Gmax)
    assert np.abs(udot).max() <= 1e-7 * np.abs(uf).max(), (udot, uf)
    assert np.abs(lam).max() > 0.1


@pytest.mark.parametrize("v", [v for v in REGULAR if v[3] == 0.0], ids=ids)
def test_an_impulse_stops_the_frames_and_never_adds_energy(built_lib, v):
    name, key, angular, _ = v
    c = dyn_case(name)
    J, u = cr.stacked_jacobian(name, key, angular), cr.gv_of(c)
    for wd in (False, True):
        dgv, lam = cr.impulse_reference(name, key, angular, 0.0, wd, with_target=False)
        A = imr.system(name, wd)
        after = u + dgv
        assert np.abs(np.einsum("eki,ei->ek", J, after)).max() <= 1e-9 * (1 + np.abs(u).max())
        e0, e1 = 0.5 * np.einsum("ei,eij,ej->e", u, A, u), 0.5 * np.einsum("ei,eij,ej->e", after, A, after)
        assert (e1 <= e0 * (1 + 1e-12)).all()


@pytest.mark.parametrize("v", [v for v in REGULAR if v[3] == 0.0], ids=ids)
def test_a_planted_error_trips_the_gates(built_lib, v):
    name, key, angular, _ = v
    c = dyn_case(name)
    for impulse in (False, True):
        x, lam = cr.impulse_reference(name, key, angular, 0.0, True) if impulse else cr.dynamics_reference(name, key, angular, 0.0)
        t = cr.target(name, key, angular, "vel" if impulse else "acc")
        xf = np.zeros((c.N, c.nv)) if impulse else cr.free_dynamics(name)
        free = None if impulse else xf
        dyn, con = cr.gates(name, key, angular, 0.0, impulse, x, lam, t, impulse, free)
        assert dyn.max() <= 1e-6 and con.max() <= 1e-6      # the reference meets its own gates
        JM = cr.delassus(name, key, angular, impulse)[1]
        bad = lam * (1 + 1e-3)
        dyn, _ = cr.gates(name, key, angular, 0.0, impulse, x, bad, t, impulse, free)
        assert dyn.max() > 1.0, (impulse, dyn.max())
        xb = xf + np.einsum("eki,ek->ei", JM, bad)
        _, con = cr.gates(name, key, angular, 0.0, impulse, xb, bad, t, impulse, free)
        assert con.max() > 1.0, (impulse, con.max())
        bar = 4 * cr.FWD32[name]["imp" if impulse else "dyn"][0]
        if name != "atlas":      # (the humanoid's bar, 4 x 7.5e-4 / 1.9e-4 of 1 + max|lambda|, is at or above the planted error: see the docstring)
            assert cr.forward_error(bad, lam).max() > bar, (impulse, cr.forward_error(bad, lam).max(), bar)


@pytest.mark.parametrize("name", cr.CASES)
def test_the_float32_restatement_meets_the_gates_and_gives_the_forward_figures(built_lib, name):
    import os
    import sys
    from common import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import constrained_restatement as rs
    cache, worst = {}, {"dyn": [0.0, 0.0], "imp": [0.0, 0.0]}
    for v in cr.variants(name):
        r = rs.run(name, *v, np.float32, cache)
        for tag in ("dyn", "imp"):
            assert r[tag + "_status_ok"], (name, v, tag, r[tag + "_status_hist"])      # every env: 0 where solvable, 1 on a dependent set without damping
            if cr.solvable(name, *v):
                assert max(r[tag + "_gates"]) <= 1.0, (name, v, tag, r[tag + "_gates"])
            else:
                assert r[tag + "_refused"] < 1.0
            if tag + "_fwd" in r:
                worst[tag] = [max(a, b) for a, b in zip(worst[tag], r[tag + "_fwd"])]
    if name in cr.FWD32:
        for tag in ("dyn", "imp"):
            assert np.allclose(worst[tag], cr.FWD32[name][tag], rtol=2e-3, atol=0), (name, tag, worst[tag], cr.FWD32[name][tag])      # (the constants carry four digits)
    else:
        assert worst == {"dyn": [0.0, 0.0], "imp": [0.0, 0.0]}      # no regular set on this case: no forward bar is used


def test_every_frame_set_is_regular_or_dependent_and_the_rows_straddle_the_lane_groups(built_lib):
    ms, regular_ms = set(), set()
    for name in cr.CASES:
        for key, angular, damping in cr.variants(name):
            m = cr.rows_of(name, key, angular)
            ms.add(m)
            for wd in (False, True):
                p = cr.pivots(name, key, angular, wd, 0.0)
                assert p.min() >= 1e-3 or p.max() <= 1e-9, (name, key, angular, wd, p.min(), p.max())      # nothing in between
                assert (p.min() >= 1e-3) == cr.regular(name, key, angular), (name, key, angular, wd)
                if damping > 0:
                    pd = cr.pivots(name, key, angular, wd, damping)
                    assert pd.min() >= damping / (1 + damping) * (1 - 1e-6), (name, key, angular, wd, pd.min())
            if cr.regular(name, key, angular):
                regular_ms.add(m)
                assert damping == 0.0
    assert ms >= {3, 6, 9, 12, 18, 24, 36, 66, 96}, sorted(ms)
    assert regular_ms >= {3, 6, 12, 18, 24}, sorted(regular_ms)
    assert cr.regular("anymal", "feet", False) and not cr.regular("anymal", "feet", True) and not cr.regular("floating0", "sixteen", True)
    assert all(not cr.regular(n, "twice", False) for n in ("floating0", "fixed2", "anymal"))
