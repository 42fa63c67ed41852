"""tests/step_balance_reference.py on the CPU, before any device result is held to it: the impulse balance on the ORACLE's own steps (it holds to 1e-12 of
the row scale on every env, converged or not: this pins the helper, not the oracle), the populations' guards (enough unconverged, overflowed, limited,
self-colliding and effort-clipped envs), and the checker's sensitivity: mutated oracle outputs have to fail it."""
import functools

import numpy as np
import pytest

import step_balance_reference as sb

CPU_CASES = ([f"fuzz_floating{s}" for s in range(12)] + [f"fuzz_fixed{s}" for s in range(6)]
             + ["anymal_contorted_air_k8", "anymal_contorted_ground_k8", "atlas_standing", "fuzz_heightmap0", "anymal_clipped"])
BAR = sb.C_STEP


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(case, oracle, its one step, per env its records, the balance of every env); computed once, nobody writes into it"""
    c = sb.case(name)
    o, ref = sb.oracle_step(c)
    con = [ref["contacts"][e][:ref["n_contacts"][e]] for e in range(c.N)]
    return c, o, ref, con, sb.balance(o, c.gc, c.gv, ref["u"], con, c.kp, c.kd, c.pt, c.dtg, c.tau_ff)


@pytest.mark.parametrize("name", CPU_CASES)
def test_the_balance_holds_on_the_oracles_own_step(name):
    """max |r0| / S <= 1e-10 on every env, S the row's sum of absolute terms, and no limit row wrong-signed beyond 1e-10 S_j (measured: 1.1e-12 worst);
    the oracle's own records obey the record laws"""
    c, o, ref, con, res = oracle_run(name)
    sb.assert_no_joint_at_a_stop(c.model.blob, c.gc)
    worst = max(x.r0_rel for x in res)
    print(f"{name}: worst |r0| / S {worst:.1e} over {c.N} envs")
    for e, x in enumerate(res):
        assert x.r0_rel <= 1e-10, (name, e, x.r0_rel)
        assert np.all(x.lim_sr >= -1e-10 * x.lim_S), (name, e, x.lim_sr, x.lim_S)
        assert x.dmax <= 1e-9 * (1 + x.U), (name, e)
    laws = sb.record_laws(ref["contacts"], ref["n_contacts"], sb.mu_of_case(c, o), c.model.nb, c.kmax)
    for law, v in laws.items():
        assert not v.any(), (name, law, int(np.argmax(v)), v.max())


@pytest.mark.parametrize("name", sorted(set(sb.CASES) - set(CPU_CASES)))
def test_no_population_draws_a_joint_onto_a_stop(name):
    """the populations only the GPU tests run: which side of a stop a joint is on must not depend on the number format"""
    c = sb.case(name)
    sb.assert_no_joint_at_a_stop(c.model.blob, c.gc)


def test_the_populations_hold_the_envs_parity_cannot_reach():
    n = dict(unconverged=0, overflow=0, limited=0, self_collision=0, clipped=0)
    for name in CPU_CASES:
        c, o, ref, con, res = oracle_run(name)
        n["unconverged"] += int(((ref["flags"] & 4) != 0).sum())
        n["overflow"] += int(((ref["flags"] & 1) != 0).sum())
        n["limited"] += sum(x.limited for x in res)
        n["self_collision"] += sum(bool((k["collision"] & sb.SELF_A).any()) for k in con)
        n["clipped"] += sum(x.clipped for x in res)
    print(n)
    assert n["unconverged"] >= 100 and n["overflow"] >= 10 and n["limited"] >= 500 and n["self_collision"] >= 50 and n["clipped"] >= 30, n
    # the fuzz draws clip rarely: the population made for it meets the count alone, and holds PD joints beside the clipped ones in every env
    c, o, ref, con, res = oracle_run("anymal_clipped")
    assert sum(x.clipped for x in res) >= 30
    assert sum(0 < len(x.clipped_dofs) < 12 for x in res) >= 30


def test_converged_solves_end_at_the_normal_velocity_their_exit_test_leaves():
    """the figure the GPU tests' T comes from, on the oracle: a floating quadruped's converged solves leave |v_n+| below the exit threshold; a fixed base's
    compliance block leaves more, which is why T is taken per population"""
    for name, below in (("anymal_standing_lpe16", True), ("atlas_standing", True), ("fuzz_fixed5", False)):
        c, o, ref, _, _ = oracle_run(name)
        fig, n = sb.normal_figure(o, c.gc, ref["u"], ref["contacts"], ref["n_contacts"], (ref["flags"] & 5) == 0)
        print(f"{name}: {n} terrain contacts in converged envs, figure {fig:.2e}, T {sb.normal_bar(o, fig):.2e}")
        assert n > 50 and (fig < o.p.threshold) == below, (name, fig)


# ------------------------------------------------------------------------------------------------------------------------------ sensitivity
def _largest(con, pick=None):
    """index of the record with the largest impulse (among those pick() accepts), or None"""
    ks = [k for k in range(len(con)) if pick is None or pick(con[k])]
    return max(ks, key=lambda k: np.abs(con[k]["impulse"]).max()) if ks else None


def _mutations(c, o, e, con, clean, u0, u1_ref):
    """{mutation: (kwargs of balance_env that differ, change of A^-1 b it makes)} for env e; a mutation that does not apply is left out"""
    dt, blob = o.p.dt, c.model.blob
    kp, kd = c.kp.astype(np.float64), c.kd.astype(np.float64)
    out = {}
    k = _largest(con)
    if k is not None:
        m = con.copy(); m["impulse"][k] *= 1.01
        out["impulse x 1.01"] = dict(con=m)
        out["contact dropped"] = dict(con=np.delete(con, k))
    k = _largest(con, lambda r: r["body"] > 0)
    if k is not None:
        m = con.copy(); m["body"][k] = blob.parent[int(con[k]["body"])]
        out["body -> parent"] = dict(con=m)
    k = _largest(con, lambda r: (r["collision"] & sb.SELF_B) != 0)
    if k is not None:
        m = con.copy(); m["impulse"][k] *= -1.0
        out["SELF_B sign"] = dict(con=m)
    j0 = 6 if blob.fixed_base else 0
    free = [d for d in range(6, o.nv) if d - j0 not in clean.lim_row]          # (a joint outside L: its row is not zeroed)
    if free:
        u1 = u1_ref.copy(); u1[free[-1]] += 1e-3 * (1 + clean.U)
        out["u1 shifted"] = dict(u1=u1)
    B, clipped = sb.pd_diagonal(o, c.gc[e], u0, kp, kd, c.pt[e], c.dtg[e], None if c.tau_ff is None else c.tau_ff[e])
    inside = np.zeros(o.nv, bool); inside[free] = True
    if (clipped & inside).any() and c.mode == 1:
        d = int(np.nonzero(clipped & inside)[0][0]); m = B.copy(); m[d] = dt * (kd[d] + dt * kp[d])
        out["B on a clipped joint"] = dict(bdiag=m)
    if ((B > 0) & inside).any():
        d = int(np.argmax(B * inside)); m = B.copy(); m[d] = 0.0
        out["B off a PD joint"] = dict(bdiag=m)
    return out


def test_a_wrong_step_fails_the_balance():
    """The oracle's own outputs, mutated one way at a time.  In every env where the mutation moves A^-1 b (for the shifted u1: u1 itself) by more than
    twice the bar 2e-4 (1 + U), max |delta| exceeds the bar; and each mutation is detectable in that sense in at least a quarter of the envs it applies to.
    An env with a joint past a stop carries one unreported scalar on that joint's row, and what a mutation changes on that row alone the balance cannot
    see: a record moved from a body to its parent changes J^T lam on the row of the joint between them and nowhere else, and in a two-joint tree with
    both joints past a stop no row is left at all (with the change taken over all rows: 226 of 11 000 mutated envs, every one with such a joint, most of
    them `body -> parent`).  There the change of A^-1 b is taken with the rows of L zeroed, as delta is - a departure from the criterion as first
    stated -; the B mutations and the shifted u1 pick a joint outside L.
    What carries information: on a clean env r is zero to rounding, so for the contact and B mutations the mutated delta IS minus the change, and
    "change > 2 bar implies |delta| > bar" holds by construction (it guards the bookkeeping, not the physics).  The shifted u1 in envs with a joint past
    a stop is not of that kind (delta = A^-1 Z A e_d s with the rows of L zeroed by Z is not the shift s), and the counts say how often a 1 % impulse
    error, a lost contact or a wrong body is LARGE against the bar: that is the share of envs in which the GPU test can see such a fault at all.
    Measured: impulse x 1.01 detectable in 988 of 1669 envs, contact dropped 1075 of 1669, body -> parent 880 of 1631, SELF_B sign 197 of 345,
    u1 shifted 2848 of 2848, B on a clipped joint 126 of 143, B off a PD joint 1649 of 2848."""
    counts = {}
    for name in CPU_CASES:
        c, o, ref, cons, res = oracle_run(name)
        kp, kd = c.kp.astype(np.float64), c.kd.astype(np.float64)
        fixed = bool(c.model.blob.fixed_base)
        j0 = 6 if fixed else 0
        for e in range(c.N):
            u0 = c.gv[e].copy()
            if fixed:
                u0[:6] = 0.0
            clean = res[e]
            for what, kw in _mutations(c, o, e, cons[e], clean, u0, ref["u"][e]).items():
                args = dict(con=cons[e], u1=ref["u"][e], bdiag=None)
                args.update(kw)
                x = sb.balance_env(o, c.gc[e], c.gv[e], args["u1"], args["con"], kp, kd, c.pt[e], c.dtg[e], None if c.tau_ff is None else c.tau_ff[e],
                                   bdiag=args["bdiag"])
                bar = BAR * (1 + x.U)
                if "u1" in kw:
                    change = np.abs(args["u1"] - ref["u"][e]).max()
                elif not clean.limited:
                    change = np.abs(x.x - clean.x).max()
                else:       # the part of the change that no limit row's unreported scalar can take up
                    moved = (x.b - clean.b) - (x.A - clean.A) @ (ref["u"][e] - u0)[j0:]
                    moved[clean.lim_row] = 0.0
                    change = np.abs(np.linalg.solve(x.A, moved)).max()
                n = counts.setdefault(what, [0, 0])
                n[0] += 1
                if change > 2 * bar:
                    n[1] += 1
                    assert x.dmax > bar, (name, e, what, x.dmax, bar, change)
    print({k: f"{v[1]} detectable of {v[0]}" for k, v in counts.items()})
    assert len(counts) == 7, counts
    for what, (applies, detectable) in counts.items():
        assert applies >= 30 and detectable >= 0.25 * applies, (what, applies, detectable)
