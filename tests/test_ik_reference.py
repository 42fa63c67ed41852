"""The inverse-kinematics iteration restated in numpy float32 (tests/ik_reference.restate), CPU tier, before any device run.

The convergence condition: on every env of every variant the restatement reaches RSB_IK_CONVERGED in at most HALF of the max_iter the GPU tests use
(30, with damping 1e-3, max_step 0.5, tolerances 1e-4), and its float32 result meets the GPU tests' residual bars when evaluated in fp64.  A condition,
not a measurement: a variant that does not meet it gets a smaller delta (ik_reference.DELTA), never a larger cap.
Sensitivity: with the rotation rows negated, with the base quaternion multiplied on the right, and with a held column left in J, the same check fails.
The restatement's Jacobian and rows are pinned against the fp64 reference's on the way."""
import numpy as np
import pytest

import ik_reference as ik
from test_dynamics_reference import dyn_case, jacobians, kinematics


def residual_check(name, v, q, st, it, cap):
    """-> (every env converged within cap and inside both bars, the figures)"""
    key, angular, base_free = v
    pr = ik.problem(name, *v)
    ep, er, tmax = ik.evaluate(name, key, q, pr.target_pos, pr.target_rot)
    bp, br = ik.bars(tmax, angular)
    fig = dict(iters=int(it.max()), unconverged=int((st != ik.CONVERGED).sum()), pos=float((ep / bp).max()), rot=float((er / br).max()) if angular else 0.0)
    return fig["unconverged"] == 0 and fig["iters"] <= cap and fig["pos"] <= 1.0 and fig["rot"] <= 1.0, fig


def test_row_count_classes_are_covered(built_lib):
    ms = {ik.rows_of(n, k, a) for n in ik.CASES for k, a, _ in ik.variants(n)}
    assert {3, 12, 6, 24} <= ms and any(32 < m <= 64 for m in ms) and any(m > 64 for m in ms), sorted(ms)
    for n in ik.CASES:
        c = dyn_case(n)
        assert c.N == (67 if n in ("floating0", "fixed2") else 64)
        assert {f for _, _, f in ik.variants(n)} == ({False} if c.fixed else {False, True})


@pytest.mark.parametrize("name", ik.CASES)
def test_restatement_converges_in_half_the_cap(built_lib, name):
    print()
    for v in ik.variants(name):
        q, err, it, st = ik.restated(name, *v)
        ok, fig = residual_check(name, v, q, st, it, ik.MAX_ITER // 2)
        print(f"  {name} {v} m={ik.rows_of(name, v[0], v[1])}: {fig}")
        assert ok, (name, v, fig)
        pr = ik.problem(name, *v)      # what is not free keeps the start's bits
        held = np.ones(dyn_case(name).model.nq, bool)
        free = ik.free_columns(name, v[2])
        held[:3] = ~free[:3]; held[3:7] = not free[3:6].any(); held[7:] = ~free[6:]
        assert q[:, held].tobytes() == pr.start[:, held].tobytes()
        # the reported error is the fp64 evaluation's within the bars' added terms
        ep, er, tmax = ik.evaluate(name, v[0], q, pr.target_pos, pr.target_rot)
        assert (np.abs(err[:, 0] - ep) <= ik.POS_BAR * (1 + tmax)).all() and (np.abs(err[:, 1] - er) <= ik.ROT_BAR).all()


@pytest.mark.parametrize("wrong,name,v", [("rot_sign", "anymal", ("feet", True, False)), ("quat_right", "floating0", ("one", True, True)),
                                          ("unmasked", "anymal", ("feet", False, False))])
def test_a_broken_convention_fails_the_residual_check(built_lib, wrong, name, v):
    pr = ik.problem(name, *v)
    args = (name, v[0], pr.start, pr.target_pos, pr.target_rot, ik.dof_mask(name, v[2]))
    q, _, it, st = ik.restate(*args)
    assert residual_check(name, v, q, st, it, ik.MAX_ITER)[0]
    q, _, it, st = ik.restate(*args, wrong=wrong)
    ok, fig = residual_check(name, v, q, st, it, ik.MAX_ITER)
    print(wrong, fig)
    assert not ok, (wrong, fig)


@pytest.mark.parametrize("name", ["fixed2", "anymal"])
def test_restated_jacobian_and_rows_match_fp64(built_lib, name):
    c = dyn_case(name)
    key, angular, base_free = ik.variants(name)[-1]
    frames, pr = ik.frame_sets(name)[key], ik.problem(name, key, angular, base_free)
    R, p, a = ik._kin32(c.blob, pr.start)
    tp = pr.target_pos.reshape(c.N, len(frames), 3)
    tr = pr.target_rot.reshape(c.N, len(frames), 9)
    e32, pts = ik._rows32(R, p, frames, tp, tr, 1.0)
    J32 = ik._jac32(c.blob, c.fixed, p, a, frames, pts, 6, np.ones(c.nv, bool))
    for e in range(0, c.N, 9):
        k = kinematics(c.blob, pr.start[e].astype(float))
        for f, (b, off) in enumerate(frames):
            pt = k.p[b] + k.R[b] @ np.asarray(off, float)
            Jl, Jr = jacobians(c.blob, k, b, pt)
            assert np.abs(J32[e, 6 * f:6 * f + 3] - Jl).max() <= 1e-5 and np.abs(J32[e, 6 * f + 3:6 * f + 6] - Jr).max() <= 1e-5
            assert np.abs(e32[e, 6 * f:6 * f + 3] - (tp[e, f] - pt)).max() <= 1e-5
            assert np.abs(e32[e, 6 * f + 3:6 * f + 6] - ik.rot_vector(tr[e, f].reshape(3, 3).astype(float) @ k.R[b].T)).max() <= 6e-5
