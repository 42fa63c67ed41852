"""What one launch of the step kernel should do travels in its request (rsbw::StepRequest, csrc/rsb_world.h), never through fields of the world:
a refused launch leaves nothing to the next one, RUNGE_KUTTA_4's contact step rewrites nothing of the world's configuration, and the done flags
of a launch are redirected without touching the world's own done output.  Every comparison is bit for bit (np.array_equal on gc and gv) against
a twin world that never made the call in question."""
import numpy as np
import pytest

from common import standing_states
from raisimlib_amd import BatchedWorld, Model, RsbError, workload

pytestmark = pytest.mark.gpu

N = 10          # ragged: 2.5 workgroups of four envs


def quadrupeds(anymal, seed, z=(0.46, 0.62)):
    """N ANYmals near the ground, PD mode with the workload's gains, targets of control step 0; (world, gc, gv)"""
    gc, gv = standing_states(N, seed=seed, z=z)
    kp, kd = workload.anymal_gains()
    w = BatchedWorld(anymal, N)
    w.set_pd_gains(kp, kd)
    w.set_pd_target(workload.anymal_targets(N, 0), np.zeros((N, 18), np.float32))
    w.set_state(gc, gv)
    return w, gc, gv


def same_state(a, b):
    (qa, ua), (qb, ub) = a.get_state(), b.get_state()
    return np.array_equal(qa, qb) and np.array_equal(ua, ub) and np.isfinite(qa).all() and np.isfinite(ua).all()


def test_refused_fused_step_leaves_nothing_behind(anymal):
    """RUNGE_KUTTA_4 refuses a fused control step.  The next plain integrate() must not inherit its targets, its obs gather or its reset."""
    import torch
    feet = np.asarray(anymal.collision_indices("_foot"), np.int32)
    w, gc, gv = quadrupeds(anymal, 31)
    twin, _, _ = quadrupeds(anymal, 31)
    other_gc, other_gv = standing_states(N, seed=32)
    g0 = torch.from_numpy(other_gc.astype(np.float32)).cuda()
    v0 = torch.from_numpy(other_gv.astype(np.float32)).cuda()
    pt = torch.from_numpy(workload.anymal_targets(N, 5).astype(np.float32)).cuda()      # (not the targets the world holds)
    obs = torch.full((N, w.obs_dim(len(feet))), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w.set_integration_scheme("runge_kutta_4")
    step = w.control_step_plan(4, obs.data_ptr(), feet, feet, g0.data_ptr(), v0.data_ptr(), N)
    with pytest.raises(RsbError, match="RUNGE_KUTTA_4"):
        step(pt.data_ptr())
    q, u = w.get_state()
    assert np.array_equal(q, gc.astype(np.float32)) and np.array_equal(u, gv.astype(np.float32))      # no env stepped, none reset
    w.set_integration_scheme("semi_implicit")
    w.integrate(4)
    twin.integrate(4)
    assert same_state(w, twin)
    assert np.array_equal(w.get_pd_target(), twin.get_pd_target())
    assert bool((obs == 7.0).all())
    assert np.array_equal(g0.cpu().numpy(), other_gc.astype(np.float32)) and np.array_equal(v0.cpu().numpy(), other_gv.astype(np.float32))
    w.close(); twin.close()


def test_refused_masked_launch_leaves_no_mask(built_lib):
    """Two contacts per primitive against a height map have no fixed-base kernel class: the masked launch is refused (test_api_errors).  Once the
    setting is taken back, a plain integrate() steps EVERY env."""
    from test_oracle_kat import FIXED_PENDULUM
    fixed = Model(urdf_string=FIXED_PENDULUM.format(l=0.5, m=1.0))
    n = 8
    gc = np.zeros((n, fixed.nq), np.float32); gc[:, 3] = 1; gc[:, -1] = 0.3 + 0.05 * np.arange(n)
    gv = np.zeros((n, fixed.nv), np.float32)
    worlds = []
    for refused in (True, False):
        w = BatchedWorld(fixed, n)
        w.add_height_map(5, 5, 4.0, 4.0, 0.0, 0.0, np.zeros((5, 5), np.float32))
        w.set_state(gc, gv)
        if refused:
            w.set_heightmap_contacts(2)
            with pytest.raises(RsbError, match="floating-base"):
                w.integrate_masked(np.arange(n) % 2, 1)
            w.set_heightmap_contacts(1)
        w.integrate(1)
        worlds.append(w)
    assert same_state(*worlds)
    assert (worlds[0].get_state()[1][:, -1] != 0).all()      # every env moved
    for w in worlds:
        w.close()


@pytest.mark.parametrize("masked", [False, True])
def test_rk4_contact_step_leaves_the_configuration_alone(anymal, masked):
    """RUNGE_KUTTA_4 runs its contact step in force mode, at theta = 1, without the effort clip and with d_tff read although the world knows it holds
    zeros.  None of that may outlive the launch: two sub-steps under RK4, then two under TRAPEZOID in PD mode, equal the same two phases run on a
    fresh world each (joined by set_state).  Warm starting is off: the fresh world of the second phase has no warm records to start from."""
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)

    def world(scheme, state=None):
        w, _, _ = quadrupeds(anymal, 33, z=(0.40, 0.52))      # (feet on the ground within the first sub-steps)
        w.set_solver_warm_start(False)
        w.set_integration_scheme("trapezoid")
        w.set_integration_scheme(scheme)
        if state is not None:
            w.set_state(*state)
        return w

    def rk4_phase(w):
        if masked:
            w.integrate_masked(mask, 2)
        else:
            w.integrate(2)

    w = world("runge_kutta_4")
    rk4_phase(w)
    w.set_integration_scheme("trapezoid")
    w.integrate(2)
    first = world("runge_kutta_4")
    rk4_phase(first)
    second = world("trapezoid", first.get_state())
    second.integrate(2)
    assert same_state(w, second)
    assert w.get_contacts()[0].sum() > 0, "no env touched the ground: the contact step had nothing to do"
    if masked:      # ... and the mask was the RK4 call's alone: the envs it held back have moved since
        q0 = standing_states(N, seed=33, z=(0.40, 0.52))[0].astype(np.float32)
        assert (w.get_state()[0][mask == 0] != q0[mask == 0]).any(axis=1).all()
    for x in (w, first, second):
        x.close()


def test_done_flags_of_the_k_step_fallback(anymal):
    """Without a resident launch rsb_control_steps runs K control steps and sends the done flags of step j to done_out + j * stride.  They equal
    those of K single control steps with rsb_set_done_output pointed at the slice - and the world's own done output is what it was before."""
    import torch
    K, stride, period = 3, N + 6, 4
    feet = np.asarray(anymal.collision_indices("_foot"), np.int32)
    bank = torch.from_numpy(np.stack([workload.anymal_targets(N, k).astype(np.float32) for k in range(period)])).cuda()
    worlds, own, flags = [], [], []
    for plan_k in (True, False):
        w, gc, gv = quadrupeds(anymal, 34)
        gc[::3, 2] = 0.1                                    # some envs start belly-down -> terminate and are reset
        w.set_state(gc, gv)
        w.set_step_residency(False)
        g0 = torch.from_numpy(gc.astype(np.float32)).cuda()
        v0 = torch.from_numpy(gv.astype(np.float32)).cuda()
        mine = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
        done = torch.full((K, stride), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        w.set_done_output(mine.data_ptr())
        one = w.control_step_plan(4, 0, feet, feet, g0.data_ptr(), v0.data_ptr(), N)
        if plan_k:
            w.control_steps_plan(4, bank.data_ptr(), period, 0, 0, feet, feet, g0.data_ptr(), v0.data_ptr(), N, done.data_ptr(), stride)(K, 0)
            w.synchronize()
            assert bool((mine == 7).all())                  # the world's own buffer was not written by the K steps ...
        else:
            for j in range(K):
                w.set_done_output(done[j].data_ptr())
                one(bank[j].data_ptr())
            w.set_done_output(mine.data_ptr())
        one(bank[K % period].data_ptr())                    # ... and is the done output again afterwards
        w.synchronize()
        worlds.append(w); own.append(mine.cpu().numpy()); flags.append(done.cpu().numpy())
    assert np.array_equal(flags[0], flags[1]) and (flags[0][:, N:] == 7).all() and (flags[0][:, :N] <= 1).all()
    assert flags[0][:, :N].sum() > 0, "no env terminated: the flags would all be zero"
    assert np.array_equal(own[0], own[1]) and (own[0] <= 1).all()
    assert same_state(*worlds)
    for w in worlds:
        w.close()
