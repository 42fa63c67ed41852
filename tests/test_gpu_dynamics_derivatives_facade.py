"""BatchedWorld::inverseDynamicsDerivatives / forwardDynamicsDerivatives through the C++ facade on the GPU
(tests/cpp/dynamics_derivatives_facade_test.cpp): the batched members on host buffers against the C-ABI they wrap, bit for bit on ANYmal - on the
facade's own world and on a second world that received the same rows through rsb_set_state, so the rows staged through the per-env views must have
been uploaded first - null outputs skipped, and M dUdotDq + dTauDq = 0.  The Python methods: torch-on-device outputs carry the bits of numpy outputs."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_dynamics_derivatives_facade_against_the_c_abi(built_lib):
    from test_dynamics_derivatives_host import BIN, URDF, compile_facade
    compile_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dynamics_derivatives_facade_test OK" in r.stdout


def test_torch_outputs_equal_numpy_outputs(built_lib, anymal):
    """BatchedWorld.inverse_dynamics_derivatives / forward_dynamics_derivatives: fresh numpy outputs, caller's numpy outputs and caller's torch CUDA
    outputs (RSB_DEVICE, torch inputs) hold the same bits; only the outputs asked for come back"""
    import torch
    from raisimlib_amd import BatchedWorld, workload
    n = 23
    dev = torch.device("cuda:0")
    gc, gv = workload.random_state(anymal.nq, anymal.nv, n, seed=11)
    rng = np.random.default_rng(5)
    nv = anymal.nv
    udot, tau = rng.normal(size=(n, nv)).astype(np.float32), rng.normal(size=(n, nv)).astype(np.float32)
    frames = [(anymal.nb - 1, (0.05, -0.02, 0.1)), (3, (0.0, 0.04, -0.06))]
    force, torque = rng.normal(size=(n, 2, 3)).astype(np.float32), rng.normal(size=(n, 2, 3)).astype(np.float32)
    w = BatchedWorld(anymal, n)
    w.set_stream(torch.cuda.current_stream().cuda_stream)
    w.set_state(gc, gv)
    t = lambda a: torch.from_numpy(a).to(dev)
    a = w.inverse_dynamics_derivatives(udot, loads=(frames, force, torque), dq=True, dv=True, dudot=True)
    b = w.forward_dynamics_derivatives(tau, loads=(frames, force, torque), udot=True, dq=True, dv=True, dtau=True)
    assert sorted(a) == ["dq", "dudot", "dv"] and sorted(b) == ["dq", "dtau", "dv", "udot"]
    assert sorted(w.inverse_dynamics_derivatives(udot)) == ["dq", "dv"] and sorted(w.forward_dynamics_derivatives(tau)) == ["dq", "dv"]
    ta = {k: torch.full(v.shape, 7.0, dtype=torch.float32, device=dev) for k, v in a.items()}
    tb = {k: torch.full(v.shape, 7.0, dtype=torch.float32, device=dev) for k, v in b.items()}
    assert w.inverse_dynamics_derivatives(t(udot), loads=(frames, t(force), t(torque)), out=ta) is ta
    assert w.forward_dynamics_derivatives(t(tau), loads=(frames, t(force), t(torque)), out=tb) is tb
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(ta[k].cpu().numpy(), a[k]), k
    for k in b:
        assert np.array_equal(tb[k].cpu().numpy(), b[k]), k
    na = {k: np.full(v.shape, 7.0, np.float32) for k, v in a.items()}
    w.inverse_dynamics_derivatives(udot, loads=(frames, force, torque), out=na)
    for k in a:
        assert np.array_equal(na[k], a[k]), k
    with pytest.raises(ValueError):
        w.inverse_dynamics_derivatives(udot, out={"dq": ta["dq"], "dv": na["dv"]})
    w.close()
