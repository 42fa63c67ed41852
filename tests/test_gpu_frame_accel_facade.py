"""BatchedWorld::getFrameAccelerations / getFrameJacobianRates / getImuReadings through the C++ facade on the GPU
(tests/cpp/frame_accel_facade_test.cpp): the batched members on host buffers against the C-ABI they wrap, bit for bit - on a second world that
received the same rows through rsb_set_state, so the rows staged through the per-env views must have been uploaded first - and against the Python
path: the program writes its state, inputs and results to a file; a Python BatchedWorld given that state answers with the same bits."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_frame_accel_facade_against_the_c_abi_and_the_python_path(built_lib, anymal, tmp_path):
    from raisimlib_amd import BatchedWorld
    from test_frame_accel_host import BIN, URDF, compile_frame_accel_facade
    compile_frame_accel_facade()
    dump = tmp_path / "facade.bin"
    r = subprocess.run([BIN, URDF, str(dump)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frame_accel_facade_test OK" in r.stdout
    raw = dump.read_bytes()
    N, nq, nv, F = (int(x) for x in np.frombuffer(raw, np.int32, 4))
    assert (nq, nv) == (anymal.nq, anymal.nv)
    at = [16]

    def take(*shape):
        a = np.frombuffer(raw, np.float32, int(np.prod(shape)), at[0]).reshape(shape)
        at[0] += a.nbytes
        return a
    gc, gv, udot = take(N, nq), take(N, nv), take(N, nv)
    frames = []
    for _ in range(F):
        frames.append((int(np.frombuffer(raw, np.int32, 1, at[0])[0]), tuple(float(x) for x in np.frombuffer(raw, np.float32, 3, at[0] + 4))))
        at[0] += 16
    lin, ang, lin_lp, ang_lp = take(N, F, 3), take(N, F, 3), take(N, F, 3), take(N, F, 3)
    jl, jr, imu = take(N, F, 3, nv), take(N, F, 3, nv), take(N, F, 6)
    assert at[0] == len(raw)
    w = BatchedWorld(anymal, N)
    w.set_state(gc, gv)
    a = w.frame_accelerations(frames, udot, lin=True, ang=True)
    b = w.frame_accelerations(frames, udot, local=True, proper=True, lin=True, ang=True)
    j = w.frame_jacobian_rates(frames, lin=True, rot=True)
    m = w.imu_observe(frames, udot)
    w.close()
    assert np.array_equal(a["lin"], lin) and np.array_equal(a["ang"], ang)
    assert np.array_equal(b["lin"], lin_lp) and np.array_equal(b["ang"], ang_lp)
    assert np.array_equal(j["lin"], jl) and np.array_equal(j["rot"], jr)
    assert np.array_equal(m, imu) and np.abs(imu).max() > 0
