"""BatchedWorld::getFrameKinematics / getFrameJacobians / addExternalWrench through the C++ facade on the GPU (tests/cpp/frames_facade_test.cpp):
every env and body of a 16-env ANYmal world against the per-env host accessors of ArticulatedSystem - a second formulation in double that shares
no code with the oracle - and the batched wrench against setExternalForce + setExternalTorque per env on a twin world."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_frames_facade_against_the_per_env_host_accessors(built_lib):
    from test_frames_host import BIN, URDF, compile_frames_facade
    compile_frames_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frames_facade_test OK" in r.stdout
