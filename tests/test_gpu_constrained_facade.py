"""BatchedWorld::constrainedForwardDynamics / getFrameImpulse through the C++ facade on the GPU (tests/cpp/constrained_facade_test.cpp): the batched
members on host buffers against the C-ABI they wrap, bit for bit - on the facade's own world and on a second world that received the same rows
through rsb_set_state, so the rows staged through the per-env views must have been uploaded first - null outputs skipped, the four feet held do not
accelerate, six rows per foot are refused without damping and solved with it."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_constrained_facade_against_the_c_abi(built_lib):
    from test_constrained_host import BIN, URDF, compile_constrained_facade
    compile_constrained_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "constrained_facade_test OK" in r.stdout
