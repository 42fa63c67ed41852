"""BatchedWorld::inverseKinematics through the C++ facade on the GPU (tests/cpp/ik_facade_test.cpp): the member on host buffers against the C-ABI it
wraps, bit for bit - on the facade's own world and on a second world that received the same rows through rsb_set_state, so the rows staged through
the per-env views must have been uploaded first - null outputs skipped, the four feet brought to reachable targets on every env."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_ik_facade_against_the_c_abi(built_lib):
    from test_ik_host import BIN, URDF, compile_ik_facade
    compile_ik_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ik_facade_test OK" in r.stdout
