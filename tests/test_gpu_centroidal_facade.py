"""BatchedWorld::getCentroidal / getCentroidalMomentumMatrices through the C++ facade on the GPU (tests/cpp/centroidal_facade_test.cpp): the batched members
against the C-ABI they wrap, bit for bit, and every env of a 21-env ANYmal world against the per-env host accessors of ArticulatedSystem (getCOM,
getLinearMomentum, getAngularMomentum, getKineticEnergy, getPotentialEnergy, getEnergy) - a second formulation in double that shares no code with the
oracle - under the bounds of tests/test_gpu_centroidal.py."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_centroidal_facade_against_the_c_abi_and_the_per_env_host_accessors(built_lib):
    from test_centroidal_host import BIN, URDF, compile_centroidal_facade
    compile_centroidal_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "centroidal_facade_test OK" in r.stdout
