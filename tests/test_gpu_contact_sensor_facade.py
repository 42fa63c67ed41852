"""BatchedWorld::getBodyContactWrenches / getContactReadings / updateContactTimers through the C++ facade on the GPU
(tests/cpp/contact_sensor_facade_test.cpp): the batched members on host buffers against the loop they replace - per env, on the host, in double,
over ArticulatedSystem::getContacts() with the poses and velocities of the per-env views - at the bars of tests/test_gpu_contact_sensor.py."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_contact_sensor_facade_against_the_host_loop_over_get_contacts(built_lib):
    from test_contact_sensor_host import BIN, URDF, compile_contact_sensor_facade
    compile_contact_sensor_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "contact_sensor_facade_test OK" in r.stdout
