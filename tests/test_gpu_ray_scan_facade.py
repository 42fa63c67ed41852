"""BatchedWorld::rayCast / rayScan / depthCameraRays through the C++ facade on the GPU (tests/cpp/ray_scan_facade_test.cpp): the sensor form
against the world-space form, the world-space form without bodies against rayTest bit for bit, the ground plane in closed form, the depth image
written into wider rows."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_ray_scan_facade_on_the_device(built_lib):
    from test_ray_scan_host import BIN, URDF, compile_ray_scan_facade
    compile_ray_scan_facade()
    r = subprocess.run([BIN, URDF], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ray_scan_facade_test OK" in r.stdout
