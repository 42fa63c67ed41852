"""Ray casts and sensor-mounted ray scans that also hit the robot (include/rsb.h: rsb_ray_cast, rsb_ray_scan), CPU tier: the C-ABI declares,
exports and prototypes the entry points and the Python layer has its methods and pattern helpers; the constants of rsb_types.h are those of
_capi; a null world is refused with a message; the kernels of raisimlib_amd/csrc/rsb_ray_scan.hip cross-compile for gfx950 with the build's flags
into code without scratch, without spills and with at most 128 VGPRs each - the bar tests/test_terrain_query_host.py sets, checked the same way;
a C++ program written against the facade's new members compiles with g++ -Wall -Werror.  tests/test_gpu_ray_scan.py runs all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_ray_cast", "rsb_ray_scan")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "ray_scan_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("ray_scan_kernel", "ray_cast_kernel")


def compile_ray_scan_facade(compile_only=False):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "ray_scan_facade_test.cpp")
    head = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include")]
    if compile_only:
        subprocess.run([*head, "-c", "-o", BIN + ".o", src], check=True)
    else:
        subprocess.run([*head, "-o", BIN, src, "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_entry_points_are_declared_exported_and_prototyped(built_lib):
    import raisimlib_amd
    from raisimlib_amd import BatchedWorld, _capi
    from test_capi_abi import header_functions
    declared = header_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name
    for meth in ("ray_cast", "ray_scan"):
        assert callable(getattr(BatchedWorld, meth, None)), meth
    for helper in ("depth_camera_rays", "lidar_rays"):
        assert callable(getattr(raisimlib_amd, helper, None)), helper


def test_pattern_helpers():
    from raisimlib_amd import depth_camera_rays, lidar_rays
    W, H, hfov = 7, 4, 1.2
    d = depth_camera_rays(W, H, hfov)
    assert d.shape == (W * H, 3) and d.dtype == np.float32
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6) and np.all(d[:, 0] > 0)
    img = d.reshape(H, W, 3)
    assert np.all(img[:, 0, 1] > 0) and np.all(img[:, -1, 1] < 0) and np.all(img[0, :, 2] > 0) and np.all(img[-1, :, 2] < 0)      # y left, z up; row 0 on top
    assert np.allclose(img[:, ::-1, 1], -img[:, :, 1], atol=1e-6) and np.allclose(img[::-1, :, 2], -img[:, :, 2], atol=1e-6)
    assert np.allclose(img[:, W // 2, 1], 0.0, atol=1e-7)      # the middle column of an odd width looks straight ahead
    # pinhole, square pixels: y / x and z / x step by one pixel = 2 tan(hfov / 2) / W, and the image's edge is at hfov / 2
    step = 2 * np.tan(hfov / 2) / W
    assert np.allclose(np.diff(img[..., 1] / img[..., 0], axis=1), -step, atol=1e-6) and np.allclose(np.diff(img[..., 2] / img[..., 0], axis=0), -step, atol=1e-6)
    assert np.isclose(img[0, 0, 1] / img[0, 0, 0] + step / 2, np.tan(hfov / 2), atol=1e-6)
    el = [-0.3, 0.0, 0.2]
    lr = lidar_rays(8, el)
    assert lr.shape == (24, 3) and np.allclose(np.linalg.norm(lr, axis=1), 1.0, atol=1e-6)
    assert np.allclose(lr.reshape(3, 8, 3)[:, :, 2], np.sin(el)[:, None], atol=1e-6)
    assert np.allclose(lr[8], [1, 0, 0], atol=1e-6) and np.allclose(lr[10], [0, 1, 0], atol=1e-6)      # from +x, counter-clockwise
    with pytest.raises(ValueError):
        depth_camera_rays(0, 4, 1.0)
    with pytest.raises(ValueError):
        lidar_rays(4, [])


def test_ray_constants_match_the_header(tmp_path):
    from raisimlib_amd import _capi
    src = tmp_path / "consts.c"
    src.write_text(r'''#include <stdio.h>
#include "rsb.h"
int main(void) { printf("%d %d %d %d %d %d %d\n", RSB_MAX_RAY_POINTS, RSB_RAY_BODIES, RSB_RAY_OWN_BODY, RSB_RAY_PLANAR, RSB_RAY_MISS_MAX, RSB_RAY_HIT_NONE, RSB_RAY_HIT_TERRAIN); return 0; }
''')
    exe = tmp_path / "consts"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [4096, 1, 2, 4, 8, -1, -2] == [_capi.RSB_MAX_RAY_POINTS, _capi.RSB_RAY_BODIES, _capi.RSB_RAY_OWN_BODY, _capi.RSB_RAY_PLANAR, _capi.RSB_RAY_MISS_MAX,
                                                 _capi.RSB_RAY_HIT_NONE, _capi.RSB_RAY_HIT_TERRAIN]


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a CPU box can run this)"""
    from raisimlib_amd import _capi
    L = built_lib
    fr = (_capi.Frame * 1)()
    buf = (C.c_float * 64)()
    assert L.rsb_ray_cast(None, buf, buf, 1, 1.0, 1, buf, None, 0) == -1 and b"rsb_ray_cast: null world" in L.rsb_last_error()
    assert L.rsb_ray_scan(None, fr, 1, buf, 1, 1, 1.0, buf, 0, None, 0) == -1 and b"rsb_ray_scan: null world" in L.rsb_last_error()


def test_ray_scan_kernels_resources(tmp_path):
    """every kernel of rsb_ray_scan.hip: 0 bytes of scratch, 0 spilled VGPRs, no scratch instruction, an allocation of at most 128 VGPRs"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "rsb_ray_scan.hip" in rb.HOST_SOURCES and "terrain_ray.h" in rb.HOST_SOURCES["rsb_ray_scan.hip"]
    out = tmp_path / "ray_scan.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_ray_scan.hip")], check=True, capture_output=True)
    txt = out.read_text()
    assert not re.search(r"\bscratch_", txt)
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]      # one metadata record per kernel
    seen = []
    for b in blocks:
        name = re.search(r"\.name:\s*(\S+)", b).group(1)
        val = {k: int(re.search(rf"\.{k}:\s*(\d+)", b).group(1)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
        seen.append(name)
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0 and val["sgpr_spill_count"] == 0, (name, val)
        assert val["vgpr_count"] <= 128, (name, val)      # min(8, 512 // allocation) >= 4 waves per SIMD
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_the_new_kernels_share_the_chain_walk_the_surface_and_one_march():
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    rs = open(os.path.join(csrc, "rsb_ray_scan.hip")).read()
    for header in ("frames_chain.h", "step_terrain.h", "terrain_ray.h"):
        assert f'#include "{header}"' in rs, header
    assert rs.count("rsbk::terrain_eval(") == 1 and rs.count("rsbk::heightmap_ray(") == 1 and "walk_chain<false>(" in rs
    assert "for (int it = 0; it < xs + ys; ++it)" not in rs      # the cell walk itself lives in terrain_ray.h


def test_ray_scan_facade_compiles_with_gxx(built_lib):
    compile_ray_scan_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_ray_scan_facade()
    if built_lib.rsb_device_count() > 0:
        pytest.skip("a GPU is visible: covered by the gpu test")
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout
