"""Batched frame kinematics, frame Jacobians and external wrenches (include/rsb.h: rsb_get_frame_kinematics, rsb_get_frame_jacobians,
rsb_add_external_wrench), CPU tier: the C-ABI declares, exports and prototypes the entry points and rsb_frame has the compiler's layout; the kernels of
raisimlib_amd/csrc/rsb_frames.hip cross-compile for gfx950 with the build's flags into code without scratch, without spills and with at most 128
VGPRs each (>= 4 waves per SIMD: they are short chains of dependent loads with nothing but other waves to hide latency with); a C++ program
written against the facade's new members compiles with g++, and the facade still links against the host double of the C-ABI, which does not
define the new symbols.  tests/test_gpu_frames.py and tests/test_gpu_frames_facade.py run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_get_frame_kinematics", "rsb_get_frame_jacobians", "rsb_add_external_wrench")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "frames_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("frame_kinematics_kernel", "frame_jacobians_kernel", "external_wrench_kernel")


def compile_frames_facade(compile_only=False):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "frames_facade_test.cpp")
    head = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include")]
    if compile_only:
        subprocess.run([*head, "-c", "-o", BIN + ".o", src], check=True)
    else:
        subprocess.run([*head, "-o", BIN, src, "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_entry_points_are_declared_exported_and_prototyped(built_lib):
    from raisimlib_amd import _capi
    from test_capi_abi import header_functions
    declared = header_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name
    for meth in ("frame_kinematics", "frame_jacobians", "add_external_wrench", "get_field"):
        from raisimlib_amd import BatchedWorld
        assert callable(getattr(BatchedWorld, meth, None)), meth


def test_rsb_frame_mirror_has_the_c_layout(tmp_path):
    from raisimlib_amd import _capi
    src = tmp_path / "sizes.c"
    src.write_text(r'''#include <stdio.h>
#include <stddef.h>
#include "rsb.h"
int main(void) { printf("%zu %zu %zu %d %d\n", sizeof(rsb_frame), offsetof(rsb_frame, body), offsetof(rsb_frame, offset), RSB_MAX_FRAMES, RSB_MAX_BODIES); return 0; }
''')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    F = _capi.Frame
    assert got[:3] == [16, 0, 4] == [C.sizeof(F), F.body.offset, F.offset.offset]
    assert got[3] == got[4] == 64 == _capi.RSB_MAX_FRAMES      # "every body" is one call


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a CPU box can run this)"""
    from raisimlib_amd import _capi
    L = built_lib
    fr = (_capi.Frame * 1)()
    buf = (C.c_float * 64)()
    assert L.rsb_get_frame_kinematics(None, fr, 1, buf, None, None, None, 0) == -1 and b"null world" in L.rsb_last_error()
    assert L.rsb_get_frame_jacobians(None, fr, 1, buf, None, 0) == -1
    assert L.rsb_add_external_wrench(None, fr, buf, None, None, 0) == -1


def test_frame_kernels_resources(tmp_path):
    """every kernel of rsb_frames.hip: 0 bytes of scratch, 0 spilled VGPRs, no scratch instruction, an allocation of at most 128 VGPRs"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "rsb_frames.hip" in rb.HOST_SOURCES
    out = tmp_path / "frames.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_frames.hip")], check=True, capture_output=True)
    txt = out.read_text()
    assert not re.search(r"\bscratch_", txt)
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]      # one metadata record per kernel
    seen = []
    for b in blocks:
        name = re.search(r"\.name:\s*(\S+)", b).group(1)
        val = {k: int(re.search(rf"\.{k}:\s*(\d+)", b).group(1)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "sgpr_spill_count")}
        seen.append(name)
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0, (name, val)
        assert val["vgpr_count"] <= 128, (name, val)      # min(8, 512 // allocation) >= 4 waves per SIMD
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_frames_facade_compiles_with_gxx(built_lib):
    compile_frames_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_frames_facade()
    if built_lib.rsb_device_count() > 0:
        pytest.skip("a GPU is visible: covered by the gpu test")
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout


def test_facade_still_links_against_the_host_double():
    """tests/cpp/rsb_host_double.cpp does not define the new entry points: the facade's new members are plain inline members that nothing the
    existing code uses refers to, so the host-double program links and runs as before"""
    from test_cpp_facade import test_facade_host_side_against_the_c_abi_double
    double = open(os.path.join(ROOT, "tests", "cpp", "rsb_host_double.cpp")).read()
    for name in NEW_ENTRY_POINTS:
        assert name not in double
    test_facade_host_side_against_the_c_abi_double()
