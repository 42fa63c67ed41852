"""Batched derivatives of inverse and forward dynamics (include/rsb.h: rsb_inverse_dynamics_derivatives, rsb_forward_dynamics_derivatives), CPU tier:
the C-ABI declares, exports and prototypes the entry points and BatchedWorld has the two methods; a null world and a bad space are refused with a
message before anything is touched; the kernels of raisimlib_amd/csrc/rsb_dynamics_derivatives.hip cross-compile for gfx950 with the build's flags
into code without scratch, without spills and within a workgroup's 64 KB of static LDS (the compiler's own metadata; nothing else of the assembly is
looked at); a C++ program written against the facade's new members compiles with g++ -Wall -Werror.  tests/test_gpu_dynamics_derivatives.py and
tests/test_gpu_dynamics_derivatives_facade.py run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_inverse_dynamics_derivatives", "rsb_forward_dynamics_derivatives")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BIN = os.path.join(BUILD, "dynamics_derivatives_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("tangent_kernel", "identity_kernel", "transpose_kernel")


def compile_facade(compile_only=False):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "dynamics_derivatives_facade_test.cpp")
    head = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include")]
    if compile_only:
        subprocess.run([*head, "-c", "-o", BIN + ".o", src], check=True)
    else:
        subprocess.run([*head, "-o", BIN, src, "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_entry_points_are_declared_exported_and_prototyped(built_lib):
    from raisimlib_amd import BatchedWorld, _capi
    from test_capi_abi import header_functions
    declared = header_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name
    assert len(_capi.PROTOTYPES["rsb_inverse_dynamics_derivatives"][1]) == 11 and len(_capi.PROTOTYPES["rsb_forward_dynamics_derivatives"][1]) == 12
    for meth in ("inverse_dynamics_derivatives", "forward_dynamics_derivatives"):
        assert callable(getattr(BatchedWorld, meth, None)), meth


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message naming the function (a CPU box can run this); the outputs keep their pattern"""
    L = built_lib
    buf = (C.c_float * 64)(*([7.0] * 64))
    assert L.rsb_inverse_dynamics_derivatives(None, None, None, 0, None, None, 0, buf, buf, buf, 0) == -1
    assert b"rsb_inverse_dynamics_derivatives: null world" in L.rsb_last_error()
    assert L.rsb_forward_dynamics_derivatives(None, None, None, 0, None, None, 0, buf, buf, buf, buf, 0) == -1
    assert b"rsb_forward_dynamics_derivatives: null world" in L.rsb_last_error()
    assert all(x == 7.0 for x in buf)


def test_derivative_kernels_resources(tmp_path):
    """the kernels of rsb_dynamics_derivatives.hip, as the compiler reports them in the code object's metadata: 0 bytes of scratch, 0 spilled VGPRs
    and SGPRs, static LDS (sized for 64 bodies, whatever the depth of the tree) within a workgroup's 64 KB, and for tangent_kernel an allocation of at
    most 168 VGPRs + AGPRs: three waves per SIMD, what its LDS allows as well"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = "rsb_dynamics_derivatives.hip"
    assert src in rb.HOST_SOURCES and "frames_chain.h" in rb.HOST_SOURCES[src]
    out = tmp_path / "derivatives.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, src)], check=True, capture_output=True)
    txt = out.read_text()
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]      # one metadata record per kernel
    seen = []
    for b in blocks:
        name = re.search(r"\.name:\s*(\S+)", b).group(1)
        val = {k: int(re.search(rf"\.{k}:\s*(\d+)", b).group(1)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "group_segment_fixed_size")}
        val["agpr_count"] = int(re.match(r"\s*(\d+)", b).group(1))
        print(name, val)
        seen.append(name)
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0 and val["sgpr_spill_count"] == 0, (name, val)
        assert val["vgpr_count"] + val["agpr_count"] <= 168, (name, val)
        assert val["group_segment_fixed_size"] <= 65536, (name, val)
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_derivatives_facade_compiles_with_gxx(built_lib):
    compile_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_facade()
    if built_lib.rsb_device_count() > 0:
        return      # a GPU is visible: tests/test_gpu_dynamics_derivatives_facade.py runs the program
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout
