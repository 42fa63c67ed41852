"""Batched inverse kinematics (include/rsb.h: rsb_inverse_kinematics), CPU tier: the C-ABI declares, exports and prototypes the entry point with its
constants and options struct, and BatchedWorld and the facade have their members; a null world is refused with a message before anything is touched;
raisimlib_amd/csrc/rsb_ik.hip cross-compiles for gfx950 with the build's flags into exactly the kernel it names, without scratch, without VGPR spills and
with at most 128 VGPRs + AGPRs (the compiler's own metadata; nothing else of the assembly is looked at), and its LDS arithmetic keeps the largest
case inside a workgroup's 64 KB; a C++ program written against the facade's new member compiles with g++ -Wall -Werror.  tests/test_gpu_ik.py and
tests/test_gpu_ik_facade.py run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

from common import ROOT

BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BIN = os.path.join(BUILD, "ik_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("ik_kernel",)


def compile_ik_facade(compile_only=False):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "ik_facade_test.cpp")
    head = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include")]
    if compile_only:
        subprocess.run([*head, "-c", "-o", BIN + ".o", src], check=True)
    else:
        subprocess.run([*head, "-o", BIN, src, "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_entry_point_is_declared_exported_and_prototyped(built_lib, tmp_path):
    from raisimlib_amd import BatchedWorld, _capi
    from test_capi_abi import header_functions
    name = "rsb_inverse_kinematics"
    header = open(os.path.join(ROOT, "include", "rsb.h")).read()
    types = open(os.path.join(ROOT, "include", "rsb_types.h")).read()
    assert name in header_functions() and hasattr(built_lib, name) and name in _capi.PROTOTYPES
    assert len(_capi.PROTOTYPES[name][1]) == 14
    assert " *   rsb_inverse_kinematics " in header      # the symbol map
    assert header.index("int rsb_frame_impulse(") < header.index("int rsb_inverse_kinematics(") < header.index("int rsb_get_terrain_height(")
    assert re.search(r"#define RSB_MAX_IK_FRAMES\s+RSB_MAX_DELASSUS_FRAMES\b", types)
    for macro, val in (("RSB_IK_ANGULAR", 1), ("RSB_IK_JOINT_LIMITS", 2), ("RSB_IK_CONVERGED", 0), ("RSB_IK_MAX_ITER", 1), ("RSB_IK_SINGULAR", 2)):
        assert re.search(rf"#define {macro}\s+{val}\b", types) and getattr(_capi, macro) == val, macro
    assert _capi.RSB_MAX_IK_FRAMES == _capi.RSB_MAX_DELASSUS_FRAMES == 16
    for word in ("RSB_HELD_PIVOT_TOL", "within 1e-6 of pi", "below about 1e-5"):      # the rule, the excluded angle and the float floor are stated at the declaration
        assert word in header, word
    assert callable(getattr(BatchedWorld, "inverse_kinematics", None))
    facade = open(os.path.join(ROOT, "include", "raisim", "World.hpp")).read()
    assert "void inverseKinematics(" in facade and facade.index("void constrainedForwardDynamics(") < facade.index("void inverseKinematics(")
    # the ctypes mirror of the options has the C compiler's layout
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsb.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(rsb_ik_options), '
                   'offsetof(rsb_ik_options, damping), offsetof(rsb_ik_options, max_step)); return 0; }\n')
    exe = tmp_path / "opt"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    O = _capi.IkOptions
    assert got == [C.sizeof(O), O.damping.offset, O.max_step.offset]


def test_entry_point_refuses_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a machine without a GPU can run this); the buffers keep their pattern"""
    from raisimlib_amd import _capi
    L = built_lib
    fr = (_capi.Frame * 1)()
    buf = (C.c_float * 64)(*([7.0] * 64))
    st = (C.c_int32 * 8)(*([7] * 8))
    opt = _capi.IkOptions(10, 1e-3, 1e-4, 1e-4, 0.5)
    assert L.rsb_inverse_kinematics(None, fr, 1, 0, buf, None, None, None, C.byref(opt), buf, buf, st, st, 0) == -1
    assert b"rsb_inverse_kinematics: null world" in L.rsb_last_error()
    assert all(x == 7.0 for x in buf) and all(x == 7 for x in st)


def test_ik_kernel_resources(tmp_path):
    """ik_kernel as the compiler reports it in the code object's metadata: the file holds exactly the kernel it names; 0 bytes of scratch, 0 spilled
    VGPRs, at most 128 VGPRs + AGPRs (4 waves per SIMD); its LDS is dynamic, so the file's own arithmetic is checked: the largest case is one env of
    less than 64 KB, the quadruped's four feet are sixteen envs per workgroup.  The kernel keeps the whole iteration - the chain walk with its
    sincosf, atan2f, the factorisation's loop bounds - in one loop, and the compiler parks some of the loop-invariant scalars in VGPR lanes (SGPR
    spills, printed here, 47 when this was written): register moves, no memory traffic, which is why scratch stays at 0."""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library itself cannot have been built"
    assert rb.HOST_SOURCES["rsb_ik.hip"] == rb._WORLD_DEPS + ["frames_chain.h"]
    out = tmp_path / "ik.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_ik.hip")], check=True, capture_output=True)
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
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0, (name, val)      # (SGPR spills go to VGPR lanes, not to memory: see the docstring)
        assert val["vgpr_count"] + val["agpr_count"] <= 128, (name, val)
        assert val["group_segment_fixed_size"] == 0, (name, val)
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen
    src = open(os.path.join(csrc, "rsb_ik.hip")).read()
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", src) == ["ik_kernel"]
    budget = int(re.search(r"kIkLdsFloats = (\d+);", src).group(1))
    assert budget * 4 + 1024 <= 65536

    def floats(m, nv, nq, nb, F):      # ik_shared + one env record (ik_layout), as the file computes them
        shared = nb * 20 + 2 * nb + 2 * 16 + 2 * 16 + 4 * 16 + 72
        pitch = (nq + nb * 7 + F * 8 + m * (nv | 1) + m * (m + 1) // 2 + 2 * m + nv) | 1
        return shared, pitch
    shared, pitch = floats(96, 69, 70, 64, 16)
    assert shared + pitch <= budget      # the largest model with the most rows: one env per workgroup
    shared, pitch = floats(12, 18, 19, 13, 4)
    assert (budget - shared) // pitch >= 16      # the quadruped's four feet: sixteen envs, the 256 threads' worth


def test_ik_facade_compiles_with_gxx(built_lib):
    compile_ik_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_ik_facade()
    if built_lib.rsb_device_count() > 0:
        return      # a GPU is visible: tests/test_gpu_ik_facade.py runs the program
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout
