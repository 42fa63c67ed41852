"""Batched constrained dynamics and frame impulses (include/rsb.h: rsb_constrained_forward_dynamics, rsb_frame_impulse), CPU tier: the C-ABI declares,
exports and prototypes the entry points and BatchedWorld and the facade have their members; a null world is refused with a message before anything is
touched; raisimlib_amd/csrc/rsb_constrained.hip cross-compiles for gfx950 with the build's flags into exactly the kernel it names, without scratch,
without spills, within a workgroup's 64 KB of LDS and with at most 128 VGPRs + AGPRs (the compiler's own metadata; nothing else of the assembly is
looked at); a C++ program written against the facade's new members compiles with g++ -Wall -Werror.  tests/test_gpu_constrained.py and
tests/test_gpu_constrained_facade.py run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_constrained_forward_dynamics", "rsb_frame_impulse")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BIN = os.path.join(BUILD, "constrained_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("held_solve_kernel",)


def compile_constrained_facade(compile_only=False):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "constrained_facade_test.cpp")
    head = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include")]
    if compile_only:
        subprocess.run([*head, "-c", "-o", BIN + ".o", src], check=True)
    else:
        subprocess.run([*head, "-o", BIN, src, "-L", lib, "-lrsb", f"-Wl,-rpath,{lib}"], check=True)


def test_entry_points_are_declared_exported_and_prototyped(built_lib):
    from raisimlib_amd import BatchedWorld, _capi
    from test_capi_abi import header_functions
    declared = header_functions()
    header = open(os.path.join(ROOT, "include", "rsb.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name
    assert " *   rsb_constrained_forward_dynamics / rsb_frame_impulse" in header      # the symbol map
    assert [len(_capi.PROTOTYPES[n][1]) for n in NEW_ENTRY_POINTS] == [11, 11]
    assert header.index("int rsb_get_frame_delassus(") < header.index("int rsb_constrained_forward_dynamics(") < header.index("int rsb_frame_impulse(")
    types = open(os.path.join(ROOT, "include", "rsb_types.h")).read()
    assert (_capi.RSB_HELD_SOLVED, _capi.RSB_HELD_SINGULAR, _capi.RSB_HELD_PIVOT_TOL) == (0, 1, 1e-5)
    assert re.search(r"#define RSB_HELD_SINGULAR\s+1\b", types) and re.search(r"#define RSB_HELD_PIVOT_TOL\s+1e-5f\b", types)
    assert "RSB_HELD_PIVOT_TOL" in header      # the rule is stated where the functions are declared
    for meth in ("constrained_forward_dynamics", "frame_impulse"):
        assert callable(getattr(BatchedWorld, meth, None)), meth
    facade = open(os.path.join(ROOT, "include", "raisim", "World.hpp")).read()
    for member in ("constrainedForwardDynamics", "getFrameImpulse"):
        assert f"void {member}(" in facade, member
    assert facade.index("void getFrameDelassus(") < facade.index("void constrainedForwardDynamics(")


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a machine without a GPU can run this); the buffers keep their pattern"""
    from raisimlib_amd import _capi
    L = built_lib
    fr = (_capi.Frame * 1)()
    buf = (C.c_float * 64)(*([7.0] * 64))
    st = (C.c_int32 * 8)(*([7] * 8))
    assert L.rsb_constrained_forward_dynamics(None, buf, fr, 1, 0, buf, 0.0, buf, buf, st, 0) == -1
    assert b"rsb_constrained_forward_dynamics: null world" in L.rsb_last_error()
    assert L.rsb_frame_impulse(None, fr, 1, 0, buf, None, 0.0, buf, buf, st, 0) == -1 and b"rsb_frame_impulse: null world" in L.rsb_last_error()
    assert all(x == 7.0 for x in buf) and all(x == 7 for x in st)


def test_constrained_kernel_resources(tmp_path):
    """held_solve_kernel as the compiler reports it in the code object's metadata: the file holds exactly the kernels it names; 0 bytes of scratch,
    0 spilled VGPRs and SGPRs, at most 128 VGPRs + AGPRs (4 waves per SIMD), static LDS within a workgroup's 64 KB"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library itself cannot have been built"
    assert rb.HOST_SOURCES["rsb_constrained.hip"] == rb._WORLD_DEPS + ["frames_chain.h"]
    out = tmp_path / "constrained.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_constrained.hip")], check=True, capture_output=True)
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
        assert val["vgpr_count"] + val["agpr_count"] <= 128, (name, val)
        assert val["group_segment_fixed_size"] <= 65536, (name, val)
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_sibling_files_keep_their_kernels_and_the_launches_are_shared():
    """the composition reaches the siblings' kernels through launches declared in rsb_world.h, and the siblings' own entry points call the same
    launches: no kernel is launched from two places"""
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    world_h = open(os.path.join(csrc, "rsb_world.h")).read()
    for fn in ("launch_accel", "launch_frame_delassus", "launch_frame_kinematics", "launch_forward_dynamics"):
        assert re.search(rf"\b{fn}\(", world_h), fn
    for src, kernel in (("rsb_frame_accel.hip", "frame_accel_kernel"), ("rsb_inverse_mass.hip", "delassus_kernel"), ("rsb_frames.hip", "frame_kinematics_kernel")):
        txt = open(os.path.join(csrc, src)).read()
        assert len(re.findall(rf"hipLaunchKernelGGL\({kernel}\b", txt)) == 1, (src, kernel)
    mine = open(os.path.join(csrc, "rsb_constrained.hip")).read()
    assert re.findall(r"hipLaunchKernelGGL\((\w+)", mine) == ["held_solve_kernel"]


def test_constrained_facade_compiles_with_gxx(built_lib):
    compile_constrained_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_constrained_facade()
    if built_lib.rsb_device_count() > 0:
        return      # a GPU is visible: tests/test_gpu_constrained_facade.py runs the program
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout
