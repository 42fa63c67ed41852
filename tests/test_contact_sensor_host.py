"""Batched contact sensors (include/rsb.h: rsb_get_body_contact_wrenches, rsb_contact_observe, rsb_contact_timers), CPU tier: the C-ABI declares,
exports and prototypes the entry points, the header's symbol map names them, the flag values stand in the header and in _capi, BatchedWorld has the
three methods and the facade its three members; a null world is refused with a message before anything is touched; the kernel of
raisimlib_amd/csrc/rsb_contact_sensor.hip cross-compiles for gfx950 with the build's flags into code without scratch, without spills, without AGPRs
and with at most 128 VGPRs (the compiler's own metadata, nothing else of the assembly is looked at); a C++ program written against the facade's new
members compiles with g++ -Wall -Werror, and the facade still links against the host double of the C-ABI, which does not define the new symbols.
tests/test_gpu_contact_sensor.py and tests/test_gpu_contact_sensor_facade.py run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_get_body_contact_wrenches", "rsb_contact_observe", "rsb_contact_timers")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BIN = os.path.join(BUILD, "contact_sensor_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("contact_sensor_kernel",)


def compile_contact_sensor_facade(compile_only=False):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "contact_sensor_facade_test.cpp")
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
    types = open(os.path.join(ROOT, "include", "rsb_types.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert hasattr(built_lib, name), name
        assert name in _capi.PROTOTYPES, name
    assert " *   rsb_get_body_contact_wrenches / rsb_contact_observe / rsb_contact_timers" in header      # the symbol map
    assert [len(_capi.PROTOTYPES[n][1]) for n in NEW_ENTRY_POINTS] == [8, 8, 11]
    assert (_capi.RSB_CONTACT_LOCAL, _capi.RSB_CONTACT_NO_SELF) == (1, 2)
    assert re.search(r"#define RSB_CONTACT_LOCAL\s+1\b", types) and re.search(r"#define RSB_CONTACT_NO_SELF\s+2\b", types)
    for meth in ("body_contact_wrenches", "contact_observe", "contact_timers"):
        assert callable(getattr(BatchedWorld, meth, None)), meth
    facade = open(os.path.join(ROOT, "include", "raisim", "World.hpp")).read()
    for member in ("getBodyContactWrenches", "getContactReadings", "updateContactTimers"):
        assert f"void {member}(" in facade, member


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a machine without a GPU can run this); the buffers keep their pattern"""
    from raisimlib_amd import _capi
    L = built_lib
    fr = (_capi.Frame * 1)()
    buf = (C.c_float * 64)(*([7.0] * 64))
    assert L.rsb_get_body_contact_wrenches(None, fr, 1, 0, buf, buf, buf, 0) == -1 and b"rsb_get_body_contact_wrenches: null world" in L.rsb_last_error()
    assert L.rsb_contact_observe(None, fr, 1, 0, 1.0, buf, 0, 0) == -1 and b"rsb_contact_observe: null world" in L.rsb_last_error()
    assert L.rsb_contact_timers(None, fr, 1, 0, 1.0, 0.02, None, buf, buf, buf, 0) == -1 and b"rsb_contact_timers: null world" in L.rsb_last_error()
    assert all(x == 7.0 for x in buf)


def test_contact_sensor_kernel_resources(tmp_path):
    """the kernel of rsb_contact_sensor.hip, as the compiler reports it in the code object's metadata: 0 bytes of scratch, 0 spilled VGPRs and SGPRs,
    no AGPRs, an allocation of at most 128 VGPRs"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library itself cannot have been built"
    assert "rsb_contact_sensor.hip" in rb.HOST_SOURCES and rb.HOST_SOURCES["rsb_contact_sensor.hip"] == rb.HOST_SOURCES["rsb_dynamics.hip"]
    out = tmp_path / "contact_sensor.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_contact_sensor.hip")], check=True, capture_output=True)
    txt = out.read_text()
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]      # one metadata record per kernel
    seen = []
    for b in blocks:
        name = re.search(r"\.name:\s*(\S+)", b).group(1)
        val = {k: int(re.search(rf"\.{k}:\s*(\d+)", b).group(1)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")}
        val["agpr_count"] = int(re.match(r"\s*(\d+)", b).group(1))
        print(name, val)
        seen.append(name)
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0 and val["sgpr_spill_count"] == 0, (name, val)
        assert val["agpr_count"] == 0 and val["vgpr_count"] <= 128, (name, val)      # min(8, 512 // allocation) >= 4 waves per SIMD
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_contact_sensor_facade_compiles_with_gxx(built_lib):
    compile_contact_sensor_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_contact_sensor_facade()
    if built_lib.rsb_device_count() > 0:
        return      # a GPU is visible: tests/test_gpu_contact_sensor_facade.py runs the program
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
