"""Batched centre of mass, momentum, energy and the centroidal momentum matrix (include/rsb.h: rsb_get_centroidal, rsb_get_centroidal_momentum_matrix),
CPU tier: the C-ABI declares, exports and prototypes the entry points and BatchedWorld has the two methods; a null world is refused with a message; the
kernels of raisimlib_amd/csrc/rsb_centroidal.hip cross-compile for gfx950 with the build's flags into code without scratch, without spills and with at
most 128 VGPRs each (the compiler's own metadata; nothing else of the assembly is looked at); a C++ program written against the facade's new members
compiles with g++ -Wall -Werror; the per-env host accessors of raisim::ArticulatedSystem match closed forms through the host double of the C-ABI
(tests/cpp/centroidal_host_test.cpp), which does not define the new symbols.  tests/test_gpu_centroidal.py and tests/test_gpu_centroidal_facade.py
run all of it on the GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from common import ROOT

NEW_ENTRY_POINTS = ("rsb_get_centroidal", "rsb_get_centroidal_momentum_matrix")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
BIN = os.path.join(BUILD, "centroidal_facade_test")
URDF = os.path.join(ROOT, "raisimlib_amd", "rsc", "anymal_c_like.urdf")
KERNELS = ("centroidal_kernel", "centroidal_matrix_kernel")


def compile_centroidal_facade(compile_only=False):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(ROOT, "raisimlib_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "centroidal_facade_test.cpp")
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
    assert len(_capi.PROTOTYPES["rsb_get_centroidal"][1]) == 8 and len(_capi.PROTOTYPES["rsb_get_centroidal_momentum_matrix"][1]) == 3
    for meth in ("centroidal", "centroidal_momentum_matrix"):
        assert callable(getattr(BatchedWorld, meth, None)), meth


def test_entry_points_refuse_a_null_world(built_lib):
    """no world, no device work: RSB_E_INVALID and a message (a CPU box can run this)"""
    L = built_lib
    buf = (C.c_float * 64)()
    assert L.rsb_get_centroidal(None, buf, None, None, None, None, None, 0) == -1 and b"rsb_get_centroidal: null world" in L.rsb_last_error()
    assert L.rsb_get_centroidal_momentum_matrix(None, buf, 0) == -1 and b"rsb_get_centroidal_momentum_matrix: null world" in L.rsb_last_error()
    assert all(x == 0.0 for x in buf)


def test_centroidal_kernels_resources(tmp_path):
    """both kernels of rsb_centroidal.hip, as the compiler reports them in the code object's metadata: 0 bytes of scratch, 0 spilled VGPRs, an
    allocation of at most 128 VGPRs, and static LDS (sized for 64 bodies, whatever the depth of the tree) within a workgroup's 64 KB"""
    from raisimlib_amd import build as rb
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "rsb_centroidal.hip" in rb.HOST_SOURCES and "frames_chain.h" in rb.HOST_SOURCES["rsb_centroidal.hip"]
    out = tmp_path / "centroidal.s"
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    subprocess.run([hipcc, *rb.FLAGS, "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", csrc, "--cuda-device-only", "-S", "-o", str(out),
                    os.path.join(csrc, "rsb_centroidal.hip")], check=True, capture_output=True)
    txt = out.read_text()
    meta = txt[txt.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]      # one metadata record per kernel
    seen = []
    for b in blocks:
        name = re.search(r"\.name:\s*(\S+)", b).group(1)
        val = {k: int(re.search(rf"\.{k}:\s*(\d+)", b).group(1)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "group_segment_fixed_size")}
        print(name, val)
        seen.append(name)
        assert val["private_segment_fixed_size"] == 0 and val["vgpr_spill_count"] == 0, (name, val)
        assert val["vgpr_count"] <= 128, (name, val)
        assert val["group_segment_fixed_size"] <= 65536, (name, val)
    assert len(seen) == len(KERNELS) and all(any(k in n for n in seen) for k in KERNELS), seen


def test_centroidal_facade_compiles_with_gxx(built_lib):
    compile_centroidal_facade(compile_only=True)      # g++ -std=c++17 -Wall -Werror, compile only
    compile_centroidal_facade()
    if built_lib.rsb_device_count() > 0:
        return      # a GPU is visible: tests/test_gpu_centroidal_facade.py runs the program
    r = subprocess.run([BIN, URDF], capture_output=True, text=True)
    assert r.returncode == 1 and "no HIP device" in r.stdout


def test_per_env_accessors_match_closed_forms_through_the_host_double(tmp_path):
    """getCOM / getLinearMomentum / getAngularMomentum / getKineticEnergy / getPotentialEnergy / getEnergy of one env, computed on the host in double
    from the env's row: a free body (com = p + R c, P = m v_c, L_c = R I R^T w, T = 1/2 m v_c^2 + 1/2 w . I_w w, U = -m g . c) and a two-link arm on a
    `world` root whose base entries of gv are ignored.  The program links tests/cpp/rsb_host_double.cpp, which does not define the new entry points:
    the facade's batched members are inline members nothing here refers to."""
    double = open(os.path.join(ROOT, "tests", "cpp", "rsb_host_double.cpp")).read()
    for name in NEW_ENTRY_POINTS:
        assert name not in double
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "centroidal_host_test")
    csrc = os.path.join(ROOT, "raisimlib_amd", "csrc")
    head = ["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc]
    subprocess.run([*head, "-Wall", "-Werror", "-c", "-o", exe + ".o", os.path.join(ROOT, "tests", "cpp", "centroidal_host_test.cpp")], check=True)
    subprocess.run([*head, "-o", exe, exe + ".o", os.path.join(ROOT, "tests", "cpp", "rsb_host_double.cpp"),
                    os.path.join(csrc, "urdf_model.cpp"), os.path.join(csrc, "terrain_io.cpp"), "-lz"], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "centroidal_host_test OK" in r.stdout, r.stdout + r.stderr


def test_eigen_overloads_compile(tmp_path):
    """the Eigen-typed overloads of the new accessors meet a compiler (tests/cpp/eigen_stub stands in for Eigen3)"""
    src = tmp_path / "eigen_centroidal.cpp"
    src.write_text(r'''#include <Eigen/Core>
#include "raisim/World.hpp"
double use(raisim::ArticulatedSystem& a) {
  Eigen::Vector3d p, l, ref, g;
  ref << 0.0, 0.0, 0.0;
  g << 0.0, 0.0, -9.81;
  a.getLinearMomentum(p);
  a.getAngularMomentum(ref, l);
  return a.getPotentialEnergy(g) + a.getEnergy(g) + p[0] + l[0] + a.getCOM()[2] + a.getKineticEnergy();
}
''')
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp", "eigen_stub"),
                    "-c", "-o", str(tmp_path / "eigen_centroidal.o"), str(src)], check=True)
