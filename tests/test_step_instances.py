"""The step kernel's instance list (RSB_STEP_INSTANCES in raisimlib_amd/csrc/step_launch.h; no GPU): build.py reads it, and the library's launcher
table defines exactly its instances.  A launcher the table names but no object defines would link into the shared library all the same and only
fail when the library is loaded on a GPU machine: the undefined-reference check catches it here."""
import re
import shutil
import subprocess

import pytest

from raisimlib_amd import _capi, build as rb


def test_the_list_holds_the_classes_and_their_profiling_twins():
    inst = rb.step_instances()
    assert len(inst) == 106 and len({i[:4] for i in inst}) == 106
    assert sum(prof for *_, prof in inst) == 45
    # the profiling twins: every class but the peer-exchange (CL bit 2), the pipelined (16) and the resident (64) ones
    assert all(prof == (0 if cl & (2 | 16 | 64) else 1) for _, _, cl, _, prof in inst)
    assert {(16, 8, 0, 4, 1), (32, 16, 0, 12, 1), (16, 8, 64, 4, 0), (16, 8, 448, 4, 0), (32, 16, 320, 12, 0)} <= set(inst)
    assert (32, 16, 64, 4, 0) not in inst and (32, 16, 448, 12, 0) not in inst     # (no resident class for a shallow tree at 16 slots; no wide actor for the humanoid)


def _launchers(path, *flags):
    out = subprocess.run(["nm", "-C", *flags, path], check=True, capture_output=True, text=True).stdout
    pat = r"rsbk::launch_step_instance<(\d+), (\d+), (\d+), (\d+), (true|false)>"
    return {(int(a), int(b), int(c), int(d), int(p == "true")) for a, b, c, d, p in re.findall(pat, out)}


def test_the_library_defines_a_launcher_for_every_listed_instance_and_no_other(built_lib):
    if not shutil.which("nm"):
        pytest.skip("nm not available")
    want = {(lpe, kmax, cl, ml, p) for lpe, kmax, cl, ml, prof in rb.step_instances() for p in range(prof + 1)}
    assert len(want) == 151
    assert _launchers(_capi.LIB_PATH, "--defined-only") == want
    assert _launchers(_capi.LIB_PATH, "--undefined-only") == set()
