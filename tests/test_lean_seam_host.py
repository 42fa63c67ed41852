"""Static shape of the lean seam (raisimlib_amd/csrc/step_spec.h RSB_LEAN_SEAM, step_phase_seam_lean.inc), read off the compiler's assembly of the benchmark's
specialised resident class <16, 8, 64, 4> (hipcc -S, no GPU), with and without -DRSB_X_NO_LEAN_SEAM: both compile without scratch; the path a control step that is
not the launch's last takes through the lean kernel has fewer scalar loads, fewer branches and fewer loops than the generic epilogue and boundary code, which the
lean kernel still holds for the last control step (the two paths are told apart by comment lines the kernel leaves in its assembly; the generic code is what the
twin runs in every control step); the switch names a kernel of its own there and changes nothing in the plain and pipelined classes.  The counts themselves are in
DESIGN.md; only the inequalities are asserted."""
import os
import re
import subprocess

import pytest

from raisimlib_amd import build as _b
from test_kernel_budget import _manifest_defs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "-DRSB_X_NO_LEAN_SEAM"


def _assembly(cl, defs, out):
    cmd = ["/opt/rocm/bin/hipcc", *[f for f in _b.FLAGS if f not in ("-fPIC", "-Wall", "-Wno-unused-function")], "-I", os.path.join(ROOT, "include"), "-I", _b.CSRC,
           "-DRSB_I_LPE=16", "-DRSB_I_KMAX=8", f"-DRSB_I_CL={cl}", "-DRSB_I_ML=4", "-DRSB_I_PROF=0", *defs, "--cuda-device-only", "-S", "-o", out,
           os.path.join(_b.CSRC, "step_instance.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = open(out).read()
    os.remove(out)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "", txt)      # (the compilation unit's id differs from run to run)


def _scratch(txt):
    return int(re.search(r"^\s+\.private_segment_fixed_size:\s+(\d+)", txt, re.M).group(1))


def _region(txt, name):
    """instruction counts between the comment lines `; rsb <name> begin` and `; rsb <name> end` (or the function's end, where the block layout put the end first)"""
    lines = txt.split("\n")
    i = next(k for k, l in enumerate(lines) if f"; rsb {name} begin" in l)
    j = next(k for k, l in enumerate(lines) if k > i and (f"; rsb {name} end" in l or l.startswith(".Lfunc_end")))
    ins = [m.group(1) for l in lines[i:j] for m in [re.match(r"^\s+([a-z_0-9]+)(?: |$)", l)] if m]
    return {"instructions": len(ins), "s_load": sum(x.startswith("s_load") for x in ins), "branches": sum(x.startswith(("s_cbranch", "s_branch")) for x in ins),
            "loops": sum("Loop Header" in l for l in lines[i:j])}


@pytest.fixture(scope="module")
def resident(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lean_seam_host")
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    return _assembly(64, defs, str(tmp / "lean.s")), _assembly(64, [*defs, SWITCH], str(tmp / "twin.s"))


def test_both_variants_compile_without_scratch_and_the_lean_path_is_the_shorter_one(resident):
    lean, twin = resident
    assert lean != twin and "rsb lean seam begin" in lean and "rsb lean seam" not in twin and "rsb generic seam" not in twin
    assert _scratch(lean) == 0 and _scratch(twin) == 0
    path, generic = _region(lean, "lean seam"), _region(lean, "generic seam")
    print("lean path:", path, "generic seam:", generic)
    assert generic["s_load"] > 0 and generic["branches"] > 0 and generic["loops"] > 0, generic      # (the counters see something)
    for k in ("s_load", "branches", "loops", "instructions"):
        assert path[k] < generic[k], (k, path, generic)


@pytest.mark.parametrize("cl", [0, 16])
def test_the_switch_changes_nothing_in_the_plain_and_pipelined_classes(tmp_path, cl):
    defs = _manifest_defs(f"16 8 {cl} 4", "TERRAIN=0")
    assert _assembly(cl, defs, str(tmp_path / "a.s")) == _assembly(cl, [*defs, SWITCH], str(tmp_path / "b.s"))
