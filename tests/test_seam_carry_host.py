"""The seam carry's parts (raisimlib_amd/csrc/step_spec.h: RSB_SEAM_JOINTS, RSB_SEAM_BASE, RSB_SEAM_LOADS) can each be switched off for an A/B
(-DRSB_X_NO_SEAM_JOINTS ... through $RSB_SPEC_EXTRA_DEFS).  A switch nobody compiles stops compiling unnoticed: every one of them is compiled here for the benchmark's
specialised resident class <16, 8, 64, 4> (hipcc -S, no GPU), has to give a kernel of its own without scratch, and - the barrier that closes the update pass stays in
every form - as many barriers as the default; -DRSB_X_NO_SEAM_CARRY with all three parts named besides is the same code as -DRSB_X_NO_SEAM_CARRY alone."""
import re

import pytest

from test_down_quads_host import _assembly, _counts
from test_kernel_budget import _manifest_defs

SWITCHES = ["-DRSB_X_NO_SEAM_JOINTS", "-DRSB_X_NO_SEAM_BASE", "-DRSB_X_NO_SEAM_LOADS"]


def _body(txt):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "", txt)      # (the compilation unit's id differs from run to run)


@pytest.fixture(scope="module")
def default(tmp_path_factory):
    return _assembly(_manifest_defs("16 8 64 4", "TERRAIN=0"), str(tmp_path_factory.mktemp("seam") / "default.s"))


@pytest.mark.parametrize("switch", SWITCHES)
def test_every_part_switch_compiles_to_a_kernel_of_its_own(default, tmp_path, switch):
    txt = _assembly([*_manifest_defs("16 8 64 4", "TERRAIN=0"), switch], str(tmp_path / "part.s"))
    a, b = _counts(default), _counts(txt)
    print(switch, b, "default:", a)
    assert _body(txt) != _body(default)
    assert b["scratch"] == 0 and b["barriers"] == a["barriers"], (a, b)


def test_the_main_switch_overrides_the_parts(tmp_path):
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    off = _assembly([*defs, "-DRSB_X_NO_SEAM_CARRY"], str(tmp_path / "off.s"))
    off_all = _assembly([*defs, "-DRSB_X_NO_SEAM_CARRY", *SWITCHES], str(tmp_path / "off_all.s"))
    parts_off = _assembly([*defs, *SWITCHES], str(tmp_path / "parts_off.s"))
    assert _body(off) == _body(off_all) == _body(parts_off)      # (all three parts off IS the code without the carry)
