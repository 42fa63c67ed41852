"""Static shape of the flat contact form (raisimlib_amd/csrc/step_spec.h RSB_FLAT_CONTACT; step_phase_columns.inc, step_phase_solver.inc), read off the compiler's
assembly (hipcc -S, no GPU) of the benchmark's specialised resident class <16, 8, 64, 4> on flat ground and on config 3's height map, with and without
-DRSB_X_NO_FLAT_CONTACT: both compile without scratch and with the LDS they had; between the comment lines the kernel leaves around the contact columns and around
the impulse scatter, the flat form has fewer branches, fewer exec-mask regions and fewer waits than the twin, and the kernel as a whole no more LDS instructions
(a dead level's store goes to the sink through the SAME instruction with a selected address, so the sink costs none; the twin's out-of-line blocks may lie
outside the comment lines, hence the whole kernel for that count).  The switch changes nothing in a non-specialised build, nor in the humanoid's class.
The counts themselves are in DESIGN.md; only the inequalities are asserted."""
import os
import re
import subprocess

import pytest

from raisimlib_amd import build as _b
from test_kernel_budget import _manifest_defs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "-DRSB_X_NO_FLAT_CONTACT"


def _assembly(lpe, kmax, cl, ml, defs, out):
    cmd = ["/opt/rocm/bin/hipcc", *[f for f in _b.FLAGS if f not in ("-fPIC", "-Wall", "-Wno-unused-function")], "-I", os.path.join(ROOT, "include"), "-I", _b.CSRC,
           f"-DRSB_I_LPE={lpe}", f"-DRSB_I_KMAX={kmax}", f"-DRSB_I_CL={cl}", f"-DRSB_I_ML={ml}", "-DRSB_I_PROF=0", *defs, "--cuda-device-only", "-S", "-o", out,
           os.path.join(_b.CSRC, "step_instance.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = open(out).read()
    os.remove(out)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "", txt)      # (the compilation unit's id differs from run to run)


def _meta(txt, key):
    return int(re.search(rf"^\s+\.{key}:\s+(\d+)", txt, re.M).group(1))


def _mnemonics(lines):
    return [m.group(1) for l in lines for m in [re.match(r"^\s+([a-z_0-9]+)(?: |$)", l)] if m]


def _count(ins):
    return {"instructions": len(ins), "branches": sum(x.startswith(("s_cbranch", "s_branch")) for x in ins), "saveexec": sum("saveexec" in x for x in ins),
            "waitcnt": sum(x == "s_waitcnt" for x in ins), "ds": sum(x.startswith("ds_") for x in ins)}


def _region(txt, name):
    lines = txt.split("\n")
    i = next(k for k, l in enumerate(lines) if f"; rsb {name} begin" in l)
    j = next(k for k, l in enumerate(lines) if k > i and f"; rsb {name} end" in l)
    return _count(_mnemonics(lines[i:j]))


@pytest.fixture(scope="module", params=["TERRAIN=0", "TERRAIN=1"])
def resident(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flat_contact_host")
    defs = _manifest_defs("16 8 64 4", request.param)
    return _assembly(16, 8, 64, 4, defs, str(tmp / "flat.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp / "twin.s"))


def test_both_variants_compile_without_scratch_and_the_flat_form_has_fewer_regions_branches_and_waits(resident):
    flat, twin = resident
    assert flat != twin
    for txt in (flat, twin):
        assert all(f"; rsb {n} {e}" in txt for n in ("columns", "scatter") for e in ("begin", "end"))
        assert _meta(txt, "private_segment_fixed_size") == 0
    assert _meta(flat, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
    assert _meta(flat, "vgpr_count") <= 512 and _meta(flat, "vgpr_spill_count") == 0
    for name in ("columns", "scatter"):
        f, t = _region(flat, name), _region(twin, name)
        print(name, "flat:", f, "twin:", t)
        assert t["branches"] > 0 and t["saveexec"] > 0 and t["waitcnt"] > 0, t      # (the counters see something)
        for k in ("branches", "saveexec", "waitcnt"):
            assert f[k] < t[k], (name, k, f, t)
    f, t = _count(_mnemonics(flat.split("\n"))), _count(_mnemonics(twin.split("\n")))
    print("kernel", "flat:", f, "twin:", t)
    assert f["ds"] <= t["ds"], (f, t)


def test_each_part_switch_compiles_and_puts_back_its_own_part(tmp_path):
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    flat, twin = _assembly(16, 8, 64, 4, defs, str(tmp_path / "a.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp_path / "b.s"))
    for sw, back, kept in (("-DRSB_X_NO_FLAT_COLUMNS", "columns", "scatter"), ("-DRSB_X_NO_FLAT_SCATTER", "scatter", "columns")):
        part = _assembly(16, 8, 64, 4, [*defs, sw], str(tmp_path / "c.s"))
        assert _meta(part, "private_segment_fixed_size") == 0
        p = {n: _region(part, n) for n in (back, kept)}
        for k in ("branches", "saveexec"):
            assert p[back][k] == _region(twin, back)[k] and p[kept][k] == _region(flat, kept)[k], (sw, k, p)


@pytest.mark.parametrize("cl", [16])
def test_the_specialised_pipelined_class_takes_the_form_within_its_register_budget(tmp_path, cl):
    for must in ("TERRAIN=0", "TERRAIN=1"):
        txt = _assembly(16, 8, cl, 4, _manifest_defs(f"16 8 {cl} 4", must), str(tmp_path / "p.s"))
        assert "; rsb columns begin" in txt and _meta(txt, "vgpr_count") <= 416 and _meta(txt, "private_segment_fixed_size") == 0


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 16, 4), (16, 8, 64, 4), (32, 16, 64, 12)])
def test_the_switch_changes_nothing_ahead_of_time_nor_in_the_humanoids_class(tmp_path, inst):
    a, b = _assembly(*inst, [], str(tmp_path / "a.s")), _assembly(*inst, [SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb columns" not in a and "; rsb scatter" not in a


def test_the_switch_changes_nothing_in_the_humanoids_specialised_class(tmp_path):
    defs = _manifest_defs("32 16 64 12")
    a, b = _assembly(32, 16, 64, 12, defs, str(tmp_path / "a.s")), _assembly(32, 16, 64, 12, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb columns" not in a
