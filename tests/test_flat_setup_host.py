"""Static shape of the flat set-up and end of the contact solve (raisimlib_amd/csrc/step_spec.h RSB_FLAT_SETUP; step_phase_solver.inc), read off the compiler's
assembly (hipcc -S, no GPU) of the benchmark's specialised resident class <16, 8, 64, 4> on flat ground and on config 3's height map, with and without
-DRSB_X_NO_FLAT_SETUP: both compile without scratch and with the LDS they had; between the comment lines the kernel leaves around the solver's set-up and around its
end, the flat form has strictly fewer waits and strictly fewer exec-mask regions than the twin, and the kernel as a whole no more LDS instructions.  Each part switch
puts back its own part and leaves the other.  The switch changes nothing in a non-specialised build, nor in the humanoid's class.
The counts themselves are in DESIGN.md; only the inequalities are asserted."""
import pytest

from test_flat_contact_host import _assembly, _count, _meta, _mnemonics, _region
from test_kernel_budget import _manifest_defs

SWITCH = "-DRSB_X_NO_FLAT_SETUP"
REGIONS = ("setup", "solver end")


@pytest.fixture(scope="module", params=["TERRAIN=0", "TERRAIN=1"])
def resident(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flat_setup_host")
    defs = _manifest_defs("16 8 64 4", request.param)
    return _assembly(16, 8, 64, 4, defs, str(tmp / "flat.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp / "twin.s"))


def test_both_variants_compile_without_scratch_and_the_flat_form_has_fewer_waits_and_regions(resident):
    flat, twin = resident
    assert flat != twin
    for txt in (flat, twin):
        assert all(f"; rsb {n} {e}" in txt for n in REGIONS for e in ("begin", "end"))
        assert _meta(txt, "private_segment_fixed_size") == 0
    assert _meta(flat, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
    assert _meta(flat, "vgpr_count") <= 512 and _meta(flat, "vgpr_spill_count") == 0
    for name in REGIONS:
        f, t = _region(flat, name), _region(twin, name)
        print(name, "flat:", f, "twin:", t)
        assert t["saveexec"] > 0 and t["waitcnt"] > 0, t      # (the counters see something)
        for k in ("waitcnt", "saveexec"):
            assert f[k] < t[k], (name, k, f, t)
    f, t = _count(_mnemonics(flat.split("\n"))), _count(_mnemonics(twin.split("\n")))
    print("kernel", "flat:", f, "twin:", t)
    assert f["ds"] <= t["ds"], (f, t)


def test_each_part_switch_compiles_and_puts_back_its_own_part(tmp_path):
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    flat, twin = _assembly(16, 8, 64, 4, defs, str(tmp_path / "a.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp_path / "b.s"))
    for sw, back, kept in (("-DRSB_X_NO_FLAT_SETUP_HEAD", "setup", "solver end"), ("-DRSB_X_NO_FLAT_SETUP_END", "solver end", "setup")):
        part = _assembly(16, 8, 64, 4, [*defs, sw], str(tmp_path / "c.s"))
        assert _meta(part, "private_segment_fixed_size") == 0 and _meta(part, "vgpr_spill_count") == 0
        assert _meta(part, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
        p = {n: _region(part, n) for n in (back, kept)}
        print(sw, p)
        # (the part put back has the twin's regions and waits again - or one more, where the compiler arranges the same source another way beside the other part -
        #  and the part that stays keeps its advantage over the twin, not its exact counts: the end without the flat set-up reads the ancestor row itself)
        for k in ("saveexec", "waitcnt"):
            assert p[back][k] >= _region(twin, back)[k] > _region(flat, back)[k] and p[kept][k] < _region(twin, kept)[k], (sw, k, p)


@pytest.mark.parametrize("cl", [16])
def test_the_specialised_pipelined_class_takes_the_form_within_its_register_budget(tmp_path, cl):
    for must in ("TERRAIN=0", "TERRAIN=1"):
        defs = _manifest_defs(f"16 8 {cl} 4", must)
        txt = _assembly(16, 8, cl, 4, defs, str(tmp_path / "p.s"))
        assert "; rsb setup begin" in txt and _meta(txt, "vgpr_count") <= 416 and _meta(txt, "private_segment_fixed_size") == 0
        assert txt != _assembly(16, 8, cl, 4, [*defs, SWITCH], str(tmp_path / "q.s"))


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 16, 4), (16, 8, 64, 4), (32, 16, 64, 12)])
def test_the_switch_changes_nothing_ahead_of_time(tmp_path, inst):
    a, b = _assembly(*inst, [], str(tmp_path / "a.s")), _assembly(*inst, [SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb setup" not in a and "; rsb solver end" not in a


def test_the_switch_changes_nothing_in_the_humanoids_specialised_class(tmp_path):
    defs = _manifest_defs("32 16 64 12")
    a, b = _assembly(32, 16, 64, 12, defs, str(tmp_path / "a.s")), _assembly(32, 16, 64, 12, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb setup" not in a
