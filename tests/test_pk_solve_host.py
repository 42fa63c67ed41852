"""Static shape of the packed fp32 form of the contact solve (raisimlib_amd/csrc/step_spec.h RSB_PK_SOLVE; step_slip_pk.h, step_phase_solver.inc), read off the
compiler's assembly (hipcc -S, no GPU) of the benchmark's specialised resident class <16, 8, 64, 4> on flat ground and on config 3's height map, with and without
-DRSB_X_NO_PK_SOLVE: both compile without scratch and with the same LDS; between the comment lines the kernel leaves around the sweep loop the packed form has more
v_pk_* and fewer VALU instructions than its twin, and outside them nothing differs; the pipelined class keeps its register budget; the switch changes nothing in
the ahead-of-time classes, in the humanoid's class or in the Coulomb class.  The counts themselves are in DESIGN.md; only the inequalities are asserted.
(The form has one part - the Delassus accumulation and the quad basin scan were built and taken out again, DESIGN.md section 9 - so there is no part switch.)"""
import pytest

from test_flat_contact_host import _assembly, _meta, _mnemonics
from test_kernel_budget import _manifest_defs

SWITCH = "-DRSB_X_NO_PK_SOLVE"
REGIONS = ("sweep",)


def _region(txt, name):
    lines = txt.split("\n")
    i = next(k for k, l in enumerate(lines) if f"; rsb {name} begin" in l)
    j = next(k for k, l in enumerate(lines) if k > i and f"; rsb {name} end" in l)
    ins = _mnemonics(lines[i:j])
    return {"valu": sum(x.startswith("v_") for x in ins), "pk": sum(x.startswith("v_pk_") for x in ins)}


@pytest.fixture(scope="module", params=["TERRAIN=0", "TERRAIN=1"])
def resident(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pk_solve_host")
    defs = _manifest_defs("16 8 64 4", request.param)
    return _assembly(16, 8, 64, 4, defs, str(tmp / "pk.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp / "twin.s"))


def test_both_variants_compile_without_scratch_and_the_packed_form_issues_fewer_valu_instructions(resident):
    pk, twin = resident
    assert pk != twin
    for txt in (pk, twin):
        assert all(f"; rsb {n} {e}" in txt for n in REGIONS for e in ("begin", "end"))
        assert _meta(txt, "private_segment_fixed_size") == 0 and _meta(txt, "vgpr_spill_count") == 0
    assert _meta(pk, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
    assert _meta(pk, "vgpr_count") <= 512
    for name in REGIONS:
        p, t = _region(pk, name), _region(twin, name)
        print(name, "packed:", p, "twin:", t)
        assert p["pk"] > t["pk"] and p["valu"] < t["valu"], (name, p, t)


def test_the_switch_moves_no_packed_instruction_outside_the_sweep_loop(resident):
    pk, twin = resident
    whole = [sum(x.startswith("v_pk_") for x in _mnemonics(t.split("\n"))) for t in (pk, twin)]
    inside = [_region(t, "sweep")["pk"] for t in (pk, twin)]
    assert whole[0] - inside[0] == whole[1] - inside[1], (whole, inside)


@pytest.mark.parametrize("cl", [16])
def test_the_specialised_pipelined_class_takes_the_form_within_its_register_budget(tmp_path, cl):
    for must in ("TERRAIN=0", "TERRAIN=1"):
        txt = _assembly(16, 8, cl, 4, _manifest_defs(f"16 8 {cl} 4", must), str(tmp_path / "p.s"))
        assert "; rsb sweep begin" in txt and _region(txt, "sweep")["pk"] > 15
        assert _meta(txt, "vgpr_count") <= 416 and _meta(txt, "private_segment_fixed_size") == 0


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 16, 4), (16, 8, 64, 4), (32, 16, 64, 12), (16, 8, 32, 4)])
def test_the_switch_changes_nothing_ahead_of_time(tmp_path, inst):
    a, b = _assembly(*inst, [], str(tmp_path / "a.s")), _assembly(*inst, [SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb sweep" not in a


def test_the_switch_changes_nothing_in_the_humanoids_specialised_class(tmp_path):
    defs = _manifest_defs("32 16 64 12")
    a, b = _assembly(32, 16, 64, 12, defs, str(tmp_path / "a.s")), _assembly(32, 16, 64, 12, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb sweep" not in a


def test_the_switch_changes_nothing_in_the_specialised_coulomb_class(tmp_path):
    defs = _manifest_defs("16 8 0 4", "TERRAIN=0")
    a, b = _assembly(16, 8, 32, 4, defs, str(tmp_path / "a.s")), _assembly(16, 8, 32, 4, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb sweep" not in a
