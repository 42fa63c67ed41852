"""Static shape of the sweep control (raisimlib_amd/csrc/step_spec.h RSB_SWEEP_CONTROL; step_phase_solver.inc, step_slip_pk.h), read off the compiler's assembly
(hipcc -S, no GPU) of the benchmark's specialised resident class <16, 8, 64, 4> on flat ground and on config 3's height map, and of the pipelined class cl = 16:
no scratch, no spill, the LDS of the twin (-DRSB_X_NO_SWEEP_CONTROL), the register budgets.

The fast continuation of the direction refresh (RSB_SWEEP_RARE) lies between the comment lines `; rsb refresh fast begin/end`: no branch, no exec-mask write and no
s_waitcnt between them.

The loop control (RSB_SWEEP_LOOP) is followed as control flow, not as text (the compiler places the blocks of a loop as it likes): from the comment line
`; rsb sweep control begin`, which the kernel leaves behind the exchange, along BOTH sides of every conditional branch, until the walk meets the comment line
`; rsb sweep control end` at the head of a pass's rule or leaves the sweep loop (`; rsb sweep end`).  Every branch instruction on the way counts, s_branch included.
A path to the next pass's rule may hold two ("another pass of this sweep", "another sweep"); the one path out of the loop holds those two and may hold a jump to
the code behind the loop.  No branch on the way may test a vcc that a v_cmp wrote: the tests are scalar compares of scalar counters and of the mask of the lanes
not yet done.  (That mask is a function of the epilogue's vector compares - convergence is decided per lane - and the compiler forms a ballot of it with one
v_cmp_ne into a register pair; what the condition rules out is the VALU compare + s_cbranch_vcc pair of profiles/r02_ubench_lone_wave_latency.txt.)

Each part switch puts back its own part only; the switch changes nothing in ahead-of-time builds, in the humanoid's specialised class or in the Coulomb class.
The counts themselves are in DESIGN.md; only these conditions are asserted."""
import re

import pytest

from test_flat_contact_host import _assembly, _meta, _mnemonics
from test_kernel_budget import _manifest_defs

SWITCH = "-DRSB_X_NO_SWEEP_CONTROL"
NO_RARE, NO_LOOP = "-DRSB_X_NO_SWEEP_CONTROL_RARE", "-DRSB_X_NO_SWEEP_CONTROL_LOOP"
FAST = ("; rsb refresh fast begin", "; rsb refresh fast end")
CTL = ("; rsb sweep control begin", "; rsb sweep control end")


def _fast_region(txt):
    lines = txt.split("\n")
    i = next(k for k, l in enumerate(lines) if FAST[0] in l)
    j = next(k for k, l in enumerate(lines) if k > i and FAST[1] in l)
    return lines[i + 1:j]


def _writes_exec(line):
    m = re.match(r"^\s+([a-z_0-9]+)\s+([^,\s]+)", line)
    return bool(m) and ("saveexec" in m.group(1) or m.group(1).startswith("v_cmpx") or m.group(2).startswith("exec"))


def _control_paths(txt):
    """every path from the loop-control begin line to the head of a pass or out of the sweep loop: (where it ended, branches on it, vcc branches fed by a v_cmp)"""
    lines = txt.split("\n")
    label = {m.group(1): k for k, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    start = [k for k, l in enumerate(lines) if CTL[0] in l]
    assert len(start) == 1, start
    out, todo, seen = [], [(start[0] + 1, 0, None, 0)], set()
    while todo:
        k, nbr, vcc_writer, fed = todo.pop()
        while True:
            assert k < len(lines) and nbr <= 8, "the walk left the kernel"
            l = lines[k]
            if CTL[1] in l or "; rsb sweep end" in l:
                out.append(("pass" if CTL[1] in l else "exit", nbr, fed))
                break
            m = re.match(r"^\s+([a-z_0-9]+)(?:\s+(.*))?$", l)
            if not m or l.lstrip().startswith(";"):
                k += 1
                continue
            op, args = m.group(1), (m.group(2) or "")
            if op == "s_branch":
                nbr += 1
                k = label[args.strip()]
                continue
            if op.startswith("s_cbranch"):
                nbr += 1
                if "vcc" in op and vcc_writer is not None and vcc_writer.startswith("v_cmp"):
                    fed += 1
                key = (k, nbr, fed)
                if key not in seen:      # (the other side of the branch)
                    seen.add(key)
                    todo.append((label[args.strip()], nbr, vcc_writer, fed))
                k += 1
                continue
            assert op != "s_endpgm"
            if re.match(r"vcc(_lo|_hi)?\b", args):
                vcc_writer = op
            k += 1
    return out


@pytest.fixture(scope="module", params=["TERRAIN=0", "TERRAIN=1"])
def resident(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sweep_control_host")
    defs = _manifest_defs("16 8 64 4", request.param)
    return {sw: _assembly(16, 8, 64, 4, [*defs, *([sw] if sw else [])], str(tmp / "a.s")) for sw in ("", SWITCH, NO_RARE, NO_LOOP)}


def _shape(txt, budget):
    assert _meta(txt, "private_segment_fixed_size") == 0 and _meta(txt, "vgpr_spill_count") == 0 and _meta(txt, "vgpr_count") <= budget
    fast = _fast_region(txt)
    ins = _mnemonics(fast)
    print("fast continuation:", ins)
    assert ins and all(x.startswith("v_cndmask") or x == "s_nop" for x in ins), ins      # (the selects that take the step, and nothing else)
    assert not any(x.startswith(("s_cbranch", "s_branch")) or x == "s_waitcnt" for x in ins) and not any(_writes_exec(l) for l in fast)
    paths = _control_paths(txt)
    print("loop control paths (end, branches, vcc branches on a v_cmp):", paths)
    assert {p[0] for p in paths} == {"pass", "exit"}
    assert all(p[1] <= 2 for p in paths if p[0] == "pass"), paths
    assert all(p[1] <= 3 for p in paths if p[0] == "exit"), paths
    assert all(p[2] == 0 for p in paths), paths


def test_the_form_compiles_without_scratch_and_its_fast_continuation_and_loop_control_have_their_shape(resident):
    form, twin = resident[""], resident[SWITCH]
    assert form != twin
    assert _meta(form, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
    assert _meta(twin, "private_segment_fixed_size") == 0 and _meta(twin, "vgpr_spill_count") == 0
    assert not any(m in twin for m in FAST + CTL)
    _shape(form, 512)


def test_each_part_switch_puts_back_its_own_part_only(resident):
    no_rare, no_loop = resident[NO_RARE], resident[NO_LOOP]
    for txt in (no_rare, no_loop):
        assert _meta(txt, "private_segment_fixed_size") == 0 and _meta(txt, "vgpr_spill_count") == 0 and _meta(txt, "vgpr_count") <= 512
        assert _meta(txt, "group_segment_fixed_size") == _meta(resident[""], "group_segment_fixed_size")
    assert not any(m in no_rare for m in FAST) and all(m in no_rare for m in CTL)
    assert not any(m in no_loop for m in CTL) and all(m in no_loop for m in FAST)
    paths = _control_paths(no_rare)
    assert all(p[1] <= 2 and p[2] == 0 for p in paths if p[0] == "pass"), paths
    ins = _mnemonics(_fast_region(no_loop))
    assert ins and all(x.startswith("v_cndmask") or x == "s_nop" for x in ins), ins
    assert len({resident[k] for k in resident}) == 4


@pytest.mark.parametrize("cl", [16])
def test_the_specialised_pipelined_class_takes_the_form_within_its_register_budget(tmp_path, cl):
    for must in ("TERRAIN=0", "TERRAIN=1"):
        defs = _manifest_defs(f"16 8 {cl} 4", must)
        txt, twin = _assembly(16, 8, cl, 4, defs, str(tmp_path / "p.s")), _assembly(16, 8, cl, 4, [*defs, SWITCH], str(tmp_path / "q.s"))
        assert _meta(txt, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
        _shape(txt, 416)


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 16, 4), (16, 8, 64, 4), (32, 16, 64, 12), (16, 8, 32, 4)])
def test_the_switches_change_nothing_ahead_of_time(tmp_path, inst):
    a = _assembly(*inst, [], str(tmp_path / "a.s"))
    assert not any(m in a for m in FAST + CTL)
    for sw in (SWITCH, NO_RARE, NO_LOOP):
        assert a == _assembly(*inst, [sw], str(tmp_path / "b.s")), sw


def test_the_switch_changes_nothing_in_the_humanoids_specialised_class(tmp_path):
    defs = _manifest_defs("32 16 64 12")
    a, b = _assembly(32, 16, 64, 12, defs, str(tmp_path / "a.s")), _assembly(32, 16, 64, 12, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and not any(m in a for m in FAST + CTL)


def test_the_switch_changes_nothing_in_the_specialised_coulomb_class(tmp_path):
    defs = _manifest_defs("16 8 0 4", "TERRAIN=0")
    a, b = _assembly(16, 8, 32, 4, defs, str(tmp_path / "a.s")), _assembly(16, 8, 32, 4, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and not any(m in a for m in FAST + CTL)
