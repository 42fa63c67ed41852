"""Static shape of the down pass's quad form (raisimlib_amd/csrc/step_phase_tree_down.inc, step_spec.h RSB_DOWN_QUADS), read off the compiler's assembly of the
benchmark's specialised resident class <16, 8, 64, 4> (hipcc -S, no GPU), against the lane = body loop compiled beside the up pass's quad form
(-DRSB_X_NO_DOWN_QUADS): no scratch, fewer barriers, and not more LDS instructions - a quad form with fewer instructions and MORE LDS operations has gained nothing
before (profiles/r07_up_quads_first_form_negative.txt).  The counts themselves are in DESIGN.md; only the inequalities are asserted."""
import os
import re
import subprocess

from raisimlib_amd import build as _b
from test_kernel_budget import _manifest_defs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assembly(defs, out):
    cmd = ["/opt/rocm/bin/hipcc", *[f for f in _b.FLAGS if f not in ("-fPIC", "-Wall", "-Wno-unused-function")], "-I", os.path.join(ROOT, "include"), "-I", _b.CSRC,
           "-DRSB_I_LPE=16", "-DRSB_I_KMAX=8", "-DRSB_I_CL=64", "-DRSB_I_ML=4", "-DRSB_I_PROF=0", *defs, "--cuda-device-only", "-S", "-o", out,
           os.path.join(_b.CSRC, "step_instance.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    txt = open(out).read()
    os.remove(out)
    return txt


def _counts(txt):
    ins = [m.group(1) for m in re.finditer(r"^\s+([a-z_0-9]+)(?: |$)", txt, re.M)]
    return {
        "scratch": int(re.search(r"^\s+\.private_segment_fixed_size:\s+(\d+)", txt, re.M).group(1)),
        # (a workgroup of one wave: the compiler drops the s_barrier instruction of a __syncthreads() and leaves the marker "; wave barrier" in its place)
        "barriers": sum(i == "s_barrier" for i in ins) + len(re.findall(r"^\s*; wave barrier\s*$", txt, re.M)),
        "ds_read": sum(i.startswith("ds_read") for i in ins),
        "ds_write": sum(i.startswith("ds_write") for i in ins),
        "instructions": len(ins),
    }


def test_quad_form_has_no_scratch_fewer_barriers_and_no_more_lds_instructions(tmp_path):
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    assert "-DRSB_SPEC_UP_QUADS=1" in defs
    quads = _counts(_assembly(defs, str(tmp_path / "quads.s")))
    lanes = _counts(_assembly([*defs, "-DRSB_X_NO_DOWN_QUADS"], str(tmp_path / "lanes.s")))
    print("quad form:", quads, "lane = body:", lanes)
    assert lanes["barriers"] > 0 and lanes["ds_read"] > 0 and lanes["ds_write"] > 0, lanes      # (the counters see something)
    assert quads != lanes      # (two different kernels were compiled)
    assert quads["scratch"] == 0, quads
    assert quads["barriers"] < lanes["barriers"], (quads, lanes)
    assert quads["ds_read"] + quads["ds_write"] <= lanes["ds_read"] + lanes["ds_write"], (quads, lanes)
