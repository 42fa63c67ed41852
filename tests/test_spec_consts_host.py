"""The contact solve's scalar settings as compile-time constants of the specialised code objects (raisimlib_amd/csrc/step_spec.h: the key fields MU ... MAX_ITER; no GPU).
The benchmark's specialised resident class <16, 8, 64, 4> is compiled to assembly (hipcc -S) by default and as its twin -DRSB_X_NO_SPEC_CONSTS, which reads the
fields from the kernel arguments as before:
  - the default holds strictly fewer scalar loads, and the difference is at least the number of loads of the folded fields' kernel-argument offsets in the twin;
  - it takes no more registers, spills no more SGPRs and uses no scratch;
  - it holds as many fused multiply-adds, reciprocal, reciprocal-square-root, square-root, division and frexp instructions as the twin: a division the compiler re-formed
    around a literal (exact where it was approximate, or folded on the host), or a product that is fused into - or left out of - another operation because a literal 0
    removed its neighbour, would move a bit, and shows here as another count (step_spec.h);
and changing one new field's value in a manifest line changes the code object's file name."""
import re

import pytest

from raisimlib_amd import _capi
from test_down_quads_host import _assembly
from test_kernel_budget import _manifest_defs
from test_spec_host import _lines, _name

C = _capi.C
TWIN = "-DRSB_X_NO_SPEC_CONSTS"
NEW_FIELDS = ["MU", "ERP", "ALPHA_INIT", "ALPHA_MIN", "ALPHA_DECAY", "THRESHOLD", "STALL_FACTOR", "MAX_ITER"]
# the StepArgs members behind the new fields: name -> dwords
MEMBERS = {"mu": 1, "erp": 1, "alpha_init": 1, "alpha_min": 1, "alpha_decay": 1, "threshold": 1, "max_iter": 1,
           "stall_factor": 1}


def _offsets():
    """kernel-argument byte offsets of MEMBERS, from the library's own StepArgs (the compiler lays the by-value argument out at offset 0 of the segment)"""
    import os
    import subprocess
    import tempfile
    from raisimlib_amd import build as _b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = "#include <cstddef>\n#include <cstdio>\n#include <hip/hip_runtime.h>\n#include \"rsb.h\"\n#include \"step_types.h\"\nint main() {\n" + \
          "".join(f'  std::printf("{m} %zu\\n", offsetof(rsbk::StepArgs, {m}));\n' for m in MEMBERS) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "off.cpp")
        open(p, "w").write(src)
        exe = os.path.join(d, "off")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(root, "include"), "-I", _b.CSRC, p, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}


def _scalar_loads(txt):
    """[(first byte, dwords)] of every scalar load of the kernel"""
    out = []
    for m in re.finditer(r"^\s+s_load_dword(x(\d+))?\s+s\[?[\d:]+\]?,\s*s\[[\d:]+\],\s*(0x[0-9a-f]+|\d+)", txt, re.M):
        out.append((int(m.group(3), 0), int(m.group(2) or 1)))
    return out


def _stats(txt):
    meta = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", txt, re.M).group(1)) for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
    for name, pat in (("fma", r"v_(pk_)?fma(c|mk|ak)?_f32"), ("rcp", r"v_rcp_f32"), ("rsq", r"v_rsq_f32"), ("sqrt", r"v_sqrt_f32"), ("div", r"v_div_(scale|fmas|fixup)_f32"), ("frexp", r"v_frexp_mant_f32")):
        meta[name] = len(re.findall(rf"^\s+{pat}", txt, re.M))
    return meta


def _body(txt):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "", txt)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("spec_consts")
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    return _assembly(defs, str(d / "default.s")), _assembly([*defs, TWIN], str(d / "twin.s"))


def test_the_folded_fields_are_no_longer_loaded_and_nothing_else_got_worse(pair):
    default, twin = pair
    off = _offsets()
    spans = [(off[m], off[m] + 4 * n) for m, n in MEMBERS.items()]

    def folded(loads):
        # (a load that STARTS at a folded member: there is no three-dword scalar load, so gx gy gz are fetched as four dwords and drag the neighbouring mu along)
        return [l for l in loads if any(lo <= l[0] < hi for lo, hi in spans)]
    ld, lt = _scalar_loads(default), _scalar_loads(twin)
    sd, st = _stats(default), _stats(twin)
    print("scalar loads: default", len(ld), "twin", len(lt), "| loads of the folded fields: default", folded(ld), "twin", folded(lt))
    print("default", sd)
    print("twin   ", st)
    assert len(lt) > 20 and folded(lt)                            # (the pattern reads this compiler's assembly)
    assert len(ld) < len(lt)
    assert len(lt) - len(ld) >= len(folded(lt))
    assert not folded(ld)
    assert sd["vgpr_count"] <= st["vgpr_count"] and sd["sgpr_count"] <= st["sgpr_count"] and sd["sgpr_spill_count"] <= st["sgpr_spill_count"]
    assert sd["private_segment_fixed_size"] == 0 and sd["vgpr_spill_count"] == 0
    for k in ("fma", "rcp", "rsq", "sqrt", "div", "frexp"):
        assert sd[k] == st[k], (k, sd[k], st[k])


def test_the_switch_compiles_to_another_kernel_without_scratch(pair):
    default, twin = pair
    assert _body(default) != _body(twin)
    assert _stats(twin)["private_segment_fixed_size"] == 0


@pytest.mark.parametrize("field", NEW_FIELDS)
def test_a_new_field_value_names_another_code_object(built_lib, field):
    line = next(l for l in _lines() if l.startswith("16 8 64 4 |") and "TERRAIN=0" in l)
    m = re.search(rf"-DRSB_SPEC_{field}=(-?\d+)( |$)", line)
    assert m, (field, line)
    other = line[:m.start(1)] + str(int(m.group(1)) + 1) + line[m.end(1):]
    rc, a = _name(line)
    rc2, b = _name(other)
    assert rc == rc2 == 0 and a != b, (field, a, b)
    if field != "MAX_ITER":
        # a float's key is its bit pattern: -0 is not +0 (a signed decimal, INT_MIN included, is a form the line parser takes)
        neg = line[:m.start(1)] + str(int(m.group(1)) - 2 ** 31 if int(m.group(1)) >= 0 else int(m.group(1)) + 2 ** 31) + line[m.end(1):]
        rc3, c = _name(neg)
        assert rc3 == 0 and c not in (a, b), (field, neg)
