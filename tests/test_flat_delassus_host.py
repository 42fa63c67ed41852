"""Static shape of the flat Delassus form (raisimlib_amd/csrc/step_spec.h RSB_FLAT_DELASSUS; step_phase_delassus.inc), read off the compiler's assembly (hipcc -S, no
GPU) of the benchmark's specialised resident class <16, 8, 64, 4> and pipelined class <16, 8, 16, 4> on flat ground and on config 3's height map, with and without
-DRSB_X_NO_FLAT_DELASSUS: both compile without scratch and with the LDS they had; between the comment lines the kernel leaves around the pair loop the flat form has
strictly fewer waits and strictly fewer exec-mask regions than the twin, and the kernel as a whole no more LDS instructions.  The switch puts back its own part only
(the set-up's and the columns' regions are what they are beside it, and their part switches leave the pair loop flat; the flat set-up's whole switch takes it along).  It changes nothing in a non-specialised build, in
the fixed-base class, nor in the humanoid's class.  The counts themselves are in DESIGN.md; only the inequalities are asserted.

The closed form the flat form takes a body's limb and level from (its host-side twin: rsb_world.hip, delassus_closed_form_ok) is compared in pure Python with the
model's parent / level tables for every body pair of anymal_c_like.urdf, and must report itself unusable on a numbering that is not four consecutive chains."""
import pytest

from test_flat_contact_host import _assembly, _count, _meta, _mnemonics, _region
from test_kernel_budget import _manifest_defs

SWITCH = "-DRSB_X_NO_FLAT_DELASSUS"
INSTANCES = [(16, 8, 64, 4), (16, 8, 16, 4)]


@pytest.fixture(scope="module", params=[(inst, terr) for inst in INSTANCES for terr in ("TERRAIN=0", "TERRAIN=1")], ids=lambda p: f"{p[0][2]}-{p[1]}")
def pair(request, tmp_path_factory):
    inst, terr = request.param
    tmp = tmp_path_factory.mktemp("flat_delassus_host")
    defs = _manifest_defs(" ".join(map(str, inst)), terr)
    return inst, _assembly(*inst, defs, str(tmp / "flat.s")), _assembly(*inst, [*defs, SWITCH], str(tmp / "twin.s"))


def test_both_variants_compile_without_scratch_and_the_flat_form_has_fewer_waits_and_regions(pair):
    inst, flat, twin = pair
    assert flat != twin
    for txt in (flat, twin):
        assert all(f"; rsb delassus {e}" in txt for e in ("begin", "end"))
        assert _meta(txt, "private_segment_fixed_size") == 0 and _meta(txt, "vgpr_spill_count") == 0
    assert _meta(flat, "group_segment_fixed_size") == _meta(twin, "group_segment_fixed_size")
    assert _meta(flat, "vgpr_count") <= (416 if inst[2] & 16 else 512), _meta(flat, "vgpr_count")      # (the pipelined classes leave 96 registers to a stage wave)
    f, t = _region(flat, "delassus"), _region(twin, "delassus")
    print(inst, "delassus", "flat:", f, "twin:", t, "vgprs", _meta(flat, "vgpr_count"), _meta(twin, "vgpr_count"))
    assert t["saveexec"] > 0 and t["waitcnt"] > 0, t      # (the counters see something)
    for k in ("waitcnt", "saveexec"):
        assert f[k] < t[k], (k, f, t)
    f, t = _count(_mnemonics(flat.split("\n"))), _count(_mnemonics(twin.split("\n")))
    print(inst, "kernel", "flat:", f, "twin:", t)
    assert f["ds"] <= t["ds"], (f, t)


def test_each_switch_puts_back_its_own_part_only(tmp_path):
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    flat, twin = _assembly(16, 8, 64, 4, defs, str(tmp_path / "a.s")), _assembly(16, 8, 64, 4, [*defs, SWITCH], str(tmp_path / "b.s"))
    # the Delassus switch leaves the columns' and the set-up's regions with the advantage they have over THEIR twins ...
    for sw, name, stays_flat in (("-DRSB_X_NO_FLAT_CONTACT", "columns", True), ("-DRSB_X_NO_FLAT_SETUP_HEAD", "setup", True), ("-DRSB_X_NO_FLAT_SETUP_END", "solver end", True),
                                 ("-DRSB_X_NO_FLAT_SETUP", "setup", False)):
        other = _assembly(16, 8, 64, 4, [*defs, sw], str(tmp_path / "c.s"))
        assert _meta(other, "private_segment_fixed_size") == 0 and _meta(other, "vgpr_spill_count") == 0
        for k in ("saveexec", "waitcnt"):
            assert _region(twin, name)[k] < _region(other, name)[k], (sw, k, _region(twin, name), _region(other, name))
            # ... and the part switches of the other forms leave the pair loop flat; the flat set-up's own switch takes the pair loop with it (step_spec.h)
            d = _region(other, "delassus")[k]
            assert (d < _region(twin, "delassus")[k]) if stays_flat else (d > _region(flat, "delassus")[k]), (sw, k, _region(other, "delassus"), _region(twin, "delassus"))
    # ... and puts back the pair loop's regions and waits
    for k in ("saveexec", "waitcnt"):
        assert _region(twin, "delassus")[k] > _region(flat, "delassus")[k]


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 16, 4), (16, 8, 64, 4), (16, 8, 1, 4), (32, 16, 64, 12)])
def test_the_switch_changes_nothing_ahead_of_time_nor_in_the_fixed_base_class(tmp_path, inst):
    a, b = _assembly(*inst, [], str(tmp_path / "a.s")), _assembly(*inst, [SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb delassus" not in a


def test_the_switch_changes_nothing_in_the_humanoids_specialised_class(tmp_path):
    defs = _manifest_defs("32 16 64 12")
    a, b = _assembly(32, 16, 64, 12, defs, str(tmp_path / "a.s")), _assembly(32, 16, 64, 12, [*defs, SWITCH], str(tmp_path / "b.s"))
    assert a == b and "; rsb delassus" not in a


def test_a_diagonal_pairs_transposed_store_writes_the_same_bits_to_the_same_address():
    """the flat form has no i != j test: for i == j both operands of every product are the same column, acc[3 r + c] and acc[3 c + r] are the same chain of fused
    multiply-adds on commuted products, and the transpose's block (j, i) IS block (i, j).  The chain is replayed here in exact arithmetic rounded to fp32 per step."""
    import numpy as np
    from fractions import Fraction
    rng = np.random.default_rng(5)
    w = (rng.normal(0.0, 1.0, (3, 9)) * 10.0 ** rng.integers(-3, 4, (3, 9))).astype(np.float32)
    w[:, 7:] = 0.0      # (entries past the shared prefix are selected to zero on both sides)

    def fma(a, b, c):      # exact product and sum, rounded once at the end (through fp64: the same on both sides of the comparison)
        return np.float32(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))
    acc = np.zeros(9, np.float32)
    for e in range(9):
        for r in range(3):
            for c in range(3):
                acc[3 * r + c] = fma(w[r, e], w[c, e], acc[3 * r + c])
    for lim in (False, True):      # (a joint-limit row's diagonal keeps the symmetry)
        a = acc.copy()
        if lim:
            a[0] = a[4] = 1.0
        B, Bt = a.reshape(3, 3), a.reshape(3, 3).T
        assert B.tobytes() == np.ascontiguousarray(Bt).tobytes()
    grp, blk = 12 * 8 + 4, 12      # (step_types.h: g_row_pitch(8), kGBlock)
    assert all(i * grp + blk * j == j * grp + blk * i for i in range(8) for j in range(8) if i == j)
    assert len({i * grp + blk * j for i in range(8) for j in range(8)}) == 64 and max(7 * grp + blk * 7 + 12, 0) <= 8 * grp      # (blocks are distinct and lie in front of the sink)


# ---- the closed form of a body's limb and level, against the model's tables

def table_lca(parent, level, depth, i, j):
    """what the pair loop's look-up gives: the number of leading levels 1.. at which the two bodies' ancestor rows agree (rsb_world.hip: build_dev_model's anc)"""
    def row(b):
        r = [-1] * depth
        while b >= 0:
            r[level[b]] = b
            b = parent[b]
        return r
    ri, rj = row(i), row(j)
    n = 0
    while n + 1 < depth and n + 1 <= level[i] and n + 1 <= level[j] and ri[n + 1] == rj[n + 1]:
        n += 1
    return n


def closed_form(depth, b):
    """(limb, level) of body b in a base + four consecutively numbered chains of depth - 1 bodies"""
    nl = depth - 1
    return ((b - 1) // nl, (b - 1) % nl + 1) if b > 0 else (-1, 0)


def closed_form_lca(depth, i, j):
    (gi, li), (gj, lj) = closed_form(depth, i), closed_form(depth, j)
    return min(li, lj) if i > 0 and j > 0 and gi == gj else 0


def closed_form_usable(parent, level, depth):
    nb = len(parent)
    return depth >= 2 and all(closed_form(depth, i)[1] == level[i] for i in range(nb)) and \
        all(closed_form_lca(depth, i, j) == table_lca(parent, level, depth, i, j) for i in range(nb) for j in range(nb))


def _anymal_tables():
    from raisimlib_amd import Model, rsc_path
    m = Model(urdf_path=rsc_path("anymal_c_like.urdf"))
    nb = m.nb
    return [int(m.blob.parent[i]) for i in range(nb)], [int(m.blob.level[i]) for i in range(nb)], int(m.blob.depth), m


def test_the_closed_form_is_the_tables_for_every_body_pair_of_the_quadruped():
    parent, level, depth, m = _anymal_tables()
    assert len(parent) == 13 and depth == 4 and len(m.up_quads()) == 3      # (the host reports four equal chains: the model the code objects are compiled for)
    for i in range(len(parent)):
        for j in range(len(parent)):      # (every body pair: the bodies of joint-limit rows are among them)
            assert closed_form_lca(depth, i, j) == table_lca(parent, level, depth, i, j), (i, j)
    assert {table_lca(parent, level, depth, i, j) for i in range(13) for j in range(13)} == {0, 1, 2, 3}
    assert closed_form_usable(parent, level, depth)


def test_the_closed_form_reports_itself_unusable_on_a_numbering_that_is_no_chain():
    parent, level, depth, _ = _anymal_tables()
    # the same tree with bodies 3 and 4 exchanged (the foot of limb 0 and the hip of limb 1): every body keeps its place in the tree, the numbers no longer run along the chains
    perm = list(range(len(parent)))
    perm[3], perm[4] = 4, 3
    inv = {new: old for old, new in enumerate(perm)}
    p2 = [perm[parent[inv[b]]] if parent[inv[b]] >= 0 else -1 for b in range(len(parent))]
    l2 = [level[inv[b]] for b in range(len(parent))]
    assert sorted(l2) == sorted(level) and not closed_form_usable(p2, l2, depth)
    # a tree whose chains have different lengths (limb 0 four bodies deep, limb 3 two): not this form's either
    p3, l3 = list(parent), list(level)
    p3[10], l3[10] = 3, 4
    assert not closed_form_usable(p3, l3, 5)
