"""Which models and worlds the step kernel tests the collision primitives of on their own bodies' lanes (raisimlib_amd/csrc/step_spec.h RSB_COL_OWN;
step_phase_collision.inc), and on which (pass, lane) - host only (rsb_model_col_own; rsb_world.hip: col_own_table).

After the down pass lane s of a 16-lane env holds the pose of body s, 1 <= s < bodies; lane 0 and the lanes >= bodies hold the base's.  Every primitive must sit
exactly once on a lane of its body; a body's primitives take ascending passes in index order; the base's fill lane 0 and the lanes >= bodies of pass 0, then of
pass 1.  Contacts are stored in primitive order: the slot of a hit is the number of hits among the lanes whose primitive - of any pass - has a lower index, and the
table's masks must give exactly that rank for EVERY subset of hits (2^20 for the quadruped, enumerated in numpy).

The assembly counts follow tests/test_flat_contact_host.py: between the comment lines `; rsb plane begin/end` the resident quadruped object has no LDS read where its
switch twin (-DRSB_X_NO_COL_OWN) reads tables and poses, and fewer branches (the centre and contact stores keep a region each per pass).  Measured from the built
objects (the resident class <16, 8, 64, 4> on the plane): form 100 instructions, 0 LDS reads, 10 LDS writes, 2 branches, 4 s_and_saveexec, 1 wait; twin 166
instructions, 12 LDS reads, 10 LDS writes, 6 branches, 6 s_and_saveexec, 4 waits.  Registers: resident 403 (twin 394) of 512, pipelined 335 (twin 324) of 416."""
import numpy as np
import pytest

from raisimlib_amd import Model
from test_flat_contact_host import _assembly, _meta, _mnemonics
from test_kernel_budget import _manifest_defs
from test_up_quads_host import _chains_urdf

SWITCH = "-DRSB_X_NO_COL_OWN"


def _popcount_table(bits):
    pc = np.zeros(1 << bits, np.uint8)
    for k in range(bits):
        pc[1 << k:1 << (k + 1)] = pc[:1 << k] + 1
    return pc


def _check_table(model, own, sample=None):
    """every primitive once, on a lane of its body, in the rule's order; the masks rank every subset of hits (or a seeded sample of them) in primitive order"""
    prim, lower, sphere = own["prim"], own["lower"], own["sphere"]
    npass, ncol, nb, blob = prim.shape[0], model.ncol, model.nb, model.blob
    assert npass == (ncol + 15) // 16
    assert sorted(int(p) for p in prim.ravel() if p >= 0) == list(range(ncol))
    base_lanes = [0, *range(nb, 16)]
    for t in range(npass):
        for s in range(16):
            p = int(prim[t, s])
            if p < 0:
                assert not lower[t, s].any() and not sphere[t, s].any()
                continue
            assert blob.col_body[p] == (s if 1 <= s < nb else 0), (t, s, p)
            assert sphere[t, s].tolist() == [np.float32(blob.col_pos[p][k]) for k in range(3)] + [np.float32(blob.col_radius[p])]
    for body in range(1, nb):      # a body's primitives: ascending passes in index order, no gap
        mine = [int(prim[t, body]) for t in range(npass)]
        have = [p for p in mine if p >= 0]
        assert have == sorted(have) and mine[:len(have)] == have and have == [i for i in range(ncol) if blob.col_body[i] == body]
    order = [int(prim[t, s]) for t in range(npass) for s in base_lanes if prim[t, s] >= 0]
    assert order == [i for i in range(ncol) if blob.col_body[i] == 0]      # the base's: lane 0 and the lanes >= bodies of pass 0, then of pass 1 ...
    # the mask rule against the rank in primitive order
    m = np.arange(1 << ncol, dtype=np.int64) if sample is None else sample
    pc16 = _popcount_table(16)
    bal = []
    for u in range(npass):
        b = np.zeros(m.shape, np.int64)
        for l in range(16):
            if prim[u, l] >= 0:
                b |= ((m >> int(prim[u, l])) & 1) << l
        bal.append(b)
    for t in range(npass):
        for s in range(16):
            p = int(prim[t, s])
            if p < 0:
                continue
            slot = sum(pc16[bal[u] & int(lower[t, s, u])].astype(np.int32) for u in range(npass))
            below = m & ((1 << p) - 1)
            rank = pc16[below & 0xffff].astype(np.int32) + pc16[(below >> 16) & 0xffff] + pc16[(below >> 32) & 0xffff] + pc16[(below >> 48) & 0xffff]
            assert np.array_equal(slot, rank), (t, s, p)


def test_the_quadruped_has_every_primitive_once_on_a_lane_of_its_body_and_the_masks_rank_every_subset_of_hits(anymal):
    own = anymal.col_own()
    assert own is not None and own["prim"].shape == (2, 16) and anymal.ncol == 20
    assert own["prim"][0].tolist() == [0, -1, 4, 6, -1, 8, 10, -1, 12, 14, -1, 16, 18, 1, 2, 3]      # base | thighs' upper ends, knees | base on the lanes that are no body
    assert own["prim"][1].tolist() == [-1, -1, 5, 7, -1, 9, 11, -1, 13, 15, -1, 17, 19, -1, -1, -1]  # thighs' lower ends, feet
    _check_table(anymal, own)      # all 2^20 subsets
    for kw in (dict(self_collision=False), dict(lanes_per_env=16)):
        again = anymal.col_own(**kw)
        assert all(np.array_equal(own[k], again[k]) for k in own)


def _tree_urdf(rng, chains, length, spheres_of):
    """_chains_urdf's four-chain skeleton with spheres_of(link) spheres on every link (link 0: the base)"""
    def cols(n):
        return "".join(f'<collision><origin xyz="{rng.uniform(-0.1, 0.1):.3f} {rng.uniform(-0.1, 0.1):.3f} {rng.uniform(-0.1, 0.1):.3f}"/><geometry><sphere radius="{rng.uniform(0.02, 0.08):.3f}"/></geometry></collision>'
                       for _ in range(n))
    txt = _chains_urdf(chains, length).replace("<collision><geometry><sphere radius=\"0.04\"/></geometry></collision>", "@")
    txt = txt.replace('name="base"><inertial>', 'name="base">' + cols(spheres_of(0)) + "<inertial>")
    k = 0
    while "@" in txt:
        k += 1
        txt = txt.replace("@", cols(spheres_of(k)), 1)
    return txt


def test_random_small_trees_satisfy_the_same_properties_whenever_they_qualify():
    rng = np.random.default_rng(20)
    seen = {True: 0, False: 0}
    for trial in range(24):
        chains, length = 4, int(rng.integers(1, 4))
        nb = 1 + chains * length
        if trial % 2:      # light: at most one primitive per body (one pass); heavy: one or two, now and then three (two passes where there are more than 16)
            counts = [int(rng.integers(0, 6))] + [int(rng.integers(0, 2)) for _ in range(nb - 1)]
        else:
            counts = [int(rng.integers(0, 10))] + [int(rng.choice([1, 1, 2, 2, 2, 2, 2, 3])) if rng.random() < 0.97 else 3 for _ in range(nb - 1)]
        if sum(counts) == 0:
            counts[1] = 1
        model = Model(urdf_string=_tree_urdf(rng, chains, length, lambda k: counts[k]))
        assert model.nb == nb and model.ncol == sum(counts)
        npass = (model.ncol + 15) // 16
        fits = max(counts[1:]) <= npass and counts[0] <= npass * (17 - nb)      # the rule: a body's primitives one per pass, the base's over its 1 + 16 - nb lanes
        own = model.col_own(kmax=8)
        # (kmax 8 with more than eight primitives is a legal world: contacts past the eighth are dropped and flagged)
        assert (own is not None) == (fits and len(model.up_quads()) > 0), (trial, counts)
        seen[own is not None] += 1
        if own is not None:
            sample = None if model.ncol <= 16 else rng.integers(0, 1 << model.ncol, 1 << 14, dtype=np.int64)
            _check_table(model, own, sample)
    assert seen[True] >= 5 and seen[False] >= 3, seen


def test_models_and_worlds_that_must_not_qualify(anymal, atlas):
    cyl = _chains_urdf(4, 3).replace('name="base"><inertial>', 'name="base"><collision><geometry><cylinder radius="0.03" length="0.1"/></geometry></collision><inertial>')
    model = Model(urdf_string=cyl)
    assert len(model.up_quads()) == 3 and any(model.blob.col_rim[i] > 0 for i in range(model.ncol)) and model.col_own() is None       # a cylinder: rim primitives
    assert Model(urdf_string=cyl.replace("cylinder", "sphere").replace(' length="0.1"', "")).col_own() is not None                  # (the same tree with a sphere there qualifies)
    three = _chains_urdf(4, 3).replace('name="c2_1"><inertial>', 'name="c2_1">' + 2 * '<collision><origin xyz="0.05 0 0"/><geometry><sphere radius="0.03"/></geometry></collision>' + "<inertial>")
    model = Model(urdf_string=three)
    assert model.nb == 13 and model.ncol == 14 and len(model.up_quads()) == 3 and model.col_own() is None      # one body with three primitives, one pass for 14
    assert atlas.col_own(kmax=16) is None and atlas.col_own(kmax=8) is None       # the humanoid: 32 lanes per env, no quad form
    assert anymal.col_own(terrain_type=1) is None                                # a height-map world
    assert anymal.col_own(kmax=16) is None and anymal.col_own(lanes_per_env=32) is None      # the 16-slot class and 32 lanes per env run no quad form
    assert Model(urdf_string=_chains_urdf(5, 2)).col_own() is None               # five bodies on a level: the lane = body loops


def _region(txt):
    lines = txt.split("\n")
    i = next(k for k, l in enumerate(lines) if "; rsb plane begin" in l)
    j = next(k for k, l in enumerate(lines) if k > i and "; rsb plane end" in l)
    ins = _mnemonics(lines[i:j])
    return {"instructions": len(ins), "branches": sum(x.startswith(("s_cbranch", "s_branch")) for x in ins), "saveexec": sum("saveexec" in x for x in ins),
            "waitcnt": sum(x == "s_waitcnt" for x in ins), "ds_read": sum(x.startswith("ds_read") for x in ins), "ds_write": sum(x.startswith("ds_write") for x in ins)}


@pytest.fixture(scope="module")
def resident(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("col_own_host")
    defs = _manifest_defs("16 8 64 4", "TERRAIN=0")
    assert "-DRSB_SPEC_COL_OWN=1" in defs
    return {sw: _assembly(16, 8, 64, 4, [*defs, *([sw] if sw else [])], str(tmp / "a.s")) for sw in ("", SWITCH)}


def test_the_plane_branch_of_the_resident_quadruped_object_reads_no_lds_and_has_fewer_branches(resident):
    form, twin = resident[""], resident[SWITCH]
    assert form != twin
    for txt in (form, twin):
        assert _meta(txt, "private_segment_fixed_size") == 0 and _meta(txt, "vgpr_spill_count") == 0 and _meta(txt, "vgpr_count") <= 512
        assert _meta(txt, "group_segment_fixed_size") == _meta(form, "group_segment_fixed_size")
    f, t = _region(form), _region(twin)
    print("plane branch  form:", f, " twin:", t, " registers:", _meta(form, "vgpr_count"), _meta(twin, "vgpr_count"))
    assert t["ds_read"] >= 12 and t["branches"] > 0 and t["saveexec"] > 0, t      # (the counters see something: two table entries of two reads and a scalar, two poses of three reads)
    assert f["ds_read"] == 0, f
    assert f["ds_read"] < t["ds_read"] and f["branches"] < t["branches"] and f["saveexec"] < t["saveexec"] and f["waitcnt"] < t["waitcnt"] and f["instructions"] < t["instructions"]
    assert f["ds_write"] <= t["ds_write"]


def test_the_specialised_pipelined_class_takes_the_form_within_its_register_budget(tmp_path):
    defs = _manifest_defs("16 8 16 4", "TERRAIN=0")
    txt = _assembly(16, 8, 16, 4, defs, str(tmp_path / "p.s"))
    assert _region(txt)["ds_read"] == 0 and _meta(txt, "vgpr_count") <= 416 and _meta(txt, "private_segment_fixed_size") == 0


def test_the_switch_changes_nothing_on_the_height_map_nor_in_the_humanoids_class(tmp_path):
    for cls, must in (("16 8 64 4", "TERRAIN=1"), ("32 16 64 12", "")):
        defs = _manifest_defs(cls, must)
        assert "-DRSB_SPEC_COL_OWN=0" in defs
        inst = [int(x) for x in cls.split()]
        assert _assembly(*inst, defs, str(tmp_path / "a.s")) == _assembly(*inst, [*defs, SWITCH], str(tmp_path / "b.s"))


@pytest.mark.parametrize("inst", [(16, 8, 0, 4), (16, 8, 64, 4)])
def test_the_switch_changes_nothing_ahead_of_time(tmp_path, inst):
    a = _assembly(*inst, [], str(tmp_path / "a.s"))
    assert "; rsb plane" not in a and a == _assembly(*inst, [SWITCH], str(tmp_path / "b.s"))
