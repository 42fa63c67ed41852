"""Host-side facts the contact solver's hand-over rests on (raisimlib_amd/csrc/step_types.h: g_row_pitch; step_phase_delassus.inc, step_phase_solver.inc):
the row-block storage of the Delassus blocks fits the region the dense rows had, and the LDS layouts of the benchmark models did not grow."""
import bench


def test_block_offsets_are_disjoint_aligned_and_inside_the_region(anymal):
    lay = anymal.delassus_layout(kmax=8, self_collision=True)
    assert lay["kcap"] == 8 and lay["block"] == 12 and lay["row_pitch"] > 0, lay
    size = 3 * lay["kcap"] * lay["dense_row"]                  # what the layout reserves for the blocks themselves (the prologue zeroes exactly this much)
    assert size <= lay["floats"], lay                         # ... inside the region between L.g and L.ginv (which other phases' scratch may widen)
    used = set()
    for i in range(lay["kcap"]):
        for k in range(lay["kcap"]):
            off = lay["row_pitch"] * i + lay["block"] * k
            assert off % 4 == 0, (i, k, off)                  # 16-byte stores and reads (the region itself starts on a 16-byte boundary: every per-env array does)
            span = set(range(off, off + lay["block"]))
            assert max(span) < size, (i, k, off)
            assert not (span & used), (i, k, off)
            used |= span
    # the eight contact lanes of an env start their 16-byte reads of one block column on eight different four-bank groups of the 64 banks
    assert len({(lay["row_pitch"] * i % 64) // 4 for i in range(8)}) == 8, lay


def test_the_large_contact_classes_keep_the_packed_triangle(atlas):
    lay = atlas.delassus_layout(kmax=16, self_collision=True)
    assert lay["kcap"] == 16 and lay["row_pitch"] == 0, lay
    assert lay["floats"] >= (16 * 17 // 2) * 12, lay


def test_lds_bytes_of_the_benchmark_models_are_what_they_were(anymal):
    """(figures of the parent commit: the row-block storage lives inside the dense rows' region, nothing else moved)"""
    assert [anymal.lds_bytes(8, True, lpe) for lpe in (0, 16, 32, 64)] == [40032, 40032, 22144, 13200]
    assert anymal.lds_bytes(8, False, 16) == 38864
    atlas = bench.Recipe(5, -1.0).model
    assert [atlas.lds_bytes(16, True, lpe) for lpe in (0, 32, 64)] == [40624, 40624, 24144]
