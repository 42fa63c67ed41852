"""Which models the step kernel runs the up pass's quad form on (four lanes per body: raisimlib_amd/csrc/step_phase_tree_up.inc, step_spec.h RSB_UP_QUADS), and
which body every quad of a 16-lane env works on at every tree level - host only (rsb_model_up_quads)."""
from raisimlib_amd import Model


def _chains_urdf(n_chains, length):
    parts = ['<robot name="chains"><link name="base"><inertial><mass value="8"/><inertia ixx="0.2" ixy="0" ixz="0" iyy="0.3" iyz="0" izz="0.4"/></inertial></link>']
    for c in range(n_chains):
        for k in range(length):
            parts.append(f'<link name="c{c}_{k}"><inertial><mass value="1"/><inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial>'
                         f'<collision><geometry><sphere radius="0.04"/></geometry></collision></link>')
            parent = "base" if k == 0 else f"c{c}_{k - 1}"
            parts.append(f'<joint name="j{c}_{k}" type="revolute"><origin xyz="{0.1 * c:.2f} 0.05 -0.15"/><parent link="{parent}"/><child link="c{c}_{k}"/>'
                         f'<axis xyz="0 1 0"/><limit effort="0" velocity="50" lower="-6" upper="6"/></joint>')
    parts.append("</robot>")
    return "\n".join(parts)


def test_the_quadruped_has_three_levels_of_four_bodies_every_body_once(anymal):
    table = anymal.up_quads()
    assert len(table) == 3 and all(len(level) == 4 for level in table), table
    assert sorted(b for level in table for b in level) == list(range(1, anymal.nb)), table
    blob = anymal.blob
    for lv, level in enumerate(table, start=1):
        for g, body in enumerate(level):
            assert blob.level[body] == lv, (lv, g, body)
            assert blob.parent[body] == (0 if lv == 1 else table[lv - 2][g]), (lv, g, body)      # quad g stays on one leg: its body's child is its body of the next level


def test_other_trees_keep_the_lane_per_body_loop(built_lib, atlas):
    assert atlas.up_quads() == []
    assert Model(urdf_string=_chains_urdf(5, 2)).up_quads() == []      # five bodies on a level
    assert Model(urdf_string=_chains_urdf(3, 3)).up_quads() == []      # three
    assert len(Model(urdf_string=_chains_urdf(4, 2)).up_quads()) == 2  # four chains of any equal length qualify
