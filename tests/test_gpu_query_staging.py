"""The RSB_HOST forms of the batched queries share one staging buffer (Staged, raisimlib_amd/csrc/frames_chain.h), sized for exactly what a call passes
and grown between calls.  One ANYmal world, N = 41 (19 envs per workgroup: two full blocks and a tail of three), on per-env height maps: the host
forms are called in order of growing need, so the buffer is grown again and again, then once more in reverse order, when every call finds it larger
than it needs.  Every result must be the RSB_DEVICE form's, bit for bit; so must the feed-forward rows after a masked external wrench."""
import numpy as np
import pytest

from common import standing_states
from raisimlib_amd import _capi
from test_gpu_terrain_query import height_points, make_maps, map_world, ray_inputs

pytestmark = pytest.mark.gpu

N = 41


def test_host_forms_give_the_device_forms_bits_while_the_staging_buffer_grows(anymal):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(41)
    nb, nv = anymal.nb, anymal.nv
    maps = make_maps()
    w = map_world(anymal, N, maps, np.arange(N, dtype=np.int32) % 3)
    w.set_stream(torch.cuda.current_stream().cuda_stream)      # the device forms' tensors are filled and read on torch's stream
    w.set_state(*standing_states(N, seed=5))
    shank = anymal.body_index("LF_SHANK")
    f2 = [(0, (0.1, 0.0, 0.05)), (shank, (0.05, -0.02, -0.3))]
    f3 = f2 + [(nb - 1, (0.0, 0.04, -0.06))]
    xy = height_points(N)[0][:, :3].copy()
    ro, rd = (a.copy() for a in ray_inputs(N, 1, hmax=float(maps.max())))
    tau, udot = (rng.normal(size=(N, nv)).astype(np.float32) for _ in range(2))
    force, torque = (rng.normal(size=(N, 2, 3)).astype(np.float32) for _ in range(2))

    def t(a):      # a host input as the device form takes it
        return torch.from_numpy(a).to(dev)

    def fresh(shapes):      # device outputs, filled with a value no query gives
        return {k: torch.full(s, 7.0, dtype=torch.float32, device=dev) for k, s in shapes.items()}

    def as_dict(x, names):
        return dict(zip(names, x if isinstance(x, tuple) else (x,)))

    def ray(d):
        return as_dict(w.ray_test(t(ro), t(rd), 6.0, out=fresh({"dist": (N, 1)})["dist"]) if d else w.ray_test(ro, rd, 6.0), ("dist",))

    def height(d):
        if d:
            out = fresh({"height": (N, 3), "normal": (N, 3, 3)})
            w.terrain_height(t(xy), out=out)
            return out
        return as_dict(w.terrain_height(xy, normal=True), ("height", "normal"))

    def centroidal(d):
        return w.centroidal(com=False, ang_mom=True, out=fresh({"ang_mom": (N, 3)}) if d else None)

    def kinematics(d):
        shapes = {"pos": (N, 2, 3), "rot": (N, 2, 3, 3), "lin_vel": (N, 2, 3), "ang_vel": (N, 2, 3)}
        return w.frame_kinematics(f2, rot=True, lin_vel=True, ang_vel=True, out=fresh(shapes) if d else None)

    def forward(d):
        loads = (f2, t(force), t(torque)) if d else (f2, force, torque)
        return as_dict(w.forward_dynamics(t(tau) if d else tau, loads=loads, out=fresh({"udot": (N, nv)})["udot"] if d else None), ("udot",))

    def inverse(d):
        loads = (f2, t(force), t(torque)) if d else (f2, force, torque)
        shapes = {"tau": (N, nv), "joint_force": (N, nb, 3), "joint_torque": (N, nb, 3)}
        return w.inverse_dynamics(t(udot) if d else udot, loads=loads, joint_force=True, joint_torque=True, out=fresh(shapes) if d else None)

    def jacobians(d):
        return w.frame_jacobians(f3, rot=True, out=fresh({"lin": (N, 3, 3, nv), "rot": (N, 3, 3, nv)}) if d else None)

    def matrix(d):
        return as_dict(w.centroidal_momentum_matrix(out=fresh({"A": (N, 6, nv)})["A"] if d else None), ("A",))

    forms = [("ray_test", ray), ("terrain_height", height), ("centroidal", centroidal),
             ("frame_kinematics", kinematics), ("forward_dynamics", forward), ("inverse_dynamics", inverse), ("frame_jacobians", jacobians),
             ("centroidal_momentum_matrix", matrix)]
    want = {name: {k: v.cpu().numpy() for k, v in form(True).items()} for name, form in forms}      # the device forms, once
    assert all(np.isfinite(a).all() and not (a == 7.0).all() for d in want.values() for a in d.values())
    for order in (forms, forms[::-1]):
        for name, form in order:
            got = form(False)
            assert set(got) == set(want[name])
            for k, a in got.items():
                assert a.tobytes() == want[name][k].reshape(a.shape).tobytes(), f"{name}: {k} differs between RSB_HOST and RSB_DEVICE"

    # a masked external wrench: the feed-forward rows after the host form and after the device form
    mask = (np.arange(N) % 3 != 1).astype(np.uint8)
    wf, wt = force[:, 0].copy(), torque[:, 1].copy()
    rows = []
    for d in (False, True):
        w.set_generalized_force(tau)
        if d:
            w.add_external_wrench(f2[1], t(wf), t(wt), t(mask))
        else:
            w.add_external_wrench(f2[1], wf, wt, mask)
        rows.append(w.get_field(_capi.RSB_F_TAU_FF))
    assert rows[0].tobytes() == rows[1].tobytes()
    assert np.array_equal(rows[0][mask == 0], tau[mask == 0]) and (rows[0][mask == 1] != tau[mask == 1]).any(axis=1).all()
    w.close()
