"""Thin Python host mirror of the batched world behind the C-ABI (include/rsb.h).

`Model` wraps rsb_model (URDF -> flat blob, host only); `BatchedWorld` wraps rsb_world: N replicas of
{raisim::World + one raisim::ArticulatedSystem + Ground/HeightMap} resident on one GPU.  Method names
follow the raisim::World / raisim::ArticulatedSystem surface [RECALL, SURVEY.md §8b] in snake_case.
Everything here is plumbing: pointers in, status codes out.  No physics and no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import (RSB_DEVICE, RSB_F_GENERALIZED_FORCE, RSB_HOST, RSB_MAX_CONTACTS, Contact, ModelBlob, check, lib)

RSC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rsc")

CONTACT_DTYPE = np.dtype([("position", "f4", 3), ("normal", "f4", 3), ("impulse", "f4", 3), ("depth", "f4"),
                          ("body", "i4"), ("collision", "i4")])
assert CONTACT_DTYPE.itemsize == C.sizeof(Contact)


def rsc_path(name):
    return os.path.join(RSC_DIR, name)


class Model:
    """Host-side articulated-system description (the role of World::addArticulatedSystem's URDF load)."""

    def __init__(self, urdf_path=None, urdf_string=None, blob=None, sample_spacing=0.0):
        """sample_spacing > 0: sampled colliders (capsule axes / box surfaces get sample primitives no further apart; rsb.h)"""
        L = lib()
        h = C.c_void_p()
        if urdf_path is not None:
            check(L.rsb_model_from_urdf_file_sampled(os.fspath(urdf_path).encode(), float(sample_spacing), C.byref(h)), "rsb_model_from_urdf_file")
        elif urdf_string is not None:
            check(L.rsb_model_from_urdf_string_sampled(urdf_string.encode(), float(sample_spacing), C.byref(h)), "rsb_model_from_urdf_string")
        elif blob is not None:
            check(L.rsb_model_from_blob(C.byref(blob), C.byref(h)), "rsb_model_from_blob")
        else:
            raise ValueError("Model needs urdf_path, urdf_string or blob")
        self.handle = h
        self.blob = ModelBlob()
        check(L.rsb_model_get_blob(self.handle, C.byref(self.blob)), "rsb_model_get_blob")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().rsb_model_destroy(h)
            except Exception:      # interpreter shutdown: the module globals lib() needs may already be gone
                pass
            self.handle = None

    nb = property(lambda self: self.blob.nb)
    nq = property(lambda self: self.blob.nq)
    nv = property(lambda self: self.blob.nv)
    ncol = property(lambda self: self.blob.ncol)
    skipped_collisions = property(lambda self: lib().rsb_model_skipped_collisions(self.handle))   # <collision> elements the loader dropped

    def body_index(self, link_name):
        return lib().rsb_model_body_index(self.handle, link_name.encode())

    def joint_index(self, joint_name):
        return lib().rsb_model_joint_index(self.handle, joint_name.encode())

    def total_mass(self):
        return lib().rsb_model_total_mass(self.handle)

    def body_names(self):
        return [self.blob.body_name[i].value.decode() for i in range(self.nb)]

    def collision_names(self):
        return [self.blob.col_name[i].value.decode() for i in range(self.ncol)]

    def lds_bytes(self, kmax=8, self_collision=True, lanes_per_env=0):
        """LDS bytes of one workgroup of the step kernel for this model (host only; rsb_model_lds_bytes)"""
        n = lib().rsb_model_lds_bytes(self.handle, int(kmax), int(bool(self_collision)), int(lanes_per_env))
        check(min(n, 0), "rsb_model_lds_bytes")
        return n

    def up_quads(self):
        """Bodies the quads of a 16-lane env work on in the up pass, one list of four per tree level below the base, or [] where the lane = body loop runs
        (host only; rsb_model_up_quads)"""
        import ctypes
        t = (ctypes.c_int * 16)()
        n = lib().rsb_model_up_quads(self.handle, t, 16)
        check(min(n, 0), "rsb_model_up_quads")
        return [[int(t[4 * lv + g]) for g in range(4)] for lv in range(n)]

    def col_own(self, kmax=8, terrain_type=0, self_collision=True, lanes_per_env=0):
        """The (pass, lane) on which the step kernel tests every collision primitive against the plane with the pose its lane already holds, or None where the
        primitive-order loop runs (host only; rsb_model_col_own): dict(prim [passes, 16] primitive or -1, sphere [passes, 16, 4] local centre and radius,
        lower [passes, 16, passes] the lanes of each pass whose primitive has a lower index, as a bit mask)"""
        import ctypes
        import numpy as np
        cap = 16 * 4
        prim, lower, sphere = (ctypes.c_int * cap)(), (ctypes.c_int * (cap * 4))(), (ctypes.c_float * (cap * 4))()
        n = lib().rsb_model_col_own(self.handle, int(kmax), int(terrain_type), int(bool(self_collision)), int(lanes_per_env), prim, lower, sphere, cap)
        check(min(n, 0), "rsb_model_col_own")
        if n == 0:
            return None
        return dict(prim=np.array(prim[:16 * n], np.int32).reshape(n, 16), sphere=np.array(sphere[:64 * n], np.float32).reshape(n, 16, 4),
                    lower=np.array(lower[:16 * n * n], np.int32).reshape(n, 16, n))

    def delassus_layout(self, kmax=8, self_collision=True):
        """Where the step kernel keeps this model's Delassus blocks in an env's LDS region: dict(kcap, floats, row_pitch, block, dense_row) - block (i, k) starts
        row_pitch * i + block * k floats into the region; row_pitch 0 = the packed-triangular storage of the 16-slot classes (host only; rsb_model_delassus_layout)"""
        import ctypes
        t = (ctypes.c_int * 4)()
        kcap = lib().rsb_model_delassus_layout(self.handle, int(kmax), int(bool(self_collision)), t)
        check(min(kcap, 0), "rsb_model_delassus_layout")
        return dict(kcap=kcap, floats=int(t[0]), row_pitch=int(t[1]), block=int(t[2]), dense_row=int(t[3]))

    def collision_indices(self, suffix):
        return [i for i, n in enumerate(self.collision_names()) if n.endswith(suffix)]

    def collision_materials(self):
        """Material name of each collision primitive (<collision><material name=../> of the URDF, "default" if absent)."""
        return [(self.blob.col_material[i].value.decode() or "default") for i in range(self.ncol)]


def heightmap_from_png(path, height_scale=1.0, height_offset=0.0):
    """[y_samples, x_samples] float32 heights of a PNG (rsb_heightmap_png_*)."""
    L = lib()
    xs, ys = C.c_int(), C.c_int()
    check(L.rsb_heightmap_png_size(os.fspath(path).encode(), C.byref(xs), C.byref(ys)), "rsb_heightmap_png_size")
    h = np.zeros((ys.value, xs.value), np.float32)
    check(L.rsb_heightmap_png_read(os.fspath(path).encode(), float(height_scale), float(height_offset), _hp(h), h.size),
          "rsb_heightmap_png_read")
    return h


def heightmap_perlin(x_samples=100, y_samples=100, x_size=10.0, y_size=10.0, frequency=0.1, z_scale=1.0, fractal_octaves=5,
                     fractal_lacunarity=2.0, fractal_gain=0.5, step_size=0.0, seed=6479, height_offset=0.0):
    """[y_samples, x_samples] float32 Perlin terrain (rsb_heightmap_perlin; defaults = raisim::TerrainProperties [RECALL])."""
    tp = _capi.TerrainProperties(frequency, z_scale, x_size, y_size, x_samples, y_samples, fractal_octaves, seed,
                                 fractal_lacunarity, fractal_gain, step_size, height_offset)
    h = np.zeros((y_samples, x_samples), np.float32)
    check(lib().rsb_heightmap_perlin(C.byref(tp), _hp(h)), "rsb_heightmap_perlin")
    return h


def heightmap_from_text(path):
    """(heights [y_samples, x_samples] float32, x_size, y_size) of the text format (rsb_heightmap_text_*)."""
    L = lib()
    xs, ys, sx, sy = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    check(L.rsb_heightmap_text_size(os.fspath(path).encode(), C.byref(xs), C.byref(ys), C.byref(sx), C.byref(sy)),
          "rsb_heightmap_text_size")
    h = np.zeros((ys.value, xs.value), np.float32)
    check(L.rsb_heightmap_text_read(os.fspath(path).encode(), _hp(h), h.size), "rsb_heightmap_text_read")
    return h, sx.value, sy.value


def _host(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class BatchedWorld:
    def __init__(self, model: Model, num_envs: int, device: int = 0):
        self.L = lib()
        self.model = model
        h = C.c_void_p()
        check(self.L.rsb_create(model.handle, int(num_envs), int(device), C.byref(h)), "rsb_create")
        self.handle = h
        self.N, self.nq, self.nv = num_envs, model.nq, model.nv
        self.device = device

    def close(self):
        if getattr(self, "handle", None):
            self.L.rsb_destroy(self.handle)
            self.handle = None

    __del__ = close

    # -- raisim::World surface ---------------------------------------------------------------
    def set_time_step(self, dt):
        check(self.L.rsb_set_timestep(self.handle, float(dt)), "rsb_set_timestep")

    def get_time_step(self):
        return self.L.rsb_get_timestep(self.handle)

    def get_world_time(self):
        return self.L.rsb_get_world_time(self.handle)

    def set_gravity(self, g):
        arr = (C.c_double * 3)(*[float(x) for x in g])
        check(self.L.rsb_set_gravity(self.handle, arr), "rsb_set_gravity")

    def set_erp(self, erp):
        check(self.L.rsb_set_erp(self.handle, float(erp)), "rsb_set_erp")

    def set_default_material(self, mu, restitution=0.0, res_threshold=0.0):
        check(self.L.rsb_set_material(self.handle, float(mu), float(restitution), float(res_threshold)), "rsb_set_material")

    def set_collision_materials(self, mu=None, restitution=None, res_threshold=None):
        """Per collision primitive contact material against the terrain (the resolved World::setMaterialPairProp table):
        [ncol] arrays, None (or a negative entry) = the world's default material."""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (mu, restitution, res_threshold)]
        for a in arrs:
            if a is not None and a.shape != (self.model.ncol,):
                raise ValueError("set_collision_materials: arrays of ncol entries expected")
        check(self.L.rsb_set_collision_materials(self.handle, *[None if a is None else a.ctypes.data for a in arrs]),
              "rsb_set_collision_materials")

    def enable_generalized_force_output(self, on=True):
        """Have every launch also write the generalized force the actuators applied in its last sub-step ([N, nv])."""
        check(self.L.rsb_enable_generalized_force_output(self.handle, int(bool(on))), "rsb_enable_generalized_force_output")

    def get_generalized_force(self):
        """ArticulatedSystem::getGeneralizedForce() of every env: clipped PD + feed-forward of the last sub-step, [N, nv]."""
        out = np.zeros((self.N, self.model.nv), np.float32)
        check(self.L.rsb_get_field(self.handle, RSB_F_GENERALIZED_FORCE, _hp(out), RSB_HOST), "rsb_get_field(GENERALIZED_FORCE)")
        return out

    def get_pd_target(self):
        """the world's own copy of the position targets, [N, nq] (what the last control step / setPdTarget left)"""
        out = np.zeros((self.N, self.model.nq), np.float32)
        check(self.L.rsb_get_field(self.handle, 2, _hp(out), RSB_HOST), "rsb_get_field(PTARGET)")
        return out

    def set_self_collision(self, enable=True):
        """Collisions between non-adjacent bodies of the system (sphere x sphere; on by default, as in RaiSim)."""
        check(self.L.rsb_set_self_collision(self.handle, int(bool(enable))), "rsb_set_self_collision")

    def ignore_collision_between(self, body_a, body_b):
        """ArticulatedSystem::ignoreCollisionBetween(bodyIdx1, bodyIdx2); per-pair materials are reset."""
        check(self.L.rsb_ignore_collision_between(self.handle, int(body_a), int(body_b)), "rsb_ignore_collision_between")

    def self_collision_pairs(self):
        """[(i, j)] candidate primitive pairs (i < j) of self-collision."""
        n = self.L.rsb_self_collision_pairs(self.handle, None, 0)
        out = np.zeros((n, 2), np.int32)
        if n:
            self.L.rsb_self_collision_pairs(self.handle, out.ctypes.data, n)
        return out

    def set_self_collision_materials(self, mu=None, restitution=None, res_threshold=None):
        """One (mu, restitution, res_threshold) per candidate pair of self_collision_pairs(); None / negative = world default."""
        n = len(self.self_collision_pairs())
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (mu, restitution, res_threshold)]
        for a in arrs:
            if a is not None and a.shape != (n,):
                raise ValueError("set_self_collision_materials: one entry per candidate pair expected")
        check(self.L.rsb_set_self_collision_materials(self.handle, *[None if a is None else a.ctypes.data for a in arrs]),
              "rsb_set_self_collision_materials")

    def set_default_friction(self, mu):
        check(self.L.rsb_set_friction(self.handle, float(mu)), "rsb_set_friction")

    def set_contact_solver_param(self, alpha_init, alpha_min, alpha_decay, max_iter, threshold):
        check(self.L.rsb_set_contact_solver_param(self.handle, float(alpha_init), float(alpha_min), float(alpha_decay),
                                                  int(max_iter), float(threshold)), "rsb_set_contact_solver_param")

    def set_solver_stagnation_exit(self, window, factor):
        check(self.L.rsb_set_solver_stagnation_exit(self.handle, int(window), float(factor)), "rsb_set_solver_stagnation_exit")

    def set_solver_friction_lag(self, freeze_after, refine=True, settle_tol=1e-4):
        check(self.L.rsb_set_solver_friction_lag(self.handle, int(freeze_after), int(bool(refine)), float(settle_tol)),
              "rsb_set_solver_friction_lag")

    def set_solver_multi_contact(self, depth=3, light_passes=False, freeze_after=0, stall_window=16):
        """Solver settings of envs with >= depth contacts on one limb (redundant sets; see rsb.h). depth 0 = no distinction."""
        check(self.L.rsb_set_solver_multi_contact(self.handle, int(depth), int(bool(light_passes)), int(freeze_after), int(stall_window)),
              "rsb_set_solver_multi_contact")

    def set_integration_scheme(self, scheme="semi_implicit"):
        """'semi_implicit' (default), 'euler', 'trapezoid' (rsb.h: rsb_set_integration_scheme); 'runge_kutta_4' is refused."""
        code = {"trapezoid": 0, "semi_implicit": 1, "euler": 2, "runge_kutta_4": 3}[scheme] if isinstance(scheme, str) else int(scheme)
        check(self.L.rsb_set_integration_scheme(self.handle, code), "rsb_set_integration_scheme")

    def set_slip_rule(self, rule="energy"):
        """Slip rule of the per-contact iteration: "energy" (default: the published least-energy point) or "coulomb" (slip velocity anti-parallel to the
        friction impulse; a kernel class of its own, see rsb_set_slip_rule in include/rsb.h)."""
        code = {"energy": 0, "coulomb": 1}[rule] if isinstance(rule, str) else int(rule)
        check(self.L.rsb_set_slip_rule(self.handle, code), "rsb_set_slip_rule")

    def set_heightmap_contacts(self, per_primitive=2, min_angle_deg=45.0):
        """Contacts per collision primitive against a height map (1 = closest feature; 2 = also a second flank's; see rsb.h)."""
        check(self.L.rsb_set_heightmap_contacts(self.handle, int(per_primitive), float(min_angle_deg)), "rsb_set_heightmap_contacts")

    def set_step_pipelining(self, on=True):
        """Consecutive control steps overlap on the device (rsb_set_step_pipelining): bit-identical results, no launch waits for the slowest wave
        of the one before it; any other call joins the pipeline first."""
        check(self.L.rsb_set_step_pipelining(self.handle, int(bool(on))), "rsb_set_step_pipelining")
        return bool(self.L.rsb_step_pipelining_enabled(self.handle))     # False although asked for: RSB_STEP_PIPELINING=0 / a serialising profiler

    def step_pipelining_enabled(self):
        return bool(self.L.rsb_step_pipelining_enabled(self.handle))

    def step_pipeline_publish(self, stream_ptr):
        """`stream_ptr` (a hipStream_t as an integer) waits for the most recent pipelined control step; the pipeline keeps running"""
        check(self.L.rsb_step_pipeline_publish(self.handle, C.c_void_p(stream_ptr)), "rsb_step_pipeline_publish")

    def step_pipeline_wait_event(self, event_ptr):
        """the next control step additionally waits for the hipEvent_t `event_ptr` (an integer; the caller keeps it alive until then)"""
        check(self.L.rsb_step_pipeline_wait_event(self.handle, C.c_void_p(event_ptr)), "rsb_step_pipeline_wait_event")

    def step_pipelining_stats(self):
        a, b = C.c_longlong(0), C.c_longlong(0)
        st = self.L.rsb_step_pipelining_stats(self.handle, C.byref(a), C.byref(b))
        if st not in (0, 1):
            check(st, "rsb_step_pipelining_stats")
        self.pipeline_overlaps = st == 0        # False: no two streams on different hardware queues were found (correct, but in order)
        return int(a.value), int(b.value)

    def step_pipeline_join(self):
        """Waits for every pipelined step / stage pass in flight; raises RsbError (status RSB_E_PIPELINE) ONCE after a device-side fault - the
        library has by then restored the last joined state and replayed the steps in lock-step (include/rsb_pipeline.h)."""
        check(self.L.rsb_step_pipeline_join(self.handle), "rsb_step_pipeline_join")

    def step_pipeline_fault(self):
        """(faults so far, device code of the last one: RSB_PIPE_ERR_*)"""
        a, b = C.c_int(0), C.c_int(0)
        check(self.L.rsb_step_pipeline_fault(self.handle, C.byref(a), C.byref(b)), "rsb_step_pipeline_fault")
        return int(a.value), int(b.value)

    def debug_pipeline_wait_stats(self):
        """(mean wait of a pipelined step workgroup for its block in us, share of workgroups that waited); needs RSB_PIPE_STATS=1"""
        a, b = C.c_double(0), C.c_double(0)
        check(self.L.rsb_debug_pipeline_wait_stats(self.handle, C.byref(a), C.byref(b)), "rsb_debug_pipeline_wait_stats")
        return float(a.value), float(b.value)

    def debug_pipeline_fault(self, kind):
        """tests: the next pipelined launch fails on the device (1: ticket, 2: time-out, 4: error word set)"""
        check(self.L.rsb_debug_pipeline_fault(self.handle, int(kind)), "rsb_debug_pipeline_fault")

    def set_capsule_contacts(self, on=True):
        """Exact capsule / cylinder / box x height map: the barrel between a capsule's or cylinder's ends and the faces and edges between a box's corners
        report their deepest point (rsb_set_capsule_contacts)."""
        check(self.L.rsb_set_capsule_contacts(self.handle, int(bool(on))), "rsb_set_capsule_contacts")

    def set_solver_anderson(self, first_sweep=2, clip=20.0):
        """Anderson acceleration of the sweep in multi-contact envs of worlds with > 8 contact slots (see rsb.h). first_sweep 0 = off."""
        check(self.L.rsb_set_solver_anderson(self.handle, int(first_sweep), float(clip)), "rsb_set_solver_anderson")

    def set_early_termination(self, on=True):
        check(self.L.rsb_set_early_termination(self.handle, 1 if on else 0), "rsb_set_early_termination")

    def set_solver_warm_start(self, on=True):
        check(self.L.rsb_set_solver_warm_start(self.handle, 1 if on else 0), "rsb_set_solver_warm_start")

    def set_max_contacts(self, kmax):
        check(self.L.rsb_set_max_contacts(self.handle, int(kmax)), "rsb_set_max_contacts")

    def max_contacts(self):
        k = C.c_int()
        check(self.L.rsb_dims(self.handle, None, None, None, None, C.byref(k)), "rsb_dims")
        return k.value

    def set_lanes_per_env(self, lanes):
        check(self.L.rsb_set_lanes_per_env(self.handle, int(lanes)), "rsb_set_lanes_per_env")

    def lanes_per_env(self):
        return self.L.rsb_get_lanes_per_env(self.handle)

    def add_ground(self, z=0.0):
        check(self.L.rsb_set_ground(self.handle, float(z)), "rsb_set_ground")

    def add_height_map(self, x_samples, y_samples, x_size, y_size, center_x, center_y, heights):
        h = _host(heights, np.float32).reshape(y_samples, x_samples)
        check(self.L.rsb_set_heightmap(self.handle, int(x_samples), int(y_samples), float(x_size), float(y_size),
                                       float(center_x), float(center_y), _hp(h)), "rsb_set_heightmap")

    def add_height_maps(self, heights, x_size, y_size, center_x, center_y, env_map):
        """Terrain curricula: heights [n_maps, y_samples, x_samples], env_map [N] -> the map each env stands on."""
        h = _host(heights, np.float32)
        idx = _host(env_map, np.int32)
        assert h.ndim == 3 and idx.shape == (self.N,)
        check(self.L.rsb_set_heightmaps(self.handle, h.shape[0], h.shape[2], h.shape[1], float(x_size), float(y_size),
                                        float(center_x), float(center_y), _hp(h), _hp(idx)), "rsb_set_heightmaps")

    def integrate(self, n_substeps=1):
        check(self.L.rsb_integrate(self.handle, int(n_substeps)), "rsb_integrate")

    def integrate_masked(self, mask, n_substeps=1):
        """integrate() of the envs whose mask byte is non-zero only (host uint8 [N]); the others are left untouched."""
        m = _host(mask, np.uint8)
        assert m.shape == (self.N,)
        check(self.L.rsb_integrate_masked(self.handle, int(n_substeps), _hp(m), RSB_HOST), "rsb_integrate_masked")

    def set_done_output(self, done_device_ptr):
        """Device uint8 [N] buffer that every following control step fills with its done flags (0 / None: off)."""
        check(self.L.rsb_set_done_output(self.handle, C.c_void_p(done_device_ptr) if done_device_ptr else None), "rsb_set_done_output")

    def integrate1(self):
        check(self.L.rsb_integrate1(self.handle), "rsb_integrate1")

    def integrate2(self):
        check(self.L.rsb_integrate2(self.handle), "rsb_integrate2")

    def synchronize(self):
        check(self.L.rsb_synchronize(self.handle), "rsb_synchronize")

    def get_stream(self):
        """The world's stream (hipStream_t as an integer).  Joins pipelined control steps first: work enqueued on it afterwards sees them."""
        return self.L.rsb_get_stream(self.handle) or 0

    def set_stream(self, hip_stream_ptr):
        check(self.L.rsb_set_stream(self.handle, C.c_void_p(hip_stream_ptr)), "rsb_set_stream")

    # -- raisim::ArticulatedSystem surface (batched) ---------------------------------------------
    def set_state(self, gc=None, gv=None, mask=None):
        gc, gv, mask = _host(gc, np.float32), _host(gv, np.float32), _host(mask, np.uint8)
        check(self.L.rsb_set_state(self.handle, _hp(gc), _hp(gv), _hp(mask), RSB_HOST), "rsb_set_state")

    def get_state(self):
        gc = np.empty((self.N, self.nq), np.float32)
        gv = np.empty((self.N, self.nv), np.float32)
        check(self.L.rsb_get_state(self.handle, _hp(gc), _hp(gv), RSB_HOST), "rsb_get_state")
        return gc, gv

    def set_control_mode(self, mode):
        check(self.L.rsb_set_control_mode(self.handle, int(mode)), "rsb_set_control_mode")

    def set_pd_gains(self, kp, kd):
        kp, kd = _host(kp, np.float32), _host(kd, np.float32)
        assert kp.shape == (self.nv,) and kd.shape == (self.nv,)
        check(self.L.rsb_set_pd_gains(self.handle, _hp(kp), _hp(kd)), "rsb_set_pd_gains")

    def set_pd_target(self, p_target=None, d_target=None):
        p, d = _host(p_target, np.float32), _host(d_target, np.float32)
        check(self.L.rsb_set_pd_target(self.handle, _hp(p), _hp(d), RSB_HOST), "rsb_set_pd_target")

    def set_pd_target_device(self, p_ptr=None, d_ptr=None):
        check(self.L.rsb_set_pd_target(self.handle, C.c_void_p(p_ptr) if p_ptr else None,
                                       C.c_void_p(d_ptr) if d_ptr else None, RSB_DEVICE), "rsb_set_pd_target")

    def set_generalized_force(self, tau):
        t = _host(tau, np.float32)
        check(self.L.rsb_set_generalized_force(self.handle, _hp(t), RSB_HOST), "rsb_set_generalized_force")

    def get_contacts(self):
        kmax = self.max_contacts()
        counts = np.empty(self.N, np.int32)
        con = np.zeros((self.N, kmax), CONTACT_DTYPE)
        check(self.L.rsb_get_contacts(self.handle, _hp(counts), _hp(con), RSB_HOST), "rsb_get_contacts")
        return counts, con

    def get_mass_matrix(self):
        M = np.empty((self.N, self.nv, self.nv), np.float32)
        check(self.L.rsb_get_mass_matrix(self.handle, _hp(M), RSB_HOST), "rsb_get_mass_matrix")
        return M

    def get_inverse_mass_matrix(self):
        out = np.zeros((self.N, self.model.nv, self.model.nv), np.float32)
        check(self.L.rsb_get_inverse_mass_matrix(self.handle, _hp(out), RSB_HOST), "rsb_get_inverse_mass_matrix")
        return out

    def get_nonlinearities(self):
        h = np.empty((self.N, self.nv), np.float32)
        check(self.L.rsb_get_nonlinearities(self.handle, _hp(h), RSB_HOST), "rsb_get_nonlinearities")
        return h

    def get_flags(self):
        f = np.empty(self.N, np.int32)
        check(self.L.rsb_get_flags(self.handle, _hp(f), RSB_HOST), "rsb_get_flags")
        return f

    def get_solver_iterations(self):
        f = np.empty(self.N, np.int32)
        check(self.L.rsb_get_solver_iterations(self.handle, _hp(f), RSB_HOST), "rsb_get_solver_iterations")
        return f

    # -- frames: kinematics, Jacobians and external wrenches of every env in one call (rsb_frames.hip) ------------------
    def get_field(self, field):
        """A whole state field (RSB_F_GC / GV / PTARGET / DTARGET / TAU_FF / GENERALIZED_FORCE) as a host array [N, dim]."""
        dim = self.nq if int(field) in (_capi.RSB_F_GC, _capi.RSB_F_PTARGET) else self.nv
        out = np.empty((self.N, dim), np.float32)
        check(self.L.rsb_get_field(self.handle, int(field), _hp(out), RSB_HOST), "rsb_get_field")
        return out

    def _frames(self, frames):
        """frames: a list of (body, offset) pairs, body indices or link names -> (ctypes array of rsb_frame, count)"""
        if isinstance(frames, (str, int, np.integer)) or (isinstance(frames, tuple) and len(frames) == 2 and np.ndim(frames[1]) == 1):
            frames = [frames]
        arr = (_capi.Frame * max(1, len(frames)))()
        for k, f in enumerate(frames):
            body, off = f if isinstance(f, (tuple, list)) else (f, (0.0, 0.0, 0.0))
            if isinstance(body, str):
                name, body = body, self.model.body_index(body)
                if body < 0:
                    raise ValueError(f"no such link: {name}")
            arr[k].body = int(body)
            arr[k].offset[:] = [float(x) for x in off]
        return arr, len(frames)

    @staticmethod
    def _is_torch(x):      # a torch tensor travels as its device pointer, anything else as a host array (as VecEnv does)
        return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")

    def _frame_outputs(self, names, want, shapes, out, what):
        """-> (space, [pointer or None per name], {name: array / tensor}).  out: {name: torch CUDA tensor} (RSB_DEVICE, no synchronisation, results
        in the caller's tensors) or {name: float32 array} (RSB_HOST); None: fresh host arrays for the outputs asked for."""
        if out is None:
            out = {n: np.empty(shapes[n], np.float32) for n in names if want[n]}
        if not out:
            raise ValueError(f"{what}: no output asked for")
        if set(out) - set(names):
            raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(names))}")
        torch_like = [self._is_torch(v) for v in out.values()]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: outputs must be all torch tensors or all numpy arrays")
        ptrs = []
        for n in names:
            v = out.get(n)
            if v is None:
                ptrs.append(None)
            elif torch_like[0]:
                if not (v.is_cuda and v.is_contiguous() and str(v.dtype) == "torch.float32" and v.numel() == int(np.prod(shapes[n])) and v.device.index == self.device):
                    raise ValueError(f"{what}: {n} must be a contiguous float32 CUDA tensor of {int(np.prod(shapes[n]))} elements on cuda:{self.device}")
                ptrs.append(C.c_void_p(v.data_ptr()))
            else:
                if not (isinstance(v, np.ndarray) and v.dtype == np.float32 and v.flags.c_contiguous and v.size == int(np.prod(shapes[n]))):
                    raise ValueError(f"{what}: {n} must be a C-contiguous float32 array of {int(np.prod(shapes[n]))} elements")
                ptrs.append(_hp(v))
        return (RSB_DEVICE if torch_like[0] else RSB_HOST), ptrs, out

    def frame_kinematics(self, frames, pos=True, rot=False, lin_vel=False, ang_vel=False, out=None):
        """ArticulatedSystem::getFramePosition / getFrameOrientation / getFrameVelocity / getFrameAngularVelocity (and getPosition / getVelocity of a
        point of a body) of every env at once -> {"pos": [N, F, 3], "rot": [N, F, 3, 3] (world <- body), "lin_vel": [N, F, 3], "ang_vel": [N, F, 3]},
        world frame, the outputs asked for only.  frames: (body, offset) pairs, body indices or link names.  out: see _frame_outputs."""
        arr, n = self._frames(frames)
        names = ("pos", "rot", "lin_vel", "ang_vel")
        shapes = {"pos": (self.N, n, 3), "rot": (self.N, n, 3, 3), "lin_vel": (self.N, n, 3), "ang_vel": (self.N, n, 3)}
        space, ptrs, out = self._frame_outputs(names, dict(pos=pos, rot=rot, lin_vel=lin_vel, ang_vel=ang_vel), shapes, out, "frame_kinematics")
        check(self.L.rsb_get_frame_kinematics(self.handle, arr, n, *ptrs, space), "rsb_get_frame_kinematics")
        return out

    def frame_jacobians(self, frames, lin=True, rot=False, out=None):
        """getDenseFrameJacobian / getDenseFrameRotationalJacobian of every env at once -> {"lin": [N, F, 3, nv], "rot": [N, F, 3, nv]}:
        lin_vel = lin @ gv, ang_vel = rot @ gv (a fixed-base model keeps its six, zero, base columns)."""
        arr, n = self._frames(frames)
        shapes = {"lin": (self.N, n, 3, self.nv), "rot": (self.N, n, 3, self.nv)}
        space, ptrs, out = self._frame_outputs(("lin", "rot"), dict(lin=lin, rot=rot), shapes, out, "frame_jacobians")
        check(self.L.rsb_get_frame_jacobians(self.handle, arr, n, *ptrs, space), "rsb_get_frame_jacobians")
        return out

    def _udot_input(self, what, udot, device):
        """udot [N, nv] or None -> (C argument, what must stay alive until the call returns); a torch CUDA tensor with torch outputs (RSB_DEVICE),
        anything else is taken as a float32 host array (RSB_HOST), as _dynamics_inputs does"""
        args, keep = self._dynamics_inputs(("udot", what), udot, None, device)
        return args[0], keep

    def frame_accelerations(self, frames, udot=None, local=False, proper=False, lin=True, ang=False, out=None):
        """ArticulatedSystem::getFrameAcceleration of every env at once -> {"lin": [N, F, 3], "ang": [N, F, 3]}, the outputs asked for only: the
        classical acceleration of the frame's point (d/dt of lin_vel of frame_kinematics) = J_lin udot + Jdot_lin gv, and the angular acceleration
        of its body = J_rot udot + Jdot_rot gv, at the resident state.  udot [N, nv]: the component-wise derivative of gv, the convention of
        inverse_dynamics (None: zeros - the bias terms Jdot gv).  World frame; local=True: in the axes of the frame's body (R^T x); proper=True:
        lin minus the world's gravity vector, the specific force at the point.  out: see _frame_outputs; torch outputs take a torch udot."""
        arr, n = self._frames(frames)
        shapes = {"lin": (self.N, n, 3), "ang": (self.N, n, 3)}
        space, ptrs, out = self._frame_outputs(("lin", "ang"), dict(lin=lin, ang=ang), shapes, out, "frame_accelerations")
        ud, keep = self._udot_input("frame_accelerations", udot, space == RSB_DEVICE)
        flags = (_capi.RSB_ACC_LOCAL if local else 0) | (_capi.RSB_ACC_PROPER if proper else 0)
        check(self.L.rsb_get_frame_accelerations(self.handle, arr, n, ud, flags, *ptrs, space), "rsb_get_frame_accelerations")
        return out

    def frame_jacobian_rates(self, frames, lin=True, rot=False, out=None):
        """getTimeDerivativeOfSparseJacobian / getTimeDerivativeOfSparseRotationalJacobian of every env at once, dense -> {"lin": [N, F, 3, nv],
        "rot": [N, F, 3, nv]}: d/dt of frame_jacobians along the resident gv, so that frame_accelerations = J @ udot + Jdot @ gv for every udot
        (a fixed-base model keeps its six, zero, base columns)."""
        arr, n = self._frames(frames)
        shapes = {"lin": (self.N, n, 3, self.nv), "rot": (self.N, n, 3, self.nv)}
        space, ptrs, out = self._frame_outputs(("lin", "rot"), dict(lin=lin, rot=rot), shapes, out, "frame_jacobian_rates")
        check(self.L.rsb_get_frame_jacobian_rates(self.handle, arr, n, *ptrs, space), "rsb_get_frame_jacobian_rates")
        return out

    def imu_observe(self, frames, udot=None, out=None, row_stride=0):
        """The IMU rows of an observation: [N, F, 6], out[e, f, 0:3] = R^T (lin_acc - g) (accelerometer: the specific force at the frame's point in
        the axes of its body), out[e, f, 3:6] = R^T omega (gyro); udot as in frame_accelerations (after a control step: forward_dynamics of the
        applied force with contacts=True).  row_stride (floats, 0 = 6 F): with a larger value `out` is the first IMU column of a wider
        [N, row_stride] buffer - a torch view such as obs[:, k:] (only its data pointer is used) or a numpy array of N * row_stride floats - whose
        other columns are left alone.  A torch `out` takes a torch udot (RSB_DEVICE, no synchronisation)."""
        arr, F = self._frames(frames)
        width = 6 * F
        stride = int(row_stride) or width
        if stride == width:
            space, ptrs, res = self._frame_outputs(("out",), dict(out=True), {"out": (self.N, F, 6)}, None if out is None else {"out": out}, "imu_observe")
            ud, keep = self._udot_input("imu_observe", udot, space == RSB_DEVICE)
            check(self.L.rsb_imu_observe(self.handle, arr, F, ud, ptrs[0], 0, space), "rsb_imu_observe")
            return res["out"]
        if out is None:
            raise ValueError("imu_observe: a row_stride needs `out`")
        if self._is_torch(out):
            if not (out.is_cuda and str(out.dtype) == "torch.float32" and out.device.index == self.device):
                raise ValueError(f"imu_observe: out must be a float32 CUDA tensor on cuda:{self.device}")
            space, optr = RSB_DEVICE, C.c_void_p(out.data_ptr())
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and (stride < width or out.size >= (self.N - 1) * stride + width)):
                raise ValueError("imu_observe: out must be a C-contiguous float32 array that holds N rows of row_stride floats")
            space, optr = RSB_HOST, _hp(out)
        ud, keep = self._udot_input("imu_observe", udot, space == RSB_DEVICE)
        check(self.L.rsb_imu_observe(self.handle, arr, F, ud, optr, stride, space), "rsb_imu_observe")
        return out

    # -- contact sensors: body wrenches, the contact rows of an observation, feet air time (rsb_contact_sensor.hip) ------
    @staticmethod
    def _contact_flags(local, include_self):
        return (_capi.RSB_CONTACT_LOCAL if local else 0) | (0 if include_self else _capi.RSB_CONTACT_NO_SELF)

    def _sensor_buffer(self, what, name, v, dtype, count, device):
        """one caller-owned buffer of a contact-sensor call (None: not asked for) -> its C argument: a contiguous torch CUDA tensor (device) or a
        C-contiguous numpy array"""
        if v is None:
            return None
        if device:
            if not (self._is_torch(v) and v.is_cuda and v.is_contiguous() and str(v.dtype) == f"torch.{dtype}" and v.numel() == count and v.device.index == self.device):
                raise ValueError(f"{what}: {name} must be a contiguous {dtype} CUDA tensor of {count} elements on cuda:{self.device}")
            return C.c_void_p(v.data_ptr())
        if not (isinstance(v, np.ndarray) and v.dtype == np.dtype(dtype) and v.flags.c_contiguous and v.size == count):
            raise ValueError(f"{what}: {name} must be a C-contiguous {dtype} array of {count} elements")
        return _hp(v)

    def body_contact_wrenches(self, frames, local=False, include_self=True, force=True, torque=False, count=False, out=None):
        """The net contact wrench on the body of each frame, from the resident contact list (what get_contacts returns), for every env at once ->
        {"force": [N, F, 3], "torque": [N, F, 3], "count": [N, F] int32}, the outputs asked for only.  A frame owns the records of its body; a
        record acts as impulse / timestep at its position (the convention of inverse_dynamics(contacts=True)).  force: the sum of the owned
        records' forces; torque: their moment about the frame's point; count: how many there are.  World axes; local=True: the axes of the
        frame's body (R^T x).  include_self=False leaves self-collision records out.  out: {name: torch CUDA tensor} (RSB_DEVICE, no
        synchronisation; count as int32) or {name: numpy array}; None: fresh host arrays."""
        what = "body_contact_wrenches"
        arr, n = self._frames(frames)
        names = ("force", "torque", "count")
        dtypes = {"force": "float32", "torque": "float32", "count": "int32"}
        sizes = {"force": self.N * n * 3, "torque": self.N * n * 3, "count": self.N * n}
        if out is None:
            want = dict(force=force, torque=torque, count=count)
            out = {k: np.empty((self.N, n, 3) if k != "count" else (self.N, n), dtypes[k]) for k in names if want[k]}
        if not out:
            raise ValueError(f"{what}: no output asked for")
        if set(out) - set(names):
            raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(names))}")
        torch_like = [self._is_torch(v) for v in out.values()]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: outputs must be all torch tensors or all numpy arrays")
        ptrs = [self._sensor_buffer(what, k, out.get(k), dtypes[k], sizes[k], torch_like[0]) for k in names]
        check(self.L.rsb_get_body_contact_wrenches(self.handle, arr, n, self._contact_flags(local, include_self), *ptrs,
                                                   RSB_DEVICE if torch_like[0] else RSB_HOST), "rsb_get_body_contact_wrenches")
        return out

    def contact_observe(self, frames, threshold=1.0, local=False, include_self=True, out=None, row_stride=0):
        """The contact rows of an observation: [N, F, 6], out[e, f] = (contact flag: 1 where the normal force exceeds `threshold` [N], else 0; the
        net force on the frame's body, the bits of body_contact_wrenches' force; the normal force sum (impulse . normal) / timestep; the slip
        speed: the largest tangential speed of the body's material point at an owned record).  local / include_self as in
        body_contact_wrenches.  row_stride (floats, 0 = 6 F): with a larger value `out` is the first contact column of a wider [N, row_stride]
        buffer - a torch view such as obs[:, k:] (only its data pointer is used) or a numpy array of N * row_stride floats - whose other columns
        are left alone.  A torch `out` means RSB_DEVICE, no synchronisation."""
        arr, F = self._frames(frames)
        width = 6 * F
        stride = int(row_stride) or width
        flags = self._contact_flags(local, include_self)
        if stride == width:
            space, ptrs, res = self._frame_outputs(("out",), dict(out=True), {"out": (self.N, F, 6)}, None if out is None else {"out": out}, "contact_observe")
            check(self.L.rsb_contact_observe(self.handle, arr, F, flags, float(threshold), ptrs[0], 0, space), "rsb_contact_observe")
            return res["out"]
        if out is None:
            raise ValueError("contact_observe: a row_stride needs `out`")
        if self._is_torch(out):
            if not (out.is_cuda and str(out.dtype) == "torch.float32" and out.device.index == self.device):
                raise ValueError(f"contact_observe: out must be a float32 CUDA tensor on cuda:{self.device}")
            space, optr = RSB_DEVICE, C.c_void_p(out.data_ptr())
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and (stride < width or out.size >= (self.N - 1) * stride + width)):
                raise ValueError("contact_observe: out must be a C-contiguous float32 array that holds N rows of row_stride floats")
            space, optr = RSB_HOST, _hp(out)
        check(self.L.rsb_contact_observe(self.handle, arr, F, flags, float(threshold), optr, stride, space), "rsb_contact_observe")
        return out

    def contact_timers(self, frames, dt, air_time, contact_time=None, touchdown=None, reset_mask=None, threshold=1.0, include_self=True):
        """Feet air time / contact time, kept in the caller's [N, F] float32 buffers and updated in place, once per control step of length dt:
        where reset_mask[e] != 0 (uint8 [N], e.g. the done flags) all three restart at 0; in contact (the flag of contact_observe)
        touchdown = the old air_time (the flight that just ended), air_time = 0, contact_time += dt; otherwise touchdown = 0, air_time += dt,
        contact_time = 0.  Either timer may be None, not both; touchdown is an output only.  All torch CUDA tensors (RSB_DEVICE, no
        synchronisation) or all numpy arrays.  -> (air_time, contact_time, touchdown)"""
        what = "contact_timers"
        arr, n = self._frames(frames)
        given = [x for x in (air_time, contact_time, touchdown, reset_mask) if x is not None]
        if air_time is None and contact_time is None:
            raise ValueError(f"{what}: air_time and contact_time are both None")
        torch_like = [self._is_torch(x) for x in given]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: the buffers must be all torch tensors or all numpy arrays")
        dev = torch_like[0]
        pairs = self.N * n
        ptrs = [self._sensor_buffer(what, "reset_mask", reset_mask, "uint8", self.N, dev), self._sensor_buffer(what, "air_time", air_time, "float32", pairs, dev),
                self._sensor_buffer(what, "contact_time", contact_time, "float32", pairs, dev), self._sensor_buffer(what, "touchdown", touchdown, "float32", pairs, dev)]
        check(self.L.rsb_contact_timers(self.handle, arr, n, self._contact_flags(False, include_self), float(threshold), float(dt), *ptrs,
                                        RSB_DEVICE if dev else RSB_HOST), "rsb_contact_timers")
        return air_time, contact_time, touchdown

    def add_external_wrench(self, frame, force=None, torque=None, mask=None):
        """setExternalForce / setExternalTorque of every env at once: tau_ff[e] += J_lin(e)^T force[e] + J_rot(e)^T torque[e] at the current state
        for the envs with mask[e] != 0 (None: all).  force / torque [N, 3] world frame, mask [N] uint8: numpy arrays, or torch CUDA tensors (no
        synchronisation).  The generalized force stays in the feed-forward rows until set_generalized_force replaces it."""
        arr, n = self._frames(frame)
        if n != 1:
            raise ValueError("add_external_wrench: one frame expected")
        given = [x for x in (force, torque, mask) if x is not None]
        torch_like = [self._is_torch(x) for x in given]
        if given and any(torch_like) != all(torch_like):
            raise ValueError("add_external_wrench: force, torque and mask must be all torch tensors or all numpy arrays")
        if given and torch_like[0]:
            for x, name, dt, cnt in ((force, "force", "torch.float32", 3 * self.N), (torque, "torque", "torch.float32", 3 * self.N), (mask, "mask", "torch.uint8", self.N)):
                if x is not None and not (x.is_cuda and x.is_contiguous() and str(x.dtype) == dt and x.numel() == cnt and x.device.index == self.device):
                    raise ValueError(f"add_external_wrench: {name} must be a contiguous {dt} CUDA tensor of {cnt} elements on cuda:{self.device}")
            ptrs = [None if x is None else C.c_void_p(x.data_ptr()) for x in (force, torque, mask)]
            space = RSB_DEVICE
        else:
            f, t, m = _host(force, np.float32), _host(torque, np.float32), _host(mask, np.uint8)
            for x, name, cnt in ((f, "force", 3 * self.N), (t, "torque", 3 * self.N), (m, "mask", self.N)):
                if x is not None and x.size != cnt:
                    raise ValueError(f"add_external_wrench: {name} must hold {cnt} elements")
            ptrs = [_hp(f), _hp(t), _hp(m)]
            space = RSB_HOST
        check(self.L.rsb_add_external_wrench(self.handle, arr, *ptrs, space), "rsb_add_external_wrench")

    # -- whole-body quantities of every env in one call (rsb_centroidal.hip) ------------------------------------------------
    def centroidal(self, com=True, com_vel=False, lin_mom=False, ang_mom=False, kinetic=False, potential=False, out=None):
        """ArticulatedSystem::getCOM / getLinearMomentum / getAngularMomentum / getKineticEnergy / getPotentialEnergy of every env at once ->
        {"com": [N, 3], "com_vel": [N, 3], "lin_mom": [N, 3], "ang_mom": [N, 3] (about the centre of mass), "kinetic": [N], "potential": [N]
        (= -M g . com with set_gravity's vector)}, world frame, the outputs asked for only.  out: see _frame_outputs."""
        names = ("com", "com_vel", "lin_mom", "ang_mom", "kinetic", "potential")
        shapes = {n: (self.N, 3) for n in names[:4]}
        shapes.update(kinetic=(self.N,), potential=(self.N,))
        want = dict(com=com, com_vel=com_vel, lin_mom=lin_mom, ang_mom=ang_mom, kinetic=kinetic, potential=potential)
        space, ptrs, out = self._frame_outputs(names, want, shapes, out, "centroidal")
        check(self.L.rsb_get_centroidal(self.handle, *ptrs, space), "rsb_get_centroidal")
        return out

    def centroidal_momentum_matrix(self, out=None):
        """The centroidal momentum matrix of every env: A [N, 6, nv] with (lin_mom, ang_mom about the centre of mass) = A @ gv; A[:, 3:, 3:6] is the
        composite inertia about the centre of mass, A[:, :3] / total mass the Jacobian of the centre of mass (a fixed-base model keeps its six,
        zero, base columns).  out: a float32 array or a torch CUDA tensor of N * 6 * nv elements (RSB_DEVICE, no synchronisation)."""
        space, ptrs, res = self._frame_outputs(("A",), dict(A=True), {"A": (self.N, 6, self.nv)}, None if out is None else {"A": out}, "centroidal_momentum_matrix")
        check(self.L.rsb_get_centroidal_momentum_matrix(self.handle, ptrs[0], space), "rsb_get_centroidal_momentum_matrix")
        return res["A"]

    # -- dynamics: inverse dynamics with joint reaction wrenches, contact-free forward dynamics of every env in one call (rsb_dynamics.hip) ---
    def _dynamics_inputs(self, what, first, loads, device):
        """first: udot / tau [N, nv] or None; loads: None or (frames, force, torque) with force / torque [N, F, 3] (either may be None).  Inputs
        follow the outputs: torch CUDA tensors with torch outputs (RSB_DEVICE), anything else is taken as a float32 host array (RSB_HOST).
        -> ([first, frames, n, force, torque] as C arguments, what must stay alive until the call returns)"""
        frames, force, torque = loads if loads is not None else ([], None, None)
        arr, n = self._frames(frames) if loads is not None else (None, 0)
        keep, ptrs = [], []
        for name, v, cnt in ((what[0], first, self.N * self.nv), ("force", force, self.N * n * 3), ("torque", torque, self.N * n * 3)):
            if v is None:
                ptrs.append(None)
            elif device:
                if not (self._is_torch(v) and v.is_cuda and v.is_contiguous() and str(v.dtype) == "torch.float32" and v.numel() == cnt and v.device.index == self.device):
                    raise ValueError(f"{what[1]}: {name} must be a contiguous float32 CUDA tensor of {cnt} elements on cuda:{self.device}")
                ptrs.append(C.c_void_p(v.data_ptr()))
            else:
                if self._is_torch(v):
                    raise ValueError(f"{what[1]}: inputs and outputs must be all torch tensors or all numpy arrays")
                a = _host(v, np.float32)
                if a.size != cnt:
                    raise ValueError(f"{what[1]}: {name} must hold {cnt} elements")
                keep.append(a)
                ptrs.append(_hp(a))
        return [ptrs[0], arr, n, ptrs[1], ptrs[2]], keep

    def inverse_dynamics(self, udot=None, loads=None, contacts=False, tau=True, joint_force=False, joint_torque=False, out=None):
        """The generalized force that accelerates every env with udot [N, nv] (None: zeros - gravity compensation at rest, h in general) at the
        resident state, in the convention of get_mass_matrix / get_nonlinearities: tau = M udot + h - J^T loads -> {"tau": [N, nv], "joint_force":
        [N, nb, 3], "joint_torque": [N, nb, 3]}, the outputs asked for only.  joint_force / joint_torque[e, i]: what body i's parent (the world for
        i = 0) exerts on body i through joint i, world frame, the torque about joint i's origin.  loads = (frames, force, torque): frames as in
        frame_kinematics, force [N, F, 3] applied at the frame's point, torque [N, F, 3] applied to its body, world frame, either may be None.
        contacts=True: the resident contact list acts too, every record as impulse / dt at its position on its body.  No PD, damping, effort clip
        or joint limits enter.  The world is left as it was.  out: see _frame_outputs; torch outputs take torch inputs (no synchronisation)."""
        names = ("tau", "joint_force", "joint_torque")
        shapes = {"tau": (self.N, self.nv), "joint_force": (self.N, self.model.nb, 3), "joint_torque": (self.N, self.model.nb, 3)}
        space, ptrs, out = self._frame_outputs(names, dict(tau=tau, joint_force=joint_force, joint_torque=joint_torque), shapes, out, "inverse_dynamics")
        args, keep = self._dynamics_inputs(("udot", "inverse_dynamics"), udot, loads, space == RSB_DEVICE)
        check(self.L.rsb_inverse_dynamics(self.handle, *args, _capi.RSB_DYN_CONTACTS if contacts else 0, *ptrs, space), "rsb_inverse_dynamics")
        return out

    def forward_dynamics(self, tau=None, loads=None, contacts=False, out=None):
        """The acceleration udot [N, nv] the generalized force tau [N, nv] (None: the resident feed-forward rows) produces at the resident state
        without contact resolution: udot = M^-1 (tau - h + J^T loads), by the articulated-body algorithm; the exact inverse of inverse_dynamics,
        with its loads and contacts arguments.  A fixed base: udot[:, :6] = 0.  out: a float32 array or a torch CUDA tensor of N * nv elements."""
        space, ptrs, res = self._frame_outputs(("udot",), dict(udot=True), {"udot": (self.N, self.nv)}, None if out is None else {"udot": out}, "forward_dynamics")
        args, keep = self._dynamics_inputs(("tau", "forward_dynamics"), tau, loads, space == RSB_DEVICE)
        check(self.L.rsb_forward_dynamics(self.handle, *args, _capi.RSB_DYN_CONTACTS if contacts else 0, ptrs[0], space), "rsb_forward_dynamics")
        return res["udot"]

    # -- the slopes of the two: analytic derivatives of every env in one call (rsb_dynamics_derivatives.hip) -------------------------------
    def inverse_dynamics_derivatives(self, udot=None, loads=None, dq=True, dv=True, dudot=False, out=None):
        """The exact derivatives of inverse_dynamics(udot, loads) at the resident state -> {"dq": [N, nv, nv] d tau_i / d x_j, "dv": [N, nv, nv]
        d tau_i / d gv_j, "dudot": [N, nv, nv] = M(q)}, the outputs asked for only.  x is the tangent coordinate of gc in gv's order: the base
        origin along the world axes, the base rotated about the WORLD axes (quaternion multiplied on the left), the joint coordinates.  gv,
        udot, gravity and the loads' world force / torque are held fixed; a load's point moves with its body.  Columns 0..2 of "dq" are zero.
        No contacts.  The world is left as it was.  out: see _frame_outputs; torch outputs take torch inputs (no synchronisation)."""
        names = ("dq", "dv", "dudot")
        shapes = {n: (self.N, self.nv, self.nv) for n in names}
        space, ptrs, out = self._frame_outputs(names, dict(dq=dq, dv=dv, dudot=dudot), shapes, out, "inverse_dynamics_derivatives")
        args, keep = self._dynamics_inputs(("udot", "inverse_dynamics_derivatives"), udot, loads, space == RSB_DEVICE)
        check(self.L.rsb_inverse_dynamics_derivatives(self.handle, *args, 0, *ptrs, space), "rsb_inverse_dynamics_derivatives")
        return out

    def forward_dynamics_derivatives(self, tau=None, loads=None, udot=False, dq=True, dv=True, dtau=False, out=None):
        """The exact derivatives of forward_dynamics(tau, loads) at the resident state -> {"udot": [N, nv] the forward dynamics itself, "dq":
        [N, nv, nv] = -M^-1 d tau / d x at that udot, "dv": [N, nv, nv] = -M^-1 d tau / d gv, "dtau": [N, nv, nv] = M^-1}, the outputs asked
        for only; the conventions of inverse_dynamics_derivatives.  With S the selection of the actuated rows, the continuous-time linearisation
        of d/dt (x, gv) is A = [[0, I], [dq, dv]], B = [[0], [dtau S^T]].  A fixed base: rows and columns 0..5 are zero."""
        names = ("udot", "dq", "dv", "dtau")
        shapes = {"udot": (self.N, self.nv), **{n: (self.N, self.nv, self.nv) for n in names[1:]}}
        space, ptrs, out = self._frame_outputs(names, dict(udot=udot, dq=dq, dv=dv, dtau=dtau), shapes, out, "forward_dynamics_derivatives")
        args, keep = self._dynamics_inputs(("tau", "forward_dynamics_derivatives"), tau, loads, space == RSB_DEVICE)
        check(self.L.rsb_forward_dynamics_derivatives(self.handle, *args, 0, *ptrs, space), "rsb_forward_dynamics_derivatives")
        return out

    # -- inverse mass: M^-1 B and the frames' Delassus matrices of every env in one call (rsb_inverse_mass.hip) -----------------------------
    def _joint_diag(self, what, joint_diag):
        """joint_diag [nv] or None -> (C argument, what must stay alive until the call returns): always a float32 HOST array"""
        if joint_diag is None:
            return None, None
        if self._is_torch(joint_diag):
            joint_diag = joint_diag.detach().cpu().numpy()
        a = _host(joint_diag, np.float32)
        if a.size != self.nv:
            raise ValueError(f"{what}: joint_diag must hold {self.nv} elements")
        return _hp(a), a

    def apply_inverse_mass(self, B, joint_diag=None, out=None):
        """X [N, R, nv] = (M(q) + diag(joint_diag))^-1 B for B [N, R, nv] (or [N, nv]: R = 1, X [N, nv]) at the resident configuration, in the
        convention of get_mass_matrix, by the articulated-body factorisation: one factorisation per env, two tree passes per column, no dense M.
        joint_diag [nv] (host; None: zeros): non-negative, zero on a floating base's six entries - dt (kd + dt kp) gives the effective mass the
        step's contact problem sees.  A fixed base: the joint block is solved, X[..., :6] = 0.  Only gc is read; the world is left as it was.
        out: a float32 array or a torch CUDA tensor of B's size (RSB_DEVICE, no synchronisation; B is then a torch CUDA tensor too); out may be B."""
        cnt = int(B.numel()) if self._is_torch(B) else int(np.size(B))
        if cnt == 0 or cnt % (self.N * self.nv):
            raise ValueError(f"apply_inverse_mass: B must hold N * R * nv = {self.N} * R * {self.nv} elements")
        R = cnt // (self.N * self.nv)
        shape = (self.N, self.nv) if (B.dim() if self._is_torch(B) else np.ndim(B)) == 2 and R == 1 else (self.N, R, self.nv)
        space, ptrs, res = self._frame_outputs(("X",), dict(X=True), {"X": shape}, None if out is None else {"X": out}, "apply_inverse_mass")
        if space == RSB_DEVICE:
            if not (self._is_torch(B) and B.is_cuda and B.is_contiguous() and str(B.dtype) == "torch.float32" and B.device.index == self.device):
                raise ValueError(f"apply_inverse_mass: B must be a contiguous float32 CUDA tensor on cuda:{self.device}")
            bp, keep = C.c_void_p(B.data_ptr()), B
        else:
            if self._is_torch(B):
                raise ValueError("apply_inverse_mass: inputs and outputs must be all torch tensors or all numpy arrays")
            keep = B if out is B else _host(B, np.float32)
            bp = _hp(keep)
        dp, dkeep = self._joint_diag("apply_inverse_mass", joint_diag)
        check(self.L.rsb_apply_inverse_mass(self.handle, bp, R, dp, ptrs[0], space), "rsb_apply_inverse_mass")
        return res["X"]

    def frame_delassus(self, frames, angular=False, joint_diag=None, G=True, JMinv=False, out=None):
        """The operational-space matrices of every env at the resident configuration -> {"G": [N, kF, kF] = J (M + D)^-1 J^T, "JMinv": [N, kF, nv]
        = J (M + D)^-1}, the outputs asked for only.  J stacks the rows of frame_jacobians: k = 3 rows per frame (lin), or with angular=True k = 6
        (lin, then rot).  G equals its transpose bit for bit and may be singular; Lambda = G^-1 (a damped Cholesky, say) is the caller's.
        frames: at most 16, as in frame_kinematics; joint_diag as in apply_inverse_mass.  out: see _frame_outputs."""
        arr, n = self._frames(frames)
        k = (6 if angular else 3) * n
        shapes = {"G": (self.N, k, k), "JMinv": (self.N, k, self.nv)}
        space, ptrs, out = self._frame_outputs(("G", "JMinv"), dict(G=G, JMinv=JMinv), shapes, out, "frame_delassus")
        dp, dkeep = self._joint_diag("frame_delassus", joint_diag)
        check(self.L.rsb_get_frame_delassus(self.handle, arr, n, _capi.RSB_DELASSUS_ANGULAR if angular else 0, dp, *ptrs, space), "rsb_get_frame_delassus")
        return out

    # -- frames held: constrained forward dynamics and frame impulses of every env in one call (rsb_constrained.hip) ------------------------
    def _held(self, what, frames, angular, tau, target, lead, want, out):
        """the arguments both held-frame queries share (tau: None for the impulse) -> (frame array, count, flags, [tau, target] as C arguments,
        output pointers (lead, lambda, status), space, outputs, the host arrays the pointers refer to: the caller holds them until its call returns).  Outputs as in _frame_outputs, but status is int32; inputs follow the outputs."""
        arr, n = self._frames(frames)
        m = (6 if angular else 3) * n
        names = (lead, "lambda", "status")
        shapes = {lead: (self.N, self.nv), "lambda": (self.N, m), "status": (self.N,)}
        if out is None:
            out = {k: np.empty(shapes[k], np.int32 if k == "status" else np.float32) for k in names if want[k]}
        if not out:
            raise ValueError(f"{what}: no output asked for")
        if set(out) - set(names):
            raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(names))}")
        torch_like = [self._is_torch(v) for v in out.values()]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: outputs must be all torch tensors or all numpy arrays")
        dev = torch_like[0]
        ptrs = []
        for k in names:
            v, cnt, dt = out.get(k), int(np.prod(shapes[k])), ("int32" if k == "status" else "float32")
            if v is None:
                ptrs.append(None)
            elif dev:
                if not (v.is_cuda and v.is_contiguous() and str(v.dtype) == "torch." + dt and v.numel() == cnt and v.device.index == self.device):
                    raise ValueError(f"{what}: {k} must be a contiguous {dt} CUDA tensor of {cnt} elements on cuda:{self.device}")
                ptrs.append(C.c_void_p(v.data_ptr()))
            else:
                if not (isinstance(v, np.ndarray) and v.dtype == np.dtype(dt) and v.flags.c_contiguous and v.size == cnt):
                    raise ValueError(f"{what}: {k} must be a C-contiguous {dt} array of {cnt} elements")
                ptrs.append(_hp(v))
        keep, ins = [], []
        for name, v, cnt in (("tau", tau, self.N * self.nv), ("target", target, self.N * m)):
            if v is None:
                ins.append(None)
            elif dev:
                if not (self._is_torch(v) and v.is_cuda and v.is_contiguous() and str(v.dtype) == "torch.float32" and v.numel() == cnt and v.device.index == self.device):
                    raise ValueError(f"{what}: {name} must be a contiguous float32 CUDA tensor of {cnt} elements on cuda:{self.device}")
                ins.append(C.c_void_p(v.data_ptr()))
            else:
                if self._is_torch(v):
                    raise ValueError(f"{what}: inputs and outputs must be all torch tensors or all numpy arrays")
                a = _host(v, np.float32)
                if a.size != cnt:
                    raise ValueError(f"{what}: {name} must hold {cnt} elements")
                keep.append(a)
                ins.append(_hp(a))
        return arr, n, (_capi.RSB_DELASSUS_ANGULAR if angular else 0), ins, ptrs, (RSB_DEVICE if dev else RSB_HOST), out, keep

    def constrained_forward_dynamics(self, frames, tau=None, angular=False, target_acc=None, damping=0.0, udot=True, lam=True, status=True, out=None):
        """Forward dynamics with frames held, every env at once -> {"udot": [N, nv], "lambda": [N, kF], "status": [N] int32}, the outputs asked for
        only.  With J, G, JMinv of frame_delassus(frames, angular) and rho = damping * max diag G:  (G + rho I) lambda = target_acc - (J udot_f +
        Jdot gv), udot = udot_f + JMinv^T lambda, udot_f = forward_dynamics(tau): then J udot + Jdot gv = target_acc - rho lambda and
        M udot + h = tau + J^T lambda.  lambda: the world force (and with angular=True torque) the constraint applies at each frame, rows ordered
        as G's.  tau [N, nv] (None: the resident feed-forward rows); target_acc [N, kF] (None: zeros - the frames are held; Baumgarte terms go
        here).  status 0: solved; 1 (RSB_HELD_SINGULAR): the rows are dependent to float precision (rsb.h) - that env's lambda is zero and its udot
        is udot_f; damping > 0 makes such a set solvable.  The world is left as it was.  out: {name: float32 array (int32 for status)} or
        {name: torch CUDA tensor} (RSB_DEVICE, no synchronisation; tau and target_acc are then torch CUDA tensors too)."""
        what = "constrained_forward_dynamics"
        arr, n, flags, ins, ptrs, space, out, keep = self._held(what, frames, angular, tau, target_acc, "udot", dict(udot=udot, status=status, **{"lambda": lam}), out)
        check(self.L.rsb_constrained_forward_dynamics(self.handle, ins[0], arr, n, flags, ins[1], float(damping), *ptrs, space), "rsb_constrained_forward_dynamics")
        return out

    def frame_impulse(self, frames, angular=False, target_vel=None, joint_diag=None, damping=0.0, dgv=True, lam=True, status=True, out=None):
        """The impulse that brings frames to target_vel [N, kF] (None: zeros - the frames are stopped), every env at once -> {"dgv": [N, nv],
        "lambda": [N, kF], "status": [N] int32}:  (G + rho I) lambda = target_vel - J gv, dgv = (M + D)^-1 J^T lambda, G and D = diag(joint_diag)
        as in frame_delassus, rho and status as in constrained_forward_dynamics.  gc and gv are read, nothing is written to the world: add dgv to
        gv.  out: as in constrained_forward_dynamics."""
        what = "frame_impulse"
        arr, n, flags, ins, ptrs, space, out, keep = self._held(what, frames, angular, None, target_vel, "dgv", dict(dgv=dgv, status=status, **{"lambda": lam}), out)
        dp, dkeep = self._joint_diag(what, joint_diag)
        check(self.L.rsb_frame_impulse(self.handle, arr, n, flags, ins[1], dp, float(damping), *ptrs, space), "rsb_frame_impulse")
        return out

    # -- inverse kinematics at frames: the configuration that puts frames at chosen places, every env in one call (rsb_ik.hip) ----------------
    def inverse_kinematics(self, frames, target_pos, target_rot=None, gc_init=None, dof_mask=None, joint_limits=False, max_iter=20, damping=1e-3,
                           pos_tol=1e-4, rot_tol=1e-4, max_step=0.5, gc=True, error=True, iterations=True, status=True, out=None):
        """The configuration that puts frames at target_pos [N, F, 3] (and, with target_rot [N, F, 9] row-major world<-body, in those orientations),
        every env at once -> {"gc": [N, nq], "error": [N, 2] (largest position row [m], largest rotation row [rad]) at gc, "iterations": [N] int32,
        "status": [N] int32}, the outputs asked for only.  A damped Gauss-Newton iteration in float from gc_init [N, nq] (None: the resident gc):
        (J J^T + damping max diag I) y = e, dq = J^T y clipped to max_step, q (+) dq with the base quaternion multiplied on the left (rsb.h states
        every step).  dof_mask [nv] (host; None: the joints are free, the base is held): the coordinates of gv's order that may move; what is not
        free keeps the start's bits.  joint_limits=True clamps every iterate's joints into the model's limits.  status 0: within pos_tol / rot_tol;
        1 (RSB_IK_MAX_ITER): max_iter steps taken; 2 (RSB_IK_SINGULAR): the rows depend on each other to float precision and damping is too small.
        max_iter=0 evaluates the start.  The world is left as it was.  out: {name: float32 array (int32 for iterations, status)} or {name: torch
        CUDA tensor} (RSB_DEVICE, no synchronisation; the targets and gc_init are then torch CUDA tensors too)."""
        what = "inverse_kinematics"
        arr, n = self._frames(frames)
        names = ("gc", "error", "iterations", "status")
        shapes = {"gc": (self.N, self.nq), "error": (self.N, 2), "iterations": (self.N,), "status": (self.N,)}
        dtypes = {"gc": "float32", "error": "float32", "iterations": "int32", "status": "int32"}
        if out is None:
            want = dict(gc=gc, error=error, iterations=iterations, status=status)
            out = {k: np.empty(shapes[k], dtypes[k]) for k in names if want[k]}
        if not out:
            raise ValueError(f"{what}: no output asked for")
        if set(out) - set(names):
            raise ValueError(f"{what}: unknown outputs {sorted(set(out) - set(names))}")
        torch_like = [self._is_torch(v) for v in out.values()]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: outputs must be all torch tensors or all numpy arrays")
        dev = torch_like[0]
        ptrs = [self._sensor_buffer(what, k, out.get(k), dtypes[k], int(np.prod(shapes[k])), dev) for k in names]
        keep, ins = [], []
        for name, v, cnt in (("target_pos", target_pos, self.N * n * 3), ("target_rot", target_rot, self.N * n * 9), ("gc_init", gc_init, self.N * self.nq)):
            if v is None:
                ins.append(None)
            elif dev:
                ins.append(self._sensor_buffer(what, name, v, "float32", cnt, True))
            else:
                if self._is_torch(v):
                    raise ValueError(f"{what}: inputs and outputs must be all torch tensors or all numpy arrays")
                a = _host(v, np.float32)
                if a.size != cnt:
                    raise ValueError(f"{what}: {name} must hold {cnt} elements")
                keep.append(a)
                ins.append(_hp(a))
        mp = None
        if dof_mask is not None:
            if self._is_torch(dof_mask):
                dof_mask = dof_mask.detach().cpu().numpy()
            mk = np.ascontiguousarray(np.asarray(dof_mask) != 0, np.uint8)
            if mk.size != self.nv:
                raise ValueError(f"{what}: dof_mask must hold {self.nv} elements")
            keep.append(mk)
            mp = _hp(mk)
        opt = _capi.IkOptions(int(max_iter), float(damping), float(pos_tol), float(rot_tol), float(max_step))
        flags = (_capi.RSB_IK_ANGULAR if target_rot is not None else 0) | (_capi.RSB_IK_JOINT_LIMITS if joint_limits else 0)
        check(self.L.rsb_inverse_kinematics(self.handle, arr, n, flags, *ins, mp, C.byref(opt), *ptrs, RSB_DEVICE if dev else RSB_HOST), "rsb_inverse_kinematics")
        return out

    # -- terrain: heights, height scans and ray tests of every env in one call (rsb_terrain_query.hip) -------------------
    def _terrain_io(self, what, inputs, out_shapes, out):
        """inputs {name: (value, shape)}, out_shapes {name: shape}, out {name: array / tensor or None} -> (space, input pointers, output pointers,
        outputs).  The conventions of _frame_outputs: torch CUDA tensors travel as device pointers (RSB_DEVICE, no synchronisation), anything else
        as float32 host arrays (RSB_HOST); inputs and outputs must agree."""
        given = [v for v, _ in inputs.values()] + [v for v in out.values() if v is not None]
        torch_like = [self._is_torch(v) for v in given]
        if any(torch_like) != all(torch_like):
            raise ValueError(f"{what}: inputs and outputs must be all torch tensors or all numpy arrays")
        dev = torch_like[0]

        def tensor_ptr(n, v, shape):
            cnt = int(np.prod(shape))
            if not (v.is_cuda and v.is_contiguous() and str(v.dtype) == "torch.float32" and v.numel() == cnt and v.device.index == self.device):
                raise ValueError(f"{what}: {n} must be a contiguous float32 CUDA tensor of {cnt} elements on cuda:{self.device}")
            return C.c_void_p(v.data_ptr())
        keep, in_ptrs, out_ptrs, res = [], [], [], {}
        for n, (v, shape) in inputs.items():
            if dev:
                in_ptrs.append(tensor_ptr(n, v, shape))
            else:
                a = _host(v, np.float32)
                if a.size != int(np.prod(shape)):
                    raise ValueError(f"{what}: {n} must hold {int(np.prod(shape))} elements")
                keep.append(a)
                in_ptrs.append(_hp(a))
        for n, shape in out_shapes.items():
            v = out.get(n)
            if v is None:
                if dev:
                    raise ValueError(f"{what}: with torch inputs pass the outputs as torch tensors (out=)")
                v = np.empty(shape, np.float32)
            if dev:
                out_ptrs.append(tensor_ptr(n, v, shape))
            else:
                if not (isinstance(v, np.ndarray) and v.dtype == np.float32 and v.flags.c_contiguous and v.size == int(np.prod(shape))):
                    raise ValueError(f"{what}: {n} must be a C-contiguous float32 array of {int(np.prod(shape))} elements")
                out_ptrs.append(_hp(v))
            res[n] = v
        return (RSB_DEVICE if dev else RSB_HOST), in_ptrs, out_ptrs, res, keep

    def terrain_height(self, points, normal=False, out=None):
        """HeightMap::getHeight (and getNormal) of every env at once: points [N, P, 2] world xy -> height [N, P], or (height, normal [N, P, 3]) with
        normal=True; coordinates outside the map are clamped to it, a ground plane gives its height and (0, 0, 1).  points a numpy array: host
        arrays back; a float32 torch CUDA tensor: out = {"height": tensor, "normal": tensor} (either one alone is enough), no synchronisation."""
        P = int(np.prod(points.shape)) // (2 * self.N)
        out = dict(out or {})
        if set(out) - {"height", "normal"}:
            raise ValueError(f"terrain_height: unknown outputs {sorted(set(out) - {'height', 'normal'})}")
        shapes = {"height": (self.N, P), "normal": (self.N, P, 3)}
        want = [n for n in shapes if n in out or (not self._is_torch(points) and (n == "height" or normal))]
        space, ins, outs, res, _keep = self._terrain_io("terrain_height", {"points": (points, (self.N, P, 2))}, {n: shapes[n] for n in want}, out)
        ptr = dict(zip(want, outs))
        check(self.L.rsb_get_terrain_height(self.handle, ins[0], P, ptr.get("height"), ptr.get("normal"), space), "rsb_get_terrain_height")
        if "normal" in res and "height" in res:
            return res["height"], res["normal"]
        return res["height"] if "height" in res else res["normal"]

    def height_scan(self, frames, pattern, yaw_aligned=True, out=None, row_stride=0):
        """Height of each frame above the terrain under a pattern of points around it: [N, F, P], out[e, f, k] = p_z - h(p_xy + M pattern[k]), p the
        frame's world position, pattern [P, 2]; yaw_aligned: M rotates the pattern about z by the frame's heading, else M = identity.  frames as in
        frame_kinematics.  row_stride (floats, 0 = F * P): with a larger value `out` is the first scan column of a wider [N, row_stride] buffer -
        a torch view such as obs[:, k:] (only its data pointer is used) or a numpy array of N * row_stride floats - whose other columns are left alone."""
        arr, F = self._frames(frames)
        P = int(np.prod(pattern.shape)) // 2
        width = F * P
        stride = int(row_stride) or width
        mode = _capi.RSB_SCAN_YAW if yaw_aligned else _capi.RSB_SCAN_WORLD
        if stride == width:
            space, ins, outs, res, _keep = self._terrain_io("height_scan", {"pattern": (pattern, (P, 2))}, {"out": (self.N, F, P)}, {"out": out})
            check(self.L.rsb_height_scan(self.handle, arr, F, ins[0], P, mode, outs[0], 0, space), "rsb_height_scan")
            return res["out"]
        if out is None or self._is_torch(out) != self._is_torch(pattern):
            raise ValueError("height_scan: a row_stride needs `out`, of the pattern's kind (torch tensor or numpy array)")
        space, ins, _, _, _keep = self._terrain_io("height_scan", {"pattern": (pattern, (P, 2))}, {}, {})
        if space == RSB_DEVICE:
            if not (out.is_cuda and str(out.dtype) == "torch.float32" and out.device.index == self.device):
                raise ValueError(f"height_scan: out must be a float32 CUDA tensor on cuda:{self.device}")
            optr = C.c_void_p(out.data_ptr())
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.size >= (self.N - 1) * stride + width):
                raise ValueError("height_scan: out must be a C-contiguous float32 array that holds N rows of row_stride floats")
            optr = _hp(out)
        check(self.L.rsb_height_scan(self.handle, arr, F, ins[0], P, mode, optr, stride, space), "rsb_height_scan")
        return out

    def ray_test(self, origins, directions, max_dist, out=None):
        """World::rayTest against the terrain for every env at once: origins, directions [N, R, 3] world frame (directions of any length) ->
        dist [N, R], metres to the first hit within max_dist, -1 for a miss (see rsb_ray_test in rsb.h for the side wall and the degenerate rays)."""
        R = int(np.prod(origins.shape)) // (3 * self.N)
        space, ins, outs, res, _keep = self._terrain_io("ray_test", {"origins": (origins, (self.N, R, 3)), "directions": (directions, (self.N, R, 3))},
                                                        {"dist": (self.N, R)}, {"dist": out})
        check(self.L.rsb_ray_test(self.handle, ins[0], ins[1], R, float(max_dist), outs[0], space), "rsb_ray_test")
        return res["dist"]

    # -- rays that also hit the robot, and ray patterns mounted on a body (rsb_ray_scan.hip) --------------------------------
    def _ray_hit_buffer(self, what, dev, given, shape, wanted):
        """the optional int32 `hit` output of ray_cast / ray_scan -> (pointer or None, array / tensor or None)"""
        if given is None and not wanted:
            return None, None
        cnt = int(np.prod(shape))
        if dev:
            if given is None:
                raise ValueError(f"{what}: with torch inputs pass hit as an int32 torch tensor (out={{'hit': ...}})")
            if not (self._is_torch(given) and given.is_cuda and given.is_contiguous() and str(given.dtype) == "torch.int32" and given.numel() == cnt
                    and given.device.index == self.device):
                raise ValueError(f"{what}: hit must be a contiguous int32 CUDA tensor of {cnt} elements on cuda:{self.device}")
            return C.c_void_p(given.data_ptr()), given
        if given is None:
            given = np.empty(shape, np.int32)
        if not (isinstance(given, np.ndarray) and given.dtype == np.int32 and given.flags.c_contiguous and given.size == cnt):
            raise ValueError(f"{what}: hit must be a C-contiguous int32 array of {cnt} elements")
        return _hp(given), given

    @staticmethod
    def _ray_flags(bodies, own_body=False, planar=False, miss_max=False):
        return ((_capi.RSB_RAY_BODIES if bodies else 0) | (_capi.RSB_RAY_OWN_BODY if own_body else 0) | (_capi.RSB_RAY_PLANAR if planar else 0)
                | (_capi.RSB_RAY_MISS_MAX if miss_max else 0))

    def ray_cast(self, origins, directions, max_dist, bodies=True, hit=False, miss_max=False, out=None):
        """World::rayTest against the terrain AND the robot for every env at once: origins, directions [N, R, 3] world frame (directions of any
        length) -> dist [N, R], metres to the first hit within max_dist, -1 for a miss (max_dist with miss_max); with hit=True (dist, hit), hit
        [N, R] int32: RSB_RAY_HIT_NONE, RSB_RAY_HIT_TERRAIN or the first collision primitive of the shape that was hit (model.blob.col_body /
        col_name of it name the link).  bodies: rays stop at the robot's collision shapes (spheres, capsules, cylinders, boxes - see rsb_ray_cast in
        rsb.h; a mesh collider is invisible); bodies=False gives ray_test's answer bit for bit.  out: the dist array / tensor, or {"dist": ..,
        "hit": ..} (either alone is enough); torch CUDA inputs need torch outputs and do not synchronise."""
        R = int(np.prod(origins.shape)) // (3 * self.N)
        outs = dict(out) if isinstance(out, dict) else ({} if out is None else {"dist": out})
        if set(outs) - {"dist", "hit"}:
            raise ValueError(f"ray_cast: unknown outputs {sorted(set(outs) - {'dist', 'hit'})}")
        dev = self._is_torch(origins)
        want_dist = "dist" in outs or not dev or "hit" not in outs
        space, ins, optrs, res, _keep = self._terrain_io("ray_cast", {"origins": (origins, (self.N, R, 3)), "directions": (directions, (self.N, R, 3))},
                                                         {"dist": (self.N, R)} if want_dist else {}, {k: v for k, v in outs.items() if k == "dist"})
        hptr, harr = self._ray_hit_buffer("ray_cast", dev, outs.get("hit"), (self.N, R), hit)
        check(self.L.rsb_ray_cast(self.handle, ins[0], ins[1], R, float(max_dist), self._ray_flags(bodies, miss_max=miss_max),
                                  optrs[0] if want_dist else None, hptr, space), "rsb_ray_cast")
        if harr is not None and want_dist:
            return res["dist"], harr
        return res["dist"] if want_dist else harr

    def ray_scan(self, frames, dirs, max_dist, bodies=True, own_body=False, planar=False, miss_max=False, hit=False, out=None, row_stride=0):
        """A depth camera or lidar mounted on a body, for every env at once: [N, F, P], out[e, f, k] = range from frame f's world point along
        R_body dirs[k], dirs [P, 3] in the axes of the frame's body (x forward, y left, z up; any length) - depth_camera_rays / lidar_rays build
        such patterns; a sensor tilted against its body rotates its pattern once, on the host.  frames as in frame_kinematics.  -1 for a miss
        (miss_max: max_dist).  bodies: rays stop at the robot's collision shapes too; own_body: also at those of the frame's own body (default: a
        sensor sees through its mount); planar: range times the cosine to the body's x axis, the depth image of a pinhole camera.  hit=True: (out,
        hit), hit [N, F, P] int32 as in ray_cast.  out: the range array / tensor, or {"out": .., "hit": ..}.  row_stride as in height_scan."""
        arr, F = self._frames(frames)
        P = int(np.prod(dirs.shape)) // 3
        width = F * P
        stride = int(row_stride) or width
        outs = dict(out) if isinstance(out, dict) else ({} if out is None else {"out": out})
        if set(outs) - {"out", "hit"}:
            raise ValueError(f"ray_scan: unknown outputs {sorted(set(outs) - {'out', 'hit'})}")
        dev = self._is_torch(dirs)
        flags = self._ray_flags(bodies, own_body, planar, miss_max)
        hptr, harr = self._ray_hit_buffer("ray_scan", dev, outs.get("hit"), (self.N, F, P), hit)
        rng = outs.get("out")
        want_out = rng is not None or not dev or harr is None
        if stride == width:
            space, ins, optrs, res, _keep = self._terrain_io("ray_scan", {"dirs": (dirs, (P, 3))}, {"out": (self.N, F, P)} if want_out else {}, {"out": rng})
            optr, rng = (optrs[0], res["out"]) if want_out else (None, None)
            stride = 0
        else:
            if rng is None or self._is_torch(rng) != dev:
                raise ValueError("ray_scan: a row_stride needs `out`, of the pattern's kind (torch tensor or numpy array)")
            space, ins, _, _, _keep = self._terrain_io("ray_scan", {"dirs": (dirs, (P, 3))}, {}, {})
            if dev:
                if not (rng.is_cuda and str(rng.dtype) == "torch.float32" and rng.device.index == self.device):
                    raise ValueError(f"ray_scan: out must be a float32 CUDA tensor on cuda:{self.device}")
                optr = C.c_void_p(rng.data_ptr())
            else:
                if not (isinstance(rng, np.ndarray) and rng.dtype == np.float32 and rng.flags.c_contiguous and rng.size >= (self.N - 1) * stride + width):
                    raise ValueError("ray_scan: out must be a C-contiguous float32 array that holds N rows of row_stride floats")
                optr = _hp(rng)
        check(self.L.rsb_ray_scan(self.handle, arr, F, ins[0], P, flags, float(max_dist), optr, stride, hptr, space), "rsb_ray_scan")
        if harr is not None and rng is not None:
            return rng, harr
        return rng if rng is not None else harr

    # -- observation block for the vectorised env / RCCL gather --------------------------------------
    def obs_dim(self, n_force_slots):
        return self.L.rsb_obs_dim(self.handle, int(n_force_slots))

    def gather_obs(self, out_device_ptr, collision_indices):
        idx = _host(collision_indices, np.int32)
        n = 0 if idx is None else idx.shape[0]
        check(self.L.rsb_gather_obs(self.handle, C.c_void_p(out_device_ptr), _hp(idx), n, RSB_DEVICE), "rsb_gather_obs")

    def reset_terminated(self, allowed_collisions, gc0, gv0):
        """Reset envs that touch the terrain with anything but `allowed_collisions` (host arrays). Returns done [N]."""
        idx = _host(allowed_collisions, np.int32)
        g0, v0 = _host(gc0, np.float32), _host(gv0, np.float32)
        rows = 1 if g0.ndim == 1 or g0.shape[0] == 1 else g0.shape[0]
        done = np.zeros(self.N, np.uint8)
        check(self.L.rsb_reset_terminated(self.handle, _hp(idx), idx.shape[0], _hp(g0), _hp(v0), rows, _hp(done), RSB_HOST),
              "rsb_reset_terminated")
        return done

    def reset_terminated_device(self, allowed_collisions, gc0_ptr, gv0_ptr, rows, done_ptr=None):
        idx = _host(allowed_collisions, np.int32)
        check(self.L.rsb_reset_terminated(self.handle, _hp(idx), idx.shape[0], C.c_void_p(gc0_ptr), C.c_void_p(gv0_ptr),
                                          int(rows), C.c_void_p(done_ptr) if done_ptr else None, RSB_DEVICE),
              "rsb_reset_terminated")

    def device_ptr(self, field):
        return self.L.rsb_device_ptr(self.handle, int(field))

    def enable_timing(self, on=True):
        """False/0: off; True/1: one event pair (last_kernel_ms); n > 1: ring of n event pairs (read_kernel_ms)."""
        check(self.L.rsb_enable_timing(self.handle, int(on)), "rsb_enable_timing")

    def set_timing_stride(self, stride):
        check(self.L.rsb_set_timing_stride(self.handle, int(stride)), "rsb_set_timing_stride")

    def read_kernel_ms(self, n):
        """Durations (ms) of the last n step-kernel launches (oldest first); synchronises the stream."""
        out = np.zeros(int(n), np.float32)
        got = self.L.rsb_read_kernel_ms(self.handle, _hp(out), int(n))
        if got < 0:
            check(got, "rsb_read_kernel_ms")
        return out[:got]

    def control_step_plan(self, n_substeps, obs_ptr, force_collisions, allowed_collisions, gc0_ptr, gv0_ptr, rows):
        """Pre-marshalled rsb_control_step call: returns f(p_target_ptr) that enqueues one control step (PD targets ->
        n_substeps x integrate -> obs gather -> reset of terminated envs) with a single foreign call."""
        fidx = _host(force_collisions, np.int32)
        aidx = _host(allowed_collisions, np.int32) if allowed_collisions is not None else None
        fn, h = self.L.rsb_control_step, self.handle
        args = (int(n_substeps), C.c_void_p(obs_ptr) if obs_ptr else None, _hp(fidx), 0 if fidx is None else fidx.shape[0],
                _hp(aidx), 0 if aidx is None else aidx.shape[0],
                C.c_void_p(gc0_ptr) if gc0_ptr else None, C.c_void_p(gv0_ptr) if gv0_ptr else None, int(rows))
        keep = (fidx, aidx)

        def step(p_target_ptr, _keep=keep):
            st = fn(h, C.c_void_p(p_target_ptr), None, *args)
            if st != 0:
                check(st, "rsb_control_step")
        return step

    # -- resident control steps (rsb_control_steps / rsb_set_step_residency: K control steps per launch, the env blocks stay in LDS) ------------
    def set_step_residency(self, on=True):
        """rsb_control_steps and the closed-loop runs with an in-repo stage use ONE resident launch per call where the world's kernel class has a
        resident twin (residency_status says whether it does)."""
        check(self.L.rsb_set_step_residency(self.handle, int(bool(on))), "rsb_set_step_residency")

    def residency_status(self, stage=0):
        """True when a resident launch exists for this world as configured now (stage 0 open loop, 1 linear policy, 2 actor network)"""
        return bool(self.L.rsb_step_residency_status(self.handle, int(stage)))

    def residency_launches(self):
        return int(self.L.rsb_step_residency_launches(self.handle))

    # -- specialised step kernels (rsb_set_specialization: the model's dimensions and the world's switches as compile-time constants) ------------
    SPEC_OFF, SPEC_CACHED, SPEC_COMPILE = 0, 1, 2

    def set_specialization(self, mode):
        """"off" / "cached" (default: use a code object found in rsb_spec_dir()) / "compile" (a miss compiles it first, ~25 s once per key)"""
        m = {"off": 0, "cached": 1, "compile": 2}.get(mode, mode)
        check(self.L.rsb_set_specialization(self.handle, int(m)), "rsb_set_specialization")

    def specialization_status(self):
        """(mode, step launches that ran a specialised code object, step launches that ran an ahead-of-time class)"""
        a, b = C.c_longlong(0), C.c_longlong(0)
        mode = self.L.rsb_specialization_status(self.handle, C.byref(a), C.byref(b))
        return int(mode), int(a.value), int(b.value)

    def debug_resident_full_writes(self, on=True):
        check(self.L.rsb_debug_resident_full_writes(self.handle, int(bool(on))), "rsb_debug_resident_full_writes")

    def control_steps_plan(self, n_substeps, targets_ptr, period, obs_ptr, obs_step_stride, force_collisions, allowed_collisions, gc0_ptr, gv0_ptr, rows,
                           done_ptr=0, done_step_stride=0):
        """Pre-marshalled rsb_control_steps call: returns f(n_steps, first) that enqueues n_steps control steps of the open loop reading the PD-target
        slices (first + j) % period of the device bank at targets_ptr ([period, N, nq]); one resident launch with set_step_residency(True)."""
        fidx = _host(force_collisions, np.int32)
        aidx = _host(allowed_collisions, np.int32) if allowed_collisions is not None else None
        fn, h = self.L.rsb_control_steps, self.handle
        head = (C.c_void_p(targets_ptr), int(period))
        tail = (int(n_substeps), C.c_void_p(obs_ptr) if obs_ptr else None, int(obs_step_stride), _hp(fidx), 0 if fidx is None else fidx.shape[0],
                _hp(aidx), 0 if aidx is None else aidx.shape[0],
                C.c_void_p(gc0_ptr) if gc0_ptr else None, C.c_void_p(gv0_ptr) if gv0_ptr else None, int(rows),
                C.c_void_p(done_ptr) if done_ptr else None, int(done_step_stride))
        keep = (fidx, aidx)

        def steps(n_steps, first, _keep=keep):
            st = fn(h, int(n_steps), *head, int(first), *tail)
            if st != 0:
                check(st, "rsb_control_steps")
        return steps

    # -- peer-mapped obs exchange (rsb_obs_peer_*: no collective, no copy kernel; see include/rsb.h) ------------
    OBS_HANDLE_BYTES = 64

    def obs_peer_create(self, n_ranks, rank, force_collisions):
        """Allocates this rank's gathered buffer; returns its IPC handle (64 bytes; zeros when the system has no hipIpc)."""
        fidx = _host(force_collisions, np.int32)
        buf = C.create_string_buffer(self.OBS_HANDLE_BYTES)
        check(self.L.rsb_obs_peer_create(self.handle, int(n_ranks), int(rank), _hp(fidx), 0 if fidx is None else fidx.shape[0], buf),
              "rsb_obs_peer_create")
        return buf.raw

    def obs_peer_connect(self, handles):
        """handles: the n_ranks IPC handles in rank order (bytes of n_ranks * 64), e.g. from dist.all_gather_object."""
        check(self.L.rsb_obs_peer_connect(self.handle, bytes(handles)), "rsb_obs_peer_connect")

    def obs_peer_connect_ptrs(self, bases):
        """Within one process: base pointers (obs_peer_base()) of all ranks' worlds in rank order (own entry ignored)."""
        arr = (C.c_void_p * len(bases))(*[C.c_void_p(b) for b in bases])
        check(self.L.rsb_obs_peer_connect_ptrs(self.handle, arr), "rsb_obs_peer_connect_ptrs")

    def obs_peer_base(self):
        return self.L.rsb_obs_peer_base(self.handle)

    def obs_peer_wait(self):
        """Stream-side wait for every rank's rows of the last control step issued; returns the gathered block's device pointer."""
        out = C.c_void_p()
        check(self.L.rsb_obs_peer_wait(self.handle, C.byref(out)), "rsb_obs_peer_wait")
        return out.value

    def obs_peer_destroy(self):
        check(self.L.rsb_obs_peer_destroy(self.handle), "rsb_obs_peer_destroy")

    def last_kernel_ms(self):
        ms = C.c_float()
        check(self.L.rsb_last_kernel_ms(self.handle, C.byref(ms)), "rsb_last_kernel_ms")
        return ms.value

    # -- debug aid: one env's contact problem (G, c, lam) of the last sub-step -----------------------
    def debug_select_env(self, env):
        check(self.L.rsb_debug_select_env(self.handle, int(env)), "rsb_debug_select_env")

    def debug_contact_problem(self):
        K = RSB_MAX_CONTACTS
        G = np.zeros(9 * K * K, np.float32)
        c = np.zeros(3 * K, np.float32)
        lam = np.zeros(3 * K, np.float32)
        nc = C.c_int()
        check(self.L.rsb_debug_read_contact_problem(self.handle, C.byref(nc), _hp(G), _hp(c), _hp(lam)),
              "rsb_debug_read_contact_problem")
        n3 = 3 * nc.value
        return nc.value, G[:n3 * n3].reshape(n3, n3).copy(), c[:n3].copy(), lam[:n3].copy()

    def debug_phase_cycles(self, enable=True, read=True):
        out = np.zeros(16, np.int64)
        check(self.L.rsb_debug_phase_cycles(self.handle, 1 if enable else 0, _hp(out) if read else None),
              "rsb_debug_phase_cycles")
        return out

    def debug_wave_profile(self):
        nb = (self.N * self.lanes_per_env() + 63) // 64
        out = np.zeros((nb, 16), np.int64)
        check(self.L.rsb_debug_wave_profile(self.handle, _hp(out), nb), "rsb_debug_wave_profile")
        return out

    def debug_wave_sweep_control(self):
        """[waves, 12] of the last launch: Newton blocks of first sweeps; rare-path test fired, first | later sweeps; energy check ran, first | later; basin check, quad |
        serial form; followed by a global search, first | later; none of the three, first | later; blocks that refused a lane's step"""
        nb = (self.N * self.lanes_per_env() + 63) // 64
        out = np.zeros((nb, 12), np.int64)
        check(self.L.rsb_debug_wave_sweep_control(self.handle, _hp(out), nb), "rsb_debug_wave_sweep_control")
        return out
