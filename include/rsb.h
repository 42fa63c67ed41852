/*
 * rsb.h — C-ABI of the MI355X-native batched rigid-body simulator ("rsb" = RaiSim-batched).
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json's north_star:
 * thousands of independent raisim::World replicas, each holding one raisim::ArticulatedSystem
 * on a Ground / HeightMap, stepped in lock-step on one GPU.
 *
 * Reference interface replaced.  The mounted reference /root/reference is a
 * three-file stub (.gitignore:1-12, .travis.yml:1-12, README.md:1) that contains NO headers, so
 * every "replaces" note below names the upstream raisimLib symbol from recollection [RECALL] and
 * the file the symbol would live in; the file:line is "absent" for all of them
 * (SURVEY.md §0, §8a).
 *
 *   rsb_create / rsb_destroy            <- raisim::World::World(), ~World(),
 *                                          World::addArticulatedSystem(urdf)      (World.hpp, absent)
 *   rsb_set_ground / rsb_set_heightmap  <- World::addGround(z), World::addHeightMap(...)
 *   rsb_set_timestep / rsb_set_gravity  <- World::setTimeStep, World::setGravity
 *   rsb_set_erp / rsb_set_contact_solver_param / rsb_set_friction
 *                                       <- World::setERP, World::setContactSolverParam,
 *                                          World::setDefaultMaterial               (World.hpp, absent)
 *   rsb_set_state / rsb_get_state       <- ArticulatedSystem::setState/getState    (ArticulatedSystem.hpp, absent)
 *   rsb_set_pd_gains / rsb_set_pd_target / rsb_set_generalized_force / rsb_set_control_mode
 *                                       <- ArticulatedSystem::setPdGains/setPdTarget/
 *                                          setGeneralizedForce/setControlMode
 *   rsb_integrate / rsb_integrate1 / rsb_integrate2
 *                                       <- World::integrate(), integrate1(), integrate2()
 *   rsb_get_contacts                    <- ArticulatedSystem::getContacts() (contact/Contact.hpp, absent)
 *   rsb_get_mass_matrix / rsb_get_nonlinearities
 *                                       <- ArticulatedSystem::getMassMatrix()/getNonlinearities()
 *   rsb_get_frame_kinematics / rsb_get_frame_jacobians / rsb_add_external_wrench
 *                                       <- ArticulatedSystem::getFramePosition/getFrameOrientation/getFrameVelocity/
 *                                          getFrameAngularVelocity/getDenseFrameJacobian/getDenseFrameRotationalJacobian/
 *                                          setExternalForce/setExternalTorque, for all envs in one call
 *   rsb_get_frame_accelerations / rsb_get_frame_jacobian_rates / rsb_imu_observe
 *                                       <- ArticulatedSystem::getFrameAcceleration / getTimeDerivativeOfSparseJacobian /
 *                                          getTimeDerivativeOfSparseRotationalJacobian, and (new) the accelerometer + gyro rows of an
 *                                          observation, for all envs in one call
 *   rsb_inverse_dynamics / rsb_forward_dynamics
 *                                       <- ArticulatedSystem::setComputeInverseDynamics / getForceAtJointInWorldFrame /
 *                                          getTorqueAtJointInWorldFrame, and the plain equations of motion, for all envs in one call
 *   rsb_inverse_dynamics_derivatives / rsb_forward_dynamics_derivatives
 *                                       <- (new) the analytic derivatives of the two with respect to configuration, velocity and
 *                                          acceleration / force, for all envs in one call
 *   rsb_apply_inverse_mass / rsb_get_frame_delassus
 *                                       <- (new) M^-1 B and the operational-space matrices J M^-1, J M^-1 J^T at chosen frames, for all
 *                                          envs in one call, without the dense getInverseMassMatrix()
 *   rsb_constrained_forward_dynamics / rsb_frame_impulse
 *                                       <- (new) forward dynamics with chosen frames held and the impulse that stops them, with the
 *                                          constraint forces and a per-env status, for all envs in one call
 *   rsb_inverse_kinematics              <- (new) the configuration that puts chosen frames at chosen places: a damped Gauss-Newton
 *                                          iteration per env with a per-env status, for all envs in one call
 *   rsb_get_terrain_height / rsb_height_scan / rsb_ray_test
 *                                       <- HeightMap::getHeight / getNormal, World::rayTest (against the terrain), for all envs
 *                                          in one call                                (HeightMap.hpp, World.hpp, absent)
 *   rsb_ray_cast / rsb_ray_scan         <- World::rayTest against the terrain AND the robot's collision bodies, and (new) its fused
 *                                          sensor form: a depth camera or lidar mounted on a body, for all envs in one call
 *   rsb_get_body_contact_wrenches / rsb_contact_observe / rsb_contact_timers <- the host loop over ArticulatedSystem::getContacts(), for all envs in one call
 *   rsb_gather_obs                      <- (new) the (q, u, contact-force) observation block that
 *                                          VectorizedEnvironment::observe() is built from
 *   rsb_env_observe_normalized / rsb_env_get_obs_stats / rsb_env_set_obs_stats
 *                                       <- VectorizedEnvironment::observe(ob, updateStatistics),
 *                                          getObStatistics/setObStatistics (raisimGymTorch, absent)
 *
 * Conventions
 *   - No exceptions cross this ABI. Every call returns RSB_OK (0) or a negative rsb_status;
 *     rsb_last_error() returns a thread-local message for the last failure.
 *   - Buffers are caller-owned.  `space` says whether a pointer is host or device memory.
 *   - Batched arrays are row-major [num_envs, dim] float32 (the layout raisimGymTorch's
 *     VectorizedEnvironment uses for observation/action matrices).
 *   - Generalized coordinates follow RaiSim: gc = [x y z  qw qx qy qz  joints...] (nq = 7+nj),
 *     gv = [world linear vel (3), world angular vel (3), joint vels...] (nv = 6+nj).
 *   - One handle owns one HIP stream (or borrows the caller's, rsb_set_stream). A handle is not
 *     re-entrant; distinct handles may be used from distinct threads.
 *   - There is NO CPU fallback: rsb_create fails with RSB_E_NO_DEVICE when no HIP device exists.
 */
#ifndef RSB_H_
#define RSB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#include "rsb_types.h"   /* constants, enums, rsb_model_blob, rsb_contact, rsb_field: what the device code shares with this header */

typedef struct rsb_model rsb_model;  /* host-side parsed model           */
typedef struct rsb_world rsb_world;  /* batched device world             */

const char* rsb_last_error(void);
const char* rsb_version(void);
/* build provenance: hash of the sources (the files of raisimlib_amd/csrc, this header, compiler flags) the loaded library was built from,
 * as raisimlib_amd/build.py: source_hash() computes it for the tree (the test-suite refuses a library that does not match its tree) */
const char* rsb_source_hash(void);

/* ---- model (host only; cold path) -------------------------------------- */
int rsb_model_from_urdf_file(const char* path, rsb_model** out);
int rsb_model_from_urdf_string(const char* xml, rsb_model** out);
/* Sampled colliders (no upstream counterpart; opt-in).  The loader turns a capsule into its two end spheres and a box into its eight
 * corners: the exact contact sets on a plane.  With sample_spacing h > 0 a capsule also gets spheres of its radius along its axis and
 * a box zero-radius points on the lattice of its edges and faces, no further apart than h, so that a height-field feature under the
 * MIDDLE of a capsule or of a box face, and a capsule touching another link with its middle, are found to within h by the same sphere
 * tests (the narrow phase of the kernel is unchanged).  Costs primitives (at most RSB_MAX_COLLISIONS per model) and adds redundant
 * contacts where the unsampled set was already exact.  h = 0: the functions above. */
int rsb_model_from_urdf_file_sampled(const char* path, double sample_spacing, rsb_model** out);
int rsb_model_from_urdf_string_sampled(const char* xml, double sample_spacing, rsb_model** out);
/* <mesh> colliders (upstream: the mesh itself against the terrain, through ODE's trimesh collider [RECALL; absent]) are loaded as a POINT SET: support
 * vertices of the mesh's convex hull, each a zero-radius primitive - exact against a plane for a convex mesh whose lowest vertices are among them.
 * n = points kept per mesh: default 8 (the body diagonals' support vertices: a box keeps its corners), at most 26 (+ the 6 axes' and the 12 face
 * diagonals'); they count against RSB_MAX_COLLISIONS.  Process-wide, read when a URDF is loaded. */
int rsb_set_mesh_point_budget(int n);
int rsb_model_from_blob(const rsb_model_blob* blob, rsb_model** out);
int rsb_model_destroy(rsb_model* m);
int rsb_model_get_blob(const rsb_model* m, rsb_model_blob* out);
int rsb_model_body_index(const rsb_model* m, const char* link_name);   /* <0 if absent */
int rsb_model_joint_index(const rsb_model* m, const char* joint_name); /* body index driven by joint */
double rsb_model_total_mass(const rsb_model* m);
int rsb_model_skipped_collisions(const rsb_model* m);   /* <collision> elements the loader could not turn into primitives (unreadable meshes, unknown geometry) */
const char* rsb_model_collision_material(const rsb_model* m, int collision);   /* material name of a collision primitive ("default" if the URDF names none) */

/* ---- world ------------------------------------------------------------------------------ */
int rsb_device_count(void);
int rsb_create(const rsb_model* m, int num_envs, int device, rsb_world** out);
int rsb_destroy(rsb_world* w);
int rsb_set_stream(rsb_world* w, void* hip_stream);   /* borrow the caller's hipStream_t (NULL = HIP default stream) */
void* rsb_get_stream(rsb_world* w);
int rsb_synchronize(rsb_world* w);

int rsb_num_envs(const rsb_world* w);
int rsb_dims(const rsb_world* w, int* nb, int* nq, int* nv, int* ncol, int* kmax);

int rsb_set_timestep(rsb_world* w, double dt);
double rsb_get_timestep(const rsb_world* w);
double rsb_get_world_time(const rsb_world* w);
int rsb_set_gravity(rsb_world* w, const double g[3]);
int rsb_set_erp(rsb_world* w, double erp);
int rsb_set_friction(rsb_world* w, double mu);
/* World::setDefaultMaterial(friction, restitution, resThreshold) [RECALL]: one material per world; a contact approaching
 * faster than res_threshold (m/s) leaves with v_n+ = -restitution * v_n- (Newton restitution), slower ones are inelastic */
int rsb_set_material(rsb_world* w, double mu, double restitution, double res_threshold);
/* World::setMaterialPairProp(material1, material2, friction, restitution, resThreshold) [RECALL; upstream Materials.hpp is
 * absent from /root/reference]: every env holds ONE terrain object, so the pair table collapses to one (mu, restitution,
 * res_threshold) triple per collision primitive of the robot = the pair (primitive's material, terrain's material).
 * Arrays of rsb_dims().ncol doubles; a NULL array (or a negative entry) means "the world's default" (rsb_set_material).
 * The C++ facade resolves material NAMES (rsb_model_collision_material, addGround(z, material)) into these arrays. */
int rsb_set_collision_materials(rsb_world* w, const double* mu, const double* restitution, const double* res_threshold);
/* Self-collision: RaiSim collides the links of one articulated system with each other, parent-child pairs excepted [RECALL;
 * upstream ArticulatedSystem.hpp is absent from /root/reference].  Here: sphere x sphere between collision primitives of two
 * bodies that are not parent and child (capsule = its two end spheres, box = its corner points against spheres; rim
 * primitives of cylinders take no part).  On by default; a self-collision takes two of the max_contacts slots.
 * rsb_ignore_collision_between = ArticulatedSystem::ignoreCollisionBetween(bodyIdx1, bodyIdx2) (not undoable).
 * rsb_self_collision_pairs lists the candidate primitive pairs (pairs[2k] < pairs[2k+1]) and returns their count;
 * rsb_set_self_collision_materials takes one (mu, restitution, res_threshold) per candidate pair in that order
 * (NULL array / negative entry = the world's default; reset when the candidate list changes). */
int rsb_set_self_collision(rsb_world* w, int enable);
int rsb_ignore_collision_between(rsb_world* w, int body_a, int body_b);
int rsb_self_collision_pairs(const rsb_world* w, int32_t* pairs, int capacity);
int rsb_set_self_collision_materials(rsb_world* w, const double* mu, const double* restitution, const double* res_threshold);
int rsb_set_contact_solver_param(rsb_world* w, double alpha_init, double alpha_min,
                                 double alpha_decay, int max_iter, double threshold);
/* ArticulatedSystem::setIntegrationScheme [RECALL; upstream file absent].  The velocity update is the same for every scheme (one
 * dynamics evaluation, one contact solve: u+ = u + M^-1 (dt tau + J^T lambda)); the scheme picks the velocity the positions move with:
 *   RSB_INTEGRATION_SEMI_IMPLICIT (default, RaiSim's)  q+ = q (+) dt u+
 *   RSB_INTEGRATION_EULER                               q+ = q (+) dt u
 *   RSB_INTEGRATION_TRAPEZOID                           q+ = q (+) dt (u + u+) / 2     (exact positions under a constant acceleration)
 *   RSB_INTEGRATION_RUNGE_KUTTA_4                       the classical four-stage scheme on the smooth equations of motion (explicit PD at the stage
 *                                                       states, the base orientation advanced on SO(3)), contacts and joint limits on top of it as in the
 *                                                       other schemes: one detection at q, one solve (rsb_rk4.hip states the construction).  Host-driven
 *                                                       over the query kernels - four dynamics evaluations with a dense M^-1 per integrate(): the slow,
 *                                                       accurate path; plain rsb_integrate / rsb_integrate_masked / World-view calls only
 *                                                       (RSB_E_UNSUPPORTED from rsb_control_step / rsb_env_step)
 * (the enum values are raisim::IntegrationScheme's [RECALL]).  EULER and TRAPEZOID run in a kernel class of their own (floating-base systems
 * of tree depth <= 13, no peer-mapped obs exchange, one contact per primitive; RSB_E_UNSUPPORTED from the step otherwise): the default's
 * kernels do not carry the choice. */
#define RSB_INTEGRATION_TRAPEZOID 0
#define RSB_INTEGRATION_SEMI_IMPLICIT 1
#define RSB_INTEGRATION_EULER 2
#define RSB_INTEGRATION_RUNGE_KUTTA_4 3
int rsb_set_integration_scheme(rsb_world* w, int scheme);
int rsb_set_max_contacts(rsb_world* w, int kmax);   /* 1..RSB_MAX_CONTACTS */

int rsb_set_ground(rsb_world* w, double height);
/* heights: host pointer, row-major [y_samples][x_samples] (x fastest), shared by all envs.
 * Beyond the footprint the terrain is the surface the queries below name: the height at the coordinates clamped to the footprint, level across
 * the border.  The collider follows it: a primitive whose centre is outside the footprint gets depth = r - (z - h(clamped x, clamped y)) and
 * normal (0, 0, 1); a centre inside it (the border included) touches the closest feature of the triangulated surface, which ends at the border. */
int rsb_set_heightmap(rsb_world* w, int x_samples, int y_samples, double x_size, double y_size,
                      double center_x, double center_y, const float* heights);
/* terrain curricula: n_maps height maps of one geometry, heights [n_maps][y_samples][x_samples] (host), and the map
 * each env stands on, env_map [num_envs] (host; may be NULL when n_maps == 1) */
int rsb_set_heightmaps(rsb_world* w, int n_maps, int x_samples, int y_samples, double x_size, double y_size,
                       double center_x, double center_y, const float* heights, const int32_t* env_map);

/* ---- height-map sources (host side, no GPU needed): fill a [y_samples][x_samples] float buffer for rsb_set_heightmap.
 * Upstream counterparts [RECALL, absent]: World::addHeightMap(pngFile, centerX, centerY, xSize, ySize, heightScale,
 * heightOffset), World::addHeightMap(centerX, centerY, TerrainProperties&), World::addHeightMap(textFile, ...).
 * PNG: non-interlaced 8/16-bit grey / grey+alpha / RGB / RGBA (first channel); height = pixel / max_pixel *
 * height_scale + height_offset; image row r, column c -> sample (y = r, x = c).
 * Perlin: fractal sum of improved Perlin noise (this repo's own permutation from `seed`: terrains are reproducible
 * here, not bit-identical to RaiSim's), h = z_scale * sum_o gain^o * noise(f lacunarity^o * (x, y)), optionally
 * rounded to multiples of step_size, + height_offset.
 * Text: "xSamples ySamples xSize ySize" followed by xSamples*ySamples heights (x fastest). */
typedef struct rsb_terrain_properties {   /* field meaning of raisim::TerrainProperties [RECALL] */
  double frequency, z_scale, x_size, y_size;
  int32_t x_samples, y_samples, fractal_octaves;
  uint32_t seed;
  double fractal_lacunarity, fractal_gain, step_size, height_offset;
} rsb_terrain_properties;
int rsb_heightmap_png_size(const char* path, int* x_samples, int* y_samples);
int rsb_heightmap_png_read(const char* path, double height_scale, double height_offset, float* heights, int n);
int rsb_heightmap_perlin(const rsb_terrain_properties* tp, float* heights);
int rsb_heightmap_text_size(const char* path, int* x_samples, int* y_samples, double* x_size, double* y_size);
int rsb_heightmap_text_read(const char* path, float* heights, int n);

/* mask: optional uint8 [num_envs] (same memspace); envs with mask==0 are left untouched */
int rsb_set_state(rsb_world* w, const float* gc, const float* gv, const uint8_t* mask, int space);
int rsb_get_state(rsb_world* w, float* gc, float* gv, int space);

/* one env's row of a state field (slow path behind the per-env raisim::ArticulatedSystem views):
 * field = RSB_F_GC / RSB_F_GV / RSB_F_PTARGET / RSB_F_DTARGET / RSB_F_TAU_FF; data is a host pointer of dim floats */
int rsb_set_env_row(rsb_world* w, int field, int env, const float* data);
int rsb_get_env_row(rsb_world* w, int field, int env, float* data);

/* a whole state field at once: field = RSB_F_GC / RSB_F_GV / RSB_F_PTARGET / RSB_F_DTARGET / RSB_F_TAU_FF, out [N, dim] float32 */
int rsb_get_field(rsb_world* w, int field, float* out, int space);
/* ArticulatedSystem::getGeneralizedForce() [RECALL; upstream ArticulatedSystem.hpp is absent from /root/reference]: the generalized
 * force the actuators applied in the last sub-step of the last integrate() - clipped PD + feed-forward on the joints (without the
 * joints' passive damping), the feed-forward wrench on the base rows.  Off by default (one more [N, nv] row written per launch);
 * once enabled it is read as field RSB_F_GENERALIZED_FORCE with rsb_get_field / rsb_get_env_row. */
int rsb_enable_generalized_force_output(rsb_world* w, int on);

int rsb_set_control_mode(rsb_world* w, int mode);
int rsb_set_pd_gains(rsb_world* w, const float* kp, const float* kd);      /* host, [nv] each  */
int rsb_set_pd_target(rsb_world* w, const float* p_target, const float* d_target, int space); /* [N,nq],[N,nv]; either may be NULL */
int rsb_set_generalized_force(rsb_world* w, const float* tau, int space);  /* [N,nv] feed-forward */

int rsb_integrate(rsb_world* w, int n_substeps);
int rsb_integrate1(rsb_world* w);
int rsb_integrate2(rsb_world* w);
/* World::integrate() of a SUBSET of the replicas: envs whose mask byte is 0 are not integrated and none of their rows
 * (state, contacts, flags, warm state) is touched.  mask: uint8 [num_envs] in `space` (a host mask is staged to the
 * device first).  This is what the per-env raisim::World views (include/raisim/World.hpp) flush through, so that N
 * views calling integrate() cost one launch in which every env advances exactly once. */
int rsb_integrate_masked(rsb_world* w, int n_substeps, const uint8_t* mask, int space);

/* One flush of the per-env raisim::World views (include/raisim/World.hpp) in ONE call and ONE stream synchronisation:
 * staged uploads -> launch -> the downloads the environments read.  What upstream's VectorizedEnvironment<ENV>::step pays per
 * World::integrate() is nothing (its worlds live on the host); here every crossing of PCIe costs a latency, so the facade
 * bundles them: round 3 paid up to five synchronous copies per integrate().  All pointers are HOST pointers (page-locked memory
 * from rsb_host_alloc makes the copies asynchronous up to the final synchronisation); a NULL pointer skips that transfer.
 *   uploads   p_target [N,nq], d_target [N,nv], tau_ff [N,nv]; gc / gv [N,nq] / [N,nv] with state_mask [N] (rows with mask 0 stay,
 *             rows with mask 1 are overwritten and their solver warm state cleared: rsb_set_state's semantics)
 *   launches  n_launches entries: launch_substeps[i] sub-steps for the envs whose launch_masks[i * N + env] != 0
 *             (launch_masks NULL = every env in every launch)
 *   downloads gc_out, gv_out, contact_counts [N], contacts [N,kmax], generalized_force [N,nv] (needs
 *             rsb_enable_generalized_force_output) */
typedef struct rsb_view_io {
  const float* p_target; const float* d_target; const float* tau_ff;
  const float* gc; const float* gv; const uint8_t* state_mask;
  int32_t n_launches;
  const int32_t* launch_substeps;
  const uint8_t* launch_masks;
  float* gc_out; float* gv_out;
  int32_t* contact_counts; rsb_contact* contacts;
  float* generalized_force;
} rsb_view_io;
int rsb_view_exchange(rsb_world* w, const rsb_view_io* io);
/* page-locked host memory for the buffers of rsb_view_exchange (and any other RSB_HOST argument) */
int rsb_host_alloc(size_t bytes, void** out);
int rsb_host_free(void* p);
/* device memory for a C / C++ caller that does not link the HIP runtime itself (a policy's weights for rsb_closed_loop_run_linear, action
 * buffers for RSB_DEVICE arguments): allocation on the world's device, synchronous copies (kind: 0 = host -> device, 1 = device -> host),
 * ordered behind everything the world has enqueued (they join a step pipeline like every other call) */
int rsb_device_alloc(rsb_world* w, size_t bytes, void** out);
int rsb_device_free(rsb_world* w, void* p);
int rsb_device_copy(rsb_world* w, void* dst, const void* src, size_t bytes, int kind);

/* contacts of the last sub-step: counts [N] int32, contacts [N,kmax] rsb_contact */
int rsb_get_contacts(rsb_world* w, int32_t* counts, rsb_contact* contacts, int space);
/* valid after rsb_integrate1: M [N,nv,nv], h [N,nv] */
int rsb_get_mass_matrix(rsb_world* w, float* M, int space);
int rsb_get_nonlinearities(rsb_world* w, float* h, int space);
/* ArticulatedSystem::getInverseMassMatrix() [RECALL]: M(q)^-1 [N, nv, nv] of the state rsb_integrate1 saw (slow path).
 * Fixed-base models: the inverse of the joint block M[6:, 6:] in the rows and columns 6.., zeros in the six base rows and columns
 * (a base of infinite inertia - the system every integration scheme steps), not the joint block of the floating-base matrix's inverse. */
int rsb_get_inverse_mass_matrix(rsb_world* w, float* Minv, int space);
/* per-env status flags of the last launch (bit0: contact overflow, bit1: non-finite state, bit2: the contact
 * solver of the last sub-step stopped without meeting the convergence test: max_iter or stagnation exit) */
int rsb_get_flags(rsb_world* w, int32_t* flags, int space);
/* iterations the contact solver used in the last sub-step, [N] int32 */
int rsb_get_solver_iterations(rsb_world* w, int32_t* iters, int space);

/* Frame kinematics of ALL envs in one call, from the resident state [RECALL upstream's per-object ArticulatedSystem::getFramePosition /
 * getFrameOrientation / getFrameVelocity / getFrameAngularVelocity / getPosition(body, pointB) / getVelocity(body, pointB)]: HIP kernels on the
 * world's stream (ordered with lock-step, pipelined and resident steps); the RSB_DEVICE forms do not synchronise, the RSB_HOST forms stage through
 * a device buffer the world owns.  frames: HOST array of n_frames (1..RSB_MAX_FRAMES) rsb_frame, passed to the kernel by value - no upload, no
 * registered state.  Outputs in `space`, any may be NULL (not all), row-major float32:
 *   pos [N,F,3] world; rot [N,F,9] row-major world<-body (what getFrameOrientation returns);
 *   lin_vel [N,F,3] world velocity of the point; ang_vel [N,F,3] world angular velocity of the body.
 * The base quaternion is normalised first, as the step kernel does.  Fixed-base model: the base does not move, whatever the base entries of gv hold. */
int rsb_get_frame_kinematics(rsb_world* w, const rsb_frame* frames, int n_frames,
                             float* pos, float* rot, float* lin_vel, float* ang_vel, int space);
/* getDenseFrameJacobian / getDenseFrameRotationalJacobian of all envs: J_lin, J_rot [N,F,3,nv] (either may be NULL): lin_vel = J_lin gv,
 * ang_vel = J_rot gv, gv in this ABI's order (base linear, base angular, joints).  Fixed-base model: nv columns as everywhere in this ABI,
 * the six base columns zero. */
int rsb_get_frame_jacobians(rsb_world* w, const rsb_frame* frames, int n_frames, float* J_lin, float* J_rot, int space);
/* setExternalForce / setExternalTorque of all envs: tau_ff[e] += J_lin(e)^T force[e] + J_rot(e)^T torque[e] for every env with mask[e] != 0
 * (mask NULL: all), J at the CURRENT state; force / torque [N,3] world frame and mask uint8 [N] in `space`, force or torque may be NULL (not both).
 * It stays in RSB_F_TAU_FF until rsb_set_generalized_force replaces it (upstream clears external forces after every integrate()). */
int rsb_add_external_wrench(rsb_world* w, const rsb_frame* frame, const float* force, const float* torque,
                            const uint8_t* mask, int space);

/* Frame accelerations, Jacobian rates and IMU readings of ALL envs in one call, from the resident state [RECALL upstream's per-object
 * ArticulatedSystem::getFrameAcceleration / getTimeDerivativeOfSparseJacobian / getTimeDerivativeOfSparseRotationalJacobian]: HIP kernels on the
 * world's stream, like the frame queries above (a pipelined world is joined first); the RSB_DEVICE forms do not synchronise, the RSB_HOST forms stage
 * through the same device buffer.  frames as in rsb_get_frame_kinematics (a HOST array).  The base quaternion is normalised first.  None of the three
 * changes a bit of the world: state, warm state, contact records, what rsb_integrate1 left and the feed-forward rows stay as they are.  An error
 * touches no output.  Fixed-base model: the base neither moves nor accelerates - no bit of the base rows of gv / udot matters.
 *
 * udot [N,nv] in `space` is the component-wise time derivative of gv, the convention of rsb_inverse_dynamics: udot[0:3] is the classical
 * acceleration of the base origin (d/dt of its world velocity), udot[3:6] the world angular acceleration of the base.  NULL = zeros.
 *
 * rsb_get_frame_accelerations: with (R, omega_i, alpha_i) of the frame's body i, ac_i the classical acceleration of its origin and o = R offset,
 *   lin_acc [N,F,3] = J_lin udot + Jdot_lin gv = ac_i + alpha_i x o + omega_i x (omega_i x o), d/dt of lin_vel of rsb_get_frame_kinematics;
 *   ang_acc [N,F,3] = J_rot udot + Jdot_rot gv = alpha_i;                         either may be NULL, not both.
 * With udot NULL these are the bias terms Jdot_lin gv, Jdot_rot gv.  World frame; flags: RSB_ACC_LOCAL - both outputs multiplied by R^T (the axes of
 * the frame's body, R = rot of rsb_get_frame_kinematics); RSB_ACC_PROPER - lin_acc minus the world's gravity vector (rsb_set_gravity): the specific
 * force at the point, what an accelerometer there reads.  Unknown flag bits: RSB_E_INVALID.
 *
 * rsb_get_frame_jacobian_rates: Jdot_lin, Jdot_rot [N,F,3,nv] (either may be NULL), d/dt of the matrices of rsb_get_frame_jacobians along the
 * resident gv: lin_acc = J_lin udot + Jdot_lin gv and ang_acc = J_rot udot + Jdot_rot gv for every udot.  Columns in this ABI's order; fixed-base
 * model: the six base columns zero.
 *
 * rsb_imu_observe: the fused IMU rows of an observation.  For env e and frame f
 *   out[e * row_stride + 6 f + 0..2] = R^T (lin_acc - g)   (accelerometer: RSB_ACC_LOCAL | RSB_ACC_PROPER of the call above, the same bits)
 *   out[e * row_stride + 6 f + 3..5] = R^T omega           (gyro)
 * row_stride, in floats: 0 = 6 F (a dense [N,F,6] output); larger values write into columns [0, 6 F) of rows of that pitch - pass a pointer into a
 * wider observation tensor - and touch no other float, as rsb_height_scan does; smaller non-zero values are RSB_E_INVALID.
 * RSB_E_INVALID, with a message: a null world; a bad `space`; every output NULL; n_frames outside 1..RSB_MAX_FRAMES, a frame whose body is out of
 * range or whose offset is not finite; unknown flag bits; a bad row_stride. */
#define RSB_ACC_LOCAL  1   /* outputs in the axes of the frame's body: R^T x, R = rot of rsb_get_frame_kinematics */
#define RSB_ACC_PROPER 2   /* lin_acc minus the world's gravity vector (rsb_set_gravity): the specific force at the point */
int rsb_get_frame_accelerations(rsb_world* w, const rsb_frame* frames, int n_frames,
                                const float* udot,    /* [N,nv] in `space`; NULL = zeros: the outputs are then the bias terms Jdot_lin gv, Jdot_rot gv */
                                int flags,
                                float* lin_acc,       /* [N,F,3] */
                                float* ang_acc,       /* [N,F,3]  either may be NULL, not both */
                                int space);
int rsb_get_frame_jacobian_rates(rsb_world* w, const rsb_frame* frames, int n_frames,
                                 float* Jdot_lin, float* Jdot_rot,   /* [N,F,3,nv], either may be NULL, not both */
                                 int space);
int rsb_imu_observe(rsb_world* w, const rsb_frame* frames, int n_frames, const float* udot,
                    float* out, long long row_stride, int space);

/* Whole-body quantities of ALL envs in one call, from the resident state [RECALL upstream's per-object ArticulatedSystem::getCOM / getLinearMomentum /
 * getAngularMomentum / getKineticEnergy / getPotentialEnergy / getEnergy]: HIP kernels on the world's stream, like the frame queries above (ordered with
 * lock-step, pipelined and resident steps; a pipelined world is joined first); the RSB_DEVICE form does not synchronise, the RSB_HOST form stages through
 * the same device buffer.  Outputs in `space`, any may be NULL (not all), float32.  The base quaternion is normalised first.  Every body of the blob
 * contributes its mass.  Fixed-base model: the base does not move, whatever the base entries of gv hold.  A model whose total mass is not positive:
 * RSB_E_UNSUPPORTED.  An error touches no output. */
int rsb_get_centroidal(rsb_world* w,
                       float* com,        /* [N,3] world position of the centre of mass                         */
                       float* com_vel,    /* [N,3] = lin_mom / total mass                                       */
                       float* lin_mom,    /* [N,3] sum m_i v_ci                                                 */
                       float* ang_mom,    /* [N,3] about the CENTRE OF MASS (L_p = L_c + (c - p) x P elsewhere) */
                       float* kinetic,    /* [N] incl. 0.5 * armature_i * qd_i^2                                */
                       float* potential,  /* [N] = - total mass * g . com, g = rsb_set_gravity's vector          */
                       int space);
/* centroidal momentum matrix A [N,6,nv]: (lin_mom, ang_mom about the COM) = A gv, gv in this ABI's order (base linear, base angular, joints); rows 0-2
 * linear, rows 3-5 angular.  A[:,3:6,3:6] is the composite inertia about the COM in the world frame, A[:,0:3,:] / total mass the COM Jacobian.
 * Fixed-base model: the six base columns are zero. */
int rsb_get_centroidal_momentum_matrix(rsb_world* w, float* A, int space);

/* Inverse and contact-free forward dynamics of ALL envs in one call, from the resident state [RECALL upstream's per-object
 * ArticulatedSystem::setComputeInverseDynamics / getForceAtJointInWorldFrame / getTorqueAtJointInWorldFrame]: HIP kernels on the world's stream, like
 * the queries above (a pipelined world is joined first); the RSB_DEVICE forms do not synchronise, the RSB_HOST forms stage through the same device
 * buffer.  Both read the resident gc / gv (the base quaternion normalised first) and the world's gravity (rsb_set_gravity).  Neither changes a bit of
 * the world: state, warm state, contact records, what rsb_integrate1 left and the feed-forward rows stay as they are.  An error touches no output.
 *
 * Convention: that of rsb_get_mass_matrix / rsb_get_nonlinearities,  M udot + h = tau + sum J^T w.  gv / udot: base linear (world velocity of the base
 * origin), base angular (world), joints; udot is the component-wise time derivative of gv.  tau[0:3] is a world force at the base origin, tau[3:6] a
 * world torque about it.  M carries the armature on its diagonal, h is Coriolis / centrifugal + gravity.  No PD, no joint damping, no effort clip, no
 * joint limits: the plain equations of motion.
 *
 * External loads: frames is a HOST array of n_frames (0..RSB_MAX_FRAMES; NULL allowed when 0) rsb_frame; force [N,F,3] is a world force applied at the
 * frame's point, torque [N,F,3] a world torque applied to the frame's body; either may be NULL, not both when n_frames > 0.
 * flags: RSB_DYN_CONTACTS - every record c < count[e] of env e's resident contact list (RSB_F_CONTACTS, RSB_F_CONTACT_COUNT: the last sub-step's) acts
 * as the world force impulse / rsb_get_timestep() at `position` on body `body`; both entries of a self-collision act, each on its own body; second-flank
 * and capsule entries act like any other.  The state is the resident one, after that sub-step.
 *
 * rsb_inverse_dynamics:  tau = M(q) udot + h(q,u) - sum_f (J_lin,f^T force_f + J_rot,f^T torque_f) - [RSB_DYN_CONTACTS] sum_c J_c^T (impulse_c / dt),
 * the total generalized force that must act besides the listed loads for the system to accelerate with udot (NULL: zeros, tau = h - loads).
 * joint_force[e,i], joint_torque[e,i]: the force and torque body i's PARENT (the world for i = 0) exerts ON body i through joint i, world frame, the
 * torque about joint i's origin (= body i's frame origin).  This sign convention is ours; upstream's cannot be read from the stub.  The armature is a
 * rotor: armature_i udot_i is part of tau_i, not of the structural wrench:
 *     revolute   a_i . joint_torque_i + armature_i udot_i = tau_i        prismatic   a_i . joint_force_i + armature_i udot_i = tau_i
 *     floating base   (joint_force_0, joint_torque_0) = (tau[0:3], tau[3:6])
 * rsb_forward_dynamics:  the exact inverse, udot = M^-1 (tau - h + sum J^T w), by the articulated-body algorithm (O(nb) per env, no dense M).
 * tau NULL: the resident feed-forward rows (RSB_F_TAU_FF).
 * Fixed-base models: the base neither moves nor accelerates, whatever the base entries of gv, udot and tau hold - no bit of them matters.  Inverse
 * dynamics: tau[0:6] = (joint_force_0, joint_torque_0) is the wrench the world applies at the base origin to hold the base.  Forward dynamics:
 * udot[0:6] = 0 and the joint rows solve the joint block (the convention of rsb_get_inverse_mass_matrix).
 * RSB_E_INVALID, with a message: every output NULL; n_frames < 0 or > RSB_MAX_FRAMES; n_frames > 0 with frames NULL, or with force and torque both
 * NULL; a frame whose body is out of range or whose offset is not finite; unknown flag bits; a bad `space`. */
int rsb_inverse_dynamics(rsb_world* w,
                         const float* udot,            /* [N,nv] in `space`; NULL = zeros                                */
                         const rsb_frame* frames, int n_frames,
                         const float* force,           /* [N,F,3] in `space`; may be NULL                                */
                         const float* torque,          /* [N,F,3] in `space`; may be NULL                                */
                         int flags,
                         float* tau,                   /* [N,nv]                                                         */
                         float* joint_force,           /* [N,nb,3]                                                       */
                         float* joint_torque,          /* [N,nb,3]   any output may be NULL, not all                     */
                         int space);
int rsb_forward_dynamics(rsb_world* w,
                         const float* tau,             /* [N,nv] in `space`; NULL = the resident feed-forward rows       */
                         const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags,
                         float* udot,                  /* [N,nv]                                                         */
                         int space);

/* The slopes of the two queries above: exact (analytic, forward-mode) derivatives of inverse and forward dynamics at the resident state, for ALL envs
 * in one call.  The same rules: HIP kernels on the world's stream (a pipelined world is joined first); the RSB_DEVICE forms do not synchronise, the
 * RSB_HOST forms stage through the same device buffer (which also holds the forward form's intermediates: it grows on first use).  Both read the
 * resident gc / gv (the base quaternion normalised first) and the world's gravity.  Neither changes a bit of the world.  An error touches no output.
 * No atomics, every sum in a fixed order: env e's results depend on env e's rows alone - the same bits for any N and any subset of outputs.
 *
 * Every matrix is [N,nv,nv], entry [e,i,j] the derivative of row i with respect to coordinate j.
 * x_j, the coordinate of dtau_dq / dudot_dq, is the TANGENT coordinate of gc that matches gv's order, so that d gc / dt corresponds to gv exactly:
 *     j < 3         the base origin moves by eps along world axis j;
 *     3 <= j < 6    the base rotates by eps about WORLD axis j-3:  R_0 <- exp(eps [e]x) R_0  (the quaternion is multiplied on the LEFT);
 *     j >= 6        joint coordinate gc[j-6+7] grows by eps.
 * While x varies the components of gv, udot, tau and gravity are held fixed as arrays.  A load's world force and torque are held fixed; its point of
 * application stays fixed ON ITS BODY, so it moves with x.  dtau_dv / dudot_dv: with respect to the components of gv.  The armature contributes to
 * dtau_dudot only.  Columns j < 3 of dtau_dq are exact zeros (translation invariance).
 *
 * rsb_inverse_dynamics_derivatives:  tau = rsb_inverse_dynamics(udot, loads);  dtau_dudot = M(q) (armature on the diagonal).
 * rsb_forward_dynamics_derivatives:  the implicit-function derivatives at udot* = rsb_forward_dynamics(tau, loads), which `udot` receives:
 *     dudot_dq = -M^-1 dtau_dq |udot*        dudot_dv = -M^-1 dtau_dv        dudot_dtau = M^-1
 *   M^-1 is applied by the factorisation of rsb_apply_inverse_mass (once per env in double, the columns in float); dudot_dtau[e,i,j] carries the bits
 *   of rsb_apply_inverse_mass(identity)[e,j,i].
 * flags must be 0: there are no derivatives with RSB_DYN_CONTACTS.
 * Fixed-base models: the six base COLUMNS of every matrix are zero.  The base ROWS of the inverse-dynamics matrices are the derivatives of the holding
 * wrench tau[0:6]; the base rows of the forward-dynamics matrices (and of udot) are zero.  No bit of the base entries of gv, udot or tau matters.
 * RSB_E_INVALID, with a message naming the function: the argument errors of rsb_inverse_dynamics, and non-zero flags. */
int rsb_inverse_dynamics_derivatives(rsb_world* w,
                         const float* udot,            /* [N,nv] in `space`; NULL = zeros                                */
                         const rsb_frame* frames, int n_frames,   /* external loads as in rsb_inverse_dynamics           */
                         const float* force, const float* torque, /* [N,F,3] in `space`; either may be NULL              */
                         int flags,                    /* must be 0                                                      */
                         float* dtau_dq,               /* [N,nv,nv]  d tau_i / d x_j                                     */
                         float* dtau_dv,               /* [N,nv,nv]  d tau_i / d gv_j                                    */
                         float* dtau_dudot,            /* [N,nv,nv]  = M(q); any output may be NULL, not all             */
                         int space);
int rsb_forward_dynamics_derivatives(rsb_world* w,
                         const float* tau,             /* [N,nv] in `space`; NULL = the resident feed-forward rows       */
                         const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags,
                         float* udot,                  /* [N,nv]  the forward dynamics itself                            */
                         float* dudot_dq,              /* [N,nv,nv]                                                      */
                         float* dudot_dv,              /* [N,nv,nv]                                                      */
                         float* dudot_dtau,            /* [N,nv,nv]  = M^-1; any output may be NULL, not all             */
                         int space);

/* M(q)^-1 applied to what the caller chooses, for ALL envs in one call, without forming M: the articulated-body factorisation of rsb_forward_dynamics
 * is done once per env, then every column costs one force and one acceleration pass over the tree (O(nb)).  HIP kernels on the world's stream, like
 * the queries above (a pipelined world is joined first); the RSB_DEVICE forms do not synchronise, the RSB_HOST forms stage through the same device
 * buffer.  Both read the resident gc ONLY (the base quaternion normalised first): gv, gravity, PD, damping, effort clips and joint limits do not
 * enter.  Neither changes a bit of the world.  An error touches no output.
 *
 * Convention: that of rsb_get_mass_matrix - gv order base linear, base angular, joints; M carries the armature on its diagonal.
 * joint_diag: HOST array [nv] or NULL (zeros), D = diag(joint_diag) is added to M: non-negative finite entries, added to the joints' diagonal exactly
 * where the armature is; the six base entries of a floating base must be 0.  With d = dt (kd + dt kp) on the joints, M + D is the effective mass the
 * step's contact problem sees under PD control.
 *
 * rsb_apply_inverse_mass:  X[e,r,:] = (M(q_e) + D)^-1 B[e,r,:] for r < n_rhs (1..RSB_MAX_DOF).  X == B is allowed and gives the same bits.
 * rsb_get_frame_delassus:  with J the stacked rows of rsb_get_frame_jacobians - row 3f+a is the row of J_lin of frame f along world axis a; with
 *   RSB_DELASSUS_ANGULAR row 6f+a is that row for a < 3 and the row of J_rot along axis a-3 for a >= 3 - and k = 3 or 6 rows per frame:
 *     JMinv [N,kF,nv] = J (M + D)^-1          G [N,kF,kF] = J (M + D)^-1 J^T          either may be NULL, not both.
 *   G[e] equals its transpose bit for bit: entries (i,j) and (j,i) both carry the value computed for i <= j - it is what a Cholesky routine is
 *   handed.  G may be singular (more rows than the frames' chains have degrees of freedom); inverting it is the caller's choice.
 *   frames as in rsb_get_frame_kinematics (a HOST array), n_frames 1..RSB_MAX_DELASSUS_FRAMES.
 * Arithmetic: the factorisation (chain walk, inertias, articulated-inertia pass, the base's LDL^T) runs once per env in double, the column passes
 * in float; inputs and outputs are float32.  No atomics; env e's results depend on env e's rows alone - the same bits for any N and any outputs.
 * Fixed-base models: the convention of rsb_get_inverse_mass_matrix - the joint block is solved; the six base rows of X and the six base columns of
 * JMinv are zero; no bit of the base entries of B and joint_diag matters.
 * RSB_E_INVALID, with a message naming the function: a null world; a bad `space`; n_rhs or n_frames out of range; B or X NULL, or every output NULL;
 * a frame whose body is out of range or whose offset is not finite; unknown flag bits; a joint_diag entry that is negative or not finite, or a
 * non-zero base entry of a floating base. */
int rsb_apply_inverse_mass(rsb_world* w,
                           const float* B,               /* [N,R,nv] in `space`                                          */
                           int n_rhs,                    /* R, 1..RSB_MAX_DOF                                            */
                           const float* joint_diag,      /* HOST [nv] or NULL                                            */
                           float* X,                     /* [N,R,nv] in `space`; X == B allowed                          */
                           int space);
int rsb_get_frame_delassus(rsb_world* w, const rsb_frame* frames, int n_frames, /* 1..RSB_MAX_DELASSUS_FRAMES */
                           int flags,                    /* RSB_DELASSUS_ANGULAR                                         */
                           const float* joint_diag,      /* HOST [nv] or NULL                                            */
                           float* G,                     /* [N,kF,kF], k = 3 or 6                                        */
                           float* JMinv,                 /* [N,kF,nv]; either output may be NULL, not both               */
                           int space);

/* Frames HELD: the motion with chosen frames constrained, and the impulse that brings them to a chosen velocity, for ALL envs in one call.  With J, G
 * and JMinv exactly those of rsb_get_frame_delassus for the same frames and flags (the same row order, m = kF rows) and
 * rho_e = damping * max_i G_e[i][i] (damping >= 0, finite: a relative Tikhonov term; 0: none):
 *
 * rsb_constrained_forward_dynamics:  udot_f = rsb_forward_dynamics(tau) without loads and with flags 0 (tau NULL: the resident feed-forward rows),
 *     a_f = J udot_f + Jdot gv, the lin_acc / ang_acc of rsb_get_frame_accelerations(udot_f) in world axes and classical form,
 *     (G + rho I) lambda = target_acc - a_f          udot = udot_f + JMinv^T lambda          D = 0
 *   so that J udot + Jdot gv = target_acc - rho lambda and M udot + h = tau + J^T lambda: lambda[e, 6f+a] (3f+a without RSB_DELASSUS_ANGULAR) is the
 *   world force (a < 3) and torque (a >= 3) the constraint applies at frame f.  target_acc NULL: zeros - the frames are held.  The equations of
 *   motion are rsb_forward_dynamics': no PD, no damping, no clips, no joint limits, no contacts; Baumgarte terms are the caller's, in target_acc.
 * rsb_frame_impulse:  v = J gv, the lin_vel / ang_vel of rsb_get_frame_kinematics,
 *     (G + rho I) lambda = target_vel - v            dgv = JMinv^T lambda = (M + D)^-1 J^T lambda          D = diag(joint_diag)
 *   target_vel NULL: zeros - the frames are stopped.  It reads gc and gv and writes nothing to the world: the caller adds dgv to gv.
 *
 * status[e] = RSB_HELD_SOLVED (0), or RSB_HELD_SINGULAR (1): G_e + rho I is factored as a Cholesky product, and a pivot - what is left of diagonal entry
 * i once the rows before it are taken out - was not above RSB_HELD_PIVOT_TOL (1e-5f) times that entry G_e[i][i] + rho itself, or was not finite: row i
 * depends on the rows before it to float precision (a definition, not a measurement).  That env's lambda is then all zeros, its udot the bits of
 * udot_f (its dgv zeros), and the call still returns RSB_OK; the other envs are not affected.  damping > 0 makes a dependent set solvable.
 * Arithmetic: float throughout - the factorisation, the two substitutions, the sum JMinv^T lambda in row order.
 * HIP kernels on the world's stream, like the queries above (a pipelined world is joined first); the RSB_DEVICE forms do not synchronise, the RSB_HOST
 * forms stage through the same device buffer, which in both forms also holds udot_f, a_f or v, G and JMinv.  No bit of the world changes.  An error
 * touches no output.  No atomics, every sum in a fixed order; env e's results depend on env e's rows alone - the same bits for any N, any subset of
 * outputs, host or device buffers.  Fixed-base models: the base rows of udot / dgv are zero; no bit of the base entries of tau, gv and joint_diag matters.
 * RSB_E_INVALID, with a message naming the function: a null world; a bad `space`; every output NULL; n_frames outside 1..RSB_MAX_DELASSUS_FRAMES or
 * frames NULL; a frame whose body is out of range or whose offset is not finite; unknown flag bits; a negative or non-finite damping; for the impulse
 * the joint_diag errors of rsb_get_frame_delassus. */
int rsb_constrained_forward_dynamics(rsb_world* w,
                           const float* tau,             /* [N,nv] in `space`; NULL = the resident feed-forward rows      */
                           const rsb_frame* frames, int n_frames,   /* HOST, 1..RSB_MAX_DELASSUS_FRAMES: the held frames  */
                           int flags,                    /* RSB_DELASSUS_ANGULAR: 6 rows per frame instead of 3          */
                           const float* target_acc,      /* [N,kF] in `space`, rows ordered as G's; NULL = zeros         */
                           float damping,                /* >= 0, finite, relative: rho_e = damping * max_i G_e[i][i]    */
                           float* udot,                  /* [N,nv]                                                       */
                           float* lambda,                /* [N,kF]                                                       */
                           int32_t* status,              /* [N]; any output may be NULL, not all                         */
                           int space);
int rsb_frame_impulse(rsb_world* w, const rsb_frame* frames, int n_frames, int flags,
                           const float* target_vel,      /* [N,kF] in `space`; NULL = zeros                              */
                           const float* joint_diag,      /* HOST [nv] or NULL, exactly as rsb_get_frame_delassus         */
                           float damping,
                           float* dgv,                   /* [N,nv]  the velocity jump (M + D)^-1 J^T lambda              */
                           float* lambda,                /* [N,kF]  the impulse                                          */
                           int32_t* status,              /* [N]; any output may be NULL, not all                         */
                           int space);

/* Inverse kinematics at frames: which configuration puts these frames at these places, for ALL envs in one call.  One HIP kernel on the world's
 * stream, like the queries above (a pipelined world is joined first); the RSB_DEVICE form does not synchronise, the RSB_HOST form stages through the
 * same device buffer.  No bit of the world changes: the iterate starts at gc_init (NULL: the resident gc) and ends in gc_out.  An error touches no output.
 *
 * Rows, ordered as in rsb_get_frame_delassus: k = 3 or 6 per frame, m = kF.  Row 3f+a is the position row of frame f along world axis a; with
 * RSB_IK_ANGULAR it is row 6f+a for a < 3, and the rotation row about world axis a-3 for a >= 3.
 * Unknowns: column d of the stacked Jacobian (gv's order: base linear, base angular, joints) takes part exactly when dof_mask[d] != 0.  dof_mask is a
 * HOST array [nv]; NULL: every joint is free and the base is held - leg and arm IK relative to a given trunk.  Non-zero base entries free that base
 * coordinate of a floating base; a fixed base's six entries are ignored.
 *
 * The iteration, in float, fixed and deterministic.  The iterate q starts at the start row (the base quaternion is normalised wherever it is read, as
 * in every query).  At each pass, `it` counting the steps taken so far:
 *   1. the rows e at q: position rows target_pos - pos; rotation rows the world-frame rotation vector of S = R_t R^T (R = rot of
 *      rsb_get_frame_kinematics): v = (S21 - S12, S02 - S20, S10 - S01) / 2, c = (tr S - 1) / 2, theta = atan2(|v|, c), rows v theta / |v|, or v
 *      itself where |v| <= 1e-6.  An angle within 1e-6 of pi has no defined axis: such targets are OUTSIDE the contract.
 *   2. err_pos, err_rot: the largest absolute position and rotation row.  err_pos <= pos_tol and err_rot <= rot_tol: stop, RSB_IK_CONVERGED.
 *      Otherwise, if it == max_iter: stop, RSB_IK_MAX_ITER.
 *   3. J with masked columns zero, A = J J^T, rho = damping * max_i A[i][i]; A + rho I is factored by the root-free Cholesky with the pivot rule of
 *      rsb_constrained_forward_dynamics (RSB_HELD_PIVOT_TOL).  A refused pivot, or max_i A[i][i] = 0: stop, RSB_IK_SINGULAR, at the current iterate.
 *   4. y = (A + rho I)^-1 e, dq = J^T y summed in row order, in gv's coordinates; if s = max|dq| exceeds max_step, dq is scaled by max_step / s.
 *   5. q <- q (+) dq on the free coordinates: joints add; the base origin adds; the base quaternion is multiplied on the LEFT by exp(dq[3:6]) and
 *      normalised - the tangent convention of rsb_inverse_dynamics_derivatives.  With RSB_IK_JOINT_LIMITS the joints are then clamped into the
 *      model's [q_lower, q_upper] (unlimited joints have none).
 *   6. it <- it + 1.
 * gc_out is the last iterate, error = (err_pos, err_rot) of exactly that iterate, iterations = it.  Coordinates that are not free carry the start
 * row's bits - the base quaternion too when no base rotation is free.  max_iter == 0 is a pure evaluation: gc_out carries the start's bits.
 * Arithmetic: float throughout; tolerances below about 1e-5 (m, rad) may never be met - the rows themselves carry float roundings of the frame
 * positions.  No atomics, every sum in a fixed order; env e's results depend on env e's rows alone - the same bits for any N, any neighbours
 * (converged, unconverged or singular), any subset of outputs, host or device buffers, gc_init NULL or equal to the resident rows.
 * RSB_E_INVALID, with a message naming the function: a null world; a bad `space`; every output NULL; n_frames outside 1..RSB_MAX_IK_FRAMES or frames
 * NULL; a frame whose body is out of range or whose offset is not finite; unknown flag bits; target_pos NULL; target_rot present without
 * RSB_IK_ANGULAR or absent with it; opt NULL; max_iter < 0; damping, a tolerance or max_step negative or not finite; max_step == 0; a mask that
 * frees no coordinate. */
int rsb_inverse_kinematics(rsb_world* w, const rsb_frame* frames, int n_frames, /* HOST, 1..RSB_MAX_IK_FRAMES */
                           int flags,                    /* RSB_IK_ANGULAR | RSB_IK_JOINT_LIMITS                         */
                           const float* target_pos,      /* [N,F,3] world, in `space`                                    */
                           const float* target_rot,      /* [N,F,9] row-major world<-body, in `space`; required with RSB_IK_ANGULAR, must be NULL without */
                           const float* gc_init,         /* [N,nq] in `space`; NULL = the resident gc                    */
                           const uint8_t* dof_mask,      /* HOST [nv] or NULL                                            */
                           const rsb_ik_options* opt,    /* HOST                                                         */
                           float* gc_out,                /* [N,nq]                                                       */
                           float* error,                 /* [N,2]: largest |position row| (m), largest |rotation row| (rad; 0 without RSB_IK_ANGULAR) at gc_out */
                           int32_t* iterations,          /* [N] steps taken                                              */
                           int32_t* status,              /* [N]; any output may be NULL, not all                         */
                           int space);

/* Terrain queries of ALL envs in one call [RECALL upstream's per-object HeightMap::getHeight / getNormal and World::rayTest, called per env on the
 * host]: HIP kernels on the world's stream, like the frame queries above; the RSB_DEVICE forms do not synchronise, the RSB_HOST forms stage through
 * the same device buffer.  They work on a ground plane and on a height map; with per-env maps (rsb_set_heightmaps) every env reads its own map.  The
 * surface is the collider's: each grid cell split along its (ix, iy)-(ix+1, iy+1) diagonal, coordinates outside the footprint clamped to it.
 *
 * rsb_get_terrain_height: xy [N,P,2] world coordinates in `space` -> height [N,P], normal [N,P,3] (the unit normal of the triangle under the point);
 * either output may be NULL, not both.  Ground plane: ground_z and (0, 0, 1). */
int rsb_get_terrain_height(rsb_world* w, const float* xy, int n_points, float* height, float* normal, int space);
/* The height scan of an exteroceptive observation: for every env, frame f and pattern point k
 *   out[e * row_stride + f * P + k] = p_z - h(p_xy + M pattern[k]),
 * p the frame's world position at the resident state (frames as in rsb_get_frame_kinematics, a HOST array), pattern [P,2] in `space`,
 * P = n_points <= RSB_MAX_SCAN_POINTS.  mode RSB_SCAN_WORLD: M = identity; RSB_SCAN_YAW: M = the rotation about z by the frame's heading,
 * (c, s) = (R[0], R[3]) / hypot(R[0], R[3]) of the body's rotation R ((1, 0) where the hypot is below 1e-6: the body's x axis is vertical).
 * row_stride, in floats: 0 = F * P (a dense [N,F,P] output); larger values write the scan into columns [0, F * P) of rows of that pitch - pass
 * a pointer into a wider observation tensor - and touch no other column; smaller non-zero values are RSB_E_INVALID. */
int rsb_height_scan(rsb_world* w, const rsb_frame* frames, int n_frames, const float* pattern, int n_points, int mode,
                    float* out, long long row_stride, int space);
/* Rays against the terrain (not against bodies): origins, directions [N,R,3] world coordinates in `space` -> dist [N,R] in metres along the
 * normalised direction (directions need not be unit length), -1 for a miss.  With [lo, hi] the part of [0, max_dist] where the ray is over the
 * map's footprint, a hit is the first s in [lo, hi] with z(s) <= h(x(s), y(s)), h as in rsb_get_terrain_height: an origin below the surface
 * gives 0, a ray that enters the footprint below the surface hits the map's side wall at s = lo, a ray that never meets the footprint misses.
 * Ground plane: the infinite plane.  A ray with a zero or non-finite direction or a non-finite origin gives -1.  max_dist must be positive and
 * finite.  There is no normal output: feed the hit's xy to rsb_get_terrain_height. */
int rsb_ray_test(rsb_world* w, const float* origins, const float* directions, int n_rays, float max_dist, float* dist, int space);

/* Rays that also stop at the robot, and ray patterns mounted on a body (a depth camera, a lidar): World::rayTest upstream hits every object of the
 * world [RECALL]; rsb_ray_test above sees the terrain only.  Both calls read the resident gc alone (base quaternion normalised first, a fixed base's
 * base rows as the world keeps them), change no bit of the world, join a pipelined world as the other queries do, and touch no output when they
 * return an error.
 *
 * The robot's shapes, built once per world from the model's collision primitives in index order:
 *   col_capsule[s] == -1                     an oriented box from its eight corners s .. s + 7
 *   col_capsule[s] = e + 1, col_rim[s] == 0  a capsule between the centres of primitives s and e, radius col_radius[s]
 *   col_capsule[s] = e + 1, col_rim[s] > 0   a cylinder with flat caps between the centres of s and e, radius col_rim[s]
 *   any other primitive with col_radius > 0  a sphere (the extra spheres of a sampled capsule lie inside it and change nothing)
 * Zero-radius points - a mesh's hull vertices, the lattice of a sampled box, a lone rim - have no surface: a MESH collider is invisible to rays.
 * A body hit is the first s >= 0 at which the ray is on or inside a shape; an origin inside a shape gives 0, as an origin under the terrain does.
 *
 * flags: RSB_RAY_BODIES    rays stop at the shapes above as well as at the terrain; without it the calls see what rsb_ray_test sees
 *        RSB_RAY_MISS_MAX  a miss reports max_dist, not -1
 *        RSB_RAY_OWN_BODY, RSB_RAY_PLANAR: rsb_ray_scan only, below.  Unknown bits are RSB_E_INVALID.
 * hit (int32, optional): RSB_RAY_HIT_NONE, RSB_RAY_HIT_TERRAIN, or the index of the FIRST collision primitive of the shape that was hit
 * (rsb_model_blob::col_body / col_name of it name the link).
 *
 * rsb_ray_cast, the world-space form: origins, directions [N,R,3] in `space` -> dist [N,R], hit [N,R]; either output may be NULL, not both.  With
 * flags == 0 dist is rsb_ray_test's, bit for bit.  With RSB_RAY_BODIES dist is the smaller of the terrain hit and the first body entry (a tie is the
 * terrain's); where the terrain wins dist carries rsb_ray_test's bits: the terrain march always runs with the call's max_dist and is never
 * shortened by a body hit - one definition of the terrain answer, for the price of an optimisation.  RSB_RAY_OWN_BODY and RSB_RAY_PLANAR are
 * RSB_E_INVALID here: a world-space ray has no frame. */
int rsb_ray_cast(rsb_world* w, const float* origins, const float* directions, int n_rays, float max_dist, int flags,
                 float* dist, int32_t* hit, int space);
/* rsb_ray_scan, the sensor form: for every env e, frame f (a HOST array, as in rsb_get_frame_kinematics) and pattern direction k
 *   out[e * row_stride + f * P + k] = range from the frame's world point along R_body(f) dirs[k],
 * dirs [P,3] in `space`, expressed in the axes of the frame's body, of any length (normalised as rsb_ray_test normalises); a zero or non-finite
 * direction gives a miss.  P = n_points <= RSB_MAX_RAY_POINTS.  Our axis convention for the pattern helpers: x forward, y left, z up ([RECALL]-
 * unknown: upstream's sensor axes cannot be read from the stub).  An rsb_frame has no orientation of its own: a sensor tilted against its body
 * rotates its pattern on the host, once.
 *   RSB_RAY_OWN_BODY  the shapes of the frame's own body are tested too (default: a sensor sees through its mount)
 *   RSB_RAY_PLANAR    out = range * (unit direction . the body's x axis): the depth image of a pinhole camera looking along x, not the range along
 *                     the ray; with RSB_RAY_MISS_MAX a miss is max_dist times the same cosine (1 for a direction that cannot be cast)
 * row_stride as in rsb_height_scan: 0 = F * P (dense [N,F,P]); a larger value writes columns [0, F * P) of rows of that pitch and touches no other
 * column; a smaller non-zero value is RSB_E_INVALID.  hit is dense [N,F,P].  Either of out, hit may be NULL, not both.  A ray's result does not
 * depend on which other frames or directions the call lists. */
int rsb_ray_scan(rsb_world* w, const rsb_frame* frames, int n_frames, const float* dirs, int n_points, int flags, float max_dist,
                 float* out, long long row_stride, int32_t* hit, int space);

/* Contact sensors of ALL envs in one call, from the resident contact list [RECALL upstream's per-object answer: a host loop over
 * ArticulatedSystem::getContacts()]: one HIP kernel on the world's stream, like the queries above (a pipelined world is joined first); the RSB_DEVICE
 * forms do not synchronise, the RSB_HOST forms stage through the same device buffer.  frames as in rsb_get_frame_kinematics (a HOST array).  None of
 * the three changes a bit of the world.  An error touches no output.
 *
 * A "record" is an entry c < min(count[e], kmax) of env e's resident contact list (RSB_F_CONTACTS / RSB_F_CONTACT_COUNT, what rsb_get_contacts
 * returns: the last sub-step's).  It acts as the world force impulse / rsb_get_timestep() at `position` on body `body`, the convention of
 * RSB_DYN_CONTACTS; inv_dt = (float)(1.0 / dt).  Frame f OWNS the records whose body == frames[f].body: every primitive of the link, second-flank
 * and capsule entries, and its entry of a self-collision.  flags: RSB_CONTACT_LOCAL - vector outputs multiplied by R^T (the axes of the frame's body,
 * R = rot of rsb_get_frame_kinematics); RSB_CONTACT_NO_SELF - records flagged RSB_CONTACT_SELF_A / _B are left out.  Sums run in ascending record
 * index in registers: no atomics, the same bits in every call, for any N, any other frames listed, any subset of outputs, host or device buffers.
 *
 * rsb_get_body_contact_wrenches: force [N,F,3] = sum of the owned records' forces; torque [N,F,3] = sum of (position_c - p_f) x force_c, p_f the
 * frame's world point (pos of rsb_get_frame_kinematics); count [N,F] int32 = number of owned records.  Any output may be NULL, not all.
 *
 * rsb_contact_observe: the fused contact rows of an observation, six floats for env e and frame f at out[e * row_stride + 6 f + 0..5]:
 *   0     1.0f if the normal force (column 4) is greater than force_threshold, else 0.0f
 *   1..3  the net force: the bits of rsb_get_body_contact_wrenches' force under the same flags
 *   4     the normal force, sum_c (impulse_c . normal_c) * inv_dt
 *   5     the slip speed, max_c |v - (v . n_c) n_c| with v = v_b + omega_b x (position_c - p_b) the velocity of the body's material point at the
 *         record's position from the resident gv; 0 without an owned record; the same under RSB_CONTACT_LOCAL
 * row_stride as in rsb_imu_observe: 0 = 6 F; a larger value writes columns [0, 6 F) of rows of that pitch and touches no other float; a smaller
 * non-zero value is RSB_E_INVALID.
 *
 * rsb_contact_timers: feet air time / contact time in the CALLER's buffers (the world stores nothing), one fp32 update per (env, frame) with
 * "contact" the predicate of column 0 above and dt the caller's control step (positive, finite):
 *   reset_mask[e] != 0    touchdown = 0               air_time = 0     contact_time = 0
 *   contact               touchdown = old air_time    air_time = 0     contact_time += dt
 *   no contact            touchdown = 0               air_time += dt   contact_time = 0
 * (touchdown: the flight that just ended, 0 if there was none.)  A timer that is NULL is taken as 0 and not written.
 *
 * Fixed-base models: body 0 does not move, whatever the base rows of gv hold - no bit of them matters.
 * RSB_E_INVALID, with a message naming the function: a null world; a bad `space`; every output NULL; n_frames outside 1..RSB_MAX_FRAMES, a frame
 * whose body is out of range or whose offset is not finite; unknown flag bits; a negative or non-finite force_threshold; a bad row_stride; a bad dt. */
int rsb_get_body_contact_wrenches(rsb_world* w, const rsb_frame* frames, int n_frames, int flags,
                                  float* force,         /* [N,F,3] */
                                  float* torque,        /* [N,F,3] */
                                  int32_t* count,       /* [N,F]    any output may be NULL, not all */
                                  int space);
int rsb_contact_observe(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, float force_threshold,
                        float* out, long long row_stride, int space);
int rsb_contact_timers(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, float force_threshold, float dt,
                       const uint8_t* reset_mask,       /* [N] or NULL: envs whose timers restart (the done flags of a step) */
                       float* air_time,                 /* [N,F] in/out */
                       float* contact_time,             /* [N,F] in/out; either timer may be NULL, not both */
                       float* touchdown,                /* [N,F] out, may be NULL */
                       int space);

/* obs block [N, nq+nv+3*n_force_slots] = (q, u, contact force on chosen collision primitives).
 * collision_indices: host array of n_force_slots collision-primitive indices (e.g. the feet);
 * NULL = primitives 0..n_force_slots-1.  Force = impulse / dt of the last sub-step (world frame). */
int rsb_obs_dim(const rsb_world* w, int n_force_slots);
int rsb_gather_obs(rsb_world* w, float* out, const int32_t* collision_indices, int n_force_slots, int space);

/* VectorizedEnvironment support (raisimGymTorch's isTerminalState()+reset() fan-out [RECALL]), on device:
 * every env whose last sub-step holds a contact on a collision primitive NOT listed in
 * allowed_collisions (host array; e.g. the feet -> "terminate on any non-foot contact"), or whose state is
 * non-finite, is reset to row e (rows == N) or row 0 (rows == 1) of gc0/gv0.  done (uint8 [N], same
 * memspace as gc0/gv0, may be NULL) receives 1 for the envs that were reset, 0 otherwise. */
int rsb_reset_terminated(rsb_world* w, const int32_t* allowed_collisions, int n_allowed, const float* gc0,
                         const float* gv0, int rows, uint8_t* done, int space);

/* One control step of VectorizedEnvironment::step() [RECALL raisimGymTorch/env/VectorizedEnvironment.hpp] enqueued
 * with a single call on the handle's stream: rsb_set_pd_target (device pointers, either may be NULL) ->
 * rsb_integrate(n_substeps) -> rsb_gather_obs (skipped when obs_out is NULL) -> rsb_reset_terminated (skipped
 * when gc0 or gv0 is NULL).  Index lists are host arrays, everything else lives on the device. */
int rsb_control_step(rsb_world* w, const float* p_target, const float* d_target, int n_substeps, float* obs_out,
                     const int32_t* force_collisions, int n_force_slots, const int32_t* allowed_collisions,
                     int n_allowed, const float* gc0, const float* gv0, int rows);

/* ---- round 6: RESIDENT control steps.  K control steps of a vectorised env in ONE launch of the step kernel: an env block's state (and the solver's
 * warm table, the model tables) stays in LDS from the first sub-step to the last; per control step only the obs block, the done flags and - env task -
 * reward / next observation go to HBM; state rows, warm records and contact records are written after the LAST control step (the world then holds exactly
 * what K separate rsb_control_step calls leave: the tests compare bit for bit).  A terminated env restarts in LDS.  Why: a launch lasts as long as its
 * slowest wave, and a wave's time over K control steps is a SUM - the tail averages out with no hand-over between launches, and the per-launch
 * prologue / epilogue (8 k of a launch's 180 k cycles) is paid once.  Upstream counterpart: the loop over VectorizedEnvironment::step
 * [RECALL raisimGymTorch/env/VectorizedEnvironment.hpp; absent from /root/reference].
 *
 * rsb_control_steps: K control steps of the OPEN loop.  p_targets [period][N][nq] device memory: control step j reads slice (first + j) % period (the
 * benchmark's pre-drawn PD-target bank; an action sequence of sampling-based MPC; a replay).  obs_out (may be NULL): control step j's obs block goes to
 * obs_out + j * obs_step_stride floats (0: every step overwrites the same block; N * rsb_obs_dim: a [K, N, obs_dim] rollout); done_out (may be NULL, device
 * memory): its done flags to done_out + j * done_step_stride bytes.  The other arguments are rsb_control_step's.
 * With residency OFF (the default), or for a world outside the resident kernel classes (see rsb_step_residency_status), the same call runs K
 * rsb_control_step launches - pipelined or in lock-step as rsb_set_step_pipelining says - with the same results. */
int rsb_control_steps(rsb_world* w, int n_steps, const float* p_targets, int period, long long first, int n_substeps, float* obs_out,
                      long long obs_step_stride, const int32_t* force_collisions, int n_force_slots, const int32_t* allowed_collisions, int n_allowed,
                      const float* gc0, const float* gv0, int rows, uint8_t* done_out, long long done_step_stride);
/* ---- multi-GPU without Python: the obs all-gather over RCCL / xGMI.  One process per GPU; envs are sharded
 * contiguously, rank r owns global envs [r*N, (r+1)*N); nothing inside integrate() communicates.  librccl.so.1 is loaded
 * at run time by the first rsb_comm_* call (a host that never calls them needs no RCCL).  Upstream has no counterpart
 * (RaiSim is single-process); this is the C/C++ twin of raisimlib_amd/dist.py.
 *   rsb_comm_get_unique_id : rank 0 creates the id (ncclGetUniqueId), the launcher hands it to the other ranks
 *   rsb_comm_init          : ncclCommInitRank on the world's device (collective: every rank calls it)
 *   rsb_allgather_obs      : the rank's obs block (rsb_gather_obs semantics) -> out [n_ranks*N, obs_dim], rank-major, on the
 *                            handle's stream; out in `space` (DEVICE: gathered in place, nothing synchronises; HOST: staged) */
/* RSB_MAX_RANKS (ranks of one node; peer-mapped obs exchange below): rsb_types.h */
#define RSB_COMM_ID_BYTES 128
/* versions of RCCL as NCCL_VERSION_CODE: of the librccl.so.1 loaded at run time (ncclGetVersion) and of the <rccl/rccl.h> this library's constants were checked
 * against when it was built (0: the header was not installed on the build host).  Either pointer may be NULL. */
int rsb_comm_rccl_version(int* runtime_version, int* header_version);
int rsb_comm_get_unique_id(char id[RSB_COMM_ID_BYTES]);
int rsb_comm_init(rsb_world* w, int n_ranks, int rank, const char id[RSB_COMM_ID_BYTES]);
int rsb_comm_destroy(rsb_world* w);
int rsb_allgather_obs(rsb_world* w, const int32_t* collision_indices, int n_force_slots, float* out, int space);

/* ---- the same exchange WITHOUT a collective or a copy kernel: peer-mapped gathered buffers.  The step kernel fills every CU
 * of the chip, so a collective's copy kernel cannot overlap it and costs a kernel slot per control step (measured: 8 % at one
 * rank).  Here every rank owns a gathered buffer [n_ranks * N, obs_dim] (double-buffered by control-step parity) that the other
 * ranks map - hipIpc handles across processes, plain pointers within one process -, and the epilogue of rsb_control_step's ONE
 * launch stores each env's obs row into the buffer of every rank (write-through stores; the other GPUs' over xGMI); the last wave
 * of the launch to finish writes the step number into every rank's flag array, and rsb_obs_peer_wait makes the stream wait
 * (command-processor poll of the flag words, no kernel) until every rank has delivered the rows of the last control step issued.
 *   rsb_obs_peer_create       allocate this rank's buffer (fine-grained device memory); `handle` (may be NULL) receives its IPC handle
 *   rsb_obs_peer_connect      handles [n_ranks][RSB_OBS_HANDLE_BYTES] of all ranks (own entry ignored), e.g. from an all-gather of the launcher
 *   rsb_obs_peer_connect_ptrs the same within ONE process: base pointers (rsb_obs_peer_base) of the other worlds, peer access enabled by the caller
 *   rsb_obs_peer_wait         see above; *gathered (may be NULL) receives the device pointer of the complete block of that step, rank-major
 * From rsb_obs_peer_connect on, every rsb_control_step of the world runs the exchange (obs_out may be NULL).  Floating-base models
 * of tree depth <= 13.  RCCL (above) stays the default of bench.py until a multi-GPU box has measured both. */
#define RSB_OBS_HANDLE_BYTES 64
int rsb_obs_peer_create(rsb_world* w, int n_ranks, int rank, const int32_t* collision_indices, int n_force_slots, char handle[RSB_OBS_HANDLE_BYTES]);
int rsb_obs_peer_connect(rsb_world* w, const char* handles);
int rsb_obs_peer_connect_ptrs(rsb_world* w, void* const* bases);
void* rsb_obs_peer_base(rsb_world* w);
int rsb_obs_peer_wait(rsb_world* w, float** gathered);
int rsb_obs_peer_destroy(rsb_world* w);

/* done flags of the fused control step: when `done_device` (uint8 [num_envs], DEVICE memory, caller-owned) is set,
 * every following rsb_control_step writes 1 for the envs it reset and 0 for the others (NULL switches it off). */
int rsb_set_done_output(rsb_world* w, uint8_t* done_device);

/* ---- device-resident vectorised env: the per-env observe / step / reward / terminate / reset of
 * VectorizedEnvironment<ENVIRONMENT> with rsg_anymal's task [RECALL raisimGymTorch/env/envs/rsg_anymal/Environment.hpp,
 * absent from /root/reference], computed on the GPU so that a learner whose policy runs on the same device never
 * crosses PCIe:
 *   action [N, nv-6]   -> PD position targets  action_mean + action_std * action  on the actuated joints
 *   observation [N, 10 + 2(nv-6)] = height, third ROW of the base rotation matrix (the world z-axis expressed in the
 *                        body frame: rsg_anymal's rot.e().row(2)), joint angles, body-frame linear velocity (3),
 *                        body-frame angular velocity (3), joint velocities
 *   reward = forward_vel_coeff * min(forward_vel_clip, body-frame v_x) + torque_coeff * |tau|^2, tau = the actuator
 *            torque the last sub-step applied (PD + feed-forward after the effort clip; upstream reads
 *            getGeneralizedForce() after the last integrate())
 *   done   = a contact on a primitive outside foot_collisions, or a non-finite state; such envs get
 *            reward += terminal_reward (upstream perAgentStep) and restart from gc_init / gv_init. */
typedef struct rsb_env_config {
  int32_t n_substeps;            /* control_dt / simulation_dt */
  float action_std;
  float forward_vel_coeff, forward_vel_clip, torque_coeff, terminal_reward;
  int32_t n_foot;
  int32_t foot_collisions[RSB_MAX_COLLISIONS];
} rsb_env_config;
/* action_mean [nv-6], gc_init [nq], gv_init [nv]: host arrays (copied) */
int rsb_env_configure(rsb_world* w, const rsb_env_config* cfg, const float* action_mean, const float* gc_init,
                      const float* gv_init);
int rsb_env_dims(const rsb_world* w, int* ob_dim, int* action_dim);
/* Per-env reset states (optional; gc0 [N, nq], gv0 [N, nv] in `space`, copied): a terminated env - and rsb_env_reset - restarts from ITS row
 * instead of the one gc_init / gv_init of rsb_env_configure (the benchmark's per-env base position and heading; raisimGymTorch environments
 * that randomise their initial state in reset() [RECALL]).  NULL, NULL: back to the single initial state. */
int rsb_env_set_reset_states(rsb_world* w, const float* gc0, const float* gv0, int space);
int rsb_env_reset(rsb_world* w);                                   /* every env to gc_init / gv_init */
int rsb_env_observe(rsb_world* w, float* ob, int space);           /* [N, ob_dim] */
/* action [N, action_dim] in; reward [N] float, done [N] uint8 and ob_next [N, ob_dim] (the observation the next step
 * starts from, i.e. after the resets) out, any of which may be NULL; all in `space`.  Two launches: the step kernel
 * (action -> PD targets in its prologue) and one reward / termination / reset / observation kernel. */
int rsb_env_step(rsb_world* w, const float* action, float* reward, uint8_t* done, float* ob_next, int space);

/* Running observation statistics of the env task, on the device (the template path's updateObservationStatisticsAndNormalize
 * [RECALL raisimGymTorch VectorizedEnvironment::observe(ob, updateStatistics), getObStatistics, setObStatistics]).  Per world, from the
 * first rsb_env_configure on: count = 1e-4, mean = 0, var = 1 (ob_dim entries each; kept in fp64, count included).  A batch of N
 * observations is merged with its mean and population variance over the N envs (Chan's formula, upstream's arithmetic); an observation
 * is normalised as clamp((ob - mean) * inv_std, -clip, clip) with inv_std = 1 / sqrt(var + 1e-8) rounded to float once, clip <= 0: none.
 * Every call is enqueued on the world's stream (ordered with steps, pipelined or resident, and closed-loop runs); the RSB_DEVICE forms
 * do not synchronise.  Each world (each rank) keeps its own statistics.  rsb_env_observe, rsb_env_step's ob_next and the closed-loop
 * runs stay raw.
 *   rsb_env_observe_normalized  rsb_env_observe, then (update_statistics != 0) the batch merged into the statistics, then normalised.
 *   rsb_env_obs_stats_update    n_batches batches of [N, ob_dim] floats, batch_stride floats apart (0: N * ob_dim), merged in order - a
 *                               closed-loop rollout's ob [K + 1, N, ob_dim]; one call over B batches = B calls over one batch, bit for bit.
 *   rsb_env_obs_normalize       rows x ob_dim floats normalised with the current statistics (in == out allowed): a stored rollout.
 *   rsb_env_get_obs_stats / rsb_env_set_obs_stats   host arrays [ob_dim] (any output may be NULL); synchronise.
 *   rsb_env_obs_stats_device    device pointers mean [ob_dim] and inv_std [ob_dim] (float), valid for the world's lifetime and updated in
 *                               stream order: an rsb_mlp_policy's ob_mean / ob_inv_std, read by each run as of its launch. */
int rsb_env_observe_normalized(rsb_world* w, float* ob, int update_statistics, float clip, int space);
int rsb_env_obs_stats_update(rsb_world* w, const float* obs, int n_batches, long long batch_stride, int space);
int rsb_env_obs_normalize(rsb_world* w, const float* in, float* out, long long rows, float clip, int space);
int rsb_env_get_obs_stats(rsb_world* w, float* mean, float* var, double* count);
int rsb_env_set_obs_stats(rsb_world* w, const float* mean, const float* var, double count);
int rsb_env_obs_stats_device(rsb_world* w, const float** mean, const float** inv_std);

/* zero-copy access to the resident state (device pointers; row-major [N,dim] float32): see rsb_field */
void* rsb_device_ptr(rsb_world* w, int field);

#ifdef __cplusplus
}
#endif

#include "rsb_ext.h"        /* what has no upstream counterpart: solver heuristics, launch scheduling (pipelining, residency), timing, debug aids */
#include "rsb_pipeline.h"   /* the closed-loop pipeline (C declarations; under hipcc also the device-side serve loop of an action stage) */

#endif /* RSB_H_ */
