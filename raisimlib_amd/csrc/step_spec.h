// step_spec.h — SPECIALISED compilation of the step kernel (rsb_specialize; rsb_spec.hip).
//
// The ahead-of-time kernel classes of step_launch.h read the model's dimensions (bodies, coordinates, tree depth, collision primitives, candidate
// pairs of self-collision ...) and the world's switches (terrain kind, sub-steps per call, warm start, solver lags ...) from their kernel arguments:
// every one of them is a scalar load, a live SGPR and - worst for the ONE wave a SIMD holds - a branch or a loop bound the compiler cannot resolve
// (a branch costs a lone wave 20-45 cycles taken or not: profiles/r02_ubench_lone_wave_latency.txt; the generic quadruped class executes ~245 of
// them per sub-step: profiles/r06_spec_log.txt).  A specialised code object is the SAME template instance compiled once more with those values as
// compile-time constants (-DRSB_SPECIALIZED -DRSB_SPEC_NB=13 ...): 30 % fewer instructions, 40 % fewer branches, less than half the spilled SGPRs,
// bit-identical results, +13 % env-steps/s on the benchmark.  The code object is loaded as a HIP module and launched with the same StepArgs.
//
// ONE list names what is specialised: RSB_SPEC_FIELDS(X) calls X(MACRO_SUFFIX, value-expression over a StepArgs `a`).  The host builds a launch's key
// and the compiler's -D flags from it (rsb_spec.hip); the kernel reads a field as RSB_DIM(SUFFIX, generic expression).
#pragma once

#define RSB_SPEC_FIELDS(X)                                                                                                              \
  X(NB, a.nb) X(NQ, a.nq) X(NV, a.nv) X(DEPTH, a.depth) X(NCOL, a.ncol) X(MAX_KID, a.max_kid) X(FIXED_BASE, (a.fixed_base != 0))      \
  X(N_SELF, a.n_self) X(NSUB, a.nsub) X(KMAX, a.kmax) X(HAS_WARM, (a.warm != nullptr)) X(TERRAIN, a.terrain_type)                      \
  X(EARLY_TERM, (a.early_term != 0)) X(SECTION_ROUNDS, a.section_rounds) X(STALL_WINDOW, a.stall_window) X(FREEZE_AFTER, a.freeze_after) \
  X(REFINE, a.refine) X(MULTI_FA, a.multi_freeze_after) X(MULTI_DEPTH, a.multi_depth) X(MULTI_LIGHT, a.multi_light)                    \
  X(MULTI_SW, a.multi_stall_window) X(CHAIN, (a.chain != 0)) X(MODEL_PITCH, a.L.model_pitch) \
  X(UP_QUADS, (a.chain == 2))

#ifdef RSB_SPECIALIZED
#define RSB_DIM(NAME, expr) (RSB_SPEC_##NAME)
#else
#define RSB_DIM(NAME, expr) (expr)
#endif

// Quad form of the up pass's level loop (step_phase_tree_up.inc): four lanes per body instead of one, in the specialised code objects of worlds whose
// every tree level holds exactly four bodies at 16 lanes per env (StepArgs::chain == 2: the quadruped).  -DRSB_X_NO_UP_QUADS (RSB_SPEC_EXTRA_DEFS,
// tools/exp/ab_defs.sh) compiles the lane = body loop of every other world instead: same results bit for bit (tests/test_gpu_up_quads.py).  The ahead-of-time
// classes always run the lane = body loop.
#if defined(RSB_SPECIALIZED) && RSB_SPEC_UP_QUADS && !defined(RSB_X_NO_UP_QUADS)
#define RSB_UP_QUADS 1
#if !RSB_SPEC_CHAIN
#error "RSB_SPEC_UP_QUADS: the quad form of the up pass is for consecutively numbered chains (RSB_SPEC_CHAIN)"
#endif
#else
#define RSB_UP_QUADS 0
#endif

// Quad form of the down pass's level loop (step_phase_tree_down.inc), for the same worlds and code objects: quad g walks DOWN chain g with the parent's pose,
// velocity and bias acceleration in its registers and writes the BODY slots lane by lane (step_kernel.h: body_pose_ld); the update pass then takes the joint axis S
// from the FACT slot, as it takes the up pass's factors there (hence: only beside the up pass's quad form).
// -DRSB_X_NO_DOWN_QUADS compiles the lane = body loop beside the up pass's quad form: same results bit for bit (tests/test_gpu_down_quads.py).
#if RSB_UP_QUADS && !defined(RSB_X_NO_DOWN_QUADS)
#define RSB_DOWN_QUADS 1
#else
#define RSB_DOWN_QUADS 0
#endif

// Seam carry, for the same worlds and code objects (the classes that run both quad forms): what one sub-step's update pass leaves for the next sub-step's down pass
// stays in registers instead of making a round trip through LDS (step_phase_tree_down.inc, step_phase_update.inc, step_kernel.h).  Three parts, each with a switch
// of its own for an A/B:
//   RSB_SEAM_JOINTS  a body lane keeps its joint's q and qd across the seam (loaded once per control step, in front of the sub-step loop)
//   RSB_SEAM_BASE    the base's q (7) and u (6) stay in registers: lane 0 updates them from its registers, thirteen row_bcast<0> moves hand them to the env's row
//   RSB_SEAM_LOADS   the lane's MODELF row and the actuation's five scalars (feed-forward torque, kp, kd, target, target velocity) are fetched as ONE batch with one
//                    wait, issued in front of the base arithmetic
// (Two more parts were built and measured, and are not here: the five scalars held in registers over a control step, and the update pass's entry of W_b read once
//  instead of per level - DESIGN.md section 9.)
// With JOINTS and BASE nothing at the top of a sub-step reads what the update pass wrote; the barrier that closes the update pass stays all the same
// (step_phase_update.inc says what it still orders).  The stores to Q and U stay: joint limits, contact columns, the epilogue and the host read them.
// -DRSB_X_NO_SEAM_CARRY compiles the code as it was: same results bit for bit (tests/test_gpu_seam_carry.py).
#if RSB_DOWN_QUADS && !defined(RSB_X_NO_SEAM_CARRY)
#define RSB_SEAM_CARRY 1
#else
#define RSB_SEAM_CARRY 0
#endif
#if RSB_SEAM_CARRY && !defined(RSB_X_NO_SEAM_JOINTS)
#define RSB_SEAM_JOINTS 1
#else
#define RSB_SEAM_JOINTS 0
#endif
#if RSB_SEAM_CARRY && !defined(RSB_X_NO_SEAM_BASE)
#define RSB_SEAM_BASE 1
#else
#define RSB_SEAM_BASE 0
#endif
#if RSB_SEAM_CARRY && !defined(RSB_X_NO_SEAM_LOADS)
#define RSB_SEAM_LOADS 1
#else
#define RSB_SEAM_LOADS 0
#endif

namespace rsbk {
#define RSB_SPEC_COUNT_ONE(NAME, expr) +1
constexpr int kSpecFields = 0 RSB_SPEC_FIELDS(RSB_SPEC_COUNT_ONE);
#undef RSB_SPEC_COUNT_ONE
}  // namespace rsbk
