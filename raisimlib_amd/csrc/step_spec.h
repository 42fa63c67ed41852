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
  X(UP_QUADS, (a.chain == 2)) \
  X(MU, rsbk::spec_bits(a.mu)) X(ERP, rsbk::spec_bits(a.erp)) X(ALPHA_INIT, rsbk::spec_bits(a.alpha_init)) X(ALPHA_MIN, rsbk::spec_bits(a.alpha_min)) \
  X(ALPHA_DECAY, rsbk::spec_bits(a.alpha_decay)) X(THRESHOLD, rsbk::spec_bits(a.threshold)) X(STALL_FACTOR, rsbk::spec_bits(a.stall_factor)) \
  X(MAX_ITER, a.max_iter) \
  X(COL_OWN, (a.col_own != 0))

#ifdef RSB_SPECIALIZED
#define RSB_DIM(NAME, expr) (RSB_SPEC_##NAME)
#else
#define RSB_DIM(NAME, expr) (expr)
#endif

// The contact solve's scalar settings (the fields from MU on): the default friction coefficient, ERP, the solver's relaxation (alpha_init, alpha_min, alpha_decay),
// its convergence threshold, stagnation factor and sweep limit.  They are fixed for a world's life in real use, and the sub-step loop read every one of them from
// the kernel arguments in every sub-step, at the solver's entry and in the contact columns: a scalar-cache round trip each, collected by an lgkmcnt(0) that also
// drains the LDS batch in flight around it (the coupling blocks, the FACT reads), and a live SGPR across the solve.  A float enters the key as its BIT PATTERN,
// written as a signed decimal integer (-0, denormals and NaN payloads are keys of their own); the kernel turns it back with a constexpr bit cast, so the value is a
// literal operand.  A world with any other value has another key: it runs its ahead-of-time class, or a code object of its own (rsb_spec.hip).
// -DRSB_X_NO_SPEC_CONSTS (RSB_SPEC_EXTRA_DEFS) reads the fields from the arguments again: same results bit for bit (tests/test_gpu_spec_consts.py).
// (The time step with gravity, and the ground height, were key fields in a first form and are not: they measured nothing, and their literals moved bits at three
//  sites that then had to be kept opaque - DESIGN.md sections 5.3 and 9.)
namespace rsbk {
constexpr int spec_bits(float f) { return __builtin_bit_cast(int, f); }
constexpr float spec_f32(int bits) { return __builtin_bit_cast(float, bits); }
}  // namespace rsbk
#if defined(RSB_SPECIALIZED) && !defined(RSB_X_NO_SPEC_CONSTS)
#define RSB_SPEC_CONSTS 1
#define RSB_DIM_F32(NAME, expr) (rsbk::spec_f32((int)(RSB_SPEC_##NAME)))
#define RSB_DIM_INT(NAME, expr) ((int)(RSB_SPEC_##NAME))
#else
#define RSB_SPEC_CONSTS 0
#define RSB_DIM_F32(NAME, expr) (expr)
#define RSB_DIM_INT(NAME, expr) (expr)
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

// Own-lane form of the plane's collision test (step_phase_collision.inc), in the code objects of the down pass's quad form whose world stands on the plane with a
// model that has no rim primitive and whose every collision primitive finds a (pass, lane) on a lane of its own body (StepArgs::col_own, the key field COL_OWN;
// rsb_world.hip: col_own_table).  Stage (3) of the down pass has just loaded Rb, rb of body s on lane s, of the base on lane 0 and on the lanes that are no body:
// a lane tests the primitives of ITS body with that pose - pc = rb + Rb pl, mat3_vec's expression - and the phase reads neither the primitive's table entry nor a
// body pose.  What a (pass, lane) tests - local centre, radius, primitive index, the lanes of every pass whose primitive has a lower index - is read from the
// table once per launch (with the prologue's global loads) and pinned in registers.  Every pass's depth test and ballot come first; a contact's slot is the number
// of hits on the lower-index lanes over all passes, so the contacts land in primitive order as before, and a slot >= kmax is dropped with flag bit 0 set.
// The centre stores for the self-collision sweep and the contact stores keep one exec-mask region each per pass (the region-free form with sink slots measured
// below them: DESIGN.md section 9).
// -DRSB_X_NO_COL_OWN compiles the primitive-order loop: same results bit for bit (tests/test_gpu_col_own.py).  The code objects of the down pass's quad form carry the comment lines `; rsb plane begin/end` around the plane branch, switch or not
// (tests/test_col_own_host.py counts between them).  The height map, a model with a cylinder and every other class compile what they compiled.
#if RSB_DOWN_QUADS && RSB_SPEC_COL_OWN && !defined(RSB_X_NO_COL_OWN)
#define RSB_COL_OWN 1
#if RSB_SPEC_TERRAIN != 0
#error "RSB_SPEC_COL_OWN: the own-lane collision test is the plane's"
#endif
#else
#define RSB_COL_OWN 0
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

// Lean seam between two control steps of ONE resident launch, in the specialised open-loop resident code objects of the quadruped classes (kernel class 64 at 16
// lanes per env and eight contact slots, a coordinate row of 17..32 and a q | u row of 33..48 floats: three row entries per lane, the targets' two): a control
// step that is not the launch's last leaves through step_phase_seam_lean.inc instead of the generic epilogue and boundary code (step_phase_epilogue.inc).  What is
// constant for the launch - the lane's row pointers into the observation block, the done flags, the target bank and the reset rows, the strides, the lane's
// obs_idx entry, do_reset, allowed - is formed once in front of the control-step loop (step_phase_seam_setup.inc); the seam itself has no trip loop and no scalar
// load: one batch of LDS reads with one wait, the stores, the foot forces handed from the contact lanes to the slot lanes by row broadcasts, the next targets
// requested at its top and stored at its end, the Delassus rows zeroed by unrolled stores.  Where the seam carry runs, its registers are refilled from LDS only
// behind a control step that reset an env of the wave.  The last control step, res_full launches, launches that ask for tau2_out / a reward / the task's
// observation or have no obs block or more force slots than lanes per env, the closed-loop classes (| 128, | 256), the humanoid, the ahead-of-time classes and
// every non-resident class run the generic code.
// -DRSB_X_NO_LEAN_SEAM compiles the code as it was: same results bit for bit (tests/test_gpu_lean_seam.py).
// (-DRSB_X_SEAM_BOUND is the deletion experiment that bounded this work - the lean path without the finite check, the obs and done stores, the zeroing and the target
//  reload; its results are wrong by design: profiles/lean_seam_bound.txt.)
// (The path reads nothing from the carried registers and does not ask for the seam carry or the quad forms: the switches of those - -DRSB_X_NO_DOWN_QUADS ... -
//  compare two forms of a tree pass, the same seam on both sides.)
#if defined(RSB_SPECIALIZED) && defined(RSB_I_CL) && (RSB_I_CL) == 64 && (RSB_I_LPE) == 16 && (RSB_I_KMAX) == 8 && RSB_SPEC_NQ > 16 && RSB_SPEC_NQ <= 32 && \
    RSB_SPEC_NQ + RSB_SPEC_NV > 32 && RSB_SPEC_NQ + RSB_SPEC_NV <= 48 && !defined(RSB_X_NO_LEAN_SEAM)
#define RSB_LEAN_SEAM 1
#else
#define RSB_LEAN_SEAM 0
#endif

// Flat contact form, in the specialised code objects of trees of at most four levels at 16 lanes per env, four factor levels and eight contact slots or fewer (the
// quadruped's lock-step, pipelined, resident and closed-loop classes): the contact columns (step_phase_columns.inc) and the impulse scatter that ends the solve
// (step_phase_solver.inc, W^T lam) without an exec-mask region per tree level.  Every `if (l < lev)` of those loops was a region with LDS traffic inside, which
// keeps its skip branch and its own lgkmcnt(0); in the usual wave every contact is a foot at the deepest level, every region is entered and no branch skips anything.
//   RSB_FLAT_COLUMNS  the level loop runs to the compile-time depth; a level the contact's body does not have reads the FACT row and the WB entry of body 1 (a child
//                     of the base in every tree: always valid, always written by this sub-step's up pass), its arithmetic runs, and its RESULTS are discarded by
//                     selects (never by a product with a zero: x - f * 0 turns -0 into +0, and a stale row may be non-finite); its column entry goes to the sink, a
//                     padding entry of the lane's own column that nobody reads (kFlatSink below).  No load sits in a region, so all of them can be in flight
//                     together.  Joint-limit rows and the J u record of a self-collision entry sit behind ONE wave-uniform branch.
//   RSB_FLAT_SCATTER  ONE region, the contact lanes'; inside it every read comes first and the three atomic adds are issued straight, in their level order; a level
//                     the body has no ancestor at (-1) adds onto the sink of the lane's own column instead (not a zero onto a live entry: lane order within an
//                     instruction, and so every sum, is what it was).  The lanes without a contact stay masked off: an LDS float atomic costs per ACTIVE lane, and
//                     the form that let them add onto a sink too - one for all of them, or one per lane - measured 4-5 % BELOW the regions.
// The form needs a padding entry in the column: cw = round4(6 + depth - 1) > 6 + depth - 1 (depth 2 and 4 of the depths up to 4).
// -DRSB_X_NO_FLAT_CONTACT compiles the code as it was, -DRSB_X_NO_FLAT_COLUMNS / -DRSB_X_NO_FLAT_SCATTER one part of it: same results bit for bit
// (tests/test_gpu_flat_contact.py).  RSB_FLAT_CLASS marks the code objects the form applies to, switch or not: they carry the comment lines `; rsb columns begin/end`
// and `; rsb scatter begin/end` in their assembly (tests/test_flat_contact_host.py counts between them).
#if defined(RSB_SPECIALIZED) && defined(RSB_I_LPE) && (RSB_I_LPE) == 16 && (RSB_I_KMAX) <= 8 && (RSB_I_ML) <= 4 && RSB_SPEC_DEPTH >= 2 && RSB_SPEC_DEPTH <= 4 && \
    RSB_SPEC_DEPTH <= (RSB_I_ML) && ((6 + RSB_SPEC_DEPTH - 1 + 3) & ~3) > 6 + RSB_SPEC_DEPTH - 1
#define RSB_FLAT_CLASS 1
#else
#define RSB_FLAT_CLASS 0
#endif
#if RSB_FLAT_CLASS && !defined(RSB_X_NO_FLAT_CONTACT)
#define RSB_FLAT_CONTACT 1
#else
#define RSB_FLAT_CONTACT 0
#endif
#if RSB_FLAT_CONTACT && !defined(RSB_X_NO_FLAT_COLUMNS)
#define RSB_FLAT_COLUMNS 1
#else
#define RSB_FLAT_COLUMNS 0
#endif
#if RSB_FLAT_CONTACT && !defined(RSB_X_NO_FLAT_SCATTER)
#define RSB_FLAT_SCATTER 1
#else
#define RSB_FLAT_SCATTER 0
#endif
#if RSB_FLAT_CLASS
namespace rsbk {
// the sink: the last entry of a contact column [z 0..5 | levels 1..depth-1 | padding].  Nothing reads the padding: the scatter and the Delassus rows stop at 5 + depth - 1.
constexpr int kFlatCw = (6 + RSB_SPEC_DEPTH - 1 + 3) & ~3, kFlatSink = kFlatCw - 1;
static_assert(kFlatSink >= 6 + RSB_SPEC_DEPTH - 1 && kFlatSink < kFlatCw, "flat contact form: the sink must be a padding entry of the column");
}  // namespace rsbk
#endif

// Flat set-up and end of the contact solve (step_phase_solver.inc), in the same code objects (row-block Delassus layout, energy slip rule).  A launch of these classes is
// one wave per SIMD: nothing hides an LDS round trip, and the set-up was a CHAIN of them - the contact record's body, that body's level, its ancestor; the record's
// collision id (a second read, in its own exec-mask region), the primitive's friction coefficient, its warm row - with the coupling blocks, which only the lane index
// addresses, issued behind all of it.  The end re-read the record's body and its ancestor row behind the row sums.
//   RSB_FLAT_SETUP_HEAD  two batches and no region.  Batch A: everything the lane index addresses (own block, inverse, velocity, floats 4-11 of the contact record as
//                        two 16-byte reads, the five coupling blocks), read by every lane at the clamped slot.  Batch B, behind one wait: PARLV and the ancestor row of
//                        the record's body, the friction coefficient and the warm row at a clamped primitive.  Selects then take or drop the RESULTS (a dropped warm
//                        row is never multiplied by a zero: it may hold anything).  The self-collision's relabelling and its SELFT read stay behind their one
//                        wave-uniform test.  The warm table is cleared by straight stores (a compile-time trip count, the last index clamped).  The ancestor row stays
//                        in registers for the end.  With it the Delassus loop's column bound is the tree's depth, not the class's level capacity.
//   RSB_FLAT_SETUP_END   (beside RSB_FLAT_SCATTER) one batch of reads in front of the row sums - the column rows with their level-3 entries, and the ancestor row
//                        where the set-up did not keep it - and ONE region of the contact lanes with the impulse stores, the warm record and the three atomics.
// -DRSB_X_NO_FLAT_SETUP compiles the code as it was, -DRSB_X_NO_FLAT_SETUP_HEAD / -DRSB_X_NO_FLAT_SETUP_END one part of it: same results bit for bit
// (tests/test_gpu_flat_setup.py).  The code objects of RSB_FLAT_CLASS carry the comment lines `; rsb setup begin/end` and `; rsb solver end begin/end`, switch or not
// (tests/test_flat_setup_host.py counts between them).
// The fixed-base classes (| 1) do not take the form: which product of the scatter's three-term sums the compiler leaves unfused is its choice per code object, and in the
// fixed-base class of a two-level tree the end's form came out one rounding away from the code it replaces (15 entries of u after four steps of
// tests/test_gpu_solver_handover.py's model; the quadruped's classes keep every bit: tests/test_gpu_flat_setup.py).  A fixed-base world is no quadruped.
#if RSB_FLAT_CLASS && !((RSB_I_CL) & (32 | 1)) && !defined(RSB_X_G_SQUARE) && !defined(RSB_X_NO_FLAT_SETUP)
#define RSB_FLAT_SETUP 1
#else
#define RSB_FLAT_SETUP 0
#endif
#if RSB_FLAT_SETUP && !defined(RSB_X_NO_FLAT_SETUP_HEAD)
#define RSB_FLAT_SETUP_HEAD 1
#else
#define RSB_FLAT_SETUP_HEAD 0
#endif
#if RSB_FLAT_SETUP && RSB_FLAT_SCATTER && !defined(RSB_X_NO_FLAT_SETUP_END)
#define RSB_FLAT_SETUP_END 1
#else
#define RSB_FLAT_SETUP_END 0
#endif

// Flat form of the Delassus phase's pair loop (step_phase_delassus.inc), in the code objects of the flat set-up that also carry RSB_SPEC_UP_QUADS (eight contact slots,
// four consecutively numbered chains of equal length: the quadruped).  A trip of the pair loop - the first one holds every pair of an env with at most five contacts -
// was a chain of round trips in front of the reads that matter: the two contact records' bodies, their levels, their ancestor rows, and only then the two columns'
// rows, whose addresses depend on the pair index alone; behind the arithmetic a region each for the joint-limit diagonal (with a dependent read), the transposed
// store and the inverse.
//   - (i, j) of pair s of the FIRST trip, the offsets of its two columns and of its three stores are functions of the lane: formed once per launch and pinned
//     (step_kernel.h: fd_*).  A later trip (more than five contacts in an env of the wave) decodes its pairs with the square root at the loop's back edge, which the
//     usual wave never takes, and runs the same body: one copy of the code, so the kernel holds no more LDS instructions than it did;
//   - ONE batch of reads by every lane: the rows of columns i and j, floats 7 and 15 of record i, float 7 of record j.  A lane whose pair its env does not have
//     (j >= nc) reads pair (0, 0); no load sits behind a condition;
//   - the shared prefix of the two support chains is a closed form of the two body indices: limb (b - 1) / NL, level (b - 1) % NL + 1, lca = min of the levels on one
//     limb and 0 otherwise.  rsb_world.hip (delassus_closed_form_ok) compares the form with the parent / level tables for every body pair before it reports the
//     model as four equal chains (StepArgs::chain == 2, the key field UP_QUADS); a model the form does not describe never gets such a code object;
//   - the joint-limit diagonal is a select on the flag read with the batch; a diagonal pair's transposed store writes the same bits to the same address as the block
//     itself (both operands of every product are the same column), so it has no test; every lane computes the inverse; a lane without a pair, or off the diagonal,
//     stores to a sink: the 64 floats of the Delassus region behind the block rows.  Blocks the loop does not write stay what they were;
//   - the inverse's contractions are written out as the loop compiles them (which product of the determinant stays unfused is the compiler's choice per context,
//     and it chose another one for the straight form: one rounding in every inverse).
// The self-collision fold behind the loop is what it was.
// -DRSB_X_NO_FLAT_DELASSUS compiles the code as it was: same results bit for bit (tests/test_gpu_flat_delassus.py).  The code objects of RSB_FLAT_CLASS carry the
// comment lines `; rsb delassus begin/end` around the pair loop, switch or not (tests/test_flat_delassus_host.py counts between them).
// (A model of RSB_FLAT_CLASS that is not four equal chains keeps the loop: the second batch of reads such a model needs - PARLV and the two ancestor rows - is not
//  written; no shipped workload has such a model.)
// (The form goes with the flat set-up: -DRSB_X_NO_FLAT_SETUP compiles the set-up, the end AND the pair loop as they were - that switch's twin stays the code it was;
//  the set-up's part switches leave the pair loop flat.)
#if RSB_FLAT_SETUP && (RSB_I_KMAX) == 8 && RSB_SPEC_UP_QUADS && !defined(RSB_X_NO_FLAT_DELASSUS)
#define RSB_FLAT_DELASSUS 1
#else
#define RSB_FLAT_DELASSUS 0
#endif

// Packed fp32 form of the contact solve's arithmetic, in the specialised code objects of the quadruped classes (16 lanes per env, eight contact slots or fewer, the
// energy slip rule: lock-step, pipelined, resident and closed-loop).  Such a launch is one wave per SIMD, and a lone wave pays ~4 cycles for every VALU instruction
// it issues whatever the instruction does (profiles/r02_ubench_lone_wave_latency.txt), so two fp32 operations that share an operand pattern are written as ONE
// v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 on a register pair, as the impulse exchange already does.  The packed instructions round each half as their scalar
// twins do; which products are fused is written out with explicit FMAs, read off the assembly of the scalar form (step_slip_pk.h), so the results are the same bits.
// What is packed is the sweep loop (step_phase_solver.inc): the own block is held as the column pairs (G0,G3) (G1,G4) (G2,G5) - the pairs the row-block layout
// stores - and row 2, its inverse's rows 0 | 1 likewise, mu * G_tt as (n01,n11) (n02,n12); the stick impulse ls[0|1], the tangential velocity vex0|vex1 and the
// coefficients kc.n0k|n1k of a direction refresh, the Newton step's N0|N1, dN0|dN1, (P, Q) and the two sums of h', the rotation with its normalisation, the energy
// check's vt0|vt1 and products, and the impulse update ln|dl|lam[0|1] are pairs.  den, mdp, h, the reciprocals, the guards and every select stay scalar.
// (Two more parts were built and are not here: the quad basin scan through the packed slip_E put the resident class 40 bytes into scratch, and the Delassus
//  accumulation on pairs measured nothing - DESIGN.md section 9.)
// -DRSB_X_NO_PK_SOLVE compiles the scalar instructions: same results bit for bit (tests/test_gpu_pk_solve.py).  RSB_PK_CLASS marks the code objects the form applies
// to, switch or not: they carry the comment lines `; rsb sweep begin/end` in their assembly (tests/test_pk_solve_host.py counts between them).  The ahead-of-time
// classes, the humanoid (KMAX 16) and the Coulomb classes (| 32) compile what they compiled.
#if defined(RSB_SPECIALIZED) && defined(RSB_I_LPE) && (RSB_I_LPE) == 16 && (RSB_I_KMAX) <= 8 && !((RSB_I_CL) & 32)
#define RSB_PK_CLASS 1
#else
#define RSB_PK_CLASS 0
#endif
#if RSB_PK_CLASS && !defined(RSB_X_NO_PK_SOLVE)
#define RSB_PK_SOLVE 1
#else
#define RSB_PK_SOLVE 0
#endif
// (One more part was built and is not here: a running copy of the env's normal impulses on every lane, fed by the exchange's broadcasts, in place of the sweep
//  epilogue's row_max - same bits, and it measured nothing beside the flat Delassus form and -0.9 % without it: DESIGN.md section 9.)

// Sweep control, in the code objects of the packed solve: the sweep loop's body runs about four times per sub-step in a lone wave, and every branch it holds costs
// that wave 20-55 cycles taken or not (profiles/r02_ubench_lone_wave_latency.txt).  Two parts (step_phase_solver.inc, step_slip_pk.h):
//   RSB_SWEEP_RARE  the direction refresh's three continuations - the energy check of a step above 0.02 rad, the basin check of an inherited direction in the first
//                   sweep, the global search of a contact whose step was refused - sit behind ONE wave-uniform test, formed behind the Newton step's core (den0, the
//                   step, the rotation, den1, the four guards; slip_newton_core_pk).  False, the usual case of a later sweep: the step is taken by the selects and the
//                   pass falls through to the magnitude, no further branch, region or wait.  True: the code as it was, with its own inner tests.  The arithmetic of
//                   both halves is untouched, and a lane that did not ask for a refresh never uses its verdict: the same bits.
//   RSB_SWEEP_LOOP  the pass count, the pass counter and the sweep counter are pinned in scalar registers and the two loops are bottom-tested: "another pass of this
//                   sweep" is s_cmp + s_cbranch_scc, "another sweep" one test of the lanes not yet done with the max_iter bound folded into its mask.  Between the
//                   exchange and the next pass's rule these are the only branches of the usual path.
// -DRSB_X_NO_SWEEP_CONTROL compiles the code as it was, -DRSB_X_NO_SWEEP_CONTROL_RARE / -DRSB_X_NO_SWEEP_CONTROL_LOOP one part of it: same results bit for bit
// (tests/test_gpu_sweep_control.py).  The code objects of the form carry the comment lines `; rsb refresh fast begin/end` and `; rsb sweep control begin/end`
// (tests/test_sweep_control_host.py counts between them).  Every other class compiles what it compiled.
// -DRSB_X_SWEEP_COUNTERS compiles twelve counters into the profiling twin (what followed each Newton block, first | later sweeps: rsb_debug_wave_sweep_control,
// tools/diag_waves.py); without it the twin's stamps time the code the other twins time.
#if RSB_PK_SOLVE && !defined(RSB_X_NO_SWEEP_CONTROL)
#define RSB_SWEEP_CONTROL 1
#else
#define RSB_SWEEP_CONTROL 0
#endif
#if RSB_SWEEP_CONTROL && !defined(RSB_X_NO_SWEEP_CONTROL_RARE)
#define RSB_SWEEP_RARE 1
#else
#define RSB_SWEEP_RARE 0
#endif
#if RSB_SWEEP_CONTROL && !defined(RSB_X_NO_SWEEP_CONTROL_LOOP)
#define RSB_SWEEP_LOOP 1
#else
#define RSB_SWEEP_LOOP 0
#endif

namespace rsbk {
#define RSB_SPEC_COUNT_ONE(NAME, expr) +1
constexpr int kSpecFields = 0 RSB_SPEC_FIELDS(RSB_SPEC_COUNT_ONE);
#undef RSB_SPEC_COUNT_ONE
}  // namespace rsbk
