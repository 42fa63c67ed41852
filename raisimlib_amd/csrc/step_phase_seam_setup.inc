// step_phase_seam_setup.inc — fragment of rsb_step_kernel (step_kernel.h), lean seam (step_spec.h: RSB_LEAN_SEAM): what the seam between two control steps needs
// and the launch does not change, formed ONCE in front of the control-step loop
  // Every value is pinned in its register behind the one wait (the empty asm): left alone, the register allocator re-reads a kernel argument where it is used - a
  // scalar-cache round trip per argument and control step, which is what this path is there to remove (as with the control-step count above).
  RSB_ARGS(al);
  static_assert(!TRI && LPE == 16 && KMAX == 8 && !PROF && STG == 0, "the lean seam is written for the open-loop quadruped classes: one env per DPP row, eight contact lanes (step_spec.h)");
  const int ls_slots_ld = al.obs_slots;
  // launches this path does not serve run the generic epilogue in every control step (ls_ok: wave-uniform, constant for the launch)
  // (the four switches are formed in a vector register and read back from it: formed as scalar compares the instruction selector leaves them in a lane mask, which
  //  no scalar register can be pinned to)
  int ls_sw = (al.res_full == 0 && al.obs_out != nullptr && al.tau2_out == nullptr && al.env_reward == nullptr && al.env_ob == nullptr &&
               ls_slots_ld <= LPE && al.res_targets != nullptr && al.res_period > 0 ? 1 : 0) | (al.do_reset != 0 ? 2 : 0) | (al.ptarget_store != nullptr ? 4 : 0) | (al.done_out != nullptr ? 8 : 0);
  asm volatile("" : "+v"(ls_sw));
  ls_sw = __builtin_amdgcn_readfirstlane(ls_sw);
  int ls_ok = ls_sw & 1, ls_do_reset = ls_sw & 2, ls_keep = ls_sw & 4, ls_has_done = ls_sw & 8;
  unsigned long long ls_allowed = al.allowed;
  int ls_period = al.res_period;
  // the bank slice of the NEXT control step: the one 64-bit remainder of the launch (vector arithmetic, hence the readfirstlane); it advances by increment and compare
  long long ls_next = al.res_first + 1, ls_per64 = ls_ok ? ls_period : 1;
  asm volatile("" : "+v"(ls_next), "+v"(ls_per64));
  int ls_slice = __builtin_amdgcn_readfirstlane((int)(ls_next % ls_per64));
  long long ls_obs_stride = al.res_obs_stride, ls_done_stride = al.res_done_stride;
  long long ls_tg_stride = (long long)al.N * nq;                      // floats between two slices of the target bank
  asm volatile("" : "+s"(ls_ok), "+s"(ls_do_reset), "+s"(ls_keep), "+s"(ls_has_done), "+s"(ls_allowed), "+s"(ls_period), "+s"(ls_slice));
  asm volatile("" : "+s"(ls_obs_stride), "+s"(ls_done_stride), "+v"(ls_tg_stride));   // (the 64-bit product is vector arithmetic)
  const int ls_slots = ls_slots_ld;
  // the lane's rows: observation block and done flag of control step 0, target bank (slice 0 and the next control step's), reset rows, the world's target copy
  // (typed as global pointers: behind the pin the compiler no longer sees where a pointer came from, and a generic one costs flat instructions)
  typedef __attribute__((address_space(1))) float rsb_gf32;
  typedef __attribute__((address_space(1))) const float rsb_gcf32;
  typedef __attribute__((address_space(1))) uint8_t rsb_gu8;
  rsb_gf32* ls_obs = (rsb_gf32*)(al.obs_out + (size_t)env * (nq + nv + 3 * ls_slots));
  rsb_gu8* ls_done = (rsb_gu8*)(al.done_out + env);
  rsb_gcf32* ls_tg0 = (rsb_gcf32*)(al.res_targets + (size_t)env * nq);
  rsb_gcf32* ls_tg = ls_tg0 + (size_t)ls_slice * (size_t)ls_tg_stride;
  const size_t ls_r0 = (al.reset_rows == 1) ? 0 : (size_t)env;
  rsb_gcf32* ls_gc0 = (rsb_gcf32*)(al.gc0 + ls_r0 * nq);
  rsb_gcf32* ls_gv0 = (rsb_gcf32*)(al.gv0 + ls_r0 * nv);
  rsb_gf32* ls_pts = (rsb_gf32*)(al.ptarget_store + (size_t)env * nq);
  int ls_want = s;                                                    // the collision primitive of the lane's force slot
  if (al.obs_idx && s < ls_slots) ls_want = al.obs_idx[s];
  asm volatile("" : "+v"(ls_obs), "+v"(ls_done), "+v"(ls_tg0), "+v"(ls_tg), "+v"(ls_gc0), "+v"(ls_gv0), "+v"(ls_pts), "+v"(ls_want));
  const float ls_inv_dt = 1.0f / dt;
  bool seam_refill = true;   // the carried registers are (re)filled from LDS at the top of the next control step
