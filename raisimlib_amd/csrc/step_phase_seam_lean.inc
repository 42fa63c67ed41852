// step_phase_seam_lean.inc — fragment of rsb_step_kernel (step_kernel.h), lean seam (step_spec.h: RSB_LEAN_SEAM): the epilogue and the boundary of a control step
// that is not the resident launch's last, for the open-loop quadruped classes.  Every float written is the expression of step_phase_epilogue.inc, which stays the
// reference (-DRSB_X_NO_LEAN_SEAM) and runs the launch's last control step: nothing but the observation block and the done flags leaves the chip here.
  {
    asm volatile("; rsb lean seam begin");     // (comment lines in the assembly: tests/test_lean_seam_host.py counts the path's instructions between them)
    // the observation's q | u entries are one row of nq + nv floats: the lane takes entries s, s + 16 and s + 32 of it (the last one clamped: no load is predicated)
    constexpr int kRow = RSB_SPEC_NQ + RSB_SPEC_NV;
    static_assert(RSB_SPEC_NQ > LPE && RSB_SPEC_NQ <= 2 * LPE && kRow > 2 * LPE && kRow <= 3 * LPE, "the lean seam's share of a row: three entries per lane, the targets' two");
    const int i_b = s + LPE, i_c = min(s + 2 * LPE, kRow - 1), i_t = min(s + LPE, nq - 1);
    const bool has_c = s + 2 * LPE < kRow, has_t = s + LPE < nq;
    // ---- the next control step's target row is requested first: its latency passes behind everything below
#ifndef RSB_X_SEAM_BOUND
    const float tg_a = ls_tg[s], tg_b = ls_tg[i_t];
#endif
    // ---- ONE batch of LDS reads, one wait: the lane's share of q and u, its contact's frame rows and impulse (lanes past the contacts read the last slot)
    nc = nc_real;                              // joint-limit rows are not contacts
    if (dead) nc = nc_dead;                    // the contacts that ended the episode
    const int ks = min(s, KMAX - 1);
    const float o_a = Q[s], o_b = *(i_b < nq ? Q + i_b : U + (i_b - nq)), o_c = U[i_c - nq];
    float c4[4], c8[4], c12[4];
    ld4(CON + ks * kConSlot + 4, c4); ld4(CON + ks * kConSlot + 8, c8); ld4(CON + ks * kConSlot + 12, c12);
    const float l0 = LAM[3 * ks], l1 = LAM[3 * ks + 1], l2 = LAM[3 * ks + 2];
    // ---- termination rule (the epilogue's): a non-finite state, or anything but an allowed primitive touching the terrain
    // (bit operations, not && and ||: a short circuit is a branch, and a branch costs the lone wave more than the compare it skips)
#ifndef RSB_X_SEAM_BOUND
    const bool bad = !isfinite(o_a) | !isfinite(o_b) | (has_c & !isfinite(o_c));
#else
    const bool bad = false;
#endif
    const int kid = __float_as_int(c8[3]);     // collision id of the lane's contact
    const int mycol = s < nc ? kid : 0;
    const bool illegal = (ls_do_reset != 0) & (s < nc) & ((mycol >= kSelfA) | !((ls_allowed >> mycol) & 1ull));
    const unsigned long long bb_ = __ballot(bad), bi_ = __ballot(illegal);
    const unsigned long long gsel = ((1ull << LPE) - 1ull) << (el * LPE);
    const bool term = env_valid & (ls_do_reset != 0) & (((bb_ | bi_) & gsel) != 0);
#ifndef RSB_X_SEAM_BOUND
    // ---- observation: q, u, then the force on every slot's primitive.  Contact lane k forms its force once - the products rounded and fused as the epilogue's loop
    // has them: c8 l1 rounded, c4 l0 and c12 l2 fused onto it - and the slot lanes pick theirs by collision id from row broadcasts, in contact order, each one
    // fma(inv_dt, sum, f) onto a force that starts at zero (a product alone would differ in the sign of a zero)
    float fs[3], ff[3] = {0.f, 0.f, 0.f};
    {
#pragma clang fp contract(off)
      RSB_UNROLL for (int j = 0; j < 3; ++j) fs[j] = __builtin_fmaf(c12[j], l2, __builtin_fmaf(c4[j], l0, c8[j] * l1));
    }
    static_for<0, KMAX>([&](auto K) {
      constexpr int k = decltype(K)::value;
      const int kid_k = __float_as_int(row_bcast<k>(__int_as_float(kid)));
      const bool hit = (k < nc) & (kid_k == ls_want);
      RSB_UNROLL for (int j = 0; j < 3; ++j) {
        const float f = __builtin_fmaf(ls_inv_dt, row_bcast<k>(fs[j]), ff[j]);
        ff[j] = hit ? f : ff[j];
      }
    });
    if (env_valid) {
      ls_obs[s] = o_a;
      ls_obs[i_b] = o_b;
      if (has_c) ls_obs[s + 2 * LPE] = o_c;
      if (s < ls_slots) { rsb_gf32* fo = ls_obs + nq + nv + 3 * s; fo[0] = ff[0]; fo[1] = ff[1]; fo[2] = ff[2]; }
      if ((s == 0) & (ls_has_done != 0)) *ls_done = term ? 1 : 0;
    }
#endif
    // ---- boundary (the epilogue's, in LDS).  A reset is rare: one uniform branch keeps its loops out of the way, and only then are the carried registers stale
    const bool redo = __ballot(term || dead) != 0;
    if (redo) {
      if (term) {
        for (int i = s; i < nq; i += LPE) Q[i] = ls_gc0[i];
        for (int i = s; i < nv; i += LPE) U[i] = ls_gv0[i];
      }
      if ((term || dead) && has_warm) for (int i = s; i < nwarm; i += LPE) WARM[i] = 0.f;
    }
#ifndef RSB_X_SEAM_BOUND
    PT[s] = tg_a;
    if (has_t) PT[s + LPE] = tg_b;
    if (ls_keep && cs + 2 == ncs) {            // the world's own copy of the PD targets: the last control step's
      ls_pts[s] = tg_a;
      if (has_t) ls_pts[s + LPE] = tg_b;
    }
    {
      // (the first sub-step of a control step meets zeros in the Delassus rows: 3 KMAX rows of 4 KMAX + 4 floats, rsb_world.hip: make_layout_pitch)
      const float z4[4] = {0.f, 0.f, 0.f, 0.f};
      constexpr int gfloats = 3 * KMAX * (4 * KMAX + 4), gfull = gfloats / (4 * LPE);
      RSB_UNROLL for (int t = 0; t < gfull; ++t) st4(G + 4 * s + 4 * LPE * t, z4);
      if (gfull * 4 * LPE + 4 * s < gfloats) st4(G + 4 * s + 4 * LPE * gfull, z4);
    }
#endif
    flag = 0; iters_used = 0; nc = 0; nc_real = 0; nselfc = 0; dead = false; nc_dead = 0;
    pbx = pby = pbz = 0.f;
    // the lane's rows of the next control step
    ls_obs += ls_obs_stride; ls_done += ls_done_stride;
    ++ls_slice;
    const bool wrap = ls_slice == ls_period;
    ls_slice = wrap ? 0 : ls_slice;
    ls_tg = wrap ? ls_tg0 : ls_tg + ls_tg_stride;
    seam_refill = redo;
    __syncthreads();
    asm volatile("; rsb lean seam end");
  }
