// step_phase_update.inc — fragment of rsb_step_kernel: du = L^-1 D^-1/2 (W_b + sum_c W_c lam_c) root -> leaves, then the position update of the integration scheme
    // =========================== du = L^-1 D^-1/2 (W_b + sum_c W_c lam_c), then integrate ========
    // base part on every lane (C^T x = w by back substitution), then the bodies level by level from the base (lane = body)
    float a0[6];
    // integration scheme of the positions (StepArgs::integ_theta; rsb_set_integration_scheme).  Schemes other than semi-implicit Euler are a kernel
    // class of their own (bit 8): the four instructions they add here moved the register allocation of the whole sub-step (-0.9 % on config 2,
    // same-box A/B) - in every other class theta is the constant 1 and the code below folds to what it was
    float theta = 1.f;
    if constexpr (TH) { RSB_ARGS(ai); theta = ai.integ_theta; }
    {
      float wv[6];
      RSB_UNROLL for (int i = 0; i < 6; ++i) wv[i] = wbb[i];
      RSB_UNROLL for (int i = 0; i < 6; ++i) wv[i] += wlam[i];   // base part of sum_c W_c lam_c (zero without contacts)
      float x[6];
      RSB_UNROLL for (int ii = 0; ii < 6; ++ii) {
        const int i = 5 - ii;
        float sacc = wv[i];
        RSB_UNROLL for (int k = i + 1; k < 6; ++k) sacc -= C[sym6(k, i)] * x[k];
        x[i] = sacc * idg[i];
      }
      a0[0] = x[3]; a0[1] = x[4]; a0[2] = x[5]; a0[3] = x[0]; a0[4] = x[1]; a0[5] = x[2];
#if RSB_SEAM_BASE
      // seam carry (step_spec.h): the base's q and u are in registers, so lane 0 has nothing to load here; what it stores it also keeps, and the thirteen values
      // reach the other lanes of the env's row by row_bcast<0> moves behind the region (below): no load and no wait at the top of the next sub-step.
      // The alternative - every lane evaluating the update itself, which would cost no register more, the registers being the wave's - does not give the same bits:
      // the solver's row sums leave every lane a sum in an order of its own (step_slip.h, row_sum_f32), so x differs from lane to lane in its last bits, and
      // the base's state is lane 0's.  Thirteen DPP moves against a store, a barrier and a load.
      if (s == 0 && !dead) {
        const float* qv = sc_qv; const float* uv = sc_uv;
#else
      if (s == 0 && !dead) {
        float qv[8], uv[8];
        ldv<2>(Q, qv); ldv<2>(U, uv);
#endif
        float un[6], up[6];
        RSB_UNROLL for (int i = 0; i < 6; ++i) { un[i] = uv[i] + x[i]; up[i] = TH ? fmaf(theta, x[i], uv[i]) : un[i]; }   // up: the velocity the positions move with
        // q+ : position, quaternion (world-frame angular velocity); theta = 1: semi-implicit Euler
        const float wn = sqrtf(up[3] * up[3] + up[4] * up[4] + up[5] * up[5]);
        const float half = 0.5f * wn * dt;
        float sh, chf;
        fast_sincos(half, &sh, &chf);
        const float sc = (wn > 1e-12f) ? sh / wn : 0.5f * dt;
        const float d0 = chf, d1 = sc * up[3], d2 = sc * up[4], d3 = sc * up[5];
        const float q0 = qv[3], q1 = qv[4], q2 = qv[5], q3 = qv[6];
#if RSB_SEAM_BASE
        // (the quaternion product written out as the compiler contracts the four expressions of the #else branch where q is loaded from LDS - the d1 product
        //  rounded, the others fused onto it one by one; with q in registers it picks other products to round, and the last bits move)
        float r0 = fmaf(-d3, q3, fmaf(-d2, q2, fmaf(d0, q0, -(d1 * q1))));
        float r1 = fmaf(-d3, q2, fmaf(d2, q3, fmaf(d0, q1, d1 * q0)));
        float r2 = fmaf(d3, q1, fmaf(d2, q0, fmaf(d0, q2, -(d1 * q3))));
        float r3 = fmaf(d3, q0, fmaf(-d2, q1, fmaf(d0, q3, d1 * q2)));
#else
        float r0 = d0 * q0 - d1 * q1 - d2 * q2 - d3 * q3;
        float r1 = d0 * q1 + d1 * q0 + d2 * q3 - d3 * q2;
        float r2 = d0 * q2 - d1 * q3 + d2 * q0 + d3 * q1;
        float r3 = d0 * q3 + d1 * q2 - d2 * q1 + d3 * q0;
#endif
        const float in = 1.0f / sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
        // joint entries of Q / U are owned by the body lanes: write only the base entries
#if RSB_SEAM_BASE
        const float qn[7] = {qv[0] + dt * up[0], qv[1] + dt * up[1], qv[2] + dt * up[2], r0 * in, r1 * in, r2 * in, r3 * in};
        RSB_UNROLL for (int i = 0; i < 7; ++i) Q[i] = qn[i];
        RSB_UNROLL for (int i = 0; i < 6; ++i) U[i] = un[i];
        RSB_UNROLL for (int i = 0; i < 7; ++i) sc_qv[i] = qn[i];      // (a dead env keeps its old values, as its rows of Q and U do)
        RSB_UNROLL for (int i = 0; i < 6; ++i) sc_uv[i] = un[i];
#else
        Q[0] = qv[0] + dt * up[0]; Q[1] = qv[1] + dt * up[1]; Q[2] = qv[2] + dt * up[2];
        Q[3] = r0 * in; Q[4] = r1 * in; Q[5] = r2 * in; Q[6] = r3 * in;
        RSB_UNROLL for (int i = 0; i < 6; ++i) U[i] = un[i];
#endif
      }
#if RSB_SEAM_BASE
      RSB_UNROLL for (int i = 0; i < 7; ++i) sc_qv[i] = row_bcast<0>(sc_qv[i]);      // (lane 0's new - or, of a dead env, old - values to the sixteen lanes of the env)
      RSB_UNROLL for (int i = 0; i < 6; ++i) sc_uv[i] = row_bcast<0>(sc_uv[i]);
#endif
    }
    // joints, level by level from the base: a body takes its parent's delta-velocity from LDS (the A slot of the parent's
    // BODY entry, free since the down pass), resolves its own joint and leaves its own for its children
#if defined(RSB_SPECIALIZED) && RSB_SPEC_CHAIN
    // serial chains numbered consecutively (StepArgs::chain): the parent of a body of level >= 2 is the lane below - its delta-velocity arrives by a DPP row
    // shift (six moves) instead of through the parent's BODY slot (two stores, the barrier, two loads: two LDS round trips per level of a lone wave)
    {
#if RSB_UP_QUADS
      // (quad form of the up pass: no body lane holds its joint's factors in registers - they come back from the FACT slot, which holds the same bits)
      float bUD[6], brsD;
#if RSB_DOWN_QUADS
      float bS[6];
#endif
      {
        float Fk[16];
        ldv<4>(FACT + bb * kFactSlot, Fk);
        RSB_UNROLL for (int i = 0; i < 6; ++i) bUD[i] = Fk[6 + i];
        brsD = Fk[12];
#if RSB_DOWN_QUADS
        RSB_UNROLL for (int i = 0; i < 6; ++i) bS[i] = Fk[i];      // (quad form of the down pass: the joint axis too)
#endif
      }
#endif
      float an[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};    // this body's own delta-velocity once its level has run
      RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
        float ap[6];
        RSB_UNROLL for (int i = 0; i < 6; ++i)
          ap[i] = (lv == 1) ? a0[i] : __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(an[i]), 0x111, 0xf, 0xf, true));   // row_shr:1
        if (mylev == lv) {
          const float xk = brsD * WB[bb + 5] - dot6(bUD, ap);   // WB = W_b plus the contact contributions scattered by the contact lanes
          const float un = bqd + xk;
#if RSB_SEAM_JOINTS
          const float qn = bqb + dt * (TH ? fmaf(theta, xk, bqd) : un);
          if (!dead) {
            U[bb + 5] = un;
            Q[bb + 6] = qn;
            sc_qd = un; sc_q = qn;      // (seam carry: what the lane stored is the next sub-step's bqd, bqb; a dead env's lanes keep their old ones)
          }
#else
          if (!dead) {
            U[bb + 5] = un;
            Q[bb + 6] = bqb + dt * (TH ? fmaf(theta, xk, bqd) : un);
          }
#endif
          RSB_UNROLL for (int i = 0; i < 6; ++i) an[i] = ap[i] + bS[i] * xk;
        }
      }
      // (seam carry: with the base's and the joints' state crossing in registers, the top of the next sub-step no longer reads what this pass stored.  The barrier
      //  stays: behind the LAST sub-step the epilogue reads Q and U - and, of a wave without contacts, the cleared warm table - across lanes; and in such a wave, where
      //  no barrier follows the up pass, it stands between the base gather's reads of UPS slot 0 and the next down pass's staging stores to the same floats.  A form
      //  with this barrier moved onto the down pass's wait for the MODELF batch was built and gave the same bits; it needs a second barrier behind the sub-step loop
      //  for the epilogue, and whether it is any faster was not measured against this form: DESIGN.md section 11.)
      __syncthreads();
    }
#else
    for (int lv = 1; lv < depth; ++lv) {
      if (mylev == lv) {
        float t6[8], ap[6];
        ld4(BODY + mypar * kBodySlot + 16, t6); ld4(BODY + mypar * kBodySlot + 20, t6 + 4);
        RSB_UNROLL for (int i = 0; i < 6; ++i) ap[i] = (mypar == 0) ? a0[i] : t6[2 + i];   // the base's is in registers on every lane
        const float xk = brsD * WB[bb + 5] - dot6(bUD, ap);   // WB = W_b plus the contact contributions scattered by the contact lanes
        const float un = bqd + xk;
        if (!dead) {
          U[bb + 5] = un;
          Q[bb + 6] = bqb + dt * (TH ? fmaf(theta, xk, bqd) : un);
        }
        if ((mykid >> 16) > 0) {
          float* Ab = BODY + bb * kBodySlot + 18;
          RSB_UNROLL for (int i = 0; i < 6; ++i) Ab[i] = ap[i] + bS[i] * xk;
        }
      }
      __syncthreads();
    }
#endif
    RSB_STAMP(7)
    if (PROF && a.prof && blockIdx.x == 0 && lane == 0 && sub == a.nsub - 1) { a.prof[8] = iters_used; a.prof[9] = ncw; }
