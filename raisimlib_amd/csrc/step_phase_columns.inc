// step_phase_columns.inc — fragment of rsb_step_kernel (inside `if (ncw > 0)`): contact columns W_c = D^-1/2 L^-T J_c^T (lane = (contact, axis))
      // ========================= contact columns (lane = column): W_c = D^-1/2 L^-T J_c^T =======
#if RSB_FLAT_CLASS
      asm volatile("; rsb columns begin");     // (comment lines in the assembly: tests/test_flat_contact_host.py counts the phase's instructions between them)
#endif
      for (int c0 = 0; c0 < 3 * ncw; c0 += LPE) {
        const int c = c0 + s;
#if RSB_FLAT_COLUMNS
        // flat form (step_spec.h): no exec region but this one in the common path - no load below sits behind a condition, so the FACT rows of all levels, the WB
        // entries, the body's velocity, the material and the ancestor row are free to be in flight together; a level the body does not have is computed on body 1's
        // row and discarded by selects on the results; every float keeps the expression it has in the code below
        if (c < 3 * nc) {
          constexpr int NL = RSB_SPEC_DEPTH - 1;     // levels below the base
          const int i = c / 3, rr = c - 3 * i;
          float CN[16];
          ldv<4>(CON + i * kConSlot, CN);
          const float* x = CN;
          float t[4];
          ld4(CON + i * kConSlot + 4 + 4 * rr, t);   // axis rr of the contact frame
          const int kb = __float_as_int(CN[7]);
          const int lev = PARLV[kb] >> 8;
          const float lsgn = CN[15];                 // != 0: joint-limit row of body kb (only its "normal" row is non-empty)
          int arow[4] = {0, 1, 1, 1};
#if RSB_SPEC_DEPTH == 4
          { const int4 r4 = *reinterpret_cast<const int4*>(ANC + kb * 4); arow[1] = r4.y; arow[2] = r4.z; arow[3] = r4.w; }
#else
          RSB_UNROLL for (int k = 1; k <= NL; ++k) arow[k] = ANC[kb * RSB_SPEC_DEPTH + k];
#endif
          float FK[NL][16], wbk[NL];
          bool live[NL];
          RSB_UNROLL for (int l = 0; l < NL; ++l) {
            const int k = lev - l;      // 1 .. NL where l < lev
            live[l] = l < lev;
            const int node = live[l] ? (k == 1 ? arow[1] : (k == 2 ? arow[2] : arow[3])) : 1;   // (dead level: body 1 - ANC holds -1 past a body's own level)
            ldv<4>(FACT + node * kFactSlot, FK[l]); wbk[l] = WB[node + 5];
          }
          float Vb[8];
          body_vel_ld(BODY + kb * kBodySlot, Vb);
          const int cid = __float_as_int(CN[11]);
          const bool second = HM2 && (cid & kExtra) != 0;
          const int cprim = second ? (cid & 0xffff) : min(cid, ncol - 1);
          const bool selfrow = !second && cid >= kSelfA;
          const float restitution_m = COLT[kColSlot * cprim + 6], res_threshold = COLT[kColSlot * cprim + 7];   // (cprim names a primitive whatever the row is)
          float Fres[6], wxx[3];
          cross3(x, t, Fres);
          Fres[3] = t[0]; Fres[4] = t[1]; Fres[5] = t[2];
          cross3(Vb, x, wxx);  // J u = t . (v_body + w_body x x)
          float cv = t[0] * (Vb[3] + wxx[0]) + t[1] * (Vb[4] + wxx[1]) + t[2] * (Vb[5] + wxx[2]);
          const float restitution = selfrow ? 0.f : restitution_m;
          const float rest = (rr == 2 && lsgn == 0.f && restitution > 0.f && cv < -res_threshold) ? restitution * cv : 0.f;
          const bool limit_row = lsgn != 0.f;
          const bool empty_row = limit_row && rr < 2;
          if (__any(limit_row | (selfrow & (rr == 2)))) {   // rare rows, ONE wave-uniform branch: the J u record of a self-collision entry; a joint-limit row's unit generalized force
            if (selfrow && rr == 2) SELFT[4 * i + 3] = cv;
            if (limit_row) {
              RSB_UNROLL for (int j = 0; j < 6; ++j) Fres[j] = 0.f;
              cv = (rr == 2) ? lsgn * U[kb + 5] : 0.f;
            }
          }
          float* Wc = WC + c * cw;
          RSB_UNROLL for (int l = 0; l < NL; ++l) {
            float yh = dot6(FK[l], Fres);
            if (l == 0) yh = limit_row ? ((rr == 2) ? lsgn : 0.f) : yh;
            const float wk = yh * FK[l][12];
            Wc[live[l] ? 5 + lev - l : kFlatSink] = wk;
            const float cvn = cv + wk * wbk[l];
            cv = live[l] ? cvn : cv;
            RSB_UNROLL for (int j = 0; j < 6; ++j) { const float fn = Fres[j] - FK[l][6 + j] * yh; Fres[j] = live[l] ? fn : Fres[j]; }
          }
          float z[6];
          RSB_UNROLL for (int j = 0; j < 6; ++j) {
            float sacc = Fres[gv2sp(j)];
            RSB_UNROLL for (int q2 = 0; q2 < j; ++q2) sacc -= C[sym6(j, q2)] * z[q2];
            z[j] = sacc * idg[j];
            cv += z[j] * wbb[j];
          }
          if (empty_row) cv = 0.f;
          cv += rest;
          st4(Wc, z); Wc[4] = z[4]; Wc[5] = z[5];
          const float cvb = cv - erp * CN[3] / dt;      // (every wave has normal rows: the division runs either way, a region around it only adds its price)
          CV[c] = (rr == 2) ? cvb : cv;
        }
#else
        if (c < 3 * nc) {
          const int i = c / 3, rr = c - 3 * i;
          float CN[16];
          ldv<4>(CON + i * kConSlot, CN);
          const float* x = CN;
          float t[4];
          ld4(CON + i * kConSlot + 4 + 4 * rr, t);   // axis rr of the contact frame
          const int kb = __float_as_int(CN[7]);
          const int lev = PARLV[kb] >> 8;
          const float lsgn = CN[15];                 // != 0: joint-limit row of body kb (only its "normal" row is non-empty)
          // prefetch the support chain's factors (independent loads), then propagate the unit impulse
          // (deep trees - ML > 4 - fetch the chain four levels at a time further down: 16 x ML registers of factors do not fit)
          constexpr int MLP = ML <= 4 ? ML : 1;
          float FK[MLP][16], wbk[MLP];
          int node[MLP];
          if constexpr (ML <= 4) {
#if defined(RSB_SPECIALIZED) && RSB_SPEC_DEPTH == 4
            // (a tree of four levels: the body's whole ancestor row is ONE 16-byte read that does not wait for the body's level - the entries are then picked by
            //  selects; read entry by entry, `lev - l` makes every read wait for the level's round trip first)
            int arow[4];
            { const int4 r4 = *reinterpret_cast<const int4*>(ANC + kb * 4); arow[0] = r4.x; arow[1] = r4.y; arow[2] = r4.z; arow[3] = r4.w; }
            RSB_UNROLL for (int l = 0; l < ML; ++l) {
              const int k = lev - l;      // 1 .. 3 where l < lev
              node[l] = (l < lev) ? (k == 1 ? arow[1] : (k == 2 ? arow[2] : arow[3])) : 0;
            }
#else
            RSB_UNROLL for (int l = 0; l < ML; ++l) {
              node[l] = 0;
              if (l < lev) node[l] = ANC[kb * depth + lev - l];
            }
#endif
            RSB_UNROLL for (int l = 0; l < ML; ++l) {
              if (l < lev) { ldv<4>(FACT + node[l] * kFactSlot, FK[l]); wbk[l] = WB[node[l] + 5]; }
            }
          }
          float Vb[8];
          body_vel_ld(BODY + kb * kBodySlot, Vb);
          float Fres[6], wxx[3];
          cross3(x, t, Fres);
          Fres[3] = t[0]; Fres[4] = t[1]; Fres[5] = t[2];
          cross3(Vb, x, wxx);  // J u = t . (v_body + w_body x x)
          float cv = t[0] * (Vb[3] + wxx[0]) + t[1] * (Vb[4] + wxx[1]) + t[2] * (Vb[5] + wxx[2]);
          // Newton restitution (oracle: "restitution"): the approach speed J u of this step re-enters the normal row
          const int cid = __float_as_int(CN[11]);
          const bool second = HM2 && (cid & kExtra) != 0;    // a primitive's second contact with the height map / the cylinder of its capsule: the primitive's material
          const int cprim = second ? (cid & 0xffff) : min(cid, ncol - 1);   // (joint-limit rows carry ids >= ncol and no restitution)
          const bool selfrow = !second && cid >= kSelfA;     // entry of a self-collision: restitution is applied to the folded contact (approach speed = sum of the two entries')
          if (selfrow && rr == 2) SELFT[4 * i + 3] = cv;
          const float restitution = selfrow ? 0.f : COLT[kColSlot * cprim + 6], res_threshold = COLT[kColSlot * cprim + 7];
          const float rest = (rr == 2 && lsgn == 0.f && restitution > 0.f && cv < -res_threshold) ? restitution * cv : 0.f;
          const bool limit_row = lsgn != 0.f;
          const bool empty_row = limit_row && rr < 2;
          if (limit_row) {   // unit generalized force s on the joint itself instead of a spatial impulse on the body
            RSB_UNROLL for (int j = 0; j < 6; ++j) Fres[j] = 0.f;
            cv = (rr == 2) ? lsgn * U[kb + 5] : 0.f;
          }
          float* Wc = WC + c * cw;
          if constexpr (ML <= 4) {
            RSB_UNROLL for (int l = 0; l < ML; ++l) {
              if (l < lev) {
                float yh = dot6(FK[l], Fres);
                if (limit_row && l == 0) yh = (rr == 2) ? lsgn : 0.f;
                const float wk = yh * FK[l][12];
                Wc[5 + lev - l] = wk;
                cv += wk * wbk[l];
                RSB_UNROLL for (int j = 0; j < 6; ++j) Fres[j] -= FK[l][6 + j] * yh;
              }
            }
          } else {
            RSB_UNROLL for (int l0 = 0; l0 < ML; l0 += 4) {
              float FQ[4][16], wq[4];
              int nq4[4];
              RSB_UNROLL for (int q4 = 0; q4 < 4; ++q4) {
                nq4[q4] = 0;
                if (l0 + q4 < lev) nq4[q4] = ANC[kb * depth + lev - (l0 + q4)];
              }
              RSB_UNROLL for (int q4 = 0; q4 < 4; ++q4) {
                if (l0 + q4 < lev) { ldv<4>(FACT + nq4[q4] * kFactSlot, FQ[q4]); wq[q4] = WB[nq4[q4] + 5]; }
              }
              RSB_UNROLL for (int q4 = 0; q4 < 4; ++q4) {
                const int l = l0 + q4;
                if (l < lev) {
                  float yh = dot6(FQ[q4], Fres);
                  if (limit_row && l == 0) yh = (rr == 2) ? lsgn : 0.f;
                  const float wk = yh * FQ[q4][12];
                  Wc[5 + lev - l] = wk;
                  cv += wk * wq[q4];
                  RSB_UNROLL for (int j = 0; j < 6; ++j) Fres[j] -= FQ[q4][6 + j] * yh;
                }
              }
            }
          }
          float z[6];
          RSB_UNROLL for (int j = 0; j < 6; ++j) {
            float sacc = Fres[gv2sp(j)];
            RSB_UNROLL for (int q2 = 0; q2 < j; ++q2) sacc -= C[sym6(j, q2)] * z[q2];
            z[j] = sacc * idg[j];
            cv += z[j] * wbb[j];
          }
          if (empty_row) cv = 0.f;
          cv += rest;
          st4(Wc, z); Wc[4] = z[4]; Wc[5] = z[5];
          if (rr == 2) cv -= erp * CN[3] / dt;
          CV[c] = cv;
        }
#endif
      }
#if RSB_FLAT_CLASS
      asm volatile("; rsb columns end");
#endif
      __syncthreads();
      RSB_STAMP(4)
