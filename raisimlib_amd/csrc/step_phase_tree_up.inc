// step_phase_tree_up.inc — fragment of rsb_step_kernel: the up pass (articulated-body inertias, b column), base gather and Cholesky factor
    // =========================== up pass: articulated inertias + b column (lane = body) ==========
    // level by level from the leaves: a body gathers what its children left in UPS, factors its joint out and leaves its own
    // articulated inertia + bias for its parent (RBDA Table 7.1)
#if RSB_UP_QUADS
    // ---- quad form: every level below the base holds exactly four bodies (StepArgs::chain == 2: four consecutively numbered chains of equal length), so quad g
    // (lanes 4 g .. 4 g + 3 of the env's row) takes the g-th body of the level - body KIDS[g] + lv - 1 - and all sixteen lanes work at every level, where the
    // lane = body loop below pays the whole body for four live lanes.  OUTPUTS are split over the quad, sums never: lane q owns rows q and q + 4 (lanes 2, 3: row 5
    // once more) of the 6 x 6 articulated inertia and the matching entries of Z; every term is added in the order of the lane = body loop (rigid part, then the
    // child), Uv_r in sym6_vec's order, the quad exchanges Uv and Z by DPP quad_perm moves, and D, 1 / D, the square root, yhat, yd, ud are the same expressions,
    // evaluated by all four lanes: the results are the lane = body loop's bit for bit (tests/test_gpu_up_quads.py; -DRSB_X_NO_UP_QUADS compiles that loop instead).
    // A quad walks up ITS chain: the rows it computed at level lv + 1 are the child's rows of its body of level lv, on the same lanes, so they stay in registers -
    // no hand-over slot is written and no barrier stands between two levels - and the rows of level 1 travel on to the base by DPP row moves (base gather below).
    // LDS.  What the body lanes hold in registers and the quads need goes through LDS ONCE per sub-step, from all body lanes at once: [rigid inertia | Z] as
    // six FULL rows on an 8-float pitch (row r = Ia[r][0..5] Z[r] pad: a quad lane fetches a row with two 16-byte reads at an address of its own) in slots of
    // kUpQuadSlot = 52 floats, S, armature and dt tau in floats 0..7 of the body's FACT slot.  The slots ALIAS the Delassus rows (L.g: nb x 52 <= 832 of its
    // 864 floats at 8 contact slots), which are dead from the end of the Gauss-Seidel phase of one sub-step to the Delassus phase of the next; the height-map narrow
    // phase uses the same floats as scratch in the collision phase (step_phase_collision.inc), which has ended here - nothing is parked there earlier than this
    // line.  The FACT slot is dead from the update phase of one sub-step to this point of the next; its floats 6, 7 end up holding ud[0], ud[1] as everywhere else.
    static_assert(LPE == 16 && !TRI, "the quad form of the up pass is for 16 lanes per env and the square Delassus layout (rsb_world.hip: up_quad_table)");
    static_assert(kBaseMerge, "the quad form of the up pass takes the base's rigid inertia and bias force from lane 0 of the env (step_phase_tree_down.inc)");
    const int upq_q = s & 3;
    const int upq_rowa = 8 * upq_q, upq_rowb = 8 * min(upq_q + 4, 5);
    float upq_oa[8], upq_ob[8];                        // the quad's rows of its body of the level that ran last; in the end: of the base's child
    {
      float (&oa)[8] = upq_oa, (&ob)[8] = upq_ob;
      if (isbody || s == 0) {                          // (lane 0 holds the base's: slot 0)
        float IA[21];
        rigid_expand(bI10, IA);
        RSB_UNROLL for (int r = 0; r < 6; ++r) {
          const float row[8] = {IA[sym6(r, 0)], IA[sym6(r, 1)], IA[sym6(r, 2)], IA[sym6(r, 3)], IA[sym6(r, 4)], IA[sym6(r, 5)], bZ[r], 0.f};
          stv<2>(UPS + bb * kUpQuadSlot + 8 * r, row);
        }
        const float F8[8] = {bS[0], bS[1], bS[2], bS[3], bS[4], bS[5], barm, bdtau};
        stv<2>(FACT + bb * kFactSlot, F8);
      }
      const int qg = s >> 2, qq = upq_q;
      const int qb0 = KIDS[qg];                        // the quad's chain: its body of level 1 (the base's children lead the list)
      const int rowa = upq_rowa, rowb = upq_rowb;
      __syncthreads();
      RSB_UNROLL for (int k = 0; k < 8; ++k) oa[k] = ob[k] = 0.f;
      RSB_UNROLL for (int lv = RSB_SPEC_DEPTH - 1; lv >= 1; --lv) {
        typedef float float2v __attribute__((ext_vector_type(2)));
        const int B = qb0 + lv - 1;
        float* R = UPS + B * kUpQuadSlot;
        float ra[8], rb[8], F8[8];
        ldv<2>(R + rowa, ra); ldv<2>(R + rowb, rb);
        ldv<2>(FACT + B * kFactSlot, F8);
        if (lv < RSB_SPEC_DEPTH - 1) {                 // rigid part + the child's rows (the lane = body loop's order)
          RSB_UNROLL for (int k2 = 0; k2 < 4; ++k2) {
            const float2v sa = float2v{ra[2 * k2], ra[2 * k2 + 1]} + float2v{oa[2 * k2], oa[2 * k2 + 1]};
            const float2v sb = float2v{rb[2 * k2], rb[2 * k2 + 1]} + float2v{ob[2 * k2], ob[2 * k2 + 1]};
            ra[2 * k2] = sa.x; ra[2 * k2 + 1] = sa.y; rb[2 * k2] = sb.x; rb[2 * k2 + 1] = sb.y;
          }
        }
        const float* qS = F8;
        const float qarm = F8[6], qdtau = F8[7];
        float ua = 0.f, ub = 0.f;                      // Uv of the own rows (sym6_vec's accumulation)
        RSB_UNROLL for (int j = 0; j < 6; ++j) ua += ra[j] * qS[j];
        RSB_UNROLL for (int j = 0; j < 6; ++j) ub += rb[j] * qS[j];
        float Uv[6], Z[6];
        Uv[0] = quad_bcast<0>(ua); Uv[1] = quad_bcast<1>(ua); Uv[2] = quad_bcast<2>(ua); Uv[3] = quad_bcast<3>(ua); Uv[4] = quad_bcast<0>(ub); Uv[5] = quad_bcast<1>(ub);
        Z[0] = quad_bcast<0>(ra[6]); Z[1] = quad_bcast<1>(ra[6]); Z[2] = quad_bcast<2>(ra[6]); Z[3] = quad_bcast<3>(ra[6]); Z[4] = quad_bcast<0>(rb[6]); Z[5] = quad_bcast<1>(rb[6]);
        const float D = dot6(qS, Uv) + qarm;
        const float invD = 1.0f / D;
        const float rsD = sqrtf(invD);
        const float yhat = qdtau - dot6(qS, Z);
        const float yd = yhat * invD;
        float ud[6];
        RSB_UNROLL for (int i = 0; i < 6; ++i) ud[i] = Uv[i] * invD;
        // entry (r, c) = Ia - Uv[max(r, c)] ud[min(r, c)]: what the packed lower-triangular store of the lane = body loop computes for (max, min)
        const float uda = ua * invD, udb = ub * invD;   // ud of the own rows
        RSB_UNROLL for (int c = 0; c < 6; ++c) {
          const bool low = c <= qq;                     // (c = 0: always, c >= 4: never)
          oa[c] = ra[c] - (low ? ua : Uv[c]) * (low ? ud[c] : uda);
        }
        RSB_UNROLL for (int c = 0; c < 5; ++c) ob[c] = rb[c] - ub * ud[c];     // rows 4, 5: c <= 4 <= r
        ob[5] = rb[5] - Uv[5] * udb;                    // (4, 5) on lane 0; (5, 5) elsewhere, where Uv[5] is ub
        oa[6] = ra[6] + ua * yd; ob[6] = rb[6] + ub * yd;
        oa[7] = 0.f; ob[7] = 0.f;
        // FACT: S is there; UD, rsD, invD, pad and W_b's entry by all four lanes (the same values to the same addresses: a predicate would cost more than the stores)
        *reinterpret_cast<float2v*>(FACT + B * kFactSlot + 6) = float2v{ud[0], ud[1]};
        { const float f4[4] = {ud[2], ud[3], ud[4], ud[5]}; st4(FACT + B * kFactSlot + 8, f4); }
        { const float f4[4] = {rsD, invD, 0.f, 0.f}; st4(FACT + B * kFactSlot + 12, f4); }
        WB[B + 5] = yhat * rsD;
      }
      __syncthreads();
    }
#else
    float bUD[6], brsD = 0.f;
    RSB_UNROLL for (int i = 0; i < 6; ++i) bUD[i] = 0.f;
    for (int lv = depth - 1; lv >= 1; --lv) {
      if (mylev == lv) {
        float IA[21], Z[6];
        rigid_expand(bI10, IA);
        RSB_UNROLL for (int i = 0; i < 6; ++i) Z[i] = bZ[i];
        const int kn = mykid >> 16, ks = mykid & 0xffff;
        // the children's 27 sums as 14 v_pk_add_f32: [IA | Z | pad] in the hand-over slot's layout, pairs as they come from ds_read_b128
        {
          typedef float float2v __attribute__((ext_vector_type(2)));
          float2v A2[14];
          RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) {
            const int i0 = 2 * k2, i1 = 2 * k2 + 1;
            A2[k2] = float2v{i0 < 21 ? IA[i0 < 21 ? i0 : 0] : Z[(i0 - 21) < 6 ? (i0 - 21) : 0], i1 < 21 ? IA[i1 < 21 ? i1 : 0] : (i1 < 27 ? Z[(i1 - 21) < 6 ? (i1 - 21) : 0] : 0.f)};
          }
          if (kn > 0) {     // the first child's index is in a register (prologue)
            float P[28];
            ldv<7>(UPS + kid_first * kUpSlot, P);
            RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) A2[k2] += float2v{P[2 * k2], P[2 * k2 + 1]};
          }
          for (int ci = 1; ci < max_kid; ++ci) {
            if (ci < kn) {
              float P[28];
              ldv<7>(UPS + KIDS[ks + ci] * kUpSlot, P);
              RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) A2[k2] += float2v{P[2 * k2], P[2 * k2 + 1]};
            }
          }
          RSB_UNROLL for (int i = 0; i < 21; ++i) IA[i] = (i & 1) ? A2[i >> 1].y : A2[i >> 1].x;
          RSB_UNROLL for (int i = 0; i < 6; ++i) Z[i] = ((21 + i) & 1) ? A2[(21 + i) >> 1].y : A2[(21 + i) >> 1].x;
        }
        float Uv[6];
        sym6_vec(IA, bS, Uv);
        const float D = dot6(bS, Uv) + barm;
        const float invD = 1.0f / D;
        const float rsD = sqrtf(invD);
        const float yhat = bdtau - dot6(bS, Z);
        const float yd = yhat * invD;
        float Fk[16], O[28];
        RSB_UNROLL for (int i = 0; i < 6; ++i) {
          const float ud = Uv[i] * invD;
          bUD[i] = ud;
          Fk[i] = bS[i]; Fk[6 + i] = ud;
          RSB_UNROLL for (int j = 0; j <= i; ++j) O[sym6(i, j)] = IA[sym6(i, j)] - Uv[i] * (Uv[j] * invD);
          O[21 + i] = Z[i] + Uv[i] * yd;
        }
        O[27] = 0.f;
        brsD = rsD;
        Fk[12] = rsD; Fk[13] = invD; Fk[14] = 0.f; Fk[15] = 0.f;
        stv<4>(FACT + bb * kFactSlot, Fk);
        WB[bb + 5] = yhat * rsD;
        stv<7>(UPS + bb * kUpSlot, O);
      }
      __syncthreads();
    }
#endif
    if (depth <= 1) __syncthreads();
    RSB_STAMP(14)
    // base (every lane): gather the bodies hanging off the base, Cholesky in gv order (lin, ang), W_b base part
    float C[21], idg[6], wbb[6];
    {
      float IA[21], Z[6];
      rigid_expand(I10b, IA);
      RSB_UNROLL for (int i = 0; i < 6; ++i) Z[i] = Zb[i];
      {
        typedef float float2v __attribute__((ext_vector_type(2)));
        float2v A2[14];
        RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) {
          const int i0 = 2 * k2, i1 = 2 * k2 + 1;
          A2[k2] = float2v{i0 < 21 ? IA[i0 < 21 ? i0 : 0] : Z[(i0 - 21) < 6 ? (i0 - 21) : 0], i1 < 21 ? IA[i1 < 21 ? i1 : 0] : (i1 < 27 ? Z[(i1 - 21) < 6 ? (i1 - 21) : 0] : 0.f)};
        }
#if RSB_UP_QUADS
        // quad form: the base's four children are the quads' bodies of level 1, their rows sit in the quads' registers.  Rigid part (slot 0, from lane 0) + child 0 on
        // quad 0, handed on to quad 1 by a row shift of four lanes, + child 1 ... : the sums of the lane = body loop in its order, complete on lanes 12..15 (lane
        // 12 + q: rows q and q + 4), from where every entry of the lower triangle and of Z reaches the sixteen lanes by a row broadcast
        {
          float ta[8], tb[8];
          ldv<2>(UPS + upq_rowa, ta); ldv<2>(UPS + upq_rowb, tb);
          RSB_UNROLL for (int k = 0; k < 7; ++k) { ta[k] += upq_oa[k]; tb[k] += upq_ob[k]; }
          RSB_UNROLL for (int g = 1; g < 4; ++g)
            RSB_UNROLL for (int k = 0; k < 7; ++k) { ta[k] = row_shr4(ta[k]) + upq_oa[k]; tb[k] = row_shr4(tb[k]) + upq_ob[k]; }
          static_for<0, 6>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const float* t = i < 4 ? ta : tb;
            RSB_UNROLL for (int j = 0; j <= i; ++j) A2[sym6(i, j) >> 1][sym6(i, j) & 1] = row_bcast<12 + (i & 3)>(t[j]);
            A2[(21 + i) >> 1][(21 + i) & 1] = row_bcast<12 + (i & 3)>(t[6]);
          });
        }
#else
        RSB_UNROLL for (int ci = 0; ci < 4; ++ci) {     // the base's children lead the list (kid_start[0] == 0); the first four indices sit in scalar registers
          if (ci < nkid0) {
            float P[28];
            ldv<7>(UPS + kid0s[ci] * kUpSlot, P);
            RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) A2[k2] += float2v{P[2 * k2], P[2 * k2 + 1]};
          }
        }
        for (int ci = 4; ci < nkid0; ++ci) {
          float P[28];
          ldv<7>(UPS + KIDS[ci] * kUpSlot, P);
          RSB_UNROLL for (int k2 = 0; k2 < 14; ++k2) A2[k2] += float2v{P[2 * k2], P[2 * k2 + 1]};
        }
#endif
        RSB_UNROLL for (int i = 0; i < 21; ++i) IA[i] = (i & 1) ? A2[i >> 1].y : A2[i >> 1].x;
        RSB_UNROLL for (int i = 0; i < 6; ++i) Z[i] = ((21 + i) & 1) ? A2[(21 + i) >> 1].y : A2[(21 + i) >> 1].x;
      }
      RSB_UNROLL for (int i = 0; i < 6; ++i) {
        RSB_UNROLL for (int j = 0; j <= i; ++j) {
          float sacc = IA[sym6(gv2sp(i), gv2sp(j))];
          RSB_UNROLL for (int k = 0; k < j; ++k) sacc -= C[sym6(i, k)] * C[sym6(j, k)];
          if (i == j) { const float ri = 1.0f / sqrtf(sacc); C[sym6(i, i)] = sacc * ri; idg[i] = ri; }
          else C[sym6(i, j)] = sacc * idg[j];
        }
      }
      // a fixed base is a base of infinite inertia: with 1 / diag(C) = 0 every base entry of the contact columns, of W_b and of
      // the velocity update vanishes, and nothing else in the step has to know
      if (fixed_base) { RSB_UNROLL for (int i = 0; i < 6; ++i) idg[i] = 0.f; }
      float tb[8];
      ldv<2>(TF, tb);
      RSB_UNROLL for (int i = 0; i < 6; ++i) {
        float sacc = dt * tb[i] - Z[gv2sp(i)];
        RSB_UNROLL for (int k = 0; k < i; ++k) sacc -= C[sym6(i, k)] * wbb[k];
        wbb[i] = sacc * idg[i];
      }
    }
    RSB_STAMP(3)
