// step_phase_tree_down.inc — fragment of rsb_step_kernel: base body (redundantly on every lane) and the down pass (lane = body): poses, velocities, bias accelerations, rigid inertias, actuation
    // =========================== base body, redundantly on every lane =========================
#ifdef RSB_X_NO_BASE_MERGE   /* (A/B: the base's rigid inertia on every lane, as before) */
    constexpr bool kBaseMerge = false;
#else
    constexpr bool kBaseMerge = LPE == 16;
#endif
#if RSB_SEAM_LOADS
    // seam carry (step_spec.h): everything the top of the sub-step needs from LDS goes out here as ONE batch, in front of the base arithmetic - which runs from
    // registers (RSB_SEAM_BASE) and hides the wait - and is collected by one pin behind it.  (The pin of the plain quad form, one empty asm per 16-byte read,
    // keeps the reads whole but makes every one of them wait for itself: eight dependent round trips of a lone wave.  One asm over all of them waits once.)
    typedef float sl_f4 __attribute__((ext_vector_type(4)));
    sl_f4 sl_mv[8];
    RSB_UNROLL for (int i = 0; i < 8; ++i) sl_mv[i] = *reinterpret_cast<const sl_f4*>(MODELF + bb * RSB_DIM(MODEL_PITCH, L.model_pitch) + 4 * i);
    float sl_act[5] = {TF[bb + 5], GAIN[2 * bb], GAIN[2 * bb + 1], PT[bb + 6], DTG[bb + 5]};
#endif
    float R0[9], V0[6], A0[6], I10b[10], Zb[6];
    {
#if RSB_SEAM_BASE
      const float* qv = sc_qv; const float* uv = sc_uv;      // (the base's state from registers: loaded at the control step's start, advanced by the update pass)
#else
      float qv[8], uv[8];
      ldv<2>(Q, qv); ldv<2>(U, uv);
#endif
      float w = qv[3], x = qv[4], y = qv[5], z = qv[6];
      const float in = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
      w *= in; x *= in; y *= in; z *= in;
      R0[0] = 1 - 2 * (y * y + z * z); R0[1] = 2 * (x * y - w * z);     R0[2] = 2 * (x * z + w * y);
      R0[3] = 2 * (x * y + w * z);     R0[4] = 1 - 2 * (x * x + z * z); R0[5] = 2 * (y * z - w * x);
      R0[6] = 2 * (x * z - w * y);     R0[7] = 2 * (y * z + w * x);     R0[8] = 1 - 2 * (x * x + y * y);
      V0[0] = uv[3]; V0[1] = uv[4]; V0[2] = uv[5]; V0[3] = uv[0]; V0[4] = uv[1]; V0[5] = uv[2];
      float wxv[3];
      cross3(V0, V0 + 3, wxv);
      A0[0] = A0[1] = A0[2] = 0.f;
      A0[3] = -wxv[0] - ab.gx; A0[4] = -wxv[1] - ab.gy; A0[5] = -wxv[2] - ab.gz;
      pbx = qv[0]; pby = qv[1]; pbz = qv[2];
      if constexpr (!kBaseMerge) {     // (16 lanes per env: the base's rigid inertia and bias force are computed by lane 0 TOGETHER with the bodies' - stage (3) below - and broadcast)
        float MF[kModelSlot];
        ldv<8>(MODELF, MF);
        const float r0[3] = {0.f, 0.f, 0.f};
        body_inertia(R0, r0, V0, A0, MF, dt, I10b, Zb);
      }
      if (s == 0) {
        float P[24];
#if RSB_DOWN_QUADS
        // (the BODY slots in the quad form's layout: step_kernel.h, body_pose_ld)
        RSB_UNROLL for (int i = 0; i < 3; ++i) {
          P[4 * i] = R0[3 * i]; P[4 * i + 1] = R0[3 * i + 1]; P[4 * i + 2] = R0[3 * i + 2]; P[4 * i + 3] = 0.f;
          P[12 + 2 * i] = V0[i]; P[13 + 2 * i] = V0[3 + i]; P[18 + 2 * i] = A0[i]; P[19 + 2 * i] = A0[3 + i];
        }
        stv<5>(BODY, P);      // (floats 20..23 hold bias accelerations only, and nothing reads the base's from its slot: the quads and lane 0 take A0 from registers)
#else
        RSB_UNROLL for (int i = 0; i < 9; ++i) P[i] = R0[i];
        P[9] = P[10] = P[11] = 0.f;
        RSB_UNROLL for (int i = 0; i < 6; ++i) { P[12 + i] = V0[i]; P[18 + i] = A0[i]; }
        stv<6>(BODY, P);
#endif
      }
    }

    // =========================== down pass: lane = body ==========================================
    // (1) every body lane: the joint's own transform E = rtree * R(axis, q)      (no dependence on the parent)
    // (2) level by level: pose, joint axis S, velocity V and bias acceleration A from the parent's (one LDS round trip per level)
    // (3) every body lane: rigid inertia about O, bias force, actuation                    (no dependence on the parent)
    float bS[6], bI10[10], bZ[6], bdtau = 0.f, barm = 1.f, bqb = 0.f, bqd = 0.f;
    bool lim_out = false;
    RSB_UNROLL for (int i = 0; i < 6; ++i) { bS[i] = 0.f; bZ[i] = 0.f; }
    RSB_UNROLL for (int i = 0; i < 10; ++i) bI10[i] = 0.f;
    float Rb[9], rb[3];      // the lane's body pose (quad form: the base's on lane 0 and on the lanes that are no body).  Out here for the own-lane collision test (step_phase_collision.inc)
    {
      float MF[kModelSlot], E9[9], Vb[6], Ab[6];
#if RSB_SEAM_LOADS
      // (the batch issued at the top of the sub-step: one pin keeps the eight 16-byte reads whole, as below, and is the one wait for all of them.
      //  The last results of the base arithmetic are operands too: they tie the pin - the wait - BEHIND that arithmetic, which the scheduler otherwise sinks below it.)
      asm volatile("" : "+v"(sl_mv[0]), "+v"(sl_mv[1]), "+v"(sl_mv[2]), "+v"(sl_mv[3]), "+v"(sl_mv[4]), "+v"(sl_mv[5]), "+v"(sl_mv[6]), "+v"(sl_mv[7]),
                        "+v"(R0[0]), "+v"(R0[4]), "+v"(R0[8]), "+v"(A0[3]), "+v"(A0[4]), "+v"(A0[5]));
      RSB_UNROLL for (int i = 0; i < 8; ++i) { MF[4 * i] = sl_mv[i].x; MF[4 * i + 1] = sl_mv[i].y; MF[4 * i + 2] = sl_mv[i].z; MF[4 * i + 3] = sl_mv[i].w; }
      asm volatile("" : "+v"(sl_act[0]), "+v"(sl_act[1]), "+v"(sl_act[2]), "+v"(sl_act[3]), "+v"(sl_act[4]));
#elif RSB_DOWN_QUADS
      // (the body lanes use every 16-byte chunk of their constants only in part, the axis and the joint's offset on the quads' side now: left to itself the compiler
      //  narrows the eight 16-byte reads to thirteen ds_read2_b32 - the pin keeps them whole)
      RSB_UNROLL for (int i = 0; i < 8; ++i) {
        typedef float float4v __attribute__((ext_vector_type(4)));
        float4v v = *reinterpret_cast<const float4v*>(MODELF + bb * RSB_DIM(MODEL_PITCH, L.model_pitch) + 4 * i);
        asm volatile("" : "+v"(v));
        MF[4 * i] = v.x; MF[4 * i + 1] = v.y; MF[4 * i + 2] = v.z; MF[4 * i + 3] = v.w;
      }
#else
      ldv<8>(MODELF + bb * RSB_DIM(MODEL_PITCH, L.model_pitch), MF);
#endif
      const int jt = __float_as_int(MF[3]);
      const float* axis = MF;
      if (isbody) {
#if RSB_SEAM_JOINTS
        bqb = sc_q; bqd = sc_qd;      // (the joint's state from registers: loaded at the control step's start, advanced by the update pass)
#else
        bqb = Q[bb + 6]; bqd = U[bb + 5];
#endif
        lim_out = (bqb > MF[30]) | (bqb < MF[29]);   // joint outside [q_lower, q_upper]: the joint-limit rows of the collision phase exist only then (rare)
        if (jt == RSB_JOINT_REVOLUTE) {
          float sn, cs;
          fast_sincos(bqb, &sn, &cs);
          const float v = 1.f - cs;
          float Rq[9];
          Rq[0] = cs + axis[0] * axis[0] * v;           Rq[1] = axis[0] * axis[1] * v - axis[2] * sn; Rq[2] = axis[0] * axis[2] * v + axis[1] * sn;
          Rq[3] = axis[1] * axis[0] * v + axis[2] * sn; Rq[4] = cs + axis[1] * axis[1] * v;           Rq[5] = axis[1] * axis[2] * v - axis[0] * sn;
          Rq[6] = axis[2] * axis[0] * v - axis[1] * sn; Rq[7] = axis[2] * axis[1] * v + axis[0] * sn; Rq[8] = cs + axis[2] * axis[2] * v;
          mat3_mul(MF + 8, Rq, E9);
        } else {
          RSB_UNROLL for (int i = 0; i < 9; ++i) E9[i] = MF[8 + i];
        }
      }
      RSB_STAMP(10)
#if RSB_DOWN_QUADS
      // ---- quad form (step_spec.h: RSB_DOWN_QUADS; the worlds of the up pass's quad form): quad g (lanes 4 g .. 4 g + 3 of the env's row) walks DOWN chain g - body
      // KIDS[g] + lv - 1 at level lv - with the parent's pose, velocity and bias acceleration in its registers: no hand-over slot, no barrier between two levels, no
      // exec-mask region, sixteen live lanes at every level.  OUTPUTS are split, sums never: lane q < 3 owns row q of Rb (it needs row q of Rp only) and entry q of
      // every 3-vector - t, rb, a3, the angular and the linear halves of S, V, A (lane 3 repeats lane 2).  The two other entries a cross product needs come from the
      // neighbours by DPP quad_perm rotations (entry q of a x b is a[q+1] b[q+2] - a[q+2] b[q+1], indices mod 3: cross3's expression of that entry).  Every float
      // is the same expression in the same operand order as in the lane = body loop (level 1 keeps its literal zeros: rp, the angular part of A0), the joint kind is a
      // select where that loop branches: bit for bit its results (tests/test_gpu_down_quads.py; -DRSB_X_NO_DOWN_QUADS compiles that loop instead).
      // LDS.  The body lanes park E9, q, qd (kDownQuadSlot floats, three 16-byte stores) in slots that alias the front of the up pass's (L.g: dead from the end of
      // Gauss-Seidel to the next Delassus phase; everything parked is finite - step_phase_prologue.inc); a quad fetches them and the joint constants of MODELF for ALL
      // its levels in one batch with one wait.  Per level a lane stores the ten floats it owns and waits for nothing: a BODY slot holds them lane by lane
      // ([R q0 q1 q2, r q] x 3 | [Vw q, Vl q] x 3 | [Aw q, Al q] x 3: step_kernel.h, body_pose_ld - a transposing exchange for the lane = body layout R9 r3 V6 A6 cost
      // more instructions than the split saved: profiles/r08_down_quads_first_form.txt).  One barrier after the loop; then the body lanes read their own slot once
      // for stage (3) and evaluate S - the lane = body loop's expression of (Rb, rb) - themselves, once for all levels.
      static_assert(LPE == 16 && !TRI && kBaseMerge, "the quad form of the down pass runs beside the up pass's (step_phase_tree_up.inc)");
      static_assert(RSB_SPEC_DEPTH >= 2 && RSB_SPEC_NB == 1 + 4 * (RSB_SPEC_DEPTH - 1), "four chains of equal length below the base (rsb_world.hip: up_quad_table)");
      static_assert(kBodySlot == 24, "the quad form's BODY layout: three 16-byte pose rows, three (Vw, Vl) pairs, three (Aw, Al) pairs");
      {
        typedef float float2v __attribute__((ext_vector_type(2)));
        if (isbody) {
          const float X[12] = {E9[0], E9[1], E9[2], E9[3], E9[4], E9[5], E9[6], E9[7], E9[8], bqb, bqd, 0.f};
          stv<3>(UPS + bb * kDownQuadSlot, X);
        }
        const int dq = s & 3, dg = s >> 2, dr = min(dq, 2);
        const bool q0 = dq == 0, q1 = dq == 1;
        auto sel3 = [&](float a0, float a1, float a2) { return q0 ? a0 : (q1 ? a1 : a2); };
        auto rot1 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x09, 0xf, 0xf, true)); };      // quad_perm [1, 2, 0, 0]: entry q + 1 (mod 3)
        auto rot2 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x52, 0xf, 0xf, true)); };      // quad_perm [2, 0, 1, 1]: entry q + 2 (mod 3)
        // the quad's chain: its body of level 1.  (Chains are consecutive runs of bodies - every body below level 1 follows its parent - of RSB_SPEC_DEPTH - 1 bodies
        // each, and there are no other bodies: rsb_world.hip, up_quad_table.  So chain g starts at body 1 + g (RSB_SPEC_DEPTH - 1): no table read.)
        const int B0 = 1 + dg * (RSB_SPEC_DEPTH - 1);
        __syncthreads();
        float QM[RSB_SPEC_DEPTH - 1][8], QX[RSB_SPEC_DEPTH - 1][12];
        RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
          ldv<2>(MODELF + (B0 + lv - 1) * RSB_DIM(MODEL_PITCH, L.model_pitch), QM[lv - 1]);      // axis3 joint-type | offset3 mass
          ldv<3>(UPS + (B0 + lv - 1) * kDownQuadSlot, QX[lv - 1]);
        }
        // the parent of level 1 is the base, in registers on every lane: lane q takes its row of R0 and its entries of V0, A0 (lane 3: those of lane 2 once more)
        float Rpr[3], rpq = 0.f, Vpw = sel3(V0[0], V0[1], V0[2]), Vpl = sel3(V0[3], V0[4], V0[5]), Apw = 0.f, Apl = sel3(A0[3], A0[4], A0[5]);
        RSB_UNROLL for (int k = 0; k < 3; ++k) Rpr[k] = sel3(R0[k], R0[3 + k], R0[6 + k]);
        float* qslot = BODY + B0 * kBodySlot + 2 * dr;
        RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
          const float* qaxis = QM[lv - 1]; const float* qoff = QM[lv - 1] + 4; const float* qE = QX[lv - 1];
          const bool qrev = __float_as_int(QM[lv - 1][3]) == RSB_JOINT_REVOLUTE;
          const float qqb = QX[lv - 1][9], qqd = QX[lv - 1][10];
          float Rbr[3];
          RSB_UNROLL for (int j = 0; j < 3; ++j) Rbr[j] = Rpr[0] * qE[j] + Rpr[1] * qE[3 + j] + Rpr[2] * qE[6 + j];      // mat3_mul(Rp, E9, Rb), own row
          const float tq = Rpr[0] * qoff[0] + Rpr[1] * qoff[1] + Rpr[2] * qoff[2];                    // mat3_vec(Rp, MF + 4, t), own entry
          float rbq;
          if (lv == 1) rbq = 0.f + tq; else rbq = rpq + tq;
          const float a3q = Rbr[0] * qaxis[0] + Rbr[1] * qaxis[1] + Rbr[2] * qaxis[2];                // mat3_vec(Rb, axis, a3), own entry
          { const float rbp = rbq + a3q * qqb; rbq = qrev ? rbq : rbp; }                              // prismatic: rb += a3 q
          const float rb1 = rot1(rbq), rb2 = rot2(rbq), a31 = rot1(a3q), a32 = rot2(a3q);
          const float crq = rb1 * a32 - rb2 * a31;                                                    // cross3(rb, a3), own entry
          const float Sw = qrev ? a3q : 0.f, Sl = qrev ? crq : a3q;
          // A = Ap + (Vp x S) qd uses the PARENT's V
          const float Vw1 = rot1(Vpw), Vw2 = rot2(Vpw), Vl1 = rot1(Vpl), Vl2 = rot2(Vpl), Sw1 = rot1(Sw), Sw2 = rot2(Sw), Sl1 = rot1(Sl), Sl2 = rot2(Sl);
          const float c1 = Vw1 * Sw2 - Vw2 * Sw1, c2 = Vw1 * Sl2 - Vw2 * Sl1, c3 = Vl1 * Sw2 - Vl2 * Sw1;
          const float Abw = Apw + c1 * qqd, Abl = Apl + (c2 + c3) * qqd;
          const float Vbw = Vpw + Sw * qqd, Vbl = Vpl + Sl * qqd;
          { const float f4[4] = {Rbr[0], Rbr[1], Rbr[2], rbq}; st4(qslot + 2 * dr, f4); }
          *reinterpret_cast<float2v*>(qslot + 12) = float2v{Vbw, Vbl};
          *reinterpret_cast<float2v*>(qslot + 18) = float2v{Abw, Abl};
          qslot += kBodySlot;
          RSB_UNROLL for (int k = 0; k < 3; ++k) Rpr[k] = Rbr[k];
          rpq = rbq; Vpw = Vbw; Vpl = Vbl; Apw = Abw; Apl = Abl;
        }
        __syncthreads();
        float P[24];
        ldv<6>(BODY + bb * kBodySlot, P);      // (lanes that are no body read slot 0: nothing uses it)
        RSB_UNROLL for (int i = 0; i < 3; ++i) {
          Rb[3 * i] = P[4 * i]; Rb[3 * i + 1] = P[4 * i + 1]; Rb[3 * i + 2] = P[4 * i + 2]; rb[i] = P[4 * i + 3];
          Vb[i] = P[12 + 2 * i]; Vb[3 + i] = P[13 + 2 * i]; Ab[i] = P[18 + 2 * i]; Ab[3 + i] = P[19 + 2 * i];
        }
      }
#else
      // (the bodies of level 1 hang off the base, whose pose, velocity and bias acceleration every lane holds in registers: their level needs neither the
      //  barrier that made BODY[0] visible nor the LDS round trip; the barrier at the end of a level covers lane 0's store for everybody else)
      if (depth <= 1) __syncthreads();
      for (int lv = 1; lv < depth; ++lv) {
        if (mylev == lv) {
          float P[24];
          if (lv == 1) {
            RSB_UNROLL for (int i = 0; i < 9; ++i) P[i] = R0[i];
            P[9] = P[10] = P[11] = 0.f;
            RSB_UNROLL for (int i = 0; i < 6; ++i) { P[12 + i] = V0[i]; P[18 + i] = A0[i]; }
          } else {
            ldv<6>(BODY + mypar * kBodySlot, P);
          }
          const float* Rp = P; const float* rp = P + 9; const float* Vp = P + 12; const float* Ap = P + 18;
          float t[3], a3[3];
          mat3_mul(Rp, E9, Rb);
          mat3_vec(Rp, MF + 4, t);
          rb[0] = rp[0] + t[0]; rb[1] = rp[1] + t[1]; rb[2] = rp[2] + t[2];
          mat3_vec(Rb, axis, a3);
          if (jt == RSB_JOINT_REVOLUTE) {
            bS[0] = a3[0]; bS[1] = a3[1]; bS[2] = a3[2];
            cross3(rb, a3, bS + 3);
          } else {
            rb[0] += a3[0] * bqb; rb[1] += a3[1] * bqb; rb[2] += a3[2] * bqb;
            bS[0] = bS[1] = bS[2] = 0.f; bS[3] = a3[0]; bS[4] = a3[1]; bS[5] = a3[2];
          }
          // A = Ap + (Vp x S) qd uses the PARENT's V
          float c1[3], c2[3], c3[3];
          cross3(Vp, bS, c1); cross3(Vp, bS + 3, c2); cross3(Vp + 3, bS, c3);
          RSB_UNROLL for (int i = 0; i < 3; ++i) { Ab[i] = Ap[i] + c1[i] * bqd; Ab[3 + i] = Ap[3 + i] + (c2[i] + c3[i]) * bqd; }
          RSB_UNROLL for (int i = 0; i < 6; ++i) Vb[i] = Vp[i] + bS[i] * bqd;
          float O[24];
          RSB_UNROLL for (int i = 0; i < 9; ++i) O[i] = Rb[i];
          RSB_UNROLL for (int i = 0; i < 3; ++i) O[9 + i] = rb[i];
          RSB_UNROLL for (int i = 0; i < 6; ++i) { O[12 + i] = Vb[i]; O[18 + i] = Ab[i]; }
          stv<6>(BODY + bb * kBodySlot, O);
        }
        __syncthreads();
      }
#endif
      RSB_STAMP(11)
      if constexpr (kBaseMerge) {
        // lane 0 of the env is no body lane (bb = 0: its MF is the base's): it takes the base's pose and runs the SAME body_inertia call as the body lanes -
        // one evaluation of the ~130 instructions for base and bodies instead of two - and its results reach every lane of the row by DPP broadcasts
        if (s == 0) {
          RSB_UNROLL for (int i = 0; i < 9; ++i) Rb[i] = R0[i];
          rb[0] = rb[1] = rb[2] = 0.f;
          RSB_UNROLL for (int i = 0; i < 6; ++i) { Vb[i] = V0[i]; Ab[i] = A0[i]; }
        }
        if (isbody || s == 0) body_inertia(Rb, rb, Vb, Ab, MF, dt, bI10, bZ);     // (lane 0 keeps the base's values in bI10 / bZ: only body lanes ever read theirs)
        RSB_UNROLL for (int i = 0; i < 10; ++i) I10b[i] = row_bcast<0>(bI10[i]);
        RSB_UNROLL for (int i = 0; i < 6; ++i) Zb[i] = row_bcast<0>(bZ[i]);
      }
      if (isbody) {
        if constexpr (!kBaseMerge) body_inertia(Rb, rb, Vb, Ab, MF, dt, bI10, bZ);
#if RSB_DOWN_QUADS
        // S of the own joint from the finished pose: the level loop's expressions (a prismatic joint's rb holds its a3 q already)
        {
          float a3[3], cr[3];
          mat3_vec(Rb, axis, a3);
          cross3(rb, a3, cr);
          const bool rev = jt == RSB_JOINT_REVOLUTE;
          RSB_UNROLL for (int i = 0; i < 3; ++i) { bS[i] = rev ? a3[i] : 0.f; bS[3 + i] = rev ? cr[i] : a3[i]; }
        }
#endif
        // actuation (oracle: actuation_impl): implicit ("stable") PD = position error at q + dt u, plus the joint-space
        // inertia dt (kd + dt kp) added to the armature; an effort-clipped joint is a constant torque source
#if RSB_SEAM_LOADS
        // (seam carry: the five scalars are in registers, from the batch at the top of the sub-step)
        const float* av = sl_act;
        // (written out as the compiler contracts the expression below where its operands are loads - the damping term a rounded product, the position term fused
        //  onto it; with the operands in registers it fuses the other product, and the last bit of tau moves)
        float tau = av[0];
        const float kpj = av[1], kdj = av[2];
        tau += fmaf(kpj, fmaf(-dt, bqd, av[3] - bqb), kdj * (av[4] - bqd));
#else
        float tau = TF[bb + 5];
        const float kpj = GAIN[2 * bb], kdj = GAIN[2 * bb + 1];
        tau += kpj * (PT[bb + 6] - bqb - dt * bqd) + kdj * (DTG[bb + 5] - bqd);
#endif
        float Bpd = dt * (kdj + dt * kpj);
        const float eff = MF[28];
        if (eff > 0.f && fabsf(tau) > eff) { tau = tau > 0.f ? eff : -eff; Bpd = 0.f; }
        tsq = tau * tau;      // (clipped PD + feed-forward, without the joint's passive damping: StepArgs::tau2_out)
        TACT[bb + 5] = tau;   // (StepArgs::tau_out)
        tau -= MF[27] * bqd;
        bdtau = dt * tau; barm = MF[26] + Bpd;
      }
    }
    RSB_STAMP(1)
    RSB_ARGS(ac);
