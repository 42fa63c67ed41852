// step_phase_solver.inc — fragment of rsb_step_kernel (inside `if (ncw > 0)`): the per-contact iteration - grouped sweep, slip searches, Anderson step (KMAX > 8), W^T lambda
      if (PROF && a.dbg && env == a.dbg_env && env_valid && s == 0) {   // debug aid: the contact problem of the real contacts (no limit rows)
        const int n3 = 3 * nc_real;
        a.dbg[0] = (float)nc_real;
        for (int i = 0; i < n3; ++i)
          for (int j = 0; j < n3; ++j)
            a.dbg[1 + i * n3 + j] = GROWS ? G[(i / 3) * GRP + kGBlock * (j / 3) + g_block_off(i % 3, j % 3)] : !TRI ? G[i * GS + 4 * (j / 3) + (j % 3)]
                                          : (i / 3 >= j / 3 ? G[tri_off(i / 3, j / 3) + 4 * (i % 3) + (j % 3)] : G[tri_off(j / 3, i / 3) + 4 * (j % 3) + (i % 3)]);
        for (int i = 0; i < n3; ++i) a.dbg[1 + n3 * n3 + i] = CV[i];
      }
      long long t_gs0 = 0, tz0 = 0; if (PROF && a.prof) t_gs0 = clock64();
      // ========================= per-contact iteration, grouped sweep (lane = contact) ===============
      // Lane j (< nc) owns contact j: own 3x3 block, its inverse, velocity (WITH the own impulse) and impulse stay in
      // registers.  Contacts are grouped by the limb they sit on (the subtree hanging off the base that holds the contact's
      // body; contacts on the base form one more group).  Contacts of different limbs couple only through the base, contacts
      // of one limb - above all two contacts on one link - couple strongly.  One sweep =
      //   for k = 0 .. (largest group size - 1):  pass k
      //     every contact that is the k-th of its group applies the per-contact rule (open / stick / slip with its friction
      //     direction refined by one guarded Newton step, else the row-cooperative global search) to the impulses the pass
      //     started with - ALL of them in one SIMD evaluation (block Jacobi across limbs, Gauss-Seidel within a limb; oracle:
      //     group_parallel) - then the impulse changes are exchanged: lane i adds G_ij dl_j for every j (DPP row_newbcast);
      //   convergence test, stagnation exit, calmest iterate.
      // A lone wave issues one instruction per ~4 cycles whatever its kind (profiles/r02_ubench_lone_wave_latency.txt), so the
      // solve is priced in instructions: a pass costs one evaluation of the rule (~60 instructions, + ~90 when a direction is
      // refined) + 16 per contact for the exchange, where the sequential sweep paid one evaluation per contact.  The usual env
      // (four feet on four legs) has one pass per sweep; sweep counts are those of the sequential iteration + 6 %.
      {
        const bool isc = s < nc;
        float Gii[9], Ginv[12], v[3], lam[3] = {0.f, 0.f, 0.f};
        const float* Gmine = GROWS ? G + GRP * min(s, KMAX - 1) : G + 3 * min(s, KMAX - 1) * GS;     // non-contact lanes read (and ignore) the last contact's rows
        RSB_UNROLL for (int q2 = 0; q2 < 9; ++q2) Gii[q2] = 0.f;
        RSB_UNROLL for (int q2 = 0; q2 < 12; ++q2) Ginv[q2] = 0.f;
        v[0] = v[1] = v[2] = 0.f;
#if RSB_FLAT_CLASS
        asm volatile("; rsb setup begin");     // (tests/test_flat_setup_host.py counts between the comment lines)
#endif
#if RSB_FLAT_SETUP_HEAD
        // flat set-up (step_spec.h): two batches of LDS reads and no exec-mask region.  Batch A is everything the lane index alone addresses - the own block, its
        // inverse, the own velocity, floats 4-11 of the contact record (body AND collision id), the five coupling blocks of the exchange's straight part - read by
        // every lane at the clamped slot a lane without a contact always used for its coupling rows.  Such a lane holds whatever that slot holds; nothing it computes
        // from it is ever used (every result that leaves a lane is selected by isc, mine, need or lost; its impulse stays the literal zero).
        static_assert(GROWS && !TRI, "flat set-up: the row-block layout of the quadruped classes");
        const int sq = min(s, KMAX - 1);
        float fq0[5][4], fq1[5][4], fq2[5], fc4[4], fc8[4];
        {
          float D[3][3];
          gblk_load(Gmine + kGBlock * sq, D);
          ldv<3>(GINV + 12 * sq, Ginv);
          v[0] = CV[3 * sq]; v[1] = CV[3 * sq + 1]; v[2] = CV[3 * sq + 2];
          ld4(CON + sq * kConSlot + 4, fc4); ld4(CON + sq * kConSlot + 8, fc8);
          RSB_UNROLL for (int k = 0; k < 5; ++k) { ld4(Gmine + kGBlock * k, fq0[k]); ld4(Gmine + kGBlock * k + 4, fq1[k]); fq2[k] = Gmine[kGBlock * k + 8]; }
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr) RSB_UNROLL for (int cc = 0; cc < 3; ++cc) Gii[3 * rr + cc] = D[rr][cc];
        }
        // Batch B is what the record addresses, behind ONE wait: the body's level and ancestor row, the primitive's friction coefficient and its warm row.  A lane
        // without a contact asks for body 0; a joint-limit row, a self-collision entry and such a lane for a primitive of the table (the index clamped) - what they
        // get is discarded below by selects on the RESULTS (a stale warm row may hold anything: never a product with a zero).
        const int kb = isc ? __float_as_int(fc4[3]) : 0;
        const int mycol = isc ? __float_as_int(fc8[3]) : 0;
        const int fci = min(mycol & 0xffff, ncol - 1);
        const int fpl = PARLV[kb];
        int fanc[4] = {0, -1, -1, -1};      // the body's ancestor row: kept for the impulse scatter that ends the solve
#if RSB_SPEC_DEPTH == 4
        { const int4 r4 = *reinterpret_cast<const int4*>(ANC + kb * 4); fanc[1] = r4.y; fanc[2] = r4.z; fanc[3] = r4.w; }
#else
        RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) fanc[lv] = ANC[kb * RSB_SPEC_DEPTH + lv];
#endif
        const float fmu = COLT[kColSlot * fci + 5];
        float fwr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (has_warm) { RSB_UNROLL for (int i = 0; i < 6; ++i) fwr[i] = WARM[6 * fci + i]; }
        __builtin_amdgcn_sched_barrier(0);      // (the whole batch is issued before its first result is waited for: left alone the scheduler puts the level test, and its wait, in front of the other reads)
        int gidc = isc ? (((fpl >> 8) >= 1) ? fanc[1] : 0) : -1 - s;            // limb of the own contact (non-contact lanes: an id nobody shares)
        float fsmu = 0.f;
#else
        int gidc = -1 - s;            // limb of the own contact (non-contact lanes: an id nobody shares)
        if (isc) {
          if constexpr (GROWS) {   // the own block of the own row
            float D[3][3];
            gblk_load(Gmine + kGBlock * s, D);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) RSB_UNROLL for (int cc = 0; cc < 3; ++cc) Gii[3 * rr + cc] = D[rr][cc];
          } else {
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
              float g4[4];
              ld4(TRI ? G + tri_off(s, s) + 4 * rr : G + (3 * s + rr) * GS + 4 * s, g4);      // blocks sit on a 4-float pitch: one 16-byte read per row
              Gii[3 * rr] = g4[0]; Gii[3 * rr + 1] = g4[1]; Gii[3 * rr + 2] = g4[2];
            }
          }
          ldv<3>(GINV + 12 * s, Ginv);
          v[0] = CV[3 * s]; v[1] = CV[3 * s + 1]; v[2] = CV[3 * s + 2];
          const int kb = __float_as_int(CON[s * kConSlot + 7]);
          gidc = ((PARLV[kb] >> 8) >= 1) ? ANC[kb * depth + 1] : 0;
        }
#endif
        // the solver's parameters, read here so that they occupy SGPRs during the solve only
        RSB_ARGS(ag);
        // the own contact's friction coefficient: that of its collision primitive against the terrain (material pairs)
#if !RSB_FLAT_SETUP_HEAD
        const int mycol = isc ? __float_as_int(CON[s * kConSlot + 11]) : 0;
#endif
        if (__any(nselfc > 0)) {   // rare
#if RSB_FLAT_SETUP_HEAD
          fsmu = SELFT[4 * sq];      // (a self-collision's material pair: read by every lane behind the wave-uniform test, taken below by its first entry)
#endif
          // a self-collision couples its two limbs strongly: their groups are merged (oracle: the same relabelling, in contact
          // order); the inert second entries keep ids of their own
          const bool prim = isc && (mycol & kSelfA) != 0;
          int gidb = __shfl_down(gidc, 1);   // the second body's limb: what the next slot (the second entry) computed for itself
          gidb = prim ? gidb : gidc;
          if (isc && (mycol & kSelfB)) { gidc = -1 - s; gidb = gidc; }
          for (int j = 0; j + 1 < ncw; ++j) {
            const int src = (lane & ~(LPE - 1)) | j;
            const int ja = __shfl(gidc, src), jb = __shfl(gidb, src), jp = __shfl(prim ? 1 : 0, src);
            const int lo = min(ja, jb), hi = max(ja, jb);
            if (jp && lo != hi) { gidc = (gidc == hi) ? lo : gidc; gidb = (gidb == hi) ? lo : gidb; }
          }
        }
#if RSB_FLAT_SETUP_HEAD
        float mu = (isc && mycol < ncol) ? fmu : RSB_DIM_F32(MU, ag.mu);
        if constexpr (HM2) mu = (isc && (mycol & kExtra)) ? fmu : mu;      // (the same table entry: mycol & 0xffff is mycol itself below ncol)
        mu = (mycol & kSelfA) ? fsmu : mu;    // material pair of the two primitives (an env with such an entry has nselfc > 0)
#else
        float mu = (isc && mycol < ncol) ? COLT[kColSlot * mycol + 5] : RSB_DIM_F32(MU, ag.mu);
        if constexpr (HM2) { if (isc && (mycol & kExtra)) mu = COLT[kColSlot * (mycol & 0xffff) + 5]; }
        if (mycol & kSelfA) mu = SELFT[4 * s];    // material pair of the two primitives
#endif
        const float mu2 = mu * mu;
        const float alpha_init = RSB_DIM_F32(ALPHA_INIT, ag.alpha_init), alpha_min = RSB_DIM_F32(ALPHA_MIN, ag.alpha_min), alpha_decay = RSB_DIM_F32(ALPHA_DECAY, ag.alpha_decay);
        const float threshold = RSB_DIM_F32(THRESHOLD, ag.threshold), stall_factor = RSB_DIM_F32(STALL_FACTOR, ag.stall_factor);
        const int max_iter = RSB_DIM_INT(MAX_ITER, ag.max_iter), section_rounds = RSB_DIM(SECTION_ROUNDS, ag.section_rounds), stall_window = RSB_DIM(STALL_WINDOW, ag.stall_window);
        const int freeze_after = RSB_DIM(FREEZE_AFTER, ag.freeze_after), refine = RSB_DIM(REFINE, ag.refine), multi_fa = RSB_DIM(MULTI_FA, ag.multi_freeze_after);
        // per-solve constants of the own contact: den(d) = a0 + a1 x + a2 y; n01.. hold mu * G_tt (see slip_prepare)
        SlipCoef sc;
        sc.a0 = Gii[8]; sc.a1 = mu * Gii[6]; sc.a2 = mu * Gii[7];
        sc.n01 = mu * Gii[0]; sc.n02 = mu * Gii[1]; sc.n11 = mu * Gii[3]; sc.n12 = mu * Gii[4];
        sc.n00 = sc.n10 = sc.vn = sc.ls0 = sc.ls1 = 0.f;
#if RSB_PK_SOLVE
        // packed form (step_spec.h, step_slip_pk.h): the own block as the column pairs (G0,G3) (G1,G4) (G2,G5) - the pairs the row-block layout stores - and row 2,
        // its inverse's rows 0 | 1 likewise, mu * G_tt as (n01,n11) (n02,n12)
        static_assert(!TRI && !COUL, "the packed sweep is the quadruped's energy-rule classes'");
        const f32x2 gcp[3] = {f32x2{Gii[0], Gii[3]}, f32x2{Gii[1], Gii[4]}, f32x2{Gii[2], Gii[5]}};
        const f32x2 gip[3] = {f32x2{Ginv[0], Ginv[3]}, f32x2{Ginv[1], Ginv[4]}, f32x2{Ginv[2], Ginv[5]}};
        const f32x2 mg1 = pk_splat(mu) * gcp[0], mg2 = pk_splat(mu) * gcp[1];
#endif
        float lam_best[3] = {0.f, 0.f, 0.f}, best_rel = 3e38f;   // calmest iterate (returned when the solve does not converge)
        float sdx = 0.f, sdy = 0.f;   // friction direction of this contact (|.| = 1 once set)
        int sdst = 0;                 // 0: none, 1: found in this solve, 3: inherited from the previous integrate() (warm state), unused so far
        float alpha = alpha_init, best_prev = 3e38f, best_cur = 3e38f;
        bool done = (nc == 0), converged = (nc == 0);
        int wcount = 0;

        // position of the own contact within its group, and the wave's largest group (= passes per sweep)
        int gpos = 0, gdw = 1;
        bool light = false;   // light passes (oracle: multi_light; opt-in): a multi-contact env refreshes ALL its directions in pass 0 only
        bool multi = false;   // multi-contact env (>= multi_depth contacts on one limb): its own lag / stagnation settings
        int sw_env = stall_window > 0 ? stall_window : -1;   // this env's stagnation window (-1: the sweep counter never gets there = no exit)
        {
          static_for<0, KMAX / 4>([&](auto bc) {
            constexpr int j0 = 4 * decltype(bc)::value;
            if (j0 < ncw) {
              static_for<0, 4>([&](auto kc2) {
                constexpr int j = j0 + decltype(kc2)::value;
                const int gj = __builtin_amdgcn_update_dpp(0, gidc, 0x150 + j, 0xf, 0xf, true);
                gpos += ((gj == gidc) & (j < s)) ? 1 : 0;
              });
            }
          });
          const int gd = row_max_i32(isc ? gpos + 1 : 1);   // the env's largest group (contact lanes sit in the env's first row)
          // multi-contact env (oracle: `multi`): >= multi_depth contacts on one limb - a redundant set, which the per-contact
          // iteration solves slowly and the quadruped-tuned accelerations cut short (rsb_set_solver_multi_contact)
          multi = (RSB_DIM(MULTI_DEPTH, ag.multi_depth) > 0) & (gd >= RSB_DIM(MULTI_DEPTH, ag.multi_depth));
          light = multi & (RSB_DIM(MULTI_LIGHT, ag.multi_light) != 0);
          sw_env = multi ? (RSB_DIM(MULTI_SW, ag.multi_stall_window) > 0 ? RSB_DIM(MULTI_SW, ag.multi_stall_window) : -1) : sw_env;
          gdw = env_groups_max<LPE>(gd);
        }
#if RSB_SWEEP_LOOP
        // (the pass count is wave-uniform and constant during the solve: pinned in a scalar register, or it waits in a vector register and every pass's loop test is
        //  a vector compare)
        gdw = __builtin_amdgcn_readfirstlane(gdw);
        asm volatile("" : "+s"(gdw));
#endif
        // Anderson acceleration of the sweep map (oracle: orc_params::anderson; rsb_set_solver_anderson) - the large-model classes
        // only: the quadruped's sweep loop has no register to spare and its envs converge in 3-4 sweeps.  aa_x: the impulse the sweep
        // started from; aa_g / aa_r: the previous sweep's result and residual.
#ifndef RSB_X_AA8
#define RSB_X_AA8 0   /* (experiment: the Anderson step in the quadruped classes too) */
#endif
        constexpr bool AA = TRI || RSB_X_AA8;
        const int aa_first = AA ? ag.anderson : 0;
        const float aa_clip = ag.anderson_clip;
        const bool aa_on = AA && multi && aa_first > 0;
        float aa_x[3] = {0.f, 0.f, 0.f}, aa_g[3] = {0.f, 0.f, 0.f}, aa_r[3] = {0.f, 0.f, 0.f};

        // exchange of impulse changes: lane i adds G_ij x_j for every contact j of its env (x_j broadcast from lane j of the
        // row).  Contacts 0-3 run as one straight block whatever the count (a slot its env does not use carries x = 0 against a
        // finite, zero-initialised block) on coupling blocks held in registers; contacts 4-7 behind one nested scalar test each
        // (the usual hard env has five), the rest in blocks of four.
        // rows of the own contact (sm) against contact k: the square layout reads them in place; the packed layout reads the stored
        // block (max, min) and transposes it in registers when k > sm (six selects per block, once per solve)
        const int sm = min(s, KMAX - 1);
        auto coupling = [&](int k, float (&g)[3][4]) {
          if constexpr (TRI) {
            const bool tr = k > sm;
            const float* bp = G + tri_off(tr ? k : sm, tr ? sm : k);
            float t[3][4];
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) ld4(bp + 4 * rr, t[rr]);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
              RSB_UNROLL for (int cc = 0; cc < 3; ++cc) g[rr][cc] = tr ? t[cc][rr] : t[rr][cc];
              g[rr][3] = 0.f;
            }
          } else if constexpr (GROWS) {
            float t[3][3];
            gblk_load(Gmine + kGBlock * k, t);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
              RSB_UNROLL for (int cc = 0; cc < 3; ++cc) g[rr][cc] = t[rr][cc];
              g[rr][3] = 0.f;
            }
          } else {
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) ld4(Gmine + rr * GS + 4 * k, g[rr]);
          }
        };
        // Packed fp32: rows 0 and 1 of a coupling block's column sit in one register pair (read as such: ds_read2_b32 at
        // the two rows' offsets), so that a column updates both rows with ONE v_pk_fma_f32 (the impulse component broadcast by op_sel):
        // 6 instead of 9 FMA instructions per contact and exchange.
#ifndef RSB_X_PK_TRI
#define RSB_X_PK_TRI 1   /* (0: the unpacked exchange of the large-model classes, for an A/B) */
#endif
        constexpr bool PK = !TRI || RSB_X_PK_TRI;
#ifndef RSB_X_NPK_TRI
#define RSB_X_NPK_TRI 12   /* (coupling blocks the large-model classes hold in registers; 8: blocks 8-11 are fetched per pass like those behind them) */
#endif
        // blocks held in registers for the whole solve.  The quadruped classes hold five - the exchange's straight part; blocks 5-7, read by the rare wave with more
        // than five contacts per env, are fetched in the pass that needs them.  Eight cost 27 registers: the pipelined classes (| 16) then no longer fit their budget
        // of 416 (step_kernel.h: a wave of the action stage must fit beside them; tests/test_kernel_budget.py), and the others run 0.7 % slower for the spill moves
        // (286.8 against 284.7 M env-steps/s on the specialised resident class, profiles/r06_spec_log.txt #7).
#ifndef RSB_X_NPK_QUAD
#define RSB_X_NPK_QUAD 5
#endif
        constexpr int NPK = TRI ? RSB_X_NPK_TRI : RSB_X_NPK_QUAD;
        typedef float float2v __attribute__((ext_vector_type(2)));
        float g0[PK ? 1 : 4][3][4];   // coupling blocks with contacts 0-3: constant during the solve, read from LDS once
        float g1[PK ? 1 : 4][3][4];   // ... and with contacts 4-7 (the hard envs of the tail have five contacts: no LDS round trip in their passes)
        float2v gp[PK ? NPK : 1][3];  // PK: rows (0, 1) of column c of the block with contact k
        float gr[PK ? NPK : 1][3];    // PK: row 2
        if constexpr (PK && !TRI) {
          // (the exchange reads blocks 0-4 whatever the count; 5-7 only behind its `ncw > 5` tests: the usual wave - four or five contacts per env - does not load them)
          RSB_UNROLL for (int k = 0; k < NPK; ++k) {
#if RSB_FLAT_SETUP_HEAD
            static_assert(NPK >= 5, "flat set-up: batch A reads the five blocks of the exchange's straight part");
            if (k < 5) {      // (read with batch A)
              gp[k][0] = float2v{fq0[k][0], fq0[k][1]}; gp[k][1] = float2v{fq0[k][2], fq0[k][3]}; gp[k][2] = float2v{fq1[k][0], fq1[k][1]};
              gr[k][0] = fq1[k][2]; gr[k][1] = fq1[k][3]; gr[k][2] = fq2[k < 5 ? k : 0];
            } else
#endif
            if (k < 5 || ncw > 5) {
              if constexpr (GROWS) {   // the block is stored as the pairs and the third row: two 16-byte reads and one scalar
                float q0[4], q1[4];
                ld4(Gmine + kGBlock * k, q0); ld4(Gmine + kGBlock * k + 4, q1);
                gp[k][0] = float2v{q0[0], q0[1]}; gp[k][1] = float2v{q0[2], q0[3]}; gp[k][2] = float2v{q1[0], q1[1]};
                gr[k][0] = q1[2]; gr[k][1] = q1[3]; gr[k][2] = Gmine[kGBlock * k + 8];
              } else {
                RSB_UNROLL for (int cc = 0; cc < 3; ++cc) {
                  gp[k][cc] = float2v{Gmine[4 * k + cc], Gmine[GS + 4 * k + cc]};
                  gr[k][cc] = Gmine[2 * GS + 4 * k + cc];
                }
              }
            }
          }
        } else if constexpr (PK) {   // packed-triangular layout: the block or its transpose, then paired (the selects write the pairs directly)
          RSB_UNROLL for (int k = 0; k < NPK; ++k) {
            float t[3][4];
            coupling(k, t);
            RSB_UNROLL for (int cc = 0; cc < 3; ++cc) { gp[k][cc] = float2v{t[0][cc], t[1][cc]}; gr[k][cc] = t[2][cc]; }
          }
        } else {
          RSB_UNROLL for (int k = 0; k < 4; ++k) coupling(k, g0[k]);
          RSB_UNROLL for (int k = 0; k < 4; ++k) coupling(4 + k, g1[k]);
        }
        float g2[(KMAX > 8 && !PK) ? 4 : 1][3][4];   // ... and, in the large-model classes, with contacts 8-11 (a collapsed humanoid)
        if constexpr (KMAX > 8 && !PK) {
          RSB_UNROLL for (int k = 0; k < 4; ++k) coupling(8 + k, g2[k]);
        }
        float gbuf[2][4][3][4];       // contacts 12.. : fetched per pass
        auto load_block = [&](auto bc) {
          constexpr int b = decltype(bc)::value;
          RSB_UNROLL for (int k = 0; k < 4; ++k) coupling(4 * b + k, gbuf[b & 1][k]);
        };
        auto exchange = [&](const float (&x)[3], float& emax) {
          auto one = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            float l0[3] = {x[0], x[1], x[2]};
            row_bcast_n<j, 3>(l0);
            if constexpr (PK && j < NPK) {
              float2v acc = {v[0], v[1]};
              RSB_UNROLL for (int cc = 0; cc < 3; ++cc) acc = __builtin_elementwise_fma(gp[j][cc], float2v{l0[cc], l0[cc]}, acc);
              v[0] = acc.x; v[1] = acc.y;
              v[2] = fmaf(gr[j][2], l0[2], fmaf(gr[j][1], l0[1], fmaf(gr[j][0], l0[0], v[2])));
            } else if constexpr (PK && !TRI && j < 8) {      // (NPK < 8: a block of contacts 5-7 that is not held in registers)
              float gt[3][4];
              coupling(j, gt);
              RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
                v[rr] = fmaf(gt[rr][2], l0[2], fmaf(gt[rr][1], l0[1], fmaf(gt[rr][0], l0[0], v[rr])));
            } else {
              const float (&gj)[3][4] = PK ? gbuf[(j / 4) & 1][j & 3] : (j < 4 ? g0[PK ? 0 : (j & 3)] : (j < 8 ? g1[PK ? 0 : (j & 3)] : (j < 12 ? g2[(KMAX > 8 && !PK ? j : 0) & 3] : gbuf[(j / 4) & 1][j & 3])));
              RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
                v[rr] = fmaf(gj[rr][2], l0[2], fmaf(gj[rr][1], l0[1], fmaf(gj[rr][0], l0[0], v[rr])));
            }
            emax = fmaxf(emax, fmaxf(fabsf(l0[0]), fmaxf(fabsf(l0[1]), fabsf(l0[2]))));
          };
          // contacts 0-4 straight: the launch lasts as long as its slowest wave, and that wave holds a five-contact env (a robot
          // on a knee); the usual four-contact waves finish a third earlier and can afford the one unused exchange
          // (pipelined classes run at the MEAN wave; putting the fifth contact behind a test there measured +0.4 %, inside the noise of the
          // loop's fetch-window phase: one code path for both)
          static_for<0, 5>(one);
          {
#if RSB_SWEEP_LOOP
            if (__builtin_expect(ncw > 5, 0)) {      // (out of line: the pass test then follows the straight part, and the next pass's rule follows the test)
#else
            if (ncw > 5) {
#endif
              one(std::integral_constant<int, 5>{});
              if (ncw > 6) {
                one(std::integral_constant<int, 6>{});
                if (ncw > 7) {
                  one(std::integral_constant<int, 7>{});
                  static_for<2, KMAX / 4>([&](auto bc) {
                    constexpr int b = decltype(bc)::value;
                    if (4 * b < ncw) {   // (these blocks load late: only models with many contacts per env get here)
                      if constexpr (b >= 3 || (PK && 4 * b >= NPK)) load_block(bc);
                      static_for<4 * b, 4 * b + 4>(one);
                    }
                  });
                }
              }
            }
          }
        };

        // warm start (oracle: lam_warm): the impulse and friction direction this collision primitive had at the end of
        // the previous integrate(); the table is then cleared, contacts alive at the end of this solve re-enter it
        if (has_warm) {
#if RSB_FLAT_SETUP_HEAD
          {
            const bool wok = isc && mycol < ncol;   // joint-limit rows (ids >= ncol) start cold: the row read with batch B is taken or dropped whole
            lam[0] = wok ? fwr[0] : 0.f; lam[1] = wok ? fwr[1] : 0.f; lam[2] = wok ? fwr[2] : 0.f;
            sdx = wok ? fwr[3] : 0.f; sdy = wok ? fwr[4] : 0.f; sdst = (wok && fwr[5] != 0.f) ? 3 : 0;
          }
          // the table is cleared by straight stores: a compile-time trip count, the last trip's index clamped to the table's last float (several lanes then store
          // the same zero to it) - no region, no skip branch
          {
            constexpr int kNw = 6 * RSB_SPEC_NCOL, kTrips = (kNw + LPE - 1) / LPE;
            RSB_UNROLL for (int t = 0; t < kTrips; ++t) WARM[(LPE * (t + 1) <= kNw) ? s + LPE * t : min(s + LPE * t, kNw - 1)] = 0.f;
          }
#else
          if (isc) {
            if (mycol < ncol) {   // joint-limit rows (ids >= ncol) start cold
              const float* wr = WARM + 6 * mycol;
              lam[0] = wr[0]; lam[1] = wr[1]; lam[2] = wr[2];
              sdx = wr[3]; sdy = wr[4]; sdst = wr[5] != 0.f ? 3 : 0;
            }
          }
          for (int i = s; i < nwarm; i += LPE) WARM[i] = 0.f;
#endif
#if RSB_FLAT_SETUP_HEAD
          if (__any(isc & ((lam[0] != 0.f) | (lam[1] != 0.f) | (lam[2] != 0.f)))) {      // (no short circuit: the compiler builds a region for one)
#else
          if (__any(isc && (lam[0] != 0.f || lam[1] != 0.f || lam[2] != 0.f))) {
#endif
            // v = c + G lam(0): one exchange of the inherited impulses (v carries the own impulse as well)
            float unused = 0.f;
            exchange(lam, unused);
          }
        }
        if (PROF && pfine) { t_prev = t_gs0; lap(t_setup); }
#if RSB_FLAT_CLASS
        asm volatile("; rsb setup end");
#endif

        // global search of contact j's direction by its 16-lane row (coefficients broadcast from lane j)
        auto search_row = [&](int j, const SlipCoef& kc, bool take) {
          if (PROF && a.prof) ++p_search;
          float c12[13] = {kc.a0, kc.a1, kc.a2, kc.n00, kc.n01, kc.n02, kc.n10, kc.n11, kc.n12, kc.vn, kc.ls0, kc.ls1, mu};
          row_bcast_dyn_n<KMAX, 13>(c12, j);
          SlipCoef kb;
          kb.a0 = c12[0]; kb.a1 = c12[1]; kb.a2 = c12[2]; kb.n00 = c12[3]; kb.n01 = c12[4]; kb.n02 = c12[5];
          kb.n10 = c12[6]; kb.n11 = c12[7]; kb.n12 = c12[8]; kb.vn = c12[9]; kb.ls0 = c12[10]; kb.ls1 = c12[11];
          float dxy[2];
          slip_search<LPE, COUL>(kb, c12[12], section_rounds, s, el, c16, s16, DIR16, dxy);
          if (take) { sdx = dxy[0]; sdy = dxy[1]; sdst = 1; }
        };

        // Every branch costs a lone wave ~20-45 cycles taken or not (profiles/r02_ubench_lone_wave_latency.txt), i.e. as much
        // as 5-10 VALU instructions: the pass is written with selects, the branches that remain guard work that is rare and large.
        // The sweep loop's place in the 32-byte instruction-fetch windows is pinned here instead of left to whatever code precedes it: the
        // same kernel shifted by n x 4 bytes measures 147.6 ... 149.5 M env-steps/s with a period of 32 bytes (profiles/r03_ab_log.txt, "alignment
        // sweep": a lone wave has nobody to hide a fetch bubble behind), and two unrelated commits had moved it from the best phase to the
        // worst.  Phase found by sweep for the quadruped classes - and again after the loop body changed (packed fp32 in the exchange: k = 0..7
        // 149.9 151.6 151.4 150.1 149.4 149.4 148.9 149.7 M; before that change k = 5-6 was the place to be); executed once per solve.
        // RSB_X_ALIGN_SWEEP overrides the phase for a new sweep: a change of the loop body needs one.
#if !defined(RSB_X_ALIGN_SWEEP) && defined(RSB_SPECIALIZED)
#define RSB_X_ALIGN_SWEEP 0   /* specialised code objects have another loop body: swept on config 2's resident class, k = 0..7: 288.5 287.5 286.8 286.0 285.6 287.0 287.9 287.0 M */
#endif
#ifndef RSB_X_ALIGN_SWEEP
#define RSB_X_ALIGN_SWEEP 7   /* (re-swept after the packed sums of the up pass moved one instruction of the loop body: 151.1 150.0 150.1 149.5 150.6 150.6 151.4 152.1) */
#endif
        // The large-model classes (measured on the Atlas-like instance, config 5): phases 0-3 17.7-17.8 M, 4-7 17.4 M, unpinned 17.5 M; with the
        // packed exchange k = 0..7: 18.40 18.40 18.35 18.21 18.03 17.93 18.19 18.30 M.
#ifndef RSB_X_ALIGN_SWEEP_TRI
#define RSB_X_ALIGN_SWEEP_TRI 7   /* (with the packed sums of the up pass, k = 0, 2..7: 18.23 18.39 17.89 18.21 18.40 18.41 18.47; k = 1: 18.33) */
#endif
        asm volatile(".p2align 5");
        static_for<0, (TRI ? RSB_X_ALIGN_SWEEP_TRI : RSB_X_ALIGN_SWEEP)>([&](auto) { asm volatile("s_nop 0"); });
#if RSB_PK_CLASS
        asm volatile("; rsb sweep begin");     // (tests/test_pk_solve_host.py counts between the comment lines)
#endif
#if RSB_SWEEP_LOOP
        // bottom-tested loops on scalar counters (step_spec.h: RSB_SWEEP_LOOP): a solve runs one sweep at least when max_iter allows any, a sweep one pass at least
        static_assert(!(TRI || RSB_X_AA8), "sweep control: the Anderson step sits behind the exit test of the loop it replaces");
        // What a sweep starts from - no pass run yet, no change seen, the env's live contact lanes - is set up in front of the loop and again in front of its back edge,
        // as values the compiler cannot see through: the sweep loop's header then holds no instruction, and the back edge lands on the first pass's rule.
        int it = 0, kp = 0;
        float err = 0.f;
        bool act = isc & !done;
        asm volatile("" : "+s"(kp), "+v"(err));
        if (max_iter > 0) for (;;) {
#else
        for (int it = 0; it < max_iter; ++it) {
#endif
          // lagged directions: a usable direction of this solve is no longer refreshed.  Two wave-uniform tests picked per env by a
          // lane mask (scalar work: the sweep loop has no vector register to spare)
#if !RSB_SWEEP_LOOP
          const bool lag = multi ? (multi_fa > 0 && it >= multi_fa) : (freeze_after > 0 && it >= freeze_after);
          float err = 0.f;
#endif
          float dl_last[3] = {0.f, 0.f, 0.f};
          if constexpr (AA) { aa_x[0] = lam[0]; aa_x[1] = lam[1]; aa_x[2] = lam[2]; }
#if RSB_SWEEP_LOOP
          do {
            asm volatile("; rsb sweep control end" : "+s"(kp), "+s"(it));     // (the loop control ends where a pass's rule begins)
            const bool lag = multi ? (multi_fa > 0 && it >= multi_fa) : (freeze_after > 0 && it >= freeze_after);      // (per pass, from the pinned counter: three scalar instructions)
            const bool mine = act & (gpos == kp);
#else
          for (int kp = 0; kp < gdw; ++kp) {
            const bool mine = isc & !done & (gpos == kp);
#endif
            if (PROF && a.prof) ++p_solves;
            // v holds the velocity WITH the own impulse: lam_stick = lam - G_ii^-1 v, v_n without it = v_n - G_ii[n,:] lam
            float ls[3];
#if RSB_PK_SOLVE
            const f32x2 ls01 = pk_stick(gip, f32x2{v[0], v[1]}, v[2], f32x2{lam[0], lam[1]});
            ls[0] = ls01.x; ls[1] = ls01.y;
            ls[2] = fmaf(-Ginv[8], v[2], fmaf(-Ginv[7], v[1], fmaf(-Ginv[6], v[0], lam[2])));
#else
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
              ls[rr] = fmaf(-Ginv[3 * rr + 2], v[2], fmaf(-Ginv[3 * rr + 1], v[1], fmaf(-Ginv[3 * rr], v[0], lam[rr])));
#endif
            const float vexn = fmaf(-Gii[8], lam[2], fmaf(-Gii[7], lam[1], fmaf(-Gii[6], lam[0], v[2])));
            const bool open = vexn > 0.f;
            const bool stick = (!open) & (ls[2] >= 0.f) & (fmaf(ls[1], ls[1], ls[0] * ls[0]) <= (mu2 * ls[2]) * ls[2]);
            const bool slip = (!open) & (!stick);
            const bool usable = (sdst == 1) & (fmaf(sc.a2, sdy, fmaf(sc.a1, sdx, sc.a0)) >= kDenFreeze * sc.a0);
            const bool keep = lag & usable;
            // who refreshes its direction in this pass: the pass's members; in an env with light passes every contact in pass 0
#if RSB_SWEEP_LOOP
            const bool refr = act & (light ? (kp == 0) : (gpos == kp));
#else
            const bool refr = isc & !done & (light ? (kp == 0) : (gpos == kp));
#endif
            bool need = refr & slip & !keep;
            // a member of a light pass keeps its direction; without a usable one (it started to slip after pass 0) it searches
            const bool lost = mine & slip & !refr & !usable;
            lap(t_rule);
#ifdef RSB_X_NO_NEWTON   /* (deletion experiment: what the direction refresh costs; results are wrong) */
            if (false) {
#else
            if (__any(need | lost)) {
#endif
              SlipCoef kc;
              kc = sc;
#if RSB_PK_SOLVE
              SlipCoefPk kp;
              pk_coef(kp, sc.a0, sc.a1, sc.a2, gcp[2], mg1, mg2, pk_vex(gcp, f32x2{v[0], v[1]}, f32x2{lam[0], lam[1]}, lam[2]), vexn, ls01);
              kc = slip_unpack(kp);      // (the serial scan, the quad scan and the global search read the scalar record: the same registers)
#else
              {
                const float vex0 = v[0] - (Gii[0] * lam[0] + Gii[1] * lam[1] + Gii[2] * lam[2]);
                const float vex1 = v[1] - (Gii[3] * lam[0] + Gii[4] * lam[1] + Gii[5] * lam[2]);
                kc.n00 = sc.a0 * vex0 - vexn * Gii[2]; kc.n01 = sc.a1 * vex0 - vexn * sc.n01; kc.n02 = sc.a2 * vex0 - vexn * sc.n02;
                kc.n10 = sc.a0 * vex1 - vexn * Gii[5]; kc.n11 = sc.a1 * vex1 - vexn * sc.n11; kc.n12 = sc.a2 * vex1 - vexn * sc.n12;
                kc.vn = vexn; kc.ls0 = ls[0]; kc.ls1 = ls[1];
              }
#endif
              // one guarded Newton step on every lane (the common case; lanes without a candidate ignore the result)
              if (PROF && a.prof) ++p_newton;
              bool p_cont = false;      // (profiling twin: a continuation of the step ran in this block)
              float nx, ny, dstep;
#if RSB_PK_SOLVE
              // the Newton step's core, then ONE test for everything that may follow it (step_spec.h: RSB_SWEEP_RARE): a step above 0.02 rad of a lane that takes it
              // (energy check), an inherited direction in the first sweep (basin check), a lane whose step was refused or that lost its direction (global search)
              f32x2 nxy;
              float den0, den1;
              const bool okcore = slip_newton_core_pk(kp, sdx, sdy, nxy, dstep, den0, den1);
              nx = nxy.x; ny = nxy.y;
              const bool okc = okcore & need & (sdst != 0) & (refine != 0);
#ifdef RSB_X_NO_BASIN
              const bool rare_l = (okc & (fabsf(dstep) > 0.02f)) | (need & !okc) | lost;
#else
              const bool rare_l = (okc & (fabsf(dstep) > 0.02f)) | ((it == 0) & okc & (sdst == 3)) | (need & !okc) | lost;
#endif
              if (PROF && pctl) {      // (the twin of the code without the test counts what the test would have said)
                if (it == 0) ++p_ctl[kCtlNewtonFirst];
                const bool pr = __any(rare_l);
                if (pr) ++p_ctl[it == 0 ? kCtlRareFirst : kCtlRareLater];
                // (the energy check is counted where it runs: behind the test only where the test is compiled)
                if ((RSB_SWEEP_RARE ? pr : true) && __any(okcore & (fabsf(dstep) > 0.02f))) { ++p_ctl[it == 0 ? kCtlEnergyFirst : kCtlEnergyLater]; p_cont = true; }
              }
#if RSB_SWEEP_RARE
              bool okf = okc;
              const bool p_rare = __any(rare_l);
              if (__builtin_expect(p_rare, 1)) {      // (the slow block stays in line and the fast side jumps over it - hinted, so that every twin keeps this layout: out of line it costs the pipelined class's twin of the Delassus switch a spill)
#endif
              bool ok = slip_newton_energy_pk(kp, mu, sdx, sdy, nxy, dstep, den0, den1, okcore) & need & (sdst != 0) & (refine != 0);
#else
              bool ok = slip_newton<COUL>(kc, mu, sdx, sdy, nx, ny, dstep) & need & (sdst != 0) & (refine != 0);
#endif
#ifdef RSB_X_STAMP_BASIN   /* (profiling twins, RSB_PROF_FINE: the basin-check block is charged to the `magnitude + dl` accumulator instead of the refresh's) */
              lap(t_newt);
#endif
#ifdef RSB_X_NO_BASIN   /* (deletion experiment: what the basin check costs; results differ) */
              if (false) {
#else
              if (it == 0 && !COUL) {      // (Coulomb: an inherited direction was a root of the previous step's problem - no basin to check)
#endif
                const bool chk = ok & (sdst == 3);
                if (__any(chk)) {
                  if (PROF && pctl) { ++p_ctl[ncw <= 4 ? kCtlBasinQuad : kCtlBasinSerial]; p_cont = true; }
                  // basin check (oracle: "basin check"): a direction inherited from the previous integrate() may sit in the
                  // local minimum the global search would not choose; it is accepted only if it is at least as good as every
                  // direction of the search's coarse scan.  Every contact lane scans the 16 directions of its OWN contact.
                  // With at most four contacts per env in the wave the four lanes 4 j .. 4 j + 3 of the env's first row scan four directions each of contact j
                  // (coefficients fetched from lane j, quad minimum, back to lane j): the same sixteen energies for a quarter of the instructions.  (Same to
                  // the last bit on twelve directions; on the four axis directions the serial scan's literal zeros and ones let the compiler fuse another
                  // product of vt0 A + vt1 B, one rounding apart - tools/ubench/basin_quad.hip.  The check compares energies that differ by far more.)
                  float ebest;
#ifndef RSB_X_SERIAL_BASIN   /* (the serial scan everywhere, for an A/B) */
                  if (ncw <= 4) {
                    const int row = lane & ~15, q = lane & 3;
                    const int from_owner = (row | ((lane >> 2) & 3)) << 2, from_quad = (row | ((lane & 3) << 2)) << 2;   // ds_bpermute addresses: 4 x source lane
                    float c13[13] = {kc.a0, kc.a1, kc.a2, kc.n00, kc.n01, kc.n02, kc.n10, kc.n11, kc.n12, kc.vn, kc.ls0, kc.ls1, mu};
                    RSB_UNROLL for (int i = 0; i < 13; ++i) c13[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(from_owner, __float_as_int(c13[i])));
                    SlipCoef kq;
                    kq.a0 = c13[0]; kq.a1 = c13[1]; kq.a2 = c13[2]; kq.n00 = c13[3]; kq.n01 = c13[4]; kq.n02 = c13[5];
                    kq.n10 = c13[6]; kq.n11 = c13[7]; kq.n12 = c13[8]; kq.vn = c13[9]; kq.ls0 = c13[10]; kq.ls1 = c13[11];
                    float e = __int_as_float(0x7f800000);
                    // direction 4 q + i of the coarse scan's table = direction i turned by q quarter turns: (c, s), (-s, c), (-c, -s), (s, -c) - a swap and two sign
                    // bits per lane on the table's first four literals (written as a four-way choice among table entries the compiler turns it into eight
                    // loads from constant MEMORY: 2 000 cycles for a lone wave, measured)
                    const bool swp = (q & 1) != 0;
                    const unsigned sgx = ((q + 1) & 2) ? 0x80000000u : 0u, sgy = (q & 2) ? 0x80000000u : 0u;
                    RSB_UNROLL for (int i = 0; i < 4; ++i) {
                      const float x = __uint_as_float(__float_as_uint(swp ? kSin16[i] : kCos16[i]) ^ sgx);
                      const float y = __uint_as_float(__float_as_uint(swp ? kCos16[i] : kSin16[i]) ^ sgy);
                      e = fminf(e, slip_E(kq, c13[12], x, y));
                    }
                    e = fminf(e, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(e), 0xB1, 0xf, 0xf, true)));   // quad_perm [1,0,3,2]
                    e = fminf(e, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(e), 0x4E, 0xf, 0xf, true)));   // quad_perm [2,3,0,1]
                    ebest = __int_as_float(__builtin_amdgcn_ds_bpermute(from_quad, __float_as_int(e)));
#ifdef RSB_X_BASIN_VERIFY   /* (debug: the serial scan beside it; a mismatch on a lane that uses the value sets flag bit 16) */
                    {
                      float e2 = slip_E(kc, mu, 1.0f, 0.0f);
                      RSB_UNROLL for (int i = 1; i < 16; ++i) e2 = fminf(e2, slip_E(kc, mu, kCos16[i], kSin16[i]));
                      if (chk && __float_as_int(e2) != __float_as_int(ebest)) flag |= 16;
                    }
#endif
                  } else
#endif
                  {
                    // (den(d) of the sixteen literal directions depends on nothing the sweeps change: left to itself the compiler computes the sixteen
                    //  reciprocals before the sweep loop, in every solve, for a branch few waves take - the empty asm pins them here)
                    SlipCoef ks = kc;
#ifndef RSB_X_SERIAL_BASIN
                    asm volatile("" : "+v"(ks.a0), "+v"(ks.a1), "+v"(ks.a2));
#endif
                    ebest = slip_E(ks, mu, 1.0f, 0.0f);
                    RSB_UNROLL for (int i = 1; i < 16; ++i) ebest = fminf(ebest, slip_E(ks, mu, kCos16[i], kSin16[i]));
                  }
                  ok = ok & !(chk & !(slip_E(kc, mu, nx, ny) <= ebest));
                }
              }
#ifdef RSB_X_STAMP_BASIN
              lap(t_mag);
#endif
              if (PROF && pctl) { if (__any(need & (sdst != 0) & !ok)) ++p_ctl[kCtlRefused]; }
              sdx = ok ? nx : sdx; sdy = ok ? ny : sdy; sdst = ok ? 1 : sdst;
              need = (need & !ok) | lost;
              if (__any(need)) {
                if (PROF && pctl) { ++p_ctl[it == 0 ? kCtlSearchFirst : kCtlSearchLater]; p_cont = true; }
                for (int j = 0; j < ncw; ++j)
                  if (__any(need && s == j)) search_row(j, kc, need && s == j);
              }
              if (PROF && pctl) { if (!p_cont) ++p_ctl[it == 0 ? kCtlNoneFirst : kCtlNoneLater]; }
              lap(t_newt);
#if RSB_SWEEP_RARE
                okf = false;      // (everything is taken: the selects below change nothing)
              }
              // the usual case comes here straight from the test: ok is okc, nobody searches - the step is taken by the selects and the pass goes on with the magnitude
              asm volatile("; rsb refresh fast begin" : "+v"(sdx), "+v"(sdy), "+v"(sdst));     // (tests/test_sweep_control_host.py counts between the comment lines)
              sdx = okf ? nx : sdx; sdy = okf ? ny : sdy; sdst = okf ? 1 : sdst;
              asm volatile("; rsb refresh fast end" : "+v"(sdx), "+v"(sdy), "+v"(sdst));
              if (PROF && pctl) { if (!p_rare) ++p_ctl[it == 0 ? kCtlNoneFirst : kCtlNoneLater]; }
              if (PROF && pfine) { if (!p_rare) {
#ifdef RSB_X_STAMP_BASIN
                lap(t_newt);
                lap(t_mag);
#endif
                lap(t_newt);
              } }
#endif
            }
            // impulse along the direction: v_n^+ = 0 on the cone boundary
            const float den = fmaf(sc.a2, sdy, fmaf(sc.a1, sdx, sc.a0));
            const float lnn = -vexn * __builtin_amdgcn_rcpf(fmaxf(den, kDenMin * sc.a0));
            const float ltn = mu * lnn;
            float ln[3];
            float dl[3];
#if RSB_PK_SOLVE
            {
              const f32x2 lt = pk_splat(ltn) * f32x2{sdx, sdy};
              ln[0] = slip ? lt.x : (stick ? ls[0] : 0.f);
              ln[1] = slip ? lt.y : (stick ? ls[1] : 0.f);
              ln[2] = slip ? lnn : (stick ? ls[2] : 0.f);
              const f32x2 l01 = f32x2{lam[0], lam[1]}, df = pk_splat(alpha) * (f32x2{ln[0], ln[1]} - l01);   // (a product of a difference: nothing to fuse)
              dl[0] = mine ? df.x : 0.f; dl[1] = mine ? df.y : 0.f;
              dl[2] = mine ? alpha * (ln[2] - lam[2]) : 0.f;
              const f32x2 ln01 = l01 + f32x2{dl[0], dl[1]};
              lam[0] = ln01.x; lam[1] = ln01.y; lam[2] += dl[2];
            }
#else
            ln[0] = slip ? ltn * sdx : (stick ? ls[0] : 0.f);
            ln[1] = slip ? ltn * sdy : (stick ? ls[1] : 0.f);
            ln[2] = slip ? lnn : (stick ? ls[2] : 0.f);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
              dl[rr] = mine ? alpha * (ln[rr] - lam[rr]) : 0.f;
              lam[rr] += dl[rr];
            }
#endif
            lap(t_mag);
            if constexpr (AA) {
              // the last pass's exchange waits for the Anderson step (one exchange carries both changes)
              if (kp + 1 < gdw) exchange(dl, err);
              else { dl_last[0] = dl[0]; dl_last[1] = dl[1]; dl_last[2] = dl[2]; }
            } else {
              exchange(dl, err);
            }
            lap(t_exch);
#if RSB_SWEEP_LOOP
            asm volatile("; rsb sweep control begin");     // (tests/test_sweep_control_host.py follows every path from here to the comment line at the head of a pass)
            ++kp;
            asm volatile("" : "+s"(kp));
          } while (__builtin_expect(kp < gdw, 0));      // (the usual env has one contact per limb: one pass per sweep, and the epilogue follows the test)
#else
          }
#endif
          if constexpr (AA)   // the deferred pass's share of the sweep's largest change (its members sit in the env's first row)
            err = fmaxf(err, row_max_f32(fmaxf(fabsf(dl_last[0]), fmaxf(fabsf(dl_last[1]), fabsf(dl_last[2])))));
          // an inherited direction that the first sweep did not pick up is dropped (oracle: same rule): a contact that starts
          // to slip later in the solve runs the global search
          if (it == 0) sdst = (sdst == 3) ? 0 : sdst;
          // ---------------- convergence: relative (fp32-aware) test and stagnation exit, identical to the oracle's
          // (rsb_oracle.c), written with selects (every lane of the env carries the same err / scale)
          const float scale = row_max_f32(isc ? lam[2] : 0.f);   // largest normal impulse of the env (contact lanes sit in the group's first row)
          {
            const bool live = !done;
            iters_used += live ? 1 : 0;
            alpha = fmaxf(alpha * alpha_decay, alpha_min);
            const float denom = scale + kLambdaFloor;
            const bool conv_now = live & (err <= threshold * denom);
            const float rel = err * __builtin_amdgcn_rcpf(denom);   // only ranks iterates (calmest iterate, stagnation window)
            const bool cont = live & !conv_now;
            const bool better = cont & (rel < best_rel);      // the calmest iterate so far
            best_rel = better ? rel : best_rel;
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) lam_best[rr] = better ? lam[rr] : lam_best[rr];
            best_cur = cont ? fminf(best_cur, rel) : best_cur;
            wcount += cont ? 1 : 0;
            const bool wfull = cont & (wcount == sw_env);
            const bool stalled = wfull & (best_cur > stall_factor * best_prev);
            best_prev = wfull ? best_cur : best_prev;
            best_cur = wfull ? 3e38f : best_cur;
            wcount = wfull ? 0 : wcount;
            converged |= conv_now;
            done |= conv_now | stalled;
#if RSB_SWEEP_LOOP
            act = act & !(conv_now | stalled);      // (= isc & !done, carried: written like the set-up's it is formed in the header again)
#endif
          }
          lap(t_epi);
#if RSB_SWEEP_LOOP
          // "another sweep" is one test: the lanes not yet done, none of them once the sweep count is used up
          ++it;
          kp = 0; err = 0.f;
          asm volatile("" : "+s"(it), "+s"(kp), "+v"(err));
          {
            unsigned long long live = __builtin_amdgcn_ballot_w64(!done);
            live = (it < max_iter) ? live : 0ull;
            asm volatile("" : "+s"(live));      // (pinned: left alone the compiler turns the fold back into a branch of its own around the epilogue's selects)
            if (live == 0ull) break;
          }
#else
          if (!__any(!done)) break;
#endif
          if constexpr (AA) {
            if (__any(aa_on & !done)) {
              // x+ = g - gamma (g - g_prev), gamma = <r, r - r_prev> / |r - r_prev|^2 over the env's contacts (they sit in the env's
              // first row: one DPP row reduction each), back into the cone; the change rides on the last pass's deferred exchange
              float rr[3], num = 0.f, den = 0.f;
              RSB_UNROLL for (int q2 = 0; q2 < 3; ++q2) {
                rr[q2] = lam[q2] - aa_x[q2];
                const float dr = rr[q2] - aa_r[q2];
                num = fmaf(rr[q2], dr, num); den = fmaf(dr, dr, den);
              }
              num = row_sum_f32(isc ? num : 0.f); den = row_sum_f32(isc ? den : 0.f);
              if constexpr (LPE > 16) {   // (lanes beyond the env's first row hold no contact; they follow the first row's verdict for uniformity only)
                num = __shfl(num, (lane & ~(LPE - 1)) | (lane & 15)); den = __shfl(den, (lane & ~(LPE - 1)) | (lane & 15));
              }
              const bool use = aa_on & !done & (it >= 1) & (it + 1 >= aa_first) & (den > 1e-30f);
              float gam = use ? num / den : 0.f;
              gam = (fabsf(gam) <= aa_clip) ? gam : 0.f;
              float xn[3], dl[3];
              RSB_UNROLL for (int q2 = 0; q2 < 3; ++q2) { xn[q2] = fmaf(-gam, lam[q2] - aa_g[q2], lam[q2]); aa_g[q2] = lam[q2]; aa_r[q2] = rr[q2]; }
              const float t2 = fmaf(xn[1], xn[1], xn[0] * xn[0]), lim = mu * xn[2];
              const float sh = (t2 > lim * lim) ? lim * __builtin_amdgcn_rsqf(t2) : 1.f;
              const bool off = xn[2] <= 0.f;
              xn[0] = off ? 0.f : xn[0] * sh; xn[1] = off ? 0.f : xn[1] * sh; xn[2] = off ? 0.f : xn[2];
              const bool app = isc & (gam != 0.f);
              RSB_UNROLL for (int q2 = 0; q2 < 3; ++q2) { dl[q2] = app ? xn[q2] - lam[q2] : 0.f; lam[q2] += dl[q2]; dl_last[q2] += dl[q2]; }
            }
            float unused = 0.f;
            exchange(dl_last, unused);   // the last pass's changes + the Anderson step's
          }
        }
#if RSB_PK_CLASS
        asm volatile("; rsb sweep end");
#endif
#if RSB_FLAT_CLASS
        asm volatile("; rsb solver end begin");     // (tests/test_flat_setup_host.py counts between the comment lines)
#endif
        if (PROF && pfine) tz0 = t_prev;
#if RSB_FLAT_SETUP_END
        flag |= converged ? 0 : 4;      // (selects: the calmest iterate of an env that did not converge)
        lam[0] = converged ? lam[0] : lam_best[0]; lam[1] = converged ? lam[1] : lam_best[1]; lam[2] = converged ? lam[2] : lam_best[2];
#else
        if (!converged) { flag |= 4; lam[0] = lam_best[0]; lam[1] = lam_best[1]; lam[2] = lam_best[2]; }
#endif
        if (__any(nselfc > 0)) {   // the second entry of a self-collision carries the first one's impulse (in its opposite frame)
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
            const float up = __shfl_up(lam[rr], 1);
            lam[rr] = (mycol & kSelfB) ? up : lam[rr];
          }
        }
#if !RSB_FLAT_SETUP_END
        if (isc) {
          LAM[3 * s] = lam[0]; LAM[3 * s + 1] = lam[1]; LAM[3 * s + 2] = lam[2];
          if (has_warm && mycol < ncol) {
            float* wr = WARM + 6 * mycol;
            wr[0] = lam[0]; wr[1] = lam[1]; wr[2] = lam[2];
            wr[3] = sdst ? sdx : 0.f; wr[4] = sdst ? sdy : 0.f; wr[5] = sdst ? 1.f : 0.f;
          }
        }
#endif
        // W^T lam: the base entries are summed over the contact lanes by a DPP row reduction (contact lanes sit in the env's
        // first row; wider envs copy the sums to their other rows); the joint entries are scattered into WB of the
        // support chain with LDS float atomics (lanes of one instruction are served in lane order: reproducible)
        {
          const int sc2 = isc ? s : 0;
          const float* W0 = WC + 3 * sc2 * cw;
          float z0[8], z1[8], z2[8];
          ld4(W0, z0); ld4(W0 + 4, z0 + 4); ld4(W0 + cw, z1); ld4(W0 + cw + 4, z1 + 4); ld4(W0 + 2 * cw, z2); ld4(W0 + 2 * cw + 4, z2 + 4);
#if RSB_FLAT_SETUP_END
          // flat end (step_spec.h): ONE batch of reads in front of the row sums - the column's rows, its entries of level 3 and up, and the ancestor row where the
          // set-up did not leave it in registers - read by every lane (a lane without a contact reads contact 0's column and body 0's row, as it reads that column's
          // rows above); the contact lanes' ONE region then holds nothing but the stores and the three atomics.
          float zt[3][RSB_SPEC_DEPTH > 3 ? RSB_SPEC_DEPTH - 3 : 1];
          RSB_UNROLL for (int lv = 3; lv < RSB_SPEC_DEPTH; ++lv) { zt[0][lv - 3] = W0[5 + lv]; zt[1][lv - 3] = W0[cw + 5 + lv]; zt[2][lv - 3] = W0[2 * cw + 5 + lv]; }
          // (pinned: left alone the compiler sinks the reads whose only use is a contact lane's into regions of their own, each with its wait)
          RSB_UNROLL for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(z0[i]), "+v"(z1[i]), "+v"(z2[i]));
#if !RSB_FLAT_SETUP_HEAD
          int fanc[4] = {0, -1, -1, -1};
          {
            const int bi = isc ? __float_as_int(CON[sc2 * kConSlot + 7]) : 0;
#if RSB_SPEC_DEPTH == 4
            const int4 r4 = *reinterpret_cast<const int4*>(ANC + bi * 4); fanc[1] = r4.y; fanc[2] = r4.z; fanc[3] = r4.w;
#else
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) fanc[lv] = ANC[bi * RSB_SPEC_DEPTH + lv];
#endif
          }
#endif
#endif
          const float l0 = isc ? lam[0] : 0.f, l1 = isc ? lam[1] : 0.f, l2 = isc ? lam[2] : 0.f;
          // (select, not a product with a zero impulse: a lane without a contact reads column memory nobody wrote)
          RSB_UNROLL for (int i = 0; i < 6; ++i) wlam[i] = row_sum_f32(isc ? z0[i] * l0 + z1[i] * l1 + z2[i] * l2 : 0.f);
          if constexpr (LPE > 16) {   // body lanes beyond the env's first row need the sum too (level-1 bodies start from the base's delta-velocity)
            RSB_UNROLL for (int i = 0; i < 6; ++i) wlam[i] = __shfl(wlam[i], (lane & ~(LPE - 1)) | (lane & 15));
          }
#if RSB_FLAT_CLASS && !RSB_FLAT_SETUP_END
          asm volatile("; rsb scatter begin");     // (tests/test_flat_contact_host.py counts between the comment lines)
#endif
#if RSB_FLAT_SETUP_END
          if (isc) {
            // (the flat scatter below, on the reads of the batch above; the impulse and the warm record are stored in the same region)
            LAM[3 * s] = lam[0]; LAM[3 * s + 1] = lam[1]; LAM[3 * s + 2] = lam[2];
            if (has_warm && mycol < ncol) {
              float* wr = WARM + 6 * mycol;
              wr[0] = lam[0]; wr[1] = lam[1]; wr[2] = lam[2];
              wr[3] = sdst ? sdx : 0.f; wr[4] = sdst ? sdy : 0.f; wr[5] = sdst ? 1.f : 0.f;
            }
            asm volatile("; rsb scatter begin");     // (the scatter proper, inside the one region: tests/test_flat_contact_host.py counts between the comment lines)
            float* sink = WC + 3 * s * cw + kFlatSink;
            float wl[4] = {0.f, 0.f, 0.f, 0.f};
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
              float w0, w1, w2;
              if (lv < 3) { w0 = z0[5 + lv]; w1 = z1[5 + lv]; w2 = z2[5 + lv]; }
              else { w0 = zt[0][lv < 3 ? 0 : lv - 3]; w1 = zt[1][lv < 3 ? 0 : lv - 3]; w2 = zt[2][lv < 3 ? 0 : lv - 3]; }
              wl[lv] = w0 * lam[0] + w1 * lam[1] + w2 * lam[2];      // (a contact lane's l0..l2 ARE its impulse: read from there, the selects above stay out of this region)
            }
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
              float* dst = (fanc[lv] >= 0) ? &WB[fanc[lv] + 5] : sink;
              atomicAdd(dst, wl[lv]);
            }
            asm volatile("; rsb scatter end");
          }
#elif RSB_FLAT_SCATTER
          if (isc) {
            // flat form (step_spec.h): ONE region, the contact lanes'; inside it the atomics are issued straight, in their level order, behind every read.  A level
            // the body has no ancestor at adds onto the sink of the lane's own column - another address, so the lanes of an instruction that do add onto WB are
            // served in the order they always were.  (The lanes WITHOUT a contact stay masked off: an LDS float atomic costs per active lane, and forty-eight more
            // of them per instruction measured - 4 % on the benchmark, one sink for all of them or one per lane: DESIGN.md section 9.)
            const int bi = __float_as_int(CON[s * kConSlot + 7]);
            int anc[4] = {0, -1, -1, -1};
#if RSB_SPEC_DEPTH == 4
            { const int4 r4 = *reinterpret_cast<const int4*>(ANC + bi * 4); anc[1] = r4.y; anc[2] = r4.z; anc[3] = r4.w; }
#else
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) anc[lv] = ANC[bi * RSB_SPEC_DEPTH + lv];
#endif
            float* sink = WC + 3 * s * cw + kFlatSink;
            // (every read in front of the first atomic: the compiler moves no load across one)
            float wl[4] = {0.f, 0.f, 0.f, 0.f};
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
              float w0, w1, w2;
              if (lv < 3) { w0 = z0[5 + lv]; w1 = z1[5 + lv]; w2 = z2[5 + lv]; }
              else { w0 = W0[5 + lv]; w1 = W0[cw + 5 + lv]; w2 = W0[2 * cw + 5 + lv]; }
              wl[lv] = w0 * l0 + w1 * l1 + w2 * l2;
            }
            RSB_UNROLL for (int lv = 1; lv < RSB_SPEC_DEPTH; ++lv) {
              float* dst = (anc[lv] >= 0) ? &WB[anc[lv] + 5] : sink;
              atomicAdd(dst, wl[lv]);
            }
          }
#else
          if (isc) {
            const int bi = __float_as_int(CON[s * kConSlot + 7]);
            // (all ancestors first: read inside the loop, every one waits for its own LDS round trip - the compiler cannot move a load across the atomic before it)
            int anc[ML + 1];
            RSB_UNROLL for (int lv = 1; lv <= ML; ++lv) anc[lv] = (lv < depth) ? ANC[bi * depth + lv] : -1;
            RSB_UNROLL for (int lv = 1; lv <= ML; ++lv) {
              if (lv < depth) {
                const int b = anc[lv];
                if (b >= 0) {
                  float w0, w1, w2;
                  if (lv < 3) { w0 = z0[5 + lv]; w1 = z1[5 + lv]; w2 = z2[5 + lv]; }
                  else { w0 = W0[5 + lv]; w1 = W0[cw + 5 + lv]; w2 = W0[2 * cw + 5 + lv]; }
                  atomicAdd(&WB[b + 5], w0 * l0 + w1 * l1 + w2 * l2);
                }
              }
            }
          }
#endif
#if RSB_FLAT_CLASS && !RSB_FLAT_SETUP_END
          asm volatile("; rsb scatter end");
#endif
        }
#if RSB_FLAT_CLASS
        asm volatile("; rsb solver end end");
#endif
      }
      __syncthreads();
      if (PROF && pfine) t_end += clock64() - tz0;
      if (PROF && a.prof) { t_gs += clock64() - t_gs0; int itw = iters_used; RSB_UNROLL for (int off = LPE; off < 64; off <<= 1) itw = max(itw, __shfl_xor(itw, off)); p_iters += itw; p_ncw = max(p_ncw, ncw); }
      if (PROF && a.dbg && env == a.dbg_env && env_valid && s == 0) {
        const int n3 = 3 * nc_real;
        for (int i = 0; i < n3; ++i) a.dbg[1 + n3 * n3 + n3 + i] = LAM[i];
      }
