// step_phase_delassus.inc — fragment of rsb_step_kernel (inside `if (ncw > 0)`): Delassus blocks G_ij = W_i W_j^T (lane = contact pair), fixed-base compliance, self-collision folding
      // ========================= Delassus blocks G_ij = W_i W_j^T (lane = contact pair) ============
#if RSB_FLAT_CLASS
      asm volatile("; rsb delassus begin");     // (comment lines in the assembly: tests/test_flat_delassus_host.py counts the pair loop's instructions between them)
#endif
      const int npw = ncw * (ncw + 1) / 2;
#if RSB_FLAT_DELASSUS
      // flat form (step_spec.h).  The first trip - pairs 0..15: every pair of an env with at most five contacts, the only trip of the usual wave - takes (i, j) and
      // the two columns' offsets from the lane's launch constants (step_kernel.h: fd_*); a later trip decodes its pairs at the loop's back edge, which the usual wave
      // never takes.  ONE batch of reads by every lane - the rows of the two columns and three floats of the contact records; a lane whose pair its env does not have
      // reads pair (0, 0) - no region, and the results of such a lane go to a sink.  Every float keeps the expression and the operand order it has in the loop
      // of the other classes below.
      static_assert(GROWS && !TRI && !FIXED && LPE == 16 && KMAX == 8 && RSB_SPEC_DEPTH - 1 <= ML, "flat Delassus form: the row-block layout of the floating-base quadruped classes");
      // the sink: the 64 floats of the Delassus region behind the KMAX block rows (rsb_world.hip, make_layout_pitch: the region keeps the dense rows' 3 KMAX x (4 KMAX + 4)
      // floats); dead from the up pass's hand-over to the seam's zeroing, read by nobody in between.  Four slots of 16 floats, taken by lane
      static_assert(3 * KMAX * (4 * KMAX + 4) - KMAX * GRP >= 64, "flat Delassus form: the sink lies behind the block rows, inside the region");
      float* const fsink = G + KMAX * GRP + 16 * (s & 3);
      int fpi = fd_i, fpj = fd_j, fwi = fd_wi, fwj = fd_wj, fob = fd_ob, fot = fd_ot, fog = fd_og;
      for (int p0 = 0;;) {
        const bool has = fpj < nc, diag = fpi == fpj;
        const int i = has ? fpi : 0, j = has ? fpj : 0;
        const float* Wi = WC + (has ? fwi : 0);
        const float* Wj = WC + (has ? fwj : 0);
#if RSB_FLAT_SETUP_HEAD
        constexpr int CWC = 6 + RSB_SPEC_DEPTH - 1;
#else
        constexpr int CWC = 6 + ML;
#endif
        float wi[3][CWC], wj[3][CWC];
        RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
          RSB_UNROLL for (int q4 = 0; q4 < (CWC + 3) / 4; ++q4) {
            float t4[4], u4[4];
            ld4(Wi + rr * cw + 4 * q4, t4); ld4(Wj + rr * cw + 4 * q4, u4);
            RSB_UNROLL for (int e = 0; e < 4; ++e)
              if (4 * q4 + e < CWC) { wi[rr][4 * q4 + e] = t4[e]; wj[rr][4 * q4 + e] = u4[e]; }
          }
        }
        const float cbi = CON[i * kConSlot + 7], clim = CON[i * kConSlot + 15], cbj = CON[j * kConSlot + 7];
        __builtin_amdgcn_sched_barrier(0);      // (the whole batch is issued before its first result is waited for)
        // shared prefix of the two support chains.  The four chains are numbered consecutively and have NL bodies each (RSB_SPEC_UP_QUADS; the host compares this
        // form with the tree tables for every body pair before it sets the field - rsb_world.hip: delassus_closed_form_ok): body b >= 1 sits on limb (b - 1) / NL
        // at level (b - 1) % NL + 1, and two bodies share min(li, lj) levels on one limb, none otherwise (the base: level 0)
        constexpr unsigned NL = RSB_SPEC_DEPTH - 1;
        const int bi = __float_as_int(cbi), bj = __float_as_int(cbj);
        const unsigned ui = (unsigned)(bi - 1), uj = (unsigned)(bj - 1), gi_ = ui / NL, gj_ = uj / NL;
        const int li = bi > 0 ? (int)(ui - gi_ * NL) + 1 : 0, lj = bj > 0 ? (int)(uj - gj_ * NL) + 1 : 0;
        const int lca = gi_ == gj_ ? min(li, lj) : 0;
        float acc[9];
        RSB_UNROLL for (int q2 = 0; q2 < 9; ++q2) acc[q2] = 0.f;
        RSB_UNROLL for (int e = 0; e < CWC; ++e) {
          const bool on = e < 6 || e < 6 + lca;
          float av[3], bv[3];
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { av[rr] = on ? wi[rr][e] : 0.f; bv[rr] = on ? wj[rr][e] : 0.f; }
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
            RSB_UNROLL for (int cc = 0; cc < 3; ++cc) acc[3 * rr + cc] += av[rr] * bv[cc];
        }
        const bool lim = diag & (clim != 0.f);   // joint-limit row: dummy tangential diagonal
        acc[0] = lim ? 1.f : acc[0]; acc[4] = lim ? 1.f : acc[4];
        // block (i, j) into contact i's row and its transpose into contact j's.  A diagonal pair stores the same bits to the same address twice (both sides of every
        // product are the same column: av == bv, and a product commutes), so there is no i != j test
        const float B[3][3] = {{acc[0], acc[1], acc[2]}, {acc[3], acc[4], acc[5]}, {acc[6], acc[7], acc[8]}};
        const float Bt[3][3] = {{acc[0], acc[3], acc[6]}, {acc[1], acc[4], acc[7]}, {acc[2], acc[5], acc[8]}};
        gblk_store(has ? G + fob : fsink, B);
        gblk_store(has ? G + fot : fsink, Bt);
        // inv3 (step_math.h) with its contractions written out as the loop below compiles them in every quadruped class - a cofactor x y - z w is fma(x, y, -(z w)),
        // the determinant fma(A2, c2, fma(A0, c0, A1 c1)): computed by every lane, beside the stores, the compiler left ANOTHER product of the determinant unfused
        float gi[12];
        {
          const float* A = acc;
          auto cof = [](float x, float y, float z, float w) { return fmaf(x, y, -(z * w)); };
          const float c0 = cof(A[4], A[8], A[5], A[7]), c1 = cof(A[5], A[6], A[3], A[8]), c2 = cof(A[3], A[7], A[4], A[6]);
          const float id = 1.0f / fmaf(A[2], c2, fmaf(A[0], c0, A[1] * c1));
          gi[0] = c0 * id; gi[1] = cof(A[2], A[7], A[1], A[8]) * id; gi[2] = cof(A[1], A[5], A[2], A[4]) * id;
          gi[3] = c1 * id; gi[4] = cof(A[0], A[8], A[2], A[6]) * id; gi[5] = cof(A[2], A[3], A[0], A[5]) * id;
          gi[6] = c2 * id; gi[7] = cof(A[1], A[6], A[0], A[7]) * id; gi[8] = cof(A[0], A[4], A[1], A[3]) * id;
        }
        gi[9] = gi[10] = gi[11] = 0.f;
        stv<3>((has & diag) ? GINV + fog : fsink, gi);
        p0 += LPE;
        if (__builtin_expect(p0 >= npw, 1)) break;
        // (more than five contacts in an env of the wave: the next sixteen pairs, decoded as in the loop below)
        const int p = p0 + s;
        fpj = (int)((__builtin_sqrtf(8.0f * (float)p + 1.5f) - 1.0f) * 0.5f);
        fpi = p - ((fpj * (fpj + 1)) >> 1);
        fwi = 3 * fpi * cw; fwj = 3 * fpj * cw;
        fob = fpi * GRP + kGBlock * fpj; fot = fpj * GRP + kGBlock * fpi; fog = 12 * fpi;
      }
#else
      for (int p0 = 0; p0 < npw; p0 += LPE) {
        const int p = p0 + s;
        // pair p = j (j + 1) / 2 + i, i <= j, without the divergent search loop (up to KMAX branches of a lone wave): 8 p + 1 = (2 j + 1)^2 on the diagonal, the
        // half added under the root keeps the hardware's 1-ulp square root on the right side of the integer (margin 0.25 / (2 j + 1))
        const int j = (int)((__builtin_sqrtf(8.0f * (float)p + 1.5f) - 1.0f) * 0.5f);
        const int i = p - ((j * (j + 1)) >> 1);
        if (j < nc) {
          const int bi = __float_as_int(CON[i * kConSlot + 7]), bj = __float_as_int(CON[j * kConSlot + 7]);
          const int li = PARLV[bi] >> 8, lj = PARLV[bj] >> 8;
          // shared support = base (6 entries) + the common prefix of the two support chains; all loads independent
          int ai[ML], aj[ML];
#if defined(RSB_SPECIALIZED) && RSB_SPEC_DEPTH == 4
          {   // (four levels: one 16-byte read per ancestor row, independent of the levels' own round trip - see the contact columns)
            const int4 ri = *reinterpret_cast<const int4*>(ANC + bi * 4), rj = *reinterpret_cast<const int4*>(ANC + bj * 4);
            const int vi[4] = {ri.y, ri.z, ri.w, -1}, vj[4] = {rj.y, rj.z, rj.w, -2};
            RSB_UNROLL for (int l = 0; l < ML; ++l) {
              ai[l] = (l + 1 <= li && l < 3) ? vi[l < 3 ? l : 3] : -1;
              aj[l] = (l + 1 <= lj && l < 3) ? vj[l < 3 ? l : 3] : -2;
            }
          }
#else
          RSB_UNROLL for (int l = 0; l < ML; ++l) {
            ai[l] = (l + 1 <= li) ? ANC[bi * depth + l + 1] : -1;
            aj[l] = (l + 1 <= lj) ? ANC[bj * depth + l + 1] : -2;
          }
#endif
          int lca = 0;
          bool same = true;
          RSB_UNROLL for (int l = 0; l < ML; ++l) { same = same && (ai[l] == aj[l]); lca += same ? 1 : 0; }
#if RSB_FLAT_SETUP_HEAD
          constexpr int CWC = 6 + RSB_SPEC_DEPTH - 1;   // (the tree's own depth: an entry past it exists in no column, and cost nine FMAs and six selects on zeros)
#else
          constexpr int CWC = 6 + ML;          // compile-time bound of the compact column width
#endif
          float wi[3][CWC], wj[3][CWC];
          const float* Wi = WC + (3 * i) * cw;
          const float* Wj = WC + (3 * j) * cw;
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
            RSB_UNROLL for (int q4 = 0; q4 < (CWC + 3) / 4; ++q4) {
              float t4[4], u4[4];
              ld4(Wi + rr * cw + 4 * q4, t4); ld4(Wj + rr * cw + 4 * q4, u4);
              RSB_UNROLL for (int e = 0; e < 4; ++e)
                if (4 * q4 + e < CWC) { wi[rr][4 * q4 + e] = t4[e]; wj[rr][4 * q4 + e] = u4[e]; }
            }
          }
          float acc[9];
          RSB_UNROLL for (int q2 = 0; q2 < 9; ++q2) acc[q2] = 0.f;
          RSB_UNROLL for (int e = 0; e < CWC; ++e) {
            const bool on = e < 6 || e < 6 + lca;   // entries past the shared prefix belong to different bodies (the base's six are always shared: no select for them)
            float av[3], bv[3];   // both sides zeroed: entries past a column's own support are stale LDS
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { av[rr] = on ? wi[rr][e] : 0.f; bv[rr] = on ? wj[rr][e] : 0.f; }
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
              RSB_UNROLL for (int cc = 0; cc < 3; ++cc) acc[3 * rr + cc] += av[rr] * bv[cc];
          }
          if (i == j && CON[i * kConSlot + 15] != 0.f) { acc[0] = 1.f; acc[4] = 1.f; }   // joint-limit row: dummy tangential diagonal
          if constexpr (TRI) {   // i <= j: the stored block is (j, i), rows = axes of contact j
            float* bp = G + tri_off(j, i);
            RSB_UNROLL for (int cc = 0; cc < 3; ++cc) {
              const float row[4] = {acc[cc], acc[3 + cc], acc[6 + cc], 0.f};
              st4(bp + 4 * cc, row);
            }
          } else if constexpr (GROWS) {   // block (i, j) into contact i's row and its transpose into contact j's: 3 + 3 16-byte stores (the diagonal pair writes once)
            const float B[3][3] = {{acc[0], acc[1], acc[2]}, {acc[3], acc[4], acc[5]}, {acc[6], acc[7], acc[8]}};
            const float Bt[3][3] = {{acc[0], acc[3], acc[6]}, {acc[1], acc[4], acc[7]}, {acc[2], acc[5], acc[8]}};
            gblk_store(G + i * GRP + kGBlock * j, B);
            if (i != j) gblk_store(G + j * GRP + kGBlock * i, Bt);
          } else {
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr)
              RSB_UNROLL for (int cc = 0; cc < 3; ++cc) {
                G[(3 * i + rr) * GS + 4 * j + cc] = acc[3 * rr + cc];   // 3x3 blocks on a 4-float pitch (16-B aligned rows of a block)
                G[(3 * j + cc) * GS + 4 * i + rr] = acc[3 * rr + cc];
              }
          }
          if (i == j) {
            float gi[12];
            inv3(acc, gi);
            gi[9] = gi[10] = gi[11] = 0.f;
            stv<3>(GINV + 12 * i, gi);
          }
        }
      }
#endif
#if RSB_FLAT_CLASS
      asm volatile("; rsb delassus end");
#endif
      __syncthreads();
      if constexpr (FIXED) {   // (a class of its own: the floating-base kernels stay what they were, instruction for instruction)
        // fixed-base systems: a body fewer than three joints from the world cannot move in every direction, its contact's block
        // is rank deficient; the same small compliance as for a self-collision (whose fold below adds it for those)
        if (s < nc && __float_as_int(CON[s * kConSlot + 11]) < kSelfA) {
          float acc[9], gi[12];
          float* dg = TRI ? G + tri_off(s, s) : (GROWS ? G + s * GRP + kGBlock * s : G + 3 * s * GS + 4 * s);     // the diagonal block (TRI, dense rows: its rows, dgs floats apart)
          const int dgs = TRI ? 4 : GS;
          if constexpr (GROWS) {
            float D[3][3];
            gblk_load(dg, D);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) RSB_UNROLL for (int cc = 0; cc < 3; ++cc) acc[3 * rr + cc] = D[rr][cc];
          } else {
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
              float g4[4];
              ld4(dg + rr * dgs, g4);
              acc[3 * rr] = g4[0]; acc[3 * rr + 1] = g4[1]; acc[3 * rr + 2] = g4[2];
            }
          }
          const float reg = kSelfReg * (acc[0] + acc[4] + acc[8]) * (1.0f / 3.0f);
          RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { acc[4 * rr] += reg; dg[GROWS ? g_block_off(rr, rr) : rr * dgs + rr] = acc[4 * rr]; }
          inv3(acc, gi);
          gi[9] = gi[10] = gi[11] = 0.f;
          stv<3>(GINV + 12 * s, gi);
        }
        __syncthreads();
      }
      if (__any(nselfc > 0)) {
        // fold the two entries of every self-collision into one solver contact: G <- P G P^T, c <- P c with P adding the second
        // entry's rows to the first's.  The second entry stays in the solver as an inert contact (zero rows, unit diagonal,
        // c = 0: its impulse stays 0) and receives the first one's impulse after the solve (same numbers in its opposite frame).
        for (int sa = 0; sa + 1 < ncw; ++sa) {
          const bool prim = sa + 1 < nc && (__float_as_int(CON[sa * kConSlot + 11]) & kSelfA) != 0;
          if (!__any(prim)) continue;
          const int sb = sa + 1;
          const float z4[4] = {0.f, 0.f, 0.f, 0.f};
          if constexpr (TRI) {
            // packed storage: lane k owns the blocks (sa, k) and (sb, k) of its contact k; the lane of contact sa owns the diagonal
            if (prim && s < nc) {
              float A[3][3], B[3][3];
              const float Z[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
              if (s != sa && s != sb) {
                tri_load(G, sa, s, A); tri_load(G, sb, s, B);
                RSB_UNROLL for (int r = 0; r < 3; ++r) RSB_UNROLL for (int c = 0; c < 3; ++c) A[r][c] += B[r][c];
                tri_store(G, sa, s, A); tri_store(G, sb, s, Z);
              } else if (s == sa) {
                float X[3][3], D[3][3];
                tri_load(G, sa, sa, A); tri_load(G, sb, sb, B); tri_load(G, sb, sa, X);
                RSB_UNROLL for (int r = 0; r < 3; ++r) RSB_UNROLL for (int c = 0; c < 3; ++c) D[r][c] = A[r][c] + B[r][c] + X[r][c] + X[c][r];
                const float ju = SELFT[4 * sa + 3] + SELFT[4 * sb + 3];   // approach speed of the two bodies' points
                float m4[4];
                ld4(SELFT + 4 * sa, m4);
                RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { CV[3 * sa + rr] += CV[3 * sb + rr]; CV[3 * sb + rr] = 0.f; }
                if (m4[1] > 0.f && ju < -m4[2]) CV[3 * sa + 2] += m4[1] * ju;
                const float reg = (FIXED ? 2.f : 1.f) * kSelfReg * (D[0][0] + D[1][1] + D[2][2]) * (1.0f / 3.0f);   // (oracle: ORC_SELF_REG, see below)
                RSB_UNROLL for (int rr = 0; rr < 3; ++rr) D[rr][rr] += reg;
                const float I3[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
                tri_store(G, sa, sa, D); tri_store(G, sb, sa, Z); tri_store(G, sb, sb, I3);
                float acc[9], gi[12];
                RSB_UNROLL for (int r = 0; r < 3; ++r) RSB_UNROLL for (int c = 0; c < 3; ++c) acc[3 * r + c] = D[r][c];
                inv3(acc, gi);
                gi[9] = gi[10] = gi[11] = 0.f;
                stv<3>(GINV + 12 * sa, gi);
                RSB_UNROLL for (int q2 = 0; q2 < 12; ++q2) gi[q2] = 0.f;
                gi[0] = gi[4] = gi[8] = 1.f;
                stv<3>(GINV + 12 * sb, gi);
              }
            }
            __syncthreads();
            continue;
          }
          if (prim && s < nc) {       // rows: lane = column block
            if constexpr (GROWS) {
              gblk_add(G + sa * GRP + kGBlock * s, G + sb * GRP + kGBlock * s);
            } else {
              RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
                float ga[4], gb[4];
                ld4(G + (3 * sa + rr) * GS + 4 * s, ga); ld4(G + (3 * sb + rr) * GS + 4 * s, gb);
                RSB_UNROLL for (int e = 0; e < 4; ++e) ga[e] += gb[e];
                st4(G + (3 * sa + rr) * GS + 4 * s, ga); st4(G + (3 * sb + rr) * GS + 4 * s, z4);
              }
            }
          }
          __syncthreads();
          if constexpr (GROWS) {      // columns: lane = row block (the three rows of contact s in one pass)
            if (prim && s < nc) gblk_add(G + s * GRP + kGBlock * sa, G + s * GRP + kGBlock * sb);
          } else if (prim) {          // columns: lane = row
            for (int r = s; r < 3 * nc; r += LPE) {
              float ga[4], gb[4];
              ld4(G + r * GS + 4 * sa, ga); ld4(G + r * GS + 4 * sb, gb);
              RSB_UNROLL for (int e = 0; e < 4; ++e) ga[e] += gb[e];
              st4(G + r * GS + 4 * sa, ga); st4(G + r * GS + 4 * sb, z4);
            }
          }
          __syncthreads();
          if (prim && s == 0) {
            float m4[4], acc[9], gi[12];
            ld4(SELFT + 4 * sa, m4);
            const float ju = m4[3] + SELFT[4 * sb + 3];   // approach speed of the two bodies' points
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { CV[3 * sa + rr] += CV[3 * sb + rr]; CV[3 * sb + rr] = 0.f; }
            if (m4[1] > 0.f && ju < -m4[2]) CV[3 * sa + 2] += m4[1] * ju;
            if constexpr (GROWS) {
              float D[3][3];
              gblk_load(G + sa * GRP + kGBlock * sa, D);
              RSB_UNROLL for (int rr = 0; rr < 3; ++rr) RSB_UNROLL for (int cc = 0; cc < 3; ++cc) acc[3 * rr + cc] = D[rr][cc];
            } else {
              RSB_UNROLL for (int rr = 0; rr < 3; ++rr) {
                float g4[4];
                ld4(G + (3 * sa + rr) * GS + 4 * sa, g4);
                acc[3 * rr] = g4[0]; acc[3 * rr + 1] = g4[1]; acc[3 * rr + 2] = g4[2];
              }
            }
            // two bodies joined by fewer than three joints cannot move relative to each other in every direction: the block is
            // rank deficient (thigh against trunk: two joints).  A small compliance keeps the per-contact rule well posed
            // (oracle: ORC_SELF_REG)
            const float reg = (FIXED ? 2.f : 1.f) * kSelfReg * (acc[0] + acc[4] + acc[8]) * (1.0f / 3.0f);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) { acc[4 * rr] += reg; G[GROWS ? sa * GRP + kGBlock * sa + g_block_off(rr, rr) : (3 * sa + rr) * GS + 4 * sa + rr] = acc[4 * rr]; }
            inv3(acc, gi);
            gi[9] = gi[10] = gi[11] = 0.f;
            stv<3>(GINV + 12 * sa, gi);
            RSB_UNROLL for (int q2 = 0; q2 < 12; ++q2) gi[q2] = 0.f;
            gi[0] = gi[4] = gi[8] = 1.f;
            stv<3>(GINV + 12 * sb, gi);
            RSB_UNROLL for (int rr = 0; rr < 3; ++rr) G[GROWS ? sb * GRP + kGBlock * sb + g_block_off(rr, rr) : (3 * sb + rr) * GS + 4 * sb + rr] = 1.f;
          }
          __syncthreads();
        }
      }
      RSB_STAMP(5)
