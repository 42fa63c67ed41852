// step_phase_collision.inc — fragment of rsb_step_kernel: collision detection - plane, height map (closest feature), second flanks / capsule barrels / box faces (class 4), self-collision, joint limits
    // =========================== collision detection (lane = collision sphere) ================
    nc = 0;
    bool illegal = false;
    // writes the contacts of one pass over the primitives (ballot + popcount compaction, contacts in primitive order)
    auto emit = [&](bool hit, int ci, int cid, int cbody, const float* c, float rad, const float* n, float dep) {   // ci: primitive, cid: the id reported (flags)
      illegal |= hit && !((ac.allowed >> ci) & 1ull);
      const unsigned long long bal = __ballot(hit);
      const unsigned long long gm = (LPE == 64) ? bal : ((bal >> (el * LPE)) & ((1ull << (LPE % 64)) - 1ull));
      const int slot = nc + __popcll(gm & ((1ull << s) - 1ull));
      if (hit && slot < kmax) {
        float P[16], t1[3], t2[3];
        contact_tangents(n, t1, t2);
        P[0] = c[0] - rad * n[0]; P[1] = c[1] - rad * n[1]; P[2] = c[2] - rad * n[2]; P[3] = dep;
        P[4] = t1[0]; P[5] = t1[1]; P[6] = t1[2]; P[7] = __int_as_float(cbody);
        P[8] = t2[0]; P[9] = t2[1]; P[10] = t2[2]; P[11] = __int_as_float(cid);
        P[12] = n[0]; P[13] = n[1]; P[14] = n[2]; P[15] = 0.f;
        stv<4>(CON + slot * kConSlot, P);
      }
      nc += __popcll(gm);
    };
    // sphere centre of primitive ci relative to the base position, radius and body
    auto sphere_of = [&](int ci, float* c, float& rad, int& cbody) {
      float ct[8], ax[4];
      ld4(COLT + kColSlot * ci, ct); ct[4] = COLT[kColSlot * ci + 4]; ld4(COLT + kColSlot * ci + 8, ax);
      cbody = __float_as_int(ct[4]);
      rad = ct[3];
      float P[12];
      body_pose_ld(BODY + cbody * kBodySlot, P);
      const float pl[3] = {ct[0], ct[1], ct[2]};
      float t[3];
      mat3_vec(P, pl, t);
      c[0] = P[9] + t[0]; c[1] = P[10] + t[1]; c[2] = P[11] + t[2];
      if (ax[3] > 0.f) {
        // rim primitive (end cap of a cylinder; oracle: "rim"): the point of the circle of radius ax[3] around c, normal to the
        // cap's axis, that is lowest along the world's vertical; a cap lying flat keeps its centre
        float aw[3];
        mat3_vec(P, ax, aw);
        const float len2 = 1.0f - aw[2] * aw[2];
        if (len2 > 1e-12f) {
          const float k = ax[3] * __builtin_amdgcn_rsqf(len2);
          c[0] += k * aw[2] * aw[0]; c[1] += k * aw[2] * aw[1]; c[2] -= k * len2;
        }
      }
      if (n_self > 0) { const float c4[4] = {c[0], c[1], c[2], rad}; st4(CEN + 4 * ci, c4); }
    };
    if (RSB_DIM(TERRAIN, ac.terrain_type) == 0) {
      // ---- plane: depth = r - (z - z0), normal z
      const float nz[3] = {0.f, 0.f, 1.f};
#if RSB_DOWN_QUADS
      asm volatile("; rsb plane begin");
#endif
#if RSB_COL_OWN
      // Own-lane form (step_spec.h: RSB_COL_OWN): the lane's pose Rb, rb of stage (3) of the down pass IS the pose of its primitives' body, and what it tests in a
      // pass is pinned in registers (step_kernel.h: own_*): no table read, no pose read, no rim code (the model has none).  All depth tests and ballots first; the
      // contact's slot is the number of hits on the lanes whose primitive - of any pass - has a lower index, which is its place in primitive order.
      {
        constexpr int NT = kOwnPasses;
        float pc[NT][3], pdep[NT];
        bool phit[NT];
        unsigned pbal[NT];
        RSB_UNROLL for (int t = 0; t < NT; ++t) {
          float tt[3];
          mat3_vec(Rb, own_pl[t], tt);
          pc[t][0] = rb[0] + tt[0]; pc[t][1] = rb[1] + tt[1]; pc[t][2] = rb[2] + tt[2];
          pdep[t] = own_rad[t] - (pbz + pc[t][2] - ac.ground_z);
          phit[t] = own_ci[t] >= 0 && pdep[t] > 0.f && !dead;
        }
        RSB_UNROLL for (int t = 0; t < NT; ++t) pbal[t] = (unsigned)(__ballot(phit[t]) >> (el * LPE)) & 0xffffu;
        // (Stores.  The form that sent the centre of a lane without a primitive and the contact of a lane without a hit to sink slots, no exec-mask region at all,
        //  measured BELOW these regions - eight 64-byte stores by sixteen lanes each cost more than the two skip branches: DESIGN.md section 9.)
        RSB_UNROLL for (int t = 0; t < NT; ++t) {
          const int ci = own_ci[t];
          int slot = 0;
          RSB_UNROLL for (int u = 0; u < NT; ++u) slot += __popc(pbal[u] & ((unsigned)own_lo[t][u >> 1] >> (16 * (u & 1))) & 0xffffu);
          illegal |= phit[t] && !((ac.allowed >> (ci & 63)) & 1ull);
          if (n_self > 0 && ci >= 0) { const float c4[4] = {pc[t][0], pc[t][1], pc[t][2], own_rad[t]}; st4(CEN + 4 * ci, c4); }
          if (phit[t] && slot < kmax) {
            float P[16], t1[3], t2[3];
            contact_tangents(nz, t1, t2);
            P[0] = pc[t][0] - own_rad[t] * nz[0]; P[1] = pc[t][1] - own_rad[t] * nz[1]; P[2] = pc[t][2] - own_rad[t] * nz[2]; P[3] = pdep[t];
            P[4] = t1[0]; P[5] = t1[1]; P[6] = t1[2]; P[7] = __int_as_float(bb);
            P[8] = t2[0]; P[9] = t2[1]; P[10] = t2[2]; P[11] = __int_as_float(ci);
            P[12] = nz[0]; P[13] = nz[1]; P[14] = nz[2]; P[15] = 0.f;
            stv<4>(CON + slot * kConSlot, P);
          }
        }
        RSB_UNROLL for (int t = 0; t < NT; ++t) nc += __popc(pbal[t]);
      }
#elif defined(RSB_SPECIALIZED)
      // The number of passes over the primitives is a constant here: every pass's table entries are read first, then every pass's body poses, then the
      // arithmetic, then the stores (centres for the self-collision sweep, contacts).  Pass by pass - the loop below - (table entry -> body pose) is two
      // dependent LDS round trips PER PASS for the lone wave, and the stores of one pass keep the compiler from issuing the next pass's loads early.
      {
        constexpr int NT = (RSB_SPEC_NCOL + LPE - 1) / LPE;
        float ct[NT][8], ax[NT][4], P[NT][12];
        RSB_UNROLL for (int t = 0; t < NT; ++t) {
          const int cic = min(t * LPE + s, ncol - 1);      // (clamped: no load is predicated)
          ld4(COLT + kColSlot * cic, ct[t]); ct[t][4] = COLT[kColSlot * cic + 4]; ld4(COLT + kColSlot * cic + 8, ax[t]);
        }
        RSB_UNROLL for (int t = 0; t < NT; ++t) body_pose_ld(BODY + __float_as_int(ct[t][4]) * kBodySlot, P[t]);
        float pc[NT][3], pdep[NT];
        bool phit[NT];
        RSB_UNROLL for (int t = 0; t < NT; ++t) {
          const float pl[3] = {ct[t][0], ct[t][1], ct[t][2]};
          float tt[3];
          mat3_vec(P[t], pl, tt);
          pc[t][0] = P[t][9] + tt[0]; pc[t][1] = P[t][10] + tt[1]; pc[t][2] = P[t][11] + tt[2];
          if (ax[t][3] > 0.f) {      // rim primitive: see sphere_of
            float aw[3];
            mat3_vec(P[t], ax[t], aw);
            const float len2 = 1.0f - aw[2] * aw[2];
            if (len2 > 1e-12f) {
              const float k = ax[t][3] * __builtin_amdgcn_rsqf(len2);
              pc[t][0] += k * aw[2] * aw[0]; pc[t][1] += k * aw[2] * aw[1]; pc[t][2] -= k * len2;
            }
          }
          pdep[t] = ct[t][3] - (pbz + pc[t][2] - ac.ground_z);
          phit[t] = (t * LPE + s < ncol) && pdep[t] > 0.f && !dead;
        }
        RSB_UNROLL for (int t = 0; t < NT; ++t) {
          const int ci = t * LPE + s;
          if (n_self > 0 && ci < ncol) { const float c4[4] = {pc[t][0], pc[t][1], pc[t][2], ct[t][3]}; st4(CEN + 4 * ci, c4); }
          emit(phit[t], ci, ci, __float_as_int(ct[t][4]), pc[t], ct[t][3], nz, pdep[t]);
        }
      }
#else
      for (int c0 = 0; c0 < ncol; c0 += LPE) {
        const int ci = c0 + s;
        bool hit = false;
        float c[3] = {0.f, 0.f, 0.f}, rad = 0.f, dep = 0.f;
        int cbody = 0;
        if (ci < ncol) {
          sphere_of(ci, c, rad, cbody);
          dep = rad - (pbz + c[2] - ac.ground_z);
          hit = dep > 0.f && !dead;
        }
        emit(hit, ci, ci, cbody, c, rad, nz, dep);
      }
#endif
#if RSB_DOWN_QUADS
      asm volatile("; rsb plane end");
#endif
    } else {
      // ---- height map: closest feature over the cells under the sphere (oracle: terrain_contact), in three steps:
      //   (1) lane = primitive: spheres whose lowest point is above the map's highest sample are dropped (exact: the surface
      //       is a convex combination of samples); the others get a slot and leave (centre, radius, cell range) in LDS;
      //   (2) lane = (slot, cell): the four lanes of a quad scan the cells of one slot, two triangles each, and agree on the
      //       closest feature (DPP quad minimum of the candidate keys); its lane resolves depth and normal;
      //   (3) lane = primitive again: contacts in primitive order.
      // Scratch: the first (kHmRec + 8) * hm_slots + ncol floats of the Delassus rows (dead here; finite values only, the up pass
      // overwrites most of them with its hand-over slots).
      const int hm_slots = ac.hm_slots;                       // one per primitive of the model (>= kHmSlots)
      float* REC = G;                                         // [hm_slots][kHmRec] x y z r | ix0 iy0 nx ny | c (relative to the base) pad | 4 x 4 corner heights
      float* RES = G + kHmRec * hm_slots;                     // [hm_slots][4] depth, normal
      float* RES2 = G + (kHmRec + 4) * hm_slots;              // [hm_slots][4] class-4 kernels: depth and normal of the second flank's contact (depth 0: none)
      int* SLOTOF = reinterpret_cast<int*>(G + (kHmRec + 8) * hm_slots);   // [ncol] slot + 1 of each primitive, 0 = dropped
      int nnear = 0;
      for (int c0 = 0; c0 < ncol; c0 += LPE) {
        const int ci = c0 + s;
        bool near = false;
        float c[3] = {0.f, 0.f, 0.f}, rad = 0.f;
        int cbody = 0, ix0 = 0, iy0 = 0, nx = 1, ny = 1;
        float hc[16];
        RSB_UNROLL for (int i = 0; i < 16; ++i) hc[i] = 0.f;
        if (ci < ncol) {
          sphere_of(ci, c, rad, cbody);
          near = (pbz + c[2] - rad <= ac.hm_max) && !dead;
          if (near) {
            // the corner heights of the sphere's cells (<= 4 x 4 samples, all loads in flight at once): the sphere can touch
            // the surface over these cells only if its lowest point is below their highest corner (exact), and the scan
            // below reads them from LDS
            hm_cell_range(ac, pbx + c[0], pby + c[1], rad, ix0, iy0, nx, ny);
            const float* H = env_heights + iy0 * ac.hm_xs + ix0;
            // (unconditional loads at clamped offsets: sixteen loads in flight, one wait; a predicated load would wait on its own)
            RSB_UNROLL for (int j = 0; j < 4; ++j)
              RSB_UNROLL for (int i = 0; i < 4; ++i) hc[4 * j + i] = H[min(j, ny) * ac.hm_xs + min(i, nx)];
            float hmax = -3e38f;
            RSB_UNROLL for (int j = 0; j < 4; ++j)
              RSB_UNROLL for (int i = 0; i < 4; ++i) hmax = fmaxf(hmax, (i <= nx && j <= ny) ? hc[4 * j + i] : -3e38f);
            near = pbz + c[2] - rad <= hmax;
          }
        }
        const unsigned long long bal = __ballot(near);
        const unsigned long long gm = (LPE == 64) ? bal : ((bal >> (el * LPE)) & ((1ull << (LPE % 64)) - 1ull));
        const int slot = nnear + __popcll(gm & ((1ull << s) - 1ull));
        const bool take = near && slot < hm_slots;
        if (take) {
          const float R[12] = {pbx + c[0], pby + c[1], pbz + c[2], rad, __int_as_float(ix0), __int_as_float(iy0), __int_as_float(nx), __int_as_float(ny),
                               c[0], c[1], c[2], 0.f};
          stv<3>(REC + kHmRec * slot, R);
          stv<4>(REC + kHmRec * slot + 12, hc);
        }
        if (ci < ncol) SLOTOF[ci] = take ? slot + 1 : 0;
        nnear += __popcll(gm);
      }
      if (nnear > hm_slots) flag |= 1;                        // more spheres near the ground than slots (cannot happen with one slot per primitive): a contact overflow
      nnear = min(nnear, hm_slots);
      const int nnw = env_groups_max<LPE>(nnear);
      __syncthreads();
      for (int k0 = 0; k0 < nnw; k0 += LPE / 4) {
        const int k = k0 + (s >> 2), t = s & 3;
        const bool valid = k < nnear;
        float R[8];
        const float* rec = REC + kHmRec * (valid ? k : 0);
        ldv<2>(rec, R);
        const int ix0 = __float_as_int(R[4]), iy0 = __float_as_int(R[5]), nx = __float_as_int(R[6]), ncell = valid ? nx * __float_as_int(R[7]) : 0;
        unsigned key = 0xffffffffu;
        float bp[3] = {0.f, 0.f, 0.f}, bn[3] = {0.f, 0.f, 1.f};
        for (int cc = t; cc < ncell; cc += 4) {
          const int cyy = (cc >= nx ? 1 : 0) + (cc >= 2 * nx ? 1 : 0), cxx = cc - cyy * nx;   // cc / nx for nx, ny <= 3 without an integer division
          hm_scan_cell(ac, rec + 12, cxx, cyy, ix0 + cxx, iy0 + cyy, 2 * cc, R[0], R[1], R[2], key, bp, bn);
        }
        unsigned kmin = min(key, (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
        kmin = min(kmin, (unsigned)__builtin_amdgcn_update_dpp((int)kmin, (int)kmin, 0x4E, 0xf, 0xf, false));            // quad_perm [2,3,0,1]
        if (valid && key == kmin) {     // the scan position makes the keys of a quad distinct
          float o4[4];
          const bool feature = hm_resolve(ac, rec + 12, ix0, iy0, bp, R[0], R[1], R[2], R[3], o4[0], o4 + 1);
          st4(RES + 4 * k, o4);
          if constexpr (HM2) { const float f4[4] = {(feature && o4[0] > 0.f) ? 1.f : 0.f, 0.f, 0.f, 1.f}; st4(RES2 + 4 * k, f4); }
        }
      }
      __syncthreads();
      if constexpr (HM2) {
        // (2b) the second flank: the quad scans its slot's cells again for the closest penetrating point at least acos(hm_second_cos)
        // away from the first normal; RES2[k] = depth (0: none), normal
        if (ac.hm_contacts >= 2) {
          for (int k0 = 0; k0 < nnw; k0 += LPE / 4) {
            const int k = k0 + (s >> 2), t = s & 3;
            const bool valid = k < nnear;
            float R[8], o1[4], f1[4];
            const float* rec = REC + kHmRec * (valid ? k : 0);
            ldv<2>(rec, R); ld4(RES + 4 * (valid ? k : 0), o1); ld4(RES2 + 4 * (valid ? k : 0), f1);
            const bool go = valid && f1[0] > 0.f;
            const int ix0 = __float_as_int(R[4]), iy0 = __float_as_int(R[5]), nx = __float_as_int(R[6]), ncell = go ? nx * __float_as_int(R[7]) : 0;
            unsigned key = 0xffffffffu;
            float bp[3] = {0.f, 0.f, 0.f};
            for (int cc = t; cc < ncell; cc += 4) {
              const int cyy = (cc >= nx ? 1 : 0) + (cc >= 2 * nx ? 1 : 0), cxx = cc - cyy * nx;
              hm_scan_cell2(ac, rec + 12, cxx, cyy, ix0 + cxx, iy0 + cyy, 2 * cc, R[0], R[1], R[2], R[3] * R[3], o1 + 1, ac.hm_second_cos, key, bp);
            }
            unsigned kmin = min(key, (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0xB1, 0xf, 0xf, false));
            kmin = min(kmin, (unsigned)__builtin_amdgcn_update_dpp((int)kmin, (int)kmin, 0x4E, 0xf, 0xf, false));
            const bool found = kmin != 0xffffffffu;
            if (valid && (found ? key == kmin : t == 0)) {
              const float dist = sqrtf(dot3(bp, bp)), id = found ? 1.0f / dist : 0.f;
              const float o4[4] = {found ? R[3] - dist : 0.f, -bp[0] * id, -bp[1] * id, found ? -bp[2] * id : 1.f};
              st4(RES2 + 4 * k, o4);
            }
          }
          __syncthreads();
        }
      }
      for (int c0 = 0; c0 < ncol; c0 += LPE) {
        const int ci = c0 + s;
        bool hit = false;
        float c[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 1.f}, rad = 0.f, dep = 0.f;
        int cbody = 0;
        const int sl = ci < ncol ? SLOTOF[ci] : 0;
        if (sl > 0) {
          float o4[4], r4[4];
          ld4(RES + 4 * (sl - 1), o4); ld4(REC + kHmRec * (sl - 1) + 8, r4);
          dep = o4[0]; n[0] = o4[1]; n[1] = o4[2]; n[2] = o4[3];
          c[0] = r4[0]; c[1] = r4[1]; c[2] = r4[2];
          rad = REC[kHmRec * (sl - 1) + 3];
          cbody = __float_as_int(COLT[kColSlot * ci + 4]);
          hit = dep > 0.f;
        }
        emit(hit, ci, ci, cbody, c, rad, n, dep);
      }
      if constexpr (HM2) {
        // second flanks: after all first contacts, in primitive order (oracle: the same), flagged ids
        if (ac.hm_contacts >= 2) {
          for (int c0 = 0; c0 < ncol; c0 += LPE) {
            const int ci = c0 + s;
            bool hit = false;
            float c[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 1.f}, rad = 0.f, dep = 0.f;
            int cbody = 0;
            const int sl = ci < ncol ? SLOTOF[ci] : 0;
            if (sl > 0) {
              float o4[4], r4[4];
              ld4(RES2 + 4 * (sl - 1), o4); ld4(REC + kHmRec * (sl - 1) + 8, r4);
              dep = o4[0]; n[0] = o4[1]; n[1] = o4[2]; n[2] = o4[3];
              c[0] = r4[0]; c[1] = r4[1]; c[2] = r4[2];
              rad = REC[kHmRec * (sl - 1) + 3];
              cbody = __float_as_int(COLT[kColSlot * ci + 4]);
              hit = dep > 0.f && RES[4 * (sl - 1)] > 0.f;
            }
            emit(hit, ci, ci | kSecond, cbody, c, rad, n, dep);
          }
        }
        // ---- the cylinders of the capsules (rsb_set_capsule_contacts; oracle: capsule_contact): the deepest point of the axis segment
        // between the two end spheres, located by kCapsuleRounds rounds of four samples (lane = (sample, cell): the four lanes of a quad
        // scan the cells under one sample); a contact of its own when it penetrates and is deeper than both ends by kCapsuleMargin
        if (ac.hm_capsule) {
          float* CAPR = G + (kHmRec + 8) * hm_slots + RSB_MAX_COLLISIONS;    // [4][4] depth, normal of the round's four samples
          for (int cp = 0; cp < ac.hm_capsule; ++cp) {
            const int ci = ac.hm_cap[2 * cp], ce = ac.hm_cap[2 * cp + 1];     // the two ends (the model's data: uniform over the wave)
            if (ce < 0) {
              // ---- a box (ci .. ci + 7 are its corners; oracle: box_face_contact): the candidates for the deepest point besides the corners are
              // (A) the terrain vertices under the box and (B) the plan-view crossings of its twelve edges with the terrain's edges; two passes
              // (the maximum, then the mean of the candidates within kBoxTie of it), lanes 0 .. 15 of the env = candidates, DPP row reductions
              float ctr[3], e[3][3], axs[3][3], len[3];
              const int cbody = __float_as_int(COLT[kColSlot * ci + 4]);
              {
                float P[12], c0[4], ck[4], t0[3], tk[3];
                body_pose_ld(BODY + cbody * kBodySlot, P);
                ld4(COLT + kColSlot * ci, c0);
                mat3_vec(P, c0, t0);
                RSB_UNROLL for (int a = 0; a < 3; ++a) {
                  ld4(COLT + kColSlot * (ci + (1 << a)), ck);
                  mat3_vec(P, ck, tk);
                  RSB_UNROLL for (int i = 0; i < 3; ++i) e[a][i] = 0.5f * (tk[i] - t0[i]);
                  len[a] = sqrtf(dot3(e[a], e[a]));
                  const float il = 1.0f / fmaxf(len[a], 1e-12f);
                  RSB_UNROLL for (int i = 0; i < 3; ++i) axs[a][i] = e[a][i] * il;
                }
                ld4(COLT + kColSlot * (ci + 7), ck);
                mat3_vec(P, ck, tk);
                RSB_UNROLL for (int i = 0; i < 3; ++i) ctr[i] = P[9 + i] + 0.5f * (t0[i] + tk[i]);
              }
              ctr[0] += pbx; ctr[1] += pby; ctr[2] += pbz;             // world
              const float low = ctr[2] - fabsf(e[0][2]) - fabsf(e[1][2]) - fabsf(e[2][2]);
              const bool near = (low <= ac.hm_max) && !dead && s < 16;
              if (!__any(near)) continue;
              float dep_c = 0.f;
              RSB_UNROLL for (int k2 = 0; k2 < 8; ++k2) { const int sl = SLOTOF[ci + k2]; dep_c = fmaxf(dep_c, sl > 0 ? RES[4 * (sl - 1)] : 0.f); }
              const int xs = ac.hm_xs, ys = ac.hm_ys;
              const float X = fabsf(e[0][0]) + fabsf(e[1][0]) + fabsf(e[2][0]), Y = fabsf(e[0][1]) + fabsf(e[1][1]) + fabsf(e[2][1]);
              int ix_lo = max((int)ceilf((ctr[0] - X - ac.hm_x0) * ac.hm_inv_dx), 0), ix_hi = min((int)floorf((ctr[0] + X - ac.hm_x0) * ac.hm_inv_dx), xs - 1);
              int iy_lo = max((int)ceilf((ctr[1] - Y - ac.hm_y0) * ac.hm_inv_dy), 0), iy_hi = min((int)floorf((ctr[1] + Y - ac.hm_y0) * ac.hm_inv_dy), ys - 1);
              bool over = false;
              if (ix_hi - ix_lo + 1 > kBoxSpan) { ix_hi = ix_lo + kBoxSpan - 1; over = true; }
              if (iy_hi - iy_lo + 1 > kBoxSpan) { iy_hi = iy_lo + kBoxSpan - 1; over = true; }
              const int ntx = env_groups_max<LPE>(near ? (ix_hi - ix_lo + 4) >> 2 : 0), nty = env_groups_max<LPE>(near ? (iy_hi - iy_lo + 4) >> 2 : 0);
              const int si = s & 3, sj = (s >> 2) & 3;
              // lane s < 12 owns box edge s: along axis k = s >> 2 from the corner with signs (sb, sc) on the two other axes
              const int ek = s >> 2;
              float p0[3], dir[3];
              {
                const float sb = (s & 1) ? 1.f : -1.f, sc = (s & 2) ? 1.f : -1.f;
                RSB_UNROLL for (int i = 0; i < 3; ++i) {
                  const float ea = ek == 0 ? e[0][i] : (ek == 1 ? e[1][i] : e[2][i]);
                  const float eb = ek == 0 ? e[1][i] : (ek == 1 ? e[2][i] : e[0][i]);
                  const float ec = ek == 0 ? e[2][i] : (ek == 1 ? e[0][i] : e[1][i]);
                  p0[i] = ctr[i] - ea + sb * eb + sc * ec; dir[i] = 2.f * ea;
                }
              }
              const float gx0 = (p0[0] - ac.hm_x0) * ac.hm_inv_dx, gy0 = (p0[1] - ac.hm_y0) * ac.hm_inv_dy, dgx = dir[0] * ac.hm_inv_dx, dgy = dir[1] * ac.hm_inv_dy;
              float dmax = -3e38f, sum[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              for (int pass = 0; pass < 2; ++pass) {
                auto cand = [&](bool ok, float d, const float* pos, const float* nn) {
                  if (pass == 0) { dmax = ok ? fmaxf(dmax, d) : dmax; return; }
                  const float w = (ok && d >= dmax - kBoxTie) ? 1.f : 0.f;
                  sum[0] += w;
                  RSB_UNROLL for (int i = 0; i < 3; ++i) { sum[1 + i] += w * (pos[i] - ctr[i]); sum[4 + i] += w * nn[i]; }
                };
                // (A) terrain vertices, 4 x 4 per round
                for (int ty = 0; ty < nty; ++ty)
                  for (int tx = 0; tx < ntx; ++tx) {
                    const int ix = ix_lo + 4 * tx + si, iy = iy_lo + 4 * ty + sj;
                    bool ok = near && ix <= ix_hi && iy <= iy_hi;
                    const float h = env_heights[min(iy, ys - 1) * xs + min(ix, xs - 1)];
                    const float x = ac.hm_x0 + (float)ix * ac.hm_dx, y = ac.hm_y0 + (float)iy * ac.hm_dy;
                    const float rx = x - ctr[0], ry = y - ctr[1];
                    float zlo = -3e38f, zup = 3e38f, nf[3] = {0.f, 0.f, 1.f};
                    RSB_UNROLL for (int k = 0; k < 3; ++k) {
                      const float rho = rx * axs[k][0] + ry * axs[k][1], az = axs[k][2];
                      const bool vert = fabsf(az) < 1e-6f;
                      ok = ok && !(vert && fabsf(rho) > len[k]);
                      const float iaz = 1.0f / (vert ? 1.f : az);
                      const float za = ctr[2] + (-len[k] - rho) * iaz, zb = ctr[2] + (len[k] - rho) * iaz;
                      const float lo = fminf(za, zb), hi = fmaxf(za, zb);
                      const bool take = !vert && lo > zlo;
                      const float sg = az > 0.f ? 1.f : -1.f;
                      zlo = take ? lo : zlo;
                      nf[0] = take ? sg * axs[k][0] : nf[0]; nf[1] = take ? sg * axs[k][1] : nf[1]; nf[2] = take ? sg * az : nf[2];
                      zup = vert ? zup : fminf(zup, hi);
                    }
                    ok = ok && zlo <= zup && zlo > -1e37f;
                    const float pos[3] = {x, y, zlo};
                    cand(ok, (h - zlo) * nf[2], pos, nf);
                  }
                // (B) box edges x terrain edges: grid lines x = const (family 0), y = const (1), cell diagonals gx - gy = const (2)
                for (int fam = 0; fam < 3; ++fam) {
                  const float g0 = fam == 0 ? gx0 : (fam == 1 ? gy0 : gx0 - gy0), dg = fam == 0 ? dgx : (fam == 1 ? dgy : dgx - dgy);
                  const float g1 = g0 + dg;
                  int lo = max((int)ceilf(fminf(g0, g1)), fam == 2 ? -(ys - 2) : 0), hi = min((int)floorf(fmaxf(g0, g1)), fam == 0 ? xs - 1 : (fam == 1 ? ys - 1 : xs - 2));
                  const bool edge = near && s < 12 && dg != 0.f;
                  if (hi - lo + 1 > kBoxSpan) { hi = lo + kBoxSpan - 1; over = over || edge; }
                  const int cnt = env_groups_max<LPE>(row_max_i32(edge ? hi - lo + 1 : 0));
                  const float idg = 1.0f / (dg != 0.f ? dg : 1.f);
                  for (int k = 0; k < cnt; ++k) {
                    const int i = lo + k;
                    bool ok = edge && i <= hi;
                    const float t = fminf(fmaxf(((float)i - g0) * idg, 0.f), 1.f);
                    const float pt[3] = {p0[0] + t * dir[0], p0[1] + t * dir[1], p0[2] + t * dir[2]};
                    const float gx = (pt[0] - ac.hm_x0) * ac.hm_inv_dx, gy = (pt[1] - ac.hm_y0) * ac.hm_inv_dy;
                    int ia, ib;          // offsets of the terrain edge's two vertices
                    float f, T[3];
                    if (fam == 0) {
                      ok = ok && gy >= 0.f && gy <= (float)(ys - 1);
                      const int j = min(max((int)floorf(gy), 0), ys - 2);
                      f = gy - (float)j; ia = j * xs + min(max(i, 0), xs - 1); ib = ia + xs;
                      T[0] = 0.f; T[1] = ac.hm_dy;
                    } else if (fam == 1) {
                      ok = ok && gx >= 0.f && gx <= (float)(xs - 1);
                      const int j = min(max((int)floorf(gx), 0), xs - 2);
                      f = gx - (float)j; ia = min(max(i, 0), ys - 1) * xs + j; ib = ia + 1;
                      T[0] = ac.hm_dx; T[1] = 0.f;
                    } else {
                      const int jx = min(max((int)floorf(gx), 0), xs - 2), jy = jx - i;
                      f = gx - (float)jx;
                      ok = ok && jy >= 0 && jy <= ys - 2 && f >= 0.f && f <= 1.f;
                      ia = min(max(jy, 0), ys - 2) * xs + jx; ib = ia + xs + 1;
                      T[0] = ac.hm_dx; T[1] = ac.hm_dy;
                    }
                    const float hA = env_heights[ia], hB = env_heights[ib];
                    T[2] = hB - hA;
                    const float h = hA + f * T[2];
                    float nn[3];
                    cross3(dir, T, nn);
                    const float n2 = dot3(nn, nn);
                    ok = ok && n2 > 1e-12f * dot3(dir, dir) * dot3(T, T);
                    const float inv = (nn[2] < 0.f ? -1.f : 1.f) * __builtin_amdgcn_rsqf(fmaxf(n2, 1e-30f));
                    RSB_UNROLL for (int q = 0; q < 3; ++q) nn[q] *= inv;
                    cand(ok, (h - pt[2]) * nn[2], pt, nn);
                  }
                }
                if (pass == 0) dmax = row_max_f32(dmax);
              }
              RSB_UNROLL for (int i = 0; i < 7; ++i) sum[i] = row_sum_f32(sum[i]);
              flag |= row_max_i32((over && near) ? 1 : 0);      // (lane 0 of the env reports the flags)
              const float icnt = 1.0f / fmaxf(sum[0], 1.f), nl2 = sum[4] * sum[4] + sum[5] * sum[5] + sum[6] * sum[6], inl = __builtin_amdgcn_rsqf(fmaxf(nl2, 1e-30f));
              const float crel[3] = {ctr[0] + sum[1] * icnt - pbx, ctr[1] + sum[2] * icnt - pby, ctr[2] + sum[3] * icnt - pbz};
              const float bn3[3] = {nl2 > 1e-18f ? sum[4] * inl : 0.f, nl2 > 1e-18f ? sum[5] * inl : 0.f, nl2 > 1e-18f ? sum[6] * inl : 1.f};
              const bool hitb = near && sum[0] > 0.f && dmax > 0.f && dmax > dep_c + kCapsuleMargin && s == 0;
              emit(hitb, ci, ci | kCapsule, cbody, crel, 0.f, bn3, dmax);
              continue;
            }
            float ca[3], cb[3];
            int cbody = 0;
            float rad = 0.f, tmin = 0.02f;
            {
              float ct[4], P[12], t[3];
              ld4(COLT + kColSlot * ci, ct);
              cbody = __float_as_int(COLT[kColSlot * ci + 4]);
              const float rim = COLT[kColSlot * ci + 11];
              rad = rim > 0.f ? rim : ct[3];          // a cylinder's ends are rim primitives (radius 0, rim = the cylinder's radius): COLT holds the cap CENTRES
              body_pose_ld(BODY + cbody * kBodySlot, P);
              mat3_vec(P, ct, t);
              ca[0] = P[9] + t[0]; ca[1] = P[10] + t[1]; ca[2] = P[11] + t[2];
              ld4(COLT + kColSlot * ce, ct);
              mat3_vec(P, ct, t);
              cb[0] = P[9] + t[0]; cb[1] = P[10] + t[1]; cb[2] = P[11] + t[2];
              if (rim > 0.f) {   // flat caps: a sample sphere must not reach past them (oracle: the same range)
                const float dx = cb[0] - ca[0], dy = cb[1] - ca[1], dz = cb[2] - ca[2];
                tmin = rad * __builtin_amdgcn_rsqf(dx * dx + dy * dy + dz * dz);
              }
            }
            const float tmax = 1.0f - tmin;
            const bool near = (pbz + fminf(ca[2], cb[2]) - rad <= ac.hm_max) && !dead && tmin < 0.5f;
            if (!__any(near)) continue;
            const int sa = SLOTOF[ci], sb = SLOTOF[ce];
            const float dep_ends = fmaxf(fmaxf(sa > 0 ? RES[4 * (sa - 1)] : 0.f, sb > 0 ? RES[4 * (sb - 1)] : 0.f), 0.f);
            float cc = 0.5f, ww = 0.5f, bd = 0.f, bt = 0.5f, bn3[3] = {0.f, 0.f, 1.f};
            const int ks = (s >> 2) & 3, t4 = s & 3;
            for (int round = 0; round < kCapsuleRounds; ++round) {
              {
                const float t = fminf(fmaxf(cc + ww * (-0.6f + 0.4f * (float)ks), tmin), tmax);
                const float x = pbx + ca[0] + t * (cb[0] - ca[0]), y = pby + ca[1] + t * (cb[1] - ca[1]), z = pbz + ca[2] + t * (cb[2] - ca[2]);
                int ix0, iy0, nx, ny;
                hm_cell_range(ac, x, y, rad, ix0, iy0, nx, ny);
                const int ncell = (near && s < 16) ? nx * ny : 0;
                unsigned key = 0xffffffffu;
                float bp[3] = {0.f, 0.f, 0.f}, bnn[3] = {0.f, 0.f, 1.f};
                for (int q = t4; q < ncell; q += 4) {
                  const int cyy = (q >= nx ? 1 : 0) + (q >= 2 * nx ? 1 : 0), cxx = q - cyy * nx;
                  hm_scan_cell_map(ac, env_heights, ix0 + cxx, iy0 + cyy, 2 * q, x, y, z, key, bp, bnn);
                }
                unsigned kmin = min(key, (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0xB1, 0xf, 0xf, false));
                kmin = min(kmin, (unsigned)__builtin_amdgcn_update_dpp((int)kmin, (int)kmin, 0x4E, 0xf, 0xf, false));
                if (near && s < 16 && key == kmin) {
                  float o4[4];
                  hm_resolve_above(ac, env_heights, bp, x, y, z, rad, o4[0], o4 + 1);
                  st4(CAPR + 4 * ks, o4);
                }
              }
              __syncthreads();
              // every lane ranks the four samples the same way: a later one must be deeper by more than 2e-6 r to win (oracle: the same rule)
              bool have = false;
              RSB_UNROLL for (int k2 = 0; k2 < 4; ++k2) {
                float o4[4];
                ld4(CAPR + 4 * k2, o4);
                const float tk = fminf(fmaxf(cc + ww * (-0.6f + 0.4f * (float)k2), tmin), tmax);
                const bool take = !have || o4[0] > bd + 2e-6f * rad;
                bd = take ? o4[0] : bd; bt = take ? tk : bt;
                bn3[0] = take ? o4[1] : bn3[0]; bn3[1] = take ? o4[2] : bn3[1]; bn3[2] = take ? o4[3] : bn3[2];
                have = true;
              }
              cc = bt; ww *= 0.4f;
              __syncthreads();
            }
            const bool hitc = near && bd > 0.f && bd > dep_ends + kCapsuleMargin && s == 0;
            const float crel[3] = {ca[0] + bt * (cb[0] - ca[0]), ca[1] + bt * (cb[1] - ca[1]), ca[2] + bt * (cb[2] - ca[2])};
            emit(hitc, ci, ci | kCapsule, cbody, crel, rad, bn3, bd);
          }
        }
      }
      __syncthreads();   // the scratch is free again (the up pass reuses it)
    }
    if (nc > kmax) { nc = kmax; flag |= 1; }
    RSB_STAMP(12)
    // ---- self-collision (oracle: "Self-collision" in step_impl): sphere x sphere over the candidate pairs (primitives of two
    // bodies that are not parent and child), lane = pair.  A hit takes TWO contact slots, one per body with opposite frames
    // (what RaiSim's contact list holds); the Delassus phase folds the pair into ONE solver contact (J = J_i - J_j).
    // The sweep over the pairs only records a hit bit per lane; everything else runs when some env of the wave has a hit.
    nselfc = 0;
    if (n_self > 0) {
      // lane = pair, batches of kSelfBatch passes (indices past the table read its last entry, a pair that cannot hit; the next
      // batch's entries are in flight while the current one is tested).  An entry holds the byte offsets of the two centres.
      const int npass = (n_self + LPE - 1) / LPE;
      const char* cenb = reinterpret_cast<const char*>(CEN);
      int prn[kSelfBatch];
      RSB_UNROLL for (int q4 = 0; q4 < kSelfBatch; ++q4) prn[q4] = SPAIR[min(q4 * LPE + s, n_self)];
      __syncthreads();   // the centres of this sub-step are in CEN
      // The sweep only answers "does any pair of this wave overlap" (one compare and a scalar OR per pair): which pair, the degenerate-distance guard and
      // everything else is the rare path's business, which tests its pairs again.  (Recording a hit bit per pass and the guard in the sweep cost 3.5 VALU
      // and a scalar AND per pair - a quarter of a phase that is 4.7 % of the benchmark's time and finds nothing in almost every sub-step.)
      bool anyhit = false;
      for (int k0 = 0; k0 < npass; k0 += kSelfBatch) {
        float ci4[kSelfBatch][4], cj4[kSelfBatch][4];
        RSB_UNROLL for (int q4 = 0; q4 < kSelfBatch; ++q4) {
          ld4(reinterpret_cast<const float*>(cenb + (prn[q4] & 0xffff)), ci4[q4]);
          ld4(reinterpret_cast<const float*>(cenb + ((unsigned)prn[q4] >> 16)), cj4[q4]);
        }
        RSB_UNROLL for (int q4 = 0; q4 < kSelfBatch; ++q4) prn[q4] = SPAIR[min((k0 + kSelfBatch + q4) * LPE + s, n_self)];
        RSB_UNROLL for (int q4 = 0; q4 < kSelfBatch; ++q4) {
          const float dx = ci4[q4][0] - cj4[q4][0], dy = ci4[q4][1] - cj4[q4][1], dz = ci4[q4][2] - cj4[q4][2], rs = ci4[q4][3] + cj4[q4][3];
          const float d2 = dx * dx + dy * dy + dz * dz;
          anyhit |= d2 < rs * rs;
        }
      }
      if (__any(anyhit && !dead)) {   // rare
        const int nc0 = nc;
        for (int k = 0; k < npass; ++k) {
          bool hit = false;
          {   // the pass's pair again, with the sweep's arithmetic
            const int pr = SPAIR[min(k * LPE + s, n_self)];
            float ci4[4], cj4[4];
            ld4(reinterpret_cast<const float*>(cenb + (pr & 0xffff)), ci4);
            ld4(reinterpret_cast<const float*>(cenb + ((unsigned)pr >> 16)), cj4);
            const float dx = ci4[0] - cj4[0], dy = ci4[1] - cj4[1], dz = ci4[2] - cj4[2], rs = ci4[3] + cj4[3];
            const float d2 = dx * dx + dy * dy + dz * dz;
            hit = (d2 < rs * rs) & (d2 >= 1e-12f) & !dead;
          }
          const unsigned long long bal = __ballot(hit);
          if (!bal) continue;
          const unsigned long long gm = (LPE == 64) ? bal : ((bal >> (el * LPE)) & ((1ull << (LPE % 64)) - 1ull));
          const int slot = nc + 2 * __popcll(gm & ((1ull << s) - 1ull));
          illegal |= hit;           // a self-collision is never a foot on the terrain: it ends the episode under the rsg_anymal rule
          if (hit && slot + 1 < kmax) {
            const int p = k * LPE + s;
            const int pr = SPAIR[p], pi = (pr & 0xffff) >> 4, pj = (int)((unsigned)pr >> 20);
            float ci4[4], cj4[4], m4[4];
            ld4(CEN + 4 * pi, ci4); ld4(CEN + 4 * pj, cj4);
            ld4(a.self_mat + 4 * (size_t)p, m4);
            float n[3] = {ci4[0] - cj4[0], ci4[1] - cj4[1], ci4[2] - cj4[2]};
            const float dist = sqrtf(dot3(n, n)), idist = 1.0f / dist, dep = ci4[3] + cj4[3] - dist;
            n[0] *= idist; n[1] *= idist; n[2] *= idist;
            const float back = ci4[3] - 0.5f * dep;   // the middle of the overlap
            float P[16], t1[3], t2[3];
            contact_tangents(n, t1, t2);
            P[0] = ci4[0] - back * n[0]; P[1] = ci4[1] - back * n[1]; P[2] = ci4[2] - back * n[2]; P[3] = dep;
            P[4] = t1[0]; P[5] = t1[1]; P[6] = t1[2]; P[7] = COLT[kColSlot * pi + 4];
            P[8] = t2[0]; P[9] = t2[1]; P[10] = t2[2]; P[11] = __int_as_float(pi | kSelfA);
            P[12] = n[0]; P[13] = n[1]; P[14] = n[2]; P[15] = 0.f;
            stv<4>(CON + slot * kConSlot, P);
            // second entry: the other body, opposite frame; its rows carry no depth of their own (the fold adds the two)
            P[3] = 0.f;
            RSB_UNROLL for (int i = 0; i < 3; ++i) { P[4 + i] = -P[4 + i]; P[8 + i] = -P[8 + i]; P[12 + i] = -P[12 + i]; }
            P[7] = COLT[kColSlot * pj + 4]; P[11] = __int_as_float(pj | kSelfB);
            stv<4>(CON + (slot + 1) * kConSlot, P);
            m4[3] = 0.f;
            st4(SELFT + 4 * slot, m4); st4(SELFT + 4 * (slot + 1), m4);
          }
          nc += 2 * __popcll(gm);
        }
        const int fit = nc0 + 2 * ((kmax - nc0) >> 1);   // a self-collision that does not get both slots is dropped
        if (nc > fit) { nc = fit; flag |= 1; }
        nselfc = (nc - nc0) >> 1;
      }
    }
    // joint limits (oracle: "joint limits" in step_impl): a joint outside [q_lower, q_upper] adds one unilateral row
    // s * qdot >= 0, carried through the solver as a contact with empty tangential rows; slots after the real contacts
    nc_real = nc;
    RSB_STAMP(13)
    // (the down pass has compared every joint with its range - body constants and coordinate were in its registers: a wave without a violation, nearly
    //  every wave, skips the three LDS reads, the wait and the ballot of this loop)
    if (__any(lim_out) && !dead) {
      for (int b0 = 1; b0 < nb; b0 += LPE) {
        const int b = b0 + s;
        float sgn = 0.f, viol = 0.f;
        if (b < nb) {
          const float qj = Q[b + 6], lo = MODELF[b * RSB_DIM(MODEL_PITCH, L.model_pitch) + 29], hi = MODELF[b * RSB_DIM(MODEL_PITCH, L.model_pitch) + 30];
          if (qj > hi) { sgn = -1.f; viol = qj - hi; } else if (qj < lo) { sgn = 1.f; viol = lo - qj; }
        }
        const unsigned long long bal = __ballot(sgn != 0.f);
        if (bal) {   // rare: nothing below runs while every joint of the wave is inside its range
          const unsigned long long gm = (LPE == 64) ? bal : ((bal >> (el * LPE)) & ((1ull << (LPE % 64)) - 1ull));
          const int slot = nc + __popcll(gm & ((1ull << s) - 1ull));
          if (sgn != 0.f && slot < kmax) {
            float P[16];
            RSB_UNROLL for (int i = 0; i < 16; ++i) P[i] = 0.f;
            P[3] = viol; P[7] = __int_as_float(b); P[11] = __int_as_float(ncol + b); P[15] = sgn;
            stv<4>(CON + slot * kConSlot, P);
          }
          nc += __popcll(gm);
        }
      }
      if (nc > kmax) { nc = kmax; flag |= 1; }
    }
    if (RSB_DIM(EARLY_TERM, ac.early_term)) {
      // early termination (opt-in, rsb_set_early_termination): the sub-step in which a primitive outside `allowed`
      // touches the terrain is not integrated, nor are the following ones; the detected contacts stay reported
      // with zero impulses and the env counts as terminated
      const unsigned long long bil = __ballot(illegal);
      const unsigned long long gsel = (LPE == 64) ? ~0ull : (((1ull << (LPE % 64)) - 1ull) << (el * LPE));
      if (!dead && (bil & gsel)) {
        dead = true; nc_dead = nc_real;
        if (s < nc) { LAM[3 * s] = 0.f; LAM[3 * s + 1] = 0.f; LAM[3 * s + 2] = 0.f; }
      }
      if (dead) nc = 0;
    }
    const int ncw = env_groups_max<LPE>(nc);   // wave-wide maximum contact count (loop bounds must be wave-uniform scalars)
    RSB_STAMP(2)
