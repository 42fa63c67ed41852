// rsb_dynamics.hip — batched inverse dynamics with joint reaction wrenches and contact-free forward dynamics from the resident state
// (rsb_inverse_dynamics, rsb_forward_dynamics; include/rsb.h, where the conventions are stated).
//
// The plain equations of motion  M udot + h = tau + sum J^T w  for all N envs in one call, from d_gc / d_gv on the world's stream.  Nothing here is
// shared with the step kernel or with the one-thread-per-env query kernel: two kernels of their own, called between two control steps, that write
// nothing but their outputs.
//
// Both kernels give a workgroup epb = 256 / nb CONSECUTIVE envs and one lane per (env, body) (EnvBlock), as rsb_centroidal.hip does.  A lane walks
// its body's support chain root -> body (walk_chain, the one walk of all batched queries: it keeps the parent's velocity and, for the inverse
// dynamics, carries the accelerations along) with everything in registers: no per-body arrays, no scratch, no cross-lane traffic.  The walk, the
// model tables, the inertia about o, the subtree sum and the staging of the RSB_HOST forms are shared with the other queries (frames_chain.h).
// Every moment is taken about the env's BASE ORIGIN o = p_0, never about the world origin: an env standing 50 m away keeps all its bits.
// External loads and contact records are added by the lane whose body they act on, in ascending index: the frame list first, then the env's contact
// records.  No atomics anywhere; every sum has a fixed order.
//
//   rnea_kernel   (1) each lane forms its body's own net wrench about o,
//                         f_i = m_i (acc_ci - g) - external      n_i = I_w alpha + omega x I_w omega + r_i x m_i (acc_ci - g) - external,
//                     I_w x = R (I (R^T x)), r_i = (p_i - o) + R_i com_i, and leaves it in LDS with its joint (a_i, s_i = p_i - o, type, qdd_i);
//                 (2) one lane per (env, body j) adds the records of the bodies i >= j of j's subtree (anc[i * depth + level[j]] == j) in ascending i:
//                     (F_j, N_j about o), shifts the torque to p_j (N_j - s_j x F_j), projects on the axis and adds armature_j qdd_j;
//                 (3) all lanes sweep the block's contiguous rows of each output, consecutive lanes writing consecutive floats.  A NULL output skips
//                     its sweep; udot == NULL and "no loads" are run-time flags in the one instruction stream.
//   aba_kernel    the articulated-body algorithm in the common frame (world axes, origin o: every transform is the identity), level-synchronous.
//                 A lane keeps its body's articulated inertia (J 6, H 9, M 6 = 21 entries of the symmetric 6 x 6 [[J, H], [H^T, M]]) and bias force (6)
//                 in registers.  Up pass, deepest level to level 1: the bodies of level l publish  IA - U U^T / D  and  pA + Ia c + U u / D  (27
//                 floats) to LDS, barrier, the bodies of level l - 1 gather from their children in ascending body order.  Base: one lane per env
//                 solves the 6 x 6 SPD system by LDL^T in registers; a fixed base takes A_0 = (0, -g).  Down pass level by level through a second LDS
//                 array of spatial accelerations.  2 (depth - 1) + 1 barriers after the staging barrier.
// Static LDS, sized for 64 bodies whatever the tree: rnea_kernel 30 464 B, aba_kernel 48 896 B.
// A result of env e depends on env e's rows alone: the same bits for any N, any subset of outputs, host or device buffers.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kWr = 15;        // rnea_kernel, per lane: f 0-2, n about o 3-5, a 6-8, s 9-11, joint type 12 (0 base, 1 revolute, 2 prismatic), qdd 13
constexpr int kOut = 7;        // ... and per (env, body) result: joint force 0-2, joint torque 3-5, tau 6
constexpr int kArt = 27;       // aba_kernel, per lane: J 0-5, H 6-14, M 15-20, bias force 21-26
constexpr int kAcc = 7;        // ... spatial acceleration (angular 0-2, linear 3-5)
constexpr int kRowsOut = 1536; // ... udot rows of the block: epb * (nb + 5) <= 256 + 5 * 256

// what acts on the bodies besides gravity: F frames with force / torque [N,F,3] (either may be null), the resident contact list (null: not asked for)
struct Loads { const float* force; const float* torque; const rsb_contact* contacts; const int32_t* count; int F, kmax; float inv_dt; };

// 1 / x: the hardware's approximation and one Newton step
__device__ __forceinline__ float recip(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.f), r, r);
}

// the external force on `body` and its moment about o: the frames of the list that sit on the body, then the env's contact records on it, ascending
__device__ __forceinline__ void body_loads(const Loads& L, const FrameList& frames, long long env, int body, const float* R, const float* po, const float* o,
                                           float* f, float* n) {
  for (int k = 0; k < 3; ++k) { f[k] = 0.f; n[k] = 0.f; }
  for (int k = 0; k < L.F; ++k) {
    if (frames.f[k].body != body) continue;
    const float off[3] = {frames.f[k].offset[0], frames.f[k].offset[1], frames.f[k].offset[2]};
    float ro[3], r[3], fo[3], to[3], rf[3];
    mat3_vec(R, off, ro);
    const size_t at = ((size_t)env * L.F + k) * 3;
    for (int c = 0; c < 3; ++c) { r[c] = po[c] + ro[c]; fo[c] = L.force ? L.force[at + c] : 0.f; to[c] = L.torque ? L.torque[at + c] : 0.f; }
    cross3(r, fo, rf);
    for (int c = 0; c < 3; ++c) { f[c] += fo[c]; n[c] += to[c] + rf[c]; }
  }
  if (L.contacts) {
    const int cnt = min(max(L.count[env], 0), L.kmax);
    const rsb_contact* con = L.contacts + (size_t)env * L.kmax;
    for (int k = 0; k < cnt; ++k) {
      if (con[k].body != body) continue;
      float r[3], fo[3], rf[3];
      for (int c = 0; c < 3; ++c) { r[c] = con[k].position[c] - o[c]; fo[c] = con[k].impulse[c] * L.inv_dt; }
      cross3(r, fo, rf);
      for (int c = 0; c < 3; ++c) { f[c] += fo[c]; n[c] += rf[c]; }
    }
  }
}

__global__ __launch_bounds__(kThreads) void rnea_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                        const float* __restrict__ udot, const FrameList frames, const Loads loads, int N, const Vec3 g,
                                                        float* __restrict__ tau, float* __restrict__ joint_force, float* __restrict__ joint_torque) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ float rec[kThreads * kWr];
  __shared__ float res[kThreads * kOut];
  const DevModel& m = *model;
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  __syncthreads();
  const int nb = m.nb, depth = m.depth, nv = m.nv;
  const auto [env0, here, el, body] = env_block(nb, N);
  if (el < here) {
    const long long env = env0 + el;
    const float* q = gc + (size_t)env * m.nq;
    const float* u = gv + (size_t)env * nv;
    const float* ud = udot ? udot + (size_t)env * nv : nullptr;
    Chain b;
    walk_chain<true>(m, rows, q, u, ud, true, body, b, NoJoint{});
    const float* x = xtra + body * kXtra;
    const float mass = rows[body * kRow + 7];
    const float gvec[3] = {g.x, g.y, g.z};
    float po[3], rc[3], r[3], t0[3], t1[3], acom[3], fi[3], wb[3], Iwb[3], Iw[3], ab[3], Iab[3], Ia[3], wIw[3], rf[3], fe[3], ne[3];
    mat3_vec(b.R, x, rc);
    for (int k = 0; k < 3; ++k) { po[k] = b.p[k] - q[k]; r[k] = po[k] + rc[k]; }
    cross3(b.al, rc, t0);                  // acc of the centre of mass = acc + alpha x rc + omega x (omega x rc)
    cross3(b.w, rc, t1);
    cross3(b.w, t1, acom);
    for (int k = 0; k < 3; ++k) { acom[k] += b.ac[k] + t0[k]; fi[k] = mass * (acom[k] - gvec[k]); }
    mat3t_vec(b.R, b.w, wb);
    sym3_vec(x + 3, wb, Iwb);
    mat3_vec(b.R, Iwb, Iw);
    mat3t_vec(b.R, b.al, ab);
    sym3_vec(x + 3, ab, Iab);
    mat3_vec(b.R, Iab, Ia);
    cross3(b.w, Iw, wIw);
    cross3(r, fi, rf);
    body_loads(loads, frames, env, body, b.R, po, q, fe, ne);
    float* s = rec + threadIdx.x * kWr;
    for (int k = 0; k < 3; ++k) {
      s[k] = fi[k] - fe[k];
      s[3 + k] = (Ia[k] + wIw[k] + rf[k]) - ne[k];
      s[6 + k] = b.a[k];
      s[9 + k] = po[k];
    }
    s[12] = __int_as_float(b.type);
    s[13] = b.qdd;
  }
  __syncthreads();
  if (el < here) {      // the wrench joint j carries: the sum over the subtree below this lane's body
    const float* s = rec + el * nb * kWr;
    float acc[6];
    subtree_sum<6>(m, nb, depth, s, kWr, body, acc);
    const float* me = s + body * kWr;
    float sf[3];
    cross3(me + 9, acc, sf);
    const float nj[3] = {acc[3] - sf[0], acc[4] - sf[1], acc[5] - sf[2]};
    const int type = __float_as_int(me[12]);
    const float along = type == 1 ? dot3(me + 6, nj) : type == 2 ? dot3(me + 6, acc) : 0.f;
    float* o = res + threadIdx.x * kOut;
    for (int k = 0; k < 3; ++k) { o[k] = acc[k]; o[3 + k] = nj[k]; }
    o[6] = along + xtra[body * kXtra + 9] * me[13];
  }
  __syncthreads();
  if (tau) {
    float* out = tau + (size_t)env0 * nv;
    for (int e = threadIdx.x; e < here * nv; e += kThreads) {
      const int k = e / nv, d = e - k * nv;
      out[e] = d < 6 ? res[k * nb * kOut + d] : res[(k * nb + d - 5) * kOut + 6];
    }
  }
  if (joint_force) {
    float* out = joint_force + (size_t)env0 * nb * 3;
    for (int e = threadIdx.x; e < here * nb * 3; e += kThreads) {
      const int l = e / 3, c = e - l * 3;
      out[e] = res[l * kOut + c];
    }
  }
  if (joint_torque) {
    float* out = joint_torque + (size_t)env0 * nb * 3;
    for (int e = threadIdx.x; e < here * nb * 3; e += kThreads) {
      const int l = e / 3, c = e - l * 3;
      out[e] = res[l * kOut + 3 + c];
    }
  }
}

// x = K^-1 rhs for the symmetric positive definite 6 x 6 K = [[J, H], [H^T, M]]: LDL^T with every index a compile-time constant (registers)
__device__ __forceinline__ void spd6_solve(const float* J, const float* H, const float* M, const float* rhs, float* x) {
  float K[6][6], Dg[6];
  const int sy[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { K[i][j] = J[sy[i][j]]; K[3 + i][3 + j] = M[sy[i][j]]; K[i][3 + j] = H[3 * i + j]; K[3 + j][i] = H[3 * i + j]; }
#pragma unroll
  for (int j = 0; j < 6; ++j) {      // K's strict lower triangle becomes L, Dg the diagonal
    float d = K[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= K[j][k] * K[j][k] * Dg[k];
    Dg[j] = d;
    const float id = recip(d);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float s = K[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= K[i][k] * K[j][k] * Dg[k];
      K[i][j] = s * id;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float s = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= K[i][k] * x[k];
    x[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] *= recip(Dg[i]);
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float s = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= K[k][i] * x[k];
    x[i] = s;
  }
}

__global__ __launch_bounds__(kThreads) void aba_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                       const float* __restrict__ tau, const FrameList frames, const Loads loads, int N, const Vec3 g,
                                                       float* __restrict__ udot) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ float art[kThreads * kArt];
  __shared__ float accl[kThreads * kAcc];
  __shared__ float outl[kRowsOut];
  const DevModel& m = *model;
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  __syncthreads();
  const int nb = m.nb, depth = m.depth, nv = m.nv;
  const auto [env0, here, el, body] = env_block(nb, N);
  const bool active = el < here;
  const int level = active ? m.level[body] : -1;
  const float gvec[3] = {g.x, g.y, g.z};
  float J[6], H[9], M[6], pA[6], sa[3], sl[3], cb[6], U[6], iD = 0.f, uu = 0.f, wxv[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < 6; ++k) { J[k] = 0.f; M[k] = 0.f; pA[k] = 0.f; cb[k] = 0.f; U[k] = 0.f; }
  for (int k = 0; k < 9; ++k) H[k] = 0.f;
  for (int k = 0; k < 3; ++k) { sa[k] = 0.f; sl[k] = 0.f; }
  const float* trow = nullptr;
  if (active) {
    const long long env = env0 + el;
    const float* q = gc + (size_t)env * m.nq;
    const float* u = gv + (size_t)env * nv;
    trow = tau + (size_t)env * nv;
    Chain b;
    walk_chain<false>(m, rows, q, u, nullptr, true, body, b, NoJoint{});
    const float* x = xtra + body * kXtra;
    const float mass = rows[body * kRow + 7];
    float po[3], rc[3], r[3], wr[3], fm[3], wb[3], Iwb[3], Iw[3], nm[3], t0[3], vo[3], fe[3], ne[3];
    mat3_vec(b.R, x, rc);
    for (int k = 0; k < 3; ++k) { po[k] = b.p[k] - q[k]; r[k] = po[k] + rc[k]; }
    cross3(b.w, rc, wr);
    for (int k = 0; k < 3; ++k) fm[k] = mass * (b.v[k] + wr[k]);      // momentum, and the angular momentum about o
    mat3t_vec(b.R, b.w, wb);
    sym3_vec(x + 3, wb, Iwb);
    mat3_vec(b.R, Iwb, Iw);
    cross3(r, fm, t0);
    for (int k = 0; k < 3; ++k) nm[k] = Iw[k] + t0[k];
    cross3(b.w, po, t0);
    for (int k = 0; k < 3; ++k) vo[k] = b.v[k] - t0[k];               // velocity of the body's point at o
    body_loads(loads, frames, env, body, b.R, po, q, fe, ne);
    float wn[3], vf[3], wf[3];
    cross3(b.w, nm, wn);
    cross3(vo, fm, vf);
    cross3(b.w, fm, wf);
    for (int k = 0; k < 3; ++k) { pA[k] = (wn[k] + vf[k]) - ne[k]; pA[3 + k] = wf[k] - fe[k]; }
    inertia_about_o(b.R, x + 3, mass, r, J);
    H[1] = -mass * r[2]; H[2] = mass * r[1]; H[3] = mass * r[2]; H[5] = -mass * r[0]; H[6] = -mass * r[1]; H[7] = mass * r[0];      // m [r]x
    M[0] = mass; M[3] = mass; M[5] = mass;
    if (body == 0) {
      cross3(b.w, b.v, wxv);
    } else {
      float ppo[3], vop[3], c0[3], c1[3];
      if (b.type == 1) {
        for (int k = 0; k < 3; ++k) sa[k] = b.a[k];
        cross3(po, b.a, sl);
      } else {
        for (int k = 0; k < 3; ++k) sl[k] = b.a[k];
      }
      for (int k = 0; k < 3; ++k) ppo[k] = b.pp[k] - q[k];
      cross3(b.wp, ppo, t0);
      for (int k = 0; k < 3; ++k) vop[k] = b.vp[k] - t0[k];
      cross3(b.wp, sa, c0);                // c = qd (V_parent x S)
      cross3(b.wp, sl, c1);
      cross3(vop, sa, t0);
      for (int k = 0; k < 3; ++k) { cb[k] = c0[k] * b.qd; cb[3 + k] = (c1[k] + t0[k]) * b.qd; }
    }
  }
  for (int l = depth - 1; l >= 1; --l) {
    if (level == l) {
      float t0[3], t1[3];
      sym3_vec(J, sa, t0); mat3_vec(H, sl, t1);
      for (int k = 0; k < 3; ++k) U[k] = t0[k] + t1[k];
      mat3t_vec(H, sa, t0); sym3_vec(M, sl, t1);
      for (int k = 0; k < 3; ++k) U[3 + k] = t0[k] + t1[k];
      const float D = (dot3(sa, U) + dot3(sl, U + 3)) + xtra[body * kXtra + 9];
      iD = recip(D);
      uu = trow[5 + body] - (dot3(sa, pA) + dot3(sl, pA + 3));
      float Ja[6], Ha[9], Ma[6];
      int n = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++n) { Ja[n] = J[n] - U[i] * U[j] * iD; Ma[n] = M[n] - U[3 + i] * U[3 + j] * iD; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ha[3 * i + j] = H[3 * i + j] - U[i] * U[3 + j] * iD;
      float* s = art + threadIdx.x * kArt;
      for (int k = 0; k < 6; ++k) { s[k] = Ja[k]; s[15 + k] = Ma[k]; }
      for (int k = 0; k < 9; ++k) s[6 + k] = Ha[k];
      sym3_vec(Ja, cb, t0); mat3_vec(Ha, cb + 3, t1);
      for (int k = 0; k < 3; ++k) s[21 + k] = pA[k] + (t0[k] + t1[k]) + U[k] * (uu * iD);
      mat3t_vec(Ha, cb, t0); sym3_vec(Ma, cb + 3, t1);
      for (int k = 0; k < 3; ++k) s[24 + k] = pA[3 + k] + (t0[k] + t1[k]) + U[3 + k] * (uu * iD);
    }
    __syncthreads();
    if (level == l - 1) {      // gather from the children, ascending body order
      const int k0 = m.kid_start[body], k1 = k0 + m.kid_count[body];
      for (int kk = k0; kk < k1; ++kk) {
        const float* s = art + (el * nb + m.kid_list[kk]) * kArt;
        for (int k = 0; k < 6; ++k) { J[k] += s[k]; M[k] += s[15 + k]; pA[k] += s[21 + k]; }
        for (int k = 0; k < 9; ++k) H[k] += s[6 + k];
      }
    }
  }
  if (level == 0) {
    float A0[6] = {0.f, 0.f, 0.f, -gvec[0], -gvec[1], -gvec[2]};
    float* o = outl + el * nv;
    if (!m.fixed_base) {
      float rhs[6];
      for (int k = 0; k < 3; ++k) { rhs[k] = trow[3 + k] - pA[k]; rhs[3 + k] = trow[k] - pA[3 + k]; }
      spd6_solve(J, H, M, rhs, A0);
      for (int k = 0; k < 3; ++k) { o[k] = A0[3 + k] + wxv[k] + gvec[k]; o[3 + k] = A0[k]; }
    } else {
      for (int k = 0; k < 6; ++k) o[k] = 0.f;
    }
    float* s = accl + threadIdx.x * kAcc;
    for (int k = 0; k < 6; ++k) s[k] = A0[k];
  }
  for (int l = 1; l < depth; ++l) {
    __syncthreads();
    if (level == l) {
      const float* ap = accl + (el * nb + m.parent[body]) * kAcc;
      float Ap[6];
      for (int k = 0; k < 6; ++k) Ap[k] = ap[k] + cb[k];
      const float qdd = (uu - (dot3(U, Ap) + dot3(U + 3, Ap + 3))) * iD;
      float* s = accl + threadIdx.x * kAcc;
      for (int k = 0; k < 3; ++k) { s[k] = Ap[k] + sa[k] * qdd; s[3 + k] = Ap[3 + k] + sl[k] * qdd; }
      outl[el * nv + 5 + body] = qdd;
    }
  }
  __syncthreads();
  float* out = udot + (size_t)env0 * nv;
  for (int e = threadIdx.x; e < here * nv; e += kThreads) out[e] = outl[e];
}

}  // namespace

// the argument checks both entry points share (after check_world); RSB_OK, or RSB_E_INVALID with a message
int check_dynamics_loads(const rsb_world* w, const char* who, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags) {
  if (n_frames < 0 || n_frames > RSB_MAX_FRAMES) return invalid(who, "n_frames must be 0.." + std::to_string(RSB_MAX_FRAMES));
  if (n_frames > 0) {
    if (!frames) return invalid(who, "frames is NULL with n_frames > 0");
    if (!force && !torque) return invalid(who, "force and torque are both NULL with n_frames > 0");
    const int st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  }
  if (flags & ~RSB_DYN_CONTACTS) return invalid(who, "unknown flag bits");
  return RSB_OK;
}

namespace {

// what the launch hands the kernels: the staged loads (either may be null) and, with RSB_DYN_CONTACTS, the resident contact list
Loads loads_of(const rsb_world* w, const float* force, const float* torque, int n_frames, int flags) {
  const bool contacts = (flags & RSB_DYN_CONTACTS) != 0;
  return {force, torque, contacts ? w->d_contacts : nullptr, contacts ? w->d_count : nullptr, n_frames, w->kmax, (float)(1.0 / w->dt)};
}

}  // namespace

int launch_forward_dynamics(rsb_world* w, hipStream_t s, const float* tau, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags,
                            float* udot) {
  hipLaunchKernelGGL(aba_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, s, (const DevModel*)w->d_model, (const float*)w->d_gc, (const float*)w->d_gv,
                     tau ? tau : (const float*)w->d_tff, n_frames ? frame_list(frames, n_frames) : FrameList{}, loads_of(w, force, torque, n_frames, flags), w->N,
                     gravity_of(w), udot);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_inverse_dynamics(rsb_world* w, const float* udot, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags, float* tau,
                         float* joint_force, float* joint_torque, int space) {
  const char* who = "rsb_inverse_dynamics";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!tau && !joint_force && !joint_torque) return invalid(who, "every output is NULL");
  st = check_dynamics_loads(w, who, frames, n_frames, force, torque, flags); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = (size_t)w->N, nv = (size_t)w->blob.nv, nb3 = (size_t)w->blob.nb * 3, lf = N * (size_t)n_frames * 3;
  const float *dud, *df, *dq;
  float *dt, *djf, *djt;
  Staged io(w, space);      // [udot | force | torque | outputs]; without frames the loads are not read
  io.in(dud, udot, N * nv); io.in(df, n_frames ? force : nullptr, lf); io.in(dq, n_frames ? torque : nullptr, lf);
  io.out(dt, tau, N * nv); io.out(djf, joint_force, N * nb3); io.out(djt, joint_torque, N * nb3);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(rnea_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc, (const float*)w->d_gv, dud,
                     n_frames ? frame_list(frames, n_frames) : FrameList{}, loads_of(w, df, dq, n_frames, flags), w->N, gravity_of(w), dt, djf, djt);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_forward_dynamics(rsb_world* w, const float* tau, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags, float* udot,
                         int space) {
  const char* who = "rsb_forward_dynamics";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!udot) return invalid(who, "the output is NULL");
  st = check_dynamics_loads(w, who, frames, n_frames, force, torque, flags); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = (size_t)w->N, nv = (size_t)w->blob.nv, lf = N * (size_t)n_frames * 3;
  const float *dt, *df, *dq;
  float* dud;
  Staged io(w, space);      // [tau | force | torque | udot]; tau == NULL: the resident feed-forward rows
  io.in(dt, tau, N * nv); io.in(df, n_frames ? force : nullptr, lf); io.in(dq, n_frames ? torque : nullptr, lf);
  io.out(dud, udot, N * nv);
  st = io.begin(); if (st != RSB_OK) return st;
  st = launch_forward_dynamics(w, stream_of(w), dt, frames, n_frames, df, dq, flags, dud); if (st != RSB_OK) return st;
  return io.end();
}

}  // extern "C"
