// rsb_inverse_mass.hip — batched inverse-mass solves and frame Delassus matrices from the resident configuration
// (rsb_apply_inverse_mass, rsb_get_frame_delassus; include/rsb.h, where the conventions are stated).
//
//   X = (M(q) + D)^-1 B      JMinv = J (M + D)^-1      G = J (M + D)^-1 J^T          D = diag(joint_diag), J the rows of rsb_get_frame_jacobians
// for all N envs in one call, from d_gc on the world's stream, without ever forming M.  The articulated-body factorisation of aba_kernel
// (rsb_dynamics.hip) depends on q alone: it is done ONCE per env, and every column then costs only the bias-force up pass, the base
// back-substitution and the acceleration down pass - O(nb) per column.
//
// Mapping: aba_kernel's.  A workgroup owns epb = 256 / nb CONSECUTIVE envs, one lane per (env, body) (EnvBlock), in the common frame: world axes,
// the env's base origin o = p_0 as the origin, so that every spatial transform is the identity.
//   phase 1, once   the chain walk (walk_chain's recursion without velocities, positions counted from o), the body's inertia about o as (J 6, H 9,
//                   M 6) and its joint's spatial axis; up pass, deepest level to level 1: the bodies of level l publish  IA - U U^T / D  (21
//                   entries) to LDS, barrier, level l - 1 gathers its children in ascending body order; D = S^T U + armature + joint_diag; an
//                   LDL^T of the base's 6 x 6 block.  ALL of phase 1 runs in DOUBLE.  In the common frame a distal joint's D, a few 1e-4 on the
//                   humanoid, is what is left of inertias about o of order 1 (m r^2 against the levers in S), and IA - U U^T / D cancels again
//                   along every axis below: float roundings there are errors of M itself that no column pass takes back.  Restated in numpy
//                   (tools/inverse_mass_restatement.py) a float phase 1 misses the residual bar |A x - b| <= 2e-5 (1 + |A||x| + |b|) by 4.1 x on
//                   the humanoid's unit right-hand sides (cond(M) 4.6e5) and ends at a forward error of 5.0e-4 where the double one ends at 3.1e-7: it is paid once
//                   per env, not per column.  A lane keeps, rounded to float, U (6), 1 / D and S in registers; the base lane keeps the factors
//                   (15 + 6 floats).  With velocities and bias accelerations zero nothing else of aba_kernel is left.
//   phase 2, per column c (the loop is uniform over the workgroup)
//                   up:    u_i = b_i - S^T p_i; level l publishes p_i + U_i u_i / D_i (6 floats), barrier, level l - 1 gathers, ascending;
//                   base:  a_0 = K^-1 (b_0 - p_0) with the kept factors; a fixed base takes a_0 = 0;
//                   down:  level by level, qdd_i = (u_i - U_i^T a_parent) / D_i, a_i = a_parent + S_i qdd_i through a second LDS array.
//     solve_kernel     b = B[e, c, :], p starts at zero, udot goes to X[e, c, :].  Every float of B is read by the lane that later writes the
//                      same float of X, before it writes: X == B is allowed.
//     delassus_kernel  column c = (frame f, axis a): b = 0 and the bias force of f's body is MINUS the unit world force along a at the frame's
//                      point (rows 0..2 of a frame) or the unit world torque about a (rows 3..5).  udot is then (M + D)^-1 J_c^T = row c of JMinv
//                      (the matrix is symmetric).  After one more barrier entry (i, c), i <= c, is read off the spatial acceleration of frame i's
//                      body, a_lin + alpha x (point_i - o) or alpha, by the env's lane i mod nb, and stored to G[i][c] AND G[c][i]: G equals its
//                      transpose bit for bit and no dense J is formed.
// Barriers after phase 1: 2 (depth - 1) per column, + 1 where G is asked for.  No atomics; every sum has a fixed order; the only reciprocals are
// phase 1's, in double; a column multiplies by what was kept.  A result of env e depends on env e's rows alone: the same bits for any N, any subset
// of outputs, host or device buffers.
// Static LDS, sized for 64 bodies whatever the tree: solve_kernel 58 112 B, delassus_kernel 58 368 B (phase 2's float arrays reuse phase 1's doubles).
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kArt = 21;       // per lane, phase 1, doubles: J 0-5, H 6-14, M 15-20 of the published articulated inertia
constexpr int kPub = 6;        // ... phase 2, floats: a column's published bias force
constexpr int kAcc = 7;        // ... spatial acceleration (angular 0-2, linear 3-5), odd pitch
constexpr int kPose = 12;      // ... delassus_kernel, phase 2, floats: R 0-8, p - o 9-11
static_assert((kPub + kPose) * sizeof(float) <= kArt * sizeof(double), "phase 2 lives in phase 1's LDS");

struct Diag { float d[RSB_MAX_DOF]; };                           // kernel arguments: joint_diag and the frames travel with the launch
struct DelFrames { rsb_frame f[RSB_MAX_DELASSUS_FRAMES]; };

// frames_chain.h's small products in double: phase 1 runs in double throughout
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void mat3_vec(const double* A, const double* x, double* o) {
  for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mat3t_vec(const double* A, const double* x, double* o) {
  for (int c = 0; c < 3; ++c) o[c] = A[c] * x[0] + A[3 + c] * x[1] + A[6 + c] * x[2];
}
__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* O) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void sym3_vec(const double* I, const double* x, double* o) {
  o[0] = I[0] * x[0] + I[1] * x[1] + I[2] * x[2];
  o[1] = I[1] * x[0] + I[3] * x[1] + I[4] * x[2];
  o[2] = I[2] * x[0] + I[4] * x[1] + I[5] * x[2];
}

// walk_chain's transforms (frames_chain.h: the same recursion, without velocities) in double and FROM THE BASE ORIGIN: on return R is the world
// transform of `body`, p = p_body - o, a its joint's axis in the world, type 0 base / 1 revolute / 2 prismatic
__device__ __forceinline__ void walk_double(const DevModel& m, const float* rows, const float* q, int body, double* R, double* p, double* a, int& type) {
  {
    double w = q[3], x = q[4], y = q[5], z = q[6];
    const double in = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= in; x *= in; y *= in; z *= in;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
    for (int k = 0; k < 3; ++k) { p[k] = 0.0; a[k] = 0.0; }
    type = 0;
  }
  const int lv = m.level[body];
  const int* anc = m.anc + body * m.depth;
  for (int l = 1; l <= lv; ++l) {
    const int i = anc[l];
    const float* row = rows + i * kRow;
    const bool revolute = __float_as_int(row[3]) == RSB_JOINT_REVOLUTE;
    const double ax[3] = {row[0], row[1], row[2]}, pt[3] = {row[4], row[5], row[6]}, qi = q[6 + i];
    double T[9], E[9], Rn[9], d[3];
    for (int k = 0; k < 9; ++k) T[k] = row[8 + k];
    if (revolute) {
      double sn, cs, Rq[9];
      sincos(qi, &sn, &cs);
      const double t = 1.0 - cs;
      Rq[0] = cs + ax[0] * ax[0] * t;         Rq[1] = ax[0] * ax[1] * t - ax[2] * sn; Rq[2] = ax[0] * ax[2] * t + ax[1] * sn;
      Rq[3] = ax[1] * ax[0] * t + ax[2] * sn; Rq[4] = cs + ax[1] * ax[1] * t;         Rq[5] = ax[1] * ax[2] * t - ax[0] * sn;
      Rq[6] = ax[2] * ax[0] * t - ax[1] * sn; Rq[7] = ax[2] * ax[1] * t + ax[0] * sn; Rq[8] = cs + ax[2] * ax[2] * t;
      mat3_mul(T, Rq, E);
    } else {
      for (int k = 0; k < 9; ++k) E[k] = T[k];
    }
    mat3_mul(R, E, Rn);
    mat3_vec(R, pt, d);
    mat3_vec(Rn, ax, a);
    if (!revolute) for (int k = 0; k < 3; ++k) d[k] += a[k] * qi;
    for (int k = 0; k < 3; ++k) p[k] += d[k];
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    type = revolute ? 1 : 2;
  }
}

// LDL^T of the symmetric positive definite 6 x 6 K = [[J, H], [H^T, M]], every index a compile-time constant (registers): L's strict lower
// triangle row by row (15) and the reciprocals of the diagonal (6)
__device__ __forceinline__ void ldl6_factor(const double* J, const double* H, const double* M, float* L, float* iDg) {
  double K[6][6], Dg[6];
  const int sy[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { K[i][j] = J[sy[i][j]]; K[3 + i][3 + j] = M[sy[i][j]]; K[i][3 + j] = H[3 * i + j]; K[3 + j][i] = H[3 * i + j]; }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = K[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= K[j][k] * K[j][k] * Dg[k];
    Dg[j] = d;
    const double id = 1.0 / d;
    iDg[j] = (float)id;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = K[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= K[i][k] * K[j][k] * Dg[k];
      K[i][j] = s * id;
      L[i * (i - 1) / 2 + j] = (float)K[i][j];
    }
  }
}

// x = K^-1 rhs from the factors
__device__ __forceinline__ void ldl6_solve(const float* L, const float* iDg, const float* rhs, float* x) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float s = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * (i - 1) / 2 + k] * x[k];
    x[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] *= iDg[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float s = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k * (k - 1) / 2 + i] * x[k];
    x[i] = s;
  }
}

// Both kernels.  DEL = false: C = n_rhs columns from B to X.  DEL = true: C = kk * F unit loads (kk = 3 or 6 rows per frame); X is JMinv (may be
// null), G may be null.  rows / xtra / art / accl, and with DEL frl, are the workgroup's LDS arrays; phase 2 reuses art's bytes for its float arrays.
template <bool DEL>
__device__ __forceinline__ void inverse_mass_body(const DevModel& m, const float* gc, const Diag& diag, int N, int C, const float* B, float* X, const DelFrames& frames,
                                                  int F, int kk, float* G, float* rows, float* xtra, double* art, float* accl, float* frl) {
  float* pub = reinterpret_cast<float*>(art);      // phase 2: a column's published bias forces, kPub per lane ...
  float* pose = pub + kThreads * kPub;             // ... and with DEL every body's (R, p - o), kPose per lane
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  if (DEL) {
    for (int k = 0; k < F; ++k)      // (a uniform index: the frames come through scalar loads)
      if (threadIdx.x == 0) {
        frl[4 * k] = __int_as_float(frames.f[k].body);
        for (int c = 0; c < 3; ++c) frl[4 * k + 1 + c] = frames.f[k].offset[c];
      }
  }
  __syncthreads();
  const int nb = m.nb, depth = m.depth, nv = m.nv;
  const bool fixed = m.fixed_base != 0;
  const auto [env0, here, el, body] = env_block(nb, N);
  const bool active = el < here;
  const int level = active ? m.level[body] : -1;
  const int parent = (active && body > 0) ? m.parent[body] : 0;
  const int k0 = active ? m.kid_start[body] : 0, k1 = active ? k0 + m.kid_count[body] : 0;
  const long long env = env0 + el;
  double J[6], H[9], M[6], S[6];      // the articulated inertia and the joint's spatial axis (angular 0-2, linear 3-5): phase 1 is in double
  float sa[3], sl[3], U[6], iD = 0.f, Rw[9], po[3];
  for (int k = 0; k < 6; ++k) { J[k] = 0.0; M[k] = 0.0; S[k] = 0.0; U[k] = 0.f; }
  for (int k = 0; k < 9; ++k) { H[k] = 0.0; Rw[k] = 0.f; }
  for (int k = 0; k < 3; ++k) po[k] = 0.f;
  float dj = 0.f;      // this lane's joint_diag entry
  for (int k = 6; k < nv; ++k) dj = (k == 5 + body) ? diag.d[k] : dj;
  // ---- phase 1: the factorisation, once per env
  if (active) {
    double R[9], p[3], a[3];
    int type;
    walk_double(m, rows, gc + (size_t)env * m.nq, body, R, p, a, type);
    const float* x = xtra + body * kXtra;
    const double mass = rows[body * kRow + 7], com[3] = {x[0], x[1], x[2]}, I[6] = {x[3], x[4], x[5], x[6], x[7], x[8]};
    double rc[3], r[3], B9[9];
    mat3_vec(R, com, rc);
    for (int k = 0; k < 3; ++k) { r[k] = p[k] + rc[k]; po[k] = (float)p[k]; }
    for (int k = 0; k < 9; ++k) Rw[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) {      // B9 = R I, then (R I R^T)_ij + m (r.r delta_ij - r_i r_j): inertia_about_o of frames_chain.h
      B9[3 * k] = R[3 * k] * I[0] + R[3 * k + 1] * I[1] + R[3 * k + 2] * I[2];
      B9[3 * k + 1] = R[3 * k] * I[1] + R[3 * k + 1] * I[3] + R[3 * k + 2] * I[4];
      B9[3 * k + 2] = R[3 * k] * I[2] + R[3 * k + 1] * I[4] + R[3 * k + 2] * I[5];
    }
    const double rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    int n = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++n)
        J[n] = (B9[3 * i] * R[3 * j] + B9[3 * i + 1] * R[3 * j + 1] + B9[3 * i + 2] * R[3 * j + 2]) + mass * ((i == j ? rr : 0.0) - r[i] * r[j]);
    H[1] = -mass * r[2]; H[2] = mass * r[1]; H[3] = mass * r[2]; H[5] = -mass * r[0]; H[6] = -mass * r[1]; H[7] = mass * r[0];      // m [r]x
    M[0] = mass; M[3] = mass; M[5] = mass;
    if (type == 1) {
      for (int k = 0; k < 3; ++k) S[k] = a[k];
      cross3(p, a, S + 3);
    } else if (type == 2) {
      for (int k = 0; k < 3; ++k) S[3 + k] = a[k];
    }
  }
  for (int k = 0; k < 3; ++k) { sa[k] = (float)S[k]; sl[k] = (float)S[3 + k]; }      // what the columns use
  for (int l = depth - 1; l >= 1; --l) {
    if (level == l) {
      double Ud[6], t0[3], t1[3];
      sym3_vec(J, S, t0); mat3_vec(H, S + 3, t1);
      for (int k = 0; k < 3; ++k) Ud[k] = t0[k] + t1[k];
      mat3t_vec(H, S, t0); sym3_vec(M, S + 3, t1);
      for (int k = 0; k < 3; ++k) Ud[3 + k] = t0[k] + t1[k];
      double D = 0.0;
      for (int k = 0; k < 3; ++k) D += S[k] * Ud[k] + S[3 + k] * Ud[3 + k];
      D = (D + (double)xtra[body * kXtra + 9]) + (double)dj;
      const double iDd = 1.0 / D;
      iD = (float)iDd;
      for (int k = 0; k < 6; ++k) U[k] = (float)Ud[k];
      double* s = art + threadIdx.x * kArt;
      int n = 0;
      for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++n) { s[n] = J[n] - Ud[i] * Ud[j] * iDd; s[15 + n] = M[n] - Ud[3 + i] * Ud[3 + j] * iDd; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s[6 + 3 * i + j] = H[3 * i + j] - Ud[i] * Ud[3 + j] * iDd;
    }
    __syncthreads();
    if (level == l - 1) {      // gather from the children, ascending body order
      for (int kd = k0; kd < k1; ++kd) {
        const double* s = art + (el * nb + m.kid_list[kd]) * kArt;
        for (int k = 0; k < 6; ++k) J[k] += s[k];
        __builtin_amdgcn_sched_barrier(0);      // (the 21 doubles in three batches: all in flight at once cost 42 registers)
        for (int k = 0; k < 9; ++k) H[k] += s[6 + k];
        __builtin_amdgcn_sched_barrier(0);
        for (int k = 0; k < 6; ++k) M[k] += s[15 + k];
      }
    }
  }
  float L[15], iDg[6];      // the base lane's factors
  for (int k = 0; k < 15; ++k) L[k] = 0.f;
  for (int k = 0; k < 6; ++k) iDg[k] = 0.f;
  if (level == 0 && !fixed) ldl6_factor(J, H, M, L, iDg);
  __syncthreads();      // (phase 2 writes where the last gather read)
  if (DEL && active) {
    float* ps = pose + threadIdx.x * kPose;
    for (int k = 0; k < 9; ++k) ps[k] = Rw[k];
    for (int k = 0; k < 3; ++k) ps[9 + k] = po[k];
  }
  // ---- phase 2: one column at a time
  for (int c = 0; c < C; ++c) {
    float p[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bj = 0.f, uu = 0.f;
    float* xo = (X && active) ? X + ((size_t)env * C + c) * nv : nullptr;
    const float* bo = (!DEL && active) ? B + ((size_t)env * C + c) * nv : nullptr;
    if (DEL) {
      const int f = c / kk, a = c - f * kk;
      if (active && body == __float_as_int(frl[4 * f])) {
        if (a < 3) {      // minus the unit force along a at the point, and its moment about o
          const float* ps = pose + threadIdx.x * kPose;
          float r[3], e[3] = {a == 0 ? 1.f : 0.f, a == 1 ? 1.f : 0.f, a == 2 ? 1.f : 0.f}, n[3];
          mat3_vec(ps, frl + 4 * f + 1, r);
          for (int k = 0; k < 3; ++k) r[k] += ps[9 + k];
          cross3(r, e, n);
          for (int k = 0; k < 3; ++k) { p[k] = -n[k]; p[3 + k] = -e[k]; }
        } else {
          for (int k = 0; k < 3; ++k) p[k] = (a - 3 == k) ? -1.f : 0.f;
        }
      }
    } else if (active && body != 0) {
      bj = bo[5 + body];
    }
    for (int l = depth - 1; l >= 1; --l) {
      if (level == l) {
        uu = bj - (dot3(sa, p) + dot3(sl, p + 3));
        float* s = pub + threadIdx.x * kPub;
        for (int k = 0; k < 6; ++k) s[k] = p[k] + U[k] * (uu * iD);
      }
      __syncthreads();
      if (level == l - 1) {
        for (int kd = k0; kd < k1; ++kd) {
          const float* s = pub + (el * nb + m.kid_list[kd]) * kPub;
          for (int k = 0; k < 6; ++k) p[k] += s[k];
        }
      }
    }
    if (level == 0) {
      float A0[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (!fixed) {
        float rhs[6];
        for (int k = 0; k < 3; ++k) { rhs[k] = (DEL ? 0.f : bo[3 + k]) - p[k]; rhs[3 + k] = (DEL ? 0.f : bo[k]) - p[3 + k]; }
        ldl6_solve(L, iDg, rhs, A0);
      }
      if (xo)
        for (int k = 0; k < 3; ++k) { xo[k] = A0[3 + k]; xo[3 + k] = A0[k]; }
      float* s = accl + threadIdx.x * kAcc;
      for (int k = 0; k < 6; ++k) s[k] = A0[k];
    }
    for (int l = 1; l < depth; ++l) {
      __syncthreads();
      if (level == l) {
        const float* ap = accl + (el * nb + parent) * kAcc;
        float Ap[6];
        for (int k = 0; k < 6; ++k) Ap[k] = ap[k];
        const float qdd = (uu - (dot3(U, Ap) + dot3(U + 3, Ap + 3))) * iD;
        float* s = accl + threadIdx.x * kAcc;
        for (int k = 0; k < 3; ++k) { s[k] = Ap[k] + sa[k] * qdd; s[3 + k] = Ap[3 + k] + sl[k] * qdd; }
        if (xo) xo[5 + body] = qdd;
      }
    }
    if (DEL && G) {      // (a kernel argument: uniform)
      __syncthreads();
      if (active) {
        float* g = G + (size_t)env * C * C;
        for (int i = body; i <= c; i += nb) {
          const int fi = i / kk, ai = i - fi * kk;
          const int bi = __float_as_int(frl[4 * fi]);
          const float* ac = accl + (el * nb + bi) * kAcc;
          float v;
          if (ai < 3) {
            const float* ps = pose + (el * nb + bi) * kPose;
            const float al[3] = {ac[0], ac[1], ac[2]};
            float r[3], t[3];
            mat3_vec(ps, frl + 4 * fi + 1, r);
            for (int k = 0; k < 3; ++k) r[k] += ps[9 + k];
            cross3(al, r, t);
            v = ac[3 + ai] + (ai == 0 ? t[0] : ai == 1 ? t[1] : t[2]);
          } else {
            v = ac[ai - 3];
          }
          g[(size_t)i * C + c] = v;
          g[(size_t)c * C + i] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void solve_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const Diag diag, int N, int R, const float* B,
                                                         float* X) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ double art[kThreads * kArt];
  __shared__ float accl[kThreads * kAcc];
  inverse_mass_body<false>(*model, gc, diag, N, R, B, X, DelFrames{}, 0, 1, nullptr, rows, xtra, art, accl, nullptr);
}

__global__ __launch_bounds__(kThreads) void delassus_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const Diag diag, int N,
                                                            const DelFrames frames, int F, int kk, float* __restrict__ G, float* __restrict__ JMinv) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ double art[kThreads * kArt];
  __shared__ float accl[kThreads * kAcc];
  __shared__ float frl[RSB_MAX_DELASSUS_FRAMES * 4];
  inverse_mass_body<true>(*model, gc, diag, N, kk * F, nullptr, JMinv, frames, F, kk, G, rows, xtra, art, accl, frl);
}

// joint_diag (HOST [nv] or NULL: zeros) as the kernels take it; RSB_OK, or RSB_E_INVALID with a message.  A fixed base's six entries are not looked at.
int diag_of(const rsb_world* w, const char* who, const float* joint_diag, Diag* out) {
  *out = Diag{};
  if (!joint_diag) return RSB_OK;
  const int nv = w->blob.nv;
  for (int k = w->blob.fixed_base ? 6 : 0; k < nv; ++k) {
    const float d = joint_diag[k];
    if (!std::isfinite(d) || d < 0.f) return invalid(who, "joint_diag[" + std::to_string(k) + "] must be finite and not negative");
    if (k < 6 && d != 0.f) return invalid(who, "joint_diag[" + std::to_string(k) + "]: the six base entries of a floating base must be 0");
    out->d[k] = d;
  }
  return RSB_OK;
}

}  // namespace

int check_joint_diag(const rsb_world* w, const char* who, const float* joint_diag) {
  Diag diag;
  return diag_of(w, who, joint_diag, &diag);
}

int launch_frame_delassus(rsb_world* w, hipStream_t s, const rsb_frame* frames, int n_frames, int flags, const float* joint_diag, float* G, float* JMinv) {
  Diag diag{};      // (joint_diag has passed check_joint_diag: copied, not looked at again; a fixed base's six entries stay zero)
  for (int k = w->blob.fixed_base ? 6 : 0; joint_diag && k < w->blob.nv; ++k) diag.d[k] = joint_diag[k];
  DelFrames fl{};
  std::copy(frames, frames + n_frames, fl.f);
  hipLaunchKernelGGL(delassus_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, s, (const DevModel*)w->d_model, (const float*)w->d_gc, diag, w->N, fl, n_frames,
                     (flags & RSB_DELASSUS_ANGULAR) ? 6 : 3, G, JMinv);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

int launch_inverse_mass_solve(rsb_world* w, hipStream_t s, int n_rhs, const float* B, float* X) {
  hipLaunchKernelGGL(solve_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, s, (const DevModel*)w->d_model, (const float*)w->d_gc, Diag{}, w->N, n_rhs, B, X);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_apply_inverse_mass(rsb_world* w, const float* B, int n_rhs, const float* joint_diag, float* X, int space) {
  const char* who = "rsb_apply_inverse_mass";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (n_rhs < 1 || n_rhs > RSB_MAX_DOF) return invalid(who, "n_rhs must be 1.." + std::to_string(RSB_MAX_DOF));
  if (!B || !X) return invalid(who, "B or X is NULL");
  Diag diag;
  st = diag_of(w, who, joint_diag, &diag); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const size_t n = (size_t)w->N * (size_t)n_rhs * (size_t)w->blob.nv;
  const float* dB;
  float* dX;
  Staged io(w, space);      // [B | X]
  io.in(dB, B, n); io.out(dX, X, n);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(solve_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc, diag, w->N, n_rhs, dB, dX);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_get_frame_delassus(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, const float* joint_diag, float* G, float* JMinv, int space) {
  const char* who = "rsb_get_frame_delassus";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!G && !JMinv) return invalid(who, "every output is NULL");
  if (!frames || n_frames < 1 || n_frames > RSB_MAX_DELASSUS_FRAMES) return invalid(who, "n_frames must be 1.." + std::to_string(RSB_MAX_DELASSUS_FRAMES));
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (flags & ~RSB_DELASSUS_ANGULAR) return invalid(who, "unknown flag bits");
  st = check_joint_diag(w, who, joint_diag); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const int kk = (flags & RSB_DELASSUS_ANGULAR) ? 6 : 3;
  const size_t N = (size_t)w->N, rows = (size_t)kk * (size_t)n_frames;
  float *dG, *dJ;
  Staged io(w, space);      // [G | JMinv]
  io.out(dG, G, N * rows * rows); io.out(dJ, JMinv, N * rows * (size_t)w->blob.nv);
  st = io.begin(); if (st != RSB_OK) return st;
  st = launch_frame_delassus(w, stream_of(w), frames, n_frames, flags, joint_diag, dG, dJ); if (st != RSB_OK) return st;
  return io.end();
}

}  // extern "C"
