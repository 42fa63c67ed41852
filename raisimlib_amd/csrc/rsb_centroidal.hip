// rsb_centroidal.hip — batched whole-body quantities from the resident state (rsb_get_centroidal, rsb_get_centroidal_momentum_matrix; include/rsb.h).
//
// What ArticulatedSystem::getCOM / getLinearMomentum / getAngularMomentum / getKineticEnergy / getPotentialEnergy / getEnergy give for one object on
// the host [RECALL], and the centroidal momentum matrix, for all N envs in one call, from d_gc / d_gv on the world's stream.  Nothing here is shared
// with the step kernel: two short kernels of their own, called between two control steps.
//
// Both kernels give a workgroup epb = 256 / nb CONSECUTIVE envs and one lane per (env, body) (EnvBlock).  A lane walks its body's support chain
// (walk_chain: the running transform and velocity in registers), so it knows R_i, p_i, omega_i, v_i of its body; the extra body constants (centre
// of mass, inertia, armature: 17-26 of DevModel::bodyf) come from an LDS table of their own (stage_xtra), not from the walk's rows.  The walk, the
// tables and the staging of the RSB_HOST forms are those of all batched queries (frames_chain.h).  centroidal_matrix_kernel keeps its own
// prologue, inertia block and subtree loop, not EnvBlock / inertia_about_o / subtree_sum: with them its instructions come in another order, 0.1 us
// slower on the Atlas-like model (profiles/query_common_ab.txt).
// Everything that is summed over bodies - first moments, angular momentum, inertia - is taken about the env's BASE ORIGIN o = p_0, never about the
// world origin: an env standing 50 m away keeps all its bits for what happens inside the robot.
//     r_i = (p_i - o) + R_i com_i      v_ci = v_i + omega_i x R_i com_i      I_w,i = R_i I_i R_i^T
//
//   centroidal_kernel         (1) every lane leaves ten partials in LDS: m_i r_i, m_i v_ci, I_w,i omega_i + m_i r_i x v_ci, and the body's kinetic
//                             energy 1/2 m_i v_ci^2 + 1/2 omega_i . I_w,i omega_i + 1/2 armature_i qd_i^2; (2) one lane per (env, partial) adds the nb
//                             bodies' values in ascending body order; (3) one lane per (env, output float) finalises: with h, P, L_o, T the sums and
//                             M the total mass, c = o + h / M, c' = P / M, L_c = L_o - (h / M) x P, U = -M g . c.  A NULL output skips its store.
//   centroidal_matrix_kernel  three phases, like the Jacobian kernel.  (1) every lane leaves its body's spatial inertia about o (m_i, m_i r_i, the six
//                             entries of I_w,i + m_i (r_i . r_i 1 - r_i r_i^T)) and its joint (a_i, s_i = p_i - o) in LDS; (2) one lane per (env, body j)
//                             adds the records of the bodies i of j's subtree (anc[i * depth + level[j]] == j) in ascending i: the composite
//                             inertia (m_j*, h_j*, I_j*) of the subtree, body 0's being the whole tree's; (3) all lanes sweep the block's contiguous
//                             6 nv floats per env, consecutive lanes writing consecutive floats.  Column 5 + j is the momentum of subtree j under unit
//                             motion of joint j, moved to the centre of mass (cb = h_0* / M):
//                                revolute   vo = s_j x a_j   P = m_j* vo + a_j x h_j*   L_o = I_j* a_j + h_j* x vo
//                                prismatic                   P = m_j* a_j               L_o = h_j* x a_j
//                                base linear e:  P = M e, L_c = 0        base angular e:  P = e x h_0*, L_o = I_0* e        L_c = L_o - cb x P
// A result of env e depends on env e's rows alone and the order of every sum is fixed: the same bits for any N, any subset of outputs, host or
// device outputs.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kPart = 11;      // centroidal_kernel: ten partials per lane, odd pitch
constexpr int kRec = 17;       // centroidal_matrix_kernel, per lane: m 0, m r 1-3, inertia about o 4-9, a 10-12, s 13-15, revolute 16
constexpr int kComp = 11;      // ... and per (env, body) composite: m* 0, h* 1-3, I* 4-9

__global__ __launch_bounds__(kThreads) void centroidal_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv, int N,
                                                              float total_mass, const Vec3 g, float* __restrict__ com, float* __restrict__ com_vel,
                                                              float* __restrict__ lin_mom, float* __restrict__ ang_mom, float* __restrict__ kinetic,
                                                              float* __restrict__ potential) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ float part[kThreads * kPart];
  __shared__ float sums[kThreads * kPart];      // per env of the block: h 0-2, P 3-5, L_o 6-8, T 9
  const DevModel& m = *model;
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  __syncthreads();
  const int nb = m.nb;
  const auto [env0, here, el, body] = env_block(nb, N);
  if (el < here) {
    const float* q = gc + (size_t)(env0 + el) * m.nq;
    const float* u = gv + (size_t)(env0 + el) * m.nv;
    Chain c;
    walk_chain<false>(m, rows, q, u, nullptr, true, body, c, NoJoint{});
    const float* x = xtra + body * kXtra;
    const float mass = rows[body * kRow + 7];
    float rc[3], wr[3], r[3], vc[3], wb[3], Iwb[3], Iw[3], rv[3];
    mat3_vec(c.R, x, rc);
    cross3(c.w, rc, wr);
    for (int k = 0; k < 3; ++k) { r[k] = (c.p[k] - q[k]) + rc[k]; vc[k] = c.v[k] + wr[k]; }
    for (int k = 0; k < 3; ++k) wb[k] = c.R[k] * c.w[0] + c.R[3 + k] * c.w[1] + c.R[6 + k] * c.w[2];      // R^T omega (not mat3t_vec: inlined here it contracts differently and the bits move)
    sym3_vec(x + 3, wb, Iwb);
    mat3_vec(c.R, Iwb, Iw);
    cross3(r, vc, rv);
    const float qd = (body >= 1) ? u[5 + body] : 0.f;
    float* s = part + threadIdx.x * kPart;
    for (int k = 0; k < 3; ++k) { s[k] = mass * r[k]; s[3 + k] = mass * vc[k]; s[6 + k] = Iw[k] + mass * rv[k]; }
    s[9] = 0.5f * mass * dot3(vc, vc) + 0.5f * dot3(wb, Iwb) + 0.5f * x[9] * qd * qd;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < here * 10; e += kThreads) {
    const int k = e / 10, j = e - k * 10;
    const float* s = part + k * nb * kPart + j;
    float acc = 0.f;
    for (int b = 0; b < nb; ++b) acc += s[b * kPart];
    sums[k * kPart + j] = acc;
  }
  __syncthreads();
  const float inv_m = 1.0f / total_mass;
  const float gvec[3] = {g.x, g.y, g.z};
  for (int e = threadIdx.x; e < here * 14; e += kThreads) {
    const int k = e / 14, j = e - k * 14;
    const float* s = sums + k * kPart;
    const long long env = env0 + k;
    const float* q = gc + (size_t)env * m.nq;
    const float cb[3] = {s[0] * inv_m, s[1] * inv_m, s[2] * inv_m};
    if (j < 3) {
      if (com) com[env * 3 + j] = q[j] + cb[j];
    } else if (j < 6) {
      if (com_vel) com_vel[env * 3 + (j - 3)] = s[j] * inv_m;
    } else if (j < 9) {
      if (lin_mom) lin_mom[env * 3 + (j - 6)] = s[j - 3];
    } else if (j < 12) {
      const int r = j - 9, r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
      if (ang_mom) ang_mom[env * 3 + r] = s[6 + r] - (cb[r1] * s[3 + r2] - cb[r2] * s[3 + r1]);
    } else if (j == 12) {
      if (kinetic) kinetic[env] = s[9];
    } else {
      const float c[3] = {q[0] + cb[0], q[1] + cb[1], q[2] + cb[2]};
      if (potential) potential[env] = -total_mass * dot3(gvec, c);
    }
  }
}

__global__ __launch_bounds__(kThreads) void centroidal_matrix_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, int N, float total_mass,
                                                                     float* __restrict__ A) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ float rec[kThreads * kRec];
  __shared__ float comp[kThreads * kComp];
  const DevModel& m = *model;
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  __syncthreads();
  const int nb = m.nb, epb = kThreads / nb, depth = m.depth;
  const long long env0 = (long long)blockIdx.x * epb;
  const int here = (int)min((long long)epb, (long long)N - env0);
  const int el = threadIdx.x / nb, body = threadIdx.x - el * nb;
  if (el < here) {
    const float* q = gc + (size_t)(env0 + el) * m.nq;
    float a[3] = {0.f, 0.f, 0.f}, sj[3] = {0.f, 0.f, 0.f}, rev = 0.f;
    Chain c;
    walk_chain<false>(m, rows, q, nullptr, nullptr, false, body, c, [&](int, int, const float* ai, const float* pi, bool revolute) {      // the last call is the body's own joint
      for (int k = 0; k < 3; ++k) { a[k] = ai[k]; sj[k] = pi[k] - q[k]; }
      rev = revolute ? 1.f : 0.f;
    });
    const float* x = xtra + body * kXtra;
    const float mass = rows[body * kRow + 7];
    float rc[3], r[3], B[9];
    mat3_vec(c.R, x, rc);
    for (int k = 0; k < 3; ++k) r[k] = (c.p[k] - q[k]) + rc[k];
    for (int k = 0; k < 3; ++k) {      // B = R I
      B[3 * k] = c.R[3 * k] * x[3] + c.R[3 * k + 1] * x[4] + c.R[3 * k + 2] * x[5];
      B[3 * k + 1] = c.R[3 * k] * x[4] + c.R[3 * k + 1] * x[6] + c.R[3 * k + 2] * x[7];
      B[3 * k + 2] = c.R[3 * k] * x[5] + c.R[3 * k + 1] * x[7] + c.R[3 * k + 2] * x[8];
    }
    const float rr = dot3(r, r);
    float* s = rec + threadIdx.x * kRec;
    s[0] = mass;
    for (int k = 0; k < 3; ++k) { s[1 + k] = mass * r[k]; s[10 + k] = a[k]; s[13 + k] = sj[k]; }
    s[16] = rev;
    int n = 4;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j, ++n)      // (R I R^T)_ij + m (r.r delta_ij - r_i r_j)
        s[n] = (B[3 * i] * c.R[3 * j] + B[3 * i + 1] * c.R[3 * j + 1] + B[3 * i + 2] * c.R[3 * j + 2]) + mass * ((i == j ? rr : 0.f) - r[i] * r[j]);
  }
  __syncthreads();
  if (el < here) {      // the composite of the subtree below this lane's body
    const int lj = m.level[body];
    const float* s = rec + el * nb * kRec;
    float acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    for (int i = body; i < nb; ++i) {      // (a subtree's bodies are numbered from its root up: parent[i] < i)
      if (m.anc[i * depth + lj] != body) continue;
      for (int k = 0; k < 10; ++k) acc[k] += s[i * kRec + k];
    }
    float* o = comp + threadIdx.x * kComp;
    for (int k = 0; k < 10; ++k) o[k] = acc[k];
  }
  __syncthreads();
  const int nv = m.nv, per = 6 * nv;
  const bool fixed = m.fixed_base != 0;
  const float inv_m = 1.0f / total_mass;
  const size_t out0 = (size_t)env0 * per;
  for (int e = threadIdx.x; e < here * per; e += kThreads) {
    const int k = e / per, rem = e - k * per, r = rem / nv, d = rem - r * nv;
    const int j = d < 6 ? 0 : d - 5;
    const float* cj = comp + (k * nb + j) * kComp;
    const float* c0 = comp + k * nb * kComp;
    const float* s = rec + (k * nb + j) * kRec;
    const float cb[3] = {c0[1] * inv_m, c0[2] * inv_m, c0[3] * inv_m};
    const float* h = cj + 1;
    float P[3] = {0.f, 0.f, 0.f}, Lo[3] = {0.f, 0.f, 0.f};
    bool centred = false;      // L_c known without the shift
    if (d < 3) {
      if (!fixed) P[d] = total_mass;
      centred = true;
    } else if (d < 6) {
      if (!fixed) {
        float ev[3] = {0.f, 0.f, 0.f};
        ev[d - 3] = 1.f;
        cross3(ev, h, P);
        sym3_vec(cj + 4, ev, Lo);
      } else {
        centred = true;
      }
    } else if (s[16] != 0.f) {
      float vo[3], ah[3], hv[3];
      cross3(s + 13, s + 10, vo);
      cross3(s + 10, h, ah);
      cross3(h, vo, hv);
      sym3_vec(cj + 4, s + 10, Lo);
      for (int t = 0; t < 3; ++t) { P[t] = cj[0] * vo[t] + ah[t]; Lo[t] += hv[t]; }
    } else {
      cross3(h, s + 10, Lo);
      for (int t = 0; t < 3; ++t) P[t] = cj[0] * s[10 + t];
    }
    float val;
    if (r < 3) {
      val = P[r];
    } else if (centred) {
      val = 0.f;
    } else {
      float cp[3];
      cross3(cb, P, cp);
      val = Lo[r - 3] - cp[r - 3];
    }
    A[out0 + e] = val;
  }
}

int check_mass(const rsb_world* w, const char* who, float* total) {
  double s = 0.0;
  for (int i = 0; i < w->blob.nb; ++i) s += w->blob.mass[i];
  if (!(s > 0.0) || !std::isfinite(s) || !((float)s > 0.f)) { rsb::set_error(std::string(who) + ": the model's total mass is not positive"); return RSB_E_UNSUPPORTED; }
  *total = (float)s;
  return RSB_OK;
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_get_centroidal(rsb_world* w, float* com, float* com_vel, float* lin_mom, float* ang_mom, float* kinetic, float* potential, int space) {
  const char* who = "rsb_get_centroidal";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  float* host[6] = {com, com_vel, lin_mom, ang_mom, kinetic, potential};
  bool any = false;
  for (float* p : host) any = any || p;
  if (!any) return invalid(who, "every output is NULL");
  float total = 0.f;
  st = check_mass(w, who, &total); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  float* dev[6];
  const size_t width[6] = {3, 3, 3, 3, 1, 1};
  Staged io(w, space);
  for (int k = 0; k < 6; ++k) io.out(dev[k], host[k], (size_t)w->N * width[k]);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(centroidal_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc,
                     (const float*)w->d_gv, w->N, total, gravity_of(w), dev[0], dev[1], dev[2], dev[3], dev[4], dev[5]);
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_get_centroidal_momentum_matrix(rsb_world* w, float* A, int space) {
  const char* who = "rsb_get_centroidal_momentum_matrix";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!A) return invalid(who, "the output is NULL");
  float total = 0.f;
  st = check_mass(w, who, &total); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  float* dA;
  Staged io(w, space);
  io.out(dA, A, (size_t)w->N * 6 * w->blob.nv);
  st = io.begin(); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(centroidal_matrix_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc, w->N,
                     total, dA);
  HIP_TRY(hipGetLastError());
  return io.end();
}

}  // extern "C"
