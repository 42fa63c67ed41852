// rsb_dynamics_derivatives.hip — batched analytic derivatives of inverse and forward dynamics at the resident state
// (rsb_inverse_dynamics_derivatives, rsb_forward_dynamics_derivatives; include/rsb.h, where the conventions are stated).
//
//   dtau_dq [i][j] = d tau_i / d x_j      dtau_dv [i][j] = d tau_i / d gv_j      dtau_dudot = M(q)          tau = ID(q, gv, udot, loads), rsb_inverse_dynamics
//   dudot_dq = -M^-1 dtau_dq |udot*       dudot_dv = -M^-1 dtau_dv               dudot_dtau = M^-1          udot* = FD(q, gv, tau, loads), rsb_forward_dynamics
// for all N envs in one call.  Exact tangents: forward-mode differentiation of rnea_kernel's recursion (rsb_dynamics.hip), no finite differences.
//
// tangent_kernel keeps rnea_kernel's mapping: a workgroup owns epb = 256 / nb CONSECUTIVE envs, one lane per (env, body) (EnvBlock).  The chain walk
// and the body's net wrench about the env's base origin o are written ONCE, as templates over their scalars: with float they are the primal pass, with
// Dual (value, tangent) the pass of one direction.  The three kinds of direction differ only in their seed and in which scalars are Dual:
//     x_j    j in 3..5: dR_0 = [e_j-3]x R_0 (rotation about a WORLD axis); j >= 6: dq_(j-5) = 1; j < 3 moves o itself and nothing measured from it:
//            those three columns are written as zeros without any work, as are a fixed base's six
//     gv_j   d gv_j = 1                udot_j   d udot_j = 1 (the armature enters here only)
// A joint direction reaches the bodies of its subtree only: the other lanes publish zeros without walking.  The tree is looked up once: the
// ancestor table goes to LDS as bytes, and a lane keeps two 64-bit masks - its ancestors (is a direction's joint among them?) and its subtree.
//   (0) every lane leaves sin / cos of its joint angle in LDS: the walks of all directions read them instead of calling sincosf again;
//   (1) primal: net wrench (f_i, n_i about o) to LDS, barrier, the sum over the subtree in ascending body order; the lane keeps F_i, N_i - s_i x F_i, a_i, s_i;
//   (2) per direction: the lane walks its chain in Dual, publishes (df_i, dn_i) - 6 floats, double-buffered: ONE barrier per direction - and keeps
//       da_i, ds_i; after the barrier the same sum gives (dF_i, dN_i) and
//           revolute  d tau_i = da_i . (N_i - s_i x F_i) + a_i . (dN_i - ds_i x F_i - s_i x dF_i)      prismatic  d tau_i = da_i . F_i + a_i . dF_i
//       (+ armature_i for udot's own direction); the base lane's six rows are dF_0 and dN_0 - ds_0 x F_0 - s_0 x dF_0;
//   (3) results gather in LDS for a chunk of CH directions, CH = min(nv, 6144 / (epb nv)) - whole rows for the shipped models - and all lanes sweep
//       them out, consecutive lanes writing consecutive floats.  A NULL output skips its directions altogether.
// The forward derivatives are a composition on the world's stream: aba_kernel for udot*, tangent_kernel at udot* writing MINUS its columns as the
// right-hand sides [N, C, nv] rsb_apply_inverse_mass reads (and the identity for M^-1), solve_kernel in place, a transposing copy to the outputs.
// udot* and the right-hand sides live in the world's query buffer.
// No atomics; every sum has a fixed order; a result of env e depends on env e's rows alone: the same bits for any N, any subset of outputs, host or
// device buffers.
// Static LDS, sized for 64 bodies whatever the tree: tangent_kernel 52 992 B (model tables 7 936 + 4 096 of ancestors, sin / cos 2 048, two wrench buffers 14 336 with
// the odd pitch of 7 floats - a lane's ds_write lands on its own bank of the 32 -, the chunk's results 24 576).  Compiler's resource report
// (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): tangent_kernel 153 VGPRs, 0 AGPRs, 87 SGPRs, 0 B of scratch, no spills:
// an allocation of 160 registers and 52 992 B of LDS each allow three workgroups per CU (3 waves per SIMD) - neither is the tighter limit;
// identity_kernel 10 and transpose_kernel 11 VGPRs, no LDS, no scratch.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kRec = 7;        // per lane and direction: df 0-2, dn about o 3-5 (odd pitch)
constexpr int kRes = 6144;     // floats of a chunk's results: CH directions of the block's epb * nv rows
enum Kind { kQ = 0, kV = 1, kA = 2, kPrimal = 3 };

struct Dual { float v, d; };      // a value and its derivative along the current direction
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator+(Dual a, float b) { return {a.v + b, a.d}; }
__device__ __forceinline__ Dual operator+(float a, Dual b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, float b) { return {a.v - b, a.d}; }
__device__ __forceinline__ Dual operator-(float a, Dual b) { return {a - b.v, -b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, float b) { return {a.v * b, a.d * b}; }
__device__ __forceinline__ Dual operator*(float a, Dual b) { return {a * b.v, a * b.d}; }

template <class T> __device__ __forceinline__ T make(float v, float d);
template <> __device__ __forceinline__ float make<float>(float v, float) { return v; }
template <> __device__ __forceinline__ Dual make<Dual>(float v, float d) { return {v, d}; }

// frames_chain.h's small products over any mix of float and Dual
template <class A, class B> using Prod = decltype(A{} * B{});
template <class A, class B> __device__ __forceinline__ void xcross(const A* a, const B* b, Prod<A, B>* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
template <class A, class B> __device__ __forceinline__ void xmat_vec(const A* M, const B* x, Prod<A, B>* o) {
  for (int r = 0; r < 3; ++r) o[r] = M[3 * r] * x[0] + M[3 * r + 1] * x[1] + M[3 * r + 2] * x[2];
}
template <class A, class B> __device__ __forceinline__ void xmatt_vec(const A* M, const B* x, Prod<A, B>* o) {
  for (int c = 0; c < 3; ++c) o[c] = M[c] * x[0] + M[3 + c] * x[1] + M[6 + c] * x[2];
}
template <class A, class B> __device__ __forceinline__ void xmat_mul(const A* X, const B* Y, Prod<A, B>* O) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O[3 * r + c] = X[3 * r] * Y[c] + X[3 * r + 1] * Y[3 + c] + X[3 * r + 2] * Y[6 + c];
}
template <class B> __device__ __forceinline__ void xsym_vec(const float* I, const B* x, B* o) {
  o[0] = I[0] * x[0] + I[1] * x[1] + I[2] * x[2];
  o[1] = I[1] * x[0] + I[3] * x[1] + I[4] * x[2];
  o[2] = I[2] * x[0] + I[4] * x[1] + I[5] * x[2];
}

// a body at the end of its chain walk: world rotation, position FROM THE BASE ORIGIN o, angular velocity, angular and classical linear acceleration,
// its joint's axis in the world and type (0 base, 1 revolute, 2 prismatic).  G, V, A: the scalars of the geometry, the velocities and the
// accelerations.  A direction of x varies all three (Dual, Dual, Dual), one of gv leaves the geometry alone (float, Dual, Dual), one of udot the
// velocities too (float, float, Dual); the primal pass is (float, float, float).  What is float costs one multiply, not three.
template <class G, class V, class A> struct Body { G R[9], p[3], a[3]; V w[3]; A al[3], ac[3]; int type; };
__device__ __forceinline__ float tangent(float) { return 0.f; }
__device__ __forceinline__ float tangent(Dual a) { return a.d; }

// walk_chain's recursion (frames_chain.h) over these scalars.  sc: the env's (sin q_i, cos q_i) pairs by body; anc: the body's row of the ancestor
// table in LDS, lv its level.  The direction (kind, j) seeds the tangents of the Dual ones (kPrimal: none).  A fixed base (moves = false) neither
// moves nor accelerates: its rows of u and ud are not read.
template <class G, class V, class A>
__device__ __forceinline__ void walk(const float* rows, const float* sc, const signed char* anc, int lv, bool moves, const float* q, const float* u, const float* ud,
                                     int kind, int j, Body<G, V, A>& c) {
  {
    float w = q[3], x = q[4], y = q[5], z = q[6];
    const float in = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    w *= in; x *= in; y *= in; z *= in;
    const float R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z),     2 * (x * z + w * y),
                        2 * (x * y + w * z),     1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y),     2 * (y * z + w * x),     1 - 2 * (x * x + y * y)};
    const int e = (kind == kQ && j >= 3 && j < 6) ? j - 3 : -1;      // dR = [e]x R: the base turns about world axis e
    for (int k = 0; k < 3; ++k) {
      c.R[k] = make<G>(R[k], e == 1 ? R[6 + k] : e == 2 ? -R[3 + k] : 0.f);
      c.R[3 + k] = make<G>(R[3 + k], e == 0 ? -R[6 + k] : e == 2 ? R[k] : 0.f);
      c.R[6 + k] = make<G>(R[6 + k], e == 0 ? R[3 + k] : e == 1 ? -R[k] : 0.f);
    }
    for (int k = 0; k < 3; ++k) {
      c.p[k] = make<G>(0.f, 0.f);
      c.w[k] = make<V>(moves ? u[3 + k] : 0.f, (moves && kind == kV && j == 3 + k) ? 1.f : 0.f);
      c.ac[k] = make<A>((moves && ud) ? ud[k] : 0.f, (moves && kind == kA && j == k) ? 1.f : 0.f);
      c.al[k] = make<A>((moves && ud) ? ud[3 + k] : 0.f, (moves && kind == kA && j == 3 + k) ? 1.f : 0.f);
      c.a[k] = make<G>(0.f, 0.f);
    }
    c.type = 0;
  }
  for (int l = 1; l <= lv; ++l) {
    const int i = anc[l];
    const float* row = rows + i * kRow;
    const bool revolute = __float_as_int(row[3]) == RSB_JOINT_REVOLUTE;
    const float ax[3] = {row[0], row[1], row[2]}, pt[3] = {row[4], row[5], row[6]};
    const float own = (j == 5 + i) ? 1.f : 0.f;
    const G qi = make<G>(q[6 + i], kind == kQ ? own : 0.f);
    const V qd = make<V>(u[5 + i], kind == kV ? own : 0.f);
    const A qdd = make<A>(ud ? ud[5 + i] : 0.f, kind == kA ? own : 0.f);
    G Rn[9], d[3], a[3];
    if (revolute) {
      const float s0 = sc[2 * i], c0 = sc[2 * i + 1], dq = kind == kQ ? own : 0.f;
      const G sn = make<G>(s0, c0 * dq), cs = make<G>(c0, -s0 * dq), t = 1.f - cs;
      G Rq[9], E[9];
      Rq[0] = cs + (ax[0] * ax[0]) * t;         Rq[1] = (ax[0] * ax[1]) * t - ax[2] * sn; Rq[2] = (ax[0] * ax[2]) * t + ax[1] * sn;
      Rq[3] = (ax[1] * ax[0]) * t + ax[2] * sn; Rq[4] = cs + (ax[1] * ax[1]) * t;         Rq[5] = (ax[1] * ax[2]) * t - ax[0] * sn;
      Rq[6] = (ax[2] * ax[0]) * t - ax[1] * sn; Rq[7] = (ax[2] * ax[1]) * t + ax[0] * sn; Rq[8] = cs + (ax[2] * ax[2]) * t;
      xmat_mul(row + 8, Rq, E);
      xmat_mul(c.R, E, Rn);
    } else {
      xmat_mul(c.R, row + 8, Rn);
    }
    xmat_vec(c.R, pt, d);
    xmat_vec(Rn, ax, a);
    if (!revolute) for (int k = 0; k < 3; ++k) d[k] = d[k] + a[k] * qi;
    V wd[3], wa[3], wwd[3];
    A ad[3];
    xcross(c.w, d, wd);
    xcross(c.w, a, wa);
    xcross(c.al, d, ad);
    xcross(c.w, wd, wwd);
    for (int k = 0; k < 3; ++k) {
      c.ac[k] = c.ac[k] + (ad[k] + wwd[k]);
      if (revolute) {
        c.al[k] = c.al[k] + (a[k] * qdd + wa[k] * qd);
        c.w[k] = c.w[k] + a[k] * qd;
      } else {
        c.ac[k] = c.ac[k] + (a[k] * qdd + 2.f * (wa[k] * qd));
      }
      c.p[k] = c.p[k] + d[k];
      c.a[k] = a[k];
    }
    for (int k = 0; k < 9; ++k) c.R[k] = Rn[k];
    c.type = revolute ? 1 : 2;
  }
}

// external loads: F frames with world force / torque [N,F,3] (either may be null), held fixed; a load's point is fixed on its body
struct ExtLoads { const float* force; const float* torque; int F; };

// the body's own net wrench about o (rnea_kernel's step 1):  f = m (acc_c - g) - external,  n = I_w alpha + omega x I_w omega + r x m (acc_c - g) - external
template <class G, class V, class A>
__device__ __forceinline__ void net_wrench(const float* rows, const float* xtra, const ExtLoads& L, const FrameList& frames, long long env, int body,
                                           const Body<G, V, A>& b, const float* g, A* f, A* n) {
  const float* x = xtra + body * kXtra;
  const float mass = rows[body * kRow + 7];
  G rc[3], r[3];
  V t1[3], t2[3], wb[3], Iwb[3], Iw[3], wIw[3];
  A t0[3], acom[3], fi[3], ab[3], Iab[3], Ia[3], rf[3];
  xmat_vec(b.R, x, rc);
  for (int k = 0; k < 3; ++k) r[k] = b.p[k] + rc[k];
  xcross(b.al, rc, t0);
  xcross(b.w, rc, t1);
  xcross(b.w, t1, t2);
  for (int k = 0; k < 3; ++k) { acom[k] = (b.ac[k] + t0[k]) + t2[k]; fi[k] = mass * (acom[k] - g[k]); }
  xmatt_vec(b.R, b.w, wb);
  xsym_vec(x + 3, wb, Iwb);
  xmat_vec(b.R, Iwb, Iw);
  xmatt_vec(b.R, b.al, ab);
  xsym_vec(x + 3, ab, Iab);
  xmat_vec(b.R, Iab, Ia);
  xcross(b.w, Iw, wIw);
  xcross(r, fi, rf);
  for (int k = 0; k < 3; ++k) { f[k] = fi[k]; n[k] = (Ia[k] + wIw[k]) + rf[k]; }
  for (int k = 0; k < L.F; ++k) {
    if (frames.f[k].body != body) continue;
    const float off[3] = {frames.f[k].offset[0], frames.f[k].offset[1], frames.f[k].offset[2]};
    const size_t at = ((size_t)env * L.F + k) * 3;
    float fo[3], to[3];
    for (int c = 0; c < 3; ++c) { fo[c] = L.force ? L.force[at + c] : 0.f; to[c] = L.torque ? L.torque[at + c] : 0.f; }
    G ro[3], rl[3], rlf[3];
    xmat_vec(b.R, off, ro);
    for (int c = 0; c < 3; ++c) rl[c] = b.p[c] + ro[c];
    xcross(rl, fo, rlf);
    for (int c = 0; c < 3; ++c) { f[c] = f[c] - fo[c]; n[c] = n[c] - (rlf[c] + to[c]); }
  }
}

// one direction for one lane: the tangents of the body's net wrench to s[0..5], those of its joint's axis and position to da, ds
template <class G, class V>
__device__ __forceinline__ void direction(const float* rows, const float* xtra, const float* sc, const signed char* anc, int lv, bool moves, const float* q, const float* u,
                                          const float* ud, const ExtLoads& L, const FrameList& frames, long long env, int body, int kind, int j, const float* g, float* s,
                                          float* da, float* ds) {
  Body<G, V, Dual> b;
  walk(rows, sc, anc, lv, moves, q, u, ud, kind, j, b);
  Dual f[3], n[3];
  net_wrench(rows, xtra, L, frames, env, body, b, g, f, n);
  for (int k = 0; k < 3; ++k) { s[k] = f[k].d; s[3 + k] = n[k].d; da[k] = tangent(b.a[k]); ds[k] = tangent(b.p[k]); }
}

// acc[0, 6) = the records of the bodies in `sub` (bit i: body i; none below `body`), kRec floats apart, in ascending body order: subtree_sum
// (frames_chain.h) with the subtree's membership looked up once
__device__ __forceinline__ void masked_sum(unsigned long long sub, int body, int nb, const float* recs, float* acc) {
  for (int k = 0; k < 6; ++k) acc[k] = 0.f;
  for (int i = body; i < nb; ++i) {
    if (!((sub >> i) & 1ull)) continue;
    for (int k = 0; k < 6; ++k) acc[k] += recs[i * kRec + k];
  }
}

// where a launch's matrices go.  m[kind] (null: not asked for) holds, `pitch` floats per env, entry (row i, direction j) at i * nv + j, or with
// `transposed` at j * nv + i (one right-hand side of rsb_apply_inverse_mass per direction); every value is multiplied by `sign`
struct Out { float* m[3]; long long pitch; int transposed; float sign; };

__global__ __launch_bounds__(kThreads) void tangent_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const float* __restrict__ gv,
                                                           const float* __restrict__ udot, const FrameList frames, const ExtLoads loads, int N, const Vec3 g, const Out out) {
  __shared__ float rows[RSB_MAX_BODIES * kRow];
  __shared__ float xtra[RSB_MAX_BODIES * kXtra];
  __shared__ float sct[kThreads * 2];
  __shared__ signed char ancl[RSB_MAX_BODIES * RSB_MAX_BODIES];      // DevModel::anc (-1 .. 63): every direction's walk reads its chain here
  __shared__ float trec[2 * kThreads * kRec];
  __shared__ float resd[kRes];
  const DevModel& m = *model;
  stage_rows(m, rows);
  stage_xtra(m, xtra);
  const int nb = m.nb, depth = m.depth, nv = m.nv;
  const bool fixed = m.fixed_base != 0;
  for (int k = threadIdx.x; k < nb * depth; k += kThreads) ancl[k] = (signed char)m.anc[k];
  const auto [env0, here, el, body] = env_block(nb, N);
  const bool active = el < here;
  const long long env = env0 + el;
  const float* q = gc + (size_t)(active ? env : 0) * m.nq;
  const float* u = gv + (size_t)(active ? env : 0) * nv;
  const float* ud = udot ? udot + (size_t)(active ? env : 0) * nv : nullptr;
  const float* sc = sct + el * nb * 2;
  const float gvec[3] = {g.x, g.y, g.z};
  if (active) {
    float sn = 0.f, cs = 1.f;
    if (body > 0) sincosf(q[6 + body], &sn, &cs);
    sct[threadIdx.x * 2] = sn; sct[threadIdx.x * 2 + 1] = cs;
  }
  __syncthreads();
  const int level = active ? m.level[body] : 0;
  const signed char* anc = ancl + (active ? body : 0) * depth;
  unsigned long long sub = 0, up = 0;      // the bodies of this lane's subtree; its ancestors and itself
  if (active) {
    for (int i = body; i < nb; ++i) sub |= (unsigned long long)(ancl[i * depth + level] == body) << i;
    for (int l = 0; l <= level; ++l) up |= 1ull << anc[l];
  }
  // ---- primal: what rnea_kernel computes; the lane keeps its joint's carried wrench
  float F[3] = {0.f, 0.f, 0.f}, nj[3] = {0.f, 0.f, 0.f}, pa[3] = {0.f, 0.f, 0.f}, ps[3] = {0.f, 0.f, 0.f};
  int type = 0;
  if (active) {
    Body<float, float, float> b;
    walk(rows, sc, anc, level, !fixed, q, u, ud, kPrimal, -1, b);
    float f[3], n[3];
    net_wrench(rows, xtra, loads, frames, env, body, b, gvec, f, n);
    float* s = trec + threadIdx.x * kRec;
    for (int k = 0; k < 3; ++k) { s[k] = f[k]; s[3 + k] = n[k]; pa[k] = b.a[k]; ps[k] = b.p[k]; }
    type = b.type;
  }
  __syncthreads();
  if (active) {
    float acc[6], sf[3];
    masked_sum(sub, body, nb, trec + el * nb * kRec, acc);
    cross3(ps, acc, sf);
    for (int k = 0; k < 3; ++k) { F[k] = acc[k]; nj[k] = acc[3 + k] - sf[k]; }
  }
  const float arm = active ? xtra[body * kXtra + 9] : 0.f;
  const int epb = kThreads / nb;
  const int CH = min(nv, kRes / (epb * nv));
  unsigned turn = 1;      // directions walked so far + 1: the primal pass used buffer 0
  for (int kind = 0; kind < 3; ++kind) {
    float* dst = out.m[kind];
    if (!dst) continue;
    const int jfirst = fixed ? 6 : (kind == kQ ? 3 : 0);
    for (int j0 = 0; j0 < nv; j0 += CH) {
      const int cur = min(CH, nv - j0);
      for (int jj = 0; jj < cur; ++jj) {
        const int j = j0 + jj;
        float r[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // body 0: the six base rows; another body: r[0] its joint's row
        if (j >= jfirst) {      // (uniform over the workgroup)
          float* tr = trec + (turn & 1u) * (kThreads * kRec);
          ++turn;
          float da[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f};
          if (active) {
            float* s = tr + threadIdx.x * kRec;
            if (j < 6 || ((up >> (j - 5)) & 1ull)) {      // a base direction reaches every body, a joint's its subtree; kind is uniform
              if (kind == kQ) direction<Dual, Dual>(rows, xtra, sc, anc, level, !fixed, q, u, ud, loads, frames, env, body, kind, j, gvec, s, da, ds);
              else if (kind == kV) direction<float, Dual>(rows, xtra, sc, anc, level, !fixed, q, u, ud, loads, frames, env, body, kind, j, gvec, s, da, ds);
              else direction<float, float>(rows, xtra, sc, anc, level, !fixed, q, u, ud, loads, frames, env, body, kind, j, gvec, s, da, ds);
            } else {
              for (int k = 0; k < 6; ++k) s[k] = 0.f;
            }
          }
          __syncthreads();
          if (active) {
            float dacc[6], t0[3], t1[3], dnj[3];
            masked_sum(sub, body, nb, tr + el * nb * kRec, dacc);
            cross3(ds, F, t0);
            cross3(ps, dacc, t1);
            for (int k = 0; k < 3; ++k) dnj[k] = dacc[3 + k] - (t0[k] + t1[k]);
            if (body == 0) {
              for (int k = 0; k < 3; ++k) { r[k] = dacc[k]; r[3 + k] = dnj[k]; }
            } else {
              const float along = type == 1 ? dot3(da, nj) + dot3(pa, dnj) : dot3(da, F) + dot3(pa, dacc);
              r[0] = along + ((kind == kA && j == 5 + body) ? arm : 0.f);
            }
          }
        }
        if (active) {
          if (body == 0) {
            for (int k = 0; k < 6; ++k) resd[out.transposed ? (el * cur + jj) * nv + k : (el * nv + k) * cur + jj] = r[k];
          } else {
            resd[out.transposed ? (el * cur + jj) * nv + 5 + body : (el * nv + 5 + body) * cur + jj] = r[0];
          }
        }
      }
      __syncthreads();
      float* o = dst + (size_t)env0 * out.pitch;
      const int per = nv * cur;
      for (int e = threadIdx.x; e < here * per; e += kThreads) {
        const int k = e / per, rem = e - k * per;
        int row, jj;
        if (out.transposed) { jj = rem / nv; row = rem - jj * nv; } else { row = rem / cur; jj = rem - row * cur; }
        const size_t at = (size_t)k * out.pitch + (out.transposed ? (size_t)(j0 + jj) * nv + row : (size_t)row * nv + j0 + jj);
        o[at] = out.sign * resd[e];
      }
      __syncthreads();
    }
  }
}

// B[e, slot nv + j, i] = (i == j): the right-hand sides of M^-1 itself
__global__ __launch_bounds__(kThreads) void identity_kernel(float* __restrict__ B, long long total, int nv, int C, int slot) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long long e = t / (nv * nv);
  const int rem = (int)(t - e * (nv * nv)), j = rem / nv, i = rem - j * nv;
  B[((size_t)e * C + (size_t)slot * nv + j) * nv + i] = i == j ? 1.f : 0.f;
}

// out[e, i, j] = X[e, slot nv + j, i]: a solved column becomes a column
__global__ __launch_bounds__(kThreads) void transpose_kernel(const float* __restrict__ X, long long total, int nv, int C, int slot, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long long e = t / (nv * nv);
  const int rem = (int)(t - e * (nv * nv)), i = rem / nv, j = rem - i * nv;
  out[t] = X[((size_t)e * C + (size_t)slot * nv + j) * nv + i];
}

int check_args(rsb_world* w, const char* who, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags, bool any_output, int space) {
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!any_output) return invalid(who, "every output is NULL");
  if (flags != 0) return invalid(who, "flags must be 0 (no derivatives with RSB_DYN_CONTACTS)");
  return check_dynamics_loads(w, who, frames, n_frames, force, torque, 0);
}

void launch_tangent(rsb_world* w, hipStream_t s, const float* dud, const rsb_frame* frames, int n_frames, const float* df, const float* dq, const Out& out) {
  hipLaunchKernelGGL(tangent_kernel, dim3(env_blocks(w)), dim3(kThreads), 0, s, (const DevModel*)w->d_model, (const float*)w->d_gc, (const float*)w->d_gv, dud,
                     n_frames ? frame_list(frames, n_frames) : FrameList{}, ExtLoads{df, dq, n_frames}, w->N, gravity_of(w), out);
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_inverse_dynamics_derivatives(rsb_world* w, const float* udot, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags,
                                     float* dtau_dq, float* dtau_dv, float* dtau_dudot, int space) {
  const char* who = "rsb_inverse_dynamics_derivatives";
  int st = check_args(w, who, frames, n_frames, force, torque, flags, dtau_dq || dtau_dv || dtau_dudot, space); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = (size_t)w->N, nv = (size_t)w->blob.nv, lf = N * (size_t)n_frames * 3;
  const float *dud, *df, *dt;
  float *oq, *ov, *oa;
  Staged io(w, space);      // [udot | force | torque | outputs]
  io.in(dud, udot, N * nv); io.in(df, n_frames ? force : nullptr, lf); io.in(dt, n_frames ? torque : nullptr, lf);
  io.out(oq, dtau_dq, N * nv * nv); io.out(ov, dtau_dv, N * nv * nv); io.out(oa, dtau_dudot, N * nv * nv);
  st = io.begin(); if (st != RSB_OK) return st;
  launch_tangent(w, stream_of(w), dud, frames, n_frames, df, dt, Out{{oq, ov, oa}, (long long)(nv * nv), 0, 1.f});
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_forward_dynamics_derivatives(rsb_world* w, const float* tau, const rsb_frame* frames, int n_frames, const float* force, const float* torque, int flags,
                                     float* udot, float* dudot_dq, float* dudot_dv, float* dudot_dtau, int space) {
  const char* who = "rsb_forward_dynamics_derivatives";
  int st = check_args(w, who, frames, n_frames, force, torque, flags, udot || dudot_dq || dudot_dv || dudot_dtau, space); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = (size_t)w->N, nv = (size_t)w->blob.nv, lf = N * (size_t)n_frames * 3, nn = N * nv * nv;
  const int sq = dudot_dq ? 0 : -1, sv = dudot_dv ? (sq + 1) : -1, sm = dudot_dtau ? (dudot_dq ? 1 : 0) + (dudot_dv ? 1 : 0) : -1;      // the matrices' slots among the columns
  const int slots = (dudot_dq ? 1 : 0) + (dudot_dv ? 1 : 0) + (dudot_dtau ? 1 : 0), C = slots * (int)nv;
  const float *dtau, *df, *dt;
  float *dud, *oq, *ov, *om, *work;
  Staged io(w, space);      // [udot* | right-hand sides | tau | force | torque | outputs]
  io.in(dtau, tau, N * nv); io.in(df, n_frames ? force : nullptr, lf); io.in(dt, n_frames ? torque : nullptr, lf);
  io.out(dud, udot, N * nv); io.out(oq, dudot_dq, nn); io.out(ov, dudot_dv, nn); io.out(om, dudot_dtau, nn);
  io.scratch(work, N * nv + (size_t)slots * nn);
  st = io.begin(); if (st != RSB_OK) return st;
  hipStream_t s = stream_of(w);
  float* ustar = dud ? dud : work;      // udot* = FD(q, gv, tau, loads)
  float* B = work + N * nv;
  st = launch_forward_dynamics(w, s, dtau, frames, n_frames, df, dt, 0, ustar); if (st != RSB_OK) return st;
  if (slots) {
    if (oq || ov) {
      const size_t one = nv * nv;
      launch_tangent(w, s, ustar, frames, n_frames, df, dt, Out{{oq ? B + sq * one : nullptr, ov ? B + sv * one : nullptr, nullptr}, (long long)C * (long long)nv, 1, -1.f});
      HIP_TRY(hipGetLastError());
    }
    if (om) {
      hipLaunchKernelGGL(identity_kernel, dim3(blocks_for(nn)), dim3(kThreads), 0, s, B, (long long)nn, (int)nv, C, sm);
      HIP_TRY(hipGetLastError());
    }
    st = launch_inverse_mass_solve(w, s, C, B, B); if (st != RSB_OK) return st;
    float* outs[3] = {oq, ov, om};
    const int slot_of[3] = {sq, sv, sm};
    for (int k = 0; k < 3; ++k) {
      if (!outs[k]) continue;
      hipLaunchKernelGGL(transpose_kernel, dim3(blocks_for(nn)), dim3(kThreads), 0, s, (const float*)B, (long long)nn, (int)nv, C, slot_of[k], outs[k]);
      HIP_TRY(hipGetLastError());
    }
  }
  return io.end();
}

}  // extern "C"
