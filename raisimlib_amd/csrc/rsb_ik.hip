// rsb_ik.hip — batched inverse kinematics at chosen frames (rsb_inverse_kinematics; include/rsb.h, where the iteration is stated step by step).
//
//   e = target - frame(q)          (J J^T + rho I) y = e          dq = J^T y, clipped to max_step          q <- q (+) dq          rho = damping * max_i (J J^T)_ii
// a damped Gauss-Newton (Levenberg-Marquardt) iteration on a configuration that lives in LDS from the first pass to the last: ONE kernel, ik_kernel,
// on the world's stream.  It reads gc (or gc_init) once and writes its outputs once; the world is not touched.
//
// ik_kernel.  m = kF rows is uniform over the launch.  An env gets a group of g lanes of ONE wave (16 / 32 / 64 by m, the rule of held_solve_kernel,
// rsb_constrained.hip; above 64 rows lane l also owns row l + 64); a workgroup takes epw = min(256 / g, what fits in LDS) consecutive envs and has
// epw * g threads.  Dynamic LDS: [model rows nb * kRow | joint limits 2 nb | chain masks, alive words, pivot flags | frames, mask | epw env records], an env record
// being  q [nq] | joint records 7 nb | frame heads 8 F | J [m][nv | 1] | the column-packed factor m (m + 1) / 2 | 1 / D [m] | the row vector [m] | dq [nv].
// The joint records - (a_i, p_i, revolute) of frame_jacobians_kernel's phase 1 (rsb_frames.hip) - are kept per BODY, not per frame: the frames of
// an env share their ancestors, the record of a body does not depend on which frame's walk leaves it (two walks store the same bits), and the
// record of an env then has one size whatever the tree's depth.  Which bodies carry frame f is a 64-bit mask per frame, built once per workgroup.
// The frames and the mask are kernel arguments by value; they are copied to LDS once, because a lane's own index into the argument segment
// costs a chain of selects over scalar registers in every pass.
// The largest case (m = 96, nv = 69, nb = 64) is 13 795 floats, one env per workgroup; the quadruped's four feet (m = 12, nv = 18) are 491 floats
// per env, sixteen envs per workgroup.  Rows of J have an odd pitch: the lanes of the product J J^T read one column of different rows.
// One pass of the loop, every step between two plain barriers (all trip counts are workgroup-uniform):
//   (1) lanes f < F walk their chains with walk_chain on the q in LDS and leave the joint records, the frame's point and the rows of e;
//   (2) every lane of the group reads e in row order: err_pos, err_rot, converged or out of steps - the same decision in every lane, in registers;
//       the groups' alive words are OR-ed by every thread: the loop ends when no env of the workgroup is running;
//   (3) the lanes fill J (masked columns zero) and the lower triangle of A = J J^T, sums over the columns in ascending order; rho; the root-free
//       Cholesky with the pivot rule of held_solve_kernel, the two substitutions (the routines are a copy of that kernel's: its own stay as they are);
//   (4) dq = J^T y in row order, its largest entry, the clip, and q (+) dq on the free coordinates only: a held coordinate's word in LDS is never
//       written.  The base quaternion is lane 0's: exp(dq[3:6]) times the normalised quaternion, normalised again.
// An env that has stopped keeps its lanes idle through the barriers.  No atomics, every sum in a fixed order, nothing of another env is read: the
// same bits for any N, any neighbours, any subset of outputs.  Everything is float.
#include "frames_chain.h"
#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kIkLdsFloats = 15872;   // dynamic LDS of a workgroup, in floats (62 KB of the 64 KB a workgroup may have)
constexpr int kIkGroups = 16;         // at most 256 / 16 envs per workgroup
constexpr int kIkRec = 7;             // per body: a 0-2, p 3-5, revolute 6
constexpr int kIkHead = 8;            // per frame: point 0-2, base position 3-5

struct IkFrames { rsb_frame f[RSB_MAX_IK_FRAMES]; };      // kernel arguments: the frames and the mask travel with the launch
struct IkMask { uint8_t free[RSB_MAX_DOF + 3]; };
struct IkLayout { int q, rec, head, J, jp, W, iD, x, dq, pitch; };      // offsets into an env record, floats

__host__ __device__ inline int ik_group(int m) { return m <= 16 ? 16 : m <= 32 ? 32 : 64; }
constexpr int kIkMaskWords = RSB_MAX_DOF + 3;
// floats ahead of the env records: model rows, joint limits, chain masks, alive words and pivot flags, the frames, the mask
__host__ __device__ inline int ik_shared(int nb) { return nb * kRow + 2 * nb + 2 * RSB_MAX_IK_FRAMES + 2 * kIkGroups + 4 * RSB_MAX_IK_FRAMES + kIkMaskWords; }
__host__ __device__ inline IkLayout ik_layout(int m, int nv, int nq, int nb, int F) {
  IkLayout L;
  L.q = 0; L.rec = L.q + nq; L.head = L.rec + nb * kIkRec; L.J = L.head + F * kIkHead; L.jp = nv | 1;
  L.W = L.J + m * L.jp; L.iD = L.W + m * (m + 1) / 2; L.x = L.iD + m; L.dq = L.x + m; L.pitch = (L.dq + nv) | 1;
  return L;
}
__host__ __device__ inline int ik_envs(int m, int nv, int nq, int nb, int F) {
  const int a = kThreads / ik_group(m), b = (kIkLdsFloats - ik_shared(nb)) / ik_layout(m, nv, nq, nb, F).pitch;
  return a < b ? a : b;
}

__global__ __launch_bounds__(kThreads) void ik_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc0, const IkFrames frames, int F, int N, int kk,
                                                      int limits, const IkMask mask, const rsb_ik_options opt, const float* __restrict__ tpos,
                                                      const float* __restrict__ trot, float* __restrict__ gc_out, float* __restrict__ error,
                                                      int32_t* __restrict__ iterations, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DevModel& M = *model;
  const int nb = M.nb, nq = M.nq, nv = M.nv, depth = M.depth;
  const int m = kk * F, g = ik_group(m), epw = blockDim.x / g;
  const IkLayout L = ik_layout(m, nv, nq, nb, F);
  float* rows = lds;
  float* lim = rows + nb * kRow;
  unsigned* cmask = reinterpret_cast<unsigned*>(lim + 2 * nb);
  int* alive = reinterpret_cast<int*>(cmask + 2 * RSB_MAX_IK_FRAMES);
  int* flag = alive + kIkGroups;
  const int el = threadIdx.x / g, lane = threadIdx.x - el * g;
  const long long env = (long long)blockIdx.x * epw + el;
  const bool active = env < N;
  float* frl = reinterpret_cast<float*>(flag + kIkGroups);      // body (int bits), offset: the arguments' copies, read with a lane's own index
  int* free_ = reinterpret_cast<int*>(frl + 4 * RSB_MAX_IK_FRAMES);
  float* E = reinterpret_cast<float*>(free_ + kIkMaskWords) + el * L.pitch;
  float *q = E + L.q, *rec = E + L.rec, *head = E + L.head, *J = E + L.J, *W = E + L.W, *iD = E + L.iD, *x = E + L.x, *dq = E + L.dq;
  const int jp = L.jp;
  auto col = [m](int k) { return k * m - k * (k - 1) / 2 - k; };      // entry (i, k), i >= k, of the column-packed factor at col(k) + i
  // ---- once per workgroup: the model rows, the joint limits, the bodies that carry each frame; once per env: q and the targets
  for (int k = threadIdx.x; k < nb * kRow; k += blockDim.x) {
    const int b = k / kRow, c = k - b * kRow;
    rows[k] = c < kRowUsed ? M.bodyf[b][c] : 0.f;
  }
  for (int k = threadIdx.x; k < nb; k += blockDim.x) { lim[2 * k] = M.bodyf[k][29]; lim[2 * k + 1] = M.bodyf[k][30]; }
  if ((int)threadIdx.x < F) {
    const int b = frames.f[threadIdx.x].body, lv = M.level[b];
    unsigned lo = 0, hi = 0;
    for (int l = 1; l <= lv; ++l) {
      const int i = M.anc[b * depth + l];
      if (i < 32) lo |= 1u << i; else hi |= 1u << (i - 32);
    }
    cmask[2 * threadIdx.x] = lo; cmask[2 * threadIdx.x + 1] = hi;
    frl[4 * threadIdx.x] = __int_as_float(b);
    for (int k = 0; k < 3; ++k) frl[4 * threadIdx.x + 1 + k] = frames.f[threadIdx.x].offset[k];
  }
  for (int k = threadIdx.x; k < nv; k += blockDim.x) free_[k] = mask.free[k];
  float tp[3] = {0, 0, 0}, tr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (active) {
    for (int k = lane; k < nq; k += g) q[k] = gc0[(size_t)env * nq + k];
    if (lane < F) {
      const size_t at = (size_t)env * F + lane;
      for (int k = 0; k < 3; ++k) tp[k] = tpos[at * 3 + k];
      if (kk == 6) for (int k = 0; k < 9; ++k) tr[k] = trot[at * 9 + k];
    }
  }
  bool live = active;
  int st = RSB_IK_CONVERGED, iters = 0;
  float ep = 0.f, er = 0.f;
  __syncthreads();
  const bool free_rot = (free_[3] | free_[4] | free_[5]) != 0;
  int my_body = 0;
  float my_off[3] = {0, 0, 0};
  if (lane < F) { my_body = __float_as_int(frl[4 * lane]); for (int k = 0; k < 3; ++k) my_off[k] = frl[4 * lane + 1 + k]; }
  for (int it = 0;; ++it) {
    // ---- (1) the rows at q
    if (live && lane < F) {
      Chain c;
      walk_chain<false>(M, rows, q, nullptr, nullptr, false, my_body, c, [rec](int, int i, const float* a, const float* p, bool revolute) {
        float* s = rec + i * kIkRec;
        for (int k = 0; k < 3; ++k) { s[k] = a[k]; s[3 + k] = p[k]; }
        s[6] = revolute ? 1.f : 0.f;
      });
      float o[3];
      mat3_vec(c.R, my_off, o);
      float* h = head + lane * kIkHead;
      for (int k = 0; k < 3; ++k) {
        const float pt = c.p[k] + o[k];
        h[k] = pt; h[3 + k] = q[k];
        x[kk * lane + k] = tp[k] - pt;
      }
      if (kk == 6) {      // the rotation vector of S = R_t R^T
        float S[9];
        for (int r = 0; r < 3; ++r)
          for (int s = 0; s < 3; ++s) S[3 * r + s] = tr[3 * r] * c.R[3 * s] + tr[3 * r + 1] * c.R[3 * s + 1] + tr[3 * r + 2] * c.R[3 * s + 2];
        const float v[3] = {0.5f * (S[7] - S[5]), 0.5f * (S[2] - S[6]), 0.5f * (S[3] - S[1])};
        const float cs = 0.5f * (S[0] + S[4] + S[8] - 1.f), n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const float k = n > 1e-6f ? atan2f(n, cs) / n : 1.f;
        for (int a = 0; a < 3; ++a) x[6 * lane + 3 + a] = v[a] * k;
      }
    }
    __syncthreads();
    // ---- (2) stop or go on: the same arithmetic in every lane of the group
    if (live) {
      bool ok = true;
      ep = 0.f; er = 0.f;
      for (int f = 0; f < F; ++f)
        for (int a = 0; a < kk; ++a) {
          const float v = fabsf(x[kk * f + a]);
          if (a < 3) { ep = fmaxf(ep, v); ok = ok && v <= opt.pos_tol; }
          else { er = fmaxf(er, v); ok = ok && v <= opt.rot_tol; }
        }
      iters = it;
      if (ok) { live = false; st = RSB_IK_CONVERGED; }
      else if (it == opt.max_iter) { live = false; st = RSB_IK_MAX_ITER; }
    }
    if (lane == 0) alive[el] = live ? 1 : 0;
    __syncthreads();
    int any = 0;
    for (int k = 0; k < epw; ++k) any |= alive[k];
    if (!any) break;      // (workgroup-uniform; at it == max_iter every env has stopped)
    // ---- (3) J, A = J J^T, the damped factorisation, y
    if (live) {
      if (lane == 0) flag[el] = 0;
      for (int e = lane; e < m * nv; e += g) {
        const int i = e / nv, d = e - i * nv, f = i / kk, a = i - f * kk;
        const bool rot = a >= 3;
        const int r = rot ? a - 3 : a, r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
        const float* h = head + f * kIkHead;
        float val = 0.f;
        if (free_[d]) {
          if (d < 3) {
            val = (!rot && d == r) ? 1.f : 0.f;
          } else if (d < 6) {                                                 // -[point - p_base]x | identity
            const int c = d - 3;
            if (rot) val = c == r ? 1.f : 0.f;
            else if (c == r1) val = h[r2] - h[3 + r2];
            else if (c == r2) val = -(h[r1] - h[3 + r1]);
          } else {
            const int j = d - 5;
            const unsigned bits = j < 32 ? cmask[2 * f] : cmask[2 * f + 1];
            if ((bits >> (j & 31)) & 1u) {                                    // body j carries the frame
              const float* s = rec + j * kIkRec;
              if (s[6] != 0.f) val = rot ? s[r] : s[r1] * (h[r2] - s[3 + r2]) - s[r2] * (h[r1] - s[3 + r1]);      // a | (a x (point - p_j))_r
              else val = rot ? 0.f : s[r];
            }
          }
        }
        J[i * jp + d] = val;
      }
    }
    __syncthreads();
    if (live)
      for (int i = lane; i < m; i += g)
        for (int k = 0; k <= i; ++k) {
          float s = 0.f;
          for (int d = 0; d < nv; ++d) s += J[i * jp + d] * J[k * jp + d];
          W[col(k) + i] = s;
          if (k == i) iD[i] = s;
        }
    __syncthreads();
    float d0[2] = {0, 0};
    if (live) {
      float gmax = iD[0];
      for (int i = 1; i < m; ++i) gmax = fmaxf(gmax, iD[i]);
      const float rho = opt.damping * gmax;
      for (int i = lane, r = 0; i < m; i += g, ++r) {
        d0[r] = W[col(i) + i] + rho;
        W[col(i) + i] = d0[r];
      }
      if (!(gmax > 0.f)) { live = false; st = RSB_IK_SINGULAR; }      // no free column reaches a row
    }
    __syncthreads();      // (iD is written again below)
    for (int j = 0; j < m; ++j) {
      if (live) {
        for (int i = lane, r = 0; i < m; i += g, ++r) {
          if (i < j) continue;
          float s = W[col(j) + i];
          for (int k = 0; k < j; ++k) s -= W[col(k) + i] * W[col(k) + j] * iD[k];
          W[col(j) + i] = s;
          if (i == j) {
            const bool bad = !(s > RSB_HELD_PIVOT_TOL * d0[r]) || !isfinite(s);
            if (bad) flag[el] = 1;
            iD[j] = bad ? 0.f : 1.f / s;
          }
        }
      }
      __syncthreads();
    }
    if (live && flag[el] != 0) { live = false; st = RSB_IK_SINGULAR; }
    for (int k = 0; k < m - 1; ++k) {
      if (live) {
        const float yk = x[k] * iD[k];
        for (int i = lane; i < m; i += g)
          if (i > k) x[i] -= W[col(k) + i] * yk;
      }
      __syncthreads();
    }
    if (live)
      for (int i = lane; i < m; i += g) x[i] *= iD[i];
    __syncthreads();
    for (int k = m - 1; k >= 1; --k) {
      if (live) {
        const float xk = x[k];
        for (int i = lane; i < m; i += g)
          if (i < k) x[i] -= W[col(i) + k] * iD[i] * xk;
      }
      __syncthreads();
    }
    // ---- (4) dq = J^T y, the clip, q (+) dq
    if (live)
      for (int d = lane; d < nv; d += g) {
        float acc = 0.f;
        for (int i = 0; i < m; ++i) acc += J[i * jp + d] * x[i];
        dq[d] = acc;
      }
    __syncthreads();
    if (live) {
      float s = 0.f;
      for (int d = 0; d < nv; ++d) s = fmaxf(s, fabsf(dq[d]));
      const float sc = s > opt.max_step ? opt.max_step / s : 1.f;
      for (int d = lane; d < nv; d += g) {
        if (!free_[d] || (d >= 3 && d < 6)) continue;
        const int k = d < 3 ? d : d + 1;
        float v = q[k] + dq[d] * sc;
        if (limits && d >= 6) v = fminf(fmaxf(v, lim[2 * (d - 5)]), lim[2 * (d - 5) + 1]);
        q[k] = v;
      }
      if (lane == 0 && free_rot) {      // exp(dq[3:6]) on the left of the normalised quaternion
        float w[3];
        for (int c = 0; c < 3; ++c) w[c] = free_[3 + c] ? dq[3 + c] * sc : 0.f;
        const float ph = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        float sh = 0.5f, ew = 1.f;
        if (ph > 1e-6f) { sh = sinf(0.5f * ph) / ph; ew = cosf(0.5f * ph); }
        const float ex = sh * w[0], ey = sh * w[1], ez = sh * w[2];
        float nw = q[3], nx = q[4], ny = q[5], nz = q[6];
        float in = 1.0f / sqrtf(nw * nw + nx * nx + ny * ny + nz * nz);
        nw *= in; nx *= in; ny *= in; nz *= in;
        float pw = ew * nw - ex * nx - ey * ny - ez * nz;
        float px = ew * nx + ex * nw + ey * nz - ez * ny;
        float py = ew * ny - ex * nz + ey * nw + ez * nx;
        float pz = ew * nz + ex * ny - ey * nx + ez * nw;
        in = 1.0f / sqrtf(pw * pw + px * px + py * py + pz * pz);
        q[3] = pw * in; q[4] = px * in; q[5] = py * in; q[6] = pz * in;
      }
    }
    __syncthreads();
  }
  if (!active) return;
  if (gc_out)
    for (int k = lane; k < nq; k += g) gc_out[(size_t)env * nq + k] = q[k];
  if (lane == 0) {
    if (error) { error[(size_t)env * 2] = ep; error[(size_t)env * 2 + 1] = er; }
    if (iterations) iterations[env] = iters;
    if (status) status[env] = st;
  }
}

}  // namespace
}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_inverse_kinematics(rsb_world* w, const rsb_frame* frames, int n_frames, int flags, const float* target_pos, const float* target_rot, const float* gc_init,
                           const uint8_t* dof_mask, const rsb_ik_options* opt, float* gc_out, float* error, int32_t* iterations, int32_t* status, int space) {
  const char* who = "rsb_inverse_kinematics";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!gc_out && !error && !iterations && !status) return invalid(who, "every output is NULL");
  if (!frames || n_frames < 1 || n_frames > RSB_MAX_IK_FRAMES) return invalid(who, "n_frames must be 1.." + std::to_string(RSB_MAX_IK_FRAMES));
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (flags & ~(RSB_IK_ANGULAR | RSB_IK_JOINT_LIMITS)) return invalid(who, "unknown flag bits");
  if (!target_pos) return invalid(who, "target_pos is NULL");
  const bool angular = (flags & RSB_IK_ANGULAR) != 0;
  if (angular && !target_rot) return invalid(who, "RSB_IK_ANGULAR needs target_rot");
  if (!angular && target_rot) return invalid(who, "target_rot without RSB_IK_ANGULAR");
  if (!opt) return invalid(who, "opt is NULL");
  if (opt->max_iter < 0) return invalid(who, "max_iter must not be negative");
  for (const float v : {opt->damping, opt->pos_tol, opt->rot_tol, opt->max_step})
    if (!std::isfinite(v) || v < 0.f) return invalid(who, "damping, pos_tol, rot_tol and max_step must be finite and not negative");
  if (opt->max_step == 0.f) return invalid(who, "max_step must be positive");
  const int nv = w->blob.nv, nq = w->blob.nq, nb = w->blob.nb;
  IkMask mask{};
  bool any = false;
  for (int d = w->blob.fixed_base ? 6 : 0; d < nv; ++d) {      // (a fixed base's six entries are ignored)
    mask.free[d] = dof_mask ? (dof_mask[d] != 0) : (d >= 6);
    any = any || mask.free[d];
  }
  if (!any) return invalid(who, "dof_mask frees no coordinate");
  HIP_TRY(hipSetDevice(w->device));
  const int kk = angular ? 6 : 3, m = kk * n_frames;
  const size_t N = (size_t)w->N, pairs = N * (size_t)n_frames;
  const int epw = ik_envs(m, nv, nq, nb, n_frames);
  if (epw < 1) { rsb::set_error(std::string(who) + ": the env record does not fit a workgroup's LDS"); return RSB_E_UNSUPPORTED; }
  const float *dtp, *dtr, *dq0;
  float *dgc, *derr, *dit, *dst;
  Staged io(w, space);
  io.in(dtp, target_pos, pairs * 3); io.in(dtr, target_rot, pairs * 9); io.in(dq0, gc_init, N * nq);
  io.out(dgc, gc_out, N * nq); io.out(derr, error, N * 2); io.out(dit, reinterpret_cast<float*>(iterations), N); io.out(dst, reinterpret_cast<float*>(status), N);
  st = io.begin(); if (st != RSB_OK) return st;
  hipStream_t s = stream_of(w);
  IkFrames fl{};
  std::copy(frames, frames + n_frames, fl.f);
  const size_t lds = ((size_t)ik_shared(nb) + (size_t)epw * ik_layout(m, nv, nq, nb, n_frames).pitch) * sizeof(float);
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ik_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ik_kernel, dim3(blocks_for(N, epw)), dim3(epw * ik_group(m)), lds, s, (const DevModel*)w->d_model, dq0 ? dq0 : (const float*)w->d_gc, fl, n_frames,
                     w->N, kk, (flags & RSB_IK_JOINT_LIMITS) ? 1 : 0, mask, *opt, dtp, dtr, dgc, derr, reinterpret_cast<int32_t*>(dit), reinterpret_cast<int32_t*>(dst));
  HIP_TRY(hipGetLastError());
  return io.end();
}

}  // extern "C"
