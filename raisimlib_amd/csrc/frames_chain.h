// frames_chain.h — the support-chain walk of the batched frame queries, shared by rsb_frames.hip (frame kinematics, Jacobians, external wrenches)
// and rsb_terrain_query.hip (the height scan's frame positions): the model rows in LDS, the running transform of the walk, and the checks of
// the frame arguments.  Everything is internal to the translation unit that includes it.
//
// A frame is a point fixed in a body (rsb_frame: body, offset in the body frame).  Its support chain is the path root -> body, at most `depth` bodies,
// listed by DevModel::anc.  walk_chain keeps the running world transform (R, p) and velocity (omega, v) of the current body in REGISTERS: no per-body
// arrays, no scratch, no cross-lane traffic.
//     p_i = p_p + R_p ptree_i (+ a_i q_i, prismatic)      R_i = R_p rtree_i Rot(axis_i, q_i)      a_i = R_i axis_i
//     v_i = v_p + omega_p x (p_i - p_p) (+ a_i qd_i, prismatic)      omega_i = omega_p (+ a_i qd_i, revolute)
//     point = p_i + R_i offset      v_point = v_i + omega_i x R_i offset
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kThreads = 256;
constexpr int kRow = 20;             // floats per body in LDS: the first 17 of DevModel::bodyf (axis 0-2, joint type 3, ptree 4-6, (mass) 7, rtree 8-16), padded
constexpr int kRowUsed = 17;

struct FrameList { rsb_frame f[RSB_MAX_FRAMES]; };      // a kernel argument: the frames travel with the launch

struct Chain { float R[9], p[3], w[3], v[3]; };

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void mat3_vec(const float* A, const float* x, float* o) {
  for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
__device__ __forceinline__ void mat3_mul(const float* A, const float* B, float* O) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

__device__ __forceinline__ void stage_rows(const DevModel& m, float* rows) {
  for (int k = threadIdx.x; k < m.nb * kRow; k += kThreads) {
    const int b = k / kRow, c = k - b * kRow;
    rows[k] = c < kRowUsed ? m.bodyf[b][c] : 0.f;
  }
}

// Walks the support chain of `body` from the base down; on return c holds the body's world transform (and, if vel, its velocity).
// on_joint(level, body i, a_i, p_i, revolute) is called once per moving joint of the chain, root first.
template <class F>
__device__ __forceinline__ void walk_chain(const DevModel& m, const float* rows, const float* q, const float* u, bool vel, int body, Chain& c, F&& on_joint) {
  {
    float w = q[3], x = q[4], y = q[5], z = q[6];
    const float in = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    w *= in; x *= in; y *= in; z *= in;
    c.R[0] = 1 - 2 * (y * y + z * z); c.R[1] = 2 * (x * y - w * z);     c.R[2] = 2 * (x * z + w * y);
    c.R[3] = 2 * (x * y + w * z);     c.R[4] = 1 - 2 * (x * x + z * z); c.R[5] = 2 * (y * z - w * x);
    c.R[6] = 2 * (x * z - w * y);     c.R[7] = 2 * (y * z + w * x);     c.R[8] = 1 - 2 * (x * x + y * y);
    const bool moves = vel && !m.fixed_base;
    for (int k = 0; k < 3; ++k) { c.p[k] = q[k]; c.v[k] = moves ? u[k] : 0.f; c.w[k] = moves ? u[3 + k] : 0.f; }
  }
  const int lv = m.level[body];
  const int* anc = m.anc + body * m.depth;
  for (int l = 1; l <= lv; ++l) {
    const int i = anc[l];
    const float* row = rows + i * kRow;
    const bool revolute = __float_as_int(row[3]) == RSB_JOINT_REVOLUTE;
    const float ax[3] = {row[0], row[1], row[2]}, pt[3] = {row[4], row[5], row[6]};
    const float qi = q[6 + i], qd = vel ? u[5 + i] : 0.f;
    float E[9], Rn[9], d[3], a[3];
    if (revolute) {
      float sn, cs, Rq[9];
      sincosf(qi, &sn, &cs);
      const float t = 1.f - cs;
      Rq[0] = cs + ax[0] * ax[0] * t;         Rq[1] = ax[0] * ax[1] * t - ax[2] * sn; Rq[2] = ax[0] * ax[2] * t + ax[1] * sn;
      Rq[3] = ax[1] * ax[0] * t + ax[2] * sn; Rq[4] = cs + ax[1] * ax[1] * t;         Rq[5] = ax[1] * ax[2] * t - ax[0] * sn;
      Rq[6] = ax[2] * ax[0] * t - ax[1] * sn; Rq[7] = ax[2] * ax[1] * t + ax[0] * sn; Rq[8] = cs + ax[2] * ax[2] * t;
      mat3_mul(row + 8, Rq, E);
    } else {
      for (int k = 0; k < 9; ++k) E[k] = row[8 + k];
    }
    mat3_mul(c.R, E, Rn);
    mat3_vec(c.R, pt, d);
    mat3_vec(Rn, ax, a);
    if (!revolute) for (int k = 0; k < 3; ++k) d[k] += a[k] * qi;
    if (vel) {
      float wd[3];
      cross3(c.w, d, wd);
      for (int k = 0; k < 3; ++k) {
        c.v[k] += wd[k] + (revolute ? 0.f : a[k] * qd);
        c.w[k] += revolute ? a[k] * qd : 0.f;
      }
    }
    for (int k = 0; k < 3; ++k) c.p[k] += d[k];
    for (int k = 0; k < 9; ++k) c.R[k] = Rn[k];
    on_joint(l, i, a, c.p, revolute);
  }
}

inline int check_world(rsb_world* w, const char* who, int space) {
  if (!w) { rsb::set_error(std::string(who) + ": null world"); return RSB_E_INVALID; }
  if (space != RSB_HOST && space != RSB_DEVICE) { rsb::set_error(std::string(who) + ": space must be RSB_HOST or RSB_DEVICE"); return RSB_E_INVALID; }
  return RSB_OK;
}

inline int check_frames(const rsb_world* w, const char* who, const rsb_frame* frames, int n) {
  if (!frames || n < 1 || n > RSB_MAX_FRAMES) { rsb::set_error(std::string(who) + ": n_frames must be 1.." + std::to_string(RSB_MAX_FRAMES)); return RSB_E_INVALID; }
  for (int i = 0; i < n; ++i) {
    if (frames[i].body < 0 || frames[i].body >= w->blob.nb) {
      rsb::set_error(std::string(who) + ": frame " + std::to_string(i) + ": body " + std::to_string(frames[i].body) + " outside [0, " + std::to_string(w->blob.nb) + ")");
      return RSB_E_INVALID;
    }
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(frames[i].offset[c])) { rsb::set_error(std::string(who) + ": frame " + std::to_string(i) + ": non-finite offset"); return RSB_E_INVALID; }
  }
  return RSB_OK;
}

inline FrameList frame_list(const rsb_frame* frames, int n) {
  FrameList fl{};
  std::copy(frames, frames + n, fl.f);
  return fl;
}

}  // namespace
}  // namespace rsbw
