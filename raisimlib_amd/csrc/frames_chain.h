// frames_chain.h — the common part of all batched queries (rsb_frames.hip, rsb_terrain_query.hip, rsb_centroidal.hip, rsb_dynamics.hip): the model
// tables in LDS, THE support-chain walk, the small vector and inertia helpers, the place of a lane in a per-body workgroup, the checks of the
// arguments, and the staging of the RSB_HOST forms.  Each is defined here once; everything is internal to the translation unit that includes it.
//
// A frame is a point fixed in a body (rsb_frame: body, offset in the body frame).  Its support chain is the path root -> body, at most `depth` bodies,
// listed by DevModel::anc.  walk_chain keeps the running world transform (R, p), velocity (omega, v) and, with ACC, acceleration (alpha, acc) of the
// current body in REGISTERS: no per-body arrays, no scratch, no cross-lane traffic.  After inlining, what a caller does not read costs nothing.
//     p_i = p_p + R_p ptree_i (+ a_i q_i, prismatic)      R_i = R_p rtree_i Rot(axis_i, q_i)      a_i = R_i axis_i      d = p_i - p_p
//     v_i = v_p + omega_p x d (+ a_i qd_i, prismatic)      omega_i = omega_p (+ a_i qd_i, revolute)
//     revolute    alpha_i = alpha_p + a_i qdd_i + omega_p x a_i qd_i        acc_i = acc_p + alpha_p x d + omega_p x (omega_p x d)
//     prismatic   alpha_i = alpha_p                                         acc_i = ... + 2 omega_p x a_i qd_i + a_i qdd_i
//     point = p_i + R_i offset      v_point = v_i + omega_i x R_i offset
// (acc: the classical acceleration of the body's origin, d/dt of its world velocity - what udot[0:3] is for the base).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "rsb_world.h"

namespace rsbw {
namespace {

constexpr int kThreads = 256;
constexpr int kRow = 20;             // floats per body in LDS: the first 17 of DevModel::bodyf (axis 0-2, joint type 3, ptree 4-6, mass 7, rtree 8-16), padded
constexpr int kRowUsed = 17;
constexpr int kXtra = 11;            // floats per body in the extra table (odd pitch): com 0-2, inertia xx xy xz yy yz zz 3-8, armature 9

struct FrameList { rsb_frame f[RSB_MAX_FRAMES]; };      // a kernel argument: the frames travel with the launch
struct Vec3 { float x, y, z; };

// a body at the end of its chain walk.  wp, vp, pp: the parent's angular velocity, velocity and position (the base's own for body 0); a, qd, qdd, type
// (0 base, 1 revolute, 2 prismatic): the body's own joint.  al, ac are carried with ACC only.
struct Chain { float R[9], p[3], w[3], v[3], al[3], ac[3], a[3], wp[3], vp[3], pp[3], qd, qdd; int type; };

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void mat3_vec(const float* A, const float* x, float* o) {
  for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
// A^T x for the row-major 3 x 3 A
__device__ __forceinline__ void mat3t_vec(const float* A, const float* x, float* o) {
  for (int c = 0; c < 3; ++c) o[c] = A[c] * x[0] + A[3 + c] * x[1] + A[6 + c] * x[2];
}
__device__ __forceinline__ void mat3_mul(const float* A, const float* B, float* O) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
// I x for the symmetric I = (xx xy xz yy yz zz)
__device__ __forceinline__ void sym3_vec(const float* I, const float* x, float* o) {
  o[0] = I[0] * x[0] + I[1] * x[1] + I[2] * x[2];
  o[1] = I[1] * x[0] + I[3] * x[1] + I[4] * x[2];
  o[2] = I[2] * x[0] + I[4] * x[1] + I[5] * x[2];
}
// the six entries of a body's inertia about o in world axes, (R I R^T)_ij + m (r.r delta_ij - r_i r_j): I = (xx xy xz yy yz zz) about the centre of
// mass in the body frame, r the centre of mass from o
__device__ __forceinline__ void inertia_about_o(const float* R, const float* I, float mass, const float* r, float* o) {
  float B[9];
  for (int k = 0; k < 3; ++k) {      // B = R I
    B[3 * k] = R[3 * k] * I[0] + R[3 * k + 1] * I[1] + R[3 * k + 2] * I[2];
    B[3 * k + 1] = R[3 * k] * I[1] + R[3 * k + 1] * I[3] + R[3 * k + 2] * I[4];
    B[3 * k + 2] = R[3 * k] * I[2] + R[3 * k + 1] * I[4] + R[3 * k + 2] * I[5];
  }
  const float rr = dot3(r, r);
  int n = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++n)
      o[n] = (B[3 * i] * R[3 * j] + B[3 * i + 1] * R[3 * j + 1] + B[3 * i + 2] * R[3 * j + 2]) + mass * ((i == j ? rr : 0.f) - r[i] * r[j]);
}

__device__ __forceinline__ void stage_rows(const DevModel& m, float* rows) {
  for (int k = threadIdx.x; k < m.nb * kRow; k += kThreads) {
    const int b = k / kRow, c = k - b * kRow;
    rows[k] = c < kRowUsed ? m.bodyf[b][c] : 0.f;
  }
}
__device__ __forceinline__ void stage_xtra(const DevModel& m, float* xtra) {
  for (int k = threadIdx.x; k < m.nb * kXtra; k += kThreads) {
    const int b = k / kXtra, c = k - b * kXtra;
    xtra[k] = c < 10 ? m.bodyf[b][17 + c] : 0.f;
  }
}

// The per-body kernels give a workgroup epb = kThreads / nb CONSECUTIVE envs, env0 on, and one lane per (env, body): this lane is body `body` of the
// block's env `el`; the envs el < here exist.
struct EnvBlock { long long env0; int here, el, body; };
__device__ __forceinline__ EnvBlock env_block(int nb, int N) {
  const int epb = kThreads / nb;
  const long long env0 = (long long)blockIdx.x * epb;
  const int here = (int)min((long long)epb, (long long)N - env0);
  const int el = threadIdx.x / nb, body = threadIdx.x - el * nb;
  return {env0, here, el, body};
}

// acc[0, W) = the first W floats of the records (one per body of an env, `pitch` floats apart) summed over the subtree below `body`, in ascending
// body order.  nb and depth MUST be m.nb and m.depth: the caller passes the copies it read before its first barrier, because read here they are
// loaded again, and waited for, in the middle of the kernel
template <int W>
__device__ __forceinline__ void subtree_sum(const DevModel& m, int nb, int depth, const float* recs, int pitch, int body, float* acc) {
  const int lj = m.level[body];
  for (int k = 0; k < W; ++k) acc[k] = 0.f;
  for (int i = body; i < nb; ++i) {      // (a subtree's bodies are numbered from its root up: parent[i] < i)
    if (m.anc[i * depth + lj] != body) continue;
    for (int k = 0; k < W; ++k) acc[k] += recs[i * pitch + k];
  }
}

struct NoJoint { __device__ __forceinline__ void operator()(int, int, const float*, const float*, bool) const {} };      // a walk that only wants its end

// Walks the support chain of `body` from the base down; on return c describes the body: its world transform, if vel its velocity, its parent's and
// its joint rate, with ACC (and vel) its accelerations under ud (null: zeros).  u is not read without vel.  A fixed base neither moves nor accelerates:
// its rows of u and ud are not read.  on_joint(level, body i, a_i, p_i, revolute) is called once per moving joint of the chain, root first.
template <bool ACC, class F>
__device__ __forceinline__ void walk_chain(const DevModel& m, const float* rows, const float* q, const float* u, const float* ud, bool vel, int body, Chain& c,
                                           F&& on_joint) {
  {
    float w = q[3], x = q[4], y = q[5], z = q[6];
    const float in = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    w *= in; x *= in; y *= in; z *= in;
    c.R[0] = 1 - 2 * (y * y + z * z); c.R[1] = 2 * (x * y - w * z);     c.R[2] = 2 * (x * z + w * y);
    c.R[3] = 2 * (x * y + w * z);     c.R[4] = 1 - 2 * (x * x + z * z); c.R[5] = 2 * (y * z - w * x);
    c.R[6] = 2 * (x * z - w * y);     c.R[7] = 2 * (y * z + w * x);     c.R[8] = 1 - 2 * (x * x + y * y);
    const bool moves = vel && !m.fixed_base;
    for (int k = 0; k < 3; ++k) {
      c.p[k] = q[k]; c.v[k] = moves ? u[k] : 0.f; c.w[k] = moves ? u[3 + k] : 0.f;
      c.ac[k] = (ACC && moves && ud) ? ud[k] : 0.f; c.al[k] = (ACC && moves && ud) ? ud[3 + k] : 0.f;
      c.a[k] = 0.f; c.wp[k] = c.w[k]; c.vp[k] = c.v[k]; c.pp[k] = c.p[k];
    }
    c.qd = 0.f; c.qdd = 0.f; c.type = 0;
  }
  const int lv = m.level[body];
  const int* anc = m.anc + body * m.depth;
  for (int l = 1; l <= lv; ++l) {
    const int i = anc[l];
    const float* row = rows + i * kRow;
    const bool revolute = __float_as_int(row[3]) == RSB_JOINT_REVOLUTE;
    const float ax[3] = {row[0], row[1], row[2]}, pt[3] = {row[4], row[5], row[6]};
    const float qi = q[6 + i], qd = vel ? u[5 + i] : 0.f, qdd = (ACC && vel && ud) ? ud[5 + i] : 0.f;
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
      float wd[3], wa[3];
      cross3(c.w, d, wd);
      cross3(c.w, a, wa);
      for (int k = 0; k < 3; ++k) { c.wp[k] = c.w[k]; c.vp[k] = c.v[k]; c.pp[k] = c.p[k]; }
      if (ACC) {
        float ad[3], wwd[3];
        cross3(c.al, d, ad);
        cross3(c.w, wd, wwd);
        for (int k = 0; k < 3; ++k) {
          c.ac[k] += ad[k] + wwd[k] + (revolute ? 0.f : 2.f * wa[k] * qd + a[k] * qdd);
          c.al[k] += revolute ? a[k] * qdd + wa[k] * qd : 0.f;
        }
      }
      for (int k = 0; k < 3; ++k) {
        c.v[k] += wd[k] + (revolute ? 0.f : a[k] * qd);
        c.w[k] += revolute ? a[k] * qd : 0.f;
      }
    }
    for (int k = 0; k < 3; ++k) { c.p[k] += d[k]; c.a[k] = a[k]; }
    for (int k = 0; k < 9; ++k) c.R[k] = Rn[k];
    c.qd = qd; c.qdd = qdd; c.type = revolute ? 1 : 2;
    on_joint(l, i, a, c.p, revolute);
  }
}

inline int invalid(const char* who, const std::string& what) { rsb::set_error(std::string(who) + ": " + what); return RSB_E_INVALID; }

inline int check_world(rsb_world* w, const char* who, int space) {
  if (!w) return invalid(who, "null world");
  if (space != RSB_HOST && space != RSB_DEVICE) return invalid(who, "space must be RSB_HOST or RSB_DEVICE");
  return RSB_OK;
}

inline int check_frames(const rsb_world* w, const char* who, const rsb_frame* frames, int n) {
  if (!frames || n < 1 || n > RSB_MAX_FRAMES) return invalid(who, "n_frames must be 1.." + std::to_string(RSB_MAX_FRAMES));
  for (int i = 0; i < n; ++i) {
    if (frames[i].body < 0 || frames[i].body >= w->blob.nb)
      return invalid(who, "frame " + std::to_string(i) + ": body " + std::to_string(frames[i].body) + " outside [0, " + std::to_string(w->blob.nb) + ")");
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(frames[i].offset[c])) return invalid(who, "frame " + std::to_string(i) + ": non-finite offset");
  }
  return RSB_OK;
}

inline FrameList frame_list(const rsb_frame* frames, int n) {
  FrameList fl{};
  std::copy(frames, frames + n, fl.f);
  return fl;
}

inline Vec3 gravity_of(const rsb_world* w) { return {(float)w->gravity[0], (float)w->gravity[1], (float)w->gravity[2]}; }

// workgroups for `lanes` units of work, `per` to a workgroup
inline unsigned blocks_for(size_t lanes, size_t per = kThreads) { return (unsigned)((lanes + per - 1) / per); }
inline unsigned env_blocks(const rsb_world* w) { return blocks_for((size_t)w->N, (size_t)(kThreads / w->blob.nb)); }      // ... of a per-body kernel (EnvBlock)

// The buffers of one query call.  The caller declares its inputs and outputs (a NULL one is declared all the same and stays NULL), then begin(),
// the launch, end().  RSB_DEVICE: every slot is the caller's own pointer and begin() / end() do nothing.  RSB_HOST: begin() sizes the world's
// staging buffer for exactly what is not NULL, gives each such buffer its slice in declaration order and enqueues the inputs' copies on the world's
// stream; end() brings the outputs back in declaration order through copy_out, which waits for the stream (the caller may reuse its host buffers on
// return) and reports a fault once - or, with no output, waits for the stream itself.  scratch() asks for device floats at the head of the same
// buffer in either space: what a query made of several launches hands from one to the next.
class Staged {
 public:
  Staged(rsb_world* w, int space) : w_(w), host_(space == RSB_HOST) {}
  void in(const float*& dev, const float* host, size_t floats) { dev = host; add({host, floats * sizeof(float), &dev, nullptr, nullptr}); }
  void in(const uint8_t*& dev, const uint8_t* host, size_t bytes) { dev = host; add({host, bytes, nullptr, &dev, nullptr}); }
  void out(float*& dev, float* host, size_t floats) { dev = host; add({host, floats * sizeof(float), nullptr, nullptr, &dev}); }
  void scratch(float*& dev, size_t floats) { dev = nullptr; scratch_slot_ = &dev; scratch_ = floats; }
  int begin() {
    if (n_ > kMax) return invalid("Staged", "more than " + std::to_string(kMax) + " buffers declared");
    if (!host_ && !scratch_) return RSB_OK;
    size_t total = scratch_;
    for (int k = 0; host_ && k < n_; ++k) total += floats(items_[k]);
    const int st = staging(w_, total); if (st != RSB_OK) return st;
    float* b = w_->d_frames_io;
    if (scratch_) { *scratch_slot_ = b; b += scratch_; }
    if (!host_) return RSB_OK;
    hipStream_t s = stream_of(w_);
    for (int k = 0; k < n_; ++k) {
      const Item& it = items_[k];
      if (!it.out) HIP_TRY(hipMemcpyAsync(b, it.host, it.bytes, hipMemcpyHostToDevice, s));
      if (it.f) *it.f = b;
      if (it.b) *it.b = (const uint8_t*)b;
      if (it.out) *it.out = b;
      b += floats(it);
    }
    return RSB_OK;
  }
  int end() {
    if (!host_) return RSB_OK;
    bool any = false;
    for (int k = 0; k < n_; ++k) {
      const Item& it = items_[k];
      if (!it.out) continue;
      any = true;
      const int st = copy_out(w_, const_cast<void*>(it.host), *it.out, it.bytes, RSB_HOST); if (st != RSB_OK) return st;
    }
    if (!any) HIP_TRY(hipStreamSynchronize(stream_of(w_)));
    return RSB_OK;
  }

 private:
  struct Item { const void* host; size_t bytes; const float** f; const uint8_t** b; float** out; };      // one of f, b, out: the caller's slot
  static size_t floats(const Item& it) { return (it.bytes + sizeof(float) - 1) / sizeof(float); }
  void add(const Item& it) { if (it.host && n_++ < kMax) items_[n_ - 1] = it; }      // (one too many: counted, not stored; begin() refuses)
  rsb_world* w_;
  bool host_;
  static constexpr int kMax = 8;
  Item items_[kMax];
  int n_ = 0;
  float** scratch_slot_ = nullptr;
  size_t scratch_ = 0;
};

}  // namespace
}  // namespace rsbw
