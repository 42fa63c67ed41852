// rsb_world.hip — host side of the C-ABI (include/rsb.h): device-resident batched world.
//
// Plays the role of N x { raisim::World + one raisim::ArticulatedSystem + Ground/HeightMap }
// [RECALL; World.hpp / ArticulatedSystem.hpp are absent from /root/reference, SURVEY.md §8b].
// State lives in HBM as row-major [N, dim] float32 rows; rsb_integrate() launches the fused step
// kernel (step_kernel.h) on the handle's stream.  No CPU fallback exists anywhere in this file.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "query_kernel.h"
#include "rsb.h"
#include "rsb_internal.h"
#include "step_launch.h"
#include "env_task.h"
#include "step_types.h"


#include "rsb_world.h"
#include "rsb_spec.h"

namespace rsbw {

// Kernel arguments in device memory: with host-resident kernargs every wave's first scalar loads cross PCIe (measured: step
// kernel prologue 20.6 k cycles instead of 9.2 k, 142 M instead of 149 M env-steps/s).  It is this image's default; set here
// (without overriding the user's choice) for runtimes where it is not - effective when the library loads before HIP starts.
// GPU_MAX_HW_QUEUES: HIP multiplexes its streams onto 4 hardware queues by default; the closed-loop pipeline needs three private streams that
// overlap (two step streams + the action stage's) beside the caller's own - 8 queues make the probe's search for such a set short.
struct DevKernargDefault { DevKernargDefault() { setenv("HIP_FORCE_DEV_KERNARG", "1", 0); setenv("GPU_MAX_HW_QUEUES", "8", 0); } } g_dev_kernarg_default;

int round4(int x) { return (x + 3) & ~3; }

void build_dev_model(const rsb_model_blob& b, DevModel* d) {
  std::memset(d, 0, sizeof *d);
  d->nb = b.nb; d->nq = b.nq; d->nv = b.nv; d->ncol = b.ncol; d->depth = b.depth;
  d->cw = round4(6 + b.depth - 1);
  d->fixed_base = b.fixed_base;
  std::vector<std::vector<int>> kids(b.nb);
  for (int i = 0; i < b.nb; ++i) {
    d->parent[i] = b.parent[i]; d->level[i] = b.level[i]; d->jtype[i] = b.jtype[i];
    if (i > 0) kids[b.parent[i]].push_back(i);
    float* f = d->bodyf[i];
    for (int c = 0; c < 3; ++c) {
      d->axis[i][c] = f[c] = (float)b.axis[i][c];
      d->ptree[i][c] = f[4 + c] = (float)b.ptree[i][c];
      d->com[i][c] = f[17 + c] = (float)b.com[i][c];
    }
    std::memcpy(&f[3], &b.jtype[i], sizeof(int));
    for (int c = 0; c < 9; ++c) d->rtree[i][c] = f[8 + c] = (float)b.rtree[i][c];
    for (int c = 0; c < 6; ++c) d->inertia[i][c] = f[20 + c] = (float)b.inertia[i][c];
    d->mass[i] = f[7] = (float)b.mass[i];
    d->armature[i] = f[26] = (float)b.armature[i];
    f[27] = (float)b.damping[i];
    f[28] = (float)b.effort[i];
    const bool limited = i > 0 && b.q_lower[i] < b.q_upper[i] && b.q_lower[i] > -1e29 && b.q_upper[i] < 1e29;
    f[29] = limited ? (float)b.q_lower[i] : -3e38f;   // joint range (an unlimited joint can never leave it)
    f[30] = limited ? (float)b.q_upper[i] : 3e38f;
  }
  for (int i = 0; i < b.nb * b.depth; ++i) d->anc[i] = -1;
  for (int i = 0; i < b.nb; ++i)
    for (int j = i; j >= 0; j = b.parent[j]) d->anc[i * b.depth + b.level[j]] = j;
  // children lists (the step kernel's up pass gathers over them); the base's children lead the list
  int pos = 0;
  d->max_kid = 0;
  for (int i = 0; i < b.nb; ++i) {
    d->kid_start[i] = pos;
    d->kid_count[i] = (int)kids[i].size();
    for (int c : kids[i]) d->kid_list[pos++] = c;
    if (i >= 1 && d->kid_count[i] > d->max_kid) d->max_kid = d->kid_count[i];
  }
  for (int s = 0; s < b.ncol; ++s) {
    d->col_body[s] = b.col_body[s];
    for (int c = 0; c < 3; ++c) d->col_pos[s][c] = (float)b.col_pos[s][c];
    d->col_pos[s][3] = (float)b.col_radius[s];
  }
}

// candidate pairs of self-collision (oracle: self_pair_ok): primitives on two bodies that are not parent and child, not both
// points, no rim primitives, bodies not excluded by the caller
std::vector<int> enumerate_self_pairs(const rsb_model_blob& b, const std::vector<uint8_t>& ignore) {
  std::vector<int> out;
  for (int i = 0; i < b.ncol; ++i)
    for (int j = i + 1; j < b.ncol; ++j) {
      const int bi = b.col_body[i], bj = b.col_body[j];
      if (bi == bj || b.parent[bi] == bj || b.parent[bj] == bi) continue;
      if (b.col_rim[i] > 0.0 || b.col_rim[j] > 0.0) continue;
      if (!(b.col_radius[i] + b.col_radius[j] > 0.0)) continue;
      if (!ignore.empty() && (ignore[bi * b.nb + bj] || ignore[bj * b.nb + bi])) continue;
      out.push_back(i); out.push_back(j);
    }
  return out;
}

// Quad form of the up pass (step_spec.h: RSB_UP_QUADS; step_phase_tree_up.inc).  A model qualifies when it is a base + FOUR consecutively numbered serial
// chains of equal length, at most 16 bodies: every tree level below the base then holds exactly four bodies, and the body of quad g (lanes 4 g .. 4 g + 3 of a
// 16-lane env) at level lv is  (g-th child of the base) + lv - 1.  Returns the number of levels below the base and fills table[(lv - 1) * 4 + g] (may be null), or 0.
int up_quad_table(const rsb_model_blob& b, int* table) {
  if (b.nb > 16 || b.depth < 2 || b.nb - 1 != 4 * (b.depth - 1)) return 0;
  int first[4], n1 = 0;
  for (int i = 1; i < b.nb; ++i) {
    if (b.level[i] == 1) { if (n1 == 4) return 0; first[n1++] = i; }
    else if (b.parent[i] != i - 1) return 0;
  }
  if (n1 != 4) return 0;
  for (int g = 0; g < 4; ++g)
    for (int lv = 1; lv < b.depth; ++lv) {
      const int body = first[g] + lv - 1;
      if (body >= b.nb || b.level[body] != lv) return 0;
      if (table) table[(lv - 1) * 4 + g] = body;
    }
  return b.depth - 1;
}

// Own-lane form of the plane's collision test (step_spec.h: RSB_COL_OWN; step_phase_collision.inc).  Stage (3) of the down pass leaves the pose of body s on lane s
// of a 16-lane env, 1 <= s < nb, and the base's on lane 0 and on the lanes >= nb.  Every collision primitive is assigned to one (pass, lane) whose lane holds the
// primitive's body, so that the test needs no pose read: a body's primitives go in index order to ascending passes of the body's lane; the base's go in index order
// over lane 0 and the lanes >= nb of pass 0, then over those lanes of pass 1, and so on.  A model qualifies when it has at most 16 bodies, no rim primitive
// (rsb_model_blob::col_rim) and the assignment needs no more passes than ceil(ncol / 16), the passes of the primitive-order loop it replaces.
// Returns the number of passes, or 0.  prim[pass * 16 + lane] = the primitive, or -1; lower[(pass * 16 + lane) * passes + u] = the lanes (bit l = lane l) whose
// primitive of pass u has a LOWER index than prim[pass * 16 + lane] (0 where that is -1): the hits among them, over all passes u, are the contacts that precede this
// primitive's in primitive order.  Both may be null.
int col_own_table(const rsb_model_blob& b, int* prim, int* lower) {
  constexpr int kLanes = 16;
  if (b.nb < 1 || b.nb > kLanes || b.ncol < 1) return 0;
  for (int i = 0; i < b.ncol; ++i) if (b.col_rim[i] > 0.0) return 0;
  const int npass = (b.ncol + kLanes - 1) / kLanes;
  std::vector<int> base_lanes(1, 0), used(b.nb, 0), P((size_t)npass * kLanes, -1);
  for (int l = b.nb; l < kLanes; ++l) base_lanes.push_back(l);
  for (int i = 0; i < b.ncol; ++i) {
    const int body = b.col_body[i];
    if (body < 0 || body >= b.nb) return 0;
    const int k = used[body]++;
    const int pass = body == 0 ? k / (int)base_lanes.size() : k, lane = body == 0 ? base_lanes[k % base_lanes.size()] : body;
    if (pass >= npass) return 0;
    P[(size_t)pass * kLanes + lane] = i;
  }
  for (int e = 0; e < npass * kLanes; ++e) {
    if (prim) prim[e] = P[e];
    if (!lower) continue;
    for (int u = 0; u < npass; ++u) {
      int mask = 0;
      for (int l = 0; l < kLanes; ++l) if (P[e] >= 0 && P[(size_t)u * kLanes + l] >= 0 && P[(size_t)u * kLanes + l] < P[e]) mask |= 1 << l;
      lower[(size_t)e * npass + u] = mask;
    }
  }
  return npass;
}

// Closed form of the flat Delassus trip (step_spec.h: RSB_FLAT_DELASSUS; step_phase_delassus.inc): in a model of four consecutively numbered chains of NL = depth - 1
// bodies, body b >= 1 sits on limb (b - 1) / NL at level (b - 1) % NL + 1, and two bodies share min(li, lj) levels of their support chains when they sit on one
// limb, none otherwise.  Compared here, for EVERY body pair (the bodies of joint-limit rows are among them), with what the kernel's look-up gives: the number of
// leading levels 1.. at which the two ancestor rows (build_dev_model: anc) agree.  A model the form does not describe is not reported as such chains.
static bool delassus_closed_form_ok(const rsb_model_blob& b) {
  const int nl = b.depth - 1;
  if (nl < 1) return false;
  std::vector<int> anc((size_t)b.nb * b.depth, -1);
  for (int i = 0; i < b.nb; ++i)
    for (int j = i; j >= 0; j = b.parent[j]) anc[(size_t)i * b.depth + b.level[j]] = j;
  auto level_of = [&](int x) { return x > 0 ? (x - 1) % nl + 1 : 0; };
  for (int i = 0; i < b.nb; ++i) {
    if (level_of(i) != b.level[i]) return false;
    for (int j = 0; j < b.nb; ++j) {
      int table = 0;
      while (table < nl && table + 1 <= b.level[i] && table + 1 <= b.level[j] && anc[(size_t)i * b.depth + table + 1] == anc[(size_t)j * b.depth + table + 1]) ++table;
      const int form = (i > 0 && j > 0 && (i - 1) / nl == (j - 1) / nl) ? std::min(level_of(i), level_of(j)) : 0;
      if (form != table) return false;
    }
  }
  return true;
}

// slots of the height-map narrow phase: one per primitive (every sphere of the model may be near the ground at once - a robot lying in a hollow)
int hm_slots_for(const rsb_model_blob& b) { return std::max(rsbk::kHmSlots, (int)b.ncol); }

// Contact capacity of the kernel class a world is dispatched to (the template's KMAX): 8 for the shallow, few-contact models (the
// quadruped's classes), 16 for kmax > 8 AND for every model deeper than five levels, whose only compiled classes are the large ones
// (do_integrate).  ONE quantity decides layout, dispatch and LDS size: the layout used to follow kmax alone, so a deep model at the
// default kmax 8 ran the KMAX-16 kernel (packed triangular Delassus blocks) on the square layout.
int kcap_of(const rsb_model_blob& b, int kmax) { return (kmax <= 8 && b.depth - 1 <= 4) ? 8 : 16; }

static LdsLayout make_layout_pitch(const rsb_model_blob& b, int kcap, int n_self, int model_pitch) {
  LdsLayout L;
  L.model_pitch = model_pitch;
  const int cw = round4(6 + b.depth - 1);
  int o = 0;
  auto take = [&](int n) { int r = o; o += round4(n); return r; };
  L.t_model = take(b.nb * model_pitch);
  L.t_gain = take(2 * b.nb);
  L.t_parlv = take(b.nb);
  L.t_anc = take(b.nb * b.depth);
  L.t_dir = take(64);
  L.t_col = take(rsbk::kColSlot * b.ncol);
  L.t_kids = take(b.nb);
  L.t_kidx = take(b.nb);
  L.t_spair = take(n_self > 0 ? n_self + 1 : 0);   // (+ one entry that cannot hit, read by the lanes past the list)
  L.shared_total = o;
  o = 0;
  L.q = take(b.nq < 8 ? 8 : b.nq); L.u = take(b.nv < 8 ? 8 : b.nv);
  L.pt = take(b.nq); L.dtg = take(b.nv); L.tf = take(b.nv < 8 ? 8 : b.nv);
  L.body = take(b.nb * rsbk::kBodySlot);
  const bool tri = kcap > 8;   // packed lower-triangular Delassus blocks (step_kernel.h: TRI); the up pass's factors then alias them too
  if (!tri) L.fact = take(b.nb * rsbk::kFactSlot);
  L.wb = take(b.nv);
  L.con = take(kcap * rsbk::kConSlot);
  L.wc = take(3 * kcap * cw);
  L.cv = take(3 * kcap);
  L.gstride = 4 * kcap + 4;   // 3x3 blocks on a 4-float pitch, +4 staggers the banks of consecutive rows
  // the up pass's [nb][28] hand-over slots and the height-map narrow phase's scratch alias the Delassus rows
  // (packed layout: [hand-over slots | joint factors] of the up pass - the factors are last read by the contact columns, before the
  // Delassus phase writes its blocks over both)
  // (square classes: the kernel stores one row of kcap 12-float blocks per contact, step_types.h: g_row_pitch - inside the dense rows' 3 kcap x gstride floats, which stay the region's size)
  static_assert(rsbk::g_row_pitch(8) <= 3 * (4 * 8 + 4), "the block rows of the Delassus phase must fit the region of the dense rows");
  const int gsize = tri ? (kcap * (kcap + 1) / 2) * 12 : 3 * kcap * L.gstride;
  const int upsize = b.nb * rsbk::kUpSlot + (tri ? b.nb * rsbk::kFactSlot : 0);
  L.g = take(std::max({gsize, upsize, (rsbk::kHmRec + 8) * hm_slots_for(b) + RSB_MAX_COLLISIONS + 16}));   // (+ 16: the capsule search's four sample results)
  if (tri) L.fact = L.g + b.nb * rsbk::kUpSlot;
  L.ginv = take(12 * kcap);
  L.lam = take(3 * kcap);
  L.warm = take(6 * b.ncol);
  L.tact = take(b.nv);
  // self-collision: the primitive centres live in the contact columns' space when they fit (dead until the column phase)
  L.cen = L.wc; L.selft = 0;
  if (n_self > 0) {
    if (4 * b.ncol > 3 * kcap * cw) L.cen = take(4 * b.ncol);
    L.selft = take(4 * kcap);
  }
  L.per_env = o + rsbk::kEnvPad;
  return L;
}

// dynamic LDS of a workgroup of 64 / lpe envs
static size_t lds_bytes_of(const LdsLayout& L, int lpe) { return sizeof(float) * ((size_t)L.shared_total + (size_t)(64 / lpe) * L.per_env); }

// The conflict-free pitch of the model table (step_types.h: kModelPitch) costs 4 floats per body - and a workgroup per CU where the layout sits on a 160-KiB
// cliff (the Atlas-like humanoid at 32 lanes per env: 3 workgroups -> 2, config 5 fell from 38.9 M to 26.4 M env-steps/s in gpurun r06d): it is taken only
// where no lanes-per-env choice loses a workgroup to it.
LdsLayout make_layout(const rsb_model_blob& b, int kcap, int n_self) {
  const LdsLayout tight = make_layout_pitch(b, kcap, n_self, rsbk::kModelSlot), wide = make_layout_pitch(b, kcap, n_self, rsbk::kModelPitch);
  auto wgs = [](const LdsLayout& L, int lpe) {
    const size_t bytes = lds_bytes_of(L, lpe);
    return bytes > 160 * 1024 ? 0 : (int)std::min<size_t>(4, (160 * 1024) / bytes);
  };
  for (int lpe : {16, 32, 64}) if (wgs(wide, lpe) != wgs(tight, lpe)) return tight;
  return wide;
}

size_t lds_bytes_for(const rsb_model_blob& b, int kcap, int lpe, int n_self) { return lds_bytes_of(make_layout(b, kcap, n_self), lpe); }

// Lanes per env: the group size that keeps the most envs resident on a CU.  The kernel runs at one wave per SIMD
// (register budget), so a CU holds min(4, 160 KiB / workgroup LDS) workgroups of 64/LPE envs each.  ANYmal-like models:
// LPE 16 (4 x 4 envs, 38 KB per workgroup: at N = 4096 one wave on every SIMD of the chip); Atlas-like, kmax 16
// (25 KB per env): every choice holds 4 envs, LPE 64 keeps all four SIMDs busy.
int default_lpe(const rsb_model_blob& b, int kmax, int n_self) {
  const int kcap = kcap_of(b, kmax);
  const int need = b.nb > 16 ? (b.nb > 32 ? 64 : 32) : 16;   // lane = body in the tree passes
  int best = 64, best_envs = 0, best_wgs = 0;
  for (int lpe = need; lpe <= 64; lpe *= 2) {
    const size_t wg = lds_bytes_for(b, kcap, lpe, n_self);
    if (wg > 160 * 1024) continue;
    if (n_self > 30 * lpe) continue;   // the self-collision sweep holds one hit bit per pass of lpe pairs (check_lpe)
    const int wgs = (int)std::min<size_t>(4, (160 * 1024) / wg);
    const int envs = wgs * (64 / lpe);
    // ties go to the layout that keeps more SIMDs busy (more, smaller workgroups)
    if (envs > best_envs || (envs == best_envs && wgs > best_wgs)) { best_envs = envs; best_wgs = wgs; best = lpe; }
  }
  return best;
}

// zero the solver's warm state of the envs whose state was overwritten (mask == NULL: all)
__global__ void warm_clear_kernel(float* warm, const uint8_t* mask, int N, int n6) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * n6) return;
  if (!mask || mask[i / n6]) warm[i] = 0.f;
}

__global__ void masked_row_copy(float* dst, const float* src, const uint8_t* mask, int N, int dim) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * dim) return;
  int e = i / dim;
  if (!mask || mask[e]) dst[i] = src[i];
}

__global__ void gather_obs_kernel(float* out, const float* gc, const float* gv, const rsb_contact* contacts,
                                  const int32_t* count, const int32_t* idx, int N, int nq, int nv, int kmax,
                                  int nslots, float inv_dt) {
  int od = nq + nv + 3 * nslots;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * od) return;
  int e = i / od, c = i - e * od;
  float v;
  if (c < nq) v = gc[(size_t)e * nq + c];
  else if (c < nq + nv) v = gv[(size_t)e * nv + c - nq];
  else {
    int sl = (c - nq - nv) / 3, ax = (c - nq - nv) - 3 * sl;
    int want = idx ? idx[sl] : sl;
    v = 0.f;
    int nc = count[e];
    for (int k = 0; k < nc; ++k) {
      const rsb_contact& ct = contacts[(size_t)e * kmax + k];
      if ((ct.collision & ~(RSB_CONTACT_SECOND | RSB_CONTACT_CAPSULE)) == want) v += ct.impulse[ax] * inv_dt;   // (a primitive's contacts with a height map add up)
    }
  }
  out[i] = v;
}

__global__ void reset_terminated_kernel(float* gc, float* gv, const rsb_contact* contacts, int32_t* count,
                                        int32_t* flags, unsigned long long allowed, const float* gc0, const float* gv0,
                                        int rows, uint8_t* done, int N, int nq, int nv, int kmax, float* warm, int n6) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  bool term = (flags[e] & 2) != 0;
  const int nc = count[e];
  for (int k = 0; k < nc; ++k) {
    const int c = contacts[(size_t)e * kmax + k].collision & ~(RSB_CONTACT_SECOND | RSB_CONTACT_CAPSULE);   // (a second flank's / a capsule cylinder's contact counts as its primitive's)
    // an entry of a self-collision (id | RSB_CONTACT_SELF_A / _B) is never a foot on the terrain: terminal, as in the fused
    // epilogue of the step kernel (and a shift by >= 64 would be undefined)
    if (c >= RSB_CONTACT_SELF_A || !((allowed >> c) & 1ull)) term = true;
  }
  if (term) {
    const size_t r = rows == 1 ? 0 : (size_t)e;
    for (int i = 0; i < nq; ++i) gc[(size_t)e * nq + i] = gc0[r * nq + i];
    for (int i = 0; i < nv; ++i) gv[(size_t)e * nv + i] = gv0[r * nv + i];
    for (int i = 0; i < n6; ++i) warm[(size_t)e * n6 + i] = 0.f;
    count[e] = 0;
    flags[e] = 0;
  }
  if (done) done[e] = term ? 1 : 0;
}

// ---- device-resident vectorised env (rsg_anymal task semantics, see rsb.h and env_task.h) ----------------------
// The step itself (action -> targets, sub-steps, reward, termination, reset, next observation) is ONE launch of the step
// kernel (StepArgs::env_*); what remains here is the stand-alone observation and the reset of all envs.
// thread = (env, observation entry): env_ob_entry is the arithmetic the fused epilogue uses (bit-identical observations), so a thread per entry
// only repeats the quaternion -> rotation part per entry - 3 us for 4096 envs where the thread-per-env loop took 13 (it opens every closed-loop run)
__global__ void env_obs_kernel(float* ob, const float* gc, const float* gv, int N, int nq, int nv) {
  const int od = 10 + 2 * (nv - 6);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * od) return;
  const int e = i / od, k = i - e * od;
  const float* q = gc + (size_t)e * nq;
  const float* u = gv + (size_t)e * nv;
  ob[i] = rsbk::env_ob_entry(k, nv - 6, [&](int j) { return q[j]; }, [&](int j) { return u[j]; });
}

__global__ void env_reset_kernel(float* gc, float* gv, int32_t* count, int32_t* flags, const float* gc0, const float* gv0, int rows,
                                 int N, int nq, int nv, float* warm, int n6) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const size_t r = rows == 1 ? 0 : (size_t)e;
  for (int i = 0; i < nq; ++i) gc[(size_t)e * nq + i] = gc0[r * nq + i];
  for (int i = 0; i < nv; ++i) gv[(size_t)e * nv + i] = gv0[r * nv + i];
  for (int i = 0; i < n6; ++i) warm[(size_t)e * n6 + i] = 0.f;
  count[e] = 0; flags[e] = 0;
}

// ---- the instances of step_launch.h's list and their launchers; the class of a launch is looked up here (a scan of ~100 entries, no allocation)
using StepLauncher = hipError_t (*)(const StepArgs&, int, size_t, hipStream_t);
struct StepInstance { int lpe, kmax, cl, ml; StepLauncher run, run_prof; };   // (run_prof: the profiling twin, nullptr where the list builds none)
template <int LPE, int KMAX, int CL, int ML, int PROF>
constexpr StepInstance step_instance() {
  if constexpr (PROF != 0) return {LPE, KMAX, CL, ML, &rsbk::launch_step_instance<LPE, KMAX, CL, ML, false>, &rsbk::launch_step_instance<LPE, KMAX, CL, ML, true>};
  else return {LPE, KMAX, CL, ML, &rsbk::launch_step_instance<LPE, KMAX, CL, ML, false>, nullptr};
}
#define RSB_STEP_ENTRY(LPE, KMAX, CL, ML, PROF) step_instance<LPE, KMAX, CL, ML, PROF>(),
constexpr StepInstance kStepInstances[] = {RSB_STEP_INSTANCES(RSB_STEP_ENTRY)};
#undef RSB_STEP_ENTRY

const StepInstance* find_instance(const StepClass& c) {
  for (const StepInstance& e : kStepInstances)
    if (e.lpe == c.lpe && e.kmax == c.kmax && e.cl == c.cl && e.ml == c.ml) return &e;
  return nullptr;
}

// launches `blocks` workgroups of class c (chosen by choose_step_class, so a miss here is a bug)
int launch_instance(const StepClass& c, const StepArgs& a, int blocks, size_t lds_bytes, hipStream_t stream) {
  const StepInstance* e = find_instance(c);
  const StepLauncher run = !e ? nullptr : c.prof ? e->run_prof : e->run;
  if (!run) { rsb::set_error("internal: step kernel class <" + std::to_string(c.lpe) + ", " + std::to_string(c.kmax) + ", " + std::to_string(c.cl) + ", " + std::to_string(c.ml) + (c.prof ? ", profiling" : "") + "> is not built"); return RSB_E_UNSUPPORTED; }
  HIP_TRY(run(a, blocks, lds_bytes, stream));
  return RSB_OK;
}

int n_self_pairs(const rsb_world* w) { return w->self_collision ? (int)w->self_pairs.size() / 2 : 0; }

// the base + consecutively numbered serial chains, at most 16 bodies (StepArgs::chain)
static bool model_is_chains(const rsb_model_blob& b) {
  if (b.nb > 16) return false;
  for (int i = 1; i < b.nb; ++i) if (b.level[i] >= 2 && b.parent[i] != i - 1) return false;
  return true;
}
// both quad forms of the tree passes run (StepArgs::chain == 2) in the specialised code objects of class (lpe, kcap) with layout L
static bool quad_forms_run(const rsb_model_blob& b, int lpe, int kcap, const LdsLayout& L) {
  return model_is_chains(b) && lpe == 16 && kcap <= 8 && up_quad_table(b, nullptr) > 0 && delassus_closed_form_ok(b) && b.nb * rsbk::kUpQuadSlot <= L.ginv - L.g;
}
// [passes][16][kColOwnRec] as the kernel reads it (StepArgs::col_own_tab); empty where the model has no table
static std::vector<float> col_own_image(const rsb_model_blob& b) {
  int prim[RSB_MAX_COLLISIONS + 16], lower[(RSB_MAX_COLLISIONS + 16) * 4];
  const int npass = b.ncol <= 64 ? col_own_table(b, prim, lower) : 0;
  std::vector<float> img((size_t)npass * 16 * rsbk::kColOwnRec, 0.f);
  for (int e = 0; e < npass * 16; ++e) {
    float* r = &img[(size_t)e * rsbk::kColOwnRec];
    const int i = prim[e];
    if (i >= 0) { r[0] = (float)b.col_pos[i][0]; r[1] = (float)b.col_pos[i][1]; r[2] = (float)b.col_pos[i][2]; r[3] = (float)b.col_radius[i]; }
    int words[3] = {i, 0, 0};
    for (int u = 0; u < npass; ++u) words[1 + (u >> 1)] |= lower[e * npass + u] << (16 * (u & 1));
    std::memcpy(r + 4, words, sizeof words);
  }
  return img;
}

}  // namespace rsbw
extern "C" int rsb_model_lds_bytes(const rsb_model* m, int kmax, int self_collision, int lanes_per_env) {
  if (!m || kmax < 1 || kmax > RSB_MAX_CONTACTS || (lanes_per_env != 0 && lanes_per_env != 16 && lanes_per_env != 32 && lanes_per_env != 64)) { rsb::set_error("rsb_model_lds_bytes: bad argument"); return RSB_E_INVALID; }
  const rsb_model_blob& b = m->blob;
  const int n_self = self_collision ? (int)rsbw::enumerate_self_pairs(b, std::vector<uint8_t>()).size() / 2 : 0;
  const int lpe = lanes_per_env ? lanes_per_env : rsbw::default_lpe(b, kmax, n_self);
  return (int)rsbw::lds_bytes_for(b, rsbw::kcap_of(b, kmax), lpe, n_self);
}
extern "C" int rsb_model_delassus_layout(const rsb_model* m, int kmax, int self_collision, int* out4) {
  if (!m || !out4 || kmax < 1 || kmax > RSB_MAX_CONTACTS) { rsb::set_error("rsb_model_delassus_layout: bad argument"); return RSB_E_INVALID; }
  const rsb_model_blob& b = m->blob;
  const int n_self = self_collision ? (int)rsbw::enumerate_self_pairs(b, std::vector<uint8_t>()).size() / 2 : 0;
  const int kcap = rsbw::kcap_of(b, kmax);
  const rsbk::LdsLayout L = rsbw::make_layout(b, kcap, n_self);
  out4[0] = L.ginv - L.g; out4[1] = kcap > 8 ? 0 : rsbk::g_row_pitch(kcap); out4[2] = rsbk::kGBlock; out4[3] = L.gstride;
  return kcap;
}
extern "C" int rsb_model_up_quads(const rsb_model* m, int* table, int capacity) {
  if (!m) { rsb::set_error("rsb_model_up_quads: null model"); return RSB_E_INVALID; }
  int t[16];
  const int levels = rsbw::up_quad_table(m->blob, t);
  if (table && capacity < 4 * levels) { rsb::set_error("rsb_model_up_quads: table too small"); return RSB_E_INVALID; }
  if (table) for (int i = 0; i < 4 * levels; ++i) table[i] = t[i];
  return levels;
}
extern "C" int rsb_model_col_own(const rsb_model* m, int kmax, int terrain_type, int self_collision, int lanes_per_env, int* prim, int* lower, float* sphere, int capacity) {
  if (!m || kmax < 1 || kmax > RSB_MAX_CONTACTS || (lanes_per_env != 0 && lanes_per_env != 16 && lanes_per_env != 32 && lanes_per_env != 64)) { rsb::set_error("rsb_model_col_own: bad argument"); return RSB_E_INVALID; }
  const rsb_model_blob& b = m->blob;
  const int n_self = self_collision ? (int)rsbw::enumerate_self_pairs(b, std::vector<uint8_t>()).size() / 2 : 0;
  const int lpe = lanes_per_env ? lanes_per_env : rsbw::default_lpe(b, kmax, n_self), kcap = rsbw::kcap_of(b, kmax);
  const rsbk::LdsLayout L = rsbw::make_layout(b, kcap, n_self);
  if (terrain_type != 0 || !rsbw::quad_forms_run(b, lpe, kcap, L)) return 0;
  int p[RSB_MAX_COLLISIONS + 16], lo[(RSB_MAX_COLLISIONS + 16) * 4];
  const int npass = rsbw::col_own_table(b, p, lo);
  if (capacity < 16 * npass && (prim || lower || sphere)) { rsb::set_error("rsb_model_col_own: tables too small"); return RSB_E_INVALID; }
  for (int e = 0; e < 16 * npass; ++e) {
    if (prim) prim[e] = p[e];
    if (lower) for (int u = 0; u < npass; ++u) lower[e * npass + u] = lo[e * npass + u];
    if (sphere) for (int k = 0; k < 4; ++k) sphere[4 * e + k] = p[e] < 0 ? 0.f : (k < 3 ? (float)b.col_pos[p[e]][k] : (float)b.col_radius[p[e]]);
  }
  return npass;
}
namespace rsbw {
int effective_lpe(const rsb_world* w) {
  int lpe = w->lpe > 0 ? w->lpe : default_lpe(w->blob, w->kmax, n_self_pairs(w));
  return lpe;
}

int check_lpe(const rsb_world* w, int lpe) {
  if (lpe != 16 && lpe != 32 && lpe != 64) { rsb::set_error("lanes_per_env must be 16, 32 or 64"); return RSB_E_INVALID; }
  if (lpe < w->blob.nb) { rsb::set_error("lanes_per_env must be >= number of moving bodies (lane = body in the tree passes)"); return RSB_E_INVALID; }
  const int kcap = kcap_of(w->blob, w->kmax);
  if (n_self_pairs(w) > 30 * lpe) { rsb::set_error("too many self-collision candidate pairs for this lanes_per_env (<= 30 per lane): exclude body pairs with rsb_ignore_collision_between or switch self-collision off"); return RSB_E_UNSUPPORTED; }
  if (lds_bytes_for(w->blob, kcap, lpe, n_self_pairs(w)) > 160 * 1024) { rsb::set_error("lanes_per_env too small: the workgroup's envs do not fit in 160 KiB of LDS"); return RSB_E_INVALID; }
  return RSB_OK;
}

bool instrumented(const rsb_world* w) {
  static const bool poison = std::getenv("RSB_POISON_LDS") != nullptr;  // debug aid, see tests/test_gpu_properties.py
  return w->d_prof || w->dbg_env >= 0 || poison;
}

// The kernel class a launch of this world runs: the features the world asks for as class bits (step_launch.h), the contact capacity and the
// support-chain capacity (ML) of its tree depth, looked up in the instance list.  A class exists if and only if it is listed; a launch whose
// class is not is refused with the reason of the feature that has none.
int choose_step_class(const rsb_world* w, const LaunchKind& k, StepClass* out) {
  const rsb_model_blob& b = w->blob;
  const bool resident = k.res_stage >= 0;
  const bool peer = resident ? w->peer.connected : k.peer;
  const bool hm2 = (w->hm_contacts >= 2 || (w->hm_capsule && w->n_cap > 0)) && w->terrain_type == 1;   // more than one contact per primitive against a height map
  const bool th = w->integ_theta != 1.0 && !k.rk4_contact, coul = w->slip_rule == RSB_SLIP_COULOMB;
  const int needs = (b.fixed_base ? 1 : 0) | (peer ? 2 : 0) | (hm2 ? 4 : 0) | (th ? 8 : 0) | (coul ? 32 : 0);
  const int mlv = b.depth - 1;
  StepClass c{effective_lpe(w), kcap_of(b, w->kmax), needs, mlv <= 4 ? 4 : mlv <= 12 ? 12 : mlv <= 16 ? 16 : 0, instrumented(w) ? 1 : 0};
  if (resident) {
    auto no = [](const char* why) { rsb::set_error(std::string("no resident launch for this world: ") + why); return RSB_E_UNSUPPORTED; };
    if (w->integ_rk4) return no("an integration scheme other than SEMI_IMPLICIT");
    if (c.prof) return no("profiling / debug instrumentation is active");
    if (w->N % (64 / c.lpe) != 0) return no("the number of envs is not a multiple of the envs per workgroup");
    const char* wide = "actor-network widths above 128 (humanoid-sized models) / 256";
    if (k.res_stage > 2) return no("unknown stage");
    if (k.res_stage == 2 && k.mlp_width > 256) return no(wide);
    c.cl |= 64 | (k.res_stage == 0 ? 0 : k.res_stage == 1 ? 128 : k.mlp_width <= 128 ? 256 : 384);     // + the action stage inside (stage_bodies.h)
    if (!find_instance(c)) {
      if (needs) return no(needs & 1 ? "fixed-base systems" : needs & 2 ? "the peer-mapped obs exchange is connected" : needs & 8 ? "an integration scheme other than SEMI_IMPLICIT"
                           : needs & 32 ? "RSB_SLIP_COULOMB" : "more than one contact per primitive against a height map");
      if (c.cl == (64 | 384) && find_instance(StepClass{c.lpe, c.kmax, 64, c.ml})) return no(wide);
      return no("compiled for tree depth <= 5 / <= 8 contact slots / 16 lanes per env and for tree depth <= 13 / 16 slots / 32 lanes per env");
    }
  } else {
    if (k.pipelined && !(needs & 2)) c.cl |= 16;      // the class's pipelined twin (StepArgs::pipe_prog): the plain instances carry none of its code
    const StepInstance* e = find_instance(c);
    if (!e) {
      rsb::set_error(th ? "integration schemes other than SEMI_IMPLICIT: built for floating-base systems of tree depth <= 13 without the peer-mapped obs exchange and with one contact per primitive"
                     : coul ? "RSB_SLIP_COULOMB: built for floating-base systems of tree depth <= 5 with <= 8 contact slots, the default integration scheme, one contact per primitive, no peer-mapped obs exchange"
                     : hm2 ? "two contacts per primitive against a height map: built for floating-base systems of tree depth <= 13 without the peer-mapped obs exchange"
                     : peer ? "the peer-mapped obs exchange is compiled for floating-base models of tree depth <= 13"
                     : "model outside the compiled kernel classes (tree depth <= 17)");
      return RSB_E_UNSUPPORTED;
    }
    // the profiling instance carries the cycle stamps / contact-problem dump / LDS poisoning; production launches use the lean one
    if (c.prof && !e->run_prof) { rsb::set_error("profiling / debug instrumentation is not built for the peer-exchange, the pipelined and the resident kernel classes: disconnect the exchange (rsb_obs_peer_destroy) / switch pipelining and residency off first"); return RSB_E_UNSUPPORTED; }
  }
  *out = c;
  return RSB_OK;
}

// what a pipelined step launch needs of the world: pipelining on, no instrumentation (the twins have no profiling build), no peer exchange, no env mask
bool pipelining_allowed(const rsb_world* w, bool peer, const uint8_t* mask) { return w->pipe_on && !instrumented(w) && !peer && !mask; }

LdsLayout world_layout(const rsb_world* w) { return make_layout(w->blob, kcap_of(w->blob, w->kmax), n_self_pairs(w)); }

// The per-block tables of the step kernel exactly as they sit in LDS (LdsLayout::t_*): the kernel copies this image with
// float4 loads instead of staging ten tables one latency-bound loop at a time.  Rebuilt when a setter changes what it bakes
// in: PD gains, control mode, contact materials - and for a launch of another layout (the model table's pitch follows the contact capacity: make_layout)
// or of the other kind: RUNGE_KUTTA_4's contact step (rk4_contact) runs in force mode, so without the gains, and without the effort clip.
std::vector<float> build_lds_image(const rsb_world* w, const LdsLayout& L, bool rk4_contact) {
  const rsb_model_blob& b = w->blob;
  auto dm = std::make_unique<DevModel>();
  build_dev_model(b, dm.get());
  std::vector<float> img((size_t)L.shared_total, 0.f);
  auto put_i = [&](int off, int v) { std::memcpy(&img[off], &v, sizeof(int)); };
  for (int i = 0; i < b.nb; ++i) {
    for (int c = 0; c < rsbk::kModelSlot; ++c) img[L.t_model + i * L.model_pitch + c] = dm->bodyf[i][c];
    if (rk4_contact) img[L.t_model + i * L.model_pitch + 28] = 0.f;      // (its generalized force carries inertial terms, the effort clip was applied in the stages)
    const bool pd = w->control_mode == RSB_PD_PLUS_FEEDFORWARD_TORQUE && !rk4_contact && i >= 1;
    img[L.t_gain + 2 * i] = pd ? w->h_kp[i + 5] : 0.f;
    img[L.t_gain + 2 * i + 1] = pd ? w->h_kd[i + 5] : 0.f;
    put_i(L.t_parlv + i, (b.parent[i] + 1) | (b.level[i] << 8));
    put_i(L.t_kids + i, dm->kid_list[i]);
    put_i(L.t_kidx + i, dm->kid_start[i] | (dm->kid_count[i] << 16));
  }
  for (int i = 0; i < b.nb * b.depth; ++i) put_i(L.t_anc + i, dm->anc[i]);
  for (int k = 0; k < 16; ++k) {   // slip-search bracket around grid point k: {cos, sin((k-1) pi/8), cos, sin((k+1) pi/8)}
    const double lo = ((k + 15) & 15) * 0.125 * M_PI, hi = ((k + 1) & 15) * 0.125 * M_PI;
    img[L.t_dir + 4 * k] = (float)std::cos(lo); img[L.t_dir + 4 * k + 1] = (float)std::sin(lo);
    img[L.t_dir + 4 * k + 2] = (float)std::cos(hi); img[L.t_dir + 4 * k + 3] = (float)std::sin(hi);
  }
  for (int i = 0; i < b.ncol; ++i) {
    float* ct = &img[L.t_col + rsbk::kColSlot * i];
    ct[0] = (float)b.col_pos[i][0]; ct[1] = (float)b.col_pos[i][1]; ct[2] = (float)b.col_pos[i][2]; ct[3] = (float)b.col_radius[i];
    put_i(L.t_col + rsbk::kColSlot * i + 4, b.col_body[i]);
    ct[8] = (float)b.col_axis[i][0]; ct[9] = (float)b.col_axis[i][1]; ct[10] = (float)b.col_axis[i][2]; ct[11] = (float)b.col_rim[i];
    // contact material of the primitive against the terrain: the per-primitive override where one is set, else the world's default
    ct[5] = (float)(w->col_mu[i] >= 0 ? w->col_mu[i] : w->mu);
    ct[6] = (float)(w->col_rest[i] >= 0 ? w->col_rest[i] : w->restitution);
    ct[7] = (float)(w->col_rthr[i] >= 0 ? w->col_rthr[i] : w->res_threshold);
  }
  // self-collision pairs as byte offsets into the centre table (16 B per primitive); the entry behind the list pairs primitive 0 with itself (never a hit)
  for (int k = 0; k < n_self_pairs(w); ++k) put_i(L.t_spair + k, (16 * w->self_pairs[2 * k]) | ((16 * w->self_pairs[2 * k + 1]) << 16));
  return img;
}

// the step kernel's per-block tables (build_lds_image) in layout L and the self-collision pairs' materials, re-uploaded when a setter dirtied them
// or the image was built for another layout or the other kind of launch.  Joins (stream_of): callers that must not join later - a closed-loop run with its action stage in
// flight - call it up front.
int upload_image(rsb_world* w, const LdsLayout& L, bool rk4_contact) {
  if (!w->image_dirty && rk4_contact == w->image_rk4_contact && std::memcmp(&L, &w->image_layout, sizeof L) == 0) return RSB_OK;
    std::vector<float> img = build_lds_image(w, L, rk4_contact);
    HIP_TRY(hipMemcpyAsync(w->d_image, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    const int np = n_self_pairs(w);
    std::vector<float> mat((size_t)4 * np, 0.f);
    for (int k = 0; k < np; ++k) {
      mat[4 * k] = (float)(w->self_mu[k] >= 0 ? w->self_mu[k] : w->mu);
      mat[4 * k + 1] = (float)(w->self_rest[k] >= 0 ? w->self_rest[k] : w->restitution);
      mat[4 * k + 2] = (float)(w->self_rthr[k] >= 0 ? w->self_rthr[k] : w->res_threshold);
    }
    if (np > 0) {
      if ((size_t)np > w->self_mat_cap) {
        if (w->d_self_mat) HIP_TRY(hipFree(w->d_self_mat));
        w->d_self_mat = nullptr; w->self_mat_cap = 0;
        HIP_TRY(hipMalloc(&w->d_self_mat, (size_t)4 * np * sizeof(float)));
        w->self_mat_cap = (size_t)np;
      }
      HIP_TRY(hipMemcpyAsync(w->d_self_mat, mat.data(), mat.size() * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    }
    HIP_TRY(hipStreamSynchronize(stream_of(w)));   // img / mat are stack-lifetime buffers
    w->image_dirty = false;
    w->image_layout = L; w->image_rk4_contact = rk4_contact;
  return RSB_OK;
}

// do_integrate, part 2: everything of StepArgs that follows from the world's configuration alone (L, c: the launch's layout and kernel class)
void fill_world_args(const rsb_world* w, const LdsLayout& L, const StepClass& c, StepArgs& a) {
  a.model = w->d_model;
  a.gc = w->d_gc; a.gv = w->d_gv; a.ptarget = w->d_pt; a.dtarget = w->d_dt; a.tauff = w->d_tff;
#ifndef RSB_X_READ_ZERO_ROWS      /* (A/B switch: read the rows although they are known to be zero, as rounds 1-4 did) */
  // (a field whose raw device pointer has been handed out - rsb_device_ptr - is read whatever the host thinks it holds: ADVICE r05)
  if (w->dt_zero && !w->raw_dt) a.dtarget = nullptr;
  if (w->tff_zero && !w->raw_tff) a.tauff = nullptr;
#endif
  a.kp = w->d_kp; a.kd = w->d_kd;
  a.contacts = w->d_contacts; a.contact_count = w->d_count; a.flags = w->d_flags; a.iters = w->d_iters;
  a.heights = w->d_heights;
  a.hm_index = w->d_hm_index;
  a.warm = w->warm_start ? w->d_warm : nullptr;
  a.lds_image = w->d_image; a.L = L; a.lds_floats = (int)(lds_bytes_of(L, c.lpe) / sizeof(float));
  a.gc0 = w->d_gc; a.gv0 = w->d_gv; a.reset_rows = w->N;      // (no reset: never dereferenced, but keep the pointers valid)
  a.tau_out = w->want_genf ? w->d_genf : nullptr;
  a.prof = w->d_prof;
  a.dbg = w->dbg_env >= 0 ? w->d_dbg : nullptr;
  a.dbg_env = w->dbg_env;
  a.N = w->N; a.kmax = w->kmax; a.control_mode = w->control_mode;
  a.nb = w->blob.nb; a.nq = w->blob.nq; a.nv = w->blob.nv; a.ncol = w->blob.ncol; a.depth = w->blob.depth;
  a.cw = round4(6 + w->blob.depth - 1); a.max_kid = w->max_kid; a.fixed_base = w->blob.fixed_base; a.chain = (w->chain && c.lpe == 16) ? 1 : 0;
  // (2: the quad form of the up pass - its 48-float hand-over slots need the square Delassus layout's rows to themselves: the packed layout keeps the joint factors there)
  // (... and the flat Delassus trip takes a body's limb and level from its index: the closed form is compared with the tree tables first)
  if (a.chain && c.kmax <= 8 && up_quad_table(w->blob, nullptr) > 0 && delassus_closed_form_ok(w->blob) && w->blob.nb * rsbk::kUpQuadSlot <= L.ginv - L.g) a.chain = 2;
  // own-lane form of the plane's collision test: the worlds of both quad forms, on the plane, with a table (rsb_create: the model has one)
  a.col_own = (a.chain == 2 && w->terrain_type == 0 && w->d_col_own != nullptr) ? 1 : 0;
  a.col_own_tab = w->d_col_own;
  a.dt = (float)w->dt; a.gx = (float)w->gravity[0]; a.gy = (float)w->gravity[1]; a.gz = (float)w->gravity[2];
  a.mu = (float)w->mu; a.erp = (float)w->erp;
  a.alpha_init = (float)w->alpha_init; a.alpha_min = (float)w->alpha_min; a.alpha_decay = (float)w->alpha_decay;
  a.threshold = (float)w->threshold; a.max_iter = w->max_iter; a.section_rounds = w->section_rounds;
  a.multi_depth = w->multi_depth; a.multi_light = w->multi_light; a.multi_freeze_after = w->multi_freeze_after; a.multi_stall_window = w->multi_stall_window;
  a.anderson = w->kmax > 8 ? w->anderson : 0;   // (rsb.h, oracle: worlds with kmax > 8 only - the large kernel classes also serve deep models at kmax <= 8)
  a.anderson_clip = (float)w->anderson_clip;
  a.hm_contacts = w->hm_contacts; a.hm_second_cos = (float)w->hm_second_cos; a.hm_slots = hm_slots_for(w->blob);
  a.hm_capsule = w->hm_capsule ? w->n_cap : 0; a.hm_cap = w->d_cap;
  a.integ_theta = (float)w->integ_theta;
  a.stall_window = w->stall_window; a.stall_factor = (float)w->stall_factor; a.freeze_after = w->freeze_after; a.refine = w->refine; a.settle_tol = (float)w->settle_tol; a.restitution = (float)w->restitution; a.res_threshold = (float)w->res_threshold;
  a.terrain_type = w->terrain_type; a.hm_xs = w->hm_xs; a.hm_ys = w->hm_ys; a.ground_z = (float)w->ground_z;
  if (w->terrain_type == 1) {
    double dx = w->hm_xsize / (w->hm_xs - 1), dy = w->hm_ysize / (w->hm_ys - 1);
    a.hm_x0 = (float)(w->hm_cx - 0.5 * w->hm_xsize); a.hm_y0 = (float)(w->hm_cy - 0.5 * w->hm_ysize);
    a.hm_dx = (float)dx; a.hm_dy = (float)dy; a.hm_inv_dx = (float)(1.0 / dx); a.hm_inv_dy = (float)(1.0 / dy);
    a.hm_max = w->hm_max;
  }
  a.n_self = n_self_pairs(w); a.self_mat = w->d_self_mat;
  static const bool poison = std::getenv("RSB_POISON_LDS") != nullptr;  // debug aid, see tests/test_gpu_properties.py
  a.poison_lds = poison ? 1 : 0;
  static const bool prof_fine = std::getenv("RSB_PROF_FINE") != nullptr;  // debug aid: also time searches / Newton steps / epilogues
  a.prof_fine = prof_fine ? 1 : 0;
}

// do_integrate, part 3: what THIS launch is asked for on top (a successful launch's only side effect on the world here: the peer exchange's step counter)
void apply_request(rsb_world* w, const StepRequest& f, StepArgs& a) {
  if (f.rk4_contact) { a.control_mode = RSB_FORCE_AND_TORQUE; a.integ_theta = 1.f; a.tauff = w->d_tff; }      // (tau_eff lives in d_tff for this launch)
  if (f.ptarget_src) { a.ptarget = f.ptarget_src; a.ptarget_store = w->d_pt; }
  if (f.act) { a.act = f.act; a.act_mean = w->d_env_mean; a.act_std = w->env_cfg.action_std; a.ptarget_store = w->d_pt; a.tau2_out = w->d_env_tau2; }
  if (f.env_task) {   // rsb_env_step: reward, termination, reset and the next observation in this launch's epilogue
    a.env_reward = f.env_reward; a.env_ob = f.env_ob;
    a.env_fwd_coeff = w->env_cfg.forward_vel_coeff; a.env_fwd_clip = w->env_cfg.forward_vel_clip;
    a.env_torque_coeff = w->env_cfg.torque_coeff; a.env_terminal_reward = w->env_cfg.terminal_reward;
    a.tau2_out = nullptr;
  }
  a.obs_out = f.obs_out; a.obs_idx = f.obs_idx; a.obs_slots = f.obs_slots;
  if (f.peer) {   // rsb_control_step with the peer-mapped obs exchange connected: rows go to every rank's gathered buffer of this step's parity
    rsb_world::Peer& P = w->peer;
    const uint32_t step = ++P.step;
    const int par = (int)(step & 1u);
    const size_t bufsz = (size_t)P.ranks * w->N * P.od;
    for (int p = 0; p < P.ranks; ++p) {
      float* pb = static_cast<float*>(P.peer_base[p]);
      a.obs_peer[p] = pb + (size_t)par * bufsz;
      a.obs_flag[p] = reinterpret_cast<uint32_t*>(pb + 2 * bufsz) + (size_t)par * RSB_MAX_RANKS + P.rank;
    }
    a.obs_ctr = reinterpret_cast<uint32_t*>(static_cast<float*>(P.base) + 2 * bufsz) + 2 * RSB_MAX_RANKS;
    a.n_obs_peers = P.ranks; a.obs_row0 = P.rank * w->N; a.obs_step = step;
    a.obs_slots = P.slots; a.obs_idx = P.idx.empty() ? nullptr : P.d_idx;
  }
  a.early_term = (w->early_term && f.have_allowed) ? 1 : 0; a.allowed = f.allowed;
  if (f.do_reset) { a.do_reset = f.do_reset; a.gc0 = f.gc0; a.gv0 = f.gv0; a.reset_rows = f.rows; }
  if (f.res_steps > 0) {
    a.res_steps = f.res_steps; a.res_full = w->res_full ? 1 : 0;
    a.res_targets = f.res_targets; a.res_period = f.res_period; a.res_first = f.res_first;
    a.res_obs_stride = f.res_obs_stride; a.res_done_stride = f.res_done_stride; a.res_pass_global0 = f.res_pass_global0;
    if (f.res_stage == 1) a.res_pol.lin = f.res_lin;
    if (f.res_stage == 2) a.res_pol.mlp = f.res_mlp;
    if (f.res_stage == 0) { a.ptarget = f.res_targets + (size_t)(f.res_first % f.res_period) * ((size_t)w->N * w->blob.nq); a.ptarget_store = w->d_pt; }
  }
  a.done_out = f.redirect_done ? f.done_out : w->d_done_out;
  a.env_mask = f.mask;
}

// do_integrate, part 4: the launch goes to its stream - one of the pipeline's private ones behind its gate (rsb_pipeline.hip), else the world's
int enqueue_step(rsb_world* w, const StepRequest& f, bool pipelined, const StepClass& c, StepArgs& a) {
  const int blocks = (w->N + 64 / c.lpe - 1) / (64 / c.lpe);
  hipStream_t ls = nullptr;
  if (pipelined) {
    int st = pipe_begin_launch(w, a, blocks, f.closed_loop, &ls);
    if (st != RSB_OK) return st;
    if (!f.closed_loop) {      // what a faulted pipeline replays in lock-step (pipe_recover); a closed-loop run has logged itself
      rsb_world::PipeLog e;
      e.req = f; e.nsub = a.nsub; e.req.pipeline = false;
      if (!f.redirect_done) { e.req.redirect_done = true; e.req.done_out = w->d_done_out; }      // (rsb_set_done_output does not join: the buffer of NOW)
      w->pipe_log.push_back(e);
    }
    w->pipe_time_logged += a.nsub * w->dt;
  } else {
    ls = stream_of(w);
    if (w->pipe_dep) { HIP_TRY(hipStreamWaitEvent(ls, w->pipe_dep, 0)); w->pipe_dep = nullptr; }
  }
  hipEvent_t e0 = w->ev0, e1 = w->ev1;
  const bool rec = w->timing && (w->launch_index++ % w->timing_stride == 0);
  if (rec && !w->ring0.empty()) { e0 = w->ring0[w->ring_next]; e1 = w->ring1[w->ring_next]; }
  if (rec) HIP_TRY(hipEventRecord(e0, ls));
  // a specialised code object of the class (rsb_spec.hip): same kernel, the model's dimensions and the world's switches as constants; else the ahead-of-time instance
  const size_t lds_bytes = lds_bytes_of(a.L, c.lpe);
  const hipFunction_t spec_fn = spec_find(w, c, a);
  const int st = spec_fn ? spec_launch(spec_fn, a, blocks, lds_bytes, ls) : launch_instance(c, a, blocks, lds_bytes, ls);
  if (st != RSB_OK) return st;
  ++(spec_fn ? w->spec_launches : w->generic_launches);
  if (f.res_steps > 0) ++w->res_launches;
  if (pipelined) pipe_end_launch(w, a, ls);
  if (rec) {
    HIP_TRY(hipEventRecord(e1, ls));
    if (!w->ring0.empty()) { w->ring_next = (w->ring_next + 1) % w->ring0.size(); if (w->ring_count < w->ring0.size()) ++w->ring_count; }
  }
  w->world_time += (double)std::max(f.res_steps, 1) * a.nsub * w->dt;
  w->integrate1_valid = false;
  // (the fused epilogue left the observation the NEXT step starts from in the world's own buffer - unless the caller holds raw pointers to the state rows
  //  and may write through them behind the library's back: then every closed-loop run recomputes its first observation, as the lock-step path does)
  w->env_ob_valid = a.env_ob != nullptr && a.env_ob == w->d_env_ob && !w->raw_state;
  return RSB_OK;
}

// EVERY launch of the step kernel.  What it should do beyond the world's configuration arrives in the request and nowhere else: a refused launch
// has written nothing to the world, and nothing on the world is rewritten for the duration of a launch.
int do_integrate(rsb_world* w, int nsub, const StepRequest& f) {
  HIP_TRY(hipSetDevice(w->device));
  if (w->integ_rk4 && !f.rk4_contact) return rk4_integrate(w, nsub, f);      // IntegrationScheme::RUNGE_KUTTA_4: host-driven over the query kernels (rsb_rk4.hip)
  int st = check_lpe(w, effective_lpe(w));
  if (st != RSB_OK) return st;
  // part 1, the kernel class: a resident launch runs K control steps in this ONE launch; a pipelined one goes to one of the two private streams, behind a
  // gate that lets it start only when the launch before it (on the other stream) has been dispatched completely - its workgroups wait for their
  // predecessors' envs (open loop) or for the action stage's rows (closed loop), which therefore must all be running or done (no deadlock: a waiting
  // workgroup never keeps a predecessor off the chip).  rsb_pipeline.hip holds the bookkeeping.
  const bool resident = f.res_steps > 0;
  LaunchKind kind;
  kind.peer = f.peer; kind.rk4_contact = f.rk4_contact;
  kind.pipelined = !resident && f.pipeline && (!f.env_task || f.closed_loop) && pipelining_allowed(w, f.peer, f.mask);
  if (resident) {
    kind.res_stage = f.res_stage;
    if (f.res_stage == 2) for (int l = 0; l <= f.res_mlp.n_layers; ++l) kind.mlp_width = std::max(kind.mlp_width, (int)f.res_mlp.dims[l]);
  }
  StepClass c;
  st = choose_step_class(w, kind, &c);
  if (st != RSB_OK) return st;
  if (resident && f.mask) { rsb::set_error("no resident launch with an env mask"); return RSB_E_UNSUPPORTED; }
  const LdsLayout L = world_layout(w);
  st = upload_image(w, L, f.rk4_contact);      // (joins - before the pipeline's bookkeeping begins)
  if (st != RSB_OK) return st;
  StepArgs a;
  std::memset(&a, 0, sizeof a);
  fill_world_args(w, L, c, a);
  apply_request(w, f, a);
  a.nsub = nsub;
  return enqueue_step(w, f, kind.pipelined, c, a);
}

// does a field the caller uploads hold nothing but zeros?  (host data: looked at; device data: unknown -> no)
bool all_zero(const float* src, size_t n, int space) {
  if (space != RSB_HOST) return false;
  for (size_t i = 0; i < n; ++i) if (src[i] != 0.f) return false;
  return true;
}
int copy_in(rsb_world* w, float* dst, const float* src, size_t n, int space) {
  HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), space == RSB_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream_of(w)));
  if (space == RSB_HOST) HIP_TRY(hipStreamSynchronize(stream_of(w)));  // the caller may reuse its host buffer
  return RSB_OK;
}
int copy_out(rsb_world* w, void* dst, const void* src, size_t bytes, int space) {
  hipStream_t s = stream_of(w);
  const int fs = fault_status(w);      // a read that joined a faulted pipeline says so ONCE (nothing is copied; the recovered state is there for the next call)
  if (fs != RSB_OK) return fs;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, space == RSB_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  if (space == RSB_HOST) HIP_TRY(hipStreamSynchronize(s));
  return RSB_OK;
}

// ONE launch per vectorised step of the env task: action -> PD targets in the prologue, control_dt / simulation_dt sub-steps, then reward,
// termination (non-foot contact or non-finite state), reset and the next observation in the epilogue
StepRequest env_task_request(const rsb_world* w, const float* act, float* reward, float* ob, uint8_t* done) {
  StepRequest f;
  f.act = act;
  f.have_allowed = 1; f.allowed = w->env_allowed;
  f.do_reset = 1; f.gc0 = w->d_env_gc0; f.gv0 = w->d_env_gv0; f.rows = 1;
  if (w->d_env_gc0_rows) { f.gc0 = w->d_env_gc0_rows; f.gv0 = w->d_env_gv0_rows; f.rows = w->N; }      // rsb_env_set_reset_states
  f.env_task = true; f.env_reward = reward; f.env_ob = ob; f.redirect_done = done != nullptr; f.done_out = done;
  return f;
}

// the (M, h) query kernel on the current state, into d_M / d_h (allocated at the first use)
int launch_mh_query(rsb_world* w, hipStream_t s) {
  const size_t N = w->N, nv = w->blob.nv;
  if (!w->d_M) {
    HIP_TRY(hipMalloc(&w->d_M, N * nv * nv * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_h, N * nv * sizeof(float)));
  }
  rsbq::QueryArgs qa;
  qa.model = w->d_model; qa.gc = w->d_gc; qa.gv = w->d_gv; qa.M = w->d_M; qa.h = w->d_h; qa.N = w->N;
  qa.gx = (float)w->gravity[0]; qa.gy = (float)w->gravity[1]; qa.gz = (float)w->gravity[2];
  return rsbq::launch_query(qa, w->blob.nb, s) == 0 ? RSB_OK : RSB_E_HIP;
}
int launch_dynamics_query(rsb_world* w, hipStream_t s) {
  const size_t N = w->N, nv = w->blob.nv;
  if (!w->d_Minv) {
    HIP_TRY(hipMalloc(&w->d_Minv, N * nv * nv * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_Mwork, N * nv * nv * sizeof(float)));
  }
  if (launch_mh_query(w, s) != RSB_OK) { rsb::set_error("RUNGE_KUTTA_4: query kernel launch failed"); return RSB_E_HIP; }
  hipLaunchKernelGGL(rsbq::rsb_minv_kernel, dim3((w->N + 63) / 64), dim3(64), 0, s, w->d_M, w->d_Mwork, w->d_Minv, w->N, w->blob.nv, w->blob.fixed_base ? 6 : 0);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}
int launch_env_obs(rsb_world* w, float* dst, hipStream_t s) {
  const int total = w->N * (10 + 2 * (w->blob.nv - 6));
  hipLaunchKernelGGL(env_obs_kernel, dim3((total + 255) / 256), dim3(256), 0, s, dst, w->d_gc, w->d_gv, w->N, w->blob.nq, w->blob.nv);
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rsb_create(const rsb_model* m, int num_envs, int device, rsb_world** out) {
  if (!m || !out || num_envs <= 0) { rsb::set_error("rsb_create: bad argument"); return RSB_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    rsb::set_error("rsb_create: no HIP device is visible (raisimlib_amd has no CPU fallback)");
    return RSB_E_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { rsb::set_error("rsb_create: device index out of range"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(device));
  // every early return below (HIP_TRY) goes through rsb_destroy, which frees whatever has been allocated so far
  struct Destroyer { void operator()(rsb_world* p) const { rsb_destroy(p); } };
  std::unique_ptr<rsb_world, Destroyer> w(new rsb_world());
  w->spec_mode = rsbw::spec_default_mode();
  w->blob = m->blob;
  w->N = num_envs;
  w->device = device;

  const int nq = w->blob.nq, nv = w->blob.nv;
  const size_t N = (size_t)num_envs;
  HIP_TRY(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&w->ev0));
  HIP_TRY(hipEventCreate(&w->ev1));
  auto dm = std::make_unique<DevModel>();
  build_dev_model(w->blob, dm.get());
  HIP_TRY(hipMalloc(&w->d_model, sizeof(DevModel)));
  HIP_TRY(hipMemcpy(w->d_model, dm.get(), sizeof(DevModel), hipMemcpyHostToDevice));
  w->max_kid = dm->max_kid;
  w->chain = w->blob.nb <= 16;
  for (int b = 1; b < w->blob.nb; ++b) if (dm->level[b] >= 2 && dm->parent[b] != b - 1) w->chain = false;
  HIP_TRY(hipMalloc(&w->d_gc, N * nq * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_gv, N * nv * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_pt, N * nq * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_dt, N * nv * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_tff, N * nv * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_kp, nv * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_kd, nv * sizeof(float)));
  HIP_TRY(hipMalloc(&w->d_contacts, N * RSB_MAX_CONTACTS * sizeof(rsb_contact)));
  HIP_TRY(hipMalloc(&w->d_count, N * sizeof(int32_t)));
  HIP_TRY(hipMalloc(&w->d_flags, N * sizeof(int32_t)));
  HIP_TRY(hipMalloc(&w->d_iters, N * sizeof(int32_t)));
  HIP_TRY(hipMalloc(&w->d_obs_idx, RSB_MAX_COLLISIONS * sizeof(int32_t)));
  HIP_TRY(hipMalloc(&w->d_image, (size_t)make_layout_pitch(w->blob, 8, w->blob.ncol * (w->blob.ncol - 1) / 2, rsbk::kModelPitch).shared_total * sizeof(float)));   // (room for every primitive pair)
  {      // the own-lane collision table: the model's alone, uploaded once (fill_world_args decides per launch whether the kernel uses it)
    const std::vector<float> own = col_own_image(w->blob);
    if (!own.empty()) {
      HIP_TRY(hipMalloc(&w->d_col_own, own.size() * sizeof(float)));
      HIP_TRY(hipMemcpy(w->d_col_own, own.data(), own.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  w->self_ignore.assign((size_t)w->blob.nb * w->blob.nb, 0);
  w->self_pairs = enumerate_self_pairs(w->blob, w->self_ignore);
  w->self_mu.assign(w->self_pairs.size() / 2, -1.0); w->self_rest = w->self_mu; w->self_rthr = w->self_mu;
  w->h_kp.assign(nv, 0.f); w->h_kd.assign(nv, 0.f);
  w->col_mu.assign(RSB_MAX_COLLISIONS, -1.0); w->col_rest.assign(RSB_MAX_COLLISIONS, -1.0); w->col_rthr.assign(RSB_MAX_COLLISIONS, -1.0);
  HIP_TRY(hipMalloc(&w->d_warm, N * (size_t)rsbk::kWarmRow * sizeof(float)));
  HIP_TRY(hipMemset(w->d_warm, 0, N * (size_t)rsbk::kWarmRow * sizeof(float)));
  HIP_TRY(hipMemset(w->d_gc, 0, N * nq * sizeof(float)));
  HIP_TRY(hipMemset(w->d_gv, 0, N * nv * sizeof(float)));
  HIP_TRY(hipMemset(w->d_pt, 0, N * nq * sizeof(float)));
  HIP_TRY(hipMemset(w->d_dt, 0, N * nv * sizeof(float)));
  HIP_TRY(hipMemset(w->d_tff, 0, N * nv * sizeof(float)));
  HIP_TRY(hipMemset(w->d_kp, 0, nv * sizeof(float)));
  HIP_TRY(hipMemset(w->d_kd, 0, nv * sizeof(float)));
  HIP_TRY(hipMemset(w->d_contacts, 0, N * RSB_MAX_CONTACTS * sizeof(rsb_contact)));
  HIP_TRY(hipMemset(w->d_count, 0, N * sizeof(int32_t)));
  HIP_TRY(hipMemset(w->d_flags, 0, N * sizeof(int32_t)));
  HIP_TRY(hipMemset(w->d_iters, 0, N * sizeof(int32_t)));
  // default state: identity orientation, everything else zero
  std::vector<float> gc(N * nq, 0.f);
  for (size_t e = 0; e < N; ++e) gc[e * nq + 3] = 1.f;
  HIP_TRY(hipMemcpy(w->d_gc, gc.data(), gc.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  *out = w.release();
  return RSB_OK;
}

int rsb_destroy(rsb_world* w) {
  if (!w) return RSB_OK;
  (void)hipSetDevice(w->device);
  if (w->stream) (void)hipStreamSynchronize(stream_of(w));
  (void)rsb_comm_destroy(w);
  (void)rsb_obs_peer_destroy(w);
  void* ptrs[] = {w->d_model, w->d_gc, w->d_gv, w->d_pt, w->d_dt, w->d_tff, w->d_kp, w->d_kd, w->d_heights,
                  w->d_tmp_gc, w->d_tmp_gv, w->d_tmp_mask, w->d_M, w->d_h, w->d_Minv, w->d_Mwork, w->d_obs_idx, w->d_dbg, w->d_prof, w->d_contacts,
                  w->d_env_mean, w->d_env_gc0, w->d_env_gv0, w->d_env_io, w->d_env_ob, w->d_env_reward, w->d_env_tau2, w->d_env_done, w->d_warm, w->d_image, w->d_self_mat, w->d_genf, w->d_hm_index, w->d_launch_mask, w->d_view_masks, w->d_cap, w->d_col_own, w->d_obs_local, w->d_obs_all,
                  w->d_count, w->d_flags, w->d_iters};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (hipEvent_t e : w->ring0) (void)hipEventDestroy(e);
  for (hipEvent_t e : w->ring1) (void)hipEventDestroy(e);
  if (w->ev0) (void)hipEventDestroy(w->ev0);
  if (w->ev1) (void)hipEventDestroy(w->ev1);
  pipe_destroy(w);
  if (w->d_rk) (void)hipFree(w->d_rk);
  if (w->d_env_act) (void)hipFree(w->d_env_act);
  if (w->d_env_gc0_rows) { (void)hipFree(w->d_env_gc0_rows); (void)hipFree(w->d_env_gv0_rows); }
  obs_stats_free(w);
  frames_free(w);
  ray_shapes_free(w);
  if (w->own_stream && w->stream) (void)hipStreamDestroy(w->stream);
  delete w;
  return RSB_OK;
}

int rsb_set_stream(rsb_world* w, void* hip_stream) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  if (w->own_stream && w->stream) HIP_TRY(hipStreamDestroy(w->stream));
  w->stream = (hipStream_t)hip_stream;  // NULL is the (legacy) default stream, a valid stream to borrow
  w->own_stream = false;
  return RSB_OK;
}
void* rsb_get_stream(rsb_world* w) { return w ? (void*)stream_of(w) : nullptr; }
int rsb_synchronize(rsb_world* w) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  return fault_status(w);
}

int rsb_num_envs(const rsb_world* w) { return w ? w->N : RSB_E_INVALID; }
int rsb_dims(const rsb_world* w, int* nb, int* nq, int* nv, int* ncol, int* kmax) {
  if (!w) return RSB_E_INVALID;
  if (nb) *nb = w->blob.nb;
  if (nq) *nq = w->blob.nq;
  if (nv) *nv = w->blob.nv;
  if (ncol) *ncol = w->blob.ncol;
  if (kmax) *kmax = w->kmax;
  return RSB_OK;
}

int rsb_set_timestep(rsb_world* w, double dt) {
  if (!w || !(dt > 0)) { rsb::set_error("rsb_set_timestep: dt must be positive"); return RSB_E_INVALID; }
  w->dt = dt;
  return RSB_OK;
}
double rsb_get_timestep(const rsb_world* w) { return w ? w->dt : 0.0; }
double rsb_get_world_time(const rsb_world* w) { return w ? w->world_time : 0.0; }
int rsb_set_gravity(rsb_world* w, const double g[3]) {
  if (!w || !g) return RSB_E_INVALID;
  for (int i = 0; i < 3; ++i) w->gravity[i] = g[i];
  return RSB_OK;
}
int rsb_set_erp(rsb_world* w, double erp) { if (!w) return RSB_E_INVALID; w->erp = erp; return RSB_OK; }
int rsb_set_friction(rsb_world* w, double mu) {
  if (!w || mu < 0) { rsb::set_error("rsb_set_friction: mu must be >= 0"); return RSB_E_INVALID; }
  w->mu = mu;
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_material(rsb_world* w, double mu, double restitution, double res_threshold) {
  if (!w || mu < 0 || restitution < 0 || restitution > 1 || res_threshold < 0) { rsb::set_error("rsb_set_material: mu >= 0, 0 <= restitution <= 1, res_threshold >= 0"); return RSB_E_INVALID; }
  w->mu = mu; w->restitution = restitution; w->res_threshold = res_threshold;
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_collision_materials(rsb_world* w, const double* mu, const double* restitution, const double* res_threshold) {
  if (!w) { rsb::set_error("rsb_set_collision_materials: null world"); return RSB_E_INVALID; }
  for (int i = 0; i < w->blob.ncol; ++i) {
    if (restitution && restitution[i] > 1.0) { rsb::set_error("rsb_set_collision_materials: restitution <= 1"); return RSB_E_INVALID; }
    if ((mu && !std::isfinite(mu[i])) || (restitution && !std::isfinite(restitution[i])) || (res_threshold && !std::isfinite(res_threshold[i]))) {
      rsb::set_error("rsb_set_collision_materials: non-finite material value"); return RSB_E_INVALID;
    }
  }
  for (int i = 0; i < w->blob.ncol; ++i) {
    w->col_mu[i] = mu ? mu[i] : -1.0;
    w->col_rest[i] = restitution ? restitution[i] : -1.0;
    w->col_rthr[i] = res_threshold ? res_threshold[i] : -1.0;
  }
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_self_collision(rsb_world* w, int enable) {
  if (!w) { rsb::set_error("rsb_set_self_collision: null world"); return RSB_E_INVALID; }
  w->self_collision = enable != 0;
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_ignore_collision_between(rsb_world* w, int body_a, int body_b) {
  if (!w || body_a < 0 || body_b < 0 || body_a >= w->blob.nb || body_b >= w->blob.nb) { rsb::set_error("rsb_ignore_collision_between: body index out of range"); return RSB_E_INVALID; }
  w->self_ignore[(size_t)body_a * w->blob.nb + body_b] = 1;
  w->self_ignore[(size_t)body_b * w->blob.nb + body_a] = 1;
  w->self_pairs = enumerate_self_pairs(w->blob, w->self_ignore);
  w->self_mu.assign(w->self_pairs.size() / 2, -1.0); w->self_rest = w->self_mu; w->self_rthr = w->self_mu;   // (the pair list changed: overrides are dropped)
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_self_collision_pairs(const rsb_world* w, int32_t* pairs, int capacity) {
  if (!w) { rsb::set_error("rsb_self_collision_pairs: null world"); return RSB_E_INVALID; }
  const int np = (int)w->self_pairs.size() / 2;
  for (int k = 0; pairs && k < np && k < capacity; ++k) { pairs[2 * k] = w->self_pairs[2 * k]; pairs[2 * k + 1] = w->self_pairs[2 * k + 1]; }
  return np;
}
int rsb_set_self_collision_materials(rsb_world* w, const double* mu, const double* restitution, const double* res_threshold) {
  if (!w) { rsb::set_error("rsb_set_self_collision_materials: null world"); return RSB_E_INVALID; }
  const size_t np = w->self_pairs.size() / 2;
  for (size_t k = 0; k < np; ++k) {
    if (restitution && restitution[k] > 1.0) { rsb::set_error("rsb_set_self_collision_materials: restitution <= 1"); return RSB_E_INVALID; }
    if ((mu && !std::isfinite(mu[k])) || (restitution && !std::isfinite(restitution[k])) || (res_threshold && !std::isfinite(res_threshold[k]))) {
      rsb::set_error("rsb_set_self_collision_materials: non-finite material value"); return RSB_E_INVALID;
    }
  }
  for (size_t k = 0; k < np; ++k) {
    w->self_mu[k] = mu ? mu[k] : -1.0;
    w->self_rest[k] = restitution ? restitution[k] : -1.0;
    w->self_rthr[k] = res_threshold ? res_threshold[k] : -1.0;
  }
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_contact_solver_param(rsb_world* w, double alpha_init, double alpha_min, double alpha_decay,
                                 int max_iter, double threshold) {
  if (!w || max_iter < 1 || !(threshold >= 0) || !(alpha_init > 0)) { rsb::set_error("rsb_set_contact_solver_param: bad argument"); return RSB_E_INVALID; }
  w->alpha_init = alpha_init; w->alpha_min = alpha_min; w->alpha_decay = alpha_decay;
  w->max_iter = max_iter; w->threshold = threshold;
  return RSB_OK;
}
int rsb_set_solver_stagnation_exit(rsb_world* w, int window, double factor) {
  if (!w || window < 0 || !(factor > 0)) { rsb::set_error("rsb_set_solver_stagnation_exit: window >= 0, factor > 0"); return RSB_E_INVALID; }
  w->stall_window = window; w->stall_factor = factor;
  return RSB_OK;
}
int rsb_set_solver_friction_lag(rsb_world* w, int freeze_after, int refine, double settle_tol) {
  if (!w || freeze_after < 0 || !(settle_tol >= 0.0)) { rsb::set_error("rsb_set_solver_friction_lag: freeze_after >= 0, settle_tol >= 0"); return RSB_E_INVALID; }
  w->freeze_after = freeze_after; w->refine = refine != 0; w->settle_tol = settle_tol;
  return RSB_OK;
}
int rsb_set_solver_multi_contact(rsb_world* w, int depth, int light_passes, int freeze_after, int stall_window) {
  if (!w || depth < 0 || freeze_after < 0 || stall_window < 0) { rsb::set_error("rsb_set_solver_multi_contact: depth, freeze_after, stall_window >= 0"); return RSB_E_INVALID; }
  w->multi_depth = depth; w->multi_light = light_passes != 0; w->multi_freeze_after = freeze_after; w->multi_stall_window = stall_window;
  return RSB_OK;
}
int rsb_set_solver_anderson(rsb_world* w, int first_sweep, double clip) {
  if (!w || first_sweep < 0 || !(clip > 0.0)) { rsb::set_error("rsb_set_solver_anderson: first_sweep >= 0 (0 = off), clip > 0"); return RSB_E_INVALID; }
  w->anderson = first_sweep; w->anderson_clip = clip;
  return RSB_OK;
}
int rsb_set_heightmap_contacts(rsb_world* w, int per_primitive, double min_angle_deg) {
  if (!w || per_primitive < 1 || per_primitive > 2 || !(min_angle_deg > 0.0 && min_angle_deg < 90.0)) {
    rsb::set_error("rsb_set_heightmap_contacts: per_primitive is 1 or 2, 0 < min_angle_deg < 90"); return RSB_E_INVALID;
  }
  w->hm_contacts = per_primitive; w->hm_second_cos = std::cos(min_angle_deg * 3.14159265358979323846 / 180.0);
  return RSB_OK;
}
int rsb_set_capsule_contacts(rsb_world* w, int on) {
  if (!w) { rsb::set_error("rsb_set_capsule_contacts: null world"); return RSB_E_INVALID; }
  if (on && !w->d_cap) {      // the end pairs of the model's capsules and cylinders (rsb_model_blob::col_capsule), once
    std::vector<int32_t> pairs;
    for (int s = 0; s < w->blob.ncol; ++s)
      if (w->blob.col_capsule[s] != 0) { pairs.push_back(s); pairs.push_back(w->blob.col_capsule[s] < 0 ? -1 : w->blob.col_capsule[s] - 1); }   // (s, -1): a box headed by corner s
    w->n_cap = (int)pairs.size() / 2;
    if (w->n_cap > 0) {
      HIP_TRY(hipSetDevice(w->device));
      HIP_TRY(hipMalloc(&w->d_cap, pairs.size() * sizeof(int32_t)));
      HIP_TRY(hipMemcpy(w->d_cap, pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
  }
  w->hm_capsule = on != 0;
  return RSB_OK;
}
int rsb_set_slip_rule(rsb_world* w, int rule) {
  if (!w || (rule != RSB_SLIP_ENERGY && rule != RSB_SLIP_COULOMB)) { rsb::set_error("rsb_set_slip_rule: RSB_SLIP_ENERGY or RSB_SLIP_COULOMB"); return RSB_E_INVALID; }
  w->slip_rule = rule;
  return RSB_OK;
}
int rsb_set_integration_scheme(rsb_world* w, int scheme) {
  if (!w) return RSB_E_INVALID;
  (void)stream_of(w);
  const bool was_rk4 = w->integ_rk4;
  w->integ_rk4 = false;
  if (scheme == RSB_INTEGRATION_SEMI_IMPLICIT) w->integ_theta = 1.0;
  else if (scheme == RSB_INTEGRATION_EULER) w->integ_theta = 0.0;
  else if (scheme == RSB_INTEGRATION_TRAPEZOID) w->integ_theta = 0.5;
  else if (scheme == RSB_INTEGRATION_RUNGE_KUTTA_4) { w->integ_theta = 1.0; w->integ_rk4 = true; }
  else { w->integ_rk4 = was_rk4; rsb::set_error("rsb_set_integration_scheme: unknown scheme"); return RSB_E_INVALID; }
  return RSB_OK;
}
int rsb_set_early_termination(rsb_world* w, int on) {
  if (!w) return RSB_E_INVALID;
  w->early_term = on != 0;
  return RSB_OK;
}
int rsb_set_solver_warm_start(rsb_world* w, int on) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  w->warm_start = on != 0;
  HIP_TRY(hipMemsetAsync(w->d_warm, 0, (size_t)w->N * rsbk::kWarmRow * sizeof(float), stream_of(w)));
  return RSB_OK;
}
int rsb_set_max_contacts(rsb_world* w, int kmax) {
  if (!w || kmax < 1 || kmax > RSB_MAX_CONTACTS) { rsb::set_error("rsb_set_max_contacts: 1..RSB_MAX_CONTACTS"); return RSB_E_INVALID; }
  w->kmax = kmax;
  return RSB_OK;
}
int rsb_set_lanes_per_env(rsb_world* w, int lanes) {
  if (!w) return RSB_E_INVALID;
  if (lanes != 0) { int st = check_lpe(w, lanes); if (st != RSB_OK) return st; }
  w->lpe = lanes;
  return RSB_OK;
}
int rsb_get_lanes_per_env(const rsb_world* w) { return w ? effective_lpe(w) : RSB_E_INVALID; }

int rsb_set_ground(rsb_world* w, double height) {
  if (!w) return RSB_E_INVALID;
  w->terrain_type = 0; w->ground_z = height;
  return RSB_OK;
}
int rsb_set_heightmaps(rsb_world* w, int n_maps, int xs, int ys, double x_size, double y_size, double cx, double cy,
                       const float* heights, const int32_t* env_map) {
  if (!w || !heights || n_maps < 1 || xs < 2 || ys < 2 || !(x_size > 0) || !(y_size > 0) || (n_maps > 1 && !env_map)) {
    rsb::set_error("rsb_set_heightmaps: bad argument");
    return RSB_E_INVALID;
  }
  if (env_map)
    for (int e = 0; e < w->N; ++e)
      if (env_map[e] < 0 || env_map[e] >= n_maps) { rsb::set_error("rsb_set_heightmaps: env_map entry out of range"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  if (w->d_heights) { HIP_TRY(hipFree(w->d_heights)); w->d_heights = nullptr; }
  if (w->d_hm_index) { HIP_TRY(hipFree(w->d_hm_index)); w->d_hm_index = nullptr; }
  const size_t n = (size_t)n_maps * xs * ys;
  HIP_TRY(hipMalloc(&w->d_heights, n * sizeof(float)));
  HIP_TRY(hipMemcpy(w->d_heights, heights, n * sizeof(float), hipMemcpyHostToDevice));
  if (env_map) {
    HIP_TRY(hipMalloc(&w->d_hm_index, (size_t)w->N * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(w->d_hm_index, env_map, (size_t)w->N * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  w->terrain_type = 1; w->hm_xs = xs; w->hm_ys = ys; w->hm_xsize = x_size; w->hm_ysize = y_size; w->hm_cx = cx; w->hm_cy = cy;
  w->hm_max = heights[0];   // highest sample of all maps: the narrow phase skips every sphere whose lowest point lies above it
  for (size_t i = 1; i < n; ++i) if (heights[i] > w->hm_max) w->hm_max = heights[i];
  return RSB_OK;
}
int rsb_set_heightmap(rsb_world* w, int xs, int ys, double x_size, double y_size, double cx, double cy, const float* heights) {
  return rsb_set_heightmaps(w, 1, xs, ys, x_size, y_size, cx, cy, heights, nullptr);
}

int rsb_set_state(rsb_world* w, const float* gc, const float* gv, const uint8_t* mask, int space) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N, nq = w->blob.nq, nv = w->blob.nv;
  w->integrate1_valid = false; w->env_ob_valid = false;
  const int n6 = rsbk::kWarmRow;
  if (!mask) {
    if (n6 > 0) hipLaunchKernelGGL(warm_clear_kernel, dim3((N * n6 + 255) / 256), dim3(256), 0, stream_of(w), w->d_warm, (const uint8_t*)nullptr, (int)N, n6);
    if (gc) { int st = copy_in(w, w->d_gc, gc, N * nq, space); if (st) return st; }
    if (gv) { int st = copy_in(w, w->d_gv, gv, N * nv, space); if (st) return st; }
    return RSB_OK;
  }
  const uint8_t* dmask = mask;
  const float *sgc = gc, *sgv = gv;
  if (space == RSB_HOST) {
    if (!w->d_tmp_gc) {
      HIP_TRY(hipMalloc(&w->d_tmp_gc, N * nq * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_gv, N * nv * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_mask, N));
    }
    HIP_TRY(hipMemcpyAsync(w->d_tmp_mask, mask, N, hipMemcpyHostToDevice, stream_of(w)));
    if (gc) HIP_TRY(hipMemcpyAsync(w->d_tmp_gc, gc, N * nq * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    if (gv) HIP_TRY(hipMemcpyAsync(w->d_tmp_gv, gv, N * nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    dmask = w->d_tmp_mask; sgc = gc ? w->d_tmp_gc : nullptr; sgv = gv ? w->d_tmp_gv : nullptr;
  }
  if (sgc) hipLaunchKernelGGL(masked_row_copy, dim3((N * nq + 255) / 256), dim3(256), 0, stream_of(w), w->d_gc, sgc, dmask, (int)N, (int)nq);
  if (sgv) hipLaunchKernelGGL(masked_row_copy, dim3((N * nv + 255) / 256), dim3(256), 0, stream_of(w), w->d_gv, sgv, dmask, (int)N, (int)nv);
  if (n6 > 0) hipLaunchKernelGGL(warm_clear_kernel, dim3((N * n6 + 255) / 256), dim3(256), 0, stream_of(w), w->d_warm, dmask, (int)N, n6);
  HIP_TRY(hipGetLastError());
  if (space == RSB_HOST) HIP_TRY(hipStreamSynchronize(stream_of(w)));
  return RSB_OK;
}

int rsb_get_state(rsb_world* w, float* gc, float* gv, int space) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  if (gc) { int st = copy_out(w, gc, w->d_gc, N * w->blob.nq * sizeof(float), space); if (st) return st; }
  if (gv) { int st = copy_out(w, gv, w->d_gv, N * w->blob.nv * sizeof(float), space); if (st) return st; }
  return RSB_OK;
}

static int env_row(rsb_world* w, int field, int env, float** base, size_t* dim) {
  if (!w || env < 0 || env >= w->N) { rsb::set_error("env row: env index out of range"); return RSB_E_INVALID; }
  switch (field) {
    case RSB_F_GC: *base = w->d_gc; *dim = w->blob.nq; break;
    case RSB_F_GV: *base = w->d_gv; *dim = w->blob.nv; break;
    case RSB_F_PTARGET: *base = w->d_pt; *dim = w->blob.nq; break;
    case RSB_F_DTARGET: *base = w->d_dt; *dim = w->blob.nv; break;
    case RSB_F_TAU_FF: *base = w->d_tff; *dim = w->blob.nv; break;
    case RSB_F_GENERALIZED_FORCE:
      if (!w->want_genf || !w->d_genf) { rsb::set_error("RSB_F_GENERALIZED_FORCE: call rsb_enable_generalized_force_output first"); return RSB_E_INVALID; }
      *base = w->d_genf; *dim = w->blob.nv; break;
    default: rsb::set_error("env row: unsupported field"); return RSB_E_INVALID;
  }
  return RSB_OK;
}
int rsb_set_env_row(rsb_world* w, int field, int env, const float* data) {
  float* base; size_t dim;
  if (field == RSB_F_GENERALIZED_FORCE) { rsb::set_error("RSB_F_GENERALIZED_FORCE is an output"); return RSB_E_INVALID; }
  int st = env_row(w, field, env, &base, &dim);
  if (st != RSB_OK || !data) return st != RSB_OK ? st : RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipMemcpyAsync(base + (size_t)env * dim, data, dim * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  if ((field == RSB_F_GC || field == RSB_F_GV) && w->blob.ncol > 0)   // the env's state was overwritten: its solver state is stale
    HIP_TRY(hipMemsetAsync(w->d_warm + (size_t)env * rsbk::kWarmRow, 0, (size_t)rsbk::kWarmRow * sizeof(float), stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  if (field == RSB_F_DTARGET && !all_zero(data, dim, RSB_HOST)) w->dt_zero = false;
  if (field == RSB_F_TAU_FF && !all_zero(data, dim, RSB_HOST)) w->tff_zero = false;
  w->integrate1_valid = false; w->env_ob_valid = false;
  return RSB_OK;
}
int rsb_get_env_row(rsb_world* w, int field, int env, float* data) {
  float* base; size_t dim;
  int st = env_row(w, field, env, &base, &dim);
  if (st != RSB_OK || !data) return st != RSB_OK ? st : RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipMemcpyAsync(data, base + (size_t)env * dim, dim * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  return RSB_OK;
}

int rsb_get_field(rsb_world* w, int field, float* out, int space) {
  float* base; size_t dim;
  int st = env_row(w, field, 0, &base, &dim);
  if (st != RSB_OK || !out) return st != RSB_OK ? st : RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  return copy_out(w, out, base, (size_t)w->N * dim * sizeof(float), space);
}

int rsb_enable_generalized_force_output(rsb_world* w, int on) {
  if (!w) { rsb::set_error("rsb_enable_generalized_force_output: null world"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  if (on && !w->d_genf) {
    const size_t bytes = (size_t)w->N * w->blob.nv * sizeof(float);
    HIP_TRY(hipMalloc(&w->d_genf, bytes));
    HIP_TRY(hipMemset(w->d_genf, 0, bytes));
  }
  w->want_genf = on != 0;
  return RSB_OK;
}
int rsb_set_control_mode(rsb_world* w, int mode) {
  if (!w || (mode != RSB_FORCE_AND_TORQUE && mode != RSB_PD_PLUS_FEEDFORWARD_TORQUE)) { rsb::set_error("rsb_set_control_mode: unknown mode"); return RSB_E_INVALID; }
  w->control_mode = mode;
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_pd_gains(rsb_world* w, const float* kp, const float* kd) {
  if (!w || !kp || !kd) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipMemcpyAsync(w->d_kp, kp, w->blob.nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  HIP_TRY(hipMemcpyAsync(w->d_kd, kd, w->blob.nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  w->h_kp.assign(kp, kp + w->blob.nv); w->h_kd.assign(kd, kd + w->blob.nv);
  w->image_dirty = true;
  return RSB_OK;
}
int rsb_set_pd_target(rsb_world* w, const float* p_target, const float* d_target, int space) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  if (p_target) { int st = copy_in(w, w->d_pt, p_target, N * w->blob.nq, space); if (st) return st; }
  if (d_target) { int st = copy_in(w, w->d_dt, d_target, N * w->blob.nv, space); if (st) return st; w->dt_zero = all_zero(d_target, N * w->blob.nv, space); }
  return RSB_OK;
}
int rsb_set_generalized_force(rsb_world* w, const float* tau, int space) {
  if (!w || !tau) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  w->tff_zero = all_zero(tau, (size_t)w->N * w->blob.nv, space);
  return copy_in(w, w->d_tff, tau, (size_t)w->N * w->blob.nv, space);
}

int rsb_integrate(rsb_world* w, int n_substeps) {
  if (!w || n_substeps < 1) { rsb::set_error("rsb_integrate: n_substeps must be >= 1"); return RSB_E_INVALID; }
  return do_integrate(w, n_substeps, StepRequest());
}

int rsb_integrate_masked(rsb_world* w, int n_substeps, const uint8_t* mask, int space) {
  if (!w || n_substeps < 1 || !mask) { rsb::set_error("rsb_integrate_masked: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  const uint8_t* dmask = mask;
  if (space == RSB_HOST) {
    if (!w->d_launch_mask) HIP_TRY(hipMalloc(&w->d_launch_mask, (size_t)w->N));
    HIP_TRY(hipMemcpyAsync(w->d_launch_mask, mask, (size_t)w->N, hipMemcpyHostToDevice, stream_of(w)));
    HIP_TRY(hipStreamSynchronize(stream_of(w)));   // pageable host memory: the caller may reuse its buffer
    dmask = w->d_launch_mask;
  }
  StepRequest req;
  req.mask = dmask;
  return do_integrate(w, n_substeps, req);
}

int rsb_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) { rsb::set_error("rsb_host_alloc: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return RSB_OK;
}
int rsb_host_free(void* p) {
  if (p) HIP_TRY(hipHostFree(p));
  return RSB_OK;
}
int rsb_device_alloc(rsb_world* w, size_t bytes, void** out) {
  if (!w || !out || bytes == 0) { rsb::set_error("rsb_device_alloc: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipMalloc(out, bytes));
  return RSB_OK;
}
int rsb_device_free(rsb_world* w, void* p) {
  if (!w) { rsb::set_error("rsb_device_free: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  if (p) { HIP_TRY(hipStreamSynchronize(stream_of(w))); HIP_TRY(hipFree(p)); }
  return RSB_OK;
}
int rsb_device_copy(rsb_world* w, void* dst, const void* src, size_t bytes, int kind) {
  if (!w || !dst || !src || (kind != 0 && kind != 1)) { rsb::set_error("rsb_device_copy: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t st = stream_of(w);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return fault_status(w);
}

// One flush of the facade's per-env views: uploads, launches and downloads queued on the world's stream, ONE synchronisation at the end.
int rsb_view_exchange(rsb_world* w, const rsb_view_io* io) {
  if (!w || !io || io->n_launches < 0 || (io->n_launches > 0 && !io->launch_substeps)) { rsb::set_error("rsb_view_exchange: bad argument"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N, nq = w->blob.nq, nv = w->blob.nv;
  // host-side cost of the exchange by part (rsb_debug_view_profile): [0] enqueue of the uploads, [1] of the launches, [2] of the downloads, [3] the wait
  const auto tp0 = std::chrono::steady_clock::now();
  auto lap_ns = [](std::chrono::steady_clock::time_point& t) { const auto n = std::chrono::steady_clock::now(); const long long d = std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count(); t = n; return d; };
  auto tp = tp0;
  if (io->p_target) HIP_TRY(hipMemcpyAsync(w->d_pt, io->p_target, N * nq * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  if (io->d_target) { HIP_TRY(hipMemcpyAsync(w->d_dt, io->d_target, N * nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w))); w->dt_zero = false; }      // (staged rows of the views: not scanned)
  if (io->tau_ff) { HIP_TRY(hipMemcpyAsync(w->d_tff, io->tau_ff, N * nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w))); w->tff_zero = false; }
  if (io->gc || io->gv) {
    if (!io->state_mask) { rsb::set_error("rsb_view_exchange: state rows need state_mask"); return RSB_E_INVALID; }
    if (!w->d_tmp_gc) {
      HIP_TRY(hipMalloc(&w->d_tmp_gc, N * nq * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_gv, N * nv * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_mask, N));
    }
    HIP_TRY(hipMemcpyAsync(w->d_tmp_mask, io->state_mask, N, hipMemcpyHostToDevice, stream_of(w)));
    if (io->gc) {
      HIP_TRY(hipMemcpyAsync(w->d_tmp_gc, io->gc, N * nq * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
      hipLaunchKernelGGL(masked_row_copy, dim3((N * nq + 255) / 256), dim3(256), 0, stream_of(w), w->d_gc, (const float*)w->d_tmp_gc, (const uint8_t*)w->d_tmp_mask, (int)N, (int)nq);
    }
    if (io->gv) {
      HIP_TRY(hipMemcpyAsync(w->d_tmp_gv, io->gv, N * nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
      hipLaunchKernelGGL(masked_row_copy, dim3((N * nv + 255) / 256), dim3(256), 0, stream_of(w), w->d_gv, (const float*)w->d_tmp_gv, (const uint8_t*)w->d_tmp_mask, (int)N, (int)nv);
    }
    hipLaunchKernelGGL(warm_clear_kernel, dim3((N * rsbk::kWarmRow + 255) / 256), dim3(256), 0, stream_of(w), w->d_warm, (const uint8_t*)w->d_tmp_mask, (int)N, rsbk::kWarmRow);
    HIP_TRY(hipGetLastError());
    w->integrate1_valid = false; w->env_ob_valid = false;
  }
  if (io->n_launches > 0 && io->launch_masks) {
    const size_t need = (size_t)io->n_launches * N;
    if (w->view_masks_cap < need) {
      if (w->d_view_masks) HIP_TRY(hipFree(w->d_view_masks));
      w->d_view_masks = nullptr; w->view_masks_cap = 0;
      HIP_TRY(hipMalloc(&w->d_view_masks, need));
      w->view_masks_cap = need;
    }
    HIP_TRY(hipMemcpyAsync(w->d_view_masks, io->launch_masks, need, hipMemcpyHostToDevice, stream_of(w)));
  }
  w->view_prof[0] += lap_ns(tp);
  for (int i = 0; i < io->n_launches; ++i) {
    if (io->launch_substeps[i] < 1) { rsb::set_error("rsb_view_exchange: launch_substeps must be >= 1"); return RSB_E_INVALID; }
    StepRequest req;
    if (io->launch_masks) req.mask = w->d_view_masks + (size_t)i * N;
    const int st = do_integrate(w, io->launch_substeps[i], req);
    if (st != RSB_OK) return st;
  }
  w->view_prof[1] += lap_ns(tp);
  if (io->gc_out) HIP_TRY(hipMemcpyAsync(io->gc_out, w->d_gc, N * nq * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
  if (io->gv_out) HIP_TRY(hipMemcpyAsync(io->gv_out, w->d_gv, N * nv * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
  if (io->contact_counts) HIP_TRY(hipMemcpyAsync(io->contact_counts, w->d_count, N * sizeof(int32_t), hipMemcpyDeviceToHost, stream_of(w)));
  if (io->contacts) HIP_TRY(hipMemcpyAsync(io->contacts, w->d_contacts, N * w->kmax * sizeof(rsb_contact), hipMemcpyDeviceToHost, stream_of(w)));
  if (io->generalized_force) {
    if (!w->want_genf || !w->d_genf) { rsb::set_error("rsb_view_exchange: generalized_force needs rsb_enable_generalized_force_output"); return RSB_E_INVALID; }
    HIP_TRY(hipMemcpyAsync(io->generalized_force, w->d_genf, N * nv * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
  }
  w->view_prof[2] += lap_ns(tp);
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  w->view_prof[3] += lap_ns(tp);
  ++w->view_prof[4];
  return RSB_OK;
}
int rsb_debug_view_profile(rsb_world* w, long long out[5], int reset) {
  if (!w) return RSB_E_INVALID;
  if (out) for (int i = 0; i < 5; ++i) out[i] = w->view_prof[i];
  if (reset) for (int i = 0; i < 5; ++i) w->view_prof[i] = 0;
  return RSB_OK;
}

int rsb_set_done_output(rsb_world* w, uint8_t* done_device) {
  if (!w) return RSB_E_INVALID;
  w->d_done_out = done_device;
  return RSB_OK;
}

// integrate1(): collision detection + M, h for the CURRENT state, into query buffers.  The state is
// not advanced; integrate2() then runs the fused step (which recomputes the same quantities from the
// unchanged state, so the pair is equivalent to integrate()).
int rsb_integrate1(rsb_world* w) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  if (launch_mh_query(w, stream_of(w)) != RSB_OK) { rsb::set_error("integrate1: query kernel launch failed"); return RSB_E_HIP; }
  w->integrate1_valid = true;
  return RSB_OK;
}
int rsb_integrate2(rsb_world* w) {
  if (!w) return RSB_E_INVALID;
  return do_integrate(w, 1, StepRequest());
}

int rsb_get_contacts(rsb_world* w, int32_t* counts, rsb_contact* contacts, int space) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N;
  if (counts) { int st = copy_out(w, counts, w->d_count, N * sizeof(int32_t), space); if (st) return st; }
  if (contacts) { int st = copy_out(w, contacts, w->d_contacts, N * w->kmax * sizeof(rsb_contact), space); if (st) return st; }
  return RSB_OK;
}
int rsb_get_mass_matrix(rsb_world* w, float* M, int space) {
  if (!w || !M) return RSB_E_INVALID;
  if (!w->integrate1_valid) { rsb::set_error("rsb_get_mass_matrix: call rsb_integrate1 first (state changed since)"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  return copy_out(w, M, w->d_M, (size_t)w->N * w->blob.nv * w->blob.nv * sizeof(float), space);
}
int rsb_get_inverse_mass_matrix(rsb_world* w, float* Minv, int space) {
  if (!w || !Minv) return RSB_E_INVALID;
  if (!w->integrate1_valid) { rsb::set_error("rsb_get_inverse_mass_matrix: call rsb_integrate1 first (state changed since)"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  const size_t n = (size_t)w->N * w->blob.nv * w->blob.nv;
  if (!w->d_Minv) {
    HIP_TRY(hipMalloc(&w->d_Minv, n * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_Mwork, n * sizeof(float)));
  }
  hipLaunchKernelGGL(rsbq::rsb_minv_kernel, dim3((w->N + 63) / 64), dim3(64), 0, stream_of(w), w->d_M, w->d_Mwork, w->d_Minv, w->N, w->blob.nv, w->blob.fixed_base ? 6 : 0);
  HIP_TRY(hipGetLastError());
  return copy_out(w, Minv, w->d_Minv, n * sizeof(float), space);
}
int rsb_get_nonlinearities(rsb_world* w, float* h, int space) {
  if (!w || !h) return RSB_E_INVALID;
  if (!w->integrate1_valid) { rsb::set_error("rsb_get_nonlinearities: call rsb_integrate1 first (state changed since)"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  return copy_out(w, h, w->d_h, (size_t)w->N * w->blob.nv * sizeof(float), space);
}
int rsb_get_flags(rsb_world* w, int32_t* flags, int space) {
  if (!w || !flags) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  return copy_out(w, flags, w->d_flags, (size_t)w->N * sizeof(int32_t), space);
}
int rsb_get_solver_iterations(rsb_world* w, int32_t* iters, int space) {
  if (!w || !iters) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  return copy_out(w, iters, w->d_iters, (size_t)w->N * sizeof(int32_t), space);
}

}  // extern "C"
namespace {
// The index list is tiny and normally the same every control step: a pageable H2D copy per call would put a
// host-side staging round trip on the stream each step, so it is re-uploaded only when it changes.
int upload_obs_idx(rsb_world* w, const int32_t* idx, int n) {
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= w->blob.ncol) { rsb::set_error("collision index out of range"); return RSB_E_INVALID; }
  if ((int)w->obs_idx_host.size() != n || std::memcmp(w->obs_idx_host.data(), idx, n * sizeof(int32_t)) != 0) {
    w->obs_idx_host.assign(idx, idx + n);
    HIP_TRY(hipMemcpyAsync(w->d_obs_idx, w->obs_idx_host.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, stream_of(w)));
    HIP_TRY(hipStreamSynchronize(stream_of(w)));
  }
  return RSB_OK;
}
// the parts of a control step's request that rsb_control_step and rsb_control_steps share: the observation block gathered in the epilogue ...
int request_obs(rsb_world* w, float* obs_out, const int32_t* force_collisions, int n_force_slots, StepRequest* f) {
  if (!obs_out) return RSB_OK;
  f->obs_out = obs_out; f->obs_slots = n_force_slots;
  if (force_collisions && n_force_slots > 0) {
    int st = upload_obs_idx(w, force_collisions, n_force_slots);
    if (st != RSB_OK) return st;
    f->obs_idx = w->d_obs_idx;
  }
  return RSB_OK;
}
// ... and the reset of the envs that touched the ground with a primitive outside the allowed set (who: the caller's name in the error message)
int request_reset(const rsb_world* w, const char* who, const int32_t* allowed_collisions, int n_allowed, const float* gc0, const float* gv0, int rows, StepRequest* f) {
  if (!gc0) return RSB_OK;
  unsigned long long allowed = 0;
  for (int i = 0; i < n_allowed; ++i) {
    if (allowed_collisions[i] < 0 || allowed_collisions[i] >= w->blob.ncol) { rsb::set_error(std::string(who) + ": collision index out of range"); return RSB_E_INVALID; }
    allowed |= 1ull << allowed_collisions[i];
  }
  f->do_reset = 1; f->have_allowed = 1; f->allowed = allowed; f->gc0 = gc0; f->gv0 = gv0; f->rows = rows;
  return RSB_OK;
}
}  // namespace
extern "C" {

int rsb_obs_dim(const rsb_world* w, int n_force_slots) {
  if (!w || n_force_slots < 0 || n_force_slots > RSB_MAX_COLLISIONS) return RSB_E_INVALID;
  return w->blob.nq + w->blob.nv + 3 * n_force_slots;
}
int rsb_gather_obs(rsb_world* w, float* out, const int32_t* collision_indices, int n_force_slots, int space) {
  if (!w || !out || n_force_slots < 0 || n_force_slots > RSB_MAX_COLLISIONS) { rsb::set_error("rsb_gather_obs: bad argument"); return RSB_E_INVALID; }
  if (space != RSB_DEVICE && space != RSB_HOST) { rsb::set_error("rsb_gather_obs: space must be RSB_DEVICE or RSB_HOST"); return RSB_E_INVALID; }
  HIP_TRY(hipSetDevice(w->device));
  if (space == RSB_HOST) {   // slow path (C hosts without a device allocator, tests): gathered on the device, then copied out
    const size_t local = (size_t)w->N * (w->blob.nq + w->blob.nv + 3 * n_force_slots);
    if (w->obs_local_cap < local) {
      if (w->d_obs_local) HIP_TRY(hipFree(w->d_obs_local));
      w->d_obs_local = nullptr; w->obs_local_cap = 0;
      HIP_TRY(hipMalloc(&w->d_obs_local, local * sizeof(float)));
      w->obs_local_cap = local;
    }
    const int st = rsb_gather_obs(w, w->d_obs_local, collision_indices, n_force_slots, RSB_DEVICE);
    if (st != RSB_OK) return st;
    return copy_out(w, out, w->d_obs_local, local * sizeof(float), RSB_HOST);
  }
  const int32_t* didx = nullptr;
  if (collision_indices && n_force_slots > 0) {
    int st = upload_obs_idx(w, collision_indices, n_force_slots);
    if (st != RSB_OK) return st;
    didx = w->d_obs_idx;
  }
  const int od = w->blob.nq + w->blob.nv + 3 * n_force_slots;
  const size_t total = (size_t)w->N * od;
  hipLaunchKernelGGL(gather_obs_kernel, dim3((total + 255) / 256), dim3(256), 0, stream_of(w), out, w->d_gc, w->d_gv,
                     w->d_contacts, w->d_count, didx, w->N, w->blob.nq, w->blob.nv, w->kmax, n_force_slots,
                     (float)(1.0 / w->dt));
  HIP_TRY(hipGetLastError());
  return RSB_OK;
}

int rsb_reset_terminated(rsb_world* w, const int32_t* allowed_collisions, int n_allowed, const float* gc0,
                         const float* gv0, int rows, uint8_t* done, int space) {
  if (!w || !gc0 || !gv0 || (rows != 1 && rows != w->N) || n_allowed < 0 || (n_allowed > 0 && !allowed_collisions)) {
    rsb::set_error("rsb_reset_terminated: bad argument");
    return RSB_E_INVALID;
  }
  HIP_TRY(hipSetDevice(w->device));
  unsigned long long allowed = 0;
  for (int i = 0; i < n_allowed; ++i) {
    if (allowed_collisions[i] < 0 || allowed_collisions[i] >= w->blob.ncol) { rsb::set_error("rsb_reset_terminated: collision index out of range"); return RSB_E_INVALID; }
    allowed |= 1ull << allowed_collisions[i];
  }
  const size_t N = w->N, nq = w->blob.nq, nv = w->blob.nv;
  const float *dgc0 = gc0, *dgv0 = gv0;
  uint8_t* ddone = done;
  if (space == RSB_HOST) {
    if (!w->d_tmp_gc) {
      HIP_TRY(hipMalloc(&w->d_tmp_gc, N * nq * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_gv, N * nv * sizeof(float)));
      HIP_TRY(hipMalloc(&w->d_tmp_mask, N));
    }
    HIP_TRY(hipMemcpyAsync(w->d_tmp_gc, gc0, (size_t)rows * nq * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    HIP_TRY(hipMemcpyAsync(w->d_tmp_gv, gv0, (size_t)rows * nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    dgc0 = w->d_tmp_gc; dgv0 = w->d_tmp_gv; ddone = done ? w->d_tmp_mask : nullptr;
  }
  hipLaunchKernelGGL(reset_terminated_kernel, dim3((N + 255) / 256), dim3(256), 0, stream_of(w), w->d_gc, w->d_gv, w->d_contacts,
                     w->d_count, w->d_flags, allowed, dgc0, dgv0, rows, ddone, (int)N, (int)nq, (int)nv, w->kmax, w->d_warm, rsbk::kWarmRow);
  HIP_TRY(hipGetLastError());
  w->integrate1_valid = false; w->env_ob_valid = false;
  if (space == RSB_HOST) {
    if (done) HIP_TRY(hipMemcpyAsync(done, w->d_tmp_mask, N, hipMemcpyDeviceToHost, stream_of(w)));
    HIP_TRY(hipStreamSynchronize(stream_of(w)));
  }
  return RSB_OK;
}

// One control step of a vectorised env, enqueued with a single call: PD targets in, n_substeps x integrate(),
// observation block out, terminated envs reset.  All pointers are device pointers; nothing synchronises.
// (done_out: where THIS step's done flags go instead of the world's rsb_set_done_output buffer; NULL: there)
static int control_step(rsb_world* w, const float* p_target, const float* d_target, int n_substeps, float* obs_out,
                        const int32_t* force_collisions, int n_force_slots, const int32_t* allowed_collisions,
                        int n_allowed, const float* gc0, const float* gv0, int rows, uint8_t* done_out) {
  if (!w || n_substeps < 1 || n_force_slots < 0 || n_force_slots > RSB_MAX_COLLISIONS || n_allowed < 0 ||
      (n_allowed > 0 && !allowed_collisions) || ((gc0 != nullptr) != (gv0 != nullptr)) || (gc0 && rows != 1 && rows != w->N)) {
    rsb::set_error("rsb_control_step: bad argument");
    return RSB_E_INVALID;
  }
  HIP_TRY(hipSetDevice(w->device));
  if (w->peer.connected) {     // (refused before anything is written: whether the exchange has a kernel class for this world)
    StepClass c;
    LaunchKind k;
    k.peer = true;
    int st = check_lpe(w, effective_lpe(w));
    if (st == RSB_OK) st = choose_step_class(w, k, &c);
    if (st != RSB_OK) return st;
  }
  if (d_target) { int st = copy_in(w, w->d_dt, d_target, (size_t)w->N * w->blob.nv, RSB_DEVICE); if (st) return st; w->dt_zero = false; }
  StepRequest f;
  f.ptarget_src = p_target;   // read in place by the launch, which also refreshes the world's own copy
  f.pipeline = p_target != nullptr && d_target == nullptr;   // (rsb_set_step_pipelining: control steps that upload nothing may overlap)
  if (w->peer.connected) {
    if (obs_out && n_force_slots != w->peer.slots) { rsb::set_error("rsb_control_step: obs_out must use the force slots the peer exchange was created with"); return RSB_E_INVALID; }
    if (obs_out) {   // ... and the same primitives in them: the launch writes ONE obs row layout to the caller's block and to the peers'
      for (int i = 0; i < n_force_slots; ++i) {
        const int32_t want = w->peer.idx.empty() ? i : w->peer.idx[i], got = force_collisions ? force_collisions[i] : i;
        if (want != got) { rsb::set_error("rsb_control_step: force_collisions differ from the list the peer exchange was created with"); return RSB_E_INVALID; }
      }
    }
    f.peer = true;
  }
  int st = request_obs(w, obs_out, force_collisions, n_force_slots, &f);
  if (st == RSB_OK) st = request_reset(w, "rsb_control_step", allowed_collisions, n_allowed, gc0, gv0, rows, &f);
  if (st != RSB_OK) return st;
  f.redirect_done = done_out != nullptr; f.done_out = done_out;
  return do_integrate(w, n_substeps, f);
}
int rsb_control_step(rsb_world* w, const float* p_target, const float* d_target, int n_substeps, float* obs_out, const int32_t* force_collisions,
                     int n_force_slots, const int32_t* allowed_collisions, int n_allowed, const float* gc0, const float* gv0, int rows) {
  return control_step(w, p_target, d_target, n_substeps, obs_out, force_collisions, n_force_slots, allowed_collisions, n_allowed, gc0, gv0, rows, nullptr);
}

// K control steps of the open loop (rsb.h): ONE resident launch when residency is on and the world's class has a resident twin, else K control steps
int rsb_control_steps(rsb_world* w, int n_steps, const float* p_targets, int period, long long first, int n_substeps, float* obs_out,
                      long long obs_step_stride, const int32_t* force_collisions, int n_force_slots, const int32_t* allowed_collisions, int n_allowed,
                      const float* gc0, const float* gv0, int rows, uint8_t* done_out, long long done_step_stride) {
  if (!w || n_steps < 1 || !p_targets || period < 1 || first < 0 || n_substeps < 1 || obs_step_stride < 0 || done_step_stride < 0 || n_force_slots < 0 ||
      n_force_slots > RSB_MAX_COLLISIONS || n_allowed < 0 || (n_allowed > 0 && !allowed_collisions) || ((gc0 != nullptr) != (gv0 != nullptr)) ||
      (gc0 && rows != 1 && rows != w->N)) {
    rsb::set_error("rsb_control_steps: bad argument");
    return RSB_E_INVALID;
  }
  HIP_TRY(hipSetDevice(w->device));
  const size_t slice = (size_t)w->N * w->blob.nq;
  StepClass c;
  LaunchKind open_loop;
  open_loop.res_stage = 0;
  if (!(w->res_on && choose_step_class(w, open_loop, &c) == RSB_OK)) {
    int st = RSB_OK;
    for (int j = 0; j < n_steps && st == RSB_OK; ++j)
      st = control_step(w, p_targets + (size_t)((first + j) % period) * slice, nullptr, n_substeps, obs_out ? obs_out + (size_t)j * (size_t)obs_step_stride : nullptr,
                        force_collisions, n_force_slots, allowed_collisions, n_allowed, gc0, gv0, rows, done_out ? done_out + (size_t)j * (size_t)done_step_stride : nullptr);
    return st;
  }
  StepRequest f;
  int st = request_obs(w, obs_out, force_collisions, n_force_slots, &f);
  if (st == RSB_OK) st = request_reset(w, "rsb_control_steps", allowed_collisions, n_allowed, gc0, gv0, rows, &f);
  if (st != RSB_OK) return st;
  f.res_steps = n_steps; f.res_stage = 0; f.res_targets = p_targets; f.res_period = period; f.res_first = first;
  f.res_obs_stride = obs_out ? obs_step_stride : 0; f.res_done_stride = done_out ? done_step_stride : 0; f.redirect_done = done_out != nullptr; f.done_out = done_out;   // (a stride without its buffer must not walk the world's own done flags)
  return do_integrate(w, n_substeps, f);
}
int rsb_set_step_residency(rsb_world* w, int on) {
  if (!w) { rsb::set_error("rsb_set_step_residency: null world"); return RSB_E_INVALID; }
  w->res_on = on != 0;
  return RSB_OK;
}
int rsb_step_residency_enabled(const rsb_world* w) { return w && w->res_on ? 1 : 0; }
int rsb_step_residency_status(rsb_world* w, int stage) {
  if (!w) { rsb::set_error("rsb_step_residency_status: null world"); return 0; }
  StepClass c;
  LaunchKind k;
  k.res_stage = stage; k.mlp_width = 128;
  return stage >= 0 && choose_step_class(w, k, &c) == RSB_OK ? 1 : 0;
}
long long rsb_step_residency_launches(const rsb_world* w) { return w ? w->res_launches : 0; }
int rsb_debug_resident_full_writes(rsb_world* w, int on) {
  if (!w) return RSB_E_INVALID;
  w->res_full = on != 0;
  return RSB_OK;
}

// ---- device-resident vectorised env ------------------------------------------------------------------------------
int rsb_env_configure(rsb_world* w, const rsb_env_config* cfg, const float* action_mean, const float* gc_init,
                      const float* gv_init) {
  if (!w || !cfg || !action_mean || !gc_init || !gv_init || cfg->n_substeps < 1 || cfg->n_foot < 0 || cfg->n_foot > RSB_MAX_COLLISIONS) {
    rsb::set_error("rsb_env_configure: bad argument");
    return RSB_E_INVALID;
  }
  unsigned long long allowed = 0;
  for (int i = 0; i < cfg->n_foot; ++i) {
    if (cfg->foot_collisions[i] < 0 || cfg->foot_collisions[i] >= w->blob.ncol) { rsb::set_error("rsb_env_configure: foot collision index out of range"); return RSB_E_INVALID; }
    allowed |= 1ull << cfg->foot_collisions[i];
  }
  HIP_TRY(hipSetDevice(w->device));
  const size_t N = w->N, nq = w->blob.nq, nv = w->blob.nv, nj = nv - 6, od = 10 + 2 * nj;
  if (!w->d_env_mean) {
    HIP_TRY(hipMalloc(&w->d_env_mean, nj * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_gc0, nq * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_gv0, nv * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_io, N * od * sizeof(float)));      // staging for host-side action / observation buffers
    HIP_TRY(hipMalloc(&w->d_env_ob, N * od * sizeof(float)));      // the fused step's observation (never the action's buffer: other waves may still have to read their actions)
    HIP_TRY(hipMalloc(&w->d_env_reward, N * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_tau2, N * sizeof(float)));
    HIP_TRY(hipMemset(w->d_env_tau2, 0, N * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_done, N));
    HIP_TRY(hipMalloc(&w->d_env_act, N * nj * sizeof(float)));     // the closed loop's action rows (rsb_closed_loop_run)
    HIP_TRY(hipMemset(w->d_env_act, 0, N * nj * sizeof(float)));
  }
  HIP_TRY(hipMemcpyAsync(w->d_env_mean, action_mean, nj * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  HIP_TRY(hipMemcpyAsync(w->d_env_gc0, gc_init, nq * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  HIP_TRY(hipMemcpyAsync(w->d_env_gv0, gv_init, nv * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  w->env_cfg = *cfg; w->env_allowed = allowed; w->env_ready = true;
  return obs_stats_init(w);      // (once per world: a later call - a new control_dt, say - keeps the statistics)
}
int rsb_env_set_reset_states(rsb_world* w, const float* gc0, const float* gv0, int space) {
  if (!w || ((gc0 != nullptr) != (gv0 != nullptr)) || (space != RSB_HOST && space != RSB_DEVICE)) { rsb::set_error("rsb_env_set_reset_states: bad argument"); return RSB_E_INVALID; }
  if (!w->env_ready) { rsb::set_error("rsb_env_set_reset_states: call rsb_env_configure first"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  hipStream_t s = stream_of(w);
  const size_t N = w->N, nq = w->blob.nq, nv = w->blob.nv;
  if (!gc0) {
    HIP_TRY(hipStreamSynchronize(s));
    if (w->d_env_gc0_rows) { HIP_TRY(hipFree(w->d_env_gc0_rows)); HIP_TRY(hipFree(w->d_env_gv0_rows)); }
    w->d_env_gc0_rows = w->d_env_gv0_rows = nullptr;
    return RSB_OK;
  }
  if (!w->d_env_gc0_rows) {
    HIP_TRY(hipMalloc(&w->d_env_gc0_rows, N * nq * sizeof(float)));
    HIP_TRY(hipMalloc(&w->d_env_gv0_rows, N * nv * sizeof(float)));
  }
  const hipMemcpyKind kind = space == RSB_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpyAsync(w->d_env_gc0_rows, gc0, N * nq * sizeof(float), kind, s));
  HIP_TRY(hipMemcpyAsync(w->d_env_gv0_rows, gv0, N * nv * sizeof(float), kind, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RSB_OK;
}
int rsb_env_dims(const rsb_world* w, int* ob_dim, int* action_dim) {
  if (!w) return RSB_E_INVALID;
  if (ob_dim) *ob_dim = 10 + 2 * (w->blob.nv - 6);
  if (action_dim) *action_dim = w->blob.nv - 6;
  return RSB_OK;
}
static int env_check(rsb_world* w, const char* who) {
  if (!w) return RSB_E_INVALID;
  if (!w->env_ready) { rsb::set_error(std::string(who) + ": call rsb_env_configure first"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  return RSB_OK;
}
int rsb_env_reset(rsb_world* w) {
  int st = env_check(w, "rsb_env_reset"); if (st != RSB_OK) return st;
  hipLaunchKernelGGL(env_reset_kernel, dim3((w->N + 255) / 256), dim3(256), 0, stream_of(w), w->d_gc, w->d_gv, w->d_count,
                     w->d_flags, w->d_env_gc0_rows ? w->d_env_gc0_rows : w->d_env_gc0, w->d_env_gc0_rows ? w->d_env_gv0_rows : w->d_env_gv0,
                     w->d_env_gc0_rows ? w->N : 1, w->N, w->blob.nq, w->blob.nv, w->d_warm, rsbk::kWarmRow);
  HIP_TRY(hipGetLastError());
  w->integrate1_valid = false; w->env_ob_valid = false;
  w->cl_passes = 0;      // (a closed-loop run's global step index - the noise slice of the reference stage - restarts with the episodes)
  return RSB_OK;
}
int rsb_env_observe(rsb_world* w, float* ob, int space) {
  int st = env_check(w, "rsb_env_observe"); if (st != RSB_OK) return st;
  if (!ob) return RSB_E_INVALID;
  const size_t od = 10 + 2 * (size_t)(w->blob.nv - 6);
  float* dob = space == RSB_DEVICE ? ob : w->d_env_io;
  st = launch_env_obs(w, dob, stream_of(w));
  if (st != RSB_OK) return st;
  if (space == RSB_HOST) return copy_out(w, ob, dob, (size_t)w->N * od * sizeof(float), RSB_HOST);
  return RSB_OK;
}
int rsb_env_step(rsb_world* w, const float* action, float* reward, uint8_t* done, float* ob_next, int space) {
  int st = env_check(w, "rsb_env_step"); if (st != RSB_OK) return st;
  if (!action) return RSB_E_INVALID;
  const int N = w->N, nv = w->blob.nv, nj = nv - 6;
  const size_t od = 10 + 2 * (size_t)nj;
  const float* dact = action;
  if (space == RSB_HOST) {
    HIP_TRY(hipMemcpyAsync(w->d_env_io, action, (size_t)N * nj * sizeof(float), hipMemcpyHostToDevice, stream_of(w)));
    dact = w->d_env_io;
  }
  float* drew = space == RSB_DEVICE ? reward : (reward ? w->d_env_reward : nullptr);
  uint8_t* ddone = space == RSB_DEVICE ? done : (done ? w->d_env_done : nullptr);
  float* dob = ob_next ? (space == RSB_DEVICE ? ob_next : w->d_env_ob) : nullptr;
  st = do_integrate(w, w->env_cfg.n_substeps, env_task_request(w, dact, drew, dob, ddone));
  if (st != RSB_OK) return st;
  w->integrate1_valid = false; w->env_ob_valid = false;
  if (space == RSB_HOST) {
    if (reward) HIP_TRY(hipMemcpyAsync(reward, w->d_env_reward, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
    if (done) HIP_TRY(hipMemcpyAsync(done, w->d_env_done, (size_t)N, hipMemcpyDeviceToHost, stream_of(w)));
    if (ob_next) HIP_TRY(hipMemcpyAsync(ob_next, w->d_env_ob, (size_t)N * od * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
    HIP_TRY(hipStreamSynchronize(stream_of(w)));
  }
  return RSB_OK;
}

void* rsb_device_ptr(rsb_world* w, int field) {
  if (!w) return nullptr;
  switch (field) {
    case RSB_F_GC: w->raw_state = true; w->env_ob_valid = false; return w->d_gc;      // (sticky: the caller may write through the pointer at any time)
    case RSB_F_GV: w->raw_state = true; w->env_ob_valid = false; return w->d_gv;
    case RSB_F_PTARGET: return w->d_pt;
    case RSB_F_DTARGET: w->dt_zero = false; w->raw_dt = true; return w->d_dt;       // (the caller may write through the pointer: the rows are read from now on, whatever a later upload of zeros says)
    case RSB_F_TAU_FF: w->tff_zero = false; w->raw_tff = true; return w->d_tff;
    case RSB_F_CONTACT_COUNT: return w->d_count;
    case RSB_F_CONTACTS: return w->d_contacts;
    case RSB_F_FLAGS: return w->d_flags;
    default: return nullptr;
  }
}

// Debug aid: the next rsb_integrate() launches dump env `env`'s contact problem of the LAST sub-step
// (Delassus matrix G [3nc,3nc], free contact velocity c [3nc], solved impulses lam [3nc], contact frame
// coordinates [t1 t2 n]); rsb_debug_read_contact_problem copies it to the host.  env < 0 disables.
int rsb_debug_select_env(rsb_world* w, int env) {
  if (!w || env >= w->N) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t n = 1 + 3 * RSB_MAX_CONTACTS * 3 * RSB_MAX_CONTACTS + 6 * RSB_MAX_CONTACTS;
  if (!w->d_dbg) HIP_TRY(hipMalloc(&w->d_dbg, n * sizeof(float)));
  HIP_TRY(hipMemsetAsync(w->d_dbg, 0, n * sizeof(float), stream_of(w)));
  w->dbg_env = env;
  return RSB_OK;
}
int rsb_debug_read_contact_problem(rsb_world* w, int* nc, float* G, float* c, float* lam) {
  if (!w || !nc || !w->d_dbg) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t n = 1 + 3 * RSB_MAX_CONTACTS * 3 * RSB_MAX_CONTACTS + 6 * RSB_MAX_CONTACTS;
  std::vector<float> buf(n);
  HIP_TRY(hipMemcpyAsync(buf.data(), w->d_dbg, n * sizeof(float), hipMemcpyDeviceToHost, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  const int k = (int)buf[0], n3 = 3 * k;
  *nc = k;
  if (G) std::memcpy(G, buf.data() + 1, sizeof(float) * n3 * n3);
  if (c) std::memcpy(c, buf.data() + 1 + n3 * n3, sizeof(float) * n3);
  if (lam) std::memcpy(lam, buf.data() + 1 + n3 * n3 + n3, sizeof(float) * n3);
  return RSB_OK;
}

// Debug aid: per-phase cycle stamps (s_memtime) of workgroup 0 in the last sub-step of each launch.
int rsb_debug_phase_cycles(rsb_world* w, int enable, long long* out16) {
  if (!w) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  const size_t nprof = 16 + 16 * (size_t)w->N;  // 16 phase stamps + 16 words per workgroup (upper bound: one env per wave)
  if (enable && !w->d_prof) { HIP_TRY(hipMalloc(&w->d_prof, nprof * sizeof(long long))); HIP_TRY(hipMemset(w->d_prof, 0, nprof * sizeof(long long))); }
  if (out16 && w->d_prof) {
    HIP_TRY(hipMemcpyAsync(out16, w->d_prof, 16 * sizeof(long long), hipMemcpyDeviceToHost, stream_of(w)));
    HIP_TRY(hipStreamSynchronize(stream_of(w)));
  }
  if (!enable && w->d_prof) { HIP_TRY(hipStreamSynchronize(stream_of(w))); HIP_TRY(hipFree(w->d_prof)); w->d_prof = nullptr; }
  return RSB_OK;
}

// per-workgroup profile of the last launch: out [4 * n_blocks] = {total cycles, Gauss-Seidel cycles, sum over
// sub-steps of the wave's max sweep count, max contact count}
int rsb_debug_wave_profile(rsb_world* w, long long* out, int n_blocks) {
  if (!w || !out || !w->d_prof || n_blocks > w->N) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipMemcpyAsync(out, w->d_prof + 16, 16 * (size_t)n_blocks * sizeof(long long), hipMemcpyDeviceToHost, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  // (the upper halves of words 2-7 carry the sweep-control counters: rsb_debug_wave_sweep_control)
  for (int b = 0; b < n_blocks; ++b)
    for (int i = 2; i < 8; ++i) out[16 * (size_t)b + i] &= 0xffffffffll;
  return RSB_OK;
}

// per-workgroup counters of the last launch's direction refreshes, out [12 * n_blocks]: Newton blocks of first sweeps; blocks in which the one rare-path test fired
// (or would have: the code without the test counts it too), first | later sweeps; blocks that ran the energy check, first | later; the basin check in its quad | serial
// form; blocks followed by a global search, first | later; blocks that ran none of the three, first | later; blocks that refused a lane's step.  Saturated at 65535.
// Counted by profiling twins compiled with -DRSB_X_SWEEP_COUNTERS (RSB_SPEC_EXTRA_DEFS) only - the counting costs a branch per counter - and zero otherwise.
int rsb_debug_wave_sweep_control(rsb_world* w, long long* out, int n_blocks) {
  if (!w || !out || !w->d_prof || n_blocks > w->N) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  std::vector<long long> raw(16 * (size_t)n_blocks);
  HIP_TRY(hipMemcpyAsync(raw.data(), w->d_prof + 16, raw.size() * sizeof(long long), hipMemcpyDeviceToHost, stream_of(w)));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  for (int b = 0; b < n_blocks; ++b)
    for (int i = 0; i < 12; ++i) out[12 * (size_t)b + i] = (raw[16 * (size_t)b + 2 + i / 2] >> (32 + 16 * (i & 1))) & 0xffff;
  return RSB_OK;
}

int rsb_enable_timing(rsb_world* w, int on) {
  if (!w || on < 0) return RSB_E_INVALID;
  HIP_TRY(hipSetDevice(w->device));
  for (hipEvent_t e : w->ring0) (void)hipEventDestroy(e);
  for (hipEvent_t e : w->ring1) (void)hipEventDestroy(e);
  w->ring0.clear(); w->ring1.clear(); w->ring_next = w->ring_count = 0;
  w->launch_index = 0;
  w->timing = on != 0;
  if (on > 1) {
    w->ring0.resize(on); w->ring1.resize(on);
    for (int i = 0; i < on; ++i) { HIP_TRY(hipEventCreate(&w->ring0[i])); HIP_TRY(hipEventCreate(&w->ring1[i])); }
  }
  return RSB_OK;
}
int rsb_set_timing_stride(rsb_world* w, int stride) {
  if (!w || stride < 1) return RSB_E_INVALID;
  w->timing_stride = stride; w->launch_index = 0;
  return RSB_OK;
}
int rsb_read_kernel_ms(rsb_world* w, float* ms, int n) {
  if (!w || !ms || n < 0) return RSB_E_INVALID;
  if (w->ring0.empty()) { rsb::set_error("rsb_read_kernel_ms: no timing ring (rsb_enable_timing(w, n) with n > 1)"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipStreamSynchronize(stream_of(w)));
  const size_t have = w->ring_count, cap = w->ring0.size();
  const size_t take = (size_t)n < have ? (size_t)n : have;
  for (size_t i = 0; i < take; ++i) {   // oldest of the last `take` launches first
    const size_t slot = (w->ring_next + cap - take + i) % cap;
    HIP_TRY(hipEventElapsedTime(&ms[i], w->ring0[slot], w->ring1[slot]));
  }
  return (int)take;
}
int rsb_last_kernel_ms(rsb_world* w, float* ms) {
  if (!w || !ms) return RSB_E_INVALID;
  if (!w->timing) { rsb::set_error("rsb_last_kernel_ms: timing is disabled (rsb_enable_timing)"); return RSB_E_STATE; }
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipEventSynchronize(w->ev1));
  HIP_TRY(hipEventElapsedTime(ms, w->ev0, w->ev1));
  return RSB_OK;
}

}  // extern "C"
