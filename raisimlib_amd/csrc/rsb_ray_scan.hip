// rsb_ray_scan.hip — ray casts and sensor-mounted ray scans that also see the robot, from the resident state (rsb_ray_cast, rsb_ray_scan;
// include/rsb.h).
//
// What World::rayTest gives upstream for one world and one ray on the host [RECALL] - the first hit among ALL objects - for all N envs in one call,
// on the world's stream, and its fused sensor form: a pattern of directions fixed in a body, cast from a frame of that body, written into an
// observation tensor at the caller's row pitch.  Nothing here is shared with the step kernel's instances.  The chain walk, the argument checks and
// the staging of the RSB_HOST forms are those of all batched queries (frames_chain.h); the surface is rsbk::terrain_eval (step_terrain.h) and the
// ray's march over it is terrain_ray.h, one definition for both kernels.
//
// The robot as rays see it: a list of SHAPES built once per world from the blob's collision primitives (ray_shapes_of below: spheres, capsules,
// cylinders with flat caps, boxes; zero-radius points have no surface), kept in the body frame in a small device buffer of the world.  A ray
// against a shape gives the first parameter at which the ray is on or inside it; the forms are free of cancellation in fp32 (entry_round, box_entry).
//
//   ray_scan_kernel  the hot path.  A workgroup takes ONE env and a chunk of kRaysPerBlock of its F * P rays (about four blocks' worth, as
//                    height_scan_kernel).  (1) model rows and the pattern into LDS; (2) lane b < nb walks the chain of body b and leaves (R, p) in
//                    LDS; (3) lane s < n_shapes writes shape s in world coordinates, lane f < F the frame's origin, both to LDS; (4) all lanes sweep
//                    the rays, consecutive lanes writing consecutive floats.  The shape loop has a uniform trip count and every lane reads the same
//                    record: an LDS broadcast.  A ray's result depends on its (env, frame, direction) alone.
//   ray_cast_kernel  world-space rays, one lane per ray, a workgroup within one env; phases (2) and (3) only where the call asks for bodies.
//                    Without them the kernel computes exactly what ray_test_kernel does, through the same functions.
#include <cstring>
#include <vector>

#include "frames_chain.h"
#include "rsb_world.h"
#include "step_terrain.h"
#include "terrain_ray.h"

namespace rsbw {
namespace {

constexpr int kRaysPerBlock = 4 * kThreads;      // ray_scan_kernel: rays of one workgroup
constexpr int kXf = 12;              // per body in LDS: R 0-8 (row-major, world <- body), p 9-11
constexpr int kShapeRec = 16;        // floats per shape: kind 0, body 1, first primitive 2 (int bits), radius 3, then by kind
                                     //   body frame (device buffer)                      world frame (LDS)
                                     //   sphere    centre 4-6                            centre 4-6
                                     //   capsule / cylinder   ends a 4-6, b 7-9          end a 4-6, unit axis a -> b 7-9, length 10
                                     //   box       centre 4-6, half-edges 7-9 10-12 13-15   centre 4-6, half-edges / their squared lengths 7-15
constexpr int kFrameRec = 4;         // per frame in LDS: origin 0-2, body 3 (int bits)
enum ShapeKind { kSphere = 0, kCapsule = 1, kCylinder = 2, kBox = 3 };
constexpr int kAllFlags = RSB_RAY_BODIES | RSB_RAY_OWN_BODY | RSB_RAY_PLANAR | RSB_RAY_MISS_MAX;

// the terrain as the step launch describes it (StepArgs' fields of the same names, the same values): rsb_terrain_query.hip's struct, which that
// file keeps to itself
struct Terrain {
  int terrain_type, hm_xs, hm_ys;
  float ground_z, hm_x0, hm_y0, hm_dx, hm_dy, hm_inv_dx, hm_inv_dy, hm_max;
  const float* heights;        // [n_maps][hm_ys][hm_xs]
  const int32_t* hm_index;     // [N] height map of each env (NULL: every env uses map 0)
};

__device__ __forceinline__ const float* map_of(const Terrain& t, int env) {
  const int map = t.hm_index ? t.hm_index[env] : 0;
  return t.heights + (size_t)map * t.hm_xs * t.hm_ys;
}

__device__ __forceinline__ float inf_f() { return __int_as_float(0x7f800000); }

// First parameter in [t0, t1] at which m + t e is within the distance r (r2 = r * r) of the origin, or +inf: the round cross-section of a sphere
// (m = origin - centre, e = the unit direction) and of an infinite cylinder (m, e: their parts normal to the axis; A = e . e).  Everything is taken
// relative to t0, where the ray is already near the shape.  Closest approach inside the range: the discriminant comes from the perpendicular
// offset q, not from |m|^2 - r^2 of a far origin.  Closest approach beyond t1: solved backwards from t1, with the root that adds, never subtracts.
__device__ __forceinline__ float entry_round(const float* m, const float* e, float A, float r2, float t0, float t1) {
  if (!(t0 <= t1)) return inf_f();
  float m0[3];
  for (int k = 0; k < 3; ++k) m0[k] = m[k] + t0 * e[k];
  if (dot3(m0, m0) <= r2) return t0;
  const float B0 = dot3(m0, e);
  if (A < 1e-20f || B0 >= 0.f) return inf_f();           // parallel to the axis, or moving away
  const float tc = -B0 / A;
  if (t0 + tc <= t1) {
    float q[3];
    for (int k = 0; k < 3; ++k) q[k] = m0[k] + tc * e[k];
    const float disc = r2 - dot3(q, q);
    if (disc < 0.f) return inf_f();
    return t0 + fmaxf(tc - sqrtf(disc / A), 0.f);
  }
  float m1[3];
  for (int k = 0; k < 3; ++k) m1[k] = m[k] + t1 * e[k];
  const float C1 = dot3(m1, m1) - r2;
  if (C1 > 0.f) return inf_f();                          // still outside at the end of the range
  const float B1 = dot3(m1, e);                          // (< 0: still approaching)
  const float back = -C1 / (-B1 + sqrtf(fmaxf(B1 * B1 - A * C1, 0.f)));
  return fmaxf(t1 - back, t0);
}

// a box by slabs in its own frame: along half-edge i the coordinate dot(x - centre, g_i), g_i = the half-edge over its squared length, runs over [-1, 1]
__device__ __forceinline__ float box_entry(const float* rec, const float* o, const float* d, float max_dist) {
  const float m[3] = {o[0] - rec[4], o[1] - rec[5], o[2] - rec[6]};
  float lo = 0.f, hi = max_dist;
  bool meets = true;
  for (int i = 0; i < 3; ++i) {
    const float* g = rec + 7 + 3 * i;
    const float oi = dot3(m, g), di = dot3(d, g);
    if (di != 0.f) { const float a = (-1.f - oi) / di, b = (1.f - oi) / di; lo = fmaxf(lo, fminf(a, b)); hi = fminf(hi, fmaxf(a, b)); }
    else meets = meets && fabsf(oi) <= 1.f;
  }
  return meets && lo <= hi ? lo : inf_f();
}

// the first parameter in [0, max_dist] at which the ray o + t d (d a unit vector) is on or inside the world-frame shape `rec`, or +inf
__device__ __forceinline__ float shape_entry(const float* rec, const float* o, const float* d, float max_dist) {
  const int kind = __float_as_int(rec[0]);
  const float r2 = rec[3] * rec[3];
  if (kind == kBox) return box_entry(rec, o, d, max_dist);
  const float m[3] = {o[0] - rec[4], o[1] - rec[5], o[2] - rec[6]};
  if (kind == kSphere) return entry_round(m, d, 1.f, r2, 0.f, max_dist);
  // capsule, cylinder: the infinite cylinder about the axis, clipped to the slab 0 <= (x - a) . n <= L between the ends
  const float* n = rec + 7;
  const float L = rec[10], dn = dot3(d, n), mn = dot3(m, n);
  float mp[3], dp[3];
  for (int k = 0; k < 3; ++k) { mp[k] = m[k] - mn * n[k]; dp[k] = d[k] - dn * n[k]; }
  float t0 = 0.f, t1 = max_dist;
  if (dn != 0.f) { const float a = -mn / dn, b = (L - mn) / dn; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
  else if (mn < 0.f || mn > L) t1 = -1.f;
  float best = entry_round(mp, dp, dot3(dp, dp), r2, t0, t1);
  if (kind == kCapsule) {                                // ... and the two end spheres
    const float mb[3] = {m[0] - L * n[0], m[1] - L * n[1], m[2] - L * n[2]};
    best = fminf(best, fminf(entry_round(m, d, 1.f, r2, 0.f, max_dist), entry_round(mb, d, 1.f, r2, 0.f, max_dist)));
  }
  return best;
}

// phase (2): lane b < nb walks body b's chain and leaves (R, p); phase (3) after the caller's barrier
__device__ __forceinline__ void body_transforms(const DevModel& m, int nb, const float* rows, const float* q, float* xf) {
  if ((int)threadIdx.x < nb) {
    Chain c;
    walk_chain<false>(m, rows, q, nullptr, nullptr, false, (int)threadIdx.x, c, NoJoint{});
    float* x = xf + threadIdx.x * kXf;
    for (int k = 0; k < 9; ++k) x[k] = c.R[k];
    for (int k = 0; k < 3; ++k) x[9 + k] = c.p[k];
  }
}
__device__ __forceinline__ void point_to_world(const float* x, const float* v, float* o) {
  float r[3];
  mat3_vec(x, v, r);
  for (int k = 0; k < 3; ++k) o[k] = x[9 + k] + r[k];
}
__device__ __forceinline__ void shapes_to_world(const float* __restrict__ shapes, int S, const float* xf, float* sw) {
  if ((int)threadIdx.x < S) {
    const float* b = shapes + threadIdx.x * kShapeRec;
    float* w = sw + threadIdx.x * kShapeRec;
    const int kind = __float_as_int(b[0]);
    const float* x = xf + __float_as_int(b[1]) * kXf;
    for (int k = 0; k < 4; ++k) w[k] = b[k];
    point_to_world(x, b + 4, w + 4);
    for (int k = 7; k < kShapeRec; ++k) w[k] = 0.f;
    if (kind == kCapsule || kind == kCylinder) {
      float e[3];
      point_to_world(x, b + 7, e);
      for (int k = 0; k < 3; ++k) e[k] -= w[4 + k];
      const float L = sqrtf(dot3(e, e));
      w[7] = L > 0.f ? e[0] / L : 0.f; w[8] = L > 0.f ? e[1] / L : 0.f; w[9] = L > 0.f ? e[2] / L : 1.f;
      w[10] = L;
    } else if (kind == kBox) {
      for (int i = 0; i < 3; ++i) {
        float e[3];
        mat3_vec(x, b + 7 + 3 * i, e);
        const float in = 1.f / dot3(e, e);               // (ray_shapes_of lists no box with a zero edge)
        for (int k = 0; k < 3; ++k) w[7 + 3 * i + k] = e[k] * in;
      }
    }
  }
}

struct RayHit { float dist; int hit; };

// one ray of env `env` with the usable unit direction d: the terrain first, with the call's max_dist whatever the bodies give (where the terrain
// wins, the answer is ray_test_kernel's), then the shapes - all but those of body `skip`
__device__ __forceinline__ RayHit cast_ray(const Terrain& t, int env, const float* o, const float* d, float max_dist, const float* sw, int S, int skip) {
  float ground;
  if (t.terrain_type != 1) {
    ground = rsbk::plane_ray(t.ground_z, o[2], d[2], max_dist);
  } else {
    const float* heights = map_of(t, env);
    const float ox = o[0], oy = o[1], oz = o[2], dx = d[0], dy = d[1], dz = d[2];
    const auto gap = [&](float s) {                      // z - h at parameter s
      float h, n[3];
      rsbk::terrain_eval(t, heights, ox + s * dx, oy + s * dy, h, n);
      return oz + s * dz - h;
    };
    ground = rsbk::heightmap_ray(t, ox, oy, oz, dx, dy, dz, max_dist, gap);
  }
  float best = inf_f();
  int which = RSB_RAY_HIT_NONE;
  for (int s = 0; s < S; ++s) {
    const float* rec = sw + s * kShapeRec;
    if (__float_as_int(rec[1]) == skip) continue;
    const float e = shape_entry(rec, o, d, max_dist);
    if (e < best) { best = e; which = __float_as_int(rec[2]); }
  }
  if (ground >= 0.f && !(best < ground)) return {ground, RSB_RAY_HIT_TERRAIN};
  if (which >= 0) return {best, which};
  return {-1.f, RSB_RAY_HIT_NONE};
}

// dynamic LDS: [nb * kRow model rows | nb * kXf body transforms | S shape records | F frame records | P * 3 pattern]
__global__ __launch_bounds__(kThreads) void ray_scan_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const FrameList frames, int F,
                                                            const Terrain t, const float* __restrict__ shapes, int S, const float* __restrict__ dirs, int P,
                                                            int flags, float max_dist, int chunks, float* __restrict__ out, long long row_stride,
                                                            int32_t* __restrict__ hit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const DevModel& m = *model;
  const int nb = m.nb;
  float* rows = lds;
  float* xf = rows + nb * kRow;
  float* sw = xf + nb * kXf;
  float* fr = sw + S * kShapeRec;
  float* pat = fr + F * kFrameRec;
  const int env = blockIdx.x / chunks, chunk = blockIdx.x - env * chunks;
  stage_rows(m, rows);
  for (int k = threadIdx.x; k < 3 * P; k += kThreads) pat[k] = dirs[k];
  __syncthreads();
  body_transforms(m, nb, rows, gc + (size_t)env * m.nq, xf);
  __syncthreads();
  shapes_to_world(shapes, S, xf, sw);
  if ((int)threadIdx.x < F) {
    const rsb_frame f = frames.f[threadIdx.x];
    float* r = fr + threadIdx.x * kFrameRec;
    point_to_world(xf + f.body * kXf, f.offset, r);
    r[3] = __int_as_float(f.body);
  }
  __syncthreads();
  const int width = F * P;
  const bool own = flags & RSB_RAY_OWN_BODY, planar = flags & RSB_RAY_PLANAR, miss_max = flags & RSB_RAY_MISS_MAX;
  for (int i = 0; i < kRaysPerBlock / kThreads; ++i) {
    const int e = chunk * kRaysPerBlock + i * kThreads + (int)threadIdx.x;
    if (e >= width) break;
    const int f = e / P, k = e - f * P;
    const float* r = fr + f * kFrameRec;
    const int body = __float_as_int(r[3]);
    const float* x = xf + body * kXf;
    const float o[3] = {r[0], r[1], r[2]};
    // the pattern's direction in the body's axes, scaled into range before it is turned; ray_unit normalises as ray_test_kernel does
    float b[3] = {pat[3 * k], pat[3 * k + 1], pat[3 * k + 2]}, d[3];
    const float big = fmaxf(fabsf(b[0]), fmaxf(fabsf(b[1]), fabsf(b[2])));
    const float sc = big > 0.f && isfinite(big) ? 1.f / big : 1.f;
    for (int c = 0; c < 3; ++c) b[c] *= sc;
    mat3_vec(x, b, d);
    RayHit h{-1.f, RSB_RAY_HIT_NONE};
    float cosx = 1.f;                                    // (a ray that cannot be cast has no cosine: its miss is reported along the ray)
    if (rsbk::ray_unit(o[0], o[1], o[2], d[0], d[1], d[2])) {
      h = cast_ray(t, env, o, d, max_dist, sw, S, own ? -1 : body);
      if (planar) cosx = d[0] * x[0] + d[1] * x[3] + d[2] * x[6];      // unit direction . the frame's x axis (the first column of R)
    }
    const float range = h.hit == RSB_RAY_HIT_NONE ? (miss_max ? max_dist * cosx : -1.f) : h.dist * cosx;
    if (out) out[(long long)env * row_stride + e] = range;
    if (hit) hit[(long long)env * width + e] = h.hit;
  }
}

// dynamic LDS (bodies only): [nb * kRow model rows | nb * kXf body transforms | S shape records]
__global__ __launch_bounds__(kThreads) void ray_cast_kernel(const DevModel* __restrict__ model, const float* __restrict__ gc, const Terrain t,
                                                            const float* __restrict__ shapes, int S, const float* __restrict__ origins,
                                                            const float* __restrict__ directions, int R, int flags, float max_dist, int chunks,
                                                            float* __restrict__ dist, int32_t* __restrict__ hit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = blockIdx.x / chunks, chunk = blockIdx.x - env * chunks;
  const float* sw = lds;
  if (S > 0) {                                           // (uniform: S is 0 unless the call asks for bodies)
    const DevModel& m = *model;
    const int nb = m.nb;
    float* rows = lds;
    float* xf = rows + nb * kRow;
    float* s = xf + nb * kXf;
    stage_rows(m, rows);
    __syncthreads();
    body_transforms(m, nb, rows, gc + (size_t)env * m.nq, xf);
    __syncthreads();
    shapes_to_world(shapes, S, xf, s);
    __syncthreads();
    sw = s;
  }
  const int ray = chunk * kThreads + (int)threadIdx.x;
  if (ray >= R) return;
  const long long idx = (long long)env * R + ray;
  const float o[3] = {origins[idx * 3], origins[idx * 3 + 1], origins[idx * 3 + 2]};
  float d[3] = {directions[idx * 3], directions[idx * 3 + 1], directions[idx * 3 + 2]};
  RayHit h{-1.f, RSB_RAY_HIT_NONE};
  if (rsbk::ray_unit(o[0], o[1], o[2], d[0], d[1], d[2])) h = cast_ray(t, env, o, d, max_dist, sw, S, -1);
  if (dist) dist[idx] = h.hit == RSB_RAY_HIT_NONE ? ((flags & RSB_RAY_MISS_MAX) ? max_dist : -1.f) : h.dist;
  if (hit) hit[idx] = h.hit;
}

Terrain terrain_of(const rsb_world* w) {       // as do_integrate fills StepArgs (rsb_world.hip)
  Terrain t{};
  t.terrain_type = w->terrain_type; t.hm_xs = w->hm_xs; t.hm_ys = w->hm_ys; t.ground_z = (float)w->ground_z;
  if (w->terrain_type == 1) {
    const double dx = w->hm_xsize / (w->hm_xs - 1), dy = w->hm_ysize / (w->hm_ys - 1);
    t.hm_x0 = (float)(w->hm_cx - 0.5 * w->hm_xsize); t.hm_y0 = (float)(w->hm_cy - 0.5 * w->hm_ysize);
    t.hm_dx = (float)dx; t.hm_dy = (float)dy; t.hm_inv_dx = (float)(1.0 / dx); t.hm_inv_dy = (float)(1.0 / dy);
    t.hm_max = w->hm_max;
  }
  t.heights = w->d_heights; t.hm_index = w->d_hm_index;
  return t;
}

// The robot's shapes, body frame, from the blob's collision primitives in index order:
//   col_capsule[s] == -1                      an oriented box from the corners s .. s + 7 (corner s + e: bit 0 of e = +x, bit 1 = +y, bit 2 = +z)
//   col_capsule[s] = e + 1, col_rim[s] == 0   a capsule between the centres of s and e, radius col_radius[s]
//   col_capsule[s] = e + 1, col_rim[s] > 0    a cylinder with flat caps between the centres of s and e, radius col_rim[s]
//   any other primitive with a radius         a sphere
// Zero-radius points - a mesh's hull vertices, the lattice of a sampled box, a lone rim - have no surface: a mesh collider is invisible to rays.
// (A box with an edge of zero length has no volume either and is left out.)
std::vector<float> ray_shapes_of(const rsb_model_blob& b) {
  std::vector<float> recs;
  std::vector<char> used(b.ncol, 0);
  const auto as_f = [](int v) { float f; std::memcpy(&f, &v, sizeof f); return f; };
  const auto begin = [&](int kind, int s, double radius) {
    recs.resize(recs.size() + kShapeRec, 0.f);
    float* r = recs.data() + recs.size() - kShapeRec;
    r[0] = as_f(kind); r[1] = as_f(b.col_body[s]); r[2] = as_f(s); r[3] = (float)radius;
    return r;
  };
  for (int s = 0; s < b.ncol; ++s) {
    if (used[s]) continue;
    const int cap = b.col_capsule[s];
    if (cap == -1 && s + 7 < b.ncol) {
      for (int k = 0; k < 8; ++k) used[s + k] = 1;
      double c[3] = {0, 0, 0}, e[3][3], len2[3] = {0, 0, 0};
      for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 8; ++j) c[k] += b.col_pos[s + j][k] / 8.0;
        for (int i = 0; i < 3; ++i) { e[i][k] = 0.5 * (b.col_pos[s + (1 << i)][k] - b.col_pos[s][k]); len2[i] += e[i][k] * e[i][k]; }
      }
      if (!(len2[0] > 0 && len2[1] > 0 && len2[2] > 0)) continue;
      float* r = begin(kBox, s, 0.0);
      for (int k = 0; k < 3; ++k) { r[4 + k] = (float)c[k]; for (int i = 0; i < 3; ++i) r[7 + 3 * i + k] = (float)e[i][k]; }
    } else if (cap > 0 && cap - 1 < b.ncol) {
      const int e = cap - 1;
      used[e] = 1;
      const bool cyl = b.col_rim[s] > 0;
      float* r = begin(cyl ? kCylinder : kCapsule, s, cyl ? b.col_rim[s] : b.col_radius[s]);
      for (int k = 0; k < 3; ++k) { r[4 + k] = (float)b.col_pos[s][k]; r[7 + k] = (float)b.col_pos[e][k]; }
    } else if (b.col_radius[s] > 0) {
      float* r = begin(kSphere, s, b.col_radius[s]);
      for (int k = 0; k < 3; ++k) r[4 + k] = (float)b.col_pos[s][k];
    }
  }
  return recs;
}

// the world's copy of them on the device, made on first use (joins a pipelined world: the upload goes down the world's stream)
int ray_shapes(rsb_world* w, const float** dev, int* n) {
  if (w->n_ray_shapes < 0) {
    const std::vector<float> recs = ray_shapes_of(w->blob);
    if (!recs.empty()) {
      HIP_TRY(hipMalloc((void**)&w->d_ray_shapes, recs.size() * sizeof(float)));
      hipStream_t s = stream_of(w);
      HIP_TRY(hipMemcpyAsync(w->d_ray_shapes, recs.data(), recs.size() * sizeof(float), hipMemcpyHostToDevice, s));
      HIP_TRY(hipStreamSynchronize(s));                  // (recs is a local)
    }
    w->n_ray_shapes = (int)(recs.size() / kShapeRec);
  }
  *dev = w->d_ray_shapes; *n = w->n_ray_shapes;
  return RSB_OK;
}

int check_ray_args(const char* who, float max_dist, int flags, int allowed) {
  if (!(max_dist > 0.f) || !std::isfinite(max_dist)) return invalid(who, "max_dist must be positive and finite");
  if (flags & ~kAllFlags) return invalid(who, "unknown bits in flags " + std::to_string(flags));
  if (flags & ~allowed) return invalid(who, "RSB_RAY_OWN_BODY and RSB_RAY_PLANAR are rsb_ray_scan's");
  return RSB_OK;
}

}  // namespace

void ray_shapes_free(rsb_world* w) {
  if (w->d_ray_shapes) (void)hipFree(w->d_ray_shapes);
  w->d_ray_shapes = nullptr; w->n_ray_shapes = -1;
}

}  // namespace rsbw
using namespace rsbw;

extern "C" {

int rsb_ray_cast(rsb_world* w, const float* origins, const float* directions, int n_rays, float max_dist, int flags, float* dist, int32_t* hit, int space) {
  const char* who = "rsb_ray_cast";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  if (!origins || !directions) return invalid(who, "origins and directions must not be NULL");
  if (!dist && !hit) return invalid(who, "every output is NULL");
  if (n_rays < 1) return invalid(who, "n_rays must be at least 1");
  st = check_ray_args(who, max_dist, flags, RSB_RAY_BODIES | RSB_RAY_MISS_MAX); if (st != RSB_OK) return st;
  HIP_TRY(hipSetDevice(w->device));
  const float* shapes = nullptr;
  int S = 0;
  if (flags & RSB_RAY_BODIES) { st = ray_shapes(w, &shapes, &S); if (st != RSB_OK) return st; }
  const size_t total = (size_t)w->N * n_rays;
  const float *dor, *ddi;
  float *dd, *dh;
  Staged io(w, space);
  io.in(dor, origins, total * 3); io.in(ddi, directions, total * 3); io.out(dd, dist, total); io.out(dh, reinterpret_cast<float*>(hit), total);
  st = io.begin(); if (st != RSB_OK) return st;
  const int chunks = (int)blocks_for((size_t)n_rays);
  const size_t lds = S > 0 ? ((size_t)w->blob.nb * (kRow + kXf) + (size_t)S * kShapeRec) * sizeof(float) : 0;
  hipLaunchKernelGGL(ray_cast_kernel, dim3((unsigned)w->N * chunks), dim3(kThreads), lds, stream_of(w), (const DevModel*)w->d_model, (const float*)w->d_gc,
                     terrain_of(w), shapes, S, dor, ddi, n_rays, flags, max_dist, chunks, dd, reinterpret_cast<int32_t*>(dh));
  HIP_TRY(hipGetLastError());
  return io.end();
}

int rsb_ray_scan(rsb_world* w, const rsb_frame* frames, int n_frames, const float* dirs, int n_points, int flags, float max_dist, float* out,
                 long long row_stride, int32_t* hit, int space) {
  const char* who = "rsb_ray_scan";
  int st = check_world(w, who, space); if (st != RSB_OK) return st;
  st = check_frames(w, who, frames, n_frames); if (st != RSB_OK) return st;
  if (!dirs) return invalid(who, "dirs must not be NULL");
  if (!out && !hit) return invalid(who, "every output is NULL");
  if (n_points < 1 || n_points > RSB_MAX_RAY_POINTS) return invalid(who, "n_points must be 1.." + std::to_string(RSB_MAX_RAY_POINTS));
  st = check_ray_args(who, max_dist, flags, kAllFlags); if (st != RSB_OK) return st;
  const long long width = (long long)n_frames * n_points;
  if (row_stride == 0) row_stride = width;
  if (row_stride < width) return invalid(who, "row_stride " + std::to_string(row_stride) + " is smaller than n_frames * n_points = " + std::to_string(width));
  HIP_TRY(hipSetDevice(w->device));
  const float* shapes = nullptr;
  int S = 0;
  if (flags & RSB_RAY_BODIES) { st = ray_shapes(w, &shapes, &S); if (st != RSB_OK) return st; }
  const size_t N = w->N;
  const float* dp;
  float *dout, *dh;
  Staged io(w, space);      // RSB_HOST: the scan is staged dense; its rows go to the caller's stride on the way back, below, not through end()
  io.in(dp, dirs, (size_t)n_points * 3); io.out(dout, out, N * width); io.out(dh, reinterpret_cast<float*>(hit), N * width);
  st = io.begin(); if (st != RSB_OK) return st;
  const long long dstride = space == RSB_HOST ? width : row_stride;
  hipStream_t s = stream_of(w);
  const int chunks = (int)blocks_for((size_t)width, kRaysPerBlock);
  const size_t lds = ((size_t)w->blob.nb * (kRow + kXf) + (size_t)S * kShapeRec + (size_t)n_frames * kFrameRec + (size_t)n_points * 3) * sizeof(float);
  hipLaunchKernelGGL(ray_scan_kernel, dim3((unsigned)N * chunks), dim3(kThreads), lds, s, (const DevModel*)w->d_model, (const float*)w->d_gc,
                     frame_list(frames, n_frames), n_frames, terrain_of(w), shapes, S, dp, n_points, flags, max_dist, chunks, dout, dstride,
                     reinterpret_cast<int32_t*>(dh));
  HIP_TRY(hipGetLastError());
  if (space == RSB_HOST) {
    const int fs = fault_status(w); if (fs != RSB_OK) return fs;
    if (out) HIP_TRY(hipMemcpy2DAsync(out, (size_t)row_stride * sizeof(float), dout, (size_t)width * sizeof(float), (size_t)width * sizeof(float), N, hipMemcpyDeviceToHost, s));
    if (hit) HIP_TRY(hipMemcpyAsync(hit, dh, N * width * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return RSB_OK;
}

}  // extern "C"
