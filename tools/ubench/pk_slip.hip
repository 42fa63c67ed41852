// pk_slip.hip — are the packed helpers of step_slip_pk.h the same numbers as the scalar ones of step_slip.h?  65 536 random coefficient sets (built like
// basin_quad.hip's contacts); the refresh coefficients (kc), slip_newton (verdict, new direction, step), slip_rotate and slip_E compared bit for bit.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -fno-hip-fp32-correctly-rounded-divide-sqrt -I include -I raisimlib_amd/csrc tools/ubench/pk_slip.hip -o /tmp/pk_slip && /tmp/pk_slip
// Prints the mismatches per output and exits 1 if there is one.  This localises a wrong fusion to one helper; the step kernel's tests remain the verdict.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include "step_slip_pk.h"
using namespace rsbk;
constexpr int NIN = 24, NOUT = 14;
// in: Gii[0..8], lam[0..2], v[0..2], ls0, ls1, mu, x0, y0 (unit), a rotation angle, 21..23 unused
__global__ void k(const float* in, float* out_s, float* out_p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = in + NIN * i;
  float Gii[9], lam[3], v[3];
  for (int j = 0; j < 9; ++j) Gii[j] = p[j];
  for (int j = 0; j < 3; ++j) { lam[j] = p[9 + j]; v[j] = p[12 + j]; }
  const float ls[2] = {p[15], p[16]}, mu = p[17], x0 = p[18], y0 = p[19], ang = p[20];
  const float vexn = fmaf(-Gii[8], lam[2], fmaf(-Gii[7], lam[1], fmaf(-Gii[6], lam[0], v[2])));
  // ---- scalar.  The refresh coefficients are written with the mul / fma structure the SPECIALISED QUADRUPED CODE OBJECTS compile the sweep loop's lines to
  // (step_phase_solver.inc; read off their assembly): left as `v - (G0 l0 + G1 l1 + G2 l2)` the compiler rounds another product alone in this translation unit
  // (G1 l1 instead of G0 l0) - an expression with two products changes its rounding with its surroundings, and this file would compare two compilers' choices.
  // slip_newton, slip_rotate and slip_E are step_slip.h's own, on the same coefficients as the packed side.
  SlipCoef sc;
  sc.a0 = Gii[8]; sc.a1 = mu * Gii[6]; sc.a2 = mu * Gii[7];
  sc.n01 = mu * Gii[0]; sc.n02 = mu * Gii[1]; sc.n11 = mu * Gii[3]; sc.n12 = mu * Gii[4];
  SlipCoef kc = sc;
  {
    const float vex0 = __fsub_rn(v[0], fmaf(Gii[2], lam[2], fmaf(Gii[1], lam[1], __fmul_rn(Gii[0], lam[0]))));
    const float vex1 = __fsub_rn(v[1], fmaf(Gii[5], lam[2], fmaf(Gii[4], lam[1], __fmul_rn(Gii[3], lam[0]))));
    kc.n00 = fmaf(sc.a0, vex0, -__fmul_rn(vexn, Gii[2])); kc.n01 = fmaf(sc.a1, vex0, -__fmul_rn(vexn, sc.n01)); kc.n02 = fmaf(sc.a2, vex0, -__fmul_rn(vexn, sc.n02));
    kc.n10 = fmaf(sc.a0, vex1, -__fmul_rn(vexn, Gii[5])); kc.n11 = fmaf(sc.a1, vex1, -__fmul_rn(vexn, sc.n11)); kc.n12 = fmaf(sc.a2, vex1, -__fmul_rn(vexn, sc.n12));
    kc.vn = vexn; kc.ls0 = ls[0]; kc.ls1 = ls[1];
  }
  float* o = out_s + NOUT * i;
  o[0] = kc.n00; o[1] = kc.n01; o[2] = kc.n02; o[3] = kc.n10; o[4] = kc.n11; o[5] = kc.n12;
  {
    float nx, ny, d;
    const bool ok = slip_newton<false>(kc, mu, x0, y0, nx, ny, d);
    o[6] = ok ? 1.f : 0.f; o[7] = nx; o[8] = ny; o[9] = d;
    float rx, ry;
    slip_rotate(x0, y0, ang, rx, ry);
    o[10] = rx; o[11] = ry;
    o[12] = slip_E(kc, mu, x0, y0); o[13] = slip_E(kc, mu, rx, ry);
  }
  // ---- packed (step_slip_pk.h)
  const f32x2 gcp[3] = {f32x2{Gii[0], Gii[3]}, f32x2{Gii[1], Gii[4]}, f32x2{Gii[2], Gii[5]}};
  const f32x2 mg1 = pk_splat(mu) * gcp[0], mg2 = pk_splat(mu) * gcp[1];
  SlipCoefPk kp;
  pk_coef(kp, sc.a0, sc.a1, sc.a2, gcp[2], mg1, mg2, pk_vex(gcp, f32x2{v[0], v[1]}, f32x2{lam[0], lam[1]}, lam[2]), vexn, f32x2{ls[0], ls[1]});
  o = out_p + NOUT * i;
  o[0] = kp.n0.x; o[1] = kp.n1.x; o[2] = kp.n2.x; o[3] = kp.n0.y; o[4] = kp.n1.y; o[5] = kp.n2.y;
  {
    float nx, ny, d;
    const bool ok = slip_newton_pk(kp, mu, x0, y0, nx, ny, d);
    o[6] = ok ? 1.f : 0.f; o[7] = nx; o[8] = ny; o[9] = d;
    const f32x2 r = slip_rotate_pk(f32x2{x0, y0}, ang);
    o[10] = r.x; o[11] = r.y;
    o[12] = slip_E_pk(kp, mu, x0, y0, pk_den(kp, x0, y0)); o[13] = slip_E_pk(kp, mu, r.x, r.y, pk_den(kp, r.x, r.y));
  }
}
int main() {
  const int n = 1 << 16;
  std::vector<float> h((size_t)NIN * n);
  srand(1);
  auto r = []() { return (float)rand() / RAND_MAX * 2.f - 1.f; };
  for (int i = 0; i < n; ++i) {
    float* p = &h[(size_t)NIN * i];
    for (int j = 0; j < NIN; ++j) p[j] = r();
    p[8] = 1.f + r() * 0.5f; p[6] *= 0.3f; p[7] *= 0.3f;       // a0 > 0, a modest tilt of den(d)
    p[0] = 1.f + 0.5f * p[0]; p[4] = 1.f + 0.5f * p[4];        // a tangential block with a diagonal
    p[14] = -fabsf(p[14]);                                     // approaching
    p[17] = 0.8f;
    const float th = 3.14159265f * p[18];
    p[18] = cosf(th); p[19] = sinf(th);
    p[20] *= (i & 1) ? 0.25f : 0.02f;                          // small and large rotation steps
  }
  float *di, *d1, *d2;
  if (hipMalloc(&di, h.size() * 4) != hipSuccess || hipMalloc(&d1, (size_t)NOUT * n * 4) != hipSuccess || hipMalloc(&d2, (size_t)NOUT * n * 4) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
  if (hipMemcpy(di, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { printf("hipMemcpy failed\n"); return 2; }
  k<<<n / 256, 256>>>(di, d1, d2, n);
  std::vector<float> a((size_t)NOUT * n), b((size_t)NOUT * n);
  if (hipMemcpy(a.data(), d1, a.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(b.data(), d2, b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("hipMemcpy failed\n"); return 2; }
  const char* name[NOUT] = {"n00", "n01", "n02", "n10", "n11", "n12", "newton.ok", "newton.x", "newton.y", "newton.step", "rotate.x", "rotate.y", "E(d0)", "E(rotated)"};
  int bad[NOUT] = {0}, shown = 0, total = 0, oks = 0, big = 0;
  for (int i = 0; i < n; ++i) {
    oks += a[(size_t)NOUT * i + 6] != 0.f; big += fabsf(a[(size_t)NOUT * i + 9]) > 0.02f;
    for (int d = 0; d < NOUT; ++d)
      if (memcmp(&a[(size_t)NOUT * i + d], &b[(size_t)NOUT * i + d], 4)) { ++bad[d]; ++total; if (shown++ < 6) printf("set %d %s: scalar %.9g packed %.9g\n", i, name[d], a[(size_t)NOUT * i + d], b[(size_t)NOUT * i + d]); }
  }
  printf("sets %d, accepted Newton steps %d, steps above 0.02 rad %d\n", n, oks, big);
  printf("mismatches:"); for (int d = 0; d < NOUT; ++d) printf(" %s %d", name[d], bad[d]); printf(" | total %d\n", total);
  return total ? 1 : 0;
}
