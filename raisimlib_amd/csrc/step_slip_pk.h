// step_slip_pk.h — packed fp32 form of the one-contact rule's slip arithmetic (step_slip.h), for the specialised quadruped code objects (step_spec.h: RSB_PK_CLASS)
//
// Two fp32 expressions with the same shape sit in the halves of a register pair and are evaluated by ONE v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: a lone wave
// pays per instruction issued, not per operation.  The packed instructions round each half exactly as v_fma_f32 / v_mul_f32 / v_add_f32 do, so the results are
// those of step_slip.h to the last bit PROVIDED the same products are fused: every function here spells out the mul / fma structure the compiler chose for the
// scalar form in the specialised quadruped classes (read off their assembly), and every function body is compiled with contraction off so that the source decides.
// A difference and a sum over the same operands (P = N1 x - N0 y, Q = N0 x + N1 y) take the pair (-y, y): (-y) a and -(y a) are the same bits, and a pair negated
// in one half is something the compiler only does with extra instructions.
// tools/ubench/pk_slip.hip compares every function with its scalar twin bit for bit on random coefficient sets.
#pragma once

#include "step_slip.h"

// (the pragma opens every function body: at file scope it would reach the rest of the translation unit, whose contraction must stay what it was)
#define RSB_PK_NO_CONTRACT _Pragma("clang fp contract(off)")

namespace rsbk {

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 pk_splat(float a) { return f32x2{a, a}; }
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk_swap(f32x2 a) { return f32x2{a.y, a.x}; }

// SlipCoef with its tangential rows paired: nk = (n0k, n1k), ls = (ls0, ls1)
struct SlipCoefPk { float a0, a1, a2, vn; f32x2 n0, n1, n2, ls; };

__device__ __forceinline__ SlipCoef slip_unpack(const SlipCoefPk& k) {
  SlipCoef s;
  s.a0 = k.a0; s.a1 = k.a1; s.a2 = k.a2; s.vn = k.vn;
  s.n00 = k.n0.x; s.n10 = k.n0.y; s.n01 = k.n1.x; s.n11 = k.n1.y; s.n02 = k.n2.x; s.n12 = k.n2.y;
  s.ls0 = k.ls.x; s.ls1 = k.ls.y;
  return s;
}

// stick impulse, tangential part: ls[r] = lam[r] - Ginv[r][0] v0 - Ginv[r][1] v1 - Ginv[r][2] v2, r = 0 | 1.  gi[k] = (Ginv[k], Ginv[3 + k])
__device__ __forceinline__ f32x2 pk_stick(const f32x2 (&gi)[3], f32x2 v01, float v2, f32x2 lam01) { RSB_PK_NO_CONTRACT
  return pk_fma(-gi[2], pk_splat(v2), pk_fma(-gi[1], pk_splat(v01.y), pk_fma(-gi[0], pk_splat(v01.x), lam01)));
}

// tangential velocity without the own impulse: vex[r] = v[r] - (G[r][0] lam0 + G[r][1] lam1 + G[r][2] lam2).  gc[c] = (Gii[c], Gii[3 + c])
__device__ __forceinline__ f32x2 pk_vex(const f32x2 (&gc)[3], f32x2 v01, f32x2 lam01, float lam2) { RSB_PK_NO_CONTRACT
  const f32x2 t = pk_fma(gc[2], pk_splat(lam2), pk_fma(gc[1], pk_splat(lam01.y), gc[0] * pk_splat(lam01.x)));
  return v01 - t;
}

// the coefficients of a direction refresh (slip_prepare): n0k | n1k = a_k vex0|1 - vexn * (G[0|1][2],  mu G[0|1][0],  mu G[0|1][1]).  mg1, mg2: mu * gc[0], mu * gc[1]
__device__ __forceinline__ void pk_coef(SlipCoefPk& k, float a0, float a1, float a2, const f32x2& g2, const f32x2& mg1, const f32x2& mg2, f32x2 vex, float vexn, f32x2 ls01) { RSB_PK_NO_CONTRACT
  k.a0 = a0; k.a1 = a1; k.a2 = a2; k.vn = vexn; k.ls = ls01;
  k.n0 = pk_fma(pk_splat(a0), vex, -(pk_splat(vexn) * g2));
  k.n1 = pk_fma(pk_splat(a1), vex, -(mg1 * pk_splat(vexn)));
  k.n2 = pk_fma(pk_splat(a2), vex, -(mg2 * pk_splat(vexn)));
}

__device__ __forceinline__ float pk_den(const SlipCoefPk& k, float x, float y) { RSB_PK_NO_CONTRACT return __builtin_fmaf(k.a2, y, __builtin_fmaf(k.a1, x, k.a0)); }

// slip_E: vt0 | vt1 and the two products of e paired.  den = pk_den(k, x, y)
__device__ __forceinline__ float slip_E_pk(const SlipCoefPk& k, float mu, float x, float y, float den) { RSB_PK_NO_CONTRACT
  const float inv = __builtin_amdgcn_rcpf(den), ln = -k.vn * inv;
  const f32x2 vt = pk_fma(pk_splat(y), k.n2, pk_fma(pk_splat(x), k.n1, k.n0)) * pk_splat(inv);
  const f32x2 ab = pk_fma(f32x2{x, y}, pk_splat(mu * ln), -k.ls);
  const float e = fmaxf(0.5f * __builtin_fmaf(vt.x, ab.x, vt.y * ab.y), 0.f);
  return (den > kDenMin * k.a0) ? e : __int_as_float(0x7f800000);
}

// slip_newton_step (energy rule): N0 | N1, dN0 | dN1, (P, Q) and the two bracketed sums of hp paired; den, mdp, h, the reciprocal stay scalar.  den = pk_den(k, x0, y0)
__device__ __forceinline__ float slip_newton_step_pk(const SlipCoefPk& k, float x0, float y0, float den, float& hp) { RSB_PK_NO_CONTRACT
  const f32x2 xx = pk_splat(x0), yy = pk_splat(y0), ym = f32x2{-y0, y0};
  const float mdp = __builtin_fmaf(k.a2, x0, -(k.a1 * y0));
  const f32x2 N = pk_fma(yy, k.n2, pk_fma(xx, k.n1, k.n0));
  const f32x2 dN = pk_fma(xx, k.n2, -(yy * k.n1));
  const f32x2 PQ = pk_fma(xx, pk_swap(N), ym * N);          // P = x N1 - y N0, Q = x N0 + y N1
  const f32x2 AB = pk_fma(xx, pk_swap(dN), ym * dN);        // dN1 x - dN0 y, dN0 x + dN1 y
  const float h = __builtin_fmaf(den, PQ.x, -(mdp * PQ.y));
  hp = __builtin_fmaf(-mdp, AB.y, __builtin_fmaf(den, AB.x, -(k.a0 * PQ.y)));
  return -h * __builtin_amdgcn_rcpf(hp);
}

// slip_rotate: the rotation and the normalisation paired
__device__ __forceinline__ f32x2 slip_rotate_pk(f32x2 d0, float d) { RSB_PK_NO_CONTRACT
  const float d2 = d * d;
  const float c = __builtin_fmaf(-d2, __builtin_fmaf(-d2, 1.0f / 24.0f, 0.5f), 1.0f);
  const float t = __builtin_fmaf(-d2, __builtin_fmaf(-d2, 1.0f / 120.0f, 1.0f / 6.0f), 1.0f);
  const f32x2 sn = f32x2{-d, d} * pk_splat(t);
  const f32x2 xy = pk_fma(d0, pk_splat(c), pk_swap(d0) * sn);   // x = x0 c - y0 sn, y = y0 c + x0 sn
  const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(xy.x, xy.x, xy.y * xy.y));
  return xy * pk_splat(inv);
}

// slip_newton (energy rule) in two halves, so that the sweep loop can put the second one behind its one rare-path test (step_spec.h: RSB_SWEEP_RARE).
// The core: den0, the step, the rotation, den1 and the four guards
__device__ __forceinline__ bool slip_newton_core_pk(const SlipCoefPk& k, float x0, float y0, f32x2& xy, float& d, float& den0, float& den1) { RSB_PK_NO_CONTRACT
  den0 = pk_den(k, x0, y0);
  float hp;
  d = slip_newton_step_pk(k, x0, y0, den0, hp);
  xy = slip_rotate_pk(f32x2{x0, y0}, d);
  den1 = pk_den(k, xy.x, xy.y);
  return (den0 > kDenNewton * k.a0) && (hp > 0.f) && (fabsf(d) <= 0.25f) && (den1 > kDenNewton * k.a0);
}
// ... and the energy check of a step above 0.02 rad (ok: the core's verdict)
__device__ __forceinline__ bool slip_newton_energy_pk(const SlipCoefPk& k, float mu, float x0, float y0, f32x2 xy, float d, float den0, float den1, bool ok) { RSB_PK_NO_CONTRACT
  if (__any(ok && fabsf(d) > 0.02f)) ok = ok && (fabsf(d) <= 0.02f || slip_E_pk(k, mu, xy.x, xy.y, den1) <= slip_E_pk(k, mu, x0, y0, den0));
  return ok;
}
__device__ __forceinline__ bool slip_newton_pk(const SlipCoefPk& k, float mu, float x0, float y0, float& x1, float& y1, float& step) { RSB_PK_NO_CONTRACT
  f32x2 xy;
  float d, den0, den1;
  const bool core = slip_newton_core_pk(k, x0, y0, xy, d, den0, den1);
  const bool ok = slip_newton_energy_pk(k, mu, x0, y0, xy, d, den0, den1, core);
  x1 = xy.x; y1 = xy.y; step = d;
  return ok;
}

}  // namespace rsbk
