// Batched RANSAC absolute pose from a MINIMAL sample (fpc_ransac_p3p / fpc_p3p_frames / fpc_p3p_bank; the rule is stated in
// include/fpc.h and restated in float64 by tests/test_p3p_ransac.py).  The fifth model of the family ransac_parts.h was built
// for, and the second absolute-pose model: where the 6-point DLT of pnp_ransac.h needs landmarks in general position, three
// points and a fourth to pick the root also solve a slot whose landmarks lie on one plane.  This header holds the minimal
// solve only -- Grunert's quartic, Ferrari's roots, the two triads, the fourth point's choice.  The pair records and their
// pack / gather kernels, the scored hypothesis (pnp_hypothesis), the fp32 count (PnpModel::counts), the Gauss-Newton refit
// (pnp_refit_body) and the reprojection tests are pnp_ransac.h's; the triad is sim3_ransac.h's; the sampler, the selection
// key and the score and refit skeletons are ransac_parts.h's.
//
//   p3p_score_kernel  score_body at 256 hypotheses per workgroup.  The solve lives in named fp64 registers: no linear
//                     system, no dynamically indexed array (an indexed store becomes scratch), every loop over registers
//                     unrolled; the walk over the four candidate roots is a loop of four trips in every lane, with the
//                     candidate's validity as a predicate.  The workgroup's LDS is the 1 024-record stage (32 KiB) alone --
//                     the DLT's 66 KiB of systems are gone -- so, as for sim3_score_kernel, THREADS is free and 256 stages
//                     every record once per 256 hypotheses.  The resource figures are in DESIGN.md section 7.
//   p3p_refit_kernel  pnp_refit_body with this header's derive step (the same device function as the score kernel's, rounded
//                     to fp32: R is a rotation by construction, there is no polar step) and 4 as the floor of a refit.
#pragma once
#include "sim3_ransac.h"

constexpr int P3P_DRAWS = 32;           // draw budget of one sample: the DLT's
constexpr int P3P_SAMPLE = 4;           // three points for the solve, the fourth picks the root
constexpr int P3P_THREADS = 256;        // hypotheses per workgroup of p3p_score_kernel
constexpr int P3P_NEWTON = 2;           // polishing Newton steps: on the resolvent cubic's root, and on each root of the quartic
constexpr double P3P_LEADING = 1e-12;   // |A4| / max |A_i| at or below which the quartic's leading coefficient vanishes
constexpr double P3P_CLOSE = 2e-6;      // relative bar on the squared side lengths a candidate must reproduce (1e-6 on the lengths)

// The minimal solve of include/fpc.h: four pairs -> R (row-major), t with X_cam = R X + t, in fp64 and in registers (every
// index is a constant once unrolled).  Contraction is off so that the score kernel and the refit kernel compute the same
// bits.  -> the sample's first pair in `first`.  false: degenerate.
__device__ __forceinline__ bool p3p_solve(const float4* __restrict__ rec, const uint32_t (&idx)[P3P_SAMPLE], const PnpArgs& g,
                                          double (&R)[9], double (&t)[3], PnpPair& first) {
#pragma clang fp contract(off)
  const double fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy;
  double X[3][3], f[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const PnpPair r = pnp_load(rec, (int)idx[i]);
    if (i == 0) first = r;
    X[i][0] = r.X; X[i][1] = r.Y; X[i][2] = r.Z;
    const double xh = ((double)r.x - cx) / fx, yh = ((double)r.y - cy) / fy;
    const double n = sqrt((xh * xh + yh * yh) + 1.0);
    f[i][0] = xh / n; f[i][1] = yh / n; f[i][2] = 1.0 / n;
  }
  const PnpPair r3 = pnp_load(rec, (int)idx[3]);
  // squared sides a2 = |X1 - X2|^2, b2 = |X0 - X2|^2, c2 = |X0 - X1|^2; cosines of the angles between the bearings
  const double e0 = X[1][0] - X[2][0], e1 = X[1][1] - X[2][1], e2 = X[1][2] - X[2][2];
  const double g0 = X[0][0] - X[2][0], g1 = X[0][1] - X[2][1], g2 = X[0][2] - X[2][2];
  const double h0 = X[0][0] - X[1][0], h1 = X[0][1] - X[1][1], h2 = X[0][2] - X[1][2];
  const double a2 = (e0 * e0 + e1 * e1) + e2 * e2, b2 = (g0 * g0 + g1 * g1) + g2 * g2, c2 = (h0 * h0 + h1 * h1) + h2 * h2;
  if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return false;              // a coincident pair of landmarks (or a NaN)
  double xt[3], yt[3], zt[3];
  if (!sim3_triad(X[0], X[1], X[2], xt, yt, zt)) return false;               // collinear landmarks
  const double ca = (f[1][0] * f[2][0] + f[1][1] * f[2][1]) + f[1][2] * f[2][2];
  const double cb = (f[0][0] * f[2][0] + f[0][1] * f[2][1]) + f[0][2] * f[2][2];
  const double cg = (f[0][0] * f[1][0] + f[0][1] * f[1][1]) + f[0][2] * f[1][2];
  const double q = (a2 - c2) / b2, r = (a2 + c2) / b2, ab = a2 / b2, cbq = c2 / b2;
  // Grunert's quartic in v = s2 / s0
  const double A4 = (q - 1.0) * (q - 1.0) - 4.0 * cbq * (ca * ca);
  const double A3 = 4.0 * ((q * (1.0 - q) * cb - (1.0 - r) * ca * cg) + 2.0 * cbq * (ca * ca) * cb);
  const double A2 = 2.0 * (((((q * q - 1.0) + 2.0 * (q * q) * (cb * cb)) + 2.0 * ((b2 - c2) / b2) * (ca * ca)) -
                            4.0 * r * ca * cb * cg) + 2.0 * ((b2 - a2) / b2) * (cg * cg));
  const double A1 = 4.0 * ((-q * (1.0 + q) * cb + 2.0 * ab * (cg * cg) * cb) - (1.0 - r) * ca * cg);
  const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * ab * (cg * cg);
  const double amax = fmax(fmax(fmax(fabs(A4), fabs(A3)), fmax(fabs(A2), fabs(A1))), fabs(A0));
  if (!(fabs(A4) > P3P_LEADING * amax) || !(amax < 1e300)) return false;     // (false for NaN)
  const double b3 = A3 / A4, bq2 = A2 / A4, b1 = A1 / A4, b0 = A0 / A4;      // monic: v^4 + b3 v^3 + bq2 v^2 + b1 v + b0
  // Ferrari.  v = y - b3 / 4:  y^4 + p y^2 + qq y + rr
  const double p = bq2 - 0.375 * (b3 * b3);
  const double qq = (b1 - 0.5 * (b3 * bq2)) + 0.125 * ((b3 * b3) * b3);
  const double rr = ((b0 - 0.25 * (b3 * b1)) + 0.0625 * ((b3 * b3) * bq2)) - 0.01171875 * ((b3 * b3) * (b3 * b3));
  // resolvent cubic m^3 + c2r m^2 + c1r m + c0r, its largest real root (> 0 unless qq = 0)
  const double c2r = p, c1r = 0.25 * (p * p) - rr, c0r = -0.125 * (qq * qq);
  const double P = c1r - (c2r * c2r) / 3.0;
  const double Q = ((2.0 * ((c2r * c2r) * c2r)) / 27.0 - (c2r * c1r) / 3.0) + c0r;
  const double D = 0.25 * (Q * Q) + ((P * P) * P) / 27.0;
  const double sd = sqrt(fmax(D, 0.0));
  const double z1 = cbrt(-0.5 * Q + sd) + cbrt(-0.5 * Q - sd);              // D > 0: the one real root
  const double rho = sqrt(fmax(-P / 3.0, 0.0));
  const double arg = fmin(1.0, fmax(-1.0, (-0.5 * Q) / ((rho * rho) * rho)));
  const double z3 = (2.0 * rho) * cos(acos(arg) / 3.0);                      // D <= 0: the largest of three
  const double z = D > 0.0 ? z1 : (rho > 0.0 ? z3 : 0.0);
  double m = z - c2r / 3.0;
#pragma unroll
  for (int i = 0; i < P3P_NEWTON; ++i) {
    const double gm = ((m + c2r) * m + c1r) * m + c0r, dm = (3.0 * m + 2.0 * c2r) * m + c1r;
    const double mn = m - gm / dm;
    m = fabs(mn) < 1e300 ? mn : m;                                           // (a zero derivative keeps m)
  }
  if (!(m > 0.0) || !(m < 1e300)) return false;
  // (y^2 + p / 2 + m)^2 = 2 m (y - qq / (4 m))^2:  y^2 - s y + (e + h) = 0  and  y^2 + s y + (e - h) = 0
  const double s = sqrt(2.0 * m), h = qq / (2.0 * s), e = 0.5 * p + m;
  const double dA = 2.0 * m - 4.0 * (e + h), dB = 2.0 * m - 4.0 * (e - h);
  const double x3 = (double)r3.x - cx, y3 = (double)r3.y - cy;
  const double X3 = r3.X, Y3 = r3.Y, Z3 = r3.Z;
  bool have = false;
  double beste = 0.0;
  // candidate k: 0, 1 the roots (s + sqrt dA) / 2, (s - sqrt dA) / 2 of the first quadratic; 2, 3 the roots
  // (-s + sqrt dB) / 2, (-s - sqrt dB) / 2 of the second.  Four trips in every lane.
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const double disc = k < 2 ? dA : dB;
    bool ok = disc >= 0.0;
    const double sq = sqrt(fmax(disc, 0.0));
    double v = 0.5 * ((k < 2 ? s : -s) + ((k & 1) ? -sq : sq)) - 0.25 * b3;
#pragma unroll
    for (int i = 0; i < P3P_NEWTON; ++i) {
      const double fv = (((v + b3) * v + bq2) * v + b1) * v + b0, dv = ((4.0 * v + 3.0 * b3) * v + 2.0 * bq2) * v + b1;
      const double vn = v - fv / dv;
      v = fabs(vn) < 1e300 ? vn : v;
    }
    ok = ok && v > 0.0;
    const double u = ((((q - 1.0) * v) * v - ((2.0 * q) * cb) * v) + (1.0 + q)) / (2.0 * (cg - v * ca));
    ok = ok && u > 0.0 && u < 1e300;                                         // (a vanishing denominator: Inf or NaN)
    const double w = (1.0 + v * v) - (2.0 * v) * cb;
    ok = ok && w > 0.0;
    const double s0 = sqrt(b2 / w), s1 = u * s0, s2 = v * s0;
    double C0[3], C1[3], C2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { C0[i] = s0 * f[0][i]; C1[i] = s1 * f[1][i]; C2[i] = s2 * f[2][i]; }
    const double m0 = C0[0] - C1[0], m1 = C0[1] - C1[1], m2 = C0[2] - C1[2];
    const double n0 = C1[0] - C2[0], n1 = C1[1] - C2[1], n2 = C1[2] - C2[2];
    const double d01 = (m0 * m0 + m1 * m1) + m2 * m2, d12 = (n0 * n0 + n1 * n1) + n2 * n2;
    ok = ok && fabs(d01 - c2) <= P3P_CLOSE * c2 && fabs(d12 - a2) <= P3P_CLOSE * a2;    // (false for NaN)
    double xq[3], yq[3], zq[3];
    ok = ok && sim3_triad(C0, C1, C2, xq, yq, zq);
    if (ok) {
      double Rk[9], tk[3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rk[i * 3 + j] = (xq[i] * xt[j] + yq[i] * yt[j]) + zq[i] * zt[j];
#pragma unroll
      for (int i = 0; i < 3; ++i) tk[i] = C0[i] - ((Rk[i * 3] * X[0][0] + Rk[i * 3 + 1] * X[0][1]) + Rk[i * 3 + 2] * X[0][2]);
      // the fourth pair: depth > 0 (the first three have s_i f_i,z > 0 by u, v > 0), squared pixel error
      const double pa = ((Rk[0] * X3 + Rk[1] * Y3) + Rk[2] * Z3) + tk[0];
      const double pb = ((Rk[3] * X3 + Rk[4] * Y3) + Rk[5] * Z3) + tk[1];
      const double pc = ((Rk[6] * X3 + Rk[7] * Y3) + Rk[8] * Z3) + tk[2];
      const double ex = fx * (pa / pc) - x3, ey = fy * (pb / pc) - y3;
      const double err = ex * ex + ey * ey;
      if (pc > 0.0 && err < 1e300 && (!have || err < beste)) {              // ties keep the lower k
        have = true;
        beste = err;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rk[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = tk[i];
      }
    }
  }
  if (!have) return false;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) finite = finite && fabs(R[i]) < 1e300;
#pragma unroll
  for (int i = 0; i < 3; ++i) finite = finite && fabs(t[i]) < 1e300;
  return finite;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// score_body's Model: PnpModel's twelve registers, threshold, records and count; the sample and its solve are this header's
struct P3pModel : PnpModel {
  static constexpr int SAMPLE = P3P_SAMPLE, DRAWS = P3P_DRAWS, REC = 2;
  __device__ __forceinline__ explicit P3pModel(const PnpArgs& a) : PnpModel(a) {}
  __device__ __forceinline__ bool solve(const PnpArgs& a, const float4* __restrict__ rec, const uint32_t (&idx)[P3P_SAMPLE],
                                        double*) {
    double R[9], t[3], P[12];
    PnpPair first;
    float P32[12];
    if (!p3p_solve(rec, idx, a, R, t, first)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      P[i * 4] = R[i * 3]; P[i * 4 + 1] = R[i * 3 + 1]; P[i * 4 + 2] = R[i * 3 + 2]; P[i * 4 + 3] = t[i];
    }
    if (!pnp_hypothesis(P, a, first, P32)) return false;
    p0 = P32[0]; p1 = P32[1]; p2 = P32[2]; p3 = P32[3]; p4 = P32[4]; p5 = P32[5];
    p6 = P32[6]; p7 = P32[7]; p8 = P32[8]; p9 = P32[9]; p10 = P32[10]; p11 = P32[11];
    return true;
  }
};

__global__ __launch_bounds__(P3P_THREADS) void p3p_score_kernel(PnpArgs a) {
  __shared__ float4 stage[2 * HF_CHUNK];                        // the staged pair chunk: the kernel's only LDS
  score_body<P3P_THREADS, P3pModel>(a, stage, nullptr);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// pnp_refit_body's Minimal: the best sample's R, t by the score kernel's device function, rounded to fp32
struct P3pMinimal {
  static constexpr int SAMPLE = P3P_SAMPLE;
  static __device__ __forceinline__ bool derive(const PnpArgs& a, const float4* __restrict__ rec, int f, unsigned long long key,
                                                int M) {
    double* const pose = pnp_refit_pose;
    uint32_t idx[P3P_SAMPLE];
    double R[9], t[3];
    PnpPair first;
    if (!(hf_sample_distinct<P3P_SAMPLE, P3P_DRAWS>(a.seed, (uint32_t)hf_frame(a.per_frame, f), ~(uint32_t)key, (uint32_t)M, idx) &&
          p3p_solve(rec, idx, a, R, t, first)))
      return false;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float v = (float)R[i];
      finite = finite && fabsf(v) < 3e38f;                        // (false for NaN and Inf)
      pose[i] = (double)v;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float v = (float)t[i];
      finite = finite && fabsf(v) < 3e38f;
      pose[9 + i] = (double)v;
    }
    return finite;
  }
};

__global__ __launch_bounds__(256) void p3p_refit_kernel(PnpArgs a, float* __restrict__ Rout, float* __restrict__ tout,
                                                        int32_t* __restrict__ ninl, uint8_t* mask, int mstride) {
  pnp_refit_body<P3pMinimal>(a, Rout, tout, ninl, mask, mstride);
}
