// Two-view bundle adjustment of a relative pose and its points (fpc_refine_pose / fpc_refine_pose_frames /
// fpc_refine_pose_bank; the rule is stated in include/fpc.h and restated in float64 by tests/test_refine_pose.py).  The pair
// records, their pack / gather kernels and the workspace are ransac_homography.h's, hf_clamp, hf_block_sum and solve_lds are
// ransac_parts.h's, pose_front is pose_epipolar.h's and lm_reprojects is landmarks.h's.
//
//   refine_pose_kernel   one workgroup of 256 per frame.  The state is (R, t) in LDS (with the gauge basis B, rebuilt with
//                 every accepted t) and one fp32 point per member in the caller's xyz, at the member's row; a row whose
//                 third coordinate is > 0 is a member (the membership pass writes the midpoints of the members and nothing
//                 else into the rows the kernel has zeroed, and a state is only ever accepted with every depth > 0).  An
//                 attempt walks the members three times at the most: the 15 + 5 + 5 sums of the reduced system (per thread
//                 over a fixed stride, then hf_block_sum), one lane's solve_lds<5> and pose update, the cost of the stepped
//                 state (every point stepped in registers), and -- on accept only -- the same step once more, written.  A
//                 thread reads and writes only its own rows of xyz, so the passes need no barrier of their own.  Every
//                 decision (reject, accept, stop) is taken from block sums or LDS: the loops are uniform around the barriers.
//                 Nothing is indexed dynamically outside LDS.
#pragma once
#include "pose_epipolar.h"
#include "landmarks.h"

constexpr int RP_NSUM = 25;               // S (upper triangle, row-major: 15), diag A (5), b (5)
constexpr double RP_SINGULAR = 1e-14;     // pivot floor of the 5 x 5 solve, of the largest diagonal entry of S
constexpr double RP_TMIN = 1e-12;         // |t'| at or below which an attempt is rejected
constexpr double RP_STOP = 1e-6;          // an accepted step that gains no more than this share of C ends the call
constexpr double RP_LAMBDA_MIN = 1e-10, RP_LAMBDA_MAX = 1e6;

struct RefineArgs {
  float q_fx, q_fy, q_cx, q_cy;           // the query camera
  float t_fx, t_fy, t_cx, t_cy;           // the train camera
  double parallax;                        // sin^2(min_parallax_deg) (the pose calls' floor at 0 degrees); below that floor
                                          // pose_front's own test decides
  int iterations;
  float lambda0;
  int min_front;
};

// the two cameras and the threshold, in fp64 registers
struct RpCams {
  double qfx, qfy, qcx, qcy, tfx, tfy, tcx, tcy, thr2;
};

// B = [b1 b2], orthonormal and orthogonal to t: b1 = (t x e_k) / |t x e_k| with k the index of the smallest |t_k| (ties to
// the lowest), b2 = (t x b1) / |t x b1|.  -> out[0 .. 2] = b1, out[3 .. 5] = b2
__device__ __forceinline__ void rp_basis(double t0, double t1, double t2, double* out) {
  const double a0 = fabs(t0), a1 = fabs(t1), a2 = fabs(t2);
  const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
  double c0 = k == 0 ? 0.0 : (k == 1 ? -t2 : t1);
  double c1 = k == 0 ? t2 : (k == 1 ? 0.0 : -t0);
  double c2 = k == 0 ? -t1 : (k == 1 ? t0 : 0.0);
  const double n1 = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
  c0 = c0 / n1; c1 = c1 / n1; c2 = c2 / n1;
  double d0 = t1 * c2 - t2 * c1, d1 = t2 * c0 - t0 * c2, d2 = t0 * c1 - t1 * c0;
  const double n2 = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  out[0] = c0; out[1] = c1; out[2] = c2;
  out[3] = d0 / n2; out[4] = d1 / n2; out[5] = d2 / n2;
}

// |pi_q(X) - p|^2 + |pi_t(R X + t) - q|^2 of one member; +inf with a depth that is not > 0 in either camera
__device__ __forceinline__ double rp_cost(const double (&R)[9], const double (&t)[3], const RpCams& g, const float4 p,
                                          double X0, double X1, double X2) {
#pragma clang fp contract(off)
  const double a = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0];
  const double b = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1];
  const double c = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
  if (!(X2 > 0.0) || !(c > 0.0)) return __builtin_inf();
  const double e0 = g.qfx * (X0 / X2) + g.qcx - (double)p.x, e1 = g.qfy * (X1 / X2) + g.qcy - (double)p.y;
  const double e2 = g.tfx * (a / c) + g.tcx - (double)p.z, e3 = g.tfy * (b / c) + g.tcy - (double)p.w;
  return (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
}

// Contraction is off in rp_cost, rp_blocks, rp_invert and rp_step_point (as in landmarks_rule): the kernel inlines the step
// twice, for the cost of the stepped state and to write it on accept, and both must compute the same bits.
// what a member contributes at the state (R, t, B, X): U (symmetric: 00 01 02 11 12 22), W (5 x 3), g_X, J_c (2 x 5), r_t
struct RpBlocks {
  double U[6], W[15], gX[3], Jc[10], rt[2];
};

__device__ __forceinline__ void rp_blocks(const double (&R)[9], const double (&t)[3], const double (&B)[6], const RpCams& g,
                                          const float4 p, double X0, double X1, double X2, RpBlocks& o) {
#pragma clang fp contract(off)
  const double a = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0];
  const double b = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1];
  const double c = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
  const double iz = 1.0 / X2, ic = 1.0 / c;
  const double rq[2] = {g.qfx * (X0 * iz) + g.qcx - (double)p.x, g.qfy * (X1 * iz) + g.qcy - (double)p.y};
  o.rt[0] = g.tfx * (a * ic) + g.tcx - (double)p.z;
  o.rt[1] = g.tfy * (b * ic) + g.tcy - (double)p.w;
  // the projection Jacobians at X (query) and at X_c (train): rows (fx / z, 0, -fx x / z^2), (0, fy / z, -fy y / z^2)
  const double Jq[6] = {g.qfx * iz, 0.0, -g.qfx * X0 * iz * iz, 0.0, g.qfy * iz, -g.qfy * X1 * iz * iz};
  const double Jp[6] = {g.tfx * ic, 0.0, -g.tfx * a * ic * ic, 0.0, g.tfy * ic, -g.tfy * b * ic * ic};
  double Jt[6];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Jt[i * 3 + j] = Jp[i * 3] * R[j] + Jp[i * 3 + 1] * R[3 + j] + Jp[i * 3 + 2] * R[6 + j];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    o.Jc[i * 5 + 0] = -(Jp[i * 3 + 1] * c - Jp[i * 3 + 2] * b);          // -J_p [X_c]x
    o.Jc[i * 5 + 1] = -(Jp[i * 3 + 2] * a - Jp[i * 3] * c);
    o.Jc[i * 5 + 2] = -(Jp[i * 3] * b - Jp[i * 3 + 1] * a);
    o.Jc[i * 5 + 3] = Jp[i * 3] * B[0] + Jp[i * 3 + 1] * B[1] + Jp[i * 3 + 2] * B[2];   // J_p B
    o.Jc[i * 5 + 4] = Jp[i * 3] * B[3] + Jp[i * 3 + 1] * B[4] + Jp[i * 3 + 2] * B[5];
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) o.U[q++] = (Jq[i] * Jq[j] + Jq[3 + i] * Jq[3 + j]) + (Jt[i] * Jt[j] + Jt[3 + i] * Jt[3 + j]);
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.W[i * 3 + j] = o.Jc[i] * Jt[j] + o.Jc[5 + i] * Jt[3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) o.gX[j] = (Jq[j] * rq[0] + Jq[3 + j] * rq[1]) + (Jt[j] * o.rt[0] + Jt[3 + j] * o.rt[1]);
}

// (U + lambda diag U)^-1 as adjugate over determinant (symmetric: 00 01 02 11 12 22); false: det not > 0 or not finite
__device__ __forceinline__ bool rp_invert(const double (&U)[6], double lambda, double (&V)[6]) {
#pragma clang fp contract(off)
  const double u00 = U[0] + lambda * U[0], u01 = U[1], u02 = U[2], u11 = U[3] + lambda * U[3], u12 = U[4],
               u22 = U[5] + lambda * U[5];
  const double c00 = u11 * u22 - u12 * u12, c01 = u02 * u12 - u01 * u22, c02 = u01 * u12 - u02 * u11;
  const double c11 = u00 * u22 - u02 * u02, c12 = u01 * u02 - u00 * u12, c22 = u00 * u11 - u01 * u01;
  const double det = (u00 * c00 + u01 * c01) + u02 * c02;
  V[0] = c00 / det; V[1] = c01 / det; V[2] = c02 / det; V[3] = c11 / det; V[4] = c12 / det; V[5] = c22 / det;
  return det > 0.0 && det < 1e300;                               // (false for NaN and Inf)
}

// the stepped point of a member: X' = s (X + dX), dX = -U*^-1 (g_X + W^T delta), rounded to fp32.  false: no inverse
__device__ __forceinline__ bool rp_step_point(const double (&R)[9], const double (&t)[3], const double (&B)[6], const RpCams& g,
                                              const float4 p, double lambda, const double (&d)[5], double sc, double X0,
                                              double X1, double X2, float& Y0, float& Y1, float& Y2) {
#pragma clang fp contract(off)
  RpBlocks k;
  rp_blocks(R, t, B, g, p, X0, X1, X2, k);
  double V[6];
  const bool ok = rp_invert(k.U, lambda, V);
  double h[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    h[j] = k.gX[j] + ((((k.W[j] * d[0] + k.W[3 + j] * d[1]) + k.W[6 + j] * d[2]) + k.W[9 + j] * d[3]) + k.W[12 + j] * d[4]);
  Y0 = (float)(sc * (X0 - ((V[0] * h[0] + V[1] * h[1]) + V[2] * h[2])));
  Y1 = (float)(sc * (X1 - ((V[1] * h[0] + V[3] * h[1]) + V[4] * h[2])));
  Y2 = (float)(sc * (X2 - ((V[2] * h[0] + V[4] * h[1]) + V[5] * h[2])));
  return ok;
}

// R' = E(omega) R, t' = (E t + B eta) / |E t + B eta| from the solution d = (omega, eta), rounded to fp32 -> nxt[0 .. 11],
// nxt[12] = s = 1 / |E t + B eta|, nxt[13 .. 17] = d.  cur: R (9), t (3), B (6).  false: |t'| not > RP_TMIN.  One lane.
__device__ __forceinline__ bool rp_step_pose(const double* cur, const double (&d)[5], double* nxt) {
  const double w0 = d[0], w1 = d[1], w2 = d[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double A = 1.0, Bc = 0.5;
  if (!(th2 < 1e-16)) {
    const double th = sqrt(th2);
    A = sin(th) / th;
    Bc = (1.0 - cos(th)) / th2;
  }
  // E = I + A [w]x + B [w]x^2,  [w]x^2 = w w^T - |w|^2 I
  const double E[9] = {1.0 + Bc * (w0 * w0 - th2), -A * w2 + Bc * w0 * w1, A * w1 + Bc * w0 * w2,
                       A * w2 + Bc * w0 * w1, 1.0 + Bc * (w1 * w1 - th2), -A * w0 + Bc * w1 * w2,
                       -A * w1 + Bc * w0 * w2, A * w0 + Bc * w1 * w2, 1.0 + Bc * (w2 * w2 - th2)};
  double tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      nxt[i * 3 + j] = (double)(float)(E[i * 3] * cur[j] + E[i * 3 + 1] * cur[3 + j] + E[i * 3 + 2] * cur[6 + j]);
    tn[i] = (E[i * 3] * cur[9] + E[i * 3 + 1] * cur[10] + E[i * 3 + 2] * cur[11]) + (cur[12 + i] * d[3] + cur[15 + i] * d[4]);
  }
  const double n = sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
  if (!(n > RP_TMIN)) return false;                              // (false for NaN)
  const double sc = 1.0 / n;
#pragma unroll
  for (int i = 0; i < 3; ++i) nxt[9 + i] = (double)(float)(sc * tn[i]);
  nxt[12] = sc;
#pragma unroll
  for (int i = 0; i < 5; ++i) nxt[13 + i] = d[i];
  return true;
}

// (xyz is read and written through this one pointer; R / t may alias Rin / tin: every thread has read its inputs before the
// first barrier, and the outputs are written behind the last)
__global__ __launch_bounds__(256) void refine_pose_kernel(HfArgs a, RefineArgs P, const float* Rin, const float* tin, float* Rout,
                                                          float* tout, int32_t* __restrict__ nfront, float* xyz,
                                                          uint8_t* __restrict__ front, float* __restrict__ stats, int ostride) {
  __shared__ double red[4 * RP_NSUM];
  __shared__ double s25[RP_NSUM];
  __shared__ double sm[5][6];
  __shared__ double cur[18], nxt[18];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const int32_t* __restrict__ row = a.row + (size_t)f * a.cap;
  float* X = xyz + (size_t)f * ostride * 3;
  RpCams g;
  g.qfx = P.q_fx; g.qfy = P.q_fy; g.qcx = P.q_cx; g.qcy = P.q_cy;
  g.tfx = P.t_fx; g.tfy = P.t_fy; g.tcx = P.t_cx; g.tcy = P.t_cy;
  g.thr2 = (double)a.thr * (double)a.thr;
  // this frame's rows of front / xyz, those past the pair count included
  for (int k = tid; k < ostride; k += 256) {
    if (front) front[(size_t)f * ostride + k] = 0;
    X[k * 3 + 0] = 0.f; X[k * 3 + 1] = 0.f; X[k * 3 + 2] = 0.f;
  }
  double R[9], t[3], B[6];
  bool any = false, finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    R[i] = (double)Rin[f * 9 + i];
    any = any || R[i] != 0.0;
    finite = finite && fabs(R[i]) < 1e300;                       // (false for NaN and Inf)
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = (double)tin[f * 3 + i];
    finite = finite && fabs(t[i]) < 1e300;
  }
  const double tlen = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  bool ok = any && finite && tlen > 0.0 && M > 0;               // (uniform)
  if (ok && tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) cur[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cur[9 + i] = (double)(float)(t[i] / tlen);
    rp_basis(cur[9], cur[10], cur[11], cur + 12);
  }
  __syncthreads();                                               // (the zeroes above are behind this barrier too)
  double m = 0.0, C = 0.0, C0 = 0.0;
  int made = 0, accepted = 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = cur[9 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) B[i] = cur[12 + i];
    // the members: their midpoints, rounded to fp32, are the start; C of that state
    double s2[2] = {0.0, 0.0};
    for (int k = tid; k < M; k += 256) {
      const float4 p = pairs[k];
      const double ph[3] = {((double)p.x - g.qcx) / g.qfx, ((double)p.y - g.qcy) / g.qfy, 1.0};
      const double qh[3] = {((double)p.z - g.tcx) / g.tfx, ((double)p.w - g.tcy) / g.tfy, 1.0};
      const double a0 = R[0] * ph[0] + R[1] * ph[1] + R[2] * ph[2], a1 = R[3] * ph[0] + R[4] * ph[1] + R[5] * ph[2],
                   a2 = R[6] * ph[0] + R[7] * ph[1] + R[8] * ph[2];
      const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = qh[0] * qh[0] + qh[1] * qh[1] + qh[2] * qh[2];
      const double ab = a0 * qh[0] + a1 * qh[1] + a2 * qh[2];
      double lam, mu;
      if (!pose_front(R, t, ph, qh, lam, mu)) continue;
      if (!(aa * bb - ab * ab > P.parallax * (aa * bb))) continue;
      const double w0 = mu * qh[0] - t[0], w1 = mu * qh[1] - t[1], w2 = mu * qh[2] - t[2];     // R^T (mu qh - t)
      const double X0 = 0.5 * (lam * ph[0] + (R[0] * w0 + R[3] * w1 + R[6] * w2));
      const double X1 = 0.5 * (lam * ph[1] + (R[1] * w0 + R[4] * w1 + R[7] * w2));
      const double X2 = 0.5 * (lam * ph[2] + (R[2] * w0 + R[5] * w1 + R[8] * w2));
      const double c0 = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0], c1 = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1],
                   c2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
      if (!lm_reprojects(g.qfx, g.qfy, g.qcx, g.qcy, (double)p.x, (double)p.y, X0, X1, X2, g.thr2)) continue;
      if (!lm_reprojects(g.tfx, g.tfy, g.tcx, g.tcy, (double)p.z, (double)p.w, c0, c1, c2, g.thr2)) continue;
      const float Y0 = (float)X0, Y1 = (float)X1, Y2 = (float)X2;
      if (!(Y2 > 0.f)) continue;                                 // (a depth below the least fp32: no point to refine)
      const int o = row[k];
      X[o * 3 + 0] = Y0; X[o * 3 + 1] = Y1; X[o * 3 + 2] = Y2;
      s2[0] += 1.0;
      s2[1] += rp_cost(R, t, g, p, (double)Y0, (double)Y1, (double)Y2);
    }
    hf_block_sum<2>(s2, red);
    m = s2[0];
    C = C0 = s2[1];
    ok = (int)m >= P.min_front;                                  // (the final count cannot exceed the members)
  }
  if (ok) {
    double lambda = (double)P.lambda0;
    for (int it = 0; it < P.iterations; ++it) {
      ++made;
      // the reduced system at the current state
      double s[RP_NSUM];
#pragma unroll
      for (int i = 0; i < RP_NSUM; ++i) s[i] = 0.0;
      int bad = 0;
      for (int k = tid; k < M; k += 256) {
        const int o = row[k];
        const float z = X[o * 3 + 2];
        if (!(z > 0.f)) continue;
        RpBlocks b;
        rp_blocks(R, t, B, g, pairs[k], (double)X[o * 3], (double)X[o * 3 + 1], (double)z, b);
        double V[6];
        if (!rp_invert(b.U, lambda, V)) { bad = 1; continue; }
        double Y[15];                                            // W U*^-1
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const double x0 = b.W[i * 3], x1 = b.W[i * 3 + 1], x2 = b.W[i * 3 + 2];
          Y[i * 3 + 0] = (x0 * V[0] + x1 * V[1]) + x2 * V[2];
          Y[i * 3 + 1] = (x0 * V[1] + x1 * V[3]) + x2 * V[4];
          Y[i * 3 + 2] = (x0 * V[2] + x1 * V[4]) + x2 * V[5];
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
#pragma unroll
          for (int j = i; j < 5; ++j)
            s[q++] += (b.Jc[i] * b.Jc[j] + b.Jc[5 + i] * b.Jc[5 + j]) -
                      ((Y[i * 3] * b.W[j * 3] + Y[i * 3 + 1] * b.W[j * 3 + 1]) + Y[i * 3 + 2] * b.W[j * 3 + 2]);
          s[15 + i] += b.Jc[i] * b.Jc[i] + b.Jc[5 + i] * b.Jc[5 + i];
          s[20 + i] += (b.Jc[i] * b.rt[0] + b.Jc[5 + i] * b.rt[1]) -
                       ((Y[i * 3] * b.gX[0] + Y[i * 3 + 1] * b.gX[1]) + Y[i * 3 + 2] * b.gX[2]);
        }
      }
      bad = __syncthreads_or(bad);
      hf_block_sum<RP_NSUM>(s, red);
      if (tid == 0) {
        int good = bad ? 0 : 1;
        if (good) {
#pragma unroll
          for (int i = 0; i < RP_NSUM; ++i) s25[i] = s[i];       // (through LDS: s[dynamic] would be scratch)
          int q = 0;
          double dmax = 0.0;
          for (int i = 0; i < 5; ++i) {
            for (int j = i; j < 5; ++j) { sm[i][j] = s25[q]; sm[j][i] = s25[q]; ++q; }
            sm[i][i] += lambda * s25[15 + i];
            sm[i][5] = -s25[20 + i];
            dmax = fmax(dmax, fabs(sm[i][i]));
          }
          good = solve_lds<5>(sm, RP_SINGULAR * dmax) ? 1 : 0;
        }
        if (good) {
          const double d[5] = {sm[0][5], sm[1][5], sm[2][5], sm[3][5], sm[4][5]};
          good = rp_step_pose(cur, d, nxt) ? 1 : 0;
        }
        solved = good;
      }
      __syncthreads();
      const bool good = solved != 0;                             // (the next write of solved is behind hf_block_sum's barriers)
      double Rn[9], tn[3], d[5], sc = 0.0, Cn = 0.0;
      if (good) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Rn[i] = nxt[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tn[i] = nxt[9 + i];
        sc = nxt[12];
#pragma unroll
        for (int i = 0; i < 5; ++i) d[i] = nxt[13 + i];
        // C' of the stepped state
        double c1[1] = {0.0};
        for (int k = tid; k < M; k += 256) {
          const int o = row[k];
          const float z = X[o * 3 + 2];
          if (!(z > 0.f)) continue;
          const float4 p = pairs[k];
          float Y0, Y1, Y2;
          rp_step_point(R, t, B, g, p, lambda, d, sc, (double)X[o * 3], (double)X[o * 3 + 1], (double)z, Y0, Y1, Y2);
          c1[0] += rp_cost(Rn, tn, g, p, (double)Y0, (double)Y1, (double)Y2);
        }
        hf_block_sum<1>(c1, red);
        Cn = c1[0];
      }
      if (good && Cn < C) {                                      // (false for NaN; uniform)
        for (int k = tid; k < M; k += 256) {                     // the same step once more, written
          const int o = row[k];
          const float z = X[o * 3 + 2];
          if (!(z > 0.f)) continue;
          float Y0, Y1, Y2;
          rp_step_point(R, t, B, g, pairs[k], lambda, d, sc, (double)X[o * 3], (double)X[o * 3 + 1], (double)z, Y0, Y1, Y2);
          X[o * 3 + 0] = Y0; X[o * 3 + 1] = Y1; X[o * 3 + 2] = Y2;
        }
        if (tid == 0) {
#pragma unroll
          for (int i = 0; i < 12; ++i) cur[i] = nxt[i];
          rp_basis(cur[9], cur[10], cur[11], cur + 12);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = cur[i];               // (the next write of cur is behind the next attempt's barriers)
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = cur[9 + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) B[i] = cur[12 + i];
        const double gain = C - Cn, before = C;
        C = Cn;
        ++accepted;
        lambda = fmax(lambda / 10.0, RP_LAMBDA_MIN);
        if (gain <= RP_STOP * before) break;
      } else {
        lambda = fmin(10.0 * lambda, RP_LAMBDA_MAX);
      }
    }
    // the members that lie in front of both cameras and pass both tests at the final state; the others lose their point
    double c1[1] = {0.0};
    for (int k = tid; k < M; k += 256) {
      const int o = row[k];
      const float z = X[o * 3 + 2];
      if (!(z > 0.f)) continue;
      const float4 p = pairs[k];
      const double X0 = (double)X[o * 3], X1 = (double)X[o * 3 + 1], X2 = (double)z;
      const double c0 = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0], cc1 = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1],
                   c2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
      const bool keep = lm_reprojects(g.qfx, g.qfy, g.qcx, g.qcy, (double)p.x, (double)p.y, X0, X1, X2, g.thr2) &&
                        lm_reprojects(g.tfx, g.tfy, g.tcx, g.tcy, (double)p.z, (double)p.w, c0, cc1, c2, g.thr2);
      if (keep) {
        c1[0] += 1.0;
      } else {
        X[o * 3 + 0] = 0.f; X[o * 3 + 1] = 0.f; X[o * 3 + 2] = 0.f;
      }
    }
    hf_block_sum<1>(c1, red);
    const int total = (int)c1[0];
    ok = total >= P.min_front;
    for (int k = tid; k < M; k += 256) {
      const int o = row[k];
      if (!(X[o * 3 + 2] > 0.f)) continue;
      if (ok) {
        if (front) front[(size_t)f * ostride + o] = 1;
      } else {
        X[o * 3 + 0] = 0.f; X[o * 3 + 1] = 0.f; X[o * 3 + 2] = 0.f;
      }
    }
    if (tid == 0) nfront[f] = ok ? total : 0;
  } else {
    for (int k = tid; k < M; k += 256) {                         // (members short of min_front: their midpoints go again)
      const int o = row[k];
      X[o * 3 + 0] = 0.f; X[o * 3 + 1] = 0.f; X[o * 3 + 2] = 0.f;
    }
    if (tid == 0) nfront[f] = 0;
  }
  // (cur was last written behind a barrier every thread has passed; with !ok it is not read)
  if (tid < 9) Rout[f * 9 + tid] = ok ? (float)cur[tid] : 0.f;
  if (tid < 3) tout[f * 3 + tid] = ok ? (float)cur[9 + tid] : 0.f;
  if (stats && tid < 4) {
    const double v = tid == 0 ? sqrt(C0 / (2.0 * m)) : (tid == 1 ? sqrt(C / (2.0 * m)) : (tid == 2 ? (double)made : (double)accepted));
    stats[f * 4 + tid] = ok ? (float)v : 0.f;
  }
}
