// Relative pose from a fundamental matrix (fpc_pose_fundamental / fpc_pose_frames / fpc_pose_bank; the rule is stated in
// include/fpc.h and restated in float64 by tests/test_pose_epipolar.py).  The pair records, their pack / gather kernels and
// the workspace are ransac_homography.h's, hf_clamp and hf_block_sum are ransac_parts.h's; the Sampson test and the Jacobi
// routine are ransac_fundamental.h's.
//
//   pose_kernel   one workgroup of 256 per frame.  One lane forms E = K_t^T F K_q, diagonalises E^T E by fm_jacobi at N = 3
//                 and builds the two rotations and the translation direction; whatever is indexed dynamically (the Jacobi
//                 matrices, the eigenvector columns, the chosen rotation) lives in LDS, so nothing spills to scratch.  All
//                 lanes then walk the pair list once, triangulating every used pair under the four candidates and counting
//                 the pairs in front (hf_block_sum<4> over 0 / 1 doubles: exact), and once more to write `front` / `xyz` of
//                 the chosen candidate through a.row.  The kernel zeroes its own rows of front / xyz first.
#pragma once
#include "ransac_fundamental.h"

constexpr double POSE_RANK = 1e-12;       // lambda2 / lambda1 of E^T E at or below which E has no plane to decompose
constexpr double POSE_PARALLEL = 1e-12;   // det / ((a.a)(b.b)) at or below which the two rays count as parallel

struct PoseArgs {
  float q_fx, q_fy, q_cx, q_cy;           // the query camera
  float t_fx, t_fy, t_cx, t_cy;           // the train camera
  int min_front;
};

// Midpoint triangulation of one pair under (R, t): a = R ph, b = qh; the ray parameters lam (query) and mu (train) that
// bring lam a + t and mu b closest.  -> the pair lies in front of both cameras.
__device__ __forceinline__ bool pose_front(const double (&R)[9], const double (&t)[3], const double (&ph)[3],
                                           const double (&qh)[3], double& lam, double& mu) {
  const double a0 = R[0] * ph[0] + R[1] * ph[1] + R[2] * ph[2];
  const double a1 = R[3] * ph[0] + R[4] * ph[1] + R[5] * ph[2];
  const double a2 = R[6] * ph[0] + R[7] * ph[1] + R[8] * ph[2];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = qh[0] * qh[0] + qh[1] * qh[1] + qh[2] * qh[2];
  const double ab = a0 * qh[0] + a1 * qh[1] + a2 * qh[2];
  const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = qh[0] * t[0] + qh[1] * t[1] + qh[2] * t[2];
  const double det = aa * bb - ab * ab;
  lam = (ab * bt - at * bb) / det;
  mu = (aa * bt - ab * at) / det;
  return det > POSE_PARALLEL * (aa * bb) && lam > 0.0 && mu > 0.0;
}

// E = K_t^T F K_q scaled to max |e| = 1 -> the rotations R_a (cand[0 .. 8]), R_b (cand[9 .. 17]) and u3 (cand[18 .. 20]) of
// include/fpc.h.  F, A, V, cand: LDS.  false: E vanishes, is not finite, or has rank below 2.  One lane.
__device__ __forceinline__ bool pose_decompose(const double* F, const PoseArgs& P, double* A, double* V, double* cand) {
  double E[9];
  {
    double G[9];                                                 // F K_q
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      G[i * 3 + 0] = F[i * 3 + 0] * (double)P.q_fx;
      G[i * 3 + 1] = F[i * 3 + 1] * (double)P.q_fy;
      G[i * 3 + 2] = F[i * 3 + 0] * (double)P.q_cx + F[i * 3 + 1] * (double)P.q_cy + F[i * 3 + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                                // K_t^T (F K_q)
      E[j] = (double)P.t_fx * G[j];
      E[3 + j] = (double)P.t_fy * G[3 + j];
      E[6 + j] = (double)P.t_cx * G[j] + (double)P.t_cy * G[3 + j] + G[6 + j];
    }
  }
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(E[i]));
  if (!(mx > 0.0) || !(mx < 1e300)) return false;               // (NaN fails the first test, Inf the second)
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = E[i] / mx;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
  fm_jacobi(A, V, 3);
  const double d0 = A[0], d1 = A[4], d2 = A[8];
  // the two largest diagonal entries in descending order, ties to the lowest index
  const int i1 = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
  const int ra = i1 == 0 ? 1 : 0, rb = i1 == 2 ? 1 : 2;         // the other two indices, ascending
  const double da = i1 == 0 ? d1 : d0, db = i1 == 2 ? d1 : d2;
  const int i2 = da >= db ? ra : rb;
  const double l1 = i1 == 0 ? d0 : (i1 == 1 ? d1 : d2), l2 = da >= db ? da : db;
  if (!(l2 > POSE_RANK * l1)) return false;                     // (false for NaN)
  const double v1[3] = {V[i1], V[3 + i1], V[6 + i1]}, v2[3] = {V[i2], V[3 + i2], V[6 + i2]};
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  double u1[3], u2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = E[i * 3] * v1[0] + E[i * 3 + 1] * v1[1] + E[i * 3 + 2] * v1[2];
    u2[i] = E[i * 3] * v2[0] + E[i * 3 + 1] * v2[1] + E[i * 3 + 2] * v2[2];
  }
  const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] = u1[i] / n1;
  const double along = u1[0] * u2[0] + u1[1] * u2[1] + u1[2] * u2[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] = u2[i] - along * u1[i];
  const double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] = u2[i] / n2;
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double s = u2[i] * v1[j] - u1[i] * v2[j], w = u3[i] * v3[j];
      cand[i * 3 + j] = s + w;
      cand[9 + i * 3 + j] = w - s;
      finite = finite && fabs(s + w) < 1e300 && fabs(w - s) < 1e300;      // (false for NaN and Inf)
    }
    cand[18 + i] = u3[i];
    finite = finite && fabs(u3[i]) < 1e300;
  }
  return finite;
}

__global__ __launch_bounds__(256) void pose_kernel(HfArgs a, PoseArgs P, const float* __restrict__ Fin, float* __restrict__ Rout,
                                                   float* __restrict__ tout, int32_t* __restrict__ nfront,
                                                   float* __restrict__ xyz, uint8_t* __restrict__ front, int ostride) {
  __shared__ double red[4 * 4];
  __shared__ double fm[9], jm[9], jv[9];
  __shared__ double cand[21];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const double thr2 = (double)a.thr * (double)a.thr;
  // this frame's rows of front / xyz, those past the pair count included
  for (int k = tid; k < ostride; k += 256) {
    if (front) front[(size_t)f * ostride + k] = 0;
    if (xyz) {
      float* x = xyz + ((size_t)f * ostride + k) * 3;
      x[0] = 0.f; x[1] = 0.f; x[2] = 0.f;
    }
  }
  double F[9];
  bool any = false, finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    F[i] = (double)Fin[f * 9 + i];
    any = any || F[i] != 0.0;
    finite = finite && fabs(F[i]) < 1e300;                       // (false for NaN and Inf)
  }
  bool ok = any && finite && M > 0;                             // (uniform)
  if (ok) {
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) fm[i] = F[i];
      solved = pose_decompose(fm, P, jm, jv, cand) ? 1 : 0;
    }
    __syncthreads();
    ok = solved != 0;
  }
  const double qfx = P.q_fx, qfy = P.q_fy, qcx = P.q_cx, qcy = P.q_cy, tfx = P.t_fx, tfy = P.t_fy, tcx = P.t_cx, tcy = P.t_cy;
  int pick = 0, total = 0;
  if (ok) {
    double Ra[9], Rb[9], tp[3], tn[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) { Ra[i] = cand[i]; Rb[i] = cand[9 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { tp[i] = cand[18 + i]; tn[i] = -cand[18 + i]; }
    double cnt[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < M; k += 256) {
      const float4 p = pairs[k];
      if (fm_inlier(F, p, thr2)) {
        const double ph[3] = {((double)p.x - qcx) / qfx, ((double)p.y - qcy) / qfy, 1.0};
        const double qh[3] = {((double)p.z - tcx) / tfx, ((double)p.w - tcy) / tfy, 1.0};
        double lam, mu;
        cnt[0] += pose_front(Ra, tp, ph, qh, lam, mu) ? 1.0 : 0.0;
        cnt[1] += pose_front(Ra, tn, ph, qh, lam, mu) ? 1.0 : 0.0;
        cnt[2] += pose_front(Rb, tp, ph, qh, lam, mu) ? 1.0 : 0.0;
        cnt[3] += pose_front(Rb, tn, ph, qh, lam, mu) ? 1.0 : 0.0;
      }
    }
    hf_block_sum<4>(cnt, red);
    double most = cnt[0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
      if (cnt[c] > most) { most = cnt[c]; pick = c; }            // ties: the lower c
    total = (int)most;
    ok = total >= P.min_front;
  }
  __syncthreads();                                               // the zeroes above are behind this barrier
  if (ok && (front || xyz)) {
    double R[9], t[3];
    const double sgn = (pick & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = cand[(pick >> 1) * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = sgn * cand[18 + i];
    for (int k = tid; k < M; k += 256) {
      const float4 p = pairs[k];
      if (!fm_inlier(F, p, thr2)) continue;
      const double ph[3] = {((double)p.x - qcx) / qfx, ((double)p.y - qcy) / qfy, 1.0};
      const double qh[3] = {((double)p.z - tcx) / tfx, ((double)p.w - tcy) / tfy, 1.0};
      double lam, mu;
      if (!pose_front(R, t, ph, qh, lam, mu)) continue;
      const size_t o = (size_t)f * ostride + a.row[(size_t)f * a.cap + k];
      if (front) front[o] = 1;
      if (xyz) {
        const double w0 = mu * qh[0] - t[0], w1 = mu * qh[1] - t[1], w2 = mu * qh[2] - t[2];   // R^T (mu qh - t)
        xyz[o * 3 + 0] = (float)(0.5 * (lam * ph[0] + (R[0] * w0 + R[3] * w1 + R[6] * w2)));
        xyz[o * 3 + 1] = (float)(0.5 * (lam * ph[1] + (R[1] * w0 + R[4] * w1 + R[7] * w2)));
        xyz[o * 3 + 2] = (float)(0.5 * (lam * ph[2] + (R[2] * w0 + R[5] * w1 + R[8] * w2)));
      }
    }
  }
  if (tid < 9) Rout[f * 9 + tid] = ok ? (float)cand[(pick >> 1) * 9 + tid] : 0.f;
  if (tid < 3) tout[f * 3 + tid] = ok ? (float)((pick & 1) ? -cand[18 + tid] : cand[18 + tid]) : 0.f;
  if (tid == 0) nfront[f] = ok ? total : 0;
}
