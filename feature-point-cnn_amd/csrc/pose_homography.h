// Relative pose from a homography (fpc_pose_homography / fpc_pose_homography_frames / fpc_pose_homography_bank; the rule is
// stated in include/fpc.h and restated in float64 by tests/test_pose_homography.py).  The pair records, their pack / gather
// kernels, the workspace and the reprojection test (hf_inlier) are ransac_homography.h's, hf_clamp and hf_block_sum are
// ransac_parts.h's, the Sampson test and the Jacobi routine are ransac_fundamental.h's, the triangulation (pose_front) is
// pose_epipolar.h's.
//
//   pose_homography_kernel   one workgroup of 256 per frame.  One lane forms H^ = K_t^-1 H K_q, diagonalises H^T H^ by
//                 fm_jacobi at N = 3 and builds either the rotation of a frame without baseline or the two (R, T, N) of the
//                 four-solution form with their F = K_t^-T [t]x R K_q^-1; whatever is indexed dynamically (the Jacobi
//                 matrices, the eigenvector columns, the candidate table, the counts) lives in LDS, so nothing spills to
//                 scratch.  All lanes then walk the pair list once for the eight counts -- per candidate the plane pairs in
//                 front and the support (hf_block_sum<8> over 0 / 1 doubles: exact); F_c and -F_c give the same Sampson
//                 distance, so two rotations, two translations and two F in registers serve all four candidates -- and
//                 once more to write `front` / `xyz` of solution `which` through a.row.  The kernel zeroes its own rows of
//                 front / xyz first.
#pragma once
#include "pose_epipolar.h"

constexpr double POSE_H_RANK = 1e-12;     // lambda3 / lambda1 of H^T H^ at or below which H has no inverse to speak of
constexpr int POSE_H_SIGN = 25;           // doubles of one sign's table entry: R [9], t [3], N [3], |T|, F [9]

struct PoseHArgs {
  float q_fx, q_fy, q_cx, q_cy;           // the query camera
  float t_fx, t_fy, t_cx, t_cy;           // the train camera
  int min_front;
  float min_baseline;
  int which;
};

// outcome of the decomposition (the kernel's mode): nothing, two signs' candidates in the table, a rotation in tab[0 .. 8]
enum { POSE_H_NONE = 0, POSE_H_CANDIDATES = 1, POSE_H_ROTATION = 2 };

// One sign of the four-solution form: u = (a v1 + sc v3) / e -> R, t = T / |T|, N, |T| and F into e (LDS, POSE_H_SIGN
// doubles).  Hn: the normalised H^ (LDS).  -> every value finite.  One lane.
__device__ __forceinline__ bool pose_h_sign(const double* Hn, const PoseHArgs& P, const double (&v1)[3], const double (&v2)[3],
                                            const double (&v3)[3], double a, double sc, double e, double* out) {
  double u[3], n[3], w0[3], w1[3], w2[3], R[9], T[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = (a * v1[i] + sc * v3[i]) / e;
  n[0] = v2[1] * u[2] - v2[2] * u[1]; n[1] = v2[2] * u[0] - v2[0] * u[2]; n[2] = v2[0] * u[1] - v2[1] * u[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    w0[i] = Hn[i * 3] * v2[0] + Hn[i * 3 + 1] * v2[1] + Hn[i * 3 + 2] * v2[2];
    w1[i] = Hn[i * 3] * u[0] + Hn[i * 3 + 1] * u[1] + Hn[i * 3 + 2] * u[2];
  }
  w2[0] = w0[1] * w1[2] - w0[2] * w1[1]; w2[1] = w0[2] * w1[0] - w0[0] * w1[2]; w2[2] = w0[0] * w1[1] - w0[1] * w1[0];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = w0[i] * v2[j] + w1[i] * u[j] + w2[i] * n[j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    T[i] = (Hn[i * 3] - R[i * 3]) * n[0] + (Hn[i * 3 + 1] - R[i * 3 + 1]) * n[1] + (Hn[i * 3 + 2] - R[i * 3 + 2]) * n[2];
  const double len = sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
  const double t[3] = {T[0] / len, T[1] / len, T[2] / len};
  // F = K_t^-T ([t]x R) K_q^-1
  double E[9], G[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                  // E K_q^-1
    G[i * 3 + 0] = E[i * 3 + 0] / (double)P.q_fx;
    G[i * 3 + 1] = E[i * 3 + 1] / (double)P.q_fy;
    G[i * 3 + 2] = E[i * 3 + 2] - G[i * 3 + 0] * (double)P.q_cx - G[i * 3 + 1] * (double)P.q_cy;
  }
  bool finite = fabs(1.0 / len) < 1e300;                         // (false for NaN and Inf: T = 0 has no direction)
#pragma unroll
  for (int j = 0; j < 3; ++j) {                                  // K_t^-T (E K_q^-1)
    const double f0 = G[j] / (double)P.t_fx, f1 = G[3 + j] / (double)P.t_fy;
    const double f2 = G[6 + j] - f0 * (double)P.t_cx - f1 * (double)P.t_cy;
    out[16 + j] = f0; out[19 + j] = f1; out[22 + j] = f2;
    finite = finite && fabs(f0) < 1e300 && fabs(f1) < 1e300 && fabs(f2) < 1e300;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    out[i] = R[i];
    finite = finite && fabs(R[i]) < 1e300;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out[9 + i] = t[i]; out[12 + i] = n[i];
    finite = finite && fabs(t[i]) < 1e300 && fabs(n[i]) < 1e300;
  }
  out[15] = len;
  return finite;
}

// H^ = K_t^-1 H K_q scaled to max |h^| = 1 -> the mode; POSE_H_CANDIDATES: tab holds the + and the - sign's entries and
// fin[s] whether sign s is finite; POSE_H_ROTATION: tab[0 .. 8] holds R.  H: fp64 of the fp32 input; A, V, Hn, tab: LDS.  One
// lane.
__device__ __forceinline__ int pose_h_decompose(const double (&H)[9], const PoseHArgs& P, double* A, double* V, double* Hn,
                                                double* tab, int* fin) {
  {
    double G[9];                                                 // H K_q
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      G[i * 3 + 0] = H[i * 3 + 0] * (double)P.q_fx;
      G[i * 3 + 1] = H[i * 3 + 1] * (double)P.q_fy;
      G[i * 3 + 2] = H[i * 3 + 0] * (double)P.q_cx + H[i * 3 + 1] * (double)P.q_cy + H[i * 3 + 2];
    }
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {                                // K_t^-1 (H K_q)
      G[j] = (G[j] - (double)P.t_cx * G[6 + j]) / (double)P.t_fx;
      G[3 + j] = (G[3 + j] - (double)P.t_cy * G[6 + j]) / (double)P.t_fy;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(G[i]));
    if (!(mx > 0.0) || !(mx < 1e300)) return POSE_H_NONE;       // (NaN fails the first test, Inf the second)
#pragma unroll
    for (int i = 0; i < 9; ++i) Hn[i] = G[i] / mx;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = Hn[i] * Hn[j] + Hn[3 + i] * Hn[3 + j] + Hn[6 + i] * Hn[6 + j];
  fm_jacobi(A, V, 3);
  const double d0 = A[0], d1 = A[4], d2 = A[8];
  // the diagonal entries in descending order, ties to the lowest index
  const int i1 = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
  const int ra = i1 == 0 ? 1 : 0, rb = i1 == 2 ? 1 : 2;         // the other two indices, ascending
  const double da = i1 == 0 ? d1 : d0, db = i1 == 2 ? d1 : d2;
  const int i2 = da >= db ? ra : rb;
  double l1 = i1 == 0 ? d0 : (i1 == 1 ? d1 : d2), l3 = da >= db ? db : da;
  const double l2 = da >= db ? da : db;
  if (!(l3 > POSE_H_RANK * l1)) return POSE_H_NONE;             // (false for NaN)
  const double s2 = sqrt(l2);
  l1 = l1 / l2; l3 = l3 / l2;
  double h[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = Hn[i] / s2;
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  const double sg = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) Hn[i] = sg * h[i];
  const double v1[3] = {V[i1], V[3 + i1], V[6 + i1]}, v2[3] = {V[i2], V[3 + i2], V[6 + i2]};
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  const double b = sqrt(l1) - sqrt(l3);
  if (!(b > (double)P.min_baseline)) {                           // no baseline to speak of: a rotation (a NaN b as well: it
    double w1[3], w2[3];                                         //  fails the finite test below)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w1[i] = Hn[i * 3] * v1[0] + Hn[i * 3 + 1] * v1[1] + Hn[i * 3 + 2] * v1[2];
      w2[i] = Hn[i * 3] * v2[0] + Hn[i * 3 + 1] * v2[1] + Hn[i * 3 + 2] * v2[2];
    }
    const double n1 = sqrt(w1[0] * w1[0] + w1[1] * w1[1] + w1[2] * w1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) w1[i] = w1[i] / n1;
    const double along = w1[0] * w2[0] + w1[1] * w2[1] + w1[2] * w2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) w2[i] = w2[i] - along * w1[i];
    const double n2 = sqrt(w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) w2[i] = w2[i] / n2;
    const double w3[3] = {w1[1] * w2[2] - w1[2] * w2[1], w1[2] * w2[0] - w1[0] * w2[2], w1[0] * w2[1] - w1[1] * w2[0]};
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double r = w1[i] * v1[j] + w2[i] * v2[j] + w3[i] * v3[j];
        tab[i * 3 + j] = r;
        finite = finite && fabs(r) < 1e300;                      // (false for NaN and Inf)
      }
    return finite ? POSE_H_ROTATION : POSE_H_NONE;
  }
  const double a = sqrt(fmax(0.0, 1.0 - l3)), c = sqrt(fmax(0.0, l1 - 1.0)), e = sqrt(l1 - l3);
  fin[0] = pose_h_sign(Hn, P, v1, v2, v3, a, c, e, tab) ? 1 : 0;
  fin[1] = pose_h_sign(Hn, P, v1, v2, v3, a, -c, e, tab + POSE_H_SIGN) ? 1 : 0;
  return POSE_H_CANDIDATES;
}

__global__ __launch_bounds__(256) void pose_homography_kernel(HfArgs a, PoseHArgs P, const float* __restrict__ Hin,
                                                              int32_t* __restrict__ kind, float* __restrict__ Rout,
                                                              float* __restrict__ tout, float* __restrict__ plane,
                                                              int32_t* __restrict__ nfront, int32_t* __restrict__ nplane,
                                                              float* __restrict__ xyz, uint8_t* __restrict__ front, int ostride) {
  __shared__ double red[4 * 8];
  __shared__ double jm[9], jv[9], hn[9];
  __shared__ double tab[2 * POSE_H_SIGN];
  __shared__ int cnts[8];
  __shared__ int fin[2];
  __shared__ int mode_s;
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
  double H[9];
  bool any = false, finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    H[i] = (double)Hin[f * 9 + i];
    any = any || H[i] != 0.0;
    finite = finite && fabs(H[i]) < 1e300;                       // (false for NaN and Inf)
  }
  int mode = POSE_H_NONE;
  if (any && finite && M > 0) {                                  // (uniform)
    if (tid == 0) mode_s = pose_h_decompose(H, P, jm, jv, hn, tab, fin);
    __syncthreads();
    mode = mode_s;
  }
  const double qfx = P.q_fx, qfy = P.q_fy, qcx = P.q_cx, qcy = P.q_cy, tfx = P.t_fx, tfy = P.t_fy, tcx = P.t_cx, tcy = P.t_cy;
  int s0 = -1, s1 = -1, left = 0;                                // the candidates of solutions 0 and 1; how many remain
  if (mode == POSE_H_CANDIDATES) {
    double Rp[9], Rm[9], tp[3], tm[3], tpn[3], tmn[3], Fp[9], Fm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      Rp[i] = tab[i]; Rm[i] = tab[POSE_H_SIGN + i];
      Fp[i] = tab[16 + i]; Fm[i] = tab[POSE_H_SIGN + 16 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      tp[i] = tab[9 + i]; tpn[i] = -tab[9 + i];
      tm[i] = tab[POSE_H_SIGN + 9 + i]; tmn[i] = -tab[POSE_H_SIGN + 9 + i];
    }
    double cnt[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};    // nplane of c = 0 .. 3, then nfront of c = 0 .. 3
    for (int k = tid; k < M; k += 256) {
      const float4 p = pairs[k];
      const double ph[3] = {((double)p.x - qcx) / qfx, ((double)p.y - qcy) / qfy, 1.0};
      const double qh[3] = {((double)p.z - tcx) / tfx, ((double)p.w - tcy) / tfy, 1.0};
      const bool on = hf_inlier(H, p, thr2), ep = fm_inlier(Fp, p, thr2), em = fm_inlier(Fm, p, thr2);
      double lam, mu;
      const bool f0 = pose_front(Rp, tp, ph, qh, lam, mu), f1 = pose_front(Rp, tpn, ph, qh, lam, mu);
      const bool f2 = pose_front(Rm, tm, ph, qh, lam, mu), f3 = pose_front(Rm, tmn, ph, qh, lam, mu);
      cnt[0] += (on && f0) ? 1.0 : 0.0; cnt[1] += (on && f1) ? 1.0 : 0.0;
      cnt[2] += (on && f2) ? 1.0 : 0.0; cnt[3] += (on && f3) ? 1.0 : 0.0;
      cnt[4] += (ep && f0) ? 1.0 : 0.0; cnt[5] += (ep && f1) ? 1.0 : 0.0;
      cnt[6] += (em && f2) ? 1.0 : 0.0; cnt[7] += (em && f3) ? 1.0 : 0.0;
    }
    hf_block_sum<8>(cnt, red);
    // the integer keys (nfront << 32) | ~c of the candidates that remain; 0: dropped
    unsigned long long key[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool keep = fin[c >> 1] != 0 && (int)cnt[c] >= P.min_front;
      key[c] = keep ? (((unsigned long long)(uint32_t)(int)cnt[4 + c] << 32) | (unsigned long long)(~(uint32_t)c)) : 0ull;
      left += keep ? 1 : 0;
    }
    unsigned long long k0 = 0ull, k1 = 0ull;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (key[c] > k0) { k0 = key[c]; s0 = c; }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c != s0 && key[c] > k1) { k1 = key[c]; s1 = c; }
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < 8; ++c) cnts[c] = (int)cnt[c];
    }
  }
  __syncthreads();                                               // the zeroes above and cnts are behind this barrier
  const int sel = P.which ? s1 : s0;
  if (sel >= 0 && (front || xyz)) {
    double R[9], t[3], F[9];
    const double sgn = (sel & 1) ? -1.0 : 1.0;
    const double* e = tab + (sel >> 1) * POSE_H_SIGN;
#pragma unroll
    for (int i = 0; i < 9; ++i) { R[i] = e[i]; F[i] = e[16 + i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = sgn * e[9 + i];
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
  // solution j = 0, 1 of the frame: candidate s0 / s1 (or none); a rotation has solution 0's R and nothing else
  if (tid < 18) {
    const int j = tid / 9, i = tid - j * 9, s = j ? s1 : s0;
    float v = 0.f;
    if (s >= 0) v = (float)tab[(s >> 1) * POSE_H_SIGN + i];
    else if (mode == POSE_H_ROTATION && j == 0) v = (float)tab[i];
    Rout[f * 18 + tid] = v;
  }
  if (tid < 6) {
    const int j = tid / 3, i = tid - j * 3, s = j ? s1 : s0;
    tout[f * 6 + tid] = s >= 0 ? (float)((s & 1) ? -tab[(s >> 1) * POSE_H_SIGN + 9 + i] : tab[(s >> 1) * POSE_H_SIGN + 9 + i]) : 0.f;
  }
  if (plane && tid < 8) {
    const int j = tid >> 2, i = tid & 3, s = j ? s1 : s0;
    float v = 0.f;
    if (s >= 0) {
      const double* e = tab + (s >> 1) * POSE_H_SIGN;
      v = i < 3 ? (float)((s & 1) ? -e[12 + i] : e[12 + i]) : (float)(1.0 / e[15]);
    }
    plane[f * 8 + tid] = v;
  }
  if (tid < 2) {
    const int s = tid ? s1 : s0;
    nfront[f * 2 + tid] = s >= 0 ? cnts[4 + s] : 0;
    if (nplane) nplane[f * 2 + tid] = s >= 0 ? cnts[s] : 0;
  }
  // include/fpc.h's FPC_POSE_H_FAILED 0, _UNIQUE 1, _TWOFOLD 2, _ROTATION 3
  if (tid == 0) kind[f] = mode == POSE_H_ROTATION ? 3 : (left >= 2 ? 2 : left);
}
