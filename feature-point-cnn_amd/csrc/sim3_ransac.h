// Batched RANSAC similarity transforms between two sets of 3-D points (fpc_ransac_sim3 / fpc_sim3_frames / fpc_sim3_bank; the
// rule is stated in include/fpc.h and restated in float64 by tests/test_sim3_ransac.py).  The fourth model of the family
// ransac_parts.h was built for.  This header holds the similarity's model -- the triad solve of three pairs, Horn's
// quaternion refit and its monotone guard, the two-camera reprojection tests -- and its pair records; the sampler, the
// selection key, the compaction and the score and refit skeletons are ransac_parts.h's, the Jacobi routine is
// ransac_fundamental.h's, the train sources (a key's arrays, a bank slot's float4 rows) are pnp_ransac.h's PnpTrain.
//
//   sim3_pack_kernel / sim3_gather_kernel   twins of pnp_pack_kernel / pnp_gather_kernel: every problem's pair list as
//                     32-byte records [Qx, Qy, Qz, Tx | Ty, Tz, row, -] (two float4; `row` is the mask row of the pair, as
//                     int bits) in the PnP reservation, the pair count, and the zeroed best key and mask.  The gather is the
//                     same gather_body; both landmarks' validity is part of the pair test.
//   sim3_score_kernel score_body at 256 hypotheses per workgroup.  The triad solve needs no linear system: it lives in
//                     registers with constant indices only, so the workgroup's LDS is the 1 024-record stage (32 KiB) alone
//                     and THREADS is free.  The walk over the pair list is VALU work (two 3 x 4 transforms and two
//                     cross-multiplied tests per record and lane) on records that every lane reads from the same LDS
//                     address, so what THREADS decides is how many waves a CU can hold once a call has more waves than
//                     the chip has SIMDs (n x T / 64 > 1 024).  The stage is per WORKGROUP: 160 KiB admit five of them.
//                     At 64 threads those would be five waves per CU, hardly more than one per SIMD, whatever the
//                     registers allow; at 256 threads a workgroup is four waves, one per SIMD, the 120 VGPRs of the
//                     kernel allow four waves per SIMD (512 / 128), and four workgroups -- 128 KiB of LDS -- fill that:
//                     the registers are the limit, not the LDS.  256 also stages every record once per 256 hypotheses
//                     instead of once per 64.  This is reasoning from the resource report, NOT a measurement: no build at
//                     THREADS = 64 or 128 was timed.  The hypothesis sits in 24 fp32 VGPRs (sR, t, R^T / s, -R^T t / s).
//   sim3_refit_kernel one workgroup of 256 per problem: one lane re-derives the best sample's model with the same device
//                     function (refit_head); then `refits` times -- or until a refit returns the model it started from,
//                     after which every further one would -- two passes over the pairs (the count and the centroids; the
//                     9 + 2 sums of a b^T, |a|^2, |b|^2) in fp64 through hf_block_sum, one lane's fm_jacobi at N = 4 on
//                     Horn's matrix in LDS, and the guard's count of the candidate; through refit_tail it writes s, R, t, the
//                     inlier count and the mask of the model it returns.
#pragma once
#include "pnp_ransac.h"

constexpr int SIM3_DRAWS = 16;          // draw budget of one sample
constexpr int SIM3_SAMPLE = 3;
constexpr int SIM3_THREADS = 256;       // hypotheses per workgroup of sim3_score_kernel (the header comment says why)
constexpr double SIM3_DEGENERATE = 1e-12;   // sin^2 of the triangle's angle at p0 at or below which a sample is degenerate
constexpr double SIM3_GAP = 1e-12;      // (lambda0 - lambda1) / sqrt(sum |a|^2 sum |b|^2) at or below which a refit is singular
constexpr int SIM3_NSUM = 11;           // 9 of a b^T, |a|^2, |b|^2

struct Sim3Args {
  float4* rec;                  // [B][cap][2]  (Qx, Qy, Qz, Tx), (Ty, Tz, row, -)
  int32_t* np;                  // [B]          pairs of the frame
  unsigned long long* best;     // [B]          (inlier count << 32) | ~t of the best hypothesis; 0: none
  int cap, n;
  int T, refits, min_inliers, fix_scale;
  float thr;
  uint32_t seed;
  float qfx, qfy, tfx, tfy;
};

struct Sim3Pair { float qx, qy, qz, tx, ty, tz; int row; };

__device__ __forceinline__ Sim3Pair sim3_load(const float4* __restrict__ rec, int k) {
  const float4 a = rec[2 * k], b = rec[2 * k + 1];
  return {a.x, a.y, a.z, a.w, b.x, b.y, __float_as_int(b.z)};
}

// x = (p1 - p0) / |p1 - p0|, z = c / |c| with c = (p1 - p0) x (p2 - p0), y = z x x.  false: c.c is not above
// SIM3_DEGENERATE |p1 - p0|^2 |p2 - p0|^2 (or a NaN).
__device__ __forceinline__ bool sim3_triad(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3],
                                           double (&x)[3], double (&y)[3], double (&z)[3]) {
#pragma clang fp contract(off)
  const double d1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double n1 = (d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2], n2 = (d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2];
  const double c[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
  const double cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  if (!(cc > (SIM3_DEGENERATE * n1) * n2)) return false;
  const double r1 = sqrt(n1), rc = sqrt(cc);
#pragma unroll
  for (int i = 0; i < 3; ++i) { x[i] = d1[i] / r1; z[i] = c[i] / rc; }
  y[0] = z[1] * x[2] - z[2] * x[1];
  y[1] = z[2] * x[0] - z[0] * x[2];
  y[2] = z[0] * x[1] - z[1] * x[0];
  return true;
}

// The minimal solve of include/fpc.h: three pairs -> s, R (row-major), t with X_query = s R X_train + t, in fp64 and in
// registers (every index is a constant once unrolled).  Contraction is off so that the score kernel and the refit kernel
// compute the same bits.  false: degenerate.
__device__ __forceinline__ bool sim3_solve3(const float4* __restrict__ rec, const uint32_t (&idx)[SIM3_SAMPLE], int fix_scale,
                                            double& s, double (&R)[9], double (&t)[3]) {
#pragma clang fp contract(off)
  double q[3][3], p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const Sim3Pair r = sim3_load(rec, (int)idx[k]);
    q[k][0] = r.qx; q[k][1] = r.qy; q[k][2] = r.qz;
    p[k][0] = r.tx; p[k][1] = r.ty; p[k][2] = r.tz;
  }
  double xq[3], yq[3], zq[3], xt[3], yt[3], zt[3];
  if (!sim3_triad(q[0], q[1], q[2], xq, yq, zq) || !sim3_triad(p[0], p[1], p[2], xt, yt, zt)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (xq[i] * xt[j] + yq[i] * yt[j]) + zq[i] * zt[j];
  double qm[3], pm[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    qm[i] = ((q[0][i] + q[1][i]) + q[2][i]) / 3.0;
    pm[i] = ((p[0][i] + p[1][i]) + p[2][i]) / 3.0;
  }
  double vq = 0.0, vp = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a0 = q[k][0] - qm[0], a1 = q[k][1] - qm[1], a2 = q[k][2] - qm[2];
    const double b0 = p[k][0] - pm[0], b1 = p[k][1] - pm[1], b2 = p[k][2] - pm[2];
    vq = vq + ((a0 * a0 + a1 * a1) + a2 * a2);
    vp = vp + ((b0 * b0 + b1 * b1) + b2 * b2);
  }
  s = fix_scale ? 1.0 : sqrt(vq / vp);
  bool finite = s > 0.0 && s < 1e300;                            // (false for NaN)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = qm[i] - s * ((R[i * 3] * pm[0] + R[i * 3 + 1] * pm[1]) + R[i * 3 + 2] * pm[2]);
    finite = finite && fabs(t[i]) < 1e300;
#pragma unroll
    for (int j = 0; j < 3; ++j) finite = finite && fabs(R[i * 3 + j]) < 1e300;
  }
  return finite;
}

// the hypothesis as it is scored, 24 fp32 values: s R (9), t (3), R^T / s (9), -R^T t / s (3).  false: one is not finite.
__device__ __forceinline__ bool sim3_hypothesis(double s, const double (&R)[9], const double (&t)[3], float (&h)[24]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      h[i * 3 + j] = (float)(s * R[i * 3 + j]);
      h[12 + i * 3 + j] = (float)(R[j * 3 + i] / s);
    }
    h[9 + i] = (float)t[i];
    h[21 + i] = (float)(-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) / s);
  }
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 24; ++i) finite = finite && fabsf(h[i]) <= 3.402823466e38f;        // (false for NaN)
  return finite;
}

// ---- pair lists -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim3_pack_kernel(Sim3Args a, const float* __restrict__ q, const float* __restrict__ t,
                                                        const int32_t* __restrict__ npairs, int stride, uint8_t* mask) {
  const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  const int M = hf_clamp(npairs[f], stride);
  if (k == 0) {
    a.np[f] = M;
    a.best[f] = 0ull;
  }
  if (k >= stride) return;
  if (mask) mask[(size_t)f * stride + k] = 0;
  if (k < M) {
    const size_t i = ((size_t)f * stride + k) * 3;
    float4* out = a.rec + ((size_t)f * a.cap + k) * 2;
    out[0] = make_float4(q[i], q[i + 1], q[i + 2], t[i]);
    out[1] = make_float4(t[i + 1], t[i + 2], __int_as_float(k), 0.f);
  }
}

// one workgroup per frame; rows i < count[f] with 0 <= match < the train count and a valid landmark on both sides, in
// ascending i.  The train set of frame f is PnpTrain's, as in pnp_gather_kernel.
__global__ __launch_bounds__(256) void sim3_gather_kernel(Sim3Args a, const float* __restrict__ qxyz,
                                                          const uint8_t* __restrict__ qvalid, const int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ match, uint8_t* mask, const PnpTrain tr) {
  const int f = blockIdx.x, cap = a.cap;
  const int cnt = hf_clamp(count[f], cap);
  const float4* lm = nullptr;
  int nt = 0;
  if (tr.slot) {
    const int sl = tr.slot[f];
    if (tr.lm && sl >= 0 && sl < tr.slots) {
      lm = tr.lm + (size_t)sl * tr.rows;
      nt = hf_clamp(tr.count[sl], tr.rows);
    }
  } else {
    nt = hf_clamp(tr.nkey[0], cap);
  }
  // gather_body's Source.  `pair` is called once per round of 256 rows, in order, so the Source counts its own row i (the
  // query landmark is part of the pair test); it keeps both landmarks for `write`.
  struct {
    const Sim3Args& a;
    const PnpTrain& tr;
    const float* q;
    const uint8_t* qv;
    const float4* lm;
    int f, nt, i, cnt;
    float Qx, Qy, Qz, X, Y, Z;
    __device__ __forceinline__ bool pair(int m) {
      const int row = i;
      i += 256;
      Qx = Qy = Qz = X = Y = Z = 0.f;
      if (!(row < cnt && m >= 0 && m < nt)) return false;
      Qx = q[3 * (size_t)row]; Qy = q[3 * (size_t)row + 1]; Qz = q[3 * (size_t)row + 2];
      if (!((!qv || qv[row] != 0) && pnp_finite3(Qx, Qy, Qz))) return false;
      if (tr.slot) {
        const float4 p = lm[m];
        X = p.x; Y = p.y; Z = p.z;
        return p.w != 0.f;
      }
      X = tr.key_xyz[3 * (size_t)m]; Y = tr.key_xyz[3 * (size_t)m + 1]; Z = tr.key_xyz[3 * (size_t)m + 2];
      return (!tr.key_valid || tr.key_valid[m] != 0) && pnp_finite3(X, Y, Z);
    }
    __device__ __forceinline__ void write(int off, int row, int) {
      float4* out = a.rec + ((size_t)f * a.cap + off) * 2;
      out[0] = make_float4(Qx, Qy, Qz, X);
      out[1] = make_float4(Y, Z, __int_as_float(row), 0.f);
    }
  } src{a, tr, qxyz + (size_t)f * cap * 3, qvalid ? qvalid + (size_t)f * cap : nullptr, lm, f, nt, (int)threadIdx.x, cnt,
        0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  gather_body(src, f, cnt, cap, match, mask, a.np, a.best);
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// score_body's Model.  The 24 values sit in named registers on purpose: an indexed store becomes scratch.  (A degenerate
// hypothesis keeps zeros: Yz = 0 is never > 0, it counts nothing.)
struct Sim3Model {
  static constexpr int SAMPLE = SIM3_SAMPLE, DRAWS = SIM3_DRAWS, REC = 2;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
  float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, b4 = 0.f, b5 = 0.f, b6 = 0.f, b7 = 0.f, b8 = 0.f, u0 = 0.f, u1 = 0.f, u2 = 0.f;
  float thr, qfx, qfy, tfx, tfy;
  __device__ __forceinline__ explicit Sim3Model(const Sim3Args& a) : thr(a.thr), qfx(a.qfx), qfy(a.qfy), tfx(a.tfx), tfy(a.tfy) {}
  static __device__ __forceinline__ const float4* records(const Sim3Args& a, int f) { return a.rec + (size_t)f * a.cap * 2; }
  static __device__ __forceinline__ int frame(const Sim3Args&, int f) { return f; }
  __device__ __forceinline__ bool solve(const Sim3Args& a, const float4* __restrict__ rec, const uint32_t (&idx)[SIM3_SAMPLE],
                                        double*) {
    double s, R[9], t[3];
    float h[24];
    if (!(sim3_solve3(rec, idx, a.fix_scale, s, R, t) && sim3_hypothesis(s, R, t, h))) return false;
    a0 = h[0]; a1 = h[1]; a2 = h[2]; a3 = h[3]; a4 = h[4]; a5 = h[5]; a6 = h[6]; a7 = h[7]; a8 = h[8];
    t0 = h[9]; t1 = h[10]; t2 = h[11];
    b0 = h[12]; b1 = h[13]; b2 = h[14]; b3 = h[15]; b4 = h[16]; b5 = h[17]; b6 = h[18]; b7 = h[19]; b8 = h[20];
    u0 = h[21]; u1 = h[22]; u2 = h[23];
    return true;
  }
  // one camera's test: the point (px, py, pz) seen by the camera against the transferred point (yx, yy, yz)
  static __device__ __forceinline__ bool within(float yx, float yy, float yz, float px, float py, float pz, float fx, float fy,
                                               float thr) {
    const float ex = fx * fmaf(yx, pz, -(px * yz)), ey = fy * fmaf(yy, pz, -(py * yz));
    const float tw = thr * (yz * pz);
    return yz > 0.f && pz > 0.f && fmaf(ex, ex, ey * ey) < tw * tw;
  }
  __device__ __forceinline__ bool counts(const float4* r) const {
    const float4 q = r[0], p = r[1];                              // Q = (q.x, q.y, q.z), T = (q.w, p.x, p.y)
    const float yx = fmaf(a2, p.y, fmaf(a1, p.x, fmaf(a0, q.w, t0)));
    const float yy = fmaf(a5, p.y, fmaf(a4, p.x, fmaf(a3, q.w, t1)));
    const float yz = fmaf(a8, p.y, fmaf(a7, p.x, fmaf(a6, q.w, t2)));
    const float wx = fmaf(b2, q.z, fmaf(b1, q.y, fmaf(b0, q.x, u0)));
    const float wy = fmaf(b5, q.z, fmaf(b4, q.y, fmaf(b3, q.x, u1)));
    const float wz = fmaf(b8, q.z, fmaf(b7, q.y, fmaf(b6, q.x, u2)));
    return within(yx, yy, yz, q.x, q.y, q.z, qfx, qfy, thr) && within(wx, wy, wz, q.w, p.x, p.y, tfx, tfy, thr);
  }
};

__global__ __launch_bounds__(SIM3_THREADS) void sim3_score_kernel(Sim3Args a) {
  __shared__ float4 stage[2 * HF_CHUNK];                         // the staged pair chunk; the model needs no LDS of its own
  score_body<SIM3_THREADS, Sim3Model>(a, stage, nullptr);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sim3_fin(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

// the inlier test of include/fpc.h in fp64, from the fp32 model m = (s, R row-major, t) held as 13 doubles
__device__ __forceinline__ bool sim3_inlier(const double (&m)[13], const Sim3Args& g, const Sim3Pair& p, double thr2) {
  const double Qx = p.qx, Qy = p.qy, Qz = p.qz, Tx = p.tx, Ty = p.ty, Tz = p.tz, s = m[0];
  const double Yx = s * (m[1] * Tx + m[2] * Ty + m[3] * Tz) + m[10];
  const double Yy = s * (m[4] * Tx + m[5] * Ty + m[6] * Tz) + m[11];
  const double Yz = s * (m[7] * Tx + m[8] * Ty + m[9] * Tz) + m[12];
  const double dx = Qx - m[10], dy = Qy - m[11], dz = Qz - m[12];
  const double Wx = (m[1] * dx + m[4] * dy + m[7] * dz) / s;
  const double Wy = (m[2] * dx + m[5] * dy + m[8] * dz) / s;
  const double Wz = (m[3] * dx + m[6] * dy + m[9] * dz) / s;
  if (!(sim3_fin(Qx) && sim3_fin(Qy) && sim3_fin(Qz) && sim3_fin(Tx) && sim3_fin(Ty) && sim3_fin(Tz) && sim3_fin(Yx) &&
        sim3_fin(Yy) && sim3_fin(Yz) && sim3_fin(Wx) && sim3_fin(Wy) && sim3_fin(Wz)))
    return false;
  if (!(Yz > 0.0 && Qz > 0.0 && Wz > 0.0 && Tz > 0.0)) return false;
  const double ex = (double)g.qfx * (Yx * Qz - Qx * Yz), ey = (double)g.qfy * (Yy * Qz - Qy * Yz);
  const double fx = (double)g.tfx * (Wx * Tz - Tx * Wz), fy = (double)g.tfy * (Wy * Tz - Ty * Wz);
  return ex * ex + ey * ey < thr2 * (Yz * Yz) * (Qz * Qz) && fx * fx + fy * fy < thr2 * (Wz * Wz) * (Tz * Tz);
}

// (s, R, t) in fp64 -> out (LDS, 13 doubles): the fp32 values.  false: one is not finite, or s is not > 0.
__device__ __forceinline__ bool sim3_round(double s, const double (&R)[9], const double (&t)[3], double* out) {
  const float s32 = (float)s;
  bool good = s32 > 0.f && s32 < 3e38f;
  out[0] = (double)s32;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float v = (float)R[i];
    good = good && fabsf(v) < 3e38f;
    out[1 + i] = (double)v;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float v = (float)t[i];
    good = good && fabsf(v) < 3e38f;
    out[10 + i] = (double)v;
  }
  return good;
}

__global__ __launch_bounds__(256) void sim3_refit_kernel(Sim3Args a, float* __restrict__ sout, float* __restrict__ Rout,
                                                         float* __restrict__ tout, int32_t* __restrict__ ninl, uint8_t* mask,
                                                         int mstride) {
  __shared__ double red[4 * SIM3_NSUM];
  __shared__ double jn[16], jv[16];
  __shared__ double pose[13], cand[13];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ rec = a.rec + (size_t)f * a.cap * 2;
  const double thr2 = (double)a.thr * (double)a.thr;
  double m[13];
  bool ok = refit_head(M >= SIM3_SAMPLE && key != 0ull, &solved, [&]() {
    uint32_t idx[SIM3_SAMPLE];
    double s, R[9], t[3];
    return hf_sample_distinct<SIM3_SAMPLE, SIM3_DRAWS>(a.seed, (uint32_t)f, ~(uint32_t)key, (uint32_t)M, idx) &&
           sim3_solve3(rec, idx, a.fix_scale, s, R, t) && sim3_round(s, R, t, pose);
  });
  if (ok) {
#pragma unroll
    for (int i = 0; i < 13; ++i) m[i] = pose[i];
    for (int r = 0; r < a.refits; ++r) {
      // first pass: the count and the two centroids over the inliers of the current model
      double c7[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int k = tid; k < M; k += 256) {
        const Sim3Pair p = sim3_load(rec, k);
        if (sim3_inlier(m, a, p, thr2)) {
          c7[0] += 1.0; c7[1] += (double)p.qx; c7[2] += (double)p.qy; c7[3] += (double)p.qz;
          c7[4] += (double)p.tx; c7[5] += (double)p.ty; c7[6] += (double)p.tz;
        }
      }
      hf_block_sum<7>(c7, red);
      if (c7[0] < 3.0) break;
      const double qm0 = c7[1] / c7[0], qm1 = c7[2] / c7[0], qm2 = c7[3] / c7[0];
      const double pm0 = c7[4] / c7[0], pm1 = c7[5] / c7[0], pm2 = c7[6] / c7[0];
      // second pass: sum a b^T (row-major), sum |a|^2, sum |b|^2 with a = T - Tm, b = Q - Qm
      double s[SIM3_NSUM];
#pragma unroll
      for (int i = 0; i < SIM3_NSUM; ++i) s[i] = 0.0;
      for (int k = tid; k < M; k += 256) {
        const Sim3Pair p = sim3_load(rec, k);
        if (sim3_inlier(m, a, p, thr2)) {
          const double av[3] = {(double)p.tx - pm0, (double)p.ty - pm1, (double)p.tz - pm2};
          const double bv[3] = {(double)p.qx - qm0, (double)p.qy - qm1, (double)p.qz - qm2};
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) s[i * 3 + j] += av[i] * bv[j];
          s[9] += av[0] * av[0] + av[1] * av[1] + av[2] * av[2];
          s[10] += bv[0] * bv[0] + bv[1] * bv[1] + bv[2] * bv[2];
        }
      }
      hf_block_sum<SIM3_NSUM>(s, red);
      if (tid == 0) {
        const double Sxx = s[0], Sxy = s[1], Sxz = s[2], Syx = s[3], Syy = s[4], Syz = s[5], Szx = s[6], Szy = s[7], Szz = s[8],
                     va = s[9], vb = s[10];
        int good = (va > 0.0 && vb > 0.0) ? 1 : 0;
        if (good) {
          // Horn's symmetric matrix; its top eigenvector is the unit quaternion (w, x, y, z)
          jn[0] = Sxx + Syy + Szz; jn[1] = Syz - Szy;       jn[2] = Szx - Sxz;        jn[3] = Sxy - Syx;
          jn[4] = jn[1];           jn[5] = Sxx - Syy - Szz; jn[6] = Sxy + Syx;        jn[7] = Szx + Sxz;
          jn[8] = jn[2];           jn[9] = jn[6];           jn[10] = -Sxx + Syy - Szz; jn[11] = Syz + Szy;
          jn[12] = jn[3];          jn[13] = jn[7];          jn[14] = jn[11];          jn[15] = -Sxx - Syy + Szz;
          fm_jacobi(jn, jv, 4);
          int top = 0;
          for (int i = 1; i < 4; ++i)
            if (jn[i * 5] > jn[top * 5]) top = i;
          double second = -1.7976931348623157e308;
          for (int i = 0; i < 4; ++i)
            if (i != top && jn[i * 5] > second) second = jn[i * 5];
          if (!(jn[top * 5] - second > SIM3_GAP * sqrt(va * vb))) good = 0;        // (false for NaN)
          if (good) {
            double w = jv[top], x = jv[4 + top], y = jv[8 + top], z = jv[12 + top];
            const double qn = sqrt(w * w + x * x + y * y + z * z);
            w /= qn; x /= qn; y /= qn; z /= qn;
            const double R[9] = {w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                                 2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x),
                                 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z};
            const double sc = a.fix_scale ? 1.0 : sqrt(vb / va);
            const double t[3] = {qm0 - sc * (R[0] * pm0 + R[1] * pm1 + R[2] * pm2),
                                 qm1 - sc * (R[3] * pm0 + R[4] * pm1 + R[5] * pm2),
                                 qm2 - sc * (R[6] * pm0 + R[7] * pm1 + R[8] * pm2)};
            good = sim3_round(sc, R, t, cand) ? 1 : 0;
          }
        }
        solved = good;
      }
      __syncthreads();
      if (!solved) break;                                                   // a singular refit keeps the model
      double mc[13];
#pragma unroll
      for (int i = 0; i < 13; ++i) mc[i] = cand[i];                         // (the next write of cand is behind hf_block_sum's barriers)
      // A refit that returns the model it started from has converged: the same model has the same inliers, the same sums
      // and the same refit, so the remaining refits would return it again, and so does stopping here.
      bool fixed = true;
#pragma unroll
      for (int i = 0; i < 13; ++i) fixed = fixed && mc[i] == m[i];
      if (fixed) break;
      // the monotone guard: the candidate's count against the current model's (c7[0])
      double c1[1] = {0.0};
      for (int k = tid; k < M; k += 256) c1[0] += sim3_inlier(mc, a, sim3_load(rec, k), thr2) ? 1.0 : 0.0;
      hf_block_sum<1>(c1, red);
      if (c1[0] < c7[0]) break;
#pragma unroll
      for (int i = 0; i < 13; ++i) m[i] = mc[i];
    }
  }
  ok = refit_tail(ok, M, a.min_inliers, red, mask, ninl + f,
                  [&](int k) { return sim3_inlier(m, a, sim3_load(rec, k), thr2); },
                  [&](int k) { return (size_t)f * mstride + sim3_load(rec, k).row; });
  if (tid == 0) {                                                           // (through LDS: m[tid] would be scratch)
#pragma unroll
    for (int i = 0; i < 13; ++i) pose[i] = ok ? m[i] : 0.0;
  }
  __syncthreads();
  if (tid == 0) sout[f] = (float)pose[0];
  if (tid < 9) Rout[f * 9 + tid] = (float)pose[1 + tid];
  if (tid < 3) tout[f * 3 + tid] = (float)pose[10 + tid];
}
