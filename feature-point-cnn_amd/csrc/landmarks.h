// Landmarks for a new key frame from its PnP pose (fpc_landmarks_pairs / fpc_landmarks_frames / fpc_landmarks_bank; the rule
// is stated in include/fpc.h and restated in float64 by tests/test_landmarks.py).  hf_clamp and hf_block_sum are
// ransac_parts.h's, pnp_finite3 and the landmark storage of the bank are pnp_ransac.h's, POSE_PARALLEL (the floor the host
// passes at 0 degrees) is pose_epipolar.h's.
//
//   landmarks_kernel<Source>   one workgroup of 256 per frame.  R, t and the two cameras sit in fp64 registers; the lanes walk
//                     the frame's output rows in strides of 256, and lane k's rows are its own from the read to the store:
//                     every row of kind / xyz is written exactly once (zeros for a row that is no pair, lies past the count
//                     or fails a test), so nothing is cleared first and no barrier orders the stores.  A Source says how
//                     many rows the frame has and reads one row -- the two pixels and the train row's landmark -- straight
//                     from the caller's arrays (LmExplicit), the last detect's results and a key (LmKey) or a bank slot
//                     (LmBank): no pair list is built, no workspace is touched.  landmarks_rule decides the row for all
//                     three; the two counts are sums of 0 / 1 doubles through hf_block_sum<2>: exact.
#pragma once
#include "pnp_ransac.h"
#include "pose_epipolar.h"

struct LmArgs {
  float q_fx, q_fy, q_cx, q_cy;           // the query camera: the frames being promoted
  float t_fx, t_fy, t_cx, t_cy;           // the train camera: the key frame
  float thr;
  double parallax;                        // sin^2(min_parallax), formed by the host; POSE_PARALLEL at 0 degrees
};

// one row as a Source reads it: the query pixel, the train pixel, and the train row's landmark when `has`
struct LmRow {
  float x, y, u, v, X, Y, Z;
  bool has;
};

// fpc_landmarks_pairs: pair k < npairs[f] of the caller's arrays, all of them [n][stride][.]
struct LmExplicit {
  const float* q_xy;
  const float* t_xy;
  const float* t_xyz;                     // or null: no row has a landmark
  const uint8_t* t_valid;                 // or null: every finite row
  const int32_t* npairs;
  int stride;
  const float* qx; const float* tx; const float* lm; const uint8_t* vl;      // frame(f) sets these: the frame's rows
  __device__ __forceinline__ int frame(int f) {
    const size_t o = (size_t)f * stride;
    qx = q_xy + o * 2; tx = t_xy + o * 2;
    lm = t_xyz ? t_xyz + o * 3 : nullptr;
    vl = t_valid ? t_valid + o : nullptr;
    return hf_clamp(npairs[f], stride);
  }
  __device__ __forceinline__ bool load(int k, LmRow& r) const {
    r.x = qx[2 * k]; r.y = qx[2 * k + 1]; r.u = tx[2 * k]; r.v = tx[2 * k + 1];
    r.has = false;
    if (lm) {
      r.X = lm[3 * k]; r.Y = lm[3 * k + 1]; r.Z = lm[3 * k + 2];
      r.has = (!vl || vl[k] != 0) && pnp_finite3(r.X, r.Y, r.Z);
    }
    return true;
  }
};

// the query side of the other two: row i < count[f] of the last detect's results with its match
struct LmFrames {
  const int32_t* xy;                      // [B][cap][2]
  const int32_t* count;                   // [B]
  const int32_t* match;                   // [n][cap]
  int cap;
};

// fpc_landmarks_frames: one key for every frame, fpc_pnp_frames' arguments plus the key's pixels
struct LmKey {
  LmFrames q;
  const int32_t* key_xy;                  // [nkey][2]
  const int32_t* nkey;
  const float* key_xyz;                   // or null
  const uint8_t* key_valid;               // or null
  const int32_t* qx; const int32_t* mt; int nt;                             // frame(f) sets these
  __device__ __forceinline__ int frame(int f) {
    qx = q.xy + (size_t)f * q.cap * 2; mt = q.match + (size_t)f * q.cap;
    nt = hf_clamp(nkey[0], q.cap);
    return hf_clamp(q.count[f], q.cap);
  }
  __device__ __forceinline__ bool load(int i, LmRow& r) const {
    const int m = mt[i];
    if (!(m >= 0 && m < nt)) return false;
    r.x = (float)qx[2 * i]; r.y = (float)qx[2 * i + 1]; r.u = (float)key_xy[2 * (size_t)m]; r.v = (float)key_xy[2 * (size_t)m + 1];
    r.has = false;
    if (key_xyz) {
      r.X = key_xyz[3 * (size_t)m]; r.Y = key_xyz[3 * (size_t)m + 1]; r.Z = key_xyz[3 * (size_t)m + 2];
      r.has = (!key_valid || key_valid[m] != 0) && pnp_finite3(r.X, r.Y, r.Z);
    }
    return true;
  }
};

// fpc_landmarks_bank: slot[f] of the bank's xy / count and of its landmark storage (null without a reservation); a slot
// outside [0, slots) leaves the frame without rows
struct LmBank {
  LmFrames q;
  const int32_t* slot;                    // [n] device
  const int32_t* bank_xy;                 // [slots][rows][2]
  const int32_t* bank_count;              // [slots]
  const float4* bank_lm;                  // [slots][rows], w != 0: valid; or null
  int rows, slots;
  const int32_t* qx; const int32_t* mt; const int32_t* txy; const float4* lm; int nt;   // frame(f) sets these
  __device__ __forceinline__ int frame(int f) {
    qx = q.xy + (size_t)f * q.cap * 2; mt = q.match + (size_t)f * q.cap;
    const int sl = slot[f];
    if (!(sl >= 0 && sl < slots)) { nt = 0; txy = nullptr; lm = nullptr; return 0; }
    txy = bank_xy + (size_t)sl * rows * 2;
    lm = bank_lm ? bank_lm + (size_t)sl * rows : nullptr;
    nt = hf_clamp(bank_count[sl], rows);
    return hf_clamp(q.count[f], q.cap);
  }
  __device__ __forceinline__ bool load(int i, LmRow& r) const {
    const int m = mt[i];
    if (!(m >= 0 && m < nt)) return false;
    r.x = (float)qx[2 * i]; r.y = (float)qx[2 * i + 1]; r.u = (float)txy[2 * m]; r.v = (float)txy[2 * m + 1];
    r.has = false;
    if (lm) {
      const float4 p = lm[m];
      r.X = p.x; r.Y = p.y; r.Z = p.z;
      r.has = p.w != 0.f && pnp_finite3(p.x, p.y, p.z);
    }
    return true;
  }
};

// the frame's constants, in fp64 registers
struct LmFrame {
  double R[9], t[3];
  double qfx, qfy, qcx, qcy, tfx, tfy, tcx, tcy;
  double thr2, parallax;
};

// the PnP inlier test of include/fpc.h for the point (a, b, c) of a camera's frame against the pixel (px, py)
__device__ __forceinline__ bool lm_reprojects(double fx, double fy, double cx, double cy, double px, double py, double a,
                                              double b, double c, double thr2) {
#pragma clang fp contract(off)
  const double ex = fx * a - (px - cx) * c, ey = fy * b - (py - cy) * c;
  return c > 0.0 && ex * ex + ey * ey < thr2 * (c * c);
}

// The rule for one row -> its kind (0: dropped, 1: transferred, 2: triangulated) and, for kinds 1 and 2, the point in the
// query camera's frame.  Contraction is off (as in pnp_solve6) so that the three instances of the kernel, which inline this
// behind different loads, compute the same bits.
__device__ __forceinline__ int landmarks_rule(const LmFrame& g, const LmRow& r, double& X0, double& X1, double& X2) {
#pragma clang fp contract(off)
  const double x = (double)r.x, y = (double)r.y, u = (double)r.u, v = (double)r.v;
  if (r.has) {                            // transfer; a row that fails is not triangulated: the map contradicts the match
    const double LX = (double)r.X, LY = (double)r.Y, LZ = (double)r.Z;
    X0 = g.R[0] * LX + g.R[1] * LY + g.R[2] * LZ + g.t[0];
    X1 = g.R[3] * LX + g.R[4] * LY + g.R[5] * LZ + g.t[1];
    X2 = g.R[6] * LX + g.R[7] * LY + g.R[8] * LZ + g.t[2];
    return lm_reprojects(g.qfx, g.qfy, g.qcx, g.qcy, x, y, X0, X1, X2, g.thr2) ? 1 : 0;
  }
  // midpoint triangulation under the known pose: the rays lam a (query) and t + mu b (train), b = R q^
  const double a0 = (x - g.qcx) / g.qfx, a1 = (y - g.qcy) / g.qfy, a2 = 1.0;
  const double q0 = (u - g.tcx) / g.tfx, q1 = (v - g.tcy) / g.tfy;
  const double b0 = g.R[0] * q0 + g.R[1] * q1 + g.R[2];
  const double b1 = g.R[3] * q0 + g.R[4] * q1 + g.R[5];
  const double b2 = g.R[6] * q0 + g.R[7] * q1 + g.R[8];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = b0 * b0 + b1 * b1 + b2 * b2, ab = a0 * b0 + a1 * b1 + a2 * b2;
  const double at = a0 * g.t[0] + a1 * g.t[1] + a2 * g.t[2], bt = b0 * g.t[0] + b1 * g.t[1] + b2 * g.t[2];
  const double det = aa * bb - ab * ab;
  const double lam = (at * bb - ab * bt) / det, mu = (ab * at - aa * bt) / det;
  X0 = (lam * a0 + g.t[0] + mu * b0) / 2.0;
  X1 = (lam * a1 + g.t[1] + mu * b1) / 2.0;
  X2 = (lam * a2 + g.t[2] + mu * b2) / 2.0;
  const double d0 = X0 - g.t[0], d1 = X1 - g.t[1], d2 = X2 - g.t[2];        // Y = R^T (X - t), in the train camera's frame
  const double Y0 = g.R[0] * d0 + g.R[3] * d1 + g.R[6] * d2;
  const double Y1 = g.R[1] * d0 + g.R[4] * d1 + g.R[7] * d2;
  const double Y2 = g.R[2] * d0 + g.R[5] * d1 + g.R[8] * d2;
  const bool keep = det > g.parallax * (aa * bb) && lam > 0.0 && mu > 0.0 &&   // (all false for NaN)
                    lm_reprojects(g.qfx, g.qfy, g.qcx, g.qcy, x, y, X0, X1, X2, g.thr2) &&
                    lm_reprojects(g.tfx, g.tfy, g.tcx, g.tcy, u, v, Y0, Y1, Y2, g.thr2);
  return keep ? 2 : 0;
}

// grid (n), one workgroup per frame; ostride: the rows of a frame in xyz / kind (the stride, or the capacity)
template <class Source>
__global__ __launch_bounds__(256) void landmarks_kernel(Source src, LmArgs P, const float* __restrict__ Rin,
                                                        const float* __restrict__ tin, float* __restrict__ xyz,
                                                        uint8_t* __restrict__ kind, int32_t* __restrict__ counts, int ostride) {
  __shared__ double red[4 * 2];
  const int f = blockIdx.x, tid = threadIdx.x;
  LmFrame g;
  bool any = false, finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    g.R[i] = (double)Rin[f * 9 + i];
    any = any || g.R[i] != 0.0;
    finite = finite && fabs(g.R[i]) < 1e300;                     // (false for NaN and Inf)
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g.t[i] = (double)tin[f * 3 + i];
    finite = finite && fabs(g.t[i]) < 1e300;
  }
  g.qfx = P.q_fx; g.qfy = P.q_fy; g.qcx = P.q_cx; g.qcy = P.q_cy;
  g.tfx = P.t_fx; g.tfy = P.t_fy; g.tcx = P.t_cx; g.tcy = P.t_cy;
  g.thr2 = (double)P.thr * (double)P.thr;
  g.parallax = P.parallax;
  int M = src.frame(f);
  if (!(any && finite)) M = 0;                                   // a failed pose: every row 0 (uniform)
  double cnt[2] = {0.0, 0.0};
  for (int k = tid; k < ostride; k += 256) {
    int kd = 0;
    double X0 = 0.0, X1 = 0.0, X2 = 0.0;
    LmRow r;
    if (k < M && src.load(k, r)) kd = landmarks_rule(g, r, X0, X1, X2);
    const size_t o = (size_t)f * ostride + k;
    kind[o] = (uint8_t)kd;
    xyz[o * 3 + 0] = kd ? (float)X0 : 0.f;
    xyz[o * 3 + 1] = kd ? (float)X1 : 0.f;
    xyz[o * 3 + 2] = kd ? (float)X2 : 0.f;
    cnt[0] += kd == 1 ? 1.0 : 0.0;
    cnt[1] += kd == 2 ? 1.0 : 0.0;
  }
  hf_block_sum<2>(cnt, red);
  if (counts && tid == 0) {
    counts[f * 2 + 0] = (int32_t)cnt[0];
    counts[f * 2 + 1] = (int32_t)cnt[1];
  }
}
