// Batched RANSAC perspective-n-point (fpc_ransac_pnp / fpc_pnp_frames / fpc_pnp_bank; the rule is stated in include/fpc.h and
// restated in float64 by tests/test_pnp_ransac.py).  This header holds the pose's model -- the DLT rows, the polar step, the
// Gauss-Newton sums and pose update, the reprojection tests -- its pair records and the landmark kernels; the sampler, the
// selection key, the compaction, the LDS solve and the score and refit skeletons are ransac_parts.h's, the Jacobi routine is
// ransac_fundamental.h's.  The full-pivot elimination inside pnp_solve6 is fm_solve8's at another size, written out again
// (ransac_fundamental.h says why).
//
//   pnp_pack_kernel / pnp_gather_kernel   twins of hf_pack_kernel / hf_gather_kernel: every problem's pair list as 32-byte
//                     records [x, y, X, Y | Z, row, -, -] (two float4; `row` is the mask row of the pair, as int bits), the
//                     pair count, and the zeroed best key and mask.  The gather is the same gather_body; a landmark's
//                     validity (its w, or valid[] and the finiteness of its coordinates) is part of the pair test.
//   pnp_score_kernel  score_body at 64 hypotheses per workgroup: the normalised 6-point DLT in fp64 by Gaussian elimination
//                     with full pivoting.  The 11 x 12 system needs dynamic row and column indices, so it lives in LDS,
//                     struct-of-arrays (sys[132][64]); the column permutation is twelve nibbles of one 64-bit register.
//                     132 doubles x 64 lanes = 66 KiB: ONE wave per workgroup, so that
//                     two workgroups share a CU's 160 KiB (128 lanes would need 132 KiB and run alone).  P then sits in 12
//                     fp32 VGPRs and the pair list is walked through the same LDS in 1 024-record chunks (32 KiB).
//   pnp_refit_kernel  one workgroup of 256 per problem: one lane re-derives the best sample's P with the same device
//                     function and takes its polar step (fm_jacobi at N = 3; refit_head); then `refits` times one pass over
//                     the pairs (the 21 + 6 sums of J^T J and J^T r, and the count, in fp64 through hf_block_sum) and one
//                     lane's 6 x 6 solve_lds; through refit_tail it writes R, t, the inlier count and the mask of the pose
//                     it returns.  Its body is pnp_refit_body<Minimal>, which p3p_ransac.h instantiates with its own derive
//                     step; this kernel's is PnpDlt.
//   pnp_landmarks_store_kernel / pnp_landmarks_invalidate_kernel   element-wise, over one slot's rows (or every slot's).
#pragma once
#include "ransac_fundamental.h"

constexpr int PNP_DRAWS = 32;          // draw budget of one sample
constexpr int PNP_SAMPLE = 6;
constexpr int PNP_THREADS = 64;        // hypotheses per workgroup of pnp_score_kernel: 66 KiB of LDS, two workgroups per CU
constexpr int PNP_ROWS = 11, PNP_COLS = 12;
constexpr int PNP_CHUNK = HF_CHUNK;    // records staged per LDS chunk (32 KiB)
constexpr double PNP_PIVOT = 1e-10;    // last pivot / first pivot below which a sample is degenerate
constexpr double PNP_RANK = 1e-12;     // lambda_min / lambda_max of A^T A at or below which P has no rotation
constexpr double PNP_SINGULAR = 1e-14; // pivot / largest diagonal entry of J^T J at or below which a refit is singular
constexpr int PNP_NSUM = 28;           // 21 of J^T J, 6 of J^T r, the inlier count

struct PnpArgs {
  float4* rec;                  // [B][cap][2]  (x, y, X, Y), (Z, row, -, -)
  int32_t* np;                  // [B]          pairs of the frame
  unsigned long long* best;     // [B]          (inlier count << 32) | ~t of the best hypothesis; 0: none
  int cap, n;
  int T, refits, min_inliers;
  float thr;
  uint32_t seed;
  float fx, fy, cx, cy;
  // fpc_pnp_bank_topk / fpc_p3p_bank_topk (match_bank_topk.h): HfArgs::per_frame's meaning -- the grid's index is a PROBLEM
  // p = f per_frame + j with its own records, count, best key, mask row and slot, while the frame f = p / per_frame selects
  // the query pixels and feeds the sampler.  0 (every other entry point): one problem per frame, p = f.
  int per_frame;
};

struct PnpPair { float x, y, X, Y, Z; int row; };

__device__ __forceinline__ PnpPair pnp_load(const float4* __restrict__ rec, int k) {
  const float4 a = rec[2 * k], b = rec[2 * k + 1];
  return {a.x, a.y, a.z, a.w, b.x, __float_as_int(b.y)};
}

__device__ __forceinline__ bool pnp_finite3(float X, float Y, float Z) {
  return fabsf(X) <= 3.402823466e38f && fabsf(Y) <= 3.402823466e38f && fabsf(Z) <= 3.402823466e38f;   // (false for NaN)
}

// The 6-point DLT.  sys: this thread's 11 x 12 system, element (r, c) at sys[(r * 12 + c) * S] (LDS).  Image points in
// normalised coordinates, landmarks translated to their centroid and scaled to an RMS distance of sqrt(3); elimination with
// full pivoting (ties: lowest row, then lowest column), the null vector by back-substitution with the last column's unknown
// = 1; P is denormalised to the landmarks' own coordinates (image side still normalised): P = [A | a4], row-major 3 x 4.
// Contraction is off so that the score kernel and the refit kernel, which inline this at different strides, compute the
// same bits.  -> the sample's first pair in `first`.  false: degenerate.
template <int S>
__device__ __forceinline__ bool pnp_solve6(double* sys, const float4* __restrict__ rec, const uint32_t (&idx)[PNP_SAMPLE],
                                           const PnpArgs& a, double (&P)[12], PnpPair& first) {
#pragma clang fp contract(off)
  PnpPair r[PNP_SAMPLE];
#pragma unroll
  for (int i = 0; i < PNP_SAMPLE; ++i) r[i] = pnp_load(rec, (int)idx[i]);
  first = r[0];
  double mx = 0.0, my = 0.0, mz = 0.0;
#pragma unroll
  for (int i = 0; i < PNP_SAMPLE; ++i) { mx += (double)r[i].X; my += (double)r[i].Y; mz += (double)r[i].Z; }
  mx = mx / 6.0; my = my / 6.0; mz = mz / 6.0;
  double var = 0.0;
#pragma unroll
  for (int i = 0; i < PNP_SAMPLE; ++i) {
    const double dx = (double)r[i].X - mx, dy = (double)r[i].Y - my, dz = (double)r[i].Z - mz;
    var += dx * dx; var += dy * dy; var += dz * dz;
  }
  var = var / 6.0;
  if (!(var > 0.0) || !(var < 1e300)) return false;             // (NaN fails the first test, Inf the second)
  const double s = sqrt(3.0 / var);
  const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
#pragma unroll
  for (int i = 0; i < PNP_SAMPLE; ++i) {
    const double X = ((double)r[i].X - mx) * s, Y = ((double)r[i].Y - my) * s, Z = ((double)r[i].Z - mz) * s;
    const double xh = ((double)r[i].x - cx) / fx, yh = ((double)r[i].y - cy) / fy;
    double* row = sys + (size_t)(2 * i) * PNP_COLS * S;
    row[0] = X; row[S] = Y; row[2 * S] = Z; row[3 * S] = 1.0; row[4 * S] = 0.0; row[5 * S] = 0.0; row[6 * S] = 0.0; row[7 * S] = 0.0;
    row[8 * S] = -xh * X; row[9 * S] = -xh * Y; row[10 * S] = -xh * Z; row[11 * S] = -xh;
    if (i < PNP_SAMPLE - 1) {                                   // (the sixth point gives its first row only)
      row += (size_t)PNP_COLS * S;
      row[0] = 0.0; row[S] = 0.0; row[2 * S] = 0.0; row[3 * S] = 0.0; row[4 * S] = X; row[5 * S] = Y; row[6 * S] = Z; row[7 * S] = 1.0;
      row[8 * S] = -yh * X; row[9 * S] = -yh * Y; row[10 * S] = -yh * Z; row[11 * S] = -yh;
    }
  }
  unsigned long long perm = 0xBA9876543210ull;                  // nibble c: the unknown that column c holds
  double firstp = 0.0, last = 0.0;
#pragma unroll 1
  for (int c = 0; c < PNP_ROWS; ++c) {
    double pv = -1.0;
    int pr = c, pc = c;
    for (int i = c; i < PNP_ROWS; ++i)
      for (int j = c; j < PNP_COLS; ++j) {
        const double v = fabs(sys[(i * PNP_COLS + j) * S]);
        if (v > pv) { pv = v; pr = i; pc = j; }
      }
    if (c == 0) firstp = pv;
    last = pv;
    if (!(pv > 0.0)) return false;
    if (pr != c)
      for (int j = c; j < PNP_COLS; ++j) {
        const double tmp = sys[(c * PNP_COLS + j) * S];
        sys[(c * PNP_COLS + j) * S] = sys[(pr * PNP_COLS + j) * S];
        sys[(pr * PNP_COLS + j) * S] = tmp;
      }
    if (pc != c) {
      for (int i = 0; i < PNP_ROWS; ++i) {
        const double tmp = sys[(i * PNP_COLS + c) * S];
        sys[(i * PNP_COLS + c) * S] = sys[(i * PNP_COLS + pc) * S];
        sys[(i * PNP_COLS + pc) * S] = tmp;
      }
      const unsigned long long nc = (perm >> (4 * c)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
      perm = (perm & ~((15ull << (4 * c)) | (15ull << (4 * pc)))) | (np << (4 * c)) | (nc << (4 * pc));
    }
    const double piv = sys[(c * PNP_COLS + c) * S];
    for (int i = c + 1; i < PNP_ROWS; ++i) {
      const double fct = sys[(i * PNP_COLS + c) * S] / piv;
      for (int j = c + 1; j < PNP_COLS; ++j)
        sys[(i * PNP_COLS + j) * S] = sys[(i * PNP_COLS + j) * S] - fct * sys[(c * PNP_COLS + j) * S];
    }
  }
  if (!(last >= PNP_PIVOT * firstp)) return false;
  // back-substitution; y_i replaces the pivot it was divided by
#pragma unroll 1
  for (int i = PNP_ROWS - 1; i >= 0; --i) {
    double acc = 0.0;
    for (int j = i + 1; j < PNP_ROWS; ++j) acc = acc + sys[(i * PNP_COLS + j) * S] * sys[(j * PNP_COLS + j) * S];
    acc = acc + sys[(i * PNP_COLS + PNP_ROWS) * S];
    sys[(i * PNP_COLS + i) * S] = -acc / sys[(i * PNP_COLS + i) * S];
  }
  double Pn[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Pn[k] = 0.0;
#pragma unroll 1
  for (int i = 0; i < PNP_COLS; ++i) {
    const double yi = i < PNP_ROWS ? sys[(i * PNP_COLS + i) * S] : 1.0;
    const int pi = (int)((perm >> (4 * i)) & 15ull);
#pragma unroll
    for (int k = 0; k < 12; ++k) Pn[k] = pi == k ? yi : Pn[k];
  }
  // P = Pn [s I, -s m; 0 1]
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    P[i * 4 + 0] = Pn[i * 4 + 0] * s;
    P[i * 4 + 1] = Pn[i * 4 + 1] * s;
    P[i * 4 + 2] = Pn[i * 4 + 2] * s;
    P[i * 4 + 3] = Pn[i * 4 + 3] - s * (mx * Pn[i * 4 + 0] + my * Pn[i * 4 + 1] + mz * Pn[i * 4 + 2]);
#pragma unroll
    for (int j = 0; j < 4; ++j) finite = finite && fabs(P[i * 4 + j]) < 1e300;        // (false for NaN and Inf)
  }
  return finite;
}

// the hypothesis as it is scored: P_px = K P scaled to max |p| = 1, w > 0 at the sample's first pair, rounded to fp32
__device__ __forceinline__ bool pnp_hypothesis(const double (&P)[12], const PnpArgs& a, const PnpPair& first, float (&P32)[12]) {
#pragma clang fp contract(off)
  double Q[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    Q[j] = (double)a.fx * P[j] + (double)a.cx * P[8 + j];
    Q[4 + j] = (double)a.fy * P[4 + j] + (double)a.cy * P[8 + j];
    Q[8 + j] = P[8 + j];
  }
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 12; ++i) mx = fmax(mx, fabs(Q[i]));
  if (!(mx > 0.0) || !(mx < 1e300)) return false;
  const double w0 = ((Q[8] * (double)first.X + Q[9] * (double)first.Y) + Q[10] * (double)first.Z) + Q[11];
  const double sg = w0 < 0.0 ? -1.0 : 1.0;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double v = sg * (Q[i] / mx);
    finite = finite && (fabs(v) <= 1.0);                        // (false for NaN)
    P32[i] = (float)v;
  }
  return finite;
}

// ---- pair lists -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pnp_pack_kernel(PnpArgs a, const float* __restrict__ xy, const float* __restrict__ xyz,
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
    const size_t i = (size_t)f * stride + k;
    float4* out = a.rec + ((size_t)f * a.cap + k) * 2;
    out[0] = make_float4(xy[i * 2], xy[i * 2 + 1], xyz[i * 3], xyz[i * 3 + 1]);
    out[1] = make_float4(xyz[i * 3 + 2], __int_as_float(k), 0.f, 0.f);
  }
}

// The landmarks of frame f: fpc_pnp_frames' key (xyz [nkey][3], valid [nkey] or null, nkey[0]) with bank.slot null, or slot
// bank.slot[f] of the bank's landmark storage (float4 [slots][rows], w = 1 valid / 0; count [slots]).  A slot outside
// [0, slots) or a bank without landmark storage leaves the frame without pairs.
struct PnpTrain {
  const float* key_xyz;
  const uint8_t* key_valid;
  const int32_t* nkey;
  const int32_t* slot;          // [n] device
  const float4* lm;             // [slots][rows]
  const int32_t* count;         // [slots]
  int rows, slots;
};

// one workgroup per frame (per problem: PnpArgs::per_frame, with tr.slot and match holding an entry per problem); rows
// i < count[f] with 0 <= match < the train count and a valid landmark, in ascending i
__global__ __launch_bounds__(256) void pnp_gather_kernel(PnpArgs a, const int32_t* __restrict__ xy, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ match, uint8_t* mask, const PnpTrain tr) {
  const int f = blockIdx.x, cap = a.cap;
  const int fq = hf_frame(a.per_frame, f);     // the frame whose keypoints are the query side
  const int cnt = hf_clamp(count[fq], cap);
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
  // gather_body's Source: row i of frame f is a pair when its match is a row of the train set with a valid landmark, which
  // `pair` keeps for `write`
  struct {
    const PnpArgs& a;
    const PnpTrain& tr;
    const int32_t* qxy;
    const float4* lm;
    int f, nt;
    float X, Y, Z;
    __device__ __forceinline__ bool pair(int m) {
      X = Y = Z = 0.f;
      if (!(m >= 0 && m < nt)) return false;
      if (tr.slot) {
        const float4 p = lm[m];
        X = p.x; Y = p.y; Z = p.z;
        return p.w != 0.f;
      }
      X = tr.key_xyz[3 * (size_t)m]; Y = tr.key_xyz[3 * (size_t)m + 1]; Z = tr.key_xyz[3 * (size_t)m + 2];
      return (!tr.key_valid || tr.key_valid[m] != 0) && pnp_finite3(X, Y, Z);
    }
    __device__ __forceinline__ void write(int off, int i, int) {
      float4* out = a.rec + ((size_t)f * a.cap + off) * 2;
      out[0] = make_float4((float)qxy[2 * i], (float)qxy[2 * i + 1], X, Y);
      out[1] = make_float4(Z, __int_as_float(i), 0.f, 0.f);
    }
  } src{a, tr, xy + (size_t)fq * cap * 2, lm, f, nt, 0.f, 0.f, 0.f};
  gather_body(src, f, cnt, cap, match, mask, a.np, a.best);
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// score_body's Model.  P sits in twelve named registers on purpose: an indexed store becomes scratch.  (A degenerate
// hypothesis keeps P = 0: w = 0 is never > 0, it counts nothing.)
struct PnpModel {
  static constexpr int SAMPLE = PNP_SAMPLE, DRAWS = PNP_DRAWS, REC = 2;
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f, p4 = 0.f, p5 = 0.f, p6 = 0.f, p7 = 0.f, p8 = 0.f, p9 = 0.f, p10 = 0.f, p11 = 0.f;
  float thr;
  __device__ __forceinline__ explicit PnpModel(const PnpArgs& a) : thr(a.thr) {}
  static __device__ __forceinline__ const float4* records(const PnpArgs& a, int f) { return a.rec + (size_t)f * a.cap * 2; }
  static __device__ __forceinline__ int frame(const PnpArgs& a, int f) { return hf_frame(a.per_frame, f); }
  __device__ __forceinline__ bool solve(const PnpArgs& a, const float4* __restrict__ rec, const uint32_t (&idx)[PNP_SAMPLE],
                                        double* sys) {
    double P[12];
    PnpPair first;
    float P32[12];
    if (!(pnp_solve6<PNP_THREADS>(sys + threadIdx.x, rec, idx, a, P, first) && pnp_hypothesis(P, a, first, P32))) return false;
    p0 = P32[0]; p1 = P32[1]; p2 = P32[2]; p3 = P32[3]; p4 = P32[4]; p5 = P32[5];
    p6 = P32[6]; p7 = P32[7]; p8 = P32[8]; p9 = P32[9]; p10 = P32[10]; p11 = P32[11];
    return true;
  }
  __device__ __forceinline__ bool counts(const float4* r) const {
    const float4 q = r[0];
    const float Z = r[1].x;
    const float w = fmaf(p10, Z, fmaf(p9, q.w, fmaf(p8, q.z, p11)));
    const float u = fmaf(p2, Z, fmaf(p1, q.w, fmaf(p0, q.z, p3)));
    const float v = fmaf(p6, Z, fmaf(p5, q.w, fmaf(p4, q.z, p7)));
    const float ex = fmaf(-w, q.x, u), ey = fmaf(-w, q.y, v);
    const float tw = thr * w;
    return w > 0.f && fmaf(ex, ex, ey * ey) < tw * tw;
  }
};

__global__ __launch_bounds__(PNP_THREADS) void pnp_score_kernel(PnpArgs a) {
  __shared__ double sys[PNP_ROWS * PNP_COLS * PNP_THREADS];  // the systems; afterwards the staged pair chunk
  static_assert(sizeof(double) * PNP_ROWS * PNP_COLS * PNP_THREADS >= sizeof(float4) * 2 * PNP_CHUNK,
                "the pair chunk reuses the systems' LDS");
  score_body<PNP_THREADS, PnpModel>(a, reinterpret_cast<float4*>(sys), sys);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// P = [A | a4] (LDS, 12 doubles) -> the nearest pose: negated if det A < 0; A^T A = V diag(lambda) V^T by fm_jacobi at
// N = 3; R = A V diag(lambda^-1/2) V^T, sigma the mean of sqrt(lambda), t = a4 / sigma; out (LDS) gets the 12 fp32 values
// (R row-major, then t) as doubles.  false: the rank test fails or the result is not finite.  One lane.
__device__ __forceinline__ bool pnp_polar(double* P, double* A, double* V, double* W, double* out) {
  const double det = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) + P[2] * (P[4] * P[9] - P[5] * P[8]);
  if (det < 0.0)
    for (int i = 0; i < 12; ++i) P[i] = -P[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = P[i] * P[j] + P[4 + i] * P[4 + j] + P[8 + i] * P[8 + j];
  fm_jacobi(A, V, 3);
  const double l0 = A[0], l1 = A[4], l2 = A[8];
  const double lmin = fmin(l0, fmin(l1, l2)), lmax = fmax(l0, fmax(l1, l2));
  if (!(lmin > PNP_RANK * lmax)) return false;                  // (false for NaN)
  const double r0 = sqrt(l0), r1 = sqrt(l1), r2 = sqrt(l2);
  const double sigma = (r0 + r1 + r2) / 3.0;
  // W = V diag(1 / sqrt(lambda)) V^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W[i * 3 + j] = V[i * 3] * V[j * 3] / r0 + V[i * 3 + 1] * V[j * 3 + 1] / r1 + V[i * 3 + 2] * V[j * 3 + 2] / r2;
  bool finite = true;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const float v = (float)(P[i * 4] * W[j] + P[i * 4 + 1] * W[3 + j] + P[i * 4 + 2] * W[6 + j]);
      finite = finite && fabsf(v) < 3e38f;                      // (false for NaN and Inf)
      out[i * 3 + j] = (double)v;
    }
    const float v = (float)(P[i * 4 + 3] / sigma);
    finite = finite && fabsf(v) < 3e38f;
    out[9 + i] = (double)v;
  }
  return finite;
}

// the reprojection test of include/fpc.h in fp64; -> (a, b, c) = R X + t
__device__ __forceinline__ bool pnp_inlier(const double (&R)[9], const double (&t)[3], const PnpArgs& g, const PnpPair& p,
                                           double thr2, double& a, double& b, double& c) {
  const double X = p.X, Y = p.Y, Z = p.Z;
  a = R[0] * X + R[1] * Y + R[2] * Z + t[0];
  b = R[3] * X + R[4] * Y + R[5] * Z + t[1];
  c = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  const double ex = (double)g.fx * a - ((double)p.x - (double)g.cx) * c, ey = (double)g.fy * b - ((double)p.y - (double)g.cy) * c;
  return c > 0.0 && ex * ex + ey * ey < thr2 * c * c;
}

// The refit kernels' LDS, at namespace scope with internal linkage so that pnp_refit_body and the derive steps name the
// arrays directly: a kernel holds those its own code reaches and no others, and the optimiser treats them as it treats a
// kernel's own (an array handed over by pointer stays whole; tests/test_static_isa.py pins pnp_refit_kernel's size).
// hf_block_sum's partial sums, the sums for the solving lane, the Gauss-Newton system, the pose (12 fp32 values as doubles:
// R row-major, then t), the derive step's verdict ...
static __shared__ double pnp_refit_red[4 * PNP_NSUM];
static __shared__ double pnp_refit_s28[PNP_NSUM];
static __shared__ double pnp_refit_sm[6][7];
static __shared__ double pnp_refit_pose[12];
static __shared__ int pnp_refit_solved;
// ... and the DLT derive's own: the 11 x 12 system, the Jacobi's matrices, P
static __shared__ double pnp_refit_sys[PNP_ROWS * PNP_COLS];
static __shared__ double pnp_refit_jm[9], pnp_refit_jv[9], pnp_refit_jw[9];
static __shared__ double pnp_refit_pw[12];

// pnp_refit_body's Minimal of the DLT: the best sample's P by the score kernel's device function, then its polar step
struct PnpDlt {
  static constexpr int SAMPLE = PNP_SAMPLE;
  static __device__ __forceinline__ bool derive(const PnpArgs& a, const float4* __restrict__ rec, int f, unsigned long long key,
                                                int M) {
    double* const sys = pnp_refit_sys;
    double* const jm = pnp_refit_jm;
    double* const jv = pnp_refit_jv;
    double* const jw = pnp_refit_jw;
    double* const pw = pnp_refit_pw;
    double* const pose = pnp_refit_pose;
    uint32_t idx[PNP_SAMPLE];
    double P[12];
    PnpPair first;
    if (!(hf_sample_distinct<PNP_SAMPLE, PNP_DRAWS>(a.seed, (uint32_t)hf_frame(a.per_frame, f), ~(uint32_t)key, (uint32_t)M, idx) &&
          pnp_solve6<1>(sys, rec, idx, a, P, first)))
      return false;
#pragma unroll
    for (int i = 0; i < 12; ++i) pw[i] = P[i];
    return pnp_polar(pw, jm, jv, jw, pose);
  }
};

// A refit kernel of the absolute-pose models (workgroup of 256, one per problem).
//   Minimal::SAMPLE          the sample's size: the fewest pairs of a frame and the fewest inliers of a refit
//   Minimal::derive(a, rec, f, key, M)   one lane: the best sample's pose into pnp_refit_pose; false: the frame fails
//                            (f: the problem; the sampler's frame is hf_frame(a.per_frame, f))
template <class Minimal>
__device__ __forceinline__ void pnp_refit_body(const PnpArgs& a, float* __restrict__ Rout, float* __restrict__ tout,
                                               int32_t* __restrict__ ninl, uint8_t* mask, int mstride) {
  double* const red = pnp_refit_red;
  double* const s28 = pnp_refit_s28;
  double (*const sm)[7] = pnp_refit_sm;
  double* const pose = pnp_refit_pose;
  int& solved = pnp_refit_solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ rec = a.rec + (size_t)f * a.cap * 2;
  const double thr2 = (double)a.thr * (double)a.thr;
  const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
  double R[9], t[3];
  bool ok = refit_head(M >= Minimal::SAMPLE && key != 0ull, &solved, [&]() { return Minimal::derive(a, rec, f, key, M); });
  if (ok) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = pose[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = pose[9 + i];
    for (int r = 0; r < a.refits; ++r) {
      // one Gauss-Newton step: J^T J (upper triangle, row-major), J^T r and the count over the inliers of (R, t)
      double s[PNP_NSUM];
#pragma unroll
      for (int i = 0; i < PNP_NSUM; ++i) s[i] = 0.0;
      for (int k = tid; k < M; k += 256) {
        const PnpPair p = pnp_load(rec, k);
        double xa, xb, xc;
        if (pnp_inlier(R, t, a, p, thr2, xa, xb, xc)) {
          const double ic = 1.0 / xc, u = xa * ic, v = xb * ic;
          const double ru = fx * (u - ((double)p.x - cx) / fx), rv = fy * (v - ((double)p.y - cy) / fy);
          const double ju[6] = {fx * (-u * v), fx * (1.0 + u * u), fx * (-v), fx * ic, 0.0, fx * (-u * ic)};
          const double jv2[6] = {fy * (-(1.0 + v * v)), fy * (u * v), fy * u, 0.0, fy * ic, fy * (-v * ic)};
          int q = 0;
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) s[q++] += ju[i] * ju[j] + jv2[i] * jv2[j];
#pragma unroll
          for (int i = 0; i < 6; ++i) s[21 + i] += ju[i] * ru + jv2[i] * rv;
          s[27] += 1.0;
        }
      }
      hf_block_sum<PNP_NSUM>(s, red);
      if (s[27] < (double)Minimal::SAMPLE) break;
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < PNP_NSUM; ++i) s28[i] = s[i];                   // (through LDS: s[dynamic] would be scratch)
        int q = 0;
        double dmax = 0.0;
        for (int i = 0; i < 6; ++i) {
          for (int j = i; j < 6; ++j) { sm[i][j] = s28[q]; sm[j][i] = s28[q]; ++q; }
          sm[i][6] = -s28[21 + i];
          dmax = fmax(dmax, fabs(sm[i][i]));
        }
        int good = solve_lds<6>(sm, PNP_SINGULAR * dmax) ? 1 : 0;
        if (good) {
          const double w0 = sm[0][6], w1 = sm[1][6], w2 = sm[2][6], v0 = sm[3][6], v1 = sm[4][6], v2 = sm[5][6];
          const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
          double A = 1.0, B = 0.5;
          if (!(th2 < 1e-16)) {
            const double th = sqrt(th2);
            A = sin(th) / th;
            B = (1.0 - cos(th)) / th2;
          }
          // E = I + A [w]x + B [w]x^2,  [w]x^2 = w w^T - |w|^2 I
          const double E[9] = {1.0 + B * (w0 * w0 - th2), -A * w2 + B * w0 * w1, A * w1 + B * w0 * w2,
                               A * w2 + B * w0 * w1, 1.0 + B * (w1 * w1 - th2), -A * w0 + B * w1 * w2,
                               -A * w1 + B * w0 * w2, A * w0 + B * w1 * w2, 1.0 + B * (w2 * w2 - th2)};
          const double vv[3] = {v0, v1, v2};
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const float v = (float)(E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j] + E[i * 3 + 2] * R[6 + j]);
              if (!(fabsf(v) < 3e38f)) good = 0;
              pose[i * 3 + j] = (double)v;
            }
            const float v = (float)(E[i * 3] * t[0] + E[i * 3 + 1] * t[1] + E[i * 3 + 2] * t[2] + vv[i]);
            if (!(fabsf(v) < 3e38f)) good = 0;
            pose[9 + i] = (double)v;
          }
        }
        solved = good;
      }
      __syncthreads();
      if (!solved) break;                                                   // a singular system keeps the previous pose
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = pose[i];                           // (the next write of pose is behind hf_block_sum's barriers)
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = pose[9 + i];
    }
  }
  ok = refit_tail(ok, M, a.min_inliers, red, mask, ninl + f,
                  [&](int k) {
                    double xa, xb, xc;
                    return pnp_inlier(R, t, a, pnp_load(rec, k), thr2, xa, xb, xc);
                  },
                  [&](int k) { return (size_t)f * mstride + pnp_load(rec, k).row; });
  if (tid == 0) {                                                           // (through LDS: R[tid] would be scratch)
#pragma unroll
    for (int i = 0; i < 9; ++i) pose[i] = ok ? R[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[9 + i] = ok ? t[i] : 0.0;
  }
  __syncthreads();
  if (tid < 9) Rout[f * 9 + tid] = (float)pose[tid];
  if (tid < 3) tout[f * 3 + tid] = (float)pose[9 + tid];
}

__global__ __launch_bounds__(256) void pnp_refit_kernel(PnpArgs a, float* __restrict__ Rout, float* __restrict__ tout,
                                                        int32_t* __restrict__ ninl, uint8_t* mask, int mstride) {
  pnp_refit_body<PnpDlt>(a, Rout, tout, ninl, mask, mstride);
}

// ---- landmarks of the key-frame bank ----------------------------------------------------------------------------------
// rows i < count[slot] get (X, Y, Z, valid && finite ? 1 : 0), the rows behind the count (0, 0, 0, 0); grid ceil(rows / 256)
__global__ __launch_bounds__(256) void pnp_landmarks_store_kernel(float4* __restrict__ lm, const int32_t* __restrict__ count,
                                                                  int rows, int slot, const float* __restrict__ xyz,
                                                                  const uint8_t* __restrict__ valid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const int cnt = hf_clamp(count[slot], rows);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < cnt) {
    v.x = xyz[3 * (size_t)i]; v.y = xyz[3 * (size_t)i + 1]; v.z = xyz[3 * (size_t)i + 2];
    v.w = ((!valid || valid[i] != 0) && pnp_finite3(v.x, v.y, v.z)) ? 1.f : 0.f;
  }
  lm[(size_t)slot * rows + i] = v;
}

// grid (ceil(rows / 256), 1): slot `slot`; slot == -1, grid (ceil(rows / 256), slots): every slot
__global__ __launch_bounds__(256) void pnp_landmarks_invalidate_kernel(float4* __restrict__ lm, int rows, int slot) {
  const int i = blockIdx.x * 256 + threadIdx.x, s = slot >= 0 ? slot : (int)blockIdx.y;
  if (i >= rows) return;
  lm[(size_t)s * rows + i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
