// Batched RANSAC fundamental matrices (fpc_ransac_fundamental / fpc_fundamental_frames / fpc_fundamental_bank; the rule is
// stated in include/fpc.h and restated in float64 by tests/test_fundamental_ransac.py).  The pair records, their pack /
// gather kernels and the workspace are ransac_homography.h's.  This header holds the fundamental matrix's model -- the
// 8-point rows, the rank-2 projection and the finish, the Sampson tests -- and fm_jacobi, which pose_epipolar.h and
// pnp_ransac.h use too; the sampler, the selection key, the score and refit skeletons and the Hartley moments are
// ransac_parts.h's.  The full-pivot elimination inside fm_solve8 is written out here and again in pnp_solve6: as one shared
// function template it returned the same bits and cost both score kernels 6 % of their time.
//
//   fm_score_kernel   score_body at 128 hypotheses per workgroup: the normalised 8-point system in fp64 by Gaussian
//                     elimination with full pivoting.  The 8 x 9 system needs dynamic row and column indices, which in
//                     registers would become scratch, so it lives in LDS, struct-of-arrays (sys[72][128]: lanes doing the
//                     same step hit consecutive banks); the column permutation is nine nibbles of one 64-bit register.
//                     F then sits in 9 fp32 VGPRs and the pair list is staged through the LDS the systems occupied.
//   fm_refit_kernel   one workgroup per problem: one lane re-derives the best sample's F with the same device function
//                     (refit_head), then `refits` times two passes over the pairs (hartley_moments; the 36 sums of
//                     M = sum a a^T, a = q (x) p) in fp64 through hf_block_sum, and one lane's cyclic Jacobi in LDS (N = 9
//                     for the eigenvector, N = 3 for the rank-2 projection); through refit_tail it writes F, the inlier
//                     count and the mask of the F it returns.
#pragma once
#include "ransac_homography.h"

constexpr int FM_DRAWS = 32;          // draw budget of one sample
constexpr int FM_SAMPLE = 8;
constexpr int FM_THREADS = 128;       // hypotheses per workgroup of fm_score_kernel: 72 KiB of LDS, two workgroups per CU
constexpr double FM_PIVOT = 1e-10;    // last pivot / first pivot below which a sample is degenerate
constexpr int FM_SWEEPS = 10;         // cyclic Jacobi sweeps
constexpr int FM_NSUM = 36;

// F = Td^T Fn Ts,  Ts = [ss 0 -ss cx; 0 ss -ss cy; 0 0 1],  Td = [sd 0 -sd cu; 0 sd -sd cv; 0 0 1]
__device__ __forceinline__ void fm_denormalise(const double (&n)[9], const FmNorm& w, double (&F)[9]) {
#pragma clang fp contract(off)
  double g[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g[i * 3 + 0] = n[i * 3 + 0] * w.ss;
    g[i * 3 + 1] = n[i * 3 + 1] * w.ss;
    g[i * 3 + 2] = n[i * 3 + 2] - w.ss * (w.cx * n[i * 3 + 0] + w.cy * n[i * 3 + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = g[j] * w.sd;
    F[3 + j] = g[3 + j] * w.sd;
    F[6 + j] = g[6 + j] - w.sd * (w.cu * g[j] + w.cv * g[3 + j]);
  }
}

// The 8-point solve in the sample's own normalised coordinates.  sys: this thread's 8 x 9 system, element (r, c) at
// sys[(r * 9 + c) * S] (LDS).  Rows [ux uy u vx vy v x y 1]; elimination with full pivoting (the entry of largest magnitude
// of the remaining rows and columns; ties: lowest row, then lowest column), the null vector by back-substitution with the
// free unknown = 1: no coordinate of F is assumed non-zero.  Contraction is off so that the score kernel and the refit
// kernel, which inline this at different strides, compute the same bits.  false: degenerate.
template <int S>
__device__ __forceinline__ bool fm_solve8(double* sys, const float4* __restrict__ pairs, const uint32_t (&idx)[FM_SAMPLE],
                                          double (&Fn)[9], FmNorm& w) {
#pragma clang fp contract(off)
  float4 r[FM_SAMPLE];
#pragma unroll
  for (int i = 0; i < FM_SAMPLE; ++i) r[i] = pairs[idx[i]];
  double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
#pragma unroll
  for (int i = 0; i < FM_SAMPLE; ++i) { sx += (double)r[i].x; sy += (double)r[i].y; su += (double)r[i].z; sv += (double)r[i].w; }
  w.cx = sx / 8.0; w.cy = sy / 8.0; w.cu = su / 8.0; w.cv = sv / 8.0;
  double vs = 0.0, vd = 0.0;
#pragma unroll
  for (int i = 0; i < FM_SAMPLE; ++i) {
    const double dx = (double)r[i].x - w.cx, dy = (double)r[i].y - w.cy, du = (double)r[i].z - w.cu, dv = (double)r[i].w - w.cv;
    vs += dx * dx; vs += dy * dy;
    vd += du * du; vd += dv * dv;
  }
  vs = vs / 8.0; vd = vd / 8.0;
  if (!(vs > 1e-12) || !(vd > 1e-12)) return false;
  w.ss = sqrt(2.0 / vs); w.sd = sqrt(2.0 / vd);
#pragma unroll
  for (int i = 0; i < FM_SAMPLE; ++i) {
    const double x = ((double)r[i].x - w.cx) * w.ss, y = ((double)r[i].y - w.cy) * w.ss;
    const double u = ((double)r[i].z - w.cu) * w.sd, v = ((double)r[i].w - w.cv) * w.sd;
    double* row = sys + (size_t)i * 9 * S;
    row[0] = u * x; row[S] = u * y; row[2 * S] = u; row[3 * S] = v * x; row[4 * S] = v * y; row[5 * S] = v;
    row[6 * S] = x; row[7 * S] = y; row[8 * S] = 1.0;
  }
  unsigned long long perm = 0x876543210ull;     // nibble c: the unknown that column c holds
  double first = 0.0, last = 0.0;
#pragma unroll 1
  for (int c = 0; c < 8; ++c) {
    double pv = -1.0;
    int pr = c, pc = c;
    for (int i = c; i < 8; ++i)
      for (int j = c; j < 9; ++j) {
        const double v = fabs(sys[(i * 9 + j) * S]);
        if (v > pv) { pv = v; pr = i; pc = j; }
      }
    if (c == 0) first = pv;
    last = pv;
    if (!(pv > 0.0)) return false;
    if (pr != c)
      for (int j = c; j < 9; ++j) {
        const double tmp = sys[(c * 9 + j) * S];
        sys[(c * 9 + j) * S] = sys[(pr * 9 + j) * S];
        sys[(pr * 9 + j) * S] = tmp;
      }
    if (pc != c) {
      for (int i = 0; i < 8; ++i) {
        const double tmp = sys[(i * 9 + c) * S];
        sys[(i * 9 + c) * S] = sys[(i * 9 + pc) * S];
        sys[(i * 9 + pc) * S] = tmp;
      }
      const unsigned long long nc = (perm >> (4 * c)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
      perm = (perm & ~((15ull << (4 * c)) | (15ull << (4 * pc)))) | (np << (4 * c)) | (nc << (4 * pc));
    }
    const double piv = sys[(c * 9 + c) * S];
    for (int i = c + 1; i < 8; ++i) {
      const double fct = sys[(i * 9 + c) * S] / piv;
      for (int j = c + 1; j < 9; ++j) sys[(i * 9 + j) * S] = sys[(i * 9 + j) * S] - fct * sys[(c * 9 + j) * S];
    }
  }
  if (!(last >= FM_PIVOT * first)) return false;
  // back-substitution; y_i replaces the pivot it was divided by
#pragma unroll 1
  for (int i = 7; i >= 0; --i) {
    double acc = 0.0;
    for (int j = i + 1; j < 8; ++j) acc = acc + sys[(i * 9 + j) * S] * sys[(j * 9 + j) * S];
    acc = acc + sys[(i * 9 + 8) * S];
    sys[(i * 9 + i) * S] = -acc / sys[(i * 9 + i) * S];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) Fn[k] = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double yi = i < 8 ? sys[(i * 9 + i) * S] : 1.0;
    const int pi = (int)((perm >> (4 * i)) & 15ull);
#pragma unroll
    for (int k = 0; k < 9; ++k) Fn[k] = pi == k ? yi : Fn[k];
  }
  return true;
}

// the hypothesis as it is scored: denormalised, scaled to max |f| = 1, rounded to fp32.  false: not finite.
__device__ __forceinline__ bool fm_hypothesis(const double (&Fn)[9], const FmNorm& w, float (&F32)[9]) {
  double F[9];
  fm_denormalise(Fn, w, F);
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(F[i]));
  if (!(mx > 0.0) || !(mx < 1e300)) return false;            // (NaN fails the first test, Inf the second)
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = F[i] / mx;
    finite = finite && (fabs(v) <= 1.0);                     // (false for NaN)
    F32[i] = (float)v;
  }
  return finite;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// score_body's Model; F is only ever indexed by constants (fully unrolled), so it stays in registers.  (A degenerate
// hypothesis keeps F = 0: 0 < 0 is false, it counts nothing.  At T = 1, 127 of 128 lanes per frame are such lanes or beyond
// T: correct and idle, their loop costs what their wave's costs anyway.)
struct FmModel {
  static constexpr int SAMPLE = FM_SAMPLE, DRAWS = FM_DRAWS, REC = 1;
  float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float thr2;
  __device__ __forceinline__ explicit FmModel(const HfArgs& a) : thr2(a.thr * a.thr) {}
  static __device__ __forceinline__ const float4* records(const HfArgs& a, int f) { return a.pairs + (size_t)f * a.cap; }
  static __device__ __forceinline__ int frame(const HfArgs& a, int f) { return hf_frame(a.per_frame, f); }
  __device__ __forceinline__ bool solve(const HfArgs&, const float4* __restrict__ pairs, const uint32_t (&idx)[FM_SAMPLE],
                                        double* sys) {
    double Fn[9];
    FmNorm w;
    float F32[9];
    if (!(fm_solve8<FM_THREADS>(sys + threadIdx.x, pairs, idx, Fn, w) && fm_hypothesis(Fn, w, F32))) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = F32[i];
    return true;
  }
  __device__ __forceinline__ bool counts(const float4* r) const {
    const float4 p = r[0];
    const float l0 = fmaf(F[1], p.y, fmaf(F[0], p.x, F[2]));
    const float l1 = fmaf(F[4], p.y, fmaf(F[3], p.x, F[5]));
    const float l2 = fmaf(F[7], p.y, fmaf(F[6], p.x, F[8]));
    const float e = fmaf(p.w, l1, fmaf(p.z, l0, l2));
    const float m0 = fmaf(F[3], p.w, fmaf(F[0], p.z, F[6]));
    const float m1 = fmaf(F[4], p.w, fmaf(F[1], p.z, F[7]));
    const float g = fmaf(m1, m1, fmaf(m0, m0, fmaf(l1, l1, l0 * l0)));
    return e * e < thr2 * g;
  }
};

__global__ __launch_bounds__(FM_THREADS) void fm_score_kernel(HfArgs a) {
  __shared__ double sys[72 * FM_THREADS];                    // the systems; afterwards the staged pair chunk
  static_assert(sizeof(double) * 72 * FM_THREADS >= sizeof(float4) * HF_CHUNK, "the pair chunk reuses the systems' LDS");
  score_body<FM_THREADS, FmModel>(a, reinterpret_cast<float4*>(sys), sys);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// Cyclic Jacobi on the symmetric N x N matrix A (row-major, LDS), FM_SWEEPS sweeps over (p, q), p < q in row-major order;
// V (LDS) gets the eigenvectors as columns.  -> the index of the smallest diagonal entry (ties: the lowest).  One lane.
__device__ __forceinline__ int fm_jacobi(double* A, double* V, int N) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < FM_SWEEPS; ++sweep)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {                          // columns p, q of A and of V
          const double ap = A[k * N + p], aq = A[k * N + q];
          A[k * N + p] = c * ap - s * aq;
          A[k * N + q] = s * ap + c * aq;
          const double vp = V[k * N + p], vq = V[k * N + q];
          V[k * N + p] = c * vp - s * vq;
          V[k * N + q] = s * vp + c * vq;
        }
        for (int k = 0; k < N; ++k) {                          // rows p, q of A
          const double ap = A[p * N + k], aq = A[q * N + k];
          A[p * N + k] = c * ap - s * aq;
          A[q * N + k] = s * ap + c * aq;
        }
      }
  int best = 0;
  for (int i = 1; i < N; ++i)
    if (A[i * N + i] < A[best * N + best]) best = i;
  return best;
}

// F <- F - (F v3) v3^T, v3 the eigenvector of F^T F's smallest eigenvalue (F: 9 doubles in LDS; A, V: Jacobi's).  One lane.
__device__ __forceinline__ void fm_rank2(double* F, double* A, double* V) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = F[i] * F[j] + F[3 + i] * F[3 + j] + F[6 + i] * F[6 + j];
  const int m = fm_jacobi(A, V, 3);
  const double v0 = V[m], v1 = V[3 + m], v2 = V[6 + m];
  for (int i = 0; i < 3; ++i) {
    const double fv = F[i * 3] * v0 + F[i * 3 + 1] * v1 + F[i * 3 + 2] * v2;
    F[i * 3] -= fv * v0; F[i * 3 + 1] -= fv * v1; F[i * 3 + 2] -= fv * v2;
  }
}

// Fn (LDS, rank 2 already) -> denormalised, Frobenius norm 1, rounded to fp32, the element of largest magnitude of the
// ROUNDED values positive (ties: the lowest index); out (LDS) gets the fp32 values as doubles.  false: not finite.
__device__ __forceinline__ bool fm_finish(const double* Fn, const FmNorm& w, double* out) {
  double n[9], F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) n[i] = Fn[i];
  fm_denormalise(n, w, F);
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) q += F[i] * F[i];
  const double nrm = sqrt(q);
  if (!(nrm > 0.0) || !(nrm < 1e300)) return false;
  bool finite = true;
  float mxv = 0.f, mxa = -1.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = F[i] / nrm;
    finite = finite && (fabs(v) <= 1.0);                     // (false for NaN)
    const float v32 = (float)v;
    F[i] = (double)v32;
    if (fabsf(v32) > mxa) { mxa = fabsf(v32); mxv = v32; }
  }
  if (!finite) return false;
  const double sgn = mxv < 0.f ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = sgn * F[i];
  return true;
}

// the Sampson distance of a pair below thr, without the division, in fp64 (the test of include/fpc.h)
__device__ __forceinline__ bool fm_inlier(const double (&F)[9], const float4& p, double thr2) {
  const double x = p.x, y = p.y, u = p.z, v = p.w;
  const double l0 = F[0] * x + F[1] * y + F[2], l1 = F[3] * x + F[4] * y + F[5], l2 = F[6] * x + F[7] * y + F[8];
  const double e = u * l0 + v * l1 + l2;
  const double m0 = F[0] * u + F[3] * v + F[6], m1 = F[1] * u + F[4] * v + F[7];
  return e * e < thr2 * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1);
}

// index of the symmetric pair (i, j) of three: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
__device__ __forceinline__ int fm_sym3(int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo * 3 - lo * (lo - 1) / 2 + (hi - lo);
}

__global__ __launch_bounds__(256) void fm_refit_kernel(HfArgs a, float* __restrict__ Fout, int32_t* __restrict__ ninl,
                                                       uint8_t* mask, int mstride) {
  __shared__ double red[4 * FM_NSUM];
  __shared__ double sys[72];
  __shared__ double jm[81], jv[81];
  __shared__ double s36[FM_NSUM];
  __shared__ double fw[9], fnew[9];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const double thr2 = (double)a.thr * (double)a.thr;
  double F[9];
  bool ok = refit_head(M >= FM_SAMPLE && key != 0ull, &solved, [&]() {
    uint32_t idx[FM_SAMPLE];
    double Fn[9];
    FmNorm w;
    if (!(hf_sample_distinct<FM_SAMPLE, FM_DRAWS>(a.seed, (uint32_t)hf_frame(a.per_frame, f), ~(uint32_t)key, (uint32_t)M, idx) &&
          fm_solve8<1>(sys, pairs, idx, Fn, w)))
      return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) fw[i] = Fn[i];  // the sample's F as it is returned: rank 2 in its normalised coordinates
    fm_rank2(fw, jm, jv);
    return fm_finish(fw, w, fnew);
  });
  if (ok) {
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = fnew[i];
    for (int r = 0; r < a.refits; ++r) {
      FmNorm w;
      if (!hartley_moments(pairs, M, 8.0, red, [&](const float4& p) { return fm_inlier(F, p, thr2); }, w)) break;
      // M = sum a a^T with a = q (x) p: s[6 qq + pp], qq in (uu uv u vv v 1), pp in (xx xy x yy y 1)
      double s[FM_NSUM];
#pragma unroll
      for (int i = 0; i < FM_NSUM; ++i) s[i] = 0.0;
      for (int k = tid; k < M; k += 256) {
        const float4 p = pairs[k];
        if (fm_inlier(F, p, thr2)) {
          const double x = ((double)p.x - w.cx) * w.ss, y = ((double)p.y - w.cy) * w.ss;
          const double u = ((double)p.z - w.cu) * w.sd, v = ((double)p.w - w.cv) * w.sd;
          const double qq[6] = {u * u, u * v, u, v * v, v, 1.0}, pp[6] = {x * x, x * y, x, y * y, y, 1.0};
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) s[i * 6 + j] += qq[i] * pp[j];
        }
      }
      hf_block_sum<FM_NSUM>(s, red);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < FM_NSUM; ++i) s36[i] = s[i];                    // (through LDS: s[dynamic] would be scratch)
        for (int i = 0; i < 9; ++i)
          for (int j = 0; j < 9; ++j) jm[i * 9 + j] = s36[6 * fm_sym3(i / 3, j / 3) + fm_sym3(i % 3, j % 3)];
        const int m = fm_jacobi(jm, jv, 9);
        for (int i = 0; i < 9; ++i) fw[i] = jv[i * 9 + m];
        fm_rank2(fw, jm, jv);
        solved = fm_finish(fw, w, fnew) ? 1 : 0;
      }
      __syncthreads();
      if (!solved) break;                                                   // a non-finite result keeps the previous F
#pragma unroll
      for (int i = 0; i < 9; ++i) F[i] = fnew[i];                           // (the next write of fnew is behind hf_block_sum's barriers)
    }
  }
  ok = refit_tail(ok, M, a.min_inliers, red, mask, ninl + f, [&](int k) { return fm_inlier(F, pairs[k], thr2); },
                  [&](int k) { return (size_t)f * mstride + a.row[(size_t)f * a.cap + k]; });
  if (tid == 0) {                                                           // (through LDS: F[tid] would be scratch)
#pragma unroll
    for (int i = 0; i < 9; ++i) fnew[i] = ok ? F[i] : 0.0;
  }
  __syncthreads();
  if (tid < 9) Fout[f * 9 + tid] = (float)fnew[tid];
}
