// Batched RANSAC homography estimation (fpc_ransac_homography / fpc_homography_frames; the rule is stated in
// include/fpc.h and restated in float64 by tests/test_homography_ransac.py).  This header holds the homography's model --
// the 4-point closed form, the refit's normal equations and denormalisation, the two inlier tests -- and the pair records
// every family shares; the sampler, the selection key, the compaction, the score and refit skeletons, the LDS solve and the
// Hartley moments are ransac_parts.h's.
//
//   hf_pack_kernel / hf_gather_kernel   build every frame's pair list [x, y, u, v] (float32, 16-byte records), the row of
//                          the caller's mask each pair belongs to, the pair count, and zero the best key and the mask.
//                          The gather is gather_body's order-preserving compaction, so the list is in ascending row
//                          order; from here on both entry points run the same kernels on the same records, which is
//                          what makes them bit-identical on equal pairs.
//   ransac_score_kernel    score_body at 256 hypotheses per workgroup: the 4-point homography in fp64 registers (closed
//                          form through the projective basis: cross products and adjugates, no pivoting, no division),
//                          kept in 9 fp32 VGPRs for the walk over the staged pair list.
//   ransac_refit_kernel    one workgroup per frame: re-derives the best sample's H, then `refits` times a Hartley-
//                          normalised least-squares fit over the current inliers -- hartley_moments, then the normal
//                          equations accumulated in fp64 per thread over a fixed stride and summed by hf_block_sum (no
//                          floating-point atomics), solved by one lane with solve_lds -- and, through refit_tail, writes
//                          H, the inlier count and the mask of the H it returns.
#pragma once
#include "ransac_parts.h"

constexpr int HF_DRAWS = 16;          // draw budget of one sample
constexpr double HF_COLLINEAR = 0.5;  // doubled triangle area (px^2) below which three points count as collinear

struct HfArgs {
  float4* pairs;                // [B][cap]  x, y (query / src), u, v (train / dst)
  int32_t* row;                 // [B][cap]  the mask row of pair k
  int32_t* np;                  // [B]       pairs of the frame
  unsigned long long* best;     // [B]       (inlier count << 32) | ~t of the best hypothesis; 0: none
  int cap, n;
  int T, refits, min_inliers;
  float thr;
  uint32_t seed;
  // fpc_homography_bank_topk (match_bank_topk.h): the grid's index is a PROBLEM p = f per_frame + j, several per frame; it
  // selects the pair list, the mask row and the slot, while the frame f = p / per_frame selects the query pixels and feeds
  // the sampler.  0 (every other entry point): one problem per frame, p = f.
  int per_frame;
};

struct HfV3 { double x, y, z; };
__device__ __forceinline__ HfV3 hf_cross(const HfV3& a, const HfV3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double hf_dot(const HfV3& a, const HfV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ HfV3 hf_scale(const HfV3& a, double s) { return {a.x * s, a.y * s, a.z * s}; }

// The homography through 4 pairs.  With p_i = (x_i, y_i, 1): l_i = the triple products (p_j x p_k) . p_3, A = [l_0 p_0,
// l_1 p_1, l_2 p_2] maps the projective basis to the src points ((1,1,1) -> det(p_0 p_1 p_2) p_3), B likewise for dst,
// H = B adj(A).  The four triple products of a side are the doubled areas of its four triangles: the collinearity test.
// H is scaled to max |h| = 1 and oriented so that w > 0 at the sample's first point.  false: degenerate.
__device__ __forceinline__ bool hf_solve4(const float4& r0, const float4& r1, const float4& r2, const float4& r3,
                                          double (&H)[9]) {
  const HfV3 p0{r0.x, r0.y, 1.0}, p1{r1.x, r1.y, 1.0}, p2{r2.x, r2.y, 1.0}, p3{r3.x, r3.y, 1.0};
  const HfV3 q0{r0.z, r0.w, 1.0}, q1{r1.z, r1.w, 1.0}, q2{r2.z, r2.w, 1.0}, q3{r3.z, r3.w, 1.0};
  const HfV3 c12 = hf_cross(p1, p2), c20 = hf_cross(p2, p0), c01 = hf_cross(p0, p1);
  const double l0 = hf_dot(c12, p3), l1 = hf_dot(c20, p3), l2 = hf_dot(c01, p3), dp = hf_dot(c01, p2);
  const double m0 = hf_dot(hf_cross(q1, q2), q3), m1 = hf_dot(hf_cross(q2, q0), q3), m2 = hf_dot(hf_cross(q0, q1), q3);
  const double dq = hf_dot(hf_cross(q0, q1), q2);
  if (!(fabs(l0) >= HF_COLLINEAR && fabs(l1) >= HF_COLLINEAR && fabs(l2) >= HF_COLLINEAR && fabs(dp) >= HF_COLLINEAR &&
        fabs(m0) >= HF_COLLINEAR && fabs(m1) >= HF_COLLINEAR && fabs(m2) >= HF_COLLINEAR && fabs(dq) >= HF_COLLINEAR))
    return false;
  const HfV3 a0 = hf_scale(c12, l1 * l2), a1 = hf_scale(c20, l2 * l0), a2 = hf_scale(c01, l0 * l1);   // rows of adj(A)
  const HfV3 b0 = hf_scale(q0, m0), b1 = hf_scale(q1, m1), b2 = hf_scale(q2, m2);                      // columns of B
  H[0] = b0.x * a0.x + b1.x * a1.x + b2.x * a2.x; H[1] = b0.x * a0.y + b1.x * a1.y + b2.x * a2.y; H[2] = b0.x * a0.z + b1.x * a1.z + b2.x * a2.z;
  H[3] = b0.y * a0.x + b1.y * a1.x + b2.y * a2.x; H[4] = b0.y * a0.y + b1.y * a1.y + b2.y * a2.y; H[5] = b0.y * a0.z + b1.y * a1.z + b2.y * a2.z;
  H[6] = b0.z * a0.x + b1.z * a1.x + b2.z * a2.x; H[7] = b0.z * a0.y + b1.z * a1.y + b2.z * a2.y; H[8] = b0.z * a0.z + b1.z * a1.z + b2.z * a2.z;
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(H[i]));
  if (!(mx > 0.0) || !(mx < 1e300)) return false;         // (NaN fails the first test, Inf the second)
  const double w0 = H[6] * p0.x + H[7] * p0.y + H[8];
  const double s = (w0 < 0.0 ? -1.0 : 1.0) / mx;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    H[i] *= s;
    finite = finite && (fabs(H[i]) <= 1.0);               // (false for NaN)
  }
  return finite && fabs(H[8]) > 1e-12;                     // H must be expressible with H[8] = 1
}

// ---- pair lists -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hf_pack_kernel(HfArgs a, const float* __restrict__ src, const float* __restrict__ dst,
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
    const size_t i = ((size_t)f * stride + k) * 2;
    a.pairs[(size_t)f * a.cap + k] = make_float4(src[i], src[i + 1], dst[i], dst[i + 1]);
    a.row[(size_t)f * a.cap + k] = k;
  }
}

// fpc_homography_bank: frame f's train coordinates are slot slot[f] of a key-frame bank (xy [slots][rows][2] passed as
// key_xy, count [slots]); a slot outside [0, slots) leaves the frame without pairs.  All null / 0 in fpc_homography_frames.
struct HfBank {
  const int32_t* slot;          // [n] device
  const int32_t* count;         // [slots]
  int rows, slots;
};

// one workgroup per frame (per problem: HfArgs::per_frame); rows i < count[f] with 0 <= match < the train set's row count,
// in ascending i
__global__ __launch_bounds__(256) void hf_gather_kernel(HfArgs a, const int32_t* __restrict__ xy, const int32_t* __restrict__ count,
                                                        int pairing, const int32_t* __restrict__ key_xy,
                                                        const int32_t* __restrict__ nkey, const int32_t* __restrict__ match,
                                                        uint8_t* mask, const HfBank bank) {
  const int f = blockIdx.x, cap = a.cap;
  const int fq = hf_frame(a.per_frame, f);     // the frame whose keypoints are the query side
  const int cnt = hf_clamp(count[fq], cap);
  const int32_t* txy = nullptr;
  int nt = 0;
  if (bank.slot) {                            // a per-frame train table: slot bank.slot[f] of key_xy [slots][rows][2]
    const int sl = bank.slot[f];
    if (sl >= 0 && sl < bank.slots) {
      txy = key_xy + (size_t)sl * bank.rows * 2;
      nt = hf_clamp(bank.count[sl], bank.rows);
    }
  } else if (pairing == 1 && f > 0) {
    txy = xy + (size_t)(f - 1) * cap * 2;
    nt = hf_clamp(count[f - 1], cap);
  } else if (key_xy) {
    txy = key_xy;
    nt = hf_clamp(nkey[0], cap);
  }
  // gather_body's Source: row i of problem f is a pair when its match is a row of the train set
  struct {
    const HfArgs& a;
    const int32_t *qxy, *txy;
    int f, nt;
    __device__ __forceinline__ bool pair(int m) { return m >= 0 && m < nt; }
    __device__ __forceinline__ void write(int off, int i, int m) {
      a.pairs[(size_t)f * a.cap + off] = make_float4((float)qxy[2 * i], (float)qxy[2 * i + 1], (float)txy[2 * m], (float)txy[2 * m + 1]);
      a.row[(size_t)f * a.cap + off] = i;
    }
  } src{a, xy + (size_t)fq * cap * 2, txy, f, nt};
  gather_body(src, f, cnt, cap, match, mask, a.np, a.best);
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// score_body's Model.  H sits in nine named registers on purpose: an indexed store becomes scratch.  (A degenerate
// hypothesis keeps H = 0: w = 0 is never > 0, it counts nothing.)
struct HfModel {
  static constexpr int SAMPLE = 4, DRAWS = HF_DRAWS, REC = 1;
  float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f, h5 = 0.f, h6 = 0.f, h7 = 0.f, h8 = 0.f;
  float thr;
  __device__ __forceinline__ explicit HfModel(const HfArgs& a) : thr(a.thr) {}
  static __device__ __forceinline__ const float4* records(const HfArgs& a, int f) { return a.pairs + (size_t)f * a.cap; }
  static __device__ __forceinline__ int frame(const HfArgs& a, int f) { return hf_frame(a.per_frame, f); }
  __device__ __forceinline__ bool solve(const HfArgs&, const float4* __restrict__ pairs, const uint32_t (&idx)[4], double*) {
    double H[9];
    if (!hf_solve4(pairs[idx[0]], pairs[idx[1]], pairs[idx[2]], pairs[idx[3]], H)) return false;
    h0 = (float)H[0]; h1 = (float)H[1]; h2 = (float)H[2]; h3 = (float)H[3]; h4 = (float)H[4];
    h5 = (float)H[5]; h6 = (float)H[6]; h7 = (float)H[7]; h8 = (float)H[8];
    return true;
  }
  __device__ __forceinline__ bool counts(const float4* r) const {
    const float4 p = r[0];
    const float w = fmaf(h7, p.y, fmaf(h6, p.x, h8));
    const float ex = fmaf(-w, p.z, fmaf(h1, p.y, fmaf(h0, p.x, h2)));
    const float ey = fmaf(-w, p.w, fmaf(h4, p.y, fmaf(h3, p.x, h5)));
    const float tw = thr * w;
    return w > 0.f && fmaf(ex, ex, ey * ey) < tw * tw;
  }
};

__global__ __launch_bounds__(256) void ransac_score_kernel(HfArgs a) {
  __shared__ float4 rec[HF_CHUNK];
  score_body<256, HfModel>(a, rec, nullptr);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// |H p - q| < thr without the division, in fp64 (sign-free: the plain reprojection test of include/fpc.h)
__device__ __forceinline__ bool hf_inlier(const double (&H)[9], const float4& p, double thr2) {
  const double x = p.x, y = p.y;
  const double w = H[6] * x + H[7] * y + H[8];
  const double ex = H[0] * x + H[1] * y + H[2] - w * (double)p.z, ey = H[3] * x + H[4] * y + H[5] - w * (double)p.w;
  return ex * ex + ey * ey < thr2 * w * w;
}

constexpr int HF_NSUM = 23;

__global__ __launch_bounds__(256) void ransac_refit_kernel(HfArgs a, float* __restrict__ Hout, int32_t* __restrict__ ninl,
                                                           uint8_t* mask, int mstride) {
  __shared__ double red[4 * HF_NSUM];
  __shared__ double sm[8][9];
  __shared__ double hnew[9];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const double thr2 = (double)a.thr * (double)a.thr;
  double H[9];
  bool ok = M >= 4 && key != 0ull;
  if (ok) {                                   // (uniform) every thread re-derives the best sample's H: same code, same bits
    uint32_t idx[4];
    ok = hf_sample_distinct<4, HF_DRAWS>(a.seed, (uint32_t)hf_frame(a.per_frame, f), ~(uint32_t)key, (uint32_t)M, idx) &&
         hf_solve4(pairs[idx[0]], pairs[idx[1]], pairs[idx[2]], pairs[idx[3]], H);
  }
  if (ok) {
    const double inv = 1.0 / H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = (double)(float)(H[i] * inv);        // the H that would be returned: fp32 values
    H[8] = 1.0;
    for (int r = 0; r < a.refits; ++r) {
      FmNorm w;
      if (!hartley_moments(pairs, M, 4.0, red, [&](const float4& p) { return hf_inlier(H, p, thr2); }, w)) break;
      const double cx = w.cx, cy = w.cy, ss = w.ss, cu = w.cu, cv = w.cv, sd = w.sd;
      // normal equations of [x y 1 0 0 0 -ux -uy | u], [0 0 0 x y 1 -vx -vy | v] in the normalised coordinates
      double s[HF_NSUM];
#pragma unroll
      for (int i = 0; i < HF_NSUM; ++i) s[i] = 0.0;
      for (int k = tid; k < M; k += 256) {
        const float4 p = pairs[k];
        if (hf_inlier(H, p, thr2)) {
          const double x = ((double)p.x - cx) * ss, y = ((double)p.y - cy) * ss;
          const double u = ((double)p.z - cu) * sd, v = ((double)p.w - cv) * sd;
          const double xx = x * x, xy = x * y, yy = y * y, w2 = u * u + v * v;
          s[0] += xx; s[1] += xy; s[2] += yy; s[3] += x; s[4] += y; s[5] += 1.0;
          s[6] += u * xx; s[7] += u * xy; s[8] += u * yy; s[9] += u * x; s[10] += u * y; s[11] += u;
          s[12] += v * xx; s[13] += v * xy; s[14] += v * yy; s[15] += v * x; s[16] += v * y; s[17] += v;
          s[18] += w2 * xx; s[19] += w2 * xy; s[20] += w2 * yy; s[21] += w2 * x; s[22] += w2 * y;
        }
      }
      hf_block_sum<HF_NSUM>(s, red);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 9; ++j) sm[i][j] = 0.0;
        sm[0][0] = s[0]; sm[0][1] = s[1]; sm[0][2] = s[3]; sm[0][6] = -s[6]; sm[0][7] = -s[7]; sm[0][8] = s[9];
        sm[1][1] = s[2]; sm[1][2] = s[4]; sm[1][6] = -s[7]; sm[1][7] = -s[8]; sm[1][8] = s[10];
        sm[2][2] = s[5]; sm[2][6] = -s[9]; sm[2][7] = -s[10]; sm[2][8] = s[11];
        sm[3][3] = s[0]; sm[3][4] = s[1]; sm[3][5] = s[3]; sm[3][6] = -s[12]; sm[3][7] = -s[13]; sm[3][8] = s[15];
        sm[4][4] = s[2]; sm[4][5] = s[4]; sm[4][6] = -s[13]; sm[4][7] = -s[14]; sm[4][8] = s[16];
        sm[5][5] = s[5]; sm[5][6] = -s[15]; sm[5][7] = -s[16]; sm[5][8] = s[17];
        sm[6][6] = s[18]; sm[6][7] = s[19]; sm[6][8] = -s[21];
        sm[7][7] = s[20]; sm[7][8] = -s[22];
        for (int i = 1; i < 8; ++i)
          for (int j = 0; j < i; ++j) sm[i][j] = sm[j][i];
        int good = solve_lds<8>(sm, 1e-10 * s[5]) ? 1 : 0;
        if (good) {
          const double n0 = sm[0][8], n1 = sm[1][8], n2 = sm[2][8], n3 = sm[3][8], n4 = sm[4][8], n5 = sm[5][8],
                       n6 = sm[6][8], n7 = sm[7][8];
          // H = Td^-1 Hn Ts,  Ts = [ss 0 -ss cx; 0 ss -ss cy; 0 0 1],  Td^-1 = [1/sd 0 cu; 0 1/sd cv; 0 0 1]
          const double m00 = n0 * ss, m01 = n1 * ss, m02 = n2 - ss * (cx * n0 + cy * n1);
          const double m10 = n3 * ss, m11 = n4 * ss, m12 = n5 - ss * (cx * n3 + cy * n4);
          const double m20 = n6 * ss, m21 = n7 * ss, m22 = 1.0 - ss * (cx * n6 + cy * n7);
          const double isd = 1.0 / sd;
          const double g0 = m00 * isd + cu * m20, g1 = m01 * isd + cu * m21, g2 = m02 * isd + cu * m22;
          const double g3 = m10 * isd + cv * m20, g4 = m11 * isd + cv * m21, g5 = m12 * isd + cv * m22;
          double mx = fmax(fmax(fmax(fabs(g0), fabs(g1)), fmax(fabs(g2), fabs(g3))), fmax(fmax(fabs(g4), fabs(g5)), fmax(fabs(m20), fabs(m21))));
          mx = fmax(mx, fabs(m22));
          if (!(mx < 1e300) || !(fabs(m22) > 1e-12 * mx)) good = 0;
          else {
            const double i22 = 1.0 / m22;
            hnew[0] = (double)(float)(g0 * i22); hnew[1] = (double)(float)(g1 * i22); hnew[2] = (double)(float)(g2 * i22);
            hnew[3] = (double)(float)(g3 * i22); hnew[4] = (double)(float)(g4 * i22); hnew[5] = (double)(float)(g5 * i22);
            hnew[6] = (double)(float)(m20 * i22); hnew[7] = (double)(float)(m21 * i22); hnew[8] = 1.0;
            for (int i = 0; i < 8; ++i)
              if (!(fabs(hnew[i]) < 3e38)) good = 0;
          }
        }
        solved = good;
      }
      __syncthreads();
      if (!solved) break;                                                   // a singular system keeps the previous H
#pragma unroll
      for (int i = 0; i < 9; ++i) H[i] = hnew[i];
    }
  }
  ok = refit_tail(ok, M, a.min_inliers, red, mask, ninl + f, [&](int k) { return hf_inlier(H, pairs[k], thr2); },
                  [&](int k) { return (size_t)f * mstride + a.row[(size_t)f * a.cap + k]; });
  if (tid == 0) {                                                           // (through LDS: H[tid] would be scratch)
#pragma unroll
    for (int i = 0; i < 9; ++i) hnew[i] = ok ? H[i] : 0.0;
  }
  __syncthreads();
  if (tid < 9) Hout[f * 9 + tid] = (float)hnew[tid];
}
