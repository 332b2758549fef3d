// match_guided_epipolar.h -- fpc_match_frames / the bank's table pass once more, under a fundamental matrix per frame as
// the gate (fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar, include/fpc.h).
//
// Everything but the gate is match_guided.h's: the sets, counts and tables are fpc_match_frames' own (mf_sets), the train
// pixels mg_train_xy's, the arguments MatchGuidedArgs with F in the H field.  Train row j at pixel (u, v) is a CANDIDATE of
// query row i at pixel (x, y) iff, in fp64 from the fp32 F of the frame, with l = F (x, y, 1)^T, l' = F^T (u, v, 1)^T and
// e = l0 u + l1 v + l2,
//     e^2 < radius^2 (l0^2 + l1^2 + l'0^2 + l'1^2)
// -- fpc_ransac_fundamental's inlier test with the radius as its threshold: no division, no sign condition -- and the
// result is fpc_match_frames' rule over the candidates only.
//
//   match_guided_epipolar_kernel   match_guided_kernel with this gate: one workgroup owns a 64-row strip of one frame, its
//                          four waves take the train tiles w, w+4, ...  The strip's 64 query rows get their line once, in
//                          fp64, into LDS (l0, l1, l2, l0^2 + l1^2; a row past the count or a non-finite F gets -inf in
//                          place of the last and passes nowhere: the bound is then -inf, or NaN).  Per train tile every
//                          lane computes l'0^2 + l'1^2 of its two train columns once, then evaluates its 64 pairs of the
//                          MFMA C/D layout (2 train columns x 32 query rows) into a 64-bit mask; a tile without a single
//                          passing pair in the wave is skipped before any descriptor load or MFMA.  Behind the mask the
//                          tile is match_guided_kernel's instruction for instruction -- the same 2 x 2
//                          v_mfma_f32_32x32x2_f32 blocks, K order, d^2 expression and clamp, so a candidate pair's d^2 has
//                          fpc_match_frames' bits; +inf for the pairs that fail the gate; the top-2 scan, the 64-bit
//                          atomicMin column minimum and the four-wave merge.
//   match_guided_finalize_kernel (match_guided.h) runs behind it as it is.
#pragma once
#include "match_guided.h"

namespace fpc {

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_epipolar_kernel(const MatchFramesArgs a, const MatchGuidedArgs g) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_l0[64], s_l1[64], s_l2[64], s_g[64];
  const int f = blockIdx.y, q0 = blockIdx.x * MF_ROWS;
  const MfSets s = mf_sets(a, f);
  if (q0 >= s.nq || s.nt == 0) return;       // (the finalize kernel reads nq / nt itself)
  const int32_t* txy = mg_train_xy(a, g, f);
  const int32_t* qxy = g.xy + (size_t)f * a.cap * 2;
  unsigned long long* top2 = a.top2 + (size_t)f * a.cap * 2;
  unsigned long long* colbest = a.colbest + (size_t)f * a.cap;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  // F of the frame (g.H: the field is shared with the homography gate), the same nine values in every lane
  const float* Ff = g.H + (size_t)f * 9;
  double fm[9];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    fm[k] = (double)Ff[k];
    finite = finite && fabs(fm[k]) <= 3.5e38;                // (false for NaN and Inf)
  }
  if (tid < 64) {
    s_qn[tid] = s.qn[min(q0 + tid, s.nq - 1)];
    const int qi = min(q0 + tid, s.nq - 1);
    const double x = (double)qxy[2 * qi], y = (double)qxy[2 * qi + 1];
    const double l0 = fm[0] * x + fm[1] * y + fm[2];
    const double l1 = fm[3] * x + fm[4] * y + fm[5];
    s_l0[tid] = l0;
    s_l1[tid] = l1;
    s_l2[tid] = fm[6] * x + fm[7] * y + fm[8];
    s_g[tid] = (finite && q0 + tid < s.nq) ? l0 * l0 + l1 * l1 : -(double)INFINITY;
  }
  __syncthreads();
  const float* qrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) qrow[i] = s.q + (size_t)min(q0 + i * 32 + l31, s.nq - 1) * a.D + half * 4;
  const int nrow = min(64, s.nq - q0);
  const int K8 = a.D / 8;
  float* tile = s_d2[wave];
  // lane = row of the strip: best and second best (strict <, columns ascending: ties keep the lower index)
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = -1, i2 = -1;
  const int ntiles = (s.nt + 63) / 64;
  for (int tt = wave; tt < ntiles; tt += 4) {
    const int t0 = tt * 64;
    const float* trow[2];
    float tn[2];
    double tu[2], tv[2], tg[2];
    bool tin[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tj = min(t0 + i * 32 + l31, s.nt - 1);
      trow[i] = s.t + (size_t)tj * a.D + half * 4;
      tn[i] = s.tn[tj];
      tu[i] = (double)txy[2 * tj];
      tv[i] = (double)txy[2 * tj + 1];
      const double m0 = fm[0] * tu[i] + fm[3] * tv[i] + fm[6];           // l' = F^T (u, v, 1)^T
      const double m1 = fm[1] * tu[i] + fm[4] * tv[i] + fm[7];
      tg[i] = m0 * m0 + m1 * m1;
      tin[i] = t0 + i * 32 + l31 < s.nt;
    }
    // the gate, in the C/D layout of the tile below: bit (mi * 16 + r) * 2 + ni of `pass`
    unsigned long long pass = 0ull;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const double l0 = s_l0[row], l1 = s_l1[row], l2 = s_l2[row], gq = s_g[row];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const double e = l0 * tu[ni] + l1 * tv[ni] + l2;
          if (tin[ni] && e * e < g.r2 * (gq + tg[ni])) pass |= 1ull << ((mi * 16 + r) * 2 + ni);
        }
      }
    if (__ballot(pass != 0ull) == 0ull) continue;            // no candidate in this tile: no loads, no MFMAs
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float4 qa[2], ta[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      qa[i] = *reinterpret_cast<const float4*>(qrow[i]);
      ta[i] = *reinterpret_cast<const float4*>(trow[i]);
    }
    for (int k8 = 0; k8 < K8; ++k8) {
      float4 qc[2], tc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        qc[i] = qa[i];
        tc[i] = ta[i];
        const int kn = k8 + 1 < K8 ? k8 + 1 : k8;
        qa[i] = *reinterpret_cast<const float4*>(qrow[i] + kn * 8);
        ta[i] = *reinterpret_cast<const float4*>(trow[i] + kn * 8);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const float af = j == 0 ? qc[mi].x : j == 1 ? qc[mi].y : j == 2 ? qc[mi].z : qc[mi].w;
            const float bf = j == 0 ? tc[ni].x : j == 1 ? tc[ni].y : j == 2 ? tc[ni].z : tc[ni].w;
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf, acc[mi][ni], 0, 0, 0);
          }
    }
    // C/D map: column (t) = lane & 31, row (q) = (r&3) + 8*(r>>2) + 4*half
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rowl = (r & 3) + 8 * (r >> 2) + 4 * half;
        const float qnr = s_qn[mi * 32 + rowl];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          float d2 = qnr + tn[ni] - 2.f * acc[mi][ni][r];
          d2 = d2 > 0.f ? d2 : 0.f;
          tile[(mi * 32 + rowl) * MF_PITCH + ni * 32 + l31] = (pass >> ((mi * 16 + r) * 2 + ni)) & 1ull ? d2 : INFINITY;
        }
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile is private to this wave
    {
      const int ncol = min(64, s.nt - t0);
      const float4* rowp = reinterpret_cast<const float4*>(tile + lane * MF_PITCH);
#pragma unroll 4
      for (int j4 = 0; j4 < 16; ++j4) {
        const float4 v = rowp[j4];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j4 * 4 + k;
          if (j < ncol) {
            if (e[k] < b1) {
              b2 = b1; i2 = i1; b1 = e[k]; i1 = t0 + j;
            } else if (e[k] < b2) {
              b2 = e[k]; i2 = t0 + j;
            }
          }
        }
      }
    }
    if (a.cross_check) {                   // lane = column of the tile: its arg-min over the strip's candidate rows
      const int tj = t0 + lane;
      float best = INFINITY;
      int bi = -1;
#pragma unroll 8
      for (int i = 0; i < 64; ++i) {
        const float e = tile[i * MF_PITCH + lane];
        if (i < nrow && e < best) { best = e; bi = i; }
      }
      if (tj < s.nt && bi >= 0)
        atomicMin(colbest + tj, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)(q0 + bi));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this tile done before the next tile overwrites it
  }
  s_top[wave][lane][0] = i1 >= 0 ? ((unsigned long long)__float_as_uint(b1) << 32) | (unsigned)i1 : ~0ull;
  s_top[wave][lane][1] = i2 >= 0 ? ((unsigned long long)__float_as_uint(b2) << 32) | (unsigned)i2 : ~0ull;
  __syncthreads();
  if (tid < MF_ROWS && q0 + tid < s.nq) {
    // top-2 of the four waves' lists on (d^2 bits, index): keys are distinct, the result is order-free
    unsigned long long m1 = ~0ull, m2 = ~0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const unsigned long long v = s_top[w][tid][k];
        if (v < m1) { m2 = m1; m1 = v; }
        else if (v < m2) m2 = v;
      }
    unsigned long long* o = top2 + (size_t)(q0 + tid) * 2;
    o[0] = m1;
    o[1] = m2;
  }
}

}  // namespace fpc
