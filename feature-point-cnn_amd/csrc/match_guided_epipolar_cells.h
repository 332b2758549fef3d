// match_guided_epipolar_cells.h -- epipolar guided matching over the spatial order of the rows: a strip visits only the train
// tiles the bands of its rows can reach (fpc_match_frames_guided_epipolar_cells / fpc_match_bank_guided_epipolar_cells,
// include/fpc.h).
//
// match_guided_epipolar_kernel (match_guided_epipolar.h) evaluates the gate against every 64 x 64 tile; rows come in
// confidence order, so a tile's pixels lie anywhere in the frame and some pair is always inside the band.  Here both sides
// are read through fpc_cell_order's permutation (cell_order_kernel, match_guided_cells.h: the kernel, its boxes and
// cell_order_passes are used as they are), and a strip tests every train tile's pixel box against the pencil of its 64
// epipolar lines before it touches the tile.  As in match_guided_cells.h the result is a function of the candidate set and
// of each candidate pair's d^2 bits alone, so the order rows are visited in does not show: the output is
// match_guided_epipolar_kernel's, bit for bit, ties included.
//
//   match_guided_epipolar_cells_kernel   the skeleton is match_guided_cells_kernel's (rows through perm, norms and pixels at
//                          the original index, the cull pass of four lanes per tile into the ascending LDS list by ballots,
//                          waves taking list entries w, w + 4, ..., 64-bit (d^2 bits, original index) keys for the top-2
//                          scan and the column atomicMin, stats); the gate and the tile are match_guided_epipolar_kernel's
//                          (the line prologue l0, l1, l2, g = l0^2 + l1^2 in LDS with g = -inf for a row that passes
//                          nowhere, l'0^2 + l'1^2 per train column, the 64-bit pass mask, 2 x 2 v_mfma_f32_32x32x2_f32
//                          blocks, K order, |q|^2 + |t|^2 - 2 q.t, clamp).
//       Cull.  In exact arithmetic (include/fpc.h): for row i and a tile with box [u0, u1] x [v0, v1], e = l0 u + l1 v + l2
//       is linear, so its range over the box is [e_lo, e_hi], the minimum and maximum over the four corners; m = 0 if
//       e_lo <= 0 <= e_hi, else min(|e_lo|, |e_hi|); G = max over the corners of l'0^2 + max over the corners of l'1^2
//       (l' = F^T (u, v, 1)); the row reaches the tile iff m^2 < radius^2 (g + G).
//       The kernel widens these bounds by an explicit rounding term, so that the argument does not depend on whether the
//       compiler contracts l0 u + l1 v + l2 into fused multiply-adds, here or in the gate.  With eps = 2^-50 (8 units in
//       the last place of a double rounded to nearest, unit u = 2^-53), the WIDENED RANGE of p s + q t + c over
//       s in [s0, s1], t in [t0, t1] is (mgec_range)
//           a0 = p s0, a1 = p s1, b0 = q t0, b1 = q t1,  A = max(|a0|, |a1|) + max(|b0|, |b1|) + |c|,
//           lo = min(a0, a1) + min(b0, b1) + c - 2 eps A,  hi = max(a0, a1) + max(b0, b1) + c + 2 eps A
//       (without the eps terms: the corner minimum and maximum), and the cull is
//           [lo, hi]   the widened range of e = l0 u + l1 v + l2 over the box,   m  = max(lo, -hi, 0),
//           [lo', hi'] that of l'0 = F00 u + F10 v + F20,                        M0 = max(|lo'|, |hi'|),  M1 likewise for l'1,
//           G = (M0 M0 + M1 M1) (1 + 2^-40),   hit iff m m < r2 (g + G).
//       Never rejects a tile that holds a candidate of the gate AS THE DEVICE COMPUTES IT.  Let (s, t) = (u, v) be a pixel
//       of the tile, u0 <= u <= u1, v0 <= v <= v1 (the box is that of the tile's ACTUAL pixels), S = |p s| + |q t| + |c|.
//       (1) Any evaluation of p s + q t + c in doubles -- two rounded products and two rounded sums, or fused multiply-adds
//           in either nesting -- rounds at most four times, each time a partial result of magnitude <= S (1 + u)^3: it lies
//           within 4.1 u S of the exact value.  The cull's corner sums round as often and the -+ 2 eps A once more: before
//           the widening they lie within 5.2 u S' of the exact corner minimum / maximum, S' the maximum of S over the box.
//           The computed A is >= (1 - u)^3 S', so 2 eps A = 16 u A exceeds 4.1 u S + 5.2 u S'.
//       (2) The exact e at (u, v) lies between the exact corner minimum and maximum (linearity).  By (1) the gate's
//           computed e_c lies in [lo, hi].  Hence |e_c| >= m >= 0, and the rounded product m m <= the rounded product
//           e_c e_c (rounding is monotone).
//       (3) The same for l': the gate's computed |m0| <= M0, |m1| <= M1.  The gate's tg = m0 m0 + m1 m1, fused or not, is
//           at most (m0^2 + m1^2) (1 + u)^2 <= (M0^2 + M1^2) (1 + u)^2; the computed M0 M0 + M1 M1 is at least
//           (M0^2 + M1^2) (1 - u)^2, and the factor 1 + 2^-40 (one more rounding) lifts it above: G >= tg.
//       (4) g + G and r2 (g + G) are the gate's g + tg and r2 (g + tg) with a larger operand: a rounded sum and a rounded
//           product by r2 > 0 (no contraction applies: no addition follows the product), monotone.  So the gate's
//           e_c e_c < r2 (g + tg) implies m m <= e_c e_c < r2 (g + tg) <= r2 (g + G): the cull keeps the tile.
//       A row past the count or a non-finite F has g = -inf: r2 (g + G) is -inf or NaN and nothing compares below it, as in
//       the gate.  Nine zeros give m = 0, g = G = 0 and 0 < 0: no tile is visited.  The widening is 2^-49 of the line's own
//       terms, far inside the 1 +- 1e-9 on the radius that the tests' float64 restatement of the exact rule allows for.
//       Selection, the list and the stats are match_guided_cells_kernel's, and match_guided_finalize_kernel / mf_row_ok run
//       unchanged behind it.
#pragma once
#include "match_guided_cells.h"

namespace fpc {

constexpr double MGEC_EPS2 = 0x1p-49;                    // 2 eps, eps = 2^-50
constexpr double MGEC_LIFT = 1.0 + 0x1p-40;

// The range of p s + q t + c over s in [s0, s1], t in [t0, t1]: the corner minimum and maximum, widened by 2 eps A.
__device__ __forceinline__ void mgec_range(double p, double q, double c, double s0, double s1, double t0, double t1,
                                           double& lo, double& hi) {
  const double a0 = p * s0, a1 = p * s1, b0 = q * t0, b1 = q * t1;
  const double A = fmax(fabs(a0), fabs(a1)) + fmax(fabs(b0), fabs(b1)) + fabs(c);
  lo = fmin(a0, a1) + fmin(b0, b1) + c - MGEC_EPS2 * A;
  hi = fmax(a0, a1) + fmax(b0, b1) + c + MGEC_EPS2 * A;
}

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_epipolar_cells_kernel(const MatchFramesArgs a, const MatchGuidedArgs g,
                                                                          const MatchCellsArgs c) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_l0[64], s_l1[64], s_l2[64], s_g[64];
  __shared__ int s_qi[64], s_ti[4][64];
  __shared__ unsigned short s_list[MGC_LIST];
  __shared__ int s_wcnt[4];
  const int f = blockIdx.y, q0 = blockIdx.x * MF_ROWS;
  const MfSets s = mf_sets(a, f);
  if (q0 >= s.nq || s.nt == 0) return;       // (the finalize kernel reads nq / nt itself)
  const int32_t* txy = mg_train_xy(a, g, f);
  const int32_t* qxy = g.xy + (size_t)f * a.cap * 2;
  const int32_t* pq = c.perm_q + (size_t)f * a.cap;
  const int32_t* pt;
  const int4* bt;
  if (a.pairing == 1 && f > 0) {             // the train set is frame f - 1: its query order
    pt = c.perm_q + (size_t)(f - 1) * a.cap;
    bt = c.box_q + (size_t)(f - 1) * c.nbox;
  } else if (a.key_slot) {
    pt = c.perm_t + (size_t)f * a.cap;
    bt = c.box_t + (size_t)f * c.nbox;
  } else {
    pt = c.perm_t;
    bt = c.box_t;
  }
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
    const int qi = pq[min(q0 + tid, s.nq - 1)];
    s_qi[tid] = qi;
    s_qn[tid] = s.qn[qi];
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
  for (int i = 0; i < 2; ++i) qrow[i] = s.q + (size_t)s_qi[i * 32 + l31] * a.D + half * 4;
  const int nrow = min(64, s.nq - q0);
  const int K8 = a.D / 8;
  float* tile = s_d2[wave];
  int* tidx = s_ti[wave];
  // lane = row of the strip: the two smallest (d^2 bits, original train index) keys
  unsigned long long k1 = ~0ull, k2 = ~0ull;
  const int ntiles = (s.nt + 63) / 64;
  int visited = 0;
  for (int lb = 0; lb < ntiles; lb += MGC_LIST) {
    // ---- the cull: four lanes per tile (16 rows of the strip each), 64 tiles per pass, into s_list in ascending order
    const int lend = min(ntiles, lb + MGC_LIST);
    int nlist = 0;
    for (int pb = lb; pb < lend; pb += 64) {
      const int tt = pb + wave * 16 + (lane >> 2);
      bool hit = false;
      if (tt < lend) {
        const int4 b = bt[tt];
        const double u0 = (double)b.x, v0 = (double)b.y, u1 = (double)b.z, v1 = (double)b.w;
        double lo, hi;
        mgec_range(fm[0], fm[3], fm[6], u0, u1, v0, v1, lo, hi);             // l'0 over the box
        const double M0 = fmax(fabs(lo), fabs(hi));
        mgec_range(fm[1], fm[4], fm[7], u0, u1, v0, v1, lo, hi);             // l'1 over the box
        const double M1 = fmax(fabs(lo), fabs(hi));
        const double G = (M0 * M0 + M1 * M1) * MGEC_LIFT;
        const int r0 = (lane & 3) * 16;
        for (int r = r0; r < r0 + 16 && !hit; ++r) {
          mgec_range(s_l0[r], s_l1[r], s_l2[r], u0, u1, v0, v1, lo, hi);     // e over the box
          const double m = fmax(fmax(lo, -hi), 0.0);
          hit = m * m < g.r2 * (s_g[r] + G);
        }
      }
      unsigned long long m = __ballot(hit);
      m |= m >> 1;
      m |= m >> 2;
      m &= 0x1111111111111111ull;                              // bit 4 k: tile k of this wave's 16 survives
      if (lane == 0) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      int at = nlist;
      for (int w = 0; w < wave; ++w) at += s_wcnt[w];
      if ((lane & 3) == 0 && ((m >> lane) & 1ull)) s_list[at + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(tt - lb);
      nlist += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      __syncthreads();
    }
    visited += nlist;
    // ---- the surviving tiles: match_guided_epipolar_kernel's tile, rows through the permutations
    for (int e = wave; e < nlist; e += 4) {
      const int t0 = (lb + (int)s_list[e]) * 64;
      const float* trow[2];
      float tn[2];
      double tu[2], tv[2], tg[2];
      bool tin[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int tj = pt[min(t0 + i * 32 + l31, s.nt - 1)];
        trow[i] = s.t + (size_t)tj * a.D + half * 4;
        tn[i] = s.tn[tj];
        tu[i] = (double)txy[2 * tj];
        tv[i] = (double)txy[2 * tj + 1];
        const double m0 = fm[0] * tu[i] + fm[3] * tv[i] + fm[6];           // l' = F^T (u, v, 1)^T
        const double m1 = fm[1] * tu[i] + fm[4] * tv[i] + fm[7];
        tg[i] = m0 * m0 + m1 * m1;
        tin[i] = t0 + i * 32 + l31 < s.nt;
      }
      const int tcol = pt[min(t0 + lane, s.nt - 1)];          // lane = column of the tile: its original train index
      tidx[lane] = tcol;
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
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the tile and its indices are private to this wave
      {
        const int ncol = min(64, s.nt - t0);
        const float4* rowp = reinterpret_cast<const float4*>(tile + lane * MF_PITCH);
#pragma unroll 4
        for (int j4 = 0; j4 < 16; ++j4) {
          const float4 v = rowp[j4];
          const float ev[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int j = j4 * 4 + k;
            if (j < ncol && ev[k] < INFINITY) {
              const unsigned long long key = ((unsigned long long)__float_as_uint(ev[k]) << 32) | (unsigned)tidx[j];
              if (key < k1) {
                k2 = k1; k1 = key;
              } else if (key < k2) {
                k2 = key;
              }
            }
          }
        }
      }
      if (a.cross_check) {                   // lane = column of the tile: the smallest (d^2 bits, original query index)
        unsigned long long best = ~0ull;
#pragma unroll 8
        for (int i = 0; i < 64; ++i) {
          const float ev = tile[i * MF_PITCH + lane];
          if (i < nrow && ev < INFINITY) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(ev) << 32) | (unsigned)s_qi[i];
            best = key < best ? key : best;
          }
        }
        if (t0 + lane < s.nt && best != ~0ull) atomicMin(colbest + tcol, best);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads of this tile done before the next tile overwrites it
    }
    __syncthreads();                                        // s_list is rebuilt by the next pass
  }
  s_top[wave][lane][0] = k1;
  s_top[wave][lane][1] = k2;
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
    unsigned long long* o = top2 + (size_t)s_qi[tid] * 2;
    o[0] = m1;
    o[1] = m2;
  }
  if (c.stats && tid == 0) {
    atomicAdd(c.stats + 2 * f, visited);
    atomicAdd(c.stats + 2 * f + 1, ntiles);
  }
}

}  // namespace fpc
