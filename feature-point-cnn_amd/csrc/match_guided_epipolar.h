// match_guided_epipolar.h -- fpc_match_frames / the bank's table pass once more, under a fundamental matrix per frame as
// the gate, plain and over the spatial order of the rows (fpc_match_frames_guided_epipolar[_cells] /
// fpc_match_bank_guided_epipolar[_cells], include/fpc.h).
//
// Everything but the gate is match_guided.h's and match_guided_cells.h's: the sets, counts and tables are
// fpc_match_frames' own (mf_sets), the train pixels mg_train_xy's, the arguments MatchGuidedArgs with F in the H field, the
// two skeletons mg_strip and mgc_strip, the order cell_order_kernel's with its boxes and cell_order_passes as they are.
// Train row j at pixel (u, v) is a CANDIDATE of query row i at pixel (x, y) iff, in fp64 from the fp32 F of the frame,
// with l = F (x, y, 1)^T, l' = F^T (u, v, 1)^T and e = l0 u + l1 v + l2,
//     e^2 < radius^2 (l0^2 + l1^2 + l'0^2 + l'1^2)
// -- fpc_ransac_fundamental's inlier test with the radius as its threshold: no division, no sign condition -- and the
// result is fpc_match_frames' rule over the candidates only.
//
//   MgEpipolar             the gate.  The strip's 64 query rows get their line once, in fp64, into LDS (l0, l1, l2,
//                          g = l0^2 + l1^2; a row past the count or a non-finite F gets -inf in place of the last and
//                          passes nowhere: the bound is then -inf, or NaN).  Per train tile every lane computes
//                          l'0^2 + l'1^2 of its two train columns once (column()).  F's nine values are kept in every
//                          lane.
//   match_guided_epipolar_kernel         the plain strip with this gate, every tile is tested: mg_strip and the gate written
//                          out in one function (see the note in front of it).
//   match_guided_epipolar_cells_kernel   mgc_strip<MgEpipolar>: a strip tests every train tile's pixel box against the
//                          pencil of its 64 epipolar lines before it touches the tile.  Rows come in confidence order, so in
//                          the plain kernel a tile's pixels lie anywhere in the frame and some pair is always inside the
//                          band; as in match_guided_cells.h the output is the plain kernel's, bit for bit, ties included.
//   match_guided_finalize_kernel (match_guided.h) runs behind both as it is.
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

struct MgEpipolar {
  struct Row { double l0, l1, l2, g; };         // a query row of the strip: its line and l0^2 + l1^2
  struct Col { double u, v, tg; };              // a train pixel and l'0^2 + l'1^2 of its line
  struct Box { double u0, v0, u1, v1, G; };     // a tile's pixel box and the cull's bound on tg over it
  double fm[9];                                 // F of the frame (g.H: the field is shared with the homography gate)
  const double r2;
  double *s_l0, *s_l1, *s_l2, *s_g;             // LDS, [64] each

  __device__ __forceinline__ MgEpipolar(const MatchGuidedArgs& g, int f, double* l0, double* l1, double* l2, double* l3)
      : r2(g.r2), s_l0(l1), s_l1(l2), s_l2(l3), s_g(l0) {
    const float* Ff = g.H + (size_t)f * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) fm[k] = (double)Ff[k];
  }

  // row i of the strip is row qi of the frame's pixels xy; live: it is below the frame's count
  __device__ __forceinline__ void row(int i, const int32_t* xy, int qi, bool live) const {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite = finite && fabs(fm[k]) <= 3.5e38;      // (false for NaN and Inf)
    const double x = (double)xy[2 * qi], y = (double)xy[2 * qi + 1];
    const double l0 = fm[0] * x + fm[1] * y + fm[2];
    const double l1 = fm[3] * x + fm[4] * y + fm[5];
    s_l0[i] = l0;
    s_l1[i] = l1;
    s_l2[i] = fm[6] * x + fm[7] * y + fm[8];
    s_g[i] = (finite && live) ? l0 * l0 + l1 * l1 : -(double)INFINITY;
  }
  __device__ __forceinline__ Row line(int i) const { return Row{s_l0[i], s_l1[i], s_l2[i], s_g[i]}; }
  __device__ __forceinline__ Col column(const int32_t* xy, int tj) const {
    const double u = (double)xy[2 * tj], v = (double)xy[2 * tj + 1];
    const double m0 = fm[0] * u + fm[3] * v + fm[6];           // l' = F^T (u, v, 1)^T
    const double m1 = fm[1] * u + fm[4] * v + fm[7];
    return Col{u, v, m0 * m0 + m1 * m1};
  }
  __device__ __forceinline__ bool pass(const Row& q, const Col& c) const {
    const double e = q.l0 * c.u + q.l1 * c.v + q.l2;
    return e * e < r2 * (q.g + c.tg);
  }

  // Cull.  In exact arithmetic (include/fpc.h): for row i and a tile with box [u0, u1] x [v0, v1], e = l0 u + l1 v + l2
  // is linear, so its range over the box is [e_lo, e_hi], the minimum and maximum over the four corners; m = 0 if
  // e_lo <= 0 <= e_hi, else min(|e_lo|, |e_hi|); G = max over the corners of l'0^2 + max over the corners of l'1^2
  // (l' = F^T (u, v, 1)); the row reaches the tile iff m^2 < radius^2 (g + G).
  // The kernel widens these bounds by an explicit rounding term, so that the argument does not depend on whether the
  // compiler contracts l0 u + l1 v + l2 into fused multiply-adds, here or in the gate.  With eps = 2^-50 (8 units in
  // the last place of a double rounded to nearest, unit u = 2^-53), the WIDENED RANGE of p s + q t + c over
  // s in [s0, s1], t in [t0, t1] is (mgec_range)
  //     a0 = p s0, a1 = p s1, b0 = q t0, b1 = q t1,  A = max(|a0|, |a1|) + max(|b0|, |b1|) + |c|,
  //     lo = min(a0, a1) + min(b0, b1) + c - 2 eps A,  hi = max(a0, a1) + max(b0, b1) + c + 2 eps A
  // (without the eps terms: the corner minimum and maximum), and the cull is
  //     [lo, hi]   the widened range of e = l0 u + l1 v + l2 over the box,   m  = max(lo, -hi, 0),
  //     [lo', hi'] that of l'0 = F00 u + F10 v + F20,                        M0 = max(|lo'|, |hi'|),  M1 likewise for l'1,
  //     G = (M0 M0 + M1 M1) (1 + 2^-40),   hit iff m m < r2 (g + G).
  // Never rejects a tile that holds a candidate of the gate AS THE DEVICE COMPUTES IT.  Let (s, t) = (u, v) be a pixel
  // of the tile, u0 <= u <= u1, v0 <= v <= v1 (the box is that of the tile's ACTUAL pixels), S = |p s| + |q t| + |c|.
  // (1) Any evaluation of p s + q t + c in doubles -- two rounded products and two rounded sums, or fused multiply-adds
  //     in either nesting -- rounds at most four times, each time a partial result of magnitude <= S (1 + u)^3: it lies
  //     within 4.1 u S of the exact value.  The cull's corner sums round as often and the -+ 2 eps A once more: before
  //     the widening they lie within 5.2 u S' of the exact corner minimum / maximum, S' the maximum of S over the box.
  //     The computed A is >= (1 - u)^3 S', so 2 eps A = 16 u A exceeds 4.1 u S + 5.2 u S'.
  // (2) The exact e at (u, v) lies between the exact corner minimum and maximum (linearity).  By (1) the gate's
  //     computed e_c lies in [lo, hi].  Hence |e_c| >= m >= 0, and the rounded product m m <= the rounded product
  //     e_c e_c (rounding is monotone).
  // (3) The same for l': the gate's computed |m0| <= M0, |m1| <= M1.  The gate's tg = m0 m0 + m1 m1, fused or not, is
  //     at most (m0^2 + m1^2) (1 + u)^2 <= (M0^2 + M1^2) (1 + u)^2; the computed M0 M0 + M1 M1 is at least
  //     (M0^2 + M1^2) (1 - u)^2, and the factor 1 + 2^-40 (one more rounding) lifts it above: G >= tg.
  // (4) g + G and r2 (g + G) are the gate's g + tg and r2 (g + tg) with a larger operand: a rounded sum and a rounded
  //     product by r2 > 0 (no contraction applies: no addition follows the product), monotone.  So the gate's
  //     e_c e_c < r2 (g + tg) implies m m <= e_c e_c < r2 (g + tg) <= r2 (g + G): the cull keeps the tile.
  // A row past the count or a non-finite F has g = -inf: r2 (g + G) is -inf or NaN and nothing compares below it, as in
  // the gate.  Nine zeros give m = 0, g = G = 0 and 0 < 0: no tile is visited.  The widening is 2^-49 of the line's own
  // terms, far inside the 1 +- 1e-9 on the radius that the tests' float64 restatement of the exact rule allows for.
  __device__ __forceinline__ Box box(const int4& b) const {
    const double u0 = (double)b.x, v0 = (double)b.y, u1 = (double)b.z, v1 = (double)b.w;
    double lo, hi;
    mgec_range(fm[0], fm[3], fm[6], u0, u1, v0, v1, lo, hi);             // l'0 over the box
    const double M0 = fmax(fabs(lo), fabs(hi));
    mgec_range(fm[1], fm[4], fm[7], u0, u1, v0, v1, lo, hi);             // l'1 over the box
    const double M1 = fmax(fabs(lo), fabs(hi));
    return Box{u0, v0, u1, v1, (M0 * M0 + M1 * M1) * MGEC_LIFT};
  }
  __device__ __forceinline__ bool reach(const Row& q, const Box& b) const {
    double lo, hi;
    mgec_range(q.l0, q.l1, q.l2, b.u0, b.u1, b.v0, b.v1, lo, hi);         // e over the box
    const double m = fmax(fmax(lo, -hi), 0.0);
    return m * m < r2 * (q.g + b.G);
  }
};

// match_guided_epipolar_kernel is NOT mg_strip<MgEpipolar>: built that way it computes the same bits but measured 0.3 - 0.8 %
// slower on the MI355X ("One tile, two gates"), so the plain epipolar strip stays the source of its own
// that it was, statement for statement mg_strip with MgEpipolar's row(), column() and pass() written out.  A change to the
// gate, to mg_tile or to mg_strip has to be repeated here; tests/test_gpu_match_epipolar_cells.py holds the two to the
// same bits.
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
          const float d2 = match_d2(qnr, tn[ni], acc[mi][ni][r]);
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

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_epipolar_cells_kernel(const MatchFramesArgs a, const MatchGuidedArgs g,
                                                                          const MatchCellsArgs c) {
  mgc_strip<MgEpipolar>(a, g, c);
}

}  // namespace fpc
