// Batched RANSAC essential matrices from MINIMAL samples (fpc_ransac_essential / fpc_essential_frames / fpc_essential_bank;
// the rule is stated in include/fpc.h and restated in float64 by tests/test_essential_ransac.py).  The calibrated model of
// the family ransac_parts.h was built for: five pairs determine the relative pose of two known cameras, a sixth picks the
// root, and the five-point problem is not degenerate on a plane, where every 8-point sample is.  This header holds the
// minimal solve -- the null space of the 5 x 9 system, the ten cubic constraints, their Gauss-Jordan reduction, B(z) and
// its determinant, the real roots by derivative interlacing, the sixth pair's choice -- and the refit on the essential
// manifold.  The pair records, their pack / gather kernels and the workspace are ransac_homography.h's; the fp32 Sampson
// count (FmModel::counts) and the fp64 inlier test (fm_inlier) are ransac_fundamental.h's; the decomposition is
// pose_epipolar.h's, the tangent basis refine_pose.h's; the sampler, the selection key, solve_lds and the score and refit
// skeletons are ransac_parts.h's.
//
//   essential_score_kernel  score_body at 64 hypotheses per workgroup.  The 10 x 20 fp64 system needs dynamic row indices
//                     (the pivoting), which in registers would become scratch, so it lives in LDS, struct-of-arrays
//                     (lanes doing the same step hit consecutive banks).  In one piece it is 100 KiB for 64 hypotheses: one
//                     workgroup, one wave, per CU.  It is reduced in two parts instead (columns 0 .. 3, then 4 .. 19 with
//                     the first part's row operations replayed from registers): sys[160][64], 80 KiB, two workgroups per
//                     CU and the same bits.  The 5 x 9 system occupies the same memory first, the root walk's break points
//                     afterwards, the staged pair chunk at the end.  The null-space basis, the polynomial expansion, B(z), det B and the walk's
//                     coefficients live in registers: every index is a constant once unrolled.
//   essential_refit_kernel  one workgroup per problem: one lane re-derives the best sample's E with the same device function
//                     (refit_head), then `refits` times one lane decomposes the current F (pose_decompose, candidate 0), all
//                     lanes accumulate the 20 sums of one Gauss-Newton step over the current inliers (hf_block_sum), one lane
//                     solves the 5 x 5 system (solve_lds) and forms the stepped F, and all lanes count its inliers: the step is
//                     kept only if it loses none.  Through refit_tail it writes F, E, the inlier count and the mask.
#pragma once
#include "refine_pose.h"

constexpr int ES_DRAWS = 32;            // draw budget of one sample: the 8-point's
constexpr int ES_SAMPLE = 6;            // five pairs for the solve, the sixth picks the root
constexpr int ES_THREADS = 64;          // hypotheses per workgroup of essential_score_kernel
constexpr int ES_SYS = 160;             // doubles of LDS per hypothesis: the 10 x 20 system without its first four columns
constexpr double ES_PIVOT5 = 1e-10;     // last pivot / first pivot of the 5 x 9 elimination below which a sample is degenerate
constexpr double ES_PIVOT10 = 1e-12;    // a Gauss-Jordan pivot at or below this share of the first one: degenerate
constexpr int ES_BISECT = 40;           // bisections of every bracket of the root walk
constexpr int ES_NEWTON = 3;            // guarded Newton steps behind them
constexpr int ES_DOUBLINGS = 64;        // trips of the search for the root bound
constexpr int ES_NSUM = 20;             // the refit's sums: J^T J (upper triangle, row-major: 15), J^T r (5)

struct EsArgs : HfArgs {
  float q_fx, q_fy, q_cx, q_cy;         // the query camera
  float t_fx, t_fy, t_cx, t_cy;         // the train camera
};

// ---- polynomials in (x, y, z, 1): variables 0 .. 3, a product's coefficient indexed by its sorted variable tuple ---------
// quadratic (i <= j): 00 01 02 03 11 12 13 22 23 33
__host__ __device__ constexpr int es_q(int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo * 4 - lo * (lo - 1) / 2 + (hi - lo);
}
// cubic: include/fpc.h's order  x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int es_c(int i, int j, int k) {
  int a = i, b = j, c = k, s = 0;
  if (a > b) { s = a; a = b; b = s; }
  if (b > c) { s = b; b = c; c = s; }
  if (a > b) { s = a; a = b; b = s; }
  const int code = a * 16 + b * 4 + c;
  constexpr int order[20] = {0, 21, 1, 5, 2, 3, 22, 23, 6, 7, 10, 11, 15, 26, 27, 31, 42, 43, 47, 63};
  for (int m = 0; m < 20; ++m)
    if (order[m] == code) return m;
  return -1;
}
static_assert(es_c(0, 0, 0) == 0 && es_c(1, 1, 1) == 1 && es_c(1, 0, 0) == 2 && es_c(2, 1, 0) == 8 && es_c(3, 1, 0) == 9 &&
              es_c(2, 0, 2) == 10 && es_c(3, 3, 0) == 12 && es_c(2, 2, 2) == 16 && es_c(3, 3, 3) == 19, "the monomial order");
static_assert(es_q(1, 1) == 4 && es_q(3, 1) == 6 && es_q(2, 2) == 7 && es_q(3, 3) == 9, "the quadratic order");

// index of the symmetric pair (i, j) of three: 00 01 02 11 12 22
__host__ __device__ constexpr int es_sym3(int i, int j) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo * 3 - lo * (lo - 1) / 2 + (hi - lo);
}

// q <- q +- a b (linear x linear), the products in the order i, j
template <bool SUB>
__device__ __forceinline__ void es_mul11(const double (&a)[4], const double (&b)[4], double (&q)[10]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) q[es_q(i, j)] = SUB ? q[es_q(i, j)] - a[i] * b[j] : q[es_q(i, j)] + a[i] * b[j];
}
// c <- c +- q a (quadratic x linear), the products in the order (i, j) of the quadratic, l
template <bool SUB>
__device__ __forceinline__ void es_mul21(const double (&q)[10], const double (&a)[4], double (&c)[20]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j)
#pragma unroll
      for (int l = 0; l < 4; ++l)
        c[es_c(i, j, l)] = SUB ? c[es_c(i, j, l)] - q[es_q(i, j)] * a[l] : c[es_c(i, j, l)] + q[es_q(i, j)] * a[l];
}
template <int N>
__device__ __forceinline__ void es_zero(double (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0.0;
}
// out <- out +- a b, polynomials in z (ascending powers), the products in the order i, j
template <bool SUB, int NA, int NB>
__device__ __forceinline__ void es_zmul(const double (&a)[NA], const double (&b)[NB], double (&out)[NA + NB - 1]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] = SUB ? out[i + j] - a[i] * b[j] : out[i + j] + a[i] * b[j];
}
// Horner from the leading coefficient down, every operation rounded
template <int N>
__device__ __forceinline__ double es_horner(const double (&c)[N], double z) {
#pragma clang fp contract(off)
  double v = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; --k) v = v * z + c[k];
  return v;
}
__host__ __device__ constexpr double es_falling(int i, int k) {          // (i + k)! / i!
  double v = 1.0;
  for (int m = i + 1; m <= i + k; ++m) v *= (double)m;
  return v;
}

// K_t^-T E K_q^-1
__device__ __forceinline__ void es_f_of_e(const double (&E)[9], const EsArgs& g, double (&F)[9]) {
#pragma clang fp contract(off)
  const double qfx = g.q_fx, qfy = g.q_fy, qcx = g.q_cx, qcy = g.q_cy, tfx = g.t_fx, tfy = g.t_fy, tcx = g.t_cx, tcy = g.t_cy;
  double G[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[i * 3] = E[i * 3] / qfx;
    G[i * 3 + 1] = E[i * 3 + 1] / qfy;
    G[i * 3 + 2] = E[i * 3 + 2] - (E[i * 3] * (qcx / qfx) + E[i * 3 + 1] * (qcy / qfy));
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = G[j] / tfx;
    F[3 + j] = G[3 + j] / tfy;
    F[6 + j] = G[6 + j] - ((tcx / tfx) * G[j] + (tcy / tfy) * G[3 + j]);
  }
}

// e and g = l0^2 + l1^2 + l'0^2 + l'1^2 of one pair under F, in fp64
__device__ __forceinline__ void es_sampson(const double (&F)[9], double x, double y, double u, double v, double& e, double& g) {
#pragma clang fp contract(off)
  const double l0 = F[0] * x + F[1] * y + F[2], l1 = F[3] * x + F[4] * y + F[5], l2 = F[6] * x + F[7] * y + F[8];
  e = u * l0 + v * l1 + l2;
  const double m0 = F[0] * u + F[3] * v + F[6], m1 = F[1] * u + F[4] * v + F[7];
  g = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
}

// The ten cubic constraints of the basis e (e[q][k]: entry q of E, basis vector k): row 0 det E, rows 1 .. 9 the entries of
// (E E^T - tr(E E^T) / 2 I) E, row-major.  HEAD: columns 0 .. 3 -> sys[(r * 4 + m) * S]; else columns 4 .. 19 ->
// sys[(r * 16 + m - 4) * S].  (Everything is unrolled: what a call does not store, it does not compute.)
template <int S, bool HEAD>
__device__ __forceinline__ void es_store_row(const double (&row)[20], int r, double* sys) {
#pragma unroll
  for (int m = 0; m < 20; ++m) {
    if (HEAD && m < 4) sys[(r * 4 + m) * S] = row[m];
    if (!HEAD && m >= 4) sys[(r * 16 + m - 4) * S] = row[m];
  }
}
template <int S, bool HEAD>
__device__ __forceinline__ void es_expand(const double (&e)[9][4], double* sys) {
#pragma clang fp contract(off)
  {
    double m0[10], m1[10], m2[10], row[20];
    es_zero(m0); es_zero(m1); es_zero(m2); es_zero(row);
    es_mul11<false>(e[4], e[8], m0); es_mul11<true>(e[5], e[7], m0);
    es_mul11<false>(e[3], e[8], m1); es_mul11<true>(e[5], e[6], m1);
    es_mul11<false>(e[3], e[7], m2); es_mul11<true>(e[4], e[6], m2);
    es_mul21<false>(m0, e[0], row); es_mul21<true>(m1, e[1], row); es_mul21<false>(m2, e[2], row);
    es_store_row<S, HEAD>(row, 0, sys);
  }
  double G[6][10];                               // E E^T - tr(E E^T) / 2 I: 00 01 02 11 12 22
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      double (&gq)[10] = G[es_sym3(i, j)];
      es_zero(gq);
      es_mul11<false>(e[i * 3], e[j * 3], gq); es_mul11<false>(e[i * 3 + 1], e[j * 3 + 1], gq);
      es_mul11<false>(e[i * 3 + 2], e[j * 3 + 2], gq);
    }
#pragma unroll
  for (int m = 0; m < 10; ++m) {
    const double tr = (G[0][m] + G[3][m]) + G[5][m];
    G[0][m] = G[0][m] - 0.5 * tr; G[3][m] = G[3][m] - 0.5 * tr; G[5][m] = G[5][m] - 0.5 * tr;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double row[20];
      es_zero(row);
      es_mul21<false>(G[es_sym3(i, 0)], e[j], row); es_mul21<false>(G[es_sym3(i, 1)], e[3 + j], row);
      es_mul21<false>(G[es_sym3(i, 2)], e[6 + j], row);
      es_store_row<S, HEAD>(row, 1 + i * 3 + j, sys);
    }
}

// One level of the root walk: P (degree D, ascending) over the break points brk[0 .. D] (LDS, stride S) -> nxt[1 .. D]; the
// caller has written nxt[0] and writes nxt[D + 1].  -> the intervals with a change of sign, bit j for interval j.
template <int S, int D>
__device__ __forceinline__ uint32_t es_level(const double (&c)[D + 1], const double* brk, double* nxt) {
#pragma clang fp contract(off)
  double dc[D];
#pragma unroll
  for (int i = 0; i < D; ++i) dc[i] = c[i + 1] * (double)(i + 1);
  uint32_t valid = 0;
#pragma unroll 1
  for (int j = 0; j < D; ++j) {
    double lo = brk[j * S], hi = brk[(j + 1) * S];
    const double top = hi;
    const bool plo = es_horner(c, lo) > 0.0, phi = es_horner(c, hi) > 0.0;
    const bool change = plo != phi;
#pragma unroll 1
    for (int b = 0; b < ES_BISECT; ++b) {
      const double mid = 0.5 * (lo + hi);
      const bool same = (es_horner(c, mid) > 0.0) == plo;
      lo = same ? mid : lo;
      hi = same ? hi : mid;
    }
    double r = 0.5 * (lo + hi);
#pragma unroll
    for (int s = 0; s < ES_NEWTON; ++s) {
      const double rn = r - es_horner(c, r) / es_horner(dc, r);
      r = (rn >= lo && rn <= hi) ? rn : r;
    }
    nxt[(j + 1) * S] = change ? r : top;
    valid |= change ? (1u << j) : 0u;
  }
  return valid;
}

template <int S, int D>
struct EsWalk {
  // levels D .. 10; brk holds level D's D + 1 break points
  static __device__ __forceinline__ uint32_t run(const double (&p)[11], double bound, double* brk, double* nxt) {
#pragma clang fp contract(off)
    double c[D + 1];
#pragma unroll
    for (int i = 0; i <= D; ++i) c[i] = p[i + 10 - D] * es_falling(i, 10 - D);
    nxt[0] = -bound;
    const uint32_t valid = es_level<S, D>(c, brk, nxt);
    nxt[(D + 1) * S] = bound;
    if constexpr (D == 10) return valid;
    else return EsWalk<S, D + 1>::run(p, bound, nxt, brk);
  }
};

// The minimal solve of include/fpc.h: six pairs -> E (normalised coordinates) and F = K_t^-T E K_q^-1, unscaled, in fp64.
// sys: this thread's ES_SYS doubles of LDS, element e at sys[e * S].  Contraction is off (here and in every helper) so that
// the score kernel and the refit kernel, which inline this at different strides, compute the same bits.  false: degenerate.
template <int S>
__device__ __forceinline__ bool es_solve5(double* sys, const float4* __restrict__ pairs, const uint32_t (&idx)[ES_SAMPLE],
                                          const EsArgs& g, double (&Eb)[9], double (&Fb)[9]) {
#pragma clang fp contract(off)
  const double qfx = g.q_fx, qfy = g.q_fy, qcx = g.q_cx, qcy = g.q_cy, tfx = g.t_fx, tfy = g.t_fy, tcx = g.t_cx, tcy = g.t_cy;
  // ---- the 5 x 9 system of rows q^ (x) p^ and its elimination with full pivoting (fm_solve8's, five rows) ----
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const float4 r = pairs[idx[i]];
    const double x = ((double)r.x - qcx) / qfx, y = ((double)r.y - qcy) / qfy;
    const double u = ((double)r.z - tcx) / tfx, v = ((double)r.w - tcy) / tfy;
    double* row = sys + (size_t)i * 9 * S;
    row[0] = u * x; row[S] = u * y; row[2 * S] = u; row[3 * S] = v * x; row[4 * S] = v * y; row[5 * S] = v;
    row[6 * S] = x; row[7 * S] = y; row[8 * S] = 1.0;
  }
  unsigned long long perm = 0x876543210ull;     // nibble c: the unknown that column c holds
  double first = 0.0, last = 0.0;
#pragma unroll 1
  for (int c = 0; c < 5; ++c) {
    double pv = -1.0;
    int pr = c, pc = c;
    for (int i = c; i < 5; ++i)
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
      for (int i = 0; i < 5; ++i) {
        const double tmp = sys[(i * 9 + c) * S];
        sys[(i * 9 + c) * S] = sys[(i * 9 + pc) * S];
        sys[(i * 9 + pc) * S] = tmp;
      }
      const unsigned long long nc = (perm >> (4 * c)) & 15ull, np = (perm >> (4 * pc)) & 15ull;
      perm = (perm & ~((15ull << (4 * c)) | (15ull << (4 * pc)))) | (np << (4 * c)) | (nc << (4 * pc));
    }
    const double piv = sys[(c * 9 + c) * S];
    for (int i = c + 1; i < 5; ++i) {
      const double fct = sys[(i * 9 + c) * S] / piv;
      for (int j = c + 1; j < 9; ++j) sys[(i * 9 + j) * S] = sys[(i * 9 + j) * S] - fct * sys[(c * 9 + j) * S];
    }
  }
  if (!(last >= ES_PIVOT5 * first)) return false;
  // ---- the four null vectors: free unknown k = 1, the other three 0; e[q][k]: entry q of E, basis vector k (X Y Z W) ----
  double e[9][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double yv[5];
#pragma unroll
    for (int i = 4; i >= 0; --i) {
      double acc = 0.0;
#pragma unroll
      for (int j = i + 1; j < 5; ++j) acc = acc + sys[(i * 9 + j) * S] * yv[j];
      acc = acc + sys[(i * 9 + 5 + k) * S];
      yv[i] = -acc / sys[(i * 9 + i) * S];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) e[q][k] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double yi = i < 5 ? yv[i < 5 ? i : 0] : (i == 5 + k ? 1.0 : 0.0);
      const int pi = (int)((perm >> (4 * i)) & 15ull);
#pragma unroll
      for (int q = 0; q < 9; ++q) e[q][k] = pi == q ? yi : e[q][k];
    }
  }
  // ---- the ten cubic constraints over the 20 monomials, and Gauss-Jordan on the left 10 x 10 block with row pivoting (ties:
  // the lowest row).  A step's row operations are decided by its own column alone and touch every later column alike, so
  // the system is reduced in two parts that never stand in LDS together -- 160 doubles instead of 200: columns 0 .. 3
  // first (10 x 4), whose four steps leave their pivot rows and factors in registers (constant indices: these steps are
  // unrolled); then columns 4 .. 19 (10 x 16), on which the four steps are replayed before steps 4 .. 9 run in place.
  // Every element sees the operations of the one-piece elimination in their order: the same bits.
  es_expand<S, true>(e, sys);
  double fac[4][10];
  int prow[4];
  double gfirst = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double pv = -1.0;
    int pr = c;
    for (int i = c; i < 10; ++i) {
      const double v = fabs(sys[(i * 4 + c) * S]);
      if (v > pv) { pv = v; pr = i; }
    }
    if (c == 0) gfirst = pv;
    if (!(pv > ES_PIVOT10 * gfirst)) return false;
    if (pr != c)
      for (int j = c; j < 4; ++j) {
        const double tmp = sys[(c * 4 + j) * S];
        sys[(c * 4 + j) * S] = sys[(pr * 4 + j) * S];
        sys[(pr * 4 + j) * S] = tmp;
      }
    prow[c] = pr;
#pragma unroll
    for (int i = 0; i < 10; ++i) fac[c][i] = sys[(i * 4 + c) * S];             // the pivot at i = c, the factors elsewhere
#pragma unroll
    for (int j = c + 1; j < 4; ++j) {
      sys[(c * 4 + j) * S] = sys[(c * 4 + j) * S] / fac[c][c];
#pragma unroll
      for (int i = 0; i < 10; ++i)
        if (i != c) sys[(i * 4 + j) * S] = sys[(i * 4 + j) * S] - fac[c][i] * sys[(c * 4 + j) * S];
    }
  }
  es_expand<S, false>(e, sys);                                                 // column m at index m - 4 of a row of 16
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int pr = prow[c];
    if (pr != c)
      for (int j = 0; j < 16; ++j) {
        const double tmp = sys[(c * 16 + j) * S];
        sys[(c * 16 + j) * S] = sys[(pr * 16 + j) * S];
        sys[(pr * 16 + j) * S] = tmp;
      }
#pragma unroll 1
    for (int j = 0; j < 16; ++j) {
      const double pj = sys[(c * 16 + j) * S] / fac[c][c];
      sys[(c * 16 + j) * S] = pj;
#pragma unroll
      for (int i = 0; i < 10; ++i)
        if (i != c) sys[(i * 16 + j) * S] = sys[(i * 16 + j) * S] - fac[c][i] * pj;
    }
  }
#pragma unroll 1
  for (int c = 4; c < 10; ++c) {
    double pv = -1.0;
    int pr = c;
    for (int i = c; i < 10; ++i) {
      const double v = fabs(sys[(i * 16 + c - 4) * S]);
      if (v > pv) { pv = v; pr = i; }
    }
    if (!(pv > ES_PIVOT10 * gfirst)) return false;
    if (pr != c)
      for (int j = c - 4; j < 16; ++j) {
        const double tmp = sys[(c * 16 + j) * S];
        sys[(c * 16 + j) * S] = sys[(pr * 16 + j) * S];
        sys[(pr * 16 + j) * S] = tmp;
      }
    const double piv = sys[(c * 16 + c - 4) * S];
    for (int j = c - 3; j < 16; ++j) sys[(c * 16 + j) * S] = sys[(c * 16 + j) * S] / piv;
    for (int i = 0; i < 10; ++i) {
      if (i == c) continue;
      const double fct = sys[(i * 16 + c - 4) * S];
      for (int j = c - 3; j < 16; ++j) sys[(i * 16 + j) * S] = sys[(i * 16 + j) * S] - fct * sys[(c * 16 + j) * S];
    }
  }
  // ---- B(z) from <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <xyz> - z <xy>: rows of (cubic, cubic, quartic) in z, ascending ----
  double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double ra[10], rb[10];
#pragma unroll
    for (int m = 0; m < 10; ++m) { ra[m] = sys[((4 + 2 * r) * 16 + 6 + m) * S]; rb[m] = sys[((5 + 2 * r) * 16 + 6 + m) * S]; }
    bx[r][0] = ra[2]; bx[r][1] = ra[1] - rb[2]; bx[r][2] = ra[0] - rb[1]; bx[r][3] = -rb[0];
    by[r][0] = ra[5]; by[r][1] = ra[4] - rb[5]; by[r][2] = ra[3] - rb[4]; by[r][3] = -rb[3];
    b1[r][0] = ra[9]; b1[r][1] = ra[8] - rb[9]; b1[r][2] = ra[7] - rb[8]; b1[r][3] = ra[6] - rb[7]; b1[r][4] = -rb[6];
  }
  double p[11];
  {
    double c0[8], c1[8], c2[7];
    es_zero(c0); es_zero(c1); es_zero(c2); es_zero(p);
    es_zmul<false>(by[1], b1[2], c0); es_zmul<true>(b1[1], by[2], c0);
    es_zmul<false>(bx[1], b1[2], c1); es_zmul<true>(b1[1], bx[2], c1);
    es_zmul<false>(bx[1], by[2], c2); es_zmul<true>(by[1], bx[2], c2);
    es_zmul<false>(bx[0], c0, p); es_zmul<true>(by[0], c1, p); es_zmul<false>(b1[0], c2, p);
  }
  // ---- the real roots of p by derivative interlacing inside a root bound (the systems' LDS holds the break points) ----
  // bound: the first power of two B with |p_10| B^10 > sum_(i < 10) |p_i| B^i (every root lies inside; within a factor 2 of
  // the root of Cauchy's polynomial, where 1 + max |p_i / p_10| can be 1e14 times too wide for the bisections)
  double ca[11];
#pragma unroll
  for (int i = 0; i < 10; ++i) ca[i] = -fabs(p[i]);
  ca[10] = fabs(p[10]);
  double bound = 1.0;
#pragma unroll 1
  for (int s = 0; s < ES_DOUBLINGS; ++s) bound = es_horner(ca, bound) > 0.0 ? bound : 2.0 * bound;
  if (!(es_horner(ca, bound) > 0.0)) return false;                            // (NaN, or roots beyond 2^64)
  double* const brk = sys;
  double* const nxt = sys + 16 * S;
  brk[0] = -bound; brk[S] = bound;
  const uint32_t valid = EsWalk<S, 1>::run(p, bound, brk, nxt);               // (level 10, an even one, ends in `brk`: entries 1 .. 10)
  // ---- every root: the null vector of B(z) -> E -> F; the sixth pair picks one ----
  const float4 r6 = pairs[idx[5]];
  const double x6 = r6.x, y6 = r6.y, u6 = r6.z, v6 = r6.w;
  bool have = false;
  double beste = 0.0;
#pragma unroll 1
  for (int j = 0; j < 10; ++j) {
    const double z = brk[(j + 1) * S];
    double bv[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) { bv[r][0] = es_horner(bx[r], z); bv[r][1] = es_horner(by[r], z); bv[r][2] = es_horner(b1[r], z); }
    const double n0 = bv[0][1] * bv[1][2] - bv[0][2] * bv[1][1];
    const double n1 = bv[0][2] * bv[1][0] - bv[0][0] * bv[1][2];
    const double n2 = bv[0][0] * bv[1][1] - bv[0][1] * bv[1][0];
    const double x = n0 / n2, y = n1 / n2;
    bool ok = ((valid >> j) & 1u) != 0 && fabs(x) < 1e300 && fabs(y) < 1e300;   // (a vanishing n2: Inf or NaN)
    double E[9], F[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) E[q] = ((x * e[q][0] + y * e[q][1]) + z * e[q][2]) + e[q][3];
    es_f_of_e(E, g, F);
    double r, gg;
    es_sampson(F, x6, y6, u6, v6, r, gg);
    const double err = (r * r) / gg;
    if (ok && err < 1e300 && (!have || err < beste)) {                       // ties keep the lower root
      have = true;
      beste = err;
#pragma unroll
      for (int q = 0; q < 9; ++q) { Eb[q] = E[q]; Fb[q] = F[q]; }
    }
  }
  return have;
}

// the hypothesis as it is scored: scaled to max |f| = 1, rounded to fp32.  false: not finite.
__device__ __forceinline__ bool es_hypothesis(const double (&F)[9], float (&F32)[9]) {
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
// score_body's Model: FmModel's nine registers, threshold, records and fp32 count; the sample and its solve are this header's
struct EsModel : FmModel {
  static constexpr int SAMPLE = ES_SAMPLE, DRAWS = ES_DRAWS, REC = 1;
  __device__ __forceinline__ explicit EsModel(const EsArgs& a) : FmModel(a) {}
  __device__ __forceinline__ bool solve(const EsArgs& a, const float4* __restrict__ pairs, const uint32_t (&idx)[ES_SAMPLE],
                                        double* sys) {
    double E[9], Fd[9];
    float F32[9];
    if (!(es_solve5<ES_THREADS>(sys + threadIdx.x, pairs, idx, a, E, Fd) && es_hypothesis(Fd, F32))) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = F32[i];
    return true;
  }
};

__global__ __launch_bounds__(ES_THREADS) void essential_score_kernel(EsArgs a) {
  __shared__ double sys[ES_SYS * ES_THREADS];                // the systems; afterwards the staged pair chunk
  static_assert(sizeof(double) * ES_SYS * ES_THREADS >= sizeof(float4) * HF_CHUNK, "the pair chunk reuses the systems' LDS");
  score_body<ES_THREADS, EsModel>(a, reinterpret_cast<float4*>(sys), sys);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// M (9 doubles) -> Frobenius norm 1, rounded to fp32, the element of largest magnitude of the ROUNDED values positive
// (ties: the lowest index); out (LDS) gets the fp32 values as doubles.  false: not finite.  (fm_finish without the
// denormalisation.)
__device__ __forceinline__ bool es_unit(const double (&Min)[9], double* out) {
  double F[9];
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) q += Min[i] * Min[i];
  const double nrm = sqrt(q);
  if (!(nrm > 0.0) || !(nrm < 1e300)) return false;
  bool finite = true;
  float mxv = 0.f, mxa = -1.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = Min[i] / nrm;
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

// K_t^-T [t]x R K_q^-1
__device__ __forceinline__ void es_f_of_pose(const double (&R)[9], const double (&t)[3], const EsArgs& g, double (&F)[9]) {
#pragma clang fp contract(off)
  double E[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
  es_f_of_e(E, g, F);
}

__global__ __launch_bounds__(256) void essential_refit_kernel(EsArgs a, float* __restrict__ Fout, float* __restrict__ Eout,
                                                              int32_t* __restrict__ ninl, uint8_t* mask, int mstride) {
  __shared__ double red[4 * ES_NSUM];
  __shared__ double sys[ES_SYS];
  __shared__ double jm[9], jv[9], cand[21];
  __shared__ double s20[ES_NSUM];
  __shared__ double sm[5][6];
  __shared__ double fw[9], fnew[9], enew[9];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const double thr2 = (double)a.thr * (double)a.thr;
  const PoseArgs cams{a.q_fx, a.q_fy, a.q_cx, a.q_cy, a.t_fx, a.t_fy, a.t_cx, a.t_cy, 0};
  const double qfx = a.q_fx, qfy = a.q_fy, qcx = a.q_cx, qcy = a.q_cy, tfx = a.t_fx, tfy = a.t_fy, tcx = a.t_cx, tcy = a.t_cy;
  double F[9];
  bool ok = refit_head(M >= ES_SAMPLE && key != 0ull, &solved, [&]() {
    uint32_t idx[ES_SAMPLE];
    double E[9], Fd[9];
    if (!(hf_sample_distinct<ES_SAMPLE, ES_DRAWS>(a.seed, (uint32_t)hf_frame(a.per_frame, f), ~(uint32_t)key, (uint32_t)M, idx) &&
          es_solve5<1>(sys, pairs, idx, a, E, Fd)))
      return false;
    return es_unit(Fd, fnew);
  });
  if (ok) {
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = fnew[i];
    double c1[1] = {0.0};
    for (int k = tid; k < M; k += 256) c1[0] += fm_inlier(F, pairs[k], thr2) ? 1.0 : 0.0;
    hf_block_sum<1>(c1, red);
    double have = c1[0];                                                    // the inliers of the current F
    for (int r = 0; r < a.refits; ++r) {
      if (have < (double)ES_SAMPLE) break;
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) fw[i] = F[i];
        solved = pose_decompose(fw, cams, jm, jv, cand) ? 1 : 0;
      }
      __syncthreads();
      if (!solved) break;
      double R[9], t[3], B[6], Fu[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = cand[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = cand[18 + i];
      rp_basis(t[0], t[1], t[2], B);
      es_f_of_pose(R, t, a, Fu);
      double s[ES_NSUM];
      es_zero(s);
      for (int k = tid; k < M; k += 256) {
        const float4 p = pairs[k];
        if (!fm_inlier(F, p, thr2)) continue;
        double e, g;
        es_sampson(Fu, (double)p.x, (double)p.y, (double)p.z, (double)p.w, e, g);
        const double sg = sqrt(g), res = e / sg;
        const double ph[3] = {((double)p.x - qcx) / qfx, ((double)p.y - qcy) / qfy, 1.0};
        const double qh[3] = {((double)p.z - tcx) / tfx, ((double)p.w - tcy) / tfy, 1.0};
        const double a0 = R[0] * ph[0] + R[1] * ph[1] + R[2] * ph[2], a1 = R[3] * ph[0] + R[4] * ph[1] + R[5] * ph[2],
                     a2 = R[6] * ph[0] + R[7] * ph[1] + R[8] * ph[2];
        const double c0 = t[1] * a2 - t[2] * a1, c1v = t[2] * a0 - t[0] * a2, c2 = t[0] * a1 - t[1] * a0;      // t x a
        const double w0 = a1 * qh[2] - a2 * qh[1], w1 = a2 * qh[0] - a0 * qh[2], w2 = a0 * qh[1] - a1 * qh[0];  // a x q^
        double J[5];
        J[0] = (c1v * qh[2] - c2 * qh[1]) / sg;                                // (t x a) x q^
        J[1] = (c2 * qh[0] - c0 * qh[2]) / sg;
        J[2] = (c0 * qh[1] - c1v * qh[0]) / sg;
        J[3] = (w0 * B[0] + w1 * B[1] + w2 * B[2]) / sg;
        J[4] = (w0 * B[3] + w1 * B[4] + w2 * B[5]) / sg;
        int q = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
#pragma unroll
          for (int j = i; j < 5; ++j) s[q++] += J[i] * J[j];
          s[15 + i] += J[i] * res;
        }
      }
      hf_block_sum<ES_NSUM>(s, red);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < ES_NSUM; ++i) s20[i] = s[i];                     // (through LDS: s[dynamic] would be scratch)
        int q = 0;
        double dmax = 0.0;
        for (int i = 0; i < 5; ++i) {
          for (int j = i; j < 5; ++j) { sm[i][j] = s20[q]; sm[j][i] = s20[q]; ++q; }
          sm[i][5] = -s20[15 + i];
          dmax = fmax(dmax, sm[i][i]);
        }
        int good = solve_lds<5>(sm, RP_SINGULAR * dmax) ? 1 : 0;
        if (good) {
          // R' = Q R with Q the rotation of the unit quaternion (1, omega / 2) / |.|;  t' = (Q t + B eta) / |.|
          const double h0 = 0.5 * sm[0][5], h1 = 0.5 * sm[1][5], h2 = 0.5 * sm[2][5], eta0 = sm[3][5], eta1 = sm[4][5];
          const double nq = sqrt(1.0 + (h0 * h0 + h1 * h1 + h2 * h2));
          const double w = 1.0 / nq, v0 = h0 / nq, v1 = h1 / nq, v2 = h2 / nq;
          const double Q[9] = {1.0 - 2.0 * (v1 * v1 + v2 * v2), 2.0 * (v0 * v1 - w * v2), 2.0 * (v0 * v2 + w * v1),
                               2.0 * (v0 * v1 + w * v2), 1.0 - 2.0 * (v0 * v0 + v2 * v2), 2.0 * (v1 * v2 - w * v0),
                               2.0 * (v0 * v2 - w * v1), 2.0 * (v1 * v2 + w * v0), 1.0 - 2.0 * (v0 * v0 + v1 * v1)};
          double Rn[9], tn[3], Fn[9];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = Q[i * 3] * R[j] + Q[i * 3 + 1] * R[3 + j] + Q[i * 3 + 2] * R[6 + j];
            tn[i] = (Q[i * 3] * t[0] + Q[i * 3 + 1] * t[1] + Q[i * 3 + 2] * t[2]) + (B[i] * eta0 + B[3 + i] * eta1);
          }
          const double nt = sqrt(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
          if (!(nt > RP_TMIN)) good = 0;                                     // (false for NaN)
          else {
#pragma unroll
            for (int i = 0; i < 3; ++i) tn[i] = tn[i] / nt;
            es_f_of_pose(Rn, tn, a, Fn);
            good = es_unit(Fn, fnew) ? 1 : 0;
          }
        }
        solved = good;
      }
      __syncthreads();
      if (!solved) break;                                                   // a singular system keeps the previous F
      double Fn[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) Fn[i] = fnew[i];
      double c2[1] = {0.0};
      for (int k = tid; k < M; k += 256) c2[0] += fm_inlier(Fn, pairs[k], thr2) ? 1.0 : 0.0;
      hf_block_sum<1>(c2, red);
      if (c2[0] < have) break;                                               // the monotone guard: a step that loses an inlier ends the refits
      have = c2[0];
#pragma unroll
      for (int i = 0; i < 9; ++i) F[i] = Fn[i];
    }
  }
  ok = refit_tail(ok, M, a.min_inliers, red, mask, ninl + f, [&](int k) { return fm_inlier(F, pairs[k], thr2); },
                  [&](int k) { return (size_t)f * mstride + a.row[(size_t)f * a.cap + k]; });
  if (tid == 0) {                                                           // (through LDS: F[tid] would be scratch)
    // E_dev: K_t^T F K_q of the returned F, unit norm, the same sign rule
    double G[9], E[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      G[i * 3 + 0] = F[i * 3 + 0] * qfx;
      G[i * 3 + 1] = F[i * 3 + 1] * qfy;
      G[i * 3 + 2] = F[i * 3 + 0] * qcx + F[i * 3 + 1] * qcy + F[i * 3 + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      E[j] = tfx * G[j];
      E[3 + j] = tfy * G[3 + j];
      E[6 + j] = tcx * G[j] + tcy * G[3 + j] + G[6 + j];
    }
    const bool eok = ok && es_unit(E, enew);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      fnew[i] = ok ? F[i] : 0.0;
      if (!eok) enew[i] = 0.0;
    }
  }
  __syncthreads();
  if (tid < 9) {
    Fout[f * 9 + tid] = (float)fnew[tid];
    if (Eout) Eout[f * 9 + tid] = (float)enew[tid];
  }
}
