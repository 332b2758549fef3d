// match_guided.h -- fpc_match_frames / the bank's table pass once more, under a homography per frame as a spatial gate
// (fpc_match_frames_guided / fpc_match_bank_guided, include/fpc.h), and the parts every guided strip kernel is built from.
//
// Query sets, train sets, counts and tables are fpc_match_frames' own (mf_sets, match_frames.h); the norms are
// mf_norms_kernel's / the bank's.  Train row j at pixel (u, v) is a CANDIDATE of query row i at pixel (x, y) iff, in fp64
// from the fp32 H of the frame,
//     w = H6 x + H7 y + H8 > 0   and   (H0 x + H1 y + H2 - w u)^2 + (H3 x + H4 y + H5 - w v)^2 < radius^2 w^2
// (no division), and the result is fpc_match_frames' rule over the candidates only.
//
// The strip kernels -- match_guided_kernel here, match_guided_cells_kernel (match_guided_cells.h) and
// match_guided_epipolar_cells_kernel (match_guided_epipolar.h; the plain epipolar strip there is written out on its own)
// -- are a skeleton instantiated with a gate:
//   a GATE (MgHomography here, MgEpipolar in match_guided_epipolar.h) decides which pairs are candidates.  It is given four
//                          double[64] LDS arrays of the skeleton (in ascending LDS order: each gate keeps the layout
//                          its kernel had), one value per query row of the strip, filled once by row(); column()
//                          keeps what it needs of a train pixel, pass() is the pair test, box() / reach() the tile cull
//                          of the ordered skeleton.  The plain skeleton asks the gate for the train side it reads
//                          (train(): these two take the train pixels, mg_train_xy; MgPose of match_guided_pose.h takes
//                          the train set's landmarks) and is templated on the gate's argument struct for that.
//   mg_pass_mask           a lane's 64 pairs of the MFMA C/D layout (2 train columns x 32 query rows) as a 64-bit mask.
//   mg_tile                mf_strip's tile behind that mask -- the same 2 x 2 v_mfma_f32_32x32x2_f32 blocks, K order, d^2
//                          expression and clamp, so a candidate pair's d^2 has fpc_match_frames' bits -- with the pairs
//                          that fail the gate written as +inf, which neither the top-2 scan nor the column minimum
//                          (strict <) ever picks.
//   mg_merge               the four waves' top-2 lists into the row's two keys.
//   mg_strip               the PLAIN skeleton, mf_strip with the gate: one workgroup owns a 64-row strip of one frame,
//                          its four waves take the train tiles w, w+4, ...  A tile without a single passing pair in the
//                          wave is skipped before any descriptor load or MFMA.  Columns ascend with the train index, so
//                          the scans go by value, ascending index and strict <.  (The ORDERED skeleton, mgc_strip, is
//                          match_guided_cells.h's; its selection differs because its columns do not ascend.)
//   match_guided_kernel    mg_strip<MgHomography>.
//   match_guided_finalize_kernel   mf_row_ok on the gated top-2; a row without a candidate -> -1 / +inf.
#pragma once
#include "match_frames.h"

namespace fpc {

struct MatchGuidedArgs {
  const float* H;               // [n][9] row-major, query pixel -> train pixel
  const int32_t* xy;            // [B][cap][2]  fpc_results().xy
  const int32_t* key_xy;        // [nkey][2]; with MatchFramesArgs::key_slot the bank's xy [slots][bank_rows][2]
  double r2;                    // radius^2
};

// frame f's train coordinates: mf_sets' choice of the train set, for the pixels (null where that set is empty)
__device__ __forceinline__ const int32_t* mg_train_xy(const MatchFramesArgs& a, const MatchGuidedArgs& g, int f) {
  if (a.pairing == 1 && f > 0) return g.xy + (size_t)(f - 1) * a.cap * 2;
  if (a.key_slot) {
    const int sl = a.key_slot[f];
    return (sl >= 0 && sl < a.bank_slots) ? g.key_xy + (size_t)sl * a.bank_rows * 2 : nullptr;
  }
  return g.key_xy;
}

// The homography gate.  The strip's 64 query pixels are projected once, in fp64, into LDS (px, py, w, rw = radius^2 w^2;
// a row past the count, w <= 0 or a non-finite H gets a bound of -1 and passes nowhere).  H stays in the 64 lanes that run
// row(); there is no per-column term.
struct MgHomography {
  struct Row { double px, py, w, rw; };         // a query row of the strip, projected
  struct Col { double u, v; };                  // a train pixel
  struct Box { double u0, v0, u1, v1; };        // a tile's pixel box
  const MatchGuidedArgs& g;
  const int f;
  double *s_px, *s_py, *s_w, *s_rw;             // LDS, [64] each
  typedef const int32_t* Train;                 // what column() reads of frame f's train set: its pixels
  static __device__ __forceinline__ Train train(const MatchFramesArgs& a, const MatchGuidedArgs& g, int f) {
    return mg_train_xy(a, g, f);
  }

  __device__ __forceinline__ MgHomography(const MatchGuidedArgs& g, int f, double* l0, double* l1, double* l2, double* l3)
      : g(g), f(f), s_px(l1), s_py(l2), s_w(l0), s_rw(l3) {}

  // row i of the strip is row qi of the frame's pixels xy; live: it is below the frame's count
  __device__ __forceinline__ void row(int i, const int32_t* xy, int qi, bool live) const {
    const float* Hf = g.H + (size_t)f * 9;
    double h[9];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      h[k] = (double)Hf[k];
      finite = finite && fabs(h[k]) <= 3.5e38;               // (false for NaN and Inf)
    }
    const double x = (double)xy[2 * qi], y = (double)xy[2 * qi + 1];
    const double w = h[6] * x + h[7] * y + h[8];
    s_px[i] = h[0] * x + h[1] * y + h[2];
    s_py[i] = h[3] * x + h[4] * y + h[5];
    s_w[i] = w;
    s_rw[i] = (finite && live && w > 0.0) ? g.r2 * w * w : -1.0;
  }
  __device__ __forceinline__ Row line(int i) const { return Row{s_px[i], s_py[i], s_w[i], s_rw[i]}; }
  __device__ __forceinline__ Col column(const int32_t* xy, int tj) const {
    return Col{(double)xy[2 * tj], (double)xy[2 * tj + 1]};
  }
  __device__ __forceinline__ bool pass(const Row& q, const Col& c) const {
    const double ex = q.px - q.w * c.u, ey = q.py - q.w * c.v;
    return ex * ex + ey * ey < q.rw;
  }

  // Cull.  Row i (px, py, w, rw = radius^2 w^2 of the prologue, rw = -1 where the row passes nowhere) can have a
  // candidate in a tile with box [u0, u1] x [v0, v1] only if
  //     dx = max(px - w u1, -(px - w u0), 0),  dy likewise,  dx dx + dy dy < rw.
  // Never rejects a tile that holds a candidate: for a pair of the tile the gate computes ex = px - w u with
  // u0 <= u <= u1 and w > 0.  A rounded product and a rounded difference (and a fused multiply-add, should the compiler
  // contract px - w u, which it then does here as well: the expression is the same) are monotone in each operand, so
  // px - w u1 <= ex <= px - w u0 holds for the COMPUTED values, hence dx <= |ex| and dy <= |ey| exactly; squares of
  // non-negative numbers, their rounded sum (or fma(dx, dx, dy dy), the same form as the gate's) are monotone again, so
  // the computed dx dx + dy dy <= the computed ex ex + ey ey < rw.
  __device__ __forceinline__ Box box(const int4& b) const { return Box{(double)b.x, (double)b.y, (double)b.z, (double)b.w}; }
  __device__ __forceinline__ bool reach(const Row& q, const Box& b) const {
    const double ax = q.px - q.w * b.u1, bx = q.px - q.w * b.u0, ay = q.py - q.w * b.v1, by = q.py - q.w * b.v0;
    const double dx = fmax(fmax(ax, -bx), 0.0), dy = fmax(fmax(ay, -by), 0.0);
    return dx * dx + dy * dy < q.rw;
  }
};

// The gate in the C/D layout of mg_tile: bit (mi * 16 + r) * 2 + ni of the result is the pair of query row
// mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half and this lane's train column ni (tin: the column is below the count).
template <class Gate>
__device__ __forceinline__ unsigned long long mg_pass_mask(const Gate& gate, const typename Gate::Col (&col)[2],
                                                           const bool (&tin)[2], int half) {
  unsigned long long pass = 0ull;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const typename Gate::Row q = gate.line(mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        if (tin[ni] && gate.pass(q, col[ni])) pass |= 1ull << ((mi * 16 + r) * 2 + ni);
    }
  return pass;
}

// One wave's 64 x 64 tile: d^2 of the rows qrow (norms s_qn, LDS) against the columns trow (norms tn) into `tile`, +inf
// where `pass` has no bit.  Returns once the tile is written: it is private to the wave.
__device__ __forceinline__ void mg_tile(const float* const (&qrow)[2], const float* const (&trow)[2], const float (&tn)[2],
                                        const float* s_qn, unsigned long long pass, float* tile, int K8, int half, int l31) {
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
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Strip row `tid`: top-2 of the four waves' lists on (d^2 bits, index) -- keys are distinct, the result is order-free --
// to row `row` of the frame's table.
__device__ __forceinline__ void mg_merge(const unsigned long long (*s_top)[64][2], int tid, unsigned long long* top2, int row) {
  unsigned long long m1 = ~0ull, m2 = ~0ull;
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned long long v = s_top[w][tid][k];
      if (v < m1) { m2 = m1; m1 = v; }
      else if (v < m2) m2 = v;
    }
  unsigned long long* o = top2 + (size_t)row * 2;
  o[0] = m1;
  o[1] = m2;
}

// The plain skeleton: one workgroup (256 threads), the 64-row strip blockIdx.x of frame blockIdx.y.  GArgs: the gate's
// arguments, with the frames' pixels in `xy`.
template <class Gate, class GArgs = MatchGuidedArgs>
__device__ __forceinline__ void mg_strip(const MatchFramesArgs& a, const GArgs& g) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_gate0[64], s_gate1[64], s_gate2[64], s_gate3[64];    // the gate's four values per row of the strip
  const int f = blockIdx.y, q0 = blockIdx.x * MF_ROWS;
  const MfSets s = mf_sets(a, f);
  if (q0 >= s.nq || s.nt == 0) return;       // (the finalize kernel reads nq / nt itself)
  const typename Gate::Train txy = Gate::train(a, g, f);
  const int32_t* qxy = g.xy + (size_t)f * a.cap * 2;
  unsigned long long* top2 = a.top2 + (size_t)f * a.cap * 2;
  unsigned long long* colbest = a.colbest + (size_t)f * a.cap;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const Gate gate(g, f, s_gate0, s_gate1, s_gate2, s_gate3);
  if (tid < 64) {
    const int qi = min(q0 + tid, s.nq - 1);
    s_qn[tid] = s.qn[qi];
    gate.row(tid, qxy, qi, q0 + tid < s.nq);
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
    typename Gate::Col col[2];
    bool tin[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tj = min(t0 + i * 32 + l31, s.nt - 1);
      trow[i] = s.t + (size_t)tj * a.D + half * 4;
      tn[i] = s.tn[tj];
      col[i] = gate.column(txy, tj);
      tin[i] = t0 + i * 32 + l31 < s.nt;
    }
    const unsigned long long pass = mg_pass_mask(gate, col, tin, half);
    if (__ballot(pass != 0ull) == 0ull) continue;            // no candidate in this tile: no loads, no MFMAs
    mg_tile(qrow, trow, tn, s_qn, pass, tile, K8, half, l31);
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
  if (tid < MF_ROWS && q0 + tid < s.nq) mg_merge(s_top, tid, top2, q0 + tid);
}

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_kernel(const MatchFramesArgs a, const MatchGuidedArgs g) {
  mg_strip<MgHomography>(a, g);
}

// grid (ceil(cap / 256), n): match_frames_finalize_kernel, plus the row that no train row passed the gate for
__global__ __launch_bounds__(256) void match_guided_finalize_kernel(const MatchFramesArgs a, float max_dist, float ratio,
                                                                    int32_t* match, float* dist) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cap) return;
  const MfSets s = mf_sets(a, f);
  const size_t o = (size_t)f * a.cap + i;
  const unsigned long long k1 = (i < s.nq && s.nt > 0) ? a.top2[2 * o] : ~0ull;
  if (k1 == ~0ull) {
    match[o] = -1;
    if (dist) dist[o] = INFINITY;
    return;
  }
  float d;
  const bool ok = mf_row_ok(k1, a.top2[2 * o + 1], i, a.cross_check ? a.colbest + (size_t)f * a.cap : nullptr, max_dist,
                            ratio, d);
  match[o] = ok ? (int)(k1 & 0xffffffffu) : -1;
  if (dist) dist[o] = d;
}

}  // namespace fpc
