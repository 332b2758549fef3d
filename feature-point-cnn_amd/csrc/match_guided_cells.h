// match_guided_cells.h -- guided matching over a spatial order of the rows: a strip visits only the train tiles its
// projected pixels can reach (fpc_cell_order / fpc_match_frames_guided_cells / fpc_match_bank_guided_cells, include/fpc.h).
//
// match_guided_kernel (match_guided.h) evaluates the gate against every 64 x 64 tile; rows come in confidence order, so a
// tile's rows lie anywhere in the image and hardly a tile is without a candidate.  Here both sides are read through a
// permutation that sorts their rows by 32-px cell, every run of 64 ordered rows carries the bounding box of its pixels, and
// a strip tests the boxes before it touches a tile.  The result of a guided match is a function of the candidate set and
// of each candidate pair's d^2 bits alone (nearest and second nearest: the two smallest (d^2 bits, index) keys; column
// minimum: the smallest key), so the order rows are visited in does not show: the output is match_guided_kernel's, bit for
// bit, ties included.
//
//   cell_order_kernel      one workgroup per point set.  cell = cy * CX + cx with cx = clamp(x >> shift, 0, CX - 1), cy
//                          likewise (arithmetic shift; shift = 5 wherever the order is public).  An LDS histogram over the
//                          cells, an exclusive prefix sum, then the rows in chunks of 256 in ascending order: a row's rank
//                          among the rows of its cell in its wave comes from one ballot per bit of the cell number, the four
//                          waves of a chunk add their groups to the running cell offsets one after the other.  No atomic
//                          decides a position: perm is the stable order by cell, ascending (cell, row), on every call.
//                          Then one wave per run of 64 ordered rows: the box [umin, vmin, umax, vmax] of its ACTUAL pixels.
//   match_guided_cells_kernel   match_guided_kernel with both sides read through their permutation: a workgroup owns 64
//                          consecutive ORDERED query rows, a tile is 64 consecutive ORDERED train rows; row pointers are
//                          base + perm[..] * D (rows are 512 B / 1 KB: no descriptor is copied), norms and pixels are read
//                          at the original index.
//       Cull.  Row i (px, py, w, rw = radius^2 w^2 of the prologue, rw = -1 where the row passes nowhere) can have a
//       candidate in a tile with box [u0, u1] x [v0, v1] only if
//           dx = max(px - w u1, -(px - w u0), 0),  dy likewise,  dx dx + dy dy < rw.
//       Never rejects a tile that holds a candidate: for a pair of the tile the gate computes ex = px - w u with
//       u0 <= u <= u1 and w > 0.  A rounded product and a rounded difference (and a fused multiply-add, should the compiler
//       contract px - w u, which it then does here as well: the expression is the same) are monotone in each operand, so
//       px - w u1 <= ex <= px - w u0 holds for the COMPUTED values, hence dx <= |ex| and dy <= |ey| exactly; squares of
//       non-negative numbers, their rounded sum (or fma(dx, dx, dy dy), the same form as the gate's) are monotone again, so
//       the computed dx dx + dy dy <= the computed ex ex + ey ey < rw.
//       The surviving tiles go into an LDS list in ascending tile order (ballots and per-wave counts, no atomics); the four
//       waves take list entries w, w + 4, ..., so they stay balanced after the cull.
//       A surviving tile is match_guided_kernel's: per-pair gate mask, per-wave skip, 2 x 2 v_mfma_f32_32x32x2_f32 blocks,
//       K order, |q|^2 + |t|^2 - 2 q.t, clamp; pairs that fail the gate are +inf and an entry is taken only if < +inf.
//       Selection.  Columns no longer ascend with the train index, so both scans order entries by their 64-bit key:
//       (d^2 bits << 32) | ORIGINAL train index for the top-2, (d^2 bits << 32) | ORIGINAL query index for the column
//       minimum.  top2 goes to the ORIGINAL query row, atomicMin to colbest of the ORIGINAL train row, and
//       match_guided_finalize_kernel / mf_row_ok run unchanged behind it.
#pragma once
#include "match_guided.h"

namespace fpc {

constexpr int MGC_MAX_CELLS = 16384;   // cells of the LDS histogram (64 KB): 32-px cells of a frame of up to 16.7 MPx
constexpr int MGC_LIST = 1024;         // surviving tiles listed per pass over the train tiles

struct CellOrderArgs {
  const int32_t* xy;      // set s: xy + src(s) * stride * 2
  const int32_t* n;       // count of set s: n[src(s)], clamped to [0, stride]
  const int32_t* slot;    // null: src(s) = s.  Else src(s) = slot[s], outside [0, nslots): an empty set
  int nslots;
  int stride;             // rows between two source sets
  int out_stride;         // rows between two perm rows (>= stride)
  int CX, CY, shift;
  int32_t* perm;          // [sets][out_stride]
  int4* box;              // [sets][box_stride] or null
  int box_stride;
};

__device__ __forceinline__ int mgc_cell(int x, int y, int CX, int CY, int shift) {
  const int cx = min(max(x >> shift, 0), CX - 1), cy = min(max(y >> shift, 0), CY - 1);
  return cy * CX + cx;
}

// grid (sets), 256 threads
__global__ __launch_bounds__(256) void cell_order_kernel(const CellOrderArgs a) {
  __shared__ int s_hist[MGC_MAX_CELLS];
  __shared__ int s_part[256];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int src = s;
  bool in = true;
  if (a.slot) {
    src = a.slot[s];
    in = src >= 0 && src < a.nslots;
  }
  const int cnt = in ? mf_clamp(a.n[src], a.stride) : 0;
  if (cnt == 0) return;
  const int32_t* xy = a.xy + (size_t)src * a.stride * 2;
  int32_t* perm = a.perm + (size_t)s * a.out_stride;
  const int cells = a.CX * a.CY;
  for (int c = tid; c < cells; c += 256) s_hist[c] = 0;
  __syncthreads();
  for (int i = tid; i < cnt; i += 256) atomicAdd(&s_hist[mgc_cell(xy[2 * i], xy[2 * i + 1], a.CX, a.CY, a.shift)], 1);
  __syncthreads();
  // exclusive prefix sum: thread t owns cells [t * per, (t + 1) * per)
  const int per = (cells + 255) / 256;
  const int c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
  int sum = 0;
  for (int c = c0; c < c1; ++c) sum += s_hist[c];
  s_part[tid] = sum;
  __syncthreads();
  if (tid < 64) {         // one wave scans the 256 partial sums, four per lane
    int v[4], t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = s_part[tid * 4 + k];
      t += v[k];
    }
    int incl = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    int run = incl - t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s_part[tid * 4 + k] = run;
      run += v[k];
    }
  }
  __syncthreads();
  {
    int run = s_part[tid];
    for (int c = c0; c < c1; ++c) {
      const int h = s_hist[c];
      s_hist[c] = run;
      run += h;
    }
  }
  __syncthreads();
  int nbits = 0;
  while ((1 << nbits) < cells) ++nbits;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < cnt; base += 256) {
    const int i = base + tid;
    const bool live = i < cnt;
    const int cell = live ? mgc_cell(xy[2 * i], xy[2 * i + 1], a.CX, a.CY, a.shift) : 0;
    // the lanes of this wave in the same cell
    unsigned long long same = __ballot(live);
    for (int b = 0; b < nbits; ++b) {
      const unsigned long long set = __ballot((cell >> b) & 1);
      same &= ((cell >> b) & 1) ? set : ~set;
    }
    const int rank = __popcll(same & below), group = __popcll(same);
    for (int w = 0; w < 4; ++w) {          // waves in row order: each adds its groups to the running offsets
      if (wave == w && live) {
        const int at = s_hist[cell];       // (every lane of the group reads before its first lane writes: one wave)
        if (rank == 0) s_hist[cell] = at + group;
        perm[at + rank] = i;
      }
      __syncthreads();
    }
  }
  if (!a.box) return;
  __syncthreads();                          // (the barrier above waits for this workgroup's stores to perm as well)
  int4* box = a.box + (size_t)s * a.box_stride;
  for (int r = wave; r * 64 < cnt; r += 4) {
    const int p = r * 64 + lane;
    int u0 = INT_MAX, v0 = INT_MAX, u1 = INT_MIN, v1 = INT_MIN;
    if (p < cnt) {
      const int i = perm[p];
      u0 = u1 = xy[2 * i];
      v0 = v1 = xy[2 * i + 1];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      u0 = min(u0, __shfl_xor(u0, d));
      v0 = min(v0, __shfl_xor(v0, d));
      u1 = max(u1, __shfl_xor(u1, d));
      v1 = max(v1, __shfl_xor(v1, d));
    }
    if (lane == 0) box[r] = make_int4(u0, v0, u1, v1);
  }
}

struct MatchCellsArgs {
  const int32_t* perm_q;   // [n][cap]   the frames' orders
  const int4* box_q;       // [n][nbox]  (unused by the kernel: the train side of FPC_PAIR_PREVIOUS)
  const int32_t* perm_t;   // the key's order [cap], or with MatchFramesArgs::key_slot one per frame [n][cap]
  const int4* box_t;       // [nbox] / [n][nbox]
  int nbox;                // ceil(cap / 64)
  int32_t* stats;          // [n][2] or null: {tiles visited, strips x tiles where both are non-empty}
};

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_cells_kernel(const MatchFramesArgs a, const MatchGuidedArgs g,
                                                                 const MatchCellsArgs c) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_px[64], s_py[64], s_w[64], s_rw[64];
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
  if (tid < 64) {
    const int qi = pq[min(q0 + tid, s.nq - 1)];
    s_qi[tid] = qi;
    s_qn[tid] = s.qn[qi];
    const float* Hf = g.H + (size_t)f * 9;
    double h[9];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      h[k] = (double)Hf[k];
      finite = finite && fabs(h[k]) <= 3.5e38;               // (false for NaN and Inf)
    }
    const double x = (double)qxy[2 * qi], y = (double)qxy[2 * qi + 1];
    const double w = h[6] * x + h[7] * y + h[8];
    s_px[tid] = h[0] * x + h[1] * y + h[2];
    s_py[tid] = h[3] * x + h[4] * y + h[5];
    s_w[tid] = w;
    s_rw[tid] = (finite && q0 + tid < s.nq && w > 0.0) ? g.r2 * w * w : -1.0;
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
        const int r0 = (lane & 3) * 16;
        for (int r = r0; r < r0 + 16 && !hit; ++r) {
          const double px = s_px[r], py = s_py[r], w = s_w[r], rw = s_rw[r];
          const double ax = px - w * u1, bx = px - w * u0, ay = py - w * v1, by = py - w * v0;
          const double dx = fmax(fmax(ax, -bx), 0.0), dy = fmax(fmax(ay, -by), 0.0);
          hit = dx * dx + dy * dy < rw;
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
    // ---- the surviving tiles: match_guided_kernel's tile, rows through the permutations
    for (int e = wave; e < nlist; e += 4) {
      const int t0 = (lb + (int)s_list[e]) * 64;
      const float* trow[2];
      float tn[2];
      double tu[2], tv[2];
      bool tin[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int tj = pt[min(t0 + i * 32 + l31, s.nt - 1)];
        trow[i] = s.t + (size_t)tj * a.D + half * 4;
        tn[i] = s.tn[tj];
        tu[i] = (double)txy[2 * tj];
        tv[i] = (double)txy[2 * tj + 1];
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
          const double px = s_px[row], py = s_py[row], w = s_w[row], rw = s_rw[row];
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const double ex = px - w * tu[ni], ey = py - w * tv[ni];
            if (tin[ni] && ex * ex + ey * ey < rw) pass |= 1ull << ((mi * 16 + r) * 2 + ni);
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
