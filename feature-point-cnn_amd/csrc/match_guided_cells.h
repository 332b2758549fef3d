// match_guided_cells.h -- guided matching over a spatial order of the rows: a strip visits only the train tiles its
// projected pixels can reach (fpc_cell_order / fpc_match_frames_guided_cells / fpc_match_bank_guided_cells, include/fpc.h).
//
// The plain skeleton (mg_strip, match_guided.h) evaluates the gate against every 64 x 64 tile; rows come in confidence
// order, so a tile's rows lie anywhere in the image and hardly a tile is without a candidate.  Here both sides are read
// through a permutation that sorts their rows by 32-px cell, every run of 64 ordered rows carries the bounding box of its
// pixels, and a strip tests the boxes before it touches a tile.  The result of a guided match is a function of the
// candidate set and of each candidate pair's d^2 bits alone (nearest and second nearest: the two smallest (d^2 bits, index)
// keys; column minimum: the smallest key), so the order rows are visited in does not show: the output is the plain
// skeleton's under the same gate, bit for bit, ties included.
//
//   cell_order_kernel      one workgroup per point set.  cell = cy * CX + cx with cx = clamp(x >> shift, 0, CX - 1), cy
//                          likewise (arithmetic shift; shift = 5 wherever the order is public).  An LDS histogram over the
//                          cells, an exclusive prefix sum, then the rows in chunks of 256 in ascending order: a row's rank
//                          among the rows of its cell in its wave comes from one ballot per bit of the cell number, the four
//                          waves of a chunk add their groups to the running cell offsets one after the other.  No atomic
//                          decides a position: perm is the stable order by cell, ascending (cell, row), on every call.
//                          Then one wave per run of 64 ordered rows: the box [umin, vmin, umax, vmax] of its ACTUAL pixels.
//   mgc_strip              the ORDERED skeleton, mg_strip with both sides read through their permutation: a workgroup owns
//                          64 consecutive ORDERED query rows, a tile is 64 consecutive ORDERED train rows; row pointers are
//                          base + perm[..] * D (rows are 512 B / 1 KB: no descriptor is copied), norms and pixels are read
//                          at the original index.
//       Cull.  Four lanes per tile, 16 rows of the strip each, ask the gate whether a row can reach the tile's box
//       (Gate::box / Gate::reach: the test and the proof that it never rejects a tile that holds a candidate are the
//       gate's).  The surviving tiles go into an LDS list in ascending tile order (ballots and per-wave counts, no atomics);
//       the four waves take list entries w, w + 4, ..., so they stay balanced after the cull.
//       A surviving tile is the plain skeleton's: mg_pass_mask, per-wave skip, mg_tile; pairs that fail the gate are +inf
//       and an entry is taken only if < +inf.
//       Selection.  Columns no longer ascend with the train index, so both scans order entries by their 64-bit key:
//       (d^2 bits << 32) | ORIGINAL train index for the top-2, (d^2 bits << 32) | ORIGINAL query index for the column
//       minimum.  top2 goes to the ORIGINAL query row, atomicMin to colbest of the ORIGINAL train row, and
//       match_guided_finalize_kernel / mf_row_ok run unchanged behind it.
//   match_guided_cells_kernel   mgc_strip<MgHomography>.
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

// The ordered skeleton: one workgroup (256 threads), the 64 ordered rows blockIdx.x of frame blockIdx.y.
template <class Gate>
__device__ __forceinline__ void mgc_strip(const MatchFramesArgs& a, const MatchGuidedArgs& g, const MatchCellsArgs& c) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_gate0[64], s_gate1[64], s_gate2[64], s_gate3[64];    // the gate's four values per row of the strip
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
  const Gate gate(g, f, s_gate0, s_gate1, s_gate2, s_gate3);
  if (tid < 64) {
    const int qi = pq[min(q0 + tid, s.nq - 1)];
    s_qi[tid] = qi;
    s_qn[tid] = s.qn[qi];
    gate.row(tid, qxy, qi, q0 + tid < s.nq);
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
        const typename Gate::Box b = gate.box(bt[tt]);
        const int r0 = (lane & 3) * 16;
        for (int r = r0; r < r0 + 16 && !hit; ++r) hit = gate.reach(gate.line(r), b);
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
    // ---- the surviving tiles: the plain skeleton's tile, rows through the permutations
    for (int e = wave; e < nlist; e += 4) {
      const int t0 = (lb + (int)s_list[e]) * 64;
      const float* trow[2];
      float tn[2];
      typename Gate::Col col[2];
      bool tin[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int tj = pt[min(t0 + i * 32 + l31, s.nt - 1)];
        trow[i] = s.t + (size_t)tj * a.D + half * 4;
        tn[i] = s.tn[tj];
        col[i] = gate.column(txy, tj);
        tin[i] = t0 + i * 32 + l31 < s.nt;
      }
      const int tcol = pt[min(t0 + lane, s.nt - 1)];          // lane = column of the tile: its original train index
      tidx[lane] = tcol;
      const unsigned long long pass = mg_pass_mask(gate, col, tin, half);
      if (__ballot(pass != 0ull) == 0ull) continue;            // no candidate in this tile: no loads, no MFMAs
      mg_tile(qrow, trow, tn, s_qn, pass, tile, K8, half, l31);   // (its fence covers tidx too)
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
    __syncthreads();                                        // the list is rebuilt by the next pass
  }
  s_top[wave][lane][0] = k1;
  s_top[wave][lane][1] = k2;
  __syncthreads();
  if (tid < MF_ROWS && q0 + tid < s.nq) mg_merge(s_top, tid, top2, s_qi[tid]);
  if (c.stats && tid == 0) {
    atomicAdd(c.stats + 2 * f, visited);
    atomicAdd(c.stats + 2 * f + 1, ntiles);
  }
}

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_cells_kernel(const MatchFramesArgs a, const MatchGuidedArgs g,
                                                                 const MatchCellsArgs c) {
  mgc_strip<MgHomography>(a, g, c);
}

}  // namespace fpc
