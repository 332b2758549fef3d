// match_bank_bf16.h -- the key-frame bank in bf16: storage at 2 B per component and fpc_match_bank / fpc_match_bank_guided
// on v_mfma_f32_32x32x16_bf16 (fpc_bank_create_ex with FPC_BANK_BF16, include/fpc.h).
//
// An opt-in format next to the fp32 bank of match_bank.h, whose kernels and bits it leaves alone.  The bank's descriptors
// are bf16 [slots][rows][D] (each fp32 component rounded to nearest even, a NaN to 0x7FC0), its norms fp32 [slots][rows]
// computed FROM THE ROUNDED rows; xy, count, the top-2 / column tables, score and best are match_bank.h's BankArgs.  The
// query sets are rounded the same way once per call into a workspace of the bank's own ([max_batch][cap][D] bf16), their
// norms go to fpc_match_frames' norm table.
//
//   bank_store_bf16_kernel      bank_store_kernel with the conversion and the norm of the rounded row in one pass.
//   bank_round_queries_kernel   the same conversion and norms for frames 0 .. n-1 of the results; stands where
//                               mf_norms_kernel stands on the fp32 path.
//   mf_strip_bf16<K16, GATED>   mf_strip's organisation -- a 64-row strip per workgroup, its four waves taking the train
//                               tiles w, w + 4, ..., a 2 x 2 tile of 32 x 32 blocks per wave -- with the K loop on
//                               __builtin_amdgcn_mfma_f32_32x32x16_bf16, K16 = D / 16 steps.  Operand map: lane l holds row
//                               l & 31, k = 16 step + 8 (l >> 5) + j, j = 0..7: ONE 16-byte global load per fragment.  The
//                               C/D layout is the 32x32x2 one, so everything behind the accumulators is mf_strip's:
//                               d^2 = max(|q|^2 + |t|^2 - 2 q.t, 0) through a wave-private LDS tile, the top-2 scan on strict
//                               <, the column scan with 64-bit atomicMin, the merge of the waves' lists on (d^2 bits, index)
//                               keys.  At D = 128 the strip's query fragments stay in registers over all tiles (64 VGPRs);
//                               the train fragments of the next tile are requested before the epilogue of this one.
//                               GATED adds match_guided_kernel's gate (the same fp64 expressions, the same 64-bit mask in
//                               the C/D layout, a tile without a passing pair skipped before any load) -- one function, so
//                               that a pair's d^2 has the same bits in the score pass, the table pass and the guided pass.
//   bank_score_bf16_kernel      grid (ceil(cap / 64), n, chunk): the strip against slot s0 + z into the bank's tables; what
//                               follows it is bank_count_kernel and bank_select_kernel as they are.
//   match_bank_bf16_kernel      grid (ceil(cap / 64), n): the strip against slot key_slot[f] into fpc_match_frames' tables
//                               (the table pass of fpc_match_bank; GATED: fpc_match_bank_guided); what follows it is
//                               match_frames_finalize_kernel / match_guided_finalize_kernel as they are.
#pragma once
#include "block_bf16.h"
#include "match_bank.h"
#include "match_guided.h"

namespace fpc {

struct BankBf16Args {
  bf16_t* desc;                 // [slots][rows][D]   the bank's rows (BankArgs::desc is null in this format)
  bf16_t* q;                    // [B][cap][D]        the query sets of the call in flight
};

struct MbSets {
  const bf16_t *q, *t;          // row 0 of the query / train set
  const float *qn, *tn;         // their squared norms (of the rounded rows)
  int nq, nt;
};

// fp32 -> bf16, round to nearest even (torch.bfloat16's bits); a NaN -> the quiet NaN 0x7FC0
__device__ __forceinline__ unsigned mb_rne(float x) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// lane l / l + 32 of a wave hold the two halves of one row, as in mf_row_norm (`row` and `out` point at element half * 4):
// rounds the lane's components, stores them when `store`, and returns |rounded row|^2 (fp32, both halves added)
__device__ __forceinline__ float mb_round_row(const float* row, bf16_t* out, int K8, bool store) {
  float s = 0.f;
  for (int k8 = 0; k8 < K8; ++k8) {
    const float4 c = *reinterpret_cast<const float4*>(row + k8 * 8);
    const unsigned r0 = mb_rne(c.x), r1 = mb_rne(c.y), r2 = mb_rne(c.z), r3 = mb_rne(c.w);
    if (store) *reinterpret_cast<uint2*>(out + k8 * 8) = make_uint2(r0 | (r1 << 16), r2 | (r3 << 16));
    const float x = bf2f((bf16_t)r0), y = bf2f((bf16_t)r1), z = bf2f((bf16_t)r2), w = bf2f((bf16_t)r3);
    s += x * x + y * y + z * z + w * w;
  }
  s += __shfl_xor(s, 32);
  return s;
}

// grid ceil(rows / 128), 256 threads: bank_store_kernel's shape and arguments
__global__ __launch_bounds__(256) void bank_store_bf16_kernel(const BankArgs b, const BankBf16Args h, int slot,
                                                              const float* __restrict__ src_desc,
                                                              const int32_t* __restrict__ src_xy,
                                                              const int32_t* __restrict__ n, int src_cap) {
  const int nr = mf_clamp(*n, min(src_cap, b.rows));
  if (blockIdx.x == 0 && threadIdx.x == 0) b.count[slot] = nr;
  if ((int)blockIdx.x * 128 >= nr) return;
  const int lane = threadIdx.x & 63, half = lane >> 5;
  const int r = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const int rr = min(r, nr - 1);
  const float s = mb_round_row(src_desc + (size_t)rr * b.D + half * 4, h.desc + ((size_t)slot * b.rows + rr) * b.D + half * 4,
                               b.D / 8, r < nr);
  if (half == 0 && r < nr) {
    b.norms[(size_t)slot * b.rows + r] = s;
    b.xy[((size_t)slot * b.rows + r) * 2] = src_xy[2 * r];
    b.xy[((size_t)slot * b.rows + r) * 2 + 1] = src_xy[2 * r + 1];
  }
}

// grid (ceil(cap / 128), n), 256 threads: mf_norms_kernel's shape without the key block
__global__ __launch_bounds__(256) void bank_round_queries_kernel(const MatchFramesArgs a, const BankBf16Args h) {
  const int f = blockIdx.y;
  const int nr = mf_clamp(a.count[f], a.cap);
  if ((int)blockIdx.x * 128 >= nr) return;
  const int lane = threadIdx.x & 63, half = lane >> 5;
  const int r = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const size_t o = ((size_t)f * a.cap + min(r, nr - 1)) * a.D + half * 4;
  const float s = mb_round_row(a.desc + o, h.q + o, a.D / 8, r < nr);
  if (half == 0 && r < nr) a.norms[(size_t)f * a.cap + r] = s;
}

// frame f against slot `slot` (outside [0, slots): an empty train set, as in mf_sets)
__device__ __forceinline__ MbSets mb_sets(const MatchFramesArgs& a, const BankArgs& b, const BankBf16Args& h, int f, int slot) {
  MbSets s;
  const bool in = slot >= 0 && slot < b.slots;
  s.q = h.q + (size_t)f * a.cap * a.D;
  s.qn = a.norms + (size_t)f * a.cap;
  s.nq = mf_clamp(a.count[f], a.cap);
  s.t = h.desc + (in ? (size_t)slot * b.rows * b.D : 0);
  s.tn = b.norms + (in ? (size_t)slot * b.rows : 0);
  s.nt = in ? mf_clamp(b.count[slot], b.rows) : 0;
  return s;
}

// the gate of one frame (match_guided.h): H [9], the frame's and the train set's pixels, radius^2
struct MbGate {
  const float* H;
  const int32_t *qxy, *txy;
  double r2;
};

// One workgroup (256 threads), one 64-row strip (rows q0 ..) of one (query set, train set) pair `s`.  top2 [..][2],
// colbest [..]: row 0 of THIS pair's tables.  K16 = D / 16.
template <int K16, bool GATED>
__device__ __forceinline__ void mf_strip_bf16(const MatchFramesArgs& a, const MbSets& s, int q0, unsigned long long* top2,
                                              unsigned long long* colbest, const MbGate& g) {
  constexpr bool QREG = K16 <= 8;            // the strip's query fragments in registers: 2 x K16 x 4 VGPRs
  constexpr int D = K16 * 16;
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ float s_qn[64];
  __shared__ double s_gate[4][GATED ? 64 : 1];   // px, py, w, radius^2 w^2 of the strip's rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  if (q0 >= s.nq || s.nt == 0) return;       // (the finalize / count kernels read nq / nt themselves)
  if (tid < 64) {
    s_qn[tid] = s.qn[min(q0 + tid, s.nq - 1)];
    if constexpr (GATED) {
      double hh[9];
      bool finite = true;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        hh[k] = (double)g.H[k];
        finite = finite && fabs(hh[k]) <= 3.5e38;             // (false for NaN and Inf)
      }
      const int qi = min(q0 + tid, s.nq - 1);
      const double x = (double)g.qxy[2 * qi], y = (double)g.qxy[2 * qi + 1];
      const double w = hh[6] * x + hh[7] * y + hh[8];
      s_gate[0][tid] = hh[0] * x + hh[1] * y + hh[2];
      s_gate[1][tid] = hh[3] * x + hh[4] * y + hh[5];
      s_gate[2][tid] = w;
      s_gate[3][tid] = (finite && q0 + tid < s.nq && w > 0.0) ? g.r2 * w * w : -1.0;
    }
  }
  __syncthreads();
  // fragment of k-step k of a row: the 16 bytes at element 16 k + 8 half
  const uint4* qrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    qrow[i] = reinterpret_cast<const uint4*>(s.q + (size_t)min(q0 + i * 32 + l31, s.nq - 1) * D + half * 8);
  uint4 qf[2][QREG ? K16 : 1];
  if constexpr (QREG) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < K16; ++k) qf[i][k] = qrow[i][2 * k];
  }
  const int nrow = min(64, s.nq - q0);
  float* tile = s_d2[wave];
  // lane = row of the strip: best and second best (strict <, columns ascending: ties keep the lower index)
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = -1, i2 = -1;
  const int ntiles = (s.nt + 63) / 64;
  uint4 tf[2][K16];
  float tnn[2];
  auto load_tile = [&](int tt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tj = min(tt * 64 + i * 32 + l31, s.nt - 1);
      const uint4* trow = reinterpret_cast<const uint4*>(s.t + (size_t)tj * D + half * 8);
#pragma unroll
      for (int k = 0; k < K16; ++k) tf[i][k] = trow[2 * k];
      tnn[i] = s.tn[tj];
    }
  };
  if constexpr (!GATED)
    if (wave < ntiles) load_tile(wave);
  for (int tt = wave; tt < ntiles; tt += 4) {
    const int t0 = tt * 64;
    unsigned long long pass = ~0ull;
    if constexpr (GATED) {
      // the gate, in the C/D layout of the tile below: bit (mi * 16 + r) * 2 + ni of `pass`
      double tu[2], tv[2];
      bool tin[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int tj = min(t0 + i * 32 + l31, s.nt - 1);
        tu[i] = (double)g.txy[2 * tj];
        tv[i] = (double)g.txy[2 * tj + 1];
        tin[i] = t0 + i * 32 + l31 < s.nt;
      }
      pass = 0ull;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          const double px = s_gate[0][row], py = s_gate[1][row], w = s_gate[2][row], rw = s_gate[3][row];
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const double ex = px - w * tu[ni], ey = py - w * tv[ni];
            if (tin[ni] && ex * ex + ey * ey < rw) pass |= 1ull << ((mi * 16 + r) * 2 + ni);
          }
        }
      if (__ballot(pass != 0ull) == 0ull) continue;            // no candidate in this tile: no loads, no MFMAs
      load_tile(tt);
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int k = 0; k < K16; ++k) {
      uint4 qk[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr (QREG) qk[i] = qf[i][k];
        else qk[i] = qrow[i][2 * k];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qk[mi]),
                                                                __builtin_bit_cast(bf16x8, tf[ni][k]), acc[mi][ni], 0, 0, 0);
    }
    const float tn[2] = {tnn[0], tnn[1]};
    if constexpr (!GATED)
      if (tt + 4 < ntiles) load_tile(tt + 4);                  // in flight during the epilogue below
    // C/D map: column (t) = lane & 31, row (q) = (r&3) + 8*(r>>2) + 4*half
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rowl = (r & 3) + 8 * (r >> 2) + 4 * half;
        const float qnr = s_qn[mi * 32 + rowl];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          float d2 = match_d2(qnr, tn[ni], acc[mi][ni][r]);
          if constexpr (GATED) d2 = (pass >> ((mi * 16 + r) * 2 + ni)) & 1ull ? d2 : INFINITY;
          tile[(mi * 32 + rowl) * MF_PITCH + ni * 32 + l31] = d2;
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
    if (a.cross_check) {                   // lane = column of the tile: its arg-min over the strip's (candidate) rows
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

// grid (ceil(cap / 64), n, slots of this chunk), 256 threads, two workgroups per CU; slot = s0 + blockIdx.z
template <int K16>
__global__ __launch_bounds__(256, 2) void bank_score_bf16_kernel(const MatchFramesArgs a, const BankArgs b,
                                                                 const BankBf16Args h, int s0) {
  const int f = blockIdx.y, z = blockIdx.z;
  const size_t pair = (size_t)f * b.chunk + z;
  mf_strip_bf16<K16, false>(a, mb_sets(a, b, h, f, s0 + z), blockIdx.x * MF_ROWS, b.top2 + pair * a.cap * 2,
                            b.colbest + pair * b.rows, MbGate{});
}

// grid (ceil(cap / 64), n), 256 threads: frame f against slot a.key_slot[f] into fpc_match_frames' tables (a.top2,
// a.colbest); GATED: under g.H[f] (g.key_xy = the bank's xy)
template <int K16, bool GATED>
__global__ __launch_bounds__(256, 2) void match_bank_bf16_kernel(const MatchFramesArgs a, const BankArgs b,
                                                                 const BankBf16Args h, const MatchGuidedArgs g) {
  const int f = blockIdx.y;
  MbGate gate{};
  if constexpr (GATED) {
    gate.H = g.H + (size_t)f * 9;
    gate.qxy = g.xy + (size_t)f * a.cap * 2;
    gate.txy = mg_train_xy(a, g, f);       // (null only where the train set is empty: the strip returns before the gate)
    gate.r2 = g.r2;
  }
  mf_strip_bf16<K16, GATED>(a, mb_sets(a, b, h, f, a.key_slot[f]), blockIdx.x * MF_ROWS, a.top2 + (size_t)f * a.cap * 2,
                            a.colbest + (size_t)f * a.cap, gate);
}

}  // namespace fpc
