// match_frames.h -- descriptor matching of a whole batch in one call, straight from the device results of the last call
// that produced keypoints with descriptors (fpc_match_frames / fpc_first_within_frames, include/fpc.h).
//
// Frame f's query set is desc[f][0 .. count[f]); its train set is the key set (FPC_PAIR_KEY) or frame f-1 of the same
// results (FPC_PAIR_PREVIOUS; frame 0 against the key, or nothing).  Every count is read on the device: the grid depends
// only on host-known sizes (n, cap), and a workgroup whose strip starts past its frame's count exits after that load.
//
//   mf_norms_kernel        |row|^2 of every frame row and every key row, ONCE per call (the key is shared by all
//                          frames), with match_gemm_kernel's own partial sums: lane l / l+32 sum the two halves of each
//                          k8 step, then one add -- so d^2 is bit-identical to fpc_match's on the same pair.
//   match_frames_kernel    one workgroup owns a 64-row strip of one frame and loops over ALL train tiles of that frame
//                          (its four waves take tiles w, w+4, ...): the exact top-2 of a row (for the ratio test) never
//                          leaves the workgroup.  Each wave's 64 x 64 tile is match_gemm_kernel's: 2 x 2
//                          v_mfma_f32_32x32x2_f32 blocks, operands straight from global memory in the same K order,
//                          d^2 = |q|^2 + |t|^2 - 2 q.t with the same clamp.  The four waves' top-2 lists are merged on
//                          (d^2 bits, index) keys: a selection, no arithmetic, so the result does not depend on order.
//                          Column minima for the cross check: 64-bit atomicMin on (d^2 bits, row) per frame, as in
//                          match.h (exact, order-independent, ties to the lower row).
//   match_frames_finalize_kernel  cross check, max_dist, ratio test; rows past count[f] -> -1.
// The strip body (mf_strip), the row norm (mf_row_norm) and the finalize rule (mf_row_ok) are device functions that the
// key-frame bank (match_bank.h) calls too; with MatchFramesArgs::key_slot the key is chosen per frame from that bank.
// In first-within mode the key is the query and frame f the train set; the lowest index below the tolerance is a
// plain minimum, and the strip's workgroup writes the output itself.
#pragma once
#include "match.h"

namespace fpc {

constexpr int MF_ROWS = 64;     // query rows per workgroup
constexpr int MF_PITCH = 68;    // LDS pitch of a wave's 64 x 64 d^2 tile (floats), as in match_gemm_kernel

struct MatchFramesArgs {
  const float* desc;            // [B][cap][D]  fpc_results().desc
  const int32_t* count;         // [B]          fpc_results().count (device)
  const float* key;             // [cap][D]     key set (may be null in FPC_PAIR_PREVIOUS)
  const int32_t* nkey;          // device int32: rows of the key set, clamped to [0, cap]
  int n, cap, D;
  int pairing;                  // 0: every frame against the key; 1: frame f against frame f-1 (frame 0 against the key)
  int first_mode;               // 1: first-within (query = key, train = frame f)
  int cross_check;
  float tol2;                   // first-within: tolerance^2
  float* norms;                 // [(n + 1)][cap]  |row|^2; row block n = the key
  unsigned long long* top2;     // [n][cap][2]     (d^2 bits << 32 | train index), best then second best
  unsigned long long* colbest;  // [n][cap]        (d^2 bits << 32 | query index), pre-filled with ~0
  int32_t* first;               // [n][cap]        first-within output
  // per-frame key (fpc_match_bank's table pass, match_bank.h): with key_slot != null frame f's train set is slot
  // key_slot[f] of a key-frame bank -- `key` is the bank's desc [slots][bank_rows][D], its norms and counts are the
  // bank's own -- and a slot outside [0, bank_slots) is an empty train set.  Null in fpc_match_frames /
  // fpc_first_within_frames, whose sets are the ones above.
  const int32_t* key_slot;      // [n]  device
  const float* bank_norms;      // [slots][bank_rows]
  const int32_t* bank_count;    // [slots]
  int bank_rows, bank_slots;
};

__device__ __forceinline__ int mf_clamp(int v, int cap) { return v < 0 ? 0 : v > cap ? cap : v; }
__device__ __forceinline__ int mf_nkey(const MatchFramesArgs& a) { return (a.key && a.nkey) ? mf_clamp(*a.nkey, a.cap) : 0; }

struct MfSets {
  const float *q, *t;      // row 0 of the query / train set
  const float *qn, *tn;    // their squared norms
  int nq, nt;
};

__device__ __forceinline__ MfSets mf_sets(const MatchFramesArgs& a, int f) {
  MfSets s;
  const float* fd = a.desc + (size_t)f * a.cap * a.D;
  const float* fn = a.norms + (size_t)f * a.cap;
  const float* kn = a.norms + (size_t)a.n * a.cap;
  if (a.first_mode) {
    s.q = a.key; s.qn = kn; s.nq = mf_nkey(a);
    s.t = fd; s.tn = fn; s.nt = mf_clamp(a.count[f], a.cap);
    return s;
  }
  s.q = fd; s.qn = fn; s.nq = mf_clamp(a.count[f], a.cap);
  if (a.pairing == 1 && f > 0) {
    s.t = a.desc + (size_t)(f - 1) * a.cap * a.D; s.tn = a.norms + (size_t)(f - 1) * a.cap;
    s.nt = mf_clamp(a.count[f - 1], a.cap);
  } else if (a.key_slot) {
    const int sl = a.key_slot[f];
    const bool in = sl >= 0 && sl < a.bank_slots;
    s.t = a.key + (in ? (size_t)sl * a.bank_rows * a.D : 0);
    s.tn = a.bank_norms + (in ? (size_t)sl * a.bank_rows : 0);
    s.nt = in ? mf_clamp(a.bank_count[sl], a.bank_rows) : 0;
  } else {
    s.t = a.key; s.tn = kn; s.nt = mf_nkey(a);
  }
  return s;
}

// lane l / l + 32 of a wave hold the two halves of one row (`row` points at float half * 4 of it): the partial sum of
// match_gemm_kernel's qn / tn step, then one add across the halves
__device__ __forceinline__ float mf_row_norm(const float* row, int K8) {
  float s = 0.f;
  for (int k8 = 0; k8 < K8; ++k8) {
    const float4 c = *reinterpret_cast<const float4*>(row + k8 * 8);
    s += c.x * c.x + c.y * c.y + c.z * c.z + c.w * c.w;     // match_gemm_kernel's qn / tn step
  }
  s += __shfl_xor(s, 32);
  return s;
}

// grid (ceil(cap / 128), n + 1), 256 threads: each wave 32 rows, lane l and l + 32 the two halves of row l & 31
__global__ __launch_bounds__(256) void mf_norms_kernel(const MatchFramesArgs a) {
  const int f = blockIdx.y;
  const int nr = f < a.n ? mf_clamp(a.count[f], a.cap) : mf_nkey(a);
  if ((int)blockIdx.x * 128 >= nr) return;
  const int lane = threadIdx.x & 63, half = lane >> 5;
  const int r = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const float* base = f < a.n ? a.desc + (size_t)f * a.cap * a.D : a.key;
  const float* row = base + (size_t)min(r, nr - 1) * a.D + half * 4;
  const float s = mf_row_norm(row, a.D / 8);
  if (half == 0 && r < nr) a.norms[(size_t)f * a.cap + r] = s;
}

// One workgroup (256 threads), one 64-row strip (rows q0 ..) of one (query set, train set) pair `s`: the body of
// match_frames_kernel, shared with the key-frame bank's score pass (match_bank.h), which runs it over a third grid
// dimension.  top2 [..][2], colbest [..], first_out [..]: row 0 of THIS pair's tables.
__device__ __forceinline__ void mf_strip(const MatchFramesArgs& a, const MfSets& s, int q0, unsigned long long* top2,
                                         unsigned long long* colbest, int32_t* first_out) {
  __shared__ __attribute__((aligned(16))) float s_d2[4][64 * MF_PITCH];
  __shared__ unsigned long long s_top[4][64][2];
  __shared__ unsigned int s_first[4][64];
  __shared__ float s_qn[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  if (q0 >= s.nq || s.nt == 0) {            // an empty strip, or no train rows: nothing to multiply
    if (a.first_mode && tid < MF_ROWS && q0 + tid < a.cap) first_out[q0 + tid] = -1;
    return;                                  // (arg-min mode: the finalize kernel reads nq / nt itself)
  }
  if (tid < 64) s_qn[tid] = s.qn[min(q0 + tid, s.nq - 1)];
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
  unsigned int firstj = ~0u;
  const int ntiles = (s.nt + 63) / 64;
  for (int tt = wave; tt < ntiles; tt += 4) {
    const int t0 = tt * 64;
    const float* trow[2];
    float tn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tj = min(t0 + i * 32 + l31, s.nt - 1);
      trow[i] = s.t + (size_t)tj * a.D + half * 4;
      tn[i] = s.tn[tj];
    }
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
        for (int ni = 0; ni < 2; ++ni)
          tile[(mi * 32 + rowl) * MF_PITCH + ni * 32 + l31] = match_d2(qnr, tn[ni], acc[mi][ni][r]);
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
            if (a.first_mode) {
              if (e[k] < a.tol2 && firstj == ~0u) firstj = (unsigned)(t0 + j);
            } else if (e[k] < b1) {
              b2 = b1; i2 = i1; b1 = e[k]; i1 = t0 + j;
            } else if (e[k] < b2) {
              b2 = e[k]; i2 = t0 + j;
            }
          }
        }
      }
    }
    if (!a.first_mode && a.cross_check) {  // lane = column of the tile: its arg-min over the strip's rows
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
  if (a.first_mode) {
    s_first[wave][lane] = firstj;
  } else {
    s_top[wave][lane][0] = i1 >= 0 ? ((unsigned long long)__float_as_uint(b1) << 32) | (unsigned)i1 : ~0ull;
    s_top[wave][lane][1] = i2 >= 0 ? ((unsigned long long)__float_as_uint(b2) << 32) | (unsigned)i2 : ~0ull;
  }
  __syncthreads();
  if (tid < MF_ROWS) {
    const int qi = q0 + tid;
    if (a.first_mode) {
      unsigned int m = ~0u;
#pragma unroll
      for (int w = 0; w < 4; ++w) m = min(m, s_first[w][tid]);
      if (qi < a.cap) first_out[qi] = (qi < s.nq && m != ~0u) ? (int)m : -1;
    } else if (qi < s.nq) {
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
      unsigned long long* o = top2 + (size_t)qi * 2;
      o[0] = m1;
      o[1] = m2;
    }
  }
}

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_frames_kernel(const MatchFramesArgs a) {
  const int f = blockIdx.y;
  mf_strip(a, mf_sets(a, f), blockIdx.x * MF_ROWS, a.top2 + (size_t)f * a.cap * 2, a.colbest + (size_t)f * a.cap,
           a.first + (size_t)f * a.cap);
}

// Row i's fate from its top-2 keys k1, k2 and the pair's column minima (null: no cross check): cross check, max_dist,
// ratio test, ANDed; d = the distance to the nearest train row.  Shared with the bank's score pass (match_bank.h).
__device__ __forceinline__ bool mf_row_ok(unsigned long long k1, unsigned long long k2, int i,
                                          const unsigned long long* colbest, float max_dist, float ratio, float& d) {
  if (k1 == ~0ull) {       // no train row at a finite distance: no index to look up in colbest
    d = INFINITY;
    return false;
  }
  const int j = (int)(k1 & 0xffffffffu);
  d = sqrtf(__uint_as_float((unsigned)(k1 >> 32)));
  bool ok = true;
  if (colbest) ok = (int)(colbest[j] & 0xffffffffu) == i;
  if (ok && max_dist > 0.f) ok = d < max_dist;
  if (ok && ratio > 0.f) ok = k2 != ~0ull && d < ratio * sqrtf(__uint_as_float((unsigned)(k2 >> 32)));
  return ok;
}

// grid (ceil(cap / 256), n)
__global__ __launch_bounds__(256) void match_frames_finalize_kernel(const MatchFramesArgs a, float max_dist, float ratio,
                                                                    int32_t* match, float* dist) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cap) return;
  const MfSets s = mf_sets(a, f);
  const size_t o = (size_t)f * a.cap + i;
  if (i >= s.nq || s.nt == 0) {
    if (match) match[o] = -1;
    if (dist) dist[o] = INFINITY;
    return;
  }
  float d;
  const int j = (int)(a.top2[2 * o] & 0xffffffffu);
  const bool ok = mf_row_ok(a.top2[2 * o], a.top2[2 * o + 1], i, a.cross_check ? a.colbest + (size_t)f * a.cap : nullptr,
                            max_dist, ratio, d);
  if (match) match[o] = ok ? j : -1;
  if (dist) dist[o] = d;
}

}  // namespace fpc
