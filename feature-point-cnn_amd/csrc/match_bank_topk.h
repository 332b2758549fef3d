// match_bank_topk.h -- verified relocalisation: the k best slots of the key-frame bank per frame, a match table against each,
// and one RANSAC problem per (frame, candidate) (fpc_bank_topk_reserve / fpc_match_bank_topk / fpc_homography_bank_topk and
// the pose and epipolar models' fpc_pnp_bank_topk / fpc_p3p_bank_topk / fpc_fundamental_bank_topk / fpc_essential_bank_topk,
// include/fpc.h).
//
// fpc_match_bank ranks the slots by appearance and keeps one; a look-alike slot that outscores the right one loses the
// frame.  Here the score pass is fpc_match_bank's own (match_bank.h / match_bank_bf16.h: the same launches, the same
// integers); what follows it works on PAIRS (f, j), j < k <= kmax, whose tables live at pair f kmax + j of a workspace that
// fpc_bank_topk_reserve allocates:
//
//   bank_topk_kernel            grid n: the k largest (score << 32) | ~slot keys of score[f][.], in descending order -- k
//                               rounds of a workgroup arg-max over the keys below the one taken last (keys are distinct, so
//                               "below the last" is the mask; no atomic, no order dependence).  Up to 1024 slots: four keys
//                               per thread, in registers.  Entries below max(min_score, 1): slot -1, score 0.
//   bank_topk_table_kernel      grid (ceil(cap / 64), n, k): mf_strip (match_frames.h), untouched, against slot
//   bank_topk_table_bf16_kernel cand_slot[f][z] -- mf_strip_bf16<K16, false> (match_bank_bf16.h) on a bf16 bank, whose rounded
//                               query rows the score pass has already written.  The strips are the ones the score pass and
//                               the guided pass run, so a pair's d^2 has their bits.  A candidate of -1 is an empty train set.
//   bank_topk_finalize_kernel   grid (ceil(cap / 256), n, k): mf_row_ok on every row of every pair -> match / dist [n][k][cap].
//   bank_pick_kernel            grid n: arg-max of ninliers[f][.] on the integer key (ninliers << 32) | ~j.
//   bank_pick_model_kernel      bank_pick_kernel, and the picked candidate's model (R and t, or F) beside it.
// The RANSAC problems run on ransac_homography.h's kernels with HfArgs::per_frame = k: problem p = f k + j has its own pair
// list, mask row and slot, and frame f's pixels and sampler -- what fpc_homography_bank computes at frame index f.  The
// fundamental and essential kernels take the same HfArgs; the absolute-pose kernels (pnp_ransac.h, p3p_ransac.h) carry
// PnpArgs::per_frame with the same meaning, on records that fpc_pnp_topk_reserve allocates.
#pragma once
#include "match_bank_bf16.h"
#include "ransac_homography.h"

namespace fpc {

constexpr int BANK_TOPK_SLOTS_PER_THREAD = 4;   // 256 threads x 4 = FPC_BANK_MAX_SLOTS

struct BankTopkArgs {
  unsigned long long* top2;     // [B][kmax][cap][2]
  unsigned long long* colbest;  // [B][kmax][rows]
  int32_t* cand_slot;           // [B][kmax]   -1: no candidate
  int32_t* cand_score;          // [B][kmax]
  int kmax;
};

// grid n, 256 threads; b.slots <= 1024.  score_out [n][slots] (may be null), slot_out [n][k], sc_out [n][k] (may be null)
__global__ __launch_bounds__(256) void bank_topk_kernel(const BankArgs b, const BankTopkArgs t, int k, int min_score,
                                                        int32_t* score_out, int32_t* slot_out, int32_t* sc_out) {
  __shared__ unsigned long long wmax[2][4];
  const int f = blockIdx.x, tid = threadIdx.x;
  // (score << 32) | ~slot: larger score, then lower slot.  ~slot is never 0 for a slot below 2^32 - 1: key 0 = none
  unsigned long long key[BANK_TOPK_SLOTS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < BANK_TOPK_SLOTS_PER_THREAD; ++i) {
    const int sl = tid + 256 * i;
    key[i] = 0ull;
    if (sl < b.slots) {
      const int sc = b.score[(size_t)f * b.slots + sl];
      if (score_out) score_out[(size_t)f * b.slots + sl] = sc;
      key[i] = ((unsigned long long)(unsigned)sc << 32) | (unsigned)~sl;
    }
  }
  const int floor = max(min_score, 1);
  unsigned long long prev = ~0ull;                                  // the key taken last: every key lies below it
  for (int j = 0; j < k; ++j) {
    unsigned long long m = 0ull;
#pragma unroll
    for (int i = 0; i < BANK_TOPK_SLOTS_PER_THREAD; ++i) m = (key[i] < prev && key[i] > m) ? key[i] : m;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long other = __shfl_xor(m, o);
      m = other > m ? other : m;
    }
    if ((tid & 63) == 0) wmax[j & 1][tid >> 6] = m;
    __syncthreads();                                                // (two buffers: one barrier per round)
#pragma unroll
    for (int w = 0; w < 4; ++w) m = wmax[j & 1][w] > m ? wmax[j & 1][w] : m;
    prev = m;                                                       // (0 once the keys are used up: nothing lies below)
    if (tid == 0) {
      const int sc = (int)(m >> 32);
      const bool ok = m != 0ull && sc >= floor;
      const int sl = ok ? (int)~(unsigned)(m & 0xffffffffu) : -1;
      t.cand_slot[(size_t)f * t.kmax + j] = sl;
      t.cand_score[(size_t)f * t.kmax + j] = ok ? sc : 0;
      slot_out[(size_t)f * k + j] = sl;
      if (sc_out) sc_out[(size_t)f * k + j] = ok ? sc : 0;
    }
  }
}

// frame f of the results against slot `slot` of the fp32 bank; a slot outside [0, slots) is an empty train set (mf_sets)
__device__ __forceinline__ MfSets bank_topk_sets(const MatchFramesArgs& a, const BankArgs& b, int f, int slot) {
  MfSets s;
  const bool in = slot >= 0 && slot < b.slots;
  s.q = a.desc + (size_t)f * a.cap * a.D;
  s.qn = a.norms + (size_t)f * a.cap;
  s.nq = mf_clamp(a.count[f], a.cap);
  s.t = b.desc + (in ? (size_t)slot * b.rows * b.D : 0);
  s.tn = b.norms + (in ? (size_t)slot * b.rows : 0);
  s.nt = in ? mf_clamp(b.count[slot], b.rows) : 0;
  return s;
}

// grid (ceil(cap / 64), n, k), 256 threads: frame f against slot cand_slot[f][z] into pair f kmax + z's tables
__global__ __launch_bounds__(256) void bank_topk_table_kernel(const MatchFramesArgs a, const BankArgs b, const BankTopkArgs t) {
  const int f = blockIdx.y, z = blockIdx.z;
  const size_t pair = (size_t)f * t.kmax + z;
  mf_strip(a, bank_topk_sets(a, b, f, t.cand_slot[pair]), blockIdx.x * MF_ROWS, t.top2 + pair * a.cap * 2,
           t.colbest + pair * b.rows, nullptr);
}

// the same on a bf16 bank, two workgroups per CU as the strip's other kernels
template <int K16>
__global__ __launch_bounds__(256, 2) void bank_topk_table_bf16_kernel(const MatchFramesArgs a, const BankArgs b,
                                                                      const BankBf16Args h, const BankTopkArgs t) {
  const int f = blockIdx.y, z = blockIdx.z;
  const size_t pair = (size_t)f * t.kmax + z;
  mf_strip_bf16<K16, false>(a, mb_sets(a, b, h, f, t.cand_slot[pair]), blockIdx.x * MF_ROWS, t.top2 + pair * a.cap * 2,
                            t.colbest + pair * b.rows, MbGate{});
}

// grid (ceil(cap / 256), n, k): match / dist [n][k][cap] (either may be null)
__global__ __launch_bounds__(256) void bank_topk_finalize_kernel(const MatchFramesArgs a, const BankArgs b, const BankTopkArgs t,
                                                                 int k, float max_dist, float ratio, int32_t* match,
                                                                 float* dist) {
  const int f = blockIdx.y, z = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.cap) return;
  const size_t pair = (size_t)f * t.kmax + z;
  const int slot = t.cand_slot[pair];
  const bool in = slot >= 0 && slot < b.slots;
  const int nq = mf_clamp(a.count[f], a.cap), nt = in ? mf_clamp(b.count[slot], b.rows) : 0;
  const size_t o = ((size_t)f * k + z) * a.cap + i;
  if (i >= nq || nt == 0) {
    if (match) match[o] = -1;
    if (dist) dist[o] = INFINITY;
    return;
  }
  const unsigned long long* t2 = t.top2 + (pair * a.cap + i) * 2;
  float d;
  const bool ok = mf_row_ok(t2[0], t2[1], i, a.cross_check ? t.colbest + pair * b.rows : nullptr, max_dist, ratio, d);
  if (match) match[o] = ok ? (int)(t2[0] & 0xffffffffu) : -1;
  if (dist) dist[o] = d;
}

// (one wave, lane j < 64, k <= 64) the j with the most inliers among ninliers[f][.] (ties to the lower j), -1 when there are
// none; the same in every lane.  The integer key (ninliers << 32) | ~j.
__device__ __forceinline__ int bank_pick(const int32_t* __restrict__ ninliers, int f, int k) {
  const int j = threadIdx.x;
  unsigned long long key = 0ull;
  if (j < k) {
    const int ni = ninliers[(size_t)f * k + j];
    if (ni > 0) key = ((unsigned long long)(unsigned)ni << 32) | (unsigned)~j;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  return key ? (int)~(unsigned)(key & 0xffffffffu) : -1;
}

// grid n, 64 threads, k <= 64: pick[f] = bank_pick; best[f] = cand_slot[f][pick[f]] or -1.  pick / best may be null.
__global__ __launch_bounds__(64) void bank_pick_kernel(const int32_t* __restrict__ ninliers, const int32_t* __restrict__ cand_slot,
                                                       int k, int32_t* pick, int32_t* best) {
  const int f = blockIdx.x;
  const int p = bank_pick(ninliers, f, k);
  if (threadIdx.x == 0) {
    if (pick) pick[f] = p;
    if (best) best[f] = p >= 0 ? cand_slot[(size_t)f * k + p] : -1;
  }
}

// The pose and epipolar top-K calls' tail (fpc_pnp_bank_topk / fpc_p3p_bank_topk / fpc_fundamental_bank_topk /
// fpc_essential_bank_topk): bank_pick_kernel, and the picked candidate's model beside it -- best0[f][.] = m0[f][pick[f]][.]
// (w0 <= 64 floats: R or F) and best1[f][.] = m1[f][pick[f]][.] (w1 <= 64 floats: t), zeros where pick[f] is -1.  Every
// output may be null (m1 with best1).  The models were written by the refit kernel launched in front of this one.
__global__ __launch_bounds__(64) void bank_pick_model_kernel(const int32_t* __restrict__ ninliers,
                                                             const int32_t* __restrict__ cand_slot, int k, int32_t* pick,
                                                             int32_t* best, const float* __restrict__ m0, int w0, float* best0,
                                                             const float* __restrict__ m1, int w1, float* best1) {
  const int f = blockIdx.x, j = threadIdx.x;
  const int p = bank_pick(ninliers, f, k);
  if (j == 0) {
    if (pick) pick[f] = p;
    if (best) best[f] = p >= 0 ? cand_slot[(size_t)f * k + p] : -1;
  }
  if (best0 && j < w0) best0[(size_t)f * w0 + j] = p >= 0 ? m0[((size_t)f * k + p) * w0 + j] : 0.f;
  if (best1 && j < w1) best1[(size_t)f * w1 + j] = p >= 0 ? m1[((size_t)f * k + p) * w1 + j] : 0.f;
}

}  // namespace fpc
