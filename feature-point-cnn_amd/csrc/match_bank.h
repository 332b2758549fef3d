// match_bank.h -- a device-resident bank of key frames and the match of a whole detect batch against ALL of its slots in
// one call (fpc_bank_* / fpc_match_bank, include/fpc.h).
//
// The bank: desc [slots][rows][D], xy [slots][rows][2], count [slots] (0 = empty) and the rows' squared norms
// [slots][rows], computed once when a slot is stored -- by mf_row_norm, mf_norms_kernel's own partial sums, so that a
// distance against a slot is bit-equal to fpc_match_frames' with the slot as its key.
//
//   bank_store_kernel      copies the first min(*n, rows) rows of a descriptor / coordinate set into a slot, computes
//                          their norms in the same pass (the float4 a lane loads for the norm is the one it stores) and
//                          writes the slot's count.  *n is read on the device.
//   bank_score_kernel      grid (ceil(cap / 64), n, chunk): match_frames_kernel's strip (mf_strip, match_frames.h -- the
//                          same 2 x 2 v_mfma_f32_32x32x2_f32 tile, K order, d^2 expression, clamp, top-2 and 64-bit
//                          atomicMin column minima) with the slot as a third grid dimension.  A strip past count[f] or
//                          a slot with count 0 exits after that load.  Slots run in chunks so that the top-2 / column
//                          tables stay at max_batch x chunk x cap entries (fpc_bank_create sizes the chunk).
//   bank_count_kernel      grid (ceil(cap / 256), n, chunk): mf_row_ok (cross check, max_dist, ratio) on every row of
//                          every (frame, slot), survivors counted by ballot + popcount and added to score[f][slot] with
//                          one integer atomicAdd per workgroup: a sum of integers, independent of the order.
//   bank_select_kernel     grid n: arg-max over score[f][.] on the integer key (score << 32) | ~slot -- the largest score,
//                          ties to the lower slot; -1 below max(min_score, 1).  Copies the scores to the caller.
// The returned table is then fpc_match_frames' own three kernels with a per-frame key (MatchFramesArgs::key_slot): the
// same code path, hence the same bits, at 1 / slots of the score pass.
#pragma once
#include "match_frames.h"

namespace fpc {

struct BankArgs {
  float* desc;                  // [slots][rows][D]
  int32_t* xy;                  // [slots][rows][2]
  int32_t* count;               // [slots]
  float* norms;                 // [slots][rows]
  int slots, rows, D;
  // fpc_match_bank's workspace
  unsigned long long* top2;     // [B][chunk][cap][2]
  unsigned long long* colbest;  // [B][chunk][rows]
  int32_t* score;               // [B][slots]
  int32_t* best;                // [B]
  int chunk;
};

// grid ceil(rows / 128), 256 threads: each wave 32 rows, lane l and l + 32 the two halves of row l & 31 (mf_norms_kernel)
// src_desc [..][D] (16-byte aligned), src_xy [..][2], *n clamped to [0, min(src_cap, rows)]
__global__ __launch_bounds__(256) void bank_store_kernel(const BankArgs b, int slot, const float* __restrict__ src_desc,
                                                         const int32_t* __restrict__ src_xy, const int32_t* __restrict__ n,
                                                         int src_cap) {
  const int nr = mf_clamp(*n, min(src_cap, b.rows));
  if (blockIdx.x == 0 && threadIdx.x == 0) b.count[slot] = nr;
  if ((int)blockIdx.x * 128 >= nr) return;
  const int lane = threadIdx.x & 63, half = lane >> 5;
  const int r = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + (lane & 31);
  const int rr = min(r, nr - 1);
  const float* row = src_desc + (size_t)rr * b.D + half * 4;
  float* out = b.desc + ((size_t)slot * b.rows + rr) * b.D + half * 4;
  const int K8 = b.D / 8;
  if (r < nr)
    for (int k8 = 0; k8 < K8; ++k8) *reinterpret_cast<float4*>(out + k8 * 8) = *reinterpret_cast<const float4*>(row + k8 * 8);
  const float s = mf_row_norm(row, K8);
  if (half == 0 && r < nr) {
    b.norms[(size_t)slot * b.rows + r] = s;
    b.xy[((size_t)slot * b.rows + r) * 2] = src_xy[2 * r];
    b.xy[((size_t)slot * b.rows + r) * 2 + 1] = src_xy[2 * r + 1];
  }
}

// slot == -1: every slot
__global__ void bank_clear_kernel(const BankArgs b, int slot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b.slots && (slot < 0 || i == slot)) b.count[i] = 0;
}

// frame f of the results against slot `slot` of the bank
__device__ __forceinline__ MfSets bank_sets(const MatchFramesArgs& a, const BankArgs& b, int f, int slot) {
  MfSets s;
  s.q = a.desc + (size_t)f * a.cap * a.D;
  s.qn = a.norms + (size_t)f * a.cap;
  s.nq = mf_clamp(a.count[f], a.cap);
  s.t = b.desc + (size_t)slot * b.rows * b.D;
  s.tn = b.norms + (size_t)slot * b.rows;
  s.nt = mf_clamp(b.count[slot], b.rows);
  return s;
}

// grid (ceil(cap / 64), n, slots of this chunk), 256 threads; slot = s0 + blockIdx.z
__global__ __launch_bounds__(256) void bank_score_kernel(const MatchFramesArgs a, const BankArgs b, int s0) {
  const int f = blockIdx.y, z = blockIdx.z;
  const size_t pair = (size_t)f * b.chunk + z;
  mf_strip(a, bank_sets(a, b, f, s0 + z), blockIdx.x * MF_ROWS, b.top2 + pair * a.cap * 2, b.colbest + pair * b.rows, nullptr);
}

// grid (ceil(cap / 256), n, slots of this chunk), 256 threads
__global__ __launch_bounds__(256) void bank_count_kernel(const MatchFramesArgs a, const BankArgs b, int s0, float max_dist,
                                                         float ratio) {
  __shared__ int wsum[4];
  const int f = blockIdx.y, z = blockIdx.z, i = blockIdx.x * 256 + threadIdx.x;
  const MfSets s = bank_sets(a, b, f, s0 + z);
  if ((int)blockIdx.x * 256 >= s.nq || s.nt == 0) return;          // (uniform over the workgroup)
  const size_t pair = (size_t)f * b.chunk + z;
  bool ok = false;
  if (i < s.nq) {
    const unsigned long long* t2 = b.top2 + (pair * a.cap + i) * 2;
    float d;
    ok = mf_row_ok(t2[0], t2[1], i, a.cross_check ? b.colbest + pair * b.rows : nullptr, max_dist, ratio, d);
  }
  const int cnt = __popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (tot) atomicAdd(b.score + (size_t)f * b.slots + s0 + z, tot);
  }
}

// grid n, 256 threads
__global__ __launch_bounds__(256) void bank_select_kernel(const BankArgs b, int min_score, int32_t* score_out, int32_t* best_out) {
  __shared__ unsigned long long wmax[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  unsigned long long key = 0ull;                                    // (score << 32) | ~slot: larger score, then lower slot
  for (int sl = tid; sl < b.slots; sl += 256) {
    const int sc = b.score[(size_t)f * b.slots + sl];
    if (score_out) score_out[(size_t)f * b.slots + sl] = sc;
    const unsigned long long k = ((unsigned long long)(unsigned)sc << 32) | (unsigned)~sl;
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0) wmax[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) key = wmax[w] > key ? wmax[w] : key;
    const int sc = (int)(key >> 32);
    const int best = sc >= max(min_score, 1) ? (int)~(unsigned)(key & 0xffffffffu) : -1;
    b.best[f] = best;
    if (best_out) best_out[f] = best;
  }
}

}  // namespace fpc
