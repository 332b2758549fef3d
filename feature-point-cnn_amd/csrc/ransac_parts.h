// The model-free parts of the three RANSAC kernel families (ransac_homography.h, ransac_fundamental.h, pnp_ransac.h), each
// written once.  A family's header holds its model -- the minimal solver, the refit's sums and solve, the inlier tests --
// and builds its kernels from:
//
//   hf_mix / hf_sample_distinct   the sampler of include/fpc.h: the first N distinct of DRAWS hashed draws.
//   hf_clamp, hf_frame, hf_block_sum   clamped counts, the frame of a problem, the fixed-shape workgroup sum.
//   hf_vote           the selection: (count << 32) | ~t, its wave maximum, one 64-bit atomicMax per wave.
//   solve_lds         partial-pivot elimination of an N x (N + 1) system in LDS (the homography's and the pose's refits).
//   hartley_moments   a refit's first pass: the inliers' moments -> the Hartley normalisation of both sides (FmNorm).
//   gather_body       the order-preserving compaction behind hf_gather_kernel / pnp_gather_kernel (ballot + popcount
//                     prefix, no atomics); a Source says which rows are pairs and writes their records.
//   score_body        a score kernel: sample, solve, walk the pair list through LDS in HF_CHUNK-record chunks, count, vote;
//                     a Model says how to solve a sample into fp32 registers and whether a record counts.
//   refit_head / refit_tail   a refit kernel's ends: one lane re-derives the best sample's model, the others wait; the final
//                     count, the min_inliers test, the mask over the pairs' rows and the count's write.
//
// Nothing here indexes a register array dynamically (that becomes scratch): loops over registers are fully unrolled, and
// whatever needs a dynamic index lives in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int HF_MAX_ITERATIONS = 4096;
constexpr int HF_CHUNK = 1024;        // records staged per LDS chunk of a score kernel

__device__ __forceinline__ int hf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the frame of problem p (HfArgs::per_frame problems per frame; 0: one, p itself)
__device__ __forceinline__ int hf_frame(int per_frame, int p) { return per_frame > 1 ? p / per_frame : p; }

// the sampler of include/fpc.h: the first N distinct of DRAWS draws (selects, not an indexed store: that becomes scratch)
__device__ __forceinline__ uint32_t hf_mix(uint32_t a) {
  a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
  return a;
}
template <int N, int DRAWS>
__device__ __forceinline__ bool hf_sample_distinct(uint32_t seed, uint32_t f, uint32_t t, uint32_t M, uint32_t (&idx)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) idx[j] = M;
  int got = 0;
  for (uint32_t k = 0; k < (uint32_t)DRAWS && got < N; ++k) {
    const uint32_t r = hf_mix(seed ^ hf_mix((f * (uint32_t)HF_MAX_ITERATIONS + t) * (uint32_t)DRAWS + k)) % M;
    bool fresh = true;
#pragma unroll
    for (int j = 0; j < N; ++j) fresh = fresh && r != idx[j];
#pragma unroll
    for (int j = 0; j < N; ++j) idx[j] = (fresh && got == j) ? r : idx[j];
    got += fresh ? 1 : 0;
  }
  return got == N;
}

// Sum of every thread's v[i] over the workgroup (256 threads), the same in every thread: xor butterfly inside a wave, then
// the four waves' sums in wave order.
template <int N>
__device__ __forceinline__ void hf_block_sum(double (&v)[N], double* red /* [4][N] */) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = v[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    v[i] = x;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[(threadIdx.x >> 6) * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
}

// The best (count, lowest t) of a problem: a 64-bit maximum over (count << 32) | ~t -- inside the wave by xor butterfly, then
// one atomicMax per wave.  Integer keys, so the result does not depend on the execution order; 0: no hypothesis.
__device__ __forceinline__ void hf_vote(unsigned long long* best, bool ok, int cnt, uint32_t t) {
  unsigned long long key = (ok && cnt > 0) ? (((unsigned long long)(uint32_t)cnt << 32) | (unsigned long long)(~t)) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// Gaussian elimination with partial pivoting and back-substitution of the N x (N + 1) system sm (LDS: dynamic indices must
// not become scratch); the solution replaces the last column.  false: a pivot at or below `tiny`.  One lane.
template <int N>
__device__ __forceinline__ bool solve_lds(double (*sm)[N + 1], double tiny) {
#pragma unroll 1
  for (int c = 0; c < N; ++c) {
    int pr = c;
    double pv = fabs(sm[c][c]);
    for (int i = c + 1; i < N; ++i) {
      const double v = fabs(sm[i][c]);
      if (v > pv) { pv = v; pr = i; }
    }
    if (!(pv > tiny)) return false;
    if (pr != c)
      for (int j = c; j <= N; ++j) { const double tmp = sm[c][j]; sm[c][j] = sm[pr][j]; sm[pr][j] = tmp; }
    const double ip = 1.0 / sm[c][c];
    for (int i = c + 1; i < N; ++i) {
      const double fct = sm[i][c] * ip;
      for (int j = c; j <= N; ++j) sm[i][j] -= fct * sm[c][j];
    }
  }
  for (int i = N - 1; i >= 0; --i) {
    double acc = sm[i][N];
    for (int j = i + 1; j < N; ++j) acc -= sm[i][j] * sm[j][N];
    sm[i][N] = acc / sm[i][i];
  }
  return true;
}

// Hartley normalisation of a pair list's two sides: centroid and the scale that brings the RMS distance to sqrt(2)
struct FmNorm { double cx, cy, ss, cu, cv, sd; };

// A refit's first pass over the M pairs [x, y, u, v] (workgroup of 256): the moments n, sum x, y, x^2 + y^2, u, v, u^2 + v^2
// of the pairs `inlier` accepts, in fp64 per thread over a fixed stride and through hf_block_sum -> their normalisation.
// false (uniform): fewer than min_count inliers, or a side without spread.
template <class Inlier>
__device__ __forceinline__ bool hartley_moments(const float4* __restrict__ pairs, int M, double min_count, double* red,
                                                Inlier inlier, FmNorm& w) {
  double mo[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < M; k += 256) {
    const float4 p = pairs[k];
    if (inlier(p)) {
      const double x = p.x, y = p.y, u = p.z, v = p.w;
      mo[0] += 1.0; mo[1] += x; mo[2] += y; mo[3] += x * x + y * y; mo[4] += u; mo[5] += v; mo[6] += u * u + v * v;
    }
  }
  hf_block_sum<7>(mo, red);
  if (mo[0] < min_count) return false;
  w.cx = mo[1] / mo[0]; w.cy = mo[2] / mo[0]; w.cu = mo[4] / mo[0]; w.cv = mo[5] / mo[0];
  const double vs = mo[3] / mo[0] - w.cx * w.cx - w.cy * w.cy, vd = mo[6] / mo[0] - w.cu * w.cu - w.cv * w.cv;
  if (!(vs > 1e-12) || !(vd > 1e-12)) return false;
  w.ss = sqrt(2.0 / vs); w.sd = sqrt(2.0 / vd);                            // RMS distance to the centroid -> sqrt(2)
  return true;
}

// ---- pair lists -------------------------------------------------------------------------------------------------------
// One workgroup of 256 compacts the rows i < cnt of problem f that are pairs, in ascending i: ballot, popcount prefix inside
// the wave, the four waves' counts through LDS -- no atomics, so the list's order is the rows'.  Zeroes the caller's mask
// (all `cap` rows) on the way and, at the end, writes the pair count and resets the best key.
//   src.pair(m)          is a row whose match is m a pair?  (may load and keep the train side's data)
//   src.write(off, i, m) record `off` of the list: row i with its match m
template <class Source>
__device__ __forceinline__ void gather_body(Source& src, int f, int cnt, int cap, const int32_t* __restrict__ match,
                                            uint8_t* mask, int32_t* np, unsigned long long* best) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int end = mask ? cap : cnt;
  int base = 0;
  for (int i0 = 0; i0 < end; i0 += 256) {
    const int i = i0 + tid;
    int m = -1;
    if (i < cnt) m = match[(size_t)f * cap + i];
    const bool flag = src.pair(m);
    if (mask && i < cap) mask[(size_t)f * cap + i] = 0;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int off = base + before;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) off += wsum[w];
      base += wsum[w];
    }
    if (flag) src.write(off, i, m);
  }
  if (tid == 0) {
    np[f] = base;
    best[f] = 0ull;
  }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
// A score kernel's body: grid ceil(T / THREADS) x problems, one thread per hypothesis t.  The thread draws its sample, the
// Model solves it (in fp64; `sys`: the workgroup's struct-of-arrays LDS systems, if it needs them) into fp32 registers, and
// every thread walks the pair list, staged through LDS (`stage`, which may be the systems' memory: they are dead by then)
// in HF_CHUNK-record chunks between two barriers -- every lane reads the same record, the broadcast case.  A degenerate
// hypothesis keeps its zero registers, with which no record counts; such lanes, and the lanes with t >= T of the last
// workgroup, still stage records and meet the barriers.
//   Model::SAMPLE, Model::DRAWS   the sample's size and draw budget;  Model::REC   float4 per record
//   Model(a)                      zero registers, the threshold
//   Model::records(a, f), Model::frame(a, f)   problem f's pair list, and the frame that keys its sampler
//   m.solve(a, rec, idx, sys)     the sample -> the registers; false: degenerate
//   m.counts(r)                   does the record at r (LDS) count?
template <int THREADS, class Model, class Args>
__device__ __forceinline__ void score_body(const Args& a, float4* stage, double* sys) {
  const int f = blockIdx.y, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  if (M < Model::SAMPLE) return;
  const float4* __restrict__ rec = Model::records(a, f);
  const uint32_t t = blockIdx.x * (uint32_t)THREADS + tid;
  Model m(a);
  bool ok = t < (uint32_t)a.T;
  if (ok) {
    uint32_t idx[Model::SAMPLE];
    ok = hf_sample_distinct<Model::SAMPLE, Model::DRAWS>(a.seed, (uint32_t)Model::frame(a, f), t, (uint32_t)M, idx) &&
         m.solve(a, rec, idx, sys);
  }
  int cnt = 0;
  for (int c0 = 0; c0 < M; c0 += HF_CHUNK) {
    const int n = min(HF_CHUNK, M - c0);
    __syncthreads();
    for (int i = tid; i < Model::REC * n; i += THREADS) stage[i] = rec[Model::REC * c0 + i];
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < n; ++k) cnt += m.counts(stage + Model::REC * k) ? 1 : 0;
  }
  hf_vote(a.best + f, ok, cnt, t);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
// (uniform ok) One lane re-derives the best sample's model with the score kernel's own device functions -- same code, same
// bits -- and leaves it in LDS; the others wait for its verdict.
template <class Derive>
__device__ __forceinline__ bool refit_head(bool ok, int* solved, Derive derive) {
  if (ok) {
    if (threadIdx.x == 0) *solved = derive() ? 1 : 0;
    __syncthreads();
    ok = *solved != 0;
  }
  return ok;
}

// (uniform ok) The end of a refit kernel (workgroup of 256): the returned model's inliers among the M pairs, counted through
// hf_block_sum<1> (0 / 1 doubles: exact); fewer than min_inliers fail the problem.  Sets the mask (zeroed by the pack /
// gather kernel) at the inliers' rows, writes the count (0 on failure) and returns ok, behind a barrier.
//   inlier(k)   the model's fp64 test of pair k;   row(k)   the index of pair k's row in the mask
template <class Inlier, class Row>
__device__ __forceinline__ bool refit_tail(bool ok, int M, int min_inliers, double* red, uint8_t* mask, int32_t* ninl,
                                           Inlier inlier, Row row) {
  int total = 0;
  if (ok) {
    double c1[1] = {0.0};
    for (int k = threadIdx.x; k < M; k += 256) c1[0] += inlier(k) ? 1.0 : 0.0;
    hf_block_sum<1>(c1, red);
    total = (int)c1[0];
    ok = total >= min_inliers;
  }
  if (ok && mask)
    for (int k = threadIdx.x; k < M; k += 256)
      if (inlier(k)) mask[row(k)] = 1;
  __syncthreads();
  if (threadIdx.x == 0) *ninl = ok ? total : 0;
  return ok;
}
