// Batched RANSAC homography estimation (fpc_ransac_homography / fpc_homography_frames; the rule is stated in
// include/fpc.h and restated in float64 by tests/test_homography_ransac.py).
//
//   hf_pack_kernel / hf_gather_kernel   build every frame's pair list [x, y, u, v] (float32, 16-byte records), the row of
//                          the caller's mask each pair belongs to, the pair count, and zero the best key and the mask.
//                          The gather is an order-preserving compaction (ballot + popcount prefix, no atomics), so the
//                          list is in ascending row order; from here on both entry points run the same kernels on the
//                          same records, which is what makes them bit-identical on equal pairs.
//   ransac_score_kernel    grid ceil(T / 256) x n, one thread per hypothesis: draws its 4 pairs, solves the 4-point
//                          homography in fp64 registers (closed form through the projective basis: cross products and
//                          adjugates, no pivoting, no division), keeps it in 9 fp32 VGPRs and walks the pair list, which
//                          is staged through LDS in chunks -- every lane reads the same 16-byte record (the broadcast
//                          case, conflict-free).  The best (count, lowest t) per frame is a 64-bit atomicMax on
//                          (count << 32) | ~t: integer keys, so the result does not depend on the execution order.
//   ransac_refit_kernel    one workgroup per frame: re-derives the best sample's H, then `refits` times a Hartley-
//                          normalised least-squares fit over the current inliers -- moments and normal equations
//                          accumulated in fp64 per thread over a fixed stride and summed by a fixed-shape butterfly /
//                          4-wave tree (no floating-point atomics), solved by one lane in LDS -- and writes H, the
//                          inlier count and the mask of the H it returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int HF_MAX_ITERATIONS = 4096;
constexpr int HF_DRAWS = 16;          // draw budget of one sample
constexpr int HF_CHUNK = 1024;        // records staged per LDS chunk (16 KiB)
constexpr double HF_COLLINEAR = 0.5;  // doubled triangle area (px^2) below which three points count as collinear

struct HfArgs {
  float4* pairs;                // [B][cap]  x, y (query / src), u, v (train / dst)
  int32_t* row;                 // [B][cap]  the mask row of pair k
  int32_t* np;                  // [B]       pairs of the frame
  unsigned long long* best;     // [B]       (inlier count << 32) | ~t of the best hypothesis; 0: none
  int cap, n;
  int T, refits, min_inliers;
  float thr;
  uint32_t seed;
  // fpc_homography_bank_topk (match_bank_topk.h): the grid's index is a PROBLEM p = f per_frame + j, several per frame; it
  // selects the pair list, the mask row and the slot, while the frame f = p / per_frame selects the query pixels and feeds
  // the sampler.  0 (every other entry point): one problem per frame, p = f.
  int per_frame;
};

__device__ __forceinline__ int hf_frame(const HfArgs& a, int p) { return a.per_frame > 1 ? p / a.per_frame : p; }

__device__ __forceinline__ int hf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the sampler of include/fpc.h
__device__ __forceinline__ uint32_t hf_mix(uint32_t a) {
  a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15; a *= 0x846ca68bu; a ^= a >> 16;
  return a;
}
__device__ __forceinline__ bool hf_sample(uint32_t seed, uint32_t f, uint32_t t, uint32_t M, uint32_t& i0, uint32_t& i1,
                                          uint32_t& i2, uint32_t& i3) {
  i0 = i1 = i2 = i3 = M;
  int got = 0;
  for (uint32_t k = 0; k < (uint32_t)HF_DRAWS && got < 4; ++k) {
    const uint32_t r = hf_mix(seed ^ hf_mix((f * (uint32_t)HF_MAX_ITERATIONS + t) * (uint32_t)HF_DRAWS + k)) % M;
    const bool fresh = r != i0 && r != i1 && r != i2;           // (selects, not an indexed store: that becomes scratch)
    i0 = (fresh && got == 0) ? r : i0;
    i1 = (fresh && got == 1) ? r : i1;
    i2 = (fresh && got == 2) ? r : i2;
    i3 = (fresh && got == 3) ? r : i3;
    got += fresh ? 1 : 0;
  }
  return got == 4;
}
// ... and of the 8-point (fundamental) and 6-point (PnP) solvers: the first N distinct of DRAWS draws (selects, not an indexed
// store: that becomes scratch)
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

struct HfV3 { double x, y, z; };
__device__ __forceinline__ HfV3 hf_cross(const HfV3& a, const HfV3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double hf_dot(const HfV3& a, const HfV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ HfV3 hf_scale(const HfV3& a, double s) { return {a.x * s, a.y * s, a.z * s}; }

// The homography through 4 pairs.  With p_i = (x_i, y_i, 1): l_i = the triple products (p_j x p_k) . p_3, A = [l_0 p_0,
// l_1 p_1, l_2 p_2] maps the projective basis to the src points ((1,1,1) -> det(p_0 p_1 p_2) p_3), B likewise for dst,
// H = B adj(A).  The four triple products of a side are the doubled areas of its four triangles: the collinearity test.
// H is scaled to max |h| = 1 and oriented so that w > 0 at the sample's first point.  false: degenerate.
__device__ __forceinline__ bool hf_solve4(const float4& r0, const float4& r1, const float4& r2, const float4& r3,
                                          double (&H)[9]) {
  const HfV3 p0{r0.x, r0.y, 1.0}, p1{r1.x, r1.y, 1.0}, p2{r2.x, r2.y, 1.0}, p3{r3.x, r3.y, 1.0};
  const HfV3 q0{r0.z, r0.w, 1.0}, q1{r1.z, r1.w, 1.0}, q2{r2.z, r2.w, 1.0}, q3{r3.z, r3.w, 1.0};
  const HfV3 c12 = hf_cross(p1, p2), c20 = hf_cross(p2, p0), c01 = hf_cross(p0, p1);
  const double l0 = hf_dot(c12, p3), l1 = hf_dot(c20, p3), l2 = hf_dot(c01, p3), dp = hf_dot(c01, p2);
  const double m0 = hf_dot(hf_cross(q1, q2), q3), m1 = hf_dot(hf_cross(q2, q0), q3), m2 = hf_dot(hf_cross(q0, q1), q3);
  const double dq = hf_dot(hf_cross(q0, q1), q2);
  if (!(fabs(l0) >= HF_COLLINEAR && fabs(l1) >= HF_COLLINEAR && fabs(l2) >= HF_COLLINEAR && fabs(dp) >= HF_COLLINEAR &&
        fabs(m0) >= HF_COLLINEAR && fabs(m1) >= HF_COLLINEAR && fabs(m2) >= HF_COLLINEAR && fabs(dq) >= HF_COLLINEAR))
    return false;
  const HfV3 a0 = hf_scale(c12, l1 * l2), a1 = hf_scale(c20, l2 * l0), a2 = hf_scale(c01, l0 * l1);   // rows of adj(A)
  const HfV3 b0 = hf_scale(q0, m0), b1 = hf_scale(q1, m1), b2 = hf_scale(q2, m2);                      // columns of B
  H[0] = b0.x * a0.x + b1.x * a1.x + b2.x * a2.x; H[1] = b0.x * a0.y + b1.x * a1.y + b2.x * a2.y; H[2] = b0.x * a0.z + b1.x * a1.z + b2.x * a2.z;
  H[3] = b0.y * a0.x + b1.y * a1.x + b2.y * a2.x; H[4] = b0.y * a0.y + b1.y * a1.y + b2.y * a2.y; H[5] = b0.y * a0.z + b1.y * a1.z + b2.y * a2.z;
  H[6] = b0.z * a0.x + b1.z * a1.x + b2.z * a2.x; H[7] = b0.z * a0.y + b1.z * a1.y + b2.z * a2.y; H[8] = b0.z * a0.z + b1.z * a1.z + b2.z * a2.z;
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) mx = fmax(mx, fabs(H[i]));
  if (!(mx > 0.0) || !(mx < 1e300)) return false;         // (NaN fails the first test, Inf the second)
  const double w0 = H[6] * p0.x + H[7] * p0.y + H[8];
  const double s = (w0 < 0.0 ? -1.0 : 1.0) / mx;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    H[i] *= s;
    finite = finite && (fabs(H[i]) <= 1.0);               // (false for NaN)
  }
  return finite && fabs(H[8]) > 1e-12;                     // H must be expressible with H[8] = 1
}

// ---- pair lists -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hf_pack_kernel(HfArgs a, const float* __restrict__ src, const float* __restrict__ dst,
                                                      const int32_t* __restrict__ npairs, int stride, uint8_t* mask) {
  const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  const int M = hf_clamp(npairs[f], stride);
  if (k == 0) {
    a.np[f] = M;
    a.best[f] = 0ull;
  }
  if (k >= stride) return;
  if (mask) mask[(size_t)f * stride + k] = 0;
  if (k < M) {
    const size_t i = ((size_t)f * stride + k) * 2;
    a.pairs[(size_t)f * a.cap + k] = make_float4(src[i], src[i + 1], dst[i], dst[i + 1]);
    a.row[(size_t)f * a.cap + k] = k;
  }
}

// fpc_homography_bank: frame f's train coordinates are slot slot[f] of a key-frame bank (xy [slots][rows][2] passed as
// key_xy, count [slots]); a slot outside [0, slots) leaves the frame without pairs.  All null / 0 in fpc_homography_frames.
struct HfBank {
  const int32_t* slot;          // [n] device
  const int32_t* count;         // [slots]
  int rows, slots;
};

// one workgroup per frame (per problem: HfArgs::per_frame); rows i < count[f] with 0 <= match < the train set's row count,
// in ascending i
__global__ __launch_bounds__(256) void hf_gather_kernel(HfArgs a, const int32_t* __restrict__ xy, const int32_t* __restrict__ count,
                                                        int pairing, const int32_t* __restrict__ key_xy,
                                                        const int32_t* __restrict__ nkey, const int32_t* __restrict__ match,
                                                        uint8_t* mask, const HfBank bank) {
  __shared__ int wsum[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cap = a.cap;
  const int fq = hf_frame(a, f);               // the frame whose keypoints are the query side
  const int cnt = hf_clamp(count[fq], cap);
  const int32_t* txy = nullptr;
  int nt = 0;
  if (bank.slot) {                            // a per-frame train table: slot bank.slot[f] of key_xy [slots][rows][2]
    const int sl = bank.slot[f];
    if (sl >= 0 && sl < bank.slots) {
      txy = key_xy + (size_t)sl * bank.rows * 2;
      nt = hf_clamp(bank.count[sl], bank.rows);
    }
  } else if (pairing == 1 && f > 0) {
    txy = xy + (size_t)(f - 1) * cap * 2;
    nt = hf_clamp(count[f - 1], cap);
  } else if (key_xy) {
    txy = key_xy;
    nt = hf_clamp(nkey[0], cap);
  }
  const int32_t* qxy = xy + (size_t)fq * cap * 2;
  const int end = mask ? cap : cnt;
  int base = 0;
  for (int i0 = 0; i0 < end; i0 += 256) {
    const int i = i0 + tid;
    int m = -1;
    if (i < cnt) m = match[(size_t)f * cap + i];
    const bool flag = m >= 0 && m < nt;
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
    if (flag) {
      a.pairs[(size_t)f * cap + off] = make_float4((float)qxy[2 * i], (float)qxy[2 * i + 1], (float)txy[2 * m], (float)txy[2 * m + 1]);
      a.row[(size_t)f * cap + off] = i;
    }
  }
  if (tid == 0) {
    a.np[f] = base;
    a.best[f] = 0ull;
  }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ransac_score_kernel(HfArgs a) {
  __shared__ float4 rec[HF_CHUNK];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  if (M < 4) return;
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const uint32_t t = blockIdx.x * 256u + tid;
  float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f, h5 = 0.f, h6 = 0.f, h7 = 0.f, h8 = 0.f;
  bool ok = t < (uint32_t)a.T;
  if (ok) {
    uint32_t i0, i1, i2, i3;
    ok = hf_sample(a.seed, (uint32_t)hf_frame(a, f), t, (uint32_t)M, i0, i1, i2, i3);
    if (ok) {
      double H[9];
      ok = hf_solve4(pairs[i0], pairs[i1], pairs[i2], pairs[i3], H);
      if (ok) {
        h0 = (float)H[0]; h1 = (float)H[1]; h2 = (float)H[2]; h3 = (float)H[3]; h4 = (float)H[4];
        h5 = (float)H[5]; h6 = (float)H[6]; h7 = (float)H[7]; h8 = (float)H[8];
      }
    }
  }
  // (a degenerate hypothesis keeps H = 0: w = 0 is never > 0, it counts nothing)
  const float thr = a.thr;
  int cnt = 0;
  for (int c0 = 0; c0 < M; c0 += HF_CHUNK) {
    const int m = min(HF_CHUNK, M - c0);
    __syncthreads();
    for (int i = tid; i < m; i += 256) rec[i] = pairs[c0 + i];
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < m; ++k) {
      const float4 p = rec[k];
      const float w = fmaf(h7, p.y, fmaf(h6, p.x, h8));
      const float ex = fmaf(-w, p.z, fmaf(h1, p.y, fmaf(h0, p.x, h2)));
      const float ey = fmaf(-w, p.w, fmaf(h4, p.y, fmaf(h3, p.x, h5)));
      const float tw = thr * w;
      cnt += (w > 0.f && fmaf(ex, ex, ey * ey) < tw * tw) ? 1 : 0;
    }
  }
  unsigned long long key = (ok && cnt > 0) ? (((unsigned long long)(uint32_t)cnt << 32) | (unsigned long long)(~t)) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0 && key) atomicMax(a.best + f, key);
}

// ---- refit ------------------------------------------------------------------------------------------------------------
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

// |H p - q| < thr without the division, in fp64 (sign-free: the plain reprojection test of include/fpc.h)
__device__ __forceinline__ bool hf_inlier(const double (&H)[9], const float4& p, double thr2) {
  const double x = p.x, y = p.y;
  const double w = H[6] * x + H[7] * y + H[8];
  const double ex = H[0] * x + H[1] * y + H[2] - w * (double)p.z, ey = H[3] * x + H[4] * y + H[5] - w * (double)p.w;
  return ex * ex + ey * ey < thr2 * w * w;
}

constexpr int HF_NSUM = 23;

__global__ __launch_bounds__(256) void ransac_refit_kernel(HfArgs a, float* __restrict__ Hout, int32_t* __restrict__ ninl,
                                                           uint8_t* mask, int mstride) {
  __shared__ double red[4 * HF_NSUM];
  __shared__ double sm[8][9];
  __shared__ double hnew[9];
  __shared__ int solved;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = hf_clamp(a.np[f], a.cap);
  const unsigned long long key = a.best[f];
  const float4* __restrict__ pairs = a.pairs + (size_t)f * a.cap;
  const double thr2 = (double)a.thr * (double)a.thr;
  double H[9];
  bool ok = M >= 4 && key != 0ull;
  if (ok) {                                   // (uniform) every thread re-derives the best sample's H: same code, same bits
    uint32_t i0, i1, i2, i3;
    ok = hf_sample(a.seed, (uint32_t)hf_frame(a, f), ~(uint32_t)key, (uint32_t)M, i0, i1, i2, i3) &&
         hf_solve4(pairs[i0], pairs[i1], pairs[i2], pairs[i3], H);
  }
  int total = 0;
  if (ok) {
    const double inv = 1.0 / H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = (double)(float)(H[i] * inv);        // the H that would be returned: fp32 values
    H[8] = 1.0;
    for (int r = 0; r < a.refits; ++r) {
      // normalisation moments of the inlier set: n, sum x, y, x^2 + y^2, u, v, u^2 + v^2
      double mo[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int k = tid; k < M; k += 256) {
        const float4 p = pairs[k];
        if (hf_inlier(H, p, thr2)) {
          const double x = p.x, y = p.y, u = p.z, v = p.w;
          mo[0] += 1.0; mo[1] += x; mo[2] += y; mo[3] += x * x + y * y; mo[4] += u; mo[5] += v; mo[6] += u * u + v * v;
        }
      }
      hf_block_sum<7>(mo, red);
      if (mo[0] < 4.0) break;
      const double cx = mo[1] / mo[0], cy = mo[2] / mo[0], cu = mo[4] / mo[0], cv = mo[5] / mo[0];
      const double vs = mo[3] / mo[0] - cx * cx - cy * cy, vd = mo[6] / mo[0] - cu * cu - cv * cv;
      if (!(vs > 1e-12) || !(vd > 1e-12)) break;
      const double ss = sqrt(2.0 / vs), sd = sqrt(2.0 / vd);              // RMS distance to the centroid -> sqrt(2)
      // normal equations of [x y 1 0 0 0 -ux -uy | u], [0 0 0 x y 1 -vx -vy | v] in the normalised coordinates
      double s[HF_NSUM];
#pragma unroll
      for (int i = 0; i < HF_NSUM; ++i) s[i] = 0.0;
      for (int k = tid; k < M; k += 256) {
        const float4 p = pairs[k];
        if (hf_inlier(H, p, thr2)) {
          const double x = ((double)p.x - cx) * ss, y = ((double)p.y - cy) * ss;
          const double u = ((double)p.z - cu) * sd, v = ((double)p.w - cv) * sd;
          const double xx = x * x, xy = x * y, yy = y * y, w2 = u * u + v * v;
          s[0] += xx; s[1] += xy; s[2] += yy; s[3] += x; s[4] += y; s[5] += 1.0;
          s[6] += u * xx; s[7] += u * xy; s[8] += u * yy; s[9] += u * x; s[10] += u * y; s[11] += u;
          s[12] += v * xx; s[13] += v * xy; s[14] += v * yy; s[15] += v * x; s[16] += v * y; s[17] += v;
          s[18] += w2 * xx; s[19] += w2 * xy; s[20] += w2 * yy; s[21] += w2 * x; s[22] += w2 * y;
        }
      }
      hf_block_sum<HF_NSUM>(s, red);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 9; ++j) sm[i][j] = 0.0;
        sm[0][0] = s[0]; sm[0][1] = s[1]; sm[0][2] = s[3]; sm[0][6] = -s[6]; sm[0][7] = -s[7]; sm[0][8] = s[9];
        sm[1][1] = s[2]; sm[1][2] = s[4]; sm[1][6] = -s[7]; sm[1][7] = -s[8]; sm[1][8] = s[10];
        sm[2][2] = s[5]; sm[2][6] = -s[9]; sm[2][7] = -s[10]; sm[2][8] = s[11];
        sm[3][3] = s[0]; sm[3][4] = s[1]; sm[3][5] = s[3]; sm[3][6] = -s[12]; sm[3][7] = -s[13]; sm[3][8] = s[15];
        sm[4][4] = s[2]; sm[4][5] = s[4]; sm[4][6] = -s[13]; sm[4][7] = -s[14]; sm[4][8] = s[16];
        sm[5][5] = s[5]; sm[5][6] = -s[15]; sm[5][7] = -s[16]; sm[5][8] = s[17];
        sm[6][6] = s[18]; sm[6][7] = s[19]; sm[6][8] = -s[21];
        sm[7][7] = s[20]; sm[7][8] = -s[22];
        for (int i = 1; i < 8; ++i)
          for (int j = 0; j < i; ++j) sm[i][j] = sm[j][i];
        // Gaussian elimination with partial pivoting, in LDS (dynamic indices must not become scratch)
        int good = 1;
        const double tiny = 1e-10 * s[5];
        for (int c = 0; c < 8 && good; ++c) {
          int pr = c;
          double pv = fabs(sm[c][c]);
          for (int i = c + 1; i < 8; ++i) {
            const double v = fabs(sm[i][c]);
            if (v > pv) { pv = v; pr = i; }
          }
          if (!(pv > tiny)) { good = 0; break; }
          if (pr != c)
            for (int j = c; j < 9; ++j) { const double tmp = sm[c][j]; sm[c][j] = sm[pr][j]; sm[pr][j] = tmp; }
          const double ip = 1.0 / sm[c][c];
          for (int i = c + 1; i < 8; ++i) {
            const double fct = sm[i][c] * ip;
            for (int j = c; j < 9; ++j) sm[i][j] -= fct * sm[c][j];
          }
        }
        if (good) {
          for (int i = 7; i >= 0; --i) {
            double acc = sm[i][8];
            for (int j = i + 1; j < 8; ++j) acc -= sm[i][j] * sm[j][8];
            sm[i][8] = acc / sm[i][i];
          }
          const double n0 = sm[0][8], n1 = sm[1][8], n2 = sm[2][8], n3 = sm[3][8], n4 = sm[4][8], n5 = sm[5][8],
                       n6 = sm[6][8], n7 = sm[7][8];
          // H = Td^-1 Hn Ts,  Ts = [ss 0 -ss cx; 0 ss -ss cy; 0 0 1],  Td^-1 = [1/sd 0 cu; 0 1/sd cv; 0 0 1]
          const double m00 = n0 * ss, m01 = n1 * ss, m02 = n2 - ss * (cx * n0 + cy * n1);
          const double m10 = n3 * ss, m11 = n4 * ss, m12 = n5 - ss * (cx * n3 + cy * n4);
          const double m20 = n6 * ss, m21 = n7 * ss, m22 = 1.0 - ss * (cx * n6 + cy * n7);
          const double isd = 1.0 / sd;
          const double g0 = m00 * isd + cu * m20, g1 = m01 * isd + cu * m21, g2 = m02 * isd + cu * m22;
          const double g3 = m10 * isd + cv * m20, g4 = m11 * isd + cv * m21, g5 = m12 * isd + cv * m22;
          double mx = fmax(fmax(fmax(fabs(g0), fabs(g1)), fmax(fabs(g2), fabs(g3))), fmax(fmax(fabs(g4), fabs(g5)), fmax(fabs(m20), fabs(m21))));
          mx = fmax(mx, fabs(m22));
          if (!(mx < 1e300) || !(fabs(m22) > 1e-12 * mx)) good = 0;
          else {
            const double i22 = 1.0 / m22;
            hnew[0] = (double)(float)(g0 * i22); hnew[1] = (double)(float)(g1 * i22); hnew[2] = (double)(float)(g2 * i22);
            hnew[3] = (double)(float)(g3 * i22); hnew[4] = (double)(float)(g4 * i22); hnew[5] = (double)(float)(g5 * i22);
            hnew[6] = (double)(float)(m20 * i22); hnew[7] = (double)(float)(m21 * i22); hnew[8] = 1.0;
            for (int i = 0; i < 8; ++i)
              if (!(fabs(hnew[i]) < 3e38)) good = 0;
          }
        }
        solved = good;
      }
      __syncthreads();
      if (!solved) break;                                                   // a singular system keeps the previous H
#pragma unroll
      for (int i = 0; i < 9; ++i) H[i] = hnew[i];
    }
    double c1[1] = {0.0};
    for (int k = tid; k < M; k += 256) c1[0] += hf_inlier(H, pairs[k], thr2) ? 1.0 : 0.0;
    hf_block_sum<1>(c1, red);
    total = (int)c1[0];
    ok = total >= a.min_inliers;
  }
  if (ok && mask)                                                           // (the pack / gather kernel zeroed the mask)
    for (int k = tid; k < M; k += 256)
      if (hf_inlier(H, pairs[k], thr2)) mask[(size_t)f * mstride + a.row[(size_t)f * a.cap + k]] = 1;
  __syncthreads();
  if (tid == 0) {                                                           // (through LDS: H[tid] would be scratch)
#pragma unroll
    for (int i = 0; i < 9; ++i) hnew[i] = ok ? H[i] : 0.0;
    ninl[f] = ok ? total : 0;
  }
  __syncthreads();
  if (tid < 9) Hout[f * 9 + tid] = (float)hnew[tid];
}
