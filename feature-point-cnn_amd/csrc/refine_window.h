// Local bundle adjustment of one key frame's landmarks over up to 16 frames (fpc_refine_window / fpc_refine_window_frames /
// fpc_refine_window_bank; the rule is stated in include/fpc.h and restated in float64 by tests/test_refine_window.py).
// hf_clamp and solve_lds' shape are ransac_parts.h's, rp_invert is refine_pose.h's, lm_reprojects and pnp_finite3 are
// landmarks.h's / pnp_ransac.h's.  One problem per call, so the work is spread over the LANDMARKS: chunks of RW_CHUNK = 64
// key rows, one workgroup each, and one-workgroup kernels wherever the chunks meet.  The state of the iteration is the
// caller's xyz (fp32 points, by key row) and RwState (fp32 poses); everything else lives in the fpc_window_reserve
// reservation.  No workgroup ever waits on another: what joins the chunks is the next launch.
//
//   rw_init_kernel<Source>      the key's landmarks -> xyz, the key pixels, the eligible flags; the poses and the live flags
//   rw_members_kernel<Source>   every observation row that passes the member test: atomicMin of its row onto (frame, landmark)
//   rw_resolve_kernel<Source>   the pixel of every (frame, landmark)'s winning row; the frames' member counts (integer atomics)
//   rw_finish_kernel            kept frames, active landmarks, Z0; no kept frame -> the call has failed and stopped
//   rw_cost_kernel              C of the current state, or C' of the stepped one (with the gauge's s, formed by every
//                               workgroup from the same ascending sum): a partial per chunk, ascending inside the chunk
//   rw_decide_kernel            sums the partials in chunk order; accept / reject / stop; on accept the stepped state is copied
//   -- per attempt: build, solve, step, cost, decide; all five return at once when RwState::stopped is set --
//   rw_build_kernel             256 threads per chunk.  RW_SUB = 8 landmarks at a time: thread (l, f) stages frame f's blocks
//                               of landmark l in LDS (W, J_c, r, J_X^T J_X, J_X^T r), thread l sums U and g over the frames
//                               in ascending order and inverts U*, thread (l, f) forms Y = W U*^-1; then thread (fa, fb) adds
//                               -Y_fa W_fb^T (and on the diagonal J_c^T J_c, diag A and b) of the 8 landmarks, in order, onto
//                               the 6 x 6 block (fa, fb) it keeps in registers for the whole chunk.  The chunk's partial S, b
//                               and diag A go to the reservation.
//   rw_solve_kernel             one workgroup: the partials in chunk order -> the D x (D + 1) system of the kept frames in LDS
//                               (at most 96 x 97 doubles), damped; elimination with partial pivoting, a column at a time
//                               across the workgroup (the arithmetic of solve_lds, without contraction); one lane's back-
//                               substitution; a thread per kept frame steps its pose.
//   rw_step_kernel              a thread per landmark walks its frames in ascending order, rebuilding U, g and W^T delta, and
//                               writes the stepped point in fp64, before the gauge's scaling.
//   rw_final_kernel             kinds, culled points, the observation mask and counts, poses and stats.
#pragma once
#include "refine_pose.h"

constexpr int RW_FRAMES = 16;             // FPC_WINDOW_MAX_FRAMES
constexpr int RW_D = 6 * RW_FRAMES;
constexpr int RW_CHUNK = 64;              // key rows per workgroup
constexpr int RW_SUB = 8;                 // landmarks staged per pass of the build kernel
constexpr int RW_PART = RW_D * RW_D + 2 * RW_D;   // a chunk's partial: S [96][96] by frame, b [96], diag A [96]
constexpr int RW_NONE = 0x7f7f7f7f;       // no row of the observation table (what the table is cleared to, bytewise)
constexpr double RW_SINGULAR = 1e-14;     // pivot floor of the reduced solve, of the largest diagonal entry of S

struct RwState {
  double lambda, C, C0, Z0;
  double delta[RW_D];                     // the solution, by frame (zeros for the frames not kept)
  double tn[RW_FRAMES][3];                // E t + upsilon of the attempt, before the gauge's scaling
  float cur[RW_FRAMES][12];               // the state: R, t
  float nxtR[RW_FRAMES][9], nxtt[RW_FRAMES][3];   // the stepped poses, rounded
  int live[RW_FRAMES], kept[RW_FRAMES], cnt[RW_FRAMES];
  int stopped, failed, ok, made, accepted, members, active, nk, nkept;
};

struct RwArgs {
  float q_fx, q_fy, q_cx, q_cy, t_fx, t_fy, t_cx, t_cy, thr;
  int iterations;
  float lambda0;
  int min_obs;
  int n, cap, S;                          // frames, key rows of every per-landmark array, rows of a frame's observation list
  RwState* st;
  int32_t* tab;                           // [16][cap]: the member row of (frame, landmark), or RW_NONE
  float2* pix;                            // [16][cap]: its pixel
  float2* kpix;                           // [cap]: the key pixels
  uint8_t* lmk;                           // [cap]: 0 none, 1 active, 2 valid and not active, 3 eligible (until rw_finish_kernel)
  double* xd;                             // [cap][3]: the stepped points before the gauge's scaling
  float* xnew;                            // [cap][3]: the stepped points
  double* part;                           // [chunks][RW_PART]
  double* cpart;                          // [chunks]
  int32_t* bad;                           // [chunks]: a determinant that was not > 0
  float* xyz;                             // the caller's [cap][3]: the points of the state
};

// ---- the three observation sources ---------------------------------------------------------------------------------------
// fpc_refine_window: pair k < nobs_in[f] of the caller's arrays; the key set is the caller's too
struct RwExplicit {
  const float* xy; const int32_t* idx; const int32_t* nobs; int stride;
  const float* key_xy; const float* key_xyz; const uint8_t* key_valid; const int32_t* nkey; int cap;
  __device__ __forceinline__ int nk() const { return hf_clamp(nkey[0], cap); }
  __device__ __forceinline__ bool live(int) const { return true; }
  __device__ __forceinline__ bool key(int j, float& kx, float& ky, float& X, float& Y, float& Z) const {
    kx = key_xy[2 * (size_t)j]; ky = key_xy[2 * (size_t)j + 1];
    X = key_xyz[3 * (size_t)j]; Y = key_xyz[3 * (size_t)j + 1]; Z = key_xyz[3 * (size_t)j + 2];
    return (!key_valid || key_valid[j] != 0) && pnp_finite3(X, Y, Z);
  }
  __device__ __forceinline__ int rows(int f) const { return hf_clamp(nobs[f], stride); }
  __device__ __forceinline__ int landmark(int f, int k) const { return idx[(size_t)f * stride + k]; }
  __device__ __forceinline__ void pixel(int f, int k, float& px, float& py) const {
    px = xy[((size_t)f * stride + k) * 2]; py = xy[((size_t)f * stride + k) * 2 + 1];
  }
};

// the query side of the other two: row i < count[f] of the last detect's results with its match
struct RwFrames {
  const int32_t* xy; const int32_t* count; const int32_t* match; int cap;
  __device__ __forceinline__ int rows(int f) const { return hf_clamp(count[f], cap); }
  __device__ __forceinline__ int landmark(int f, int i) const { return match[(size_t)f * cap + i]; }
  __device__ __forceinline__ void pixel(int f, int i, float& px, float& py) const {
    px = (float)xy[((size_t)f * cap + i) * 2]; py = (float)xy[((size_t)f * cap + i) * 2 + 1];
  }
};

// fpc_refine_window_frames: one key set, fpc_landmarks_frames' arguments
struct RwKey {
  RwFrames q;
  const int32_t* key_xy; const float* key_xyz; const uint8_t* key_valid; const int32_t* nkey;
  __device__ __forceinline__ int nk() const { return hf_clamp(nkey[0], q.cap); }
  __device__ __forceinline__ bool live(int) const { return true; }
  __device__ __forceinline__ bool key(int j, float& kx, float& ky, float& X, float& Y, float& Z) const {
    kx = (float)key_xy[2 * (size_t)j]; ky = (float)key_xy[2 * (size_t)j + 1];
    X = key_xyz[3 * (size_t)j]; Y = key_xyz[3 * (size_t)j + 1]; Z = key_xyz[3 * (size_t)j + 2];
    return (!key_valid || key_valid[j] != 0) && pnp_finite3(X, Y, Z);
  }
  __device__ __forceinline__ int rows(int f) const { return q.rows(f); }
  __device__ __forceinline__ int landmark(int f, int i) const { return q.landmark(f, i); }
  __device__ __forceinline__ void pixel(int f, int i, float& px, float& py) const { q.pixel(f, i, px, py); }
};

// fpc_refine_window_bank: the key set is slot key_slot[0] of the bank (no rows with a slot outside [0, slots) or without
// landmark storage); frame f takes part iff slot is null or slot[f] is that slot
struct RwBank {
  RwFrames q;
  const int32_t* key_slot; const int32_t* slot;
  const int32_t* bank_xy; const int32_t* bank_count; const float4* bank_lm;
  int rows_, slots;
  __device__ __forceinline__ int nk() const {
    const int ks = key_slot[0];
    return (bank_lm && ks >= 0 && ks < slots) ? hf_clamp(bank_count[ks], rows_ < q.cap ? rows_ : q.cap) : 0;
  }
  __device__ __forceinline__ bool live(int f) const { return !slot || slot[f] == key_slot[0]; }
  __device__ __forceinline__ bool key(int j, float& kx, float& ky, float& X, float& Y, float& Z) const {   // (j < nk())
    const size_t o = (size_t)key_slot[0] * rows_ + j;
    kx = (float)bank_xy[2 * o]; ky = (float)bank_xy[2 * o + 1];
    const float4 p = bank_lm[o];
    X = p.x; Y = p.y; Z = p.z;
    return p.w != 0.f && pnp_finite3(p.x, p.y, p.z);
  }
  __device__ __forceinline__ int rows(int f) const { return q.rows(f); }
  __device__ __forceinline__ int landmark(int f, int i) const { return q.landmark(f, i); }
  __device__ __forceinline__ void pixel(int f, int i, float& px, float& py) const { q.pixel(f, i, px, py); }
};

// ---- per-member arithmetic: contraction off, so that the kernels that inline it compute the same bits ---------------------
// Y = R X + t with P = (R row-major, t)
__device__ __forceinline__ void rw_transform(const double* P, double X0, double X1, double X2, double& a, double& b, double& c) {
#pragma clang fp contract(off)
  a = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[9];
  b = P[3] * X0 + P[4] * X1 + P[5] * X2 + P[10];
  c = P[6] * X0 + P[7] * X1 + P[8] * X2 + P[11];
}

// |pi(Y) - p|^2 of a point (a, b, c) of a camera's frame; +inf with a depth that is not > 0
__device__ __forceinline__ double rw_cost_term(double fx, double fy, double cx, double cy, double px, double py, double a,
                                               double b, double c) {
#pragma clang fp contract(off)
  if (!(c > 0.0)) return __builtin_inf();
  const double e0 = fx * (a / c) + cx - px, e1 = fy * (b / c) + cy - py;
  return e0 * e0 + e1 * e1;
}

// the key camera's term of a landmark: U_k (symmetric: 00 01 02 11 12 22) and g_k
__device__ __forceinline__ void rw_key_blocks(double fx, double fy, double cx, double cy, double kx, double ky, double X0,
                                              double X1, double X2, double (&U)[6], double (&g)[3]) {
#pragma clang fp contract(off)
  const double iz = 1.0 / X2;
  const double r0 = fx * (X0 * iz) + cx - kx, r1 = fy * (X1 * iz) + cy - ky;
  const double J[6] = {fx * iz, 0.0, -fx * X0 * iz * iz, 0.0, fy * iz, -fy * X1 * iz * iz};
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) U[q++] = J[i] * J[j] + J[3 + i] * J[3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) g[j] = J[j] * r0 + J[3 + j] * r1;
}

// what an observation contributes: J_c (2 x 6), r, W = J_c^T J_X (6 x 3), J_X^T J_X (symmetric) and J_X^T r
struct RwBlocks {
  double Jc[12], r[2], W[18], UX[6], gX[3];
};

__device__ __forceinline__ void rw_blocks(const double* P, double fx, double fy, double cx, double cy, double px, double py,
                                          double X0, double X1, double X2, RwBlocks& o) {
#pragma clang fp contract(off)
  double a, b, c;
  rw_transform(P, X0, X1, X2, a, b, c);
  const double ic = 1.0 / c;
  o.r[0] = fx * (a * ic) + cx - px;
  o.r[1] = fy * (b * ic) + cy - py;
  const double Jp[6] = {fx * ic, 0.0, -fx * a * ic * ic, 0.0, fy * ic, -fy * b * ic * ic};
  double JX[6];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) JX[i * 3 + j] = Jp[i * 3] * P[j] + Jp[i * 3 + 1] * P[3 + j] + Jp[i * 3 + 2] * P[6 + j];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    o.Jc[i * 6 + 0] = -(Jp[i * 3 + 1] * c - Jp[i * 3 + 2] * b);          // -J_p [Y]x
    o.Jc[i * 6 + 1] = -(Jp[i * 3 + 2] * a - Jp[i * 3] * c);
    o.Jc[i * 6 + 2] = -(Jp[i * 3] * b - Jp[i * 3 + 1] * a);
    o.Jc[i * 6 + 3] = Jp[i * 3]; o.Jc[i * 6 + 4] = Jp[i * 3 + 1]; o.Jc[i * 6 + 5] = Jp[i * 3 + 2];
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) o.UX[q++] = JX[i] * JX[j] + JX[3 + i] * JX[3 + j];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.W[i * 3 + j] = o.Jc[i] * JX[j] + o.Jc[6 + i] * JX[3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) o.gX[j] = JX[j] * o.r[0] + JX[3 + j] * o.r[1];
}

// the poses of the state (or, cand, the stepped ones under the gauge's s) as doubles in LDS: P [16][12]; threads 0 .. 15
__device__ __forceinline__ void rw_load_poses(const RwState* st, bool cand, double s, double (*P)[12], int* kept) {
#pragma clang fp contract(off)
  const int f = threadIdx.x;
  if (f < RW_FRAMES) {
    kept[f] = st->kept[f];
#pragma unroll
    for (int i = 0; i < 9; ++i) P[f][i] = cand ? (double)st->nxtR[f][i] : (double)st->cur[f][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) P[f][9 + i] = cand ? (double)(float)(s * st->tn[f][i]) : (double)st->cur[f][9 + i];
  }
}

// sum of value(0 .. n - 1) in ascending order, the same in every thread: tiles of blockDim.x values through LDS, added by
// thread 0 one after the other (a padding value is +0.0, which changes no sum)
template <class F>
__device__ __forceinline__ double rw_sum_ascending(int n, F value, double* tile /* [blockDim.x] */, double* out /* [1] */) {
  double acc = 0.0;
  for (int base = 0; base < n; base += blockDim.x) {
    const int j = base + threadIdx.x;
    tile[threadIdx.x] = j < n ? value(j) : 0.0;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < (int)blockDim.x; ++i) acc += tile[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = acc;
  __syncthreads();
  return *out;
}

// ---- membership ------------------------------------------------------------------------------------------------------------
template <class Source>
__global__ __launch_bounds__(256) void rw_init_kernel(Source src, RwArgs a, const float* Rin, const float* tin) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int nk = src.nk();
  if (j < a.cap) {
    float kx = 0.f, ky = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
    bool valid = false, eligible = false;
    if (j < nk) {
      valid = src.key(j, kx, ky, X, Y, Z);
      eligible = valid && lm_reprojects((double)a.t_fx, (double)a.t_fy, (double)a.t_cx, (double)a.t_cy, (double)kx, (double)ky,
                                        (double)X, (double)Y, (double)Z, (double)a.thr * (double)a.thr);
    }
    a.xyz[j * 3 + 0] = valid ? X : 0.f; a.xyz[j * 3 + 1] = valid ? Y : 0.f; a.xyz[j * 3 + 2] = valid ? Z : 0.f;
    a.kpix[j] = make_float2(kx, ky);
    a.lmk[j] = eligible ? 3 : (valid ? 2 : 0);
  }
  if (blockIdx.x == 0) {
    RwState* st = a.st;
    const int f = threadIdx.x;
    if (f < RW_FRAMES) {
      bool any = false, finite = true;
      float v[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) v[i] = 0.f;
      if (f < a.n) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          v[i] = Rin[f * 9 + i];
          any = any || v[i] != 0.f;
          finite = finite && fabsf(v[i]) < 3.0e38f;              // (false for NaN and Inf)
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          v[9 + i] = tin[f * 3 + i];
          finite = finite && fabsf(v[9 + i]) < 3.0e38f;
        }
      }
      const bool live = f < a.n && any && finite && src.live(f);
#pragma unroll
      for (int i = 0; i < 12; ++i) st->cur[f][i] = live ? v[i] : 0.f;
      st->live[f] = live ? 1 : 0;
      st->kept[f] = 0;
      st->cnt[f] = 0;
    }
    if (f == 0) {
      st->lambda = (double)a.lambda0;
      st->C = st->C0 = st->Z0 = 0.0;
      st->stopped = st->failed = st->ok = st->made = st->accepted = st->members = st->active = st->nkept = 0;
      st->nk = nk;
    }
  }
}

// every row of frame f that names an eligible landmark and passes the test under the frame's pose: the lowest one wins
template <class Source>
__global__ __launch_bounds__(256) void rw_members_kernel(Source src, RwArgs a) {
  const int f = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  const RwState* st = a.st;
  if (!st->live[f] || k >= src.rows(f)) return;
  const int j = src.landmark(f, k);
  if (!(j >= 0 && j < st->nk) || a.lmk[j] != 3) return;
  double P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = (double)st->cur[f][i];
  float px, py;
  src.pixel(f, k, px, py);
  double y0, y1, y2;
  rw_transform(P, (double)a.xyz[j * 3], (double)a.xyz[j * 3 + 1], (double)a.xyz[j * 3 + 2], y0, y1, y2);
  if (lm_reprojects((double)a.q_fx, (double)a.q_fy, (double)a.q_cx, (double)a.q_cy, (double)px, (double)py, y0, y1, y2,
                    (double)a.thr * (double)a.thr))
    atomicMin(&a.tab[(size_t)f * a.cap + j], k);
}

template <class Source>
__global__ __launch_bounds__(256) void rw_resolve_kernel(Source src, RwArgs a) {
  const int f = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  RwState* st = a.st;
  bool has = false;
  if (st->live[f] && j < st->nk) {
    const int k = a.tab[(size_t)f * a.cap + j];
    if (k != RW_NONE) {
      float px, py;
      src.pixel(f, k, px, py);
      a.pix[(size_t)f * a.cap + j] = make_float2(px, py);
      has = true;
    }
  }
  const int c = __syncthreads_count(has ? 1 : 0);
  if (threadIdx.x == 0 && c) atomicAdd(&st->cnt[f], c);
}

__global__ __launch_bounds__(256) void rw_finish_kernel(RwArgs a) {
  __shared__ int kept[RW_FRAMES], sums[2];
  __shared__ double tile[256], out[1];
  RwState* st = a.st;
  const int tid = threadIdx.x, nk = st->nk;
  if (tid < RW_FRAMES) {
    kept[tid] = (st->live[tid] && st->cnt[tid] >= a.min_obs) ? 1 : 0;
    st->kept[tid] = kept[tid];
  }
  if (tid < 2) sums[tid] = 0;
  __syncthreads();
  int members = 0, active = 0;
  for (int j = tid; j < nk; j += 256) {
    if (a.lmk[j] != 3) continue;
    int m = 0;
    for (int f = 0; f < RW_FRAMES; ++f) m += (kept[f] && a.tab[(size_t)f * a.cap + j] != RW_NONE) ? 1 : 0;
    a.lmk[j] = m ? 1 : 2;
    members += m;
    active += m ? 1 : 0;
  }
  if (members) atomicAdd(&sums[0], members);
  if (active) atomicAdd(&sums[1], active);
  __syncthreads();                                               // (lmk is read back below by other threads: same workgroup)
  const double z0 = rw_sum_ascending(nk, [&](int j) { return a.lmk[j] == 1 ? (double)a.xyz[j * 3 + 2] : 0.0; }, tile, out);
  if (tid == 0) {
    int nkept = 0;
    for (int f = 0; f < RW_FRAMES; ++f) nkept += kept[f];
    st->nkept = nkept;
    st->members = sums[0];
    st->active = sums[1];
    st->Z0 = z0;
    if (!nkept) st->failed = st->stopped = 1;
  }
}

// ---- cost -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RW_CHUNK) void rw_cost_kernel(RwArgs a, int cand) {
  __shared__ double P[RW_FRAMES][12];
  __shared__ int kept[RW_FRAMES];
  __shared__ double tile[RW_CHUNK], out[1];
  RwState* st = a.st;
  if (st->failed || (cand && (st->stopped || !st->ok))) return;  // (uniform)
  const int tid = threadIdx.x, nk = st->nk, j = blockIdx.x * RW_CHUNK + tid;
  if (blockIdx.x * RW_CHUNK >= nk) return;
  double s = 1.0;
  bool good = true;
  if (cand) {
#pragma clang fp contract(off)
    const double z = rw_sum_ascending(nk, [&](int i) { return a.lmk[i] == 1 ? a.xd[(size_t)i * 3 + 2] : 0.0; }, tile, out);
    s = st->Z0 / z;
    good = s > 0.0 && s < 1e300;                                 // (false for NaN and Inf)
  }
  rw_load_poses(st, cand != 0, s, P, kept);
  __syncthreads();
  if (cand && blockIdx.x == 0 && tid < RW_FRAMES) {
#pragma unroll
    for (int i = 0; i < 3; ++i) st->nxtt[tid][i] = (float)P[tid][9 + i];
  }
  double c = 0.0;
  if (j < nk && a.lmk[j] == 1) {
#pragma clang fp contract(off)
    float x0, x1, x2;
    if (cand) {
      x0 = (float)(s * a.xd[(size_t)j * 3]); x1 = (float)(s * a.xd[(size_t)j * 3 + 1]); x2 = (float)(s * a.xd[(size_t)j * 3 + 2]);
      a.xnew[j * 3] = x0; a.xnew[j * 3 + 1] = x1; a.xnew[j * 3 + 2] = x2;
    } else {
      x0 = a.xyz[j * 3]; x1 = a.xyz[j * 3 + 1]; x2 = a.xyz[j * 3 + 2];
    }
    const float2 kp = a.kpix[j];
    c = rw_cost_term((double)a.t_fx, (double)a.t_fy, (double)a.t_cx, (double)a.t_cy, (double)kp.x, (double)kp.y, (double)x0,
                     (double)x1, (double)x2);
    for (int f = 0; f < RW_FRAMES; ++f) {
      if (!kept[f] || a.tab[(size_t)f * a.cap + j] == RW_NONE) continue;
      const float2 p = a.pix[(size_t)f * a.cap + j];
      double y0, y1, y2;
      rw_transform(P[f], (double)x0, (double)x1, (double)x2, y0, y1, y2);
      c += rw_cost_term((double)a.q_fx, (double)a.q_fy, (double)a.q_cx, (double)a.q_cy, (double)p.x, (double)p.y, y0, y1, y2);
    }
  }
  tile[tid] = c;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int i = 0; i < RW_CHUNK; ++i) acc += tile[i];
    a.cpart[blockIdx.x] = good ? acc : __builtin_inf();
  }
}

// first: C = C0 of the start state.  Otherwise the end of an attempt.
__global__ __launch_bounds__(256) void rw_decide_kernel(RwArgs a, int first) {
  __shared__ int accept;
  RwState* st = a.st;
  if (st->failed || st->stopped) return;                         // (uniform; written by this kernel's thread 0 behind the barrier)
  const int tid = threadIdx.x, nk = st->nk, chunks = (nk + RW_CHUNK - 1) / RW_CHUNK;
  if (tid == 0) {
    double c = 0.0;
    accept = 0;
    if (first || st->ok)
      for (int i = 0; i < chunks; ++i) c += a.cpart[i];
    if (first) {
      st->C = st->C0 = c;
    } else {
      st->made += 1;
      if (st->ok && c < st->C) {                                 // (false for NaN)
        const double gain = st->C - c, before = st->C;
        st->C = c;
        st->accepted += 1;
        st->lambda = fmax(st->lambda / 10.0, RP_LAMBDA_MIN);
        accept = gain <= RP_STOP * before ? 2 : 1;
      } else {
        st->lambda = fmin(10.0 * st->lambda, RP_LAMBDA_MAX);
      }
    }
  }
  __syncthreads();
  if (accept) {
    for (int j = tid; j < nk; j += 256) {
      if (a.lmk[j] != 1) continue;
      a.xyz[j * 3] = a.xnew[j * 3]; a.xyz[j * 3 + 1] = a.xnew[j * 3 + 1]; a.xyz[j * 3 + 2] = a.xnew[j * 3 + 2];
    }
    if (tid < RW_FRAMES && st->kept[tid]) {
#pragma unroll
      for (int i = 0; i < 9; ++i) st->cur[tid][i] = st->nxtR[tid][i];
#pragma unroll
      for (int i = 0; i < 3; ++i) st->cur[tid][9 + i] = st->nxtt[tid][i];
    }
  }
  __syncthreads();                                               // (every thread has read stopped above)
  if (tid == 0 && !first && (accept == 2 || st->made >= a.iterations)) st->stopped = 1;
}

// ---- an attempt ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rw_build_kernel(RwArgs a) {
  constexpr int NS = RW_SUB * RW_FRAMES;                         // 128 staged observations
  __shared__ double Wl[NS][18], Yl[NS][18], Jcl[NS][12], rl[NS][2], UXl[NS][6], gXl[NS][3];
  __shared__ double Vl[RW_SUB][6], gl[RW_SUB][3];
  __shared__ double P[RW_FRAMES][12];
  __shared__ int kept[RW_FRAMES], hasl[NS];
  const RwState* st = a.st;
  if (st->stopped) return;                                       // (uniform)
  const int tid = threadIdx.x, nk = st->nk, first = blockIdx.x * RW_CHUNK;
  if (first >= nk) return;
  const double lambda = st->lambda;
  rw_load_poses(st, false, 1.0, P, kept);
  __syncthreads();
  const int fa = tid >> 4, fb = tid & 15;
  double S[36], dA[6], bb[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) S[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) dA[i] = bb[i] = 0.0;
  int bad = 0;
  for (int sub = 0; sub < RW_CHUNK / RW_SUB; ++sub) {
    const int base = first + sub * RW_SUB;
    bool has = false;
    if (tid < NS) {                                              // thread (l, f): the blocks of one observation
      const int l = tid >> 4, f = tid & 15, j = base + l;
      has = j < nk && a.lmk[j] == 1 && kept[f] && a.tab[(size_t)f * a.cap + j] != RW_NONE;
      hasl[tid] = has ? 1 : 0;
      if (has) {
        const float2 p = a.pix[(size_t)f * a.cap + j];
        RwBlocks o;
        rw_blocks(P[f], (double)a.q_fx, (double)a.q_fy, (double)a.q_cx, (double)a.q_cy, (double)p.x, (double)p.y,
                  (double)a.xyz[j * 3], (double)a.xyz[j * 3 + 1], (double)a.xyz[j * 3 + 2], o);
#pragma unroll
        for (int i = 0; i < 18; ++i) Wl[tid][i] = o.W[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) Jcl[tid][i] = o.Jc[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) UXl[tid][i] = o.UX[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) gXl[tid][i] = o.gX[i];
        rl[tid][0] = o.r[0]; rl[tid][1] = o.r[1];
      }
    }
    __syncthreads();
    if (tid < RW_SUB) {                                          // thread l: U and g over the frames in ascending order
      const int j = base + tid;
      if (j < nk && a.lmk[j] == 1) {
#pragma clang fp contract(off)
        const float2 kp = a.kpix[j];
        double U[6], g[3], V[6];
        rw_key_blocks((double)a.t_fx, (double)a.t_fy, (double)a.t_cx, (double)a.t_cy, (double)kp.x, (double)kp.y,
                      (double)a.xyz[j * 3], (double)a.xyz[j * 3 + 1], (double)a.xyz[j * 3 + 2], U, g);
        for (int f = 0; f < RW_FRAMES; ++f) {
          if (!hasl[tid * RW_FRAMES + f]) continue;
#pragma unroll
          for (int i = 0; i < 6; ++i) U[i] += UXl[tid * RW_FRAMES + f][i];
#pragma unroll
          for (int i = 0; i < 3; ++i) g[i] += gXl[tid * RW_FRAMES + f][i];
        }
        if (!rp_invert(U, lambda, V)) bad = 1;
#pragma unroll
        for (int i = 0; i < 6; ++i) Vl[tid][i] = V[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) gl[tid][i] = g[i];
      }
    }
    __syncthreads();
    if (has) {                                                   // thread (l, f): Y = W U*^-1
#pragma clang fp contract(off)
      const int l = tid >> 4;
      double V[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) V[i] = Vl[l][i];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double x0 = Wl[tid][i * 3], x1 = Wl[tid][i * 3 + 1], x2 = Wl[tid][i * 3 + 2];
        Yl[tid][i * 3 + 0] = (x0 * V[0] + x1 * V[1]) + x2 * V[2];
        Yl[tid][i * 3 + 1] = (x0 * V[1] + x1 * V[3]) + x2 * V[4];
        Yl[tid][i * 3 + 2] = (x0 * V[2] + x1 * V[4]) + x2 * V[5];
      }
    }
    __syncthreads();
    for (int l = 0; l < RW_SUB; ++l) {                           // thread (fa, fb): its block, the landmarks in order
#pragma clang fp contract(off)
      const int ia = l * RW_FRAMES + fa, ib = l * RW_FRAMES + fb;
      if (!hasl[ia] || !hasl[ib]) continue;
      double Y[18], W[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) { Y[i] = Yl[ia][i]; W[i] = Wl[ib][i]; }
      if (fa == fb) {
        double Jc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) Jc[i] = Jcl[ia][i];
        const double r0 = rl[ia][0], r1 = rl[ia][1], g0 = gl[l][0], g1 = gl[l][1], g2 = gl[l][2];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int k = 0; k < 6; ++k)
            S[i * 6 + k] += (Jc[i] * Jc[k] + Jc[6 + i] * Jc[6 + k]) -
                            ((Y[i * 3] * W[k * 3] + Y[i * 3 + 1] * W[k * 3 + 1]) + Y[i * 3 + 2] * W[k * 3 + 2]);
          dA[i] += Jc[i] * Jc[i] + Jc[6 + i] * Jc[6 + i];
          bb[i] += (Jc[i] * r0 + Jc[6 + i] * r1) - ((Y[i * 3] * g0 + Y[i * 3 + 1] * g1) + Y[i * 3 + 2] * g2);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int k = 0; k < 6; ++k)
            S[i * 6 + k] += 0.0 - ((Y[i * 3] * W[k * 3] + Y[i * 3 + 1] * W[k * 3 + 1]) + Y[i * 3 + 2] * W[k * 3 + 2]);
      }
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  double* part = a.part + (size_t)blockIdx.x * RW_PART;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = 0; k < 6; ++k) part[(fa * 6 + i) * RW_D + fb * 6 + k] = S[i * 6 + k];
  if (fa == fb) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      part[RW_D * RW_D + fa * 6 + i] = bb[i];
      part[RW_D * RW_D + RW_D + fa * 6 + i] = dA[i];
    }
  }
  if (tid == 0) a.bad[blockIdx.x] = bad;
}

// R' = E(omega) R rounded to fp32 and E t + upsilon in fp64 of one frame, from its d = (omega, upsilon).  One lane.
__device__ __forceinline__ void rw_step_pose(const float* cur, const double (&d)[6], float* Rn, double* tn) {
  const double w0 = d[0], w1 = d[1], w2 = d[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double A = 1.0, Bc = 0.5;
  if (!(th2 < 1e-16)) {
    const double th = sqrt(th2);
    A = sin(th) / th;
    Bc = (1.0 - cos(th)) / th2;
  }
  const double E[9] = {1.0 + Bc * (w0 * w0 - th2), -A * w2 + Bc * w0 * w1, A * w1 + Bc * w0 * w2,
                       A * w2 + Bc * w0 * w1, 1.0 + Bc * (w1 * w1 - th2), -A * w0 + Bc * w1 * w2,
                       -A * w1 + Bc * w0 * w2, A * w0 + Bc * w1 * w2, 1.0 + Bc * (w2 * w2 - th2)};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Rn[i * 3 + j] = (float)(E[i * 3] * (double)cur[j] + E[i * 3 + 1] * (double)cur[3 + j] + E[i * 3 + 2] * (double)cur[6 + j]);
    tn[i] = (E[i * 3] * (double)cur[9] + E[i * 3 + 1] * (double)cur[10] + E[i * 3 + 2] * (double)cur[11]) + d[3 + i];
  }
}

__global__ __launch_bounds__(256) void rw_solve_kernel(RwArgs a) {
  __shared__ double sm[RW_D][RW_D + 1];
  __shared__ double fct[RW_D];
  __shared__ double tiny;
  __shared__ int kf[RW_FRAMES], pos[RW_FRAMES], D_, good, prow;
  RwState* st = a.st;
  if (st->stopped) return;                                       // (uniform)
  const int tid = threadIdx.x, chunks = (st->nk + RW_CHUNK - 1) / RW_CHUNK;
  const double lambda = st->lambda;
  if (tid == 0) {
    int d = 0;
    for (int f = 0; f < RW_FRAMES; ++f) {
      pos[f] = d;
      if (st->kept[f]) kf[d++] = f;
    }
    D_ = 6 * d;
    int g = 1;
    for (int c = 0; c < chunks; ++c) g = a.bad[c] ? 0 : g;
    good = g;
  }
  __syncthreads();
  const int D = D_;
  for (int e = tid; e < D * (D + 1); e += 256) {                 // the partials in chunk order
#pragma clang fp contract(off)
    const int i = e / (D + 1), j = e % (D + 1);
    const int fi = kf[i / 6] * 6 + i % 6;
    const int src = j < D ? fi * RW_D + kf[j / 6] * 6 + j % 6 : RW_D * RW_D + fi;
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += a.part[(size_t)c * RW_PART + src];
    if (i == j) {
      double da = 0.0;
      for (int c = 0; c < chunks; ++c) da += a.part[(size_t)c * RW_PART + RW_D * RW_D + RW_D + fi];
      v = v + lambda * da;
    }
    sm[i][j] = j < D ? v : -v;
  }
  __syncthreads();
  if (tid == 0) {
    double dmax = 0.0;
    for (int i = 0; i < D; ++i) dmax = fmax(dmax, fabs(sm[i][i]));
    tiny = RW_SINGULAR * dmax;
  }
  __syncthreads();
  bool g = good != 0;                                            // (thread 0 writes good next behind the barriers above)
  for (int c = 0; c < D && g; ++c) {                             // solve_lds, a column at a time across the workgroup
    if (tid == 0) {
      int pr = c;
      double pv = fabs(sm[c][c]);
      for (int i = c + 1; i < D; ++i) {
        const double v = fabs(sm[i][c]);
        if (v > pv) { pv = v; pr = i; }
      }
      prow = pr;
      if (!(pv > tiny)) good = 0;
    }
    __syncthreads();
    g = good != 0;                                               // (uniform; its next write is behind the barriers below)
    if (!g) break;
    const int pr = prow;
    if (pr != c && tid >= c && tid <= D) {
      const double tmp = sm[c][tid]; sm[c][tid] = sm[pr][tid]; sm[pr][tid] = tmp;
    }
    __syncthreads();
    if (tid > c && tid < D) {
#pragma clang fp contract(off)
      const double ip = 1.0 / sm[c][c];
      fct[tid] = sm[tid][c] * ip;
    }
    __syncthreads();
    const int rows = D - 1 - c, cols = D - c;                    // rows c + 1 .. D - 1, columns c + 1 .. D
    for (int e = tid; e < rows * cols; e += 256) {
#pragma clang fp contract(off)
      const int i = c + 1 + e / cols, j = c + 1 + e % cols;
      sm[i][j] = sm[i][j] - fct[i] * sm[c][j];
    }
    __syncthreads();
  }
  if (tid == 0 && g) {
#pragma clang fp contract(off)
    for (int i = D - 1; i >= 0; --i) {
      double acc = sm[i][D];
      for (int j = i + 1; j < D; ++j) acc = acc - sm[i][j] * sm[j][D];
      sm[i][D] = acc / sm[i][i];
    }
  }
  __syncthreads();
  if (tid < RW_FRAMES) {
    const bool k = g && st->kept[tid];
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      d[i] = k ? sm[pos[tid] * 6 + i][D] : 0.0;
      st->delta[tid * 6 + i] = d[i];
    }
    if (k) rw_step_pose(st->cur[tid], d, st->nxtR[tid], st->tn[tid]);
  }
  if (tid == 0) st->ok = g ? 1 : 0;
}

__global__ __launch_bounds__(RW_CHUNK) void rw_step_kernel(RwArgs a) {
#pragma clang fp contract(off)
  __shared__ double P[RW_FRAMES][12], dl[RW_D];
  __shared__ int kept[RW_FRAMES];
  const RwState* st = a.st;
  if (st->stopped || !st->ok) return;                            // (uniform)
  const int tid = threadIdx.x, nk = st->nk, j = blockIdx.x * RW_CHUNK + tid;
  if (blockIdx.x * RW_CHUNK >= nk) return;
  const double lambda = st->lambda;
  rw_load_poses(st, false, 1.0, P, kept);
  for (int i = tid; i < RW_D; i += RW_CHUNK) dl[i] = st->delta[i];
  __syncthreads();
  if (!(j < nk && a.lmk[j] == 1)) return;
  const double X0 = (double)a.xyz[j * 3], X1 = (double)a.xyz[j * 3 + 1], X2 = (double)a.xyz[j * 3 + 2];
  const float2 kp = a.kpix[j];
  double U[6], g[3], V[6], h[3] = {0.0, 0.0, 0.0};
  rw_key_blocks((double)a.t_fx, (double)a.t_fy, (double)a.t_cx, (double)a.t_cy, (double)kp.x, (double)kp.y, X0, X1, X2, U, g);
  for (int f = 0; f < RW_FRAMES; ++f) {                          // the frames one at a time
    if (!kept[f] || a.tab[(size_t)f * a.cap + j] == RW_NONE) continue;
    const float2 p = a.pix[(size_t)f * a.cap + j];
    RwBlocks o;
    rw_blocks(P[f], (double)a.q_fx, (double)a.q_fy, (double)a.q_cx, (double)a.q_cy, (double)p.x, (double)p.y, X0, X1, X2, o);
#pragma unroll
    for (int i = 0; i < 6; ++i) U[i] += o.UX[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      g[i] += o.gX[i];
      h[i] += ((((o.W[i] * dl[f * 6] + o.W[3 + i] * dl[f * 6 + 1]) + o.W[6 + i] * dl[f * 6 + 2]) + o.W[9 + i] * dl[f * 6 + 3]) +
               o.W[12 + i] * dl[f * 6 + 4]) + o.W[15 + i] * dl[f * 6 + 5];
    }
  }
  rp_invert(U, lambda, V);                                       // (the build kernel has inverted the same U*)
#pragma unroll
  for (int i = 0; i < 3; ++i) h[i] = g[i] + h[i];
  a.xd[(size_t)j * 3 + 0] = X0 - ((V[0] * h[0] + V[1] * h[1]) + V[2] * h[2]);
  a.xd[(size_t)j * 3 + 1] = X1 - ((V[1] * h[0] + V[3] * h[1]) + V[4] * h[2]);
  a.xd[(size_t)j * 3 + 2] = X2 - ((V[2] * h[0] + V[4] * h[1]) + V[5] * h[2]);
}

// ---- the result -------------------------------------------------------------------------------------------------------------
// (nobs and obs have been cleared by the host path, stream-ordered; R / t may alias the inputs, which rw_init_kernel has read)
__global__ __launch_bounds__(256) void rw_final_kernel(RwArgs a, float* R, float* t, int32_t* nobs, uint8_t* kind, uint8_t* obs,
                                                       float* stats) {
  __shared__ double P[RW_FRAMES][12];
  __shared__ int kept[RW_FRAMES];
  const RwState* st = a.st;
  const int tid = threadIdx.x, nk = st->nk, j = blockIdx.x * 256 + tid;
  rw_load_poses(st, false, 1.0, P, kept);
  __syncthreads();
  const double thr2 = (double)a.thr * (double)a.thr;
  if (j < a.cap) {
    const int lm = j < nk ? a.lmk[j] : 0;
    int k = lm == 2 ? 2 : 0;
    if (lm == 1) {
      const double X0 = (double)a.xyz[j * 3], X1 = (double)a.xyz[j * 3 + 1], X2 = (double)a.xyz[j * 3 + 2];
      const float2 kp = a.kpix[j];
      if (lm_reprojects((double)a.t_fx, (double)a.t_fy, (double)a.t_cx, (double)a.t_cy, (double)kp.x, (double)kp.y, X0, X1, X2, thr2)) {
        k = 1;
        for (int f = 0; f < RW_FRAMES; ++f) {
          const int row = kept[f] ? a.tab[(size_t)f * a.cap + j] : RW_NONE;
          if (row == RW_NONE) continue;
          const float2 p = a.pix[(size_t)f * a.cap + j];
          double y0, y1, y2;
          rw_transform(P[f], X0, X1, X2, y0, y1, y2);
          if (!lm_reprojects((double)a.q_fx, (double)a.q_fy, (double)a.q_cx, (double)a.q_cy, (double)p.x, (double)p.y, y0, y1, y2, thr2))
            continue;
          atomicAdd(&nobs[f], 1);
          if (obs) obs[(size_t)f * a.S + row] = 1;
        }
      }
    }
    kind[j] = (uint8_t)k;
    if (!k) { a.xyz[j * 3] = 0.f; a.xyz[j * 3 + 1] = 0.f; a.xyz[j * 3 + 2] = 0.f; }
  }
  if (blockIdx.x == 0) {
    for (int e = tid; e < a.n * 9; e += 256) R[e] = kept[e / 9] ? st->cur[e / 9][e % 9] : 0.f;
    for (int e = tid; e < a.n * 3; e += 256) t[e] = kept[e / 3] ? st->cur[e / 3][9 + e % 3] : 0.f;
    if (stats && tid < 4) {
      const double m = (double)(st->members + st->active);
      const double v = tid == 0 ? sqrt(st->C0 / m) : (tid == 1 ? sqrt(st->C / m) : (tid == 2 ? (double)st->made : (double)st->accepted));
      stats[tid] = st->failed ? 0.f : (float)v;
    }
  }
}
