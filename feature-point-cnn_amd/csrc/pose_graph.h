// Pose-graph optimisation over the bank's slots (fpc_graph_reserve / _set_nodes / _clear / _get / _add_edges / _optimise /
// _apply_scale; the rule is stated in include/fpc.h and restated in float64 by tests/test_pose_graph.py).  Sim(3) nodes
// (s, R, t) with X_i = s_i R_i X_w + t_i, edges X_to = s R X_from + t appended on the device from what the PnP and Sim(3)
// calls write, Levenberg-Marquardt on the seven-number residual of every edge, the linear system solved by block-Jacobi
// preconditioned conjugate gradients.  hf_clamp is ransac_parts.h's, pnp_finite3 pnp_ransac.h's, RP_LAMBDA_MIN / _MAX and
// RP_STOP refine_pose.h's.  The state is the node arrays of the fpc_graph_reserve reservation; everything else lives there
// too.  No workgroup ever waits on another: what joins the nodes and the edges is the next launch.
//
//   pg_set_nodes_kernel         a range of nodes from the caller's arrays
//   pg_add_edges_kernel         one workgroup: tiles of 256 candidate edges, taken ones ranked by ballot / popcount and appended
//                               at count + rank; FPC_GRAPH_INIT_TO: lane 0 then walks the appended edges in ascending order
//   pg_degree_kernel            a thread per node counts its active edges (both ends set)
//   pg_begin_kernel             one workgroup: the gauge test, the members, the prefix of the degrees, the state of the call
//   pg_fill_kernel              a thread per node lists its active edges in ascending order (edge * 2 + side)
//   pg_edges_kernel<CAND>       a thread per edge: E = M o S_a o S_b^-1, its residual and cost term from the state (or, CAND,
//                               the stepped state); the state's linearisation goes to the reservation; a chunk of 64 edges adds
//                               its terms in ascending order
//   pg_decide_kernel            sums the chunks in order; accept / reject / stop; on accept the stepped state is copied
//   -- per attempt: edges<false> (behind an earlier attempt), blocks, solve, retract, edges<true>, decide; all return at once
//      when PgState::stopped is set --
//   pg_blocks_kernel            a thread per member node: g and the 7 x 7 block of J^T W J over its edges in ascending order, the
//                               damped block inverted by Gauss-Jordan with partial pivoting on a 7 x 14 tableau in LDS
//   pg_solve_kernel             ONE workgroup, a node per thread, up to 1024: the whole conjugate-gradient solve of the attempt.
//                               Search direction and residual in LDS (2 x 56 KiB at 1024 nodes), the solution in the
//                               reservation; a matrix-vector product re-applies every edge's Jacobians from its 32 stored
//                               doubles (a thread per edge forms w (J_a p_a + J_b p_b), a barrier, a thread per node adds
//                               J^T of its edges' vectors), so no 7 x 7 block per edge is kept; dot products by a fixed tree
//   pg_retract_kernel           a thread per node: S <- D(delta) S rounded to fp32, into the stepped state
//   pg_scale_*_kernel           fpc_graph_apply_scale: edges, the bank's landmark rows, then the nodes
#pragma once
#include "refine_window.h"

constexpr int PG_MAX_NODES = 1024;        // FPC_BANK_MAX_SLOTS: one node per thread of the solve's workgroup
constexpr int PG_MAX_EDGES = 16384;       // FPC_GRAPH_MAX_EDGES
constexpr int PG_CHUNK = 64;              // edges per workgroup of pg_edges_kernel, nodes per workgroup of the node kernels
constexpr int PG_LIN = 32;                // doubles of an edge's linearisation: R 9, d = t - t_E 3, s, R_E 9, s_E, w, e 7, -
constexpr double PG_SINGULAR = RW_SINGULAR;

struct PgState {
  double lambda, C, C0;
  int stopped, failed, ok, made, accepted, fixed, count;
};

struct PgArgs {
  int nodes, edges;                       // the reservation's capacities
  float *ns, *nR, *nt;                    // node state: [nodes], [nodes][9], [nodes][3]
  int32_t *efrom, *eto;                   // edges: [edges]
  float *es, *eR, *et, *ew;               // [edges], [edges][9], [edges][3], [edges]
  int32_t* count;                         // [2]: edges held, edges dropped
  PgState* st;
  float *cs, *cR, *ct;                    // the stepped state
  int32_t *deg, *adj;                     // [nodes + 1] (degrees, then offsets), [2 edges]: edge * 2 + side (0 from, 1 to)
  uint8_t* member;                        // [nodes]: an unknown of the problem
  int32_t* bad;                           // [nodes]: a 7 x 7 block without a pivot
  double *lin;                            // [edges][PG_LIN]
  double *g, *dH, *delta;                 // [7][PG_MAX_NODES] each
  double *Minv;                           // [49][PG_MAX_NODES]
  double *cpart;                          // [chunks]
  double *eq;                             // [edges][8]: w (J_a p_a + J_b p_b) of the solve's current product
  int iterations, cg_iterations;
  double lambda0, tol2, iu;               // cg_tol^2 and 1 / trans_unit, formed in fp64 from the fp32 parameters
};

__device__ __forceinline__ bool pg_set(float s) { return s > 0.f; }     // (false for NaN)

// E = M o S_a o S_b^-1 in fp64 from fp32 values: Q = R_a R_b^T, k = s_a / s_b, u = t_a - k Q t_b, R_E = R Q,
// t_E = s R u + t, s_E = s k
__device__ __forceinline__ void pg_compose(const float* Ms, const float* MR, const float* Mt, float sa, const float* Ra,
                                           const float* ta, float sb, const float* Rb, const float* tb, double& sE,
                                           double (&RE)[9], double (&tE)[3]) {
#pragma clang fp contract(off)
  double Q[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Q[i * 3 + j] = (double)Ra[i * 3] * (double)Rb[j * 3] + (double)Ra[i * 3 + 1] * (double)Rb[j * 3 + 1] +
                     (double)Ra[i * 3 + 2] * (double)Rb[j * 3 + 2];
  const double k = (double)sa / (double)sb, s = (double)Ms[0];
  double u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    u[i] = (double)ta[i] - k * (Q[i * 3] * (double)tb[0] + Q[i * 3 + 1] * (double)tb[1] + Q[i * 3 + 2] * (double)tb[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      RE[i * 3 + j] = (double)MR[i * 3] * Q[j] + (double)MR[i * 3 + 1] * Q[3 + j] + (double)MR[i * 3 + 2] * Q[6 + j];
    tE[i] = s * ((double)MR[i * 3] * u[0] + (double)MR[i * 3 + 1] * u[1] + (double)MR[i * 3 + 2] * u[2]) + (double)Mt[i];
  }
  sE = s * k;
}

// log_SO(3): v = vee(R - R^T) / 2, theta = atan2(|v|, (tr R - 1) / 2), omega = (theta / |v|) v, or v where |v| < 1e-12
__device__ __forceinline__ void pg_log_so3(const double (&R)[9], double (&w)[3]) {
#pragma clang fp contract(off)
  const double v0 = 0.5 * (R[7] - R[5]), v1 = 0.5 * (R[2] - R[6]), v2 = 0.5 * (R[3] - R[1]);
  const double sn = sqrt(v0 * v0 + v1 * v1 + v2 * v2), cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  double f = 1.0;
  if (!(sn < 1e-12)) f = atan2(sn, cs) / sn;
  w[0] = f * v0; w[1] = f * v1; w[2] = f * v2;
}

// E(omega), the PnP refit's exponential (rw_step_pose's form)
__device__ __forceinline__ void pg_exp_so3(double w0, double w1, double w2, double (&E)[9]) {
#pragma clang fp contract(off)
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double A = 1.0, Bc = 0.5;
  if (!(th2 < 1e-16)) {
    const double th = sqrt(th2);
    A = sin(th) / th;
    Bc = (1.0 - cos(th)) / th2;
  }
  E[0] = 1.0 + Bc * (w0 * w0 - th2); E[1] = -A * w2 + Bc * w0 * w1; E[2] = A * w1 + Bc * w0 * w2;
  E[3] = A * w2 + Bc * w0 * w1; E[4] = 1.0 + Bc * (w1 * w1 - th2); E[5] = -A * w0 + Bc * w1 * w2;
  E[6] = -A * w1 + Bc * w0 * w2; E[7] = A * w0 + Bc * w1 * w2; E[8] = 1.0 + Bc * (w2 * w2 - th2);
}

// ---- storage and edges -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_set_nodes_kernel(PgArgs a, int first, int count, const float* s, const float* R,
                                                           const float* t) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const int i = first + k;
  a.ns[i] = s ? s[k] : 1.f;
  for (int j = 0; j < 9; ++j) a.nR[i * 9 + j] = R[k * 9 + j];
  for (int j = 0; j < 3; ++j) a.nt[i * 3 + j] = t[k * 3 + j];
}

__device__ __forceinline__ bool pg_edge_ok(const PgArgs& a, int from, int to, float s, const float* R, const float* t) {
  if (from < 0 || from >= a.nodes || to < 0 || to >= a.nodes || from == to) return false;
  bool fin = isfinite(s) && s > 0.f && pnp_finite3(t[0], t[1], t[2]), any = false;
  for (int j = 0; j < 9; ++j) {
    fin = fin && isfinite(R[j]);
    any = any || R[j] != 0.f;
  }
  return fin && any;
}

__global__ __launch_bounds__(256) void pg_add_edges_kernel(PgArgs a, int n, const int32_t* from, const int32_t* to, const float* s,
                                                           const float* R, const float* t, const int32_t* ninl, int min_inliers,
                                                           int init_to) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = hf_clamp(a.count[0], a.edges);                // (count[0] is written behind the last barrier below)
  int taken = 0;
  for (int tile = 0; tile < n; tile += 256) {
    const int f = tile + tid;
    bool take = false;
    float sv = 1.f, wv = 1.f;
    if (f < n) {
      sv = s ? s[f] : 1.f;
      const int ni = ninl ? ninl[f] : 0;
      wv = ninl ? (float)ni : 1.f;
      take = pg_edge_ok(a, from[f], to[f], sv, R + (size_t)f * 9, t + (size_t)f * 3) && (!ninl || ni >= min_inliers);
    }
    const unsigned long long bal = __ballot(take);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const int pos = base + taken + before;
    if (take && pos < a.edges) {
      a.efrom[pos] = from[f]; a.eto[pos] = to[f]; a.es[pos] = sv; a.ew[pos] = wv;
      for (int j = 0; j < 9; ++j) a.eR[(size_t)pos * 9 + j] = R[(size_t)f * 9 + j];
      for (int j = 0; j < 3; ++j) a.et[(size_t)pos * 3 + j] = t[(size_t)f * 3 + j];
    }
    taken += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (tid != 0) return;                                          // (the edges written above are visible behind the barrier)
  const int end = base + taken < a.edges ? base + taken : a.edges;
  if (init_to) {
#pragma clang fp contract(off)
    for (int e = base; e < end; ++e) {
      const int fa = a.efrom[e], tb = a.eto[e];
      const float sa = a.ns[fa];
      if (!pg_set(sa) || pg_set(a.ns[tb])) continue;
      const double sm = (double)a.es[e];
      const float* Rm = a.eR + (size_t)e * 9; const float* Ra = a.nR + fa * 9; const float* ta = a.nt + fa * 3;
      float Rn[9], tn[3];
      const float sn = (float)(sm * (double)sa);
      bool fin = isfinite(sn) && sn > 0.f;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
          Rn[i * 3 + j] = (float)((double)Rm[i * 3] * (double)Ra[j] + (double)Rm[i * 3 + 1] * (double)Ra[3 + j] +
                                  (double)Rm[i * 3 + 2] * (double)Ra[6 + j]);
          fin = fin && isfinite(Rn[i * 3 + j]);
        }
        tn[i] = (float)(sm * ((double)Rm[i * 3] * (double)ta[0] + (double)Rm[i * 3 + 1] * (double)ta[1] +
                              (double)Rm[i * 3 + 2] * (double)ta[2]) + (double)a.et[(size_t)e * 3 + i]);
        fin = fin && isfinite(tn[i]);
      }
      if (!fin) continue;
      a.ns[tb] = sn;
      for (int j = 0; j < 9; ++j) a.nR[tb * 9 + j] = Rn[j];
      for (int j = 0; j < 3; ++j) a.nt[tb * 3 + j] = tn[j];
    }
  }
  a.count[0] = end;
  a.count[1] += base + taken - end;
}

// ---- the problem of a call ---------------------------------------------------------------------------------------------------
// the active edges of node i: both ends set.  `list`: their codes in ascending edge order, else only their number.
__device__ __forceinline__ int pg_incident(const PgArgs& a, int i, int count, int32_t* list) {
  int d = 0;
  for (int e = 0; e < count; ++e) {
    const int fa = a.efrom[e], tb = a.eto[e];
    if (fa != i && tb != i) continue;
    if (!pg_set(a.ns[fa == i ? tb : fa])) continue;
    if (list) list[d] = e * 2 + (tb == i ? 1 : 0);
    ++d;
  }
  return d;
}

__global__ __launch_bounds__(PG_CHUNK) void pg_degree_kernel(PgArgs a) {
  const int i = blockIdx.x * PG_CHUNK + threadIdx.x;
  if (i >= a.nodes) return;
  a.deg[i] = pg_set(a.ns[i]) ? pg_incident(a, i, hf_clamp(a.count[0], a.edges), nullptr) : 0;
}

__global__ __launch_bounds__(1024) void pg_begin_kernel(PgArgs a, const int32_t* fixed, float* stats) {
  __shared__ int scan[PG_MAX_NODES];
  const int i = threadIdx.x;
  const int fx = fixed[0];
  const bool failed = fx < 0 || fx >= a.nodes || !pg_set(a.ns[fx]);
  const int d = i < a.nodes ? a.deg[i] : 0;
  scan[i] = d;
  __syncthreads();
  for (int o = 1; o < PG_MAX_NODES; o <<= 1) {                   // inclusive prefix of the degrees (integers: any order)
    const int v = i >= o ? scan[i - o] : 0;
    __syncthreads();
    scan[i] += v;
    __syncthreads();
  }
  if (i < a.nodes) {
    a.deg[i] = scan[i] - d;
    a.member[i] = (!failed && d > 0 && i != fx) ? 1 : 0;
    a.bad[i] = 0;
  }
  if (i == a.nodes - 1) a.deg[a.nodes] = scan[i];
  if (i == 0) {
    PgState* st = a.st;
    st->lambda = a.lambda0; st->C = st->C0 = 0.0;
    st->stopped = st->failed = failed ? 1 : 0;
    st->ok = 1; st->made = st->accepted = 0; st->fixed = fx; st->count = hf_clamp(a.count[0], a.edges);
    stats[0] = stats[1] = stats[2] = stats[3] = 0.f;
  }
}

__global__ __launch_bounds__(PG_CHUNK) void pg_fill_kernel(PgArgs a) {
  const int i = blockIdx.x * PG_CHUNK + threadIdx.x;
  if (i >= a.nodes || a.st->stopped || a.deg[i + 1] == a.deg[i]) return;
  pg_incident(a, i, a.st->count, a.adj + a.deg[i]);
}

// CAND: the cost of the stepped state.  Otherwise the cost of the state and its linearisation.
template <bool CAND>
__global__ __launch_bounds__(PG_CHUNK) void pg_edges_kernel(PgArgs a) {
#pragma clang fp contract(off)
  __shared__ double tile[PG_CHUNK];
  const PgState* st = a.st;
  if (st->stopped || (CAND && !st->ok)) return;                  // (uniform)
  const int e = blockIdx.x * PG_CHUNK + threadIdx.x;
  const float *ns = CAND ? a.cs : a.ns, *nR = CAND ? a.cR : a.nR, *nt = CAND ? a.ct : a.nt;
  double c = 0.0;
  if (e < st->count) {
    const int fa = a.efrom[e], tb = a.eto[e];
    const float sa = ns[fa], sb = ns[tb];
    if (pg_set(sa) && pg_set(sb)) {
      double sE, RE[9], tE[3], r[7];
      pg_compose(a.es + e, a.eR + (size_t)e * 9, a.et + (size_t)e * 3, sa, nR + fa * 9, nt + fa * 3, sb, nR + tb * 9, nt + tb * 3, sE,
                 RE, tE);
      double w3[3];
      pg_log_so3(RE, w3);
      r[0] = w3[0]; r[1] = w3[1]; r[2] = w3[2];
      r[3] = tE[0] * a.iu; r[4] = tE[1] * a.iu; r[5] = tE[2] * a.iu;
      r[6] = log(sE);
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < 7; ++k) q = q + r[k] * r[k];
      const double w = (double)a.ew[e];
      c = w * q;
      if (!CAND) {
        double* L = a.lin + (size_t)e * PG_LIN;
#pragma unroll
        for (int k = 0; k < 9; ++k) L[k] = (double)a.eR[(size_t)e * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) L[9 + k] = (double)a.et[(size_t)e * 3 + k] - tE[k];
        L[12] = (double)a.es[e];
#pragma unroll
        for (int k = 0; k < 9; ++k) L[13 + k] = RE[k];
        L[22] = sE; L[23] = w;
#pragma unroll
        for (int k = 0; k < 7; ++k) L[24 + k] = r[k];
      }
    }
  }
  tile[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int k = 0; k < PG_CHUNK; ++k) acc = acc + tile[k];
    a.cpart[blockIdx.x] = acc;
  }
}

// first: C = C0 of the start state.  Otherwise the end of an attempt.
__global__ __launch_bounds__(1024) void pg_decide_kernel(PgArgs a, int first, float* stats) {
  __shared__ int accept;
  PgState* st = a.st;
  if (st->stopped) return;                                       // (uniform; written by this kernel's thread 0 behind the barrier)
  const int tid = threadIdx.x;
  if (tid == 0) {
    double c = 0.0;
    accept = 0;
    const int chunks = (st->count + PG_CHUNK - 1) / PG_CHUNK;
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
      st->ok = 1;
    }
    stats[0] = (float)st->C0; stats[1] = (float)st->C; stats[2] = (float)st->made; stats[3] = (float)st->accepted;
  }
  __syncthreads();
  if (accept && tid < a.nodes && a.member[tid]) {
    a.ns[tid] = a.cs[tid];
    for (int j = 0; j < 9; ++j) a.nR[tid * 9 + j] = a.cR[tid * 9 + j];
    for (int j = 0; j < 3; ++j) a.nt[tid * 3 + j] = a.ct[tid * 3 + j];
  }
  __syncthreads();                                               // (every thread has read stopped above)
  if (tid == 0 && !first && (accept == 2 || st->made >= a.iterations)) st->stopped = 1;
}

// ---- an attempt --------------------------------------------------------------------------------------------------------------
// J of edge L on one side (0: the `from` node a, 1: the `to` node b), 7 x 7 row-major, the e_t rows times iu
__device__ __forceinline__ void pg_jacobian(const double* L, int side, double iu, double (&J)[49]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 49; ++k) J[k] = 0.0;
  if (side == 0) {
    const double d0 = L[9], d1 = L[10], d2 = L[11], s = L[12];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double c0 = L[j], c1 = L[3 + j], c2 = L[6 + j];      // column j of R
      J[0 * 7 + j] = c0; J[1 * 7 + j] = c1; J[2 * 7 + j] = c2;
      J[3 * 7 + j] = (d1 * c2 - d2 * c1) * iu;                    // ([t]x - [t_E]x) R = d x (column)
      J[4 * 7 + j] = (d2 * c0 - d0 * c2) * iu;
      J[5 * 7 + j] = (d0 * c1 - d1 * c0) * iu;
      J[3 * 7 + 3 + j] = s * c0 * iu; J[4 * 7 + 3 + j] = s * c1 * iu; J[5 * 7 + 3 + j] = s * c2 * iu;
    }
    J[3 * 7 + 6] = -d0 * iu; J[4 * 7 + 6] = -d1 * iu; J[5 * 7 + 6] = -d2 * iu;   // (t_E - t) / unit
    J[48] = 1.0;
  } else {
    const double sE = L[22];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        J[i * 7 + j] = -L[13 + i * 3 + j];
        J[(3 + i) * 7 + 3 + j] = -(sE * L[13 + i * 3 + j]) * iu;
      }
    J[48] = -1.0;
  }
}

__global__ __launch_bounds__(PG_CHUNK) void pg_blocks_kernel(PgArgs a) {
#pragma clang fp contract(off)
  __shared__ double T[7 * 14][PG_CHUNK];
  const PgState* st = a.st;
  if (st->stopped) return;                                       // (uniform)
  const int tid = threadIdx.x, i = blockIdx.x * PG_CHUNK + tid;
  if (i >= a.nodes || !a.member[i]) return;                      // (no barrier below: a thread works on its own columns)
  double g[7], H[28];
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 28; ++k) H[k] = 0.0;
  for (int p = a.deg[i]; p < a.deg[i + 1]; ++p) {
    const int code = a.adj[p];
    const double* L = a.lin + (size_t)(code >> 1) * PG_LIN;
    double J[49];
    pg_jacobian(L, code & 1, a.iu, J);
    const double w = L[23];
    int q = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int r = 0; r < 7; ++r) acc = acc + J[r * 7 + j] * L[24 + r];
      g[j] = g[j] + w * acc;
#pragma unroll
      for (int k = j; k < 7; ++k) {
        double h = 0.0;
#pragma unroll
        for (int r = 0; r < 7; ++r) h = h + J[r * 7 + j] * J[r * 7 + k];
        H[q] = H[q] + w * h;
        ++q;
      }
    }
  }
  const double lambda = st->lambda;
  double dmax = 0.0;
  {
    int q = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      a.g[j * PG_MAX_NODES + i] = g[j];
#pragma unroll
      for (int k = j; k < 7; ++k) {
        double v = H[q++];
        if (k == j) {
          a.dH[j * PG_MAX_NODES + i] = v;
          v = v + lambda * v;
          dmax = fmax(dmax, fabs(v));
        }
        T[j * 14 + k][tid] = v; T[k * 14 + j][tid] = v;
        T[j * 14 + 7 + k][tid] = k == j ? 1.0 : 0.0; T[k * 14 + 7 + j][tid] = k == j ? 1.0 : 0.0;
      }
    }
  }
  const double tiny = PG_SINGULAR * dmax;
  bool good = true;
  for (int c = 0; c < 7 && good; ++c) {                          // Gauss-Jordan, partial pivoting: the first largest pivot
    int pr = c;
    double pv = fabs(T[c * 14 + c][tid]);
    for (int r = c + 1; r < 7; ++r) {
      const double v = fabs(T[r * 14 + c][tid]);
      if (v > pv) { pv = v; pr = r; }
    }
    if (!(pv > tiny)) { good = false; break; }
    if (pr != c)
      for (int k = 0; k < 14; ++k) {
        const double tmp = T[c * 14 + k][tid]; T[c * 14 + k][tid] = T[pr * 14 + k][tid]; T[pr * 14 + k][tid] = tmp;
      }
    const double ip = 1.0 / T[c * 14 + c][tid];
    for (int k = 0; k < 14; ++k) T[c * 14 + k][tid] = T[c * 14 + k][tid] * ip;
    for (int r = 0; r < 7; ++r) {
      if (r == c) continue;
      const double f = T[r * 14 + c][tid];
      for (int k = 0; k < 14; ++k) T[r * 14 + k][tid] = T[r * 14 + k][tid] - f * T[c * 14 + k][tid];
    }
  }
  a.bad[i] = good ? 0 : 1;
  for (int j = 0; j < 7; ++j)
    for (int k = 0; k < 7; ++k) a.Minv[(j * 7 + k) * PG_MAX_NODES + i] = good ? T[j * 14 + 7 + k][tid] : 0.0;
}

// the sum of every thread's v by the fixed tree: partials by node index, stride halving from blockDim / 2 (the nodes beyond
// the workgroup are +0 terms of the 1024-leaf tree the header states)
__device__ __forceinline__ double pg_tree(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// (H + lambda diag H) delta = -g by block-Jacobi preconditioned conjugate gradients; blockDim: the power of two >= nodes
__global__ __launch_bounds__(1024) void pg_solve_kernel(PgArgs a) {
#pragma clang fp contract(off)
  __shared__ double P[7][PG_MAX_NODES], Rr[7][PG_MAX_NODES], red[PG_MAX_NODES];
  PgState* st = a.st;
  if (st->stopped) return;                                       // (uniform)
  const int i = threadIdx.x;
  const bool mem = i < a.nodes && a.member[i];
  if (__syncthreads_or(mem && a.bad[i])) {                       // a block without a pivot rejects the attempt
    if (i == 0) st->ok = 0;
    return;
  }
  const double lambda = st->lambda, iu = a.iu;
  const int count = st->count;
  const int p0 = mem ? a.deg[i] : 0, p1 = mem ? a.deg[i + 1] : 0;
  double part = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    Rr[k][i] = mem ? -a.g[k * PG_MAX_NODES + i] : 0.0;
    if (i < a.nodes) a.delta[k * PG_MAX_NODES + i] = 0.0;
  }
  double* Z = a.g;                                               // (g is in Rr now: its columns hold z from here on)
#pragma unroll 1
  for (int k = 0; k < 7; ++k) {
    double acc = 0.0;
    if (mem)
#pragma unroll
      for (int j = 0; j < 7; ++j) acc = acc + a.Minv[(k * 7 + j) * PG_MAX_NODES + i] * Rr[j][i];
    if (mem) Z[k * PG_MAX_NODES + i] = acc;
    P[k][i] = acc;
    part = part + Rr[k][i] * acc;
  }
  double rz = pg_tree(part, red);                                // (its barriers publish P)
  const double rz0 = rz;
  if (!(rz0 > 0.0)) return;                                      // nothing to solve: delta = 0
  for (int it = 0; it < a.cg_iterations; ++it) {
    for (int e = i; e < count; e += blockDim.x) {                // q = w (J_a p_a + J_b p_b) of every active edge
      const int na = a.efrom[e], nb = a.eto[e];
      if (!pg_set(a.ns[na]) || !pg_set(a.ns[nb])) continue;
      const double* L = a.lin + (size_t)e * PG_LIN;
      double Rw[3], Ru[3], Ew[3], Eu[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Rw[r] = L[r * 3] * P[0][na] + L[r * 3 + 1] * P[1][na] + L[r * 3 + 2] * P[2][na];
        Ru[r] = L[r * 3] * P[3][na] + L[r * 3 + 1] * P[4][na] + L[r * 3 + 2] * P[5][na];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Ew[r] = L[13 + r * 3] * P[0][nb] + L[13 + r * 3 + 1] * P[1][nb] + L[13 + r * 3 + 2] * P[2][nb];
        Eu[r] = L[13 + r * 3] * P[3][nb] + L[13 + r * 3 + 1] * P[4][nb] + L[13 + r * 3 + 2] * P[5][nb];
      }
      const double d0 = L[9], d1 = L[10], d2 = L[11], s = L[12], sE = L[22], w = L[23];
      const double sga = P[6][na], sgb = P[6][nb];
      double* q = a.eq + (size_t)e * 8;
      q[0] = w * (Rw[0] - Ew[0]); q[1] = w * (Rw[1] - Ew[1]); q[2] = w * (Rw[2] - Ew[2]);
      q[3] = w * (((d1 * Rw[2] - d2 * Rw[1]) + s * Ru[0] - d0 * sga - sE * Eu[0]) * iu);
      q[4] = w * (((d2 * Rw[0] - d0 * Rw[2]) + s * Ru[1] - d1 * sga - sE * Eu[1]) * iu);
      q[5] = w * (((d0 * Rw[1] - d1 * Rw[0]) + s * Ru[2] - d2 * sga - sE * Eu[2]) * iu);
      q[6] = w * (sga - sgb);
    }
    __syncthreads();                                             // (the workgroup's own writes to eq, on its own CU)
    double ap[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) ap[k] = 0.0;
#pragma unroll 1
    for (int p = p0; p < p1; ++p) {                              // A p of this node: J^T q of its edges in ascending order
      const int code = a.adj[p], e = code >> 1;
      const double* L = a.lin + (size_t)e * PG_LIN;
      const double* q = a.eq + (size_t)e * 8;
      const double qt0 = q[3] * iu, qt1 = q[4] * iu, qt2 = q[5] * iu;
      if ((code & 1) == 0) {                                     // J_a^T q
        const double d0 = L[9], d1 = L[10], d2 = L[11], s = L[12];
        const double m0 = q[0] + (qt1 * d2 - qt2 * d1), m1 = q[1] + (qt2 * d0 - qt0 * d2), m2 = q[2] + (qt0 * d1 - qt1 * d0);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ap[j] = ap[j] + (L[j] * m0 + L[3 + j] * m1 + L[6 + j] * m2);
          ap[3 + j] = ap[3 + j] + s * (L[j] * qt0 + L[3 + j] * qt1 + L[6 + j] * qt2);
        }
        ap[6] = ap[6] + (q[6] - (d0 * qt0 + d1 * qt1 + d2 * qt2));
      } else {                                                   // J_b^T q
        const double sE = L[22];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          ap[j] = ap[j] - (L[13 + j] * q[0] + L[16 + j] * q[1] + L[19 + j] * q[2]);
          ap[3 + j] = ap[3 + j] - sE * (L[13 + j] * qt0 + L[16 + j] * qt1 + L[19 + j] * qt2);
        }
        ap[6] = ap[6] - q[6];
      }
    }
    part = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (mem) ap[k] = ap[k] + lambda * a.dH[k * PG_MAX_NODES + i] * P[k][i];
      part = part + P[k][i] * ap[k];
    }
    const double pAp = pg_tree(part, red);
    if (!(pAp > 0.0)) break;                                     // (uniform; false for NaN)
    const double alpha = rz / pAp;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (mem) a.delta[k * PG_MAX_NODES + i] = a.delta[k * PG_MAX_NODES + i] + alpha * P[k][i];
      Rr[k][i] = Rr[k][i] - alpha * ap[k];
    }
    part = 0.0;
#pragma unroll 1
    for (int k = 0; k < 7; ++k) {
      double acc = 0.0;
      if (mem)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc = acc + a.Minv[(k * 7 + j) * PG_MAX_NODES + i] * Rr[j][i];
      if (mem) Z[k * PG_MAX_NODES + i] = acc;
      part = part + Rr[k][i] * acc;
    }
    const double rzn = pg_tree(part, red);                       // (every read of P by the product above lies behind it)
    if (rzn <= a.tol2 * rz0) break;
    const double beta = rzn / rz;
#pragma unroll
    for (int k = 0; k < 7; ++k) P[k][i] = (mem ? Z[k * PG_MAX_NODES + i] : 0.0) + beta * P[k][i];
    rz = rzn;
    __syncthreads();
  }
}

__global__ __launch_bounds__(PG_CHUNK) void pg_retract_kernel(PgArgs a) {
#pragma clang fp contract(off)
  PgState* st = a.st;
  if (st->stopped || !st->ok) return;                            // (ok is cleared below only by atomics of this launch:
  const int i = blockIdx.x * PG_CHUNK + threadIdx.x;            //  a thread that reads 0 early skips work nobody will use)
  if (i >= a.nodes) return;
  const float s = a.ns[i];
  if (!a.member[i]) {
    a.cs[i] = s;
    for (int j = 0; j < 9; ++j) a.cR[i * 9 + j] = a.nR[i * 9 + j];
    for (int j = 0; j < 3; ++j) a.ct[i * 3 + j] = a.nt[i * 3 + j];
    return;
  }
  double d[7], E[9];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = a.delta[k * PG_MAX_NODES + i];
  pg_exp_so3(d[0], d[1], d[2], E);
  const double es = exp(d[6]);
  const float* R = a.nR + i * 9; const float* t = a.nt + i * 3;
  const float sn = (float)(es * (double)s);
  bool fin = isfinite(sn) && sn > 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = (float)(E[r * 3] * (double)R[j] + E[r * 3 + 1] * (double)R[3 + j] + E[r * 3 + 2] * (double)R[6 + j]);
      a.cR[i * 9 + r * 3 + j] = v;
      fin = fin && isfinite(v);
    }
    const float v = (float)(es * (E[r * 3] * (double)t[0] + E[r * 3 + 1] * (double)t[1] + E[r * 3 + 2] * (double)t[2]) + d[3 + r]);
    a.ct[i * 3 + r] = v;
    fin = fin && isfinite(v);
  }
  a.cs[i] = sn;
  if (!fin) atomicExch(&st->ok, 0);                              // a stepped node that left fp32 rejects the attempt
}

// ---- fpc_graph_apply_scale: edges, landmarks, nodes -- in that order, each reads the nodes the last one rewrites --------------
__global__ __launch_bounds__(256) void pg_scale_edges_kernel(PgArgs a) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= hf_clamp(a.count[0], a.edges)) return;
  const float fa = a.ns[a.efrom[e]], fb = a.ns[a.eto[e]];
  const double sa = pg_set(fa) ? (double)fa : 1.0, sb = pg_set(fb) ? (double)fb : 1.0;
  a.es[e] = (float)((double)a.es[e] * sa / sb);
  for (int j = 0; j < 3; ++j) a.et[(size_t)e * 3 + j] = (float)((double)a.et[(size_t)e * 3 + j] / sb);
}

// grid (ceil(rows / 256), slots)
__global__ __launch_bounds__(256) void pg_scale_points_kernel(PgArgs a, float4* lm, const int32_t* count, int rows) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x, slot = blockIdx.y;
  const float s = a.ns[slot];
  if (!pg_set(s) || s == 1.f || r >= hf_clamp(count[slot], rows)) return;
  float4 v = lm[(size_t)slot * rows + r];
  if (v.w == 0.f) return;
  const double inv = 1.0 / (double)s;
  v.x = (float)((double)v.x * inv); v.y = (float)((double)v.y * inv); v.z = (float)((double)v.z * inv);
  lm[(size_t)slot * rows + r] = v;
}

__global__ __launch_bounds__(256) void pg_scale_nodes_kernel(PgArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nodes) return;
  const float s = a.ns[i];
  if (!pg_set(s) || s == 1.f) return;
  const double inv = 1.0 / (double)s;
  for (int j = 0; j < 3; ++j) a.nt[i * 3 + j] = (float)((double)a.nt[i * 3 + j] * inv);
  a.ns[i] = 1.f;
}
