// match_guided_pose.h -- fpc_match_frames / the bank's table pass once more, under an absolute pose per frame as the gate
// (fpc_match_frames_guided_pose / fpc_match_bank_guided_pose, include/fpc.h): "search by projection" on the device.
//
// Everything but the gate is match_guided.h's: the sets, counts and tables are fpc_match_frames' own (mf_sets), the strip
// is mg_strip, the tile mg_tile, the finalize kernel match_guided_finalize_kernel.  The train set carries landmarks --
// fpc_pnp_frames' key (xyz [nkey][3], valid [nkey] or null) or the bank's float4 rows (fpc_bank_store_landmarks) -- and
// train row j with landmark (X, Y, Z) is a CANDIDATE of query row i at pixel (x, y) iff, in fp64 from the fp32 R and t of
// the frame, with (a, b, c) = R X + t,
//     landmark j is valid,   c > 0   and   (fx a - (x - cx) c)^2 + (fy b - (y - cy) c)^2 < radius^2 c^2
// -- pnp_inlier (pnp_ransac.h) with the radius as its threshold: no division -- and the result is fpc_match_frames' rule
// over the candidates only.  The train PIXELS are never read: the gate knows the landmark's depth, which is what tells two
// landmarks on one viewing ray of the key camera apart where the epipolar band cannot.
//
//   MgPose                 the gate.  The strip's 64 query rows get xs = x - cx and ys = y - cy once, in fp64, into LDS; a
//                          row past the count gets NaN for xs, its live marker: every comparison with it fails.  Per
//                          train tile every lane transforms the landmarks of its two train columns once (column():
//                          A = fx a, B = fy b, c and the bound rc = radius^2 c^2; rc = -1 where the landmark is invalid,
//                          c <= 0 or R / t is not finite, which nothing compares below), about 16 fp64 operations against
//                          the 32 pair tests per column; the pair test is ex = A - xs c, ey = B - ys c,
//                          ex ex + ey ey < rc, the homography gate's operation count.  R and t are kept in every lane.
//   match_guided_pose_kernel   mg_strip<MgPose, MatchPoseArgs>.  Rows come in confidence order, so a tile's landmarks
//                          project anywhere in the frame; the discs are small, and a tile without a candidate is skipped
//                          before any descriptor load or MFMA, as in match_guided_kernel.
#pragma once
#include "match_guided.h"

namespace fpc {

struct MatchPoseArgs {
  const float* R;               // [n][9] row-major, landmark frame -> query camera: X_cam = R X + t
  const float* t;               // [n][3]
  const int32_t* xy;            // [B][cap][2]  fpc_results().xy
  const float* key_xyz;         // [nkey][3]    the key's landmarks (null with MatchFramesArgs::key_slot)
  const uint8_t* key_valid;     // [nkey] or null: every row
  const float4* lm;             // with MatchFramesArgs::key_slot the bank's landmarks [slots][bank_rows], w != 0 valid;
                                // null without a landmark reservation: no row is valid
  double fx, fy, cx, cy;        // the query camera
  double r2;                    // radius^2
};

struct MgPose {
  struct Row { double xs, ys; };                // a query row of the strip: its pixel from the principal point
  struct Col { double A, B, c, rc; };           // a train landmark in the camera: fx a, fy b, c and radius^2 c^2
  struct Train {                                // frame f's landmarks: the bank slot's row 0, or the key's
    const float4* lm;
    const float* xyz;
    const uint8_t* valid;
    bool bank;
  };
  double rt[12];                                // R, then t, of the frame
  bool finite;
  const double fx, fy, cx, cy, r2;
  double *s_xs, *s_ys;                          // LDS, [64] each

  __device__ __forceinline__ MgPose(const MatchPoseArgs& g, int f, double* l0, double* l1, double*, double*)
      : fx(g.fx), fy(g.fy), cx(g.cx), cy(g.cy), r2(g.r2), s_xs(l0), s_ys(l1) {
    const float* Rf = g.R + (size_t)f * 9;
    const float* tf = g.t + (size_t)f * 3;
    finite = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      rt[k] = (double)(k < 9 ? Rf[k] : tf[k - 9]);
      finite = finite && fabs(rt[k]) <= 3.5e38;              // (false for NaN and Inf)
    }
  }

  // mf_sets' choice of the train set, for the landmarks (a slot outside [0, slots): the set is empty, nothing is read)
  static __device__ __forceinline__ Train train(const MatchFramesArgs& a, const MatchPoseArgs& g, int f) {
    if (a.key_slot) {
      const int sl = a.key_slot[f];
      return Train{(g.lm && sl >= 0 && sl < a.bank_slots) ? g.lm + (size_t)sl * a.bank_rows : nullptr, nullptr, nullptr, true};
    }
    return Train{nullptr, g.key_xyz, g.key_valid, false};
  }

  // row i of the strip is row qi of the frame's pixels xy; live: it is below the frame's count
  __device__ __forceinline__ void row(int i, const int32_t* xy, int qi, bool live) const {
    const double x = (double)xy[2 * qi], y = (double)xy[2 * qi + 1];
    s_xs[i] = live ? x - cx : (double)NAN;
    s_ys[i] = y - cy;
  }
  __device__ __forceinline__ Row line(int i) const { return Row{s_xs[i], s_ys[i]}; }
  __device__ __forceinline__ Col column(const Train& tr, int tj) const {
    float Xf = 0.f, Yf = 0.f, Zf = 0.f;
    bool ok = false;
    if (tr.bank) {
      if (tr.lm) {
        const float4 p = tr.lm[tj];
        Xf = p.x; Yf = p.y; Zf = p.z;
        ok = p.w != 0.f;
      }
    } else {
      Xf = tr.xyz[3 * (size_t)tj]; Yf = tr.xyz[3 * (size_t)tj + 1]; Zf = tr.xyz[3 * (size_t)tj + 2];
      ok = (!tr.valid || tr.valid[tj] != 0) && fabsf(Xf) <= 3.402823466e38f && fabsf(Yf) <= 3.402823466e38f &&
           fabsf(Zf) <= 3.402823466e38f;                     // (false for NaN: fpc_pnp_frames' validity rule)
    }
    const double X = Xf, Y = Yf, Z = Zf;
    const double a = rt[0] * X + rt[1] * Y + rt[2] * Z + rt[9];
    const double b = rt[3] * X + rt[4] * Y + rt[5] * Z + rt[10];
    const double c = rt[6] * X + rt[7] * Y + rt[8] * Z + rt[11];
    return Col{fx * a, fy * b, c, (ok && finite && c > 0.0) ? r2 * c * c : -1.0};
  }
  // pnp_inlier's expression, its fx a and fy b taken from the column
  __device__ __forceinline__ bool pass(const Row& q, const Col& c) const {
    const double ex = c.A - q.xs * c.c, ey = c.B - q.ys * c.c;
    return ex * ex + ey * ey < c.rc;
  }
};

// grid (ceil(cap / 64), n), 256 threads
__global__ __launch_bounds__(256) void match_guided_pose_kernel(const MatchFramesArgs a, const MatchPoseArgs g) {
  mg_strip<MgPose, MatchPoseArgs>(a, g);
}

}  // namespace fpc
