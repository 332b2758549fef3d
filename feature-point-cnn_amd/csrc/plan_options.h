// plan_options.h -- the launch-plan options of a context: one struct, one table, one pure resolver.
//
// Every option has a default, most have a FPC_PLAN_* bit of fpc_config::plan_flags (include/fpc.h) and an FPC_*
// environment variable that overrides the flag for A/B runs of an unmodified caller.  resolve_plan_options reads
// nothing but its arguments, so the whole block is tested without a GPU (tests/test_plan_options.py).
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>

#include "../../include/fpc.h"

namespace fpc {

struct PlanOptions {
  // ---- which kernels the plan builders choose
  bool fuse_blocks = true;           // one launch per ResNetBlock (FPC_FUSE=0: conv1 / conv2 launches)
  bool winograd = true;              // stride-1 blocks with <= 128 channels: Winograd (FPC_WINOGRAD=0: direct)
  int winograd_gen = 3;              // 64- and 128-channel Winograd layers on wblock36_kernel (3: F(4x4,3x3)), wblock16_kernel (2) or wblock_mfma_kernel (1; FPC_WINOGRAD_GEN)
  bool winograd_in1 = true;          // descriptor.layer_in.1 (256 ch): conv-only Winograd x2 + 1x1 (FPC_WINOGRAD_IN1=0: fused direct block)
  bool winograd_det = true;          // ... also the detector's 65-channel blocks (FPC_WINOGRAD_DET=0: direct)
  bool winograd_det_gen3 = true;     // ... on wblock36_dust_kernel in batch calls (FPC_WINOGRAD_DET_GEN=1: generation 1's kernel)
  bool w36_paired = true;            // the 64-channel F(4x4,3x3) layers on wblock36p_kernel, two waves per SIMD (FPC_W36_PAIRED=0: wblock36_kernel<1, ..>)
  bool latency_tiles = true;         // calls of a few frames run the 128-channel Winograd blocks on 4 x 16 tiles (FPC_LATENCY_TILES=0: 8 x 16)
  bool tiles_round6 = true;          // tiles chosen by the matrix rows they issue: layer2.0 on 4 x 16 (FPC_TILES_ROUND6=0: 3 x 20)
  bool layer1_t816 = false;          // direct (non-Winograd) layer1 blocks on 8x16 tiles instead of 16x16 (FPC_L1_T816)
  bool conv_lean = true;             // OP_CONV launches on conv2_mfma_kernel where it applies (FPC_CONV_LEAN=0: conv_mfma_kernel)
  bool fuse_stem_pool = true;        // conv1+bn1+relu+max_pool in one launch (FPC_FUSE_STEM=0: two)
  bool stem_lean = true;             // ... on stem_pool2_kernel where the conv map is whole 16 x 16 tiles (FPC_STEM_LEAN=0: stem_pool_kernel)
  bool stem2 = false;                // derived by build_plan: stem_lean, fp32 MFMA mode, fused stem + pool, whole tiles
  bool fuse_softmax = true;          // FPC_BF16's detector.layer.1 with the exp-softmax epilogue (FPC_FUSE_SOFTMAX=0: its own launch)
  bool convt_fused = true;           // FPC_BF16's ConvTranspose as ONE launch (FPC_CONVT_FUSED=0: four phases)
  // ---- how a launch walks its tiles
  int persist_min_tiles = 1;         // FPC_PERSIST_MIN: tiles per CU from which the Winograd kernel runs persistent (0 = never)
  bool xcd_order = true;             // FPC_XCD_ORDER=0: plain tile order in the persistent Winograd kernel
  int w36_cus = 0;                   // FPC_W36_CUS: CUs a generation-3 launch may take (0 = all): A/B knob for contexts that share the GPU
  int bf16_grid = 0;                 // FPC_BF16_GRID: workgroups a persistent FPC_BF16 launch may take (0 = blocks per CU x CUs): A/B and test knob, w36_cus' twin
  // ---- NMS
  bool nms_one_workgroup = false;    // one workgroup per frame sorts its survivors (FPC_NMS_CHUNKED=0); default: in slices
  int nms_passes = 2;                // parallel NMS launches before the per-frame finish (FPC_NMS_PASSES)
  int nms_g = 0;                     // FPC_NMS_G: workgroups per frame of the NMS rounds kernel (0 = 512 / frames, at most 16)
  // ---- streams
  int nsub = 2;                      // sub-batches of one call, each on a stream of its own (FPC_STREAMS)
  int nside = 2;                     // ... of which the first `nside` have a side stream
  int min_sub = 8;                   // smallest sub-batch worth its own stream (FPC_MIN_SUB); calls below twice this take the latency plan
  bool split_heads = false;          // detector head + NMS of a sub-batch on a side stream next to its descriptor head (FPC_SPLIT_HEADS)
  bool nms_aside = true;             // NMS on the side stream (FPC_NMS_ASIDE=0: in line on the sub-batch stream)
  // ---- test facility
  bool guard_zones = false;          // canary zones behind every carved buffer (FPC_GUARD_ZONES: a whole test run under them)
};

// How a variable's text becomes the option's value.
enum OptionRead {
  READ_NONZERO,   // atoi(e) != 0
  READ_ZERO,      // atoi(e) == 0: the variable names the opposite of the field
  READ_PRESENT,   // set at all, whatever its value
  READ_GE3,       // atoi(e) >= 3
  READ_CLAMP      // atoi(e) clamped to lo .. hi
};

// One option: its field (a bool or an int), the flag bit and the value the field takes when the bit is set (0: no
// flag), the variable (null: none) and how it is read.  The flag first, then the variable over it.
struct OptionRow {
  bool PlanOptions::*b;
  int PlanOptions::*i;
  unsigned flag;
  int flag_value;
  const char* env;
  OptionRead read;
  int lo, hi;
};

#define FPC_OPT_BOOL(field, flag, value, env, read) {&PlanOptions::field, nullptr, flag, value, env, read, 0, 0}
#define FPC_OPT_INT(field, flag, value, env, lo, hi) {nullptr, &PlanOptions::field, flag, value, env, READ_CLAMP, lo, hi}
static const OptionRow g_plan_options[] = {
    FPC_OPT_BOOL(fuse_blocks, FPC_PLAN_NO_FUSED_BLOCKS, 0, "FPC_FUSE", READ_NONZERO),
    FPC_OPT_BOOL(winograd, FPC_PLAN_NO_WINOGRAD, 0, "FPC_WINOGRAD", READ_NONZERO),
    // (two rows of one field, in order: the gen1 flag wins over the gen2 flag, the variable over both)
    FPC_OPT_INT(winograd_gen, FPC_PLAN_WINOGRAD_GEN2, 2, nullptr, 0, 0),
    FPC_OPT_INT(winograd_gen, FPC_PLAN_WINOGRAD_GEN1, 1, "FPC_WINOGRAD_GEN", 1, 3),
    FPC_OPT_BOOL(winograd_in1, FPC_PLAN_NO_WINOGRAD_LAYER_IN1, 0, "FPC_WINOGRAD_IN1", READ_NONZERO),
    FPC_OPT_BOOL(winograd_det, FPC_PLAN_NO_WINOGRAD_DETECTOR, 0, "FPC_WINOGRAD_DET", READ_NONZERO),
    FPC_OPT_BOOL(winograd_det_gen3, FPC_PLAN_DETECTOR_GEN1, 0, "FPC_WINOGRAD_DET_GEN", READ_GE3),
    FPC_OPT_BOOL(w36_paired, FPC_PLAN_W36_ONE_WAVE, 0, "FPC_W36_PAIRED", READ_NONZERO),
    FPC_OPT_BOOL(latency_tiles, FPC_PLAN_NO_LATENCY_TILES, 0, "FPC_LATENCY_TILES", READ_NONZERO),
    FPC_OPT_BOOL(tiles_round6, FPC_PLAN_TILES_ROUND5, 0, "FPC_TILES_ROUND6", READ_NONZERO),
    FPC_OPT_BOOL(layer1_t816, FPC_PLAN_LAYER1_TILE_8x16, 1, "FPC_L1_T816", READ_PRESENT),
    FPC_OPT_BOOL(conv_lean, FPC_PLAN_CONV_ROUND1, 0, "FPC_CONV_LEAN", READ_NONZERO),
    FPC_OPT_BOOL(fuse_stem_pool, FPC_PLAN_NO_FUSED_STEM_POOL, 0, "FPC_FUSE_STEM", READ_NONZERO),
    FPC_OPT_BOOL(stem_lean, FPC_PLAN_STEM_ROUND3, 0, "FPC_STEM_LEAN", READ_NONZERO),
    FPC_OPT_BOOL(fuse_softmax, FPC_PLAN_NO_FUSED_SOFTMAX, 0, "FPC_FUSE_SOFTMAX", READ_NONZERO),
    FPC_OPT_BOOL(convt_fused, FPC_PLAN_CONVT_PHASES, 0, "FPC_CONVT_FUSED", READ_NONZERO),
    FPC_OPT_INT(persist_min_tiles, FPC_PLAN_NO_PERSISTENT_GRID, 0, "FPC_PERSIST_MIN", INT_MIN, INT_MAX),
    FPC_OPT_BOOL(xcd_order, FPC_PLAN_NO_XCD_ORDER, 0, "FPC_XCD_ORDER", READ_NONZERO),
    FPC_OPT_INT(w36_cus, 0, 0, "FPC_W36_CUS", 0, INT_MAX),
    FPC_OPT_INT(bf16_grid, 0, 0, "FPC_BF16_GRID", 0, INT_MAX),
    FPC_OPT_BOOL(nms_one_workgroup, FPC_PLAN_NMS_ONE_WORKGROUP, 1, "FPC_NMS_CHUNKED", READ_ZERO),
    FPC_OPT_INT(nms_passes, 0, 0, "FPC_NMS_PASSES", 0, 64),
    FPC_OPT_INT(nms_g, 0, 0, "FPC_NMS_G", 0, 64),
    FPC_OPT_INT(min_sub, 0, 0, "FPC_MIN_SUB", 1, INT_MAX),
    FPC_OPT_BOOL(guard_zones, FPC_PLAN_GUARD_ZONES, 1, "FPC_GUARD_ZONES", READ_NONZERO),
};
#undef FPC_OPT_BOOL
#undef FPC_OPT_INT

// The persistent grid of an FPC_BF16 launch of `tiles` tiles in `parts` gridDim.y parts: a multiple of 8 (the tile walk
// is per XCD), at most `resident` workgroups (blocks per CU x CUs) shared by the parts -- or at most `cap` (bf16_grid)
// where that is set.
inline int bf16_persistent_grid(int tiles, int resident, int parts, int cap) {
  return std::min((tiles + 7) / 8 * 8, std::max(8, (cap > 0 ? cap : resident) / parts / 8 * 8));
}

inline int read_option(const char* e, const OptionRow& r) {
  switch (r.read) {
    case READ_NONZERO: return atoi(e) != 0;
    case READ_ZERO: return atoi(e) == 0;
    case READ_PRESENT: return 1;
    case READ_GE3: return atoi(e) >= 3;
    case READ_CLAMP: break;
  }
  return std::max(r.lo, std::min(r.hi, atoi(e)));
}

// The options of a context created with `cfg` in an environment read through `env` (getenv's signature): the defaults,
// the config's fields, the table, then the rules that depend on more than one input -- the stream options, in order.
inline PlanOptions resolve_plan_options(const fpc_config& cfg, const char* (*env)(const char*)) {
  PlanOptions o;
  const unsigned pf = cfg.plan_flags;
  const bool vgg = cfg.arch == FPC_ARCH_VGG, bf16 = cfg.dtype == FPC_BF16;
  const bool split = cfg.dtype == FPC_F32_SPLIT || cfg.dtype == FPC_F32_SPLIT_F16;
  auto env_bool = [&](const char* name, bool* v) {
    if (const char* e = env(name)) *v = atoi(e) != 0;
  };
  if (cfg.min_sub_batch > 0) o.min_sub = cfg.min_sub_batch;
  if (cfg.nms_round_launches > 0) o.nms_passes = std::min(64, cfg.nms_round_launches);
  else if (cfg.nms_round_launches < 0) o.nms_passes = 0;
  auto set = [&](const OptionRow& r, int v) {
    if (r.b) o.*r.b = v != 0;
    else o.*r.i = v;
  };
  for (const OptionRow& r : g_plan_options) {
    if (pf & r.flag) set(r, r.flag_value);
    const char* e = r.env ? env(r.env) : nullptr;
    if (e) set(r, read_option(e, r));
  }
  // measured: 2 sub-batches for the fp32-MFMA kernels, 3 for the (shorter) split-operand ones
  o.nsub = cfg.num_streams > 0 ? std::min(8, cfg.num_streams) : (split ? 3 : 2);
  if (const char* e = env("FPC_STREAMS")) o.nsub = std::max(1, std::min(8, atoi(e)));
  // Detector head + NMS of a sub-batch on a side stream next to its descriptor head: the default of the Python network
  // in FPC_F32 with two or more sub-batches, where it was measured to pay.  With the streams on hardware queues of their
  // own, one context, two sub-batches: 10 740 -> 10 845 frames/s (steady 10 790 -> 10 930; two runs each); the C++
  // network loses 2 %, bf16 HD and the QVGA detector do not move, one-sub-batch contexts +0.1 %.  The variable
  // overrides either way.
  o.split_heads = (pf & FPC_PLAN_SPLIT_HEADS) != 0;
  if (!(pf & FPC_PLAN_HEADS_IN_LINE) && o.nsub >= 2 && !vgg && !bf16 && !split) o.split_heads = true;
  env_bool("FPC_SPLIT_HEADS", &o.split_heads);
  o.nms_aside = !split;   // measured: +1.5 % with two sub-batches (fp32-MFMA kernels), nothing with three (split modes)
  if (pf & FPC_PLAN_NMS_IN_LINE) o.nms_aside = false;
  env_bool("FPC_NMS_ASIDE", &o.nms_aside);
  if (o.split_heads) o.nms_aside = false;
  // one side stream per sub-batch only while main + aux + side <= 4 streams, otherwise just the first
  o.nside = 2 * o.nsub <= 4 ? o.nsub : 1;
  return o;
}

}  // namespace fpc
